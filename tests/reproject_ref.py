"""numpy float32 reference of the temporal reprojection pass (include/prt.h prt_reproject, DESIGN.md "Temporal
reprojection"), and the camera sequences and oracle frames its tests share.

Every operation is one correctly rounded f32 + - * / or sqrt (plus floor, fabs, min and compares) in the order the
definition writes it, vectorised over the pixels with a loop over the four taps in their stated order, so
csrc/prt_temporal.hip (built without FMA contraction, with IEEE division) must reproduce it bit for bit."""
import dataclasses

import numpy as np

import denoise_ref as dr

F = np.float32
FAR = dr.FAR
DEFAULTS = dict(depth_tol=0.05, normal_min=0.9, max_history=16.0)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _unit(N):
    return N * (F(1) / np.sqrt(_dot(N, N)))[..., None]


def plane(cam):
    """(pos, TL, TR, BL) float32 of a prt.Camera (or such a tuple itself)."""
    if isinstance(cam, tuple):
        return tuple(np.asarray(a, F) for a in cam)
    return tuple(np.asarray(a, F) for a in (cam.camPos, cam.topLeft, cam.topRight, cam.bottomLeft))


def reproject(color, normal_depth, cam, W, H, history=None, history_nd=None, prev_cam=None, depth_tol=0.05,
              normal_min=0.9, max_history=16.0, info=None):
    """color / normal_depth / history / history_nd: float32 [W*H, 4]; cam / prev_cam: prt.Camera or (pos, TL, TR, BL).
    Returns out [W*H, 4] (rgb, w = history length).  info (a dict) receives per-pixel masks and positions:
    hit, valid (entered the gather), has_history, px, py."""
    color = np.asarray(color, F).reshape(H, W, 4)
    fresh = color.copy()
    fresh[..., 3] = 1
    if history is None:
        assert history_nd is None and prev_cam is None
        return fresh.reshape(-1, 4)
    nd = np.asarray(normal_depth, F).reshape(H, W, 4)
    hist = np.asarray(history, F).reshape(H, W, 4)
    hnd = np.asarray(history_nd, F).reshape(H, W, 4)
    depth_tol, normal_min, max_history = F(depth_tol), F(normal_min), F(max_history)
    pos, TL, TR, BL = plane(cam)
    pp, TLp, TRp, BLp = plane(prev_cam)
    e0, eu, ev = TLp - pp, TRp - TLp, BLp - TLp
    cuv, cv0, c0u = _cross(eu, ev), _cross(ev, e0), _cross(e0, eu)
    det = _dot(e0, cuv)
    fW, fH = F(W), F(H)
    with np.errstate(all="ignore"):
        Z = nd[..., 3]
        hit = Z < FAR
        ys, xs = np.mgrid[0:H, 0:W]
        u = xs.astype(F) * (F(1) / fW)
        v = ys.astype(F) * (F(1) / fH)
        P = (TL + u[..., None] * (TR - TL)) + v[..., None] * (BL - TL)
        d = P - pos
        D = d * (F(1) / np.sqrt(_dot(d, d)))[..., None]
        X = pos + Z[..., None] * D
        w = X - pp
        s, sa, sb = _dot(w, cuv) / det, _dot(w, cv0) / det, _dot(w, c0u) / det
        px, py = (sa / s) * fW, (sb / s) * fH
        Zp = np.sqrt(_dot(w, w))
        valid = hit & (s > 0) & (px >= F(-1)) & (px < fW) & (py >= F(-1)) & (py < fH)  # NaN compares false
        fx, fy = np.floor(px), np.floor(py)
        ax, ay = px - fx, py - fy
        ix = np.where(valid, fx, F(0)).astype(np.int32)
        iy = np.where(valid, fy, F(0)).astype(np.int32)
        n = _unit(nd[..., :3])
        acc = np.zeros((H, W, 4), F)
        ws = np.zeros((H, W), F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                inside = valid & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                G, Hq = hnd[qyc, qxc], hist[qyc, qxc]
                wb = (ax if i else F(1) - ax) * (ay if j else F(1) - ay)
                keep = (inside & (G[..., 3] < FAR) & (np.abs(G[..., 3] - Zp) <= depth_tol * Zp)
                        & (_dot(n, _unit(G[..., :3])) >= normal_min) & (Hq[..., 3] >= F(1)))
                assert wb.dtype == F
                acc = np.where(keep[..., None], acc + wb[..., None] * Hq, acc)
                ws = np.where(keep, ws + wb, ws)
        ok = valid & (ws > F(1) / F(64))
        h = acc / ws[..., None]
        ln = np.minimum(h[..., 3] + F(1), max_history)
        a = F(1) / ln
        rgb = h[..., :3] + a[..., None] * (color[..., :3] - h[..., :3])
        blended = np.concatenate([rgb, ln[..., None]], axis=-1)
        assert blended.dtype == F
        out = np.where(ok[..., None], blended, fresh)
    if info is not None:
        info.update(hit=hit.ravel(), valid=valid.ravel(), has_history=ok.ravel(), px=px.ravel(), py=py.ravel())
    return out.reshape(-1, 4)


# ---- the camera sequences the tests share: positions are offsets added to the scene's camera, the target stays
SLOW_STEP, FAST_STEP = (0.05, 0.0, 0.02), (0.25, 0.05, 0.1)
SLOW_FRAMES, FAST_FRAMES = 8, 6


def positions(sd, seq):
    """[(camera position, target)] of a sequence, float32."""
    p, t = np.asarray(sd.cam_pos, F), np.asarray(sd.cam_target, F)
    if seq == "slow":
        return [(p + np.array(SLOW_STEP, F) * F(k), t) for k in range(SLOW_FRAMES)]
    if seq == "fast":
        return [(p + np.array(FAST_STEP, F) * F(k), t) for k in range(FAST_FRAMES)]
    if seq == "rest":
        return [(p, t), (p, t)]
    if seq == "behind":  # the previous camera looks the other way: every point has s < 0
        return [(p, F(2) * p - t), (p, t)]
    raise KeyError(seq)


def cameras(sd, W, H, seq):
    import prt
    return [prt.Camera(p, t, F(W) / F(H)) for p, t in positions(sd, seq)]


# ---- oracle frames of the sequences (made once per process, never modified)
_osc, _views, _conv = {}, {}, {}


def _oracle_at(name, pos, target):
    """The scene's OracleScene (its own, not denoise_ref's) with the camera moved."""
    import oracle
    sd, W, H = dr.scene_of(name)
    if name not in _osc:
        _osc[name] = oracle.OracleScene(sd, W, H)
    osc = _osc[name]
    osc.sd = dataclasses.replace(sd, cam_pos=np.asarray(pos, F), cam_target=np.asarray(target, F))
    osc.set_camera(W, H)
    return osc, W, H


def view(name, seq, k, frame=False):
    """dict(cam, nd[, color]) of view k of a sequence: the camera, the oracle's normal_depth and, with frame=True, its
    2-spp depth-4 frame with frame_index = k."""
    import oracle
    key = (name, seq, k)
    sd, W, H = dr.scene_of(name)
    if key not in _views:
        pos, tgt = positions(sd, seq)[k]
        osc, _, _ = _oracle_at(name, pos, tgt)
        _, nd, _, _ = dr.oracle_guides(osc, W, H, oracle.NORMALMAP)
        nd.setflags(write=False)
        _views[key] = dict(cam=cameras(sd, W, H, seq)[k], nd=nd)
    g = _views[key]
    if frame and "color" not in g:
        pos, tgt = positions(sd, seq)[k]
        osc, _, _ = _oracle_at(name, pos, tgt)
        g["color"] = osc.render(W, H, spp=2, bounces=4, frame_index=k)[0]
        g["color"].setflags(write=False)
    return g


def converged_last_slow(name):
    """The oracle's 1024-spp frame (frame_index 1000) of the last view of `slow`."""
    if name not in _conv:
        sd, W, H = dr.scene_of(name)
        pos, tgt = positions(sd, "slow")[-1]
        osc, _, _ = _oracle_at(name, pos, tgt)
        _conv[name] = osc.render(W, H, spp=1024, bounces=4, frame_index=1000)[0]
        _conv[name].setflags(write=False)
    return _conv[name]


def chain(frames, nds, cams, W, H, **par):
    """The outputs of reprojecting frame after frame, starting a history at the first."""
    outs = [reproject(frames[0], nds[0], cams[0], W, H)]
    for k in range(1, len(frames)):
        outs.append(reproject(frames[k], nds[k], cams[k], W, H, outs[-1], nds[k - 1], cams[k - 1], **par))
    return outs


def quality(name, last_frame, reprojected, albedo, nd):
    """The figures of the two quality bounds: (rmse of the last frame, rmse reprojected, rmse of the reprojected image
    denoised, rmse of the last frame denoised), against converged_last_slow(name)."""
    _, W, H = dr.scene_of(name)
    conv = converged_last_slow(name)
    den_r = dr.denoise(reprojected, albedo, nd, W, H, **dr.DEFAULTS)
    den_f = dr.denoise(last_frame, albedo, nd, W, H, **dr.DEFAULTS)
    return dr.rmse(last_frame, conv), dr.rmse(reprojected, conv), dr.rmse(den_r, conv), dr.rmse(den_f, conv)


def oracle_albedo(name, seq, k):
    import oracle
    sd, W, H = dr.scene_of(name)
    pos, tgt = positions(sd, seq)[k]
    osc, _, _ = _oracle_at(name, pos, tgt)
    return dr.oracle_guides(osc, W, H, oracle.NORMALMAP)[0]
