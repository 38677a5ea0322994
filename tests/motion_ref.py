"""numpy float32 reference of the motion-aware temporal reprojection pass (include/prt.h prt_reproject_motion, DESIGN.md
"Moving instances"), a float64 statement of prt_instance_motion, and the instance sequences and oracle frames its tests
share.

The pass is reproject_ref.reproject with the pixel's hit and normal carried back by the motion matrix of the pixel's
instance and the taps optionally compared by instance id: every operation is one correctly rounded f32 + - * / or sqrt
in the order the definition writes it, so csrc/prt_motion.hip must reproduce it bit for bit."""
import dataclasses

import numpy as np

import denoise_ref as dr
import reproject_ref as rr

F = np.float32
FAR = dr.FAR
MISS = np.uint32(0xFFFFFFFF)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


def _row3(A, r, v):
    return (A[..., r, 0] * v[..., 0] + A[..., r, 1] * v[..., 1]) + A[..., r, 2] * v[..., 2]


def reproject_motion(color, normal_depth, instance, cam, W, H, history=None, history_nd=None, prev_cam=None,
                     history_instance=None, motion=None, depth_tol=0.05, normal_min=0.9, max_history=16.0, info=None):
    """color / normal_depth / history / history_nd: float32 [W*H, 4]; instance / history_instance: uint32 [W*H];
    motion: float32 [count, 12] (row-major 3 x 4 per instance); cam / prev_cam: prt.Camera or (pos, TL, TR, BL).
    Returns out [W*H, 4] (rgb, w = history length).  info (a dict) receives per-pixel masks and positions:
    hit, known (hit with an id below count), valid (entered the gather), has_history, px, py."""
    color = np.asarray(color, F).reshape(H, W, 4)
    fresh = color.copy()
    fresh[..., 3] = 1
    if history is None:
        assert history_nd is None and prev_cam is None and history_instance is None and motion is None
        return fresh.reshape(-1, 4)
    nd = np.asarray(normal_depth, F).reshape(H, W, 4)
    hist = np.asarray(history, F).reshape(H, W, 4)
    hnd = np.asarray(history_nd, F).reshape(H, W, 4)
    ids = np.asarray(instance, np.uint32).reshape(H, W)
    hids = np.asarray(history_instance, np.uint32).reshape(H, W) if history_instance is not None else None
    mo = np.asarray(motion, F).reshape(-1, 3, 4)
    count = len(mo)
    assert count > 0
    depth_tol, normal_min, max_history = F(depth_tol), F(normal_min), F(max_history)
    pos, TL, TR, BL = rr.plane(cam)
    pp, TLp, TRp, BLp = rr.plane(prev_cam)
    e0, eu, ev = TLp - pp, TRp - TLp, BLp - TLp
    cuv, cv0, c0u = rr._cross(eu, ev), rr._cross(ev, e0), rr._cross(e0, eu)
    det = rr._dot(e0, cuv)
    fW, fH = F(W), F(H)
    with np.errstate(all="ignore"):
        Z = nd[..., 3]
        hit = Z < FAR
        known = hit & (ids < np.uint32(count))  # a hit whose id has no matrix starts over; no matrix is read for it
        A = mo[np.where(known, ids, np.uint32(0)).astype(np.int64)]  # [H, W, 3, 4]
        ys, xs = np.mgrid[0:H, 0:W]
        u = xs.astype(F) * (F(1) / fW)
        v = ys.astype(F) * (F(1) / fH)
        P = (TL + u[..., None] * (TR - TL)) + v[..., None] * (BL - TL)
        d = P - pos
        D = d * (F(1) / np.sqrt(rr._dot(d, d)))[..., None]
        X = pos + Z[..., None] * D
        Xp = np.stack([_row3(A, r, X) + A[..., r, 3] for r in range(3)], axis=-1)
        w = Xp - pp
        s, sa, sb = rr._dot(w, cuv) / det, rr._dot(w, cv0) / det, rr._dot(w, c0u) / det
        px, py = (sa / s) * fW, (sb / s) * fH
        Zp = np.sqrt(rr._dot(w, w))
        valid = known & (s > 0) & (px >= F(-1)) & (px < fW) & (py >= F(-1)) & (py < fH)  # NaN compares false
        fx, fy = np.floor(px), np.floor(py)
        ax, ay = px - fx, py - fy
        ix = np.where(valid, fx, F(0)).astype(np.int32)
        iy = np.where(valid, fy, F(0)).astype(np.int32)
        N = nd[..., :3]
        n = rr._unit(np.stack([_row3(A, r, N) for r in range(3)], axis=-1))
        assert Xp.dtype == F and n.dtype == F
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
                        & (rr._dot(n, rr._unit(G[..., :3])) >= normal_min) & (Hq[..., 3] >= F(1)))
                if hids is not None:
                    keep = keep & (hids[qyc, qxc] == ids)
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
        info.update(hit=hit.ravel(), known=known.ravel(), valid=valid.ravel(), has_history=ok.ravel(), px=px.ravel(),
                    py=py.ravel())
    return out.reshape(-1, 4)


def motion_matrices(cur, prev):
    """float64 [count, 3, 4]: prev * inverse(cur) of two sets of row-major 4 x 4 transforms read as affine; the
    identity for a pair that is bytewise equal as float32, and for a current transform that is non-finite or
    singular."""
    cur32, prev32 = np.asarray(cur, F).reshape(-1, 4, 4), np.asarray(prev, F).reshape(-1, 4, 4)
    out = np.zeros((len(cur32), 3, 4), np.float64)
    for k, (c, p) in enumerate(zip(cur32, prev32)):
        out[k] = np.eye(4)[:3]
        c64, p64 = c.astype(np.float64), p.astype(np.float64)
        c64[3], p64[3] = (0, 0, 0, 1), (0, 0, 0, 1)
        if c.tobytes() == p.tobytes() or not np.all(np.isfinite(c64)) or np.linalg.det(c64[:3, :3]) == 0:
            continue
        out[k] = (p64 @ np.linalg.inv(c64))[:3]
    return out


def motion_f32(cur, prev):
    """motion_matrices rounded once to float32, [count, 12]: what prt_instance_motion returns up to a rounding
    boundary."""
    return motion_matrices(cur, prev).astype(F).reshape(-1, 12)


def identity(count):
    return np.tile(IDENTITY, (count, 1))


# ---- the instance sequences: instance MOVER of multi_96x72 moves, T_k = Translate(k t) * T_0 * RotY(k a) in float64
# rounded to float32; every other instance is fixed
SCENE, MOVER, FRAMES = "multi_96x72", 1, 8
SEQS = {"A": ((0.06, 0.0, 0.04), 0.06), "B": ((0.15, 0.0, 0.1), 0.15), "frozen": ((0.0, 0.0, 0.0), 0.0)}


def transforms(mseq, k):
    """float32 [count, 4, 4]: the scene's instance transforms at frame k of an instance sequence."""
    sd, _, _ = dr.scene_of(SCENE)
    t, a = SEQS[mseq]
    xf = np.stack([np.asarray(T, F).reshape(4, 4) for _, T in sd.instances])
    c, s = np.cos(k * a), np.sin(k * a)
    tr, rot = np.eye(4), np.eye(4)
    tr[:3, 3] = k * np.asarray(t, np.float64)
    rot[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    xf[MOVER] = (tr @ xf[MOVER].astype(np.float64) @ rot).astype(F)
    return xf


def scene_at(mseq, k):
    """The scene with its instances at frame k (the meshes, lights and camera are the scene's)."""
    sd, _, _ = dr.scene_of(SCENE)
    xf = transforms(mseq, k)
    return dataclasses.replace(sd, instances=[(mi, xf[i]) for i, (mi, _) in enumerate(sd.instances)])


def camera_positions(cseq):
    """[(camera position, target)] of the FRAMES frames: `rest` is the scene camera throughout, `slow` rr's."""
    sd, _, _ = dr.scene_of(SCENE)
    if cseq == "rest":
        return [rr.positions(sd, "rest")[0]] * FRAMES
    assert cseq == "slow" and rr.SLOW_FRAMES == FRAMES
    return rr.positions(sd, "slow")


def cameras(cseq):
    import prt
    _, W, H = dr.scene_of(SCENE)
    return [prt.Camera(p, t, F(W) / F(H)) for p, t in camera_positions(cseq)]


def ids_of(t, inst):
    return np.where(np.asarray(t, F) < FAR, np.asarray(inst, np.uint32), MISS).astype(np.uint32)


def oracle_ids(name, seq, k):
    """The oracle's first-hit instance ids of view k of one of rr's camera sequences (static instances)."""
    sd, W, H = dr.scene_of(name)
    pos, tgt = rr.positions(sd, seq)[k]
    osc, _, _ = rr._oracle_at(name, pos, tgt)
    t, _, _, _, inst = osc.primary_hits(W, H)
    return ids_of(t, inst)


# ---- oracle frames of the sequences (made once per process, never modified)
_osc, _views, _conv = {}, {}, {}


def _oracle_at(mseq, cseq, k):
    import oracle
    _, W, H = dr.scene_of(SCENE)
    key = (mseq, k) if mseq != "frozen" else ("frozen", 0)
    if key not in _osc:
        _osc[key] = oracle.OracleScene(scene_at(mseq, k), W, H)
    osc = _osc[key]
    pos, tgt = camera_positions(cseq)[k]
    osc.sd = dataclasses.replace(osc.sd, cam_pos=np.asarray(pos, F), cam_target=np.asarray(tgt, F))
    osc.set_camera(W, H)
    return osc, W, H


def view(mseq, cseq, k):
    """dict(cam, color, nd, ids, xf) of frame k: the camera, the oracle's 2-spp depth-4 frame with frame_index = k (a
    fresh accumulation), its normal_depth, its first-hit instance ids and the instance transforms."""
    import oracle
    key = (mseq, cseq, k)
    if key not in _views:
        osc, W, H = _oracle_at(mseq, cseq, k)
        _, nd, _, _ = dr.oracle_guides(osc, W, H, oracle.NORMALMAP)
        t, _, _, _, inst = osc.primary_hits(W, H)
        color = osc.render(W, H, spp=2, bounces=4, frame_index=k)[0]
        g = dict(cam=cameras(cseq)[k], color=color, nd=nd, ids=ids_of(t, inst), xf=transforms(mseq, k))
        for a in (g["color"], g["nd"], g["ids"], g["xf"]):
            a.setflags(write=False)
        _views[key] = g
    return _views[key]


def converged_last(mseq, cseq):
    """The oracle's 1024-spp frame (frame_index 1000) of the last frame's configuration."""
    key = (mseq, cseq)
    if key not in _conv:
        osc, W, H = _oracle_at(mseq, cseq, FRAMES - 1)
        _conv[key] = osc.render(W, H, spp=1024, bounces=4, frame_index=1000)[0]
        _conv[key].setflags(write=False)
    return _conv[key]


def step(vs, k, hist, plain=False, with_ids=True, motion=None, **par):
    """Frame k of the views `vs` reprojected onto `hist` (the output of frame k - 1; None starts a history): by
    rr.reproject (plain) or by reproject_motion with motion_f32 of the two frames' transforms unless `motion` is
    given."""
    _, W, H = dr.scene_of(SCENE)
    v = vs[k]
    if plain:
        if k == 0:
            return rr.reproject(v["color"], v["nd"], v["cam"], W, H)
        u = vs[k - 1]
        return rr.reproject(v["color"], v["nd"], v["cam"], W, H, hist, u["nd"], u["cam"], **par)
    if k == 0:
        return reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], W, H)
    u = vs[k - 1]
    mo = motion if motion is not None else motion_f32(v["xf"], u["xf"])
    return reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist, u["nd"], u["cam"],
                            u["ids"] if with_ids else None, mo, **par)


def chain(vs, plain=False, **kw):
    """The outputs of reprojecting frame after frame, each on its own previous output."""
    outs = [step(vs, 0, None, plain)]
    for k in range(1, len(vs)):
        outs.append(step(vs, k, outs[-1], plain, **kw))
    return outs


def has_history(out):
    """A pixel whose output is a blend has a history length above 1 (a length is >= 1, and 1 + 1 after a blend)."""
    return np.asarray(out)[:, 3] > F(1)


def figures(vs, plain_out, motion_out, conv):
    """The figures of the quality assertions over the last frame vs[-1]: dict(frac_plain, frac_motion, len_plain,
    len_motion, rmse_frame, rmse_plain, rmse_motion over the mover's pixels; static_plain, static_motion: the RMSE over
    the other hit pixels)."""
    ids = vs[-1]["ids"]
    mover, static = ids == MOVER, (ids != MOVER) & (ids != MISS)
    assert mover.any() and static.any()
    return dict(frac_plain=float(has_history(plain_out)[mover].mean()),
                frac_motion=float(has_history(motion_out)[mover].mean()),
                len_plain=float(plain_out[mover, 3].mean()), len_motion=float(motion_out[mover, 3].mean()),
                rmse_frame=dr.rmse(vs[-1]["color"][mover], conv[mover]),
                rmse_plain=dr.rmse(plain_out[mover], conv[mover]), rmse_motion=dr.rmse(motion_out[mover], conv[mover]),
                static_plain=dr.rmse(plain_out[static], conv[static]),
                static_motion=dr.rmse(motion_out[static], conv[static]))


def check_quality(f):
    """The issue's bounds on figures(): the fraction with history rises by >= 0.15, the mover's RMSE falls to <= 0.85 of
    the plain pass's, and the static pixels' RMSE is the same within 1e-6."""
    assert f["frac_motion"] - f["frac_plain"] >= 0.15, f
    assert f["rmse_motion"] <= 0.85 * f["rmse_plain"], f
    assert abs(f["static_motion"] - f["static_plain"]) <= 1e-6, f
