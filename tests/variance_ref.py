"""numpy float32 reference of the reprojection pass that carries luminance moments and of the variance-guided a-trous
filter (include/prt.h prt_reproject_moments / prt_denoise_variance, DESIGN.md "Variance guidance"), and the sequences
and figures their tests share.

reproject_moments is motion_ref.reproject_motion with the two luminance moments gathered over the same taps, an optional
clamp of the gathered history and a variance estimate; denoise_variance is denoise_ref.denoise with the colour weight
scaled by the pre-filtered variance.  Every operation is one correctly rounded f32 + - * / or sqrt in the order the
definition writes it, so csrc/prt_variance.hip must reproduce both bit for bit."""
import dataclasses

import numpy as np

import denoise_ref as dr
import motion_ref as mr
import reproject_ref as rr

F = np.float32
FAR = dr.FAR
TEMPORAL_DEFAULTS = dict(depth_tol=0.05, normal_min=0.9, max_history=16.0, clamp_k=0.0, min_temporal=4.0)
FILTER_DEFAULTS = dict(iterations=5, normal_power=3, sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.25,
                       color_decay=1.0, variance_floor=1e-6)
G3 = [F(0.25), F(0.5), F(0.25)]  # the 3 x 3 Gaussian's factors: products 1/16, 1/8, 1/4


def luminance(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def reproject_moments(color, normal_depth, instance, cam, W, H, history=None, history_nd=None, prev_cam=None,
                      history_instance=None, motion=None, history_moments=None, depth_tol=0.05, normal_min=0.9,
                      max_history=16.0, clamp_k=0.0, min_temporal=4.0, info=None):
    """The arguments of mr.reproject_motion, and history_moments: float32 [W*H, 4].  Returns (out [W*H, 4],
    moments [W*H, 4]): (rgb, history length) and (m1, m2, variance, 0).  info (a dict) receives mr.reproject_motion's
    masks and: temporal (hit pixels whose variance comes from the moments), spatial (the other hit pixels), and with
    clamp_k > 0 clamped [W*H, 3] (the history after the clamp), lo, hi [W*H, 3] (the clamp's bounds)."""
    color = np.asarray(color, F).reshape(H, W, 4)
    nd = np.asarray(normal_depth, F).reshape(H, W, 4)
    ids = np.asarray(instance, np.uint32).reshape(H, W)
    clamp_k, min_temporal = F(clamp_k), F(min_temporal)
    hit = nd[..., 3] < FAR
    L = luminance(color)
    fresh = color.copy()
    fresh[..., 3] = 1
    with np.errstate(all="ignore"):
        if history is None:
            assert history_nd is None and prev_cam is None and history_instance is None and motion is None
            assert history_moments is None
            out, m1, m2 = fresh, L, L * L
            ok = np.zeros((H, W), bool)
            if info is not None:
                info.update(hit=hit.ravel(), has_history=ok.ravel())
        else:
            hist = np.asarray(history, F).reshape(H, W, 4)
            hnd = np.asarray(history_nd, F).reshape(H, W, 4)
            hmom = np.asarray(history_moments, F).reshape(H, W, 4)
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
            Z = nd[..., 3]
            known = hit & (ids < np.uint32(count))
            A = mo[np.where(known, ids, np.uint32(0)).astype(np.int64)]
            ys, xs = np.mgrid[0:H, 0:W]
            u = xs.astype(F) * (F(1) / fW)
            v = ys.astype(F) * (F(1) / fH)
            P = (TL + u[..., None] * (TR - TL)) + v[..., None] * (BL - TL)
            d = P - pos
            D = d * (F(1) / np.sqrt(rr._dot(d, d)))[..., None]
            X = pos + Z[..., None] * D
            Xp = np.stack([mr._row3(A, r, X) + A[..., r, 3] for r in range(3)], axis=-1)
            w = Xp - pp
            s, sa, sb = rr._dot(w, cuv) / det, rr._dot(w, cv0) / det, rr._dot(w, c0u) / det
            px, py = (sa / s) * fW, (sb / s) * fH
            Zp = np.sqrt(rr._dot(w, w))
            valid = known & (s > 0) & (px >= F(-1)) & (px < fW) & (py >= F(-1)) & (py < fH)
            fx, fy = np.floor(px), np.floor(py)
            ax, ay = px - fx, py - fy
            ix = np.where(valid, fx, F(0)).astype(np.int32)
            iy = np.where(valid, fy, F(0)).astype(np.int32)
            n = rr._unit(np.stack([mr._row3(A, r, nd[..., :3]) for r in range(3)], axis=-1))
            acc = np.zeros((H, W, 4), F)
            am = np.zeros((H, W, 2), F)
            ws = np.zeros((H, W), F)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    inside = valid & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    G, Hq, Mq = hnd[qyc, qxc], hist[qyc, qxc], hmom[qyc, qxc]
                    wb = (ax if i else F(1) - ax) * (ay if j else F(1) - ay)
                    keep = (inside & (G[..., 3] < FAR) & (np.abs(G[..., 3] - Zp) <= depth_tol * Zp)
                            & (rr._dot(n, rr._unit(G[..., :3])) >= normal_min) & (Hq[..., 3] >= F(1)))
                    if hids is not None:
                        keep = keep & (hids[qyc, qxc] == ids)
                    acc = np.where(keep[..., None], acc + wb[..., None] * Hq, acc)
                    am = np.where(keep[..., None], am + wb[..., None] * Mq[..., :2], am)
                    ws = np.where(keep, ws + wb, ws)
            ok = valid & (ws > F(1) / F(64))
            h = acc / ws[..., None]
            hm = am / ws[..., None]
            ln = np.minimum(h[..., 3] + F(1), max_history)
            a = F(1) / ln
            hc = h[..., :3]
            if clamp_k > 0:  # the 3 x 3 neighbourhood of this frame's colour, row-major, in-image pixels only
                s1, s2, cnt = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F), np.zeros((H, W), F)
                inimg = np.ones((H, W), bool)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        inq = dr._shift(inimg, dy, dx, False)
                        c = dr._shift(color[..., :3], dy, dx, F(0))
                        s1 = np.where(inq[..., None], s1 + c, s1)
                        s2 = np.where(inq[..., None], s2 + c * c, s2)
                        cnt = np.where(inq, cnt + F(1), cnt)
                mu = s1 / cnt[..., None]
                sg = np.sqrt(np.fmax(s2 / cnt[..., None] - mu * mu, F(0)))
                lo, hi = mu - clamp_k * sg, mu + clamp_k * sg
                hc = np.fmin(np.fmax(hc, lo), hi)
                if info is not None:
                    info.update(clamped=hc.reshape(-1, 3), lo=lo.reshape(-1, 3), hi=hi.reshape(-1, 3))
            rgb = hc + a[..., None] * (color[..., :3] - hc)
            blended = np.concatenate([rgb, ln[..., None]], axis=-1)
            out = np.where(ok[..., None], blended, fresh)
            m1 = np.where(ok, hm[..., 0] + a * (L - hm[..., 0]), L)
            m2 = np.where(ok, hm[..., 1] + a * (L * L - hm[..., 1]), L * L)
            assert out.dtype == F and m1.dtype == F and m2.dtype == F
            if info is not None:
                info.update(hit=hit.ravel(), known=known.ravel(), valid=valid.ravel(), has_history=ok.ravel(),
                            px=px.ravel(), py=py.ravel())
        # the variance: the moments' once the history is min_temporal long, the 5 x 5 window's before that
        ln = out[..., 3]
        temporal = hit & (ln >= min_temporal)
        s1, s2, cnt = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                keep = dr._shift(hit, dy, dx, False) & (dr._shift(ids, dy, dx, np.uint32(0)) == ids)
                Lq = dr._shift(L, dy, dx, F(0))
                s1 = np.where(keep, s1 + Lq, s1)
                s2 = np.where(keep, s2 + Lq * Lq, s2)
                cnt = np.where(keep, cnt + F(1), cnt)
        mu = s1 / cnt
        spatial = np.fmax(s2 / cnt - mu * mu, F(0)) * (min_temporal / ln)
        var = np.where(temporal, np.fmax(m2 - m1 * m1, F(0)), spatial)
        var = np.where(hit, var, F(0))
        assert var.dtype == F
    if info is not None:
        info.update(temporal=temporal.ravel(), spatial=(hit & ~temporal).ravel())
    mom = np.stack([m1, m2, var, np.zeros((H, W), F)], axis=-1)
    return out.reshape(-1, 4), mom.reshape(-1, 4)


def denoise_variance(color, moments, albedo, normal_depth, W, H, iterations=5, normal_power=3, sigma_color=2.0,
                     sigma_depth=0.1, sigma_albedo=0.25, color_decay=1.0, variance_floor=1e-6):
    """color / moments / albedo / normal_depth: float32 [W*H, 4] (albedo may be None when sigma_albedo == 0; of
    moments only z, the variance, is read).  Returns (out [W*H, 4], variance [W*H]): rgb filtered with w copied from
    color, and the variance after the last iteration."""
    color = np.asarray(color, F).reshape(H, W, 4)
    nd = np.asarray(normal_depth, F).reshape(H, W, 4)
    sigma_depth, sigma_albedo = F(sigma_depth), F(sigma_albedo)
    color_decay, variance_floor = F(color_decay), F(variance_floor)
    use_albedo = sigma_albedo > 0
    A = np.asarray(albedo, F).reshape(H, W, 4)[..., :3] if use_albedo else None
    Z = nd[..., 3]
    hit = Z < FAR
    N = nd[..., :3]
    with np.errstate(all="ignore"):
        inv = F(1) / np.sqrt(dr._dot(N, N))
        n = N * inv[..., None]
        I = color[..., :3].copy()
        V = np.asarray(moments, F).reshape(H, W, 4)[..., 2].copy()
        sc = F(sigma_color)
        for i in range(iterations):
            s = 1 << i
            sc2 = sc * sc
            gs, gw = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    okq = dr._shift(hit, dy, dx, False)
                    g = G3[dy + 1] * G3[dx + 1]
                    gs = np.where(okq, gs + g * dr._shift(V, dy, dx, F(0)), gs)
                    gw = np.where(okq, gw + g, gw)
            den = sc2 * np.fmax(gs / gw, variance_floor)
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            vsum = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ok = dr._shift(hit, s * dy, s * dx, False)  # inside the image and a hit
                    Iq = dr._shift(I, s * dy, s * dx, F(0))
                    Vq = dr._shift(V, s * dy, s * dx, F(0))
                    if dx == 0 and dy == 0:
                        w = np.full((H, W), dr.H5[2] * dr.H5[2], F)
                    else:
                        nq = dr._shift(n, s * dy, s * dx, F(0))
                        Zq = dr._shift(Z, s * dy, s * dx, F(1))
                        dn = dr._dot(n, nq)
                        wn = np.where(dn > 0, dn, F(0))
                        for _ in range(normal_power):
                            wn = wn * wn
                        dist = F(s * max(abs(dx), abs(dy)))
                        rz = (Zq - Z) / ((sigma_depth * Z) * dist)
                        wz = F(1) / (F(1) + rz * rz)
                        dc = Iq - I
                        c2 = dr._dot(dc, dc)
                        wc = F(1) / (F(1) + c2 / den)
                        w = ((dr.H5[dy + 2] * dr.H5[dx + 2]) * wn) * wz
                        w = w * wc
                        if use_albedo:
                            da = dr._shift(A, s * dy, s * dx, F(0)) - A
                            w = w * (F(1) / (F(1) + dr._dot(da, da) / (sigma_albedo * sigma_albedo)))
                    assert w.dtype == F
                    acc = np.where(ok[..., None], acc + w[..., None] * Iq, acc)
                    wsum = np.where(ok, wsum + w, wsum)
                    vsum = np.where(ok, vsum + (w * w) * Vq, vsum)
            I = np.where(hit[..., None], acc / wsum[..., None], I)  # miss pixels pass through
            V = np.where(hit, vsum / (wsum * wsum), V)
            assert I.dtype == F and V.dtype == F
            sc = sc * color_decay
    out = color.copy()
    out[..., :3] = I
    return out.reshape(-1, 4), V.reshape(-1)


# ---- chains over the views of motion_ref (dicts of cam, color, nd, ids, xf)
def step(vs, k, hist, W, H, **par):
    """Frame k of the views `vs` reprojected onto hist = (out, moments) of frame k - 1 (None starts a history)."""
    v = vs[k]
    if hist is None:
        return reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], W, H, **par)
    u = vs[k - 1]
    return reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"], u["ids"],
                             mr.motion_f32(v["xf"], u["xf"]), hist[1], **par)


def chain(vs, W, H, infos=None, **par):
    """[(out, moments)] of reprojecting frame after frame, each on its own previous output; infos (a list) receives
    one info dict per frame."""
    outs, hist = [], None
    for k in range(len(vs)):
        info = {}
        hist = step(vs, k, hist, W, H, info=info, **par)
        outs.append(hist)
        if infos is not None:
            infos.append(info)
    return outs


def motion_chain(vs, W, H):
    """The parent pipeline's chain over the same views: mr.reproject_motion with ids, frame after frame."""
    outs = []
    for k, v in enumerate(vs):
        if k == 0:
            outs.append(mr.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], W, H))
            continue
        u = vs[k - 1]
        outs.append(mr.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], W, H, outs[-1], u["nd"], u["cam"],
                                        u["ids"], mr.motion_f32(v["xf"], u["xf"])))
    return outs


# ---- the sequences of the quality figures: (name, views, albedo of the last view, converged last frame, W, H)
QUALITY = ["B/rest", "B/slow", "A/rest", "multi_96x72/slow", "small_70x45/slow"]
# measured new / parent RMSE ratio of each sequence with FILTER_DEFAULTS (DESIGN.md "Variance guidance")
MEASURED = {"B/rest": 0.7327, "B/slow": 0.7528, "A/rest": 0.7394, "multi_96x72/slow": 0.7385,
            "small_70x45/slow": 0.7839}
_alb = {}


def _identity_xf(name):
    sd, _, _ = dr.scene_of(name)
    return np.stack([np.asarray(T, F).reshape(4, 4) for _, T in sd.instances])


def sequence(key):
    """(vs, albedo, converged, W, H) of one of QUALITY."""
    import oracle
    a, cseq = key.split("/")
    if a in mr.SEQS:
        _, W, H = dr.scene_of(mr.SCENE)
        vs = [mr.view(a, cseq, k) for k in range(mr.FRAMES)]
        if key not in _alb:
            osc, _, _ = mr._oracle_at(a, cseq, mr.FRAMES - 1)
            _alb[key] = dr.oracle_guides(osc, W, H, oracle.NORMALMAP)[0]
        return vs, _alb[key], mr.converged_last(a, cseq), W, H
    _, W, H = dr.scene_of(a)
    xf = _identity_xf(a)
    vs = []
    for k in range(rr.SLOW_FRAMES):
        g = rr.view(a, cseq, k, frame=True)
        vs.append(dict(cam=g["cam"], color=g["color"], nd=g["nd"], ids=mr.oracle_ids(a, cseq, k), xf=xf))
    return vs, rr.oracle_albedo(a, cseq, rr.SLOW_FRAMES - 1), rr.converged_last_slow(a), W, H


def quality(key, **filt):
    """(rmse new, rmse parent) of the last frame of a sequence against the converged frame: denoise_variance of the
    reproject_moments chain against dr.denoise (dr.DEFAULTS) of the reproject_motion chain."""
    vs, alb, conv, W, H = sequence(key)
    out, mom = chain(vs, W, H)[-1]
    par = dict(FILTER_DEFAULTS)
    par.update(filt)
    new = denoise_variance(out, mom, alb, vs[-1]["nd"], W, H, **par)[0]
    old = dr.denoise(motion_chain(vs, W, H)[-1], alb, vs[-1]["nd"], W, H, **dr.DEFAULTS)
    return dr.rmse(new, conv), dr.rmse(old, conv)


def bound(measured):
    """The asserted limit on a new / parent ratio: halfway from the measured ratio to 1 (no gain); for a sequence
    that measured >= 1, the measured ratio + 0.02."""
    return measured + (1.0 - measured) / 2.0 if measured < 1.0 else measured + 0.02


# ---- the lighting change: 8 frames at rest on multi_96x72, the four point lights' colours permuted from frame 4 on
LIGHT_FRAMES, LIGHT_CHANGE, LIGHT_PERM = 8, 4, [1, 2, 3, 0]
_light = {}


def _relit(sd):
    lt = sd.lights
    pc = np.asarray(lt.point_col, F).reshape(4, 3)[LIGHT_PERM].copy()
    return dataclasses.replace(sd, lights=dataclasses.replace(lt, point_col=pc))


def light_views():
    """(vs, [converged frame under the new lights], W, H): the oracle's 2-spp depth-4 frames (frame_index = k), the
    lights changed from frame LIGHT_CHANGE on; nothing moves."""
    import oracle
    if "vs" not in _light:
        sd, W, H = dr.scene_of(mr.SCENE)
        base = mr.view("frozen", "rest", 0)
        osc_new = oracle.OracleScene(_relit(sd), W, H)
        vs = []
        for k in range(LIGHT_FRAMES):
            if k < LIGHT_CHANGE:
                color = mr.view("frozen", "rest", k)["color"]
            else:
                color = osc_new.render(W, H, spp=2, bounces=4, frame_index=k)[0]
                color.setflags(write=False)
            vs.append(dict(cam=base["cam"], color=color, nd=base["nd"], ids=base["ids"], xf=base["xf"]))
        conv = osc_new.render(W, H, spp=1024, bounces=4, frame_index=1000)[0]
        conv.setflags(write=False)
        _light.update(vs=vs, conv=conv, W=W, H=H)
    return _light["vs"], _light["conv"], _light["W"], _light["H"]
