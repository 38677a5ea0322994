"""numpy float32 reference of the two passes that let the temporal reprojection follow a deforming mesh (include/prt.h
prt_render_aov_deform's offset output and prt_reproject_deform, DESIGN.md "Deforming meshes"), and the deforming
sequence and figures their tests share.

offset_ref interpolates the differences between a primitive's snapshotted and current corners with the hit's
barycentrics; reproject_deform is variance_ref.reproject_moments restated with that offset, under the previous instance
transform's 3 x 3, added to the point carried back.  Every operation is one correctly rounded f32 + - * / or sqrt in
the order the definition writes it, so csrc/prt_deform.hip must reproduce both bit for bit.  Nothing here reads the
oracle's or the device's results of these two passes: the oracle only supplies frames, hits and guides."""
import dataclasses

import numpy as np

import deform
import denoise_ref as dr
import motion_ref as mr
import reproject_ref as rr
import variance_ref as vr

F = np.float32
FAR = dr.FAR


def corners(mesh):
    """float32 [T, 3, 3]: vertices[indices[3p + k]] of a scenes.Mesh, the p[9] of its ShadeTri records."""
    V = np.asarray(mesh.vertices, F).reshape(-1, 3)
    return V[np.asarray(mesh.indices, np.int64).reshape(-1, 3)]


def offset_ref(hits, instance_mesh, meshes_now, meshes_snapshot):
    """hits: records with fields t, u, v, prim, inst (prt_trace_primary's, or a tuple of five arrays in that order);
    instance_mesh: the mesh index of every instance; meshes_now / meshes_snapshot: one scenes.Mesh per mesh, None in
    meshes_snapshot for a mesh without a snapshot.  Returns float32 [n, 4]: (offset, 1), or zeros for a miss and for a
    mesh without a snapshot."""
    if isinstance(hits, tuple):
        t, u, v, prim, inst = hits
    else:
        t, u, v, prim, inst = (hits[k] for k in ("t", "u", "v", "prim", "inst"))
    t, u, v = np.asarray(t, F), np.asarray(u, F), np.asarray(v, F)
    prim, inst = np.asarray(prim, np.int64), np.asarray(inst, np.int64)
    imesh = np.asarray(instance_mesh, np.int64)
    out = np.zeros((len(t), 4), F)
    hit = t < FAR
    mi = np.where(hit, imesh[np.where(hit, inst, 0)], -1)
    for m, (now, snap) in enumerate(zip(meshes_now, meshes_snapshot)):
        sel = np.flatnonzero(mi == m)
        if snap is None or sel.size == 0:
            continue
        c, q = corners(now)[prim[sel]], corners(snap)[prim[sel]]
        d = q - c
        uu, vv = u[sel][:, None], v[sel][:, None]
        w0 = (F(1) - uu) - vv
        xyz = (w0 * d[:, 0] + uu * d[:, 1]) + vv * d[:, 2]
        assert xyz.dtype == F
        out[sel, :3] = xyz
        out[sel, 3] = 1
    return out


def reproject_deform(color, normal_depth, instance, cam, W, H, history=None, history_nd=None, prev_cam=None,
                     history_instance=None, motion=None, history_moments=None, offset=None, prev_transforms=None,
                     depth_tol=0.05, normal_min=0.9, max_history=16.0, clamp_k=0.0, min_temporal=4.0, info=None):
    """The arguments of vr.reproject_moments, and offset: float32 [W*H, 4] (offset_ref's), prev_transforms: float32
    [count, 4, 4]; both None or both given, and given only with a history.  Returns (out [W*H, 4], moments [W*H, 4]).
    info (a dict) receives vr.reproject_moments' masks and Xp [W*H, 3] (the point carried back), ws [W*H]."""
    assert (offset is None) == (prev_transforms is None) and (offset is None or history is not None)
    color = np.asarray(color, F).reshape(H, W, 4)
    nd = np.asarray(normal_depth, F).reshape(H, W, 4)
    ids = np.asarray(instance, np.uint32).reshape(H, W)
    clamp_k, min_temporal = F(clamp_k), F(min_temporal)
    hit = nd[..., 3] < FAR
    L = vr.luminance(color)
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
            sel = np.where(known, ids, np.uint32(0)).astype(np.int64)
            A = mo[sel]
            ys, xs = np.mgrid[0:H, 0:W]
            u = xs.astype(F) * (F(1) / fW)
            v = ys.astype(F) * (F(1) / fH)
            P = (TL + u[..., None] * (TR - TL)) + v[..., None] * (BL - TL)
            d = P - pos
            D = d * (F(1) / np.sqrt(rr._dot(d, d)))[..., None]
            X = pos + Z[..., None] * D
            Xp = np.stack([mr._row3(A, r, X) + A[..., r, 3] for r in range(3)], axis=-1)
            if offset is not None:  # the one change: the surface point itself moved within its mesh
                off = np.asarray(offset, F).reshape(H, W, 4)
                pl = np.asarray(prev_transforms, F).reshape(-1, 4, 4)
                assert len(pl) == count
                Lm = pl[sel]
                moved = Xp + np.stack([mr._row3(Lm, r, off[..., :3]) for r in range(3)], axis=-1)
                Xp = np.where((off[..., 3] != 0)[..., None], moved, Xp)
            assert Xp.dtype == F
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
            rgb = hc + a[..., None] * (color[..., :3] - hc)
            blended = np.concatenate([rgb, ln[..., None]], axis=-1)
            out = np.where(ok[..., None], blended, fresh)
            m1 = np.where(ok, hm[..., 0] + a * (L - hm[..., 0]), L)
            m2 = np.where(ok, hm[..., 1] + a * (L * L - hm[..., 1]), L * L)
            assert out.dtype == F and m1.dtype == F and m2.dtype == F
            if info is not None:
                info.update(hit=hit.ravel(), known=known.ravel(), valid=valid.ravel(), has_history=ok.ravel(),
                            px=px.ravel(), py=py.ravel(), Xp=Xp.reshape(-1, 3), ws=ws.ravel(), X=X.reshape(-1, 3))
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


# ---- the deforming sequence: multi_96x72 with instance MOVER on a mesh of its own (a copy of the height field), which
# deforms by deform.travelling_sine with t = k * DT at frame k; nothing else moves, the camera rests
SCENE, MOVER, FRAMES = mr.SCENE, mr.MOVER, 8
AMP, DT, WAVE_K = 1.5, 0.5, 0.5


def scene():
    """(sd, W, H): the scene with meshes [height field, its copy] and instance MOVER on mesh 1."""
    sd, W, H = dr.scene_of(SCENE)
    inst = [(1 if i == MOVER else mi, T) for i, (mi, T) in enumerate(sd.instances)]
    return dataclasses.replace(sd, meshes=[sd.meshes[0], sd.meshes[0]], instances=inst, name=sd.name + "+own"), W, H


def mesh_at(k, amp=AMP, dt=DT):
    sd, _, _ = dr.scene_of(SCENE)
    return deform.travelling_sine(sd.meshes[0], amp, t=k * dt, k=WAVE_K)


def scene_at(k, amp=AMP, dt=DT):
    sd, W, H = scene()
    return dataclasses.replace(sd, meshes=[sd.meshes[0], mesh_at(k, amp, dt)]), W, H


def instance_mesh(sd):
    return np.asarray([mi for mi, _ in sd.instances], np.int64)


def transforms(sd):
    return np.stack([np.asarray(T, F).reshape(4, 4) for _, T in sd.instances])


def with_offsets(vs):
    """The views `vs` (dicts with hits, sd among the rest) with off: offset_ref of frame k against frame k - 1's
    geometry of mesh 1, the mesh snapshotted after every frame (frame 0: no snapshot)."""
    out = []
    for k, v in enumerate(vs):
        snap = [None, vs[k - 1]["sd"].meshes[1]] if k else [None, None]
        out.append(dict(v, off=offset_ref(v["hits"], instance_mesh(v["sd"]), v["sd"].meshes, snap)))
    return out


def step(vs, k, hist, W, H, follow=True, **par):
    """Frame k of the views reprojected onto hist = (out, moments) of frame k - 1 (None starts a history): by
    reproject_deform with the views' offsets (follow) or by vr.reproject_moments (the baseline)."""
    v = vs[k]
    if hist is None:
        return vr.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], W, H, **par)
    u = vs[k - 1]
    mo = mr.motion_f32(v["xf"], u["xf"])
    if not follow:
        return vr.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"],
                                    u["ids"], mo, hist[1], **par)
    return reproject_deform(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"], u["ids"], mo,
                            hist[1], v["off"], u["xf"], **par)


def chain(vs, W, H, follow=True, **par):
    outs, hist = [], None
    for k in range(len(vs)):
        hist = step(vs, k, hist, W, H, follow, **par)
        outs.append(hist)
    return outs


def figures(vs, base_out, new_out, conv):
    """Over the last frame: the fraction with history and the RMSE against `conv` over the deforming instance's pixels
    for the baseline and the new pass, and the RMSE over the other hit pixels."""
    ids = vs[-1]["ids"]
    mover, static = ids == MOVER, (ids != MOVER) & (ids != mr.MISS)
    assert mover.any() and static.any()
    return dict(frac_base=float(mr.has_history(base_out)[mover].mean()),
                frac_new=float(mr.has_history(new_out)[mover].mean()),
                rmse_frame=dr.rmse(vs[-1]["color"][mover], conv[mover]),
                rmse_base=dr.rmse(base_out[mover], conv[mover]), rmse_new=dr.rmse(new_out[mover], conv[mover]),
                static_base=dr.rmse(base_out[static], conv[static]), static_new=dr.rmse(new_out[static], conv[static]))


# measured with this reference on the oracle's frames (DESIGN.md "Deforming meshes"): the fraction with history over
# the deforming instance's pixels of the last frame, and the RMSE ratio new / baseline
MEASURED = dict(frac_base=0.3202, frac_new=0.8258, ratio=0.5598)


def check_quality(f, measured=None):
    """The new pass's fraction exceeds the baseline's by at least half the measured gain, its RMSE ratio to the
    baseline is below the midpoint between the measured ratio and 1, and the static pixels' RMSE agrees within 1e-6."""
    m = measured or MEASURED
    assert f["frac_new"] - f["frac_base"] >= 0.5 * (m["frac_new"] - m["frac_base"]), f
    assert f["rmse_new"] / f["rmse_base"] <= m["ratio"] + (1.0 - m["ratio"]) / 2.0, f
    assert abs(f["static_new"] - f["static_base"]) <= 1e-6, f


# ---- oracle frames of the sequence (made once per process, never modified)
_views, _conv = {}, {}


def oracle_view(k, amp=AMP, dt=DT):
    """dict(cam, color, nd, ids, xf, hits, sd) of frame k: the oracle's 2-spp depth-4 frame (frame_index k), guides,
    first hits and the scene at frame k."""
    import oracle
    import prt
    key = (k, amp, dt)
    if key not in _views:
        sd, W, H = scene_at(k, amp, dt)
        osc = oracle.OracleScene(sd, W, H)
        _, nd, _, _ = dr.oracle_guides(osc, W, H, oracle.NORMALMAP)
        hits = osc.primary_hits(W, H)
        color = osc.render(W, H, spp=2, bounces=4, frame_index=k)[0]
        cam = prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H))
        _views[key] = dict(cam=cam, color=color, nd=nd, ids=mr.ids_of(hits[0], hits[4]), xf=transforms(sd), hits=hits,
                           sd=sd)
    return _views[key]


def oracle_views(amp=AMP, dt=DT):
    return with_offsets([oracle_view(k, amp, dt) for k in range(FRAMES)])


def oracle_converged(amp=AMP, dt=DT):
    """The oracle's 1024-spp frame (frame_index 1000) of the last frame's geometry."""
    import oracle
    key = (amp, dt)
    if key not in _conv:
        sd, W, H = scene_at(FRAMES - 1, amp, dt)
        _conv[key] = oracle.OracleScene(sd, W, H).render(W, H, spp=1024, bounces=4, frame_index=1000)[0]
    return _conv[key]
