"""CPU tests of the definition of the reprojection that follows deforming meshes (tests/deform_ref.py, the numpy float32
reference the GPU passes must match bit for bit) on the oracle's frames, and of the host-only part of its C ABI
(include/prt.h prt_snapshot_mesh, prt_render_aov_deform, prt_reproject_deform: their refusals)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import deform
import deform_ref as df
import denoise_ref as dr
import motion_ref as mr
import variance_ref as vr
import prt
from prt import _lib

F = np.float32
U = 2.0 ** -24  # the unit roundoff of float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("par", [dict(), dict(clamp_k=1.5, min_temporal=1.0)], ids=["defaults", "clamp"])
def test_no_offset_and_zero_offset_equal_the_moments_pass(oracle_mod, par):
    """Sequence B/slow (a moving instance and a moving camera), steps 1 and 2: offset=None gives
    vr.reproject_moments' output bit for bit, and so does an all-zero offset with w = 1 (every added term is +0)."""
    _, W, H = dr.scene_of(mr.SCENE)
    vs = [mr.view("B", "slow", k) for k in range(3)]
    hist = vr.step(vs, 0, None, W, H, **par)
    for k in (1, 2):
        v, u = vs[k], vs[k - 1]
        mo = mr.motion_f32(v["xf"], u["xf"])
        info = {}
        want = vr.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"],
                                    u["ids"], mo, hist[1], info=info, **par)
        assert info["has_history"].any() and (info["hit"] & ~info["has_history"]).any()
        none = df.reproject_deform(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"],
                                   u["ids"], mo, hist[1], **par)
        zero = np.zeros((W * H, 4), F)
        zero[:, 3] = 1
        zinfo = {}
        zer = df.reproject_deform(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"],
                                  u["ids"], mo, hist[1], zero, u["xf"], info=zinfo, **par)
        for got in (none, zer):
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), k
        assert np.array_equal(zinfo["has_history"], info["has_history"])
        hist = want
    fresh = df.reproject_deform(vs[0]["color"], vs[0]["nd"], vs[0]["ids"], vs[0]["cam"], W, H, **par)
    want = vr.step(vs, 0, None, W, H, **par)
    assert np.array_equal(_bits(fresh[0]), _bits(want[0])) and np.array_equal(_bits(fresh[1]), _bits(want[1]))


def test_offset_rows(oracle_mod):
    """Frame 1 of the deforming sequence: misses and the pixels of the mesh without a snapshot get zero rows, the
    deforming instance's pixels (offset, 1) with a non-zero offset; a snapshot equal to the current positions gives
    exactly (0, 0, 0, 1); no snapshot at all gives zeros everywhere."""
    v = df.oracle_views()[1]
    ids, off = v["ids"], v["off"]
    mover = ids == df.MOVER
    assert mover.any() and (ids == mr.MISS).any() and (~mover & (ids != mr.MISS)).any()
    assert not off[~mover].any()
    assert np.all(off[mover, 3] == 1) and np.all(np.any(off[mover, :3] != 0, axis=1))
    same = df.offset_ref(v["hits"], df.instance_mesh(v["sd"]), v["sd"].meshes, list(v["sd"].meshes))
    hit = ids != mr.MISS
    assert np.array_equal(_bits(same[hit]), _bits(np.tile(np.array([0, 0, 0, 1], F), (hit.sum(), 1))))
    assert not same[~hit].any()
    assert not df.offset_ref(v["hits"], df.instance_mesh(v["sd"]), v["sd"].meshes, [None, None]).any()
    # the offset leads from the current surface point to the previous one: current point + offset is the point with the
    # same barycentrics on the snapshotted triangle, up to the rounding of the interpolation
    t, u, w, prim, _ = v["hits"]
    sel = np.flatnonzero(mover)
    now, snap = df.corners(v["sd"].meshes[1]).astype(np.float64), df.corners(df.mesh_at(0)).astype(np.float64)
    bary = np.stack([1.0 - u[sel].astype(np.float64) - w[sel], u[sel], w[sel]], 1)
    p_now = np.einsum("nk,nkj->nj", bary, now[prim[sel]])
    p_old = np.einsum("nk,nkj->nj", bary, snap[prim[sel]])
    assert np.allclose(p_now + off[sel, :3], p_old, atol=1e-5)


def _dyadic_case():
    """The rigid case: mesh 1 with coordinates that are multiples of 2^-8 moves by the object-space translation TAU
    (dyadic, so every corner difference is exact) between frame 0 and frame 1."""
    sd, W, H = df.scene()
    P = np.round(deform.positions(sd.meshes[0]) * 256.0) / 256.0
    m0 = deform.with_positions(sd.meshes[0], P)
    m1 = deform.with_positions(sd.meshes[0], P + TAU)
    assert np.array_equal(df.corners(m0) - df.corners(m1), np.broadcast_to(-TAU.astype(F), (m0.tri_count, 3, 3)))
    return [dataclasses.replace(sd, meshes=[sd.meshes[0], m]) for m in (m0, m1)], W, H


TAU = np.array([0.25, 0.125, -0.125])
# float32 roundings on the way to a coordinate of X' (DESIGN.md "Deforming meshes"): route A (the offset) -- w0 2, the
# interpolation 5, L * delta 5, the final sum 1 (the identity motion's row4 is exact); route B (the instance
# transform) -- the translated transform's rounding 1, the motion matrix's entries 4 (three products and the
# translation), row4 6
N_A, N_B = 13, 11


def test_rigid_translation_equals_instance_motion(oracle_mod):
    """The same translation once as a deformation (offset = -TAU through prt_reproject_deform's definition, identity
    motion) and once through the instance transform (T * Translate(TAU), vr.reproject_moments): both carried-back
    points lie within N * 2^-24 * M of the float64 closed form X - L * TAU (M: the largest magnitude on the way), the
    has-history masks are equal, and the outputs agree within the bound that the two points' distance allows through
    the bilinear gather.  Measured: printed (DESIGN.md has the figures)."""
    import oracle
    (sd0, sd1), W, H = _dyadic_case()
    views = []
    for k, sd in enumerate((sd0, sd1)):
        osc = oracle.OracleScene(sd, W, H)
        _, nd, _, _ = dr.oracle_guides(osc, W, H, oracle.NORMALMAP)
        hits = osc.primary_hits(W, H)
        color = osc.render(W, H, spp=2, bounces=4, frame_index=k)[0]
        views.append(dict(cam=prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H)), color=color, nd=nd,
                          ids=mr.ids_of(hits[0], hits[4]), xf=df.transforms(sd), hits=hits, sd=sd))
    u, v = views
    hist = vr.reproject_moments(u["color"], u["nd"], u["ids"], u["cam"], W, H)
    off = df.offset_ref(v["hits"], df.instance_mesh(sd1), sd1.meshes, [None, sd0.meshes[1]])
    mover = v["ids"] == df.MOVER
    assert mover.any() and np.allclose(off[mover, :3], -TAU, atol=1e-6) and not off[~mover].any()
    ia, ib = {}, {}
    A = df.reproject_deform(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"], u["ids"],
                            mr.identity(len(v["xf"])), hist[1], off, u["xf"], info=ia)
    xf_b = v["xf"].copy()
    tr = np.eye(4)
    tr[:3, 3] = TAU
    xf_b[df.MOVER] = (v["xf"][df.MOVER].astype(np.float64) @ tr).astype(F)
    mo_b = mr.motion_f32(xf_b, u["xf"])
    B = df.reproject_deform(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"], u["ids"], mo_b,
                            hist[1], info=ib)
    want = vr.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist[0], u["nd"], u["cam"], u["ids"],
                                mo_b, hist[1])
    assert np.array_equal(_bits(B[0]), _bits(want[0])) and np.array_equal(_bits(B[1]), _bits(want[1]))
    # the float64 closed form of the point carried back, and the largest magnitude met on the way
    Lm = u["xf"][df.MOVER, :3, :3].astype(np.float64)
    X = ia["X"][mover].astype(np.float64)
    closed = X - Lm @ TAU
    M = max(np.abs(X).max(), np.abs(closed).max()) + np.abs(Lm).sum(axis=1).max() * np.abs(TAU).sum()
    ea = np.abs(ia["Xp"][mover] - closed).max()
    eb = np.abs(ib["Xp"][mover] - closed).max()
    print(f"carried-back point against the float64 closed form: offset route {ea:.3e} (bound {N_A * U * M:.3e}), "
          f"transform route {eb:.3e} (bound {N_B * U * M:.3e}); M = {M:.3f}")
    assert ea <= N_A * U * M and eb <= N_B * U * M
    assert np.array_equal(ia["has_history"], ib["has_history"]) and ia["has_history"][mover].any()
    # through the projection: the screen plane is 2 away and 2 high, so a world displacement e at view depth z moves the
    # projection by at most 2 e H / z pixels per axis (lateral and along the view axis together), z >= Zp * cos(corner)
    e = (N_A + N_B) * U * M
    aspect = float(W) / float(H)
    cosc = 2.0 / np.sqrt(4.0 + 1.0 + aspect * aspect)
    zp = np.linalg.norm(closed - np.asarray(u["cam"].camPos, np.float64), axis=1).min()
    dp = 2.0 * e * H / (zp * cosc)
    # through the gather: each of the four weights moves by at most 2 dp, so h = (sum wb Hq) / ws by at most
    # 16 dp S / ws (S: the largest history value); every history length is 1 here, so len = 2, a = 1/2 and the output
    # moves by half of that; 64 roundings of S cover the arithmetic after the weights
    has = ia["has_history"] & mover
    ws = np.minimum(ia["ws"], ib["ws"])[has].astype(np.float64)
    for name, a, b, S in (("colour", A[0][has, :3], B[0][has, :3], float(np.abs(hist[0][:, :3]).max())),
                          ("moments", A[1][has, :2], B[1][has, :2], float(np.abs(hist[1][:, :2]).max()))):
        tol = 8.0 * dp * S / ws + 64 * U * S
        err = np.abs(a.astype(np.float64) - b).max(axis=1)
        print(f"{name}: max |offset route - transform route| {err.max():.3e}, smallest bound {tol.min():.3e}, "
              f"dp {dp:.3e} pixels")
        assert np.all(err <= tol)
    assert np.array_equal(A[0][has, 3], B[0][has, 3]) and np.all(A[0][has, 3] == 2)
    rest = ~mover
    assert np.array_equal(_bits(A[0][rest]), _bits(B[0][rest])) and np.array_equal(_bits(A[1][rest]), _bits(B[1][rest]))


def test_quality_and_coverage(oracle_mod):
    """multi_96x72 with the mover on a mesh of its own that deforms by deform.travelling_sine (amplitude 1.5, k 0.5,
    t = 0.5 per frame), eight 2-spp frames at depth 4, each pass chained on its own output; over the deforming
    instance's pixels of the last frame against the oracle's 1024-spp frame.  Measured with this reference (DESIGN.md
    "Deforming meshes"): fraction with history 0.3202 -> 0.8258, RMSE 0.3933 -> 0.2202 (ratio 0.5598; the frame alone
    0.4411); the static hit pixels 0.1466 in both."""
    _, W, H = df.scene()
    vs = df.oracle_views()
    base = df.chain(vs, W, H, follow=False)[-1][0]
    new = df.chain(vs, W, H, follow=True)[-1][0]
    assert np.all(np.isfinite(new))
    f = df.figures(vs, base, new, df.oracle_converged())
    print(", ".join(f"{k} {v:.4f}" for k, v in f.items()) + f", ratio {f['rmse_new'] / f['rmse_base']:.4f}")
    df.check_quality(f)


def test_abi_without_a_device():
    """The three entry points refuse NULL, and prt_reproject_deform's own argument rules answer
    PRT_ERR_INVALID_ARGUMENT before the context is used (a fake non-NULL handle is never dereferenced), leaving the
    outputs untouched."""
    L = prt.load()
    assert L.prt_snapshot_mesh(None, 0) == -1
    bufs = [np.zeros((16, 4), F) for _ in range(9)]
    col, nd, hist, hnd, hmom, off, out, mom, alb = (b.ctypes.data for b in bufs)
    idb = [np.zeros(16, np.uint32) for _ in range(3)]
    ids, hids, out8 = (b.ctypes.data for b in idb)
    assert L.prt_render_aov_deform(None, 4, 4, 0, alb, nd, ids, off, 0) == -1
    tp = prt.temporal_defaults()
    mo, pxf = mr.identity(2), np.tile(np.eye(4, dtype=F).ravel(), (2, 1))
    cam = _lib.CameraDesc()
    cp = C.byref(cam)
    fake = C.c_void_p(col)

    def call(ctx=fake, p=tp, W=4, H=4, c=cp, color=col, g=nd, i=ids, pc=cp, h=hist, hg=hnd, hi=hids,
             m=mo.ctypes.data, n=2, hm=hmom, of=off, px=pxf.ctypes.data, o=out, om=mom, o8=out8):
        return L.prt_reproject_deform(ctx, C.byref(p) if p is not None else None, W, H, c, color, g, i, pc, h, hg, hi,
                                      m, n, hm, of, px, o, om, o8, 0)

    assert call(ctx=None) == -1 and call(p=None) == -1 and call(c=None) == -1
    assert call(color=None) == -1 and call(g=None) == -1 and call(i=None) == -1 and call(om=None) == -1
    assert call(o=None, o8=None) == -1 and call(W=0) == -1 and call(H=-3) == -1
    # offset and prev_transforms go together, and only with a history
    assert call(of=None) == -1 and call(px=None) == -1
    none = dict(pc=None, h=None, hg=None, hi=None, m=None, n=0, hm=None)
    assert call(**none) == -1 and call(of=None, **none) == -1 and call(px=None, **none) == -1
    assert call(o=off) == -1 and call(om=off) == -1  # the offset is an input
    # prt_reproject_moments' rules hold: the history group, the aliasing
    for kw in (dict(pc=None), dict(h=None), dict(hg=None), dict(m=None), dict(n=0), dict(n=-1), dict(hm=None)):
        assert call(**kw) == -1, kw
    assert call(o=col) == -1 and call(o=hist) == -1 and call(om=hmom) == -1 and call(o8=ids) == -1
    assert call(p=prt.temporal_defaults(clamp_k=-1.0)) == -1 and call(p=prt.temporal_defaults(min_temporal=0.5)) == -1
    assert not any(b.any() for b in bufs) and not any(b.any() for b in idb)
