"""CPU tests of the definitions of the moments-carrying reprojection and the variance-guided filter
(tests/variance_ref.py, the numpy float32 reference the GPU passes must match bit for bit) on the oracle's frames, and
of the host-only part of their C ABI (include/prt.h prt_temporal_defaults, prt_denoise_variance_defaults and the
refusals of prt_reproject_moments / prt_denoise_variance)."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import motion_ref as mr
import reproject_ref as rr
import variance_ref as vr
import prt
from prt import _lib

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _views(mseq, cseq):
    return [mr.view(mseq, cseq, k) for k in range(mr.FRAMES)]


# ---- the identities that pin the definition to the existing passes
@pytest.mark.parametrize("cseq", ["rest", "slow"])
def test_colour_equals_reproject_motion(oracle_mod, cseq):
    """(a) clamp_k = 0: at every step of B/rest and B/slow the colour output is mr.reproject_motion's bit for bit."""
    _, W, H = dr.scene_of(mr.SCENE)
    vs = _views("B", cseq)
    got, want = vr.chain(vs, W, H), vr.motion_chain(vs, W, H)
    assert np.any(want[-1][:, 3] > 1) and np.any(want[-1][:, 3] == 1)
    for k in range(mr.FRAMES):
        assert np.array_equal(_bits(got[k][0]), _bits(want[k])), k


@pytest.mark.parametrize("name", list(dr.CASES))
def test_identity_equals_plain_pass(oracle_mod, name):
    """(b) identity matrices, no history ids, clamp_k = 0: the colour output is rr.reproject's bit for bit (`slow`
    step 1, where both the blend and the start-over branch occur)."""
    _, W, H = dr.scene_of(name)
    a, b = rr.view(name, "slow", 0, frame=True), rr.view(name, "slow", 1, frame=True)
    ia, ib = mr.oracle_ids(name, "slow", 0), mr.oracle_ids(name, "slow", 1)
    count = int(ib[ib != mr.MISS].max()) + 1
    hist = rr.reproject(a["color"], a["nd"], a["cam"], W, H)
    h0, m0 = vr.reproject_moments(a["color"], a["nd"], ia, a["cam"], W, H)
    assert np.array_equal(_bits(h0), _bits(hist))
    info = {}
    want = rr.reproject(b["color"], b["nd"], b["cam"], W, H, hist, a["nd"], a["cam"], info=info)
    got, _ = vr.reproject_moments(b["color"], b["nd"], ib, b["cam"], W, H, hist, a["nd"], a["cam"], None,
                                  mr.identity(count), m0)
    assert info["has_history"].any() and (info["hit"] & ~info["has_history"]).any()
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", list(dr.CASES))
def test_ones_variance_equals_denoise(oracle_mod, name):
    """(c) the variance 1 everywhere, variance_floor <= 1, color_decay 0.5, one iteration: G3 is x / x = 1 and
    sc2 * 1 = sc2, so the colour is dr.denoise(iterations=1)'s bit for bit; the variance output is not all ones."""
    c = dr.case(name)
    W, H = c["W"], c["H"]
    mom = np.zeros((W * H, 4), F)
    mom[:, 2] = 1
    par = dict(dr.DEFAULTS, iterations=1)
    want = dr.denoise(c["noisy"], c["albedo"], c["nd"], W, H, **par)
    got, var = vr.denoise_variance(c["noisy"], mom, c["albedo"], c["nd"], W, H, color_decay=0.5, variance_floor=1.0,
                                   **par)
    assert np.array_equal(_bits(got), _bits(want))
    hit = c["nd"][:, 3] < dr.FAR
    assert np.all(var[~hit] == 1) and np.all(var[hit] <= 1) and np.any(var[hit] < 1) and np.all(var[hit] > 0)


# ---- the moments
def test_moments_at_rest(oracle_mod):
    """Frozen mover, resting camera, 8 frames.  Per hit pixel m1 follows m_k = h + (L_k - h) / len_k, with h the
    gather of m_{k-1}; were h = m_{k-1}(p) and len_k = k exactly, m_8 would be the mean of the eight luminances.  Two
    things separate it from that mean.  (1) Rounding: one step is the gather (4 products, 4 sums, a division), 1 / len
    and the blend (3 operations), under 16 roundings of values no larger than Lmax, and the factor 1 - 1 / len <= 1
    does not amplify what the step before left: <= 7 * 16 * 2^-24 * Lmax over the 7 blending steps.  (2) The
    reprojected position of a pixel at rest is its own centre only up to rounding, eps = max |px - x|, |py - y| (read
    from the reference's own geometry, info['px'] / info['py']), so the other taps enter with weight <= 2 eps and
    values within Lmax of the pixel's: <= 7 * 2 * eps * Lmax.  The bound is the sum of the two.
    Also: var >= 0, a miss has var 0 and carries (L, L * L), and the spatial estimate serves the first min_temporal - 1
    frames and the temporal one afterwards (both branches occur)."""
    _, W, H = dr.scene_of(mr.SCENE)
    vs = _views("frozen", "rest")
    infos = []
    outs = vr.chain(vs, W, H, infos=infos)
    hit = vs[0]["ids"] != mr.MISS
    assert 0 < hit.sum() < hit.size
    Ls = np.stack([vr.luminance(np.asarray(v["color"])) for v in vs]).astype(np.float64)
    ys, xs = np.divmod(np.arange(W * H), W)
    eps = max(float(np.abs(i["px"][hit] - xs[hit]).max()) for i in infos[1:])
    eps = max(eps, max(float(np.abs(i["py"][hit] - ys[hit]).max()) for i in infos[1:]))
    assert eps < 1e-3  # at rest
    bound = 7 * (16 * 2.0 ** -24 + 2 * eps) * Ls.max()
    m1 = outs[-1][1][:, 0].astype(np.float64)
    err = np.abs(m1 - Ls.mean(axis=0))[hit].max()
    print(f"m1 against the mean of 8 luminances: max error {err:.3e}, bound {bound:.3e} (eps {eps:.3e}, "
          f"Lmax {Ls.max():.3f})")
    assert err <= bound
    for k, (out, mom) in enumerate(outs):
        assert np.all(np.isfinite(mom)) and np.all(mom[:, 2] >= 0) and np.all(mom[:, 3] == 0), k
        assert np.all(mom[~hit, 2] == 0), k
        L = vr.luminance(np.asarray(vs[k]["color"]))
        assert np.array_equal(_bits(mom[~hit, 0]), _bits(L[~hit]))
        assert np.array_equal(_bits(mom[~hit, 1]), _bits((L * L)[~hit]))
        assert np.array_equal(infos[k]["temporal"] | infos[k]["spatial"], hit)
        assert np.array_equal(infos[k]["temporal"], hit & (out[:, 3] >= F(4)))
    assert infos[0]["spatial"][hit].all() and infos[2]["spatial"][hit].all()
    assert infos[7]["temporal"][hit].all()
    # the temporal variance is the moments' own
    out, mom = outs[-1]
    t = infos[7]["temporal"]
    assert np.array_equal(_bits(mom[t, 2]), _bits(np.fmax(mom[t, 1] - mom[t, 0] * mom[t, 0], F(0))))
    assert np.any(mom[t, 2] > 0)


def test_spatial_estimate_serves_short_histories(oracle_mod):
    """B/slow, the last frame: the disoccluded pixels (history shorter than min_temporal) carry the spatial estimate --
    recomputed here per pixel in a plain loop over the 5 x 5 window -- and the others the temporal one; both occur.
    min_temporal = 1 leaves no spatial pixel, and a pixel that starts over then has variance 0."""
    _, W, H = dr.scene_of(mr.SCENE)
    vs = _views("B", "slow")
    infos = []
    out, mom = vr.chain(vs, W, H, infos=infos)[-1]
    sp, tp = infos[-1]["spatial"], infos[-1]["temporal"]
    print(f"B/slow frame 7: {tp.sum()} temporal, {sp.sum()} spatial of {infos[-1]['hit'].sum()} hit pixels")
    assert sp.sum() > 50 and tp.sum() > 50 and np.all(out[sp, 3] < 4) and np.all(out[tp, 3] >= 4)
    v = vs[-1]
    L = vr.luminance(np.asarray(v["color"])).reshape(H, W)
    ids, hit = v["ids"].reshape(H, W), (v["nd"][:, 3] < dr.FAR).reshape(H, W)
    for p in np.flatnonzero(sp)[::7]:
        y, x = divmod(int(p), W)
        s1, s2, n = F(0), F(0), F(0)
        for qy in range(y - 2, y + 3):
            for qx in range(x - 2, x + 3):
                if 0 <= qy < H and 0 <= qx < W and hit[qy, qx] and ids[qy, qx] == ids[y, x]:
                    s1, s2, n = s1 + L[qy, qx], s2 + L[qy, qx] * L[qy, qx], n + F(1)
        mu = s1 / n
        want = np.fmax(s2 / n - mu * mu, F(0)) * (F(4) / out[p, 3])
        assert _bits(mom[p, 2]) == _bits(want), (p, mom[p, 2], want)
    infos = []
    out1, mom1 = vr.chain(vs, W, H, infos=infos, min_temporal=1.0)[-1]
    assert not infos[-1]["spatial"].any()
    assert np.array_equal(_bits(out1), _bits(out))
    assert np.all(mom1[out1[:, 3] == 1, 2] == 0)


# ---- the clamp
def test_clamp_bounds_the_history(oracle_mod):
    """clamp_k = 1.5 on B/slow: at every step the clamped history of every blended pixel lies in [mu - k sigma,
    mu + k sigma] of the 3 x 3 neighbourhood (recomputed here in float64 for a sample of pixels, borders included),
    some histories are moved by the clamp, and the output is the blend of the clamped history."""
    _, W, H = dr.scene_of(mr.SCENE)
    vs = _views("B", "slow")
    infos = []
    outs = vr.chain(vs, W, H, infos=infos, clamp_k=1.5)
    plain = vr.chain(vs, W, H)
    moved = 0
    for k in range(1, mr.FRAMES):
        i, has = infos[k], infos[k]["has_history"]
        assert has.any()
        assert np.all(i["clamped"][has] >= i["lo"][has]) and np.all(i["clamped"][has] <= i["hi"][has])
        col = np.asarray(vs[k]["color"], np.float64).reshape(H, W, 4)[..., :3]
        for p in np.flatnonzero(has)[::11]:
            y, x = divmod(int(p), W)
            win = col[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].reshape(-1, 3)
            mu, sg = win.mean(axis=0), win.std(axis=0)
            tol = 1e-5 * (1 + np.abs(win).max())
            assert np.all(i["clamped"][p] >= mu - 1.5 * sg - tol) and np.all(i["clamped"][p] <= mu + 1.5 * sg + tol)
        out = outs[k][0]
        a = F(1) / out[has, 3]
        c = np.asarray(vs[k]["color"])[has, :3]
        hc = i["clamped"][has]
        assert np.array_equal(_bits(out[has, :3]), _bits(hc + a[:, None] * (c - hc)))
        moved += int(np.any(_bits(out[has]) != _bits(plain[k][0][has]), axis=1).sum())
    assert moved > 100
    border = np.zeros((H, W), bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    assert (infos[-1]["has_history"] & border.ravel()).any()


def test_lighting_change(oracle_mod):
    """8 frames at rest on multi_96x72, the four point lights' colours permuted from frame 4 on: against the oracle's
    1024-spp frame under the new lights, the RMSE of each of the frames 4..7 is lower with the clamp (k = 1.5) than
    without.  Measured: 0.1412 -> 0.1282, 0.1286 -> 0.1165, 0.1187 -> 0.1083, 0.1116 -> 0.1019."""
    vs, conv, W, H = vr.light_views()
    assert not np.array_equal(vs[3]["color"], vs[4]["color"])
    off, on = vr.chain(vs, W, H), vr.chain(vs, W, H, clamp_k=1.5)
    pairs = [(dr.rmse(off[k][0], conv), dr.rmse(on[k][0], conv)) for k in range(vr.LIGHT_CHANGE, vr.LIGHT_FRAMES)]
    print("lighting change, RMSE without / with the clamp: " + ", ".join(f"{a:.4f} / {b:.4f}" for a, b in pairs))
    for a, b in pairs:
        assert b < a


# ---- quality
def test_default_sigma_color_is_the_grid_minimum(oracle_mod):
    """The default sigma_color (2) is the one of {0.5, 1, 2, 4, 8} with the least RMSE on B/rest (color_decay 1)."""
    rm = {s: vr.quality("B/rest", sigma_color=s)[0] for s in (0.5, 1.0, 2.0, 4.0, 8.0)}
    print("B/rest RMSE by sigma_color: " + ", ".join(f"{s}: {v:.4f}" for s, v in rm.items()))
    assert min(rm, key=rm.get) == vr.FILTER_DEFAULTS["sigma_color"]


@pytest.mark.parametrize("key", vr.QUALITY)
def test_quality(oracle_mod, key):
    """The last frame of an 8-frame sequence: RMSE of denoise_variance(reproject_moments chain) over RMSE of the
    parent pipeline (dr.denoise with dr.DEFAULTS of the reproject_motion chain), both against the oracle's 1024-spp
    frame, is at most halfway from the measured ratio (vr.MEASURED) to 1.  sigma_color was chosen on B/rest alone."""
    new, old = vr.quality(key)
    print(f"{key}: RMSE {new:.4f} against the parent's {old:.4f}, ratio {new / old:.4f} "
          f"(measured {vr.MEASURED[key]:.4f}, limit {vr.bound(vr.MEASURED[key]):.4f})")
    assert new / old <= vr.bound(vr.MEASURED[key])


# ---- the host-side ABI
def test_defaults():
    tp, dp = prt.temporal_defaults(), prt.denoise_variance_defaults()
    got = {k: getattr(tp, k) for k, _ in tp._fields_}
    assert got == {k: F(v) for k, v in vr.TEMPORAL_DEFAULTS.items()}
    rp = prt.reproject_defaults()
    assert (tp.depth_tol, tp.normal_min, tp.max_history) == (rp.depth_tol, rp.normal_min, rp.max_history)
    got = {k: getattr(dp, k) for k, _ in dp._fields_}
    want = {k: (v if isinstance(v, int) else F(v)) for k, v in vr.FILTER_DEFAULTS.items()}
    assert got == want
    L = prt.load()
    assert L.prt_temporal_defaults(None) == -1 and L.prt_denoise_variance_defaults(None) == -1
    with pytest.raises(TypeError):
        prt.temporal_defaults(sigma=1)
    with pytest.raises(TypeError):
        prt.denoise_variance_defaults(clamp_k=1)


def test_reproject_moments_abi_without_a_device():
    """Every refusal of prt_reproject_moments comes with PRT_ERR_INVALID_ARGUMENT before the context is used (a fake
    non-NULL handle is never dereferenced) and leaves the outputs untouched."""
    L = prt.load()
    tp = prt.temporal_defaults()
    bufs = [np.zeros((16, 4), F) for _ in range(7)]
    col, nd, hist, hnd, hmom, out, omom = (b.ctypes.data for b in bufs)
    idb = [np.zeros(16, np.uint32) for _ in range(3)]
    ids, hids, out8 = (b.ctypes.data for b in idb)
    mo = mr.identity(2)
    cam = _lib.CameraDesc()
    cp = C.byref(cam)
    fake = C.c_void_p(col)

    def call(ctx=fake, p=tp, W=4, H=4, c=cp, color=col, g=nd, i=ids, pc=cp, h=hist, hg=hnd, hi=hids,
             m=mo.ctypes.data, n=2, hm=hmom, o=out, om=omom, o8=out8):
        return L.prt_reproject_moments(ctx, C.byref(p) if p is not None else None, W, H, c, color, g, i, pc, h, hg,
                                       hi, m, n, hm, o, om, o8, 0)

    assert call(ctx=None) == -1 and call(p=None) == -1 and call(c=None) == -1
    assert call(color=None) == -1 and call(g=None) == -1 and call(o=None, o8=None) == -1
    assert call(om=None) == -1  # out_moments is required
    assert call(i=None) == -1  # the ids are always required ...
    assert call(i=None, pc=None, h=None, hg=None, hi=None, m=None, n=0, hm=None) == -1  # ... even to start a history
    assert call(W=0) == -1 and call(H=-3) == -1
    for kw in (dict(depth_tol=-0.1), dict(depth_tol=float("nan")), dict(normal_min=1.5), dict(max_history=0.5),
               dict(max_history=float("nan")), dict(clamp_k=-0.5), dict(clamp_k=float("nan")),
               dict(clamp_k=float("inf")), dict(min_temporal=0.5), dict(min_temporal=float("nan")),
               dict(min_temporal=float("inf"))):
        assert call(p=prt.temporal_defaults(**kw)) == -1, kw
    # prev_camera, history, its normal_depth, motion, count > 0 and history_moments go together
    for kw in (dict(pc=None), dict(h=None), dict(hg=None), dict(m=None), dict(n=0), dict(n=-1), dict(hm=None),
               dict(pc=None, h=None, hg=None, m=None, n=0), dict(pc=None, h=None, hg=None, m=None, hm=None),
               dict(pc=None, h=None, hg=None, hi=None, m=None, n=0), dict(h=None, hm=None),
               dict(pc=None, h=None, hg=None, m=None, n=0, hm=None),  # history_instance alone
               dict(pc=None, h=None, hg=None, hi=None, m=None, n=-2, hm=None)):
        assert call(**kw) == -1, kw
    assert call(o=col) == -1  # the pass reads the neighbours of color_rgba
    assert call(o=col, pc=None, h=None, hg=None, hi=None, m=None, n=0, hm=None) == -1
    assert call(om=hmom) == -1  # taps are gathered
    assert call(o=hist) == -1 and call(o=hnd) == -1 and call(o=hmom) == -1 and call(o=omom) == -1
    assert call(om=col) == -1 and call(om=hist) == -1 and call(o8=hids) == -1 and call(o8=ids) == -1
    assert not any(b.any() for b in bufs) and not any(b.any() for b in idb)


def test_denoise_variance_abi_without_a_device():
    """Every refusal of prt_denoise_variance: NULL arguments, sizes, the parameter ranges (variance_floor <= 0 among
    them) and a NULL albedo with sigma_albedo > 0."""
    L = prt.load()
    dp = prt.denoise_variance_defaults()
    bufs = [np.zeros((16, 4), F) for _ in range(5)]
    col, mom, alb, nd, out = (b.ctypes.data for b in bufs)
    var, out8 = np.zeros(16, F), np.zeros(16, np.uint32)
    fake = C.c_void_p(col)

    def call(ctx=fake, p=dp, W=4, H=4, c=col, m=mom, a=alb, g=nd, o=out, v=var.ctypes.data, o8=out8.ctypes.data):
        return L.prt_denoise_variance(ctx, C.byref(p) if p is not None else None, W, H, c, m, a, g, o, v, o8, 0)

    assert call(ctx=None) == -1 and call(p=None) == -1 and call(c=None) == -1 and call(m=None) == -1
    assert call(g=None) == -1 and call(o=None, o8=None) == -1 and call(a=None) == -1
    assert call(W=0) == -1 and call(H=-1) == -1 and call(W=16385) == -1
    for kw in (dict(iterations=0), dict(iterations=9), dict(normal_power=-1), dict(normal_power=8),
               dict(sigma_color=0.0), dict(sigma_color=float("nan")), dict(sigma_depth=0.0), dict(sigma_albedo=-1.0),
               dict(color_decay=0.0), dict(color_decay=-1.0), dict(color_decay=float("inf")),
               dict(color_decay=float("nan")), dict(variance_floor=0.0), dict(variance_floor=-1e-6),
               dict(variance_floor=float("inf")), dict(variance_floor=float("nan"))):
        assert call(p=prt.denoise_variance_defaults(**kw)) == -1, kw
    assert not any(b.any() for b in bufs) and not var.any() and not out8.any()
