"""CPU tests of the denoiser's definition (tests/denoise_ref.py, the numpy float32 reference the GPU filter must match
bit for bit) and of the host-only part of its C ABI (include/prt.h prt_render_aov / prt_denoise*)."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import prt
from prt import _lib

F = np.float32


@pytest.mark.parametrize("name", list(dr.CASES))
def test_reference_filter_halves_the_error(oracle_mod, name):
    """The oracle's 2-spp frame filtered at the defaults, guided by the oracle's first-hit base colour, shading
    normal and depth, against its 1024-spp frame: at most half the unfiltered RMSE (the filter gives 0.31-0.33 of
    it here, so a no-op fails and a regression of the definition shows)."""
    c = dr.case(name)
    out = dr.denoise(c["noisy"], c["albedo"], c["nd"], c["W"], c["H"], **dr.DEFAULTS)
    before, after = dr.rmse(c["noisy"], c["converged"]), dr.rmse(out, c["converged"])
    print(f"{name}: rmse {before:.4f} -> {after:.4f} (ratio {after / before:.3f})")
    assert after <= 0.5 * before, (before, after)
    assert np.array_equal(out[:, 3], c["noisy"][:, 3])  # w copied from the input


def _random_guides(W, H, seed):
    rng = np.random.default_rng(seed)
    n = W * H
    alb = np.concatenate([rng.uniform(0, 1, (n, 3)), np.ones((n, 1))], axis=1).astype(F)
    nd = np.concatenate([rng.normal(0, 1, (n, 3)), rng.uniform(1, 20, (n, 1))], axis=1).astype(F)
    miss = rng.uniform(0, 1, n) < 0.2
    alb[miss] = 0
    nd[miss] = (0, 0, 0, 1e30)
    return alb, nd, miss


@pytest.mark.parametrize("seed", [3, 11])
def test_constant_image_stays_constant(seed):
    """Any guides, a constant colour: every output is a weighted mean of equal values.

    Channels that are powers of two stay within 2 ulp (in fact exact): every product w * v is exact, so acc goes
    through the same roundings as wsum scaled by v and acc / wsum == v.  This is the normalisation check: a tap
    counted in one sum and not the other, or a missing division, breaks it.

    A general constant does NOT stay within 2 ulp under the definition itself: the 25 products round, and this
    reference deviates by up to 6 ulp after one iteration and 11 ulp after five (0.3, 0.9, 1.7 over these guides).
    What rounding analysis guarantees is asserted instead: with non-negative weights one iteration adds a relative
    error of at most (25 + 24 + 1) u, u = 2^-24 (a product and up to 24 additions per term of acc, 24 additions per
    term of wsum, one division), so `iterations` of them stay below 51 * iterations * u."""
    W, H = 37, 23
    alb, nd, _ = _random_guides(W, H, seed)
    v = np.array([1.0, 0.5, 2.0, 0.5], F)
    col = np.tile(v, (W * H, 1))
    out = dr.denoise(col, alb, nd, W, H, **dr.DEFAULTS)
    assert np.all(np.abs(out[:, :3] - v[:3]) <= 2 * np.spacing(v[:3]))
    assert np.array_equal(out[:, 3], col[:, 3])
    v = np.array([0.3, 0.9, 1.7, 0.0], F)
    col = np.tile(v, (W * H, 1))
    out = dr.denoise(col, alb, nd, W, H, **dr.DEFAULTS)
    dev = np.abs(out[:, :3].astype(np.float64) - v[:3].astype(np.float64))
    print("general constant: max deviation in ulp", (dev / np.spacing(v[:3])).max(axis=0))
    assert np.all(dev <= 51 * dr.DEFAULTS["iterations"] * 2.0 ** -24 * v[:3].astype(np.float64))


def test_miss_pixels_pass_through():
    W, H = 37, 23
    alb, nd, miss = _random_guides(W, H, 4)
    col = np.random.default_rng(5).uniform(0, 2, (W * H, 4)).astype(F)
    out = dr.denoise(col, alb, nd, W, H, **dr.DEFAULTS)
    assert miss.any() and np.array_equal(out[miss], col[miss])
    assert not np.array_equal(out[~miss, :3], col[~miss, :3])


def test_small_image_is_finite():
    """9 x 7: from step 4 on most taps fall outside the image; the centre tap keeps wsum >= 9/64."""
    W, H = 9, 7
    alb, nd, _ = _random_guides(W, H, 6)
    col = np.random.default_rng(7).uniform(0, 2, (W * H, 4)).astype(F)
    out = dr.denoise(col, alb, nd, W, H, iterations=8)
    assert np.all(np.isfinite(out))


def test_pack_rgb8_matches_oracle(oracle_mod):
    x = np.array([[-1, 0, 0.5, 0], [1, 2, 0.999, 0], [0.00390625, 0.2, 1e-9, 0]], F)
    assert [int(v) for v in dr.pack_rgb8(x)] == [oracle_mod.pack_rgb8(r) for r in x]


def test_denoise_abi_without_a_device():
    """prt_denoise_defaults returns the documented defaults; NULL contexts and out-of-range parameters are refused
    with PRT_ERR_INVALID_ARGUMENT before any device is touched."""
    L = prt.load()
    dp = _lib.DenoiseParams()
    assert L.prt_denoise_defaults(C.byref(dp)) == 0
    assert (dp.iterations, dp.normal_power) == (5, 3)
    assert (dp.sigma_color, dp.sigma_depth, dp.sigma_albedo) == (4.0, float(F(0.1)), 0.25)
    assert L.prt_denoise_defaults(None) == -1
    assert {k: getattr(prt.denoise_defaults(), k) for k in ("iterations", "normal_power", "sigma_color")} == \
        dict(iterations=5, normal_power=3, sigma_color=4.0)
    assert prt.denoise_defaults(iterations=2, sigma_albedo=0).iterations == 2
    buf = np.zeros((16, 4), F)
    p = buf.ctypes.data
    assert L.prt_render_aov(None, 4, 4, 0, p, p, 0) == -1
    assert L.prt_denoise(None, C.byref(dp), 4, 4, p, p, p, p, None, 0) == -1
    assert L.prt_denoise_timings(None, None, 1) == -1
    # parameter and argument checks come before the context is used: a fake non-NULL handle is never dereferenced
    fake = C.c_void_p(buf.ctypes.data)
    bad = [dict(iterations=0), dict(iterations=9), dict(normal_power=-1), dict(normal_power=8),
           dict(sigma_color=-1.0), dict(sigma_color=0.0), dict(sigma_depth=float("nan")), dict(sigma_depth=0.0),
           dict(sigma_albedo=-0.5), dict(sigma_albedo=float("inf"))]
    for kw in bad:
        q = prt.denoise_defaults(**kw)
        assert L.prt_denoise(fake, C.byref(q), 4, 4, p, p, p, p, None, 0) == -1, kw
    assert L.prt_denoise(fake, C.byref(dp), 0, 4, p, p, p, p, None, 0) == -1   # non-positive size
    assert L.prt_denoise(fake, C.byref(dp), 4, 4, p, p, p, None, None, 0) == -1  # no output at all
    assert L.prt_denoise(fake, None, 4, 4, p, p, p, p, None, 0) == -1
    assert L.prt_render_aov(fake, 4, -1, 0, p, p, 0) == -1
