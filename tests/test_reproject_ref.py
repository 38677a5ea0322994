"""CPU tests of the temporal reprojection's definition (tests/reproject_ref.py, the numpy float32 reference the GPU pass
must match bit for bit) on the oracle's frames, and of the host-only part of its C ABI (include/prt.h prt_reproject*)."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import reproject_ref as rr
import prt
from prt import _lib

F = np.float32
NAMES = list(dr.CASES)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _fresh(color):
    out = np.array(color, F)
    out[:, 3] = 1
    return out


def _history(W, H, seed=1, length=3.0):
    h = np.random.default_rng(seed).uniform(0, 2, (W * H, 4)).astype(F)
    h[:, 3] = length
    return h


def test_no_history_starts_one(oracle_mod):
    _, W, H = dr.scene_of("multi_96x72")
    v = rr.view("multi_96x72", "slow", 0, frame=True)
    out = rr.reproject(v["color"], v["nd"], v["cam"], W, H)
    assert np.array_equal(_bits(out), _bits(_fresh(v["color"])))


def test_behind_the_previous_camera_starts_over(oracle_mod):
    """The previous camera looks away from the scene: s < 0 for every point, so no pixel enters the gather."""
    _, W, H = dr.scene_of("multi_96x72")
    prev, cur = rr.view("multi_96x72", "behind", 0), rr.view("multi_96x72", "behind", 1)
    col = rr.view("multi_96x72", "slow", 0, frame=True)["color"]
    info = {}
    out = rr.reproject(col, cur["nd"], cur["cam"], W, H, _history(W, H), prev["nd"], prev["cam"], info=info)
    assert info["hit"].any() and not info["valid"].any()
    assert np.array_equal(_bits(out), _bits(_fresh(col)))


def test_history_of_length_zero_is_no_history(oracle_mod):
    """A raw avg_rgba (w = 0) as history: every tap is rejected by Hq.w >= 1."""
    _, W, H = dr.scene_of("multi_96x72")
    a, b = rr.view("multi_96x72", "slow", 0, frame=True), rr.view("multi_96x72", "slow", 1, frame=True)
    assert not a["color"][:, 3].any()
    info = {}
    out = rr.reproject(b["color"], b["nd"], b["cam"], W, H, a["color"], a["nd"], a["cam"], info=info)
    assert info["valid"].any() and not info["has_history"].any()
    assert np.array_equal(_bits(out), _bits(_fresh(b["color"])))


@pytest.mark.parametrize("name", NAMES)
def test_resting_camera(oracle_mod, name):
    """prev_camera == camera: every hit pixel finds history, the reprojected position is the pixel itself up to
    rounding, and a constant history of a power of two with this frame's colour equal to it comes back exactly (the
    bilinear weights need not be (1, 0, 0, 0): every product and sum is exact then)."""
    _, W, H = dr.scene_of(name)
    v = rr.view(name, "rest", 0)
    hist = np.tile(np.array([0.5, 2.0, 0.25, 4.0], F), (W * H, 1))
    col = np.tile(np.array([0.5, 2.0, 0.25, 0.0], F), (W * H, 1))
    info = {}
    out = rr.reproject(col, v["nd"], v["cam"], W, H, hist, v["nd"], rr.view(name, "rest", 1)["cam"], info=info)
    hit = info["hit"]
    assert 0 < hit.sum() < hit.size and np.array_equal(info["has_history"], hit)
    ys, xs = np.divmod(np.arange(W * H), W)
    ex, ey = np.abs(info["px"][hit] - xs[hit]).max(), np.abs(info["py"][hit] - ys[hit]).max()
    print(f"{name}: max |px - x| {ex:.2e}, |py - y| {ey:.2e}")
    assert ex < 1e-3 and ey < 1e-3
    assert np.array_equal(_bits(out[hit, :3]), _bits(hist[hit, :3]))
    assert np.all(out[hit, 3] == 5) and np.all(out[~hit, 3] == 1)
    assert np.all(np.isfinite(out))


COVERAGE = [("multi_96x72", "slow", 0.9, 1), ("small_70x45", "slow", 0.9, 1), ("multi_96x72", "fast", 0.9, 100)]


@pytest.mark.parametrize("name,seq,share_min,lost_min", COVERAGE)
def test_coverage(oracle_mod, name, seq, share_min, lost_min):
    """Geometry alone: at every step of the sequence most hit pixels find history and some do not, so the bitwise
    tests of the device pass cover both the blend and the disocclusion branch; no NaN or inf comes out."""
    _, W, H = dr.scene_of(name)
    steps = len(rr.positions(dr.scene_of(name)[0], seq))
    col, hist = _history(W, H, 2), _history(W, H, 3)
    for k in range(1, steps):
        a, b = rr.view(name, seq, k - 1), rr.view(name, seq, k)
        info = {}
        out = rr.reproject(col, b["nd"], b["cam"], W, H, hist, a["nd"], a["cam"], info=info)
        hit, has = info["hit"], info["has_history"]
        share, lost = has.sum() / hit.sum(), int((hit & ~has).sum())
        print(f"{name} {seq} step {k}: {share:.3f} of {hit.sum()} hit pixels have history, {lost} have none")
        assert info["valid"].any() and np.all(np.isfinite(out))
        assert share >= share_min and lost >= lost_min
        assert not has[~hit].any()


@pytest.mark.parametrize("name", NAMES)
def test_quality(oracle_mod, name):
    """`slow`, 8 frames of 2 spp at depth 4, frame_index = k, against the oracle's 1024-spp frame of the last view.
    The reprojected image's RMSE is at most 0.45 of the last single frame's (measured 0.302 and 0.327: DESIGN.md), and
    denoising the reprojected image beats denoising the last frame alone."""
    _, W, H = dr.scene_of(name)
    vs = [rr.view(name, "slow", k, frame=True) for k in range(rr.SLOW_FRAMES)]
    outs = rr.chain([v["color"] for v in vs], [v["nd"] for v in vs], [v["cam"] for v in vs], W, H)
    assert np.all(np.isfinite(outs[-1]))
    assert abs(outs[-1][:, 3].max() - rr.SLOW_FRAMES) < 1e-4  # a length is a weighted mean: whole up to rounding
    alb = rr.oracle_albedo(name, "slow", rr.SLOW_FRAMES - 1)
    single, repro, den_r, den_f = rr.quality(name, vs[-1]["color"], outs[-1], alb, vs[-1]["nd"])
    print(f"{name}: rmse last frame {single:.4f}, reprojected {repro:.4f} (ratio {repro / single:.3f}); "
          f"denoised: reprojected {den_r:.4f}, last frame {den_f:.4f}")
    assert repro <= 0.45 * single, (single, repro)
    assert den_r < den_f, (den_r, den_f)


def test_reproject_abi_without_a_device():
    """prt_reproject_defaults returns the documented defaults; every refusal comes with PRT_ERR_INVALID_ARGUMENT before
    the context is used (a fake non-NULL handle is never dereferenced) and leaves the output untouched."""
    L = prt.load()
    rp = _lib.ReprojectParams()
    assert L.prt_reproject_defaults(C.byref(rp)) == 0
    assert (rp.depth_tol, rp.normal_min, rp.max_history) == (float(F(0.05)), float(F(0.9)), 16.0)
    assert L.prt_reproject_defaults(None) == -1
    assert prt.reproject_defaults(max_history=4).max_history == 4
    with pytest.raises(TypeError):
        prt.reproject_defaults(sigma=1)
    bufs = [np.zeros((16, 4), F) for _ in range(5)]
    col, nd, hist, hnd, out = (b.ctypes.data for b in bufs)
    cam = _lib.CameraDesc()
    cp = C.byref(cam)
    fake = C.c_void_p(col)

    def call(ctx=fake, p=rp, W=4, H=4, c=cp, color=col, g=nd, pc=cp, h=hist, hg=hnd, o=out, o8=None):
        return L.prt_reproject(ctx, C.byref(p) if p is not None else None, W, H, c, color, g, pc, h, hg, o, o8, 0)

    assert call(ctx=None) == -1 and call(p=None) == -1 and call(c=None) == -1
    assert call(color=None) == -1 and call(g=None) == -1 and call(o=None) == -1
    assert call(W=0) == -1 and call(H=-3) == -1
    for kw in (dict(depth_tol=-0.1), dict(depth_tol=float("nan")), dict(depth_tol=float("inf")),
               dict(normal_min=1.5), dict(normal_min=-1.5), dict(normal_min=float("nan")),
               dict(max_history=0.5), dict(max_history=float("inf")), dict(max_history=float("nan"))):
        assert call(p=prt.reproject_defaults(**kw)) == -1, kw
    # prev_camera, history and its normal_depth go together
    for kw in (dict(pc=None), dict(h=None), dict(hg=None), dict(pc=None, h=None), dict(pc=None, hg=None),
               dict(h=None, hg=None)):
        assert call(**kw) == -1, kw
    assert call(o=hist) == -1 and call(o=hnd) == -1  # taps are gathered: no output into a history buffer
    assert not bufs[4].any() and not bufs[2].any() and not bufs[3].any()
