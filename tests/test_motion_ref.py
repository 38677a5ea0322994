"""CPU tests of the motion-aware temporal reprojection's definition (tests/motion_ref.py, the numpy float32 reference
the GPU pass must match bit for bit) on the oracle's frames of a scene whose instance 1 moves, and of the host-only part
of its C ABI (include/prt.h prt_instance_motion, prt_reproject_motion's refusals)."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import motion_ref as mr
import reproject_ref as rr
import prt
from prt import _lib, scenes

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _views(mseq, cseq):
    return [mr.view(mseq, cseq, k) for k in range(mr.FRAMES)]


@pytest.mark.parametrize("name", list(dr.CASES))
def test_identity_equals_plain_pass(oracle_mod, name):
    """Identity matrices and no history_instance: every added product and sum is exact, so the output is
    rr.reproject's bit for bit (`slow` step 1, where both the blend and the start-over branch occur)."""
    _, W, H = dr.scene_of(name)
    a, b = rr.view(name, "slow", 0, frame=True), rr.view(name, "slow", 1, frame=True)
    ids = mr.oracle_ids(name, "slow", 1)
    count = int(ids[ids != mr.MISS].max()) + 1
    hist = rr.reproject(a["color"], a["nd"], a["cam"], W, H)
    info, minfo = {}, {}
    want = rr.reproject(b["color"], b["nd"], b["cam"], W, H, hist, a["nd"], a["cam"], info=info)
    got = mr.reproject_motion(b["color"], b["nd"], ids, b["cam"], W, H, hist, a["nd"], a["cam"], None,
                              mr.identity(count), info=minfo)
    assert info["has_history"].any() and (info["hit"] & ~info["has_history"]).any()
    assert np.array_equal(info["has_history"], minfo["has_history"])
    assert np.array_equal(_bits(got), _bits(want))


def test_static_instances_are_untouched(oracle_mod):
    """B/rest: at each of the 7 steps both passes get the same history (the motion chain's) and the same step inputs;
    every pixel whose instance has the identity matrix comes out bit-equal (no history_instance: the id test is the
    one thing that could tell a static pixel's taps apart).  The mover's pixels do differ."""
    _, W, H = dr.scene_of(mr.SCENE)
    vs = _views("B", "rest")
    hist = mr.step(vs, 0, None)
    for k in range(1, mr.FRAMES):
        mo = mr.motion_f32(vs[k]["xf"], vs[k - 1]["xf"])
        static_inst = np.flatnonzero(np.all(mo == mr.IDENTITY, axis=1))
        assert list(static_inst) == [0, 2]
        plain = mr.step(vs, k, hist, plain=True)
        moved = mr.step(vs, k, hist, with_ids=False)
        static = np.isin(vs[k]["ids"], static_inst) | (vs[k]["ids"] == mr.MISS)
        assert static.any() and (~static).any()
        assert np.array_equal(_bits(plain[static]), _bits(moved[static])), k
        assert not np.array_equal(_bits(plain[~static]), _bits(moved[~static])), k
        hist = mr.step(vs, k, hist)


def _ulp_row_bound(ref64):
    """One float32 ulp of each row's largest magnitude, per element: [count, 3, 1]."""
    big = np.abs(ref64).max(axis=2, keepdims=True).astype(F)
    return np.spacing(big).astype(np.float64)


def test_instance_motion_matches_reference():
    """prt_instance_motion (host only: the library loads without a GPU) against motion_ref.motion_matrices: both
    round a double result whose own error is about 1e-13, so they differ at most at a rounding boundary -- one
    float32 ulp of the row's largest magnitude.  cur: the three instances of multi_instance and the first 16 of
    instance_field(70); prev: perturbed copies."""
    rng = np.random.default_rng(7)
    cur = np.stack([np.asarray(T, F).reshape(4, 4) for _, T in
                    scenes.multi_instance(scenes.config_small(40, 30)).instances
                    + scenes.instance_field(70).instances[:16]])
    assert len(cur) == 19
    prev = cur.copy()
    for k in range(len(cur)):
        a, t = rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5, 3)
        R, Tm = np.eye(4), np.eye(4)
        R[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        Tm[:3, 3] = t
        prev[k] = (Tm @ cur[k].astype(np.float64) @ R).astype(F)
    prev[5] = cur[5]  # one at rest
    got = prt.instance_motion(cur, prev).reshape(-1, 3, 4)
    ref = mr.motion_matrices(cur, prev)
    assert np.array_equal(got[5].ravel(), mr.IDENTITY)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"max |C - numpy| in ulps of the row's largest: {(err / _ulp_row_bound(ref)).max():.3f}")
    assert np.all(err <= _ulp_row_bound(ref))
    assert not np.array_equal(got[0].ravel(), mr.IDENTITY)
    # A maps a point of the current frame to where it was: A * cur == prev on the instance's own points
    for k in (0, 1, 7):
        A = np.vstack([got[k].astype(np.float64), [0, 0, 0, 1]])
        assert np.allclose(A @ cur[k].astype(np.float64), prev[k].astype(np.float64), atol=1e-5)
    # bytewise-equal inputs: the exact identity; a singular or non-finite current transform: the identity too
    same = prt.instance_motion(cur, cur)
    assert np.array_equal(same, mr.identity(len(cur)))
    bad = cur.copy()
    bad[1, :3, :3] = 0
    bad[2, 0, 0] = np.nan
    bad[3, :3, :3] = np.array([[1, 2, 3], [2, 4, 6], [0, 1, 0]], F)  # two dependent rows: determinant 0
    got = prt.instance_motion(bad, prev).reshape(-1, 3, 4)
    for k in (1, 2, 3):
        assert np.array_equal(got[k].ravel(), mr.IDENTITY), k
    ref = mr.motion_matrices(bad, prev)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= _ulp_row_bound(ref))
    L = prt.load()
    out = np.full(12, 7, F)
    assert L.prt_instance_motion(None, None, 0, None) == 0
    assert L.prt_instance_motion(None, prev.ctypes.data, 1, out.ctypes.data) == -1
    assert L.prt_instance_motion(cur.ctypes.data, None, 1, out.ctypes.data) == -1
    assert L.prt_instance_motion(cur.ctypes.data, prev.ctypes.data, 1, None) == -1
    assert L.prt_instance_motion(cur.ctypes.data, prev.ctypes.data, -1, out.ctypes.data) == -1
    assert np.all(out == 7)
    with pytest.raises(ValueError):
        prt.instance_motion(cur, prev[:3])


@pytest.mark.parametrize("cseq", ["rest", "slow"])
def test_quality_and_coverage(oracle_mod, cseq):
    """Sequence B, 8 frames of 2 spp at depth 4, each pass chained on its own output, over the mover's pixels of the
    last frame against the oracle's 1024-spp frame: the fraction with history rises by >= 0.15 and the RMSE falls to
    <= 0.85 of the plain pass's; over the static hit pixels the RMSE is the same within 1e-6.  Measured with this
    reference (DESIGN.md "Moving instances"): B/rest fraction 0.321 -> 0.739, RMSE 0.2881 -> 0.1995; B/slow fraction
    0.522 -> 0.726, RMSE 0.2582 -> 0.1921."""
    vs = _views("B", cseq)
    plain, moved = mr.chain(vs, plain=True)[-1], mr.chain(vs)[-1]
    assert np.all(np.isfinite(moved))
    f = mr.figures(vs, plain, moved, mr.converged_last("B", cseq))
    print(f"B/{cseq}: " + ", ".join(f"{k} {v:.4f}" for k, v in f.items()))
    mr.check_quality(f)


def test_frozen_mover(oracle_mod):
    """t = 0, a = 0, resting camera: every hit pixel has history after 8 steps, of length 8 up to rounding."""
    vs = _views("frozen", "rest")
    assert np.array_equal(mr.motion_f32(vs[1]["xf"], vs[0]["xf"]), mr.identity(3))
    out = mr.chain(vs)[-1]
    hit = vs[-1]["ids"] != mr.MISS
    assert 0 < hit.sum() < hit.size
    print(f"frozen: fraction with history {mr.has_history(out)[hit].mean():.3f}, mean length {out[hit, 3].mean():.3f}")
    assert mr.has_history(out)[hit].all()
    assert np.all(np.abs(out[hit, 3] - mr.FRAMES) < 1e-4)
    assert np.all(out[~hit, 3] == 1)


def test_instance_ids_out_of_range(oracle_mod):
    """count below the largest id: the pixels of the instances without a matrix start over, the others are as with
    all the matrices."""
    _, W, H = dr.scene_of(mr.SCENE)
    vs = _views("B", "rest")
    v, u = vs[1], vs[0]
    hist = mr.step(vs, 0, None)
    mo = mr.motion_f32(v["xf"], u["xf"])
    full = mr.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist, u["nd"], u["cam"], u["ids"], mo)
    for count in (1, 2):
        info = {}
        cut = mr.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], W, H, hist, u["nd"], u["cam"], u["ids"],
                                  mo[:count], info=info)
        beyond = (v["ids"] != mr.MISS) & (v["ids"] >= count)
        assert beyond.any() and not info["known"][beyond].any() and not info["has_history"][beyond].any()
        fresh = np.array(v["color"])
        fresh[:, 3] = 1
        assert np.array_equal(_bits(cut[beyond]), _bits(fresh[beyond]))
        assert np.array_equal(_bits(cut[~beyond]), _bits(full[~beyond]))
        assert mr.has_history(full)[beyond].any()


def test_reproject_motion_abi_without_a_device():
    """Every refusal of prt_reproject_motion comes with PRT_ERR_INVALID_ARGUMENT before the context is used (a fake
    non-NULL handle is never dereferenced) and leaves the outputs untouched."""
    L = prt.load()
    rp = prt.reproject_defaults()
    bufs = [np.zeros((16, 4), F) for _ in range(5)]
    col, nd, hist, hnd, out = (b.ctypes.data for b in bufs)
    idb = [np.zeros(16, np.uint32) for _ in range(3)]
    ids, hids, out8 = (b.ctypes.data for b in idb)
    mo = mr.identity(2)
    cam = _lib.CameraDesc()
    cp = C.byref(cam)
    fake = C.c_void_p(col)

    def call(ctx=fake, p=rp, W=4, H=4, c=cp, color=col, g=nd, i=ids, pc=cp, h=hist, hg=hnd, hi=hids,
             m=mo.ctypes.data, n=2, o=out, o8=out8):
        return L.prt_reproject_motion(ctx, C.byref(p) if p is not None else None, W, H, c, color, g, i, pc, h, hg, hi,
                                      m, n, o, o8, 0)

    assert call(ctx=None) == -1 and call(p=None) == -1 and call(c=None) == -1
    assert call(color=None) == -1 and call(g=None) == -1 and call(o=None, o8=None) == -1
    assert call(W=0) == -1 and call(H=-3) == -1
    for kw in (dict(depth_tol=-0.1), dict(depth_tol=float("nan")), dict(normal_min=1.5), dict(max_history=0.5),
               dict(max_history=float("nan"))):
        assert call(p=prt.reproject_defaults(**kw)) == -1, kw
    # prev_camera, history, its normal_depth, motion and count > 0 go together; history_instance needs them
    for kw in (dict(pc=None), dict(h=None), dict(hg=None), dict(m=None), dict(n=0), dict(n=-1),
               dict(pc=None, h=None, hg=None, m=None), dict(pc=None, h=None, hg=None, n=0),
               dict(pc=None, h=None, hg=None, m=None, n=0), dict(pc=None, h=None, hg=None, hi=None, m=None, n=-2)):
        assert call(**kw) == -1, kw
    assert call(i=None) == -1  # the ids are required with a history
    assert call(o=hist) == -1 and call(o=hnd) == -1 and call(o8=hids) == -1  # taps are gathered
    assert not bufs[4].any() and not bufs[2].any() and not bufs[3].any() and not any(b.any() for b in idb)
