"""Luminance moments and the variance-guided filter on the device (include/prt.h prt_reproject_moments,
prt_denoise_variance; csrc/prt_variance.hip) against the numpy float32 reference (tests/variance_ref.py) bit for bit on
the GPU's own frames, AOVs and instance ids: single steps and an 8-step chain with and without the clamp and the spatial
branch, the identities against prt_reproject_motion, prt_reproject and prt_denoise, the filter's iterations, decay,
outputs and aliasing, the pointer variants, frames in flight, a shard group, no side effect, the timing slots,
Renderer.TickTemporalVariance and the error against a converged render.

Scenes: multi_instance(config_small(40, 30)) at 96 x 72 and 9 x 7 (smaller than one block; the filter's taps leave the
image from step 4 on), config_small(40, 30) at 70 x 45 (no multiple of the 32 x 8 pixel block), instance_field(70) at
64 x 48 (its ids come through the instance BVH)."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import motion_ref as mr
import reproject_ref as rr
import variance_ref as vr
from helpers import gpu_scene

pytestmark = pytest.mark.gpu

F = np.float32
_views, _loaded, _chains = {}, {}, {}
W0, H0 = dr.CASES[mr.SCENE][1:]
# the shapes: name -> (scene, W, H, instance sequence or None, camera sequence)
SHAPES = {"multi_96x72": (mr.SCENE, W0, H0, "B", "slow"), "multi_9x7": (mr.SCENE, 9, 7, "B", "slow"),
          "small_70x45": ("small_70x45", 70, 45, None, "slow"), "field_64x48": ("field", 64, 48, None, "slow"),
          "multi_rest": (mr.SCENE, W0, H0, "B", "rest"), "multi_A_rest": (mr.SCENE, W0, H0, "A", "rest"),
          "multi_static": (mr.SCENE, W0, H0, "frozen", "slow")}


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import prt
    c = prt.Context(0)
    yield c
    _views.clear()
    _loaded.clear()
    _chains.clear()
    c.close()


def _scene_data(scene):
    from prt import scenes
    return scenes.instance_field(70) if scene == "field" else dr.scene_of(scene)[0]


def _blases(scene, xf):
    return [(mi, xf[i]) for i, (mi, _) in enumerate(scene.blases)]


def _load(ctx, shape):
    """The shape's scene in the module's context (loaded again only when another one was there)."""
    name, W, H, _, _ = SHAPES[shape]
    if _loaded.get("key") != (name, W, H):
        _loaded["scene"] = gpu_scene(ctx, _scene_data(name), W, H)[0]
        _loaded["key"] = (name, W, H)
    return _loaded["scene"]


def _view(ctx, shape, k):
    """The GPU's own 2-spp frame (default flags, depth 4, frame_index k), AOVs and instance ids of frame k of a shape's
    sequence, made once."""
    import prt
    key = (shape, k)
    if key not in _views:
        name, W, H, mseq, cseq = SHAPES[shape]
        sd = _scene_data(name)
        scene = _load(ctx, shape)
        if mseq is not None:
            xf = mr.transforms(mseq, k)
            pos, tgt = mr.camera_positions(cseq)[k]
        else:
            xf = np.stack([np.asarray(T, F).reshape(4, 4) for _, T in scene.blases])
            pos, tgt = rr.positions(sd, cseq)[k]
        cam = prt.Camera(pos, tgt, F(W) / F(H))
        ctx.set_instances(_blases(scene, xf))
        ctx.set_camera(cam)
        ctx.reset_accumulation(full=True)
        avg, _, _ = ctx.render(W, H, 2, 4, frame_index=k)
        alb, nd, ids = ctx.render_aov_ids(W, H)
        ctx.reset_accumulation(full=True)
        for a in (avg, alb, nd, ids, xf):
            a.setflags(write=False)
        _views[key] = dict(cam=cam, color=avg, alb=alb, nd=nd, ids=ids, xf=xf, W=W, H=H)
    return _views[key]


def _ref_step(v, u, hist, info=None, **par):
    import prt
    if u is None:
        return vr.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], v["W"], v["H"], info=info, **par)
    return vr.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], v["W"], v["H"], hist[0], u["nd"], u["cam"],
                                u["ids"], prt.instance_motion(v["xf"], u["xf"]), hist[1], info=info, **par)


def _dev_step(ctx, v, u, hist, **par):
    import prt
    tp = prt.temporal_defaults(**par)
    if u is None:
        return ctx.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], width=v["W"], height=v["H"], params=tp)
    return ctx.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"], u["ids"],
                                 prt.instance_motion(v["xf"], u["xf"]), hist[1], width=v["W"], height=v["H"],
                                 params=tp)


def _ref_chain(ctx, shape, upto, **par):
    """The reference's (out, moments) of steps 0..upto over the GPU's frames."""
    outs = _chains.setdefault((shape, tuple(sorted(par.items()))), [])
    while len(outs) <= upto:
        k = len(outs)
        outs.append(_ref_step(_view(ctx, shape, k), _view(ctx, shape, k - 1) if k else None, outs[-1] if k else None,
                              **par))
    return outs


def _assert_equal(v, got, ref, what):
    out, mom, rgb8 = got
    for name, a, b in (("colour", out, ref[0]), ("moments", mom, ref[1])):
        bad = np.flatnonzero(np.any(_bits(a) != _bits(b), axis=1))
        if bad.size:
            lines = [f"pixel {p} (x {p % v['W']}, y {p // v['W']}): gpu {a[p]} ref {b[p]} color {v['color'][p]} "
                     f"normal_depth {v['nd'][p]} id {v['ids'][p]}" for p in bad[:4]]
            raise AssertionError(f"{what}: {name}: {bad.size} of {len(a)} pixels differ\n" + "\n".join(lines))
    assert np.array_equal(rgb8, dr.pack_rgb8(ref[0])), what


# ---- prt_reproject_moments
PARAMS = [dict(), dict(clamp_k=1.5), dict(min_temporal=1.0), dict(clamp_k=1.5, min_temporal=1.0)]
_pid = lambda v: "-".join(f"{k}{x}" for k, x in v.items()) or "defaults"


@pytest.mark.parametrize("par", PARAMS[:3:2], ids=_pid)
@pytest.mark.parametrize("shape", ["multi_96x72", "multi_9x7", "small_70x45", "field_64x48"])
def test_fresh_start_bitwise(ctx, shape, par):
    """A history starts: out = (colour, 1), the moments are (L, L * L) and every hit pixel's variance is the spatial
    estimate (min_temporal 4) or 0 (min_temporal 1)."""
    v = _view(ctx, shape, 0)
    info = {}
    ref = _ref_step(v, None, None, info=info, **par)
    assert info["hit"].any()
    assert info["spatial"].any() == (par.get("min_temporal", 4.0) > 1)
    _assert_equal(v, _dev_step(ctx, v, None, None, **par), ref, f"{shape} fresh {par}")
    if shape == "field_64x48":
        assert len(np.unique(v["ids"][info["hit"]])) > 8


@pytest.mark.parametrize("par", PARAMS, ids=_pid)
@pytest.mark.parametrize("shape,k", [("multi_rest", 1), ("multi_rest", 5), ("multi_96x72", 1), ("multi_96x72", 5),
                                     ("multi_9x7", 2), ("small_70x45", 2), ("field_64x48", 2)])
def test_step_matches_reference_bitwise(ctx, shape, k, par):
    """One device step, the history being the reference's output of the step before: colour, history length, the
    moments, the variance and the packed pixels equal the reference's."""
    v, u = _view(ctx, shape, k), _view(ctx, shape, k - 1)
    hist = _ref_chain(ctx, shape, k - 1, **par)[-1]
    info = {}
    ref = _ref_step(v, u, hist, info=info, **par)
    has, hit = info["has_history"], info["hit"]
    print(f"{shape} step {k} {par}: {has.sum()} of {hit.sum()} hit pixels have history, {info['temporal'].sum()} "
          f"temporal, {info['spatial'].sum()} spatial")
    assert has.any()
    if shape == "multi_96x72":
        assert (hit & ~has).any()
        if k == 5 and par.get("min_temporal", 4.0) > 1:
            assert info["temporal"].any() and info["spatial"].any()
    if par.get("min_temporal", 4.0) == 1:
        assert not info["spatial"].any()
    _assert_equal(v, _dev_step(ctx, v, u, hist, **par), ref, f"{shape} step {k} {par}")


@pytest.mark.parametrize("par", PARAMS[:2], ids=_pid)
def test_chain_on_the_device(ctx, par):
    """Eight steps of B/slow with the device's own outputs as the next history equal the reference's chain."""
    ref = _ref_chain(ctx, "multi_96x72", mr.FRAMES - 1, **par)
    got = None
    for k in range(mr.FRAMES):
        v = _view(ctx, "multi_96x72", k)
        got = _dev_step(ctx, v, _view(ctx, "multi_96x72", k - 1) if k else None, got, **par)
    _assert_equal(v, got, ref[-1], f"chain {par}")
    assert got[0][:, 3].max() > mr.FRAMES - 1e-3


@pytest.mark.parametrize("shape", ["multi_96x72", "multi_rest", "multi_9x7"])
def test_colour_equals_prt_reproject_motion(ctx, shape):
    """clamp_k = 0: out_rgba and out_rgb8 are prt_reproject_motion's bit for bit (step 3, and a fresh start)."""
    import prt
    v, u = _view(ctx, shape, 3), _view(ctx, shape, 2)
    hist = _ref_chain(ctx, shape, 2)[-1]
    mo = prt.instance_motion(v["xf"], u["xf"])
    want, want8 = ctx.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"], u["ids"],
                                       mo, width=v["W"], height=v["H"])
    out, _, rgb8 = _dev_step(ctx, v, u, hist)
    assert np.any(want[:, 3] > 1) and np.array_equal(_bits(out), _bits(want)) and np.array_equal(rgb8, want8)
    want, want8 = ctx.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], width=v["W"], height=v["H"])
    out, _, rgb8 = _dev_step(ctx, v, None, None)
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(rgb8, want8)


@pytest.mark.parametrize("shape", ["small_70x45", "field_64x48"])
def test_identity_equals_prt_reproject(ctx, shape):
    """Identity matrices, no history ids, clamp_k = 0: the colour is prt_reproject's bit for bit (`slow` step 1)."""
    v, u = _view(ctx, shape, 1), _view(ctx, shape, 0)
    W, H = v["W"], v["H"]
    hist = _ref_chain(ctx, shape, 0)[-1]
    want, want8 = ctx.reproject(v["color"], v["nd"], v["cam"], hist[0], u["nd"], u["cam"], width=W, height=H)
    out, _, rgb8 = ctx.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"], None,
                                         mr.identity(len(v["xf"])), hist[1], width=W, height=H)
    assert np.any(want[:, 3] > 1) and np.array_equal(_bits(out), _bits(want)) and np.array_equal(rgb8, want8)


# ---- prt_denoise_variance
def _filter_input(ctx, shape):
    """(view, out, moments) of step 3 of the shape's reference chain: blended and disoccluded pixels, both variances."""
    return (_view(ctx, shape, 3),) + tuple(_ref_chain(ctx, shape, 3)[-1])


def _check_filter(ctx, shape, **par):
    import prt
    v, out, mom = _filter_input(ctx, shape)
    W, H = v["W"], v["H"]
    alb = v["alb"] if par.get("sigma_albedo", 0.25) > 0 else None
    want, wantv = vr.denoise_variance(out, mom, alb, v["nd"], W, H, **dict(vr.FILTER_DEFAULTS, **par))
    got, var, rgb8 = ctx.denoise_variance(out, mom, alb, v["nd"], W, H, prt.denoise_variance_defaults(**par))
    bad = np.flatnonzero(np.any(_bits(got) != _bits(want), axis=1) | (_bits(var) != _bits(wantv)))
    if bad.size:
        lines = [f"pixel {p} (x {p % W}, y {p // W}): gpu {got[p]} {var[p]} ref {want[p]} {wantv[p]} in {out[p]} "
                 f"{mom[p]}" for p in bad[:4]]
        raise AssertionError(f"{shape} {par}: {bad.size} of {len(got)} pixels differ\n" + "\n".join(lines))
    assert np.array_equal(rgb8, dr.pack_rgb8(want))
    assert np.array_equal(_bits(got[:, 3]), _bits(out[:, 3]))  # w is the input's
    assert not np.array_equal(_bits(got[:, :3]), _bits(out[:, :3]))
    return got, var, rgb8


@pytest.mark.parametrize("iterations", [1, 3, 5, 8])
@pytest.mark.parametrize("shape", ["multi_96x72", "multi_9x7", "small_70x45", "field_64x48"])
def test_filter_matches_reference_bitwise(ctx, shape, iterations):
    """The filtered colour, the variance output and the packed pixels equal the reference's at 1, 3, 5 and 8 iterations
    (1: no intermediate image; 2 and more: both of them)."""
    _, var, _ = _check_filter(ctx, shape, iterations=iterations)
    assert np.all(var >= 0) and np.any(var > 0)


@pytest.mark.parametrize("par", [dict(color_decay=0.5), dict(sigma_albedo=0.0), dict(sigma_color=0.5, color_decay=2.0),
                                 dict(variance_floor=1e-2), dict(normal_power=0, sigma_depth=1.0)], ids=_pid)
def test_filter_parameter_variants_bitwise(ctx, par):
    """prt_denoise's schedule (color_decay 0.5), a NULL albedo with sigma_albedo 0, a growing sigma, a variance floor
    that binds and the ends of the other parameters, 3 iterations on multi_96x72."""
    _check_filter(ctx, "multi_96x72", iterations=3, **par)


def test_filter_outputs_and_aliasing(ctx):
    """Device pointers on a torch stream: out_variance NULL, out_rgba NULL (rgb8 only), out_rgba == color_rgba at 1
    and 3 iterations; the inputs are left alone otherwise."""
    import torch
    import prt
    v, out, mom = _filter_input(ctx, "multi_96x72")
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    res = {}
    try:
        with torch.cuda.stream(stream):
            col, mo, alb, nd = (torch.from_numpy(np.array(a)).to("cuda") for a in (out, mom, v["alb"], v["nd"]))
        for it in (1, 3):
            dp = prt.denoise_variance_defaults(iterations=it)
            with torch.cuda.stream(stream):
                o, inplace = torch.zeros((n, 4), dtype=torch.float32, device="cuda"), col.clone()
                var, var2 = (torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
                r8, only8 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
            args = (mo.data_ptr(), alb.data_ptr(), nd.data_ptr(), W, H, dp)
            ctx.denoise_variance(col.data_ptr(), *args, device_out=True, out=o.data_ptr(), variance=var.data_ptr(),
                                 rgb8=r8.data_ptr())
            ctx.denoise_variance(inplace.data_ptr(), *args, device_out=True, out=inplace.data_ptr())
            ctx.denoise_variance(col.data_ptr(), *args, device_out=True, rgb8=only8.data_ptr(),
                                 variance=var2.data_ptr())
            res[it] = (o, inplace, var, var2, r8, only8)
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    assert np.array_equal(_bits(col.cpu().numpy()), _bits(out)) and np.array_equal(_bits(mo.cpu().numpy()), _bits(mom))
    for it, (o, inplace, var, var2, r8, only8) in res.items():
        want, wantv = vr.denoise_variance(out, mom, v["alb"], v["nd"], W, H, **dict(vr.FILTER_DEFAULTS, iterations=it))
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), it
        assert np.array_equal(_bits(inplace.cpu().numpy()), _bits(want)), it
        assert np.array_equal(_bits(var.cpu().numpy()), _bits(wantv)), it
        assert np.array_equal(_bits(var2.cpu().numpy()), _bits(wantv)), it
        assert np.array_equal(r8.cpu().numpy().view(np.uint32), dr.pack_rgb8(want)), it
        assert np.array_equal(only8.cpu().numpy().view(np.uint32), dr.pack_rgb8(want)), it
    # host pointers, out_variance NULL
    got, var, rgb8 = ctx.denoise_variance(out, mom, v["alb"], v["nd"], W, H, want_variance=False)
    want, _ = vr.denoise_variance(out, mom, v["alb"], v["nd"], W, H)
    assert var is None and np.array_equal(_bits(got), _bits(want)) and np.array_equal(rgb8, dr.pack_rgb8(want))


@pytest.mark.parametrize("shape", ["multi_96x72", "small_70x45", "multi_9x7"])
def test_ones_variance_equals_prt_denoise(ctx, shape):
    """The variance 1 everywhere, variance_floor 1, color_decay 0.5, one iteration: the colour is prt_denoise's bit for
    bit."""
    import prt
    v, out, mom = _filter_input(ctx, shape)
    W, H = v["W"], v["H"]
    ones = np.zeros_like(mom)
    ones[:, 2] = 1
    want, want8 = ctx.denoise(out, v["alb"], v["nd"], W, H, prt.denoise_defaults(iterations=1))
    got, var, rgb8 = ctx.denoise_variance(out, ones, v["alb"], v["nd"], W, H, prt.denoise_variance_defaults(
        iterations=1, sigma_color=4.0, color_decay=0.5, variance_floor=1.0))
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(rgb8, want8)
    assert not np.array_equal(_bits(got[:, :3]), _bits(out[:, :3])) and np.all(var <= 1)


def test_timings_are_recorded(ctx):
    """timed=True fills prt_denoise_timings' slots: ms[1] the prep, ms[2 + i] iteration i; the others read 0."""
    import prt
    v, out, mom = _filter_input(ctx, "small_70x45")
    ctx.denoise_variance(out, mom, v["alb"], v["nd"], v["W"], v["H"], prt.denoise_variance_defaults(iterations=3),
                         timed=True)
    ms = ctx.denoise_timings()
    assert len(ms) == 10 and all(m > 0 for m in ms[1:5]) and not any(ms[5:])


# ---- plumbing
def test_no_side_effect(ctx):
    """The two calls between two accumulating renders: the accumulation blob and the ray totals are the same before
    and after, and the second render equals the one made without the calls."""
    import prt
    v, u = _view(ctx, "multi_96x72", 1), _view(ctx, "multi_96x72", 0)
    hist = _ref_chain(ctx, "multi_96x72", 0)[-1]
    W, H = v["W"], v["H"]
    ctx.set_instances(_blases(_load(ctx, "multi_96x72"), v["xf"]))
    ctx.set_camera(v["cam"])
    try:
        ctx.reset_accumulation(full=True)
        ctx.render(W, H, 2, 4, frame_index=0)
        want, want8, _ = ctx.render(W, H, 2, 4, frame_index=1)
        ctx.reset_accumulation(full=True)
        a0, _, _ = ctx.render(W, H, 2, 4, frame_index=0)
        blob, totals = ctx.save_accumulation(), ctx.ray_totals()
        out, mom, _ = ctx.reproject_moments(a0, v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"], u["ids"],
                                            prt.instance_motion(v["xf"], u["xf"]), hist[1], width=W, height=H)
        flt, _, _ = ctx.denoise_variance(out, mom, v["alb"], v["nd"], W, H)
        assert not np.array_equal(out[:, :3], a0[:, :3]) and not np.array_equal(flt[:, :3], out[:, :3])
        assert ctx.save_accumulation() == blob and ctx.ray_totals() == totals
        got, got8, _ = ctx.render(W, H, 2, 4, frame_index=1)
    finally:
        ctx.reset_accumulation(full=True)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got8, want8)


def _dev(stream, *arrays):
    import torch
    with torch.cuda.stream(stream):
        return [torch.from_numpy(np.array(a).view(np.int32) if a.dtype == np.uint32 else np.array(a)).to("cuda")
                for a in arrays]


def test_device_pointers(ctx):
    """prt_reproject_moments with device-pointer images on a torch stream (PRT_OUT_DEVICE, no host wait) gives the
    host path's images; out_rgba or out_rgb8 may be absent, history_instance may be absent, starting a history works
    with device pointers too.  The matrices are a host array changed right after each call: it was copied."""
    import torch
    import prt
    v, u = _view(ctx, "multi_96x72", 3), _view(ctx, "multi_96x72", 2)
    hist = _ref_chain(ctx, "multi_96x72", 2)[-1]
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    mo = prt.instance_motion(v["xf"], u["xf"])
    tp = prt.temporal_defaults(clamp_k=1.5)
    want = ctx.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"], u["ids"], mo,
                                 hist[1], width=W, height=H, params=tp)
    want_noids = ctx.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"], None, mo,
                                       hist[1], width=W, height=H, params=tp)
    want_first = ctx.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], width=W, height=H, params=tp)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        col, nd, ids, h, hnd, hids, hm = _dev(stream, v["color"], v["nd"], v["ids"], hist[0], u["nd"], u["ids"],
                                              hist[1])
        with torch.cuda.stream(stream):
            o = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
            m = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(5)]
            r8 = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
            first = torch.zeros((n, 4), dtype=torch.float32, device="cuda")  # (cleared on the stream that writes it)

        def call(hi=hids.data_ptr(), **kw):
            mm = mo.copy()
            ctx.reproject_moments(col.data_ptr(), nd.data_ptr(), ids.data_ptr(), v["cam"], h.data_ptr(),
                                  hnd.data_ptr(), u["cam"], hi, mm, hm.data_ptr(), width=W, height=H, params=tp,
                                  device_out=True, **kw)
            mm[:] = np.nan  # the call has copied the matrices

        call(out=o[0].data_ptr(), moments=m[0].data_ptr(), rgb8=r8[0].data_ptr())
        call(out=o[1].data_ptr(), moments=m[1].data_ptr())
        call(moments=m[2].data_ptr(), rgb8=r8[1].data_ptr())
        call(hi=None, out=o[2].data_ptr(), moments=m[3].data_ptr())
        ctx.reproject_moments(col.data_ptr(), nd.data_ptr(), ids.data_ptr(), v["cam"], width=W, height=H, params=tp,
                              device_out=True, out=first.data_ptr(), moments=m[4].data_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    assert np.array_equal(_bits(col.cpu().numpy()), _bits(v["color"]))  # the inputs are left alone
    assert np.array_equal(_bits(hm.cpu().numpy()), _bits(hist[1]))
    for k in (0, 1):
        assert np.array_equal(_bits(o[k].cpu().numpy()), _bits(want[0]))
        assert np.array_equal(r8[k].cpu().numpy().view(np.uint32), want[2])
    for k in (0, 1, 2):
        assert np.array_equal(_bits(m[k].cpu().numpy()), _bits(want[1]))
    assert np.array_equal(_bits(o[2].cpu().numpy()), _bits(want_noids[0]))
    assert np.array_equal(_bits(m[3].cpu().numpy()), _bits(want_noids[1]))
    assert np.array_equal(_bits(first.cpu().numpy()), _bits(want_first[0]))
    assert np.array_equal(_bits(m[4].cpu().numpy()), _bits(want_first[1]))


def _queued(flights, sd, W, H, cams, xfs):
    """Frame 0: instances, a frame, AOVs with ids and the start of a history; frame 1: the moved instances, two
    accumulating device-output renders without stats, AOVs with ids, the reprojection of the second and its filter,
    all with device pointers on one stream: nothing waits on the host before the final synchronise."""
    import torch
    import prt
    n = W * H
    stream = torch.cuda.Stream()
    c = prt.Context(0)
    try:
        c.set_stream(stream.cuda_stream)
        scene, _ = gpu_scene(c, sd, W, H)
        c.set_frames_in_flight(flights)
        with torch.cuda.stream(stream):
            f4 = lambda: torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            avg, nd, alb = [f4() for _ in range(3)], [f4() for _ in range(2)], f4()
            ids = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
            h0, m0, out, mom, flt = (f4() for _ in range(5))
        c.set_instances(_blases(scene, xfs[0]))
        c.set_camera(cams[0])
        c.render(W, H, 2, 4, frame_index=0, avg=avg[0].data_ptr(), device_out=True, stats=False)
        c.render_aov_ids(W, H, device_out=True, normal_depth=nd[0].data_ptr(), instance=ids[0].data_ptr())
        c.reproject_moments(avg[0].data_ptr(), nd[0].data_ptr(), ids[0].data_ptr(), cams[0], width=W, height=H,
                            device_out=True, out=h0.data_ptr(), moments=m0.data_ptr())
        c.set_instances(_blases(scene, xfs[1]))
        c.set_camera(cams[1])
        c.reset_accumulation(full=True)
        for f in (1, 2):
            c.render(W, H, 2, 4, frame_index=f, avg=avg[f].data_ptr(), device_out=True, stats=False)
        c.render_aov_ids(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=nd[1].data_ptr(),
                         instance=ids[1].data_ptr())
        c.reproject_moments(avg[2].data_ptr(), nd[1].data_ptr(), ids[1].data_ptr(), cams[1], h0.data_ptr(),
                            nd[0].data_ptr(), cams[0], ids[0].data_ptr(), prt.instance_motion(xfs[1], xfs[0]),
                            m0.data_ptr(), width=W, height=H, device_out=True, out=out.data_ptr(),
                            moments=mom.data_ptr())
        c.denoise_variance(out.data_ptr(), mom.data_ptr(), alb.data_ptr(), nd[1].data_ptr(), W, H, device_out=True,
                           out=flt.data_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
        res = [t.cpu().numpy() for t in (avg[0], avg[2], nd[0], nd[1], alb, h0, m0, out, mom, flt)]
        return res + [t.cpu().numpy().view(np.uint32) for t in ids]
    finally:
        c.close()


def test_frames_in_flight():
    """The calls join the frames in flight: a frame still running on an internal stream when they are enqueued is
    reprojected and filtered complete, as if the frames had been rendered one at a time."""
    import prt
    sd, W, H = dr.scene_of(mr.SCENE)
    cams = [prt.Camera(p, t, F(W) / F(H)) for p, t in mr.camera_positions("slow")[:2]]
    xfs = [mr.transforms("B", k) for k in (0, 1)]
    one, two = _queued(1, sd, W, H, cams, xfs), _queued(2, sd, W, H, cams, xfs)
    for a, b in zip(one, two):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    a0, a2, nd0, nd1, alb, h0, m0, out, mom, flt, i0, i1 = two
    r0 = vr.reproject_moments(a0, nd0, i0, cams[0], W, H)
    assert np.array_equal(_bits(h0), _bits(r0[0])) and np.array_equal(_bits(m0), _bits(r0[1]))
    r1 = vr.reproject_moments(a2, nd1, i1, cams[1], W, H, h0, nd0, cams[0], i0,
                              prt.instance_motion(xfs[1], xfs[0]), m0)
    assert np.any(r1[0][:, 3] > 1)
    assert np.array_equal(_bits(out), _bits(r1[0])) and np.array_equal(_bits(mom), _bits(r1[1]))
    assert np.array_equal(_bits(flt), _bits(vr.denoise_variance(out, mom, alb, nd1, W, H)[0]))


def test_group_context(ctx):
    """A local shard group of two members on one device runs the calls over the whole image on member 0's device: the
    same images."""
    import prt
    v, u = _view(ctx, "multi_96x72", 1), _view(ctx, "multi_96x72", 0)
    hist = _ref_chain(ctx, "multi_96x72", 0)[-1]
    W, H = v["W"], v["H"]
    mo = prt.instance_motion(v["xf"], u["xf"])
    want = _dev_step(ctx, v, u, hist)
    wantf = ctx.denoise_variance(want[0], want[1], v["alb"], v["nd"], W, H)
    grp = prt.Context(group=[0, 0])
    try:
        scene, _ = gpu_scene(grp, dr.scene_of(mr.SCENE)[0], W, H)
        grp.set_instances(_blases(scene, v["xf"]))
        grp.set_camera(v["cam"])
        avg, _, _ = grp.render(W, H, 2, 4, frame_index=1)
        alb, nd, ids = grp.render_aov_ids(W, H)
        got = grp.reproject_moments(avg, nd, ids, v["cam"], hist[0], u["nd"], u["cam"], u["ids"], mo, hist[1],
                                    width=W, height=H)
        gotf = grp.denoise_variance(got[0], got[1], alb, nd, W, H)
    finally:
        grp.close()
    assert np.array_equal(_bits(avg), _bits(v["color"])) and np.array_equal(ids, v["ids"])
    for a, b in zip(got + gotf, want + wantf):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_argument_checks(ctx):
    """The refusals on a live context leave the outputs untouched, and the same calls with nothing wrong run."""
    import prt
    v, u = _view(ctx, "multi_96x72", 1), _view(ctx, "multi_96x72", 0)
    hist = _ref_chain(ctx, "multi_96x72", 0)[-1]
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    col, nd, ids = np.array(v["color"]), np.array(v["nd"]), np.array(v["ids"])
    mo = prt.instance_motion(v["xf"], u["xf"])
    with pytest.raises(prt.PrtError, match="prt error -1"):
        ctx.reproject_moments(col, nd, ids, v["cam"], hist[0], u["nd"], u["cam"], u["ids"], mo, None, width=W, height=H)
    with pytest.raises(prt.PrtError, match="prt error -1"):
        ctx.reproject_moments(col, nd, None, v["cam"], width=W, height=H)
    L, tp = ctx.L, prt.temporal_defaults()
    out, om = np.full((n, 4), 7, F), np.full((n, 4), 7, F)
    cp = C.byref(v["cam"].desc)
    rc = L.prt_reproject_moments(ctx.h, C.byref(tp), W, H, cp, col.ctypes.data, nd.ctypes.data, ids.ctypes.data, None,
                                 None, None, None, None, 0, None, col.ctypes.data, om.ctypes.data, None, 0)
    assert rc == -1 and np.all(om == 7) and np.array_equal(_bits(col), _bits(v["color"]))
    rc = L.prt_reproject_moments(ctx.h, C.byref(tp), W, H, cp, col.ctypes.data, nd.ctypes.data, ids.ctypes.data, None,
                                 None, None, None, None, 0, None, out.ctypes.data, om.ctypes.data, None, 0)
    assert rc == 0 and np.all(out[:, 3] == 1) and np.all(om[:, 3] == 0)
    with pytest.raises(prt.PrtError, match="prt error -1"):
        ctx.denoise_variance(out, om, v["alb"], nd, W, H, prt.denoise_variance_defaults(variance_floor=0.0))
    with pytest.raises(prt.PrtError, match="prt error -1"):
        ctx.denoise_variance(out, om, None, nd, W, H)


# ---- the Renderer mirror
def test_renderer_tick_temporal_variance():
    """Renderer.TickTemporalVariance over 4 frames of B/slow, the scene's blases updated each frame, equals the
    reference chain on the renderer's own frames; the history is the unfiltered output; a following
    TickTemporal(motion=True) starts a new history, and so does ResetTemporal()."""
    import prt
    sd, W, H = dr.scene_of(mr.SCENE)
    cams = [prt.Camera(p, t, F(W) / F(H)) for p, t in mr.camera_positions("slow")[:4]]
    R = prt.Renderer(prt.Scene.from_data(sd), prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H)), W, H)
    tp, fp = prt.temporal_defaults(clamp_k=1.5), prt.denoise_variance_defaults(iterations=3)
    try:
        hist = u = None
        for k, cam in enumerate(cams):
            xf = mr.transforms("B", k)
            R.scene.blases = _blases(R.scene, xf)
            R.camera = cam
            flt, scr, out = R.TickTemporalVariance(tp, fp)
            alb, nd, ids = R.ctx.render_aov_ids(W, H)
            v = dict(cam=cam, color=R.average, nd=nd, ids=ids, xf=xf, W=W, H=H)
            ref = _ref_step(v, u, hist, clamp_k=1.5)
            assert np.array_equal(_bits(out), _bits(ref[0])), k
            want = vr.denoise_variance(ref[0], ref[1], alb, nd, W, H, **dict(vr.FILTER_DEFAULTS, iterations=3))[0]
            assert np.array_equal(_bits(flt), _bits(want)) and np.array_equal(scr, dr.pack_rgb8(want)), k
            hist, u = ref, v
        assert out[:, 3].max() > len(cams) - 1e-3
        out, _ = R.TickTemporal(motion=True)
        assert np.all(out[:, 3] == 1)
        R.TickTemporalVariance()
        assert np.any(R.TickTemporalVariance()[2][:, 3] > 1)
        R.ResetTemporal()
        assert np.all(R.TickTemporalVariance()[2][:, 3] == 1)
        R.isPostProcessed = True
        with pytest.raises(ValueError, match="plane projection only"):
            R.TickTemporalVariance()
    finally:
        R.ctx.close()


# ---- quality on the device's own frames
# new / parent RMSE ratios measured on the device's frames (DESIGN.md "Variance guidance")
MEASURED = {"multi_rest": 0.7327, "multi_96x72": 0.7528, "multi_A_rest": 0.7394, "multi_static": 0.7385,
            "small_70x45": 0.7839}


@pytest.mark.parametrize("shape", list(MEASURED))
def test_quality_on_the_device(ctx, oracle_mod, shape):
    """tests/test_variance_ref.py::test_quality on the GPU's own frames, both pipelines chained on the device, against
    the oracle's 1024-spp frame of the last view: the ratio new / parent is at most halfway from the measured one to 1
    (B/rest, B/slow, A/rest, and `slow` over both scenes at rest)."""
    import prt
    vs = [_view(ctx, shape, k) for k in range(mr.FRAMES)]
    W, H = vs[0]["W"], vs[0]["H"]
    new = old = None
    for k, v in enumerate(vs):
        u = vs[k - 1] if k else None
        new = _dev_step(ctx, v, u, new)
        args = (old, u["nd"], u["cam"], u["ids"], prt.instance_motion(v["xf"], u["xf"])) if k else ()
        old, _ = ctx.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], *args, width=W, height=H)
    v = vs[-1]
    flt, _, _ = ctx.denoise_variance(new[0], new[1], v["alb"], v["nd"], W, H)
    par, _ = ctx.denoise(old, v["alb"], v["nd"], W, H)
    name, _, _, mseq, cseq = SHAPES[shape]
    conv = mr.converged_last(mseq, cseq) if mseq else rr.converged_last_slow(name)
    a, b = dr.rmse(flt, conv), dr.rmse(par, conv)
    print(f"{shape} on the device: RMSE {a:.4f} against the parent's {b:.4f}, ratio {a / b:.4f} "
          f"(measured {MEASURED[shape]:.4f}, limit {vr.bound(MEASURED[shape]):.4f})")
    assert a / b <= vr.bound(MEASURED[shape])
