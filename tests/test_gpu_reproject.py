"""Temporal reprojection on the device (include/prt.h prt_reproject, csrc/prt_temporal.hip) against the numpy float32
reference (tests/reproject_ref.py) bit for bit on the GPU's own frames and AOVs of moving cameras, an 8-step chain, no
side effect on the progressive accumulation, the pointer variants, frames in flight, a shard group, the argument
checks, Renderer.TickTemporal and the error against a converged render.

Scenes: multi_instance(config_small(40, 30)) at 96 x 72 and config_small(40, 30) at 70 x 45 (no multiple of the 32 x 8
pixel block), plus config_small at 9 x 7 under the fast sequence, where most taps leave the image."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import reproject_ref as rr
from helpers import gpu_scene

pytestmark = pytest.mark.gpu

F = np.float32
_views, _loaded = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _scene(name):
    if name == "small_9x7":
        return dr.scene_of("small_70x45")[0], 9, 7
    return dr.scene_of(name)


@pytest.fixture(scope="module")
def ctx():
    import prt
    c = prt.Context(0)
    yield c
    _views.clear()
    _loaded.clear()
    c.close()


def _load(ctx, name):
    sd, W, H = _scene(name)
    if _loaded.get("name") != name:
        gpu_scene(ctx, sd, W, H)
        _loaded["name"] = name
    return sd, W, H


def _view(ctx, name, seq, k):
    """The GPU's own 2-spp frame (default flags, depth 4, frame_index k) and AOVs of view k of a sequence, made once."""
    key = (name, seq, k)
    if key not in _views:
        sd, W, H = _load(ctx, name)
        cam = rr.cameras(sd, W, H, seq)[k]
        ctx.set_camera(cam)
        ctx.reset_accumulation(full=True)
        avg, _, _ = ctx.render(W, H, 2, 4, frame_index=k)
        alb, nd = ctx.render_aov(W, H)
        ctx.reset_accumulation(full=True)
        for a in (avg, alb, nd):
            a.setflags(write=False)
        _views[key] = dict(cam=cam, color=avg, alb=alb, nd=nd, W=W, H=H)
    return _views[key]


def _ref_chain(ctx, name, seq, upto):
    """The reference's outputs of steps 0..upto over the GPU's frames."""
    key = (name, seq, "chain")
    outs = _views.setdefault(key, [])
    while len(outs) <= upto:
        k = len(outs)
        v = _view(ctx, name, seq, k)
        if k == 0:
            outs.append(rr.reproject(v["color"], v["nd"], v["cam"], v["W"], v["H"]))
        else:
            u = _view(ctx, name, seq, k - 1)
            outs.append(rr.reproject(v["color"], v["nd"], v["cam"], v["W"], v["H"], outs[-1], u["nd"], u["cam"]))
        outs[-1].setflags(write=False)
    return outs


def _assert_equal(v, u, hist, out, rgb8, ref, what):
    """All four channels bit for bit and the packed pixels; on a mismatch the differing pixels' inputs are shown."""
    bad = np.flatnonzero(np.any(_bits(out) != _bits(ref), axis=1))
    if bad.size:
        lines = [f"pixel {p} (x {p % v['W']}, y {p // v['W']}): gpu {out[p]} ref {ref[p]} color {v['color'][p]} "
                 f"normal_depth {v['nd'][p]} history[p] {hist[p]} history_normal_depth[p] {u['nd'][p]}"
                 for p in bad[:4]]
        raise AssertionError(f"{what}: {bad.size} of {len(out)} pixels differ\n" + "\n".join(lines))
    if rgb8 is not None:
        assert np.array_equal(rgb8, dr.pack_rgb8(ref)), what


STEP_CASES = [("multi_96x72", "slow", 1), ("multi_96x72", "slow", 7), ("multi_96x72", "fast", 1),
              ("small_70x45", "slow", 1), ("multi_96x72", "rest", 1), ("multi_96x72", "behind", 1),
              ("small_9x7", "fast", 1)]


@pytest.mark.parametrize("name,seq,k", STEP_CASES, ids=lambda v: str(v))
def test_step_matches_reference_bitwise(ctx, name, seq, k):
    """One device step on the GPU's own frames and AOVs, the history being the reference's output of the step before:
    rgb, the history length and the packed pixels equal the reference's."""
    v, u = _view(ctx, name, seq, k), _view(ctx, name, seq, k - 1)
    hist = _ref_chain(ctx, name, seq, k - 1)[-1]
    W, H = v["W"], v["H"]
    info = {}
    ref = rr.reproject(v["color"], v["nd"], v["cam"], W, H, hist, u["nd"], u["cam"], info=info)
    out, rgb8 = ctx.reproject(v["color"], v["nd"], v["cam"], hist, u["nd"], u["cam"], width=W, height=H)
    hit, has = info["hit"], info["has_history"]
    print(f"{name} {seq} step {k}: {has.sum()} of {hit.sum()} hit pixels have history")
    assert hit.any()
    if seq == "behind":
        assert not info["valid"].any()
    elif name != "small_9x7":
        assert has.any() and (seq == "rest" or (hit & ~has).any())  # both branches are compared
    _assert_equal(v, u, hist, out, rgb8, ref, f"{name} {seq} step {k}")


VARIANTS = [dict(depth_tol=0.0), dict(normal_min=1.0), dict(normal_min=-1.0), dict(max_history=1.0), "checkerboard"]


@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: v if isinstance(v, str) else
                         "-".join(f"{k}{x}" for k, x in v.items()))
def test_parameter_variants_bitwise(ctx, var):
    """multi_96x72, slow: the ends of the parameter ranges, and a history whose length is 0 in a checkerboard (those
    taps are rejected one by one, so the bilinear weights no longer sum to 1)."""
    import prt
    k = 3
    v, u = _view(ctx, "multi_96x72", "slow", k), _view(ctx, "multi_96x72", "slow", k - 1)
    hist = np.array(_ref_chain(ctx, "multi_96x72", "slow", k - 1)[-1])
    W, H = v["W"], v["H"]
    kw = {}
    if var == "checkerboard":
        ys, xs = np.divmod(np.arange(W * H), W)
        hist[(xs + ys) % 2 == 0, 3] = 0
    else:
        kw = var
    info = {}
    ref = rr.reproject(v["color"], v["nd"], v["cam"], W, H, hist, u["nd"], u["cam"], info=info, **kw)
    out, rgb8 = ctx.reproject(v["color"], v["nd"], v["cam"], hist, u["nd"], u["cam"], width=W, height=H,
                              params=prt.reproject_defaults(**kw))
    _assert_equal(v, u, hist, out, rgb8, ref, str(var))
    has = info["has_history"]
    if kw.get("max_history") == 1.0:  # the output is this frame: h + 1 * (c - h), c up to the rounding of the two sums
        assert has.any() and np.all(out[:, 3] == 1)
        tol = 2.0 ** -22 * (np.abs(v["color"][:, :3]) + np.abs(hist[:, :3]).max())
        assert np.all(np.abs(out[:, :3] - v["color"][:, :3]) <= tol)
    if var == "checkerboard":
        assert has.any() and (info["hit"] & ~has).any()
    if kw.get("normal_min") == -1.0:  # no normal rejects a tap
        dflt = {}
        rr.reproject(v["color"], v["nd"], v["cam"], W, H, hist, u["nd"], u["cam"], info=dflt)
        assert has.sum() >= dflt["has_history"].sum() > 0


def test_chain_on_the_device(ctx):
    """Eight steps of `slow` with the device's own output as the next history equal the reference's chain."""
    name = "multi_96x72"
    ref = _ref_chain(ctx, name, "slow", rr.SLOW_FRAMES - 1)
    out = None
    for k in range(rr.SLOW_FRAMES):
        v = _view(ctx, name, "slow", k)
        if k == 0:
            out, rgb8 = ctx.reproject(v["color"], v["nd"], v["cam"], width=v["W"], height=v["H"])
        else:
            u = _view(ctx, name, "slow", k - 1)
            out, rgb8 = ctx.reproject(v["color"], v["nd"], v["cam"], out, u["nd"], u["cam"], width=v["W"],
                                      height=v["H"])
    assert np.array_equal(_bits(out), _bits(ref[-1])) and np.array_equal(rgb8, dr.pack_rgb8(ref[-1]))
    assert out[:, 3].max() > rr.SLOW_FRAMES - 1e-3


def test_no_side_effect(ctx):
    """reproject between two accumulating renders: the accumulation blob and the ray totals are the same before and
    after, and the second render equals the one made without the call."""
    name = "multi_96x72"
    v, u = _view(ctx, name, "slow", 1), _view(ctx, name, "slow", 0)
    hist = _ref_chain(ctx, name, "slow", 0)[-1]
    W, H = v["W"], v["H"]
    _load(ctx, name)
    ctx.set_camera(v["cam"])
    try:
        ctx.reset_accumulation(full=True)
        ctx.render(W, H, 2, 4, frame_index=0)
        want, want8, _ = ctx.render(W, H, 2, 4, frame_index=1)
        ctx.reset_accumulation(full=True)
        a0, _, _ = ctx.render(W, H, 2, 4, frame_index=0)
        blob, totals = ctx.save_accumulation(), ctx.ray_totals()
        out, _ = ctx.reproject(a0, v["nd"], v["cam"], hist, u["nd"], u["cam"], width=W, height=H)
        assert not np.array_equal(out[:, :3], a0[:, :3])
        assert ctx.save_accumulation() == blob and ctx.ray_totals() == totals
        got, got8, _ = ctx.render(W, H, 2, 4, frame_index=1)
    finally:
        ctx.reset_accumulation(full=True)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got8, want8)


def _dev(stream, *arrays):
    import torch
    with torch.cuda.stream(stream):
        return [torch.from_numpy(np.array(a)).to("cuda") for a in arrays]


@pytest.mark.parametrize("name", list(dr.CASES))
def test_device_pointers_and_aliasing(ctx, name):
    """Device-pointer images on a torch stream (PRT_OUT_DEVICE, no host wait) give the host path's image; out_rgba may
    be the colour buffer itself; either output may be absent; starting a history works with device pointers too."""
    import torch
    v, u = _view(ctx, name, "slow", 1), _view(ctx, name, "slow", 0)
    hist = _ref_chain(ctx, name, "slow", 0)[-1]
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    want, want8 = ctx.reproject(v["color"], v["nd"], v["cam"], hist, u["nd"], u["cam"], width=W, height=H)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        col, nd, h, hnd, inplace = _dev(stream, v["color"], v["nd"], hist, u["nd"], v["color"])
        with torch.cuda.stream(stream):
            out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            first = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            rgb, only8 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        args = (nd.data_ptr(), v["cam"], h.data_ptr(), hnd.data_ptr(), u["cam"])
        ctx.reproject(col.data_ptr(), *args, width=W, height=H, device_out=True, out=out.data_ptr(),
                      rgb8=rgb.data_ptr())
        ctx.reproject(inplace.data_ptr(), *args, width=W, height=H, device_out=True, out=inplace.data_ptr())
        ctx.reproject(col.data_ptr(), *args, width=W, height=H, device_out=True, rgb8=only8.data_ptr())
        ctx.reproject(col.data_ptr(), nd.data_ptr(), v["cam"], width=W, height=H, device_out=True,
                      out=first.data_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    assert np.array_equal(_bits(col.cpu().numpy()), _bits(v["color"]))  # the inputs are left alone
    assert np.array_equal(_bits(h.cpu().numpy()), _bits(hist))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(inplace.cpu().numpy()), _bits(want))
    assert np.array_equal(rgb.cpu().numpy().view(np.uint32), want8)
    assert np.array_equal(only8.cpu().numpy().view(np.uint32), want8)
    fresh = np.array(v["color"])
    fresh[:, 3] = 1
    assert np.array_equal(_bits(first.cpu().numpy()), _bits(fresh))


def _queued(flights, sd, W, H, cams):
    """View 0: a frame, AOVs and the start of a history; view 1: two accumulating device-output renders without
    stats, AOVs and the reprojection of the second, all with device pointers on one stream: nothing waits on the
    host before the final synchronise."""
    import torch
    import prt
    n = W * H
    stream = torch.cuda.Stream()
    c = prt.Context(0)
    try:
        c.set_stream(stream.cuda_stream)
        gpu_scene(c, sd, W, H)
        c.set_frames_in_flight(flights)
        with torch.cuda.stream(stream):
            avg = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
            nd = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
            h0, out = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        c.set_camera(cams[0])
        c.render(W, H, 2, 4, frame_index=0, avg=avg[0].data_ptr(), device_out=True, stats=False)
        c.render_aov(W, H, device_out=True, normal_depth=nd[0].data_ptr())
        c.reproject(avg[0].data_ptr(), nd[0].data_ptr(), cams[0], width=W, height=H, device_out=True,
                    out=h0.data_ptr())
        c.set_camera(cams[1])
        c.reset_accumulation(full=True)
        for f in (1, 2):
            c.render(W, H, 2, 4, frame_index=f, avg=avg[f].data_ptr(), device_out=True, stats=False)
        c.render_aov(W, H, device_out=True, normal_depth=nd[1].data_ptr())
        c.reproject(avg[2].data_ptr(), nd[1].data_ptr(), cams[1], h0.data_ptr(), nd[0].data_ptr(), cams[0], width=W,
                    height=H, device_out=True, out=out.data_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (avg[0], avg[2], nd[0], nd[1], h0, out)]
    finally:
        c.close()


def test_frames_in_flight_then_reproject():
    """The call joins the frames in flight: a frame still running on an internal stream when it is enqueued is
    reprojected complete, as if the frames had been rendered one at a time."""
    sd, W, H = dr.scene_of("multi_96x72")
    cams = rr.cameras(sd, W, H, "slow")[:2]
    one, two = _queued(1, sd, W, H, cams), _queued(2, sd, W, H, cams)
    for a, b in zip(one, two):
        assert np.array_equal(_bits(a), _bits(b))
    a0, a2, nd0, nd1, h0, out = two
    assert np.array_equal(_bits(h0), _bits(rr.reproject(a0, nd0, cams[0], W, H)))
    assert np.array_equal(_bits(out), _bits(rr.reproject(a2, nd1, cams[1], W, H, h0, nd0, cams[0])))


def test_group_context(ctx):
    """A local shard group runs the call over the whole image on member 0's device: the same image."""
    import prt
    name = "multi_96x72"
    v, u = _view(ctx, name, "slow", 1), _view(ctx, name, "slow", 0)
    hist = _ref_chain(ctx, name, "slow", 0)[-1]
    W, H = v["W"], v["H"]
    want, want8 = ctx.reproject(v["color"], v["nd"], v["cam"], hist, u["nd"], u["cam"], width=W, height=H)
    grp = prt.Context(group=[0, 0])
    try:
        gpu_scene(grp, _scene(name)[0], W, H)
        grp.set_camera(v["cam"])
        avg, _, _ = grp.render(W, H, 2, 4, frame_index=1)
        _, nd = grp.render_aov(W, H)
        out, rgb8 = grp.reproject(avg, nd, v["cam"], hist, u["nd"], u["cam"], width=W, height=H)
    finally:
        grp.close()
    assert np.array_equal(_bits(avg), _bits(v["color"])) and np.array_equal(_bits(nd), _bits(v["nd"]))
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(rgb8, want8)


def test_argument_checks(ctx):
    """Every refusal returns PRT_ERR_INVALID_ARGUMENT (-1) on a live context and leaves the output untouched."""
    import prt
    from prt import _lib
    name = "multi_96x72"
    v, u = _view(ctx, name, "slow", 1), _view(ctx, name, "slow", 0)
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    hist = np.array(_ref_chain(ctx, name, "slow", 0)[-1])
    hnd = np.array(u["nd"])
    out = np.full((n, 4), 7, F)
    out8 = np.full(n, 7, np.uint32)
    L, rp = ctx.L, prt.reproject_defaults()
    cp, pp = C.byref(v["cam"].desc), C.byref(u["cam"].desc)
    col, nd = np.array(v["color"]), np.array(v["nd"])

    def call(h=ctx.h, p=rp, w=W, hh=H, c=cp, color=col.ctypes.data, g=nd.ctypes.data, pc=pp, hi=hist.ctypes.data,
             hg=hnd.ctypes.data, o=out.ctypes.data, o8=out8.ctypes.data):
        return L.prt_reproject(h, C.byref(p) if p is not None else None, w, hh, c, color, g, pc, hi, hg, o, o8, 0)

    assert call(h=None) == -1 and call(p=None) == -1 and call(c=None) == -1
    assert call(color=None) == -1 and call(g=None) == -1 and call(o=None, o8=None) == -1
    assert call(w=0) == -1 and call(hh=0) == -1 and call(w=-W) == -1
    for kw in (dict(depth_tol=-0.1), dict(depth_tol=float("nan")), dict(depth_tol=float("inf")),
               dict(normal_min=1.5), dict(normal_min=-1.5), dict(normal_min=float("nan")),
               dict(max_history=0.5), dict(max_history=float("inf")), dict(max_history=float("nan"))):
        assert call(p=prt.reproject_defaults(**kw)) == -1, kw
    for kw in (dict(pc=None), dict(hi=None), dict(hg=None), dict(pc=None, hi=None), dict(pc=None, hg=None),
               dict(hi=None, hg=None)):
        assert call(**kw) == -1, kw
    keep_h, keep_g = hist.copy(), hnd.copy()
    assert call(o=hist.ctypes.data) == -1 and call(o=hnd.ctypes.data) == -1
    assert np.all(out == 7) and np.all(out8 == 7)
    assert np.array_equal(_bits(hist), _bits(keep_h)) and np.array_equal(_bits(hnd), _bits(keep_g))
    with pytest.raises(prt.PrtError, match="prt error -1"):
        ctx.reproject(col, nd, v["cam"], hist, None, u["cam"], width=W, height=H)
    assert call() == 0 and not np.all(out == 7)  # the same call with nothing wrong runs


def test_renderer_tick_temporal():
    """Renderer.TickTemporal over `slow` equals the explicit loop of Context calls, ResetTemporal() restarts the
    history, isPostProcessed raises, and a following Tick() equals that of a renderer that went through the same
    resets and Tick() calls with no reprojection."""
    import prt
    sd, W, H = dr.scene_of("small_70x45")
    cams = rr.cameras(sd, W, H, "slow")[:4]
    A, B = (prt.Renderer(prt.Scene.from_data(sd), prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H)), W, H)
            for _ in range(2))
    try:
        hist = hnd = prev = None
        for k, cam in enumerate(cams):
            A.camera = B.camera = cam
            out, scr = A.TickTemporal()
            B.ctx.set_camera(cam)
            B.ctx.reset_accumulation(full=True)
            B.Tick()
            assert np.array_equal(_bits(A.average), _bits(B.average)) and np.array_equal(A.screen, B.screen)
            _, nd = B.ctx.render_aov(W, H)
            want, want8 = B.ctx.reproject(B.average, nd, cam, hist, hnd, prev, width=W, height=H)
            assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(scr, want8), k
            ref = rr.reproject(B.average, nd, cam, W, H, hist, hnd, prev)
            assert np.array_equal(_bits(out), _bits(ref)), k
            hist, hnd, prev = want, nd, cam
        assert out[:, 3].max() > len(cams) - 1e-3
        A.isPostProcessed = True
        with pytest.raises(ValueError, match="plane projection only"):
            A.TickTemporal()
        A.isPostProcessed = False
        A.ResetTemporal()
        out, _ = A.TickTemporal(prt.reproject_defaults(max_history=4))
        B.ctx.reset_accumulation(full=True)
        B.Tick()
        assert np.all(out[:, 3] == 1) and np.array_equal(_bits(out[:, :3]), _bits(B.average[:, :3]))
        A.Tick()
        B.Tick()
        assert np.array_equal(_bits(A.average), _bits(B.average)) and np.array_equal(A.screen, B.screen)
    finally:
        A.ctx.close()
        B.ctx.close()


@pytest.mark.parametrize("name", list(dr.CASES))
def test_quality_on_the_device(ctx, oracle_mod, name):
    """The two assertions of tests/test_reproject_ref.py::test_quality on the GPU's own frames and AOVs, chained on
    the device, against the oracle's 1024-spp frame of the last view."""
    out = None
    for k in range(rr.SLOW_FRAMES):
        v = _view(ctx, name, "slow", k)
        args = (out, _view(ctx, name, "slow", k - 1)["nd"], _view(ctx, name, "slow", k - 1)["cam"]) if k else ()
        out, _ = ctx.reproject(v["color"], v["nd"], v["cam"], *args, width=v["W"], height=v["H"])
    single, repro, den_r, den_f = rr.quality(name, v["color"], out, v["alb"], v["nd"])
    print(f"{name}: rmse last frame {single:.4f}, reprojected {repro:.4f} (ratio {repro / single:.3f}); "
          f"denoised: reprojected {den_r:.4f}, last frame {den_f:.4f}")
    assert repro <= 0.45 * single, (single, repro)
    assert den_r < den_f, (den_r, den_f)
