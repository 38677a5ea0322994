"""First-hit AOVs and the a-trous denoiser on the device (include/prt.h prt_render_aov / prt_denoise,
csrc/prt_denoise.hip): the AOVs against the oracle's debug views and the primary hits bit for bit, the filter against
the numpy float32 reference (tests/denoise_ref.py) bit for bit, no side effect on the progressive accumulation, the
pointer variants, inputs from frames in flight and from a shard group, and the error against a converged render.

Scenes: multi_instance(config_small(40, 30)) at 96 x 72 and config_small(40, 30) at 70 x 45 -- the second is no
multiple of the 32 x 8 pixel block, and with a height below 65 the step-16 taps leave the image vertically -- plus
config_small at 9 x 7, where most taps of every step but the first lie outside."""
import numpy as np
import pytest

import denoise_ref as dr
from helpers import gpu_scene

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = list(dr.CASES)
_gpu = {}


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
    _gpu.clear()
    c.close()


def _case(ctx, name):
    """The GPU's own 2-spp frame (default flags, depth 4) and AOVs of a scene, made once; leaves `name` loaded."""
    sd, W, H = _scene(name)
    gpu_scene(ctx, sd, W, H)
    if name not in _gpu:
        avg, _, _ = ctx.render(W, H, 2, 4)
        alb, nd = ctx.render_aov(W, H)
        ctx.reset_accumulation(full=True)
        for a in (avg, alb, nd):
            a.setflags(write=False)
        _gpu[name] = dict(sd=sd, W=W, H=H, avg=avg, alb=alb, nd=nd)
    return _gpu[name]


def _assert_filter_equal(g, out, rgb8, ref, what):
    """rgb bit for bit, w copied, the packed pixels equal; on a mismatch the differing pixels' inputs are shown."""
    bad = np.flatnonzero(np.any(_bits(out[:, :3]) != _bits(ref[:, :3]), axis=1))
    if bad.size:
        k = bad[:4]
        lines = [f"pixel {p} (x {p % g['W']}, y {p // g['W']}): gpu {out[p]} ref {ref[p]} color {g['avg'][p]} "
                 f"albedo {g['alb'][p]} normal_depth {g['nd'][p]}" for p in k]
        raise AssertionError(f"{what}: {bad.size} of {len(out)} pixels differ\n" + "\n".join(lines))
    assert np.array_equal(_bits(out[:, 3]), _bits(g["avg"][:, 3])), what
    if rgb8 is not None:
        assert np.array_equal(rgb8, dr.pack_rgb8(ref)), what


@pytest.mark.parametrize("flags_name", ["NORMALMAP", "smooth"])
@pytest.mark.parametrize("name", NAMES)
def test_aov_parity(ctx, oracle_mod, name, flags_name):
    """albedo == the BASECOLOR view, (normal + 1) * 0.5 == the SHADINGNORMAL view (oracle and prt_render's own debug
    modes), w == prt_trace_primary's t, the miss masks agree; with and without normal mapping (the smooth branch
    leaves the normal unnormalised)."""
    import prt
    flags = prt.FLAG_NORMALMAP if flags_name == "NORMALMAP" else 0
    g = _case(ctx, name)
    W, H = g["W"], g["H"]
    alb, nd = ctx.render_aov(W, H, flags)
    osc = oracle_mod.OracleScene(g["sd"], W, H)
    m1, tp, _ = osc.render_frames(W, H, spp=1, bounces=1, flags=flags, mode=1)
    m3, _, _ = osc.render_frames(W, H, spp=1, bounces=1, flags=flags, mode=3)
    hit = nd[:, 3] < dr.FAR
    assert 0 < hit.sum() < hit.size
    assert np.array_equal(hit, tp[0] < dr.FAR)
    view3 = ((nd[:, :3] + F(1)) * F(0.5)).astype(F)
    assert np.array_equal(_bits(alb[hit, :3]), _bits(m1[0][hit, :3]))
    assert np.array_equal(_bits(view3[hit]), _bits(m3[0][hit, :3]))
    assert np.all(alb[hit, 3] == 1) and not alb[~hit].any()
    assert np.array_equal(nd[~hit], np.tile(np.array([0, 0, 0, 1e30], F), ((~hit).sum(), 1)))
    hits, _ = ctx.trace_primary(W, H)
    assert np.array_equal(_bits(nd[:, 3]), _bits(hits["t"]))
    try:
        g1, _, _ = ctx.render(W, H, 1, 1, flags=flags, mode=prt._lib.MODE_BASECOLOR)
        g3, _, _ = ctx.render(W, H, 1, 1, flags=flags, mode=prt._lib.MODE_SHADINGNORMAL)
    finally:
        ctx.reset_accumulation(full=True)
    assert np.array_equal(_bits(alb[hit, :3]), _bits(g1[hit, :3]))
    assert np.array_equal(_bits(view3[hit]), _bits(g3[hit, :3]))
    if flags_name == "NORMALMAP":
        assert np.array_equal(_bits(alb), _bits(g["alb"])) and np.array_equal(_bits(nd), _bits(g["nd"]))


def test_no_side_effect(ctx):
    """render_aov + denoise between two accumulating renders: the accumulation blob and the ray totals are the same
    before and after, and the second render equals the one made without the calls."""
    g = _case(ctx, "multi_96x72")
    W, H = g["W"], g["H"]
    try:
        ctx.render(W, H, 2, 4, frame_index=0)
        want, want8, _ = ctx.render(W, H, 2, 4, frame_index=1)
        ctx.reset_accumulation(full=True)
        a0, _, _ = ctx.render(W, H, 2, 4, frame_index=0)
        blob, totals = ctx.save_accumulation(), ctx.ray_totals()
        alb, nd = ctx.render_aov(W, H)
        out, _ = ctx.denoise(a0, alb, nd, W, H)
        assert not np.array_equal(out, a0)
        assert ctx.save_accumulation() == blob and ctx.ray_totals() == totals
        got, got8, _ = ctx.render(W, H, 2, 4, frame_index=1)
    finally:
        ctx.reset_accumulation(full=True)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got8, want8)


FILTER_CASES = [(n, {}) for n in NAMES] + [(n, dict(iterations=1)) for n in NAMES] + [
    ("small_70x45", dict(iterations=8)), ("multi_96x72", dict(iterations=2)),
    ("multi_96x72", dict(normal_power=0)), ("small_70x45", dict(normal_power=0)),
    ("multi_96x72", dict(normal_power=7)), ("small_70x45", dict(normal_power=7)),
    ("multi_96x72", dict(sigma_albedo=0.0)), ("small_70x45", dict(sigma_albedo=0.0)),
    ("small_9x7", {}), ("small_9x7", dict(iterations=8)),
]


@pytest.mark.parametrize("name,kw", FILTER_CASES, ids=lambda v: v if isinstance(v, str) else
                         ("defaults" if not v else "-".join(f"{k}{x}" for k, x in v.items())))
def test_filter_matches_reference_bitwise(ctx, name, kw):
    """The device filter of the GPU's own 2-spp frame with the GPU's AOVs against the numpy float32 reference: rgb bit
    for bit and the packed pixels, over the defaults, one, two and eight iterations,
    both ends of normal_power, no albedo guide, and the 9 x 7 image."""
    import prt
    g = _case(ctx, name)
    W, H = g["W"], g["H"]
    par = dict(dr.DEFAULTS, **kw)
    out, rgb8 = ctx.denoise(g["avg"], g["alb"], g["nd"], W, H, prt.denoise_defaults(**kw))
    ref = dr.denoise(g["avg"], g["alb"], g["nd"], W, H, **par)
    assert np.all(np.isfinite(ref))
    _assert_filter_equal(g, out, rgb8, ref, f"{name} {kw}")
    if par["sigma_albedo"] == 0:  # the albedo pointer is not needed then
        out2, _ = ctx.denoise(g["avg"], None, g["nd"], W, H, prt.denoise_defaults(**kw))
        assert np.array_equal(_bits(out2), _bits(out))


def _dev(stream, *arrays):
    import torch
    with torch.cuda.stream(stream):
        return [torch.from_numpy(np.array(a)).to("cuda") for a in arrays]


@pytest.mark.parametrize("name", NAMES)
def test_device_pointers_and_aliasing(ctx, name):
    """Device-pointer inputs and outputs (PRT_OUT_DEVICE, no host wait) give the host path's images; out_rgba may
    be the colour buffer itself (also for a single iteration, which filters a copy); either output may be absent."""
    import torch
    import prt
    g = _case(ctx, name)
    W, H, n = g["W"], g["H"], g["W"] * g["H"]
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            alb_t = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            nd_t = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            out_t = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            rgb_t = torch.zeros(n, dtype=torch.int32, device="cuda")
        col_t, = _dev(stream, g["avg"])
        ctx.render_aov(W, H, device_out=True, albedo=alb_t.data_ptr(), normal_depth=nd_t.data_ptr())
        ctx.denoise(col_t.data_ptr(), alb_t.data_ptr(), nd_t.data_ptr(), W, H, device_out=True,
                    out=out_t.data_ptr(), rgb8=rgb_t.data_ptr())
        res = {}
        for it in (1, 5):
            par = prt.denoise_defaults(iterations=it)
            inplace, = _dev(stream, g["avg"])
            ctx.denoise(inplace.data_ptr(), alb_t.data_ptr(), nd_t.data_ptr(), W, H, par, device_out=True,
                        out=inplace.data_ptr())
            with torch.cuda.stream(stream):  # zero-filled in the stream the filter writes it in, not beside it
                only8 = torch.zeros_like(rgb_t)
            ctx.denoise(col_t.data_ptr(), alb_t.data_ptr(), nd_t.data_ptr(), W, H, par, device_out=True,
                        rgb8=only8.data_ptr())
            res[it] = (inplace, only8)
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    assert np.array_equal(_bits(alb_t.cpu().numpy()), _bits(g["alb"]))
    assert np.array_equal(_bits(nd_t.cpu().numpy()), _bits(g["nd"]))
    assert np.array_equal(_bits(col_t.cpu().numpy()), _bits(g["avg"]))  # the input is left alone
    for it in (1, 5):
        want, want8 = ctx.denoise(g["avg"], g["alb"], g["nd"], W, H, prt.denoise_defaults(iterations=it))
        assert np.array_equal(_bits(res[it][0].cpu().numpy()), _bits(want)), it
        assert np.array_equal(res[it][1].cpu().numpy().view(np.uint32), want8), it
        if it == 5:
            assert np.array_equal(_bits(out_t.cpu().numpy()), _bits(want))
            assert np.array_equal(rgb_t.cpu().numpy().view(np.uint32), want8)


def _queued_frames(flights, sd, W, H, frames=3):
    """`frames` accumulating device-output renders without stats, then AOVs and the filter of the last frame, all with
    device pointers on one stream: nothing waits on the host before the final synchronise."""
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
            avg = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(frames)]
            rgb = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(frames)]
            alb, nd, out = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3))
        for f in range(frames):
            c.render(W, H, 2, 4, frame_index=f, avg=avg[f].data_ptr(), rgb8=rgb[f].data_ptr(), device_out=True,
                     stats=False)
        c.render_aov(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=nd.data_ptr())
        c.denoise(avg[-1].data_ptr(), alb.data_ptr(), nd.data_ptr(), W, H, device_out=True, out=out.data_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (avg[-1], alb, nd, out)]
    finally:
        c.close()


def test_frames_in_flight_then_denoise():
    """The AOV and filter calls join the frames in flight: a frame still running on an internal stream when they are
    enqueued is filtered complete, as if the frames had been rendered one at a time."""
    sd, W, H = dr.scene_of("multi_96x72")
    one, two = _queued_frames(1, sd, W, H), _queued_frames(2, sd, W, H)
    for a, b in zip(one, two):
        assert np.array_equal(_bits(a), _bits(b))
    avg, alb, nd, out = two
    assert np.array_equal(_bits(out), _bits(dr.denoise(avg, alb, nd, W, H, **dr.DEFAULTS)))


def test_group_context(ctx):
    """A local shard group runs both calls over the whole image on member 0's device: same AOVs, same image."""
    import prt
    g = _case(ctx, "multi_96x72")
    W, H = g["W"], g["H"]
    want, want8 = ctx.denoise(g["avg"], g["alb"], g["nd"], W, H)
    grp = prt.Context(group=[0, 0])
    try:
        gpu_scene(grp, g["sd"], W, H)
        avg, _, _ = grp.render(W, H, 2, 4)
        alb, nd = grp.render_aov(W, H)
        out, rgb8 = grp.denoise(avg, alb, nd, W, H)
    finally:
        grp.close()
    assert np.array_equal(_bits(avg), _bits(g["avg"]))
    assert np.array_equal(_bits(alb), _bits(g["alb"])) and np.array_equal(_bits(nd), _bits(g["nd"]))
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(rgb8, want8)


def test_renderer_denoise_leaves_the_renderer_alone():
    """Renderer.Denoise() filters the current average with fresh AOVs and returns the images; average, screen and the
    accumulation stay as Tick() left them."""
    import prt
    sd, W, H = dr.scene_of("small_70x45")
    R = [prt.Renderer(prt.Scene.from_data(sd), prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H)), W, H)
         for _ in range(2)]
    try:
        for r in R:
            r.bounces = 4
            r.Tick()
        avg0, scr0 = R[0].average.copy(), R[0].screen.copy()
        den, den8 = R[0].Denoise()
        assert np.array_equal(R[0].average, avg0) and np.array_equal(R[0].screen, scr0)
        alb, nd = R[0].ctx.render_aov(W, H)
        assert np.array_equal(_bits(den), _bits(dr.denoise(avg0, alb, nd, W, H, **dr.DEFAULTS)))
        assert np.array_equal(den8, dr.pack_rgb8(den))
        for r in R:
            r.Tick()
        assert np.array_equal(_bits(R[0].average), _bits(R[1].average)) and np.array_equal(R[0].screen, R[1].screen)
    finally:
        for r in R:
            r.ctx.close()


def test_aov_needs_scene_and_camera():
    """PRT_ERR_NOT_READY (-5) before a scene, and with a scene but no camera."""
    import prt
    sd, W, H = dr.scene_of("small_70x45")
    c = prt.Context(0)
    try:
        with pytest.raises(prt.PrtError, match="prt error -5"):
            c.render_aov(W, H)
        c.set_scene(prt.Scene.from_data(sd))
        with pytest.raises(prt.PrtError, match="prt error -5"):
            c.render_aov(W, H)
        c.set_camera(prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H)))
        alb, nd = c.render_aov(W, H)
        assert (nd[:, 3] < dr.FAR).any()
    finally:
        c.close()


def test_timings_are_recorded(ctx):
    """timed=True records one HIP event pair per pass; untimed entries read 0."""
    import prt
    g = _case(ctx, "small_70x45")
    W, H = g["W"], g["H"]
    ctx.render_aov(W, H, timed=True)
    ctx.denoise(g["avg"], g["alb"], g["nd"], W, H, prt.denoise_defaults(iterations=3), timed=True)
    ms = ctx.denoise_timings()
    assert len(ms) == 10 and all(m > 0 for m in ms[:5]) and not any(ms[5:])


@pytest.mark.parametrize("name", NAMES)
def test_quality_on_the_device(ctx, oracle_mod, name):
    """The GPU's 2-spp frame filtered with the GPU's AOVs against the oracle's 1024-spp frame: at most half the
    unfiltered RMSE, as for the reference on the CPU (tests/test_denoise_ref.py)."""
    g = _case(ctx, name)
    conv = dr.case(name)["converged"]
    out, _ = ctx.denoise(g["avg"], g["alb"], g["nd"], g["W"], g["H"])
    before, after = dr.rmse(g["avg"], conv), dr.rmse(out, conv)
    print(f"{name}: rmse {before:.4f} -> {after:.4f} (ratio {after / before:.3f})")
    assert after <= 0.5 * before, (before, after)
