"""Moving instances in the temporal reprojection on the device (include/prt.h prt_render_aov_ids, prt_instance_motion,
prt_reproject_motion; csrc/prt_motion.hip) against the numpy float32 reference (tests/motion_ref.py) bit for bit on the
GPU's own frames, AOVs and instance ids of a scene whose instance 1 moves: the id AOV, single steps, an 8-step chain,
the identity against prt_reproject, ids without a matrix, no side effect, the pointer variants, frames in flight, a
shard group, the argument checks, Renderer.TickTemporal(motion=True) and the error against a converged render.

Scenes: multi_instance(config_small(40, 30)) at 96 x 72 and 9 x 7, config_small(40, 30) at 70 x 45 (no multiple of the
32 x 8 pixel block), instance_field(70) at 64 x 48 (its ids come through the instance BVH)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import denoise_ref as dr
import motion_ref as mr
import reproject_ref as rr
from helpers import gpu_scene

pytestmark = pytest.mark.gpu

F = np.float32
_views, _loaded = {}, {}
W0, H0 = dr.CASES[mr.SCENE][1:]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import prt
    c = prt.Context(0)
    yield c
    _views.clear()
    _loaded.clear()
    c.close()


def _load(ctx, name, sd, W, H):
    """The scene `name` in the module's context (loaded again only when another one was there)."""
    if _loaded.get("name") != name:
        _loaded["scene"] = gpu_scene(ctx, sd, W, H)[0]
        _loaded["name"] = name
    return _loaded["scene"]


def _blases(scene, xf):
    return [(mi, xf[i]) for i, (mi, _) in enumerate(scene.blases)]


def _cams(cseq, W, H):
    import prt
    return [prt.Camera(p, t, F(W) / F(H)) for p, t in mr.camera_positions(cseq)]


def _view(ctx, mseq, cseq, k, W=W0, H=H0):
    """The GPU's own 2-spp frame (default flags, depth 4, frame_index k), AOVs and instance ids of frame k of an
    instance sequence under a camera sequence, made once."""
    key = (mseq, cseq, k, W, H)
    if key not in _views:
        scene = _load(ctx, mr.SCENE, dr.scene_of(mr.SCENE)[0], W, H)
        xf = mr.transforms(mseq, k)
        cam = _cams(cseq, W, H)[k]
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


def _static_view(ctx, name, seq, k):
    """A view of one of rr's camera sequences over a scene at rest, with the ids."""
    key = (name, seq, k)
    if key not in _views:
        sd, W, H = dr.scene_of(name)
        scene = _load(ctx, name, sd, W, H)
        ctx.set_instances(scene.blases)
        cam = rr.cameras(sd, W, H, seq)[k]
        ctx.set_camera(cam)
        ctx.reset_accumulation(full=True)
        avg, _, _ = ctx.render(W, H, 2, 4, frame_index=k)
        alb, nd, ids = ctx.render_aov_ids(W, H)
        ctx.reset_accumulation(full=True)
        xf = np.stack([np.asarray(T, F).reshape(4, 4) for _, T in scene.blases])
        for a in (avg, alb, nd, ids, xf):
            a.setflags(write=False)
        _views[key] = dict(cam=cam, color=avg, alb=alb, nd=nd, ids=ids, xf=xf, W=W, H=H)
    return _views[key]


def _ref_step(v, u, hist, with_ids=True, motion=None, info=None, **par):
    if u is None:
        return mr.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], v["W"], v["H"])
    mo = motion if motion is not None else mr.motion_f32(v["xf"], u["xf"])
    return mr.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], v["W"], v["H"], hist, u["nd"], u["cam"],
                               u["ids"] if with_ids else None, mo, info=info, **par)


def _dev_step(ctx, v, u, hist, with_ids=True, motion=None, params=None):
    if u is None:
        return ctx.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], width=v["W"], height=v["H"])
    import prt
    mo = motion if motion is not None else prt.instance_motion(v["xf"], u["xf"])
    return ctx.reproject_motion(v["color"], v["nd"], v["ids"], v["cam"], hist, u["nd"], u["cam"],
                                u["ids"] if with_ids else None, mo, width=v["W"], height=v["H"], params=params)


def _ref_chain(ctx, mseq, cseq, upto, W=W0, H=H0):
    """The reference's outputs of steps 0..upto over the GPU's frames (history_instance given)."""
    outs = _views.setdefault((mseq, cseq, "chain", W, H), [])
    while len(outs) <= upto:
        k = len(outs)
        v = _view(ctx, mseq, cseq, k, W, H)
        u = _view(ctx, mseq, cseq, k - 1, W, H) if k else None
        outs.append(_ref_step(v, u, outs[-1] if k else None))
        outs[-1].setflags(write=False)
    return outs


def _assert_equal(v, out, rgb8, ref, what):
    bad = np.flatnonzero(np.any(_bits(out) != _bits(ref), axis=1))
    if bad.size:
        lines = [f"pixel {p} (x {p % v['W']}, y {p // v['W']}): gpu {out[p]} ref {ref[p]} color {v['color'][p]} "
                 f"normal_depth {v['nd'][p]} id {v['ids'][p]}" for p in bad[:4]]
        raise AssertionError(f"{what}: {bad.size} of {len(out)} pixels differ\n" + "\n".join(lines))
    assert np.array_equal(rgb8, dr.pack_rgb8(ref)), what


# ---- the instance-id AOV
def _aov_scene(name):
    from prt import scenes
    if name == "instance_field_64x48":
        return scenes.instance_field(70), 64, 48
    return dr.scene_of(name)


@pytest.mark.parametrize("name", ["multi_96x72", "small_70x45", "instance_field_64x48"])
def test_render_aov_ids(ctx, name):
    """albedo and normal_depth are render_aov's bit for bit, and instance is trace_primary's inst where t < 1e30 and
    0xFFFFFFFF elsewhere; with more than 64 instances the ids come through the instance BVH."""
    import prt
    sd, W, H = _aov_scene(name)
    scene = _load(ctx, name, sd, W, H)
    ctx.set_instances(scene.blases)
    ctx.set_camera(prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H)))
    alb0, nd0 = ctx.render_aov(W, H)
    hits, _ = ctx.trace_primary(W, H)
    blob, totals = ctx.save_accumulation(), ctx.ray_totals()
    alb, nd, ids = ctx.render_aov_ids(W, H)
    assert ctx.save_accumulation() == blob and ctx.ray_totals() == totals
    assert np.array_equal(_bits(alb), _bits(alb0)) and np.array_equal(_bits(nd), _bits(nd0))
    hit = hits["t"] < F(1e30)
    assert 0 < hit.sum() < hit.size
    assert np.array_equal(ids, np.where(hit, hits["inst"], mr.MISS))
    assert np.array_equal(ids != mr.MISS, nd[:, 3] < F(1e30))
    seen = np.unique(ids[hit])
    print(f"{name}: {len(seen)} instances visible of {len(sd.instances)}")
    if name != "small_70x45":
        assert len(seen) >= 3


def test_render_aov_ids_null_outputs_and_device_pointers(ctx):
    """Every combination of absent outputs, with device pointers on a torch stream and with host pointers: the outputs
    asked for are the full call's, the others stay as they were; a timed call records the pass."""
    import torch
    sd, W, H = dr.scene_of(mr.SCENE)
    scene = _load(ctx, mr.SCENE, sd, W, H)
    ctx.set_instances(scene.blases)
    ctx.set_camera(rr.cameras(sd, W, H, "slow")[0])
    n = W * H
    alb, nd, ids = ctx.render_aov_ids(W, H, timed=True)
    assert ctx.denoise_timings()[0] > 0
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        got = []
        for use in itertools.product((False, True), repeat=3):
            with torch.cuda.stream(stream):
                a, g = (torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
                i = torch.full((n,), 7, dtype=torch.int32, device="cuda")
            ctx.render_aov_ids(W, H, device_out=True, albedo=a.data_ptr() if use[0] else None,
                               normal_depth=g.data_ptr() if use[1] else None, instance=i.data_ptr() if use[2] else None)
            got.append((use, a, g, i))
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    for use, a, g, i in got:
        a, g, i = a.cpu().numpy(), g.cpu().numpy(), i.cpu().numpy().view(np.uint32)
        assert np.array_equal(_bits(a), _bits(alb)) if use[0] else np.all(a == 7), use
        assert np.array_equal(_bits(g), _bits(nd)) if use[1] else np.all(g == 7), use
        assert np.array_equal(i, ids) if use[2] else np.all(i == 7), use
    L = ctx.L
    for use in itertools.product((False, True), repeat=3):  # host pointers
        a, g, i = np.full((n, 4), 7, F), np.full((n, 4), 7, F), np.full(n, 7, np.uint32)
        rc = L.prt_render_aov_ids(ctx.h, W, H, 8, a.ctypes.data if use[0] else None, g.ctypes.data if use[1] else None,
                                  i.ctypes.data if use[2] else None, 0)
        assert rc == 0
        assert np.array_equal(_bits(a), _bits(alb)) if use[0] else np.all(a == 7), use
        assert np.array_equal(_bits(g), _bits(nd)) if use[1] else np.all(g == 7), use
        assert np.array_equal(i, ids) if use[2] else np.all(i == 7), use
    assert L.prt_render_aov_ids(None, W, H, 8, None, None, None, 0) == -1
    assert L.prt_render_aov_ids(ctx.h, 0, H, 8, None, None, None, 0) == -1


# ---- single steps
STEP_CASES = [("A", "rest", 1, W0, H0), ("B", "rest", 1, W0, H0), ("B", "rest", 7, W0, H0), ("B", "slow", 3, W0, H0),
              ("B", "slow", 1, 9, 7)]


@pytest.mark.parametrize("with_ids", [True, False], ids=["ids", "noids"])
@pytest.mark.parametrize("mseq,cseq,k,W,H", STEP_CASES, ids=lambda v: str(v))
def test_step_matches_reference_bitwise(ctx, mseq, cseq, k, W, H, with_ids):
    """One device step on the GPU's own frames, AOVs and ids, the history being the reference's output of the step
    before: rgb, the history length and the packed pixels equal the reference's, with and without history_instance."""
    import prt
    v, u = _view(ctx, mseq, cseq, k, W, H), _view(ctx, mseq, cseq, k - 1, W, H)
    hist = _ref_chain(ctx, mseq, cseq, k - 1, W, H)[-1]
    mo = prt.instance_motion(v["xf"], u["xf"])
    assert not np.array_equal(mo[mr.MOVER], mr.IDENTITY) and np.array_equal(mo[0], mr.IDENTITY)
    info = {}
    ref = _ref_step(v, u, hist, with_ids, mo, info=info)
    out, rgb8 = _dev_step(ctx, v, u, hist, with_ids, mo)
    hit, has, mover = info["hit"], info["has_history"], v["ids"] == mr.MOVER
    print(f"{mseq}/{cseq} step {k} {W}x{H}: {has.sum()} of {hit.sum()} hit pixels have history, "
          f"{(has & mover).sum()} of {mover.sum()} on the mover")
    assert hit.any() and has.any()
    if (W, H) == (W0, H0):
        assert (has & mover).any() and (hit & ~has).any()  # the mover's blend and the start-over branch are compared
    _assert_equal(v, out, rgb8, ref, f"{mseq}/{cseq} step {k}")


@pytest.mark.parametrize("with_ids", [True, False], ids=["ids", "noids"])
def test_step_single_instance_identity(ctx, with_ids):
    """small_70x45 (one instance, `slow`, the identity matrix) step 1."""
    v, u = _static_view(ctx, "small_70x45", "slow", 1), _static_view(ctx, "small_70x45", "slow", 0)
    hist = _ref_step(u, None, None)
    info = {}
    ref = _ref_step(v, u, hist, with_ids, mr.identity(1), info=info)
    out, rgb8 = _dev_step(ctx, v, u, hist, with_ids, mr.identity(1))
    assert info["has_history"].any() and (info["hit"] & ~info["has_history"]).any()
    _assert_equal(v, out, rgb8, ref, "small_70x45 slow step 1")


VARIANTS = [dict(depth_tol=0.0), dict(normal_min=1.0), dict(normal_min=-1.0), dict(max_history=1.0), "checkerboard"]


@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: v if isinstance(v, str) else
                         "-".join(f"{k}{x}" for k, x in v.items()))
def test_parameter_variants_bitwise(ctx, var):
    """B/slow step 3 at the ends of the parameter ranges, and with a history whose length is 0 in a checkerboard."""
    import prt
    k = 3
    v, u = _view(ctx, "B", "slow", k), _view(ctx, "B", "slow", k - 1)
    hist = np.array(_ref_chain(ctx, "B", "slow", k - 1)[-1])
    kw = {}
    if var == "checkerboard":
        ys, xs = np.divmod(np.arange(W0 * H0), W0)
        hist[(xs + ys) % 2 == 0, 3] = 0
    else:
        kw = var
    info = {}
    ref = _ref_step(v, u, hist, info=info, **kw)
    out, rgb8 = _dev_step(ctx, v, u, hist, params=prt.reproject_defaults(**kw))
    _assert_equal(v, out, rgb8, ref, str(var))
    if kw.get("max_history") == 1.0:
        assert info["has_history"].any() and np.all(out[:, 3] == 1)
    if var == "checkerboard":
        assert info["has_history"].any() and (info["hit"] & ~info["has_history"]).any()


@pytest.mark.parametrize("name", list(dr.CASES))
def test_identity_equals_prt_reproject(ctx, name):
    """Identity matrices and no history_instance: the output is prt_reproject's bit for bit (`slow` step 1)."""
    v, u = _static_view(ctx, name, "slow", 1), _static_view(ctx, name, "slow", 0)
    W, H = v["W"], v["H"]
    hist = rr.reproject(u["color"], u["nd"], u["cam"], W, H)
    want, want8 = ctx.reproject(v["color"], v["nd"], v["cam"], hist, u["nd"], u["cam"], width=W, height=H)
    count = len(v["xf"])
    out, rgb8 = _dev_step(ctx, v, u, hist, False, mr.identity(count))
    assert np.any(want[:, 3] > 1) and np.array_equal(_bits(out), _bits(want)) and np.array_equal(rgb8, want8)
    import prt
    assert np.array_equal(prt.instance_motion(v["xf"], u["xf"]), mr.identity(count))


def test_chain_on_the_device(ctx):
    """Eight steps of B/slow with the device's own output as the next history equal the reference's chain."""
    ref = _ref_chain(ctx, "B", "slow", mr.FRAMES - 1)
    out = None
    for k in range(mr.FRAMES):
        v = _view(ctx, "B", "slow", k)
        out, rgb8 = _dev_step(ctx, v, _view(ctx, "B", "slow", k - 1) if k else None, out)
    assert np.array_equal(_bits(out), _bits(ref[-1])) and np.array_equal(rgb8, dr.pack_rgb8(ref[-1]))
    assert out[:, 3].max() > mr.FRAMES - 1e-3


def test_count_below_the_largest_id(ctx):
    """The pixels of instances without a matrix start over; the others equal the reference (and the full call)."""
    v, u = _view(ctx, "B", "rest", 1), _view(ctx, "B", "rest", 0)
    hist = _ref_chain(ctx, "B", "rest", 0)[-1]
    mo = mr.motion_f32(v["xf"], u["xf"])
    full, _ = _dev_step(ctx, v, u, hist, True, mo)
    for count in (1, 2):
        out, rgb8 = _dev_step(ctx, v, u, hist, True, mo[:count])
        _assert_equal(v, out, rgb8, _ref_step(v, u, hist, True, mo[:count]), f"count {count}")
        beyond = (v["ids"] != mr.MISS) & (v["ids"] >= count)
        assert beyond.any() and np.all(out[beyond, 3] == 1) and np.any(full[beyond, 3] > 1)
        assert np.array_equal(_bits(out[beyond, :3]), _bits(v["color"][beyond, :3]))
        assert np.array_equal(_bits(out[~beyond]), _bits(full[~beyond]))


# ---- the pass's properties
def test_no_side_effect(ctx):
    """reproject_motion between two accumulating renders: the accumulation blob and the ray totals are the same before
    and after, and the second render equals the one made without the call."""
    v, u = _view(ctx, "B", "slow", 1), _view(ctx, "B", "slow", 0)
    hist = _ref_chain(ctx, "B", "slow", 0)[-1]
    W, H = v["W"], v["H"]
    ctx.set_instances(_blases(_load(ctx, mr.SCENE, dr.scene_of(mr.SCENE)[0], W, H), v["xf"]))
    ctx.set_camera(v["cam"])
    try:
        ctx.reset_accumulation(full=True)
        ctx.render(W, H, 2, 4, frame_index=0)
        want, want8, _ = ctx.render(W, H, 2, 4, frame_index=1)
        ctx.reset_accumulation(full=True)
        a0, _, _ = ctx.render(W, H, 2, 4, frame_index=0)
        blob, totals = ctx.save_accumulation(), ctx.ray_totals()
        out, _ = ctx.reproject_motion(a0, v["nd"], v["ids"], v["cam"], hist, u["nd"], u["cam"], u["ids"],
                                      mr.motion_f32(v["xf"], u["xf"]), width=W, height=H)
        assert not np.array_equal(out[:, :3], a0[:, :3])
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


def test_device_pointers_and_aliasing(ctx):
    """Device-pointer images on a torch stream (PRT_OUT_DEVICE, no host wait) give the host path's image; out_rgba may
    be the colour buffer itself; either output may be absent; history_instance may be absent; starting a history works
    with device pointers too.  The matrices are a host array that is changed right after each call: it was copied."""
    import torch
    v, u = _view(ctx, "B", "slow", 1), _view(ctx, "B", "slow", 0)
    hist = _ref_chain(ctx, "B", "slow", 0)[-1]
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    mo = mr.motion_f32(v["xf"], u["xf"])
    want, want8 = _dev_step(ctx, v, u, hist, True, mo)
    want_noids, _ = _dev_step(ctx, v, u, hist, False, mo)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        col, nd, ids, h, hnd, hids, inplace = _dev(stream, v["color"], v["nd"], v["ids"], hist, u["nd"], u["ids"],
                                                   v["color"])
        with torch.cuda.stream(stream):
            out, first, noids = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3))
            rgb, only8 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))

        def call(color, hi=hids.data_ptr(), **kw):
            m = mo.copy()
            ctx.reproject_motion(color, nd.data_ptr(), ids.data_ptr(), v["cam"], h.data_ptr(), hnd.data_ptr(),
                                 u["cam"], hi, m, width=W, height=H, device_out=True, **kw)
            m[:] = np.nan  # the call has copied the matrices

        call(col.data_ptr(), out=out.data_ptr(), rgb8=rgb.data_ptr())
        call(inplace.data_ptr(), out=inplace.data_ptr())
        call(col.data_ptr(), rgb8=only8.data_ptr())
        call(col.data_ptr(), hi=None, out=noids.data_ptr())
        ctx.reproject_motion(col.data_ptr(), nd.data_ptr(), ids.data_ptr(), v["cam"], width=W, height=H,
                             device_out=True, out=first.data_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    assert np.array_equal(_bits(col.cpu().numpy()), _bits(v["color"]))  # the inputs are left alone
    assert np.array_equal(_bits(h.cpu().numpy()), _bits(hist))
    assert np.array_equal(hids.cpu().numpy().view(np.uint32), u["ids"])
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(inplace.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(noids.cpu().numpy()), _bits(want_noids))
    assert np.array_equal(rgb.cpu().numpy().view(np.uint32), want8)
    assert np.array_equal(only8.cpu().numpy().view(np.uint32), want8)
    fresh = np.array(v["color"])
    fresh[:, 3] = 1
    assert np.array_equal(_bits(first.cpu().numpy()), _bits(fresh))


def _queued(flights, sd, W, H, cams, xfs):
    """Frame 0: instances, a frame, AOVs with ids and the start of a history; frame 1: the moved instances, two
    accumulating device-output renders without stats, AOVs with ids and the reprojection of the second, all with device
    pointers on one stream: nothing waits on the host before the final synchronise."""
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
            avg = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
            nd = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
            ids = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
            h0, out = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        c.set_instances(_blases(scene, xfs[0]))
        c.set_camera(cams[0])
        c.render(W, H, 2, 4, frame_index=0, avg=avg[0].data_ptr(), device_out=True, stats=False)
        c.render_aov_ids(W, H, device_out=True, normal_depth=nd[0].data_ptr(), instance=ids[0].data_ptr())
        c.reproject_motion(avg[0].data_ptr(), nd[0].data_ptr(), ids[0].data_ptr(), cams[0], width=W, height=H,
                           device_out=True, out=h0.data_ptr())
        c.set_instances(_blases(scene, xfs[1]))
        c.set_camera(cams[1])
        c.reset_accumulation(full=True)
        for f in (1, 2):
            c.render(W, H, 2, 4, frame_index=f, avg=avg[f].data_ptr(), device_out=True, stats=False)
        c.render_aov_ids(W, H, device_out=True, normal_depth=nd[1].data_ptr(), instance=ids[1].data_ptr())
        c.reproject_motion(avg[2].data_ptr(), nd[1].data_ptr(), ids[1].data_ptr(), cams[1], h0.data_ptr(),
                           nd[0].data_ptr(), cams[0], ids[0].data_ptr(), prt.instance_motion(xfs[1], xfs[0]), width=W,
                           height=H, device_out=True, out=out.data_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
        res = [t.cpu().numpy() for t in (avg[0], avg[2], nd[0], nd[1], h0, out)]
        return res + [t.cpu().numpy().view(np.uint32) for t in ids]
    finally:
        c.close()


def test_frames_in_flight_then_reproject():
    """The calls join the frames in flight: a frame still running on an internal stream when they are enqueued is
    reprojected complete, as if the frames had been rendered one at a time."""
    sd, W, H = dr.scene_of(mr.SCENE)
    cams = _cams("slow", W, H)[:2]
    xfs = [mr.transforms("B", k) for k in (0, 1)]
    one, two = _queued(1, sd, W, H, cams, xfs), _queued(2, sd, W, H, cams, xfs)
    for a, b in zip(one, two):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    a0, a2, nd0, nd1, h0, out, i0, i1 = two
    assert np.array_equal(_bits(h0), _bits(mr.reproject_motion(a0, nd0, i0, cams[0], W, H)))
    ref = mr.reproject_motion(a2, nd1, i1, cams[1], W, H, h0, nd0, cams[0], i0, mr.motion_f32(xfs[1], xfs[0]))
    assert np.any(ref[i1 == mr.MOVER, 3] > 1) and np.array_equal(_bits(out), _bits(ref))


def test_group_context(ctx):
    """A local shard group runs the calls over the whole image on member 0's device: the same images."""
    import prt
    v, u = _view(ctx, "B", "slow", 1), _view(ctx, "B", "slow", 0)
    hist = _ref_chain(ctx, "B", "slow", 0)[-1]
    W, H = v["W"], v["H"]
    mo = mr.motion_f32(v["xf"], u["xf"])
    want, want8 = _dev_step(ctx, v, u, hist, True, mo)
    grp = prt.Context(group=[0, 0])
    try:
        scene, _ = gpu_scene(grp, dr.scene_of(mr.SCENE)[0], W, H)
        grp.set_instances(_blases(scene, v["xf"]))
        grp.set_camera(v["cam"])
        avg, _, _ = grp.render(W, H, 2, 4, frame_index=1)
        _, nd, ids = grp.render_aov_ids(W, H)
        out, rgb8 = grp.reproject_motion(avg, nd, ids, v["cam"], hist, u["nd"], u["cam"], u["ids"], mo, width=W,
                                         height=H)
    finally:
        grp.close()
    assert np.array_equal(_bits(avg), _bits(v["color"])) and np.array_equal(_bits(nd), _bits(v["nd"]))
    assert np.array_equal(ids, v["ids"])
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(rgb8, want8)


def test_argument_checks(ctx):
    """Every refusal returns PRT_ERR_INVALID_ARGUMENT (-1) on a live context and leaves the outputs untouched."""
    import prt
    v, u = _view(ctx, "B", "slow", 1), _view(ctx, "B", "slow", 0)
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    hist, hnd, hids = np.array(_ref_chain(ctx, "B", "slow", 0)[-1]), np.array(u["nd"]), np.array(u["ids"])
    out = np.full((n, 4), 7, F)
    out8 = np.full(n, 7, np.uint32)
    L, rp = ctx.L, prt.reproject_defaults()
    cp, pp = C.byref(v["cam"].desc), C.byref(u["cam"].desc)
    col, nd, ids = np.array(v["color"]), np.array(v["nd"]), np.array(v["ids"])
    mo = mr.motion_f32(v["xf"], u["xf"])

    def call(h=ctx.h, p=rp, w=W, hh=H, c=cp, color=col.ctypes.data, g=nd.ctypes.data, i=ids.ctypes.data, pc=pp,
             hi=hist.ctypes.data, hg=hnd.ctypes.data, hj=hids.ctypes.data, m=mo.ctypes.data, cnt=len(mo),
             o=out.ctypes.data, o8=out8.ctypes.data):
        return L.prt_reproject_motion(h, C.byref(p) if p is not None else None, w, hh, c, color, g, i, pc, hi, hg, hj,
                                      m, cnt, o, o8, 0)

    assert call(h=None) == -1 and call(p=None) == -1 and call(c=None) == -1
    assert call(color=None) == -1 and call(g=None) == -1 and call(o=None, o8=None) == -1
    assert call(w=0) == -1 and call(hh=0) == -1 and call(w=-W) == -1
    for kw in (dict(depth_tol=-0.1), dict(depth_tol=float("nan")), dict(depth_tol=float("inf")),
               dict(normal_min=1.5), dict(normal_min=-1.5), dict(normal_min=float("nan")),
               dict(max_history=0.5), dict(max_history=float("inf")), dict(max_history=float("nan"))):
        assert call(p=prt.reproject_defaults(**kw)) == -1, kw
    for kw in (dict(pc=None), dict(hi=None), dict(hg=None), dict(m=None), dict(cnt=0), dict(cnt=-1),
               dict(pc=None, hi=None), dict(pc=None, hi=None, hg=None), dict(pc=None, hi=None, hg=None, m=None),
               dict(pc=None, hi=None, hg=None, cnt=0), dict(pc=None, hi=None, hg=None, m=None, cnt=0),
               dict(i=None)):
        assert call(**kw) == -1, kw
    keep_h, keep_g, keep_j = hist.copy(), hnd.copy(), hids.copy()
    assert call(o=hist.ctypes.data) == -1 and call(o=hnd.ctypes.data) == -1 and call(o8=hids.ctypes.data) == -1
    assert np.all(out == 7) and np.all(out8 == 7)
    assert np.array_equal(_bits(hist), _bits(keep_h)) and np.array_equal(_bits(hnd), _bits(keep_g))
    assert np.array_equal(hids, keep_j)
    with pytest.raises(prt.PrtError, match="prt error -1"):
        ctx.reproject_motion(col, nd, ids, v["cam"], hist, None, u["cam"], hids, mo, width=W, height=H)
    assert call(pc=None, hi=None, hg=None, hj=None, m=None, cnt=0, i=None) == 0  # a history starts: no ids needed
    assert np.all(out[:, 3] == 1)
    out[:] = 7
    assert call() == 0 and not np.all(out == 7)  # the same call with nothing wrong runs


# ---- the Renderer mirror
def test_renderer_tick_temporal_motion():
    """Renderer.TickTemporal(motion=True) over B/slow, the scene's blases updated each frame, equals the explicit loop
    of Context calls and the reference; motion=False on the same renderer gives today's TickTemporal outputs; a
    changed instance count restarts the history."""
    import prt
    sd, W, H = dr.scene_of(mr.SCENE)
    cams = _cams("slow", W, H)[:4]
    mk = lambda: prt.Renderer(prt.Scene.from_data(sd), prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H)), W, H)
    A, B, P = mk(), mk(), mk()
    try:
        hist = hnd = hids = prev = pxf = None
        for k, cam in enumerate(cams):
            xf = mr.transforms("B", k)
            A.scene.blases = _blases(A.scene, xf)
            A.camera = B.camera = cam
            out, scr = A.TickTemporal(motion=True)
            B.ctx.set_instances(_blases(B.scene, xf))
            B.ctx.set_camera(cam)
            B.ctx.reset_accumulation(full=True)
            B.Tick()
            assert np.array_equal(_bits(A.average), _bits(B.average)) and np.array_equal(A.screen, B.screen)
            _, nd, ids = B.ctx.render_aov_ids(W, H)
            mo = prt.instance_motion(xf, pxf) if k else None
            want, want8 = B.ctx.reproject_motion(B.average, nd, ids, cam, hist, hnd, prev, hids, mo, width=W, height=H)
            assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(scr, want8), k
            ref = mr.reproject_motion(B.average, nd, ids, cam, W, H, hist, hnd, prev, hids, mo)
            assert np.array_equal(_bits(out), _bits(ref)), k
            hist, hnd, hids, prev, pxf = want, nd, ids, cam, xf
        assert out[ids == mr.MOVER, 3].max() > len(cams) - 1e-3
        # motion=False is the plain TickTemporal: a renderer that never used motion gives the same outputs
        A.ResetTemporal()
        for cam in cams[:2]:
            A.camera = P.camera = cam
            P.scene.blases = list(A.scene.blases)
            P.ctx.set_instances(P.scene.blases)
            P.frame = A.frame  # the same samples
            got, got8 = A.TickTemporal()
            want, want8 = P.TickTemporal()
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got8, want8)
        assert np.any(got[:, 3] > 1)
        # a changed instance count starts a new history
        A.TickTemporal(motion=True)
        out, _ = A.TickTemporal(motion=True)
        assert np.any(out[:, 3] > 1)
        A.scene.blases = A.scene.blases[:2]
        out, _ = A.TickTemporal(motion=True)
        assert np.all(out[:, 3] == 1)
        out, _ = A.TickTemporal(motion=True)
        assert np.any(out[:, 3] > 1)
        A.isPostProcessed = True
        with pytest.raises(ValueError, match="plane projection only"):
            A.TickTemporal(motion=True)
    finally:
        for r in (A, B, P):
            r.ctx.close()


def test_quality_on_the_device(ctx, oracle_mod):
    """The assertions of tests/test_motion_ref.py::test_quality_and_coverage for B/rest on the GPU's own frames, both
    passes chained on the device, against the oracle's 1024-spp frame of the last frame's configuration."""
    vs = [_view(ctx, "B", "rest", k) for k in range(mr.FRAMES)]
    plain = moved = None
    for k, v in enumerate(vs):
        u = vs[k - 1] if k else None
        args = (plain, u["nd"], u["cam"]) if k else ()
        plain, _ = ctx.reproject(v["color"], v["nd"], v["cam"], *args, width=v["W"], height=v["H"])
        moved, _ = _dev_step(ctx, v, u, moved)
    f = mr.figures(vs, plain, moved, mr.converged_last("B", "rest"))
    print("B/rest on the device: " + ", ".join(f"{k} {x:.4f}" for k, x in f.items()))
    mr.check_quality(f)
