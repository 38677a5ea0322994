"""The reprojection that follows deforming meshes on the device (include/prt.h prt_snapshot_mesh,
prt_render_aov_deform, prt_reproject_deform; csrc/prt_deform.hip) against the numpy float32 reference
(tests/deform_ref.py) bit for bit on the GPU's own hits, frames and AOVs: the offset output over scenes, builders and
both update paths, the snapshot's semantics, single steps and an eight-frame chain of the pass, its identities against
prt_reproject_moments, the pointer variants, frames in flight, a shard group, no side effect, the refusals,
Renderer.TrackModel / TickTemporalVariance(deform=True) and the quality figures on the device's frames.

Scenes: multi_instance(config_small(40, 30)) with the mover on a mesh of its own (deform_ref.scene(): one of two meshes
snapshotted) at 96 x 72 and 70 x 45 (no multiple of the 32 x 8 pixel block), the same scene with all three instances
on the one snapshotted mesh, config_small(40, 30) at 70 x 45, and instance_field(70) at 64 x 48 (70 instances of the
snapshotted torus, reached through the instance BVH)."""
import numpy as np
import pytest

import deform
import deform_ref as df
import denoise_ref as dr
import motion_ref as mr
import variance_ref as vr
from helpers import gpu_scene
from prt import _lib

pytestmark = pytest.mark.gpu

F = np.float32
BUILDERS = {"host_sah": _lib.BUILDER_HOST_SAH, "host_sbvh": _lib.BUILDER_HOST_SBVH, "gpu_ploc": _lib.BUILDER_GPU_PLOC}
_views, _chains, _state = {}, {}, {}


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import prt
    c = prt.Context(0)
    yield c
    _views.clear()
    _chains.clear()
    _state.clear()
    c.close()


class _DeviceMesh:
    def __init__(self, m):
        import torch
        for n in ("triangles", "fixed_normals", "fixed_uvs", "vertices", "face_normals"):
            setattr(self, n, torch.from_numpy(np.ascontiguousarray(getattr(m, n), np.float32)).cuda())
        self.indices = torch.from_numpy(np.ascontiguousarray(m.indices, np.int32)).cuda()
        self.albedo, self.normal, self.metalness, self.emission = m.albedo, m.normal, m.metalness, m.emission
        torch.cuda.synchronize()


def _disturb():
    """The module's context no longer holds a frame of the sequence (_view loads it again)."""
    _state.clear()


def _update(c, index, mesh, device=False):
    if device:
        c.update_mesh(index, _DeviceMesh(mesh), device=True)
    else:
        c.update_mesh(index, mesh)


# name -> (scene, W, H, index of the mesh that is snapshotted and deformed, its deformed version)
def _offset_case(name):
    from prt import scenes
    if name == "multi_own":
        sd, W, H = df.scene()
        return sd, W, H, 1, df.mesh_at(1)
    if name == "multi_shared":
        sd, W, H = dr.scene_of(mr.SCENE)
        return sd, W, H, 0, deform.travelling_sine(sd.meshes[0], 0.4, t=0.7, k=1.0)
    if name == "small_70x45":
        sd, W, H = dr.scene_of("small_70x45")
        return sd, W, H, 0, deform.sine_twist(sd.meshes[0], amp=0.3, twist=0.05)
    assert name == "field_64x48"
    sd = scenes.instance_field(70)
    return sd, 64, 48, 1, deform.sine_twist(sd.meshes[1], amp=0.04, twist=1.0)


def _with_mesh(sd, index, mesh):
    ms = list(sd.meshes)
    ms[index] = mesh
    return ms


def _snaps(sd, index, mesh):
    return [mesh if m == index else None for m in range(len(sd.meshes))]


def _assert_rows(got, want, what):
    bad = np.flatnonzero(np.any(_bits(got) != _bits(want), axis=1))
    if bad.size:
        lines = [f"pixel {p}: gpu {got[p]} ref {want[p]}" for p in bad[:4]]
        raise AssertionError(f"{what}: {bad.size} of {len(got)} rows differ\n" + "\n".join(lines))


# ---- the offset output
@pytest.mark.parametrize("name,builder,device", [
    ("multi_own", "host_sah", False), ("multi_own", "gpu_ploc", True), ("multi_shared", "host_sbvh", False),
    ("multi_shared", "host_sah", True), ("small_70x45", "host_sbvh", True), ("small_70x45", "gpu_ploc", False),
    ("field_64x48", "host_sah", False), ("field_64x48", "gpu_ploc", True)])
def test_offset_matches_reference_bitwise(name, builder, device):
    """Snapshot, update (host arrays or PRT_IN_DEVICE), then the offset equals offset_ref fed the device's own
    prt_trace_primary hits, bit for bit; the other three outputs are prt_render_aov_ids'."""
    import prt
    sd, W, H, mi, v1 = _offset_case(name)
    c = prt.Context(0)
    try:
        c.set_bvh_builder(BUILDERS[builder])
        gpu_scene(c, sd, W, H)
        c.snapshot_mesh(mi)
        _update(c, mi, v1, device)
        hits, _ = c.trace_primary(W, H)
        alb, nd, ids, off = c.render_aov_deform(W, H)
        want = c.render_aov_ids(W, H)
    finally:
        c.close()
    ref = df.offset_ref(hits, df.instance_mesh(sd), _with_mesh(sd, mi, v1), _snaps(sd, mi, sd.meshes[mi]))
    on = ref[:, 3] == 1
    print(f"{name} {builder}: {on.sum()} of {len(ref)} pixels on the snapshotted mesh, "
          f"{len(np.unique(ids[on]))} instances, largest offset {np.abs(ref[:, :3]).max():.3f}")
    assert on.any() and (~on).any() and np.any(ref[on, :3] != 0)
    if name in ("multi_shared", "field_64x48"):
        assert len(np.unique(ids[on])) >= 2  # one snapshotted mesh under several instances
    if name in ("multi_own", "field_64x48"):
        assert np.any((ids != mr.MISS) & ~on)  # hits on a mesh without a snapshot
    _assert_rows(off, ref, f"{name} {builder}")
    for a, b in zip((alb, nd, ids), want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_snapshot_semantics(ctx):
    """No snapshot: zeros.  A snapshot without an update: exactly (0, 0, 0, 1) on that mesh.  Two updates after one
    snapshot measure against the snapshot, not the state in between.  A second snapshot overwrites the first.
    prt_set_meshes discards the snapshot.  The other outputs are prt_render_aov_ids' with and without a snapshot."""
    _disturb()
    sd, W, H = df.scene()
    gpu_scene(ctx, sd, W, H)
    imesh = df.instance_mesh(sd)
    v0, v1, v2 = sd.meshes[1], df.mesh_at(1), df.mesh_at(3)
    want = ctx.render_aov_ids(W, H)
    alb, nd, ids, off = ctx.render_aov_deform(W, H)
    assert not off.any()
    for a, b in zip((alb, nd, ids), want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    ctx.snapshot_mesh(1)
    alb, nd, ids, off = ctx.render_aov_deform(W, H)
    mover = ids == df.MOVER
    assert mover.any() and (~mover & (ids != mr.MISS)).any()
    assert np.array_equal(_bits(off[mover]), _bits(np.tile(np.array([0, 0, 0, 1], F), (mover.sum(), 1))))
    assert not off[~mover].any()
    for a, b in zip((alb, nd, ids), want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    ctx.update_mesh(1, v1)
    ctx.update_mesh(1, v2)
    hits, _ = ctx.trace_primary(W, H)
    off = ctx.render_aov_deform(W, H)[3]
    _assert_rows(off, df.offset_ref(hits, imesh, [sd.meshes[0], v2], [None, v0]), "two updates")
    assert not np.array_equal(_bits(off), _bits(df.offset_ref(hits, imesh, [sd.meshes[0], v2], [None, v1])))
    ctx.snapshot_mesh(1)  # overwrites: the previous positions are v2's now
    ctx.update_mesh(1, v1)
    hits, _ = ctx.trace_primary(W, H)
    _assert_rows(ctx.render_aov_deform(W, H)[3], df.offset_ref(hits, imesh, [sd.meshes[0], v1], [None, v2]),
                 "second snapshot")
    # only the offset, and nothing at all
    only = ctx.render_aov_deform(W, H, device_out=False)[3]
    n = W * H
    buf = np.zeros((n, 4), F)
    assert ctx.L.prt_render_aov_deform(ctx.h, W, H, 0, None, None, None, buf.ctypes.data, 0) == 0
    assert np.array_equal(_bits(buf), _bits(only))
    assert ctx.L.prt_render_aov_deform(ctx.h, W, H, 0, None, None, None, None, 0) == 0
    gpu_scene(ctx, sd, W, H)  # prt_set_meshes
    assert not ctx.render_aov_deform(W, H)[3].any()


# ---- prt_reproject_deform on the deforming sequence (deform_ref: mesh 1 at frame k is mesh_at(k))
SHAPES = {"own_96x72": (96, 72), "own_70x45": (70, 45)}


def _view(ctx, shape, k):
    """Frame k of the sequence at a shape: the GPU's own 2-spp frame (depth 4, frame_index k), AOVs, ids, offset and
    hits; the mesh is snapshotted after every frame.  Frame k needs frame k - 1's geometry as the snapshot: where the
    context does not hold it, the scene is loaded at frame 0, updated to frame k - 1 and snapshotted first."""
    import prt
    if (shape, k) not in _views:
        sd = df.scene_at(0)[0]
        W, H = SHAPES[shape]
        if k == 0 or _state.get("at") != (shape, k - 1):
            gpu_scene(ctx, sd, W, H)
            if k > 1:
                ctx.update_mesh(1, df.mesh_at(k - 1))
            if k:
                ctx.snapshot_mesh(1)
        if k:
            ctx.update_mesh(1, df.mesh_at(k))
        cam = prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H))
        ctx.set_camera(cam)
        ctx.reset_accumulation(full=True)
        avg, _, _ = ctx.render(W, H, 2, 4, frame_index=k)
        alb, nd, ids, off = ctx.render_aov_deform(W, H)
        hits, _ = ctx.trace_primary(W, H)
        ctx.reset_accumulation(full=True)
        ctx.snapshot_mesh(1)
        _state["at"] = (shape, k)
        _views[(shape, k)] = dict(cam=cam, color=avg, alb=alb, nd=nd, ids=ids, off=off, hits=hits, xf=df.transforms(sd),
                                  sd=df.scene_at(k)[0], W=W, H=H)
    return _views[(shape, k)]


def _seq(ctx, shape, upto):
    for k in range(upto + 1):
        _view(ctx, shape, k)
    return [_views[(shape, k)] for k in range(upto + 1)]


def _ref_chain(ctx, shape, upto, **par):
    vs = _seq(ctx, shape, upto)
    outs = _chains.setdefault((shape, tuple(sorted(par.items()))), [])
    while len(outs) <= upto:
        k = len(outs)
        outs.append(df.step(vs, k, outs[-1] if k else None, vs[0]["W"], vs[0]["H"], **par))
    return outs


def _dev_step(ctx, v, u, hist, with_ids=True, **par):
    import prt
    tp = prt.temporal_defaults(**par)
    if u is None:
        return ctx.reproject_deform(v["color"], v["nd"], v["ids"], v["cam"], width=v["W"], height=v["H"], params=tp)
    return ctx.reproject_deform(v["color"], v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"],
                                u["ids"] if with_ids else None, prt.instance_motion(v["xf"], u["xf"]), hist[1],
                                v["off"], u["xf"], width=v["W"], height=v["H"], params=tp)


def _assert_equal(got, ref, what):
    _assert_rows(got[0], ref[0], what + ": colour")
    _assert_rows(got[1], ref[1], what + ": moments")
    assert np.array_equal(got[2], dr.pack_rgb8(ref[0])), what


def test_sequence_offsets_match_reference(ctx):
    """Every frame's offset output of the sequence equals offset_ref of the device's hits against the previous frame's
    geometry."""
    vs = _seq(ctx, "own_96x72", 3)
    assert not vs[0]["off"].any()
    for k in (1, 2, 3):
        ref = df.offset_ref(vs[k]["hits"], df.instance_mesh(vs[k]["sd"]), vs[k]["sd"].meshes,
                            [None, vs[k - 1]["sd"].meshes[1]])
        _assert_rows(vs[k]["off"], ref, f"frame {k}")
        assert np.any(ref[:, 3] == 1)


@pytest.mark.parametrize("par", [dict(), dict(clamp_k=1.5)], ids=["defaults", "clamp"])
@pytest.mark.parametrize("with_ids", [True, False], ids=["ids", "noids"])
@pytest.mark.parametrize("shape,k", [("own_96x72", 1), ("own_96x72", 3), ("own_70x45", 2)])
def test_step_matches_reference_bitwise(ctx, shape, k, with_ids, par):
    """One device step, the history being the reference's output of the step before: colour, history length, moments,
    variance and packed pixels equal the reference's, and the deforming instance's pixels do follow."""
    vs = _seq(ctx, shape, k)
    v, u = vs[k], vs[k - 1]
    hist = _ref_chain(ctx, shape, k - 1, **par)[-1]
    info, binfo = {}, {}
    ref = df.reproject_deform(v["color"], v["nd"], v["ids"], v["cam"], v["W"], v["H"], hist[0], u["nd"], u["cam"],
                              u["ids"] if with_ids else None, mr.identity(len(v["xf"])), hist[1], v["off"], u["xf"],
                              info=info, **par)
    vr.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], v["W"], v["H"], hist[0], u["nd"], u["cam"],
                         u["ids"] if with_ids else None, mr.identity(len(v["xf"])), hist[1], info=binfo, **par)
    mover = v["ids"] == df.MOVER
    print(f"{shape} step {k}: history on {info['has_history'][mover].sum()} of {mover.sum()} deforming pixels "
          f"(plain pass {binfo['has_history'][mover].sum()})")
    assert info["has_history"][mover].any() and (info["hit"] & ~info["has_history"]).any()
    assert not np.array_equal(info["has_history"], binfo["has_history"])
    _assert_equal(_dev_step(ctx, v, u, hist, with_ids, **par), ref, f"{shape} step {k} {par}")


def test_chain_on_the_device(ctx):
    """Eight frames with the device's own outputs as the next history equal the reference's chain."""
    ref = _ref_chain(ctx, "own_96x72", df.FRAMES - 1)
    vs = _seq(ctx, "own_96x72", df.FRAMES - 1)
    got = None
    for k, v in enumerate(vs):
        got = _dev_step(ctx, v, vs[k - 1] if k else None, got)
    _assert_equal(got, ref[-1], "chain")
    assert got[0][:, 3].max() > df.FRAMES - 1e-3


@pytest.mark.parametrize("shape", list(SHAPES))
def test_null_and_zero_offset_equal_prt_reproject_moments(ctx, shape):
    """offset and prev_transforms NULL: prt_reproject_moments' outputs bit for bit, also when a history starts; an
    offset image whose xyz are +0 (w = 1 on every hit pixel) gives them too."""
    import prt
    vs = _seq(ctx, shape, 2)
    v, u = vs[2], vs[1]
    W, H = v["W"], v["H"]
    hist = _ref_chain(ctx, shape, 1)[-1]
    mo = prt.instance_motion(v["xf"], u["xf"])
    args = (v["color"], v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"], u["ids"], mo, hist[1])
    want = ctx.reproject_moments(*args, width=W, height=H)
    assert np.any(want[0][:, 3] > 1)
    zero = np.zeros((W * H, 4), F)
    zero[v["ids"] != mr.MISS, 3] = 1
    for got in (ctx.reproject_deform(*args, width=W, height=H),
                ctx.reproject_deform(*args, zero, u["xf"], width=W, height=H)):
        for a, b in zip(got, want):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    moved = _dev_step(ctx, v, u, hist)
    assert not np.array_equal(_bits(moved[0]), _bits(want[0]))
    first = ctx.reproject_deform(*args[:4], width=W, height=H)
    for a, b in zip(first, ctx.reproject_moments(*args[:4], width=W, height=H)):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- plumbing
def _dev(stream, *arrays):
    import torch
    with torch.cuda.stream(stream):
        return [torch.from_numpy(np.array(a).view(np.int32) if a.dtype == np.uint32 else np.array(a)).to("cuda")
                for a in arrays]


def test_device_pointers(ctx):
    """prt_render_aov_deform and prt_reproject_deform with device-pointer images on a torch stream (PRT_OUT_DEVICE, no
    host wait) give the host path's images; the matrices and the previous transforms are host arrays changed right
    after each call: they were copied.  An offset that is an output is refused."""
    import torch
    import prt
    vs = _seq(ctx, "own_96x72", 3)
    v, u = vs[3], vs[2]
    hist = _ref_chain(ctx, "own_96x72", 2)[-1]
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    mo = prt.instance_motion(v["xf"], u["xf"])
    want = _dev_step(ctx, v, u, hist)
    want_aov = ctx.render_aov_deform(W, H)  # of whatever frame the context holds: only the two paths are compared
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        col, nd, ids, h, hnd, hids, hm, off = _dev(stream, v["color"], v["nd"], v["ids"], hist[0], u["nd"], u["ids"],
                                                   hist[1], v["off"])
        with torch.cuda.stream(stream):
            o, m, a_alb, a_nd, a_off = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(5))
            r8, a_ids = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        mm, px = mo.copy(), np.array(u["xf"], F).reshape(-1, 16).copy()
        ctx.reproject_deform(col.data_ptr(), nd.data_ptr(), ids.data_ptr(), v["cam"], h.data_ptr(), hnd.data_ptr(),
                             u["cam"], hids.data_ptr(), mm, hm.data_ptr(), off.data_ptr(), px, width=W, height=H,
                             device_out=True, out=o.data_ptr(), moments=m.data_ptr(), rgb8=r8.data_ptr())
        mm[:] = np.nan
        px[:] = np.nan
        with pytest.raises(prt.PrtError, match="prt error -1"):
            ctx.reproject_deform(col.data_ptr(), nd.data_ptr(), ids.data_ptr(), v["cam"], h.data_ptr(), hnd.data_ptr(),
                                 u["cam"], hids.data_ptr(), mo, hm.data_ptr(), off.data_ptr(), u["xf"], width=W,
                                 height=H, device_out=True, out=off.data_ptr(), moments=m.data_ptr())
        ctx.render_aov_deform(W, H, device_out=True, albedo=a_alb.data_ptr(), normal_depth=a_nd.data_ptr(),
                              instance=a_ids.data_ptr(), offset=a_off.data_ptr())
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    assert np.array_equal(_bits(off.cpu().numpy()), _bits(v["off"]))  # the inputs are left alone
    assert np.array_equal(_bits(o.cpu().numpy()), _bits(want[0]))
    assert np.array_equal(_bits(m.cpu().numpy()), _bits(want[1]))
    assert np.array_equal(r8.cpu().numpy().view(np.uint32), want[2])
    for t, w in zip((a_alb, a_nd, a_ids, a_off), want_aov):
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(w).view(np.uint32).reshape(-1))


def test_no_side_effect(ctx):
    """The three calls between two accumulating renders: the accumulation blob and the ray totals are the same before
    and after, and the second render equals the one made without the calls."""
    vs = _seq(ctx, "own_96x72", 1)
    v, u = vs[1], vs[0]
    hist = _ref_chain(ctx, "own_96x72", 0)[-1]
    W, H = v["W"], v["H"]
    _disturb()
    ctx.set_camera(v["cam"])
    try:
        ctx.reset_accumulation(full=True)
        ctx.render(W, H, 2, 4, frame_index=0)
        want, want8, _ = ctx.render(W, H, 2, 4, frame_index=1)
        ctx.reset_accumulation(full=True)
        ctx.render(W, H, 2, 4, frame_index=0)
        blob, totals = ctx.save_accumulation(), ctx.ray_totals()
        ctx.snapshot_mesh(1)
        ctx.render_aov_deform(W, H)
        out = _dev_step(ctx, v, u, hist)[0]
        assert np.any(out[:, 3] > 1)
        assert ctx.save_accumulation() == blob and ctx.ray_totals() == totals
        got, got8, _ = ctx.render(W, H, 2, 4, frame_index=1)
    finally:
        ctx.reset_accumulation(full=True)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got8, want8)


def _loop_group():
    """_loop's frames on a local group of two members on one device, with host outputs."""
    import prt
    sd, W, H = df.scene()
    c = prt.Context(group=[0, 0])
    try:
        gpu_scene(c, sd, W, H)
        avg, nd, off = [], [], []
        for k in range(3):
            if k:
                c.update_mesh(1, df.mesh_at(k))
            c.reset_accumulation(full=True)
            avg.append(c.render(W, H, 2, 4, frame_index=k)[0])
            _, g, _, o = c.render_aov_deform(W, H)
            nd.append(g)
            off.append(o)
            c.snapshot_mesh(1)
        return avg + nd + off
    finally:
        c.close()


def _loop(flights):
    """Three frames of the sequence in the loop's order -- update, render, AOVs with the offset, snapshot -- with
    device outputs on one stream and `flights` frames in flight."""
    import torch
    import prt
    sd, W, H = df.scene()
    n = W * H
    stream = torch.cuda.Stream()
    c = prt.Context(0)
    try:
        c.set_stream(stream.cuda_stream)
        gpu_scene(c, sd, W, H)
        c.set_frames_in_flight(flights)
        with torch.cuda.stream(stream):
            avg = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
            off = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
            nd = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
        for k in range(3):
            if k:
                c.update_mesh(1, df.mesh_at(k))
            c.reset_accumulation(full=True)
            c.render(W, H, 2, 4, frame_index=k, avg=avg[k].data_ptr(), device_out=True, stats=False)
            c.render_aov_deform(W, H, device_out=True, normal_depth=nd[k].data_ptr(), offset=off[k].data_ptr())
            c.snapshot_mesh(1)
        stream.synchronize()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in avg + nd + off]
    finally:
        c.close()


def test_frames_in_flight_and_group():
    """prt_set_frames_in_flight(2): update, render and snapshot in the loop's order give the same images as one frame
    at a time; a local group of two members on one device gives them too (the snapshot reaches every member, the
    passes run on member 0)."""
    one, two, grp = _loop(1), _loop(2), _loop_group()
    for a, b, g in zip(one, two, grp):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(g))
    assert not one[6].any() and np.any(one[7][:, 3] == 1) and np.any(one[8][:, :3] != 0)


def test_argument_checks(ctx):
    """The stated statuses on a live context; a refused call leaves the outputs untouched."""
    import prt
    L = ctx.L
    fresh = prt.Context(0)
    try:
        assert L.prt_snapshot_mesh(fresh.h, 0) == -5  # no meshes
    finally:
        fresh.close()
    vs = _seq(ctx, "own_96x72", 1)
    v, u = vs[1], vs[0]
    hist = _ref_chain(ctx, "own_96x72", 0)[-1]
    W, H, n = v["W"], v["H"], v["W"] * v["H"]
    _disturb()
    assert L.prt_snapshot_mesh(ctx.h, -1) == -1 and L.prt_snapshot_mesh(ctx.h, 2) == -1
    assert L.prt_snapshot_mesh(ctx.h, 0) == 0 and L.prt_snapshot_mesh(ctx.h, 1) == 0
    mo = prt.instance_motion(v["xf"], u["xf"])
    args = (v["color"], v["nd"], v["ids"], v["cam"], hist[0], u["nd"], u["cam"], u["ids"], mo, hist[1])
    with pytest.raises(prt.PrtError, match="prt error -1"):
        ctx.reproject_deform(*args, v["off"], None, width=W, height=H)
    with pytest.raises(prt.PrtError, match="prt error -1"):
        ctx.reproject_deform(*args, None, u["xf"], width=W, height=H)
    with pytest.raises(prt.PrtError, match="prt error -1"):  # an offset without a history
        ctx.reproject_deform(*args[:4], offset=v["off"], prev_transforms=u["xf"], width=W, height=H)
    out = ctx.reproject_deform(*args, v["off"], u["xf"], width=W, height=H)[0]
    assert np.any(out[:, 3] > 1)


# ---- the Renderer mirror
def test_renderer_track_model():
    """Renderer.TrackModel + UpdateModel + TickTemporalVariance(deform=True) over 4 frames equals the reference chain on
    the renderer's own frames; TickTemporalVariance() without deform is unchanged: prt_reproject_moments' chain."""
    import prt
    sd, W, H = df.scene()
    tp, fp = prt.temporal_defaults(clamp_k=1.5), prt.denoise_variance_defaults(iterations=3)
    imesh = df.instance_mesh(sd)
    for follow in (True, False):
        R = prt.Renderer(prt.Scene.from_data(sd), prt.Camera(sd.cam_pos, sd.cam_target, F(W) / F(H)), W, H)
        try:
            R.TrackModel(1)
            seq = [sd.meshes[1]] + [df.mesh_at(k) for k in (1, 2, 3)]
            hist = u = None
            for k in range(4):
                if k:
                    R.UpdateModel(1, seq[k])
                hits, _ = R.ctx.trace_primary(W, H)
                off = df.offset_ref(hits, imesh, [sd.meshes[0], seq[k]], [None, seq[max(k - 1, 0)]])
                flt, scr, out = R.TickTemporalVariance(tp, fp, deform=follow)
                alb, nd, ids = R.ctx.render_aov_ids(W, H)
                v = dict(cam=R.camera, color=R.average, nd=nd, ids=ids, xf=df.transforms(sd), off=off)
                if follow:
                    ref = df.step([u, v] if u else [v], 1 if u else 0, hist, W, H, clamp_k=1.5)
                else:
                    ref = vr.step([u, v] if u else [v], 1 if u else 0, hist, W, H, clamp_k=1.5)
                _assert_rows(out, ref[0], f"deform={follow} frame {k}")
                want = vr.denoise_variance(ref[0], ref[1], alb, nd, W, H, **dict(vr.FILTER_DEFAULTS, iterations=3))[0]
                assert np.array_equal(_bits(flt), _bits(want)) and np.array_equal(scr, dr.pack_rgb8(want)), k
                hist, u = ref, v
            assert out[:, 3].max() > 4 - 1e-3
        finally:
            R.ctx.close()


# ---- quality on the device's own frames
def test_quality_on_the_device(ctx, oracle_mod):
    """tests/test_deform_ref.py::test_quality_and_coverage on the GPU's own frames, both passes chained on the device,
    against the oracle's 1024-spp frame of the last frame's geometry: deform_ref.check_quality's bounds hold."""
    import prt
    vs = _seq(ctx, "own_96x72", df.FRAMES - 1)
    W, H = vs[0]["W"], vs[0]["H"]
    new = base = None
    for k, v in enumerate(vs):
        u = vs[k - 1] if k else None
        new = _dev_step(ctx, v, u, new)
        args = (base[0], u["nd"], u["cam"], u["ids"], prt.instance_motion(v["xf"], u["xf"]), base[1]) if k else ()
        base = ctx.reproject_moments(v["color"], v["nd"], v["ids"], v["cam"], *args, width=W, height=H)
    f = df.figures(vs, base[0], new[0], df.oracle_converged())
    print("on the device: " + ", ".join(f"{k} {x:.4f}" for k, x in f.items())
          + f", ratio {f['rmse_new'] / f['rmse_base']:.4f}")
    df.check_quality(f)
