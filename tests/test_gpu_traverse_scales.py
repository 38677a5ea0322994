"""Small geometry seen from far away and geometry at large coordinates through the HIP traversals and the device
builders (tests/far_scenes.py; the CPU side, with the measured counts, is tests/test_traverse_scales.py).

At these scales the Node8 child test absorbs the quantised byte and its raw slab mask passes the inverted box of
unoccupied child slots: a count of 0 in the persistent kernels' triangle step, an instance-slot entry of 0xFFFFFFFF in
the instance BVH.  A node visit hands on occupied slots only (prt_node8.h), and the box tests stay conservative, so
every result here is np.array_equal to a reference: the numpy brute force over all triangles (identity instances)
or the oracle (instances, primary rays, frames) -- every field, every ray, every pixel, no tolerated fraction."""
import numpy as np
import pytest

import degenerate as dg
import far_scenes as fs
import oracle
import prt
from helpers import gpu_scene
from prt import _lib

pytestmark = pytest.mark.gpu

FIELDS = ("t", "u", "v", "prim", "inst")
BUILDERS = {"host_sah": _lib.BUILDER_HOST_SAH, "gpu_lbvh": _lib.BUILDER_GPU_LBVH, "host_sbvh": _lib.BUILDER_HOST_SBVH,
            "gpu_ploc": _lib.BUILDER_GPU_PLOC}
NAMES = sorted(fs.PLACEMENTS) + ["P"]
W, H, SPP, BOUNCES = 32, 24, 2, 3

_refs = {}


def _tmax_pair(t):
    hit = t < dg.FAR
    return hit, {"at": np.where(hit, t, dg.FAR).astype(np.float32),
                 "past": np.where(hit, np.nextafter(t, np.float32(np.inf)), dg.FAR).astype(np.float32)}


def _freeze(ref):
    for a in ref["hits"] + tuple(ref["tmax"].values()):
        a.setflags(write=False)
    return ref


def _ref(name):
    """The brute force's answers for one placement, computed once and left unchanged: the hit records, the same with
    tmax at and one ulp past the hit, and the any-hit answers of both."""
    if name not in _refs:
        tris = fs.placement_tris(name)
        O, D = fs.placement_rays(name)
        hits = dg.brute_force(tris, O, D)[:5]
        hit, tmax = _tmax_pair(hits[0])
        bf = {k: dg.brute_force(tris, O, D, tmax=tm) for k, tm in tmax.items()}
        _refs[name] = _freeze({"sd": fs.placement_scene(name), "O": O, "D": D, "hits": hits, "hit": hit, "tmax": tmax,
                               "hits_tmax": {k: v[:5] for k, v in bf.items()},
                               "occ": {k: (v[5] > 0).astype(np.int32) for k, v in bf.items()}})
    return _refs[name]


def _field_ref(n, dist):
    key = ("field", n, dist)
    if key not in _refs:
        sd = fs.field(n)
        osc = oracle.OracleScene(sd)
        O, D = fs.field_rays(n, dist)
        hits = osc.intersect(O, D)
        hit, tmax = _tmax_pair(hits[0])
        _refs[key] = _freeze({"sd": sd, "O": O, "D": D, "hits": hits, "hit": hit, "tmax": tmax,
                              "hits_tmax": {k: osc.intersect(O, D, tm) for k, tm in tmax.items()},
                              "occ": {k: osc.occluded(O, D, tm) for k, tm in tmax.items()}})
    return _refs[key]


def _assert_hits(g, want, what):
    for k, f in enumerate(FIELDS):
        assert np.array_equal(g[f], want[k]), (what, f, int((g[f] != want[k]).sum()))


def _check_queries(ctx, ref, min_hits):
    O, D, hit = ref["O"], ref["D"], ref["hit"]
    assert O.shape[0] % 64 != 0 and hit.sum() >= min_hits
    _assert_hits(ctx.intersect(O, D), ref["hits"], "all")
    for name, s in fs.SLICES.items():
        _assert_hits(ctx.intersect(O[s], D[s]), [a[s] for a in ref["hits"]], name)
    for k in ("at", "past"):
        tm = ref["tmax"][k]
        occ = ctx.occluded(O, D, tm)
        assert np.array_equal(occ != 0, ref["occ"][k] != 0), (k, int(((occ != 0) != (ref["occ"][k] != 0)).sum()))
        assert occ[hit].astype(bool).sum() == (0 if k == "at" else hit.sum()) and not occ[~hit].any(), k
        _assert_hits(ctx.intersect(O, D, tm), ref["hits_tmax"][k], "tmax " + k)
    occ = ctx.occluded(O, D, np.full(O.shape[0], dg.FAR, np.float32))
    assert np.array_equal(occ != 0, hit)
    _, st = ctx.trace_primary(16, 8)  # the context's overflow count is cumulative; the wrapper raises on it too
    assert st.stack_overflows == 0


@pytest.mark.parametrize("builder", sorted(BUILDERS))
@pytest.mark.parametrize("name", NAMES)
def test_queries_equal_the_brute_force(gpu_ctx, name, builder):
    """prt_intersect / prt_occluded (blas_traverse8 in the query kernels) on every placement, each BLAS builder."""
    ref = _ref(name)
    try:
        gpu_ctx.set_bvh_builder(BUILDERS[builder])
        gpu_scene(gpu_ctx, ref["sd"], W, H)
        assert gpu_ctx.scene_info().builder == BUILDERS[builder]
        _check_queries(gpu_ctx, ref, 0 if name == "P" else 3000)
        if name == "P":
            assert not ref["hit"].any()
    finally:
        gpu_ctx.set_bvh_builder(_lib.BUILDER_HOST_SAH)


@pytest.mark.parametrize("dist", fs.FIELD_DISTS)
@pytest.mark.parametrize("n", [65, 300])
def test_instance_bvh_queries_equal_the_oracle(gpu_ctx, n, dist):
    """tlas_traverse8 over field(n) from 1e6 and 1e7 units: the raw mask would look up 0xFFFFFFFF there."""
    ref = _field_ref(n, dist)
    gpu_scene(gpu_ctx, ref["sd"], W, H)
    assert gpu_ctx.scene_info().tlas_depth > 0
    _check_queries(gpu_ctx, ref, 100)
    assert len(np.unique(ref["hits"][4][ref["hit"]])) >= 20


# ---- cameras

def _device_camera(ctx, sd, tele):
    cam = prt.Camera(sd.cam_pos, sd.cam_target, np.float32(W) / np.float32(H))
    if tele is not None:
        for k, v in tele.items():
            getattr(cam.desc, k)[:] = [float(x) for x in v]
    ctx.set_camera(cam)
    ctx.reset_accumulation(full=True)


def _oracle_scene(sd, tele):
    osc = oracle.OracleScene(sd, W, H)
    if tele is not None:
        osc.L.orc_set_camera(osc.h, *[tele[k].ctypes.data for k in ("pos", "top_left", "top_right", "bottom_left")])
    return osc


VIEWS = {
    "C": lambda: (fs.placement_scene("C"), fs.placement_telephoto("C")),
    "D": lambda: (fs.placement_scene("D"), fs.placement_telephoto("D")),
    "P": lambda: (fs.placement_scene("P"), None),
    "field300": lambda: (fs.field(300), fs.field_telephoto(1e6)),
    "blocker": lambda: (fs.blocker(), None),
    "blocker_open": lambda: (fs.blocker(with_far=False), None),
}
FLAGS = {"P": _lib.FLAGS_DEFAULT & ~_lib.FLAG_AA}
_views, _frames, _primary = {}, {}, {}


def _view(name):
    if name not in _views:
        sd, tele = VIEWS[name]()
        _views[name] = (sd, tele, _oracle_scene(sd, tele))
    return _views[name]


def _oracle_frame(name):
    if name not in _frames:
        _, _, osc = _view(name)
        a, r, _, st = osc.render(W, H, spp=SPP, bounces=BOUNCES, flags=FLAGS.get(name, oracle.DEFAULT_FLAGS))
        _frames[name] = {"avg": a, "rgb8": r, "segments": int(st.segments), "shadow_rays": int(st.shadow_rays)}
        a.setflags(write=False)
        r.setflags(write=False)
    return _frames[name]


@pytest.mark.parametrize("name", ["C", "D", "field300"])
def test_trace_primary_through_a_telephoto_camera(gpu_ctx, name):
    """k_primary_hits: every primary ray crosses the small nodes; every field of every pixel equals the oracle's."""
    sd, tele, osc = _view(name)
    gpu_scene(gpu_ctx, sd, W, H)
    _device_camera(gpu_ctx, sd, tele)
    hits, st = gpu_ctx.trace_primary(W, H)
    want = osc.primary_hits(W, H)
    _assert_hits(hits, want, "primary")
    assert (want[0] < dg.FAR).mean() >= (0.5 if name != "field300" else 0.1)
    assert st.segments == W * H and st.stack_overflows == 0


def _render_equals_oracle(ctx, name):
    sd, tele, _ = _view(name)
    want = _oracle_frame(name)
    gpu_scene(ctx, sd, W, H)
    _device_camera(ctx, sd, tele)
    a, r, st = ctx.render(W, H, SPP, BOUNCES, flags=FLAGS.get(name, _lib.FLAGS_DEFAULT))
    assert (st.segments, st.shadow_rays) == (want["segments"], want["shadow_rays"])
    assert np.array_equal(a[:, :3], want["avg"][:, :3]), int((a[:, :3] != want["avg"][:, :3]).any(axis=1).sum())
    assert np.array_equal(r, want["rgb8"])
    assert st.stack_overflows == 0
    return a, st


@pytest.mark.parametrize("tail,merge", [("1", "1"), ("0", "0"), ("1", "0"), ("0", "1")])
@pytest.mark.parametrize("name", ["C", "blocker"])
def test_frames_tail_and_merge(gpu_ctx, monkeypatch, name, tail, merge):
    """A frame (2 spp, 3 bounces) through the persistent kernels with the cooperative tail and the merged pipeline off
    and on.  C: every primary ray meets the condition in closest-hit mode; blocker: every shadow ray towards the far
    light does in any-hit mode."""
    monkeypatch.setenv("PRT_TAIL", tail)
    monkeypatch.setenv("PRT_MERGE", merge)
    _, st = _render_equals_oracle(gpu_ctx, name)
    assert st.segments >= W * H
    if name == "blocker":
        assert st.shadow_rays > 0


@pytest.mark.parametrize("name", ["D", "P", "field300"])
def test_frames(gpu_ctx, name):
    """D: large coordinates; P: the point at the origin through the look-at camera, AA off (the centre ray travels
    through it); field300: the instance BVH of the persistent kernels (next_node's instance-slot lookup)."""
    _render_equals_oracle(gpu_ctx, name)


@pytest.mark.parametrize("builder", ["gpu_lbvh", "host_sbvh"])
def test_frames_other_builders(gpu_ctx, builder):
    try:
        gpu_ctx.set_bvh_builder(BUILDERS[builder])
        _render_equals_oracle(gpu_ctx, "C")
    finally:
        gpu_ctx.set_bvh_builder(_lib.BUILDER_HOST_SAH)


def test_blocker_is_not_vacuous(gpu_ctx):
    """The far patch decides the frame: shadow rays are traced, and the same frame without it differs."""
    a, st = _render_equals_oracle(gpu_ctx, "blocker")
    b, st2 = _render_equals_oracle(gpu_ctx, "blocker_open")
    assert st.shadow_rays > 0 and st2.shadow_rays > 0
    assert not np.array_equal(a[:, :3], b[:, :3])
    assert (b[:, :3].astype(np.float64).sum() > a[:, :3].astype(np.float64).sum())  # the far light reaches the patch
