"""Degenerate geometry and exact ties through the HIP traversal and the device builders (tests/degenerate.py; the
CPU side is tests/test_degenerate_ref.py): duplicate and zero-area triangles, coincident centroids, meshes of 1 to 9
triangles, coincident / mirrored / non-uniformly scaled instances, rays with exact signed-zero direction components
through shared vertices and edges, tmax at the hit distance itself.

The hit rule (prt_traverse.h) is implemented in the query kernels' leaf update, the persistent kernels' leaf step,
the cooperative tail's team merge and the oracle's better(); these inputs tie on thousands of rays, so every
comparison here is np.array_equal against the oracle over every ray or pixel -- no tolerated fraction."""
import numpy as np
import pytest

import degenerate as dg
import oracle
from helpers import gpu_scene
from prt import _lib

pytestmark = pytest.mark.gpu

FIELDS = ("t", "u", "v", "prim", "inst")
BUILDERS = {"host_sah": _lib.BUILDER_HOST_SAH, "gpu_lbvh": _lib.BUILDER_GPU_LBVH, "host_sbvh": _lib.BUILDER_HOST_SBVH,
            "gpu_ploc": _lib.BUILDER_GPU_PLOC}
SCENES = {"soup1": dg.soup1, "soup4": dg.soup4, "tiny": dg.tiny, "coincident70": dg.coincident70}
W, H = 96, 64

_refs = {}


def _ref(name):
    """The oracle's answers for one scene, computed once and left unchanged: hit records of edge_rays(1), of the
    same rays with tmax at and one ulp past the hit, and the any-hit results of both."""
    if name not in _refs:
        sd = SCENES[name]()
        osc = oracle.OracleScene(sd)
        O, D, slices = dg.edge_rays(1)
        hits = osc.intersect(O, D)
        t = hits[0]
        hit = t < dg.FAR
        at = np.where(hit, t, dg.FAR).astype(np.float32)
        past = np.where(hit, np.nextafter(t, np.float32(np.inf)), dg.FAR).astype(np.float32)
        _refs[name] = {"sd": sd, "osc": osc, "O": O, "D": D, "slices": slices, "hits": hits, "hit": hit,
                       "tmax": {"at": at, "past": past},
                       "hits_tmax": {k: osc.intersect(O, D, tm) for k, tm in (("at", at), ("past", past))},
                       "occ": {k: osc.occluded(O, D, tm) for k, tm in (("at", at), ("past", past))}}
        for a in _refs[name]["hits"] + (at, past):
            a.setflags(write=False)
    return _refs[name]


def _assert_hits(g, want, what):
    for k, f in enumerate(FIELDS):
        assert np.array_equal(g[f], want[k]), (what, f, int((g[f] != want[k]).sum()))


def _check_queries(ctx, ref):
    """prt_intersect / prt_occluded against the oracle on the full ray set (no multiple of 64), on 1-, 63- and
    65-ray batches, and with tmax at / one ulp past the hit; the triangle count; no traversal stack overflow."""
    O, D, hit = ref["O"], ref["D"], ref["hit"]
    assert hit.sum() >= 100
    _assert_hits(ctx.intersect(O, D), ref["hits"], "all")
    for name, s in ref["slices"].items():
        _assert_hits(ctx.intersect(O[s], D[s]), [a[s] for a in ref["hits"]], name)
    for k in ("at", "past"):
        tm = ref["tmax"][k]
        occ = ctx.occluded(O, D, tm)
        assert np.array_equal(occ, ref["occ"][k]), (k, int((occ != ref["occ"][k]).sum()))
        # a closest hit needs t < tmax: no hit ray is occluded at tmax = t, every one at nextafter(t)
        assert occ[hit].sum() == (0 if k == "at" else hit.sum()) and not occ[~hit].any(), k
        _assert_hits(ctx.intersect(O, D, tm), ref["hits_tmax"][k], "tmax " + k)
    assert ctx.scene_info().triangles == sum(m.tri_count for m in ref["sd"].meshes)
    _, st = ctx.trace_primary(16, 8)  # the context's overflow count is cumulative; the wrapper raises on it too
    assert st.stack_overflows == 0


@pytest.mark.parametrize("builder", sorted(BUILDERS))
@pytest.mark.parametrize("scene", ["soup1", "tiny"])
def test_queries_every_builder(gpu_ctx, scene, builder):
    """The soup (duplicates, a pile of one Morton code, zero-area triangles, a zero-thickness lattice) and the five
    meshes of 1, 2, 7, 8 and 9 triangles, built by each BLAS builder: hit records equal the oracle's for every ray."""
    ref = _ref(scene)
    try:
        gpu_ctx.set_bvh_builder(BUILDERS[builder])
        gpu_scene(gpu_ctx, ref["sd"], W, H)
        assert gpu_ctx.scene_info().builder == BUILDERS[builder]
        _check_queries(gpu_ctx, ref)
    finally:
        gpu_ctx.set_bvh_builder(_lib.BUILDER_HOST_SAH)


@pytest.mark.parametrize("case", ["soup4_linear", "soup4_tlas", "coincident70"])
def test_instance_ties(gpu_ctx, monkeypatch, case):
    """Ties between instances: soup4's instance 1 coincides with instance 0 and never wins, through the linear
    instance list and through the instance BVH (PRT_TLAS=1); 70 coincident instances (the instance BVH by
    itself) tie 70 ways on every hit, which reports instance 0."""
    scene = "coincident70" if case == "coincident70" else "soup4"
    ref = _ref(scene)
    if case == "soup4_tlas":
        monkeypatch.setenv("PRT_TLAS", "1")
    try:
        gpu_scene(gpu_ctx, ref["sd"], W, H)
        assert (gpu_ctx.scene_info().tlas_depth > 0) == (case != "soup4_linear")
        _check_queries(gpu_ctx, ref)
        g = gpu_ctx.intersect(ref["O"], ref["D"])
        ghit = g["t"] < dg.FAR
        if scene == "soup4":
            assert not (g["inst"][ghit] == 1).any() and {0, 2, 3} <= set(np.unique(g["inst"][ghit]))
        else:
            assert ghit.sum() >= 1000 and not g["inst"].any()
    finally:
        if case == "soup4_tlas":
            monkeypatch.delenv("PRT_TLAS")
            gpu_scene(gpu_ctx, ref["sd"], W, H)  # instances re-packed without the instance BVH for later tests
            assert gpu_ctx.scene_info().tlas_depth == 0


def test_primary_hits_soup4(gpu_ctx):
    """trace_primary on soup4 against OracleScene.primary_hits: every field of every pixel."""
    ref = _ref("soup4")
    gpu_scene(gpu_ctx, ref["sd"], W, H)
    hits, st = gpu_ctx.trace_primary(W, H)
    want = oracle.OracleScene(ref["sd"], W, H).primary_hits(W, H)
    _assert_hits(hits, want, "primary")
    hit = want[0] < dg.FAR
    assert hit.mean() >= 0.5 and not (hits["inst"][hit] == 1).any()
    assert st.segments == W * H


_frame = {}


def _oracle_frame():
    if not _frame:
        a, r, _, st = oracle.OracleScene(dg.soup4(), W, H).render(W, H, spp=2, bounces=3)
        _frame.update(avg=a, rgb8=r, segments=st.segments, shadow_rays=st.shadow_rays)
    return _frame


@pytest.mark.parametrize("tail,merge,builder", [("0", "0", "host_sah"), ("1", "0", "host_sah"), ("0", "1", "host_sah"),
                                                ("1", "1", "host_sah"), ("1", "1", "gpu_lbvh")])
def test_frames_soup4(gpu_ctx, monkeypatch, tail, merge, builder):
    """A frame of soup4 (2 spp, 3 bounces) through the persistent kernels, with the cooperative tail off and on and
    the merged pipeline off and on, and once on the device LBVH tree: on the doubled mesh every shaded hit and every
    shadow ray meets a tie, and the texture coordinates differ between coincident triangles, so the image, RGB8,
    segments and shadow rays equal the oracle's only if every tie goes the oracle's way."""
    want = _oracle_frame()
    monkeypatch.setenv("PRT_TAIL", tail)
    monkeypatch.setenv("PRT_MERGE", merge)
    try:
        gpu_ctx.set_bvh_builder(BUILDERS[builder])
        gpu_scene(gpu_ctx, dg.soup4(), W, H)
        a, r, st = gpu_ctx.render(W, H, 2, 3)
        assert (st.segments, st.shadow_rays) == (want["segments"], want["shadow_rays"])
        assert np.array_equal(a[:, :3], want["avg"][:, :3]), int((a[:, :3] != want["avg"][:, :3]).any(axis=1).sum())
        assert np.array_equal(r, want["rgb8"])
        assert st.stack_overflows == 0
    finally:
        gpu_ctx.set_bvh_builder(_lib.BUILDER_HOST_SAH)
