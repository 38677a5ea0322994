"""Degenerate geometry and exact ties on the CPU (tests/degenerate.py): the oracle against a numpy brute force that
restates the hit rule on its own, the conditions the inputs have to meet to be worth tracing, and the host builders'
invariants on these meshes.  tests/test_gpu_degenerate.py runs the same inputs through the HIP traversal and the
device builders.

Measured on the soup (651 triangles) with edge_rays(1) (4,746 rays; 4,227 hit), from the brute force:
  2,003 hits on the doubled heightfield, every one on the upper copy (prims 240-479);
  1,014 hits on the pile of 40 identical triangles, all on its last prim (519), each a 40-way tie;
  1,210 hits on the lattice; none on a zero-area triangle;
  1,114 rays whose best t is shared by at least 4 distinct triangles, 74 of them exact 6-way ties on lattice
  vertices."""
import numpy as np
import pytest

import degenerate as dg
import oracle
from test_bvh_build import _run, checker  # noqa: F401  (the bvh_check fixture and its runner)

FIELDS = ("t", "u", "v", "prim", "inst")


@pytest.fixture(scope="module")
def soup():
    tris, ranges = dg.degenerate_soup()
    O, D, slices = dg.edge_rays(1)
    return {"tris": tris, "ranges": ranges, "O": O, "D": D, "slices": slices, "bf": dg.brute_force(tris, O, D)}


def _tmax_cases(t):
    """tmax at the hit distance itself (no hit: a closest hit needs t < tmax), one ulp past it (the same hit), and a
    mix of shorter and longer limits; 1e30 on the rays that miss."""
    hit = t < dg.FAR
    at = np.where(hit, t, dg.FAR).astype(np.float32)
    past = np.where(hit, np.nextafter(t, np.float32(np.inf)), dg.FAR).astype(np.float32)
    mix = np.where(hit, t * np.float32(0.5), dg.FAR).astype(np.float32)
    mix[::3] = past[::3]
    return {"at": at, "past": past, "mix": mix}


@pytest.mark.parametrize("ninst", [1, 2])
def test_oracle_matches_brute_force(oracle_mod, soup, ninst):
    """OracleScene.intersect equals the brute force in every field for every ray, on the soup at one identity
    instance and at two coincident ones (every hit ties between the instances: instance 0), without tmax and with
    tmax at, just past and well before the hit; occluded equals t_brute < tmax."""
    osc = oracle.OracleScene(dg.soup_identity(ninst))
    O, D = soup["O"], soup["D"]
    want = dg.brute_force(soup["tris"], O, D, ninst)
    got = osc.intersect(O, D)
    for k, f in enumerate(FIELDS):
        assert np.array_equal(got[k], want[k]), f
    t = want[0]
    hit = t < dg.FAR
    for name, tm in _tmax_cases(t).items():
        want_tm = dg.brute_force(soup["tris"], O, D, ninst, tm)
        got_tm = osc.intersect(O, D, tm)
        for k, f in enumerate(FIELDS):
            assert np.array_equal(got_tm[k], want_tm[k]), (name, f)
        assert np.array_equal(osc.occluded(O, D, tm).astype(bool), t < tm), name
    at = osc.intersect(O, D, _tmax_cases(t)["at"])
    assert np.array_equal(at[0], np.where(hit, t, dg.FAR).astype(np.float32))
    assert not at[1].any() and not at[2].any() and not at[3].any() and not at[4].any()  # the miss record


def test_oracle_matches_brute_force_tiny(oracle_mod):
    """The five meshes of 1, 2, 7, 8 and 9 triangles at one identity instance each; every mesh is hit."""
    O, D, _ = dg.edge_rays(1)
    want = dg.brute_force_meshes(dg.tiny_pieces(), O, D)
    got = oracle.OracleScene(dg.tiny()).intersect(O, D)
    for k, f in enumerate(FIELDS):
        assert np.array_equal(got[k], want[k]), f
    hit = want[0] < dg.FAR
    for i in range(5):
        assert (hit & (want[4] == i)).sum() >= 10, i


def test_input_conditions(soup):
    """The inputs contain what they are for (from the brute force, never from the code under test)."""
    t, u, v, prim, inst, ties = soup["bf"]
    R = soup["ranges"]
    hit = ties > 0
    within = lambda name: hit & (prim >= R[name][0]) & (prim < R[name][1])
    d = within("doubled")
    half = (R["doubled"][1] - R["doubled"][0]) // 2
    assert d.sum() >= 1000 and (prim[d] >= R["doubled"][0] + half).all()  # the upper copy wins every tie
    assert (ties[d] >= 2).all()
    p = within("pile")
    assert p.sum() >= 100 and (prim[p] == R["pile"][1] - 1).all()
    assert within("lattice").sum() >= 1000
    assert within("zero_area").sum() == 0
    assert (ties >= 4).sum() >= 40
    assert (ties[within("lattice")] == 6).sum() >= 40  # interior lattice vertices
    # exact zeros of either sign in the directions, and the ragged batch sizes
    D = soup["D"]
    assert ((D == 0) & np.signbit(D)).any() and ((D == 0) & ~np.signbit(D)).any()
    assert D.shape[0] % 64 != 0
    s = soup["slices"]
    assert [s[k].stop - s[k].start for k in ("one", "s63", "s65")] == [1, 63, 65]
    assert hit[s["one"]].all() and hit[s["s63"]].any() and hit[s["s65"]].any()


def test_coincident70_inputs(oracle_mod):
    """70 coincident instances: the oracle reports instance 0 on every hit, as the brute force does."""
    O, D, _ = dg.edge_rays(1)
    want = dg.brute_force(dg.big_quad(), O, D, 70)
    got = oracle.OracleScene(dg.coincident70()).intersect(O, D)
    for k, f in enumerate(FIELDS):
        assert np.array_equal(got[k], want[k]), f
    assert (want[5] > 0).sum() >= 1000 and not got[4].any()


def test_soup4_primary_hits(oracle_mod):
    """soup4 from its camera: most primary rays hit, on instances 0, 2 and 3 and never on instance 1, the coincident
    copy that must always lose."""
    t, u, v, prim, inst = oracle.OracleScene(dg.soup4(), 96, 64).primary_hits(96, 64)
    hit = t < dg.FAR
    assert hit.mean() >= 0.5
    assert set(np.unique(inst[hit])) == {0, 2, 3}


def _tris_file(tmp_path, tris):
    path = str(tmp_path / "tris.bin")
    np.ascontiguousarray(dg.soup_mesh(tris).triangles, np.float32).tofile(path)
    return path


BLAS_MESHES = {
    "soup": lambda: dg.degenerate_soup()[0],
    "pile": dg.pile,
    "zero_area": dg.zero_area,
    "copies4096": lambda: dg.pile(4096),
    **{f"tiny{t.shape[0]}": (lambda t=t: t) for t in dg.tiny_pieces()},
}


@pytest.mark.parametrize("mesh", sorted(BLAS_MESHES))
@pytest.mark.parametrize("spatial", [0, 1])
def test_host_blas_invariants(checker, tmp_path, mesh, spatial):  # noqa: F811
    """bvh_build.cpp on coincident centroids, zero-area triangles, one to nine triangles and 4,096 copies of one
    triangle: every primitive referenced, every triangle inside its slot's box, the depth as reported."""
    tris = BLAS_MESHES[mesh]()
    out = _run(checker, "blas", _tris_file(tmp_path, tris), str(spatial))
    assert out["tris"] == tris.shape[0]
    if not spatial:
        assert out["refs"] == tris.shape[0]


def test_host_tlas_coincident_boxes(checker, tmp_path):  # noqa: F811
    """70 coincident instance boxes: every instance in exactly one slot of the instance BVH, inside its box."""
    P = dg.big_quad().reshape(-1, 3)
    box = np.concatenate([P.min(0), P.max(0)]).astype(np.float32)
    path = str(tmp_path / "boxes.bin")
    np.tile(box, (70, 1)).tofile(path)
    out = _run(checker, "tlas", path)
    assert out["instances"] == 70
