"""Host BVH builder invariants on the CPU (tests/cpp/bvh_check.cpp over physically-based-ray-tracer_amd/csrc/
bvh_build.cpp): the BLASes the object-split (PRT_BUILDER_HOST_SAH) and spatial-split (PRT_BUILDER_HOST_SBVH, the
reference's BuildHQ, Core/tiny_bvh.h:1968-2284) builders emit reference every primitive, keep every referenced
triangle inside its slot's dequantised box (the conservative-box contract behind the BVH-independent hit rule) and
report their true depth; the instance BVH (Core/tiny_bvh.h:1732-1770) holds every instance once, inside its box.
The checker's one tree-check function also runs over trees read from files (`dump` then `tree`): the host trees pass
it, and each defect planted in the dumped bytes is refused for its own reason -- the evidence that the checker, which
tests/test_gpu_builder_trees.py runs over the device builders' trees, catches what it claims.
The GPU tests check the same trees render bit-identically (test_gpu_parity.py::test_gpu_builder_renders_identical)."""
import json
import os
import subprocess

import numpy as np
import pytest

from prt import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physically-based-ray-tracer_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bvh") / "bvh_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "bvh_check.cpp"),
                    os.path.join(CSRC, "bvh_build.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and out["ok"], out
    return out


MESHES = {
    "heightfield": lambda: scenes.config_small(60, 40).meshes[0],
    "torus": lambda: scenes.torus(100, 50),
    "deep": lambda: scenes.deep_bvh().meshes[0],
}


@pytest.mark.parametrize("mesh", sorted(MESHES))
@pytest.mark.parametrize("spatial", [0, 1])
def test_blas_invariants(checker, tmp_path, mesh, spatial):
    m = MESHES[mesh]()
    path = str(tmp_path / "tris.bin")
    np.ascontiguousarray(m.triangles, np.float32).tofile(path)
    out = _run(checker, "blas", path, str(spatial))
    assert out["tris"] == m.tri_count
    if mesh == "deep":
        assert out["depth"] > 19  # deeper than every LDS stack: the HBM spill path's test scene
    if not spatial:
        assert out["refs"] == m.tri_count


def test_spatial_splits_duplicate_within_budget(checker, tmp_path):
    """Long thin slivers at random angles across a square (every box spans most of it, the triangles barely
    touch): the spatial splits cut references, so there are more references than triangles, within the 1.5x
    budget, and every part still lies inside its slot box."""
    n = 400
    rng = np.random.default_rng(2)
    a = rng.uniform(0, np.pi, n)
    c = rng.uniform(-1, 1, (n, 2))
    d = np.stack([np.cos(a), np.sin(a)], 1)
    p0, p1 = c - 6 * d, c + 6 * d
    w = 0.01 * np.stack([-d[:, 1], d[:, 0]], 1)
    P = np.zeros((n, 3, 4), np.float32)
    P[:, 0, [0, 2]], P[:, 1, [0, 2]], P[:, 2, [0, 2]] = p0, p1, p1 + w
    P[:, :, 1] = rng.uniform(0, 0.05, n)[:, None]
    path = str(tmp_path / "slivers.bin")
    P.reshape(-1).tofile(path)
    out = _run(checker, "blas", path, "1")
    assert n < out["refs"] <= 1.5 * n + 8
    assert _run(checker, "blas", path, "0")["refs"] == n


def _dump(exe, tris_path, spatial, d):
    """The host builder's tree over tris_path as raw bytes: (nodes file, records file, the dump's JSON)."""
    n, r = str(d / f"nodes{spatial}.bin"), str(d / f"recs{spatial}.bin")
    return n, r, _run(exe, "dump", tris_path, str(spatial), n, r)


@pytest.mark.parametrize("mesh", sorted(MESHES))
@pytest.mark.parametrize("spatial", [0, 1])
def test_dumped_tree_passes_the_file_checker(checker, tmp_path, mesh, spatial):
    """dump then tree: the tree read from files passes every invariant and is the tree `blas` checks."""
    m = MESHES[mesh]()
    path = str(tmp_path / "tris.bin")
    np.ascontiguousarray(m.triangles, np.float32).tofile(path)
    n, r, d = _dump(checker, path, spatial, tmp_path)
    tree = _run(checker, "tree", path, n, r, str(spatial), str(d["depth"]))
    blas = _run(checker, "blas", path, str(spatial))
    assert tree == blas
    assert (tree["nodes"], tree["refs"], tree["depth"]) == (d["nodes"], d["refs"], d["depth"])
    assert tree["leaf_slots"] == d["leaves"] and 1 <= tree["max_count"] <= 3 and tree["cost"] > 0
    assert os.path.getsize(n) == 80 * d["nodes"] and os.path.getsize(r) == 48 * d["refs"]


# ---- defects planted in a dumped tree: Node8 is px py pz (3 f32) | ex ey ez imask | child_base tri_base (u32) |
# meta[8] | qlox qloy qloz qhix qhiy qhiz [8] each; TriMT is v0[3] prim e1[3] 0 e2[3] 0

QHIX = 56


class _Tree:
    def __init__(self, nodes, recs, tris):
        self.nodes, self.recs, self.tris = nodes.copy(), recs.copy(), tris
        self.child_base = self.nodes[:, 16:20].view(np.uint32).reshape(-1)
        self.tri_base = self.nodes[:, 20:24].view(np.uint32).reshape(-1)
        self.prim = self.recs[:, 12:16].view(np.uint32).reshape(-1)

    def interior(self, j):
        """[(slot, child)] of node j, in slot order."""
        out = []
        for s in range(8):
            if (self.nodes[j, 15] >> s) & 1:
                out.append((s, int(self.child_base[j]) + len(out)))
        return out

    def leaves(self, j):
        """[(slot, first record, count)] of node j, in slot order."""
        out = []
        for s in range(8):
            meta = int(self.nodes[j, 24 + s])
            if not (self.nodes[j, 15] >> s) & 1 and meta & 7:
                out.append((s, int(self.tri_base[j]) + (meta >> 3), meta & 7))
        return out

    def parents(self):
        """{child: (parent, slot)}."""
        return {c: (j, s) for j in range(len(self.nodes)) for s, c in self.interior(j)}

    def hi_x(self, j, s):
        px = float(self.nodes[j, 0:4].view(np.float32)[0])
        return px + float(self.nodes[j, QHIX + s]) * 2.0 ** (int(self.nodes[j, 12]) - 127)

    def max_x(self, first, cnt):
        return float(self.tris[self.prim[first:first + cnt]][:, :, 0].max())

    def shrink_hi_x(self, j, s, first, cnt):
        """Lower slot s of node j's high x plane, a quantum at a time, until a vertex of the records sticks out."""
        while self.hi_x(j, s) >= self.max_x(first, cnt):
            assert self.nodes[j, QHIX + s] > 0
            self.nodes[j, QHIX + s] -= 1


def _leaf_box(t):
    j = next(j for j in range(len(t.nodes)) if t.leaves(j))
    s, first, cnt = t.leaves(j)[0]
    t.shrink_hi_x(j, s, first, cnt)


def _ancestor_box(t):
    """The slot two levels above a leaf slot: the leaf slot's own box, and its parent's, stay as they were."""
    up = t.parents()
    j = next(j for j in range(len(t.nodes)) if t.leaves(j) and j in up and up[j][0] in up)
    _, first, cnt = t.leaves(j)[0]
    g, gs = up[up[j][0]]
    own = t.nodes[j].copy()
    t.shrink_hi_x(g, gs, first, cnt)
    assert np.array_equal(t.nodes[j], own)


def _swap_prim(t):
    """The prim of record 0 and of the first record whose triangle leaves record 0's slot box."""
    j, (s, first, cnt) = next((j, l) for j in range(len(t.nodes)) for l in t.leaves(j) if l[1] == 0)
    other = next(i for i in range(cnt, len(t.recs)) if t.max_x(i, 1) > t.hi_x(j, s))
    t.prim[0], t.prim[other] = t.prim[other], t.prim[0]


def _duplicate_prim(t):
    """Within one leaf slot (so that both records stay inside the box): one primitive twice, one nowhere."""
    first = next(l[1] for j in range(len(t.nodes)) for l in t.leaves(j) if l[2] >= 2)
    t.prim[first] = t.prim[first + 1]


def _shared_children(t):
    """The later of two siblings points at the earlier one's children (which the walk has then already reached)."""
    for j in range(len(t.nodes)):
        kids = [c for _, c in t.interior(j) if t.interior(c)]
        if len(kids) >= 2:
            t.child_base[kids[1]] = t.child_base[kids[0]]
            return
    raise AssertionError("no two sibling nodes with children")


def _orphan(t):
    """A node's last interior slot emptied (the earlier slots keep their children): its subtree hangs loose."""
    j = next(j for j in range(len(t.nodes)) if t.interior(j))
    s = t.interior(j)[-1][0]
    t.nodes[j, 15] &= np.uint8(~(1 << s) & 0xFF)
    assert t.nodes[j, 24 + s] == 0
    t.nodes[j, [32 + s, 40 + s, 48 + s]] = 255  # emptied as a builder empties a slot: the inverted box qlo = 255,
    t.nodes[j, [56 + s, 64 + s, 72 + s]] = 0    # qhi = 0 (without it the checker stops at the slot itself, below)


def _not_inverted(t):
    """An interior slot's imask bit cleared and nothing else: an unoccupied slot (meta 0) that kept a real box."""
    j = next(j for j in range(len(t.nodes)) if t.interior(j))
    s = t.interior(j)[-1][0]
    t.nodes[j, 15] &= np.uint8(~(1 << s) & 0xFF)
    assert t.nodes[j, 24 + s] == 0 and t.nodes[j, 32 + s] <= t.nodes[j, 56 + s]


def _overlap(t):
    j = next(j for j in range(len(t.nodes)) if len(t.leaves(j)) >= 2)
    s = t.leaves(j)[1][0]
    assert t.nodes[j, 24 + s] >> 3 >= 1
    t.nodes[j, 24 + s] -= 8  # its range now starts on the last record of the slot before it


def _count_4(t):
    j = next(j for j in range(len(t.nodes)) if t.leaves(j))
    s = t.leaves(j)[0][0]
    t.nodes[j, 24 + s] = (t.nodes[j, 24 + s] & 0xF8) | 4


def _e1_bit(t):
    t.recs[0, 16] ^= 1  # the lowest mantissa bit of e1.x (little-endian float32)


def _truncate(t):
    t.nodes = t.nodes[:-1]


DEFECTS = {
    "leaf_box": (_leaf_box, 0, "triangle outside its slot box"),
    "ancestor_box": (_ancestor_box, 0, "triangle outside an ancestor's slot box"),
    "swap_prim": (_swap_prim, 0, "triangle outside its slot box"),
    "duplicate_prim": (_duplicate_prim, 0, "primitive in several leaves"),
    "shared_children": (_shared_children, 0, "node reached twice"),
    "orphan": (_orphan, 0, "node not reached from the root"),
    "not_inverted": (_not_inverted, 0, "empty slot without the inverted box"),
    "overlap": (_overlap, 0, "record in two leaf ranges"),
    "count_4": (_count_4, 0, "leaf count above the maximum"),
    "depth_plus": (lambda t: None, 1, "reported depth differs"),
    "depth_minus": (lambda t: None, -1, "reported depth differs"),
    "e1_bit": (_e1_bit, 0, "record differs from its triangle"),
    "truncate": (_truncate, 0, "interior child out of range"),
}


@pytest.fixture(scope="module")
def dumped(checker, tmp_path_factory):
    """config_small(40, 30)'s object-split tree, dumped once: (tris file, Node8 bytes, TriMT bytes, corners, depth)."""
    d = tmp_path_factory.mktemp("dumped")
    m = scenes.config_small(40, 30).meshes[0]
    path = str(d / "tris.bin")
    np.ascontiguousarray(m.triangles, np.float32).tofile(path)
    n, r, out = _dump(checker, path, 0, d)
    corners = np.asarray(m.triangles, np.float32).reshape(-1, 3, 4)[:, :, :3]
    return path, np.fromfile(n, np.uint8).reshape(-1, 80), np.fromfile(r, np.uint8).reshape(-1, 48), corners, out["depth"]


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_checker_refuses_a_planted_defect(checker, dumped, tmp_path, defect):
    """One defect per case, planted at the first place it applies (a scan in node order, nothing random); the
    unmutated bytes pass; the mutated tree is refused, and for the reason that names the defect.  ancestor_box is the
    one only the chain of ancestor boxes can catch: the leaf slot's own box still holds its triangles."""
    path, nodes, recs, corners, depth = dumped
    mutate, ddepth, what = DEFECTS[defect]
    t = _Tree(nodes, recs, corners)
    mutate(t)
    assert ddepth or t.nodes.shape != nodes.shape or not (np.array_equal(t.nodes, nodes) and np.array_equal(t.recs, recs))
    n, r = str(tmp_path / "nodes.bin"), str(tmp_path / "recs.bin")
    nodes.tofile(n)
    recs.tofile(r)
    assert _run(checker, "tree", path, n, r, "0", str(depth))["nodes"] == len(nodes)
    t.nodes.tofile(n)
    t.recs.tofile(r)
    res = subprocess.run([checker, "tree", path, n, r, "0", str(depth + ddepth)], capture_output=True, text=True, timeout=60)
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert res.returncode == 1 and out["ok"] is False and out["what"] == what, out


def test_tlas_invariants(checker, tmp_path):
    sd = scenes.instance_field(300)
    boxes = []
    for mi, xf in sd.instances:
        P = sd.meshes[mi].vertices.reshape(-1, 3).astype(np.float64)
        W = P @ xf[:3, :3].T.astype(np.float64) + xf[:3, 3]
        boxes.append(np.concatenate([W.min(0), W.max(0)]))
    path = str(tmp_path / "boxes.bin")
    np.asarray(boxes, np.float32).tofile(path)
    out = _run(checker, "tlas", path)
    assert out["instances"] == len(sd.instances) and out["depth"] >= 3 and not out["median"]


@pytest.mark.parametrize("n", [1, 2, 9, 65, 1000, 5000])
def test_tlas_depth_cap_and_median_fallback(checker, tmp_path, n):
    """build_tlas8's depth cap (prt_api_instance.cpp ensure_instances sizes the traversal stacks at an instance count's first
    build and caps the worker's later builds there): a cap at the SAH tree's own depth keeps the SAH tree; a cap
    below it yields the balanced median-split tree, within tlas8_median_depth(n) levels; both keep every instance in
    exactly one slot, inside its slot's box, and at most max(n, 1) nodes."""
    rng = np.random.default_rng(n)
    c = rng.uniform(-4.5, 4.5, (n, 3)).astype(np.float32)
    c[:, 1] *= np.float32(0.1)
    h = np.array([0.4, 0.15, 0.4], np.float32)
    path = str(tmp_path / "boxes.bin")
    np.concatenate([c - h, c + h], axis=1).astype(np.float32).tofile(path)
    free = _run(checker, "tlas", path)
    same = _run(checker, "tlas", path, str(free["depth"]))
    assert not same["median"] and same["depth"] == free["depth"] and same["nodes"] == free["nodes"]
    capped = _run(checker, "tlas", path, str(free["median_depth"]))
    assert capped["depth"] <= free["median_depth"]
    assert capped["median"] == (free["depth"] > free["median_depth"])
