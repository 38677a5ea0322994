"""The trees the device builders emit (csrc/bvh_gpu.hip: Morton keys, the Karras radix tree, PLOC merging, treelet
restructuring, the SAH-optimal 8-wide collapse, outward quantisation, k_prim_records), read back with prt_read_blas /
prt_read_blas_tris and checked structurally by tests/cpp/bvh_check.cpp's `tree` mode -- the checker whose every reason
tests/test_bvh_build.py shows firing on a planted defect -- instead of only through the rays a few views happen to fire:
every node reached once, every record in one leaf range, every primitive referenced once, every triangle inside the
boxes of its leaf slot and of all the slots above it, the records' bytes, the reported depth; the host builders' trees
byte for byte through the upload; two meshes side by side; after a refit; two builds giving one tree; the treelet
passes changing the tree, and the SAH cost of the device trees against the host builder's; the cooperative traversal
tail (the one reader of what k_prim_records writes) on device-built trees.

No tree that fails a check, and no mutated tree, is ever uploaded: the checker runs on the CPU over bytes read back.

Meshes (the smallest at which each path exists): the first n triangles of config_small(40, 30)'s heightfield for n at
the single leaf, the treelet pass's n < 3 skip, one wide node against two (8 slots x 3 triangles), PLOC's search radius
of 64 and the 256-thread block edge; the whole heightfield (2,400), torus(40, 20) (1,600), deep_bvh(1000), and the
identical-Morton-code and zero-extent meshes of tests/degenerate.py."""
import contextlib
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import deform
import degenerate
import oracle
import prt
from helpers import gpu_scene
from prt import _lib, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physically-based-ray-tracer_amd", "csrc")
W, H = 64, 48  # (the tree tests render nothing: the camera's aspect only)
LBVH, PLOC = _lib.BUILDER_GPU_LBVH, _lib.BUILDER_GPU_PLOC
DEVICE = {"gpu_lbvh": LBVH, "gpu_ploc": PLOC}
PREFIXES = (1, 2, 3, 8, 9, 24, 25, 64, 65, 256, 257)

# SAH cost of the device builders' wide trees over the host SAH builder's on the same mesh (bvh_check's `cost`, the
# same code and formula for both), measured on an MI355X on 2026-10-20; the builds are deterministic, so the figures
# reproduce to rounding, and the tests allow 5 % for harmless retuning.  LBVH_0: the LBVH tree without its treelet
# passes, recorded so that what the 2 default passes buy stands beside it: without them the tree costs 45 % more on
# the heightfield and 15 % more on the torus, so a build that silently lost its passes overshoots the margin on both.
COST_RATIO = {
    "heightfield": {"gpu_lbvh": 1.130517, "gpu_ploc": 1.080353, "gpu_lbvh_0": 1.638657},  # host cost 9.144072
    "torus": {"gpu_lbvh": 1.022945, "gpu_ploc": 0.990947, "gpu_lbvh_0": 1.173061},        # host cost 11.818170
}
COST_MARGIN = 1.05


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bvh") / "bvh_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "bvh_check.cpp"), os.path.join(CSRC, "bvh_build.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


_MESHES = None


def meshes():
    """{name: scenes.Mesh}, made once."""
    global _MESHES
    if _MESHES is None:
        hf = scenes.config_small(40, 30).meshes[0]
        corners = degenerate.mesh_tris(hf)
        out = {f"hf[:{n}]": degenerate.soup_mesh(corners[:n]) for n in PREFIXES}
        out["heightfield"] = hf
        tor = scenes.torus(40, 20)
        tor.albedo, tor.metalness = 0, 2
        out["torus"] = tor
        out["deep"] = scenes.deep_bvh(1000).meshes[0]
        for name in ("doubled", "pile", "zero_area", "lattice"):
            out[name] = degenerate.soup_mesh(getattr(degenerate, name)())
        out["slivers"] = degenerate.soup_mesh(degenerate.slivers())
        _MESHES = out
    return _MESHES


def scene_of(*names):
    """The named meshes at one identity instance each, with config_small's textures, lights and sky."""
    base = scenes.deep_bvh(1000) if names == ("deep",) else scenes.config_small(40, 30)
    ms = [meshes()[n] for n in names]
    eye = np.eye(4, dtype=np.float32)
    return dataclasses.replace(base, meshes=ms, instances=[(i, eye) for i in range(len(ms))], name="+".join(names))


@contextlib.contextmanager
def context(builder):
    c = prt.Context(0)
    try:
        c.set_bvh_builder(builder)
        yield c
    finally:
        c.close()


def tris_file(mesh, path):
    np.ascontiguousarray(mesh.triangles, np.float32).tofile(path)
    return path


def run_tree(exe, d, mesh, nodes, recs, depth, spatial=0):
    """bvh_check tree over (mesh's triangles, nodes, recs): its JSON line, ok or not."""
    t, n, r = tris_file(mesh, str(d / "tris.bin")), str(d / "nodes.bin"), str(d / "recs.bin")
    nodes.tofile(n)
    recs.tofile(r)
    res = subprocess.run([exe, "tree", t, n, r, str(spatial), str(depth)], capture_output=True, text=True, timeout=120)
    assert res.stdout.strip(), (res.returncode, res.stderr[-2000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert (res.returncode == 0) == bool(out["ok"])
    return out


def host_tree(exe, d, mesh, spatial=0):
    """The host builder's tree over mesh: (Node8 bytes, TriMT bytes, the checker's JSON for it)."""
    t, n, r = tris_file(mesh, str(d / "host_tris.bin")), str(d / "host_nodes.bin"), str(d / "host_recs.bin")
    res = subprocess.run([exe, "dump", t, str(spatial), n, r], capture_output=True, text=True, timeout=120)
    dump = json.loads(res.stdout.strip().splitlines()[-1])
    assert res.returncode == 0 and dump["ok"]
    nodes, recs = np.fromfile(n, np.uint8).reshape(-1, 80), np.fromfile(r, np.uint8).reshape(-1, 48)
    out = run_tree(exe, d, mesh, nodes, recs, dump["depth"], spatial)
    assert out["ok"], out
    return nodes, recs, out


def build_and_check(c, exe, d, name):
    """Mesh `name` alone in context c, under c's builder: its tree read back and checked against the mesh, the depth
    the scene reports as the reported depth, and the scene's counts against what the walk found.  Returns the
    checker's JSON ({"ok": False, ...} with the reason on a violation)."""
    m = meshes()[name]
    gpu_scene(c, scene_of(name), W, H)
    info = c.scene_info()
    nodes, recs = c.read_blas(0), c.read_blas_tris(0)
    out = run_tree(exe, d, m, nodes, recs, info.max_depth)
    if out["ok"]:
        got = dict(tris=info.triangles, nodes=info.blas_nodes, refs=len(recs), leaf_slots=info.blas_leaves)
        want = dict(tris=m.tri_count, nodes=out["nodes"], refs=m.tri_count, leaf_slots=out["leaf_slots"])
        if got != want or out["tris"] != m.tri_count or out["refs"] != m.tri_count:
            return dict(ok=False, what="scene_info or record count", got=got, want=want)
    return out


# ---- every device tree, structurally

@pytest.mark.parametrize("builder,passes", [("gpu_lbvh", "0"), ("gpu_lbvh", None), ("gpu_lbvh", "3"), ("gpu_ploc", None),
                                            ("gpu_ploc", "1")])
def test_device_trees_hold_every_invariant(checker, tmp_path, monkeypatch, builder, passes):
    """PRT_TRBVH passes: None is the builder's default (2 on LBVH, 0 on PLOC).  deep_bvh's PLOC tree is deeper than
    the 64 levels the renderer accepts (tests/test_gpu_mesh_update.py); it is set, read and checked like the others,
    and nothing here renders."""
    if passes is None:
        monkeypatch.delenv("PRT_TRBVH", raising=False)
    else:
        monkeypatch.setenv("PRT_TRBVH", passes)
    names = [f"hf[:{n}]" for n in PREFIXES] + ["heightfield", "torus", "deep", "doubled", "pile", "zero_area", "lattice"]
    bad, depths = {}, {}
    with context(DEVICE[builder]) as c:
        for name in names:
            out = build_and_check(c, checker, tmp_path, name)
            assert c.scene_info().builder == DEVICE[builder]
            if not out["ok"]:
                bad[name] = out
            else:
                depths[name] = out["depth"]
    print(builder, passes, "depths", depths)
    assert not bad, bad
    assert depths["hf[:1]"] == depths["hf[:2]"] == depths["hf[:3]"] == 1 and depths["heightfield"] >= 3


# ---- the host builders' trees through the upload and back

@pytest.mark.parametrize("builder,spatial", [(_lib.BUILDER_HOST_SAH, 0), (_lib.BUILDER_HOST_SBVH, 1)])
def test_host_trees_come_back_byte_for_byte(checker, tmp_path, builder, spatial):
    """Three meshes in one scene, so that the second and third sit at non-zero node and record offsets: what
    prt_read_blas and prt_read_blas_tris return is what the host builder made (bvh_check dump), through the rebase into
    the concatenated arrays, the upload and the reads' way back.  The slivers' spatial-split tree has more records
    than triangles."""
    names = ("heightfield", "torus", "slivers")
    with context(builder) as c:
        gpu_scene(c, scene_of(*names), W, H)
        info = c.scene_info()
        got = [(c.read_blas(i), c.read_blas_tris(i)) for i in range(len(names))]
    depth = total_nodes = total_leaves = 0
    for name, (nodes, recs) in zip(names, got):
        m = meshes()[name]
        want_nodes, want_recs, out = host_tree(checker, tmp_path, m, spatial)
        assert np.array_equal(nodes, want_nodes), name
        assert np.array_equal(recs, want_recs), name
        assert len(recs) == m.tri_count if not spatial else len(recs) >= m.tri_count, name
        depth, total_nodes, total_leaves = max(depth, out["depth"]), total_nodes + out["nodes"], total_leaves + out["leaf_slots"]
    assert (info.max_depth, info.blas_nodes, info.blas_leaves) == (depth, total_nodes, total_leaves)
    if spatial:
        assert len(got[2][1]) > meshes()["slivers"].tri_count


def test_read_blas_tris_refusals():
    """prt_read_blas_tris refuses what prt_read_blas refuses: no meshes, an index out of range, a buffer too small;
    tris == NULL only reports the byte count."""
    n = _lib.C.c_uint64(7)
    with context(LBVH) as c:
        assert c.L.prt_read_blas_tris(c.h, 0, None, 0, _lib.C.byref(n)) == -5 and n.value == 7  # no scene yet
        gpu_scene(c, scene_of("hf[:9]", "torus"), W, H)
        for i in (-1, 2):
            assert c.L.prt_read_blas_tris(c.h, i, None, 0, _lib.C.byref(n)) == -1 and n.value == 7
        assert c.L.prt_read_blas_tris(c.h, 0, None, 0, _lib.C.byref(n)) == 0 and n.value == 9 * 48
        assert c.L.prt_read_blas_tris(c.h, 1, None, 0, _lib.C.byref(n)) == 0 and n.value == 1600 * 48
        buf = np.full(n.value, 0xAB, np.uint8)
        assert c.L.prt_read_blas_tris(c.h, 1, buf.ctypes.data, n.value - 1, None) == -1
        assert b"buffer too small" in c.L.prt_last_error() and np.all(buf == 0xAB)
        assert c.L.prt_read_blas_tris(c.h, 1, buf.ctypes.data, n.value, None) == 0
        assert np.array_equal(buf.reshape(-1, 48), c.read_blas_tris(1))


# ---- two meshes

@pytest.mark.parametrize("builder", sorted(DEVICE))
def test_two_meshes_each_check_out_alone(checker, tmp_path, builder):
    """The heightfield and the torus set together: each mesh's tree, read back with mesh-relative offsets, passes the
    checker against its own triangles and is the tree the mesh gets when it is built alone (the same canonical hash,
    the builds being deterministic: test_two_builds_give_one_tree) -- neither build wrote into the other's range."""
    names = ("heightfield", "torus")
    with context(DEVICE[builder]) as c:
        alone = [build_and_check(c, checker, tmp_path, n) for n in names]
        assert all(a["ok"] for a in alone), alone
        gpu_scene(c, scene_of(*names), W, H)
        info = c.scene_info()
        got = [(c.read_blas(i), c.read_blas_tris(i)) for i in range(2)]
    for name, a, (nodes, recs) in zip(names, alone, got):
        out = run_tree(checker, tmp_path, meshes()[name], nodes, recs, a["depth"])
        assert out["ok"], (name, out)
        assert out == a, (name, out, a)
    assert info.max_depth == max(a["depth"] for a in alone)
    assert info.blas_nodes == sum(a["nodes"] for a in alone) and info.blas_leaves == sum(a["leaf_slots"] for a in alone)
    assert info.triangles == sum(meshes()[n].tri_count for n in names)


# ---- after a refit

@pytest.mark.parametrize("builder", sorted(DEVICE))
def test_refitted_tree_holds_every_invariant(checker, tmp_path, builder):
    """prt_update_mesh over a device-built tree: the tree read back passes the checker against V1's triangles (every
    ancestor box, the records' bytes), with the topology's counts and depth unchanged and other boxes than before."""
    hf = meshes()["heightfield"]
    v1 = deform.sine_twist(hf, amp=0.5, twist=0.08)
    with context(DEVICE[builder]) as c:
        before = build_and_check(c, checker, tmp_path, "heightfield")
        assert before["ok"], before
        c.update_mesh(0, v1)
        info = c.scene_info()
        nodes, recs = c.read_blas(0), c.read_blas_tris(0)
    after = run_tree(checker, tmp_path, v1, nodes, recs, before["depth"])
    assert after["ok"], after
    assert after["canon"] != before["canon"]
    assert all(after[k] == before[k] for k in ("tris", "nodes", "refs", "depth", "leaf_slots", "max_count"))
    assert (info.max_depth, info.blas_nodes, info.blas_leaves) == (before["depth"], before["nodes"], before["leaf_slots"])
    stale = run_tree(checker, tmp_path, hf, nodes, recs, before["depth"])  # (the refitted tree is V1's, not V0's)
    assert not stale["ok"]


# ---- two builds, one tree

@pytest.mark.parametrize("builder", sorted(DEVICE))
def test_two_builds_give_one_tree(checker, tmp_path, builder):
    """Two fresh contexts build the heightfield: the same canonical tree (topology, boxes, leaf contents; where the
    atomic counters placed nodes and ranges is left out of the hash) and so the same cost."""
    outs = []
    for _ in range(2):
        with context(DEVICE[builder]) as c:
            outs.append(build_and_check(c, checker, tmp_path, "heightfield"))
    assert outs[0]["ok"] and outs[1]["ok"], outs
    assert outs[0] == outs[1]


# ---- the treelet passes restructure, and what the trees cost

@pytest.mark.parametrize("name", ["heightfield", "torus"])
def test_restructuring_changes_the_tree_and_cost_stays_on_record(checker, tmp_path, monkeypatch, name):
    """LBVH at its default 2 passes and at 0 passes: another tree, and a cheaper one; each device builder's cost over
    the host SAH builder's stays within COST_MARGIN of the recorded ratio."""
    monkeypatch.delenv("PRT_TRBVH", raising=False)
    _, _, host = host_tree(checker, tmp_path, meshes()[name])
    out = {}
    for key, builder, passes in (("gpu_lbvh", LBVH, None), ("gpu_lbvh_0", LBVH, "0"), ("gpu_ploc", PLOC, None)):
        if passes is not None:
            monkeypatch.setenv("PRT_TRBVH", passes)
        with context(builder) as c:
            out[key] = build_and_check(c, checker, tmp_path, name)
        monkeypatch.delenv("PRT_TRBVH", raising=False)
        assert out[key]["ok"], (key, out[key])
    ratio = {k: v["cost"] / host["cost"] for k, v in out.items()}
    print(name, "host cost", host["cost"], "ratios", {k: round(v, 6) for k, v in ratio.items()})
    assert out["gpu_lbvh"]["canon"] != out["gpu_lbvh_0"]["canon"]  # the passes still rewire
    assert out["gpu_lbvh"]["cost"] < out["gpu_lbvh_0"]["cost"]      # and towards a lower SAH cost
    for key in ("gpu_lbvh", "gpu_ploc"):
        assert ratio[key] <= COST_RATIO[name][key] * COST_MARGIN, (key, ratio[key])


# ---- the cooperative traversal tail over device-built trees

TW, TH, TSPP, TB = 128, 96, 4, 4
_TAIL = {}


def tail_case():
    """(scene, scene over V1, V1, the oracle's frame and ray totals for each), made once."""
    if not _TAIL:
        sd = scenes.multi_instance(scenes.config_small(60, 50))
        v1 = deform.sine_twist(sd.meshes[0], amp=0.5, twist=0.08)
        sd1 = dataclasses.replace(sd, meshes=[v1] + list(sd.meshes[1:]))
        want = []
        for s in (sd, sd1):
            avg, rgb8, _, st = oracle.OracleScene(s, TW, TH).render(TW, TH, spp=TSPP, bounces=TB)
            want.append((avg, rgb8, (int(st.segments), int(st.shadow_rays))))
        _TAIL.update(sd=sd, sd1=sd1, v1=v1, want=want)
    return _TAIL


@pytest.mark.parametrize("builder", sorted(DEVICE))
def test_traversal_tail_on_device_built_trees(monkeypatch, builder):
    """k_prim_records (device builders only) writes each primitive's record index into ShadeTri.pad[0], which only the
    cooperative tail reads (prt_persist.h): with the tail on and off the frames and ray totals are identical and the
    oracle's, and again after prt_update_mesh."""
    t = tail_case()

    def frames(c, sd):
        out = {}
        for mode in ("0", "1"):
            monkeypatch.setenv("PRT_TAIL", mode)
            c.set_camera(prt.Camera(sd.cam_pos, sd.cam_target, np.float32(TW) / np.float32(TH)))
            c.reset_accumulation(full=True)
            avg, rgb8, st = c.render(TW, TH, TSPP, TB)
            out[mode] = (avg, rgb8, (int(st.segments), int(st.shadow_rays)))
        monkeypatch.delenv("PRT_TAIL")
        return out

    with context(DEVICE[builder]) as c:
        gpu_scene(c, t["sd"], TW, TH)
        assert c.scene_info().builder == DEVICE[builder]
        got = [frames(c, t["sd"])]
        c.update_mesh(0, t["v1"])
        got.append(frames(c, t["sd1"]))
    for which, (g, want) in enumerate(zip(got, t["want"])):
        for mode in ("0", "1"):
            assert np.array_equal(g[mode][0], want[0]) and np.array_equal(g[mode][1], want[1]), (which, mode)
            assert g[mode][2] == want[2], (which, mode)
    assert not np.array_equal(t["want"][0][0], t["want"][1][0])  # the deformation shows
