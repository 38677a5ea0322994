"""Device skinning (include/prt.h prt_set_mesh_skin / prt_skin_mesh, csrc/prt_skin.hip): with R = skin_ref(mesh, skin,
M), a context that binds the skin and calls skin_mesh(M) returns, bit for bit, what a context returns after
update_mesh(R) and what the oracle returns over R -- the BLAS bytes (within one context for the device builders, whose
node placement differs from build to build), the queries, the frame -- for all four builders;
a pose sequence there and back is byte-identical and leaves the other mesh alone; 1, 300 and 65,536 joints (the last
two beyond the LDS staging); a pose that collapses triangles; device matrices; the instance boxes, the instance BVH, the
kept primary hits and the deform chain follow; frames in flight with a pose before every frame equal one frame at a
time; refusals change nothing; prt_set_meshes drops the binding; a local group; Renderer.SkinModel.

Scenes and shapes are tests/test_gpu_mesh_update.py's: config_small(40, 30) (the height field, V = 1,271, T = 2,400,
with its normal map), the same through multi_instance, instance_field(300) (instance BVH; the torus is skinned) and the
height field plus torus(40, 20) (the torus, mesh 1, is skinned).  Image 96 x 72, 2 spp, depth 3; 8,192 random rays."""
import contextlib
import dataclasses

import numpy as np
import pytest

import oracle
import prt
import skin_ref
from helpers import gpu_scene, random_rays
from prt import _lib, scenes

pytestmark = pytest.mark.gpu

W, H, SPP, B, NRAYS = 96, 72, 2, 3, 8192
BUILDERS = {"host_sah": _lib.BUILDER_HOST_SAH, "gpu_lbvh": _lib.BUILDER_GPU_LBVH, "host_sbvh": _lib.BUILDER_HOST_SBVH,
            "gpu_ploc": _lib.BUILDER_GPU_PLOC}
F32 = np.float32


def _two_mesh():
    base = scenes.config_small(40, 30)
    tor = scenes.torus(40, 20)
    tor.albedo, tor.metalness = 0, 2
    T = np.eye(4, dtype=F32)
    T[:3, 3] = (0.4, 1.1, 0.3)
    return dataclasses.replace(base, meshes=list(base.meshes) + [tor], instances=list(base.instances) + [(1, T)],
                               name="hf+torus")


def _scene(name):
    """(scene, index of the skinned mesh)"""
    if name == "small":
        return scenes.config_small(40, 30), 0
    if name == "multi":
        return scenes.multi_instance(scenes.config_small(40, 30)), 0
    if name == "field":
        return scenes.instance_field(300), 1
    assert name == "two"
    return _two_mesh(), 1


_SETUPS = {}
_ORACLE = {}
# Where the pose `flat` collapses what follows joint 0 alone: a point off the camera's axis and a few units from every
# coordinate plane.  The pose `flat0` collapses into the origin instead, the point the scenes' cameras look at: the
# first AA sample of the centre pixel travels exactly through it, and a BLAS node whose whole extent is the 2e-7 of an
# inflated point at the origin is smaller than half an ulp of the ray's distance to it.  There the slab test's
# fma(255, b, a) rounds to a and the inverted box of an unoccupied child slot (255 .. 0) no longer misses; a node
# visit hands on occupied slots only (prt_node8.h), so the pose renders like any other (before that rule the
# wavefront traversal's triangle step took such a slot's count of 0 for a count, which underflowed).  A box around a
# point p is inflated by |p| * 1e-6, so a few units away the node is some 1e-6 wide and the slab test is exact again:
# `flat` never met the condition, and stays as the ordinary case.
COLLAPSE_POINT = (-2.5, 1.0, 1.5)


@dataclasses.dataclass
class Setup:
    sd: object
    mi: int
    skin: object
    M: dict   # pose name -> [J, 12]
    _R: dict = dataclasses.field(default_factory=dict)

    def R(self, pose):
        """skin_ref's mesh for a pose, computed once"""
        if pose not in self._R:
            self._R[pose] = skin_ref.skin_mesh(self.sd.meshes[self.mi], self.skin, self.M[pose])
        return self._R[pose]

    def scene(self, pose):
        ms = list(self.sd.meshes)
        ms[self.mi] = self.R(pose)
        return dataclasses.replace(self.sd, meshes=ms)


def setup(name, J=3):
    """The scene `name` with its mesh bound to J joints (above 8: seven of them used, the first and the last among
    them) and the poses m1, m2 (ordinary), x2 (every joint doubles the extent), flat (the first joint collapses what
    follows it alone, into COLLAPSE_POINT) and flat0 (the same into the origin)."""
    if (name, J) not in _SETUPS:
        sd, mi = _scene(name)
        mesh = sd.meshes[mi]
        used = None if J <= 8 else np.unique(np.concatenate([np.arange(0, J, max(1, J // 6)), [J - 1]]))
        j, w = skin_ref.smooth_weights(mesh.vertices.reshape(-1, 3), J, used=used)
        skin = scenes.Skin.from_mesh(mesh, j, w, J)
        amount = 0.3 if name == "field" else 1.0
        M = {"m1": skin_ref.pose(J, seed=11 + J, amount=amount, used=used),
             "m2": skin_ref.pose(J, seed=23 + J, amount=0.6 * amount, used=used),
             "x2": np.tile(skin_ref.rigid(scale=2.0), (J, 1))}
        M["flat"] = M["m1"].copy()
        M["flat"][0] = (0, 0, 0, -2.5, 0, 0, 0, 1.0, 0, 0, 0, 1.5)  # see COLLAPSE_POINT
        M["flat0"] = M["m1"].copy()
        M["flat0"][0] = 0.0  # into the origin
        _SETUPS[(name, J)] = Setup(sd, mi, skin, M)
    return _SETUPS[(name, J)]


def rays(sd):
    O, D = random_rays(sd, NRAYS, seed=11)
    tmax = np.random.default_rng(12).uniform(0.5, 12.0, NRAYS).astype(F32)
    return O, D, tmax


def oracle_results(key, sd):
    """What the oracle returns for scene sd, computed once per key and shared."""
    if key not in _ORACLE:
        osc = oracle.OracleScene(sd, W, H)
        O, D, tmax = rays(sd)
        avg, rgb8, _, st = osc.render(W, H, spp=SPP, bounces=B)
        _ORACLE[key] = dict(primary=osc.primary_hits(W, H), closest=osc.intersect(O, D), occluded=osc.occluded(O, D, tmax),
                            avg=avg, rgb8=rgb8, totals=(int(st.segments), int(st.shadow_rays)))
    return _ORACLE[key]


def gpu_results(c, sd):
    """The same from a context that holds the scene (camera and accumulation reset first)."""
    c.set_camera(prt.Camera(sd.cam_pos, sd.cam_target, F32(W) / F32(H)))
    c.reset_accumulation(full=True)
    O, D, tmax = rays(sd)
    hits, _ = c.trace_primary(W, H)
    cl = c.intersect(O, D)
    avg, rgb8, st = c.render(W, H, SPP, B)
    return dict(primary=tuple(hits[k] for k in ("t", "u", "v", "prim", "inst")),
                closest=tuple(cl[k] for k in ("t", "u", "v", "prim", "inst")), occluded=c.occluded(O, D, tmax),
                avg=avg, rgb8=rgb8, totals=(int(st.segments), int(st.shadow_rays)))


def assert_same(got, want, what=""):
    for k in ("primary", "closest"):
        for i, f in enumerate(("t", "u", "v", "prim", "inst")):
            assert np.array_equal(got[k][i], want[k][i]), (what, k, f)
    assert np.array_equal(got["occluded"], want["occluded"]), what
    assert np.array_equal(got["avg"], want["avg"]), (what, float(np.mean(np.all(got["avg"] == want["avg"], axis=1))))
    assert np.array_equal(got["rgb8"], want["rgb8"]), what
    assert got["totals"] == want["totals"], what


@contextlib.contextmanager
def context(builder=None, sd=None, group=None):
    c = prt.Context(0, group=group)
    try:
        if builder is not None:
            c.set_bvh_builder(builder)
        if sd is not None:
            gpu_scene(c, sd, W, H)
        yield c
    finally:
        c.close()


def blas_bytes(c, n):
    return [(c.read_blas(i).tobytes(), c.read_blas_tris(i).tobytes()) for i in range(n)]


def skinned_equals_updated(s, pose, builder=None, key=None, device=False):
    """Context A: set_mesh_skin + skin_mesh(M).  Context B: update_mesh(R).  The queries and the frame are equal, and
    equal the oracle's over R.  The BLAS bytes (prt_read_blas, prt_read_blas_tris) of every mesh: A's after skin_mesh
    equal A's own after a following update_mesh(R) -- the contract's "same context", the same tree -- for every
    builder, and equal B's for the host builders.  (Two contexts' device builds are one canonical tree, but their
    atomic counters place the nodes and record ranges differently from build to build -- tests/
    test_gpu_builder_trees.py test_two_builds_give_one_tree -- so their raw bytes cannot be compared.)  Returns A's
    results and the bind pose's."""
    sd1 = s.scene(pose)
    with context(builder, s.sd) as a, context(builder, s.sd) as b:
        before = gpu_results(a, s.sd)
        a.set_mesh_skin(s.mi, s.skin)
        if device:
            import torch
            t = torch.from_numpy(np.ascontiguousarray(s.M[pose], F32)).cuda()
            torch.cuda.synchronize()
            a.skin_mesh(s.mi, t, device=True)
        else:
            a.skin_mesh(s.mi, s.M[pose])
        b.update_mesh(s.mi, s.R(pose))
        n = len(s.sd.meshes)
        skinned = blas_bytes(a, n)
        if builder in (None, _lib.BUILDER_HOST_SAH, _lib.BUILDER_HOST_SBVH):
            assert skinned == blas_bytes(b, n)
        got = gpu_results(a, sd1)
        assert_same(got, gpu_results(b, sd1), "update_mesh(R)")
        a.update_mesh(s.mi, s.R(pose))
        assert blas_bytes(a, n) == skinned
    if key is not None:
        assert_same(got, oracle_results(key, sd1), "oracle")
    return got, before


# ---- equals update_mesh(R) and the oracle, for every builder

@pytest.mark.parametrize("builder", sorted(BUILDERS))
@pytest.mark.parametrize("name", ["small", "multi", "two", "field"])
def test_skin_equals_update_and_oracle(name, builder):
    s = setup(name)
    got, before = skinned_equals_updated(s, "m1", BUILDERS[builder], key=(name, 3, "m1"))
    assert 0 < np.count_nonzero(got["primary"][0] < 1e30)
    assert not np.array_equal(before["avg"], got["avg"])  # the pose shows
    if name == "two":
        inst = got["primary"][4][got["primary"][0] < 1e30]
        assert (inst == 0).any() and (inst == 1).any()  # both meshes are seen


@pytest.mark.parametrize("builder", ["host_sah", "gpu_ploc"])
def test_pose_sequence_there_and_back_is_byte_identical(builder):
    s = setup("two")
    n = len(s.sd.meshes)
    with context(BUILDERS[builder], s.sd) as c:
        bind = blas_bytes(c, n)
        c.set_mesh_skin(s.mi, s.skin)
        c.skin_mesh(s.mi, s.M["m1"])
        first = blas_bytes(c, n)
        r1 = gpu_results(c, s.scene("m1"))
        c.skin_mesh(s.mi, s.M["m2"])
        second = blas_bytes(c, n)
        c.skin_mesh(s.mi, s.M["m1"])
        assert blas_bytes(c, n) == first
        assert_same(gpu_results(c, s.scene("m1")), r1, "M1 again")
    assert first[s.mi] != bind[s.mi] and second[s.mi] != first[s.mi]
    assert first[0] == bind[0] and second[0] == bind[0]  # the other mesh is untouched


# ---- joint counts: one, and two beyond the LDS staging

@pytest.mark.parametrize("J", [1, 300, 65536])
def test_joint_counts(J):
    s = setup("small", J)
    used = np.unique(s.skin.joints)
    assert used.min() == 0 and used.max() == J - 1 and len(used) <= 8  # most joints are unused
    skinned_equals_updated(s, "m1", key=("small", J, "m1"))


def test_collapsed_triangles_render_as_update_mesh_does():
    s = setup("small")
    z = ~s.R("flat").face_normals.reshape(-1, 3).any(axis=1)
    assert 0 < z.sum() < z.size and np.array_equal(s.R("flat").fixed_normals.reshape(-1, 4)[3 * np.flatnonzero(z)[0], :3],
                                                   [0, 1, 0])
    skinned_equals_updated(s, "flat", key=("small", 3, "flat"))


def test_collapse_into_the_origin_renders_as_update_mesh_does():
    """The pose that could not be tested before a node visit skipped unoccupied slots (see COLLAPSE_POINT): what
    follows joint 0 alone collapses into the point the camera looks at."""
    s = setup("small")
    R = s.R("flat0")
    z = ~R.face_normals.reshape(-1, 3).any(axis=1)
    assert 0 < z.sum() < z.size
    at_origin = ~np.asarray(R.triangles, F32).reshape(-1, 3, 4)[:, :, :3].any(axis=(1, 2))
    assert at_origin.sum() >= 100 and not (at_origin & ~z).any()  # whole triangles sit at the origin, exactly
    skinned_equals_updated(s, "flat0", key=("small", 3, "flat0"))


def test_device_matrices_give_the_same_bytes_and_frames():
    """The matrices as a torch device tensor with PRT_IN_DEVICE: the bytes and frames of update_mesh(R) and the oracle,
    and the bytes host matrices give (HOST_SAH, whose trees two contexts can compare)."""
    import torch
    skinned_equals_updated(setup("multi"), "m2", key=("multi", 3, "m2"), device=True)
    skinned_equals_updated(setup("small", 300), "m2", device=True)
    s = setup("two")
    with context(None, s.sd) as h, context(None, s.sd) as d:
        for c in (h, d):
            c.set_mesh_skin(s.mi, s.skin)
        t = torch.from_numpy(np.ascontiguousarray(s.M["m2"], F32)).cuda()
        torch.cuda.synchronize()
        h.skin_mesh(s.mi, s.M["m2"])
        d.skin_mesh(s.mi, t, device=True)
        assert blas_bytes(h, 2) == blas_bytes(d, 2)


# ---- everything downstream follows

@pytest.mark.parametrize("name,tlas", [("field", None), ("multi", "1")])
def test_instance_boxes_and_instance_bvh_follow(monkeypatch, name, tlas):
    """Every joint doubles the mesh's extent: were the instances' world boxes (and the instance BVH over them) not
    refreshed, rays would miss what now sticks out of the old boxes.  Then back to the bind pose."""
    if tlas:
        monkeypatch.setenv("PRT_TLAS", tlas)
    s = setup(name)
    ident = np.tile(skin_ref.rigid(), (3, 1))
    with context(None, s.sd) as c:
        gpu_results(c, s.sd)
        assert c.scene_info().tlas_depth > 0
        c.set_mesh_skin(s.mi, s.skin)
        c.skin_mesh(s.mi, s.M["x2"])
        got = gpu_results(c, s.scene("x2"))
        c.skin_mesh(s.mi, ident)  # and back, through the worker thread's rebuild
        back = gpu_results(c, s.sd)
    assert_same(got, oracle_results((name, 3, "x2"), s.scene("x2")), "oracle x2")
    s.M["ident"] = ident
    assert_same(back, oracle_results((name, 3, "ident"), s.scene("ident")), "oracle, identity pose")


def test_kept_primary_hits_and_light_visibility_go_stale(monkeypatch):
    """A static camera, three calls (primary hits kept, light visibility learned and used), then a pose: the next
    frames equal those of a context with PRT_PRIMARY_REUSE=0, and the dense primary pass ran again."""
    s = setup("multi")

    def call(c, k):
        a, r, st = c.render(W, H, 4, B, frame_index=2 * k)
        return a, r, (int(st.segments), int(st.shadow_rays))

    with context(None, s.sd) as c, context(None, s.sd) as ref:
        for x in (c, ref):
            x.set_mesh_skin(s.mi, s.skin)
        for k in range(3):
            got = call(c, k)
            monkeypatch.setenv("PRT_PRIMARY_REUSE", "0")
            want = call(ref, k)
            monkeypatch.delenv("PRT_PRIMARY_REUSE")
        assert np.array_equal(got[0], want[0])
        assert c.primary_rays() == (W * H, W * H * 5) and c.shadow_reuse() > 0
        c.skin_mesh(s.mi, s.M["m1"])
        ref.skin_mesh(s.mi, s.M["m1"])
        for k in range(3, 6):
            got = call(c, k)
            monkeypatch.setenv("PRT_PRIMARY_REUSE", "0")
            want = call(ref, k)
            monkeypatch.delenv("PRT_PRIMARY_REUSE")
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], k
            assert c.primary_rays() == (2 * W * H, W * H * (5 + 2 * (k - 3) + 1)), k
        assert ref.primary_rays() == (0, 0)


def test_deform_chain_follows():
    """skin_mesh(M1), snapshot_mesh, skin_mesh(M2), render_aov_deform: all four outputs equal those of a context driven
    by update_mesh(R1), snapshot_mesh, update_mesh(R2)."""
    s = setup("two")
    with context(None, s.sd) as a, context(None, s.sd) as b:
        a.set_mesh_skin(s.mi, s.skin)
        a.skin_mesh(s.mi, s.M["m1"])
        a.snapshot_mesh(s.mi)
        a.skin_mesh(s.mi, s.M["m2"])
        b.update_mesh(s.mi, s.R("m1"))
        b.snapshot_mesh(s.mi)
        b.update_mesh(s.mi, s.R("m2"))
        got, want = a.render_aov_deform(W, H), b.render_aov_deform(W, H)
    for x, y in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
    off = got[3]
    assert np.any(off[:, 3] == 1) and np.any(off[off[:, 3] == 1, :3] != 0) and np.any(off[:, 3] == 0)


# ---- frames in flight

def _flight_frames(c, s, poses, stream, n):
    import torch
    outs = []
    inst = [(m, np.array(T, F32)) for m, T in s.sd.instances]
    for f in range(n):
        c.skin_mesh(s.mi, poses[f % len(poses)])
        moved = []
        for k, (m, T) in enumerate(inst):
            T = T.copy()
            if k > 0:
                T[0, 3] += F32(0.05 * ((f % 3) - 1))
                T[1, 3] += F32(0.02 * f)
            moved.append((m, T))
        c.set_instances(moved)
        with torch.cuda.stream(stream):
            avg = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        c.render(W, H, 2, B, frame_index=f, avg=avg.data_ptr(), rgb8=rgb.data_ptr(), device_out=True, stats=False)
        outs.append((avg, rgb))
    c.finish()
    stream.synchronize()
    torch.cuda.synchronize()
    return [(a.cpu().numpy(), r.cpu().numpy()) for a, r in outs], c.ray_totals(reset=True)


def test_frames_in_flight_with_a_pose_before_every_frame():
    import torch
    s = setup("multi")
    poses = [s.M["m1"], s.M["m2"], np.tile(skin_ref.rigid(), (3, 1))]
    stream = torch.cuda.Stream()
    res = []
    for fl in (1, 4):
        with context(None) as c:
            c.set_stream(stream.cuda_stream)
            gpu_scene(c, s.sd, W, H)
            c.set_mesh_skin(s.mi, s.skin)
            c.set_frames_in_flight(fl)
            res.append(_flight_frames(c, s, poses, stream, 7))
    (f1, t1), (f2, t2) = res
    for k, ((a1, r1), (a2, r2)) in enumerate(zip(f1, f2)):
        assert np.array_equal(a1, a2) and np.array_equal(r1, r2), k
    assert t1 == t2
    assert not np.array_equal(f1[0][1], f1[1][1])


# ---- refusals, and the life of a binding

def _bind(c, index, skin, **over):
    """prt_set_mesh_skin through the raw ABI with fields overridden"""
    a = dict(P=np.ascontiguousarray(skin.positions, F32), N=np.ascontiguousarray(skin.normals, F32),
             I=np.ascontiguousarray(skin.indices, np.int32), J=np.ascontiguousarray(skin.joints, np.uint16),
             W=np.ascontiguousarray(skin.weights, F32))
    a.update({k: v for k, v in over.items() if k in a})
    st = _lib.Skin(over.get("V", a["P"].size // 3), over.get("T", a["I"].size // 3), over.get("joints", skin.joint_count),
                   a["P"].ctypes.data, a["N"].ctypes.data, a["I"].ctypes.data, a["J"].ctypes.data, a["W"].ctypes.data)
    return c.L.prt_set_mesh_skin(c.h, index, _lib.C.byref(st))


def test_refusals_change_nothing():
    s = setup("two")
    V, T = s.skin.positions.shape[0], s.skin.indices.size // 3
    M = np.ascontiguousarray(s.M["m1"], F32)
    with context(None, s.sd) as c:
        L, h = c.L, c.h
        assert L.prt_skin_mesh(h, s.mi, M.ctypes.data, 3, 0) == -5 and b"no skin" in L.prt_last_error()  # no binding
        want = gpu_results(c, s.sd)
        assert _bind(c, s.mi, s.skin, V=V - 1) == -1 and _bind(c, s.mi, s.skin, T=T + 1) == -1
        assert _bind(c, 0, s.skin) == -1                       # another mesh's counts
        assert _bind(c, 2, s.skin) == -1 and _bind(c, -1, s.skin) == -1
        assert _bind(c, s.mi, s.skin, joints=0) == -1 and _bind(c, s.mi, s.skin, joints=65537) == -1
        bad_j = np.array(s.skin.joints, np.uint16)
        bad_j[V // 2, 3] = 3
        assert _bind(c, s.mi, s.skin, J=bad_j) == -1 and b"joint out of range" in L.prt_last_error()
        bad_i = np.array(s.skin.indices, np.int32)
        bad_i[5] = V
        assert _bind(c, s.mi, s.skin, I=bad_i) == -1 and b"index out of range" in L.prt_last_error()
        bad_i[5] = -1
        assert _bind(c, s.mi, s.skin, I=bad_i) == -1
        assert L.prt_set_mesh_skin(h, s.mi, _lib.C.byref(_lib.Skin(V, T, 3))) == -1  # no arrays
        assert L.prt_skin_mesh(h, s.mi, M.ctypes.data, 3, 0) == -5  # still no binding
        assert _bind(c, s.mi, s.skin) == 0
        assert L.prt_skin_mesh(h, s.mi, M.ctypes.data, 2, 0) == -1 and L.prt_skin_mesh(h, s.mi, M.ctypes.data, 4, 0) == -1
        assert L.prt_skin_mesh(h, s.mi, None, 3, 0) == -1
        assert L.prt_skin_mesh(h, s.mi, M.ctypes.data, 3, 2) == -1  # unknown flag
        assert L.prt_skin_mesh(h, 2, M.ctypes.data, 3, 0) == -1 and L.prt_skin_mesh(h, -1, M.ctypes.data, 3, 0) == -1
        assert L.prt_skin_mesh(h, 0, M.ctypes.data, 3, 0) == -5     # the other mesh has no binding
        assert_same(gpu_results(c, s.sd), want, "after the refusals")
        # a refused binding leaves the accepted one in place
        assert _bind(c, s.mi, s.skin, J=bad_j) == -1
        c.skin_mesh(s.mi, s.M["m1"])
        assert_same(gpu_results(c, s.scene("m1")), oracle_results(("two", 3, "m1"), s.scene("m1")), "oracle")
    with context() as e:
        assert _bind(e, 0, s.skin) == -5 and e.L.prt_skin_mesh(e.h, 0, M.ctypes.data, 3, 0) == -5  # no scene
        assert e.L.prt_set_mesh_skin(e.h, 0, None) == -5


def test_set_meshes_drops_the_binding_and_none_removes_it():
    s = setup("small")
    with context(None, s.sd) as c:
        c.set_mesh_skin(s.mi, s.skin)
        c.skin_mesh(s.mi, s.M["m1"])
        c.update_mesh(s.mi, s.sd.meshes[s.mi])  # leaves the binding alone
        c.skin_mesh(s.mi, s.M["m1"])
        gpu_scene(c, s.sd, W, H)                # prt_set_meshes
        with pytest.raises(_lib.PrtError, match="prt error -5"):
            c.skin_mesh(s.mi, s.M["m1"])
        assert_same(gpu_results(c, s.sd), oracle_results(("small", 3, "bind"), s.sd), "the bind pose")
        c.set_mesh_skin(s.mi, s.skin)
        c.set_mesh_skin(s.mi, None)
        with pytest.raises(_lib.PrtError, match="prt error -5"):
            c.skin_mesh(s.mi, s.M["m1"])
        c.set_mesh_skin(s.mi, None)             # removing what is not there is no error
        # a scene that carries its skin and pose: set_scene binds and poses
        sc = prt.Scene.from_data(s.sd)
        sc.set_skin(s.mi, s.skin)
        sc.skin_model(s.mi, s.M["m1"])
        c.set_scene(sc)
        assert_same(gpu_results(c, s.scene("m1")), oracle_results(("small", 3, "m1"), s.scene("m1")), "set_scene")


def test_local_group():
    """Host matrices reach every member of a two-member local group on one GPU (the oracle's frame); device matrices
    are PRT_ERR_UNSUPPORTED there."""
    import torch
    s = setup("multi")
    sd1 = s.scene("m1")
    with context(None, s.sd, group=[0, 0]) as g:
        g.set_mesh_skin(s.mi, s.skin)
        t = torch.from_numpy(np.ascontiguousarray(s.M["m1"], F32)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(_lib.PrtError, match="prt error -6"):
            g.skin_mesh(s.mi, t, device=True)
        g.skin_mesh(s.mi, s.M["m1"])
        g.set_camera(prt.Camera(s.sd.cam_pos, s.sd.cam_target, F32(W) / F32(H)))
        g.reset_accumulation(full=True)
        avg, rgb8, st = g.render(W, H, SPP, B)
    want = oracle_results(("multi", 3, "m1"), sd1)
    assert np.array_equal(avg, want["avg"]) and np.array_equal(rgb8, want["rgb8"])
    assert (int(st.segments), int(st.shadow_rays)) == want["totals"]


def test_renderer_skin_model():
    """The mirror's convenience: Renderer.SetSkin binds, Renderer.SkinModel poses and restarts the accumulation; the
    next Tick is the oracle's frame of R."""
    s = setup("multi")
    R = prt.Renderer(prt.Scene.from_data(s.sd), prt.Camera(s.sd.cam_pos, s.sd.cam_target, F32(W) / F32(H)), W, H)
    try:
        R.bounces = B
        R.Tick()
        R.SetSkin(s.mi, s.skin)
        R.SkinModel(s.mi, s.M["m1"])
        R.frame = 0
        R.Tick()
        want = oracle_results(("multi", 3, "m1"), s.scene("m1"))
        assert np.array_equal(R.average, want["avg"]) and np.array_equal(R.screen, want["rgb8"])
        assert R.scene.models[s.mi] is s.sd.meshes[s.mi] and np.array_equal(R.scene.poses[s.mi], s.M["m1"])
    finally:
        R.ctx.close()
