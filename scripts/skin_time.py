#!/usr/bin/env python3
"""prt_skin_mesh on C4 (1M triangles, 64 joints), one MI355X, one process (profiles/skin_mesh_c4.txt):
    python3 scripts/skin_time.py time      device time (torch events on the context stream; median / min / max of 20
                                           after 5 warm-up, the three ways interleaved) of
                                             (a) prt_skin_mesh (host matrices; device matrices beside it),
                                             (b) prt_update_mesh(PRT_IN_DEVICE) of precomputed arrays: the refit alone,
                                             (c) the same skinning and derivation written in torch on the device,
                                                 followed by (b): what a user without prt_skin_mesh has to do,
                                           the host time of each call, and the kernels' compulsory bytes against
                                           k_wave_init's streaming rate.  Exits non-zero unless (a) <= (c).
    python3 scripts/skin_time.py kernels   20 prt_skin_mesh calls and nothing else after the set-up, for a run under
                                           rocprofv3 --kernel-trace --stats (the per-kernel durations)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physically-based-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import skin_ref  # noqa: E402
import prt  # noqa: E402
from prt import _lib, scenes  # noqa: E402

J = 64
WAVE_INIT_TBS = 6.1  # k_wave_init on C4: 300 MB written in 49.5 us


class DeviceMesh:
    def __init__(self, m):
        for n in ("triangles", "fixed_normals", "fixed_uvs", "vertices", "face_normals"):
            setattr(self, n, torch.from_numpy(np.ascontiguousarray(getattr(m, n), np.float32)).cuda())
        self.indices = torch.from_numpy(np.ascontiguousarray(m.indices, np.int32)).cuda()
        self.albedo, self.normal, self.metalness, self.emission = m.albedo, m.normal, m.metalness, m.emission
        torch.cuda.synchronize()


class TorchSkin:
    """The definition in torch on the device, writing into a DeviceMesh's arrays (what a user's stop-gap looks like:
    elementwise kernels and gathers; no claim of bit-exactness)."""

    def __init__(self, skin, out):
        dev = "cuda"
        self.P = torch.from_numpy(np.ascontiguousarray(skin.positions, np.float32)).to(dev)
        self.N = torch.from_numpy(np.ascontiguousarray(skin.normals, np.float32)).to(dev)
        self.j = torch.from_numpy(np.ascontiguousarray(skin.joints, np.int64)).to(dev)
        self.w = torch.from_numpy(np.ascontiguousarray(skin.weights, np.float32)).to(dev)
        self.idx = torch.from_numpy(np.ascontiguousarray(skin.indices, np.int64)).to(dev)
        self.out = out
        self.up = torch.tensor([0.0, 1.0, 0.0], device=dev)

    def __call__(self, M):
        M = M.reshape(-1, 12)
        B = (self.w[:, 0:1] * M[self.j[:, 0]] + self.w[:, 1:2] * M[self.j[:, 1]] + self.w[:, 2:3] * M[self.j[:, 2]]
             + self.w[:, 3:4] * M[self.j[:, 3]]).reshape(-1, 3, 4)
        Po = (B[:, :, :3] * self.P[:, None, :]).sum(-1) + B[:, :, 3]
        n = (B[:, :, :3] * self.N[:, None, :]).sum(-1)
        No = n * torch.rsqrt((n * n).sum(-1, keepdim=True))
        No = torch.where(torch.isfinite(No).all(-1, keepdim=True), No, self.up)
        o = self.out
        o.vertices.copy_(Po.reshape(-1))
        tri = o.triangles.view(-1, 4)
        tri[:, :3] = Po[self.idx]
        o.fixed_normals.view(-1, 4)[:, :3] = No[self.idx]
        c = tri[:, :3].reshape(-1, 3, 3)
        x = torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        fn = x * torch.rsqrt((x * x).sum(-1, keepdim=True))
        o.face_normals.copy_(torch.where(torch.isfinite(fn).all(-1, keepdim=True), fn, torch.zeros_like(fn)).reshape(-1))


def stats(v):
    return f"median {np.median(v):.3f}  min {min(v):.3f}  max {max(v):.3f}"


def set_up():
    sd = scenes.config_c4()
    mesh = sd.meshes[0]
    j, w = skin_ref.smooth_weights(mesh.vertices.reshape(-1, 3), J)
    skin = scenes.Skin.from_mesh(mesh, j, w, J)
    poses = [skin_ref.pose(J, seed=k, amount=0.05) for k in (1, 2)]
    c = prt.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.set_bvh_builder(_lib.BUILDER_HOST_SAH)
    c.set_scene(prt.Scene.from_data(sd))
    c.set_mesh_skin(0, skin)
    return sd, mesh, skin, poses, c


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (t1 - t0) * 1e3


def part_time(n=20, warm=5):
    sd, mesh, skin, poses, c = set_up()
    T, V = mesh.tri_count, mesh.vertices.size // 3
    info = c.scene_info()
    N = int(info.blas_nodes)
    print(f"C4: {T} triangles, {V} vertices, {J} joints, HOST_SAH tree of {N} nodes, depth {info.max_depth}")
    dposes = [torch.from_numpy(p).cuda() for p in poses]
    pre = DeviceMesh(skin_ref.skin_mesh(mesh, skin, poses[0]))  # (b): precomputed arrays
    out = DeviceMesh(mesh)                                      # (c): the arrays the torch skinning writes
    tskin = TorchSkin(skin, out)
    tskin(dposes[0])
    torch.cuda.synchronize()
    worst = max(float((getattr(out, k) - getattr(pre, k)).abs().max()) for k in ("triangles", "fixed_normals", "vertices"))
    print(f"the torch skinning against skin_ref, largest difference of a coordinate or normal component: {worst:.2e}")
    ways = {
        "(a) prt_skin_mesh, host matrices": lambda k: c.skin_mesh(0, poses[k % 2]),
        "(a') prt_skin_mesh, device matrices": lambda k: c.skin_mesh(0, dposes[k % 2], device=True),
        "(b) prt_update_mesh(PRT_IN_DEVICE), precomputed arrays": lambda k: c.update_mesh(0, pre, device=True),
        "(c) torch skinning on the device + (b)": lambda k: (tskin(dposes[k % 2]), c.update_mesh(0, out, device=True)),
    }
    dev = {k: [] for k in ways}
    host = {k: [] for k in ways}
    for i in range(warm + n):
        for name, fn in ways.items():
            d, h = timed(lambda: fn(i))
            if i >= warm:
                dev[name].append(d)
                host[name].append(h)
    for name in ways:
        print(f"{name}: device ms {stats(dev[name])}; host ms of the call {stats(host[name])}")
    a, b, cc = (float(np.median(dev[k])) for k in list(ways)[:1] + list(ways)[2:])
    print(f"(a) / (b) = {a / b:.2f}; (a) / (c) = {a / cc:.2f}")
    # compulsory bytes.  k_skin_vertices: 24 B bind pose + 8 B joints + 16 B weights read, 2 x 16 B written per vertex
    # (the 64 matrices, 3 KiB, once per block).  k_skin_prims: 12 B indices + 48 B of its ShadeTri read, 48 B fat
    # triangle + 112 B ShadeTri written per primitive, and the 32 B per vertex of the skinned vertices read once.
    # Then the refit's record pass without its ShadeTri kernel and its node pass, as scripts/mesh_update_time.py.
    vert = V * (24 + 8 + 16 + 32)
    prim = T * (12 + 48 + 48 + 112) + V * 32
    rec = T * (48 + 48 + 48)
    node = N * (80 + 80 + 24 + 24) + T * 48
    total = vert + prim + rec + node
    print(f"compulsory bytes: k_skin_vertices {vert / 1e6:.1f} MB, k_skin_prims {prim / 1e6:.1f} MB, k_refit_tris "
          f"{rec / 1e6:.1f} MB, node pass {node / 1e6:.1f} MB; at k_wave_init's {WAVE_INIT_TBS} TB/s: "
          f"{total / WAVE_INIT_TBS / 1e9:.3f} ms; prt_skin_mesh reaches {total / WAVE_INIT_TBS / 1e9 / a * 100:.0f} % of that rate")
    c.close()
    if not a <= cc:
        sys.exit(f"prt_skin_mesh ({a:.3f} ms) is slower than the torch route ({cc:.3f} ms)")


def part_kernels():
    _, _, _, poses, c = set_up()
    for k in range(20):
        c.skin_mesh(0, poses[k % 2])
    torch.cuda.synchronize()
    c.close()


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "time"
    if part == "time":
        part_time()
    elif part == "kernels":
        part_kernels()
    else:
        sys.exit(__doc__)
