#!/usr/bin/env python3
"""prt_rebuild_mesh and prt_blas_cost on C4 (1M triangles), one MI355X, one process (DESIGN.md 8,
profiles/rebuild_mesh_c4.txt):
    python3 scripts/rebuild_time.py time     device time (torch events on the context stream) and host time of the call:
                                             prt_rebuild_mesh with device arrays for both builders and with host
                                             arrays (median / min / max of 5 after one warm-up), beside
                                             prt_set_meshes' build_ms with GPU_PLOC and prt_update_mesh (20 after 5);
                                             prt_blas_cost (20 after 5) with the bytes of the nodes it reads against
                                             k_wave_init's streaming rate
    python3 scripts/rebuild_time.py frames   the height field carried far from its build pose (tests/deform.py
                                             sine_twist, amplitude 1, 0.5 rad of twist per unit): ms per frame
                                             (1920x1080, 4 spp, depth 4, two frames in flight, the camera moved before
                                             every call) on the refitted GPU_PLOC tree against the tree
                                             prt_rebuild_mesh leaves, interleaved, three runs each, with prt_blas_cost
                                             of both
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physically-based-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import deform  # noqa: E402
import prt  # noqa: E402
from prt import _lib, scenes  # noqa: E402

W, H, SPP, BOUNCES = 1920, 1080, 4, 4
WAVE_INIT_TBS = 6.1  # k_wave_init on C4: 300 MB written in 49.5 us
FAR = dict(amp=1.0, twist=0.5)
BUILDERS = (("GPU_PLOC", _lib.BUILDER_GPU_PLOC), ("GPU_LBVH", _lib.BUILDER_GPU_LBVH))


class DeviceMesh:
    def __init__(self, m):
        for n in ("triangles", "fixed_normals", "fixed_uvs", "vertices", "face_normals"):
            setattr(self, n, torch.from_numpy(np.ascontiguousarray(getattr(m, n), np.float32)).cuda())
        self.indices = torch.from_numpy(np.ascontiguousarray(m.indices, np.int32)).cuda()
        self.albedo, self.normal, self.metalness, self.emission = m.albedo, m.normal, m.metalness, m.emission
        torch.cuda.synchronize()


def stats(v):
    return f"median {np.median(v):.3f}  min {min(v):.3f}  max {max(v):.3f}"


def new_context(sd, builder):
    c = prt.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.set_bvh_builder(builder)
    c.set_scene(prt.Scene.from_data(sd))
    return c


def timed(fn, n, warm):
    dev, host = [], []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            dev.append(e0.elapsed_time(e1))
            host.append((t1 - t0) * 1e3)
    return dev, host


def part_time():
    sd = scenes.config_c4()
    m0 = sd.meshes[0]
    m1 = deform.sine_twist(m0, **FAR)
    c = new_context(sd, _lib.BUILDER_GPU_PLOC)
    info = c.scene_info()
    print(f"C4: {m0.tri_count} triangles, GPU_PLOC tree of {info.blas_nodes} nodes, depth {info.max_depth} "
          f"(prt_set_meshes build_ms {info.build_ms:.1f})")
    d1 = DeviceMesh(m1)
    dev, host = timed(lambda: c.update_mesh(0, d1, device=True), 20, 5)
    print(f"prt_update_mesh, device arrays: device ms {stats(dev)}; host ms of the call {stats(host)}")
    for name, b in BUILDERS:
        dev, host = timed(lambda: c.rebuild_mesh(0, d1, device=True, builder=b), 5, 1)
        info = c.scene_info()
        print(f"prt_rebuild_mesh {name}, device arrays: device ms {stats(dev)}; host ms of the call {stats(host)}; "
              f"{info.blas_nodes} nodes, depth {info.max_depth}")
    dev, host = timed(lambda: c.rebuild_mesh(0, m1, builder=_lib.BUILDER_GPU_PLOC), 3, 1)
    print(f"prt_rebuild_mesh GPU_PLOC, host arrays: device ms {stats(dev)}; host ms of the call {stats(host)}")
    N = int(c.scene_info().blas_nodes)
    costs = []
    dev, host = timed(lambda: costs.append(c.blas_cost(0)), 20, 5)
    assert len(set(costs)) == 1
    best = float(np.median(dev))
    print(f"prt_blas_cost over {N} nodes ({80 * N / 1e6:.1f} MB): device ms {stats(dev)}; host ms of the call "
          f"{stats(host)}; {80 * N / best / 1e9:.3f} TB/s at the median, {80 * N / best / 1e9 / WAVE_INIT_TBS * 100:.0f} % of "
          f"k_wave_init's {WAVE_INIT_TBS} TB/s; cost {costs[0]:.6f}, the same bits from {len(costs)} calls")
    c.close()


def part_frames(runs=3, steps=20, warm=5):
    sd = scenes.config_c4()
    m0 = sd.meshes[0]
    m1 = deform.sine_twist(m0, **FAR)
    aspect = np.float32(W) / np.float32(H)
    cams = [prt.Camera(np.asarray(sd.cam_pos, np.float32) + np.float32(0.002 * i) * np.asarray([1, 0, 1], np.float32),
                       sd.cam_target, aspect) for i in range(64)]
    avg = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    rgb = torch.zeros(H * W, dtype=torch.int32, device="cuda")

    def frames(c, n, first):
        for i in range(n):
            c.set_camera(cams[(first + i) % len(cams)])
            c.render(W, H, SPP, BOUNCES, frame_index=2 * (first + i), avg=avg.data_ptr(), rgb8=rgb.data_ptr(),
                     device_out=True, stats=False)
        torch.cuda.synchronize()

    trees = {"refitted": new_context(sd, _lib.BUILDER_GPU_PLOC), "rebuilt": new_context(sd, _lib.BUILDER_GPU_PLOC)}
    built = trees["refitted"].blas_cost(0)
    trees["refitted"].update_mesh(0, m1)
    trees["rebuilt"].rebuild_mesh(0, m1, builder=_lib.BUILDER_GPU_PLOC)
    cost = {k: c.blas_cost(0) for k, c in trees.items()}
    print(f"prt_blas_cost: as built {built:.4f}; at the far pose refitted {cost['refitted']:.4f}, rebuilt "
          f"{cost['rebuilt']:.4f}, ratio {cost['refitted'] / cost['rebuilt']:.3f}")
    ms = {k: [] for k in trees}
    for c in trees.values():
        c.set_frames_in_flight(2)
    for _ in range(runs):
        for k, c in trees.items():
            frames(c, warm, 1)
            t0 = time.perf_counter()
            frames(c, steps, 1 + warm)
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    print("ms per frame, camera moved before every call; median [min .. max] of three interleaved runs: " + "; ".join(
        f"{k} {np.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}]" for k, v in ms.items()))
    print(f"refitted / rebuilt = {np.median(ms['refitted']) / np.median(ms['rebuilt']):.3f}")
    for c in trees.values():
        c.close()


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "time"
    if part == "time":
        part_time()
    elif part == "frames":
        part_frames()
    else:
        sys.exit(__doc__)
