#!/usr/bin/env python3
"""prt_update_mesh on C4 (1M triangles), one MI355X, one process (profiles/mesh_update_c4.txt):
    python3 scripts/mesh_update_time.py update    the update's device time (torch events on the context stream, device
                                                  arrays, median / min / max of 20 after 5 warm-up), the host time
                                                  of the call with its 28-byte readback, the same with host arrays, prt_set_meshes with
                                                  GPU_PLOC re-measured in the same process, and the pass's compulsory
                                                  bytes against k_wave_init's streaming rate
    python3 scripts/mesh_update_time.py kernels   20 updates and nothing else after the set-up, for a run under
                                                  rocprofv3 --kernel-trace --stats (the per-kernel durations)
    python3 scripts/mesh_update_time.py quality   ms per frame (1920x1080, 4 spp, depth 4, two frames in flight, the
                                                  camera moved before every call as scripts/moving_camera.py) on the
                                                  height field displaced by a travelling sine of three amplitudes, on
                                                  the refitted HOST_SAH tree, a fresh HOST_SAH tree and a fresh
                                                  GPU_PLOC tree over the same vertices; interleaved, three runs each
"""
import dataclasses
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


def time_updates(c, mesh, device, n=20, warm=5):
    dev, host = [], []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        c.update_mesh(0, mesh, device=device)
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            dev.append(e0.elapsed_time(e1))
            host.append((t1 - t0) * 1e3)
    return dev, host


def part_update(kernels_only=False):
    sd = scenes.config_c4()
    m0 = sd.meshes[0]
    m1 = deform.travelling_sine(m0, 0.05, 0.7)
    T, V = m0.tri_count, m0.vertices.size // 3
    c = new_context(sd, _lib.BUILDER_HOST_SAH)
    info = c.scene_info()
    N = int(info.blas_nodes)
    d1 = DeviceMesh(m1)
    if kernels_only:
        for _ in range(20):
            c.update_mesh(0, d1, device=True)
        torch.cuda.synchronize()
        c.close()
        return
    print(f"C4: {T} triangles, {V} vertices, HOST_SAH tree of {N} nodes, depth {info.max_depth} "
          f"(prt_set_meshes {info.build_ms:.1f} ms)")
    dev, host = time_updates(c, d1, True)
    print(f"prt_update_mesh, device arrays: device ms {stats(dev)}; host ms of the call (with the 28-byte readback) "
          f"{stats(host)}")
    best = float(np.median(dev))
    dev, host = time_updates(c, m1, False, n=10, warm=2)
    print(f"prt_update_mesh, host arrays (pinned staging, {220 * T + 12 * V >> 20} MiB): device ms {stats(dev)}; host ms "
          f"of the call {stats(host)}")
    # compulsory bytes: records read + written, the triangle array read by both passes, the shading inputs read once,
    # ShadeTri's 112 written bytes, nodes read + written, boxes written and read once each
    rec = T * (48 + 48 + 48) + T * (112 + 48 + 24 + 12 + 12) + V * 12
    node = N * (80 + 80 + 24 + 24) + T * 48
    print(f"compulsory bytes: record pass {rec / 1e6:.1f} MB, node pass {node / 1e6:.1f} MB; at k_wave_init's "
          f"{WAVE_INIT_TBS} TB/s: {(rec + node) / WAVE_INIT_TBS / 1e9:.3f} ms; the update reaches "
          f"{(rec + node) / WAVE_INIT_TBS / 1e9 / best * 100:.0f} % of that rate")
    c.close()
    p = new_context(sd, _lib.BUILDER_GPU_PLOC)
    ms = []
    for _ in range(5):
        p.set_scene(prt.Scene.from_data(dataclasses.replace(sd, meshes=[m1])))
        ms.append(p.scene_info().build_ms)
    print(f"prt_set_meshes with GPU_PLOC, same process: ms {stats(ms[1:])} (4 calls after one warm-up)")
    p.close()


def part_quality(runs=3, steps=20, warm=5):
    sd = scenes.config_c4()
    m0 = sd.meshes[0]
    spacing = 10.0 / 1000.0
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

    refit = new_context(sd, _lib.BUILDER_HOST_SAH)
    print("ms per frame, camera moved before every call; median [min .. max] of three interleaved runs")
    for name, amp in (("small (0.1 x spacing)", 0.1 * spacing), ("the grid spacing", spacing), ("10 x spacing", 10 * spacing)):
        m1 = deform.travelling_sine(m0, amp, 0.7, k=40.0)
        sd1 = dataclasses.replace(sd, meshes=[m1])
        refit.update_mesh(0, m1)
        trees = {"refitted HOST_SAH": refit, "fresh HOST_SAH": new_context(sd1, _lib.BUILDER_HOST_SAH),
                 "fresh GPU_PLOC": new_context(sd1, _lib.BUILDER_GPU_PLOC)}
        ms = {k: [] for k in trees}
        for c in trees.values():
            c.set_frames_in_flight(2)
        for _ in range(runs):
            for k, c in trees.items():
                frames(c, warm, 1)
                t0 = time.perf_counter()
                frames(c, steps, 1 + warm)
                ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
        print(f"amplitude {name} ({amp:.4f}): " + "; ".join(
            f"{k} {np.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}]" for k, v in ms.items()))
        for k, c in trees.items():
            if c is not refit:
                c.close()
    refit.close()


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "update"
    if part == "update":
        part_update()
    elif part == "kernels":
        part_update(kernels_only=True)
    elif part == "quality":
        part_quality()
    else:
        sys.exit(__doc__)
