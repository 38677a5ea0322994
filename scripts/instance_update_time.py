#!/usr/bin/env python3
"""prt_update_instances against prt_set_instances on drifting instances, one MI355X, one process (DESIGN.md 8
"Instance updates: the TLAS refit"):
    python3 scripts/instance_update_time.py time     per update, at 1,000 and 10,000 instances: the host time of the
                                                     calling thread inside the call and the device time on the context
                                                     stream (torch events around the call, which for prt_set_instances
                                                     includes the stream's wait for the worker's build), for
                                                     prt_set_instances, prt_update_instances from host memory and from
                                                     device memory (median / min / max of 30 after 5, every instance moved
                                                     before every call, nothing else queued)
    python3 scripts/instance_update_time.py frames   10,000 instances: ms per frame (1280x720, 2 spp, depth 3, static
                                                     instances, 20 frames after 5, three interleaved runs) and
                                                     prt_tlas_cost with the freshly built tree, after the refit has
                                                     followed 200 drift steps, and after one prt_set_instances on top
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physically-based-ray-tracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import prt  # noqa: E402
from prt import _lib, scenes  # noqa: E402

W, H = 1280, 720
STREAM = torch.cuda.Stream()  # the contexts' stream: the events below are recorded in their work's order


def stats(v):
    return f"median {np.median(v):.3f}  min {min(v):.3f}  max {max(v):.3f}"


class Field:
    """instance_field(n) with every torus drifting in x and z, wrapping at the field's edge (scripts/tlas_drift.py)"""

    def __init__(self, n):
        self.sd = scenes.instance_field(n, seed=17)
        self.mi = np.array([m for m, _ in self.sd.instances], np.uint32)
        self.T = np.stack([np.array(T, np.float32) for _, T in self.sd.instances])
        self.vel = np.random.default_rng(3).uniform(-0.08, 0.08, (len(self.mi), 2)).astype(np.float32)

    def step(self):
        T = self.T.copy()
        mv = self.mi == 1
        for k, a in ((0, 0), (1, 2)):
            x = T[:, a, 3] + self.vel[:, k]
            x = np.where(x > 4.5, x - np.float32(9.0), np.where(x < -4.5, x + np.float32(9.0), x)).astype(np.float32)
            T[:, a, 3] = np.where(mv, x, T[:, a, 3])
        self.T = T
        return T

    def context(self):
        c = prt.Context(0)
        c.set_stream(STREAM.cuda_stream)
        c.set_scene(prt.Scene.from_data(self.sd))
        c.set_camera(prt.Camera(self.sd.cam_pos, self.sd.cam_target, np.float32(W) / np.float32(H)))
        return c


def set_instances(c, mi, T):  # the ABI calls themselves, without the list packing of the Python mirror
    _lib.check(c.L.prt_set_instances(c.h, T.ctypes.data, mi.ctypes.data, len(mi)))


def update_host(c, T):
    _lib.check(c.L.prt_update_instances(c.h, T.ctypes.data, len(T), 0))


def update_device(c, t):
    _lib.check(c.L.prt_update_instances(c.h, t.data_ptr(), t.numel() // 16, _lib.IN_DEVICE))


def timed(prepare, call, n, warm):
    dev, host = [], []
    for i in range(warm + n):
        arg = prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(STREAM)
        t0 = time.perf_counter()
        call(arg)
        t1 = time.perf_counter()
        e1.record(STREAM)
        torch.cuda.synchronize()
        if i >= warm:
            dev.append(e0.elapsed_time(e1))
            host.append((t1 - t0) * 1e3)
    return dev, host


def part_time():
    for n in (1000, 10000):
        f = Field(n)
        c = f.context()
        c.render(64, 48, 2, 2)  # the instance state is on the device, the kernels are loaded
        info = c.scene_info()
        print(f"{n} drifting instances (instance BVH of {len(c.read_tlas()[0])} nodes, {info.tlas_depth} levels planned):")

        def to_device():
            with torch.cuda.stream(STREAM):
                return torch.from_numpy(f.step()).cuda()

        for name, prepare, call in (("prt_set_instances", f.step, lambda T: set_instances(c, f.mi, T)),
                                    ("prt_update_instances, host memory", f.step, lambda T: update_host(c, T)),
                                    ("prt_update_instances, device memory", to_device, lambda t: update_device(c, t))):
            dev, host = timed(prepare, call, 30, 5)
            print(f"  {name}: host ms of the call {stats(host)}; device ms on the stream {stats(dev)}")
        info = c.scene_info()
        print(f"  ({info.tlas_rebuilds} rebuilds counted, {info.tlas_async} on the worker, last worker build "
              f"{info.tlas_build_ms:.2f} ms)")
        c.close()


def part_frames(runs=3, steps=20, warm=5, drift=200):
    f = Field(10000)
    avg = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    rgb = torch.zeros(H * W, dtype=torch.int32, device="cuda")

    def frames(c, n):
        for i in range(n):
            c.render(W, H, 2, 3, frame_index=i, avg=avg.data_ptr(), rgb8=rgb.data_ptr(), device_out=True, stats=False)
        c.finish()
        torch.cuda.synchronize()

    def ms_per_frame(c):
        frames(c, warm)
        t0 = time.perf_counter()
        frames(c, steps)
        return (time.perf_counter() - t0) * 1e3 / steps

    ctx = {"refitted": f.context(), "rebuilt": f.context()}
    built = [ms_per_frame(ctx["refitted"]) for _ in range(runs)]
    cost_built = ctx["refitted"].tlas_cost()
    for _ in range(drift):
        T = f.step()
        for c in ctx.values():
            update_host(c, T)
    set_instances(ctx["rebuilt"], f.mi, f.T)
    cost = {k: c.tlas_cost() for k, c in ctx.items()}
    ms = {k: [] for k in ctx}
    for _ in range(runs):
        for k, c in ctx.items():
            ms[k].append(ms_per_frame(c))
    info = ctx["refitted"].scene_info()
    print(f"10,000 instances, {W}x{H}, 2 spp, depth 3, ms per frame, median [min .. max] of {runs} runs of {steps} frames:")
    print(f"  freshly built tree (the scene's own positions): {np.median(built):.3f} [{min(built):.3f} .. {max(built):.3f}], "
          f"prt_tlas_cost {cost_built:.4f}")
    for k, what in (("refitted", f"after the refit has followed {drift} drift steps"),
                    ("rebuilt", "after one prt_set_instances on top of that")):
        v = ms[k]
        print(f"  {what}: {np.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}], prt_tlas_cost {cost[k]:.4f}")
    print(f"  refitted / rebuilt = {np.median(ms['refitted']) / np.median(ms['rebuilt']):.3f} in frame time, "
          f"{cost['refitted'] / cost['rebuilt']:.3f} in cost; the refitted context counted {info.tlas_rebuilds} rebuilds")
    for c in ctx.values():
        c.close()


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "time"
    if part == "time":
        part_time()
    elif part == "frames":
        part_frames()
    else:
        sys.exit(__doc__)
