#!/usr/bin/env python3
"""prt_rebuild_instances against prt_set_instances on drifting instances, one MI355X (DESIGN.md 8 "Instance rebuild:
a device build of the instance BVH"):
    python3 scripts/instance_rebuild_time.py time      per rebuild, at 1,000 and 10,000 instances: the host time of the
                                                       calling thread inside the call and the device time on the context
                                                       stream (torch events around the call), for both device builders
                                                       and the three transform sources (host memory, device memory,
                                                       NULL over device-resident transforms), beside prt_set_instances
                                                       (median [min .. max] of 30 after 5, every instance moved before
                                                       every call, nothing else queued); the builder's stream
                                                       synchronisations per build (PRT_REBUILD_TRACE) and what one costs
                                                       on an idle stream; whether two rebuilds give the same bytes
    python3 scripts/instance_rebuild_time.py quality   10,000 instances after the refit has followed 200 drift steps:
                                                       prt_tlas_cost and ms per frame (1280x720, 2 spp, depth 3, 20
                                                       frames after 5, three interleaved runs) with the kept tree, after
                                                       prt_rebuild_instances with each builder and after
                                                       prt_set_instances (the host SAH tree), and each device tree's
                                                       ratio to the SAH tree in both measures
    python3 scripts/instance_rebuild_time.py all       both parts, each as a child process under its own
                                                       `timeout -k 10`; stops at the first part that fails
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1280, 720
PART_LIMIT_S = {"time": 420, "quality": 420}


def main_all():
    for part, limit in PART_LIMIT_S.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), part])
        if r.returncode:
            sys.exit(f"part {part} ended with status {r.returncode}: nothing more is started on the GPU")


if __name__ == "__main__" and (len(sys.argv) < 2 or sys.argv[1] == "all"):
    main_all()
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "physically-based-ray-tracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import prt  # noqa: E402
from prt import _lib, scenes  # noqa: E402

STREAM = torch.cuda.Stream()  # the contexts' stream: the events below are recorded in their work's order
BUILDERS = (("GPU_LBVH", _lib.BUILDER_GPU_LBVH), ("GPU_PLOC", _lib.BUILDER_GPU_PLOC))


def stats(v):
    return f"median {np.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}]"


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


def rebuild_host(c, T, b):
    _lib.check(c.L.prt_rebuild_instances(c.h, T.ctypes.data, len(T), 0, b))


def rebuild_device(c, t, b):
    _lib.check(c.L.prt_rebuild_instances(c.h, t.data_ptr(), t.numel() // 16, _lib.IN_DEVICE, b))


def rebuild_kept(c, n, b):
    _lib.check(c.L.prt_rebuild_instances(c.h, None, n, 0, b))


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


def sync_round_trip_ms(n=200):
    """one 4-byte read-back and wait on the idle stream: what one of the builder's synchronisations costs at least"""
    with torch.cuda.stream(STREAM):
        x = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.zeros(1, dtype=torch.int32).pin_memory()
        v = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out.copy_(x, non_blocking=True)
            STREAM.synchronize()
            v.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(v[20:]))


def part_time():
    rt = sync_round_trip_ms()
    print(f"one read-back + stream synchronisation on the idle stream: median {rt * 1e3:.1f} us")
    for n in (1000, 10000):
        f = Field(n)
        c = f.context()
        c.render(64, 48, 2, 2)  # the instance state is on the device, the kernels are loaded
        info = c.scene_info()
        print(f"{n} drifting instances (host SAH tree: {len(c.read_tlas()[0])} nodes, {info.tlas_depth} levels planned):")

        def to_device():
            with torch.cuda.stream(STREAM):
                t = torch.from_numpy(f.step()).cuda()
            STREAM.synchronize()
            return t

        def kept_on_device():
            t = to_device()
            update_device(c, t)
            return t

        dev, host = timed(f.step, lambda T: set_instances(c, f.mi, T), 30, 5)
        print(f"  prt_set_instances: host ms of the call {stats(host)}; device ms on the stream {stats(dev)}")
        for bname, b in BUILDERS:
            os.environ["PRT_REBUILD_TRACE"] = "1"  # one traced call: nodes, depth, the builder's synchronisations
            sys.stdout.flush()
            rebuild_host(c, f.step(), b)
            del os.environ["PRT_REBUILD_TRACE"]
            sys.stderr.flush()
            nodes1 = c.read_tlas()
            rebuild_kept(c, len(f.mi), b)
            nodes2 = c.read_tlas()
            same = np.array_equal(nodes1[0], nodes2[0]) and np.array_equal(nodes1[1], nodes2[1])
            print(f"  {bname}: {len(nodes1[0])} nodes, prt_tlas_cost {c.tlas_cost():.4f}; two rebuilds of one state: "
                  f"{'the same bytes' if same else 'the same node count, another order within a level' if len(nodes1[0]) == len(nodes2[0]) else 'DIFFERENT TREES'}")
            for name, prepare, call in ((f"prt_rebuild_instances {bname}, host memory", f.step, lambda T: rebuild_host(c, T, b)),
                                        (f"prt_rebuild_instances {bname}, device memory", to_device, lambda t: rebuild_device(c, t, b)),
                                        (f"prt_rebuild_instances {bname}, NULL (device-resident)", kept_on_device,
                                         lambda t: rebuild_kept(c, len(f.mi), b))):
                dev, host = timed(prepare, call, 30, 5)
                print(f"  {name}: host ms of the call {stats(host)}; device ms on the stream {stats(dev)}")
        info = c.scene_info()
        print(f"  ({info.tlas_rebuilds} worker rebuilds counted, {info.tlas_async} on the worker, {info.tlas_depth} levels planned)")
        c.close()


def part_quality(runs=3, steps=20, warm=5, drift=200):
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

    names = {"kept": f"the tree the refit kept over {drift} drift steps",
             "lbvh": "prt_rebuild_instances GPU_LBVH", "ploc": "prt_rebuild_instances GPU_PLOC",
             "sah": "prt_set_instances (host SAH)"}
    ctx = {k: f.context() for k in names}
    for c in ctx.values():
        frames(c, 1)
    for _ in range(drift):
        T = f.step()
        for c in ctx.values():
            update_host(c, T)
    rebuild_kept(ctx["lbvh"], len(f.mi), _lib.BUILDER_GPU_LBVH)
    rebuild_kept(ctx["ploc"], len(f.mi), _lib.BUILDER_GPU_PLOC)
    set_instances(ctx["sah"], f.mi, f.T)
    cost = {k: c.tlas_cost() for k, c in ctx.items()}
    depth = {k: c.scene_info().tlas_depth for k, c in ctx.items()}
    nodes = {k: len(c.read_tlas()[0]) for k, c in ctx.items()}
    ms = {k: [] for k in ctx}
    for _ in range(runs):
        for k, c in ctx.items():
            ms[k].append(ms_per_frame(c))
    print(f"10,000 instances after {drift} drift steps, {W}x{H}, 2 spp, depth 3, ms per frame, median [min .. max] of "
          f"{runs} interleaved runs of {steps} frames:")
    for k, what in names.items():
        print(f"  {what}: {stats(ms[k])}, prt_tlas_cost {cost[k]:.4f}, {nodes[k]} nodes, {depth[k]} levels planned")
    for k in ("kept", "lbvh", "ploc"):
        print(f"  {k} / sah = {np.median(ms[k]) / np.median(ms['sah']):.3f} in frame time, {cost[k] / cost['sah']:.3f} in cost")
    for c in ctx.values():
        c.close()


if __name__ == "__main__":
    part = sys.argv[1]
    if part == "time":
        part_time()
    elif part == "quality":
        part_quality()
    else:
        sys.exit(__doc__)
