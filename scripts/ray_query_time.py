#!/usr/bin/env python3
"""prt_query_rays against prt_intersect / prt_occluded on C4 (1M triangles), one MI355X, one process (DESIGN.md
"Ray queries").  Three batches:
    a   the 1920 x 1080 camera rays (pixel order, coherent), closest hits
    b   2M cosine-distributed rays leaving the primary hit points (seeded, incoherent), closest hits
    c   2M shadow queries from those points to point light 0 (tmax = the distance to the light), any hits

    python3 scripts/ray_query_time.py time      per batch: the stream time of one prt_query_rays call on device tensors
                                                (torch events on the context stream, median / min / max of 20 after 5)
                                                and its Mrays/s, the whole-call time of prt_query_rays on host arrays,
                                                and the whole-call time of prt_intersect / prt_occluded on the same
                                                host arrays (median of 5 after 1); batch a + b's surface pass too
    python3 scripts/ray_query_time.py kernels   per batch 6 device calls of prt_query_rays, then 6 lock-step calls, and
                                                nothing else after the set-up, for a run under
                                                rocprofv3 --kernel-trace --output-format csv
    python3 scripts/ray_query_time.py summary <kernel_trace.csv>
                                                the kernel-only times of that run: k_query against k_intersect /
                                                k_occluded per batch (median of the last 5 dispatches of each group)
"""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physically-based-ray-tracer_amd"))

W, H = 1920, 1080
N2 = 2_000_000
REPS = 6  # dispatches per group in the `kernels` part (the first one warms up)


def stats(v):
    import numpy as np
    return f"median {np.median(v):.3f}  min {min(v):.3f}  max {max(v):.3f}"


def setup():
    """The context with C4 on a torch stream, and the three batches as device tensors (origins, dirs, tmax or None)."""
    import numpy as np
    import torch
    import prt
    from prt import scenes
    sd = scenes.config_c4()
    stream = torch.cuda.Stream()
    c = prt.Context(0)
    c.set_stream(stream.cuda_stream)
    c.set_scene(prt.Scene.from_data(sd))
    cam = prt.Camera(sd.cam_pos, sd.cam_target, np.float32(W) / np.float32(H))
    c.set_camera(cam)
    with torch.cuda.stream(stream):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
        ys, xs = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        u = (xs.reshape(-1, 1).float() / W)
        v = (ys.reshape(-1, 1).float() / H)
        pos, tl, tr, bl = (dev(x) for x in (cam.camPos, cam.topLeft, cam.topRight, cam.bottomLeft))
        Da = (tl + u * (tr - tl) + v * (bl - tl) - pos).contiguous()
        Oa = pos.expand(W * H, 3).contiguous()
        # the primary hit points and their geometry normals, towards the viewer
        hits, _ = c.query_rays(Oa, Da)
        gn = c.query_surface(hits, None, albedo=False, normal_depth=False, material=False)["geometry_normal"][:, :3]
        hit = torch.nonzero(hits[:, 0] < 1e30).reshape(-1)
        g = torch.Generator(device="cuda")
        g.manual_seed(2024)
        pick = hit[torch.randint(hit.numel(), (N2,), generator=g, device="cuda")]
        d = Da[pick] / Da[pick].norm(dim=1, keepdim=True)
        n = gn[pick] / gn[pick].norm(dim=1, keepdim=True)
        n = torch.where((n * d).sum(1, keepdim=True) > 0, -n, n)
        P = Oa[pick] + hits[pick, 0:1] * d + 1e-3 * n
        # cosine-distributed directions about n (a unit vector on the sphere around n's tip)
        s = torch.randn((N2, 3), generator=g, device="cuda")
        s = s / s.norm(dim=1, keepdim=True)
        Db = n + 0.999 * s
        L = dev(sd.lights.point_pos[0])
        Dc = L - P
        tc = (Dc.norm(dim=1) - 1e-3).contiguous()
        batches = {"a": (Oa, Da, None, False), "b": (P.contiguous(), Db.contiguous(), None, False),
                   "c": (P.contiguous(), Dc.contiguous(), tc, True)}
    stream.synchronize()
    print(f"C4: {sd.meshes[0].tri_count} triangles, BLAS depth {c.scene_info().max_depth}; batch a {W * H} rays "
          f"({hit.numel()} hits), b and c {N2} rays")
    return c, stream, batches, hits


def device_call(c, O, D, tm, any_hit, out):
    from prt import _lib
    _lib.check(c.L.prt_query_rays(c.h, O.shape[0], O.data_ptr(), D.data_ptr(), tm.data_ptr() if tm is not None else None,
                                  None if any_hit else out.data_ptr(), out.data_ptr() if any_hit else None,
                                  _lib.OUT_DEVICE))


def lockstep_call(c, O, D, tm, any_hit):
    return c.occluded(O, D, tm) if any_hit else c.intersect(O, D, tm)


def part_time():
    import numpy as np
    import torch
    c, stream, batches, hits = setup()
    for name, (O, D, tm, any_hit) in batches.items():
        n = O.shape[0]
        with torch.cuda.stream(stream):
            out = torch.empty(n if any_hit else 5 * n, dtype=torch.int32 if any_hit else torch.float32, device="cuda")
        dev, host = [], []
        for i in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            t0 = time.perf_counter()
            device_call(c, O, D, tm, any_hit, out)
            t1 = time.perf_counter()
            e1.record(stream)
            torch.cuda.synchronize()
            if i >= 5:
                dev.append(e0.elapsed_time(e1))
                host.append((t1 - t0) * 1e3)
        On, Dn, tn = O.cpu().numpy(), D.cpu().numpy(), None if tm is None else tm.cpu().numpy()
        whole = {"prt_query_rays, host arrays": [], "lock-step": []}
        for i in range(6):
            t0 = time.perf_counter()
            got = c.query_rays(On, Dn, tn, closest=not any_hit, any_hit=any_hit)[1 if any_hit else 0]
            t1 = time.perf_counter()
            want = lockstep_call(c, On, Dn, tn, any_hit)
            t2 = time.perf_counter()
            assert got.tobytes() == want.tobytes()  # (and the device call's: the same kernels on the same rays)
            if i >= 1:
                whole["prt_query_rays, host arrays"].append((t1 - t0) * 1e3)
                whole["lock-step"].append((t2 - t1) * 1e3)
        kind = "any-hit" if any_hit else "closest"
        print(f"batch {name} ({n} rays, {kind}): prt_query_rays on device arrays: stream ms {stats(dev)} = "
              f"{n / np.median(dev) / 1e3:.0f} Mrays/s; host ms of the call {stats(host)}")
        print(f"  whole call on host arrays, ms: prt_query_rays {stats(whole['prt_query_rays, host arrays'])}; "
              f"{'prt_occluded' if any_hit else 'prt_intersect'} {stats(whole['lock-step'])}")
    # the surface pass at batch a's hits
    ms = []
    for i in range(25):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        with torch.cuda.stream(stream):
            c.query_surface(hits)
        e1.record(stream)
        torch.cuda.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1))
    print(f"prt_query_surface, {W * H} records, all four outputs (with torch's four allocations): stream ms {stats(ms)}")
    c.close()


def part_kernels():
    import torch
    c, stream, batches, _ = setup()
    for name, (O, D, tm, any_hit) in batches.items():
        n = O.shape[0]
        with torch.cuda.stream(stream):
            out = torch.empty(n if any_hit else 5 * n, dtype=torch.int32 if any_hit else torch.float32, device="cuda")
        for _ in range(REPS):
            device_call(c, O, D, tm, any_hit, out)
        torch.cuda.synchronize()
        On, Dn, tn = O.cpu().numpy(), D.cpu().numpy(), None if tm is None else tm.cpu().numpy()
        for _ in range(REPS):
            lockstep_call(c, On, Dn, tn, any_hit)
    torch.cuda.synchronize()
    c.close()


def part_summary(path):
    import numpy as np
    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").split("::")[-1].split("<")[0]
        if name in ("k_query", "k_intersect", "k_occluded"):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    rows = rows[1:]  # the set-up's own query of batch a
    want = [("a", "k_query"), ("a", "k_intersect"), ("b", "k_query"), ("b", "k_intersect"), ("c", "k_query"),
            ("c", "k_occluded")]
    assert len(rows) == REPS * len(want), len(rows)
    med = {}
    for k, (batch, name) in enumerate(want):
        grp = rows[k * REPS:(k + 1) * REPS]
        assert all(g[2] == name for g in grp), (batch, name, [g[2] for g in grp])
        us = [(e - s) / 1e3 for s, e, _ in grp[1:]]
        med[batch, name] = float(np.median(us))
        print(f"batch {batch} {name:12s} us: median {np.median(us):.1f}  min {min(us):.1f}  max {max(us):.1f}")
    for batch, ref in (("a", "k_intersect"), ("b", "k_intersect"), ("c", "k_occluded")):
        print(f"batch {batch}: k_query / {ref} = {med[batch, 'k_query'] / med[batch, ref]:.3f}")


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "time"
    if part == "time":
        part_time()
    elif part == "kernels":
        part_kernels()
    elif part == "summary" and len(sys.argv) > 2:
        part_summary(sys.argv[2])
    else:
        sys.exit(__doc__)
