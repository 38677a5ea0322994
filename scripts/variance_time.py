#!/usr/bin/env python3
"""Device time of the moments-carrying reprojection (include/prt.h prt_reproject_moments) against prt_reproject_motion,
and of the variance-guided filter (prt_denoise_variance) against prt_denoise, at the bench frame: C4 scene plus MOVERS
tori, 1920 x 1080, 4 spp, depth 4, the passes' defaults.

Two histories of FRAMES frames are built on the device: `rest` (nothing moves: every hit pixel's history is FRAMES - 1
long, so no lane takes the 5 x 5 spatial branch) and `motion` (a camera step of (0.05, 0, 0.02) and an instance step per
frame: the disoccluded pixels take it).  Everything stays in device memory (PRT_OUT_DEVICE) on one torch stream the
context works on.  For each history the last frame's prt_reproject_motion and prt_reproject_moments (clamp_k 0 and 1.5)
run interleaved, one repetition of each in turn, between torch events; then prt_denoise and prt_denoise_variance (5
iterations each) likewise, with the per-iteration times of PRT_OUT_TIMED.  The median, the minimum and the maximum of
REPS repetitions after WARM warm-up ones are printed, and the AOV pass as context.

usage: variance_time.py [reps]        (default 20, after 5 warm-up repetitions)"""
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physically-based-ray-tracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import prt  # noqa: E402
from prt import scenes  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARM = 5
MOVERS = 8
FRAMES = 6
W, H, SPP, BOUNCES = 1920, 1080, 4, 4
n = W * H
F = np.float32


def scene_and_transforms():
    """C4 with MOVERS tori over the heightfield around the camera target, and their transforms in the FRAMES frames."""
    base = scenes.config_c4()
    tor = scenes.torus(24, 12, 0.22, 0.08)
    tor.albedo, tor.metalness = 0, 2
    rng = np.random.default_rng(11)
    tgt = np.asarray(base.cam_target, np.float64)
    frames = [[] for _ in range(FRAMES)]
    for _ in range(MOVERS):
        a, sc = rng.uniform(0, 2 * np.pi), rng.uniform(2.0, 4.0)
        at = tgt + np.array([rng.uniform(-2.5, 2.5), rng.uniform(0.8, 1.6), rng.uniform(-2.5, 2.5)])
        for k in range(FRAMES):
            ang, p = a + 0.15 * k, at + k * np.array([0.15, 0.0, 0.1])
            M = np.eye(4)
            M[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) * sc
            M[:3, 3] = p
            frames[k].append(M.astype(F))
    mesh = len(base.meshes)
    sd = dataclasses.replace(base, meshes=list(base.meshes) + [tor],
                             instances=list(base.instances) + [(mesh, M) for M in frames[0]], name="c4+movers")
    xf = [np.stack([np.asarray(T, F).reshape(4, 4) for _, T in base.instances] + frames[k]) for k in range(FRAMES)]
    return sd, xf


sd, xf = scene_and_transforms()
aspect = F(W) / F(H)
stream = torch.cuda.Stream()
ctx = prt.Context(0)
ctx.set_stream(stream.cuda_stream)
scene = prt.Scene.from_data(sd)
ctx.set_scene(scene)
f4 = lambda: torch.zeros((n, 4), dtype=torch.float32, device="cuda")  # noqa: E731
u1 = lambda: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
with torch.cuda.stream(stream):
    avg, alb, out, mom, flt = f4(), f4(), f4(), f4(), f4()
    var, rgb = torch.zeros(n, dtype=torch.float32, device="cuda"), u1()
tp0, tp1 = prt.temporal_defaults(), prt.temporal_defaults(clamp_k=1.5)
rp = prt.reproject_defaults()
dp, vp = prt.denoise_defaults(), prt.denoise_variance_defaults()


def history(moving):
    """The device buffers of the last step of a FRAMES-frame chain: dict(cam, prev, nd, pnd, ids, pids, h, hm, motion);
    avg / alb hold the last frame afterwards."""
    with torch.cuda.stream(stream):
        nd, ids = [f4(), f4()], [u1(), u1()]
        h, hm = [f4(), f4()], [f4(), f4()]
    prev = None
    for k in range(FRAMES):
        j = k if moving else 0
        cam = prt.Camera(np.asarray(sd.cam_pos, F) + np.array([0.05, 0.0, 0.02], F) * F(j), sd.cam_target, aspect)
        ctx.set_instances([(mi, xf[j][i]) for i, (mi, _) in enumerate(scene.blases)])
        ctx.set_camera(cam)
        ctx.reset_accumulation(full=True)
        ctx.render(W, H, SPP, BOUNCES, frame_index=(SPP // 2) * k, avg=avg.data_ptr(), rgb8=rgb.data_ptr(),
                   device_out=True, stats=False)
        a, b = k & 1, (k & 1) ^ 1
        ctx.render_aov_ids(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=nd[a].data_ptr(),
                           instance=ids[a].data_ptr())
        if k == FRAMES - 1:
            motion = prt.instance_motion(xf[j], xf[j - 1 if moving else 0])
            return dict(cam=cam, prev=prev, nd=nd[a], pnd=nd[b], ids=ids[a], pids=ids[b], h=h[b], hm=hm[b],
                        motion=motion)
        if k == 0:
            ctx.reproject_moments(avg.data_ptr(), nd[a].data_ptr(), ids[a].data_ptr(), cam, width=W, height=H,
                                  device_out=True, out=h[a].data_ptr(), moments=hm[a].data_ptr())
        else:
            ctx.reproject_moments(avg.data_ptr(), nd[a].data_ptr(), ids[a].data_ptr(), cam, h[b].data_ptr(),
                                  nd[b].data_ptr(), prev, ids[b].data_ptr(),
                                  prt.instance_motion(xf[j], xf[j - 1 if moving else 0]), hm[b].data_ptr(), width=W,
                                  height=H, device_out=True, out=h[a].data_ptr(), moments=hm[a].data_ptr())
        prev = cam


def event_ms(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stat(a):
    a = np.asarray(a)
    return float(np.median(a)), float(a.min()), float(a.max())


def row(label, a):
    med, lo, hi = stat(a)
    print(f"   {label:52s} {med:8.4f}  ({lo:.4f} .. {hi:.4f})")
    return med


print(f"variance_time: C4 + {MOVERS} tori {W}x{H}, {SPP} spp depth {BOUNCES}, the last of {FRAMES} frames; "
      f"{REPS} repetitions after {WARM} warm-up, interleaved, median (min .. max) ms")
for moving in (False, True):
    g = history(moving)

    def motion_pass():
        ctx.reproject_motion(avg.data_ptr(), g["nd"].data_ptr(), g["ids"].data_ptr(), g["cam"], g["h"].data_ptr(),
                             g["pnd"].data_ptr(), g["prev"], g["pids"].data_ptr(), g["motion"], width=W, height=H,
                             params=rp, device_out=True, out=out.data_ptr(), rgb8=rgb.data_ptr())

    def moments_pass(tp=tp0):
        ctx.reproject_moments(avg.data_ptr(), g["nd"].data_ptr(), g["ids"].data_ptr(), g["cam"], g["h"].data_ptr(),
                              g["pnd"].data_ptr(), g["prev"], g["pids"].data_ptr(), g["motion"], g["hm"].data_ptr(),
                              width=W, height=H, params=tp, device_out=True, out=out.data_ptr(),
                              moments=mom.data_ptr(), rgb8=rgb.data_ptr())

    def aov():
        ctx.render_aov_ids(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=g["nd"].data_ptr(),
                           instance=g["ids"].data_ptr(), timed=True)
        return ctx.denoise_timings()[0]

    def plain_filter():
        ctx.denoise(out.data_ptr(), alb.data_ptr(), g["nd"].data_ptr(), W, H, dp, device_out=True, out=flt.data_ptr(),
                    rgb8=rgb.data_ptr(), timed=True)

    def variance_filter():
        ctx.denoise_variance(out.data_ptr(), mom.data_ptr(), alb.data_ptr(), g["nd"].data_ptr(), W, H, vp,
                             device_out=True, out=flt.data_ptr(), variance=var.data_ptr(), rgb8=rgb.data_ptr(),
                             timed=True)

    calls = {"motion": motion_pass, "moments": moments_pass, "clamp": lambda: moments_pass(tp1)}
    ms = {k: [] for k in list(calls) + ["aov", "denoise", "denoise_var"]}
    its = {"denoise": [], "denoise_var": []}
    for r in range(WARM + REPS):  # one repetition of each in turn
        for k, f in calls.items():
            t = event_ms(f)
            if r >= WARM:
                ms[k].append(t)
        moments_pass()  # out / mom: the filters' input
        t = aov()
        if r >= WARM:
            ms["aov"].append(t)
        for k, f in (("denoise", plain_filter), ("denoise_var", variance_filter)):
            t = event_ms(f)
            if r >= WARM:
                ms[k].append(t)
                its[k].append(ctx.denoise_timings()[1:7])
    stream.synchronize()
    o, m, i1 = out.cpu().numpy(), mom.cpu().numpy(), g["ids"].cpu().numpy().view(np.uint32)
    hit = i1 != 0xFFFFFFFF
    spatial = hit & (o[:, 3] < tp0.min_temporal)
    print(f"{'camera and instances move' if moving else 'at rest'}: first-hit pixels {hit.mean():.3f}, of them with "
          f"history {np.mean(o[hit, 3] > 1):.3f}, in the spatial branch (len < {tp0.min_temporal:g}) "
          f"{spatial.sum() / hit.sum():.3f}; mean variance {m[hit, 2].mean():.4f}")
    a = row("prt_reproject_motion (history ids)", ms["motion"])
    b = row("prt_reproject_moments, clamp_k 0", ms["moments"])
    c = row("prt_reproject_moments, clamp_k 1.5", ms["clamp"])
    print(f"   moments / motion = {b / a:.3f} (124 B / pixel against 92: byte-scaled 1.35; 18 IEEE divisions and "
          f"square roots per blended pixel against 16, + 3 in the spatial branch with up to 25 x 24 B of taps), with "
          f"the clamp "
          f"{c / a:.3f} (+ 9 x 16 B of taps, 6 divisions, 3 square roots)")
    row("AOV pass, prt_render_aov_ids", ms["aov"])
    d = row("prt_denoise, 5 iterations", ms["denoise"])
    e = row("prt_denoise_variance, 5 iterations", ms["denoise_var"])
    for k in ("denoise", "denoise_var"):
        t = np.median(np.asarray(its[k]), axis=0)
        print(f"      {k:12s} prep {t[0]:.4f}, iterations " + " ".join(f"{x:.4f}" for x in t[1:]))
    print(f"   denoise_variance / denoise = {e / d:.3f} (per tap the same 48 B and 6 divisions, + 1 multiply and 1 "
          f"multiply-add; per pixel + 9 x 8 B of pre-filter taps and 2 divisions; the prep writes 16 B more)")
ctx.close()
