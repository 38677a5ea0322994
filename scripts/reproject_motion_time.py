#!/usr/bin/env python3
"""Device time of the motion-aware reprojection pass (include/prt.h prt_reproject_motion) against prt_reproject at the
bench frame: C4 scene plus MOVERS moving tori (so that the matrix gather sees several instances), 1920 x 1080, 4 spp,
depth 4, two frames one camera step of (0.05, 0, 0.02) and one instance step apart, the pass's defaults.

Everything stays in device memory (PRT_OUT_DEVICE) on one torch stream the context works on: frame 0 is rendered and
starts a history, frame 1 is rendered, then prt_reproject and prt_reproject_motion (with and without history_instance)
run interleaved, one repetition of each in turn, between torch events; the median, the minimum and the maximum of REPS
repetitions after WARM warm-up ones are printed.  The AOV pass is timed the same way with and without the id output
(PRT_OUT_TIMED HIP events around the primary hits and the attribute kernels).

usage: reproject_motion_time.py [reps]        (default 20, after 5 warm-up repetitions)"""
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
W, H, SPP, BOUNCES = 1920, 1080, 4, 4
n = W * H
F = np.float32


def scene_and_transforms():
    """C4 with MOVERS tori over the heightfield around the camera target, and their transforms in the two frames."""
    base = scenes.config_c4()
    tor = scenes.torus(24, 12, 0.22, 0.08)
    tor.albedo, tor.metalness = 0, 2
    rng = np.random.default_rng(11)
    tgt = np.asarray(base.cam_target, np.float64)
    frames = [[], []]
    for _ in range(MOVERS):
        a, sc = rng.uniform(0, 2 * np.pi), rng.uniform(2.0, 4.0)
        at = tgt + np.array([rng.uniform(-2.5, 2.5), rng.uniform(0.8, 1.6), rng.uniform(-2.5, 2.5)])
        for k in (0, 1):
            ang, p = a + 0.15 * k, at + k * np.array([0.15, 0.0, 0.1])
            M = np.eye(4)
            M[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) * sc
            M[:3, 3] = p
            frames[k].append(M.astype(F))
    mesh = len(base.meshes)
    sd = dataclasses.replace(base, meshes=list(base.meshes) + [tor],
                             instances=list(base.instances) + [(mesh, M) for M in frames[0]], name="c4+movers")
    xf = [np.stack([np.asarray(T, F).reshape(4, 4) for _, T in base.instances] + frames[k]) for k in (0, 1)]
    return sd, xf


sd, xf = scene_and_transforms()
aspect = F(W) / F(H)
cams = [prt.Camera(np.asarray(sd.cam_pos, F) + np.array([0.05, 0.0, 0.02], F) * F(k), sd.cam_target, aspect)
        for k in (0, 1)]
stream = torch.cuda.Stream()
ctx = prt.Context(0)
ctx.set_stream(stream.cuda_stream)
scene = prt.Scene.from_data(sd)
ctx.set_scene(scene)
with torch.cuda.stream(stream):
    avg, alb, h0, out = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    nd = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    ids = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    rgb = torch.zeros(n, dtype=torch.int32, device="cuda")
par = prt.reproject_defaults()
motion = prt.instance_motion(xf[1], xf[0])


def view(k):
    ctx.set_instances([(mi, xf[k][i]) for i, (mi, _) in enumerate(scene.blases)])
    ctx.set_camera(cams[k])
    ctx.reset_accumulation(full=True)
    ctx.render(W, H, SPP, BOUNCES, frame_index=(SPP // 2) * k, avg=avg.data_ptr(), rgb8=rgb.data_ptr(),
               device_out=True, stats=False)
    ctx.render_aov_ids(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=nd[k].data_ptr(),
                       instance=ids[k].data_ptr())


view(0)
ctx.reproject_motion(avg.data_ptr(), nd[0].data_ptr(), ids[0].data_ptr(), cams[0], width=W, height=H, device_out=True,
                     out=h0.data_ptr())
view(1)


def plain():
    ctx.reproject(avg.data_ptr(), nd[1].data_ptr(), cams[1], h0.data_ptr(), nd[0].data_ptr(), cams[0], width=W,
                  height=H, params=par, device_out=True, out=out.data_ptr(), rgb8=rgb.data_ptr())


def moved(with_ids=True):
    ctx.reproject_motion(avg.data_ptr(), nd[1].data_ptr(), ids[1].data_ptr(), cams[1], h0.data_ptr(),
                         nd[0].data_ptr(), cams[0], ids[0].data_ptr() if with_ids else None, motion, width=W, height=H,
                         params=par, device_out=True, out=out.data_ptr(), rgb8=rgb.data_ptr())


def aov(with_ids):
    if with_ids:
        ctx.render_aov_ids(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=nd[1].data_ptr(),
                           instance=ids[1].data_ptr(), timed=True)
    else:
        ctx.render_aov(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=nd[1].data_ptr(), timed=True)
    return ctx.denoise_timings()[0]


def event_ms(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


calls = {"reproject": plain, "motion": moved, "motion_noids": lambda: moved(False)}
ms = {k: [] for k in list(calls) + ["aov", "aov_ids"]}
for r in range(WARM + REPS):  # one repetition of each in turn
    for k, f in calls.items():
        t = event_ms(f)
        if r >= WARM:
            ms[k].append(t)
    for k, w in (("aov", False), ("aov_ids", True)):
        t = aov(w)
        if r >= WARM:
            ms[k].append(t)


def stat(k):
    a = np.asarray(ms[k])
    return float(np.median(a)), float(a.min()), float(a.max())


moved()
stream.synchronize()
i1 = ids[1].cpu().numpy().view(np.uint32)
o = out.cpu().numpy()
hit, mover = i1 != 0xFFFFFFFF, (i1 != 0xFFFFFFFF) & (i1 >= len(xf[0]) - MOVERS)
plain()
stream.synchronize()
op = out.cpu().numpy()
print(f"reproject_motion_time: C4 + {MOVERS} moving tori {W}x{H}, {SPP} spp depth {BOUNCES}, frames one camera step "
      f"(0.05, 0, 0.02) and one instance step apart; defaults depth_tol={par.depth_tol:g} normal_min={par.normal_min:g} "
      f"max_history={par.max_history:g}; {REPS} repetitions after {WARM} warm-up, interleaved, median (min .. max) ms")
print(f"first-hit pixels {hit.mean():.3f}, on the movers {mover.mean():.4f} ({len(np.unique(i1[mover]))} of {MOVERS} "
      f"visible); movers' pixels with history: prt_reproject {np.mean(op[mover, 3] > 1):.3f}, "
      f"prt_reproject_motion {np.mean(o[mover, 3] > 1):.3f}")
rows = (("reproject", "prt_reproject (out_rgba + out_rgb8)"), ("motion", "prt_reproject_motion, history ids"),
        ("motion_noids", "prt_reproject_motion, no history ids"), ("aov", "AOV pass, prt_render_aov"),
        ("aov_ids", "AOV pass, prt_render_aov_ids"))
for k, label in rows:
    med, lo, hi = stat(k)
    print(f"   {label:40s} {med:8.4f}  ({lo:.4f} .. {hi:.4f})")
rp, mo, mn = stat("reproject"), stat("motion"), stat("motion_noids")
print(f"   motion / reproject = {mo[0] / rp[0]:.3f} with history ids (92 B / pixel against 84: byte-scaled 1.095), "
      f"{mn[0] / rp[0]:.3f} without (88 B: 1.048)")
print(f"   aov_ids - aov = {stat('aov_ids')[0] - stat('aov')[0]:+.4f} ms (the id kernel reads 20 B and writes 4 B per "
      f"pixel: {n * 24 / 1e6:.1f} MB)")
ctx.close()
