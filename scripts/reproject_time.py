#!/usr/bin/env python3
"""Device time of the temporal reprojection pass (include/prt.h prt_reproject) at the bench frame: C4 scene,
1920 x 1080, 4 spp, depth 4, two views one step of (0.05, 0, 0.02) apart, the pass's defaults.

Everything stays in device memory (PRT_OUT_DEVICE) on one torch stream the context works on: view 0 is rendered and
starts a history, view 1 is rendered, then REPS repetitions of prt_reproject run between torch events; the median and
the minimum are printed.  The denoiser's prep pass (32 B per pixel, PRT_OUT_TIMED) is timed in the same process as
the yardstick of a pass that only moves its bytes, and the frame time of the same context gives the share.

usage: reproject_time.py [reps]        (default 20, after 5 warm-up repetitions)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physically-based-ray-tracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import prt  # noqa: E402
from prt import scenes  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARM = 5
W, H, SPP, BOUNCES = 1920, 1080, 4, 4
n = W * H
F = np.float32
sd = scenes.config_c4()
aspect = F(W) / F(H)
cams = [prt.Camera(np.asarray(sd.cam_pos, F) + np.array([0.05, 0.0, 0.02], F) * F(k), sd.cam_target, aspect)
        for k in (0, 1)]
stream = torch.cuda.Stream()
ctx = prt.Context(0)
ctx.set_stream(stream.cuda_stream)
ctx.set_scene(prt.Scene.from_data(sd))
with torch.cuda.stream(stream):
    avg, alb, h0, out = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    nd = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    rgb = torch.zeros(n, dtype=torch.int32, device="cuda")
par = prt.reproject_defaults()


def frame(i):
    ctx.render(W, H, SPP, BOUNCES, frame_index=(SPP // 2) * i, avg=avg.data_ptr(), rgb8=rgb.data_ptr(),
               device_out=True, stats=False)


def frame_ms(reps):
    ctx.finish()
    stream.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        frame(i)
    ctx.finish()
    stream.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def view(k):
    ctx.set_camera(cams[k])
    ctx.reset_accumulation(full=True)
    frame(k)
    ctx.render_aov(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=nd[k].data_ptr())


ctx.set_camera(cams[0])
frame_ms(10)
fms = frame_ms(40)
view(0)
ctx.reproject(avg.data_ptr(), nd[0].data_ptr(), cams[0], width=W, height=H, device_out=True, out=h0.data_ptr())
view(1)


def events(call):
    ms = []
    for r in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if r >= WARM:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def reproject(rgb8=True, history=True):
    hist = (h0.data_ptr(), nd[0].data_ptr(), cams[0]) if history else ()
    ctx.reproject(avg.data_ptr(), nd[1].data_ptr(), cams[1], *hist, width=W, height=H, params=par, device_out=True,
                  out=out.data_ptr(), rgb8=rgb.data_ptr() if rgb8 else None)


rp = events(reproject)
rp_no8 = events(lambda: reproject(rgb8=False))
rp_start = events(lambda: reproject(history=False))
one = prt.denoise_defaults(iterations=1)
prep = []
for r in range(WARM + REPS):
    ctx.denoise(avg.data_ptr(), alb.data_ptr(), nd[1].data_ptr(), W, H, one, device_out=True, out=out.data_ptr(),
                timed=True)
    if r >= WARM:
        prep.append(ctx.denoise_timings()[1])
prep_med, prep_min = float(np.median(prep)), float(np.min(prep))
reproject()
stream.synchronize()
hit = float((nd[1][:, 3] < 1e30).float().mean().item())
kept = float((out[:, 3] > 1).float().sum().item()) / max(1.0, hit * n)
print(f"reproject_time: C4 {W}x{H}, {SPP} spp depth {BOUNCES}, views (0.05, 0, 0.02) apart; defaults depth_tol="
      f"{par.depth_tol:g} normal_min={par.normal_min:g} max_history={par.max_history:g}; {REPS} repetitions after {WARM} "
      f"warm-up, median (min) ms, torch events on the context stream; first-hit pixels {hit:.3f}, of them with "
      f"history {kept:.3f}")
print(f"frame (prt_render, device outputs, no stats, one at a time, 40 frames): {fms:.3f} ms")
print(f"   reproject (out_rgba + out_rgb8)    {rp[0]:8.4f}  ({rp[1]:.4f}) = {100 * rp[0] / fms:.2f} % of the frame")
print(f"   reproject (out_rgba only)          {rp_no8[0]:8.4f}  ({rp_no8[1]:.4f})")
print(f"   reproject (no history: a copy)     {rp_start[0]:8.4f}  ({rp_start[1]:.4f})")
print(f"   denoiser prep pass (32 B / pixel)  {prep_med:8.4f}  ({prep_min:.4f})   PRT_OUT_TIMED HIP events")
# compulsory traffic per pixel: colour, normal_depth, one history and one history normal_depth item read (the other
# taps are shared with the neighbours), out_rgba and the RGB8 word written
scaled = prep_med * 84.0 / 32.0
print(f"   byte-scaled prep (84 B / pixel)    {scaled:8.4f}   reproject / byte-scaled prep = {rp[0] / scaled:.2f}")
print(f"   compulsory traffic {n * 84 / 1e9:.3f} GB -> {n * 84 / 1e9 / rp[0] * 1e3:.0f} GB/s over the reproject time")
ctx.close()
