#!/usr/bin/env python3
"""Device time of the first-hit AOV pass and of each pass of the a-trous denoiser (include/prt.h prt_render_aov /
prt_denoise) at the bench frame: C4 scene, 1920 x 1080, 4 spp, depth 4, the denoiser's defaults.

Everything stays in device memory (PRT_OUT_DEVICE): one C4 frame is rendered, then REPS repetitions of
prt_render_aov + prt_denoise run with PRT_OUT_TIMED, which records HIP events around the AOV pass, the prep pass and
every filter iteration; the median of each over the repetitions is printed, with the frame time of the same context
(device outputs, no stats, one frame at a time) for the share.

usage: denoise_time.py [reps]        (default 20, after 5 warm-up repetitions)"""
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
sd = scenes.config_c4()
ctx = prt.Context(0)
ctx.set_scene(prt.Scene.from_data(sd))
ctx.set_camera(prt.Camera(sd.cam_pos, sd.cam_target, np.float32(W) / np.float32(H)))
avg, alb, nd, out = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(4))
rgb = torch.zeros(n, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()  # (the buffers are filled on the null stream, the context works on its own stream)
par = prt.denoise_defaults()
iters = par.iterations


def frame(i):
    ctx.render(W, H, SPP, BOUNCES, frame_index=(SPP // 2) * i, avg=avg.data_ptr(), rgb8=rgb.data_ptr(),
               device_out=True, stats=False)


def frame_ms(reps):
    ctx.finish()
    ctx.ray_totals()  # waits for the stream
    t0 = time.perf_counter()
    for i in range(reps):
        frame(i)
    ctx.finish()
    ctx.ray_totals()
    return (time.perf_counter() - t0) * 1e3 / reps


def one():
    ctx.render_aov(W, H, device_out=True, albedo=alb.data_ptr(), normal_depth=nd.data_ptr(), timed=True)
    ctx.denoise(avg.data_ptr(), alb.data_ptr(), nd.data_ptr(), W, H, par, device_out=True, out=out.data_ptr(),
                rgb8=rgb.data_ptr(), timed=True)
    return ctx.denoise_timings()[:2 + iters]


frame_ms(10)
fms = frame_ms(40)
ctx.reset_accumulation(full=True)
frame(0)  # the noisy input: one fresh C4 frame
rows = []
for r in range(WARM + REPS):
    t = one()
    if r >= WARM:
        rows.append(t)
prim_ms = float(np.median([ctx.trace_primary(W, H)[1].ms for _ in range(5)]))  # the hits kernel alone
hit = float((nd[:, 3] < 1e30).float().mean().item())
print(f"denoise_time: C4 {W}x{H}, {SPP} spp depth {BOUNCES}; defaults iterations={iters} normal_power={par.normal_power} "
      f"sigma_color={par.sigma_color:g} sigma_depth={par.sigma_depth:g} sigma_albedo={par.sigma_albedo:g}; "
      f"{REPS} repetitions after {WARM} warm-up, median (min) ms per pass, HIP events; first-hit pixels {hit:.3f}")
print(f"frame (prt_render, device outputs, no stats, one at a time, 40 frames): {fms:.3f} ms")
names = ["aov (primary hits + k_aov)", "prep (unit normal + depth)"] + [f"filter step {1 << i}" for i in range(iters)]
a = np.array(rows)
med = np.median(a, axis=0)
for k, nm in enumerate(names):
    print(f"   {nm:30s} {med[k]:8.4f}  ({a[:, k].min():.4f})")
print(f"   (of the aov pass, k_primary_hits alone by prt_trace_primary's events: {prim_ms:.4f})")
den = float(med[1:].sum())
tot = float(med.sum())
print(f"   denoise (prep + {iters} passes)     {den:8.4f} = {100 * den / fms:.1f} % of the frame;  aov + denoise {tot:8.4f} = "
      f"{100 * tot / fms:.1f} %")
# compulsory traffic: a pass reads 48 B and writes 16 B per pixel (+ 4 B rgb8 in the last), the prep pass 16 + 16
gb = n * (64 * iters + 4 + 32) / 1e9
print(f"   compulsory traffic {gb:.3f} GB -> {gb / den * 1e3:.0f} GB/s over the denoise time")
ctx.close()
