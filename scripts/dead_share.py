#!/usr/bin/env python3
"""Share of dead shadow rays (prt_shadow_dead) in bench.py's configuration: the C4 frame (1920x1080, 4 spp, depth 4,
two frames in flight), static camera and camera moved before every call:
    python3 scripts/dead_share.py [--steps 10] [--warmup 56] [--inflight 2]
After the warm-up calls (the light-visibility record of a static view is then learned, as in the bench's timed steps)
the counters are reset and `steps` calls run; per variant one line with the shadow rays per step (prt_ray_totals),
the dead ones (counted, not traced), those answered from the record, and what is left to trace.  A ray under the
record counts there and never as dead, so the static view's dead share is below the share of dead rays among all the
shadow rays the reference casts, which the moving camera shows (no record, every dead ray counted)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physically-based-ray-tracer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=56)
    ap.add_argument("--inflight", type=int, default=2)
    args = ap.parse_args()

    import torch
    import prt
    from prt import scenes

    W, H, spp, bounces = 1920, 1080, 4, 4
    F = spp // 2
    sd = scenes.config_c4()
    ctx = prt.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_scene(prt.Scene.from_data(sd))
    aspect = np.float32(W) / np.float32(H)
    cams = [prt.Camera(np.asarray(sd.cam_pos, np.float32) + np.float32(0.002 * i) * np.asarray([1, 0, 1], np.float32),
                       sd.cam_target, aspect) for i in range(64)]
    ctx.set_frames_in_flight(args.inflight)
    avg = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    rgb = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out = {}
    for moving in (False, True):
        ctx.set_camera(cams[0])
        ctx.reset_accumulation(full=True)

        def run(first, n):
            for i in range(first, first + n):
                if moving:
                    ctx.set_camera(cams[i % len(cams)])
                ctx.render(W, H, spp, bounces, frame_index=F * i, avg=avg.data_ptr(), rgb8=rgb.data_ptr(),
                           device_out=True, stats=False)

        run(0, args.warmup)
        ctx.ray_totals(reset=True)
        ctx.shadow_dead(reset=True)
        ctx.shadow_reuse(reset=True)
        run(args.warmup, args.steps)
        _, shadow = ctx.ray_totals()
        dead, reused = ctx.shadow_dead(), ctx.shadow_reuse()
        n = args.steps
        name = "moving" if moving else "static"
        out[name] = {"shadow_per_step": shadow // n, "dead_per_step": dead // n, "reused_per_step": reused // n,
                     "traced_per_step": (shadow - dead - reused) // n, "dead_share": round(dead / shadow, 4),
                     "dead_share_of_not_reused": round(dead / (shadow - reused), 4)}
        print(f"{name:6s} camera: shadow rays per step {shadow // n}, dead {dead // n} ({dead / shadow:.4f}), from the "
              f"record {reused // n}, traced {(shadow - dead - reused) // n}; dead share of the rays not under the "
              f"record {dead / (shadow - reused):.4f}", flush=True)
    print(json.dumps({"workload": "c4 1920x1080 4spp depth 4", "frames_in_flight": args.inflight, "steps": args.steps,
                      **out}))
    ctx.close()


if __name__ == "__main__":
    main()
