#!/usr/bin/env python3
"""Cost of the rectifier (yv_rectify_run), in one session.

The workload: 2048 stereo frames per step (4096 images) of 512 x 1392 remapped to 376 x 1241 through the
KITTI-raw-like model of tests/rectify_reference.py for both maps.  Three arms alternate in one process for --rounds
rounds, each --warmup untimed and --steps timed steps between two device events on one stream:

    default   the LDS-staged tile kernel for the tiles whose source box fits, the direct kernel for the rest
    direct    yv_rectify_debug_force_direct: every tile through the direct kernel
    copy      a device-to-device copy of the same destination bytes, the yardstick

Every round is reported; the summary holds the rounds' mean, minimum and maximum per arm (the spread a difference has
to clear), nanoseconds per image and each arm's share of the copy's rate.  The two rectifying arms must write the same
bytes.

    python tools/bench_rectify.py [--frames 2048] [--out profiles/r16/rectify.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HS, WS, H, W = 512, 1392, 376, 1241


def _stats(v):
    return {"mean": round(float(np.mean(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "rounds": [round(float(x), 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048, help="stereo frames per step (two images each)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import ya_vo_amd as yv
    from ya_vo_amd import io as yio
    import rectify_reference as rr

    ctx = yv.Context(0)
    n = 2 * a.frames
    rect = yio.Rectifier(ctx, 2, (HS, WS), (H, W))
    model = rr.kitti_raw_model(HS, WS, H, W)
    for m in range(2):
        rect.set_model(m, *model)
    tiles = rect.tiles(0)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1234)
    d_src = torch.randint(0, 256, (n, HS, WS), dtype=torch.uint8, device="cuda:0", generator=gen)
    d_dst = torch.zeros((n, H, W), dtype=torch.uint8, device="cuda:0")
    d_copy = torch.zeros_like(d_dst)
    stream = torch.cuda.ExternalStream(ctx.stream)  # the context's stream: the runs, the copies and the events
    torch.cuda.synchronize()

    def step(arm):
        if arm == "copy":
            with torch.cuda.stream(stream):
                d_copy.copy_(d_dst, non_blocking=True)
        else:
            rect.run(d_src.data_ptr(), d_dst.data_ptr(), n)

    arms = ("default", "direct", "copy")
    ms = {arm: [] for arm in arms}
    sums = {}
    for _ in range(a.rounds):
        for arm in arms:
            rect.force_direct(arm == "direct")
            if arm != "copy":
                d_dst.zero_()
                torch.cuda.synchronize()
            for _ in range(a.warmup):
                step(arm)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.steps):
                step(arm)
            e1.record(stream)
            torch.cuda.synchronize()
            ms[arm].append(e0.elapsed_time(e1) / a.steps)
            if arm != "copy":  # what the arm wrote, for the comparison of the two
                sums[arm] = d_dst.clone()
    equal = bool(torch.equal(sums["default"], sums["direct"])) and bool(sums["default"].any())
    rect.force_direct(False)
    rect.close()
    ctx.close()

    rec = {"shape": f"{HS}x{WS} -> {H}x{W}", "images_per_step": n, "steps": a.steps, "warmup": a.warmup,
           "model": "kitti_raw (k1 -0.373, k2 0.204, k3 -0.072, roll 0.01 rad), both maps",
           "tiles_lds": tiles[0], "tiles_direct": tiles[1], "outputs_equal": equal,
           "bytes_read_per_image": HS * WS, "bytes_written_per_image": H * W,
           "unit": "ms per step between device events"}
    for arm in arms:
        rec[arm] = _stats(ms[arm])
        rec[arm]["ns_per_image"] = round(1e6 * rec[arm]["mean"] / n, 2)
    for arm in ("default", "direct"):
        rec[arm]["share_of_copy_rate"] = round(rec["copy"]["mean"] / rec[arm]["mean"], 4)
    spread = max(rec[arm]["max"] - rec[arm]["min"] for arm in ("default", "direct"))
    rec["direct_minus_default_ms"] = round(rec["direct"]["mean"] - rec["default"]["mean"], 4)
    rec["rounds_spread_ms"] = round(spread, 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
