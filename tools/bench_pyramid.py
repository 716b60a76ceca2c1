#!/usr/bin/env python3
"""Cost of the scale pyramid (yv_batch_set_pyramid), in one session.

The workload: --images KITTI-sized images (376 x 1241, synthetic texture) per yv_batch_run, paired two by two as stereo
pairs, max_kp 2000.  The arms alternate in one process for --rounds rounds, each --warmup untimed and --steps timed
runs between two device events on the context's stream:

    single    the pyramid off: the step every batch ran before
    pyr4      4 levels at 1.2, area-proportional quotas that sum to max_kp
    pyr8      8 levels at 1.2

Every round is reported; the summary holds the rounds' mean, minimum and maximum per arm, the batch's own per-stage
times (stage 0 holds the level images and the levels' detect, 1 their cut, 2 their BRIEF and the merge) and the bytes
the level images must move (every level read once and written once).  The level kernel's and the merge kernel's own
times come from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/bench_pyramid.py).

    python tools/bench_pyramid.py [--images 512] [--out profiles/r22/pyramid.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, MAX_KP = 376, 1241, 2000


def _stats(v):
    return {"mean": round(float(np.mean(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "rounds": [round(float(x), 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512, help="images per run (an even number: stereo pairs)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import ya_vo_amd as yv
    from ya_vo_amd import pyramid as yp
    from ya_vo_amd.synth import synth_frame

    n = a.images
    ctx = yv.Context(0)
    ctx.set_brief_offsets(np.fromfile(os.path.join(ROOT, "tests", "golden", "brief_offsets_mt19937_42.bin"), np.int8))
    frames = np.stack([synth_frame(1234, i // 2, 5 * (i % 2), H, W) for i in range(n)])
    d = torch.from_numpy(frames).to("cuda:0")
    stream = torch.cuda.ExternalStream(ctx.stream)
    torch.cuda.synchronize()

    arms = {"single": 1, "pyr4": 4, "pyr8": 8}
    batches, sizes = {}, {}
    for arm, levels in arms.items():
        b = yv.Batch(ctx, n, H, W, MAX_KP, n // 2)
        b.set_pairs([(2 * i, 2 * i + 1) for i in range(n // 2)])
        sizes[arm] = yp.level_sizes(H, W, levels)
        b.set_pyramid(sizes[arm], yp.level_quotas(MAX_KP, sizes[arm]))
        batches[arm] = b

    ms = {arm: [] for arm in arms}
    stages = {arm: [] for arm in arms}
    kps = {}
    for _ in range(a.rounds):
        for arm, b in batches.items():
            for _ in range(a.warmup):
                b.run(d.data_ptr(), n, W, H * W, 20)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.steps):
                b.run(d.data_ptr(), n, W, H * W, 20)
            e1.record(stream)
            torch.cuda.synchronize()
            ms[arm].append(e0.elapsed_time(e1) / a.steps)
            # the stages' share, from runs of their own (an event between every two stages)
            b.enable_timing(True)
            for _ in range(a.steps):
                b.run(d.data_ptr(), n, W, H * W, 20)
            ctx.sync()
            t, runs = b.stage_times()
            b.enable_timing(False)
            stages[arm].append([float(x) / runs for x in t[:5]])
            kps[arm] = float(ctx.download(b.view().kp_count, np.int32, n).mean())

    rec = {"shape": f"{H}x{W}", "images_per_step": n, "max_kp": MAX_KP, "steps": a.steps, "warmup": a.warmup,
           "unit": "ms per step between device events"}
    for arm in arms:
        rec[arm] = _stats(ms[arm])
        rec[arm]["us_per_image"] = round(1e3 * rec[arm]["mean"] / n, 2)
        rec[arm]["stage_ms"] = dict(zip(yv.STAGE_NAMES[:5], (round(x, 4) for x in np.mean(stages[arm], 0))))
        rec[arm]["keypoints_per_image"] = round(kps[arm], 1)
        rec[arm]["sizes"] = [list(s) for s in sizes[arm]]
        s = sizes[arm]
        rec[arm]["level_bytes_per_image"] = int(sum(s[l - 1][0] * s[l - 1][1] + s[l][0] * s[l][1]
                                                    for l in range(1, len(s))))
    for arm in ("pyr4", "pyr8"):
        rec[arm]["step_over_single"] = round(rec[arm]["mean"] / rec["single"]["mean"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for b in batches.values():
        b.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
