#!/usr/bin/env python3
"""Cost of the sub-pixel stereo refinement inside stage 4 of the batch, in one session.

The workload: 512 synthetic stereo frames of 376 x 1241 per run (1024 images), 2000 keypoints per image, the stereo and
temporal pairs of the pipeline, every stereo pair marked for refinement at (half_win, search).  Batch.enable_timing /
stage_times give slot 4 (Matches records + removeOutliers, and the refinement when it is on).  The modes alternate
refinement off / on for --rounds rounds, each --warmup untimed and --steps timed runs; every round is reported, and the
summary holds the rounds' mean, minimum and maximum per mode: the spread a difference has to clear.  The refined
matches are counted from the status array of the last round with the refinement on (every round runs the same images),
so the difference also reads as nanoseconds per attempted match.

--parent-lib PATH measures the same stage with another build of libyavo.so (the parent commit's, which has no
refinement) in a child process of this one, before and after the rounds, so both sides come from the same box and
session.

    python tools/bench_stereo_subpix.py [--parent-lib ya_vo_amd/lib/libyavo_parent.so] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_KP = 2000
THR = 20
NEW_SYMBOLS = ("yv_stereo_subpix", "yv_batch_set_stereo_subpix", "yv_batch_subpix_view_get", "yv_triangulate_subpix")


def _stats(v):
    return {"mean": round(float(np.mean(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "rounds": [round(float(x), 4) for x in v]}


def measure(a, modes):
    """-> {mode: [stage-4 ms per run, one per round]}, attempted matches per run with the refinement on"""
    import torch
    import ya_vo_amd as yv
    from ya_vo_amd.synth import H_KITTI, W_KITTI, synth_stereo_batch

    if a.pre_subpix_lib:  # the parent's library has none of the new symbols to bind
        for name in NEW_SYMBOLS:
            yv.SIGNATURES.pop(name, None)
            yv.GEOM_SIGNATURES.pop(name, None)
    ctx = yv.Context(0)
    ctx.set_brief_offsets(np.fromfile(os.path.join(ROOT, "tests", "golden", "brief_offsets_mt19937_42.bin"), np.int8))
    images = synth_stereo_batch(1234, a.frames)
    d = torch.from_numpy(images).to("cuda:0")
    torch.cuda.synchronize()
    n = len(images)
    batch = yv.Batch(ctx, n, H_KITTI, W_KITTI, MAX_KP, 2 * a.frames)
    batch.set_pairs([(2 * k, 2 * k + 1) for k in range(a.frames)] + [(2 * k - 2, 2 * k) for k in range(1, a.frames)])
    stage = {m: [] for m in modes}
    attempted = 0
    for _ in range(a.rounds):
        for mode in modes:
            if not a.pre_subpix_lib:
                batch.set_stereo_subpix(list(range(a.frames)) if mode == "on" else None, a.half_win, a.search)
            batch.enable_timing(False)
            for _ in range(a.warmup):
                batch.run(d.data_ptr(), n, W_KITTI, H_KITTI * W_KITTI, THR)
            ctx.sync()
            batch.enable_timing(True)
            for _ in range(a.steps):
                batch.run(d.data_ptr(), n, W_KITTI, H_KITTI * W_KITTI, THR)
            ctx.sync()
            ms, runs = batch.stage_times()
            stage[mode].append(float(ms[4]) / runs)
            if mode == "on":
                st = ctx.download(batch.subpix_view().status, np.uint8, a.frames * MAX_KP)
                attempted = int((st != yv.YV_SUBPIX_NONE).sum())
    batch.enable_timing(False)
    batch.close()
    ctx.close()
    return stage, attempted


def measure_parent(a):
    """Stage 4 of another libyavo.so, in a fresh child process."""
    env = dict(os.environ, YAVO_LIB=os.path.abspath(a.parent_lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--modes", "off", "--pre-subpix-lib", "--rounds", str(a.rounds),
           "--steps", str(a.steps), "--warmup", str(a.warmup), "--frames", str(a.frames)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True, timeout=a.child_timeout).stdout
    return json.loads(out.strip().splitlines()[-1])["off"]["rounds"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=512, help="stereo frames per run (two images each)")
    ap.add_argument("--half-win", type=int, default=5)
    ap.add_argument("--search", type=int, default=3)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pre-subpix-lib", action="store_true", help="the library loaded (YAVO_LIB) predates the feature")
    ap.add_argument("--child-timeout", type=float, default=180.0, help="seconds a --parent-lib child may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    modes = a.modes.split(",")
    parent = []
    if a.parent_lib:
        parent += measure_parent(a)
    stage, attempted = measure(a, modes)
    if a.parent_lib:
        parent += measure_parent(a)
    rec = {"shape": "376x1241", "images_per_run": 2 * a.frames, "max_kp": MAX_KP, "steps": a.steps,
           "warmup": a.warmup, "half_win": a.half_win, "search": a.search,
           "unit": "ms per run, stage 4 (match records, removeOutliers, refinement) by device events"}
    for m in modes:
        rec[m] = _stats(stage[m])
    if parent:
        rec["parent_off"] = _stats(parent)
    if "on" in rec and "off" in rec:
        rec["attempted_matches_per_run"] = attempted
        rec["refinement_ms_per_run"] = round(rec["on"]["mean"] - rec["off"]["mean"], 4)
        if attempted:
            rec["refinement_ns_per_match"] = round(1e6 * (rec["on"]["mean"] - rec["off"]["mean"]) / attempted, 3)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
