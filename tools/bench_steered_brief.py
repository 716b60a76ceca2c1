#!/usr/bin/env python3
"""Stage time of the rotation-steered BRIEF against the unsteered descriptor, in one session.

The headline shape: 512 images of 376 x 1241 per run (256 synthetic stereo frames), 2000 keypoints per image, the stereo
and temporal pairs of the pipeline.  Batch.enable_timing / stage_times give slot 2, the descriptor stage alone.  The
modes alternate steering off / on for --rounds rounds, each --warmup untimed and --steps timed runs; every round is
reported, and the summary holds the rounds' mean, minimum and maximum per mode: the spread a difference has to clear.

--parent-lib PATH measures the same unsteered stage with another build of libyavo.so (the parent commit's) in a child
process of this one, before and after the rounds, so both sides of the ratio come from the same box and session.

    python tools/bench_steered_brief.py [--parent-lib ya_vo_amd/lib/libyavo_parent.so] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 256  # stereo frames per run: 512 images
MAX_KP = 2000
THR = 20


def _stats(v):
    return {"mean": round(float(np.mean(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
            "rounds": [round(float(x), 4) for x in v]}


def measure(a, modes):
    """-> {mode: [brief ms per run, one per round]}, {mode: [mean keypoints per image]}"""
    import torch
    import ya_vo_amd as yv
    from ya_vo_amd.steering import steering_tables
    from ya_vo_amd.synth import H_KITTI, W_KITTI, synth_stereo_batch

    if a.pre_steering_lib:  # the parent's library has none of the steering symbols to bind
        for name in ("yv_set_brief_steering", "yv_orient", "yv_batch_orient_view_get"):
            yv.SIGNATURES.pop(name, None)
    ctx = yv.Context(0)
    offsets = np.fromfile(os.path.join(ROOT, "tests", "golden", "brief_offsets_mt19937_42.bin"), np.int8)
    ctx.set_brief_offsets(offsets)
    images = synth_stereo_batch(1234, FRAMES)
    d = torch.from_numpy(images).to("cuda:0")
    torch.cuda.synchronize()
    n = len(images)
    batch = yv.Batch(ctx, n, H_KITTI, W_KITTI, MAX_KP, 2 * FRAMES)
    batch.set_pairs([(2 * k, 2 * k + 1) for k in range(FRAMES)] + [(2 * k - 2, 2 * k) for k in range(1, FRAMES)])
    tables = steering_tables(offsets.reshape(256, 4), a.bins) if "steered" in modes else None
    brief = {m: [] for m in modes}
    kps = {m: [] for m in modes}
    for _ in range(a.rounds):
        for mode in modes:
            if not a.pre_steering_lib:
                ctx.set_brief_steering(tables if mode == "steered" else None, a.radius)
            batch.enable_timing(False)
            for _ in range(a.warmup):
                batch.run(d.data_ptr(), n, W_KITTI, H_KITTI * W_KITTI, THR)
            ctx.sync()
            batch.enable_timing(True)
            for _ in range(a.steps):
                batch.run(d.data_ptr(), n, W_KITTI, H_KITTI * W_KITTI, THR)
            ctx.sync()
            ms, runs = batch.stage_times()
            brief[mode].append(float(ms[2]) / runs)
            kps[mode].append(float(ctx.download(batch.view().kp_count, np.int32, n).mean()))
    batch.enable_timing(False)
    batch.close()
    ctx.close()
    return brief, kps


def measure_parent(a):
    """The unsteered stage of another libyavo.so, in a fresh child process."""
    env = dict(os.environ, YAVO_LIB=os.path.abspath(a.parent_lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--modes", "unsteered", "--pre-steering-lib", "--rounds",
           str(a.rounds), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])["unsteered"]["rounds"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--radius", type=int, default=15)
    ap.add_argument("--modes", default="unsteered,steered")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pre-steering-lib", action="store_true", help="the library loaded (YAVO_LIB) predates steering")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    modes = a.modes.split(",")
    parent = []
    if a.parent_lib:
        parent += measure_parent(a)
    brief, kps = measure(a, modes)
    if a.parent_lib:
        parent += measure_parent(a)
    rec = {"shape": "376x1241", "images_per_run": 2 * FRAMES, "max_kp": MAX_KP, "steps": a.steps, "warmup": a.warmup,
           "bins": a.bins, "radius": a.radius, "unit": "ms per run, stage 2 (descriptors) by device events"}
    for m in modes:
        rec[m] = _stats(brief[m])
        rec[f"{m}_mean_kp"] = round(float(np.mean(kps[m])), 1)
    if parent:
        rec["parent_unsteered"] = _stats(parent)
    base = rec.get("parent_unsteered", rec.get("unsteered"))
    if base and "steered" in rec:
        rec["steered_over_unsteered"] = round(rec["steered"]["mean"] / base["mean"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
