#!/usr/bin/env python3
"""Stage times of the keypoint selection against the plain cut, in one process.

The bench's pair layout through FrameShard (temporal L_{k-1} -> L_k and stereo L_k -> R_k per frame, the halo frame in
the same run), Batch.enable_timing / stage_times, the mean of --steps timed steps per mode; the modes alternate
selection off / on for --rounds rounds.  Reports slot 1 (top-K + checkBoundry; with selection on the selection kernels
run inside it), the kept keypoints per image, the kept temporal and stereo records, the pose edges and inliers and the
non-empty 32 x 32 cells per image (over the first --sample images), one JSON line per measurement and one summary line.

    python tools/bench_keypoint_select.py --frames 2048 --select 1,32,32,6 [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
CELL = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--select", default="1,32,32,6", help="nms_radius,cell_rows,cell_cols,per_cell (per_cell 0: no quota)")
    ap.add_argument("--sample", type=int, default=64, help="images whose keypoints are read back for the cell count")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r, cr, cc, q = (int(x) for x in a.select.split(","))

    import torch
    import ya_vo_amd as yv
    from ya_vo_amd import scene
    from ya_vo_amd.sharding import FrameShard, shard_images
    from ya_vo_amd.synth import synth_stereo_batch

    ctx = yv.Context(0)
    ctx.set_brief_offsets(np.fromfile(os.path.join(ROOT, "tests", "golden", "brief_offsets_mt19937_42.bin"), np.int8))
    B = a.frames
    fr = synth_stereo_batch(1234, B + 1, start=0)
    images = shard_images(fr[2:], fr[0], None)
    del fr
    d_frames = torch.from_numpy(images).to("cuda:0")
    # in order: every stage's events bracket its own kernels only
    shard = FrameShard(ctx, B, 1, scene.K_KITTI, T_RIGHT, halo=True, overlap_mode=0)
    batch = shard.batch
    H, W, K = batch.H, batch.W, batch.max_kp
    n_cells = ((H + CELL - 1) // CELL) * ((W + CELL - 1) // CELL)

    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    summary = {"frames": B, "pairs": len(shard.pairs), "steps": a.steps, "select": [r, cr, cc, q],
               "cells_per_image": n_cells}
    for rnd in range(a.rounds):
        for mode in ("off", "select"):
            if mode == "select":
                ctx.set_keypoint_select(r, (cr, cc) if q > 0 else None, q)
            else:
                ctx.set_keypoint_select()
            batch.enable_timing(False)
            for _ in range(a.warmup):
                shard.step(d_frames.data_ptr())
            shard.drain()
            batch.enable_timing(True)
            for _ in range(a.steps):
                shard.step(d_frames.data_ptr())
            shard.drain()
            ms, n = batch.stage_times()
            v = batch.view()
            cand = ctx.download(v.cand_count, np.uint32, shard.n_images)
            kp = ctx.download(v.kp_count, np.int32, shard.n_images)
            filt = ctx.download(v.filt_count, np.int32, len(shard.pairs))
            edges = ctx.download(v.edge_count, np.int32, shard.n_tracks)
            inl = ctx.download(v.track_inliers, np.int32, shard.n_tracks)
            occupied = []
            for i in range(min(a.sample, shard.n_images)):
                k = ctx.download(v.keypoints + i * K * 48, yv.KEYPOINT_DTYPE, int(kp[i]))
                occupied.append(len(np.unique((k["x"] // CELL) * ((W + CELL - 1) // CELL) + k["y"] // CELL)))
            rec = {"round": rnd, "mode": mode, "runs": n, "detect_ms": round(float(ms[0]) / n, 4),
                   "topk_ms": round(float(ms[1]) / n, 4), "brief_ms": round(float(ms[2]) / n, 4),
                   "match_ms": round(float(ms[3]) / n, 4), "mean_corners": round(float(cand.mean()), 1),
                   "mean_kp": round(float(kp.mean()), 1), "filtered_temporal": int(filt[0::2].sum()),
                   "filtered_stereo": int(filt[1::2].sum()), "edges_total": int(edges.sum()),
                   "inliers_total": int(inl.sum()), "mean_nonempty_cells": round(float(np.mean(occupied)), 1)}
            emit(rec)
            summary[f"{mode}_{rnd}"] = rec
    ctx.set_keypoint_select()
    batch.enable_timing(False)
    off = [summary[f"off_{k}"]["topk_ms"] for k in range(a.rounds)]
    on = [summary[f"select_{k}"]["topk_ms"] for k in range(a.rounds)]
    summary["topk_ms_off"] = off
    summary["topk_ms_select"] = on
    summary["selection_ms"] = round(float(np.mean(on) - np.mean(off)), 4)
    emit(summary)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    shard.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
