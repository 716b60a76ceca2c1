#!/usr/bin/env python3
"""Stage times of the gated matcher against the ungated one, in one process.

The bench's pair layout through FrameShard (temporal L_{k-1} -> L_k and stereo L_k -> R_k per frame, the halo frame in
the same run), Batch.enable_timing / stage_times, the mean of --steps timed steps per mode; the modes alternate
gates off / gates on for --rounds rounds.  Gates: stereo (-2, 2, -128, 0), temporal (-40, 40, -60, 60).  Reports slot 3
(the order of every slot + the matcher; ungated: the matcher), slot 4 (finalize), the kept records and the pose edges
per step, one JSON line per measurement and one summary line.

    python tools/bench_match_gate.py --frames 2048 [--filter] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEREO = (-2, 2, -128, 0)
TEMPORAL = (-40, 40, -60, 60)
T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--filter", action="store_true", help="ratio 4/5 + mutual on in both modes (top-2 + swapped pairs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

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
    # FrameShard's pairs: temporal (L_{k-1}, L_k), then stereo (L_k, R_k), per frame
    gates = [TEMPORAL if p % 2 == 0 else STEREO for p in range(len(shard.pairs))]
    if a.filter:
        batch.set_match_filter(ratio=(4, 5), mutual=True)

    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    summary = {"frames": B, "pairs": len(shard.pairs), "filter": bool(a.filter), "steps": a.steps,
               "gates": {"stereo": STEREO, "temporal": TEMPORAL}}
    for rnd in range(a.rounds):
        for mode in ("off", "gated"):
            batch.set_match_gates(gates if mode == "gated" else None)
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
            kp = ctx.download(v.kp_count, np.int32, shard.n_images)
            filt = ctx.download(v.filt_count, np.int32, len(shard.pairs))
            edges = ctx.download(v.edge_count, np.int32, shard.n_tracks)
            inl = ctx.download(v.track_inliers, np.int32, shard.n_tracks)
            rec = {"round": rnd, "mode": mode, "runs": n, "match_ms": round(float(ms[3]) / n, 4),
                   "finalize_ms": round(float(ms[4]) / n, 4), "track_edges_ms": round(float(ms[5]) / n, 4),
                   "track_pose_ms": round(float(ms[6]) / n, 4), "mean_kp": round(float(kp.mean()), 1),
                   "filtered_temporal": int(filt[0::2].sum()), "filtered_stereo": int(filt[1::2].sum()),
                   "edges_total": int(edges.sum()), "inliers_total": int(inl.sum())}
            emit(rec)
            summary[f"{mode}_{rnd}"] = rec
    batch.enable_timing(False)
    off = [summary[f"off_{r}"]["match_ms"] for r in range(a.rounds)]
    on = [summary[f"gated_{r}"]["match_ms"] for r in range(a.rounds)]
    summary["gated_not_above_ungated"] = bool(max(on) <= min(off))
    emit(summary)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    shard.close()
    ctx.close()
    return 0 if summary["gated_not_above_ungated"] else 1


if __name__ == "__main__":
    sys.exit(main())
