"""The deferred match-records kernel without a detect beside it: the bench's shard (2048 frames, overlap mode 1), every
step drained before the next, so match_records_kernel runs beside the edge build and the LM only.  Meant for a kernel
trace, whose match_records_kernel durations are the "alone" figure next to the plain bench's "beside detect" one:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o trace -- python tools/bench_records.py [--steps 6]
    python tools/kernel_by_grid.py OUT/trace_kernel_trace.csv match_records_kernel

On its own it prints the host time of a drained step."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--frames", type=int, default=2048)
    args = ap.parse_args()
    import torch
    import ya_vo_amd as yv
    from ya_vo_amd import scene
    from ya_vo_amd.sharding import FrameShard, shard_images
    from ya_vo_amd.synth import synth_stereo_batch

    T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
    offsets = np.fromfile(os.path.join(ROOT, "tests", "golden", "brief_offsets_mt19937_42.bin"), np.int8)
    ctx = yv.Context(0)
    ctx.set_brief_offsets(offsets)
    B = args.frames
    fr = synth_stereo_batch(1234, B + 1, start=0)
    d_frames = torch.from_numpy(shard_images(fr[2:], fr[0], None)).to("cuda:0")
    del fr
    shard = FrameShard(ctx, B, 1, scene.K_KITTI, T_RIGHT, halo=True, overlap_mode=1)
    for _ in range(2):
        shard.step(d_frames.data_ptr())
        shard.drain()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        shard.step(d_frames.data_ptr())
        shard.drain()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(f"drained step: {ms:.3f} ms over {args.steps} steps of {B} frames")
    shard.close()
    ctx.close()


if __name__ == "__main__":
    main()
