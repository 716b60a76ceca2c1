#!/usr/bin/env python3
"""The BA window's multi-view mode against the two-view window on the sequence leg: the front end of
tools/bench_sequence.py's timed loop (synthetic frames resident in HBM, device window, chunks of 20) run with
SequenceFrontend(multiview=False) and (multiview=True) alternating in one process, `--repeats` timed runs each after
one warm-up run each.  Reports per mode the median frames/s (min / max beside it), the window solve's time on the BA
stream (HIP events around every solve_begin, in an extra untimed run: graph build + LM + write-back, beside the next
chunk's front end as in the timed loop), the windows' landmarks, edges and mean observations per landmark, and the
trajectory RMSE against the synthetic ground truth at every length of `--rmse-frames`.

    python tools/bench_window_tracks.py [--frames 1000] [--chunk 20] [--repeats 5] [--rmse-frames 200,1000,2000]
                                        [--out f.json]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)


def window_stats(fe, n, chunk, n_fixed, multiview):
    """Landmarks and edges of every window the run solved, from the recorded counts and links."""
    counts = [len(fe.win.read(g)[1]) for g in range(n)]
    roots = [int((fe.win.read_links(g)[2] < 0).sum()) for g in range(n)] if multiview else counts
    L = E = 0
    for last in range(chunk - 1, n, chunk):
        lo = max(0, last - (chunk + n_fixed) + 1)
        nodes = sum(counts[lo + 1:last + 1])
        lm = (counts[lo + 1] + sum(roots[lo + 2:last + 1])) if last > lo else 0
        L += lm
        E += nodes + lm
    return L, E


def measure(frames=1000, chunk=20, n_fixed=2, ba_iters=10, repeats=5, rmse_frames=(200, 1000, 2000)):
    import torch
    import ya_vo_amd as yv
    from ya_vo_amd import scene
    from ya_vo_amd.sequence import SequenceFrontend
    from ya_vo_amd.synth import synth_sequence
    from sequence_chain import ground_truth, rmse_translation

    K = scene.K_KITTI
    longest = max([frames] + list(rmse_frames))
    if any(m % chunk for m in [frames] + list(rmse_frames)):
        raise ValueError("frames and rmse-frames must be multiples of chunk")
    fr = synth_sequence(1234, longest, stereo=True)
    H, W = fr.shape[2:]
    ctx = yv.Context(0)
    ctx.set_brief_offsets(np.fromfile(os.path.join(ROOT, "tests", "golden", "brief_offsets_mt19937_42.bin"), np.int8))
    d = torch.from_numpy(fr.reshape(2 * longest, H, W)).to(torch.device("cuda", ctx.device))
    torch.cuda.synchronize()

    def run(m, multiview, events=None):
        fe = SequenceFrontend(ctx, chunk, K, T_RIGHT, n_fixed=n_fixed, ba_iters=ba_iters, H=H, W=W,
                              expected_frames=m, multiview=multiview)
        if events is not None:  # HIP events on the BA stream around every window's build + solve + write-back
            begin = fe._local_ba_device_begin

            def timed_begin():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(fe.ba_stream)
                begin()
                b.record(fe.ba_stream)
                events.append((a, b))
            fe._local_ba_device_begin = timed_begin
        gc.collect()
        gc.disable()
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c in range(m // chunk):
                fe.process_chunk(d[2 * c * chunk:2 * (c + 1) * chunk])
            fe.flush()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            gc.enable()
        return fe, dt

    modes = (("two_view", False), ("multi_view", True))
    times = {name: [] for name, _ in modes}
    for name, mv in modes:  # warm-up (first launches, allocations)
        run(frames, mv)[0].close()
    for _ in range(repeats):
        for name, mv in modes:
            fe, dt = run(frames, mv)
            times[name].append(dt)
            fe.close()
    out = {"workload": f"sequence leg, {frames} synthetic frames resident in HBM, chunks of {chunk}, windows of "
                       f"{chunk + n_fixed} poses ({n_fixed} fixed), {ba_iters} LM iterations, device window, 1 x MI355X",
           "statistic": f"median of {repeats} runs per mode, the modes alternating in one process after a warm-up "
                        "run each"}
    for name, mv in modes:
        t = times[name]
        t_med = float(np.median(t))
        ev = []
        fe, _ = run(frames, mv, ev)
        solve_ms = [a.elapsed_time(b) for a, b in ev]
        L, E = window_stats(fe, frames, chunk, n_fixed, mv)
        log = list(fe.ba_log)
        fe.close()
        res = {"frames_per_s": round(frames / t_med, 2), "frames_per_s_min": round(frames / max(t), 2),
               "frames_per_s_max": round(frames / min(t), 2), "seconds_all_runs": [round(x, 4) for x in t],
               "window_solves": len(log), "window_solve_ms_median": round(float(np.median(solve_ms)), 4),
               "window_solve_ms_mean": round(float(np.mean(solve_ms)), 4),
               "window_landmarks": L, "window_edges": E, "observations_per_landmark": round(E / max(L, 1), 3),
               "lm_iterations_mean": round(float(np.mean([x[1] for x in log])), 2),
               "chi2_last_over_first_mean": round(float(np.mean([x[3] / x[2] for x in log])), 4),
               "rmse_vs_ground_truth_m": {}}
        for m in rmse_frames:
            fe, _ = run(m, mv)
            res["rmse_vs_ground_truth_m"][str(m)] = rmse_translation(fe.trajectory(), ground_truth(m, K))
            fe.close()
        out[name] = res
    out["multi_over_two_view_frames_per_s"] = round(out["multi_view"]["frames_per_s"] / out["two_view"]["frames_per_s"], 4)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--n-fixed", type=int, default=2)
    ap.add_argument("--ba-iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rmse-frames", default="200,1000,2000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = measure(args.frames, args.chunk, args.n_fixed, args.ba_iters, args.repeats,
                  tuple(int(x) for x in args.rmse_frames.split(",") if x))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
