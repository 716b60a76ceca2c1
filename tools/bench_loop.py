"""Times of the loop-closure verification (yv_loop_verify_batch) and of the keyframe store's add (yv_loop_add_batch) at
the bench's shape: query slots of 2000 keypoints, top_k candidates each, 64 P3P hypotheses per problem.

    python tools/bench_loop.py [--problems 256,1024,4096] [--unique 64] [--add-entries 2048]

Prints one JSON object per problem count and one for the add.  Times: HIP events around `reps` back-to-back calls on
one stream after a warm-up call, inputs resident in HBM, the median of `windows` such windows and their range.

The scene: `unique` synthetic stereo frames through one Batch run; every left image is a keyframe (added from the batch
with its stereo landmarks); query q is left slot q % unique with the candidate row [its own keyframe, the next three].
The frames are consecutive frames of one synthetic sequence, a few pixels apart, so every candidate overlaps its query
almost fully and is verified (`verified` and `edges_mean_verified` in the output say so): the most expensive mix, every
problem with about 1900 edges through the RANSAC and the LM.  A verify call is timed whole and stage by stage (yv_debug_loop_stages: a call that launches one stage on what the
last full call left).  The yardsticks of the three reused stages are the same launchers called alone on the same shapes:
launch_match with second-best keys over as many pairs of random 2000-descriptor lists plus the reverse direction
(yv_debug_loop_match), yv_pnp_ransac_batch and yv_pose_lm_batch over the call's own edges compacted into the offsets
layout (the LM from the RANSAC poses, over the problems the RANSAC found).  `glue_share` is the four glue stages' time
(stage + pairs, edges, gate, result) over the whole call's.  Problem 0's counts are compared with the host form's on every
size."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W_IMG, MAX_KP = 376, 1241, 2000
STAGES = (("stage_pairs", 1), ("match", 2), ("finalize", 4), ("edges", 8), ("ransac", 16), ("gate", 32), ("lm", 64),
          ("result", 128))
GLUE = ("stage_pairs", "edges", "gate", "result")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="256,1024,4096")
    ap.add_argument("--unique", type=int, default=64, help="distinct stereo frames = keyframes of the store")
    ap.add_argument("--add-entries", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--iters", type=int, default=64)
    args = ap.parse_args()
    import torch
    import ya_vo_amd as yv
    from ya_vo_amd import bow, loop, scene
    from ya_vo_amd.synth import synth_stereo_batch

    U, top_k = args.unique, args.top_k
    sizes = [int(x) for x in args.problems.split(",")]
    ctx = yv.Context(0)
    ctx.set_brief_offsets(np.fromfile(os.path.join(ROOT, "tests", "golden", "brief_offsets_mt19937_42.bin"), np.int8))
    dev = "cuda:0"
    d_imgs = torch.from_numpy(synth_stereo_batch(1234, U)).to(dev)  # [2 U, H, W]: L_k, R_k interleaved
    ts = torch.cuda.Stream()  # one explicit stream for the library launches and the events
    torch.cuda.set_stream(ts)
    stream = ts.cuda_stream
    batch = yv.Batch(ctx, 2 * U, H, W_IMG, MAX_KP, U)
    batch.set_pairs([(2 * k, 2 * k + 1) for k in range(U)])
    batch.run(d_imgs.data_ptr(), 2 * U, W_IMG, H * W_IMG, 20, stream=stream)
    torch.cuda.synchronize()
    K, T_right = scene.K_KITTI, np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)  # bench.py's rig
    counts = ctx.download(batch.view().kp_count, np.int32, 2 * U)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.reps)
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    left = [2 * k for k in range(U)]
    for P in sizes:
        nq = P // top_k
        lv = loop.LoopVerifier(ctx, K, T_right, max_entries=U, max_problems=P, max_kp=MAX_KP)
        lv.set_params(20, 3, 4, 5, args.iters, 2.0, 12, seed=0)
        lv.add_batch(batch, left, list(range(U)), list(range(U)), stream=stream)
        slots = np.array([left[q % U] for q in range(nq)], np.int32)
        cand = np.full((nq, 16), -1, np.int32)
        for q in range(nq):
            cand[q, :top_k] = [(q + k) % U for k in range(top_k)]
        d_cand = torch.from_numpy(cand).to(dev)
        d_count = torch.full((nq,), top_k, dtype=torch.int32, device=dev)

        def verify(mask=255):
            assert ctx.lib.yv_debug_loop_stages(lv.handle, mask) == 0
            lv.verify_batch(batch, slots, d_cand.data_ptr(), d_count.data_ptr(), top_k, stream=stream)

        out = {"problems": P, "queries": nq, "top_k": top_k, "keyframes": U, "iters": args.iters,
               "keypoints_mean": round(float(counts[0::2].mean()), 1), "reps_per_window": args.reps,
               "windows": args.windows}
        out["verify_all"] = timed(verify)
        for name, mask in STAGES:
            verify()  # what the stage reads: a full call's
            out[name] = timed(lambda: verify(mask))
        verify()
        torch.cuda.synchronize()
        res = lv.results()
        out["verified"] = int(res["verified"].sum())
        out["edges_mean_verified"] = round(float(res["n_edges"][res["verified"] == 1].mean()), 1)
        glue = sum(out[g]["ms_median"] for g in GLUE)
        out["glue_ms"] = round(glue, 4)
        out["glue_share"] = round(glue / out["verify_all"]["ms_median"], 4)
        out["stages_sum_ms"] = round(sum(out[name]["ms_median"] for name, _ in STAGES), 4)

        # ---- yardstick: the matcher alone, P pairs of random 2000-descriptor lists, forward (top 2) + reverse ----
        g = torch.Generator(device=dev).manual_seed(P)
        n_lists = min(2 * P, 2048)
        d_desc = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_lists, MAX_KP, 8), dtype=torch.int32, device=dev, generator=g)
        d_cnt = torch.full((n_lists,), MAX_KP, dtype=torch.int32, device=dev)
        pr = np.stack([np.arange(P) % n_lists, (np.arange(P) + n_lists // 2) % n_lists], 1).astype(np.int32)
        d_pairs = torch.from_numpy(pr).to(dev)
        d_pairs_rev = torch.from_numpy(np.ascontiguousarray(pr[:, ::-1])).to(dev)
        d_k1 = torch.zeros((P, MAX_KP), dtype=torch.int32, device=dev)
        d_k2 = torch.zeros((P, MAX_KP), dtype=torch.int32, device=dev)
        d_kr = torch.zeros((P, MAX_KP), dtype=torch.int32, device=dev)

        def match():
            assert ctx.lib.yv_debug_loop_match(ctx.handle, d_desc.data_ptr(), d_cnt.data_ptr(), MAX_KP,
                                               d_pairs.data_ptr(), P, MAX_KP, d_k1.data_ptr(), d_k2.data_ptr(),
                                               stream) == 0
            assert ctx.lib.yv_debug_loop_match(ctx.handle, d_desc.data_ptr(), d_cnt.data_ptr(), MAX_KP,
                                               d_pairs_rev.data_ptr(), P, MAX_KP, d_kr.data_ptr(), None, stream) == 0
        out["match_yardstick"] = timed(match)
        del d_desc, d_k1, d_k2, d_kr

        # ---- yardsticks: yv_pnp_ransac_batch / yv_pose_lm_batch over the call's edges in the offsets layout ----
        v = lv.view()
        ne = ctx.download(v.edge_count, np.int32, P)
        off = np.concatenate([[0], np.cumsum(ne)]).astype(np.int32)
        Xs, uvs = np.zeros((max(int(off[-1]), 1), 3)), np.zeros((max(int(off[-1]), 1), 2))
        for p in np.flatnonzero(ne):
            Xs[off[p]:off[p + 1]] = ctx.download(v.edge_X + 24 * MAX_KP * int(p), np.float64, 3 * int(ne[p])).reshape(-1, 3)
            uvs[off[p]:off[p + 1]] = ctx.download(v.edge_uv + 16 * MAX_KP * int(p), np.float64, 2 * int(ne[p])).reshape(-1, 2)
        d_off, d_X, d_uv = (torch.from_numpy(a).to(dev) for a in (off, Xs, uvs))
        d_K = torch.from_numpy(np.tile(np.asarray(K, np.float64).reshape(9), (P, 1))).to(dev)
        d_draws = torch.from_numpy(yv.ransac_draws(args.iters, 0).view(np.int32)).to(dev)  # the uint32 bits
        ident = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (P, 1))
        d_prior, d_pose = torch.from_numpy(ident).to(dev), torch.from_numpy(ident.copy()).to(dev)
        d_mask = torch.zeros(max(int(off[-1]), 1), dtype=torch.uint8, device=dev)
        d_inl, d_found = (torch.zeros(P, dtype=torch.int32, device=dev) for _ in range(2))

        def ransac():
            d_pose.copy_(d_prior)
            assert ctx.lib.yv_pnp_ransac_batch(ctx.handle, P, d_off.data_ptr(), d_X.data_ptr(), d_uv.data_ptr(),
                                               d_K.data_ptr(), d_draws.data_ptr(), args.iters, 2.0, 12,
                                               d_pose.data_ptr(), d_mask.data_ptr(), d_inl.data_ptr(),
                                               d_found.data_ptr(), stream) == 0
        out["ransac_yardstick"] = timed(ransac)
        torch.cuda.synchronize()
        found = d_found.cpu().numpy() != 0
        out["yardstick_found"] = int(found.sum())
        off_lm = np.concatenate([[0], np.cumsum(np.where(found, ne, 0))]).astype(np.int32)
        keep_rows = np.concatenate([np.arange(off[p], off[p + 1]) for p in np.flatnonzero(found)] or
                                   [np.zeros(0, np.int64)]).astype(np.int64)
        d_off_lm = torch.from_numpy(off_lm).to(dev)
        d_X_lm = torch.from_numpy(np.ascontiguousarray(Xs[keep_rows]) if len(keep_rows) else np.zeros((1, 3))).to(dev)
        d_uv_lm = torch.from_numpy(np.ascontiguousarray(uvs[keep_rows]) if len(keep_rows) else np.zeros((1, 2))).to(dev)
        d_start = d_pose.clone()
        d_out = torch.zeros(max(len(keep_rows), 1), dtype=torch.uint8, device=dev)

        def lm():
            d_pose.copy_(d_start)
            assert ctx.lib.yv_pose_lm_batch(ctx.handle, P, d_off_lm.data_ptr(), d_X_lm.data_ptr(), d_uv_lm.data_ptr(),
                                            d_K.data_ptr(), d_pose.data_ptr(), d_out.data_ptr(), d_inl.data_ptr(),
                                            stream) == 0
        out["lm_yardstick"] = timed(lm)

        # problem 0 against the host form (which the GPU tests hold to the specification)
        kp0 = ctx.download(batch.view().keypoints, yv.KEYPOINT_DTYPE, int(counts[0]))
        host = lv.verify(kp0, [int(cand[0, 0])])[0]
        ints = ("entry", "n_kept", "n_edges", "ransac_inliers", "lm_inliers", "verified")
        out["problem0_counts_equal_host_form"] = bool(all(host[f] == res[0][f] for f in ints))
        # (the host form's LM sums in yv_loop_lm_sum_mode(1), the call's in yv_loop_lm_sum_mode(P): the same bits only
        # where the two modes are the same)
        out["problem0_pose_max_abs_diff"] = float(np.abs(host["pose"] - res[0]["pose"]).max())
        out["lm_sum_modes"] = [loop.lm_sum_mode(1), loop.lm_sum_mode(P)]
        print(json.dumps(out), flush=True)
        lv.close()

    # ---- one add of `add_entries` keyframes against the yv_bow_add_batch of the same slots ----
    E = args.add_entries
    slots = np.array([left[i % U] for i in range(E)], np.int32)
    pairs = np.array([i % U for i in range(E)], np.int32)
    fids = np.arange(E, dtype=np.int64)
    lv = loop.LoopVerifier(ctx, K, T_right, max_entries=E, max_problems=4, max_kp=MAX_KP)
    kp_all = ctx.download(batch.view().keypoints, yv.KEYPOINT_DTYPE, 2 * U * MAX_KP).reshape(2 * U, MAX_KP)
    pool = np.concatenate([kp_all[i, :counts[i]]["featVec"] for i in range(0, 2 * U, 2)])
    words = bow.train_vocabulary(pool, 1024, 0, 0)
    idx = bow.BowIndex(ctx, words, None, max_entries=E, max_queries=E, max_kp=MAX_KP)

    def add_loop():
        lv.reset()
        lv.add_batch(batch, slots, pairs, fids, stream=stream)

    def add_bow():
        idx.reset()
        idx.add_batch(batch, slots, fids, stream=stream)
    out = {"add_entries": E, "keyframes": U, "reps_per_window": args.reps, "windows": args.windows,
           "loop_add_batch": timed(add_loop), "bow_add_batch_1024_words": timed(add_bow)}
    out["loop_over_bow"] = round(out["loop_add_batch"]["ms_median"] / out["bow_add_batch_1024_words"]["ms_median"], 3)
    print(json.dumps(out), flush=True)
    lv.close()
    idx.close()
    batch.close()
    ctx.close()


if __name__ == "__main__":
    main()
