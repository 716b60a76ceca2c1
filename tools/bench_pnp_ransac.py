"""Time of the P3P-RANSAC absolute pose (yv_pnp_ransac_batch) beside the pose LM (yv_pose_lm_batch) on the same
problems, at the bench's shape: 2048 problems (one per frame of a bench step) of 2000 edges, 64 hypotheses.

    python tools/bench_pnp_ransac.py [--problems 2048] [--n 2000] [--iters 64] [--outliers 0.5]

Prints one JSON object.  Times: HIP events around `reps` back-to-back launches on one stream after a warm-up launch,
inputs resident in HBM, the median of `windows` such windows and their range.  The scenes are
ya_vo_amd.scene.random_scene (0.3 px noise) with the world moved far from the identity (tests/pnp_scenes.py); the LM is
timed from the RANSAC's poses (its use) and from the identity (what it replaces).  Problem 0 is compared with the
specification tests/pnp_ransac_reference.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=2048)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--outliers", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    import torch
    import ya_vo_amd as yv
    import pnp_ransac_reference as ref
    from pnp_scenes import IDENTITY, K9, pnp_scene

    ctx = yv.Context(0)
    dev = "cuda:0"
    P, n, iters = args.problems, args.n, args.iters
    probs = [pnp_scene(n, seed=1000 + i, outlier_frac=args.outliers) for i in range(P)]
    draws = yv.ransac_draws(iters, 0)
    d_off = torch.from_numpy((np.arange(P + 1) * n).astype(np.int32)).to(dev)
    d_X = torch.from_numpy(np.concatenate([p[0] for p in probs])).to(dev)
    d_uv = torch.from_numpy(np.concatenate([p[1] for p in probs])).to(dev)
    d_K = torch.from_numpy(np.tile(K9, (P, 1))).to(dev)
    d_draws = torch.from_numpy(draws.view(np.int32)).to(dev)
    d_ident = torch.from_numpy(np.tile(IDENTITY, (P, 1))).to(dev)
    d_pose = d_ident.clone()
    d_lm = d_ident.clone()
    d_mask = torch.zeros(P * n, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(P * n, dtype=torch.uint8, device=dev)
    d_inl = torch.zeros(P, dtype=torch.int32, device=dev)
    d_found = torch.zeros(P, dtype=torch.int32, device=dev)
    d_res = torch.zeros(P, dtype=torch.int32, device=dev)
    ts = torch.cuda.Stream()  # one explicit stream for the library launches, the copies and the events
    torch.cuda.set_stream(ts)
    stream = ts.cuda_stream

    def ransac():
        ctx.pnp_ransac_batch(P, d_off.data_ptr(), d_X.data_ptr(), d_uv.data_ptr(), d_K.data_ptr(),
                             d_draws.data_ptr(), iters, d_pose.data_ptr(), d_mask.data_ptr(), d_inl.data_ptr(),
                             d_found.data_ptr(), thr=2.0, min_inliers=12, stream=stream)

    def lm_from(d_prior):
        def fn():
            d_lm.copy_(d_prior)
            assert ctx.lib.yv_pose_lm_batch(ctx.handle, P, d_off.data_ptr(), d_X.data_ptr(), d_uv.data_ptr(),
                                            d_K.data_ptr(), d_lm.data_ptr(), d_out.data_ptr(), d_res.data_ptr(),
                                            stream) == 0
        return fn

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

    out = {"problems": P, "edges_per_problem": n, "hypotheses": iters, "outlier_fraction": args.outliers,
           "reps_per_window": args.reps, "windows": args.windows}
    out["pnp_ransac_batch"] = timed(ransac)
    torch.cuda.synchronize()
    clean = np.stack([p[3] for p in probs])
    mask = d_mask.cpu().numpy().reshape(P, n).astype(bool)
    found = d_found.cpu().numpy()
    out["found"] = int(found.sum())
    out["clean_edges_kept"] = round(float((mask & clean).sum() / clean.sum()), 5)
    out["outliers_accepted"] = int((mask & ~clean).sum())
    w = ref.pnp_ransac(probs[0][0], probs[0][1], K9, draws, 2.0, 12, IDENTITY)
    out["problem0_bit_identical"] = bool(d_pose[0].cpu().numpy().tobytes() == w[0].tobytes() and
                                         np.array_equal(mask[0], w[1]) and int(d_inl[0]) == w[2])
    d_ransac_pose = d_pose.clone()
    for name, prior in (("pose_lm_from_ransac", d_ransac_pose), ("pose_lm_from_identity", d_ident)):
        t = timed(lm_from(prior))
        torch.cuda.synchronize()
        kept = ~d_out.cpu().numpy().reshape(P, n).astype(bool)
        t["clean_edges_kept"] = round(float((kept & clean).sum() / clean.sum()), 5)
        out[name] = t
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
