"""Times of the bag-of-words keyframe index (yv_bow_query_batch / yv_bow_add_batch) at the bench's shape: the 4096 slots
of one bench step (2048 stereo frames, 2000 keypoints per image) queried against E stored keyframes with a vocabulary
of W words.

    python tools/bench_bow.py [--slots 4096] [--words 1024,4096] [--entries 1024,4096,16384] [--unique 64]

Prints one JSON object per (W, E).  Times: HIP events around `reps` back-to-back calls on one stream after a warm-up
call, inputs resident in HBM, the median of `windows` such windows and their range.  The four kernels are timed together
(a whole query call) and one at a time (yv_debug_bow_stages: a call that launches one kernel on what the last full call
left).  The yardstick of the word kernel is launch_match (yavo_match.hip, unchanged) over as many pairs of the same
sizes: `slots` query lists of 2000 descriptors against one train list of W descriptors (<= 2048: the FP4 matcher, above:
the int8 one), random bits, the train list shared by every pair as the vocabulary is; `words_over_match` is the ratio
of the two medians.  Achieved rates are operations counted from the shapes over the measured time.

The images are `unique` stereo frames of one synthetic field tiled over the slots (the kernels' work does not depend
on the descriptors' values; the histogram's LDS atomics see real word distributions).  Slot 0's words, vector and
candidates are compared with tests/bow_reference.py on every configuration."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W_IMG, MAX_KP = 376, 1241, 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--words", default="1024,4096")
    ap.add_argument("--entries", default="1024,4096,16384")
    ap.add_argument("--unique", type=int, default=64, help="distinct stereo frames tiled over the slots")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=4)
    args = ap.parse_args()
    import torch
    import ya_vo_amd as yv
    from ya_vo_amd import bow
    from ya_vo_amd.synth import synth_stereo_batch
    import bow_reference as ref

    S = args.slots
    ctx = yv.Context(0)
    ctx.set_brief_offsets(np.fromfile(os.path.join(ROOT, "tests", "golden", "brief_offsets_mt19937_42.bin"), np.int8))
    dev = "cuda:0"
    uniq = min(args.unique, (S + 1) // 2)
    imgs = torch.from_numpy(synth_stereo_batch(1234, uniq)).to(dev)  # [2 uniq, H, W]
    d_imgs = imgs.repeat((S + 2 * uniq - 1) // (2 * uniq), 1, 1)[:S].contiguous()
    del imgs
    ts = torch.cuda.Stream()  # one explicit stream for the library launches and the events
    torch.cuda.set_stream(ts)
    stream = ts.cuda_stream
    batch = yv.Batch(ctx, S, H, W_IMG, MAX_KP, 0)
    batch.run(d_imgs.data_ptr(), S, W_IMG, H * W_IMG, 20, stream=stream)
    torch.cuda.synchronize()
    v = batch.view()
    counts = ctx.download(v.kp_count, np.int32, S)
    kp0 = ctx.download(v.keypoints, yv.KEYPOINT_DTYPE, 2 * uniq * MAX_KP).reshape(2 * uniq, MAX_KP)
    pool = np.concatenate([kp0[i, :counts[i]]["featVec"] for i in range(2 * uniq)])
    slots, frames = np.arange(S, dtype=np.int32), np.arange(S, dtype=np.int64) + 10 ** 6

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

    n_desc = int(counts.sum())
    for n_words in [int(x) for x in args.words.split(",")]:
        words = bow.train_vocabulary(pool, n_words, 0, 0)
        idf = bow.idf_table([bow.assign_words(kp0[i, :counts[i]], words) for i in range(min(2 * uniq, 16))], n_words)
        idf = np.maximum(idf, 1).astype(np.uint16)  # the tiled images repeat: keep every word's weight positive
        w_pad = (n_words + 63) // 64 * 64

        # the yardstick: launch_match on `S` pairs (2000 queries each) against one shared train list of n_words
        g = torch.Generator(device=dev).manual_seed(n_words)
        d_desc = torch.randint(-2 ** 31, 2 ** 31 - 1, (S + 1, 4096, 8), dtype=torch.int32, device=dev, generator=g)
        d_cnt = torch.full((S + 1,), MAX_KP, dtype=torch.int32, device=dev)
        d_cnt[S] = n_words
        d_pairs = torch.stack([torch.arange(S, dtype=torch.int32), torch.full((S,), S, dtype=torch.int32)], 1).to(dev)
        d_keys = torch.zeros((S, 4096), dtype=torch.int32, device=dev)
        yard_pairs = min(S, 65535)

        def match():
            assert ctx.lib.yv_debug_match_keys(ctx.handle, d_desc.data_ptr(), d_cnt.data_ptr(), 4096,
                                               d_pairs.data_ptr(), yard_pairs, n_words, d_keys.data_ptr(), stream) == 0
        t_match = timed(match)
        del d_desc, d_keys

        for E in [int(x) for x in args.entries.split(",")]:
            idx = bow.BowIndex(ctx, words, idf, max_entries=E, max_queries=S, max_kp=MAX_KP)
            done = 0
            while done < E:  # the run's slots over and over, as many keyframes as asked for
                m = min(S, E - done)
                idx.add_batch(batch, slots[:m], np.arange(done, done + m, dtype=np.int64), stream=stream)
                done += m

            def query(mask=15):
                assert ctx.lib.yv_debug_bow_stages(idx.handle, mask) == 0
                idx.query_batch(batch, slots, frames, exclude=0, top_k=args.top_k, stream=stream)

            out = {"slots": S, "descriptors": n_desc, "words": n_words, "entries": E, "top_k": args.top_k,
                   "reps_per_window": args.reps, "windows": args.windows}
            out["query_all"] = timed(query)
            for name, mask in (("words", 1), ("vector", 2), ("score", 4), ("topk", 8)):
                out[name] = timed(lambda: query(mask))
            query()
            torch.cuda.synchronize()
            # operations from the shapes: 2 * 256 per descriptor-word pair, 2 * w_pad per query-entry pair
            out["words_tops"] = round(2.0 * 256 * n_desc * n_words / (out["words"]["ms_median"] * 1e-3) / 1e12, 2)
            out["score_tops"] = round(2.0 * w_pad * S * E / (out["score"]["ms_median"] * 1e-3) / 1e12, 2)
            out["match_yardstick"] = t_match
            out["match_yardstick_tops"] = round(2.0 * 256 * yard_pairs * MAX_KP * n_words /
                                                (t_match["ms_median"] * 1e-3) / 1e12, 2)
            # per descriptor: the yardstick's pairs hold 2000 each, the slots counts[i]
            per_word = out["words"]["ms_median"] / n_desc
            per_match = t_match["ms_median"] / (yard_pairs * MAX_KP)
            out["words_over_match"] = round(per_word / per_match, 3)
            # slot 0 against the specification
            spec = ref.Index(words, idf)
            for e in range(min(E, 2 * uniq)):
                spec.add(kp0[e % (2 * uniq), :counts[e % (2 * uniq)]]["featVec"], e)
            vw = idx.view()
            d0 = kp0[0, :counts[0]]["featVec"]
            w0, _ = ref.words_of(d0, words)
            v0, n0 = spec.vector(d0)
            ok = np.array_equal(ctx.download(vw.q_word, np.int32, int(counts[0])), w0)
            ok = ok and np.array_equal(ctx.download(vw.q_vectors, np.int8, n_words), v0)
            ok = ok and int(ctx.download(vw.q_norm2, np.int32, 1)[0]) == n0
            if E <= 2 * uniq:  # the whole index is in the specification's: the candidates as well
                exp = spec.query(d0, int(frames[0]), 0, args.top_k)[0]
                got = ctx.download(vw.cand_entry, np.int32, 16)[:len(exp)]
                ok = ok and list(got) == [e for e, _, _ in exp]
            out["slot0_bit_identical"] = bool(ok)
            print(json.dumps(out), flush=True)
            idx.close()
    batch.close()
    ctx.close()


if __name__ == "__main__":
    main()
