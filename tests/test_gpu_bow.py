"""GPU parity of the bag-of-binary-words keyframe index (yv_bow_*, ya_vo_amd/csrc/yavo_bow.hip) against the numpy
specification (tests/bow_reference.py): every array of the view is compared bit for bit."""
import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import bow

import bow_reference as ref
import bow_scenes

pytestmark = pytest.mark.gpu

K16 = 16


def _rand_desc(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def _near(rng, words, n, flips=20):
    """n descriptors a few bit flips away from random words (so the distances and the histograms are uneven)"""
    d = words[rng.integers(0, len(words), n)].copy()
    for _ in range(flips):
        d[np.arange(n), rng.integers(0, 32, n)] ^= (1 << rng.integers(0, 8, n)).astype(np.uint8)
    return d


def _vocabulary(rng, W):
    words = _rand_desc(rng, W)
    if W >= 3:  # duplicate words: the first index wins
        words[W - 1] = words[0]
        words[W // 2] = words[0]
    return words


def _view_arrays(ctx, idx):
    """every array of the view, cut to the entries / queries in use"""
    v = idx.view()
    E, Q, wp = v.n_entries, v.n_queries, v.w_pad
    dl = ctx.download
    out = dict(v=v)
    out["vectors"] = dl(v.vectors, np.int8, max(E, 1) * wp).reshape(-1, wp)[:E]
    out["norm2"] = dl(v.norm2, np.int32, max(E, 1))[:E]
    out["frame_id"] = dl(v.frame_id, np.int64, max(E, 1))[:E]
    out["q_word"] = dl(v.q_word, np.int32, max(Q, 1) * v.max_kp).reshape(-1, v.max_kp)[:Q]
    out["q_dist"] = dl(v.q_dist, np.int32, max(Q, 1) * v.max_kp).reshape(-1, v.max_kp)[:Q]
    out["q_vectors"] = dl(v.q_vectors, np.int8, max(Q, 1) * wp).reshape(-1, wp)[:Q]
    out["q_norm2"] = dl(v.q_norm2, np.int32, max(Q, 1))[:Q]
    out["dots"] = dl(v.dots, np.int32, max(Q, 1) * v.max_entries).reshape(-1, v.max_entries)[:Q, :E]
    out["cand_entry"] = dl(v.cand_entry, np.int32, max(Q, 1) * K16).reshape(-1, K16)[:Q]
    out["cand_score"] = dl(v.cand_score, np.float64, max(Q, 1) * K16).reshape(-1, K16)[:Q]
    out["cand_dot"] = dl(v.cand_dot, np.int32, max(Q, 1) * K16).reshape(-1, K16)[:Q]
    out["cand_count"] = dl(v.cand_count, np.int32, max(Q, 1))[:Q]
    return out


def _check_index(ctx, idx, spec):
    a = _view_arrays(ctx, idx)
    W = spec.n_words
    assert a["v"].n_entries == len(spec.vectors) == len(idx) and a["v"].w_pad == (W + 63) // 64 * 64
    if spec.vectors:
        np.testing.assert_array_equal(a["vectors"][:, :W], np.stack(spec.vectors))
        assert not a["vectors"][:, W:].any()  # the pad bytes
    np.testing.assert_array_equal(a["norm2"], np.array(spec.norm2, np.int32))
    np.testing.assert_array_equal(a["frame_id"], np.array(spec.frames, np.int64))
    return a


def _check_query(ctx, idx, spec, descs, frames, exclude, top_k):
    """the view after a query call over `descs` against the specification, array by array"""
    a = _check_index(ctx, idx, spec)
    W, E = spec.n_words, len(spec.vectors)
    assert a["v"].n_queries == len(descs)
    for q, (d, f) in enumerate(zip(descs, frames)):
        cands, row, v, n2 = spec.query(d, f, exclude, top_k)
        w, dist = ref.words_of(d, spec.words)
        np.testing.assert_array_equal(a["q_word"][q, :len(d)], w)
        np.testing.assert_array_equal(a["q_dist"][q, :len(d)], dist)
        np.testing.assert_array_equal(a["q_vectors"][q, :W], v)
        assert not a["q_vectors"][q, W:].any() and a["q_norm2"][q] == n2
        np.testing.assert_array_equal(a["dots"][q], row[:E])
        assert a["cand_count"][q] == len(cands)
        exp_e = np.full(K16, -1, np.int32)
        exp_s, exp_d = np.zeros(K16, np.float64), np.zeros(K16, np.int32)
        for k, (e, s, dd) in enumerate(cands):
            exp_e[k], exp_s[k], exp_d[k] = e, s, dd
        np.testing.assert_array_equal(a["cand_entry"][q], exp_e)
        np.testing.assert_array_equal(a["cand_score"][q].view(np.uint64), exp_s.view(np.uint64))  # bit for bit
        np.testing.assert_array_equal(a["cand_dot"][q], exp_d)
    return a


@pytest.mark.parametrize("W", [1, 17, 100, 2048, 2049, 4096])
def test_words_vectors_and_queries_over_vocabulary_sizes(ctx, W):
    """n in {0, 1, 17, 2000} descriptors per image at every vocabulary size: the pad (W no multiple of 64), more than
    one LDS chunk of words, more than one workgroup of descriptors (2000 > 512), duplicate words."""
    rng = np.random.default_rng(W)
    words = _vocabulary(rng, W)
    idf = None if W == 100 else rng.integers(0, 3000, W).astype(np.uint16)
    if idf is not None:
        idf[0] = 65535  # the largest weight: t_w = c_w * 65535
    imgs = [np.concatenate([_near(rng, words, n - n // 4), _rand_desc(rng, n // 4)]) if n else _rand_desc(rng, 0)
            for n in (0, 1, 17, 2000)]
    spec = ref.Index(words, idf)
    idx = bow.BowIndex(ctx, words, idf, max_entries=8, max_queries=4, max_kp=2000)
    try:
        for d in imgs:
            w, dist = idx.words(d)
            ew, ed = ref.words_of(d, words)
            np.testing.assert_array_equal(w, ew)
            np.testing.assert_array_equal(dist, ed)
            v, n2 = idx.vector(d)
            ev, en2 = spec.vector(d)
            np.testing.assert_array_equal(v, ev)
            assert n2 == en2
        for f, d in enumerate(imgs + [imgs[3]]):  # the last entry repeats one: equal scores, index order
            assert idx.add(d, 10 * f) == f
            spec.add(d, 10 * f)
        for f, d in enumerate(imgs):
            got = idx.query(d, 100 + f, 0, 16)  # top_k above the number of eligible entries
            exp = spec.query(d, 100 + f, 0, 16)[0]
            assert got == [(e, spec.frames[e], s, dd) for e, s, dd in exp]
            _check_query(ctx, idx, spec, [d], [100 + f], 0, 16)
        if W > 1:
            assert [c[0] for c in idx.query(imgs[3], 0, 0, 2)] == [3, 4]
    finally:
        idx.close()


def test_entries_ties_exclusion_reset_and_capacity(ctx):
    """E in {0, 1, 17, 300} entries with duplicates among them, top_k above the eligible entries, x = 0 and an x that
    excludes the best entry, reset, and an add beyond the capacity."""
    rng = np.random.default_rng(7)
    W = 100
    words = _vocabulary(rng, W)
    pool = [_near(rng, words, 40 + (i % 5), flips=30) for i in range(24)]
    spec = ref.Index(words, None)
    idx = bow.BowIndex(ctx, words, None, max_entries=300, max_queries=2, max_kp=64)
    try:
        queries = [pool[0], pool[5]]
        for E in (0, 1, 17, 300):
            while len(spec.vectors) < E:
                e = len(spec.vectors)
                d = pool[(e * 7) % 24]  # every image comes back every 24 entries: equal scores
                assert idx.add(d, 3 * e) == e
                spec.add(d, 3 * e)
            for top_k in (1, 16):
                for q in queries:
                    got = idx.query(q, 1000, 0, top_k)
                    assert [(e, s, dd) for e, _, s, dd in got] == spec.query(q, 1000, 0, top_k)[0]
                    _check_query(ctx, idx, spec, [q], [1000], 0, top_k)
        # the best entry of pool[0] is entry 0 (itself, frame 0); from frame 10 a window of 11 excludes it
        assert idx.query(pool[0], 10, 0, 4)[0][0] == 0
        got = idx.query(pool[0], 10, 11, 16)
        exp = spec.query(pool[0], 10, 11, 16)[0]
        assert [(e, s, dd) for e, _, s, dd in got] == exp and 0 not in [e for e, _, _ in exp] and len(exp) == 16
        assert all(abs(10 - f) >= 11 for _, f, _, _ in got)
        _check_query(ctx, idx, spec, [pool[0]], [10], 11, 16)
        # a full index refuses an add and stays as it was
        with pytest.raises(yv.YavoError) as err:
            idx.add(pool[1], 5000)
        assert err.value.status == yv.YV_ERR_CAPACITY and len(idx) == 300
        _check_index(ctx, idx, spec)
        # more descriptors than max_kp
        with pytest.raises(yv.YavoError) as err:
            idx.words(_rand_desc(rng, 65))
        assert err.value.status == yv.YV_ERR_CAPACITY
        idx.reset()
        spec.reset()
        assert len(idx) == 0 and idx.query(pool[0], 10, 0, 4) == []
        assert idx.add(pool[3], 9) == 0
        spec.add(pool[3], 9)
        assert idx.query(pool[3], 10, 0, 4) == [(0, 9, 1.0, spec.norm2[0])]
        _check_query(ctx, idx, spec, [pool[3]], [10], 0, 4)
    finally:
        idx.close()


def test_all_zero_idf_gives_norm_zero_and_no_candidate(ctx):
    rng = np.random.default_rng(9)
    words = _vocabulary(rng, 17)
    idf = np.zeros(17, np.uint16)
    spec = ref.Index(words, idf)
    idx = bow.BowIndex(ctx, words, idf, max_entries=4, max_queries=1, max_kp=64)
    try:
        d = _near(rng, words, 50)
        idx.add(d, 0)
        spec.add(d, 0)
        v, n2 = idx.vector(d)
        assert not v.any() and n2 == 0
        assert idx.query(d, 50, 0, 4) == []
        a = _check_query(ctx, idx, spec, [d], [50], 0, 4)
        assert a["norm2"][0] == 0 and a["dots"][0, 0] == 0 and a["cand_count"][0] == 0
    finally:
        idx.close()


def test_device_training_equals_the_specification(ctx):
    rng = np.random.default_rng(11)
    centres = _rand_desc(rng, 12)
    desc = _near(rng, centres, 700, flips=25)
    np.testing.assert_array_equal(bow.BowIndex.train(ctx, desc, 12, 2, 3, max_kp=512),
                                  ref.train_vocabulary(desc, 12, 2, 3))


def test_batch_forms_over_a_real_run(ctx):
    """The 16 places and 16 revisits of the CPU retrieval test through Batch.run: add_batch / query_batch read the
    slots' descriptors in HBM and give what the host forms and the specification give, the CPU test's candidates."""
    import torch
    places, revisits, words, idf = bow_scenes.scene(256, 0)
    H, Wd, n = bow_scenes.H, bow_scenes.W, bow_scenes.N_PLACES
    imgs = np.stack([bow_scenes.place_image(i) for i in range(n)] + [bow_scenes.revisit_image(i) for i in range(n)])
    d_imgs = torch.from_numpy(np.ascontiguousarray(imgs)).to("cuda:0")
    torch.cuda.synchronize()
    b = yv.Batch(ctx, 2 * n, H, Wd, bow_scenes.MAX_KP, 0)
    idx = bow.BowIndex(ctx, words, idf, max_entries=20, max_queries=16, max_kp=bow_scenes.MAX_KP)
    host = bow.BowIndex(ctx, words, idf, max_entries=20, max_queries=1, max_kp=bow_scenes.MAX_KP)
    try:
        b.run(d_imgs.data_ptr(), 2 * n, Wd, H * Wd, 20)
        idx.add_batch(b, list(range(n)), list(range(n)))
        idx.query_batch(b, list(range(n, 2 * n)), [100 + i for i in range(n)], exclude=0, top_k=16)
        got = idx.candidates()
        v = b.view()
        counts = ctx.download(v.kp_count, np.int32, 2 * n)
        kps = ctx.download(v.keypoints, yv.KEYPOINT_DTYPE, 2 * n * bow_scenes.MAX_KP).reshape(2 * n, -1)
        for i in range(2 * n):  # the run's keypoints are the oracle's (the front end's own parity tests)
            np.testing.assert_array_equal(kps[i, :counts[i]], (places + revisits)[i])
        spec = ref.Index(words, idf)
        for i in range(n):
            spec.add(places[i]["featVec"], i)
            host.add(kps[i, :counts[i]], i)
        _check_query(ctx, idx, spec, [r["featVec"] for r in revisits], [100 + i for i in range(n)], 0, 16)
        for i in range(n):
            exp = spec.query(revisits[i]["featVec"], 100 + i, 0, 16)[0]
            assert got[i] == [(e, e, s, dd) for e, s, dd in exp]
            assert host.query(kps[n + i, :counts[n + i]], 100 + i, 0, 16) == got[i]
            assert got[i][0][0] == i  # the revisit's own place
            assert got[i][0][2] - max([s for e, _, s, _ in got[i] if e != i], default=0.0) > 0.2
        # a slot outside the batch, a batch with more keypoints per slot than the index, too many queries
        for bad in (-1, 2 * n + 1):
            with pytest.raises(yv.YavoError) as err:
                idx.query_batch(b, [bad], [0])
            assert err.value.status == yv.YV_ERR_INVALID
        with pytest.raises(yv.YavoError) as err:
            idx.query_batch(b, list(range(17)), list(range(17)))
        assert err.value.status == yv.YV_ERR_CAPACITY
        small = bow.BowIndex(ctx, words, idf, max_entries=2, max_queries=2, max_kp=bow_scenes.MAX_KP - 1)
        with pytest.raises(yv.YavoError) as err:
            small.add_batch(b, [0], [0])
        assert err.value.status == yv.YV_ERR_INVALID
        small.close()
        with pytest.raises(yv.YavoError) as err:
            idx.add_batch(b, list(range(5)), list(range(5)))  # 16 + 5 > 20: nothing is added
        assert err.value.status == yv.YV_ERR_CAPACITY and len(idx) == n
        _check_index(ctx, idx, spec)
    finally:
        host.close()
        idx.close()
        b.close()
