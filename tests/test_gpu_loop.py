"""GPU parity of the keyframe store and the candidate verification (yv_loop_*, ya_vo_amd.loop.LoopVerifier) against the
specification tests/loop_reference.py over the CPU oracle: the store's arrays, every field of every result, every edge
array up to edge_count, both masks and the pose, bit for bit, in the batch forms and the host forms."""
import functools

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import loop

import loop_reference as ref
import loop_scenes as sc
from pnp_scenes import K9, pnp_scene

pytestmark = pytest.mark.gpu

TOP_K = 4


# ---- reading a call back ----
def _read_call(ctx, lv):
    """The last verify call's view arrays over its problems"""
    v = lv.view()
    n, kp = v.n_problems, v.max_kp
    ctx.sync()
    return dict(n=n, kp=kp, results=ctx.download(v.results, yv.LOOP_RESULT_DTYPE, n),
                edge_count=ctx.download(v.edge_count, np.int32, n),
                edge_X=ctx.download(v.edge_X, np.float64, n * kp * 3).reshape(n, kp, 3),
                edge_uv=ctx.download(v.edge_uv, np.float64, n * kp * 2).reshape(n, kp, 2),
                edge_query=ctx.download(v.edge_query, np.int32, n * kp).reshape(n, kp),
                edge_train=ctx.download(v.edge_train, np.int32, n * kp).reshape(n, kp),
                ransac_inlier=ctx.download(v.ransac_inlier, np.uint8, n * kp).reshape(n, kp),
                lm_outlier=ctx.download(v.lm_outlier, np.uint8, n * kp).reshape(n, kp))


def _same_result(row, r, what):
    got = tuple(int(row[f]) for f in ("entry", "n_kept", "n_edges", "ransac_inliers", "lm_inliers", "verified"))
    want = (r.entry, r.n_kept, r.n_edges, r.ransac_inliers, r.lm_inliers, r.verified)
    assert got == want, (what, got, want)
    assert row["pose"].tobytes() == np.asarray(r.pose, np.float64).tobytes(), (what, row["pose"], r.pose)


def _same_problem(call, v, r, what):
    _same_result(call["results"][v], r, what)
    ne = r.n_edges
    if r.entry < 0:
        return
    assert call["edge_count"][v] == ne, what
    assert call["edge_X"][v, :ne].tobytes() == np.ascontiguousarray(r.edge_X).tobytes(), what
    assert call["edge_uv"][v, :ne].tobytes() == np.ascontiguousarray(r.edge_uv).tobytes(), what
    np.testing.assert_array_equal(call["edge_query"][v, :ne], r.edge_query, what)
    np.testing.assert_array_equal(call["edge_train"][v, :ne], r.edge_train, what)
    np.testing.assert_array_equal(call["ransac_inlier"][v, :ne], r.ransac_inlier.astype(np.uint8), what)
    np.testing.assert_array_equal(call["lm_outlier"][v, :ne], r.lm_outlier.astype(np.uint8), what)


def _set_params(lv, P):
    lv.set_params(P.match_thr, P.flags, P.num, P.den, len(P.draws), P.thr_px, P.min_inliers, draws=P.draws)


# ---- the scene on the device: one batch run over all 24 stereo frames ----
@pytest.fixture(scope="module")
def scene_batch(ctx):
    import torch
    d = torch.from_numpy(np.array(sc.frames())).to("cuda:0")
    torch.cuda.synchronize()
    b = yv.Batch(ctx, 2 * sc.N_FRAMES, sc.H, sc.W, sc.MAX_KP, sc.N_FRAMES)
    b.set_pairs([(2 * k, 2 * k + 1) for k in range(sc.N_FRAMES)])  # pair k: the stereo pair of frame k
    b.run(d.data_ptr(), 2 * sc.N_FRAMES, sc.W, sc.H * sc.W, sc.MATCH_THR)
    ctx.sync()
    yield b
    b.close()


def _store_arrays(ctx, lv, n):
    v = lv.view()
    kp = v.max_kp
    ctx.sync()
    return dict(kp_count=ctx.download(v.kp_count, np.int32, n), frame_id=ctx.download(v.frame_id, np.int64, n),
                desc=ctx.download(v.desc, np.uint8, n * kp * 32).reshape(n, kp, 32),
                pos=ctx.download(v.pos, np.int32, n * kp * 2).reshape(n, kp, 2),
                X=ctx.download(v.X, np.float64, n * kp * 3).reshape(n, kp, 3),
                has=ctx.download(v.has, np.uint8, n * kp).reshape(n, kp))


@pytest.mark.parametrize("max_kp", [sc.MAX_KP, 512])  # the batch's row length, and a store with longer rows
def test_store_parity(ctx, scene_batch, max_kp):
    spec = sc.store()
    lv = loop.LoopVerifier(ctx, sc.K, sc.T_RIGHT, max_entries=6, max_problems=4, max_kp=max_kp)
    host = loop.LoopVerifier(ctx, sc.K, sc.T_RIGHT, max_entries=6, max_problems=4, max_kp=max_kp)
    try:
        lv.add_batch(scene_batch, [0, 2, 4, 6], [0, 1, 2, 3], [100, 101, 102, 103])
        assert len(lv) == 4 and lv.entry_frames == [100, 101, 102, 103]
        got = _store_arrays(ctx, lv, 4)
        for e in range(4):
            want, n = spec.entries[e], len(spec.entries[e].kp)
            assert got["kp_count"][e] == n and got["frame_id"][e] == 100 + e
            np.testing.assert_array_equal(got["desc"][e, :n], want.kp["featVec"])
            np.testing.assert_array_equal(got["pos"][e, :n], np.stack([want.kp["x"], want.kp["y"]], 1))
            np.testing.assert_array_equal(got["has"][e, :n], want.has.astype(np.uint8))
            assert not got["has"][e, n:].any()
            assert got["X"][e, :n].tobytes() == np.ascontiguousarray(want.X).tobytes()
            assert not got["X"][e, n:].any()
            host.add(want.kp, want.X, want.has, 100 + e)
        same = _store_arrays(ctx, host, 4)
        for key in ("kp_count", "frame_id", "has"):
            np.testing.assert_array_equal(same[key], got[key], key)
        assert same["X"].tobytes() == got["X"].tobytes()
        for e in range(4):
            n = got["kp_count"][e]
            np.testing.assert_array_equal(same["desc"][e, :n], got["desc"][e, :n])
            np.testing.assert_array_equal(same["pos"][e, :n], got["pos"][e, :n])
    finally:
        lv.close()
        host.close()


@pytest.fixture(scope="module")
def scene_verifier(ctx, scene_batch):
    """Frames 0 .. 19 of the scene in a store, added from the batch"""
    lv = loop.LoopVerifier(ctx, sc.K, sc.T_RIGHT, max_entries=32, max_problems=64, max_kp=sc.MAX_KP)
    ks = list(range(sc.N_OUT))
    lv.add_batch(scene_batch, [2 * k for k in ks], ks, ks)
    yield lv
    lv.close()


# the table's problems as candidate rows: frame 20 has five entries, so its slot is queried twice
TABLE_ROWS = [(20, [0, 1, 2, 4]), (20, [10]), (21, [1, 12]), (22, [2]), (23, [3, 15])]


def _upload_rows(rows, counts=None):
    """rows: (query frame, entries) per query; counts: the rows' counts where they are not the entries' number"""
    import torch
    cand = np.full((len(rows), 16), -1, np.int32)
    count = np.zeros(len(rows), np.int32)
    for q, (_, entries) in enumerate(rows):
        cand[q, :len(entries)] = entries
        count[q] = len(entries) if counts is None else counts[q]
    return cand, count, torch.from_numpy(cand).to("cuda:0"), torch.from_numpy(count).to("cuda:0")


@pytest.mark.parametrize("flags", [0, 3])
def test_verify_parity(ctx, oracle, scene_batch, scene_verifier, flags):
    lv, P, spec = scene_verifier, sc.params(flags), sc.store()
    _set_params(lv, P)
    cand, count, d_cand, d_count = _upload_rows(TABLE_ROWS)
    n = len(TABLE_ROWS) * TOP_K
    mode = loop.lm_sum_mode(n)
    lv.verify_batch(scene_batch, [2 * f for f, _ in TABLE_ROWS], d_cand.data_ptr(), d_count.data_ptr(), TOP_K)
    call = _read_call(ctx, lv)
    assert call["n"] == n
    table = dict(zip(sc.PROBLEMS, sc.reference(flags, mode)))
    seen = set()
    for q, (f, entries) in enumerate(TABLE_ROWS):
        for k in range(TOP_K):
            r = table[(f, entries[k])] if k < len(entries) else ref.skipped()
            _same_problem(call, TOP_K * q + k, r, (flags, f, k))
            seen.add((f, entries[k]) if k < len(entries) else None)
    assert seen == set(sc.PROBLEMS) | {None}
    if flags == 3:
        assert all(table[key].verified for key in sc.OWN + sc.PARTIAL) and not any(table[key].found for key in sc.NONE)
    np.testing.assert_array_equal(lv.results(), call["results"])
    # the host form, one query list against its entries
    for f in (20, 23):
        entries = [e for ff, e in sc.PROBLEMS if ff == f] + [-1, sc.N_OUT]
        got = lv.verify(sc.keypoints(f)[0], entries)
        call = _read_call(ctx, lv)
        want = sc.reference(flags, loop.lm_sum_mode(len(entries)))
        for v, e in enumerate(entries):
            r = want[sc.PROBLEMS.index((f, e))] if 0 <= e < sc.N_OUT else ref.skipped()
            _same_result(got[v], r, (flags, f, e))
            _same_problem(call, v, r, (flags, f, e))


@pytest.mark.parametrize("top_k,rows,counts", [
    # top_k 1: the second candidate is not looked at; an empty row
    (1, [(20, [0, 1]), (21, [12]), (22, []), (23, [3])], None),
    # a full row; valid entries behind a count of 0; -1 and entries past the store; a count below the entries' number
    (16, [(20, list(range(16))), (21, [0, 1, 2, 3]), (22, [-1, 2, 99, 20]), (23, [3, 15])], [16, 0, 4, 1]),
    # one query
    (4, [(23, [15, 3, 3])], None),
])
def test_candidate_rows_and_skips(ctx, oracle, scene_batch, scene_verifier, top_k, rows, counts):
    lv, P, spec = scene_verifier, sc.params(3), sc.store()
    _set_params(lv, P)
    cand, count, d_cand, d_count = _upload_rows(rows, counts)
    n = len(rows) * top_k
    lv.verify_batch(scene_batch, [2 * f for f, _ in rows], d_cand.data_ptr(), d_count.data_ptr(), top_k)
    call = _read_call(ctx, lv)
    want = ref.verify_rows(oracle, [sc.keypoints(f)[0] for f, _ in rows], spec, cand, count, top_k, sc.K, P,
                           loop.lm_sum_mode(n))
    assert call["n"] == n == len(want)
    for v, r in enumerate(want):
        _same_problem(call, v, r, (top_k, v))
    assert sum(r.entry < 0 for r in want) > 0 and sum(r.verified for r in want) > 0
    # a second, different call on the same object gives its own result: no key or mask state is left behind
    cand2, count2, d_cand2, d_count2 = _upload_rows([(21, [1, 12])])
    lv.verify_batch(scene_batch, [42], d_cand2.data_ptr(), d_count2.data_ptr(), 2)
    call = _read_call(ctx, lv)
    table = dict(zip(sc.PROBLEMS, sc.reference(3, loop.lm_sum_mode(2))))
    _same_problem(call, 0, table[(21, 1)], "second call")
    _same_problem(call, 1, table[(21, 12)], "second call")


# ---- small shapes on synthetic keyframes (host add) ----
SYN_KP = 4096
SIZES = [0, 1, 2, 3, 11, 12, 63, 64, 65, 1023, 1024, 1025, 4096]
# (nq, n, has): every size on both sides, lists of different lengths, an entry without landmarks, few landmarks
SYN_CASES = [(s, s, "all") for s in SIZES] + [(65, 1025, "all"), (1025, 63, "all"), (0, 12, "all"), (12, 0, "all"),
                                               (4096, 257, "all"), (300, 300, "none"), (300, 300, "two"),
                                               (300, 300, "seven"), (300, 300, "most")]


def _records(desc, x, y):
    k = np.zeros(len(desc), yv.KEYPOINT_DTYPE)
    k["featVec"], k["x"], k["y"], k["id"] = desc, x, y, np.arange(len(desc))
    return k


@functools.lru_cache(maxsize=None)
def _synthetic(nq, n, has_kind):
    """-> (query records, entry records, X [n][3], has [n]): the query is a permutation of the entry's descriptors
    with up to 8 bits flipped (and unrelated descriptors past them), at the pixels the entry's landmarks project to."""
    rng = np.random.default_rng(1000 * nq + n + len(has_kind))
    X, uv, _, _ = pnp_scene(n, seed=nq + n, outlier_frac=0.0 if n <= 12 else 0.3)
    X, uv = X.reshape(-1, 3), np.rint(uv.reshape(-1, 2))
    td = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    qx, qy = rng.integers(0, 300, nq), rng.integers(0, 1200, nq)
    perm = rng.permutation(n)[:nq]
    for i, j in enumerate(perm):
        bits = np.unpackbits(td[j])
        bits[rng.choice(256, rng.integers(0, 9), replace=False)] ^= 1
        qd[i] = np.packbits(bits)
        qx[i], qy[i] = uv[j]
    has = np.ones(n, bool)
    if has_kind == "none":
        has[:] = False
    elif has_kind in ("two", "seven"):
        has[:] = False
        has[perm[:2 if has_kind == "two" else 7]] = True
    elif has_kind == "most":
        has[rng.random(n) < 0.2] = False
    return _records(qd, qx, qy), _records(td, rng.integers(0, 300, n), rng.integers(0, 1200, n)), X, has


@pytest.fixture(scope="module")
def syn_verifier(ctx):
    lv = loop.LoopVerifier(ctx, K9, sc.T_RIGHT, max_entries=len(SYN_CASES) + 1, max_problems=4, max_kp=SYN_KP)
    _set_params(lv, ref.params(20, 3, 4, 5, 64, 3, 2.0, 12))
    q, t, X, has = _synthetic(40, 50, "most")  # entry 0: the second call of every case
    lv.add(t, X, has, 0)
    yield lv
    lv.close()


@functools.lru_cache(maxsize=None)
def _second_reference(mode):
    import oracle_bind
    q, t, X, has = _synthetic(40, 50, "most")
    s = ref.Store()
    s.add(t, X, has, 0)
    return ref.verify(oracle_bind.Oracle(), q, s, 0, K9, ref.params(20, 3, 4, 5, 64, 3, 2.0, 12), mode)


@pytest.mark.parametrize("nq,n,has_kind", SYN_CASES)
def test_small_shapes(ctx, oracle, syn_verifier, nq, n, has_kind):
    lv, P = syn_verifier, ref.params(20, 3, 4, 5, 64, 3, 2.0, 12)
    q, t, X, has = _synthetic(nq, n, has_kind)
    s = ref.Store()
    s.add(t, X, has, 7)
    e = lv.add(t, X, has, 7)
    mode = loop.lm_sum_mode(1)
    want = ref.verify(oracle, q, s, 0, K9, P, mode)
    want.entry = e
    got = lv.verify(q, [e])
    _same_result(got[0], want, (nq, n, has_kind))
    _same_problem(_read_call(ctx, lv), 0, want, (nq, n, has_kind))
    if has_kind == "all" and min(nq, n) >= 63:
        assert want.verified and want.n_edges == min(nq, n)
    if has_kind in ("none", "two", "seven") or min(nq, n) < 12:
        assert not want.found and want.n_edges == {"none": 0, "two": 2, "seven": 7}.get(has_kind, min(nq, n))
    # the second call: entry 0 against its own query, after whatever this case left in the buffers
    got = lv.verify(_synthetic(40, 50, "most")[0], [0])
    second = _second_reference(mode)
    _same_result(got[0], second, "second call")
    _same_problem(_read_call(ctx, lv), 0, second, "second call")
    assert second.verified


# ---- capacity and ordering ----
def test_capacity_and_reset(ctx, oracle, scene_batch):
    spec, P = sc.store(), sc.params(3)
    lv = loop.LoopVerifier(ctx, sc.K, sc.T_RIGHT, max_entries=2, max_problems=8, max_kp=sc.MAX_KP)
    try:
        import torch
        d_cand = torch.zeros((4, 16), dtype=torch.int32, device="cuda:0")
        d_count = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        with pytest.raises(yv.YavoError) as err:  # before yv_loop_set_params
            lv.verify_batch(scene_batch, [40], d_cand.data_ptr(), d_count.data_ptr(), 4)
        assert err.value.status == yv.YV_ERR_INVALID
        _set_params(lv, P)
        with pytest.raises(yv.YavoError) as err:  # 3 * 4 > 8
            lv.verify_batch(scene_batch, [40, 42, 44], d_cand.data_ptr(), d_count.data_ptr(), 4)
        assert err.value.status == yv.YV_ERR_CAPACITY
        with pytest.raises(yv.YavoError) as err:
            lv.verify(sc.keypoints(20)[0], list(range(9)))
        assert err.value.status == yv.YV_ERR_CAPACITY
        with pytest.raises(yv.YavoError) as err:  # a stereo pair whose query slot is not the left slot given
            lv.add_batch(scene_batch, [0], [1], [0])
        assert err.value.status == yv.YV_ERR_INVALID
        with pytest.raises(yv.YavoError) as err:  # three entries into a store of two: nothing is added
            lv.add_batch(scene_batch, [0, 2, 4], [0, 1, 2], [0, 1, 2])
        assert err.value.status == yv.YV_ERR_CAPACITY and len(lv) == 0
        lv.add_batch(scene_batch, [0, 2], [0, 1], [0, 1])
        for e in (spec.entries[2],):
            with pytest.raises(yv.YavoError) as err:
                lv.add(e.kp, e.X, e.has, 2)
            assert err.value.status == yv.YV_ERR_CAPACITY and len(lv) == 2
        big = np.zeros(sc.MAX_KP + 1, yv.KEYPOINT_DTYPE)
        with pytest.raises(yv.YavoError) as err:
            lv.verify(big, [0])
        assert err.value.status == yv.YV_ERR_CAPACITY
        table = dict(zip(sc.PROBLEMS, sc.reference(3, loop.lm_sum_mode(1))))
        _same_result(lv.verify(sc.keypoints(21)[0], [1])[0], table[(21, 1)], "before reset")
        # reset empties the store and keeps the parameters
        lv.reset()
        assert len(lv) == 0 and lv.entry_frames == []
        _same_result(lv.verify(sc.keypoints(21)[0], [1])[0], ref.skipped(), "empty store")
        lv.add_batch(scene_batch, [2], [1], [1])
        want = table[(21, 1)]
        want0 = ref.verify(oracle, sc.keypoints(21)[0], spec, 1, sc.K, P, loop.lm_sum_mode(1))
        want0.entry = 0
        _same_result(lv.verify(sc.keypoints(21)[0], [0])[0], want0, "after reset")
        assert want0.pose.tobytes() == want.pose.tobytes()
    finally:
        lv.close()
