"""GPU tests of the 2-NN matcher and the match filter on host keypoint lists (yv_match_knn2 / yv_match_robust):
every field against a numpy brute force written here.  All arithmetic is integer, so every comparison is exact.

The inputs hold exact duplicate train descriptors (d2 == d1 ties with j2 != j1), near copies (clear ratio passes)
and unrelated descriptors; the reference alone must show queries in every class before the GPU is touched."""
import functools

import numpy as np
import pytest

import ya_vo_amd as yv

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
THR = 20
RATIOS = ((4, 5), (1, 1), (1, 2))
# (nq, nt): degenerate lists; partial tiles and a partial 128-train chunk; the last FP4 size (full index field); the
# int8 matcher forward; the int8 matcher in the reverse direction under a small FP4 forward; the capacity
SHAPES = [(1, 1), (7, 1), (5, 0), (0, 5), (33, 2), (513, 511), (2048, 2048), (65, 2049), (2049, 65), (4096, 33)]


def _keypoints(desc):
    k = np.zeros(len(desc), yv.KEYPOINT_DTYPE)
    k["x"] = 3 * np.arange(len(desc)) + 1
    k["y"] = 7 * np.arange(len(desc)) + 2
    k["id"] = np.arange(len(desc))
    k["featVec"] = desc
    return k


@functools.lru_cache(maxsize=None)
def _inputs(nq, nt):
    rng = np.random.default_rng(131 * nq + nt)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    half, eighth = nt // 2, nt // 8
    if eighth > 0:  # exact duplicate trains: d2 == d1 ties with j2 != j1
        t[half:] = t[rng.integers(0, eighth, nt - half)]
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    if nt > 0:
        for i in np.flatnonzero(rng.random(nq) < 0.6):  # a train descriptor with 0..39 bits flipped
            bits = np.unpackbits(t[rng.integers(0, nt)])
            bits[rng.choice(256, rng.integers(0, 40), replace=False)] ^= 1
            q[i] = np.packbits(bits)
    q, t = _keypoints(q), _keypoints(t)
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


def hamming_matrix(q, t):
    """d(i, j) [nq, nt] int32.  One matmul of the 0/1 bit matrices: popcount(a ^ b) = |a| + |b| - 2 a.b; every
    product and sum is an integer <= 256, exact in float32 (the BLAS path), then int32."""
    a = np.unpackbits(q["featVec"], axis=1).astype(np.float32)
    b = np.unpackbits(t["featVec"], axis=1).astype(np.float32)
    dot = (a @ b.T).astype(np.int32)
    return a.sum(1).astype(np.int32)[:, None] + b.sum(1).astype(np.int32)[None, :] - 2 * dot


def knn2_reference(q, t):
    """(nn2 [nq] MATCH2_DTYPE, rev [nt] int32) by brute force: first index at every minimum."""
    nq, nt = len(q), len(t)
    nn2 = np.zeros(nq, yv.MATCH2_DTYPE)
    nn2["d1"], nn2["d2"] = INT_MAX, INT_MAX
    nn2["j1"], nn2["j2"] = -1, -1
    rev = np.full(nt, -1, np.int32)
    if nq == 0 or nt == 0:
        return nn2, rev
    D = hamming_matrix(q, t)
    rows = np.arange(nq)
    j1 = D.argmin(1)
    nn2["j1"], nn2["d1"] = j1, D[rows, j1]
    if nt >= 2:
        D2 = D.copy()
        D2[rows, j1] = INT_MAX
        j2 = D2.argmin(1)
        nn2["j2"], nn2["d2"] = j2, D2[rows, j2]
    rev[:] = D.argmin(0)
    return nn2, rev


def outlier_limit(d1, thr):
    """removeOutliers' limit max(2 * min_dist, thr) with the int wrap, over all queries of the pair."""
    twice = np.array([2 * int(d1.min())], np.int64).astype(np.int32)[0]
    return max(int(twice), thr)


def mutual_reference(nn2, rev):
    """j1(i) >= 0 and i1(j1(i)) == i"""
    if len(rev) == 0:
        return np.zeros(len(nn2), bool)
    return (nn2["j1"] >= 0) & (rev[np.maximum(nn2["j1"], 0)] == np.arange(len(nn2)))


def keep_reference(nn2, rev, thr, flags, num, den):
    if len(nn2) == 0:
        return np.zeros(0, bool)
    d1, d2 = nn2["d1"].astype(np.int64), nn2["d2"].astype(np.int64)
    keep = d1 < outlier_limit(nn2["d1"], thr)
    if flags & yv.YV_MATCH_RATIO:
        keep &= d1 * den < d2 * num
    if flags & yv.YV_MATCH_MUTUAL:
        keep &= mutual_reference(nn2, rev)
    return keep


@functools.lru_cache(maxsize=None)
def _reference(nq, nt):
    q, t = _inputs(nq, nt)
    nn2, rev = knn2_reference(q, t)
    nn2.setflags(write=False)
    rev.setflags(write=False)
    return nn2, rev


def _classes(nq, nt):
    nn2, rev = _reference(nq, nt)
    ratio = nn2["d1"].astype(np.int64) * 5 < nn2["d2"].astype(np.int64) * 4
    mutual = mutual_reference(nn2, rev)
    ties = nn2["d1"] == nn2["d2"]
    kept = keep_reference(nn2, rev, THR, 3, 4, 5)
    return ratio, mutual, ties, kept


@pytest.mark.parametrize("nq,nt", [s for s in SHAPES if min(s) >= 64])
def test_reference_has_every_class(nq, nt):
    """On the reference alone: a test that trivially keeps or drops everything is a failed test."""
    ratio, mutual, ties, kept = _classes(nq, nt)
    print(f"{nq} x {nt}: ratio passes {ratio.sum()}, mutual passes {mutual.sum()}, ties {ties.sum()}, "
          f"kept {kept.sum()}")
    assert ratio.sum() >= 5 and (~ratio).sum() >= 5
    assert mutual.sum() >= 5 and (~mutual).sum() >= 5
    assert ties.sum() >= 5
    assert kept.sum() >= 5 and (~kept).sum() >= 5


@pytest.mark.parametrize("nq,nt", SHAPES)
def test_match_knn2_equals_brute_force(ctx, nq, nt):
    q, t = _inputs(nq, nt)
    ref, ref_rev = _reference(nq, nt)
    nn2, rev = ctx.match_knn2(q, t)
    assert nn2.dtype == yv.MATCH2_DTYPE and len(nn2) == nq and len(rev) == nt
    for f in ("d1", "j1", "d2", "j2"):
        np.testing.assert_array_equal(nn2[f], ref[f], err_msg=f)
    np.testing.assert_array_equal(rev, ref_rev)
    if nt < 2:
        assert np.all(nn2["d2"] == INT_MAX) and np.all(nn2["j2"] == -1)
    # the new kernel agrees with the shipped 1-NN matcher
    m = ctx.match_features(q, t)
    np.testing.assert_array_equal(nn2["d1"], m["distance"])
    if nt > 0:
        np.testing.assert_array_equal(nn2["j1"], m["pt2"]["id"])
        np.testing.assert_array_equal(t[nn2["j1"]]["x"], m["pt2"]["x"])


@pytest.mark.parametrize("nq,nt", SHAPES)
def test_match_robust_equals_reference(ctx, nq, nt):
    q, t = _inputs(nq, nt)
    nn2, rev = _reference(nq, nt)
    m = ctx.match_features(q, t)
    # flags = 0: the two reference calls
    f0, k0 = ctx.match_robust(q, t, THR, ratio=None, mutual=False)
    np.testing.assert_array_equal(f0, ctx.filter_matches(m, THR))
    np.testing.assert_array_equal(k0, keep_reference(nn2, rev, THR, 0, 0, 1))
    cases = [(yv.YV_MATCH_MUTUAL, None)] + [(fl, r) for fl in (yv.YV_MATCH_RATIO, 3) for r in RATIOS]
    for flags, ratio in cases:
        num, den = ratio if ratio else (0, 1)
        filt, keep = ctx.match_robust(q, t, THR, ratio=ratio, mutual=bool(flags & yv.YV_MATCH_MUTUAL))
        ref_keep = keep_reference(nn2, rev, THR, flags, num, den)
        np.testing.assert_array_equal(keep, ref_keep, err_msg=f"flags {flags} ratio {ratio}")
        want = m[ref_keep].copy()
        want["pt1"]["matched"] = 1
        want["pt2"]["matched"] = 1
        np.testing.assert_array_equal(filt, want, err_msg=f"flags {flags} ratio {ratio}")


def _match_records(q, t, nn2):
    """matchFeatures' records from the brute force: the query, its nearest train point's x / y / id, the distance."""
    m = np.zeros(len(q), yv.MATCH_DTYPE)
    m["pt1"] = q
    has = nn2["j1"] >= 0
    for f in ("x", "y", "id"):
        m["pt2"][f][has] = t[f][nn2["j1"][has]]
    m["distance"] = nn2["d1"]
    return m


def _kept_records(m, keep):
    want = m[keep].copy()
    want["pt1"]["matched"] = 1
    want["pt2"]["matched"] = 1
    return want


def test_host_matchers_in_sequence_on_one_context(ctx):
    """The five host matchers share the single-image workspace and its key buffers: lists that shrink after a larger
    call (a key left behind past the new nq / nt would surface) on both sides of the 2048 train points between the FP4
    and the int8 matcher, every result against the brute force of its own inputs."""
    open_gate = (-65535, 65535, -65535, 65535)

    def check_nn2(got, shape, what):
        ref, ref_rev = _reference(*shape)
        nn2, rev = got
        assert len(nn2) == shape[0] and len(rev) == shape[1]
        for f in ("d1", "j1", "d2", "j2"):
            np.testing.assert_array_equal(nn2[f], ref[f], err_msg=f"{what} {f}")
        np.testing.assert_array_equal(rev, ref_rev, err_msg=f"{what} rev")

    # 1: the filtering finalize with both tests, FP4 in both directions
    big = (513, 511)
    q, t = _inputs(*big)
    nn2, rev = _reference(*big)
    records = _match_records(q, t, nn2)
    filt, keep = ctx.match_robust(q, t, THR, ratio=(4, 5), mutual=True)
    ref_keep = keep_reference(nn2, rev, THR, 3, 4, 5)
    np.testing.assert_array_equal(keep, ref_keep, err_msg="1 keep")
    np.testing.assert_array_equal(filt, _kept_records(records, ref_keep), err_msg="1 filtered")
    # 2: the plain matcher and finalize on far shorter lists
    small = (33, 2)
    m = ctx.match_features(*_inputs(*small))
    np.testing.assert_array_equal(m, _match_records(*_inputs(*small), _reference(*small)[0]), err_msg="2")
    # 3: int8 forward, FP4 reverse
    check_nn2(ctx.match_knn2(*_inputs(65, 2049)), (65, 2049), "3")
    # 4: the gated matcher behind an open gate is the 2-NN matcher
    check_nn2(ctx.match_gated(*_inputs(*small), open_gate), small, "4")
    # 5
    check_nn2(ctx.match_knn2(*_inputs(7, 1)), (7, 1), "5")
    # 6: back to the first lists through the plain path
    m = ctx.match_features(q, t)
    np.testing.assert_array_equal(m, records, err_msg="6 matches")
    np.testing.assert_array_equal(ctx.filter_matches(m, THR),
                                  _kept_records(records, keep_reference(nn2, rev, THR, 0, 0, 1)), err_msg="6 filtered")
