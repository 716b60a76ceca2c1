"""GPU tests of the gated matcher on host keypoint lists (yv_match_gated): every field against a numpy brute force
written here, which masks the Hamming matrix by the gate and takes the sorted (d, j) keys.  All arithmetic is integer,
so every comparison is exact.

The descriptors are those of test_gpu_match_knn2 (exact duplicate trains, near copies, unrelated ones); the positions
lie in an H x W field, and 60 % of the queries sit at their source train point plus (-2..2 rows, 0..47 columns), so
true partners fall inside and outside the gates.  The reference alone must show queries of every class before the GPU
is touched."""
import functools

import numpy as np
import pytest

import ya_vo_amd as yv

from test_gpu_match_knn2 import hamming_matrix, knn2_reference

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
NONE_KEY = np.int64(1) << 40
OPEN = (-65535, 65535, -65535, 65535)
# (nq, nt), field (H, W), gate
CASES = [
    ((1, 1), (16, 16), (-2, 2, -2, 2)),
    ((5, 0), (16, 16), (-2, 2, -2, 2)),
    ((0, 5), (16, 16), (-2, 2, -2, 2)),
    ((33, 2), (16, 16), (-8, 8, -8, 0)),
    ((513, 511), (64, 256), (-1, 1, -32, 0)),            # partial waves and chunks
    ((2048, 2048), (376, 1241), (-2, 2, -128, 0)),       # the stereo gate at workload density
    ((4096, 4096), (376, 1241), (-40, 40, -60, 60)),     # capacity, the temporal window
    ((300, 700), (2, 4096), (-1, 1, -4000, 0)),          # two rows: the staging loop, a bucket far above a band
]
EMPTY_GATES = [(0, 0, 0, 0), (3, 9, 5, 5)]


@functools.lru_cache(maxsize=None)
def _inputs(nq, nt, H, W):
    rng = np.random.default_rng(131 * nq + nt)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    half, eighth = nt // 2, nt // 8
    if eighth > 0:  # exact duplicate trains
        t[half:] = t[rng.integers(0, eighth, nt - half)]
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    tpos = np.stack([rng.integers(0, H, nt), rng.integers(0, W, nt)], 1)
    qpos = np.stack([rng.integers(0, H, nq), rng.integers(0, W, nq)], 1)
    if nt > 0:
        for i in np.flatnonzero(rng.random(nq) < 0.6):  # a train descriptor with 0..39 bits flipped, placed near it
            src = rng.integers(0, nt)
            bits = np.unpackbits(t[src])
            bits[rng.choice(256, rng.integers(0, 40), replace=False)] ^= 1
            q[i] = np.packbits(bits)
            qpos[i] = tpos[src] + (rng.integers(-2, 3), rng.integers(0, 48))
    qpos = np.clip(qpos, 0, 65535)
    out = []
    for desc, pos in ((q, qpos), (t, tpos)):
        k = np.zeros(len(desc), yv.KEYPOINT_DTYPE)
        k["x"], k["y"] = pos[:, 0], pos[:, 1]
        k["id"] = np.arange(len(desc))
        k["featVec"] = desc
        k.setflags(write=False)
        out.append(k)
    return tuple(out)


def gate_mask(q, t, gate):
    """[nq, nt] bool: train j is a candidate of query i (train minus query position inside the gate)."""
    dr = t["x"].astype(np.int64)[None, :] - q["x"].astype(np.int64)[:, None]
    dc = t["y"].astype(np.int64)[None, :] - q["y"].astype(np.int64)[:, None]
    return (dr >= gate[0]) & (dr <= gate[1]) & (dc >= gate[2]) & (dc <= gate[3])


def gated_reference(q, t, gate):
    """(nn2 [nq] MATCH2_DTYPE, rev [nt] int32): the two smallest keys (d << 16 | j) among every query's candidates,
    and for every train point the smallest key (d << 16 | i) among the queries it is a candidate of."""
    nq, nt = len(q), len(t)
    nn2 = np.zeros(nq, yv.MATCH2_DTYPE)
    nn2["d1"], nn2["d2"] = INT_MAX, INT_MAX
    nn2["j1"], nn2["j2"] = -1, -1
    rev = np.full(nt, -1, np.int32)
    if nq == 0 or nt == 0:
        return nn2, rev
    D = hamming_matrix(q, t).astype(np.int64)
    mask = gate_mask(q, t, gate)
    rows = np.arange(nq)
    keys = np.where(mask, (D << 16) | np.arange(nt)[None, :], NONE_KEY)
    for d, j in (("d1", "j1"), ("d2", "j2")):
        a = keys.argmin(1)
        k = keys[rows, a]
        has = k != NONE_KEY
        nn2[d][has], nn2[j][has] = (k >> 16)[has], (k & 0xFFFF)[has]
        keys[rows, a] = NONE_KEY
    rkeys = np.where(mask, (D << 16) | rows[:, None], NONE_KEY).min(0)
    has = rkeys != NONE_KEY
    rev[has] = (rkeys & 0xFFFF)[has]
    return nn2, rev


@functools.lru_cache(maxsize=None)
def _reference(shape, field, gate):
    q, t = _inputs(*shape, *field)
    nn2, rev = gated_reference(q, t, gate)
    nn2.setflags(write=False)
    rev.setflags(write=False)
    return nn2, rev


@pytest.mark.parametrize("shape,field,gate", [c for c in CASES if c[0] in ((513, 511), (2048, 2048))])
def test_reference_has_every_class(shape, field, gate):
    """On the reference alone: a test that trivially matches everything or nothing is a failed test."""
    q, t = _inputs(*shape, *field)
    nn2, rev = _reference(shape, field, gate)
    ungated, _ = knn2_reference(q, t)
    n_cand = gate_mask(q, t, gate).sum(1)
    ties = (nn2["d1"] == nn2["d2"]) & (nn2["j2"] >= 0)
    differ = nn2["j1"] != ungated["j1"]
    print(f"{shape}: none {(n_cand == 0).sum()}, one {(n_cand == 1).sum()}, two or more {(n_cand >= 2).sum()}, "
          f"ties {ties.sum()}, differ {differ.sum()}, train points without a query {(rev < 0).sum()}")
    assert (n_cand == 0).sum() >= 5 and (n_cand == 1).sum() >= 5 and (n_cand >= 2).sum() >= 5
    assert ties.sum() >= 5 and differ.sum() >= 5
    assert np.array_equal(nn2["j1"] < 0, n_cand == 0) and np.array_equal(nn2["j2"] < 0, n_cand < 2)
    # the near copies placed inside the gate are found: the gate does not cut every true partner either
    assert (nn2["d1"] < 40).sum() >= 5


def test_two_row_case_fills_more_than_any_staging_chunk():
    shape, field, gate = CASES[-1]
    q, t = _inputs(*shape, *field)
    n_cand = gate_mask(q, t, gate).sum(1)
    assert n_cand.max() >= 600 and set(np.unique(t["x"])) == {0, 1}


def _assert_equal(got, ref, what):
    nn2, rev = got
    ref_nn2, ref_rev = ref
    assert nn2.dtype == yv.MATCH2_DTYPE and len(nn2) == len(ref_nn2) and len(rev) == len(ref_rev)
    for f in ("d1", "j1", "d2", "j2"):
        np.testing.assert_array_equal(nn2[f], ref_nn2[f], err_msg=f"{what} {f}")
    np.testing.assert_array_equal(rev, ref_rev, err_msg=f"{what} rev")


@pytest.mark.parametrize("shape,field,gate", CASES)
def test_match_gated_equals_brute_force(ctx, shape, field, gate):
    q, t = _inputs(*shape, *field)
    _assert_equal(ctx.match_gated(q, t, gate), _reference(shape, field, gate), f"{shape} {gate}")


def test_open_gate_equals_the_ungated_matcher(ctx):
    shape, field = (513, 511), (64, 256)
    q, t = _inputs(*shape, *field)
    ref = knn2_reference(q, t)
    _assert_equal(gated_reference(q, t, OPEN), ref, "references")
    got = ctx.match_gated(q, t, OPEN)
    _assert_equal(got, ref, "open gate")
    _assert_equal(got, ctx.match_knn2(q, t), "open gate vs match_knn2")


@pytest.mark.parametrize("gate", EMPTY_GATES)
def test_gates_without_any_candidate(ctx, gate):
    """Asymmetric and one-sided gates that no pair of the input satisfies: nothing but INT32_MAX / -1.  The positions
    are spread out so that no two points are (0, 0) or (3..9, 5) apart."""
    shape, field = (513, 511), (64, 256)
    q, t = (k.copy() for k in _inputs(*shape, *field))
    q["x"], q["y"] = 20 * (np.arange(len(q)) % 23), 20 * (np.arange(len(q)) // 23)
    t["x"], t["y"] = 20 * (np.arange(len(t)) % 23) + 1, 20 * (np.arange(len(t)) // 23) + 1
    assert not gate_mask(q, t, gate).any()
    nn2, rev = ctx.match_gated(q, t, gate)
    assert np.all(nn2["d1"] == INT_MAX) and np.all(nn2["d2"] == INT_MAX)
    assert np.all(nn2["j1"] == -1) and np.all(nn2["j2"] == -1) and np.all(rev == -1)
    _assert_equal((nn2, rev), gated_reference(q, t, gate), f"empty {gate}")


def test_a_call_after_an_ungated_one_and_back(ctx):
    """The gated and the ungated host calls share one workspace and its key buffers."""
    shape, field, gate = CASES[4]
    q, t = _inputs(*shape, *field)
    ref_open = knn2_reference(q, t)
    _assert_equal(ctx.match_knn2(q, t), ref_open, "before")
    _assert_equal(ctx.match_gated(q, t, gate), _reference(shape, field, gate), "gated")
    _assert_equal(ctx.match_knn2(q, t), ref_open, "after")
