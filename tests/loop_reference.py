"""The specification of the keyframe store and the candidate verification (include/yavo/yavo_loop.h) -- test
infrastructure only.  Every step is an operation specified elsewhere; this file fixes their composition:

  the 2-NN match filter        restated here from include/yavo/yavo.h (yv_match_knn2 / yv_match_robust): first index
                               at every minimum, removeOutliers' limit over all queries of the pair, the ratio test in
                               int64, the mutual check;
  the stereo landmarks         the CPU oracle's matchFeatures + removeOutliers + triangulation (the track builders'
                               stereo leg, tests/track_chain.py);
  P3P-RANSAC                   tests/pnp_ransac_reference.py;
  the pose LM                  the CPU oracle's, in the sum_mode the caller names (yv_loop_lm_sum_mode).
"""
from types import SimpleNamespace

import numpy as np

import pnp_ransac_reference as pnp

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
INT_MAX = 2 ** 31 - 1
MATCH_RATIO, MATCH_MUTUAL = 1, 2
CAND_STRIDE = 16


def params(match_thr=20, flags=3, num=4, den=5, iters=64, seed=0, thr_px=2.0, min_inliers=12):
    return SimpleNamespace(match_thr=match_thr, flags=flags, num=num, den=den, draws=pnp.make_draws(iters, seed),
                           thr_px=thr_px, min_inliers=min_inliers)


# ---- the 2-NN match filter ----
def hamming_matrix(qd, td):
    """d(i, j) [nq, nt] int32 of descriptors [n][32] uint8: popcount(a ^ b) = |a| + |b| - 2 a.b over the 0 / 1 bit
    matrices; every product and sum is an integer <= 256, exact in float32."""
    a = np.unpackbits(np.ascontiguousarray(qd, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    b = np.unpackbits(np.ascontiguousarray(td, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    dot = (a @ b.T).astype(np.int32)
    return a.sum(1).astype(np.int32)[:, None] + b.sum(1).astype(np.int32)[None, :] - 2 * dot


def knn2(qd, td):
    """-> (d1, j1, d2 [nq] int64, rev [nt]): nearest and second nearest train point of every query (INT_MAX / -1:
    none) and every train point's nearest query, the first index at every minimum."""
    nq, nt = len(qd), len(td)
    d1, d2 = np.full(nq, INT_MAX, np.int64), np.full(nq, INT_MAX, np.int64)
    j1, rev = np.full(nq, -1, np.int64), np.full(nt, -1, np.int64)
    if nq == 0 or nt == 0:
        return d1, j1, d2, rev
    D = hamming_matrix(qd, td)
    rows = np.arange(nq)
    j1 = D.argmin(1)
    d1 = D[rows, j1].astype(np.int64)
    if nt >= 2:
        D2 = D.copy()
        D2[rows, j1] = INT_MAX
        d2 = D2[rows, D2.argmin(1)].astype(np.int64)
    rev = D.argmin(0)
    return d1, j1.astype(np.int64), d2, rev.astype(np.int64)


def outlier_limit(d1, thr):
    """removeOutliers' limit max(2 * min_dist, thr) with the reference's int wrap, over all queries of the pair"""
    twice = np.array([2 * int(d1.min())], np.int64).astype(np.int32)[0]
    return max(int(twice), int(thr))


def match_robust(qd, td, thr, flags, num, den):
    """-> (keep [nq] bool, j1 [nq]) of yv_match_robust(q, t, thr, flags, num, den)"""
    d1, j1, d2, rev = knn2(qd, td)
    if len(d1) == 0:
        return np.zeros(0, bool), j1
    keep = d1 < outlier_limit(d1, thr)
    if flags & MATCH_RATIO:
        keep &= d1 * int(den) < d2 * int(num)
    if flags & MATCH_MUTUAL:
        keep &= (j1 >= 0) & (rev[np.maximum(j1, 0)] == np.arange(len(d1))) if len(rev) else np.zeros(len(d1), bool)
    return keep, j1


# ---- the store ----
def stereo_landmarks(orc, kl, kr, K, T_right, thr=20):
    """The stereo form's landmarks of a left keypoint list against its right list -> (X [n][3], has [n] bool): keypoint
    j has one iff its stereo match is kept by removeOutliers and triangulates (Ta identity, Tb T_right) with Z > 0.
    X is zero elsewhere."""
    n = len(kl)
    X, has = np.zeros((n, 3)), np.zeros(n, bool)
    if n == 0 or len(kr) == 0:
        return X, has
    ms = orc.match(kl, kr)
    kept_ids = set(orc.remove_outliers(ms, thr)["pt1"]["id"].tolist())
    js = np.array([j for j, i in enumerate(ms["pt1"]["id"].tolist()) if i in kept_ids], np.int64)
    if len(js) == 0:
        return X, has
    _, Xa, ok = orc.triangulate_matches(IDENTITY, T_right, K, ms[js])
    has[js[ok]] = True
    X[js[ok]] = Xa[ok]
    return X, has


class Store:
    """Entries in insertion order: (keypoint records, X [n][3], has [n] bool, frame id)."""

    def __init__(self):
        self.entries = []

    def __len__(self):
        return len(self.entries)

    def add(self, kp, X=None, has=None, frame_id=0):
        n = len(kp)
        has = np.zeros(n, bool) if has is None else np.asarray(has).astype(bool).reshape(n)
        Xs = np.zeros((n, 3))
        if X is not None:
            Xs[has] = np.asarray(X, np.float64).reshape(n, 3)[has]
        self.entries.append(SimpleNamespace(kp=kp, X=Xs, has=has, frame=int(frame_id)))
        return len(self.entries) - 1

    def add_stereo(self, orc, kl, kr, K, T_right, frame_id, thr=20):
        X, has = stereo_landmarks(orc, kl, kr, K, T_right, thr)
        return self.add(kl, X, has, frame_id)


# ---- verification ----
def skipped():
    return SimpleNamespace(entry=-1, n_kept=0, n_edges=0, ransac_inliers=0, lm_inliers=0, verified=0, found=False,
                           pose=IDENTITY.copy(), edge_X=np.zeros((0, 3)), edge_uv=np.zeros((0, 2)),
                           edge_query=np.zeros(0, np.int32), edge_train=np.zeros(0, np.int32),
                           ransac_inlier=np.zeros(0, bool), lm_outlier=np.zeros(0, bool))


def verify(orc, q, store, entry, K, P, sum_mode):
    """Query keypoint records q against entry `entry` of the store under the parameters P (params()); the LM sums in
    the oracle's `sum_mode`."""
    if entry < 0 or entry >= len(store):
        return skipped()
    e = store.entries[entry]
    keep, j1 = match_robust(q["featVec"], e.kp["featVec"], P.match_thr, P.flags, P.num, P.den)
    idx = np.array([i for i in range(len(q)) if keep[i] and e.has[j1[i]]], np.int64)
    tr = j1[idx].astype(np.int64) if len(idx) else np.zeros(0, np.int64)
    X = e.X[tr].reshape(-1, 3)
    uv = np.stack([q["x"][idx], q["y"][idx]], 1).astype(np.float64).reshape(-1, 2)
    pose, mask, inl, found, _ = pnp.pnp_ransac(X, uv, K, P.draws, P.thr_px, P.min_inliers, IDENTITY)
    r = SimpleNamespace(entry=int(entry), n_kept=int(keep.sum()), n_edges=len(idx), ransac_inliers=int(inl),
                        lm_inliers=0, verified=0, found=bool(found), pose=IDENTITY.copy(), edge_X=X, edge_uv=uv,
                        edge_query=idx.astype(np.int32), edge_train=tr.astype(np.int32),
                        ransac_inlier=np.asarray(mask, bool), lm_outlier=np.zeros(len(idx), bool))
    if found:
        T, out, lm_inl = orc.pose_lm(X, uv, K, pose, sum_mode)
        r.pose, r.lm_outlier, r.lm_inliers = T, out, int(lm_inl)
        r.verified = int(r.lm_inliers >= P.min_inliers)
    return r


def verify_rows(orc, queries, store, cand_entry, cand_count, top_k, K, P, sum_mode):
    """The batch form: problem v = top_k * q + k is queries[q] against cand_entry[q][k], skipped when k >= cand_count[q]
    or the entry is outside the store -> the nq * top_k results."""
    cand_entry = np.asarray(cand_entry).reshape(len(queries), CAND_STRIDE)
    out = []
    for qi, q in enumerate(queries):
        for k in range(top_k):
            e = int(cand_entry[qi, k])
            out.append(verify(orc, q, store, e, K, P, sum_mode) if k < int(cand_count[qi]) else skipped())
    return out
