"""The numpy specification of the sub-pixel stereo refinement (yv_stereo_subpix): the footprint
test, the SAD search in the order 0, -1, +1, ..., the parabola's vertex in 1/256 pixel.  Integer only (int64
throughout), so every GPU comparison against it is exact equality.  Also the fixture with a known sub-pixel disparity
and the triangulation of refined matches through the oracle's or_triangulate_one."""
import numpy as np

from ya_vo_amd import MATCH_DTYPE
from ya_vo_amd.synth import _GAUSS13, _noise

NONE, OK, OUTSIDE, EDGE = 0, 1, 2, 3


def inside(H, W, r, c, r2, c2, w, s):
    """The eight footprint conditions."""
    return (r - w >= 0 and r + w < H and c - w >= 0 and c + w < W and r2 - w >= 0 and r2 + w < H
            and c2 - s - w >= 0 and c2 + s + w < W)


def search_order(s):
    """0, -1, +1, -2, +2, ..., -s, +s."""
    return [0] + [k for d in range(1, s + 1) for k in (-d, d)]


def sads(L, R, r, c, r2, c2, w, s):
    """{k: SAD_k} for k in -s..s of an inside match."""
    a = L[r - w:r + w + 1, c - w:c + w + 1].astype(np.int64)
    return {k: int(np.abs(a - R[r2 - w:r2 + w + 1, c2 + k - w:c2 + k + w + 1].astype(np.int64)).sum())
            for k in range(-s, s + 1)}


def subpix_one(L, R, r, c, r2, c2, w, s):
    """-> (dcol_q8, sad, status) of one match."""
    H, W = L.shape
    if not inside(H, W, r, c, r2, c2, w, s):
        return 0, -1, OUTSIDE
    sad = sads(L, R, r, c, r2, c2, w, s)
    best = None
    for k in search_order(s):
        if best is None or sad[k] < sad[best]:  # strict: the first minimum in the order
            best = k
    if abs(best) == s:
        return 0, sad[best], EDGE
    a, b, cc = sad[best - 1], sad[best], sad[best + 1]
    den = a + cc - 2 * b
    assert den >= 0 and abs(a - cc) <= den
    frac = 0 if den == 0 else (256 * (a - cc) + den) // (2 * den)  # python's // floors
    assert -128 <= frac <= 128
    return 256 * best + frac, b, OK


def subpix_slow(L, R, rc1, rc2, w, s):
    """subpix_one of every match: the specification as it is written down."""
    rc1 = np.asarray(rc1, np.int64).reshape(-1, 2)
    rc2 = np.asarray(rc2, np.int64).reshape(-1, 2)
    out = [subpix_one(L, R, int(a[0]), int(a[1]), int(b[0]), int(b[1]), w, s) for a, b in zip(rc1, rc2)]
    o = np.array(out, np.int64).reshape(-1, 3)
    return o[:, 0].astype(np.int32), o[:, 1].astype(np.int32), o[:, 2].astype(np.uint8)


def subpix(L, R, rc1, rc2, w, s):
    """Every match (rc1[i] in L, rc2[i] in R; (row, col)) -> (dcol_q8 [n] int32, sad [n] int32, status [n] uint8).
    The same arithmetic as subpix_one over all matches at once (tests/test_stereo_subpix_abi.py holds the two
    together)."""
    L, R = np.asarray(L), np.asarray(R)
    assert L.shape == R.shape and 1 <= w <= 7 and 1 <= s <= 8
    H, W = L.shape
    rc1 = np.asarray(rc1, np.int64).reshape(-1, 2)
    rc2 = np.asarray(rc2, np.int64).reshape(-1, 2)
    n = len(rc1)
    dq, sad, st = np.zeros(n, np.int64), np.full(n, -1, np.int64), np.full(n, OUTSIDE, np.int64)
    r, c, r2, c2 = rc1[:, 0], rc1[:, 1], rc2[:, 0], rc2[:, 1]
    ins = ((r - w >= 0) & (r + w < H) & (c - w >= 0) & (c + w < W) & (r2 - w >= 0) & (r2 + w < H)
           & (c2 - s - w >= 0) & (c2 + s + w < W))
    idx = np.nonzero(ins)[0]
    if len(idx) == 0:
        return dq.astype(np.int32), sad.astype(np.int32), st.astype(np.uint8)
    d = np.arange(-w, w + 1)
    r, c, r2, c2 = r[idx, None, None], c[idx, None, None], r2[idx, None, None], c2[idx, None, None]
    a = L[r + d[None, :, None], c + d[None, None, :]].astype(np.int64)
    S = np.stack([np.abs(a - R[r2 + d[None, :, None], c2 + k + d[None, None, :]].astype(np.int64)).sum((1, 2))
                  for k in range(-s, s + 1)], 1)                      # [m, 2 s + 1], column k + s
    order = np.array(search_order(s))
    pos = np.argmin(S[:, order + s], axis=1)                          # argmin returns the first minimum
    kb = order[pos]
    rows = np.arange(len(idx))
    b = S[rows, kb + s]
    edge = np.abs(kb) == s
    ka = np.where(edge, 0, kb)                                        # any bracketed shift: masked below
    av, cv = S[rows, ka - 1 + s], S[rows, ka + 1 + s]
    den = av + cv - 2 * b
    ok = ~edge
    assert (den[ok] >= 0).all() and (np.abs(av - cv)[ok] <= den[ok]).all()
    frac = np.where(den == 0, 0, (256 * (av - cv) + den) // np.where(den == 0, 1, 2 * den))  # // floors
    assert (np.abs(frac[ok]) <= 128).all()
    dq[idx] = np.where(edge, 0, 256 * kb + frac)
    sad[idx] = b
    st[idx] = np.where(edge, EDGE, OK)
    return dq.astype(np.int32), sad.astype(np.int32), st.astype(np.uint8)


def subpix_matches(L, R, m, w, s):
    """subpix of MATCH_DTYPE records (pt1 in L, pt2 in R)."""
    m = np.asarray(m, MATCH_DTYPE)
    return subpix(L, R, np.stack([m["pt1"]["x"], m["pt1"]["y"]], 1), np.stack([m["pt2"]["x"], m["pt2"]["y"]], 1), w, s)


def make_matches(rc1, rc2):
    """MATCH_DTYPE records with pt1 = rc1[i], pt2 = rc2[i] (row, col), ids = the index."""
    rc1 = np.asarray(rc1, np.int64).reshape(-1, 2)
    rc2 = np.asarray(rc2, np.int64).reshape(-1, 2)
    m = np.zeros(len(rc1), MATCH_DTYPE)
    for pt, rc in (("pt1", rc1), ("pt2", rc2)):
        m[pt]["x"], m[pt]["y"], m[pt]["id"] = rc[:, 0], rc[:, 1], np.arange(len(rc))
    return m


def refined_column(c2, dcol_q8):
    """(double)c2 + (double)dcol_q8 * (1.0 / 256.0): exact in double."""
    return np.asarray(c2, np.float64) + np.asarray(dcol_q8, np.float64) * (1.0 / 256.0)


def triangulate_refined(oracle, Ta, Tb, K, m, dcol_q8=None):
    """triangulate2View's per-match part with the refined right column: pixel2camera of both points as
    or_triangulate_matches forms it (the column of pt2 replaced), or_triangulate_one, ok = success and Z > 0.
    -> (X [n, 3], ok [n] bool).  dcol_q8 None: the integer column."""
    m = np.asarray(m, MATCH_DTYPE)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    Ta, Tb = np.ascontiguousarray(Ta, np.float64), np.ascontiguousarray(Tb, np.float64)
    n = len(m)
    y2 = m["pt2"]["y"].astype(np.float64)
    if dcol_q8 is not None:
        y2 = refined_column(m["pt2"]["y"], dcol_q8)
    pa = np.stack([(m["pt1"]["x"].astype(np.float64) - K[2]) * 1.0 / K[0],
                   (m["pt1"]["y"].astype(np.float64) - K[5]) * 1.0 / K[4]], 1)
    pb = np.stack([(m["pt2"]["x"].astype(np.float64) - K[2]) * 1.0 / K[0], (y2 - K[5]) * 1.0 / K[4]], 1)
    pa, pb = np.ascontiguousarray(pa), np.ascontiguousarray(pb)
    X = np.zeros((max(n, 1), 3))
    ok = np.zeros(n, bool)
    for i in range(n):
        s = oracle.lib.or_triangulate_one(Ta.ctypes.data, Tb.ctypes.data, pa[i:i + 1].ctypes.data,
                                          pb[i:i + 1].ctypes.data, X[i:i + 1].ctypes.data)
        ok[i] = bool(s) and X[i, 2] > 0
    return X[:n], ok


# ---- the fixture with a known sub-pixel disparity ----
FIX_H, FIX_W = 96, 320
_FINE0 = 128                                                       # the left crop's fine column offset
_GAUSS49 = np.rint(256.0 * np.exp(-np.arange(-24, 25) ** 2 / 128.0)).astype(np.int64)


def _coarse_field(seed, n_fine):
    """[FIX_H, n_fine] int64: the noise field at 4x column resolution, blurred vertically with _GAUSS13 and
    horizontally with _GAUSS49 (valid parts; integer sums)."""
    n = _noise(seed, 0, 0, FIX_H + 12, n_fine + 48)
    v = np.zeros((FIX_H, n_fine + 48), np.int64)
    for i, g in enumerate(_GAUSS13):
        v += g * n[i:i + FIX_H, :]
    h = np.zeros((FIX_H, n_fine), np.int64)
    for j, g in enumerate(_GAUSS49):
        h += g * v[:, j:j + n_fine]
    return h


def disparity_pair(dq, seed=7):
    """(left, right) uint8 FIX_H x FIX_W images of one scene at true disparity dq / 4 pixels: the content of left column
    c is at right column c - dq / 4.  Each pixel is the sum of four fine columns, scaled to mean 128 / std 56 with the
    left image's own statistics."""
    f = _coarse_field(seed, _FINE0 + dq + 4 * FIX_W)

    def crop(off):
        return f[:, off:off + 4 * FIX_W].reshape(FIX_H, FIX_W, 4).sum(2).astype(np.float64)

    left, right = crop(_FINE0), crop(_FINE0 + dq)
    mean, std = left.mean(), left.std()
    q = [np.clip(np.floor(128.0 + 56.0 * (x - mean) / std + 0.5), 0, 255).astype(np.uint8) for x in (left, right)]
    return q[0], q[1]


def disparity_points(dq, n=300, seed=11):
    """n seeded left positions rc1 and start positions rc2 in the right image: the rounded true match plus a seeded
    column offset in {-1, 0, 1}, every footprint inside for every (w, s) of the envelope.  -> (rc1, rc2, true right
    column [n] float64)."""
    rng = np.random.default_rng(seed)
    r = rng.integers(7, FIX_H - 7, n)
    c = rng.integers(32, 301, n)
    true_c2 = c - dq / 4.0
    c2 = np.floor(true_c2 + 0.5).astype(np.int64) + rng.integers(-1, 2, n)
    rc1, rc2 = np.stack([r, c], 1), np.stack([r, c2], 1)
    assert all(inside(FIX_H, FIX_W, *a, *b, 7, 8) for a, b in zip(rc1.tolist(), rc2.tolist()))
    return rc1, rc2, true_c2
