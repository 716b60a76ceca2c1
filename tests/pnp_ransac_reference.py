"""The specification of the P3P-RANSAC absolute pose (yv_pnp_ransac / yv_pnp_ransac_batch, ya_vo_amd/csrc/yavo_pnp.hip).

Every value is an IEEE float64 and every expression is written out as scalar operations in one stated order: a
product or a sum of several terms associates from the left exactly as it is written here, a division and a square
root are the correctly rounded ones, and nothing is contracted into a fused multiply-add (the kernels are built with
-ffp-contract=off).  No np.dot, np.cross, np.linalg, np.roots and no Python complex: the GPU result equals this file bit
for bit, so it is the only place where the order of the operations is decided.  The hypothesis part runs on Python
floats (IEEE doubles; _div and _sqrt give the IEEE result where Python would raise); the score of a pose runs the same
scalar expression on every edge at once as element-wise numpy arrays, which add no operation and reorder none.

Conventions are the pose LM's (include/yavo/yavo_geom.h): X [n][3] world points, uv [n][2] measurements with uv[0]
along K's first row, K [9] row-major, pose [7] = {qx, qy, qz, qw, tx, ty, tz} (T_cw).

    sampling   hypothesis h uses the edges draws[h][k] % n, k = 0, 1, 2; two equal indices: no candidate
    bearings   j = ((u - K[2]) / K[0], (v - K[5]) / K[4], 1) / norm
    solver     Grunert's P3P: the quartic in v = s3 / s1, Durand-Kerner on the monic quartic (kSweeps Gauss-Seidel
               sweeps from the fixed starting points (0.4 + 0.9i)^k, no data-dependent stop)
    pose       the rotation between the orthonormal frames of the world triangle and of the camera triangle
               Qi = si ji, its quaternion by Eigen's branches (oracle or_se3_from_Rt), normalised in or_se3_inverse's
               summation order, t = Q1 - R P1
    score      edge i is an inlier iff its camera-frame z > 0 and e0^2 + e1^2 < thr^2, e the pose LM's edge error
               (yavo_se3.h se3_act, yavo_edge.h edge_error_pc) at that pose[7]
    selection  most inliers; ties to the lowest hypothesis, then the lowest root; found iff count >= min_inliers,
               otherwise the pose is left as it was, the mask is zero and the count is 0
"""
import math

import numpy as np

kSweeps = 40
kMaxEdges = 4096  # the batch form scores (and samples) a problem's first 4096 edges, as the pose LM does
_NAN = float("nan")
_INF = float("inf")


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return _NAN
        return math.copysign(_INF, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(a):
    """IEEE sqrt (Python raises on a negative argument; sqrt(-0.0) = -0.0)."""
    if a < 0.0:
        return _NAN
    return math.sqrt(a)


def _finite(a):
    return a - a == 0.0  # false for NaN and the infinities


def _dist2(A, B):
    dx = A[0] - B[0]
    dy = A[1] - B[1]
    dz = A[2] - B[2]
    return dx * dx + dy * dy + dz * dz


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def bearing(u, v, K):
    x = _div(u - K[2], K[0])
    y = _div(v - K[5], K[4])
    n = _sqrt(x * x + y * y + 1.0)
    return (_div(x, n), _div(y, n), _div(1.0, n))


def quartic(P, j):
    """Grunert's quartic of the triangle P[3] seen along the bearings j[3] -> None (b^2 is not > 0) or
    (A[5] = A0 .. A4, (q, a2, b2, ca, cb, cg))."""
    a2 = _dist2(P[1], P[2])
    b2 = _dist2(P[0], P[2])
    c2 = _dist2(P[0], P[1])
    if not (b2 > 0.0):
        return None
    ca = _dot(j[1], j[2])
    cb = _dot(j[0], j[2])
    cg = _dot(j[0], j[1])
    q = (a2 - c2) / b2
    p = (a2 + c2) / b2
    rab = a2 / b2
    rcb = c2 / b2
    ca2 = ca * ca
    cb2 = cb * cb
    cg2 = cg * cg
    A4 = (q - 1.0) * (q - 1.0) - 4.0 * rcb * ca2
    A3 = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * rcb * ca2 * cb)
    A2 = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb2 + 2.0 * ((b2 - c2) / b2) * ca2 - 4.0 * p * ca * cb * cg
                + 2.0 * ((b2 - a2) / b2) * cg2)
    A1 = 4.0 * (-q * (1.0 + q) * cb + 2.0 * rab * cg2 * cb - (1.0 - p) * ca * cg)
    A0 = (1.0 + q) * (1.0 + q) - 4.0 * rab * cg2
    return (A0, A1, A2, A3, A4), (q, a2, b2, ca, cb, cg)


def dk_quartic(c0, c1, c2, c3):
    """The four roots of x^4 + c3 x^3 + c2 x^2 + c1 x + c0 -> (re[4], im[4]): Durand-Kerner, complex arithmetic in real
    operations (the shape of yavo_essential.hip's dk_solve), root i updated from the roots j < i of this sweep and
    j > i of the last one."""
    xr = [0.0] * 4
    xi = [0.0] * 4
    pr, pi = 1.0, 0.0
    for i in range(4):
        xr[i] = pr
        xi[i] = pi
        tr = pr * 0.4 - pi * 0.9
        ti = pr * 0.9 + pi * 0.4
        pr, pi = tr, ti
    cs = (c2, c1, c0)
    for _ in range(kSweeps):
        for i in range(4):
            pr = xr[i]
            pi = xi[i]
            # Horner: ((x + c3) x + c2) x + c1) x + c0
            nr = pr + c3
            ni = pi
            for c in cs:
                tr = nr * pr - ni * pi
                ti = nr * pi + ni * pr
                nr = tr + c
                ni = ti
            # the product of (x_i - x_j), j != i in ascending order
            first = True
            dr = 0.0
            di = 0.0
            for j in range(4):
                if j == i:
                    continue
                sr = pr - xr[j]
                si = pi - xi[j]
                if first:
                    dr, di = sr, si
                    first = False
                else:
                    ur = dr * sr - di * si
                    ui = dr * si + di * sr
                    dr, di = ur, ui
            t = _div(1.0, dr * dr + di * di)
            qr = (nr * dr + ni * di) * t
            qi = (ni * dr - nr * di) * t
            xr[i] = pr - qr
            xi[i] = pi - qi
    return xr, xi


def _frame(A, B, C):
    """e1 = (B - A) / |B - A|, e3 = (e1 x (C - A)) / |.|, e2 = e3 x e1"""
    d = (B[0] - A[0], B[1] - A[1], B[2] - A[2])
    n1 = _sqrt(_dot(d, d))
    e1 = (_div(d[0], n1), _div(d[1], n1), _div(d[2], n1))
    g = (C[0] - A[0], C[1] - A[1], C[2] - A[2])
    c = (e1[1] * g[2] - e1[2] * g[1], e1[2] * g[0] - e1[0] * g[2], e1[0] * g[1] - e1[1] * g[0])
    n3 = _sqrt(_dot(c, c))
    e3 = (_div(c[0], n3), _div(c[1], n3), _div(c[2], n3))
    e2 = (e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0])
    return e1, e2, e3


def quat_from_R(R):
    """Eigen's quaternion of a rotation matrix (row-major R[9]) by or_se3_from_Rt's branches, then the division by its
    norm in or_se3_inverse's summation order -> [x, y, z, w]"""
    q = [0.0] * 4
    tr = (R[0] + R[4]) + R[8]
    if tr > 0.0:
        tr = _sqrt(tr + 1.0)
        q[3] = 0.5 * tr
        tr = _div(0.5, tr)
        q[0] = (R[7] - R[5]) * tr
        q[1] = (R[2] - R[6]) * tr
        q[2] = (R[3] - R[1]) * tr
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        tr = _sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
        q[i] = 0.5 * tr
        tr = _div(0.5, tr)
        q[3] = (R[3 * k + j] - R[3 * j + k]) * tr
        q[j] = (R[3 * j + i] + R[3 * i + j]) * tr
        q[k] = (R[3 * k + i] + R[3 * i + k]) * tr
    ln = _sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    return [_div(q[0], ln), _div(q[1], ln), _div(q[2], ln), _div(q[3], ln)]


def p3p_candidates(P, j):
    """The candidate poses of one hypothesis (world triangle P[3], bearings j[3]) -> a list of (root index, pose[7]) in
    root order."""
    qa = quartic(P, j)
    if qa is None:
        return []
    (A0, A1, A2, A3, A4), (q, a2, b2, ca, cb, cg) = qa
    if not (abs(A4) > 0.0):
        return []
    re, im = dk_quartic(_div(A0, A4), _div(A1, A4), _div(A2, A4), _div(A3, A4))
    w1, w2, w3 = _frame(P[0], P[1], P[2])
    out = []
    for r in range(4):
        v = re[r]
        if not (abs(im[r]) <= 1e-7 * (1.0 + abs(v))):
            continue
        if not (v > 0.0):
            continue
        du = 2.0 * (cg - v * ca)
        if not (abs(du) > 0.0):
            continue
        u = ((q - 1.0) * v * v - 2.0 * q * cb * v + 1.0 + q) / du
        if not (u > 0.0):
            continue
        ds = 1.0 + v * v - 2.0 * v * cb
        if not (ds > 0.0):
            continue
        s1 = _sqrt(b2 / ds)
        s2 = u * s1
        s3 = v * s1
        Q1 = (s1 * j[0][0], s1 * j[0][1], s1 * j[0][2])
        Q2 = (s2 * j[1][0], s2 * j[1][1], s2 * j[1][2])
        Q3 = (s3 * j[2][0], s3 * j[2][1], s3 * j[2][2])
        k1, k2, k3 = _frame(Q1, Q2, Q3)
        R = [0.0] * 9
        for a in range(3):
            for b in range(3):
                R[3 * a + b] = k1[a] * w1[b] + k2[a] * w2[b] + k3[a] * w3[b]
        t = [Q1[a] - (R[3 * a] * P[0][0] + R[3 * a + 1] * P[0][1] + R[3 * a + 2] * P[0][2]) for a in range(3)]
        qt = quat_from_R(R)
        pose = qt + t
        if not all(_finite(x) for x in R) or not all(_finite(x) for x in pose):
            continue
        out.append((r, pose))
    return out


def inlier_mask(pose, X, uv, K, thr):
    """What the pose LM's own edge says about `pose`: se3_act (Eigen's quaternion rotation) and edge_error_pc, the same
    scalar expression on every edge (element-wise arrays) -> bool [n]"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    q0, q1, q2, q3, t0, t1, t2 = (np.float64(x) for x in pose)
    K = [np.float64(x) for x in K]
    v0, v1, v2 = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        uv0 = q1 * v2 - q2 * v1
        uv1 = q2 * v0 - q0 * v2
        uv2 = q0 * v1 - q1 * v0
        uv0 = uv0 + uv0
        uv1 = uv1 + uv1
        uv2 = uv2 + uv2
        c0 = q1 * uv2 - q2 * uv1
        c1 = q2 * uv0 - q0 * uv2
        c2 = q0 * uv1 - q1 * uv0
        p0 = (v0 + q3 * uv0 + c0) + t0
        p1 = (v1 + q3 * uv1 + c1) + t1
        p2 = (v2 + q3 * uv2 + c2) + t2
        u0 = K[0] * p0 + K[1] * p1 + K[2] * p2
        u1 = K[3] * p0 + K[4] * p1 + K[5] * p2
        u2 = K[6] * p0 + K[7] * p1 + K[8] * p2
        e0 = uv[:, 0] - u0 / u2
        e1 = uv[:, 1] - u1 / u2
        thr2 = np.float64(thr) * np.float64(thr)
        return (p2 > 0.0) & (e0 * e0 + e1 * e1 < thr2)


def hypothesis_candidates(X, uv, K, draw, n):
    """Candidates of the hypothesis with draws `draw` [3] over the first n edges."""
    if n <= 0:
        return []
    i0, i1, i2 = (int(d) % n for d in draw)
    if i0 == i1 or i0 == i2 or i1 == i2:
        return []
    P = [tuple(float(x) for x in X[i]) for i in (i0, i1, i2)]
    j = [bearing(float(uv[i][0]), float(uv[i][1]), K) for i in (i0, i1, i2)]
    return p3p_candidates(P, j)


def pnp_ransac(X, uv, K, draws, thr, min_inliers, pose=None):
    """-> (pose [7], inlier mask bool [n], inliers, found, candidate counts [iters]).  `pose` is what a caller passed
    in and gets back when nothing is found (zeros if None).  A problem of more than kMaxEdges edges is solved on its
    first kMaxEdges, and the mask past them is False."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    K = [float(x) for x in np.asarray(K, np.float64).reshape(9)]
    draws = np.asarray(draws, np.uint32).reshape(-1, 3)
    n_all = len(X)
    n = min(n_all, kMaxEdges)
    out_pose = np.zeros(7) if pose is None else np.array(pose, np.float64).reshape(7).copy()
    best, best_pose, best_mask = -1, None, None
    ncand = np.zeros(len(draws), np.int32)
    for h in range(len(draws)):
        cands = hypothesis_candidates(X, uv, K, draws[h], n)
        ncand[h] = len(cands)
        for _, T in cands:
            m = inlier_mask(T, X[:n], uv[:n], K, thr)
            c = int(m.sum())
            if c > best:  # strict: the first candidate in (hypothesis, root) order keeps a tie
                best, best_pose, best_mask = c, T, m
    mask = np.zeros(n_all, bool)
    if best >= min_inliers and best >= 0:
        mask[:n] = best_mask
        return np.array(best_pose, np.float64), mask, best, True, ncand
    return out_pose, mask, 0, False, ncand


def make_draws(iters, seed=0):
    """The draws table of Batch.set_track_ransac / Context.pnp_ransac(seed=...): uint32 [iters][3]"""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(iters, 3), dtype=np.uint32)
