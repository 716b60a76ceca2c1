"""Synthetic two-view scenes for the findEssentialMat / recoverPose tests (KITTI intrinsics)."""
import numpy as np

K_KITTI = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])


def two_view_scene(n, outlier_frac=0.0, seed=0, noise=0.0, angle=0.05, t=(0.2, 0.01, 1.0), rounded=True):
    """points1 in camera 1, points2 = R X + t in camera 2, projected with the KITTI K -> (p1, p2, R, t_unit)."""
    r = np.random.default_rng(seed)
    X = np.c_[r.uniform(-10, 10, n), r.uniform(-3, 3, n), r.uniform(5, 40, n)]
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = np.asarray(t, np.float64)
    X2 = X @ R.T + t

    def proj(P):
        return (P / P[:, 2:3]) @ K_KITTI.T

    p1, p2 = proj(X)[:, :2], proj(X2)[:, :2]
    if noise:
        p1 = p1 + r.normal(0, noise, p1.shape)
        p2 = p2 + r.normal(0, noise, p2.shape)
    if rounded:
        p1, p2 = np.round(p1), np.round(p2)
    k = int(outlier_frac * n)
    if k:
        p2[:k] += r.uniform(-60, 60, (k, 2))
    return p1, p2, R, t / np.linalg.norm(t)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


# ------------------------------------------------------------------------------------------------
# Degenerate corpus (tests/test_gpu_essential_degenerate.py): inputs that leave the five-point solver's one common path
# (regular LU, degree 10, no coincident Durand-Kerner iterates, no solveZ reject, 300 sweeps, an even model count).  All
# seeded; pixel coordinates are float32-exact so the oracle and the kernels read the same numbers.
# ------------------------------------------------------------------------------------------------
FOCAL, PP = 718.856, (607.1928, 185.2157)


def normalize(p, focal=FOCAL, pp=PP):
    """(p - c) / f as OpenCV's MatExpr evaluates it (or_normalize_points)."""
    a = 1. / focal
    p = np.asarray(p, np.float64)
    return np.stack([p[:, 0] * a + (-pp[0] * a), p[:, 1] * a + (-pp[1] * a)], 1)


def planar_scene(n, seed, rounded=True):
    """A scene whose points lie on one plane (a homography between the images: the five-point solver's classic
    degenerate structure)."""
    r = np.random.default_rng(seed)
    x, y = r.uniform(-10, 10, n), r.uniform(-3, 3, n)
    X = np.c_[x, y, 20 + 0.3 * x - 0.5 * y]
    c, s = np.cos(0.05), np.sin(0.05)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    X2 = X @ R.T + np.array([0.2, 0.01, 1.0])
    p1, p2 = ((X / X[:, 2:3]) @ K_KITTI.T)[:, :2], ((X2 / X2[:, 2:3]) @ K_KITTI.T)[:, :2]
    return (np.round(p1), np.round(p2)) if rounded else (p1, p2)


def _yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rotation_scene(n, seed):
    """A camera that only turns (no translation); sub-pixel coordinates."""
    r = np.random.default_rng(seed)
    X = np.c_[r.uniform(-10, 10, n), r.uniform(-3, 3, n), r.uniform(5, 40, n)]
    X2 = X @ _yaw(0.05).T
    return ((X / X[:, 2:3]) @ K_KITTI.T)[:, :2], ((X2 / X2[:, 2:3]) @ K_KITTI.T)[:, :2]


def collinear_scene(n, seed):
    """Every point of both images on one image row."""
    r = np.random.default_rng(seed)
    row = float(r.integers(20, 350))
    u = r.integers(0, 1200, n).astype(np.float64)
    p1 = np.c_[u, np.full(n, row)]
    p2 = np.c_[u + r.integers(-30, 31, n), np.full(n, row)]
    return p1, p2


FIVE_POINT_FAMILIES = ("general", "identical", "rotation", "collinear", "unit", "lattice", "same", "zeros", "duplicate",
                       "planar", "threshold")
# "unit" seeds (found with the traced oracle) whose solveZ vectors have a last component near the 1e-10 reject: seed
# 1068 has roots on both sides (1.4e-10 kept, 8.2e-11 rejected), the others lie between 6e-13 and 4e-9
THRESHOLD_SEEDS = (1068, 10736, 1166, 11153, 10023, 10330, 10927, 11548)


def five_point_subset(family, seed):
    """One subset of five NORMALISED correspondences (q1, q2 [5, 2] float64) of the family."""
    r = np.random.default_rng(1000 + seed)
    if family == "threshold":
        return five_point_subset("unit", THRESHOLD_SEEDS[seed % len(THRESHOLD_SEEDS)])
    if family == "general":  # rounded pixels of a general scene: the path every other test takes
        p1, p2, _, _ = two_view_scene(5, seed=seed)
    elif family == "identical":  # a stationary camera: both images the same
        p1, _, _, _ = two_view_scene(5, seed=seed)
        p2 = p1
    elif family == "rotation":  # no translation, sub-pixel coordinates
        p1, p2 = rotation_scene(5, seed)
    elif family == "collinear":
        p1, p2 = collinear_scene(5, seed)
    elif family == "unit":  # coordinates in {-1, 0, 1} after normalisation
        return r.integers(-1, 2, (5, 2)).astype(np.float64), r.integers(-1, 2, (5, 2)).astype(np.float64)
    elif family == "lattice":  # 64-pixel steps around the principal point
        c = np.round(np.array(PP))
        p1, p2 = c + 64.0 * r.integers(-2, 3, (5, 2)), c + 64.0 * r.integers(-2, 3, (5, 2))
    elif family == "same":  # all five the same correspondence
        p1 = np.tile(r.integers(0, 1200, (1, 2)).astype(np.float64), (5, 1))
        p2 = np.tile(r.integers(0, 1200, (1, 2)).astype(np.float64), (5, 1))
    elif family == "zeros":
        return np.zeros((5, 2)), np.zeros((5, 2))
    elif family == "duplicate":  # one correspondence twice
        p1, p2, _, _ = two_view_scene(5, seed=seed)
        p1[4], p2[4] = p1[0], p2[0]
    elif family == "planar":
        p1, p2 = planar_scene(5, seed)
    else:
        raise ValueError(family)
    return normalize(p1), normalize(p2)


def five_point_corpus(per_family=64):
    """-> (q1, q2 [n, 5, 2], family index [n]); neighbouring subsets come from different families (subset k is of family
    k % 11), so the four rows of a group-form wave and the 64 lanes of a lane-form wave take different arms at once."""
    nf = len(FIVE_POINT_FAMILIES)
    q1, q2, fam = [], [], []
    for k in range(per_family * nf):
        a, b = five_point_subset(FIVE_POINT_FAMILIES[k % nf], k // nf)
        q1.append(a)
        q2.append(b)
        fam.append(k % nf)
    return np.array(q1), np.array(q2), np.array(fam)


def _poly_from_roots(roots):
    c = np.array([1.0])
    for z in roots:
        c = np.convolve(c, np.array([-float(z), 1.0]))  # ascending coefficients
    return c


def poly_corpus():
    """-> (coeffs [n, 11] ascending, names [n]).  The named shapes at every degree 1 .. 10, the trim and 0 / 0 cases, and
    polynomials found (by a search with the traced oracle) to bring two Durand-Kerner iterates to exactly the same
    value at degrees above 3; consecutive entries have different degrees."""
    polys = []
    for k in range(1, 11):
        e = np.zeros(k + 1)
        e[k] = 1.0
        polys.append((f"z^{k}", e.copy()))
        e[0] = 1.0
        polys.append((f"z^{k}+1", e.copy()))
        e[0] = -1.0
        polys.append((f"z^{k}-1", e.copy()))
        polys.append((f"(z-1)..(z-{k})", _poly_from_roots(range(1, k + 1))))
        if k >= 2:
            polys.append((f"(z-1)^2 z^{k - 2}", np.r_[np.zeros(k - 2), 1.0, -2.0, 1.0]))
    polys.append(("zero", np.zeros(11)))
    polys.append(("constant", np.array([3.0])))
    polys.append(("leading 1e-17", np.r_[_poly_from_roots([0.5, -1.5, 2.0, -0.25, 3.0, 1.25, -2.5, 0.75, -3.5]), 1e-17]))
    for name, c in COINCIDENT_POLYS:
        polys.append((name, np.asarray(c, np.float64)))
    # interleave the degrees: sort round-robin over the degree classes
    by_deg = {}
    for name, c in polys:
        by_deg.setdefault(len(c), []).append((name, c))
    order = []
    while any(by_deg.values()):
        for d in sorted(by_deg):
            if by_deg[d]:
                order.append(by_deg[d].pop(0))
    coeffs = np.zeros((len(order), 11))
    for i, (_, c) in enumerate(order):
        coeffs[i, :len(c)] = c
    return coeffs, [n for n, _ in order]


# polynomials (ascending coefficients) on which cv::solvePoly's Durand-Kerner meets two exactly equal iterates
# at degrees 4, 6, 7, 8, 9 and 10 ((z-1)^2 and (z-1)^2 z do at degrees 2 and 3; a search of 400,000 polynomials with
# coefficients in -2 .. 2 found none at degree 5)
COINCIDENT_POLYS = [
    ("z^2 (z^2-1)", [0, 0, -1, 0, 1]),
    ("z^3 (z-1)", [0, 0, 0, -1, 1]),
    ("coincident 6", [-1, -2, 2, 2, 1, 0, -2]),
    ("coincident 7", [0, -1, -1, 2, 1, 0, 0, -1]),
    ("coincident 8", [1, -1, 2, -2, 1, -2, -1, 1, 1]),
    ("coincident 9", [0, 2, -2, 1, -2, -2, 2, 2, 0, -1]),
    ("coincident 10a", [-1, 2, -1, 0, -2, 0, 1, 2, 2, -2, -1]),
    ("coincident 10b", [0, 1, -2, 2, 0, 2, -2, -2, -2, 1, 2]),
]


def _f32(p1, p2):
    return np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)


def degenerate_lists():
    """-> [(name, p1, p2)] float32 pixel lists for findEssentialMat + recoverPose: degenerate structure (most subsets
    take the solver's singular arm) and the sizes around the subset kernels' switches (5: the non-RANSAC path, whose E
    is the all-NaN first model here; 64: the parallel draw's smallest list; below it the sequential draw, which
    re-draws often at 6 and 7)."""
    out = []
    for n in (5, 64, 200):
        a, _, _, _ = two_view_scene(n, seed=20 + n)
        out.append((f"identical{n}", a, a))
    out.append(("zeros50", np.zeros((50, 2)), np.zeros((50, 2))))
    out.append(("collinear200",) + collinear_scene(200, 31))
    r = np.random.default_rng(32)
    out.append(("repeated100", np.tile(r.integers(0, 1200, (1, 2)), (100, 1)), np.tile(r.integers(0, 1200, (1, 2)), (100, 1))))
    a, b, _, _ = two_view_scene(100, outlier_frac=0.2, seed=33)
    out.append(("twice200", np.repeat(a, 2, 0), np.repeat(b, 2, 0)))
    out.append(("rotation200",) + rotation_scene(200, 34))
    out.append(("planar200",) + planar_scene(200, 35))
    for n in (6, 7, 63, 64, 65):
        a, b, _, _ = two_view_scene(n, outlier_frac=0.1, seed=40 + n)
        out.append((f"general{n}", a, b))
    return [(name,) + _f32(a, b) for name, a, b in out]


def outlier_list():
    """The 300-point, 50 %-outlier list of the workspace-parameter cases."""
    a, b, _, _ = two_view_scene(300, outlier_frac=0.5, seed=14)
    return _f32(a, b)


def pose_scenes(n=40):
    """-> [(name, p1, p2)] float32: yaw +-0.05 and 3.0, translation along +-z, +-x and mostly y, each also with the two
    images swapped -- between them every one of recoverPose's four candidates wins somewhere."""
    out = []
    for ai, angle in enumerate((0.05, -0.05, 3.0)):
        for ti, t in enumerate(((0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0.1, 1.0, 0.1))):
            a, b, _, _ = two_view_scene(n, seed=60 + 5 * ai + ti, angle=angle, t=t)
            out.append((f"yaw{angle}_t{ti}",) + _f32(a, b))
            out.append((f"yaw{angle}_t{ti}_swapped",) + _f32(b, a))
    return out
