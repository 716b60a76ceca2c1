"""Degenerate inputs of the pose solvers (pose_lm_kernel / pose_gn_kernel and their 6 x 6 LDLT), host only.

lm_corpus() -> pose problems in families that take the solvers' data-dependent arms ("the pose solvers'
data-dependent arms"): rounds without an active edge, an LDLT that is not positive, a non-finite trial chi2, zero and NaN
pivots, non-finite operands beside and away from Huber-weighted edges, far priors, tiny and coincident point sets.
interleave() orders them so that neighbouring workgroups of one launch take different arms.  ldlt_corpus() -> the
systems (H, lambda, b) of the direct LDLT test.  tests/test_gpu_pose_degenerate.py asserts on the oracle's traces that
the corpus is where it claims to be."""
import itertools

import numpy as np

from ya_vo_amd import scene

K_KITTI = scene.K_KITTI
DBL_MIN = 2.2250738585072014e-308


def _scene(n, seed, noise=0.3, outl=0.0, rot=0.02, trans=0.1, K=K_KITTI):
    """A random scene and a perturbed prior (rot = 0: the exact pose)."""
    X, uv, T, _ = scene.random_scene(max(n, 1), seed=seed, noise_px=noise, outlier_frac=outl, K=K)
    prior = scene.perturb(T, np.random.default_rng(seed + 1000), rot=rot, trans=trans) if rot else T.copy()
    return np.ascontiguousarray(X[:n]), np.ascontiguousarray(uv[:n]), K.copy(), prior


def _scaled_K(f):
    K = K_KITTI.copy()
    K[0, 0] *= f
    K[1, 1] *= f
    return K


def non_finite_scene(n, seed):
    """A scene whose prior puts some points exactly in the camera plane (pc_z = 0: u / 0 = inf, 0 / 0 = NaN errors)
    (tests/test_gpu_geom.py's _non_finite_scene)."""
    rng = np.random.default_rng(seed)
    T = scene.pose([0.0, 0.0, 0.0, 1.0], [0.25, -0.5, -5.0])  # identity rotation: pc = X + t exactly
    z = rng.uniform(9.0, 40.0, n)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.25, 0.25, n) * z, z], 1)
    X[:3, 2] = 5.0                                  # pc_z = 0 under the prior
    X[3] = [-0.25, 0.5, 5.0]                        # pc = 0: 0 / 0
    uv = scene.project(T, X) + rng.normal(scale=0.4, size=(n, 2))
    uv[:4] = [[600.0, 180.0], [10.0, 20.0], [1200.0, 300.0], [607.0, 185.0]]
    return np.ascontiguousarray(X), np.ascontiguousarray(uv), K_KITTI.copy(), T


# ------------------------------------------------------------------------------------------------
# the families: name -> function of a seed index s = 0, 1, ... -> (X [n, 3], uv [n, 2], K [3, 3], prior [7])
# ------------------------------------------------------------------------------------------------
def _far_prior(s):  # every edge an outlier after round 0: the later rounds have no active edge
    X, uv, K, prior = _scene(40 + 7 * s, 200 + s, rot=3.1)
    return X, uv, K, prior


def _random_uv(s):
    X, uv, K, prior = _scene(30 + 5 * s, 210 + s)
    rng = np.random.default_rng(s)
    return X, np.ascontiguousarray(rng.uniform(0, 1200, uv.shape)), K, prior


def _uv_huge(s):
    X, uv, K, prior = _scene((3, 50, 200)[s % 3], 220 + s)
    return X, uv * 1e160, K, prior


def _k_huge(s):  # H overflows: the LDLT reports not positive
    K = _scaled_K((1e100, 1e120, 1e150)[s % 3])
    X, uv, _, prior = _scene((3, 200)[s % 2], 230 + s, K=K)
    return X, uv, K, prior


def _k_overflow(s):  # exact data at the exact prior (weights 1), H's diagonal overflows to inf: lambda starts non-finite
    K = _scaled_K((1e160, 1e200, 1e250)[s % 3])
    X, uv, _, prior = _scene((50, 3, 200)[s % 3] + s, 380 + s, noise=0.0, rot=0, K=K)
    return X, uv, K, prior


def _x_huge(s):  # trial chi2 non-finite with a positive LDLT; zero pivots at k > 0
    X, uv, K, prior = _scene((20, 200, 64)[s % 3], 240 + s)
    return X * (1e153, 1e155, 1e160)[s % 3], uv, K, prior


def _in_camera_frame(X, prior, tz):
    """The scene's points in the camera frame, and a prior that keeps them exactly there: identity rotation and
    t = (tx, ty, tz) of a few bits each, so that pc = X + t is exact in z whenever X_z + tz is."""
    pc = scene.transform(prior, X)
    return pc, scene.pose([0.0, 0.0, 0.0, 1.0], [0.25, -0.5, tz])


def _z_tiny(s):  # camera-frame z = 1e-170 exactly (identity rotation, t_z = 0): every point, or every third one
    X, uv, K, prior = _scene(30 + s, 250 + s, rot=0)
    pc, prior = _in_camera_frame(X, prior, 0.0)
    pc[slice(None) if s % 2 == 0 else slice(0, None, 3), 2] = 1e-170
    return np.ascontiguousarray(pc - prior[4:]), uv, K, prior


def _k_tiny(s):
    K = _scaled_K(1e-165)
    X, uv, _, prior = _scene(30 + 9 * s, 260 + s)
    return X, uv, K, prior


def _near_plane(s):  # two near-plane points among 200 normal ones
    X, uv, K, prior = non_finite_scene(200, 270 + s)
    X[:4, 2] = 5.0 + np.array([1e-9, -1e-12, 1e-7, 2e-10]) * (s + 1)
    X[2:4] = X[4:6]
    uv[2:4] = scene.project(prior, X[2:4])
    return X, uv, K, prior


def _tiny_n(s):  # n = 0 .. 6
    X, uv, K, prior = _scene(s % 7, 280 + s)
    return X, uv, K, prior


def _coincident(s):
    X, uv, K, prior = _scene(24 + s, 290 + s)
    X[:] = X[0]
    if s % 2:
        uv[:] = uv[0]
    return X, uv, K, prior


def _collinear(s):
    X, uv, K, prior = _scene(40 + s, 300 + s, rot=0)
    d = np.random.default_rng(s).normal(size=3)
    X = X[0] + np.linspace(-1.0, 1.0, len(X))[:, None] * d
    prior2 = scene.perturb(prior, np.random.default_rng(s), rot=0.02 * (s % 3), trans=0.1)
    return np.ascontiguousarray(X), scene.project(prior, X), K, prior2


def _exact(s):  # exact data with the exact prior
    return _scene(50 + 30 * s, 310 + s, noise=0.0, rot=0)


def _rotated(s):
    return _scene(80 + 11 * s, 320 + s, outl=0.1 * (s % 2), rot=(0.3, 1.0, 2.5, 3.1)[s % 4])


def _behind(s):  # points behind the camera (all of them, or every third)
    X, uv, K, prior = _scene(60 + s, 330 + s)
    pc = scene.transform(prior, X)
    sel = slice(None) if s % 2 == 0 else slice(0, None, 3)
    pc[sel, 2] *= -1.0
    R = scene.quat_to_R(prior[:4])
    return np.ascontiguousarray((R.T @ (pc - prior[4:]).T).T), uv, K, prior


_BAD = (("point", np.nan), ("point", np.inf), ("meas", np.nan), ("meas", -np.inf))


def _poison(X, uv, where, s):
    what, v = _BAD[s % 4]
    (X if what == "point" else uv)[where, s % (3 if what == "point" else 2)] = v


def _bad_quiet(s):  # a non-finite operand in a wave whose other edges all stay below the Huber threshold
    X, uv, K, prior = _scene(48 + s, 340 + s, noise=0.1, rot=0)
    _poison(X, uv, 5 + s, s)
    return X, uv, K, prior


def _bad_huber(s):  # ... and in a wave that has Huber-weighted edges
    X, uv, K, prior = _scene(56 + s, 350 + s, noise=0.5, outl=0.2)
    _poison(X, uv, 7 + s, s)
    return X, uv, K, prior


def _bad_two_waves(s):  # wave 0 quiet with the bad edge, wave 1 with Huber-weighted edges
    X, uv, K, prior = _scene(128, 360 + s, noise=0.1, rot=0)
    rng = np.random.default_rng(s)
    uv[64:] += rng.normal(scale=3.0, size=(64, 2))
    _poison(X, uv, 11 + s, s)
    return X, uv, K, prior


def _camera_plane(s):
    return non_finite_scene(150 + 20 * s, 5 + s)


def _normal(s):  # ordinary noisy scenes with outliers between the degenerate ones
    return _scene(100 + 37 * s, 370 + s, noise=0.5, outl=0.1)


LM_FAMILIES = {
    "far_prior": _far_prior, "random_uv": _random_uv, "uv_huge": _uv_huge, "k_huge": _k_huge, "k_overflow": _k_overflow, "x_huge": _x_huge,
    "z_tiny": _z_tiny, "k_tiny": _k_tiny, "near_plane": _near_plane, "tiny_n": _tiny_n, "coincident": _coincident,
    "collinear": _collinear, "exact": _exact, "rotated": _rotated, "behind": _behind, "bad_quiet": _bad_quiet,
    "bad_huber": _bad_huber, "bad_two_waves": _bad_two_waves, "camera_plane": _camera_plane, "normal": _normal,
}
# far_prior: seeds 7 .. 10 keep the GN going for all ten iterations; k_huge: one seed in three has a trial whose LDLT is
# not positive; bad_two_waves: a -inf measurement (s % 4 == 3) is past the Huber threshold itself
LM_SEEDS = {"far_prior": 11, "k_huge": 15, "tiny_n": 7, "rotated": 8, "bad_quiet": 8, "bad_huber": 8, "bad_two_waves": 8}
DEFAULT_SEEDS = 6


def lm_corpus():
    """-> list of (family, X, uv, K, prior), family by family."""
    out = []
    for name, fn in LM_FAMILIES.items():
        for s in range(LM_SEEDS.get(name, DEFAULT_SEEDS)):
            X, uv, K, prior = fn(s)
            out.append((name, np.ascontiguousarray(X, np.float64).reshape(-1, 3),
                        np.ascontiguousarray(uv, np.float64).reshape(-1, 2), np.ascontiguousarray(K, np.float64),
                        np.ascontiguousarray(prior, np.float64)))
    return out


def interleave(problems):
    """The same problems round-robin over the families: neighbours of one launch belong to different families."""
    by = {}
    for p in problems:
        by.setdefault(p[0], []).append(p)
    out = []
    for row in itertools.zip_longest(*by.values()):
        out.extend(p for p in row if p is not None)
    return out


# GN: a single point at z == 0 / at the origin of the camera, one edge (an indefinite H), NaN input
def _gn_single(s):
    """s % 3 == 0: pc_z == 0 off the optical axis (u / 0); 1: the point at the camera centre (0 / 0); 2: an ordinary
    point.  The first two under an identity-rotation prior, t_z = -5 - s / 4: X_z = -t_z makes pc_z = X_z + t_z an
    exact zero (through a rotation the zero would be lost to rounding)."""
    X, uv, K, prior = _scene(1, 400 + s, rot=0)
    if s % 3 == 2:
        return X, uv, K, prior
    pc, prior = _in_camera_frame(X, prior, -5.0 - 0.25 * s)
    if s % 3 == 0:
        pc[0, 2] = 0.0
    else:
        pc[0] = 0.0
    return np.ascontiguousarray(pc - prior[4:]), uv, K, prior


GN_SINGLE_SEEDS = 18  # six of each kind


def gn_corpus():
    """The LM corpus plus the GN-only family, interleaved."""
    extra = [("gn_single", *_gn_single(s)) for s in range(GN_SINGLE_SEEDS)]
    return interleave(lm_corpus() + [(n, np.ascontiguousarray(X), np.ascontiguousarray(uv), K, p)
                                     for n, X, uv, K, p in extra])


# ------------------------------------------------------------------------------------------------
# the LDLT corpus
# ------------------------------------------------------------------------------------------------
def _jtj(rng, edges):
    """J^T J of `edges` pose edges (rank 2 per edge) and a matching -J^T e."""
    H, b = np.zeros((6, 6)), np.zeros(6)
    for _ in range(edges):
        z = rng.uniform(4, 40)
        x, y = rng.uniform(-0.6, 0.6) * z, rng.uniform(-0.25, 0.25) * z
        fx = fy = 718.856
        J = np.array([[-fx / z, 0, fx * x / z**2, fx * x * y / z**2, -fx - fx * x * x / z**2, fx * y / z],
                      [0, -fy / z, fy * y / z**2, fy + fy * y * y / z**2, -fy * x * y / z**2, -fy * x / z]])
        H += J.T @ J
        b -= J.T @ rng.normal(size=2)
    return H, b


def ldlt_corpus():
    """-> (names, H [n, 6, 6] symmetric, lam [n], b [n, 6])."""
    rng = np.random.default_rng(7)
    names, Hs, lams, bs = [], [], [], []

    def add(name, H, lam=0.0, b=None):
        H = np.array(H, np.float64)
        il = np.tril_indices(6, -1)
        H.T[il] = H[il]  # the lower triangle decides (NaN / inf placed there stay symmetric)
        names.append(name)
        Hs.append(H)
        lams.append(lam)
        bs.append(rng.normal(size=6) if b is None else np.asarray(b, np.float64))

    def spd(diag, off=0.01):
        A = rng.normal(size=(6, 6)) * off
        A = (A + A.T) * 0.5 * np.sqrt(np.abs(np.outer(diag, diag)))
        np.fill_diagonal(A, diag)
        return A

    # all 720 orders of six distinct diagonal magnitudes
    mags = np.array([1.0, 2.5, 6.0, 15.0, 40.0, 100.0])
    for k, perm in enumerate(itertools.permutations(range(6))):
        add(f"order{k}", spd(mags[list(perm)]), lam=0.0 if k % 2 else 1e-3)
    # ties of |diag|
    add("tie all equal", spd(np.full(6, 3.0)))
    add("tie all equal damped", spd(np.full(6, 3.0)), lam=0.5)
    add("tie pairs", spd([2, 2, 5, 5, 9, 9.0]))
    add("tie late", spd([1, 7, 3, 7, 2, 7.0]))
    add("tie opposite signs", spd([4, -4, 4, -4, 2, -2.0]))
    add("tie opposite signs 2", spd([-3, 3, 1, -1, 3, -3.0]))
    add("tie after damping", spd([1, 3, 1, 3, 1, 3.0]) , lam=2.0)
    # H_ii == -lambda
    for i in range(6):
        add(f"H{i}{i} == -lambda", spd([2, 3, 4, 5, 6, 7.0]) - np.diag(np.eye(6)[i] * (i + 2 + 1.5)), lam=1.5)
    add("diag == -lambda", np.diag(np.full(6, -1.5)), lam=1.5)
    add("diag == -lambda, off-diagonal", spd(np.full(6, 1.5)) - 3.0 * np.eye(6), lam=1.5)
    # -0.0
    add("-0.0 diagonal", np.diag([-0.0, 1, 2, -0.0, 3, 4.0]))
    add("-0.0 everywhere", np.full((6, 6), -0.0))
    add("-0.0 first", np.diag([-0.0, -0.0, -0.0, -0.0, -0.0, -0.0]), lam=0.0, b=np.ones(6))
    H = spd([5, 4, 3, 2, 1, 6.0]); H[3, 1] = -0.0; H[5, 0] = -0.0
    add("-0.0 off-diagonal", H)
    # NaN and inf on and off the diagonal
    for i in (0, 2, 5):
        for v, vn in ((np.nan, "NaN"), (np.inf, "inf"), (-np.inf, "-inf")):
            H = spd([5, 4, 3, 2, 1, 6.0]); H[i, i] = v
            add(f"{vn} at {i}{i}", H, lam=0.1)
    for (i, j) in ((1, 0), (4, 2), (5, 4)):
        for v, vn in ((np.nan, "NaN"), (np.inf, "inf")):
            H = spd([5, 4, 3, 2, 1, 6.0]); H[i, j] = v
            add(f"{vn} at {i}{j}", H, lam=0.1)
    add("all NaN", np.full((6, 6), np.nan))
    add("all inf", np.full((6, 6), np.inf))
    add("NaN lambda", spd([5, 4, 3, 2, 1, 6.0]), lam=np.nan)
    add("inf lambda", spd([5, 4, 3, 2, 1, 6.0]), lam=np.inf)
    add("NaN b", spd([5, 4, 3, 2, 1, 6.0]), b=[1, np.nan, 2, 3, np.inf, 4])
    # pivots at, just above and just below DBL_MIN
    for f, fn in ((1.0, "at"), (1.0 + 2**-52, "above"), (1.0 - 2**-53, "below"), (0.5, "half"), (4.0, "4x")):
        add(f"pivot {fn} DBL_MIN", np.diag([1.0, 2.0, DBL_MIN * f, 3.0, 4.0, 5.0]))
        add(f"pivot -{fn} DBL_MIN", np.diag([1.0, 2.0, -DBL_MIN * f, 3.0, 4.0, 5.0]))
        add(f"all pivots {fn} DBL_MIN", np.diag(np.full(6, DBL_MIN * f)))
        add(f"pivot {fn} DBL_MIN by damping", np.diag([1.0, 2.0, 0.0, 3.0, 4.0, 5.0]), lam=DBL_MIN * f)
    # denormal matrices
    add("denormal diagonal", np.diag(np.arange(1, 7) * 5e-324))
    add("denormal spd", spd(np.array([3, 9, 2, 7, 5, 8.0]) * 1e-310))
    add("denormal full", rng.normal(size=(6, 6)) * 1e-315)
    add("denormal and normal", spd([1e-310, 1.0, 1e-315, 2.0, 5e-324, 3.0], off=0.0))
    # rank 2 and rank 4 J^T J from one and two edges, with and without damping
    for k in range(4):
        for edges in (1, 2):
            H, b = _jtj(rng, edges)
            add(f"rank {2 * edges} JtJ {k}", H, 0.0, b)
            add(f"rank {2 * edges} JtJ {k} damped", H, 1e-5 * np.abs(np.diag(H)).max(), b)
    # exactly singular small-integer matrices (zero pivots at k > 0 without rounding)
    for k in range(8):
        r = int(rng.integers(1, 6))
        A = rng.integers(-3, 4, size=(6, r)).astype(np.float64)
        add(f"integer rank {r} #{k}", A @ A.T)
        add(f"-integer rank {r} #{k}", -(A @ A.T))
    # indefinite, negative definite and zero
    for k in range(6):
        d = rng.uniform(1, 10, 6) * rng.choice([-1, 1], 6)
        add(f"indefinite {k}", spd(d, off=0.3))
    for k in range(6):
        add(f"negative definite {k}", -spd(rng.uniform(1, 10, 6)), lam=(0.0, 0.5)[k % 2])
    add("zero", np.zeros((6, 6)))
    add("zero, b zero", np.zeros((6, 6)), b=np.zeros(6))
    add("zero damped", np.zeros((6, 6)), lam=1e-3)
    add("zero, negative damping", np.zeros((6, 6)), lam=-2.0)
    add("first pivot zero, rest not", np.diag([0.0, 0, 0, 0, 0, 0]) + np.tril(np.ones((6, 6)), -1))
    return names, np.array(Hs), np.array(lams), np.array(bs)
