"""Bundle-adjustment graphs of general structure for the BA tests (a helper like pose_scene.py, not a conftest).

scene.ba_window draws one graph shape: edges in landmark order, every landmark seen by `obs` consecutive poses in
ascending order, no duplicate edge, no pose or landmark without edges.  general_graph keeps that generator's poses,
points and perturbed start (so every point stays in front of every pose) and draws the edges as random (pose,
landmark) pairs instead, with the structure yv_ba_set_problem has to cope with as options."""
import numpy as np

from ya_vo_amd import scene

# skew, off-diagonal entries and a third row other than (0, 0, 1): the error uses all nine entries, the Jacobian
# K[0][0] and K[1][1] only (the reference's linearizeOplus)
K_SKEW = np.array([[700.0, 3.5, 600.0], [0.2, 715.0, 180.0], [1e-4, -2e-4, 1.01]])


def general_graph(n_poses, n_landmarks, n_edges, seed=0, duplicates=0, isolated_pose=None, empty_landmarks=0,
                  fixed_only=0, fixed_below=2, shuffle=True, K=scene.K_KITTI, noise_px=1.0, init_rot=0.005,
                  init_trans=0.05, init_point=0.1):
    """n_edges edges over the poses and points of scene.ba_window(n_poses, n_landmarks, seed=seed):
      duplicates       of the n_edges, this many repeat the (pose, landmark) of another edge (own noise)
      isolated_pose    a pose that gets no edge (None: every pose may)
      empty_landmarks  the last this many landmarks get no edge
      fixed_only       the first this many landmarks are seen by poses < fixed_below only
      shuffle          True: the edges in random order (a landmark's poses not ascending, the per-pose and per-pair
                       lists not monotone); False: sorted by (landmark, pose) like ba_window
    Every other landmark may still end up with no edge or a single one (H_ll rank-deficient without lambda): callers
    that rely on it check the degrees.  Measurements are scene.project of the truth plus N(0, noise_px).  Returns
    ba_window's dict (poses_true, X_true, poses0, X0, ep, el, meas)."""
    w = scene.ba_window(n_poses=n_poses, n_landmarks=n_landmarks, obs=1, noise_px=0.0, seed=seed, K=K,
                        init_rot=init_rot, init_trans=init_trans, init_point=init_point)
    T, X = w["poses_true"], w["X_true"]
    depth = np.array([scene.transform(Tp, X)[:, 2] for Tp in T])
    assert depth.min() > 1.0, "a point behind (or too close to) a pose"
    rng = np.random.default_rng(seed + 7919)
    poses = np.array([p for p in range(n_poses) if p != isolated_pose])
    pairs = []
    for l in range(n_landmarks - empty_landmarks):
        seen_by = poses[poses < fixed_below] if l < fixed_only else poses
        pairs += [(p, l) for p in seen_by]
    pairs = np.array(pairs, np.int32)
    n_distinct = n_edges - duplicates
    assert 0 < n_distinct <= len(pairs)
    edges = pairs[rng.choice(len(pairs), n_distinct, replace=False)]
    if duplicates:
        edges = np.concatenate([edges, edges[rng.integers(0, n_distinct, duplicates)]])
    if shuffle:
        edges = edges[rng.permutation(len(edges))]
    else:
        edges = edges[np.lexsort((edges[:, 0], edges[:, 1]))]
    ep = np.ascontiguousarray(edges[:, 0])
    el = np.ascontiguousarray(edges[:, 1])
    meas = np.zeros((len(ep), 2))
    for p in np.unique(ep):
        sel = ep == p
        meas[sel] = scene.project(T[p], X[el[sel]], K)
    meas += rng.normal(scale=noise_px, size=meas.shape)
    return dict(poses_true=T, X_true=X, poses0=w["poses0"], X0=w["X0"], ep=ep, el=el, meas=meas)


def case(name):
    """The named inputs shared by the oracle's arm checks (test_oracle_ba.py) and the GPU parity tests
    (test_gpu_ba_graphs.py) -> (graph, K).  The seeds are pinned: the arm checks assert what each one reaches."""
    if name == "general":  # duplicates, a pose and 5 landmarks without edges, landmarks on poses 0 / 1 only, shuffled
        return general_graph(7, 120, 520, seed=0, duplicates=20, isolated_pose=3, empty_landmarks=5,
                             fixed_only=6), scene.K_KITTI
    if name == "skew":
        return general_graph(6, 100, 450, seed=0, duplicates=10, K=K_SKEW), K_SKEW
    if name == "long":  # no fixed pose: the gauge directions of S are lambda alone, which LM shrinks to rounding level
        return general_graph(6, 100, 450, seed=138, duplicates=10, isolated_pose=3, empty_landmarks=4,
                             fixed_only=5), scene.K_KITTI
    if name == "poor":  # the same graph from a start 0.2 rad, 3 m (poses) and 5 m (points) off, 2 px noise
        return general_graph(6, 100, 450, seed=138, duplicates=10, isolated_pose=3, empty_landmarks=4, fixed_only=5,
                             noise_px=2.0, init_rot=0.2, init_trans=3.0, init_point=5.0), scene.K_KITTI
    if name == "nan":  # one measurement NaN: chi2, rho and the trial state are NaN from the start
        w, K = case("long")
        w["meas"] = w["meas"].copy()
        w["meas"][17, 1] = np.nan
        return w, K
    if name == "restart":
        return general_graph(5, 60, 260, seed=158, duplicates=30, empty_landmarks=3, fixed_only=4), scene.K_KITTI
    raise KeyError(name)


def shuffled(w, seed=0):
    """The same graph with its edges in a random order (ep, el, meas permuted together)."""
    perm = np.random.default_rng(seed).permutation(len(w["ep"]))
    out = dict(w)
    out["ep"], out["el"], out["meas"] = (np.ascontiguousarray(w[k][perm]) for k in ("ep", "el", "meas"))
    return out


def ticket_groups(grid):
    """(group size, workgroups in the last group) of a last-workgroup ticket over `grid` workgroups: consecutive
    workgroups in groups of max(16, ceil(grid / 64)) (yavo_ba.hip ba_last_block_h)."""
    gs = max(16, -(-grid // 64))
    return gs, grid - (-(-grid // gs) - 1) * gs


def pair_counts(w):
    """[P, P] co-visible pairs per pose block (p1 <= p2 used): for each landmark every ordered pair of its edges."""
    P, L = len(w["poses0"]), len(w["X0"])
    C = np.zeros((max(L, 1), P), np.int64)
    np.add.at(C, (w["el"], w["ep"]), 1)
    return np.triu(C.T @ C)


def degrees(w):
    """(edges per pose [P], edges per landmark [L], duplicated (pose, landmark) edges beyond the first)."""
    P, L = len(w["poses0"]), len(w["X0"])
    key = w["ep"].astype(np.int64) * max(L, 1) + w["el"]
    return np.bincount(w["ep"], minlength=P), np.bincount(w["el"], minlength=L), len(key) - len(np.unique(key))
