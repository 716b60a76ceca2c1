"""CPU oracle for the sliding-window bundle adjustment (oracle/yavo_oracle_ba.c; BASELINE.json config 5, SURVEY.md
8d-8e).  g2o is absent and the reference holds no multi-pose BA fixture (its Optimizer::partialBA is a pose-only
stub), so parity with a g2o build is unpinned; these tests pin the restatement by its algebra: the LDLT against
numpy, exact recovery of a noise-free window, chi2 monotonicity of LM, the gauge (fixed poses untouched) and the
degenerate graphs."""
import numpy as np
import pytest

import ba_graphs
from oracle_bind import Oracle
from ya_vo_amd import scene


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _spd(n, seed, cond=1e3):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    d = np.geomspace(1.0, cond, n)
    return (Q * d) @ Q.T


@pytest.mark.parametrize("n,seed", [(1, 0), (6, 1), (30, 2), (114, 3)])
def test_ldlt_solves_spd(oracle, n, seed):
    H = _spd(n, seed)
    b = np.random.default_rng(seed + 100).normal(size=n)
    x, pos = oracle.ldlt_solve(H, b)
    assert pos
    np.testing.assert_allclose(H @ x, b, rtol=0, atol=1e-9 * np.abs(b).max() * 1e3)


def test_ldlt_pivots_and_flags_indefinite(oracle):
    H = np.diag([1.0, -4.0, 2.0, 9.0])
    H[0, 3] = H[3, 0] = 0.5
    b = np.array([1.0, 2.0, 3.0, 4.0])
    x, pos = oracle.ldlt_solve(H, b)
    assert not pos
    np.testing.assert_allclose(H @ x, b, atol=1e-12)


def test_ldlt_zero_matrix(oracle):
    x, pos = oracle.ldlt_solve(np.zeros((3, 3)), np.ones(3))
    assert pos and not x.any()


def _run(oracle, w, n_fixed, iters=10):
    return oracle.ba_lm(w["poses0"], n_fixed, w["X0"], w["ep"], w["el"], w["meas"], scene.K_KITTI, iters)


def test_ba_noise_free_recovers_truth(oracle):
    # two fixed poses fix the gauge, scale included: the truth is the unique minimum
    w = scene.ba_window(n_poses=6, n_landmarks=300, obs=4, noise_px=0.0, seed=1)
    w["poses0"][1] = w["poses_true"][1]
    T, X, it, log = _run(oracle, w, 2, 20)
    assert log[-1] < 1e-12 * log[0]
    np.testing.assert_allclose(T, w["poses_true"], atol=1e-7)
    np.testing.assert_allclose(X, w["X_true"], rtol=2e-5, atol=1e-6)


def test_ba_noisy_chi2_decreases(oracle):
    w = scene.ba_window(n_poses=10, n_landmarks=1000, obs=5, noise_px=1.0, seed=2)
    T, X, it, log = _run(oracle, w, 1, 10)
    assert it >= 1 and np.all(np.diff(log) <= 0)
    E = len(w["ep"])
    dof = 2 * E - 6 * 9 - 3 * 1000
    assert 0.8 < log[-1] / dof < 1.2  # sigma = 1 px: chi2 ~ the degrees of freedom
    np.testing.assert_array_equal(T[0], w["poses0"][0])


def test_ba_fixed_poses_untouched_and_landmarks_only(oracle):
    w = scene.ba_window(n_poses=5, n_landmarks=200, obs=3, noise_px=0.5, seed=3)
    w["poses0"] = w["poses_true"].copy()
    T, X, it, log = _run(oracle, w, 5, 10)
    np.testing.assert_array_equal(T, w["poses_true"])
    assert log[-1] < 0.05 * log[0]


def test_ba_all_free(oracle):
    w = scene.ba_window(n_poses=4, n_landmarks=150, obs=4, noise_px=0.3, seed=4)
    T, X, it, log = _run(oracle, w, 0, 8)
    assert np.all(np.diff(log) <= 0) and log[-1] < log[0]


def test_ba_empty_graph(oracle):
    poses = scene.ba_window(n_poses=3, n_landmarks=1, obs=1, seed=5)["poses0"]
    T, X, it, log = oracle.ba_lm(poses, 1, np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32),
                                 np.zeros((0, 2)), scene.K_KITTI, 5)
    np.testing.assert_array_equal(T, poses)
    assert it == 1 and log[0] == 0.0


# ---- g2o's own summation orders (or_ba_lm mode 1): the CPU reference the device trajectory is measured against ----

def _run_mode(oracle, w, n_fixed, iters, mode):
    return oracle.ba_lm(w["poses0"], n_fixed, w["X0"], w["ep"], w["el"], w["meas"], scene.K_KITTI, iters, mode=mode)


def test_ba_g2o_order_noise_free_recovers_truth(oracle):
    w = scene.ba_window(n_poses=6, n_landmarks=300, obs=4, noise_px=0.0, seed=1)
    w["poses0"][1] = w["poses_true"][1]
    T, X, it, log = _run_mode(oracle, w, 2, 20, 1)
    assert log[-1] < 1e-12 * log[0]
    np.testing.assert_allclose(T, w["poses_true"], atol=1e-7)
    np.testing.assert_allclose(X, w["X_true"], rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("n_fixed", [0, 1, 2])
def test_ba_g2o_order_is_a_different_order_with_the_same_solution(oracle, n_fixed):
    """The two orders are different arithmetic (some bit of the result differs) converging to the same minimum: poses
    within 1e-9, chi2 logs within 1e-9 relative, chi2 non-increasing in both."""
    w = scene.ba_window(n_poses=8, n_landmarks=800, obs=4, noise_px=1.0, seed=7)
    T0, X0, it0, log0 = _run_mode(oracle, w, n_fixed, 10, 0)
    T1, X1, it1, log1 = _run_mode(oracle, w, n_fixed, 10, 1)
    assert it0 == it1
    assert np.all(np.diff(log1) <= 0)
    assert not (np.array_equal(T0, T1) and np.array_equal(X0, X1) and np.array_equal(log0, log1))
    np.testing.assert_allclose(T1, T0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(log1, log0, rtol=1e-9)
    np.testing.assert_array_equal(T1[:n_fixed], w["poses0"][:n_fixed])


def _dense_lm_step(oracle, w, n_fixed, K=scene.K_KITTI):
    """One damped step of the full (unreduced) normal equations in numpy -- an order-free restatement of what an
    accepted first LM trial does: H = J^T J over all free variables, lambda = 1e-5 max diag, (H + lambda I) x =
    -J^T e, T_p <- exp(x_p) T_p, X_l <- X_l + x_l.  The error projects with all of K; the Jacobian uses fx = K[0][0]
    and fy = K[1][1] only, as the reference's linearizeOplus does."""
    P, L = len(w["poses0"]), len(w["X0"])
    npz = P - n_fixed
    n = 6 * npz + 3 * L
    H = np.zeros((n, n))
    b = np.zeros(n)
    for e, (p, l) in enumerate(zip(w["ep"], w["el"])):
        T, X = w["poses0"][p], w["X0"][l]
        pc = oracle.se3_act(T, X)
        R = oracle.quat_to_R(T[:4])
        uvw = np.asarray(K) @ pc
        err = w["meas"][e] - uvw[:2] / uvw[2]
        fx, fy = K[0][0], K[1][1]
        x, y, z = pc
        Jp = np.array([[-fx / z, 0, fx * x / z ** 2, fx * x * y / z ** 2, -fx - fx * x * x / z ** 2, fx * y / z],
                       [0, -fy / z, fy * y / z ** 2, fy + fy * y * y / z ** 2, -fy * x * y / z ** 2, -fy * x / z]])
        Jl = Jp[:, :3] @ R
        J = np.zeros((2, n))
        if p >= n_fixed:
            J[:, 6 * (p - n_fixed):6 * (p - n_fixed) + 6] = Jp
        J[:, 6 * npz + 3 * l:6 * npz + 3 * l + 3] = Jl
        H += J.T @ J
        b -= J.T @ err
    lam = 1e-5 * np.max(np.abs(np.diag(H)))
    x = np.linalg.solve(H + lam * np.eye(n), b)
    T = w["poses0"].copy()
    for p in range(n_fixed, P):
        T[p] = oracle.se3_mul(oracle.se3_exp(x[6 * (p - n_fixed):6 * (p - n_fixed) + 6]), T[p])
    return T, w["X0"] + x[6 * npz:].reshape(L, 3)


@pytest.mark.parametrize("mode", [0, 1])
def test_ba_first_step_equals_dense_normal_equations(oracle, mode):
    """The Schur-complement step (both orders) equals the dense solve of the unreduced system (numpy, its own
    order) when the first trial is accepted: an independent check of H_pp / H_pl / H_ll, the Schur complement,
    b_schur and the back-substitution."""
    w = scene.ba_window(n_poses=4, n_landmarks=60, obs=3, noise_px=0.5, seed=11)
    T_ref, X_ref = _dense_lm_step(oracle, w, 1)
    T, X, it, log = _run_mode(oracle, w, 1, 1, mode)
    assert log[1] < log[0]  # accepted
    np.testing.assert_allclose(T, T_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(X, X_ref, rtol=0, atol=1e-9)


# ---- general graphs (ba_graphs.py): the conditions tests/test_gpu_ba_graphs.py rests on, checked on the CPU ----

def _trials(oracle, name, n_fixed, iters, start=None):
    w, K = ba_graphs.case(name)
    T0, X0 = start if start is not None else (w["poses0"], w["X0"])
    return (w,) + oracle.ba_lm_trials(T0, n_fixed, X0, w["ep"], w["el"], w["meas"], K, iters)


@pytest.mark.parametrize("n_fixed", [0, 1, 2, 6])
def test_arm_general_graph_structure(oracle, n_fixed):
    """The general graph holds what ba_window never does: a shuffled edge order (per-pose and per-landmark lists not
    contiguous, a landmark's poses not ascending), duplicate edges, a pose and landmarks without edges, landmarks
    with one edge, landmarks seen by fixed poses only, and with six fixed poses a 6 x 6 reduced system."""
    w, T, X, it, log, trials = _trials(oracle, "general", n_fixed, 10)
    ep, el = w["ep"], w["el"]
    deg_p, deg_l, dups = ba_graphs.degrees(w)
    assert len(ep) == 520 and dups == 20
    assert np.any(np.diff(el) < 0) and np.any(np.diff(ep) < 0)
    assert any(np.any(np.diff(ep[el == l]) < 0) for l in range(120))  # some landmark's poses not ascending
    assert np.flatnonzero(deg_p == 0).tolist() == [3]
    assert np.all(deg_l[-5:] == 0) and np.sum(deg_l == 1) >= 3
    assert ba_graphs.pair_counts(w).diagonal().sum() == 520 + 2 * 20  # a duplicate adds (a, b) and (b, a)
    # the pose without edges is free for n_fixed <= 3 (its S block is lambda I); with six fixed poses the one free
    # pose has edges and the reduced system is 6 x 6
    assert deg_p[6] > 0
    if n_fixed >= 2:
        seen_by_fixed_only = [l for l in range(120) if deg_l[l] and np.all(ep[el == l] < n_fixed)]
        assert len(seen_by_fixed_only) >= 5
    assert it == 10 and np.all(trials[:, 0] == 1) and log[1] < log[0]  # every first trial accepted (the stage check)
    np.testing.assert_array_equal(T[:n_fixed], w["poses0"][:n_fixed])


def test_arm_skew_K_tells_error_from_jacobian():
    """Every entry of K that the Jacobian ignores is set: skew, K[1][0], a third row other than (0, 0, 1)."""
    K = ba_graphs.K_SKEW
    assert K[0][1] != 0 and K[1][0] != 0 and K[2][0] != 0 and K[2][1] != 0 and K[2][2] != 1
    w, _ = ba_graphs.case("skew")
    u_full = scene.project(w["poses_true"][1], w["X_true"][:5], K)
    K_diag = np.array([[K[0][0], 0, K[0][2]], [0, K[1][1], K[1][2]], [0, 0, 1.0]])
    assert np.abs(u_full - scene.project(w["poses_true"][1], w["X_true"][:5], K_diag)).min() > 0.1  # pixels


@pytest.mark.parametrize("P,L,obs,most", [(3, 4300, 3, 2), (2, 4300, 2, 2), (2, 8300, 2, 3)])
def test_arm_wrapped_pose_sums(P, L, obs, most):
    """More edges per pose and pairs per block than the tree4096 sums have leaves: L - 4096 leaves hold two items
    at 4,300 (a + b = b + a: the wrap shows, the order within a leaf does not), L - 8192 hold three at 8,300 (the
    order shows)."""
    w = ba_graphs.shuffled(scene.ba_window(P, L, obs=obs, seed=0), 1)
    assert np.all(ba_graphs.degrees(w)[0] == L)
    pairs = ba_graphs.pair_counts(w)[np.triu_indices(P)]
    assert np.all(pairs == L)  # every landmark is seen by every pose once
    assert -(-L // 4096) == most and L - 4096 * (most - 1) in (204, 108)
    assert np.any(np.diff(w["el"]) < 0)


def test_arm_grids_and_blocks():
    """The shapes' launch geometry: block totals wrap the 256 leaves; ticket groups above 16 with a ragged last one."""
    # wrapped landmark blocks: leaves 0 and 1 hold two block totals; its middle pose sees every landmark, so its
    # tree4096 leaves hold 16 or 17 items (the within-leaf order shows)
    assert -(-66000 // 256) == 258 and 66000 // 4096 == 16
    reduce_grid = 16 * (66 - 1) + -(-400 // 256)  # wide grids: ba_window(66, 400), one fixed pose
    assert reduce_grid == 1042 and ba_graphs.ticket_groups(reduce_grid) == (17, 5)
    chi2_grid = -(-270000 // 256)  # wide chi2 grid: ba_window(70, 270000); four or five block totals per leaf, so
    assert chi2_grid == 1055 and ba_graphs.ticket_groups(chi2_grid) == (17, 1)  # the order of the fold shows
    assert chi2_grid // 256 == 4
    assert ba_graphs.ticket_groups(680) == (16, 8)  # the largest grid of test_gpu_ba.py: group size 16


def test_arm_long_run(oracle):
    """80 iterations allowed (a chi2 log past the 65 preallocated entries): LM shrinks lambda until the reduced
    system, whose gauge directions hold lambda alone, stops being positive; those trials and others are rejected, and
    the run ends on rho == 0 in a trial after the first."""
    w, T, X, it, log, trials = _trials(oracle, "long", 0, 80)
    assert 80 + 1 > 65
    assert trials[:, 1].sum() >= 2            # LDLT not positive
    assert np.sum(trials[:, 0] > 1) >= 4      # iterations with rejected trials
    assert trials[-1, 3] == 2 and trials[-1, 0] >= 2 and it < 80  # rho == 0 after a rejected trial
    assert np.all(trials[:-1, 3] == 0)


@pytest.mark.parametrize("n_fixed", [0, 2])
def test_arm_poor_start(oracle, n_fixed):
    w, T, X, it, log, trials = _trials(oracle, "poor", n_fixed, 80)
    """A start 0.2 rad, 3 m and 5 m off: chi2 falls by more than a thousand, through iterations that reject trials."""
    assert log[0] > 1e3 * log[-1]
    assert np.sum(trials[:, 0] >= 2) >= 3 and trials[:, 0].max() in (2, 3, 4)  # several iterations, a few trials each


def test_arm_restart_at_the_minimum(oracle):
    """From the estimate a 64-iteration run ends in, an iteration rejects ten trials: the stop on q == 10, the
    estimate unchanged."""
    w, T, X, it, log, trials = _trials(oracle, "restart", 1, 64)
    _, T2, X2, it2, log2, trials2 = _trials(oracle, "restart", 1, 40, start=(T, X))
    assert it2 <= 3 and trials2[-1, 0] == 10 and trials2[-1, 3] & 1
    np.testing.assert_array_equal(T2, T)
    np.testing.assert_array_equal(X2, X)


def test_arm_nan_measurement(oracle):
    """rho is NaN in every trial: rejected, the trial loop left after one trial, lambda x2, x4, ... until it is not
    finite, which stops the run at iteration 45; the estimate is the start."""
    w, T, X, it, log, trials = _trials(oracle, "nan", 1, 80)
    assert it == 45 and np.all(trials[:, 0] == 1) and np.all(trials[:, 2] == 1)
    assert np.all(trials[:-1, 3] == 0) and trials[-1, 3] == 4
    assert np.all(np.isnan(log))
    np.testing.assert_array_equal(T, w["poses0"])
    np.testing.assert_array_equal(X, w["X0"])


def test_arm_zero_iterations(oracle):
    w, T, X, it, log, trials = _trials(oracle, "general", 1, 0)
    assert it == 0 and len(log) == 1 and log[0] > 0 and len(trials) == 0
    np.testing.assert_array_equal(T, w["poses0"])
    np.testing.assert_array_equal(X, w["X0"])


def test_trial_log_and_dump_leave_the_solve_alone(oracle):
    """The diagnostics are counters and copies: the same bits with and without them."""
    w, K = ba_graphs.case("long")
    args = (w["poses0"], 0, w["X0"], w["ep"], w["el"], w["meas"], K)
    T, X, it, log = oracle.ba_lm(*args, 40)
    T2, X2, it2, log2, _ = oracle.ba_lm_trials(*args, 40)
    assert it == it2
    for a, b in ((T, T2), (X, X2), (log, log2)):
        np.testing.assert_array_equal(a, b)
    dump = oracle.ba_dump(*args, dump_iter=0)
    T1, X1, _, _ = oracle.ba_lm(*args, 1)
    np.testing.assert_array_equal(dump["poses"].reshape(-1, 7), T1)  # the first trial was accepted
    np.testing.assert_array_equal(dump["X"].reshape(-1, 3), X1)


# Bounds: ten times the differences measured on this graph (max |difference|; the chi2 log relative). Single-edge
# landmarks are invertible through lambda alone, so the agreement is seed-dependent: the factor of ten covers that.
#   one step, mode 0 against dense: poses 2.82e-15, landmarks 7.11e-15 (mode 1 against dense: 2.04e-15, 7.11e-15)
#   ten iterations, mode 0 against mode 1: poses 8.88e-15, landmarks 1.57e-12, chi2 log 8.33e-15 relative
_STEP_T, _STEP_X = 2.82e-14, 7.11e-14
_TEN_T, _TEN_X, _TEN_LOG = 8.88e-14, 1.57e-11, 8.33e-14


def _algebra_graph():
    return ba_graphs.general_graph(7, 120, 520, seed=0, duplicates=20, isolated_pose=3, empty_landmarks=5,
                                   fixed_only=6, K=ba_graphs.K_SKEW), ba_graphs.K_SKEW


@pytest.mark.parametrize("mode", [0, 1])
def test_ba_general_graph_first_step_equals_dense_normal_equations(oracle, mode):
    """The dense check on the general graph (duplicates, a pose and landmarks without edges, single-edge landmarks)
    with a K whose every entry matters to the error: full K in the projection, fx / fy only in the Jacobian."""
    w, K = _algebra_graph()
    assert np.sum(ba_graphs.degrees(w)[1] == 1) >= 3
    T_ref, X_ref = _dense_lm_step(oracle, w, 1, K)
    T, X, it, log = oracle.ba_lm(w["poses0"], 1, w["X0"], w["ep"], w["el"], w["meas"], K, 1, mode=mode)
    assert log[1] < log[0]  # accepted
    print(f"mode {mode} vs dense: poses {np.abs(T - T_ref).max():.3g} landmarks {np.abs(X - X_ref).max():.3g}")
    np.testing.assert_allclose(T, T_ref, rtol=0, atol=_STEP_T)
    np.testing.assert_allclose(X, X_ref, rtol=0, atol=_STEP_X)


def test_ba_general_graph_both_orders_reach_the_same_minimum(oracle):
    w, K = _algebra_graph()
    args = (w["poses0"], 1, w["X0"], w["ep"], w["el"], w["meas"], K, 10)
    T0, X0, it0, log0 = oracle.ba_lm(*args, mode=0)
    T1, X1, it1, log1 = oracle.ba_lm(*args, mode=1)
    assert it0 == it1 == 10 and np.all(np.diff(log0) <= 0) and np.all(np.diff(log1) <= 0)
    print(f"mode 0 vs 1: poses {np.abs(T1 - T0).max():.3g} landmarks {np.abs(X1 - X0).max():.3g} "
          f"chi2 {np.abs(log1 / log0 - 1).max():.3g}")
    np.testing.assert_allclose(T1, T0, rtol=0, atol=_TEN_T)
    np.testing.assert_allclose(X1, X0, rtol=0, atol=_TEN_X)
    np.testing.assert_allclose(log1, log0, rtol=_TEN_LOG)
