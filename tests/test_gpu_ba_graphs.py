"""GPU parity of the bundle adjustment (yv_ba, ya_vo_amd/csrc/yavo_ba*.hip) with the CPU oracle (or_ba_lm, mode 0) on
what scene.ba_window never produces: general graphs (shuffled edges, duplicates, poses and landmarks without edges,
single-edge landmarks, landmarks on fixed poses only), a K whose every entry matters, sums that wrap the tree4096 and
landmark-block leaves, ticket groups above 16 workgroups, and the LM control's stop arms on the device, in the host
loop and across resumes.  Poses, landmarks, the chi2 log and the iteration count are compared bit for bit (NaN equal
to NaN).  tests/test_oracle_ba.py checks on the CPU that every named input reaches the arm it is named for."""
import numpy as np
import pytest

import ba_graphs
import ya_vo_amd as yv
from ya_vo_amd import scene

pytestmark = pytest.mark.gpu

CONTROL = pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])

_cache = {}


def _reference(oracle, key, build, n_fixed, iters):
    """(graph, K, the oracle's poses, landmarks, iterations, chi2 log, trial log), computed once per key."""
    if key not in _cache:
        w, K = build()
        _cache[key] = (w, K) + oracle.ba_lm_trials(w["poses0"], n_fixed, w["X0"], w["ep"], w["el"], w["meas"], K,
                                                   iters)
    return _cache[key]


def _solve_and_compare(ba, ref, n_fixed, iters, on_device):
    """One solve against the reference; the resumes counter rises by one per rejected trial after which the trial
    loop goes on (device control), sum(q - 1) over the iterations run, and not at all under host control."""
    w, K, oT, oX, oit, olog, trials = ref
    ba.set_control(on_device)
    ba.set_problem(len(w["poses0"]), n_fixed, len(w["X0"]), w["ep"], w["el"], w["meas"], K)
    before = ba.resumes()
    T, X, log, it = ba.solve(w["poses0"], w["X0"], iters)
    assert it == oit
    np.testing.assert_array_equal(log, olog)
    np.testing.assert_array_equal(T, oT)
    np.testing.assert_array_equal(X, oX)
    assert ba.resumes() - before == (int((trials[:, 0] - 1).sum()) if on_device else 0)
    return T, X, log


def _run(ctx, oracle, key, build, n_fixed, iters, on_device):
    ref = _reference(oracle, key, build, n_fixed, iters)
    w = ref[0]
    ba = yv.BundleAdjuster(ctx, len(w["poses0"]), len(w["X0"]), len(w["ep"]))
    try:
        return _solve_and_compare(ba, ref, n_fixed, iters, on_device) + (ref,)
    finally:
        ba.close()


@CONTROL
@pytest.mark.parametrize("n_fixed", [0, 1, 2, 6])
def test_ba_general_graph(ctx, oracle, n_fixed, on_device):
    """The structure lists and the pair order of a shuffled graph with duplicates; a free pose without edges (S block
    lambda I: tied pivots); landmarks without edges, with one edge, on fixed poses only; six fixed poses: ns = 6."""
    _run(ctx, oracle, ("general", n_fixed), lambda: ba_graphs.case("general"), n_fixed, 10, on_device)


@CONTROL
def test_ba_skew_K(ctx, oracle, on_device):
    """K with skew, K[1][0] and a third row other than (0, 0, 1): all nine entries in the error, K[0][0] and K[1][1]
    only in the Jacobian."""
    _run(ctx, oracle, "skew", lambda: ba_graphs.case("skew"), 1, 10, on_device)


@CONTROL
@pytest.mark.parametrize("P,L,obs,n_fixed", [(3, 4300, 3, 1), (2, 4300, 2, 0), (2, 8300, 2, 0)])
def test_ba_wrapped_pose_sums(ctx, oracle, P, L, obs, n_fixed, on_device):
    """More edges per pose and pairs per block than tree4096 has leaves, shuffled. 4,300: 204 leaves hold two items
    (both must be summed; two items commute, so their order does not show). 8,300: 108 leaves hold three, which pins
    the ascending order within a leaf."""
    _run(ctx, oracle, ("wrap", P, L), lambda: (ba_graphs.shuffled(scene.ba_window(P, L, obs=obs, seed=0), 1),
                                            scene.K_KITTI), n_fixed, 4, on_device)


@CONTROL
def test_ba_wrapped_landmark_blocks(ctx, oracle, on_device):
    """66,000 landmarks: 258 block totals folded into 256 leaves, so leaves 0 and 1 hold two (two totals commute: the
    order of the fold is pinned by test_ba_wide_chi2_grid, up to five per leaf). The middle pose has 66,000 edges and
    its diagonal block 66,000 pairs: 16 or 17 items per tree4096 leaf, in ascending order."""
    _run(ctx, oracle, "blocks", lambda: (scene.ba_window(3, 66000, obs=2, seed=0), scene.K_KITTI), 1, 3, on_device)


@CONTROL
def test_ba_wide_reduce_grid(ctx, oracle, on_device):
    """65 free poses: the reduce kernel's 1,042 workgroups arrive in ticket groups of 17, the last one of 5."""
    _run(ctx, oracle, "wide", lambda: (scene.ba_window(66, 400, obs=6, seed=0), scene.K_KITTI), 1, 4, on_device)


def test_ba_wide_chi2_grid(ctx, oracle):
    """270,000 landmarks: the chi2 and step kernels' 1,055 workgroups arrive in ticket groups of 17, the last one of
    1, and their block totals fold four or five to a leaf, in ascending block order (device control only; most of
    the time is the generator's and the structure build's on the host)."""
    _run(ctx, oracle, "wide_chi2", lambda: (scene.ba_window(70, 270000, obs=2, seed=0), scene.K_KITTI), 1, 2, True)


@CONTROL
def test_ba_long_run_then_reuse(ctx, oracle, on_device):
    """max_iters = 80 grows the chi2 log past its 65 entries; the run has trials whose LDLT is not positive (chi2 =
    DBL_MAX), rejected trials and a stop on rho == 0 in a resumed trial loop.  A shorter solve of another graph (and
    K) on the same workspace follows."""
    ref = _reference(oracle, "long", lambda: ba_graphs.case("long"), 0, 80)
    ref2 = _reference(oracle, "skew5", lambda: ba_graphs.case("skew"), 2, 5)
    ba = yv.BundleAdjuster(ctx, 6, 100, 450)
    try:
        _, _, log = _solve_and_compare(ba, ref, 0, 80, on_device)
        assert len(log) < 65 < 80 + 1
        _solve_and_compare(ba, ref2, 2, 5, on_device)
    finally:
        ba.close()


@CONTROL
@pytest.mark.parametrize("n_fixed", [0, 2])
def test_ba_poor_start(ctx, oracle, n_fixed, on_device):
    """A start far off (0.2 rad, 3 m, 5 m; 2 px noise): iterations that take two to four trials, 80 iterations."""
    _run(ctx, oracle, ("poor", n_fixed), lambda: ba_graphs.case("poor"), n_fixed, 80, on_device)


@CONTROL
def test_ba_restart_at_the_minimum(ctx, oracle, on_device):
    """Both sides start from the estimate a 64-iteration oracle run ends in: ten rejected trials in one iteration
    (nine resumes), the stop on q == 10, the estimate unchanged."""
    def build():
        w, K = ba_graphs.case("restart")
        T, X, _, _ = oracle.ba_lm(w["poses0"], 1, w["X0"], w["ep"], w["el"], w["meas"], K, 64)
        return dict(w, poses0=T, X0=X), K

    T, X, log, ref = _run(ctx, oracle, "restart", build, 1, 40, on_device)
    assert ref[-1][-1, 0] == 10
    np.testing.assert_array_equal(T, ref[0]["poses0"])
    np.testing.assert_array_equal(X, ref[0]["X0"])


@CONTROL
def test_ba_nan_measurement(ctx, oracle, on_device):
    """One NaN measurement: rho is NaN in every trial (rejected; the trial loop ends after one trial and the run goes
    on), lambda doubles, quadruples, ... until it is not finite at iteration 45; the estimate returned is the start."""
    T, X, log, ref = _run(ctx, oracle, "nan", lambda: ba_graphs.case("nan"), 1, 80, on_device)
    assert len(log) == 46 and np.all(np.isnan(log))
    np.testing.assert_array_equal(T, ref[0]["poses0"])
    np.testing.assert_array_equal(X, ref[0]["X0"])


@CONTROL
def test_ba_zero_iterations(ctx, oracle, on_device):
    T, X, log, ref = _run(ctx, oracle, "zero", lambda: ba_graphs.case("general"), 1, 0, on_device)
    assert len(log) == 1 and log[0] > 0
    np.testing.assert_array_equal(T, ref[0]["poses0"])
    np.testing.assert_array_equal(X, ref[0]["X0"])


# yv_ba_debug_read's `which` of the buffers the ABI still serves, in the order the kernels produce them
_STAGES = [(0, "err"), (1, "J_pose"), (2, "J_point"), (7, "H_ll"), (8, "b_l"), (5, "H_pp"), (6, "b_p"), (10, "S"),
           (11, "b_schur"), (12, "x_p"), (13, "x_l"), (14, "poses"), (15, "X")]


@CONTROL
@pytest.mark.parametrize("n_fixed", [0, 2])
def test_ba_stages_match_oracle(ctx, oracle, n_fixed, on_device):
    """One iteration whose first trial is accepted: every buffer the workspace still holds equals the oracle's dump of
    iteration 0, bit for bit; the first stage that differs is named. H_pl, W and Dinv (3, 4, 9) are not stored."""
    w, K = ba_graphs.case("general")
    ref = _reference(oracle, ("stage", n_fixed), lambda: (w, K), n_fixed, 1)
    olog, trials = ref[5], ref[6]
    assert trials[0, 0] == 1 and olog[1] < olog[0]  # one trial, accepted
    dump = oracle.ba_dump(w["poses0"], n_fixed, w["X0"], w["ep"], w["el"], w["meas"], K, dump_iter=0)
    P = len(w["poses0"])
    ba = yv.BundleAdjuster(ctx, P, len(w["X0"]), len(w["ep"]))
    try:
        _solve_and_compare(ba, ref, n_fixed, 1, on_device)
        for which, name in _STAGES:
            want = dump[name]
            got = ba.debug_read(which, len(want))
            if name in ("H_pp", "b_p"):  # the rows of fixed poses are never written
                per = len(want) // P
                want, got = want[per * n_fixed:], got[per * n_fixed:]
            bad = np.flatnonzero(~((want == got) | (np.isnan(want) & np.isnan(got))))
            assert len(bad) == 0, (f"first differing stage: {name} (which = {which}), {len(bad)} of {len(want)} "
                                   f"entries, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}")
        for which in (3, 4, 9):
            with pytest.raises(yv.YavoError) as err:
                ba.debug_read(which, 1)
            assert err.value.status == yv.YV_ERR_INVALID
    finally:
        ba.close()
