"""CPU tests of the oracle's cv::calcOpticalFlowPyrLK restatement.  OpenCV is not in
this image and the reference holds no LK fixtures, so parity to the reference binary is unpinned: pyrDown and
Scharr are pinned by independent numpy restatements, LK by recovering known synthetic motion and, one Newton step
at a time, by the float64 statement of tests/lk_reference.py."""
import numpy as np
import pytest

import lk_cases
import lk_reference as ref
from ya_vo_amd.synth import synth_frame


def _reflect(p, n):
    if n == 1:  # cv::borderInterpolate(REFLECT_101) on a length-1 axis
        return np.zeros_like(p)
    p = np.abs(p)
    return np.where(p >= n, 2 * n - p - 2, p)


def _np_pyr_down(img):
    H, W = img.shape
    w = np.array([1, 4, 6, 4, 1], np.int64)
    ys = np.arange((H + 1) // 2)
    xs = np.arange((W + 1) // 2)
    out = np.zeros((len(ys), len(xs)), np.int64)
    src = img.astype(np.int64)
    for i in range(5):
        rows = src[_reflect(2 * ys + i - 2, H)]
        for j in range(5):
            out += w[i] * w[j] * rows[:, _reflect(2 * xs + j - 2, W)]
    return ((out + 128) >> 8).astype(np.uint8)


def _np_scharr(img):
    H, W = img.shape
    s = img.astype(np.int64)
    up = s[_reflect(np.arange(H) - 1, H)]
    dn = s[_reflect(np.arange(H) + 1, H)]
    t0 = (up + dn) * 3 + s * 10
    t1 = dn - up
    xl, xr = _reflect(np.arange(W) - 1, W), _reflect(np.arange(W) + 1, W)
    dx = t0[:, xr] - t0[:, xl]
    dy = (t1[:, xr] + t1[:, xl]) * 3 + t1 * 10
    return np.stack([dx, dy], -1).astype(np.int16)


@pytest.mark.parametrize("shape", [(376, 1241), (47, 156), (13, 12), (1, 5)])
def test_pyr_down_matches_numpy(oracle, shape):
    img = synth_frame(3, 0, 0, max(shape[0], 1), shape[1]) if shape[0] > 1 else \
        np.random.default_rng(0).integers(0, 256, shape).astype(np.uint8)
    img = img[:shape[0], :shape[1]]
    np.testing.assert_array_equal(oracle.pyr_down(img), _np_pyr_down(img))


@pytest.mark.parametrize("shape", [(376, 1241), (20, 33)])
def test_scharr_matches_numpy(oracle, shape):
    img = synth_frame(4, 0, 0, shape[0], shape[1])
    np.testing.assert_array_equal(oracle.scharr(img), _np_scharr(img))


def test_lk_recovers_motion(oracle):
    """Frame k+1 is frame k shifted by (-1 row, -3 cols): LK from k to k+1 moves every tracked point by
    (dx, dy) = (-3, -1), sub-pixel accurate; both sum orders agree to float rounding."""
    prev, nxt = synth_frame(11, 0, 0), synth_frame(11, 1, 3)
    rng = np.random.default_rng(0)
    pts = np.stack([rng.integers(20, 1220, 400), rng.integers(20, 356, 400)], 1).astype(np.float32)
    p0, st0, e0, lv = oracle.lk(prev, nxt, pts, sum_mode=0)
    assert lv == 3
    assert st0.mean() > 0.95
    d = p0[st0] - pts[st0]
    np.testing.assert_allclose(np.median(d, 0), [-3.0, -1.0], atol=0.02)
    assert np.mean(np.abs(d - [-3.0, -1.0]).max(1) < 0.1) > 0.9
    p1, st1, e1, _ = oracle.lk(prev, nxt, pts, sum_mode=1)
    np.testing.assert_array_equal(st0, st1)
    np.testing.assert_allclose(p1, p0, atol=1e-3)
    # points pushed off the image lose their status; out-of-range starts are rejected at level 0
    far = np.array([[-30.0, 10.0], [1300.0, 100.0]], np.float32)
    _, stf, ef, _ = oracle.lk(prev, nxt, far)
    assert not stf.any() and np.all(ef == 0)


# ---- the traced entry, the defined float -> int, and one Newton step against a float64 statement ----

# Largest |step32 - step64| (px, either coordinate) over the one-step fixture below in OpenCV's scalar sum order
# (sum_mode 0), measured: 1.061e-5 (win 16; 7.2e-6, 3.8e-6, 6.6e-6, 6.8e-6 at win 3, 4, 11, 22).  It has no closed
# form (it scales with 1 / D), so it is measured once on the reference order and both orders are then held to 4 x it:
# another order of the same float32 terms errs by the same order of magnitude.
LK_STEP_ERR = 1.1e-5
LK_STEP_TOL = 4 * LK_STEP_ERR

_step_cache = {}


def _step_fixture(oracle, win):
    """Per window, computed once: the points, the float64 statement's (result, exit, status, margin) per point and
    the oracle's traced results in both sum orders."""
    if win not in _step_cache:
        prev, nxt = lk_cases.step_pair()
        pts = lk_cases.step_points(win)
        d = ref.scharr(prev)
        rows = []
        for p in pts:
            r = ref.newton_step(prev, nxt, p, win, d)
            rows.append((r,) + ref.decide(r, p, prev.shape, win, 1e-3, 0.01))
        orc = {sm: oracle.lk(prev, nxt, pts, win=win, max_level=0, max_count=1, sum_mode=sm, trace=True)
               for sm in (0, 1)}
        _step_cache[win] = (pts, rows, orc)
    return _step_cache[win]


def test_reference_reflect101_is_the_repeated_reflection():
    for n in (1, 2, 3, 5, 12):
        for p in range(-4 * n - 3, 5 * n + 3):
            q = p
            while n > 1 and (q < 0 or q >= n):
                q = -q if q < 0 else 2 * n - 2 - q
            assert ref.reflect101(p, n) == (q if n > 1 else 0)


def test_reference_scharr_matches_oracle(oracle):
    img = lk_cases.step_pair()[0]
    dx, dy = ref.scharr(img)
    np.testing.assert_array_equal(np.stack([dx, dy], -1), oracle.scharr(img))


def test_lk_trace_leaves_the_results_alone(oracle):
    prev, nxt = lk_cases.env_pair()
    pts = lk_cases.env_points(1)
    for sm in (0, 1):
        plain = oracle.lk(prev, nxt, pts, sum_mode=sm)
        traced = oracle.lk(prev, nxt, pts, sum_mode=sm, trace=True)
        for a, b in zip(plain, traced[:4]):
            np.testing.assert_array_equal(a, b)
        ex, steps = traced[4]["exit"], traced[4]["steps"]
        lv = traced[3]
        assert lv == 3 and np.all(ex[:, lv + 1:] == oracle.LK_NOT_RUN) and np.all(ex[:, :lv + 1] != oracle.LK_NOT_RUN)
        assert np.all(steps[ex < oracle.LK_LEFT_IMAGE] == 0) and steps.max() <= 30
        # status is 1 exactly after a level-0 exit that ends the iteration inside the image with an error window
        ok = np.isin(ex[:, 0], [oracle.LK_EPS, oracle.LK_OSCILLATION, oracle.LK_MAX_COUNT])
        np.testing.assert_array_equal(traced[1], ok)


def test_lk_non_finite_and_huge_points_are_rejected(oracle):
    """floor of a NaN, an infinity or a value past 2^31 is INT_MIN (cvFloor on x86): the window check rejects the point
    at every level, status 0, err 0, next = the input (scaled down and up again: unchanged, NaN stays NaN)."""
    prev, nxt = lk_cases.env_pair()
    bad = [np.nan, np.inf, -np.inf, 3e9, -3e9, 1e30, -1e30]
    pts = np.array([[b, 40.0] for b in bad] + [[50.0, b] for b in bad] + [[b, b] for b in bad] + [[60.0, 40.0]],
                   np.float32)
    for sm in (0, 1):
        nx, st, err, lv, tr = oracle.lk(prev, nxt, pts, sum_mode=sm, trace=True)
        assert not st[:-1].any() and np.all(err[:-1] == 0) and st[-1]
        assert np.all(tr["exit"][:-1, :lv + 1] == oracle.LK_WINDOW_OUTSIDE)
        np.testing.assert_array_equal(nx[:-1], pts[:-1])


@pytest.mark.parametrize("sum_mode", [0, 1])
@pytest.mark.parametrize("win", lk_cases.STEP_WINDOWS)
def test_lk_one_step_matches_float64(oracle, win, sum_mode):
    """max_level 0, max_count 1: the oracle's next - prev is one Newton step.  Its window integers are exact, so the
    float32 step differs from the float64 statement's only by the rounding of the sums, the 2x2 solve and the final
    prev + step: within LK_STEP_TOL = 4 x the error measured in OpenCV's order, in both sum orders."""
    pts, rows, orc = _step_fixture(oracle, win)
    nx, st, err, lv, tr = orc[sum_mode]
    assert lv == 0
    worst, n = 0.0, 0
    for i, (r, code, status, margin) in enumerate(rows):
        if code >= ref.EPS and tr["exit"][i, 0] >= oracle.LK_EPS:  # both took the step
            d = np.abs(nx[i].astype(np.float64) - pts[i].astype(np.float64) - np.array(r["step"])).max()
            worst, n = max(worst, d), n + 1
    print(f"win {win} sum_mode {sum_mode}: {n} steps, worst |step32 - step64| = {worst:.3e}")
    assert n >= 150
    assert worst <= LK_STEP_TOL


@pytest.mark.parametrize("win", lk_cases.STEP_WINDOWS)
def test_lk_one_step_decisions_match_float64(oracle, win):
    """Status and the traced exit equal the float64 statement's own decision at every point whose deciding numbers
    (minEig against the threshold; D against FLT_EPSILON once minEig passes; the error window's corner against the
    range check; |step| against eps) stand farther than LK_STEP_ERR from their thresholds.  At most 2 % of the points
    may be that close, and the fixture must reach both rejections and the step."""
    pts, rows, orc = _step_fixture(oracle, win)
    aside = [i for i, row in enumerate(rows) if row[3] <= LK_STEP_ERR]
    print(f"win {win}: {len(aside)} of {len(pts)} points set aside")
    assert len(aside) <= 0.02 * len(pts)
    codes = np.array([row[1] for row in rows])
    for c in (ref.WINDOW_OUTSIDE, ref.MIN_EIG, ref.MAX_COUNT, ref.ERR_OUTSIDE):
        assert np.sum(codes == c) >= 3, c
    keep = np.setdiff1d(np.arange(len(pts)), aside)
    for sm in (0, 1):
        nx, st, err, lv, tr = orc[sm]
        np.testing.assert_array_equal(tr["exit"][keep, 0], codes[keep])
        np.testing.assert_array_equal(st[keep], np.array([row[2] for row in rows])[keep])
        np.testing.assert_array_equal(tr["steps"][keep, 0], (codes[keep] >= ref.EPS).astype(np.int32))


def test_lk_exit_arms_are_populated(oracle):
    """The cases tests/test_gpu_lk_envelope.py runs reach every exit at level 0, and every exit that exists there at
    an upper level, with at least 5 points each (counted here on the CPU; the GPU module asserts it again before it
    compares)."""
    level0, upper, _ = lk_cases.exit_arm_counts(oracle, lk_cases.exit_arm_cases())
    print("level 0:", level0.tolist(), "upper levels:", upper.tolist())
    assert np.all(level0[oracle.LK_WINDOW_OUTSIDE:] >= 5)
    assert np.all(upper[oracle.LK_WINDOW_OUTSIDE:oracle.LK_ERR_OUTSIDE] >= 5) and upper[oracle.LK_ERR_OUTSIDE] == 0
