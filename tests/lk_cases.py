"""Inputs shared by the LK tests: the float64 one-step fixture of tests/test_oracle_lk.py and the cases whose exit
arms tests/test_oracle_lk.py counts on the CPU and tests/test_gpu_lk_envelope.py then runs on the GPU."""
import numpy as np

from ya_vo_amd.synth import synth_frame

# ---- the one-step fixture (tests/lk_reference.py against the oracle) ----
STEP_SHAPE = (48, 64)
STEP_WINDOWS = (3, 4, 11, 16, 22)
STEP_POINTS = 300
STEP_SEED = 20


def step_pair():
    H, W = STEP_SHAPE
    return synth_frame(STEP_SEED, 0, 0, H, W), synth_frame(STEP_SEED, 1, 3, H, W)


def step_points(win):
    """300 points: 180 anywhere up to win / 2 + 2 outside the image, and 30 within win of each of the four borders
    (either side of it)."""
    H, W = STEP_SHAPE
    rng = np.random.default_rng(1000 + win)
    m = win / 2 + 2
    free = np.stack([rng.uniform(-m, W - 1 + m, 180), rng.uniform(-m, H - 1 + m, 180)], 1)
    along_x, along_y = rng.uniform(-m, W - 1 + m, (2, 30)), rng.uniform(-m, H - 1 + m, (2, 30))
    near = rng.uniform(-m, win, (4, 30))
    edges = [np.stack([near[0], along_y[0]], 1), np.stack([W - 1 - near[1], along_y[1]], 1),
             np.stack([along_x[0], near[2]], 1), np.stack([along_x[1], H - 1 - near[3]], 1)]
    return np.concatenate([free] + edges).astype(np.float32)


# ---- the envelope cases ----
ENV_SHAPE = (96, 128)
ENV_POINTS = 400


def env_pair(shape=ENV_SHAPE):
    return synth_frame(20, 0, 0, *shape), synth_frame(20, 1, 3, *shape)


def env_points(seed, shape=ENV_SHAPE, n=ENV_POINTS, margin=18.0):
    """n points drawn uniformly over the image and up to `margin` px outside it."""
    H, W = shape
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-margin, W - 1 + margin, n), rng.uniform(-margin, H - 1 + margin, n)], 1).astype(
        np.float32)


# (win, max_count, eps, min_eig): every max_count of {0, 1, 3, 30, 100, 250}, every eps of {0, 0.01, 10, 25, -1} and
# every min_eig of {0, 1e-3, 0.05, 1e9} at least once; 250 / 25 / -1 are the values the clips to 100 / 10 / 0 change
TERMINATION_GRID = [
    (11, 30, 0.01, 1e-3), (16, 30, 0.01, 1e-3),
    (11, 0, 0.01, 1e-3), (16, 0, 0.0, 0.0),
    (11, 1, 0.0, 1e-3), (16, 1, 10.0, 0.05),
    (11, 3, 0.0, 1e-3), (16, 3, 0.01, 0.0),
    (11, 100, 0.0, 0.0), (16, 100, 0.0, 0.0),
    (11, 250, 0.0, 1e-3), (16, 250, -1.0, 1e-3),
    (11, 30, 10.0, 1e-3), (16, 30, 25.0, 1e-3),
    (11, 30, -1.0, 0.05), (16, 100, 25.0, 0.0),
    (11, 3, 25.0, 0.05), (16, 30, 0.01, 1e9),
    (11, 1, 0.01, 1e9), (11, 250, 0.01, 0.0),
]


def exit_arm_cases():
    """The cases over which every exit arm must be populated: the termination grid (case k on its own 400 points)
    and the error-window case.  -> [(name, prev, next, pts, kwargs of oracle.lk / calc_optical_flow_pyr_lk)]."""
    prev, nxt = env_pair()
    cases = [(f"win{win}-count{mc}-eps{eps:g}-mineig{me:g}", prev, nxt, env_points(100 + k),
              dict(win=win, max_level=3, max_count=mc, eps=eps, min_eig=me))
             for k, (win, mc, eps, me) in enumerate(TERMINATION_GRID)]
    return cases + [("error-window-outside",) + err_outside_case()]


def exit_arm_counts(oracle, cases):
    """-> (level-0 counts [9], upper-level counts [9]) of the oracle's exit codes over the cases, and the oracle's
    results per case (next, status, err, top level) in sum_mode 1."""
    level0, upper, results = np.zeros(9, np.int64), np.zeros(9, np.int64), []
    for _, prev, nxt, pts, kw in cases:
        nx, st, err, lv, tr = oracle.lk(prev, nxt, pts, sum_mode=1, trace=True, **kw)
        level0 += np.bincount(tr["exit"][:, 0], minlength=9)
        upper += np.bincount(tr["exit"][:, 1:lv + 1].ravel(), minlength=9)
        results.append((nx, st, err, lv))
    return level0, upper, results


def err_outside_case():
    """Points whose final error window lies outside the image (the level-0-only exit): the next frame is the previous
    one moved 25 px to the right, the points start 2 .. 9 px inside the right border, and few steps are allowed, so
    that the last step taken carries the window's corner past the border before the in-iteration check sees it.
    -> (prev, next, pts, kwargs)."""
    H, W = ENV_SHAPE
    prev, nxt = synth_frame(20, 0, 25, H, W), synth_frame(20, 0, 0, H, W)
    rng = np.random.default_rng(77)
    pts = np.stack([W - 1 - rng.uniform(2, 9, ENV_POINTS), rng.uniform(8, H - 9, ENV_POINTS)], 1).astype(np.float32)
    return prev, nxt, pts, dict(win=11, max_level=3, max_count=2, eps=0.0, min_eig=1e-3)
