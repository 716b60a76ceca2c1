"""The pose solvers' data-dependent arms ("the pose solvers' data-dependent arms"), bit for bit against the CPU
oracle: NaNs at the same positions, every other value equal as bits, no tolerance anywhere.

tests/test_gpu_geom.py feeds random scenes of 7 to 2000 edges and one family with points in the camera plane.  Here the
corpus of tests/pose_scene.py takes the other arms of pose_lm_kernel / pose_gn_kernel and of the two 6 x 6 LDLT forms:
rounds without an active edge, an LDLT that is not positive, a non-finite trial chi2, zero / NaN pivots at k == 0 and
after, a non-finite operand in a wave with and without Huber-weighted edges, the edge counts around the 64- / 256- /
512-thread strides up to kMaxEdges, and problems past it.  The families are interleaved so that neighbouring workgroups
take different arms.  test_corpus_reaches_the_arms (CPU only) asserts on the oracle's traces that the corpus is where it
claims to be.

The trial loop's exit on a non-finite lambda is reached where H's diagonal overflows (fx, fy scaled by 1e160 and up:
lambda = 1e-5 max|H_ii| starts as inf; family k_overflow).  Not reached through or_pose_lm: an LDLT of sign 2.  The
diagonal of J^T W J + lambda I is a sum of squares times weights >= 0 plus lambda >= 0, so the first pivot, the largest
|diagonal|, is positive, zero (the k == 0 exit) or NaN (the same exit), never negative, and sign 2 needs a negative
first pivot; 6000 problems of the families here with X, uv, fx / fy or the prior's translation scaled by 1e-300 ..
1e300 reached none.  The direct LDLT test covers sign 2 on the LDLT side (negative definite and semidefinite systems)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import pose_scene
from ya_vo_amd import scene

gpu = pytest.mark.gpu
CAP = 4096  # kMaxEdges
ENVELOPE = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 2049, 4095, 4096)
GN_ORDER = 1
WIDTHS = [pytest.param(1, id="512-thread"), pytest.param(3, id="256-thread")]  # corpus repeats: <= 256 / > 256 problems


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    g, w = got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} values differ as bits, first {got[~gn][bad[0]]!r} vs {want[~wn][bad[0]]!r}"


def _lm_mode(count):
    import ya_vo_amd as yv
    return yv.lm_sum_mode(count)


# ------------------------------------------------------------------------------------------------
# the corpora and their oracle results, computed once
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _corpus():
    with np.errstate(all="ignore"):
        probs = pose_scene.interleave(pose_scene.lm_corpus())
    for p in probs:
        for a in p[1:]:
            a.setflags(write=False)
    return probs


@functools.lru_cache(None)
def _gn_corpus():
    with np.errstate(all="ignore"):
        probs = pose_scene.gn_corpus()
    for p in probs:
        for a in p[1:]:
            a.setflags(write=False)
    return probs


@functools.lru_cache(None)
def _lm_refs(oracle, mode):
    """(pose, outlier, inliers, trace) of every corpus problem in the oracle's order `mode`; the plain entry point gives
    the same bits as the traced one."""
    refs = []
    for name, X, uv, K, prior in _corpus():
        T, out, inl, tr = oracle.pose_lm_ex(X, uv, K, prior, mode)
        pT, pout, pinl = oracle.pose_lm(X, uv, K, prior, mode)
        assert_same_bits(pT, T, f"{name}: or_pose_lm vs its traced form")
        assert pinl == inl and np.array_equal(pout, out), name
        refs.append((T, out, inl, tr))
    return refs


@functools.lru_cache(None)
def _gn_refs(oracle):
    refs = []
    for name, X, uv, K, prior in _gn_corpus():
        T, it, tr = oracle.pose_gn_ex(X, uv, K, prior, GN_ORDER)
        pT, pit = oracle.pose_gn(X, uv, K, prior, GN_ORDER)
        assert_same_bits(pT, T, f"{name}: or_pose_gn vs its traced form")
        assert pit == it, name
        refs.append((T, it, tr))
    return refs


def _damped(H, lam):
    Hl = np.array(H, np.float64)
    Hl[np.diag_indices(6)] = np.diag(H) + lam
    return Hl


@functools.lru_cache(None)
def _ldlt_refs(oracle):
    """-> (names, H, lam, b, per variant (x [n, 6], positive [n]), traces of variant 0)."""
    names, H, lam, b = pose_scene.ldlt_corpus()
    res, traces = [], []
    for variant in (0, 1):
        xs, ps = np.zeros((len(names), 6)), np.zeros(len(names), np.int32)
        for k in range(len(names)):
            pos, x, tr = oracle.ldlt6_ex(_damped(H[k], lam[k]), b[k], variant)
            ppos, px = oracle.ldlt6(_damped(H[k], lam[k]), b[k], variant)
            assert_same_bits(px, x, f"{names[k]}: or_ldlt6_solve vs its traced form")
            assert ppos == pos, names[k]
            xs[k], ps[k] = x, pos
            if variant == 0:
                traces.append(tr)
        res.append((xs, ps))
    for a in (H, lam, b):
        a.setflags(write=False)
    return names, H, lam, b, res, traces


@functools.lru_cache(None)
def _envelope():
    """Noisy scenes with 10 % outliers at the edge counts around the kernels' strides, up to kMaxEdges."""
    probs = []
    for k, n in enumerate(ENVELOPE):
        X, uv, T, _ = scene.random_scene(n, seed=500 + k, noise_px=0.5, outlier_frac=0.1)
        prior = scene.perturb(T, np.random.default_rng(500 + k))
        probs.append((f"n={n}", np.ascontiguousarray(X), np.ascontiguousarray(uv), scene.K_KITTI.copy(), prior))
    return probs


@functools.lru_cache(None)
def _envelope_lm_refs(oracle, mode):
    return [oracle.pose_lm(X, uv, K, prior, mode) for _, X, uv, K, prior in _envelope()]


@functools.lru_cache(None)
def _envelope_gn_refs(oracle):
    return [oracle.pose_gn(X, uv, K, prior, GN_ORDER) for _, X, uv, K, prior in _envelope()]


# ------------------------------------------------------------------------------------------------
# CPU: the corpus is where it claims to be
# ------------------------------------------------------------------------------------------------
# The LM's arms as conditions on one round's trace (oracle_bind.Oracle.LM_TRACE_FIELDS), and the families that
# DESIGN.md's arms table names for each: every named family reaches the arm in at least one of its problems, and the
# families together in at least five.
LM_ARMS = {
    "a round with no active edge": (
        lambda r: r["active"] == 0 and r["iters"] == -1,
        "far_prior random_uv uv_huge k_huge z_tiny k_tiny rotated behind coincident"),
    "LDLT not positive (ok2 == 0), sign 1 -> 3": (
        lambda r: r["not_positive"] > 0 and r["ldlt_signs"] & 8, "k_huge"),
    "trial chi2 non-finite, ok2 == 1": (
        lambda r: r["chi_nonfinite"] > 0,
        "uv_huge k_overflow x_huge z_tiny bad_quiet bad_huber bad_two_waves camera_plane"),
    "LDLT exit at k == 0": (
        lambda r: r["ldlt_k0"] > 0, "uv_huge z_tiny k_tiny bad_quiet bad_huber bad_two_waves camera_plane"),
    "LDLT zero pivot at k > 0": (lambda r: r["ldlt_zero_pivot"] > 0, "x_huge k_huge k_overflow"),
    "the solve's > DBL_MIN test zeroes an entry": (
        lambda r: r["ldlt_zeroed"] > 0, "uv_huge k_huge k_overflow x_huge z_tiny k_tiny bad_quiet camera_plane"),
    "a transposition": (lambda r: r["ldlt_pivoted"] > 0, "normal exact rotated"),
    "classification at a rejected Tlast": (
        lambda r: r["last_rejected"] and r["active"] > 0, "normal exact near_plane k_huge x_huge z_tiny tiny_n"),
    "the literal pass (a non-finite operand)": (
        lambda r: r["literal"], "k_huge k_overflow x_huge bad_quiet bad_huber bad_two_waves camera_plane"),
    "... on a Huber edge in a wave without a Huber-weighted edge": (
        lambda r: r["literal_waves"] & 1, "bad_quiet bad_two_waves k_overflow"),
    "... a NaN chi2 there (the kernel's w = 1.0 against the oracle's NaN)": (
        lambda r: r["literal_waves"] & 8, "bad_quiet bad_two_waves camera_plane"),
    "... in a wave with Huber-weighted edges": (lambda r: r["literal_waves"] & 2, "bad_huber x_huge camera_plane"),
    "... in a quiet wave while another wave of the pass has Huber-weighted edges": (
        lambda r: r["literal_waves"] & 4, "bad_two_waves"),
    "trials rejected": (lambda r: r["rejected"] > 0, "normal exact near_plane"),
    "trials accepted": (lambda r: r["accepted"] > 0, "normal rotated collinear"),
    "the trial loop runs ten iterations": (
        lambda r: r["active"] > 0 and r["end"] == 0, "far_prior random_uv behind normal"),
    "the trial loop ends on qmax == 10": (lambda r: r["end"] & 1, "k_huge rotated normal"),
    "the trial loop ends on rho == 0": (lambda r: r["end"] & 2, "exact tiny_n near_plane collinear k_tiny"),
    "the trial loop ends on a non-finite lambda": (lambda r: r["end"] & 4, "k_overflow"),
    "the round replays the one before": (lambda r: r["replay"], "exact far_prior"),
}


def test_corpus_reaches_the_arms(oracle):
    """Each arm in at least five corpus problems (LM, in both of the kernel's summation orders, and GN) or systems
    (LDLT), the `ok2 == 0` arm also in at least five trials, and each arm in every family that DESIGN.md's table
    names for it.  Conditions on the inputs that the traces cannot show (camera-frame z of exactly 1e-170 or 0, a
    point exactly at the camera centre) are asserted on the transformed input as well."""
    probs = _corpus()
    fams = [p[0] for p in probs]
    # neighbours differ: every aligned group of eight problems among the first 64 holds eight families
    assert all(len(set(fams[k:k + 8])) == 8 for k in range(0, 64, 8))
    for name, X, uv, K, prior in probs:
        if name == "z_tiny":  # the family's camera-frame z is 1e-170 as a value, not a rounding residue
            assert (scene.transform(prior, X)[::3, 2] == 1e-170).all()
    for mode in (6, 7):  # the 256- and the 512-thread kernel's orders
        traces = [r[3] for r in _lm_refs(oracle, mode)]
        for arm, (pred, named) in LM_ARMS.items():
            hit = [f for f, tr in zip(fams, traces) if any(pred(r) for r in tr)]
            assert len(hit) >= 5, arm
            assert set(named.split()) <= set(hit), f"{arm}: not in {set(named.split()) - set(hit)}"
        assert sum(r["not_positive"] for tr in traces for r in tr) >= 5                 # ok2 == 0 in five trials
        assert not any(r["ldlt_signs"] & 4 for tr in traces for r in tr)                # sign 2: not reachable
        replay = [r["replay"] for tr in traces for r in tr[1:]]
        assert sum(replay) >= 5 and sum(not v for v in replay) >= 5

    gprobs = _gn_corpus()
    gtraces = [r[2] for r in _gn_refs(oracle)]
    gfams = [p[0] for p in gprobs]

    def gn_hit(pred, named):
        hit = [f for f, t, p in zip(gfams, gtraces, gprobs) if pred(t, p)]
        assert set(named.split()) <= set(hit), set(named.split()) - set(hit)
        return len(hit)

    # isnan(dx[0]) at iteration 0; a cost increase; |dx| < 1e-6; all ten iterations
    assert gn_hit(lambda t, p: t["stop"][0] == 1, "x_huge z_tiny bad_quiet bad_huber bad_two_waves camera_plane") >= 5
    assert gn_hit(lambda t, p: 2 in t["stop"], "far_prior behind") >= 5
    assert gn_hit(lambda t, p: 3 in t["stop"], "normal exact tiny_n") >= 5
    assert gn_hit(lambda t, p: t["stop"][9] == 0, "far_prior random_uv rotated near_plane") >= 5
    assert gn_hit(lambda t, p: len(p[1]) == 1 and 3 in t["sign"], "gn_single") >= 5     # an indefinite H from one edge
    # a single point with pc_z == 0 (u / 0) and one at the camera centre (0 / 0): exact zeros in the oracle's own
    # transform and in numpy's, each stopping on isnan(dx[0]) at iteration 0
    for bit, at in ((1, "plane"), (2, "centre")):
        hit = [p for t, p in zip(gtraces, gprobs) if len(p[1]) == 1 and t["plane"][0] == bit and t["stop"][0] == 1]
        assert len(hit) >= 5 and {p[0] for p in hit} == {"gn_single"}, at
        for name, X, uv, K, prior in hit:
            pc = scene.transform(prior, X)[0]
            assert pc[2] == 0 and (pc[0] != 0 and pc[1] != 0 if bit == 1 else (pc == 0).all()), at
    assert gn_hit(lambda t, p: any(v > 0 and v & 1 for v in t["ldlt"]), "uv_huge k_tiny") >= 5          # k == 0 exit
    assert gn_hit(lambda t, p: any(v > 0 and v & 2 for v in t["ldlt"]), "gn_single coincident camera_plane") >= 5

    names, H, lam, b, res, ltraces = _ldlt_refs(oracle)
    assert len({t["tr"] for t in ltraces[:720]}) == 720                                 # every transposition sequence
    for sign in (0, 1, 2, 3):
        assert sum(t["sign"] == sign for t in ltraces) >= 5, sign
    assert sum(t["k0_exit"] for t in ltraces) >= 5
    assert sum(t["zero_pivots"] > 0 for t in ltraces) >= 5
    assert sum(t["zeroed"] > 0 for t in ltraces) >= 5
    assert sum(bool(np.isnan(x).any()) for x in res[0][0]) >= 5
    assert sum(bool((x0.view(np.uint64) != x1.view(np.uint64)).any()) for x0, x1 in zip(res[0][0], res[1][0])) >= 5


def _trig_arguments():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(-7, 7, 2000), rng.uniform(-1e3, 1e3, 2000), rng.uniform(-1048575, 1048575, 2000),
                           np.arange(1, 400) * (np.pi / 2), np.nextafter(np.arange(1, 400) * (np.pi / 2), 0),
                           [0.7853981633974484, 0.7853981633974483, 1048575.9, -1048575.9, 3.141592653589793, 355.0,
                            0.0, -0.0, 1e-300, 5e-324]])


@gpu
def test_sin_cos_match_oracle(ctx, oracle):
    """k_sin / k_cos of yavo_se3.h against the oracle's, bit for bit on finite arguments below 2^20 (the polynomial
    range and the shared reduction); past it both sides call their own library: NaN where the oracle's is (inf, NaN)."""
    x = np.concatenate([_trig_arguments(), [np.inf, -np.inf, np.nan]])
    s, c = np.full(len(x), 7.0), np.full(len(x), 7.0)
    lib = _lib()
    assert lib.yv_debug_sincos(x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data) == 0
    assert_same_bits(s, [oracle.lib.or_ksin(float(v)) for v in x], "k_sin")
    assert_same_bits(c, [oracle.lib.or_kcos(float(v)) for v in x], "k_cos")


def test_sin_cos_past_quarter_pi(oracle):
    """The restated sin / cos of SE3::exp between pi/4 and 2^20 (the reduction the GPU shares; far priors and the GN's
    undamped steps get there): within 2.3e-16 of the C library's, also next to multiples of pi/2, where the reduced
    argument cancels."""
    for x in map(float, _trig_arguments()):  # each side's error is below an ulp, and an ulp of a value below 1 is at most 1.1e-16
        assert abs(oracle.lib.or_ksin(x) - math.sin(x)) <= 2.3e-16, x
        assert abs(oracle.lib.or_kcos(x) - math.cos(x)) <= 2.3e-16, x


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def _lib():
    import ya_vo_amd as yv
    lib = yv.load_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.yv_debug_ldlt6.argtypes = [ci, vp, vp, vp, ci, vp, vp]
    lib.yv_debug_ldlt6.restype = ci
    lib.yv_debug_track_pose.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.yv_debug_track_pose.restype = ci
    lib.yv_debug_sincos.argtypes = [vp, ci, vp, vp]
    lib.yv_debug_sincos.restype = ci
    return lib


SENTINEL = 7


def _launch_lm(ctx, probs, track=False):
    """yv_pose_lm_batch (CSR) or yv_debug_track_pose (fixed stride) on (name, X, uv, K, prior) problems -> per problem
    (pose, outlier bytes of the problem's whole range, inliers)."""
    import torch
    P = len(probs)
    counts = np.array([len(p[1]) for p in probs], np.int32)
    dev = "cuda:0"
    K = torch.from_numpy(np.stack([p[3].reshape(9) for p in probs])).to(dev)
    priors = np.stack([p[4] for p in probs])
    if track:
        stride = int(counts.max())
        X, uv = np.zeros((P, stride, 3)), np.zeros((P, stride, 2))
        for k, p in enumerate(probs):
            X[k, :counts[k]], uv[k, :counts[k]] = p[1], p[2]
        starts = np.arange(P, dtype=np.int64) * stride
    else:
        X = np.concatenate([p[1] for p in probs] + [np.zeros((1, 3))])
        uv = np.concatenate([p[2] for p in probs] + [np.zeros((1, 2))])
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        starts = offs[:-1].astype(np.int64)
    d_X, d_uv = torch.from_numpy(np.ascontiguousarray(X)).to(dev), torch.from_numpy(np.ascontiguousarray(uv)).to(dev)
    d_out = torch.full((int(X.size // 3),), SENTINEL, dtype=torch.uint8, device=dev)
    d_inl = torch.full((P,), -1, dtype=torch.int32, device=dev)
    d_prior = torch.from_numpy(priors.copy()).to(dev)
    torch.cuda.synchronize()
    if track:
        d_cnt = torch.from_numpy(counts).to(dev)
        d_pose = torch.full((P, 7), 3.0, dtype=torch.float64, device=dev)
        st = _lib().yv_debug_track_pose(ctx.handle, P, d_cnt.data_ptr(), stride, d_X.data_ptr(), d_uv.data_ptr(),
                                        K.data_ptr(), d_prior.data_ptr(), d_pose.data_ptr(), d_out.data_ptr(),
                                        d_inl.data_ptr(), None)
    else:
        d_off = torch.from_numpy(offs).to(dev)
        d_pose = d_prior
        st = ctx.lib.yv_pose_lm_batch(ctx.handle, P, d_off.data_ptr(), d_X.data_ptr(), d_uv.data_ptr(), K.data_ptr(),
                                      d_pose.data_ptr(), d_out.data_ptr(), d_inl.data_ptr(), None)
    assert st == 0
    ctx.sync()
    if track:  # the priors are read only
        assert_same_bits(d_prior.cpu().numpy(), priors, "priors after the launch")
    pose, out, inl = d_pose.cpu().numpy(), d_out.cpu().numpy(), d_inl.cpu().numpy()
    return [(pose[k], out[starts[k]:starts[k] + counts[k]], int(inl[k])) for k in range(P)]


def _check_lm(got, ref, what):
    T, out, inl = ref[:3]
    assert_same_bits(got[0], T, f"{what}: pose")
    np.testing.assert_array_equal(got[1], out.astype(np.uint8), err_msg=f"{what}: outlier flags")
    assert got[2] == inl, f"{what}: inliers"


@gpu
@pytest.mark.parametrize("track", [pytest.param(False, id="csr"), pytest.param(True, id="track")])
@pytest.mark.parametrize("repeat", WIDTHS)
def test_lm_corpus_matches_oracle(ctx, oracle, repeat, track):
    """The interleaved corpus in one launch of yv_pose_lm_batch (CSR) and of launch_track_pose (the benchmark's
    fixed-stride layout, priors and poses in separate buffers), by the 512- and the 256-thread kernel: pose, outlier
    flags and inlier count of every problem."""
    probs = _corpus() * repeat
    assert (len(probs) <= 256) == (repeat == 1)
    refs = _lm_refs(oracle, _lm_mode(len(probs))) * repeat
    got = _launch_lm(ctx, probs, track)
    for k, p in enumerate(probs):
        _check_lm(got[k], refs[k], f"problem {k} ({p[0]}, n = {len(p[1])})")


@gpu
def test_lm_host_matches_oracle(ctx, oracle):
    """One problem of each family through the host yv_pose_lm; a non-finite prior is YV_ERR_INVALID."""
    import ya_vo_amd as yv
    probs, refs = _corpus(), _lm_refs(oracle, _lm_mode(1))
    seen = set()
    for k, (name, X, uv, K, prior) in enumerate(probs):
        if name in seen:
            continue
        seen.add(name)
        T, out, inl = ctx.pose_lm(X, uv, K, prior)
        _check_lm((T, out.astype(np.uint8), inl), refs[k], name)
    assert seen == set(pose_scene.LM_FAMILIES)
    name, X, uv, K, prior = probs[0]
    for bad in (np.nan, np.inf):
        for q in (0, 5):
            p = prior.copy()
            p[q] = bad
            with pytest.raises(yv.YavoError) as e:
                ctx.pose_lm(X, uv, K, p)
            assert e.value.status == yv.YV_ERR_INVALID
            with pytest.raises(yv.YavoError) as e:
                ctx.pose_gn(X, uv, K, p)
            assert e.value.status == yv.YV_ERR_INVALID


@gpu
def test_set_tracks_refuses_a_non_finite_extrinsic(ctx):
    """yv_batch_set_tracks shares the host calls' pose check: a NaN or infinite T_right entry is YV_ERR_INVALID, and
    the finite one is taken afterwards."""
    import ya_vo_amd as yv
    T_right = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
    b = yv.Batch(ctx, 4, 376, 1241, 2000, 4)
    try:
        b.set_pairs([(0, 2), (2, 3)])
        for bad in (np.nan, np.inf, -np.inf):
            for q in (3, 5):
                T = T_right.copy()
                T[q] = bad
                with pytest.raises(yv.YavoError) as e:
                    b.set_tracks([(1, 0)], scene.K_KITTI, T)
                assert e.value.status == yv.YV_ERR_INVALID
        b.set_tracks([(1, 0)], scene.K_KITTI, T_right)
    finally:
        b.close()


def _launch_gn(ctx, probs):
    import torch
    P = len(probs)
    counts = np.array([len(p[1]) for p in probs], np.int32)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    dev = "cuda:0"
    d_off = torch.from_numpy(offs).to(dev)
    d_X = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[1] for p in probs] + [np.zeros((1, 3))]))).to(dev)
    d_uv = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[2] for p in probs] + [np.zeros((1, 2))]))).to(dev)
    d_K = torch.from_numpy(np.stack([p[3].reshape(9) for p in probs])).to(dev)
    d_P = torch.from_numpy(np.stack([p[4] for p in probs])).to(dev)
    d_it = torch.full((P,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert ctx.lib.yv_pose_gn_batch(ctx.handle, P, d_off.data_ptr(), d_X.data_ptr(), d_uv.data_ptr(), d_K.data_ptr(),
                                    d_P.data_ptr(), d_it.data_ptr(), None) == 0
    ctx.sync()
    return d_P.cpu().numpy(), d_it.cpu().numpy()


@gpu
def test_gn_corpus_matches_oracle(ctx, oracle):
    """The corpus and the GN-only single-point problems through yv_pose_gn_batch and, one of each family, the host
    yv_pose_gn: pose and accepted iterations."""
    probs, refs = _gn_corpus(), _gn_refs(oracle)
    P, it = _launch_gn(ctx, probs)
    seen = set()
    for k, (name, X, uv, K, prior) in enumerate(probs):
        what = f"problem {k} ({name}, n = {len(X)})"
        assert_same_bits(P[k], refs[k][0], what)
        assert it[k] == refs[k][1], what
        if name not in seen or name == "gn_single":
            seen.add(name)
            hT, hit = ctx.pose_gn(X, uv, K, prior)
            assert_same_bits(hT, refs[k][0], f"host {what}")
            assert hit == refs[k][1], f"host {what}"


@gpu
@pytest.mark.parametrize("form", [pytest.param(0, id="ldlt6_solve_lds<0>"), pytest.param(1, id="ldlt6_solve<1>")])
def test_ldlt6_matches_oracle(oracle, ctx, form):
    """The two device LDLT forms on the matrix corpus against or_ldlt6_solve variants 0 and 1: x and the positive flag."""
    names, H, lam, b, res, _ = _ldlt_refs(oracle)
    n = len(names)
    Hc, lc, bc = np.ascontiguousarray(H.reshape(n, 36)), np.ascontiguousarray(lam), np.ascontiguousarray(b)
    x = np.full((n, 6), 7.0)
    pos = np.full(n, -1, np.int32)
    assert _lib().yv_debug_ldlt6(form, Hc.ctypes.data, lc.ctypes.data, bc.ctypes.data, n, x.ctypes.data,
                                 pos.ctypes.data) == 0
    for k, name in enumerate(names):
        assert pos[k] == res[form][1][k], name
        assert_same_bits(x[k], res[form][0][k], name)


@gpu
@pytest.mark.parametrize("repeat", [pytest.param(1, id="512-thread"), pytest.param(19, id="256-thread")])
def test_lm_edge_count_envelope(ctx, oracle, repeat):
    """n = 1, the counts around the 64- / 256- / 512-thread strides, 1024, 2049 and kMaxEdges - 1 / kMaxEdges."""
    probs = _envelope() * repeat
    assert (len(probs) <= 256) == (repeat == 1)
    refs = _envelope_lm_refs(oracle, _lm_mode(len(probs))) * repeat
    got = _launch_lm(ctx, probs)
    for k, p in enumerate(probs):
        _check_lm(got[k], refs[k], f"problem {k} ({p[0]})")


@gpu
def test_gn_edge_count_envelope(ctx, oracle):
    probs, refs = _envelope(), _envelope_gn_refs(oracle)
    P, it = _launch_gn(ctx, probs)
    for k, p in enumerate(probs):
        assert_same_bits(P[k], refs[k][0], p[0])
        assert it[k] == refs[k][1], p[0]


@gpu
def test_lm_over_capacity(ctx, oracle):
    """yv_pose_lm_batch solves the first kMaxEdges edges of a longer problem: the pose and flags of the oracle on those,
    inliers = kMaxEdges - outliers, outlier bytes past them untouched.  The host calls refuse such a problem."""
    import ya_vo_amd as yv
    probs = []
    for k, n in enumerate((CAP + 1, 6000)):
        X, uv, T, _ = scene.random_scene(n, seed=600 + k, noise_px=0.5, outlier_frac=0.1)
        probs.append((f"n={n}", np.ascontiguousarray(X), np.ascontiguousarray(uv), scene.K_KITTI.copy(),
                      scene.perturb(T, np.random.default_rng(600 + k))))
    got = _launch_lm(ctx, probs)
    for g, (name, X, uv, K, prior) in zip(got, probs):
        T, out, inl = oracle.pose_lm(X[:CAP], uv[:CAP], K, prior, _lm_mode(len(probs)))
        assert_same_bits(g[0], T, name)
        np.testing.assert_array_equal(g[1][:CAP], out.astype(np.uint8), err_msg=name)
        assert (g[1][CAP:] == SENTINEL).all(), f"{name}: outlier bytes past kMaxEdges"
        assert g[2] == inl == CAP - int(out.sum()), name
    name, X, uv, K, prior = probs[0]
    for call in (ctx.pose_lm, ctx.pose_gn):
        with pytest.raises(yv.YavoError) as e:
            call(X, uv, K, prior)
        assert e.value.status == yv.YV_ERR_CAPACITY
