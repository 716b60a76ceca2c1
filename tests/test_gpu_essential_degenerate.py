"""The five-point solver's data-dependent arms ("findEssentialMat: the solver's arms"), bit for bit against
the CPU oracle: NaNs at the same positions, every other value equal as bits, no tolerance anywhere.

tests/test_gpu_essential.py feeds general scenes only, which take one path: a regular LU, degree 10, no coincident
Durand-Kerner iterates, no solveZ reject, all 300 sweeps, an even model count.  Here the corpus of
tests/epipolar_scene.py (stationary cameras, pure rotations, collinear / lattice / repeated points, planar scenes)
takes the others, with the families interleaved so that the rows of a group-form wave and the lanes of a lane-form
wave take different arms at the same time.  test_corpus_reaches_the_arms (CPU only) asserts on the oracle's trace that
the corpus is where it claims to be.

Coincident iterates (solvePoly skips the factor; the kernels' kSel select / replay): the polynomial set has one at
degrees 2, 3, 4, 6, 7, 8, 9 and 10; none was found at degree 5 (epipolar_scene.COINCIDENT_POLYS)."""
import ctypes
import functools

import numpy as np
import pytest

import epipolar_scene as scene
from epipolar_scene import FOCAL, K_KITTI, PP

gpu = pytest.mark.gpu
FORMS = [pytest.param(1, id="group"), pytest.param(9, id="lane")]  # lists in the workspace: <= 8 group form, else lane


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    g, w = got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} values differ as bits, first {got[~gn][bad[0]]!r} vs {want[~wn][bad[0]]!r}"


# ------------------------------------------------------------------------------------------------
# the corpus and its oracle results, computed once
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _five_point(oracle):
    q1, q2, fam = scene.five_point_corpus(64)
    models = np.zeros((len(q1), 10, 9))
    counts = np.zeros(len(q1), np.int32)
    traces = []
    for k in range(len(q1)):
        models[k], counts[k], tr = oracle.em_kernel_ex(q1[k], q2[k])
        traces.append(tr)
    for a in (q1, q2, fam, models, counts):
        a.setflags(write=False)
    return q1, q2, fam, models, counts, traces


@functools.lru_cache(None)
def _polys(oracle):
    coeffs, names = scene.poly_corpus()
    roots = np.zeros((len(coeffs), 10, 2))
    traces = []
    for k, c in enumerate(coeffs):
        roots[k], tr = oracle.solve_poly_ex(c)
        traces.append(tr)
    assert_same_bits(np.array([_plain_roots(oracle, c) for c in coeffs]), roots, "or_solve_poly vs its traced form")
    coeffs.setflags(write=False)
    roots.setflags(write=False)
    return coeffs, names, roots, traces


def _plain_roots(oracle, c):
    z, _ = oracle.solve_poly(c)  # or_solve_poly itself: the traced form is the same function
    return np.stack([z.real, z.imag], 1)


def _reference(oracle, p1, p2, **kw):
    """findEssentialMat + recoverPose of the oracle on one float32 list."""
    ok, E, mask, st = oracle.find_essential(p1, p2, FOCAL, PP, **kw)
    good, R, t, per = oracle.recover_pose(E if ok else np.zeros((3, 3)), p1, p2, K_KITTI)
    return dict(ok=ok, E=E if ok else np.zeros((3, 3)), mask=mask, stats=(st["iters"], st["models"], st["best"]),
                good=good, R=R, t=t, per=tuple(int(v) for v in per))


STRIDE = 200


@functools.lru_cache(None)
def _lists(oracle):
    """The degenerate lists, one whose count exceeds the stride (clipped to it) and one with a negative count (clipped
    to 0) -> (names, pts1 [P, STRIDE, 2], pts2, counts as passed, references on the clipped lists)."""
    lists = scene.degenerate_lists()
    names = [n for n, _, _ in lists]
    a, b, _, _ = scene.two_view_scene(STRIDE, outlier_frac=0.3, seed=50)
    over = len(lists) // 2  # not the last list: its count stays inside the arrays even unclipped
    lists.insert(over, ("count>stride", a.astype(np.float32), b.astype(np.float32)))
    names.insert(over, "count>stride")
    lists.append(("count<0", a.astype(np.float32), b.astype(np.float32)))
    names.append("count<0")
    P = len(lists)
    pts1, pts2 = np.zeros((P, STRIDE, 2), np.float32), np.zeros((P, STRIDE, 2), np.float32)
    counts = np.zeros(P, np.int32)
    refs = []
    for p, (name, x, y) in enumerate(lists):
        n = len(x)
        pts1[p, :n], pts2[p, :n] = x, y
        counts[p] = n
        if name == "count>stride":
            counts[p] = STRIDE + 60
        if name == "count<0":
            counts[p], n = -3, 0
        refs.append(_reference(oracle, pts1[p, :n], pts2[p, :n]))
    for arr in (pts1, pts2, counts):
        arr.setflags(write=False)
    return names, pts1, pts2, counts, refs


PARAM_CASES = [dict(max_iters=1), dict(max_iters=65), dict(max_iters=1025), dict(max_iters=3000), dict(prob=0.5),
               dict(prob=0.999999), dict(threshold=0.1), dict(threshold=10.0)]


@functools.lru_cache(None)
def _param_refs(oracle):
    p1, p2 = scene.outlier_list()
    return p1, p2, [_reference(oracle, p1, p2, **kw) for kw in PARAM_CASES]


@functools.lru_cache(None)
def _pose_cases(oracle):
    """recoverPose alone: (name, E, p1, p2) with E made by the oracle."""
    cases = []
    good_E = None
    for name, p1, p2 in scene.pose_scenes():
        ok, E, _, _ = oracle.find_essential(p1, p2, FOCAL, PP)
        assert ok, name
        cases.append((name, E, p1, p2))
        if name == "yaw0.05_t0":
            good_E = (E, p1, p2)
    E, p1, p2 = good_E
    cases.append(("-E", -E, p1, p2))
    cases.append(("E^T", np.ascontiguousarray(E.T), p1, p2))
    cases.append(("E=0", np.zeros((3, 3)), p1, p2))
    for n in (1, 16, 17):  # rp_count_kernel takes 16 points per wave
        cases.append((f"n={n}", E, p1[:n], p2[:n]))
    a = scene.degenerate_lists()[1]  # identical64: no candidate has a point in front of both cameras -- the tie
    ok, Et, _, _ = oracle.find_essential(a[1], a[2], FOCAL, PP)
    assert ok
    cases.append(("tie", Et, a[1], a[2]))
    refs = [oracle.recover_pose(E, p1, p2, K_KITTI) for _, E, p1, p2 in cases]
    return cases, refs


# ------------------------------------------------------------------------------------------------
# CPU: the corpus is where it claims to be
# ------------------------------------------------------------------------------------------------
def test_corpus_reaches_the_arms(oracle):
    _, _, fam, models, counts, traces = _five_point(oracle)
    singular = {t["singular"] for t in traces} - {0}
    assert len(singular) >= 2, singular  # the LU gives up at different pivots
    degrees = {t["degree"] for t in traces}
    assert {1, 8, 9, 10} <= degrees, degrees
    assert any(t["solvez"] for t in traces)
    assert any(c % 2 == 1 for c in counts) and any(c == 0 for c in counts), sorted(set(counts.tolist()))
    assert any(np.isnan(models[k, :counts[k]]).any() for k in range(len(counts)))
    assert any(t["sweeps"] < 300 for t in traces) and any(t["sweeps"] == 300 for t in traces)
    # neighbours differ: every aligned group of four subsets (a group-form wave) holds four families
    assert all(len(set(fam[k:k + 4])) == 4 for k in range(0, len(fam), 4))
    arms = [(t["singular"] != 0, t["degree"]) for t in traces]
    assert sum(len(set(arms[k:k + 4])) > 1 for k in range(0, len(arms), 4)) > len(arms) // 8  # waves that diverge

    coeffs, names, roots, ptraces = _polys(oracle)
    assert {t["degree"] for t in ptraces} == set(range(1, 11))
    by_degree = {}
    for t in ptraces:
        by_degree.setdefault(t["degree"], []).append(t)
    assert {d for d, ts in by_degree.items() if any(t["skips"] for t in ts)} == {2, 3, 4, 6, 7, 8, 9, 10}
    assert {d for d, ts in by_degree.items() if any(t["sweeps"] < 300 for t in ts)} >= {1, 2, 3, 4}
    assert np.isnan(roots[names.index("zero")][0]).all() and np.isnan(roots[names.index("constant")][0]).any()
    assert ptraces[names.index("leading 1e-17")]["degree"] == 9
    degs = [t["degree"] for t in ptraces]
    assert sum(len(set(degs[k:k + 4])) == 4 for k in range(0, len(degs) - 3, 4)) >= len(degs) // 4 - 3

    names_l, _, _, _, refs = _lists(oracle)
    for name in ("identical64", "identical200"):
        ref = refs[names_l.index(name)]
        assert ref["ok"] and ref["stats"] == (1, 10, int(name[9:])) and ref["mask"].all() and ref["per"] == (0, 0, 0, 0)
    assert np.isnan(refs[names_l.index("identical5")]["E"]).all()  # n = 5 returns the first model: the all-NaN one
    assert not refs[names_l.index("count<0")]["ok"]
    _, _, prefs = _param_refs(oracle)
    assert prefs[1]["stats"][0] == 65 and prefs[6]["stats"][0] == 1000  # a second round of one; every iteration run
    assert 64 < prefs[2]["stats"][0] < 1024

    cases, rrefs = _pose_cases(oracle)
    picks = {int(np.argmax(per)) for (_, _, _, per) in rrefs if max(per) > 0}
    assert picks == {0, 1, 2, 3}, picks
    assert any(sum(v > 0 for v in per) >= 2 for (_, _, _, per) in rrefs)  # two candidates with points in front
    tie = rrefs[[c[0] for c in cases].index("tie")]
    assert tuple(tie[3]) == (0, 0, 0, 0) and tie[0] == 0


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def _lib():
    import ya_vo_amd as yv
    lib = yv.load_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.yv_debug_ess_models.argtypes = [vp, vp, vp, ci, vp, vp, vp]
    lib.yv_debug_ess_models.restype = ci
    lib.yv_debug_ess_solve_poly.argtypes = [ci, vp, ci, vp, vp]
    lib.yv_debug_ess_solve_poly.restype = ci
    return lib


@gpu
@pytest.mark.parametrize("capacity", FORMS)
def test_five_point_models_match_oracle(ctx, oracle, capacity):
    """ess_models_kernel in the workspace's own form on the interleaved families, 64 subsets a launch (a lane-form
    round): the model count and every model of every subset."""
    import torch
    import ya_vo_amd as yv
    lib = _lib()
    q1, q2, fam, models, counts, _ = _five_point(oracle)
    es = yv.Essential(ctx, capacity, 5 * 64)
    d1, d2 = torch.from_numpy(q1.copy()).cuda(), torch.from_numpy(q2.copy()).cuda()
    dm = torch.full((len(q1), 10, 9), 7.0, dtype=torch.float64, device="cuda:0")
    dn = torch.full((len(q1),), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.yv_debug_ess_models(es.handle, d1.data_ptr(), d2.data_ptr(), 65, dm.data_ptr(), dn.data_ptr(), None) != 0
    for k0 in range(0, len(q1), 64):
        assert lib.yv_debug_ess_models(es.handle, d1[k0:].data_ptr(), d2[k0:].data_ptr(), 64, dm[k0:].data_ptr(),
                                       dn[k0:].data_ptr(), None) == 0
    ctx.sync()
    es.close()
    got_n, got = dn.cpu().numpy(), dm.cpu().numpy()
    for k in range(len(q1)):
        what = f"subset {k} ({scene.FIVE_POINT_FAMILIES[fam[k]]})"
        assert got_n[k] == counts[k], what
        assert_same_bits(got[k, :counts[k]], models[k, :counts[k]], what)


@gpu
@pytest.mark.parametrize("group_form", [pytest.param(1, id="group"), pytest.param(0, id="lane")])
def test_solve_poly_matches_oracle(ctx, oracle, group_form):
    """The trim loop and every dk_group<N> / dk_solve<N> against or_solve_poly, degrees interleaved in a wave."""
    import torch
    lib = _lib()
    coeffs, names, roots, _ = _polys(oracle)
    dc = torch.from_numpy(coeffs.copy()).cuda()
    dr = torch.full((len(coeffs), 10, 2), 7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.yv_debug_ess_solve_poly(group_form, dc.data_ptr(), len(coeffs), dr.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = dr.cpu().numpy()
    for k, name in enumerate(names):
        assert_same_bits(got[k], roots[k], name)


def _run_batch(ctx, capacity, pts1, pts2, counts, max_iters=1000, **kw):
    """Essential.find + Essential.recover on lists [P, stride, 2] -> per-list dicts shaped like _reference's."""
    import torch
    import ya_vo_amd as yv
    P, stride = pts1.shape[0], pts1.shape[1]
    dev = "cuda:0"
    d1, d2 = torch.from_numpy(pts1.copy()).to(dev), torch.from_numpy(pts2.copy()).to(dev)
    dc = torch.from_numpy(counts.copy()).to(dev)
    dE = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    dmask = torch.zeros((P, stride), dtype=torch.uint8, device=dev)
    dfound = torch.zeros(P, dtype=torch.int32, device=dev)
    dstats = torch.zeros((P, 3), dtype=torch.int32, device=dev)
    dR = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    dt = torch.zeros((P, 3), dtype=torch.float64, device=dev)
    dgood = torch.zeros(P, dtype=torch.int32, device=dev)
    es = yv.Essential(ctx, capacity, stride, max_iters)
    torch.cuda.synchronize()
    es.find(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), P, stride, dE.data_ptr(), dfound.data_ptr(), dmask.data_ptr(),
            dstats.data_ptr(), FOCAL, PP, **kw)
    es.recover(dE.data_ptr(), d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), P, stride, K_KITTI, dR.data_ptr(),
               dt.data_ptr(), dgood.data_ptr())
    ctx.sync()
    es.close()
    E, found, mask, stats = dE.cpu().numpy(), dfound.cpu().numpy(), dmask.cpu().numpy(), dstats.cpu().numpy()
    R, t, good = dR.cpu().numpy(), dt.cpu().numpy(), dgood.cpu().numpy()
    return [dict(ok=bool(found[p]), E=E[p].reshape(3, 3), mask=mask[p].astype(bool), stats=tuple(int(v) for v in stats[p]),
                 good=int(good[p]), R=R[p].reshape(3, 3), t=t[p]) for p in range(P)]


def _check(got, ref, what):
    n = len(ref["mask"])
    assert got["ok"] == ref["ok"], what
    assert_same_bits(got["E"], ref["E"], f"{what}: E")
    np.testing.assert_array_equal(got["mask"][:n], ref["mask"], err_msg=f"{what}: mask")
    assert not got["mask"][n:].any(), f"{what}: mask past the list"
    if n >= 5:  # a shorter list returns before the statistics are written
        assert got["stats"] == ref["stats"], what
    assert got["good"] == ref["good"], what
    assert_same_bits(got["R"], ref["R"], f"{what}: R")
    assert_same_bits(got["t"], ref["t"], f"{what}: t")


@gpu
@pytest.mark.parametrize("capacity", [pytest.param(8, id="group"), pytest.param(17, id="lane")])
def test_degenerate_lists_match_oracle(ctx, oracle, capacity):
    """Whole lists through Essential.find + Essential.recover: E, the mask, found, the statistics, R, t and good.  The
    group form takes them eight lists a call."""
    names, pts1, pts2, counts, refs = _lists(oracle)
    step = min(capacity, len(names))
    for p0 in range(0, len(names), step):
        got = _run_batch(ctx, capacity, pts1[p0:p0 + step], pts2[p0:p0 + step], counts[p0:p0 + step])
        for i, g in enumerate(got):
            _check(g, refs[p0 + i], names[p0 + i])


@gpu
def test_degenerate_lists_host_match_oracle(ctx, oracle):
    """The same lists through the host drop-ins (yv_find_essential / yv_recover_pose)."""
    names, pts1, pts2, counts, refs = _lists(oracle)
    for p, name in enumerate(names):
        if name in ("count>stride", "count<0"):  # the drop-ins take the length itself
            continue
        n = int(counts[p])
        ok, E, mask = ctx.find_essential(pts1[p, :n], pts2[p, :n], FOCAL, PP)
        good, R, t = ctx.recover_pose(E, pts1[p, :n], pts2[p, :n], K_KITTI)
        ref = refs[p]
        assert ok == ref["ok"], name
        assert_same_bits(E, ref["E"], f"{name}: E")
        np.testing.assert_array_equal(mask, ref["mask"], err_msg=name)
        assert good == ref["good"], name
        assert_same_bits(R, ref["R"], f"{name}: R")
        assert_same_bits(t, ref["t"], f"{name}: t")


@gpu
@pytest.mark.parametrize("capacity", FORMS)
@pytest.mark.parametrize("case", range(len(PARAM_CASES)), ids=[f"{k}={v}" for kw in PARAM_CASES for k, v in kw.items()])
def test_workspace_parameters_match_oracle(ctx, oracle, capacity, case):
    """max_iters 1 / 65 (a second narrow round of one iteration) / 1025 and 3000 (the wide form's sequential draws, RNG
    state carried between rounds), prob and threshold away from 0.999 and 1, on a 300-point, 50 %-outlier list."""
    p1, p2, refs = _param_refs(oracle)
    kw = dict(PARAM_CASES[case])
    max_iters = kw.pop("max_iters", 1000)
    got = _run_batch(ctx, capacity, p1[None], p2[None], np.array([len(p1)], np.int32), max_iters, **kw)
    _check(got[0], refs[case], str(PARAM_CASES[case]))


@gpu
def test_recover_pose_alone_matches_oracle(ctx, oracle):
    """recoverPose on oracle-made E: every candidate wins somewhere, two candidates non-zero at once, the all-tie (pick
    0), E = 0, -E, E^T, and 1 / 16 / 17 points (a wave of rp_count_kernel takes 16)."""
    import torch
    import ya_vo_amd as yv
    cases, refs = _pose_cases(oracle)
    P, stride = len(cases), 64
    pts1, pts2 = np.zeros((P, stride, 2), np.float32), np.zeros((P, stride, 2), np.float32)
    counts, Es = np.zeros(P, np.int32), np.zeros((P, 9))
    for p, (_, E, a, b) in enumerate(cases):
        pts1[p, :len(a)], pts2[p, :len(a)], counts[p], Es[p] = a, b, len(a), E.reshape(9)
    dev = "cuda:0"
    d1, d2, dc, dE = (torch.from_numpy(x).to(dev) for x in (pts1, pts2, counts, Es))
    dR = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    dt = torch.zeros((P, 3), dtype=torch.float64, device=dev)
    dgood = torch.full((P,), -1, dtype=torch.int32, device=dev)
    es = yv.Essential(ctx, P, stride)
    torch.cuda.synchronize()
    es.recover(dE.data_ptr(), d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), P, stride, K_KITTI, dR.data_ptr(),
               dt.data_ptr(), dgood.data_ptr())
    ctx.sync()
    es.close()
    R, t, good = dR.cpu().numpy(), dt.cpu().numpy(), dgood.cpu().numpy()
    for p, (name, _, _, _) in enumerate(cases):
        og, oR, ot, _ = refs[p]
        assert good[p] == og, name
        assert_same_bits(R[p].reshape(3, 3), oR, f"{name}: R")
        assert_same_bits(t[p], ot, f"{name}: t")
