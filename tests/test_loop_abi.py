"""CPU tests of the keyframe store and candidate verification (include/yavo/yavo_loop.h): every yv_loop_* symbol and
its ctypes binding, the layout of yv_loop_result and yv_loop_view against the C compiler's, the argument checks that
come before the context or the object is looked at (no GPU here), and the specification alone (tests/loop_reference.py)
over the CPU oracle on the loop scene (tests/loop_scenes.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv

import loop_reference as ref
import loop_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = yv.YV_ERR_INVALID, yv.YV_ERR_CAPACITY
NAMES = ["yv_loop_create", "yv_loop_destroy", "yv_loop_reset", "yv_loop_count", "yv_loop_set_params",
         "yv_loop_lm_sum_mode", "yv_loop_add", "yv_loop_verify", "yv_loop_add_batch", "yv_loop_verify_batch",
         "yv_loop_view_get", "yv_loop_results_copy"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


def _p(a):
    return a.ctypes.data


def test_symbols_and_bindings(lib):
    hdr = open(os.path.join(ROOT, "include", "yavo", "yavo_loop.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in yv.LOOP_SIGNATURES and name + "(" in hdr, name
    assert '#include "yavo_loop.h"' in open(os.path.join(ROOT, "include", "yavo", "yavo.h")).read()
    from ya_vo_amd import loop
    assert loop.LoopVerifier and loop.lm_sum_mode(1) == yv.track_lm_sum_mode(1)
    assert loop.lm_sum_mode(4096) == yv.track_lm_sum_mode(4096)


def _probe(tmp_path, struct, fields):
    src = tmp_path / f"probe_{struct}.c"
    body = " ".join(f'printf("%zu ", offsetof({struct}, {f}));' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yavo/yavo.h"\n'
                   f'int main(void){{{body} printf("%zu\\n", sizeof({struct})); return 0;}}\n')
    exe = tmp_path / f"probe_{struct}"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_result_and_view_layouts_match_the_compiler(tmp_path):
    dt = yv.LOOP_RESULT_DTYPE
    vals = _probe(tmp_path, "yv_loop_result", list(dt.names))
    assert vals == [dt.fields[f][1] for f in dt.names] + [80] and dt.itemsize == 80
    fields = [f for f, _ in yv._LoopView._fields_]
    vals = _probe(tmp_path, "yv_loop_view", fields)
    assert vals == [getattr(yv._LoopView, f).offset for f in fields] + [ctypes.sizeof(yv._LoopView)]


def test_argument_checks_come_before_the_object(lib):
    """With a NULL context / object: YV_ERR_INVALID for every bad argument that needs neither, then what a missing
    object gives (YV_ERR_NODEVICE on a machine without a GPU, YV_ERR_INVALID with one)."""
    none = yv.YV_ERR_NODEVICE if lib.yv_device_count() == 0 else INVALID
    K = np.ascontiguousarray(sc.K.reshape(9))
    T = sc.T_RIGHT.copy()
    out = ctypes.c_void_p()

    def create(k=K, t=T, max_entries=8, max_problems=4, max_kp=16, o=ctypes.byref(out)):
        return lib.yv_loop_create(None, _p(k) if k is not None else None, _p(t) if t is not None else None,
                                  max_entries, max_problems, max_kp, o)
    assert create() == none
    assert create(k=None) == INVALID and create(t=None) == INVALID and create(o=None) == INVALID
    bad_k, bad_t = K.copy(), T.copy()
    bad_k[4], bad_t[5] = np.nan, np.inf
    assert create(k=bad_k) == INVALID and create(t=bad_t) == INVALID
    for bad in (0, -1, 65537):
        assert create(max_entries=bad) == INVALID
    for bad in (0, 4097):
        assert create(max_problems=bad) == INVALID
    for bad in (0, 4097):
        assert create(max_kp=bad) == INVALID
    assert create(max_entries=65536, max_problems=4096, max_kp=4096) == none

    lib.yv_loop_destroy(None)
    n = ctypes.c_int()
    assert lib.yv_loop_reset(None) == none
    assert lib.yv_loop_count(None, None) == INVALID and lib.yv_loop_count(None, ctypes.byref(n)) == none
    assert lib.yv_loop_lm_sum_mode(1) == lib.yv_track_lm_sum_mode(1)

    draws = ref.pnp.make_draws(64, 0)

    def set_params(flags=3, num=4, den=5, iters=64, d=_p(draws), thr=2.0, min_inl=12):
        return lib.yv_loop_set_params(None, 20, flags, num, den, iters, d, thr, min_inl)
    assert set_params() == none and set_params(flags=0, num=0, den=0) == none and set_params(iters=1) == none
    assert set_params(iters=1024, d=_p(ref.pnp.make_draws(1024, 0))) == none and set_params(min_inl=4) == none
    assert set_params(flags=-1) == INVALID and set_params(flags=4) == INVALID
    assert set_params(num=0) == INVALID and set_params(num=6) == INVALID and set_params(den=32769) == INVALID
    assert set_params(flags=2, num=0, den=0) == none  # the ratio is looked at with YV_MATCH_RATIO only
    assert set_params(iters=0) == INVALID and set_params(iters=1025) == INVALID and set_params(d=None) == INVALID
    assert set_params(thr=0.0) == INVALID and set_params(thr=-1.0) == INVALID and set_params(thr=np.nan) == INVALID
    assert set_params(thr=np.inf) == INVALID and set_params(min_inl=3) == INVALID

    kp = np.zeros(4, yv.KEYPOINT_DTYPE)
    X, has = np.zeros((4, 3)), np.zeros(4, np.uint8)
    assert lib.yv_loop_add(None, _p(kp), 4, _p(X), _p(has), 7) == none
    assert lib.yv_loop_add(None, _p(kp), 4, None, None, 7) == none
    assert lib.yv_loop_add(None, None, 0, None, None, 7) == none
    assert lib.yv_loop_add(None, _p(kp), -1, _p(X), _p(has), 7) == INVALID
    assert lib.yv_loop_add(None, None, 4, _p(X), _p(has), 7) == INVALID
    assert lib.yv_loop_add(None, _p(kp), 4, _p(X), None, 7) == INVALID
    assert lib.yv_loop_add(None, _p(kp), 4, None, _p(has), 7) == INVALID

    ent = np.zeros(2, np.int32)
    res = np.zeros(2, yv.LOOP_RESULT_DTYPE)
    assert lib.yv_loop_verify(None, _p(kp), 4, _p(ent), 2, _p(res)) == none
    assert lib.yv_loop_verify(None, None, 0, _p(ent), 2, _p(res)) == none
    assert lib.yv_loop_verify(None, _p(kp), 4, None, 0, None) == none
    assert lib.yv_loop_verify(None, None, 4, _p(ent), 2, _p(res)) == INVALID
    assert lib.yv_loop_verify(None, _p(kp), -1, _p(ent), 2, _p(res)) == INVALID
    assert lib.yv_loop_verify(None, _p(kp), 4, _p(ent), -1, _p(res)) == INVALID
    assert lib.yv_loop_verify(None, _p(kp), 4, None, 2, _p(res)) == INVALID
    assert lib.yv_loop_verify(None, _p(kp), 4, _p(ent), 2, None) == INVALID

    slots, pairs, fids = np.zeros(2, np.int32), np.ones(2, np.int32), np.zeros(2, np.int64)

    def add_batch(s=_p(slots), p=_p(pairs), f=_p(fids), n_add=2):
        return lib.yv_loop_add_batch(None, None, s, p, f, n_add, None)
    assert add_batch() == none and add_batch(None, None, None, 0) == none
    assert add_batch(n_add=-1) == INVALID and add_batch(s=None) == INVALID and add_batch(p=None) == INVALID
    assert add_batch(f=None) == INVALID

    # (no device memory here: any non-NULL address stands for the candidate arrays, which are not read before the object)
    cand = np.zeros(32, np.int32)

    def verify_batch(s=_p(slots), nq=2, ce=_p(cand), cc=_p(cand), top_k=4):
        return lib.yv_loop_verify_batch(None, None, s, nq, ce, cc, top_k, None)
    assert verify_batch() == none and verify_batch(top_k=1) == none and verify_batch(top_k=16) == none
    assert verify_batch(None, 0, None, None) == none
    assert verify_batch(nq=-1) == INVALID and verify_batch(s=None) == INVALID and verify_batch(ce=None) == INVALID
    assert verify_batch(cc=None) == INVALID and verify_batch(top_k=0) == INVALID and verify_batch(top_k=17) == INVALID

    assert lib.yv_loop_view_get(None, None) == INVALID
    assert lib.yv_loop_view_get(None, ctypes.byref(yv._LoopView())) == none
    assert lib.yv_loop_results_copy(None, -1, _p(res), None) == INVALID
    assert lib.yv_loop_results_copy(None, 2, None, None) == INVALID
    assert lib.yv_loop_results_copy(None, 2, _p(res), None) == none
    assert lib.yv_loop_results_copy(None, 0, None, None) == none


# ---- the specification alone ----
def test_spec_match_filter_is_the_oracles_matcher_and_remove_outliers(oracle):
    """flags 0: j1 / d1 are matchFeatures' and keep is removeOutliers'; the ratio and the mutual check only remove."""
    q, t = sc.keypoints(20)[0], sc.keypoints(0)[0]
    m = oracle.match(q, t)
    d1, j1, d2, rev = ref.knn2(q["featVec"], t["featVec"])
    np.testing.assert_array_equal(t["id"][j1], m["pt2"]["id"])
    np.testing.assert_array_equal(d1, m["distance"])
    keep0, _ = ref.match_robust(q["featVec"], t["featVec"], sc.MATCH_THR, 0, 0, 1)
    kept = oracle.remove_outliers(m, sc.MATCH_THR)
    np.testing.assert_array_equal(q["id"][keep0], kept["pt1"]["id"])
    keep3, _ = ref.match_robust(q["featVec"], t["featVec"], sc.MATCH_THR, 3, 4, 5)
    assert not np.any(keep3 & ~keep0) and 0 < keep3.sum() <= keep0.sum()
    # degenerate lists
    assert ref.match_robust(q["featVec"][:0], t["featVec"], 20, 3, 4, 5)[0].shape == (0,)
    k, j = ref.match_robust(q["featVec"][:5], t["featVec"][:0], 20, 3, 4, 5)
    assert not k.any() and (j == -1).all()


def test_spec_store_and_skips(oracle):
    s = sc.store()
    assert len(s) == sc.N_OUT
    print([(len(e.kp), int(e.has.sum())) for e in s.entries])
    for e in s.entries:
        assert 0 < e.has.sum() < len(e.kp) <= sc.MAX_KP  # some keypoints with a landmark, some without
        assert (e.X[e.has, 2] > 0).all() and not e.X[~e.has].any()
    for i in sorted({e for _, e in sc.PROBLEMS}):  # the keyframes of the table
        e = s.entries[i]
        assert 369 <= len(e.kp) <= 382 and 352 <= e.has.sum() <= 365, i
    P, q = sc.params(3), sc.keypoints(20)[0]
    for bad in (-1, sc.N_OUT, 1000):
        r = ref.verify(oracle, q, s, bad, sc.K, P, 7)
        assert (r.entry, r.n_kept, r.n_edges, r.ransac_inliers, r.lm_inliers, r.verified) == (-1, 0, 0, 0, 0, 0)
        assert r.pose.tobytes() == ref.IDENTITY.tobytes()
    cand = np.full((1, 16), -1, np.int32)
    cand[0, :3] = [0, sc.N_OUT, 10]
    rows = ref.verify_rows(oracle, [q], s, cand, [2], 4, sc.K, P, 7)
    assert [r.entry for r in rows] == [0, -1, -1, -1] and rows[0].verified == 1


@pytest.mark.parametrize("sum_mode", [6, 7])
def test_spec_on_the_loop_scene(sum_mode):
    """What the specification must say about the scene: the revisits are verified against their own places and the
    partially overlapping ones with the scene's translation, and nothing is found where the places share nothing."""
    res = dict(zip(sc.PROBLEMS, sc.reference(3, sum_mode)))
    for key, r in res.items():
        print(key, r.n_kept, r.n_edges, r.ransac_inliers, r.found, r.lm_inliers, r.pose[4:])
    for key in sc.OWN:
        r = res[key]
        assert r.verified == 1 and r.found and r.lm_inliers >= 300 and r.n_kept >= r.n_edges >= r.lm_inliers
        assert np.abs(r.pose[4:] - np.array([-0.0675, -0.27, 0.0])).max() < 1e-3
        assert np.abs(r.pose[:4] - ref.IDENTITY[:4]).max() < 1e-3
    for key in sc.PARTIAL:
        r = res[key]
        assert r.verified == 1 and r.lm_inliers >= 100
    for key in sc.NONE:
        r = res[key]
        assert not r.found and (r.ransac_inliers, r.lm_inliers, r.verified) == (0, 0, 0)
        assert r.pose.tobytes() == ref.IDENTITY.tobytes() and not r.ransac_inlier.any() and not r.lm_outlier.any()
    # flags 0 on a pair of places that share nothing: more matches kept, still nothing found
    r0 = sc.reference(0, sum_mode)[sc.PROBLEMS.index((20, 10))]
    assert r0.n_kept > res[(20, 10)].n_kept and not r0.found and r0.lm_inliers == 0
