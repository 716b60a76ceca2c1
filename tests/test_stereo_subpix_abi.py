"""CPU tests of the sub-pixel stereo refinement (yv_stereo_subpix, yv_triangulate_subpix, yv_batch_set_stereo_subpix,
yv_batch_subpix_view_get): the symbols are exported and bound, every argument check answers before the context, the
view struct agrees with ctypes, and the numpy specification of tests/stereo_subpix_reference.py gives the stated
results on hand-made images and has the property the feature is for: on a fixture with a known sub-pixel disparity
the refined column is within a quarter pixel of the truth, and the depth triangulated from it is closer to f b / d than
the depth from the integer column."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd.scene import K_KITTI

import stereo_subpix_reference as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yv_stereo_subpix", "yv_batch_set_stereo_subpix", "yv_batch_subpix_view_get")
T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


# ---- surface ----
def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in yv.SIGNATURES, name
    assert hasattr(lib, "yv_triangulate_subpix") and "yv_triangulate_subpix" in yv.GEOM_SIGNATURES
    for cls, method in ((yv.Context, "stereo_subpix"), (yv.Context, "triangulate"), (yv.Batch, "set_stereo_subpix"),
                        (yv.Batch, "subpix_view")):
        assert callable(getattr(cls, method))
    assert (yv.YV_SUBPIX_NONE, yv.YV_SUBPIX_OK, yv.YV_SUBPIX_OUTSIDE, yv.YV_SUBPIX_EDGE) == (0, 1, 2, 3)
    assert (ssr.NONE, ssr.OK, ssr.OUTSIDE, ssr.EDGE) == (0, 1, 2, 3)
    assert yv.YV_SUBPIX_DROP_EDGE == 1
    assert lib.yv_abi_version() == 2


def test_header_constants_match_the_binding(tmp_path):
    src = tmp_path / "probe_const.c"
    src.write_text('#include <stdio.h>\n#include "yavo/yavo.h"\n'
                   'int main(void){printf("%d %d %d %d %d\\n", YV_SUBPIX_NONE, YV_SUBPIX_OK, YV_SUBPIX_OUTSIDE, '
                   'YV_SUBPIX_EDGE, YV_SUBPIX_DROP_EDGE); return 0;}\n')
    exe = tmp_path / "probe_const"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == [0, 1, 2, 3, 1]


def test_subpix_view_layout_matches_ctypes(tmp_path):
    fields = [f for f, _ in yv._BatchSubpixView._fields_]
    assert fields == ["dcol_q8", "sad", "status"]
    src = tmp_path / "probe_subpix.c"
    body = " ".join(f'printf("%zu ", offsetof(yv_batch_subpix_view, {f}));' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yavo/yavo.h"\n'
                   f'int main(void){{{body} printf("%zu\\n", sizeof(yv_batch_subpix_view)); return 0;}}\n')
    exe = tmp_path / "probe_subpix"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == [getattr(yv._BatchSubpixView, f).offset for f in fields] + [ctypes.sizeof(yv._BatchSubpixView)]


def _null_ctx_status(lib):
    """What a fully valid call answers for the NULL context."""
    return yv.YV_ERR_INVALID if lib.yv_device_count() > 0 else yv.YV_ERR_NODEVICE


def _call(lib, H=40, W=64, stride=None, rc1=((20, 30), (7, 15)), rc2=((20, 26), (7, 15)), n=None, w=5, s=3, null=None):
    img = np.zeros((max(H, 1), max(W, 1)), np.uint8)
    m = ssr.make_matches(rc1, rc2)
    n = len(m) if n is None else n
    buf = m if len(m) else np.zeros(1, yv.MATCH_DTYPE)
    dq, sad = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    st = np.zeros(max(n, 1), np.uint8)
    a = {"left": img.ctypes.data, "right": img.ctypes.data, "m": buf.ctypes.data, "dcol_q8": dq.ctypes.data,
         "sad": sad.ctypes.data, "status": st.ctypes.data}
    if null:
        a[null] = None
    return lib.yv_stereo_subpix(None, a["left"], a["right"], H, W, W if stride is None else stride, a["m"], n, w, s,
                                a["dcol_q8"], a["sad"], a["status"])


def test_arguments_are_checked_before_the_context(lib):
    for name in ("left", "right", "m", "dcol_q8", "sad", "status"):
        assert _call(lib, null=name) == yv.YV_ERR_INVALID, name
    assert _call(lib, n=-1) == yv.YV_ERR_INVALID
    assert _call(lib, H=8) == yv.YV_ERR_INVALID
    assert _call(lib, W=8) == yv.YV_ERR_INVALID
    assert _call(lib, stride=63) == yv.YV_ERR_INVALID
    for w in (0, -1, 8, 2 ** 31 - 1):
        assert _call(lib, w=w) == yv.YV_ERR_INVALID, w
    for s in (0, -1, 9, 2 ** 31 - 1):
        assert _call(lib, s=s) == yv.YV_ERR_INVALID, s
    for pos in ((-1, 5), (5, -1), (40, 5), (5, 64), (2 ** 31 - 1, 0), (0, -2 ** 31)):
        assert _call(lib, rc1=[(5, 6), pos], rc2=[(5, 6), (5, 6)]) == yv.YV_ERR_INVALID, pos
        assert _call(lib, rc1=[(5, 6), (5, 6)], rc2=[pos, (5, 6)]) == yv.YV_ERR_INVALID, pos


def test_capacity_is_checked_before_the_context(lib):
    rc = np.zeros((4097, 2), np.int32)
    assert _call(lib, rc1=rc, rc2=rc) == yv.YV_ERR_CAPACITY
    # valid calls, the largest list and the envelope's corners included: what is left is the NULL context
    want = _null_ctx_status(lib)
    assert _call(lib, rc1=rc[:4096], rc2=rc[:4096]) == want
    assert _call(lib) == want
    assert _call(lib, H=9, W=9, rc1=[(0, 0), (8, 8)], rc2=[(8, 8), (0, 0)], w=7, s=8) == want
    assert _call(lib, w=1, s=1, stride=200) == want
    assert _call(lib, rc1=[], rc2=[], n=0) == want
    assert lib.yv_stereo_subpix(None, None, None, 9, 9, 9, None, 0, 5, 3, None, None, None) == want  # n = 0


def test_batch_calls_and_triangulate_with_null_handles(lib):
    idx = np.zeros(1, np.int32)
    assert lib.yv_batch_set_stereo_subpix(None, idx.ctypes.data, 1, 5, 3, 0) == yv.YV_ERR_INVALID
    assert lib.yv_batch_set_stereo_subpix(None, None, 0, 5, 3, 0) == yv.YV_ERR_INVALID
    v = yv._BatchSubpixView()
    assert lib.yv_batch_subpix_view_get(None, ctypes.byref(v)) == yv.YV_ERR_INVALID
    n = ctypes.c_int()
    assert lib.yv_triangulate_subpix(None, None, None, None, None, None, 0, None, None,
                                     ctypes.byref(n)) == yv.YV_ERR_INVALID


# ---- hand-made cases for the specification ----
def _one(L, R, r, c, r2, c2, w, s):
    dq, sad, st = ssr.subpix(L, R, [(r, c)], [(r2, c2)], w, s)
    return int(dq[0]), int(sad[0]), int(st[0])


@pytest.mark.parametrize("w,s", [(1, 1), (5, 3), (7, 8)])
def test_constant_image(w, s):
    L = np.full((40, 64), 77, np.uint8)
    assert _one(L, L, 20, 30, 18, 32, w, s) == (0, 0, ssr.OK)
    # den = 0 with a nonzero SAD: every shift costs the same, k* = 0, frac = 0
    R = np.full((40, 64), 87, np.uint8)
    assert _one(L, R, 20, 30, 20, 30, w, s) == (0, 10 * (2 * w + 1) ** 2, ssr.OK)


@pytest.mark.parametrize("w,s", [(1, 1), (5, 3), (7, 8)])
def test_column_ramp_runs_to_the_edge_of_the_bracket(w, s):
    c = np.arange(64, dtype=np.int64)
    L = np.broadcast_to((3 * c + 60).astype(np.uint8), (40, 64)).copy()
    R = np.broadcast_to((3 * c).astype(np.uint8), (40, 64)).copy()
    n2 = (2 * w + 1) ** 2
    # SAD_k = n^2 |60 - 3 k|: falls all the way to k = +s
    assert _one(L, R, 20, 30, 20, 30, w, s) == (0, n2 * (60 - 3 * s), ssr.EDGE)
    assert _one(R, L, 20, 30, 20, 30, w, s) == (0, n2 * (60 - 3 * s), ssr.EDGE)  # and to k = -s


def test_period_two_columns_resolve_ties_in_the_stated_order():
    c = np.arange(64, dtype=np.int64)
    L = np.broadcast_to((100 + 50 * (c % 2)).astype(np.uint8), (40, 64)).copy()
    assert ssr.search_order(3) == [0, -1, 1, -2, 2, -3, 3]
    # in phase: SAD = 0 at k = 0, +-2: k* = 0, a = c: frac = 0
    assert _one(L, L, 20, 30, 20, 30, 5, 3) == (0, 0, ssr.OK)
    # out of phase: SAD = 0 at k = -1, +1, -3, +3: the first in the order is -1
    assert _one(L, L, 20, 30, 20, 31, 5, 3) == (-256, 0, ssr.OK)
    assert _one(L, L, 20, 30, 20, 31, 5, 2) == (-256, 0, ssr.OK)
    assert _one(L, L, 20, 30, 20, 31, 5, 1) == (0, 0, ssr.EDGE)


def test_parabola_vertex_rounds_half_up_and_floors():
    # one bright column in L, the same column one to the right in R plus a weaker copy beside it
    L = np.zeros((40, 64), np.uint8)
    R = np.zeros((40, 64), np.uint8)
    L[:, 30] = 200
    R[:, 31] = 200
    dq, sad, st = _one(L, R, 20, 30, 20, 30, 2, 3)
    assert (dq, sad, st) == (256, 0, ssr.OK)  # a = c: the vertex sits on k* = 1
    R[:, 32] = 40
    s = ssr.sads(L, R, 20, 30, 20, 30, 2, 3)
    a, b, cc = s[0], s[1], s[2]
    den = a + cc - 2 * b
    want = (256 * (a - cc) + den) // (2 * den)
    assert _one(L, R, 20, 30, 20, 30, 2, 3) == (256 + want, b, ssr.OK)
    assert want != 0 and -128 <= want <= 128
    # the mirrored scene gives the mirrored vertex up to the rounding: floor((x + 1/2)) and floor((-x + 1/2))
    dq_m, _, _ = _one(L[:, ::-1].copy(), R[:, ::-1].copy(), 20, 33, 20, 33, 2, 3)
    assert dq_m in (-(256 + want), -(256 + want) + 1)


BORDERS = [  # (name, the match that touches the border exactly, the step that crosses it)
    ("r - w >= 0", lambda H, W, w, s: (w, 30, 20, 30), (-1, 0, 0, 0)),
    ("r + w < H", lambda H, W, w, s: (H - 1 - w, 30, 20, 30), (1, 0, 0, 0)),
    ("c - w >= 0", lambda H, W, w, s: (20, w, 20, 30), (0, -1, 0, 0)),
    ("c + w < W", lambda H, W, w, s: (20, W - 1 - w, 20, 30), (0, 1, 0, 0)),
    ("r2 - w >= 0", lambda H, W, w, s: (20, 30, w, 30), (0, 0, -1, 0)),
    ("r2 + w < H", lambda H, W, w, s: (20, 30, H - 1 - w, 30), (0, 0, 1, 0)),
    ("c2 - s - w >= 0", lambda H, W, w, s: (20, 30, 20, s + w), (0, 0, 0, -1)),
    ("c2 + s + w < W", lambda H, W, w, s: (20, 30, 20, W - 1 - s - w), (0, 0, 0, 1)),
]


@pytest.mark.parametrize("w,s", [(1, 1), (5, 3), (7, 8)])
@pytest.mark.parametrize("name,touch,step", BORDERS, ids=[b[0] for b in BORDERS])
def test_footprint_touching_and_crossing_every_border(name, touch, step, w, s):
    H, W = 41, 67
    img = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
    t = touch(H, W, w, s)
    assert ssr.inside(H, W, *t, w, s), name
    assert _one(img, img, *t, w, s)[2] != ssr.OUTSIDE
    x = tuple(a + b for a, b in zip(t, step))
    assert not ssr.inside(H, W, *x, w, s), name
    assert _one(img, img, *x, w, s) == (0, -1, ssr.OUTSIDE)


def test_smallest_image_has_exactly_the_footprints_that_fit():
    img = np.random.default_rng(6).integers(0, 256, (9, 9), dtype=np.uint8)
    # the same image: SAD_0 = 0 comes first in the order, so k* = 0 and only the vertex moves with a - c
    for w, s in ((1, 1), (2, 2), (3, 1), (1, 3)):
        dq, sad, st = _one(img, img, 4, 4, 4, 4, w, s)
        assert (sad, st) == (0, ssr.OK) and abs(dq) <= 128, (w, s)
    assert _one(img, img, 4, 4, 4, 4, 2, 3)[2] == ssr.OUTSIDE
    assert _one(img, img, 4, 4, 4, 4, 5, 1)[2] == ssr.OUTSIDE


@pytest.mark.parametrize("w,s", [(1, 1), (2, 2), (5, 3), (7, 8)])
def test_the_array_form_is_the_written_specification(w, s):
    """ssr.subpix (all matches at once, what the GPU tests compare against) equals ssr.subpix_one match by match, on
    noise with every status present and on the period-2 columns with their ties."""
    rng = np.random.default_rng(100 * w + s)
    H, W = 48, 90
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = np.roll(L, -3, axis=1) // 2 + rng.integers(0, 128, (H, W), dtype=np.uint8)
    n = 400
    rc1 = np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1)
    rc2 = rc1 + np.stack([rng.integers(-2, 3, n), rng.integers(-6, 1, n)], 1)
    rc2 = np.clip(rc2, 0, [H - 1, W - 1])
    got, want = ssr.subpix(L, R, rc1, rc2, w, s), ssr.subpix_slow(L, R, rc1, rc2, w, s)
    for g, x in zip(got, want):
        np.testing.assert_array_equal(g, x)
    assert set(np.unique(got[2]).tolist()) >= ({ssr.OK, ssr.OUTSIDE, ssr.EDGE} if s > 1 else {ssr.OUTSIDE, ssr.EDGE})
    P = np.broadcast_to((100 + 50 * (np.arange(W) % 2)).astype(np.uint8), (H, W)).copy()
    for g, x in zip(ssr.subpix(P, P, rc1, rc2, w, s), ssr.subpix_slow(P, P, rc1, rc2, w, s)):
        np.testing.assert_array_equal(g, x)


# ---- accuracy on the fixture with a known sub-pixel disparity ----
DQS = (32, 33, 34, 35, 37, 50)


@pytest.fixture(scope="module")
def fixtures():
    return {dq: (ssr.disparity_pair(dq), ssr.disparity_points(dq)) for dq in DQS}


def _errors(fix, w, s):
    (left, right), (rc1, rc2, true_c2) = fix
    dq8, _, st = ssr.subpix(left, right, rc1, rc2, w, s)
    err = np.abs(ssr.refined_column(rc2[:, 1], dq8) - true_c2)
    start = np.abs(rc2[:, 1] - true_c2)
    return st, err, start


@pytest.mark.parametrize("dq", DQS)
def test_refined_column_is_within_a_quarter_pixel_of_the_truth(fixtures, dq):
    """The bounds are the issue's: every point OK, every error below 0.25 px (the fixture's own disparity step), the
    mean below 0.12 px, against an integer start that is more than half a pixel off on average.  Measured with the
    committed fixture at (w, s) = (5, 3) over dq = 32, 33, 34, 35, 37, 50: mean error 0.012-0.088 px, maximum
    0.047-0.145 px, the start's mean 0.677-0.840 px (the figures per dq are printed).  The image statistics are 128.2 /
    54.5: the clip to [0, 255] takes 2.5 % of the pixels and a little of the standard deviation."""
    left, right = fixtures[dq][0]
    assert left.shape == (ssr.FIX_H, ssr.FIX_W) and abs(float(left.mean()) - 128) < 1 and abs(float(left.std()) - 56) < 2
    st, err, start = _errors(fixtures[dq], 5, 3)
    print(f"dq {dq} (5, 3): OK {int((st == ssr.OK).sum())}/{len(st)}, mean {err.mean():.4f}, max {err.max():.4f}, "
          f"start mean {start.mean():.4f}")
    assert (st == ssr.OK).all()
    assert err.max() < 0.25
    assert err.mean() < 0.12
    assert start.mean() > 0.5


@pytest.mark.parametrize("dq", DQS)
def test_the_widest_window_and_range_find_the_same_minimum(fixtures, dq):
    """Measured at (7, 8): every point OK, maximum error 0.027-0.121 px."""
    st, err, _ = _errors(fixtures[dq], 7, 8)
    print(f"dq {dq} (7, 8): OK {int((st == ssr.OK).sum())}/{len(st)}, mean {err.mean():.4f}, max {err.max():.4f}")
    assert (st == ssr.OK).all()
    assert err.max() < 0.25


def test_refined_depth_is_closer_to_f_b_over_d(oracle, fixtures):
    """True disparity 8.25 px under KITTI's geometry: Z = f b / d = 47.05 m.  The share of the points whose refined Z
    is closer to it than the Z of the integer column is asserted to be at least 95 % (measured: 300 of 300; mean |Z - Z true| 0.50 m refined, 4.65 m integer)."""
    (left, right), (rc1, rc2, _) = fixtures[33]
    dq8, _, st = ssr.subpix(left, right, rc1, rc2, 5, 3)
    assert (st == ssr.OK).all()
    m = ssr.make_matches(rc1, rc2)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    Xi, oki = ssr.triangulate_refined(oracle, ident, T_RIGHT, K_KITTI, m)
    Xr, okr = ssr.triangulate_refined(oracle, ident, T_RIGHT, K_KITTI, m, dq8)
    assert oki.all() and okr.all()
    z_true = float(np.asarray(K_KITTI).reshape(3, 3)[1, 1]) * 0.54 / 8.25
    closer = np.abs(Xr[:, 2] - z_true) < np.abs(Xi[:, 2] - z_true)
    print(f"Z true {z_true:.3f} m: refined closer for {closer.mean():.4f} of {len(closer)} points; mean |dZ| refined "
          f"{np.abs(Xr[:, 2] - z_true).mean():.3f} m, integer {np.abs(Xi[:, 2] - z_true).mean():.3f} m")
    assert closer.mean() >= 0.95
    # the integer arm is the oracle's own triangulate_matches, bit for bit
    _, X0, ok0 = oracle.triangulate_matches(ident, T_RIGHT, K_KITTI, m)
    assert X0.tobytes() == Xi.tobytes() and np.array_equal(ok0, oki)
