"""CPU tests of the scale pyramid (yv_batch_set_pyramid): the symbols are exported and bound, every
argument check answers before the context, ya_vo_amd.pyramid's sizes and quotas keep their invariants, and the numpy
specification of tests/pyramid_reference.py keeps its source positions inside the source."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import pyramid as yp

import pyramid_reference as pr
import rectify_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yv_batch_set_pyramid", "yv_batch_pyramid_view_get", "yv_detect_describe_pyramid", "yv_pyramid_image")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


def _null_ctx_status(lib):
    return yv.YV_ERR_INVALID if lib.yv_device_count() > 0 else yv.YV_ERR_NODEVICE


# ---- surface ----
def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in yv.SIGNATURES, name
    for method in ("set_pyramid", "pyramid_view"):
        assert callable(getattr(yv.Batch, method))
    for method in ("detect_describe_pyramid", "pyramid_image"):
        assert callable(getattr(yv.Context, method))
    assert callable(yp.level_sizes) and callable(yp.level_quotas)
    assert lib.yv_abi_version() == 2


def test_view_struct_matches_the_header(tmp_path):
    src = tmp_path / "probe_pyr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yavo/yavo.h"\n'
                   'int main(void){printf("%d %zu %zu %zu\\n", YV_PYRAMID_MAX_LEVELS, sizeof(yv_batch_pyramid_view),'
                   ' offsetof(yv_batch_pyramid_view, image), offsetof(yv_batch_pyramid_view, level_rc)); return 0;}\n')
    exe = tmp_path / "probe_pyr"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    levels, size, off_image, off_rc = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.split())
    V = yv._BatchPyramidView
    assert levels == pr.MAX_LEVELS == yp.MAX_LEVELS == 8
    assert (size, off_image, off_rc) == (ctypes.sizeof(V), V.image.offset, V.level_rc.offset)


# ---- argument checks, through a NULL context ----
def _ddp(lib, H, W, sizes, keep, n_levels=None, stride=None, img=True, n_out=True, arrays=(True, True)):
    """yv_detect_describe_pyramid(NULL, ...) with output buffers large enough for any accepted call."""
    hw = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    kp = np.ascontiguousarray(np.asarray(keep, np.int32).reshape(-1))
    image = np.zeros((max(H, 1), max(W, 1)), np.uint8)
    out = np.zeros(4096, yv.KEYPOINT_DTYPE)
    level = np.zeros(4096, np.uint8)
    rc = np.zeros((4096, 2), np.int32)
    n = ctypes.c_int(-7)
    st = lib.yv_detect_describe_pyramid(None, image.ctypes.data if img else None, H, W, W if stride is None else stride,
                                        len(hw) if n_levels is None else n_levels,
                                        hw.ctypes.data if arrays[0] else None, kp.ctypes.data if arrays[1] else None,
                                        out.ctypes.data, level.ctypes.data, rc.ctypes.data,
                                        ctypes.byref(n) if n_out else None)
    assert n.value == -7  # nothing is written without a context
    return st


GOOD = dict(H=40, W=64, sizes=[(40, 64), (33, 53), (28, 44)], keep=[100, 60, 40])


def test_host_form_checks_come_before_the_context(lib):
    want = _null_ctx_status(lib)
    inv, cap = yv.YV_ERR_INVALID, yv.YV_ERR_CAPACITY
    assert _ddp(lib, **GOOD) == want
    # the envelope's corners are valid: 8 levels, a shrink of exactly 2 on odd sizes, equal sizes, quotas of 0, the
    # whole keypoint capacity, one level
    assert _ddp(lib, 47, 33, [(47, 33), (24, 17), (12, 9)], [1, 0, 0]) == want
    assert _ddp(lib, 40, 64, [(40, 64)] * 8, [512] * 8) == want
    assert _ddp(lib, 40, 64, [(40, 64)], [4096]) == want
    assert _ddp(lib, 8192, 2048, [(8192, 2048), (4096, 1024)], [10, 10]) == want
    # NULL arrays with more than one level, NULL image / n_out
    assert _ddp(lib, **GOOD, arrays=(False, True)) == inv
    assert _ddp(lib, **GOOD, arrays=(True, False)) == inv
    assert _ddp(lib, **GOOD, img=False) == inv
    assert _ddp(lib, **GOOD, n_out=False) == inv
    assert _ddp(lib, **GOOD, stride=63) == inv
    # more than 8 levels, fewer than 1
    assert _ddp(lib, 40, 64, [(40, 64)] * 9, [1] * 9) == inv
    assert _ddp(lib, 40, 64, [(40, 64)], [1], n_levels=0) == inv
    # increasing sizes, in either axis
    assert _ddp(lib, 40, 64, [(40, 64), (41, 64)], [1, 1]) == inv
    assert _ddp(lib, 40, 64, [(40, 64), (33, 53), (33, 54)], [1, 1, 1]) == inv
    # a shrink of more than 2, in either axis
    assert _ddp(lib, 41, 64, [(41, 64), (20, 32)], [1, 1]) == inv
    assert _ddp(lib, 40, 65, [(40, 65), (20, 32)], [1, 1]) == inv
    # a negative quota
    assert _ddp(lib, 40, 64, GOOD["sizes"], [100, -1, 40]) == inv
    # a level 0 that differs from the image
    assert _ddp(lib, 40, 64, [(40, 63), (33, 53)], [1, 1]) == inv
    assert _ddp(lib, 40, 64, [(39, 64), (33, 53)], [1, 1]) == inv
    # a side below the detector's 9
    assert _ddp(lib, 16, 64, [(16, 64), (8, 32)], [1, 1]) == inv
    # the quotas' sum above the capacity; a level the batch refuses
    assert _ddp(lib, 40, 64, GOOD["sizes"], [4000, 60, 37]) == cap
    assert _ddp(lib, 40, 2049, [(40, 2049), (40, 2048)], [1, 1]) == cap
    assert _ddp(lib, 8193, 64, [(8193, 64), (8192, 64)], [1, 1]) == cap
    # INVALID wins over CAPACITY
    assert _ddp(lib, 40, 64, GOOD["sizes"], [5000, -1, 0]) == inv


def test_batch_form_checks_what_needs_no_batch(lib):
    hw = np.asarray(GOOD["sizes"], np.int32)
    keep = np.asarray(GOOD["keep"], np.int32)

    def call(n, a, b):
        return lib.yv_batch_set_pyramid(None, n, a.ctypes.data if a is not None else None,
                                        b.ctypes.data if b is not None else None)

    inv = yv.YV_ERR_INVALID
    assert call(3, None, keep) == inv and call(3, hw, None) == inv and call(3, None, None) == inv
    assert call(9, np.tile(hw[:1], (9, 1)), np.ones(9, np.int32)) == inv
    assert call(2, np.asarray([(40, 64), (41, 64)], np.int32), keep) == inv
    assert call(2, np.asarray([(40, 64), (19, 64)], np.int32), keep) == inv
    assert call(3, hw, np.asarray([1, -1, 1], np.int32)) == inv
    assert call(3, hw, np.asarray([4000, 90, 7], np.int32)) == yv.YV_ERR_CAPACITY
    assert call(2, np.asarray([(40, 2049), (40, 2048)], np.int32), keep) == yv.YV_ERR_CAPACITY
    # valid arguments, and switching it off: what is left is the NULL batch
    assert call(3, hw, keep) == inv
    assert call(0, None, None) == inv and call(1, hw, keep) == inv
    v = yv._BatchPyramidView()
    assert lib.yv_batch_pyramid_view_get(None, ctypes.byref(v)) == inv


def test_pyramid_image_checks_come_before_the_context(lib):
    src = np.zeros((64, 64), np.uint8)
    dst = np.zeros((64, 64), np.uint8)

    def call(sh=40, sw=64, ss=64, dh=33, dw=53, ds=64, s=True, d=True):
        return lib.yv_pyramid_image(None, src.ctypes.data if s else None, sh, sw, ss, dh, dw,
                                    dst.ctypes.data if d else None, ds)

    inv, want = yv.YV_ERR_INVALID, _null_ctx_status(lib)
    assert call() == want and call(dh=40, dw=64) == want and call(dh=20, dw=32) == want
    assert call(sh=1, sw=1, ss=1, dh=1, dw=1) == want
    assert call(s=False) == inv and call(d=False) == inv
    assert call(dh=41) == inv and call(dw=65, ds=65) == inv  # larger than the source
    assert call(dh=19) == inv and call(dw=31) == inv          # less than half of it
    assert call(dh=0) == inv and call(dw=0) == inv
    assert call(ss=63) == inv and call(ds=52) == inv
    assert call(sh=8193, dh=8192) == inv


# ---- ya_vo_amd.pyramid ----
@pytest.mark.parametrize("H,W", [(376, 1241), (120, 360), (9, 9), (10, 4000), (37, 53), (8192, 2048)])
@pytest.mark.parametrize("scale", [1.0, 1.2, 1.5, 2.0, 3.0])
def test_level_sizes_keep_the_rule(H, W, scale):
    for n in range(1, 9):
        sizes = yp.level_sizes(H, W, n, scale)
        assert len(sizes) == n and sizes[0] == (H, W)
        pr.check_sizes(sizes)
        assert sizes == yp.level_sizes(H, W, 8, scale)[:n]  # a level does not depend on the levels after it
    if scale == 1.2 and (H, W) == (376, 1241):
        assert yp.level_sizes(H, W, 4) == [(376, 1241), (313, 1034), (261, 862), (218, 718)]
    if scale == 1.0:
        assert all(s == (H, W) for s in yp.level_sizes(H, W, 8, scale))


def test_level_sizes_refuse_bad_arguments():
    for bad in ((40, 64, 0), (40, 64, 9), (8, 64, 2), (40, 8, 2)):
        with pytest.raises(ValueError):
            yp.level_sizes(*bad)
    with pytest.raises(ValueError):
        yp.level_sizes(40, 64, 2, 0.9)


@pytest.mark.parametrize("max_kp", [0, 1, 7, 500, 2000, 4096])
def test_level_quotas_sum_to_max_kp(max_kp):
    for H, W in ((376, 1241), (120, 360), (9, 9)):
        for n in (1, 2, 4, 8):
            sizes = yp.level_sizes(H, W, n)
            q = yp.level_quotas(max_kp, sizes)
            assert len(q) == n and sum(q) == max_kp and min(q) >= 0
            # area-proportional, rounded down, the remainder to level 0
            total = sum(h * w for h, w in sizes)
            assert q[1:] == [max_kp * h * w // total for h, w in sizes[1:]]
            assert q[0] >= max_kp * sizes[0][0] * sizes[0][1] // total


# ---- the specification ----
def test_source_positions_stay_inside_the_source():
    """Exhaustive over 9 <= H_l <= H_(l-1) <= 2 H_l <= 64: every position lies in [0, (n_src - 1) * 32], grows with the
    index, and a tap one past the end carries weight 0; the box of any 16 (128) destination rows (columns) spans at most
    33 (257) source rows (columns), the kernel's LDS box."""
    for nd in range(9, 33):
        for ns in range(nd, min(2 * nd, 64) + 1):
            q = pr.src_pos(ns, nd)
            assert q.min() >= 0 and q.max() <= (ns - 1) * 32
            assert np.all(np.diff(q) >= 32) and np.all(np.diff(q) <= 64)
            i, a = q >> 5, q & 31
            assert np.all((i + 1 <= ns - 1) | (a == 0))
            # the closed form before the clamp, with Python's integers
            raw = [((2 * r + 1) * ns - nd) * 16 // nd for r in range(nd)]
            assert min(raw) >= 0 and list(q) == [min(v, (ns - 1) * 32) for v in raw]
            for r in range(0, nd, 16):
                last = min(r + 16, nd) - 1
                assert min(i[last] + 1, ns - 1) - i[r] + 1 <= 33
    # the widest tile: 128 columns at a shrink of exactly 2 and just below it
    for nd, ns in ((1024, 2048), (1025, 2048), (640, 1241)):
        i = pr.src_pos(ns, nd) >> 5
        for c in range(0, nd, 128):
            last = min(c + 128, nd) - 1
            assert min(i[last] + 1, ns - 1) - i[c] + 1 <= 257


def test_equal_sizes_are_the_identity_and_a_half_is_the_box_mean():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (24, 40), dtype=np.uint8)
    assert np.array_equal(pr.resample(img, 24, 40), img)
    assert np.array_equal(pr.src_pos(40, 40), 32 * np.arange(40))
    # a shrink of exactly 2 samples the centre of every 2 x 2 block: the rounded mean of its four pixels
    s = img.astype(np.int64)
    mean = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(pr.resample(img, 12, 20), mean.astype(np.uint8))


@pytest.mark.parametrize("shape,dst", [((24, 40), (20, 33)), ((33, 47), (17, 24)), ((16, 9), (9, 9))])
def test_resample_is_the_pixelwise_form_and_the_remap_of_its_map(shape, dst):
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    out = pr.resample(img, *dst)
    assert np.array_equal(out, pr.resample_slow(img, *dst))
    assert np.array_equal(out, rr.remap(img, pr.level_map(*shape, *dst)))


def test_merge_order_ids_and_mapping():
    sizes = [(40, 64), (33, 53), (20, 27)]
    per = []
    for l, n in enumerate((3, 0, 2)):
        k = np.zeros(n, yv.KEYPOINT_DTYPE)
        k["x"], k["y"], k["id"] = np.arange(n) + 10, np.arange(n) + 5, np.arange(n) * 7
        k["matched"] = 1 if l else 0
        k["featVec"] = l + 1
        per.append(k)
    m, level, rc = pr.merge(per, sizes)
    assert list(level) == [0, 0, 0, 2, 2] and list(m["id"]) == [0, 7, 14, 3, 4]
    assert list(m["matched"]) == [0] * 5 and list(m["featVec"][:, 0]) == [1, 1, 1, 3, 3]
    assert rc.tolist() == [[10, 5], [11, 6], [12, 7], [10, 5], [11, 6]]
    assert list(m["x"][3:]) == [(2 * 10 + 1) * 40 // 40, (2 * 11 + 1) * 40 // 40]
    assert list(m["y"][3:]) == [(2 * 5 + 1) * 64 // 54, (2 * 6 + 1) * 64 // 54]
    # the mapping lands inside level 0, at the pixel that holds the level pixel's centre
    for n0, nl in ((40, 20), (41, 21), (1241, 718), (9, 9)):
        x = pr.to_level0(np.arange(nl), n0, nl)
        assert x.min() >= 0 and x.max() <= n0 - 1 and np.all(np.diff(x) >= 1)
        assert np.array_equal(x, np.floor((np.arange(nl) + 0.5) * n0 / nl).astype(np.int64))
