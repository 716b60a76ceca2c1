"""CPU tests of the 2-NN match filter's boundary (include/yavo/yavo.h): the new symbols are exported and bound, the
record and view layouts agree with the C compiler, and the argument checks answer before any device work."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yv_match_knn2", "yv_match_robust", "yv_batch_set_match_filter", "yv_batch_match2_view_get")
K_MAX_KP = 4096


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in yv.SIGNATURES, name
    # the fifth public name of the feature: the record type, on both sides of the boundary
    assert yv.MATCH2_DTYPE.names == ("d1", "j1", "d2", "j2")
    assert (yv.YV_MATCH_RATIO, yv.YV_MATCH_MUTUAL) == (1, 2)
    for method in ("match_knn2", "match_robust"):
        assert callable(getattr(yv.Context, method))
    for method in ("set_match_filter", "match2_view"):
        assert callable(getattr(yv.Batch, method))


def test_match2_layouts_match_the_c_compiler(tmp_path):
    fields = [f for f, _ in yv._BatchMatch2View._fields_]
    assert fields == ["nn2", "rev", "keep"]
    body = " ".join(f'printf("%zu ", offsetof(yv_batch_match2_view, {f}));' for f in fields)
    rec = " ".join(f'printf("%zu ", offsetof(yv_match2, {f}));' for f in ("d1", "j1", "d2", "j2"))
    src = tmp_path / "probe_match2.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yavo/yavo.h"\n'
                   f'int main(void){{printf("%zu ", sizeof(yv_match2)); {rec} {body} '
                   'printf("%zu %d %d\\n", sizeof(yv_batch_match2_view), YV_MATCH_RATIO, YV_MATCH_MUTUAL); return 0;}\n')
    exe = tmp_path / "probe_match2"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    md = yv.MATCH2_DTYPE
    expect = ([16] + [md.fields[f][1] for f in ("d1", "j1", "d2", "j2")] +
              [getattr(yv._BatchMatch2View, f).offset for f in fields] +
              [ctypes.sizeof(yv._BatchMatch2View), yv.YV_MATCH_RATIO, yv.YV_MATCH_MUTUAL])
    assert md.itemsize == 16 and vals[0] == 16
    assert vals == expect


def _robust(lib, nq=1, nt=1, flags=0, num=4, den=5, ctx=None):
    """yv_match_robust on valid dummy buffers (never read: every case returns before device work)."""
    q = np.zeros(1, yv.KEYPOINT_DTYPE)
    out = np.zeros(1, yv.MATCH_DTYPE)
    n = ctypes.c_int(-7)
    return lib.yv_match_robust(ctx, q.ctypes.data, nq, q.ctypes.data, nt, 20, flags, num, den, out.ctypes.data,
                               ctypes.byref(n), None)


def test_flags_outside_0_to_3_are_invalid(lib):
    for flags in (-1, 4, 7, 1 << 20):
        assert _robust(lib, flags=flags) == yv.YV_ERR_INVALID
        assert lib.yv_batch_set_match_filter(None, flags, 4, 5) == yv.YV_ERR_INVALID


def test_ratio_must_satisfy_0_lt_num_le_den_le_32768(lib):
    for num, den in ((0, 5), (-1, 5), (6, 5), (4, 0), (1, 32769), (32769, 32769)):
        for flags in (yv.YV_MATCH_RATIO, yv.YV_MATCH_RATIO | yv.YV_MATCH_MUTUAL):
            assert _robust(lib, flags=flags, num=num, den=den) == yv.YV_ERR_INVALID, (num, den)
            assert lib.yv_batch_set_match_filter(None, flags, num, den) == yv.YV_ERR_INVALID, (num, den)


def test_capacity_is_checked_before_the_device(lib):
    q = np.zeros(1, yv.KEYPOINT_DTYPE)
    out = np.zeros(1, yv.MATCH2_DTYPE)
    for nq, nt in ((K_MAX_KP + 1, 1), (1, K_MAX_KP + 1)):
        assert _robust(lib, nq=nq, nt=nt, flags=3) == yv.YV_ERR_CAPACITY
        assert lib.yv_match_knn2(None, q.ctypes.data, nq, q.ctypes.data, nt, out.ctypes.data, None) == \
            yv.YV_ERR_CAPACITY
    assert lib.yv_match_knn2(None, q.ctypes.data, -1, q.ctypes.data, 1, out.ctypes.data, None) == yv.YV_ERR_INVALID
    assert lib.yv_match_knn2(None, None, 1, q.ctypes.data, 1, out.ctypes.data, None) == yv.YV_ERR_INVALID


def test_valid_arguments_without_a_context(lib):
    # in-range arguments: the ratio bounds themselves are accepted; what is left is the missing context, which is
    # "no usable GPU" on a machine without one (no CPU path) and a plain bad argument where a GPU exists
    expect = yv.YV_ERR_NODEVICE if lib.yv_device_count() == 0 else yv.YV_ERR_INVALID
    for flags, num, den in ((0, 0, 0), (2, 0, 0), (1, 1, 1), (3, 32768, 32768), (1, 1, 32768), (3, 4, 5)):
        assert _robust(lib, flags=flags, num=num, den=den) == expect, (flags, num, den)
    q = np.zeros(1, yv.KEYPOINT_DTYPE)
    out = np.zeros(1, yv.MATCH2_DTYPE)
    assert lib.yv_match_knn2(None, q.ctypes.data, 1, q.ctypes.data, 1, out.ctypes.data, None) == expect


def test_batch_calls_reject_a_null_batch(lib):
    assert lib.yv_batch_set_match_filter(None, 0, 0, 0) == yv.YV_ERR_INVALID
    assert lib.yv_batch_set_match_filter(None, 3, 4, 5) == yv.YV_ERR_INVALID
    v = yv._BatchMatch2View()
    assert lib.yv_batch_match2_view_get(None, ctypes.byref(v)) == yv.YV_ERR_INVALID
