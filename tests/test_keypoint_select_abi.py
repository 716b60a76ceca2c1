"""CPU tests of the keypoint selection's boundary (include/yavo/yavo.h): the two symbols are exported and bound, the
Python methods exist, and every argument check answers before any device work and before the context is looked at."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yv_set_keypoint_select", "yv_select_corners")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in yv.SIGNATURES, name
    assert callable(getattr(yv.Context, "set_keypoint_select"))
    assert callable(getattr(yv.Context, "select_corners"))
    assert lib.yv_abi_version() == 2


BAD_SETTINGS = [(-1, 0, 0, 0), (9, 0, 0, 0), (2 ** 31 - 1, 0, 0, 0), (0, 32, 32, -1), (0, 32, 32, 4097),
                (0, 7, 32, 1), (0, 32, 7, 1), (0, 8193, 32, 1), (0, 32, 8193, 1), (0, 0, 0, 1), (3, -5, 32, 2),
                (8, 32, 32, 2 ** 31 - 1)]
GOOD_SETTINGS = [(0, 0, 0, 0), (8, 0, 0, 0), (1, -7, 99999, 0), (0, 8, 8, 1), (0, 8192, 8192, 4096), (3, 32, 32, 5),
                 (2, 47, 61, 3)]


def test_setting_ranges_are_checked_before_the_context(lib):
    for s in BAD_SETTINGS:
        assert lib.yv_set_keypoint_select(None, *s) == yv.YV_ERR_INVALID, s
    # valid values: what is left is the NULL context (with per_cell == 0 the cell sides are ignored)
    for s in GOOD_SETTINGS:
        assert lib.yv_set_keypoint_select(None, *s) == yv.YV_ERR_INVALID, s


def _select(lib, H=40, W=64, rc=None, resp=None, n=None, max_kp=100, null=None):
    """yv_select_corners with a NULL context on small valid buffers; `null` names one pointer to pass as NULL."""
    rc = np.array([[5, 6], [20, 30]], np.int32) if rc is None else np.ascontiguousarray(rc, np.int32)
    resp = np.ones(max(len(rc), 1), np.float32) if resp is None else resp
    n = len(rc) if n is None else n
    out_rc = np.zeros((max(max_kp, 1), 2), np.int32)
    out_resp = np.zeros(max(max_kp, 1), np.float32)
    m = ctypes.c_int(-7)
    args = {"rc": rc.ctypes.data, "resp": resp.ctypes.data, "out_rc": out_rc.ctypes.data,
            "out_resp": out_resp.ctypes.data, "n_out": ctypes.byref(m)}
    if null:
        args[null] = None
    return lib.yv_select_corners(None, H, W, args["rc"], args["resp"], n, max_kp, args["out_rc"], args["out_resp"],
                                 args["n_out"])


def test_null_pointers_are_invalid(lib):
    for name in ("rc", "resp", "out_rc", "n_out"):
        assert _select(lib, null=name) == yv.YV_ERR_INVALID, name


def test_bad_counts_and_sizes_are_invalid(lib):
    assert _select(lib, n=-1) == yv.YV_ERR_INVALID
    assert _select(lib, max_kp=-1) == yv.YV_ERR_INVALID
    assert _select(lib, H=8) == yv.YV_ERR_INVALID
    assert _select(lib, W=8) == yv.YV_ERR_INVALID
    assert _select(lib, H=-40) == yv.YV_ERR_INVALID


def test_positions_outside_the_image_are_invalid(lib):
    for pos in ((-1, 5), (5, -1), (40, 5), (5, 64), (2 ** 31 - 1, 0), (0, -2 ** 31)):
        assert _select(lib, rc=[[5, 6], pos]) == yv.YV_ERR_INVALID, pos
        assert _select(lib, rc=[pos, [5, 6]]) == yv.YV_ERR_INVALID, pos


def test_capacity_is_checked_before_the_device(lib):
    H, W = 12, 13  # (H - 8)(W - 8) = 20 corners at the most
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rc = np.stack([r.ravel(), c.ravel()], 1).astype(np.int32)
    expect = yv.YV_ERR_NODEVICE if lib.yv_device_count() == 0 else yv.YV_ERR_INVALID
    assert _select(lib, H=H, W=W, rc=rc[:21]) == yv.YV_ERR_CAPACITY
    assert _select(lib, H=H, W=W, rc=rc[:20]) == expect
    # an invalid position wins over the capacity: the list is looked at first
    bad = rc[:21].copy()
    bad[20] = (H, 0)
    assert _select(lib, H=H, W=W, rc=bad) == yv.YV_ERR_INVALID


def test_valid_arguments_without_a_context(lib):
    # what is left is the missing context: "no usable GPU" on a machine without one (there is no CPU path) and a plain
    # bad argument where a GPU exists
    expect = yv.YV_ERR_NODEVICE if lib.yv_device_count() == 0 else yv.YV_ERR_INVALID
    assert _select(lib) == expect
    assert _select(lib, null="out_resp") == expect  # out_resp may be NULL
    assert _select(lib, n=0) == expect
    assert _select(lib, max_kp=0) == expect
    assert _select(lib, H=9, W=9, rc=[[0, 0]]) == expect
    assert _select(lib, rc=[[0, 0], [39, 63]]) == expect
    weird = np.array([0xFFFFFFFF, 0x80000000], np.uint32).view(np.float32)  # any bit pattern is a response
    assert _select(lib, resp=weird) == expect
