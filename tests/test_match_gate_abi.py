"""CPU tests of the gated matcher's boundary (include/yavo/yavo.h): the two symbols are exported and bound, the Python
methods exist, and every argument check answers before any device work and before the context is looked at."""
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yv_match_gated", "yv_batch_set_match_gates")
K_MAX_KP = 4096
COORD_MAX = 65535
GATE = (-2, 2, -128, 0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in yv.SIGNATURES, name
    assert callable(getattr(yv.Context, "match_gated"))
    assert callable(getattr(yv.Batch, "set_match_gates"))
    assert lib.yv_abi_version() == 2


def _gated(lib, nq=1, nt=1, gate=GATE, q=None, t=None, null=None):
    """yv_match_gated with a NULL context on small valid buffers; `null` names one pointer to pass as NULL."""
    q = np.zeros(1, yv.KEYPOINT_DTYPE) if q is None else q
    t = np.zeros(1, yv.KEYPOINT_DTYPE) if t is None else t
    g = np.array(gate, np.int32)
    out = np.zeros(max(len(q), 1), yv.MATCH2_DTYPE)
    args = {"q": q.ctypes.data, "t": t.ctypes.data, "gate": g.ctypes.data, "out": out.ctypes.data}
    if null:
        args[null] = None
    return lib.yv_match_gated(None, args["q"], nq, args["t"], nt, args["gate"], args["out"], None)


def test_null_pointers_are_invalid(lib):
    for name in ("gate", "q", "t", "out"):
        assert _gated(lib, null=name) == yv.YV_ERR_INVALID, name


def test_negative_counts_are_invalid(lib):
    assert _gated(lib, nq=-1) == yv.YV_ERR_INVALID
    assert _gated(lib, nt=-1) == yv.YV_ERR_INVALID


BAD_GATES = [(1, 0, 0, 0), (0, 0, 1, 0), (3, 2, -5, 5), (-COORD_MAX - 1, 0, 0, 0), (0, COORD_MAX + 1, 0, 0),
             (0, 0, -COORD_MAX - 1, 0), (0, 0, 0, COORD_MAX + 1), (0, 0, 0, 2 ** 31 - 1), (-2 ** 31, 0, 0, 0)]


def test_bad_gates_are_invalid(lib):
    for gate in BAD_GATES:
        assert _gated(lib, gate=gate) == yv.YV_ERR_INVALID, gate


def test_keypoints_outside_16_bits_are_invalid(lib):
    for field in ("x", "y"):
        for value in (-1, COORD_MAX + 1, 2 ** 31 - 1):
            for side in ("q", "t"):
                k = np.zeros(3, yv.KEYPOINT_DTYPE)
                k[field][2] = value
                assert _gated(lib, **{"n" + side: 3, side: k}) == yv.YV_ERR_INVALID, (field, value, side)


def test_capacity_is_checked_before_the_device(lib):
    assert _gated(lib, nq=K_MAX_KP + 1) == yv.YV_ERR_CAPACITY
    assert _gated(lib, nt=K_MAX_KP + 1) == yv.YV_ERR_CAPACITY


def test_valid_arguments_without_a_context(lib):
    # what is left is the missing context: "no usable GPU" on a machine without one (there is no CPU path) and a plain
    # bad argument where a GPU exists
    expect = yv.YV_ERR_NODEVICE if lib.yv_device_count() == 0 else yv.YV_ERR_INVALID
    edge = np.zeros(2, yv.KEYPOINT_DTYPE)
    edge["x"], edge["y"] = (0, COORD_MAX), (COORD_MAX, 0)
    for gate in (GATE, (-40, 40, -60, 60), (0, 0, 0, 0), (3, 9, 5, 5), (-COORD_MAX, COORD_MAX, -COORD_MAX, COORD_MAX)):
        assert _gated(lib, gate=gate) == expect, gate
        assert _gated(lib, nq=2, nt=2, q=edge, t=edge, gate=gate) == expect, gate
    assert _gated(lib, nq=0, nt=0) == expect


def test_batch_call_rejects_a_null_batch(lib):
    g = np.array(GATE, np.int32)
    assert lib.yv_batch_set_match_gates(None, g.ctypes.data, 1) == yv.YV_ERR_INVALID
    assert lib.yv_batch_set_match_gates(None, None, 0) == yv.YV_ERR_INVALID
    for gate in BAD_GATES:
        g = np.array(gate, np.int32)
        assert lib.yv_batch_set_match_gates(None, g.ctypes.data, 1) == yv.YV_ERR_INVALID
