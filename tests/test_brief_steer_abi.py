"""CPU tests of the rotation-steered BRIEF (yv_set_brief_steering, yv_orient, yv_batch_orient_view_get): the symbols are
exported and bound, every argument check answers before the context, ya_vo_amd.steering builds the committed tables, and
the numpy specification of tests/steer_reference.py is tied to the oracle and has the properties the feature is for: a
quarter turn of the image leaves the descriptors equal bit for bit, and a rotation the unsteered descriptor does not
survive keeps the steered recall."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd.steering import steering_tables
from ya_vo_amd.synth import synth_frame

import steer_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "brief_steer_b32.npz")
NEW_SYMBOLS = ("yv_set_brief_steering", "yv_orient", "yv_batch_orient_view_get")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


@pytest.fixture(scope="module")
def tables(offsets):
    return steering_tables(offsets, 32)


def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in yv.SIGNATURES, name
    for cls, method in ((yv.Context, "set_brief_steering"), (yv.Context, "orient"), (yv.Batch, "orient_view")):
        assert callable(getattr(cls, method))
    assert lib.yv_abi_version() == 2


# ---- yv_set_brief_steering ----
def _set(lib, n_bins, radius=15, dirs="ok", off="ok"):
    nb = max(n_bins, 1) if 0 <= n_bins <= 64 else 1
    d = np.ascontiguousarray(dirs, np.int16) if isinstance(dirs, np.ndarray) else np.zeros((nb, 2), np.int16)
    o = np.ascontiguousarray(off, np.int8) if isinstance(off, np.ndarray) else np.zeros((nb, 256, 4), np.int8)
    return lib.yv_set_brief_steering(None, n_bins, radius, None if dirs is None else d.ctypes.data,
                                     None if off is None else o.ctypes.data)


def test_setting_is_checked_before_the_context(lib):
    for n_bins in (-1, 65, 2 ** 31 - 1, -2 ** 31):
        assert _set(lib, n_bins) == yv.YV_ERR_INVALID, n_bins
    for radius in (0, -1, 16, 2 ** 31 - 1):
        assert _set(lib, 4, radius=radius) == yv.YV_ERR_INVALID, radius
    assert _set(lib, 4, dirs=None) == yv.YV_ERR_INVALID
    assert _set(lib, 4, off=None) == yv.YV_ERR_INVALID
    for bad in (257, -257, 32767, -32768):
        for at in ((0, 0), (3, 1)):
            d = np.zeros((4, 2), np.int16)
            d[at] = bad
            assert _set(lib, 4, dirs=d) == yv.YV_ERR_INVALID, (bad, at)
    for bad in (16, -16, 127, -128):
        for at in ((0, 0, 0), (3, 255, 3), (1, 100, 2)):
            o = np.zeros((4, 256, 4), np.int8)
            o[at] = bad
            assert _set(lib, 4, off=o) == yv.YV_ERR_INVALID, (bad, at)


def test_valid_settings_reach_the_null_context(lib):
    # what is left is the NULL context; with n_bins = 0 the radius and the tables are ignored
    assert lib.yv_set_brief_steering(None, 0, -5, None, None) == yv.YV_ERR_INVALID
    assert _set(lib, 0, radius=99, dirs=None, off=None) == yv.YV_ERR_INVALID
    for n_bins in (1, 5, 32, 64):
        for radius in (1, 7, 15):
            d = np.full((n_bins, 2), 256, np.int16)
            d[-1] = -256
            o = np.full((n_bins, 256, 4), 15, np.int8)
            o[-1] = -15
            assert _set(lib, n_bins, radius=radius, dirs=d, off=o) == yv.YV_ERR_INVALID


# ---- yv_orient ----
def _orient(lib, H=40, W=64, stride=None, rc=((5, 6), (20, 30)), n=None, null=None):
    img = np.zeros((H if H > 0 else 1, max(W, 1)), np.uint8)
    rc = np.ascontiguousarray(np.asarray(rc, np.int64).reshape(-1, 2), np.int32)
    n = len(rc) if n is None else n
    buf = rc if len(rc) else np.zeros((1, 2), np.int32)
    mom = np.zeros((max(n, 1), 2), np.int32)
    b = np.zeros(max(n, 1), np.uint8)
    args = {"img": img.ctypes.data, "rc": buf.ctypes.data, "moments": mom.ctypes.data, "bin": b.ctypes.data}
    if null:
        args[null] = None
    return lib.yv_orient(None, args["img"], H, W, W if stride is None else stride, args["rc"], n, args["moments"],
                         args["bin"])


def test_orient_arguments_are_checked_before_the_context(lib):
    for name in ("img", "rc", "moments", "bin"):
        assert _orient(lib, null=name) == yv.YV_ERR_INVALID, name
    assert _orient(lib, n=-1) == yv.YV_ERR_INVALID
    assert _orient(lib, H=8) == yv.YV_ERR_INVALID
    assert _orient(lib, W=8) == yv.YV_ERR_INVALID
    assert _orient(lib, stride=63) == yv.YV_ERR_INVALID
    for pos in ((-1, 5), (5, -1), (40, 5), (5, 64), (2 ** 31 - 1, 0), (0, -2 ** 31)):
        assert _orient(lib, rc=[(5, 6), pos]) == yv.YV_ERR_INVALID, pos
        assert _orient(lib, rc=[pos, (5, 6)]) == yv.YV_ERR_INVALID, pos


def test_orient_capacity_is_checked_before_the_context(lib):
    rc = np.zeros((4097, 2), np.int32)
    assert _orient(lib, rc=rc) == yv.YV_ERR_CAPACITY
    # valid lists, the largest one included: what is left is the NULL context
    assert _orient(lib, rc=rc[:4096]) == yv.YV_ERR_INVALID
    assert _orient(lib) == yv.YV_ERR_INVALID
    assert _orient(lib, rc=[(0, 0), (39, 63)]) == yv.YV_ERR_INVALID
    assert _orient(lib, rc=[], n=0) == yv.YV_ERR_INVALID
    assert lib.yv_orient(None, None, 9, 9, 9, None, 0, None, None) == yv.YV_ERR_INVALID  # n = 0: no pointer is needed


def test_orient_view_of_a_null_batch(lib):
    v = yv._BatchOrientView()
    assert lib.yv_batch_orient_view_get(None, ctypes.byref(v)) == yv.YV_ERR_INVALID


# ---- the default tables ----
def test_steering_tables_reproduce_the_golden_fixture(offsets, tables):
    g = np.load(GOLDEN)
    dirs, off = tables
    assert dirs.dtype == np.int16 and dirs.shape == (32, 2) and off.dtype == np.int8 and off.shape == (32, 256, 4)
    np.testing.assert_array_equal(dirs, g["dirs"])
    np.testing.assert_array_equal(off, g["offsets"])
    assert np.abs(off.astype(np.int32)).max() <= 11
    np.testing.assert_array_equal(off[0], offsets)
    want = [(256, 0), (251, 50), (237, 98), (213, 142), (181, 181), (142, 213), (98, 237), (50, 251), (0, 256)]
    np.testing.assert_array_equal(dirs[:9], want)
    for n_bins in (0, 2, 30, 68, -4):
        with pytest.raises(ValueError):
            steering_tables(offsets, n_bins)
    for n_bins in (4, 64):
        d, o = steering_tables(offsets, n_bins)
        assert d.shape == (n_bins, 2) and o.shape == (n_bins, 256, 4)


def test_every_bin_is_the_quarter_turn_of_the_bin_eight_before(tables):
    dirs, off = tables
    o = off.astype(np.int32).reshape(32, 256, 2, 2)
    d = dirs.astype(np.int32)
    for k in range(32):
        q = (k + 8) % 32
        np.testing.assert_array_equal(o[q, ..., 0], o[k, ..., 1], err_msg=f"bin {k}")   # drow' = dcol
        np.testing.assert_array_equal(o[q, ..., 1], -o[k, ..., 0], err_msg=f"bin {k}")  # dcol' = -drow
        np.testing.assert_array_equal(d[q], (-d[k, 1], d[k, 0]), err_msg=f"bin {k}")


# ---- the reference against the oracle ----
def test_one_bin_with_the_plain_table_is_the_oracles_brief(oracle, offsets):
    """Keypoints with 8 <= row <= H - 9 and 8 <= col <= W - 9 sample neither column W nor row H, so the clamped
    sampling and the reference's linear index read the same pixels."""
    rng = np.random.default_rng(11)
    dirs, off = sr.plain_table(offsets)
    for img in (synth_frame(5, 0, 0, 64, 97), rng.integers(0, 256, (41, 30), dtype=np.uint8)):
        H, W = img.shape
        rc = np.stack([rng.integers(8, H - 8, 200), rng.integers(8, W - 8, 200)], 1)
        rc[:4] = [(8, 8), (8, W - 9), (H - 9, 8), (H - 9, W - 9)]
        want = oracle.brief(img, rc, offsets)
        assert len(want) == len(rc)
        got, k, _ = sr.describe_records(sr.blur(oracle, img), rc, dirs, off)
        assert not k.any()
        assert got.tobytes() == want.tobytes()


# ---- what the feature is for, on the reference alone ----
def _noise_image(seed, H, W, oracle):
    img = np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    return oracle.blur(img)


@pytest.mark.parametrize("name", ["noise60x83", "synth120x160"])
def test_a_quarter_turn_keeps_the_descriptor_and_shifts_the_bin(oracle, offsets, tables, name):
    """np.rot90 takes pixel (r, c) of an H x W image to (W - 1 - c, r).  The blur kernel is symmetric and the clamped
    sampling turns with the image, so the moments turn exactly: the bin moves by 24 of 32 and, every bin's pattern being
    the exact quarter turn of the bin eight before, the descriptor does not change in any bit, border included."""
    dirs, off = tables
    if name == "noise60x83":
        img = np.random.default_rng(3).integers(0, 256, (60, 83), dtype=np.uint8)
    else:
        img = synth_frame(21, 0, 0, 120, 160)
    H, W = img.shape
    rng = np.random.default_rng(4)
    rc = np.stack([rng.integers(0, H, 300), rng.integers(0, W, 300)], 1)
    rc[:4] = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    rc_t = np.stack([W - 1 - rc[:, 1], rc[:, 0]], 1)
    b, b_t = sr.blur(oracle, img), sr.blur(oracle, np.rot90(img))
    np.testing.assert_array_equal(b_t, np.rot90(b))
    f, k, m = sr.describe(b, rc, dirs, off)
    f_t, k_t, m_t = sr.describe(b_t, rc_t, dirs, off)
    # no argmax ties among these positions: a tie would pick the smaller index on both sides, not the turned one
    d = dirs.astype(np.int64)
    score = m[:, 0:1] * d[None, :, 0] + m[:, 1:2] * d[None, :, 1]
    assert ((score == score.max(1, keepdims=True)).sum(1) == 1).all()
    np.testing.assert_array_equal((k.astype(np.int32) + 24) % 32, k_t)
    np.testing.assert_array_equal(f, f_t)
    assert len(np.unique(k)) >= 16
    # unsteered, the same positions lose about half their bits
    pd, po = sr.plain_table(offsets)
    u, _, _ = sr.describe(b, rc, pd, po)
    u_t, _, _ = sr.describe(b_t, rc_t, pd, po)
    assert np.median(sr.hamming(u, u_t)) >= 100


@pytest.fixture(scope="module")
def recall_inputs(oracle):
    """The two 240 x 320 images and 400 positions in the disc of 90 pixels about the centre: a patch and its blur
    support stay inside the image under every rotation about the centre."""
    imgs = {"synth": synth_frame(31, 0, 0, 240, 320), "noise": _noise_image(32, 240, 320, oracle)}
    rng = np.random.default_rng(33)
    rad, ang = 90.0 * np.sqrt(rng.random(400)), 2 * np.pi * rng.random(400)
    rc = np.rint(np.stack([119.5 + rad * np.sin(ang), 159.5 + rad * np.cos(ang)], 1)).astype(np.int64)
    return imgs, rc


@pytest.mark.parametrize("degrees", [30, 45, 77])
@pytest.mark.parametrize("name", ["synth", "noise"])
def test_rotation_recall_steered_against_unsteered(oracle, offsets, tables, recall_inputs, name, degrees):
    """Each original descriptor against the turned image's descriptors at the mapped positions, nearest neighbour: the
    steered descriptor keeps its recall where the unsteered one has none.  Conditions on the specification, not
    measurements of the kernel."""
    imgs, rc = recall_inputs
    img = imgs[name]
    turned, forward = sr.rotate_bilinear(img, degrees)
    rc_t = forward(rc)
    b, b_t = sr.blur(oracle, img), sr.blur(oracle, turned)
    dirs, off = tables
    f, _, _ = sr.describe(b, rc, dirs, off)
    f_t, _, _ = sr.describe(b_t, rc_t, dirs, off)
    pd, po = sr.plain_table(offsets)
    u, _, _ = sr.describe(b, rc, pd, po)
    u_t, _, _ = sr.describe(b_t, rc_t, pd, po)
    steered, plain = sr.recall(f, f_t), sr.recall(u, u_t)
    print(f"{name} {degrees} deg: steered recall {steered:.3f}, unsteered {plain:.3f}")
    assert steered >= 0.9
    assert plain <= 0.1
