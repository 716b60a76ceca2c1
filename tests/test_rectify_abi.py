"""CPU tests of the rectifier (yv_rectify_*): the symbols are exported and bound, YV_RECTIFY_OUTSIDE is the header's,
every argument check answers before the context, and the numpy specification of tests/rectify_reference.py gives the
stated results on hand-made maps and keeps the rounding's own bound on the model maps."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import io as yio

import rectify_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yv_rectify_create", "yv_rectify_destroy", "yv_rectify_set_model", "yv_rectify_set_map",
               "yv_rectify_map_read", "yv_rectify_run", "yv_rectify_image", "yv_rectify_debug_tiles",
               "yv_rectify_debug_force_direct")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


# ---- surface ----
def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in yv.IO_SIGNATURES, name
    for method in ("set_model", "set_map", "map", "run", "close", "tiles", "force_direct"):
        assert callable(getattr(yio.Rectifier, method))
    assert callable(yio.rectify_image) and callable(yio.rectify_matrix)
    assert lib.yv_abi_version() == 2


def test_outside_is_the_headers(tmp_path):
    src = tmp_path / "probe_rect.c"
    src.write_text('#include <stdio.h>\n#include "yavo/yavo_io.h"\n'
                   'int main(void){printf("%lld\\n", (long long)YV_RECTIFY_OUTSIDE); return 0;}\n')
    exe = tmp_path / "probe_rect"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    val = int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
    assert val == -2 ** 31 == rr.OUTSIDE == yio.YV_RECTIFY_OUTSIDE


def test_rectify_matrix_is_the_inverse():
    K, _, _ = rr.kitti_raw_model()
    R = rr._rot(0.02, -0.01, 0.03)
    M = yio.rectify_matrix(K.reshape(3, 3), R)
    assert M.shape == (9,) and M.tobytes() == rr.rectify_matrix(K, R).tobytes()
    np.testing.assert_allclose(M.reshape(3, 3) @ (K.reshape(3, 3) @ R), np.eye(3), atol=1e-12)


def _null_ctx_status(lib):
    return yv.YV_ERR_INVALID if lib.yv_device_count() > 0 else yv.YV_ERR_NODEVICE


def test_create_checks_come_before_the_context(lib):
    h = ctypes.c_void_p()
    ok = dict(n_maps=2, sh=512, sw=1392, dh=376, dw=1241)

    def create(out=True, **kw):
        a = {**ok, **kw}
        return lib.yv_rectify_create(None, a["n_maps"], a["sh"], a["sw"], a["dh"], a["dw"],
                                     ctypes.byref(h) if out else None)

    assert create(out=False) == yv.YV_ERR_INVALID
    for key in ("sh", "sw", "dh", "dw"):
        for bad in (0, -1, 8193, 2 ** 31 - 1):
            assert create(**{key: bad}) == yv.YV_ERR_INVALID, (key, bad)
    for bad in (0, -1, 17):
        assert create(n_maps=bad) == yv.YV_ERR_INVALID, bad
    # valid calls, the envelope's corners included: what is left is the NULL context
    want = _null_ctx_status(lib)
    assert create() == want
    assert create(n_maps=1, sh=1, sw=1, dh=1, dw=1) == want
    assert create(n_maps=16, sh=8192, sw=8192, dh=8192, dw=8192) == want
    assert h.value is None


def test_handle_calls_refuse_a_null_handle(lib):
    k = np.zeros(9)
    q = np.zeros((4, 4, 2), np.int32)
    a, b = ctypes.c_int32(), ctypes.c_int32()
    assert lib.yv_rectify_set_model(None, 0, k.ctypes.data, k.ctypes.data, k.ctypes.data) == yv.YV_ERR_INVALID
    assert lib.yv_rectify_set_map(None, 0, q.ctypes.data) == yv.YV_ERR_INVALID
    assert lib.yv_rectify_map_read(None, 0, q.ctypes.data) == yv.YV_ERR_INVALID
    assert lib.yv_rectify_run(None, q.ctypes.data, 4, 16, q.ctypes.data, 4, 16, 1, None) == yv.YV_ERR_INVALID
    assert lib.yv_rectify_run(None, None, 4, 16, None, 4, 16, 0, None) == yv.YV_ERR_INVALID
    assert lib.yv_rectify_debug_tiles(None, 0, ctypes.byref(a), ctypes.byref(b)) == yv.YV_ERR_INVALID
    assert lib.yv_rectify_debug_force_direct(None, 1) == yv.YV_ERR_INVALID
    lib.yv_rectify_destroy(None)  # a no-op


def test_rectify_image_checks_come_before_the_context(lib):
    src = np.zeros((33, 61), np.uint8)
    q = rr.identity_map(20, 40)
    dst = np.zeros((20, 45), np.uint8)
    ok = dict(src=src.ctypes.data, sh=33, sw=61, ss=61, q=q.ctypes.data, dst=dst.ctypes.data, dh=20, dw=40, ds=45)

    def call(**kw):
        a = {**ok, **kw}
        return lib.yv_rectify_image(None, a["src"], a["sh"], a["sw"], a["ss"], a["q"], a["dst"], a["dh"], a["dw"],
                                    a["ds"])

    for key in ("src", "q", "dst"):
        assert call(**{key: None}) == yv.YV_ERR_INVALID, key
    for key in ("sh", "sw", "dh", "dw"):
        for bad in (0, -1, 8193):
            assert call(**{key: bad}) == yv.YV_ERR_INVALID, (key, bad)
    assert call(ss=60) == yv.YV_ERR_INVALID
    assert call(ds=39) == yv.YV_ERR_INVALID
    want = _null_ctx_status(lib)
    assert call() == want
    assert call(ss=61, ds=40) == want
    assert call(sh=1, sw=1, ss=1, dh=1, dw=1, ds=1) == want
    assert not dst.any()


# ---- hand cases on the specification ----
def _noise(H, W, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def test_identity_reproduces_the_source():
    src = _noise(33, 61)
    assert rr.remap(src, rr.identity_map(33, 61)).tobytes() == src.tobytes()


@pytest.mark.parametrize("dx,dy", [(3, 2), (-3, -2), (70, 0), (0, -40), (-61, 33), (5, -1)])
def test_integer_shift_moves_the_image_with_zeros_outside(dx, dy):
    Hs, Ws = 33, 61
    src = _noise(Hs, Ws, 2)
    got = rr.remap(src, rr.identity_map(Hs, Ws, 32 * dx, 32 * dy))
    want = np.zeros_like(src)
    for v in range(Hs):
        for u in range(Ws):
            if 0 <= v + dy < Hs and 0 <= u + dx < Ws:
                want[v, u] = src[v + dy, u + dx]
    assert got.tobytes() == want.tobytes()
    if abs(dx) >= Ws or abs(dy) >= Hs:
        assert not got.any()


def test_half_pixel_map_averages_neighbours_against_a_zero_tap():
    src = _noise(20, 40, 3)
    got = rr.remap(src, rr.identity_map(20, 40, 16, 0))
    p = src.astype(np.int64)
    nxt = np.concatenate([p[:, 1:], np.zeros((20, 1), np.int64)], 1)  # the last column's right tap is outside: 0
    assert got.tobytes() == ((p + nxt + 1) >> 1).astype(np.uint8).tobytes()


def test_column_ramp_gives_the_rounded_column():
    Hs, Ws = 30, 256
    src = np.broadcast_to(np.arange(Ws, dtype=np.uint8), (Hs, Ws)).copy()
    rng = np.random.default_rng(4)
    q = np.stack([rng.integers(0, 32 * (Ws - 1), (50, 70)), rng.integers(0, 32 * (Hs - 1), (50, 70))], -1)
    q = q.astype(np.int32)
    got = rr.remap(src, q)  # every tap inside
    np.testing.assert_array_equal(got, (q[..., 0] + 16) >> 5)


def test_outside_and_extreme_entries_give_zero():
    src = np.full((9, 9), 255, np.uint8)
    assert not rr.remap(src, rr.outside_map(7, 5)).any()
    q = rr.identity_map(4, 4)
    q[0, 0] = (2 ** 31 - 1, 2 ** 31 - 1)
    q[0, 1] = (-2 ** 31 + 1, -2 ** 31 + 1)
    q[0, 2] = (2 ** 31 - 1, 64)
    q[0, 3] = (64, -2 ** 31 + 1)
    q[1, 0] = (rr.OUTSIDE, 64)  # one component OUTSIDE: no source
    q[1, 1] = (64, rr.OUTSIDE)
    got = rr.remap(src, q)
    assert not got[0].any() and got[1, 0] == 0 and got[1, 1] == 0 and (got[2:] == 255).all()
    assert got.tobytes() == rr.remap_slow(src, q).tobytes()


def test_one_by_one_source_and_destination():
    src = np.array([[200]], np.uint8)
    for q, want in (((0, 0), 200), ((16, 0), 100), ((0, 16), 100), ((16, 16), 50), ((-32, 0), 0), ((-16, -16), 50),
                    ((32, 0), 0), ((-1, 0), (31 * 200 * 32 + 512) >> 10)):
        got = rr.remap(src, np.array([[q]], np.int32))
        assert got.shape == (1, 1) and got[0, 0] == want, q


@pytest.mark.parametrize("shape", [((9, 9), (9, 9)), ((33, 61), (20, 40)), ((64, 300), (50, 90))])
def test_the_array_form_is_the_written_specification(shape):
    (Hs, Ws), (H, W) = shape
    src = _noise(Hs, Ws, 5)
    for q in (rr.random_map(Hs, Ws, H, W, 6), rr.split_map(Hs, Ws, H, W, 7), rr.rotation_map(Hs, Ws, H, W)):
        q = q.copy()
        q[0, 0] = (rr.OUTSIDE, 5)
        assert rr.remap(src, q).tobytes() == rr.remap_slow(src, q).tobytes()


# ---- model maps ----
def test_zero_distortion_with_the_inverse_camera_is_the_identity():
    K, _, _ = rr.kitti_raw_model()
    M = np.linalg.inv(K.reshape(3, 3)).reshape(9)
    q = rr.model_map_q5(K, np.zeros(8), M, 376, 1241)
    assert q.tobytes() == rr.identity_map(376, 1241).tobytes()


@pytest.mark.parametrize("name,sizes", [("kitti_raw", (512, 1392, 376, 1241)), ("full", (512, 1392, 376, 1241)),
                                        ("kitti_raw", (64, 300, 200, 320)), ("full", (64, 300, 200, 320))])
def test_quantisation_keeps_the_roundings_own_bound(name, sizes):
    Hs, Ws, H, W = sizes
    K, dist, M = rr.MODELS[name](Hs, Ws, H, W)
    mu, mv = rr.model_map(K, dist, M, H, W)
    q = rr.model_map_q5(K, dist, M, H, W)
    ins = q[..., 0] != rr.OUTSIDE
    assert ins.all() and np.array_equal(ins, q[..., 1] != rr.OUTSIDE)
    assert np.abs(q[..., 0] / 32.0 - mu).max() <= 1 / 64 and np.abs(q[..., 1] / 32.0 - mv).max() <= 1 / 64
    # the map lands on the source: most destination pixels have all four taps inside
    ix, iy = q[..., 0] >> 5, q[..., 1] >> 5
    inside = (ix >= 0) & (ix + 1 < Ws) & (iy >= 0) & (iy + 1 < Hs)
    assert inside.mean() > 0.9


def test_a_horizon_inside_the_image_is_outside_and_never_nan():
    Hs, Ws, H, W = 512, 1392, 376, 1241
    K, dist, M = rr.horizon_model(Hs, Ws, H, W)
    Wd = (M[6] * np.arange(W)[None, :] + M[7] * np.arange(H)[:, None]) + M[8]
    assert (Wd > 0).any() and (Wd < 0).any()  # the plane Wd = 0 crosses the destination
    M0 = M.copy()
    M0[8] -= Wd[100, 200]  # and passes exactly through pixel (200, 100): a division by zero
    for Mx in (M, M0):
        mu, mv = rr.model_map(K, dist, Mx, H, W)
        q = rr.model_map_q5(K, dist, Mx, H, W)
        out = q[..., 0] == rr.OUTSIDE
        assert out.any() and not out.all() and np.array_equal(out, q[..., 1] == rr.OUTSIDE)
        big = ~((np.abs(mu) < 65536) & (np.abs(mv) < 65536))  # infinities and NaN included
        assert np.array_equal(out, big)
        assert np.abs(q[~out].astype(np.int64)).max() <= 65536 * 32
    assert (q[100, 200] == rr.OUTSIDE).all()
    img = rr.remap(_noise(Hs, Ws, 8), q)
    assert not img[out].any()
