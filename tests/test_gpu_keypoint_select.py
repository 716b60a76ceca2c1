"""Keypoint selection before the cut (yv_set_keypoint_select / yv_select_corners) against a numpy
reference: non-maximum suppression among the FAST corners and per-cell quotas, both on the 64-bit key
(~ord(response)) << 32 | row * W + col the cut itself ranks by (a smaller key is better).

The reference below is the specification.  It builds the keys from (response, index) exactly as key_resp
(ya_vo_amd/csrc/yavo_internal.h) inverts them, suppresses through a dense minimum-key map and the minimum over the
(2r + 1)^2 shifts of it (taken as 2r + 1 row shifts, then 2r + 1 column shifts: the same minimum), applies the quota by a
lexsort on (cell, key) and the cut by a sort on the key.  With every parameter off it equals oracle.fast bit for bit
(test_reference_off_equals_the_oracle, no GPU), which ties it to the oracle; every GPU comparison is exact.

The kernels stage nothing in chunks sized by the candidate count: the suppression wave walks its tile's corners 64 at a
time and the quota threads stride over the list, so no list here is "larger than a chunk" -- the 150,000-corner list
puts 721 corners into its fullest 32 x 64 suppression tile (12 trips) and the one-cell lists thousands into one cell."""
import functools

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd.synth import synth_frame

from test_gpu_envelope import SHAPES, _images as _envelope_images, _max_corners, _to_device

gpu = pytest.mark.gpu

THR = 20
OFF = (0, 0, 0, 0)
# (nms_radius, cell_rows, cell_cols, per_cell); the cell sides are ignored with per_cell == 0
PARAMS = [(1, 0, 0, 0), (4, 0, 0, 0), (8, 0, 0, 0), (0, 32, 32, 3), (0, 16, 16, 2), (3, 32, 32, 5), (2, 47, 61, 3),
          (8, 8, 8, 1)]
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _pid(p):
    return "off" if p == OFF else f"r{p[0]}-{p[1]}x{p[2]}-q{p[3]}"


# ---------------------------------------------------------------------------------------------------------------------
# the numpy reference
# ---------------------------------------------------------------------------------------------------------------------
def make_keys(idx, resp):
    """(~ord(resp)) << 32 | idx from the responses' bits as they are (-0.0 and 0.0 differ), ord as make_key's"""
    u = np.ascontiguousarray(resp, np.float32).view(np.uint32)
    ordv = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return ((~ordv).astype(np.uint64) << np.uint64(32)) | np.asarray(idx).astype(np.uint64)


def key_resp(keys):
    """key_resp of yavo_internal.h: the response's bits back from a key"""
    ordv = ~(keys >> np.uint64(32)).astype(np.uint32)
    u = np.where(ordv & np.uint32(0x80000000), ordv & np.uint32(0x7FFFFFFF), ~ordv).astype(np.uint32)
    return u.view(np.float32)


def _window_min(dense, r, H, W):
    """minimum over the (2r + 1)^2 window of a map padded by r on every side -> [H, W]"""
    rows = dense[0:H, :].copy()
    for d in range(1, 2 * r + 1):
        np.minimum(rows, dense[d:d + H, :], out=rows)
    out = rows[:, 0:W].copy()
    for d in range(1, 2 * r + 1):
        np.minimum(out, rows[:, d:d + W], out=out)
    return out


def select_reference(keys, H, W, params, keep):
    """-> dict: rc / resp of the selection + cut, and what the reach test counts: `alive` (per input corner, after
    suppression), `cells` (survivors per occupied cell, before the quota), `remaining` (corners the cut sees)"""
    r, cell_rows, cell_cols, q = params
    keys = np.asarray(keys, np.uint64)
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    row, col = idx // W, idx % W
    alive = np.ones(len(keys), bool)
    if r > 0 and len(keys):
        dense = np.full((H + 2 * r, W + 2 * r), NONE64, np.uint64)
        dense[row + r, col + r] = keys
        alive = _window_min(dense, r, H, W)[row, col] == keys  # no other corner of the window has a smaller key
    left = keys[alive]
    cells = np.zeros(0, np.int64)
    if q > 0 and len(left):
        li = (left & np.uint64(0xFFFFFFFF)).astype(np.int64)
        cell = (li // W) // cell_rows * ((W + cell_cols - 1) // cell_cols) + (li % W) // cell_cols
        order = np.lexsort((left, cell))
        sc = cell[order]
        first = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
        cells = np.diff(np.r_[first, len(sc)])
        rank = np.arange(len(sc)) - np.repeat(first, cells)
        left = left[order][rank < q]
    out = np.sort(left)[:keep]
    oi = (out & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return {"rc": np.stack([oi // W, oi % W], 1).astype(np.int32), "resp": key_resp(out), "alive": alive,
            "cells": cells, "remaining": len(left)}


# ---------------------------------------------------------------------------------------------------------------------
# images and their oracle candidates
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _image(name):
    if name == "a":
        img = synth_frame(77, 0, 0, 200, 320)
    elif name == "b":
        img = np.random.default_rng(3).integers(0, 256, (120, 160)).astype(np.uint8)
    elif name == "c":  # a period-4 texture below row 48: many corners share a response bit for bit
        img = synth_frame(2, 0, 0, 96, 128).copy()
        img[48:] = np.tile(np.random.default_rng(2).integers(0, 256, (4, 4)), (12, 32)).astype(np.uint8)
    elif name == "d":
        img = _envelope_images("1100x200")["noise"]
    elif name == "e":
        img = np.full((200, 320), 97, np.uint8)
    elif name in ("8192x24", "1025x24"):
        img = _envelope_images(name)["noise"]
    elif name == "2000x320":
        img = synth_frame(11, 0, 0, 2000, 320)
    else:  # the batch case: run k's left image, its crop 8 columns further, the shifted frame
        kind, k = name.split(":")
        k = int(k)
        img = {"L": lambda: synth_frame(77, k, 3 * k, 200, 320), "R": lambda: synth_frame(77, k, 3 * k + 8, 200, 320),
               "S": lambda: synth_frame(77, k + 2, 3 * k + 6, 200, 320)}[kind]()
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


_CAND = {}


def _candidates(oracle, name):
    """(keys of every FAST corner, corner count) from the oracle's candidate list; -0.0 becomes 0.0 as in make_key of
    the detect kernel (the reference's sort compares them equal)"""
    if name not in _CAND:
        img = _image(name)
        _, _, nc, ci, cr = oracle.fast(img, 1, with_candidates=True)
        cr = np.where(cr == 0, np.float32(0), cr).astype(np.float32)
        keys = make_keys(ci, cr)
        keys.setflags(write=False)
        _CAND[name] = (keys, nc)
    return _CAND[name]


_SEL = {}


def _reference(oracle, name, params, keep):
    k = (name, params, keep)
    if k not in _SEL:
        keys, nc = _candidates(oracle, name)
        H, W = _image(name).shape
        ref = select_reference(keys, H, W, params, keep)
        ref["nc"] = nc
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _SEL[k] = ref
    return _SEL[k]


def _set(ctx, params):
    r, cr, cc, q = params
    ctx.set_keypoint_select(r, (cr, cc) if q > 0 else None, q)


def _assert_detect(ctx, oracle, name, params, max_kp, max_corners=2000):
    ref = _reference(oracle, name, params, min(max_corners, max_kp))
    rc, resp, nc = ctx.detect(_image(name), max_kp)
    msg = f"{name} {_pid(params)} max_kp {max_kp}"
    print(f"{msg}: {ref['nc']} corners, {ref['remaining']} after selection, {len(ref['rc'])} kept")
    assert nc == ref["nc"], msg
    assert len(rc) == len(ref["rc"]), msg
    np.testing.assert_array_equal(rc, ref["rc"], err_msg=msg)
    np.testing.assert_array_equal(resp.view(np.uint32), ref["resp"].view(np.uint32), err_msg=msg)


# ---------------------------------------------------------------------------------------------------------------------
# 0. the reference with everything off is the oracle (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_kp", [("a", 2000), ("a", 100), ("b", 2000), ("c", 2000), ("c", 100), ("d", 4096),
                                         ("e", 2000)])
def test_reference_off_equals_the_oracle(oracle, name, max_kp):
    ref = _reference(oracle, name, OFF, max_kp)
    rc, resp, nc = oracle.fast(_image(name), max_kp)
    if nc == 0:
        rc, resp = rc[:0], resp[:0]
    assert ref["nc"] == nc and ref["remaining"] == nc
    np.testing.assert_array_equal(ref["rc"], rc)
    np.testing.assert_array_equal(ref["resp"].view(np.uint32), resp.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. yv_detect under every parameter set
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("params", PARAMS, ids=_pid)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_detect_selection(ctx, oracle, name, params):
    """max_kp 2000: the selection alone decides; 100: the cut bites after it."""
    try:
        _set(ctx, params)
        for max_kp in (2000, 100):
            _assert_detect(ctx, oracle, name, params, max_kp)
    finally:
        ctx.set_keypoint_select()


D_PARAMS = [OFF, (0, 16, 16, 2), (0, 8, 8, 1)]


@gpu
@pytest.mark.parametrize("params", D_PARAMS, ids=_pid)
def test_detect_selection_more_than_4096_corners(ctx, oracle, params):
    """1100 x 200 noise at max_kp 4096: off, the real cut (4096 is below the corner count); (0, 16, 16, 2) and, with
    3,450 cells, (0, 8, 8, 1), which hands top-K more than 2048 keys and fewer than its capacity."""
    try:
        with _max_corners(ctx, 4096):
            _set(ctx, params)
            _assert_detect(ctx, oracle, "d", params, 4096, max_corners=4096)
    finally:
        ctx.set_keypoint_select()


@gpu
def test_detect_flat_image(ctx, oracle):
    try:
        _set(ctx, (3, 32, 32, 5))
        _assert_detect(ctx, oracle, "e", (3, 32, 32, 5), 2000)
    finally:
        ctx.set_keypoint_select()


# ---------------------------------------------------------------------------------------------------------------------
# 2. switching selection off again is the context that never switched it on
# ---------------------------------------------------------------------------------------------------------------------
def _batch_bytes(c, b, n, max_kp):
    v = b.view()
    out = [c.download(v.cand_count, np.uint32, n), c.download(v.det_count, np.int32, n),
           c.download(v.kp_count, np.int32, n)]
    for i in range(n):
        out.append(c.download(v.det_rc + i * max_kp * 8, np.int32, 2 * max_kp))
        out.append(c.download(v.det_resp + i * max_kp * 4, np.uint32, max_kp))
        out.append(c.download(v.keypoints + i * max_kp * 48, np.uint8, 48 * max_kp))
    return [a.copy() for a in out]


@gpu
def test_off_again_is_never_on(ctx, offsets):
    imgs = [_image("a"), _image("L:1")]
    frames = np.stack(imgs)
    d = _to_device(frames)
    fresh = yv.Context(0)
    try:
        fresh.set_brief_offsets(offsets)
        want_detect = [fresh.detect(im, 2000) for im in imgs]
        fb = yv.Batch(fresh, 2, 200, 320, 2000, 0)
        fb.run(d.data_ptr(), 2, 320, 200 * 320, THR)
        fresh.sync()
        want = _batch_bytes(fresh, fb, 2, 2000)
        fb.close()
    finally:
        fresh.close()
    b = yv.Batch(ctx, 2, 200, 320, 2000, 0)
    try:
        _set(ctx, (2, 32, 32, 4))
        on_detect = ctx.detect(imgs[0], 2000)
        b.run(d.data_ptr(), 2, 320, 200 * 320, THR)
        ctx.sync()
        assert len(on_detect[0]) < len(want_detect[0][0])  # the selection was on
        ctx.set_keypoint_select()
        for im, (rc, resp, nc) in zip(imgs, want_detect):
            g_rc, g_resp, g_nc = ctx.detect(im, 2000)
            assert g_nc == nc and g_rc.tobytes() == rc.tobytes() and g_resp.tobytes() == resp.tobytes()
        b.run(d.data_ptr(), 2, 320, 200 * 320, THR)
        ctx.sync()
        got = _batch_bytes(ctx, b, 2, 2000)
        counts = got[1]
        # the arrays past each image's count keep the longer lists of nothing: compare what the counts cover
        assert all(a.tobytes() == w.tobytes() for a, w in zip(got[:3], want[:3]))
        for i in range(2):
            for j, unit in ((0, 2), (1, 1)):
                a, w = got[3 + 3 * i + j], want[3 + 3 * i + j]
                assert a[:unit * counts[i]].tobytes() == w[:unit * counts[i]].tobytes(), (i, j)
            a, w = got[5 + 3 * i], want[5 + 3 * i]
            assert a[:48 * got[2][i]].tobytes() == w[:48 * got[2][i]].tobytes(), i
    finally:
        ctx.set_keypoint_select()
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. yv_select_corners on hand-made lists
# ---------------------------------------------------------------------------------------------------------------------
def _assert_select(ctx, rc, resp, H, W, params, max_kp, max_corners=2000):
    rc = np.asarray(rc, np.int32).reshape(-1, 2)
    resp = np.asarray(resp, np.float32)
    keys = make_keys(rc[:, 0].astype(np.int64) * W + rc[:, 1], resp)
    ref = select_reference(keys, H, W, params, min(max_corners, max_kp))
    try:
        _set(ctx, params)
        g_rc, g_resp = ctx.select_corners(rc, resp, H, W, max_kp)
    finally:
        ctx.set_keypoint_select()
    msg = f"{H}x{W} n={len(rc)} {_pid(params)}"
    print(f"{msg}: {ref['remaining']} after selection, {len(ref['rc'])} kept")
    assert len(g_rc) == len(ref["rc"]), msg
    np.testing.assert_array_equal(g_rc, ref["rc"], err_msg=msg)
    np.testing.assert_array_equal(g_resp.view(np.uint32), ref["resp"].view(np.uint32), err_msg=msg)
    return ref


@gpu
@pytest.mark.parametrize("params", [OFF, (1, 0, 0, 0), (0, 8, 8, 1), (3, 32, 32, 5)], ids=_pid)
def test_select_corners_empty_and_single(ctx, params):
    _assert_select(ctx, np.zeros((0, 2), np.int32), np.zeros(0, np.float32), 40, 64, params, 2000)
    for pos in ((0, 0), (39, 63), (17, 30)):
        ref = _assert_select(ctx, [pos], [1.5], 40, 64, params, 2000)
        assert len(ref["rc"]) == 1


def _dense_list(bits):
    """every pixel FAST can test of a 40 x 64 image, one response"""
    r, c = np.meshgrid(np.arange(4, 36), np.arange(4, 60), indexing="ij")
    rc = np.stack([r.ravel(), c.ravel()], 1).astype(np.int32)
    return rc, np.full(len(rc), bits, np.uint32).view(np.float32)


@gpu
@pytest.mark.parametrize("bits", [0x42F60000, 0xFFFFFFFF, 0x80000000], ids=["123.0", "worst-bits", "minus-zero"])
@pytest.mark.parametrize("params", [OFF, (1, 0, 0, 0), (8, 0, 0, 0), (0, 8, 8, 1), (4, 8, 8, 1)], ids=_pid)
def test_select_corners_every_pixel_one_response(ctx, params, bits):
    """The buffer's capacity, (H - 8)(W - 8) corners, all with one response: the index decides everything.  The bits
    0xFFFFFFFF give the largest upper key half there is, the value the suppression map uses for "no corner"."""
    rc, resp = _dense_list(bits)
    assert len(rc) == (40 - 8) * (64 - 8)
    perm = np.random.default_rng(1).permutation(len(rc))  # the list's order must not matter
    _assert_select(ctx, rc[perm], resp[perm], 40, 64, params, 2000)


@functools.lru_cache(maxsize=None)
def _big_list():
    H, W, n = 376, 1241, 150000
    rng = np.random.default_rng(150)
    idx = rng.choice(H * W, n, replace=False)
    values = np.r_[np.float32([0.0, -0.0, -1.5, -3e-30, 7.25]), rng.normal(0, 50, 57).astype(np.float32),
                   np.uint32([0xFFFFFFFF, 0x7FFFFFFF]).view(np.float32)].astype(np.float32)
    assert len(values) == 64 and len(np.unique(values.view(np.uint32))) == 64
    resp = values[rng.integers(0, 64, n)]
    rc = np.stack([idx // W, idx % W], 1).astype(np.int32)
    return H, W, rc, resp


@gpu
@pytest.mark.parametrize("params", [(2, 32, 32, 6), (0, 8, 8, 4096), (8, 0, 0, 0)], ids=_pid)
def test_select_corners_150000(ctx, params):
    """150,000 distinct positions over the whole 376 x 1241 image (the border a detector never reports included),
    responses from 64 bit patterns: negatives, 0.0, -0.0 and the two extreme patterns."""
    H, W, rc, resp = _big_list()
    try:
        ctx.set_fast_params(40, 4096)
        _assert_select(ctx, rc, resp, H, W, params, 4096, max_corners=4096)
    finally:
        ctx.set_fast_params(40, 2000)


def _one_cell_list():
    rng = np.random.default_rng(64)
    idx = rng.choice(64 * 64, 3000, replace=False)
    rc = np.stack([64 + idx // 64, 64 + idx % 64], 1).astype(np.int32)
    resp = rng.integers(0, 40, 3000).astype(np.float32)  # many equal responses
    return rc, resp


@gpu
@pytest.mark.parametrize("params", [(0, 64, 64, 5), (0, 64, 64, 2999), (0, 64, 64, 3000), (1, 64, 64, 7),
                                    (0, 8192, 8192, 1500)], ids=_pid)
def test_select_corners_one_cell(ctx, params):
    """3,000 corners in one 64 x 64 cell of a 200 x 320 image (two suppression tiles), and the whole image as one cell."""
    rc, resp = _one_cell_list()
    _assert_select(ctx, rc, resp, 200, 320, params, 2000)


# ---------------------------------------------------------------------------------------------------------------------
# 4. a batch of four images, pairs through the carry slot, two chained runs
# ---------------------------------------------------------------------------------------------------------------------
BATCH_PARAMS = (1, 32, 32, 6)
BATCH_NAMES = ("L", "R", "flat", "S")
B_CARRY = 4
B_PAIRS = [(B_CARRY, 0), (0, 1), (3, 0), (2, 1)]  # temporal through the carry slot, stereo, shifted, a flat query


def _batch_image(kind, run):
    return _image("e") if kind == "flat" else _image(f"{kind}:{run}")


def _assert_batch_images(ctx, oracle, offsets, b, names, params, max_kp, keep):
    """per image: cand_count, det_count, det_rc, det_resp, kp_count and the keypoint records -> the records"""
    v = b.view()
    n = len(names)
    candc = ctx.download(v.cand_count, np.uint32, n)
    detc = ctx.download(v.det_count, np.int32, n)
    kpc = ctx.download(v.kp_count, np.int32, n)
    out = []
    for i, name in enumerate(names):
        ref = _reference(oracle, name, params, keep)
        msg = f"image {i} ({name})"
        assert candc[i] == ref["nc"] and detc[i] == len(ref["rc"]), msg
        rc = ctx.download(v.det_rc + i * max_kp * 8, np.int32, 2 * detc[i]).reshape(-1, 2)
        np.testing.assert_array_equal(rc, ref["rc"], err_msg=msg)
        resp = ctx.download(v.det_resp + i * max_kp * 4, np.uint32, detc[i])
        np.testing.assert_array_equal(resp, ref["resp"].view(np.uint32), err_msg=msg)
        want = oracle.brief(_image(name), ref["rc"], offsets) if len(ref["rc"]) else np.zeros(0, yv.KEYPOINT_DTYPE)
        assert kpc[i] == len(want), msg
        kps = ctx.download(v.keypoints + i * max_kp * 48, yv.KEYPOINT_DTYPE, kpc[i])
        np.testing.assert_array_equal(kps, want, err_msg=msg)
        out.append(kps)
    return out


@gpu
def test_batch_selection_pipeline(ctx, oracle, offsets):
    K = 2000
    b = yv.Batch(ctx, 4, 200, 320, K, len(B_PAIRS))
    try:
        b.set_pairs(B_PAIRS)
        _set(ctx, BATCH_PARAMS)
        prev = None
        for run in range(2):
            names = ["e" if k == "flat" else f"{k}:{run}" for k in BATCH_NAMES]
            d = _to_device(np.stack([_image(nm) for nm in names]))
            b.run(d.data_ptr(), 4, 320, 200 * 320, THR, carry_from=0)
            ctx.sync()
            kps = _assert_batch_images(ctx, oracle, offsets, b, names, BATCH_PARAMS, K, K)
            assert len(kps[2]) == 0 and len(kps[0]) > 100  # the flat slot stays empty
            v = b.view()
            mc = ctx.download(v.match_count, np.int32, len(B_PAIRS))
            fc = ctx.download(v.filt_count, np.int32, len(B_PAIRS))
            for p, (qi, ti) in enumerate(B_PAIRS):
                msg = f"run {run} pair {p}"
                qk = prev if qi == B_CARRY else kps[qi]
                if qk is None or len(qk) == 0:
                    assert mc[p] == 0 and fc[p] == 0, msg
                    continue
                om = oracle.match(qk, kps[ti])
                assert mc[p] == len(om), msg
                np.testing.assert_array_equal(ctx.download(v.matches + p * K * 100, yv.MATCH_DTYPE, mc[p]), om,
                                              err_msg=msg)
                np.testing.assert_array_equal(ctx.download(v.filtered + p * K * 100, yv.MATCH_DTYPE, fc[p]),
                                              oracle.remove_outliers(om, THR), err_msg=msg)
            prev = kps[0]
    finally:
        ctx.set_keypoint_select()
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. tall shapes and the cell limit
# ---------------------------------------------------------------------------------------------------------------------
TALL_PARAMS = (1, 8, 8, 1)


@gpu
@pytest.mark.parametrize("name", ["8192x24", "1025x24"])
def test_batch_selection_tall(ctx, oracle, offsets, name):
    """8192 x 24 with 8 x 8 cells: 3,072 cells, 256 tile rows; 1025 x 24: one bank class in top-K's band counters."""
    H, W, max_kp, _ = SHAPES[name]
    with _max_corners(ctx, max_kp):
        b = yv.Batch(ctx, 1, H, W, max_kp, 0)
        try:
            _set(ctx, TALL_PARAMS)
            d = _to_device(_image(name)[None])
            b.run(d.data_ptr(), 1, W, H * W, THR)
            ctx.sync()
            _assert_batch_images(ctx, oracle, offsets, b, [name], TALL_PARAMS, max_kp, max_kp)
        finally:
            ctx.set_keypoint_select()
            b.close()


@gpu
def test_batch_refuses_more_than_8192_cells(ctx, oracle, offsets):
    """2000 x 320 with 8 x 8 cells is 10,000 cells: YV_ERR_CAPACITY from run, the batch as it was; with selection off
    the same batch runs normally."""
    H, W, K = 2000, 320, 2000
    img = _image("2000x320")
    d = _to_device(img[None])
    b = yv.Batch(ctx, 1, H, W, K, 0)
    try:
        ctx.set_keypoint_select(1, (8, 8), 1)
        with pytest.raises(yv.YavoError) as e:
            b.run(d.data_ptr(), 1, W, H * W, THR)
        assert e.value.status == yv.YV_ERR_CAPACITY
        with pytest.raises(yv.YavoError) as e:
            ctx.detect(img, K)
        assert e.value.status == yv.YV_ERR_CAPACITY
        with pytest.raises(yv.YavoError) as e:
            ctx.select_corners([[5, 5]], [1.0], H, W, K)
        assert e.value.status == yv.YV_ERR_CAPACITY
        v = b.view()
        assert ctx.download(v.det_count, np.int32, 1)[0] == 0 and ctx.download(v.kp_count, np.int32, 2).sum() == 0
        ctx.set_keypoint_select(0, (8, 8), 0)
        b.run(d.data_ptr(), 1, W, H * W, THR)
        ctx.sync()
        _assert_batch_images(ctx, oracle, offsets, b, ["2000x320"], OFF, K, K)
    finally:
        ctx.set_keypoint_select()
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the reference alone reaches every case (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _neighbour_any(mask_pos, pos, r, H, W):
    """per position of `pos`: is any position of `mask_pos` inside its (2r + 1)^2 window"""
    dense = np.zeros((H + 2 * r, W + 2 * r), np.uint64)
    dense[mask_pos[:, 0] + r, mask_pos[:, 1] + r] = 1
    return (NONE64 - _window_min(NONE64 - dense, r, H, W))[pos[:, 0], pos[:, 1]] > 0


def test_reference_reaches_every_case(oracle):
    differs, more, quota_under = 0, 0, 0
    for name in ("a", "b", "c"):
        keys, nc = _candidates(oracle, name)
        H, W = _image(name).shape
        idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        pos = np.stack([idx // W, idx % W], 1)
        default = _reference(oracle, name, OFF, 2000)
        for params in PARAMS:
            ref = _reference(oracle, name, params, 2000)
            r, _, _, q = params
            msg = f"{name} {_pid(params)}"
            if r > 0:
                dead = ~ref["alive"]
                shadow = _neighbour_any(pos[dead], pos[ref["alive"]], r, H, W)
                print(f"{msg}: {nc} corners, {dead.sum()} suppressed, {shadow.sum()} survivors beside one")
                assert dead.sum() >= 5 and shadow.sum() >= 5, msg
            if q > 0:
                over, under = int((ref["cells"] > q).sum()), int((ref["cells"] < q).sum())
                print(f"{msg}: occupied cells over the quota {over}, under it {under}")
                if r >= max(params[1], params[2]):
                    # two corners of one cell are inside each other's window: suppression leaves one per cell at the
                    # most, and the quota has nothing left to take
                    assert over == 0 and ref["cells"].max() == 1, msg
                else:
                    assert over >= 1, msg  # (96 x 128 has nine 47 x 61 cells)
                    quota_under += int(over >= 5 and under >= 5)
            assert ref["remaining"] < nc, msg
            small = _reference(oracle, name, params, 100)
            print(f"{msg}: {ref['remaining']} corners reach the cut")
            assert ref["remaining"] < 2000 and len(ref["rc"]) == ref["remaining"], msg  # fewer than keep = 2000
            if ref["remaining"] > 100:                                                  # more than keep = 100
                assert len(small["rc"]) == 100, msg
                more += 1
            differs += int(not np.array_equal(small["rc"], default["rc"][:len(small["rc"])]))
    # at least five cells under the quota beside at least five over it, selections that leave more than keep, selected lists that are not
    # the default cut's: each in at least five (image, parameter set) cases
    assert quota_under >= 5 and more >= 5 and differs >= 5, (quota_under, more, differs)
    # (c): equal responses inside the radius, decided by the index
    keys, nc = _candidates(oracle, "c")
    H, W = _image("c").shape
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    row, col = idx // W, idx % W
    hi = keys >> np.uint64(32)
    r = 4
    dense = np.full((H + 2 * r, W + 2 * r), NONE64, np.uint64)
    dense[row + r, col + r] = hi
    best = _window_min(dense, r, H, W)[row, col]
    pairs, by_index = 0, 0
    for dr in range(-r, r + 1):
        for dc in range(-r, r + 1):
            if (dr, dc) != (0, 0):
                same = dense[row + r + dr, col + r + dc] == hi
                pairs += int(same.sum())
                by_index += int((same & (best == hi)).sum())
    shared = int((np.unique(hi, return_counts=True)[1] > 1).sum())
    print(f"c: {nc} corners, {shared} responses shared, {pairs} ordered equal pairs inside radius 4, {by_index} of them "
          f"with no better corner in the window")
    assert pairs >= 5 and by_index >= 5
    # (d): the cut bites with selection off, and (0, 8, 8, 1) leaves more than 2048 and fewer than 4096
    assert _reference(oracle, "d", OFF, 4096)["nc"] > 4096
    dref = _reference(oracle, "d", (0, 8, 8, 1), 4096)
    print(f"d: {dref['nc']} corners, (0, 8, 8, 1) leaves {dref['remaining']}, (0, 16, 16, 2) "
          f"{_reference(oracle, 'd', (0, 16, 16, 2), 4096)['remaining']}")
    assert 2048 < dref["remaining"] < 4096
    # the hand-made lists: a full tile, every cell over the quota, all in one cell
    H, W, rc, resp = _big_list()
    tile = np.bincount((rc[:, 0] // 32) * ((W + 63) // 64) + rc[:, 1] // 64)
    print(f"150000: the fullest 32 x 64 tile holds {tile.max()} corners")
    assert tile.max() > 64 * 8
    # the cell counts of the tall shapes
    assert ((8192 + 7) // 8) * ((24 + 7) // 8) == 3072
    assert ((2000 + 7) // 8) * ((320 + 7) // 8) == 10000 > 8192
    assert ((376 + 7) // 8) * ((1241 + 7) // 8) == 7332 <= 8192
