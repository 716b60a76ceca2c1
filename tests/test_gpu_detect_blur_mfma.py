"""The detect kernel's fused 9x9 blur (batch path) against the oracle's blur, byte for byte.

With every tap <= 127 both passes run on the int8 matrix cores inside the detect kernel: the horizontal sums stay in
registers, are split into a high and a low byte (each as b - 128) and feed the vertical MFMA under a relabelled K
order.  A tap above 127 does not fit int8: the batch then runs the detect kernel without blur and the stand-alone
blur kernel after it, into the same pitched buffer.  The shapes cover reflection with clamping (9 x 9), exactly one
tile, one-row and one-column remainder tiles, an interior tile (the unaligned-dword staging) and odd sizes; the images
the extremes of the signed byte split (all 255: h = 65280, hi = 255, lo = 0; all 0), noise (any wrong row <-> K-slot
pairing) and a row / column pattern; the tap sets an asymmetric one (a flipped band), one with only the window's ends
and centre (the 9-row reach), a tap at exactly 127, one just above it and the largest tap the ABI admits (both on the
two-kernel route).  Further tests switch the route on one batch, pass a source stride and image pitch that differ
from W and H * W through both routes, and compare the two-kernel route's candidates and keypoints with the oracle's.
"""
import numpy as np
import pytest

import ya_vo_amd as yv

pytestmark = pytest.mark.gpu

SHAPES = [(9, 9), (56, 64), (57, 65), (120, 200), (131, 203)]
TAPS = {
    "default": list(yv.DEFAULT_BLUR_KERNEL),
    "asymmetric": [1, 3, 9, 27, 81, 60, 40, 25, 10],
    "ends_centre": [100, 0, 0, 0, 56, 0, 0, 0, 100],
    "tap_127": [0, 0, 1, 64, 127, 64, 0, 0, 0],
    "tap_128_fallback": [0, 0, 0, 64, 128, 64, 0, 0, 0],
    "tap_255": [0, 0, 0, 0, 255, 1, 0, 0, 0],
}
MAX_KP = 2000


def _k9(name):
    k9 = np.array(TAPS[name], np.uint16)
    assert int(k9.sum()) == 256
    return k9


def _frames(H, W):
    r, c = np.indices((H, W))
    noise = np.random.default_rng(1000 * H + W).integers(0, 256, (H, W)).astype(np.uint8)
    return np.stack([np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8), noise,
                     ((37 * r + 11 * c) % 256).astype(np.uint8)])


def _noise_frames(H, W, seeds):
    return np.stack([np.random.default_rng(s).integers(0, 256, (H, W)).astype(np.uint8) for s in seeds])


def _to_device(host):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0")
    torch.cuda.synchronize()
    return d


def _run_batch(ctx, frames):
    n, H, W = frames.shape
    d = _to_device(frames)
    b = yv.Batch(ctx, n, H, W, MAX_KP, 0)
    b.run(d.data_ptr(), n, W, H * W, 20)
    ctx.sync()
    return b, d


def _assert_blur(ctx, oracle, b, frames, k9):
    _, H, W = frames.shape
    v = b.view()
    bp = v.blur_pitch
    for i, img in enumerate(frames):
        blur = ctx.download(v.blurred + i * H * bp, np.uint8, H * bp).reshape(H, bp)[:, :W]
        np.testing.assert_array_equal(blur, oracle.blur(img, k9), err_msg=f"image {i}")


def _assert_keypoints(ctx, oracle, offsets, b, frames, k9):
    """Candidate count, the kept corners in response order and the keypoint records (BRIEF on the oracle's blur with
    the same taps) of every image equal the oracle's."""
    v = b.view()
    n = len(frames)
    candc = ctx.download(v.cand_count, np.uint32, n)
    detc = ctx.download(v.det_count, np.int32, n)
    kpc = ctx.download(v.kp_count, np.int32, n)
    for i, img in enumerate(frames):
        orc, _, onc = oracle.fast(img, MAX_KP)
        assert onc > 0 and candc[i] == onc and detc[i] == len(orc), f"image {i}"
        rc = ctx.download(v.det_rc + i * MAX_KP * 8, np.int32, 2 * detc[i]).reshape(-1, 2)
        np.testing.assert_array_equal(rc, orc, err_msg=f"image {i}")
        kps = ctx.download(v.keypoints + i * MAX_KP * 48, yv.KEYPOINT_DTYPE, kpc[i])
        np.testing.assert_array_equal(kps, oracle.brief(img, orc, offsets, k9), err_msg=f"image {i}")


@pytest.fixture
def restore_taps(ctx):
    yield
    ctx.set_blur_kernel(np.array(yv.DEFAULT_BLUR_KERNEL, np.uint16))


@pytest.mark.parametrize("taps", list(TAPS.keys()))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_blur_matches_oracle(ctx, oracle, shape, taps):
    H, W = shape
    k9 = np.array(TAPS[taps], np.uint16)
    assert int(k9.sum()) == 256
    frames = _frames(H, W)
    b = None
    try:
        ctx.set_blur_kernel(k9)
        b, _d = _run_batch(ctx, frames)
        v = b.view()
        bp = v.blur_pitch
        for i, img in enumerate(frames):
            blur = ctx.download(v.blurred + i * H * bp, np.uint8, H * bp).reshape(H, bp)[:, :W]
            np.testing.assert_array_equal(blur, oracle.blur(img, k9), err_msg=f"image {i}")
    finally:
        ctx.set_blur_kernel(np.array(yv.DEFAULT_BLUR_KERNEL, np.uint16))
        if b is not None:
            b.close()


def test_batch_keypoints_unchanged(ctx, oracle, offsets):
    """Harris and the blur are independent phases after the FAST barrier: candidates, responses' order and
    descriptors of a noise batch (tiles with more than 64 corners, so Harris runs on every wave) equal the oracle's."""
    H, W = 120, 200
    frames = np.stack([np.random.default_rng(s).integers(0, 256, (H, W)).astype(np.uint8) for s in (11, 12, 13)])
    b, _d = _run_batch(ctx, frames)
    try:
        v = b.view()
        kpc = ctx.download(v.kp_count, np.int32, len(frames))
        for i, img in enumerate(frames):
            rc, _, _ = oracle.fast(img, 2000)
            kps = ctx.download(v.keypoints + i * 2000 * 48, yv.KEYPOINT_DTYPE, kpc[i])
            np.testing.assert_array_equal(kps, oracle.brief(img, rc, offsets))
    finally:
        b.close()


def test_two_kernel_route_candidates_and_keypoints(ctx, oracle, offsets, restore_taps):
    """A tap above 127 on the noise batch of test_batch_keypoints_unchanged: the detect kernel without blur feeds top-K
    what the fused one does (candidate count and the kept corners equal the oracle's) and BRIEF reads the stand-alone
    kernel's blur (the keypoint records equal the oracle's with the same taps)."""
    k9 = _k9("tap_128_fallback")
    frames = _noise_frames(120, 200, (11, 12, 13))
    ctx.set_blur_kernel(k9)
    b, _d = _run_batch(ctx, frames)
    try:
        _assert_blur(ctx, oracle, b, frames, k9)
        _assert_keypoints(ctx, oracle, offsets, b, frames, k9)
    finally:
        b.close()


def test_route_follows_the_context_taps_on_every_run(ctx, oracle, offsets, restore_taps):
    """One batch, three runs: default taps (fused), a tap above 127 (two kernels), default taps again.  The blur is
    right after every run and the last run's keypoints equal the oracle's, so the route is chosen from the context's
    taps at each run and the detect kernel without blur leaves nothing behind that the fused one trips over."""
    H, W = 57, 65
    frames = _noise_frames(H, W, (21, 22))
    d = _to_device(frames)
    b = yv.Batch(ctx, len(frames), H, W, MAX_KP, 0)
    try:
        for name in ("default", "tap_128_fallback", "default"):
            k9 = _k9(name)
            ctx.set_blur_kernel(k9)
            b.run(d.data_ptr(), len(frames), W, H * W, 20)
            ctx.sync()
            _assert_blur(ctx, oracle, b, frames, k9)
        _assert_keypoints(ctx, oracle, offsets, b, frames, k9)
    finally:
        b.close()


@pytest.mark.parametrize("taps", ["default", "tap_128_fallback"])
def test_source_stride_and_pitch(ctx, oracle, offsets, restore_taps, taps):
    """Frames embedded in a larger buffer, stride = W + 7 and image_pitch = stride * H + 13, the gaps filled with
    noise: both routes (the second passes stride and pitch to two kernels) read only the frames."""
    H, W, n = 57, 65, 3
    stride = W + 7
    pitch = stride * H + 13
    frames = _noise_frames(H, W, (31, 32, 33))
    host = np.random.default_rng(34).integers(0, 256, n * pitch).astype(np.uint8)
    for i in range(n):
        host[i * pitch:i * pitch + stride * H].reshape(H, stride)[:, :W] = frames[i]
    k9 = _k9(taps)
    d = _to_device(host)
    b = yv.Batch(ctx, n, H, W, MAX_KP, 0)
    try:
        ctx.set_blur_kernel(k9)
        b.run(d.data_ptr(), n, stride, pitch, 20)
        ctx.sync()
        _assert_blur(ctx, oracle, b, frames, k9)
        _assert_keypoints(ctx, oracle, offsets, b, frames, k9)
    finally:
        b.close()
