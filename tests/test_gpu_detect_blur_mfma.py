"""The detect kernel's fused 9x9 blur (batch path) against the oracle's blur, byte for byte.

With every tap <= 127 both passes run on the int8 matrix cores: the horizontal sums stay in registers, are split into
a high and a low byte (each as b - 128) and feed the vertical MFMA under a relabelled K order; a tap above 127 takes
the v_dot4 / v_dot2 passes through LDS.  The shapes cover reflection with clamping (9 x 9), exactly one tile, one-row
and one-column remainder tiles, an interior tile (the unaligned-dword staging) and odd sizes; the images the extremes
of the signed byte split (all 255: h = 65280, hi = 255, lo = 0; all 0), noise (any wrong row <-> K-slot pairing) and a
row / column pattern; the tap sets an asymmetric one (a flipped band), one with only the window's ends and centre (the
9-row reach), a tap at exactly 127 and one just above it (the fallback path).
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
}


def _frames(H, W):
    r, c = np.indices((H, W))
    noise = np.random.default_rng(1000 * H + W).integers(0, 256, (H, W)).astype(np.uint8)
    return np.stack([np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8), noise,
                     ((37 * r + 11 * c) % 256).astype(np.uint8)])


def _run_batch(ctx, frames):
    import torch
    n, H, W = frames.shape
    d = torch.from_numpy(np.ascontiguousarray(frames)).to("cuda:0")
    torch.cuda.synchronize()
    b = yv.Batch(ctx, n, H, W, 2000, 0)
    b.run(d.data_ptr(), n, W, H * W, 20)
    ctx.sync()
    return b, d


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
