"""brief_kernel as persistent workers: few workers walking many (band, image) items, against the oracle.

brief_kernel is a grid of at most two workers per CU; a worker takes items from an eight-headed queue (its own XCD
label's range first, then the other labels'), and its LDS keeps what the band before left there: pixels, the zero rows
past the image, the column-W bytes and the keypoint list.  A band without keypoints stages nothing.  The rest of the
suite runs at most a few items per worker, so here

  * the batch cycles through four kinds of image -- noise, flat, noise in the even 32-row bands only, noise in the odd
    bands only -- so that in item order full bands follow empty ones and empty ones full ones, the last band of an
    image (with zero rows past its end) precedes the first band of the next, and bands with many keypoints precede
    bands with few;
  * yv_debug_set_brief_workers caps the workers at 1, 2, 3 and 8: with one worker every item follows its predecessor
    in one LDS region, with fewer than eight every range of a missing label is reached by stealing only;
  * the batch runs twice on one Batch with the images rotated, so the queue heads are zeroed twice and no slot can
    pass on the records of the run before;
  * 400 images (1,600 items) run at the default cap: more items than workers on any device.

Every comparison is exact (test_gpu_envelope.py's _assert_images).  test_corpus_reaches_every_case runs without a GPU:
on the oracle's output alone it asserts that the corpus holds the cases above."""
import ctypes
import functools

import numpy as np
import pytest

import ya_vo_amd as yv

from test_gpu_envelope import BAND, THR, _assert_images, _bands, _reference, _to_device

gpu = pytest.mark.gpu

MAX_KP = 2000
# name -> (H, W, images): 96 / 24 / 32 items; 72 x 1400 is past the LDS-DMA part of the band (W > 1320: the rest of
# the band goes through registers) and puts nearly every keypoint of an even-bands image into band 0
CORPUS = {"100x80": (100, 80, 24), "72x1400": (72, 1400, 8), "40x64": (40, 64, 16)}
KINDS = ("noise", "flat", "even", "odd")
CAPS = [1, 2, 3, 8, 0]
MANY = 400


@functools.lru_cache(maxsize=None)
def _corpus(name):
    """[images][H][W] uint8, read-only: image i is of kind KINDS[i % 4], every noise field its own"""
    H, W, n = CORPUS[name]
    band = np.arange(H) // BAND
    out = np.full((n, H, W), 97, np.uint8)
    for i in range(n):
        kind = KINDS[i % 4]
        if kind == "flat":
            continue
        noise = np.random.default_rng(100000 * H + 100 * W + i).integers(0, 256, (H, W)).astype(np.uint8)
        rows = {"noise": band >= 0, "even": band % 2 == 0, "odd": band % 2 == 1}[kind]
        out[i, rows] = noise[rows]
    out.setflags(write=False)
    return out


def _refs(oracle, offsets, name):
    return [_reference(oracle, offsets, ("persistent", name, i), img, MAX_KP) for i, img in enumerate(_corpus(name))]


def _item_counts(refs, H):
    """keypoints per item in queue order (image major, band minor)"""
    nb = (H + BAND - 1) // BAND
    out = np.zeros((len(refs), nb), np.int64)
    for i, r in enumerate(refs):
        c = _bands(r["kps"]) if len(r["kps"]) else np.zeros(0, np.int64)
        out[i, :len(c)] = c
    return out.reshape(-1)


class _Cap:
    """yv_debug_set_brief_workers(ctx, n) for the block, the default (0) after it"""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.fn = ctx.lib.yv_debug_set_brief_workers
        self.fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.fn.restype = ctypes.c_int

    def __enter__(self):
        assert self.fn(self.ctx.handle, self.n) == 0
        return self

    def __exit__(self, *exc):
        assert self.fn(self.ctx.handle, 0) == 0
        return False


@gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", list(CORPUS))
def test_forced_looping_batch(ctx, oracle, offsets, name, cap):
    """Two runs of one Batch under the cap; the second with the images rotated by one, so every slot changes its kind
    (a slot that was flat must get records, and none may keep the run before's)."""
    H, W, n = CORPUS[name]
    frames, refs = _corpus(name), _refs(oracle, offsets, name)
    with _Cap(ctx, cap):
        b = yv.Batch(ctx, n, H, W, MAX_KP, 0)
        try:
            for shift in (0, 1):
                order = [(i + shift) % n for i in range(n)]
                d = _to_device(frames[order])
                b.run(d.data_ptr(), n, W, H * W, THR)
                ctx.sync()
                _assert_images(ctx, b, [refs[i] for i in order], MAX_KP, H, W)
        finally:
            b.close()


@gpu
@pytest.mark.parametrize("cap", [1, 2])
def test_forced_looping_describe(ctx, oracle, offsets, cap):
    """yv_describe under a cap: kp_boundary_kernel zeroes the heads, the grid covers one image's items."""
    for name in ("100x80", "72x1400"):
        frames, refs = _corpus(name), _refs(oracle, offsets, name)
        with _Cap(ctx, cap):
            for i in (0, 2, 3, 1, 0):  # noise, even, odd, flat, noise again
                got = ctx.describe(frames[i], refs[i]["rc"])
                np.testing.assert_array_equal(got, refs[i]["kps"], err_msg=f"{name} image {i}")


@gpu
def test_more_items_than_workers(ctx, oracle, offsets):
    """400 images of 100 x 80 at the default cap: 1,600 items against at most 2 x CUs workers, so every worker loops
    and ranges that finish early are refilled by stealing.  The 24 distinct images repeated in a shuffled order."""
    name = "100x80"
    H, W, n = CORPUS[name]
    frames, refs = _corpus(name), _refs(oracle, offsets, name)
    idx = np.random.default_rng(5).permutation(np.arange(MANY) % n)
    d = _to_device(frames[idx])
    b = yv.Batch(ctx, MANY, H, W, MAX_KP, 0)
    try:
        b.run(d.data_ptr(), MANY, W, H * W, THR)
        ctx.sync()
        _assert_images(ctx, b, [refs[i] for i in idx], MAX_KP, H, W)
    finally:
        b.close()


def test_corpus_reaches_every_case(oracle, offsets):
    off = np.asarray(offsets, np.int32).reshape(-1, 2, 2)  # [test][point](dr, dc)
    assert (off[..., 0] == 8).any() and (off[..., 1] == 8).any()  # samples on the row and the column past a patch
    for name, (H, W, n) in CORPUS.items():
        refs = _refs(oracle, offsets, name)
        c = _item_counts(refs, H)
        empty = c == 0
        e2f = int((empty[:-1] & ~empty[1:]).sum())
        f2e = int((~empty[:-1] & empty[1:]).sum())
        kps = np.concatenate([r["kps"] for r in refs])
        print(f"{name}: {len(c)} items, {int(empty.sum())} empty, {e2f} empty->full, {f2e} full->empty, "
              f"up to {int(c.max())} keypoints per item")
        assert len(c) == n * ((H + BAND - 1) // BAND)
        assert e2f >= 1 and f2e >= 1, name
        # an image's first band with keypoints (zero rows above) after a band with keypoints and zero rows below
        nb = (H + BAND - 1) // BAND
        last = max(k for k in range(nb) if k * BAND <= H - 8)  # the last band that can hold a keypoint
        assert last * BAND + 41 > H
        full = np.flatnonzero(~empty)
        assert any(a % nb == last and z % nb == 0 for a, z in zip(full[:-1], full[1:])), name
        # a band's list shorter than the one staged before it (stale entries stay behind its end)
        assert any(c[z] < c[a] for a, z in zip(full[:-1], full[1:])), name
        assert (kps["x"] == H - 8).any(), name  # with dr == 8: the zero row past the image
        assert (kps["y"] == W - 8).any(), name  # with dc == 8: the column-W patch
        if name == "72x1400":
            assert W > 1320 and c.max() > 1024  # the register path; a second record load per thread
        # the rotated second run of test_forced_looping_batch changes every slot's kind
        assert n % 4 == 0
