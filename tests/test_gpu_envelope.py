"""The front end over the whole (H, W, max_kp, image count) envelope that yv_batch_create accepts, against the oracle.

The rest of the GPU suite runs detect -> top-K -> BRIEF -> match at KITTI size and below with max_kp = 2000.  The cases
here are the smallest inputs that flip each size switch of the front-end kernels (ya_vo_amd/csrc/yavo_detect.hip,
yavo_topk.hip, yavo_brief.hip, yavo_match.hip) and of yv_batch_create / yv_batch_run (yavo_batch.hip):

  * boundary_compact's (band, bank class) counters: 32 bands x 32 classes = 1024 counters (two trips of top-K's
    512-thread scan), one class above 32 bands (H > 1024), K > 2048 (two chunks of 4 x 512 points), 256 bands (every
    entry of the band offsets table) and the K == 0 write of that table;
  * brief_kernel's band staging: widths whose band has more than 4 x 1024 16-B words (the rest goes through
    registers, with a column-W patch selected by (W >> 2) & 3 and 8 * (W & 3)), W & 15 == 0 and 15, kMaxWidth, and
    bands that hold more than 1024 / 2048 / 3072 keypoints (the four record loads per thread);
  * the batch's matcher choice (max_kp > 2048: the int8 kernels, several pairs per launch, 1-NN, top-2 and reverse)
    and slot strides that are no multiple of the matchers' tiles (1, 33, 100) with every slot full;
  * launch_blur9's slices above 65,535 images.

Every quantity is an integer, or a float the oracle evaluates operation for operation, so every comparison is exact.
test_reference_reaches_every_regime runs without a GPU: on the oracle's output alone it asserts that each input
really is in the regime it was built for."""
import contextlib
import functools

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd.synth import synth_frame

from test_gpu_match_knn2 import keep_reference, knn2_reference

gpu = pytest.mark.gpu

DEFAULT_TAPS = np.array(yv.DEFAULT_BLUR_KERNEL, np.uint16)
THR = 20
RATIO = (4, 5)
FLAGS = yv.YV_MATCH_RATIO | yv.YV_MATCH_MUTUAL
BAND = 32  # kBandRows

# ---------------------------------------------------------------------------------------------------------------------
# 1. image shapes: name -> (H, W, max_kp, with a flat image)
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = {
    "1000x64": (1000, 64, 2000, False),    # 32 bands x 32 classes: the counter scan's second trip
    "1025x24": (1025, 24, 4096, False),    # 33 bands: one class
    "1100x200": (1100, 200, 4096, True),   # one class, K > 2048
    "8192x24": (8192, 24, 4096, True),     # 256 bands: the whole offsets table, the height limit
    "40x2048": (40, 2048, 4096, False),    # kMaxWidth, W & 15 == 0, dw_fix 0, a band with > 1024 keypoints
    "41x2047": (41, 2047, 2000, False),    # W & 15 == 15, LS == 2048, dw_fix 3
    "25x1334": (25, 1334, 2000, False),    # dw_fix 1, sh_fix 16: the register path holds zero rows only
    "25x1339": (25, 1339, 2000, False),    # dw_fix 2, sh_fix 24: the same
    "72x1718": (72, 1718, 2000, False),    # dw_fix 1, sh_fix 16, with column-W patches in the register path
    "72x1723": (72, 1723, 2000, False),    # dw_fix 2, sh_fix 24, the same
}
TALL = ("1000x64", "1025x24", "1100x200", "8192x24")
WIDE = ("40x2048", "41x2047", "25x1334", "25x1339", "72x1718", "72x1723")
CUT = ("1000x64", "1100x200", "8192x24", "41x2047", "72x1718", "72x1723")  # noise: more corners than max_kp
MIN_BANDS = {"1000x64": 30, "1100x200": 33, "1025x24": 25, "8192x24": 200}


@functools.lru_cache(maxsize=None)
def _images(name):
    """{"synth", "noise"[, "flat"]} -> read-only [H, W] uint8"""
    H, W, _, flat = SHAPES[name]
    out = {"synth": synth_frame(11, 0, 0, H, W),
           "noise": np.random.default_rng(1000 * H + W).integers(0, 256, (H, W)).astype(np.uint8)}
    if flat:
        out["flat"] = np.full((H, W), 97, np.uint8)
    for a in out.values():
        a.setflags(write=False)
    return out


_REF = {}


def _reference(oracle, offsets, key, img, max_kp, k9=DEFAULT_TAPS):
    """The oracle's outputs for one image, computed once per (key, max_kp) and never modified."""
    k = (key, max_kp, tuple(int(t) for t in k9))
    if k not in _REF:
        rc, resp, nc = oracle.fast(img, max_kp)
        if max_kp == 0 or nc == 0:
            rc, resp = rc[:0], resp[:0]
        ref = {"rc": rc, "resp": resp, "nc": nc, "blur": oracle.blur(img, k9),
               "kps": oracle.brief(img, rc, offsets, k9)}
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[k] = ref
    return _REF[k]


def _bands(kps):
    """keypoint count per 32-row band (the record's x is the row)"""
    return np.bincount(kps["x"] // BAND)


def _edge_points(H, W):
    """Hand-placed points whose patches touch column W (col + 8 == W: the wrap to the next row's first pixel) and the
    last 16 columns, on every row checkBoundry admits, plus a few it refuses."""
    rows = np.arange(8, H - 8 + 1)
    cols = np.array([W - 8, W - 9, W - 12, W - 16, W - 8, 8])
    rc = np.stack(np.meshgrid(rows, cols, indexing="ij"), -1).reshape(-1, 2)
    bad = np.array([[7, W - 8], [H - 7, W - 8], [8, W - 7], [8, 7]])
    return np.concatenate([rc[:len(rc) // 2], bad, rc[len(rc) // 2:]]).astype(np.int32)


def _register_patch_hits(kps, W, offsets):
    """Keypoints with a test sample at column W whose band row's patch word lies past the band's first 4 x 1024 16-B
    words, i.e. is written by brief_kernel's register path (word index (row + dr - r0 + 8) * (LS / 16) + (W >> 4))."""
    wpr = ((W + 1 + 15) & ~15) >> 4
    off = np.asarray(offsets, np.int32).reshape(-1, 2, 2)  # [test][point](dr, dc)
    dr8 = off[..., 0][off[..., 1] == 8]
    if len(dr8) == 0:
        return 0
    at_edge = kps[kps["y"] + 8 == W]
    jmax = at_edge["x"] % BAND + 8 + int(dr8.max())
    return int((jmax * wpr + (W >> 4) >= 4 * 1024).sum())


@contextlib.contextmanager
def _max_corners(ctx, max_kp):
    """FastDetector's maxCorners (2000) caps every cut; the batches above it lift it for their runs."""
    if max_kp > 2000:
        ctx.set_fast_params(40, 4096)
    try:
        yield
    finally:
        ctx.set_fast_params(40, 2000)


def _to_device(host):
    import torch
    d = torch.from_numpy(np.array(host)).to("cuda:0")  # a writable copy: the inputs are read-only
    torch.cuda.synchronize()
    return d


def _assert_images(ctx, b, refs, max_kp, H, W):
    """tests/test_gpu_detect_blur_mfma.py's _assert_keypoints, extended: per image the candidate count, the kept
    corners (count, row / column, the bits of the Harris response), the blurred image and the keypoint records equal the
    oracle's.  An image without corners is admitted (refs[i]["nc"] == 0)."""
    v = b.view()
    n = len(refs)
    assert v.max_kp == max_kp and (v.H, v.W) == (H, W)
    bp = v.blur_pitch
    assert bp % 128 == 0 and bp > W
    candc = ctx.download(v.cand_count, np.uint32, n)
    detc = ctx.download(v.det_count, np.int32, n)
    kpc = ctx.download(v.kp_count, np.int32, n)
    out = []
    for i, ref in enumerate(refs):
        msg = f"image {i}"
        assert candc[i] == ref["nc"] and detc[i] == len(ref["rc"]) and kpc[i] == len(ref["kps"]), msg
        rc = ctx.download(v.det_rc + i * max_kp * 8, np.int32, 2 * detc[i]).reshape(-1, 2)
        np.testing.assert_array_equal(rc, ref["rc"], err_msg=msg)
        resp = ctx.download(v.det_resp + i * max_kp * 4, np.uint32, detc[i])
        np.testing.assert_array_equal(resp, ref["resp"].view(np.uint32), err_msg=msg)
        blur = ctx.download(v.blurred + i * H * bp, np.uint8, H * bp).reshape(H, bp)[:, :W]
        np.testing.assert_array_equal(blur, ref["blur"], err_msg=msg)
        kps = ctx.download(v.keypoints + i * max_kp * 48, yv.KEYPOINT_DTYPE, kpc[i])
        np.testing.assert_array_equal(kps, ref["kps"], err_msg=msg)
        out.append(kps)
    return out


@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_regimes_batch(ctx, oracle, offsets, name):
    """Two runs of one batch per shape.  With a flat image the second run rotates the images, so the slot that held a
    textured image (a full band offsets table) then holds the one without corners: its table is rewritten (K == 0) and
    BRIEF writes no record there -- the slot's records stay byte for byte what run 1 left."""
    H, W, max_kp, flat = SHAPES[name]
    imgs = _images(name)
    order = ["synth", "noise"] + (["flat"] if flat else [])
    with _max_corners(ctx, max_kp):
        b = yv.Batch(ctx, len(order), H, W, max_kp, 0)
        try:
            for run in range(2):
                frames = np.stack([imgs[k] for k in order])
                d = _to_device(frames)
                b.run(d.data_ptr(), len(order), W, H * W, THR)
                ctx.sync()
                refs = [_reference(oracle, offsets, (name, k), imgs[k], max_kp) for k in order]
                _assert_images(ctx, b, refs, max_kp, H, W)
                if flat and run == 0:
                    v = b.view()
                    n0 = len(refs[0]["kps"])
                    before = ctx.download(v.keypoints, yv.KEYPOINT_DTYPE, n0).copy()
                    order = ["flat", "synth", "noise"]  # slot 0: textured -> flat
                elif flat:
                    assert refs[0]["nc"] == 0
                    np.testing.assert_array_equal(ctx.download(b.view().keypoints, yv.KEYPOINT_DTYPE, n0), before)
        finally:
            b.close()


@gpu
@pytest.mark.parametrize("name", ["1000x64", "1100x200"])
def test_tall_shapes_host_calls(ctx, oracle, offsets, name):
    """yv_detect at both tall shapes (top-K on the single-image workspace, max_kp = 4096 there) and yv_describe at
    1100 x 200 (kp_boundary_kernel with one bank class), on the synthetic and the noise image."""
    H, W, max_kp, _ = SHAPES[name]
    with _max_corners(ctx, max_kp):
        for key in ("synth", "noise"):
            img = _images(name)[key]
            ref = _reference(oracle, offsets, (name, key), img, max_kp)
            rc, resp, nc = ctx.detect(img, max_kp)
            assert nc == ref["nc"]
            np.testing.assert_array_equal(rc, ref["rc"])
            np.testing.assert_array_equal(resp.view(np.uint32), ref["resp"].view(np.uint32))
            if name == "1100x200":
                np.testing.assert_array_equal(ctx.describe(img, ref["rc"]), ref["kps"], err_msg=key)


@gpu
@pytest.mark.parametrize("name", WIDE)
def test_wide_shapes_column_w_points(ctx, oracle, offsets, name):
    """Hand-placed points on the last columns of every row (col + 8 == W samples column W) through yv_describe."""
    H, W, _, _ = SHAPES[name]
    rc = _edge_points(H, W)
    for key in ("synth", "noise"):
        img = _images(name)[key]
        np.testing.assert_array_equal(ctx.describe(img, rc), oracle.brief(img, rc, offsets), err_msg=key)


@gpu
@pytest.mark.parametrize("args,status", [((1, 8193, 24, 2000, 0), yv.YV_ERR_CAPACITY),
                                         ((1, 40, 2049, 2000, 0), yv.YV_ERR_CAPACITY),
                                         ((1, 40, 64, 4097, 0), yv.YV_ERR_INVALID)])
def test_batch_create_refuses_outside_the_envelope(ctx, args, status):
    with pytest.raises(yv.YavoError) as e:
        yv.Batch(ctx, *args)
    assert e.value.status == status


# ---------------------------------------------------------------------------------------------------------------------
# 2. one band holding every keypoint
# ---------------------------------------------------------------------------------------------------------------------
ONE_BAND_H, ONE_BAND_W = 40, 400
# (points, share that fails checkBoundry): with none refused the band holds exactly n records -- 1025 and 3073 are the
# first counts that need the second and the fourth record load of a thread, 4096 fills all four
ONE_BAND = [(4096, 0.1), (4096, 0.0), (1025, 0.0), (3073, 0.0), (1025, 0.1), (3073, 0.1)]


@functools.lru_cache(maxsize=None)
def _one_band_input(n, bad):
    H, W = ONE_BAND_H, ONE_BAND_W
    rng = np.random.default_rng(7 * n + int(100 * bad))
    img = rng.integers(0, 256, (H, W)).astype(np.uint8)
    rc = np.stack([rng.integers(8, 32, n), rng.integers(8, W - 8 + 1, n)], 1).astype(np.int32)
    dup = rng.choice(n, n // 16, replace=False)          # exact duplicates of other points
    rc[dup] = rc[rng.integers(0, n, len(dup))]
    rc[::97] = [31, W - 8]                               # the band's last row at the wrap column, many times
    nbad = int(bad * n)
    if nbad:
        where = rng.choice(n, nbad, replace=False)
        kinds = np.array([[7, 50], [33, 50], [20, 7], [20, W - 7]])
        rc[where] = kinds[np.arange(nbad) % 4]
    img.setflags(write=False)
    rc.setflags(write=False)
    return img, rc


@gpu
@pytest.mark.parametrize("n,bad", ONE_BAND)
def test_describe_one_full_band(ctx, oracle, offsets, n, bad):
    img, rc = _one_band_input(n, bad)
    np.testing.assert_array_equal(ctx.describe(img, rc), oracle.brief(img, rc, offsets))


# ---------------------------------------------------------------------------------------------------------------------
# 3. keypoint capacities in the batch
# ---------------------------------------------------------------------------------------------------------------------
PH, PW = 200, 320
N_FRAMES = 2                 # stereo frames per run: 4 images, 4 pairs (temporal through the carry slot + stereo)
CARRY = 2 * N_FRAMES
PAIRS = [p for k in range(N_FRAMES) for p in ((CARRY if k == 0 else 2 * (k - 1), 2 * k), (2 * k, 2 * k + 1))]
CAPACITIES = [4096, 2049, 2048, 100, 33, 1]
FILTER_CAPACITIES = [4096, 100]
DENSE_SPECKLE, DENSE_LEFT_COLS = 0.034, 80


@functools.lru_cache(maxsize=None)
def _pipeline_frames(dense):
    """[2 runs][4 images L R L R][PH][PW].  Frame k is the crop at (k, 3 k) of one field, its right image 8 columns
    further, as tests/test_gpu_batch_match_filter.py's _frames(): a synthetic field with a block of its own texture
    pasted a second time (identical descriptors: ties).  dense: salt-and-pepper speckle on top, which takes the right
    images from ~650 to more than 2048 keypoints (train lists past the FP4 matcher's size, the repeated block
    included); the left images are flat right of column DENSE_LEFT_COLS, so the query lists stay short and the
    oracle's scalar matcher quick."""
    nk = 2 * N_FRAMES
    world = synth_frame(77, 0, 0, PH + nk, PW + 3 * nk + 8).copy()
    if dense:
        m = np.random.default_rng(5).random(world.shape)
        world[m < DENSE_SPECKLE] = 0
        world[m > 1 - DENSE_SPECKLE] = 255
        world[100:180, 10:60] = world[10:90, 10:60]  # repeated texture, inside the left images' textured part
    else:
        world[100:180, 170:290] = world[10:90, 20:140]  # repeated texture
    f = np.stack([world[k:k + PH, c:c + PW] for k in range(nk) for c in (3 * k, 3 * k + 8)]).reshape(2, nk, PH, PW)
    if dense:
        f[:, 0::2, :, DENSE_LEFT_COLS:] = 128
    f.setflags(write=False)
    return f


def _pipeline_reference(oracle, offsets, max_kp):
    """[run][image] oracle references of the frames a batch of this capacity runs on."""
    dense = max_kp > 2000
    fr = _pipeline_frames(dense)
    return fr, [[_reference(oracle, offsets, ("pipeline", dense, run, i), fr[run, i], max_kp)
                 for i in range(2 * N_FRAMES)] for run in range(2)]


def _pair_lists(refs, run, qi, ti):
    """oracle keypoints of a pair's query and train slot in `run` (None: the empty carry slot of the first run)"""
    if qi == CARRY:
        if run == 0:
            return None, refs[run][ti]["kps"]
        return refs[run - 1][2 * (N_FRAMES - 1)]["kps"], refs[run][ti]["kps"]
    return refs[run][qi]["kps"], refs[run][ti]["kps"]


_MATCH = {}


def _oracle_match(oracle, key, qk, tk):
    """oracle.match of one pair, once for the plain and the filtered run of a capacity"""
    if key not in _MATCH:
        _MATCH[key] = oracle.match(qk, tk)
        _MATCH[key].setflags(write=False)
    return _MATCH[key]


def _class_counts(q, t):
    """(kept, dropped, tied) queries of the ratio 4/5 + mutual filter, by the brute force"""
    nn2, rev = knn2_reference(q, t)
    keep = keep_reference(nn2, rev, THR, FLAGS, *RATIO)
    return int(keep.sum()), int((~keep).sum()), int((nn2["d1"] == nn2["d2"]).sum())


def _run_pipeline(ctx, oracle, offsets, max_kp, filtered):
    fr, refs = _pipeline_reference(oracle, offsets, max_kp)
    n_img, K = 2 * N_FRAMES, max_kp
    with _max_corners(ctx, max_kp):
        b = yv.Batch(ctx, n_img, PH, PW, K, len(PAIRS))
        try:
            b.set_pairs(PAIRS)
            if filtered:
                b.set_match_filter(ratio=RATIO, mutual=True)
            for run in range(2):
                d = _to_device(fr[run])
                b.run(d.data_ptr(), n_img, PW, PH * PW, THR, carry_from=2 * (N_FRAMES - 1))
                ctx.sync()
                kps = _assert_images(ctx, b, refs[run], K, PH, PW)
                v = b.view()
                if K <= 100:  # every slot is full
                    assert np.all(ctx.download(v.det_count, np.int32, n_img) == K)
                kpc = ctx.download(v.kp_count, np.int32, n_img + 1)
                mc = ctx.download(v.match_count, np.int32, len(PAIRS))
                fc = ctx.download(v.filt_count, np.int32, len(PAIRS))
                for p, (qi, ti) in enumerate(PAIRS):
                    msg = f"run {run} pair {p}"
                    qk, tk = _pair_lists(refs, run, qi, ti)
                    if qk is None:
                        assert mc[p] == 0 and fc[p] == 0, msg
                        continue
                    if qi == CARRY:  # the carry slot holds the previous run's last left image
                        assert kpc[CARRY] == len(qk)
                        got = ctx.download(v.keypoints + CARRY * K * 48, yv.KEYPOINT_DTYPE, kpc[CARRY])
                        np.testing.assert_array_equal(got, qk, err_msg=msg)
                    om = _oracle_match(oracle, (max_kp, run, p), qk, tk)
                    assert mc[p] == len(om) == len(qk), msg
                    m = ctx.download(v.matches + p * K * 100, yv.MATCH_DTYPE, mc[p])
                    np.testing.assert_array_equal(m, om, err_msg=msg)
                    dj = ctx.download(v.match_dj + p * K * 8, np.int32, 2 * mc[p]).reshape(-1, 2)
                    if len(tk):  # no match refers to a neighbouring slot's records
                        assert dj[:, 1].min() >= 0 and dj[:, 1].max() < len(tk), msg
                        for fld in ("x", "y", "id"):  # (a Matches record carries no descriptor)
                            np.testing.assert_array_equal(m["pt2"][fld], tk[dj[:, 1]][fld], err_msg=msg)
                        np.testing.assert_array_equal(dj[:, 0], om["distance"], err_msg=msg)
                    f = ctx.download(v.filtered + p * K * 100, yv.MATCH_DTYPE, fc[p])
                    if not filtered:
                        np.testing.assert_array_equal(f, oracle.remove_outliers(om, THR), err_msg=msg)
                        continue
                    # the batch's own keypoints (= the oracle's, asserted above) through the numpy brute force
                    bq = kps[qi] if qi != CARRY else got
                    ref_nn2, ref_rev = knn2_reference(bq, kps[ti])
                    ref_keep = keep_reference(ref_nn2, ref_rev, THR, FLAGS, *RATIO)
                    v2 = b.match2_view()
                    nn2 = ctx.download(v2.nn2 + p * K * 16, yv.MATCH2_DTYPE, len(bq))
                    rev = ctx.download(v2.rev + p * K * 4, np.int32, len(tk))
                    keep = ctx.download(v2.keep + p * K, np.uint8, len(bq)).astype(bool)
                    for fld in ("d1", "j1", "d2", "j2"):
                        np.testing.assert_array_equal(nn2[fld], ref_nn2[fld], err_msg=f"{msg} {fld}")
                    np.testing.assert_array_equal(rev, ref_rev, err_msg=msg)
                    np.testing.assert_array_equal(keep, ref_keep, err_msg=msg)
                    assert fc[p] == ref_keep.sum(), msg
                    want = m[ref_keep].copy()
                    want["pt1"]["matched"] = 1
                    want["pt2"]["matched"] = 1
                    np.testing.assert_array_equal(f, want, err_msg=msg)
        finally:
            b.close()


@gpu
@pytest.mark.parametrize("max_kp", CAPACITIES)
def test_capacity_regimes_pipeline(ctx, oracle, offsets, max_kp):
    """Images, matches and removeOutliers lists of two chained runs equal the oracle's on its own (cut) keypoint lists:
    the int8 matcher over four pairs at max_kp 4096 and 2049, the last FP4 size, and slot strides 100 / 33 / 1 with
    every slot full, where a slot's last matcher tile overlaps the next slot's records."""
    _run_pipeline(ctx, oracle, offsets, max_kp, filtered=False)


@gpu
@pytest.mark.parametrize("max_kp", FILTER_CAPACITIES)
def test_capacity_regimes_match_filter(ctx, oracle, offsets, max_kp):
    """The same runs with the ratio 4/5 + mutual filter: nn2, rev, keep, the filtered lists and the counts against
    test_gpu_match_knn2.py's brute force (the top-2 int8 kernel and the reverse int8 match, four pairs per launch, at
    4096; the FP4 kernels at slot stride 100)."""
    _run_pipeline(ctx, oracle, offsets, max_kp, filtered=True)


# ---------------------------------------------------------------------------------------------------------------------
# 4. more than 65,535 images
# ---------------------------------------------------------------------------------------------------------------------
MANY, MH, MW = 65537, 9, 16
MANY_CHECK = (0, 65534, 65535, 65536)
TAPS_255 = np.array([0, 0, 0, 0, 255, 1, 0, 0, 0], np.uint16)
MANY_NOISE_SEED = 7  # the first seed whose 9 x 16 noise holds two FAST corners


@functools.lru_cache(maxsize=None)
def _patterns():
    """all 255, all 0, noise (with FAST corners), ramp"""
    r, c = np.indices((MH, MW))
    noise = np.random.default_rng(MANY_NOISE_SEED).integers(0, 256, (MH, MW)).astype(np.uint8)
    p = np.stack([np.full((MH, MW), 255, np.uint8), np.zeros((MH, MW), np.uint8), noise,
                  ((37 * r + 11 * c) % 256).astype(np.uint8)])
    p.setflags(write=False)
    return p



@gpu
def test_more_than_65535_images(ctx, oracle, offsets):
    """65,537 images of 9 x 16, image i = pattern i % 4.  With a tap above 127 the blur is launch_blur9's: its second
    slice holds images 65,535 and 65,536.  Every image's blur, and the counts of the images around the slice boundary,
    equal the oracle's, on that route and on the fused one."""
    pat = _patterns()
    frames = pat[np.arange(MANY) % 4]
    d = _to_device(frames)
    b = yv.Batch(ctx, MANY, MH, MW, 1, 0)
    try:
        for k9 in (TAPS_255, DEFAULT_TAPS):
            ctx.set_blur_kernel(k9)
            b.run(d.data_ptr(), MANY, MW, MH * MW, THR)
            ctx.sync()
            v = b.view()
            bp = v.blur_pitch
            blur = ctx.download(v.blurred, np.uint8, MANY * MH * bp).reshape(MANY, MH, bp)[:, :, :MW]
            want = np.stack([oracle.blur(p, k9) for p in pat])
            for j in range(4):
                got = blur[j::4]
                wrong = np.flatnonzero((got != want[j]).any(axis=(1, 2)))
                assert len(wrong) == 0, f"taps {k9.tolist()}: pattern {j}, first wrong image {4 * wrong[0] + j}"
            candc = ctx.download(v.cand_count, np.uint32, MANY)
            detc = ctx.download(v.det_count, np.int32, MANY)
            kpc = ctx.download(v.kp_count, np.int32, MANY)
            for i in MANY_CHECK:
                ref = _reference(oracle, offsets, ("many", i % 4), pat[i % 4], 1, k9)
                assert (candc[i], detc[i], kpc[i]) == (ref["nc"], len(ref["rc"]), len(ref["kps"])), i
                rc = ctx.download(v.det_rc + i * 8, np.int32, 2 * detc[i]).reshape(-1, 2)
                np.testing.assert_array_equal(rc, ref["rc"], err_msg=f"image {i}")
            # and every image of a pattern has that pattern's counts
            for j in range(4):
                assert np.all(candc[j::4] == candc[j]) and np.all(detc[j::4] == detc[j]), j
    finally:
        ctx.set_blur_kernel(DEFAULT_TAPS)
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the reference alone reaches every regime (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_reaches_every_regime(oracle, offsets):
    # bank classes, the counter scan, the offsets table: occupied bands
    for name in TALL:
        H, W, max_kp, flat = SHAPES[name]
        assert (H + BAND - 1) // BAND == {"1000x64": 32, "1025x24": 33, "1100x200": 35, "8192x24": 256}[name]
        ref = _reference(oracle, offsets, (name, "synth"), _images(name)["synth"], max_kp)
        occupied = int((_bands(ref["kps"]) > 0).sum())
        print(f"{name}: {len(ref['kps'])} keypoints in {occupied} bands")
        assert occupied >= MIN_BANDS[name], name
        if flat:
            fl = _reference(oracle, offsets, (name, "flat"), _images(name)["flat"], max_kp)
            assert fl["nc"] == 0 and len(fl["kps"]) == 0 and ref["nc"] > 0
    # K > 2048 with one class: the noise image fills the slot
    ref = _reference(oracle, offsets, ("1100x200", "noise"), _images("1100x200")["noise"], 4096)
    print(f"1100x200 noise: {ref['nc']} candidates, det {len(ref['rc'])}, {len(ref['kps'])} keypoints")
    assert ref["nc"] > 4096 and len(ref["rc"]) == 4096 and len(ref["kps"]) > 2048
    # the top-K cut really cuts on every noise image
    for name, (H, W, max_kp, _) in SHAPES.items():
        ref = _reference(oracle, offsets, (name, "noise"), _images(name)["noise"], max_kp)
        print(f"{name} noise: {ref['nc']} candidates for max_kp {max_kp}")
        if name in CUT:
            assert ref["nc"] > max_kp, name
    # a band with more than 1024 keypoints
    ref = _reference(oracle, offsets, ("40x2048", "noise"), _images("40x2048")["noise"], 4096)
    print(f"40x2048 noise: bands {_bands(ref['kps']).tolist()}")
    assert _bands(ref["kps"]).max() > 1024
    # the wide shapes: samples on the column-W patch, and its four dword / two byte selections
    sel = set()
    for name in WIDE:
        H, W, max_kp, _ = SHAPES[name]
        assert W >= 1328  # more than 4 x 1024 words in a band
        sel.add(((W >> 2) & 3, 8 * (W & 3)))
        rc = _edge_points(H, W)
        for key in ("synth", "noise"):
            img = _images(name)[key]
            own = _reference(oracle, offsets, (name, key), img, max_kp)["kps"]
            placed = oracle.brief(img, rc, offsets)
            touch = sum(int(((k["y"] + 8 == W) | (k["y"] >= W - 16)).sum()) for k in (own, placed))
            hits = _register_patch_hits(own, W, offsets) + _register_patch_hits(placed, W, offsets)
            print(f"{name} {key}: {touch} keypoints at the last columns, {hits} with a register-path patch sample")
            assert touch >= 20, name
            if name not in ("25x1334", "25x1339"):
                assert hits >= 20, name
    assert {s[0] for s in sel} == {0, 1, 2, 3} and len({s[1] for s in sel}) >= 2
    assert SHAPES["40x2048"][1] & 15 == 0 and SHAPES["41x2047"][1] & 15 == 15
    # one band holding every keypoint
    for n, bad in ONE_BAND:
        img, rc = _one_band_input(n, bad)
        kps = oracle.brief(img, rc, offsets)
        nb = _bands(kps)
        print(f"one band n={n} bad={bad}: {nb.tolist()}")
        assert len(nb) == 1 and len(np.unique(rc, axis=0)) < n
        if bad == 0:
            assert nb[0] == n
        else:
            assert len(kps) == n - int(bad * n) and nb[0] > {4096: 3072, 3073: 2048, 1025: 0}[n]
    # capacities: every slot full below the corner count; lists past 2048 for the int8 matcher
    for max_kp in CAPACITIES:
        fr, refs = _pipeline_reference(oracle, offsets, max_kp)
        counts = [len(r["kps"]) for run in refs for r in run]
        cands = [r["nc"] for run in refs for r in run]
        print(f"max_kp {max_kp}: candidates {min(cands)}..{max(cands)}, keypoints {min(counts)}..{max(counts)}")
        if max_kp <= 100:
            assert min(cands) > max_kp and all(len(r["rc"]) == max_kp for run in refs for r in run)
        if max_kp > 2048:  # the int8 matcher; at 4096 every right image's list is past the FP4 matcher's 2048 as well
            right = [r for run in refs for r in run[1::2]]
            assert all(len(r["rc"]) == min(max_kp, r["nc"]) > 2048 for r in right)
            assert max_kp < 4096 or min(len(r["kps"]) for r in right) > 2048
        if max_kp == 2048:
            assert max(len(r["rc"]) for run in refs for r in run) == 2048
    # the filter runs: every class in every pair
    for max_kp in FILTER_CAPACITIES:
        _, refs = _pipeline_reference(oracle, offsets, max_kp)
        for run in range(2):
            for p, (qi, ti) in enumerate(PAIRS):
                qk, tk = _pair_lists(refs, run, qi, ti)
                if qk is None:
                    continue
                kept, dropped, tied = _class_counts(qk, tk)
                print(f"filter max_kp {max_kp} run {run} pair {p}: kept {kept}, dropped {dropped}, tied {tied}")
                assert kept >= 5 and dropped >= 5 and tied >= 5, (max_kp, run, p)
    # 65,537 images: the slices' boundary lies inside the batch and the noise pattern has corners
    assert MANY > 65535 and 65534 % 4 == 2
    noise = _reference(oracle, offsets, ("many", 2), _patterns()[2], 1)
    assert noise["nc"] >= 2 and len(noise["rc"]) == 1
