"""GPU tests of the scale pyramid (yv_batch_set_pyramid, yv_detect_describe_pyramid, yv_pyramid_image; DESIGN.md section
22) against the numpy specification of tests/pyramid_reference.py: the level images byte for byte (and against
yv_rectify_image through the formula's map), every level's keypoints against yv_detect + yv_describe on the downloaded
level image, the merge record for record, the batch's match stage on the merged slots against the host matchers, and
the benefit on a zoomed KITTI crop against the CPU oracle's counts."""
import os

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import io as yio
from ya_vo_amd import pyramid as yp
from ya_vo_amd.steering import steering_tables
from ya_vo_amd.synth import synth_frame

import pyramid_reference as pr
from test_gpu_batch_match_filter import H, K, RATIO, THR, W, _assert_same, _match2, _snapshot, d_frames, frames  # noqa: F401
from test_gpu_match_knn2 import keep_reference

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = yp.level_sizes(H, W, 3)            # (200, 320), (167, 267), (139, 222)
QUOTAS = yp.level_quotas(K, SIZES)


@pytest.fixture(autouse=True)
def _context_as_it_was(ctx):
    """The context is the session's: no test leaves steering or selection on."""
    yield
    ctx.set_brief_steering(None)
    ctx.set_keypoint_select()


def _device(imgs):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(imgs)).to("cuda:0")
    torch.cuda.synchronize()
    return d


# ---- level images ----
def _texture(shape, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    img[0, :], img[-1, :], img[:, 0], img[:, -1] = 255, 1, 2, 254  # the borders' taps are told apart
    return img


@pytest.mark.parametrize("src,dst", [((24, 40), (20, 33)), ((33, 47), (17, 24)), ((24, 40), (24, 40)),
                                     ((40, 300), (34, 251)), ((40, 300), (20, 150)), ((70, 41), (35, 21))])
def test_level_image_equals_the_specification_and_the_remap(ctx, src, dst):
    img = _texture(src, src[1])
    want = pr.resample(img, *dst)
    got = ctx.pyramid_image(img, *dst)
    assert got.tobytes() == want.tobytes()
    assert yio.rectify_image(ctx, img, pr.level_map(*src, *dst)).tobytes() == want.tobytes()
    if src == dst:
        assert got.tobytes() == img.tobytes()


@pytest.mark.parametrize("stride", [41, 43, 64])
def test_level_image_with_a_stride_above_the_width(ctx, stride):
    """Rows `stride` bytes apart, odd strides included (the staged rows then start at every alignment); the bytes
    between the rows differ from the image's and must not show."""
    big = _texture((33, stride), stride)
    img = big[:, :40]
    want = pr.resample(np.ascontiguousarray(img), 20, 33)
    assert ctx.pyramid_image(img, 20, 33).tobytes() == want.tobytes()
    # the destination's stride: the bytes between its rows stay the caller's
    dst = np.full((20, 48), 0xA5, np.uint8)
    st = ctx.lib.yv_pyramid_image(ctx.handle, big.ctypes.data, 33, 40, stride, 20, 33, dst.ctypes.data, 48)
    assert st == yv.YV_OK and dst[:, :33].tobytes() == want.tobytes() and np.all(dst[:, 33:] == 0xA5)


def _level_images(ctx, v, n_images):
    """Level l >= 1's images of the last run, [n_images, H_l, W_l] each (None for level 0)."""
    out = [None]
    for l in range(1, v.n_levels):
        raw = ctx.download(v.image[l], np.uint8, n_images * v.pitch[l]).reshape(n_images, v.H[l], v.stride[l])
        out.append(raw[:, :, :v.W[l]].copy())
    return out


def test_a_three_level_chain_in_the_batch(ctx, frames, d_frames):
    """Images L0 R0 of a pitched run: every level of every image equals the specification's chain."""
    b = yv.Batch(ctx, 2, H, W, K, 0)
    b.set_pyramid(SIZES, QUOTAS)
    b.run(d_frames.data_ptr(), 2, W, H * W, THR)
    ctx.sync()
    v = b.pyramid_view()
    assert v.n_levels == 3 and [(v.H[l], v.W[l]) for l in range(3)] == [tuple(s) for s in SIZES]
    assert list(v.keep[:3]) == QUOTAS and not v.image[0]
    got = _level_images(ctx, v, 2)
    for i in range(2):
        want = pr.build_levels(np.array(frames[i]), SIZES)
        for l in range(1, 3):
            assert got[l][i].tobytes() == want[l].tobytes(), (i, l)
    b.close()


# ---- per-level keypoints and the merge ----
def _slot(ctx, ptr, dtype, slot, n, per=1):
    item = np.dtype(dtype).itemsize * per
    return ctx.download(ptr + slot * K * item, dtype, n * per)


def _merged(ctx, b, slot):
    """(keypoints, level, level_rc) of a slot's merged list."""
    n = int(ctx.download(b.view().kp_count, np.int32, slot + 1)[slot])
    pv = b.pyramid_view()
    return (_slot(ctx, b.view().keypoints, yv.KEYPOINT_DTYPE, slot, n), _slot(ctx, pv.level, np.uint8, slot, n),
            _slot(ctx, pv.level_rc, np.int32, slot, n, 2).reshape(-1, 2))


def _check_levels_and_merge(ctx, b, imgs, sizes, quotas, steer=False):
    """After a run with the pyramid on: every level's records equal yv_detect + yv_describe on the downloaded level
    image with max_kp = the level's quota, and the slot holds the specification's merge of them -> per image the
    levels' keypoint counts."""
    ctx.sync()
    n_images, L = len(imgs), len(sizes)
    v, pv = b.view(), b.pyramid_view()
    lv_imgs = _level_images(ctx, pv, n_images)
    counts = []
    for i in range(n_images):
        per, bins, moms = [], [], []
        for l in range(L):
            img = imgs[i] if l == 0 else lv_imgs[l][i]
            rc, _, _ = ctx.detect(img, quotas[l])
            want = ctx.describe(img, rc)
            n_det = int(ctx.download(pv.det_count[l], np.int32, n_images)[i])
            n_kp = int(ctx.download(pv.kp_count[l], np.int32, n_images)[i])
            assert (n_det, n_kp) == (len(rc), len(want)), (i, l)
            got = _slot(ctx, pv.keypoints[l], yv.KEYPOINT_DTYPE, i, n_kp)
            assert got.tobytes() == want.tobytes(), (i, l)
            per.append(want)
            if steer:
                mom, bn = ctx.orient(img, rc)
                bins.append(bn[want["id"]])
                moms.append(mom[want["id"]])
        want, want_level, want_rc = pr.merge(per, sizes)
        got, level, rc = _merged(ctx, b, i)
        assert len(got) == len(want) == sum(len(p) for p in per)
        assert got.tobytes() == want.tobytes(), i
        assert level.tobytes() == want_level.tobytes() and rc.tobytes() == want_rc.tobytes(), i
        assert got["x"].max(initial=0) < sizes[0][0] and got["y"].max(initial=0) < sizes[0][1]
        if steer:
            ov = b.orient_view()
            assert _slot(ctx, ov.bin, np.uint8, i, len(got)).tobytes() == np.concatenate(bins).tobytes(), i
            assert _slot(ctx, ov.moments, np.int32, i, len(got), 2).tobytes() == np.concatenate(moms).tobytes(), i
        # the base view's detect arrays stay level 0's
        assert int(ctx.download(v.det_count, np.int32, n_images)[i]) == len(ctx.detect(imgs[i], quotas[0])[0])
        counts.append([len(p) for p in per])
    return counts


@pytest.mark.parametrize("select", [False, True], ids=["cut", "select"])
@pytest.mark.parametrize("steer", [False, True], ids=["brief", "steered"])
def test_levels_equal_detect_and_describe_and_the_slot_their_merge(ctx, offsets, frames, d_frames, steer, select):
    if steer:
        ctx.set_brief_steering(steering_tables(offsets, 32))
    if select:
        ctx.set_keypoint_select(3, (32, 32), 6)
    b = yv.Batch(ctx, 2, H, W, K, 0)
    b.set_pyramid(SIZES, QUOTAS)
    b.run(d_frames.data_ptr(), 2, W, H * W, THR)
    counts = _check_levels_and_merge(ctx, b, [np.array(frames[0]), np.array(frames[1])], SIZES, QUOTAS, steer)
    print("keypoints per level:", counts)
    assert all(min(c) > 20 for c in counts)  # every level contributes
    b.close()


def _run_one(ctx, img, sizes, quotas):
    """A one-image batch run with the pyramid on -> the per-level keypoint counts (all checks applied)."""
    b = yv.Batch(ctx, 1, img.shape[0], img.shape[1], K, 0)
    b.set_pyramid(sizes, quotas)
    d = _device(img[None])
    b.run(d.data_ptr(), 1, img.shape[1], img.size, THR)
    counts = _check_levels_and_merge(ctx, b, [img], sizes, quotas)[0]
    # the host-pointer form gives the same list
    got = ctx.detect_describe_pyramid(img, sizes, quotas)
    want = _merged(ctx, b, 0)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    pv = b.pyramid_view()
    dets = [int(ctx.download(pv.det_count[l], np.int32, 1)[0]) for l in range(len(sizes))]
    b.close()
    return counts, dets


def test_merge_with_a_quota_of_zero_in_the_middle(ctx):
    img = synth_frame(5, 0, 0, 96, 160)
    sizes = yp.level_sizes(96, 160, 3)
    counts, dets = _run_one(ctx, img, sizes, [300, 0, 200])
    assert counts[0] > 0 and counts[1] == 0 and counts[2] > 0 and dets[1] == 0


def test_merge_with_quotas_the_corners_do_not_fill(ctx):
    img = synth_frame(6, 0, 0, 96, 160)
    sizes = yp.level_sizes(96, 160, 4)
    quotas = [800, 500, 400, 300]
    counts, dets = _run_one(ctx, img, sizes, quotas)
    assert all(0 < d < q for d, q in zip(dets, quotas)) and all(c > 0 for c in counts)


def test_merge_with_quotas_that_cut_every_level(ctx):
    img = synth_frame(7, 0, 0, 96, 160)
    sizes = yp.level_sizes(96, 160, 3)
    quotas = [40, 7, 1]
    counts, dets = _run_one(ctx, img, sizes, quotas)
    assert dets == quotas


def test_merge_with_levels_whose_corners_all_fail_checkBoundry(ctx):
    """A level of fewer than 16 rows has corners (FAST tests rows 4 .. H - 5) and none with 8 <= row <= H - 8."""
    img = synth_frame(8, 0, 0, 28, 200)
    sizes = [(28, 200), (15, 167), (12, 139)]
    counts, dets = _run_one(ctx, img, sizes, [300, 200, 100])
    assert counts[0] > 0 and counts[1:] == [0, 0] and dets[1] > 0 and dets[2] > 0


def test_merge_with_flat_levels(ctx):
    """Stripes of period 2 under a shrink of exactly 2: every later level is flat and holds no corner (a flat level
    makes every level after it flat: the empty level between two others is the quota-of-zero case above)."""
    img = synth_frame(9, 0, 0, 64, 128).copy()
    img[:, 0::2], img[:, 1::2] = np.minimum(img[:, 0::2], 60), 255 - np.minimum(img[:, 0::2], 60)
    sizes = [(64, 128), (32, 64), (27, 53)]
    b = yv.Batch(ctx, 1, 64, 128, K, 0)
    b.set_pyramid(sizes, [500, 300, 200])
    d = _device(img[None])
    b.run(d.data_ptr(), 1, 128, img.size, THR)
    counts = _check_levels_and_merge(ctx, b, [img], sizes, [500, 300, 200])[0]
    lv = _level_images(ctx, b.pyramid_view(), 1)
    assert np.ptp(lv[1][0][:, 1:-1]) <= 1 and counts[1:] == [0, 0]
    b.close()


def test_argument_checks_on_a_batch(ctx):
    b = yv.Batch(ctx, 1, 96, 160, 500, 0)
    with pytest.raises(yv.YavoError) as e:
        b.pyramid_view()  # invalid until the pyramid was switched on
    assert e.value.status == yv.YV_ERR_INVALID
    for sizes, quotas, status in (([(96, 161), (80, 133)], [1, 1], yv.YV_ERR_INVALID),
                                  ([(96, 160), (47, 133)], [1, 1], yv.YV_ERR_INVALID),
                                  ([(96, 160), (80, 133)], [1, -1], yv.YV_ERR_INVALID),
                                  ([(96, 160), (80, 133)], [400, 101], yv.YV_ERR_CAPACITY)):
        with pytest.raises(yv.YavoError) as e:
            b.set_pyramid(sizes, quotas)
        assert e.value.status == status, (sizes, quotas)
    b.set_pyramid([(96, 160), (80, 133)], [400, 100])
    assert b.pyramid_view().n_levels == 2
    b.set_pyramid(None)
    b.close()


# ---- the batch: carry slot, match stage, off again ----
GATES = [(-6, 6, -24, 8), (-10, 10, -16, 16)]


def _lists(ctx, b, n_slots):
    return [_merged(ctx, b, s) for s in range(n_slots)]


@pytest.fixture(scope="module")
def two_runs(ctx, d_frames):
    """A batch of 2 images + the carry slot: run 1 on (L0, R0) carrying L0, run 2 on (L1, R1); pairs (L1, R1) stereo
    and (carry = L0, L1) temporal.  -> (batch, the merged lists of run 1's slots, run 2's snapshot and lists)."""
    b = yv.Batch(ctx, 2, H, W, K, 2)
    b.set_pairs([(0, 1), (2, 0)])
    b.set_pyramid(SIZES, QUOTAS)
    b.run(d_frames.data_ptr(), 2, W, H * W, THR, carry_from=0)
    ctx.sync()
    first = _lists(ctx, b, 2)
    b.run(d_frames.data_ptr() + 2 * H * W, 2, W, H * W, THR, carry_from=0)
    snap = _snapshot(ctx, b, 2, 2, 0)
    yield b, first, snap, _lists(ctx, b, 3)
    b.close()


def test_the_carry_slot_holds_the_first_runs_list_and_sidecar(ctx, two_runs):
    b, first, snap, lists = two_runs
    for got, want in zip(lists[2], first[0]):
        assert len(want) > 100 and got.tobytes() == want.tobytes()
    assert lists[2][1].max() == 2  # keypoints of every level were carried
    pv = b.pyramid_view()
    n0 = ctx.download(pv.kp_count[0], np.int32, 3)
    assert n0[2] == (first[0][1] == 0).sum() and n0[0] == (lists[0][1] == 0).sum()


def test_match_stage_on_the_merged_slots_equals_the_host_matchers(ctx, two_runs):
    b, _, snap, lists = two_runs
    for p, (qi, ti) in enumerate([(0, 1), (2, 0)]):
        kq, kt = lists[qi][0], lists[ti][0]
        m = ctx.match_features(kq, kt)
        f = ctx.filter_matches(m, THR)
        assert snap["match_count"][p] == len(kq) and snap["filt_count"][p] == len(f) > 20
        np.testing.assert_array_equal(snap[f"match_dj{p}"][:, 0], m["distance"])
        np.testing.assert_array_equal(snap[f"matches{p}"], m)
        np.testing.assert_array_equal(snap[f"filtered{p}"], f)
        dj = snap[f"match_dj{p}"]
        np.testing.assert_array_equal(kt["id"][dj[:, 1]], m["pt2"]["id"])
        # matches reach into the upper levels on both sides
        assert (lists[qi][1][f["pt1"]["id"]] > 0).sum() > 5 and (lists[ti][1][f["pt2"]["id"]] > 0).sum() > 5


def test_gate_and_filter_on_the_merged_slots(ctx, two_runs, d_frames):
    b, _, _, _ = two_runs
    flags = yv.YV_MATCH_RATIO | yv.YV_MATCH_MUTUAL
    try:
        # the 2-NN filter alone: yv_match_robust on the same lists
        b.set_match_filter(ratio=RATIO, mutual=True)
        b.run(d_frames.data_ptr() + 2 * H * W, 2, W, H * W, THR)
        snap, lists = _snapshot(ctx, b, 2, 2, 0), _lists(ctx, b, 3)
        for p, (qi, ti) in enumerate([(0, 1), (2, 0)]):
            f, keep = ctx.match_robust(lists[qi][0], lists[ti][0], THR, RATIO, True)
            assert snap["filt_count"][p] == len(f) > 10
            np.testing.assert_array_equal(snap[f"filtered{p}"], f)
            np.testing.assert_array_equal(_match2(ctx, b, p, len(keep), len(lists[ti][0]))[2], keep)
        # gates under it: yv_match_gated on the same lists, and the filter's rule on its result
        b.set_match_gates(GATES)
        b.run(d_frames.data_ptr() + 2 * H * W, 2, W, H * W, THR)
        snap, lists = _snapshot(ctx, b, 2, 2, 0), _lists(ctx, b, 3)
        for p, (qi, ti) in enumerate([(0, 1), (2, 0)]):
            kq, kt = lists[qi][0], lists[ti][0]
            ref_nn2, ref_rev = ctx.match_gated(kq, kt, GATES[p])
            nn2, rev, keep = _match2(ctx, b, p, len(kq), len(kt))
            assert nn2.tobytes() == ref_nn2.tobytes() and rev.tobytes() == ref_rev.tobytes()
            ref_keep = keep_reference(ref_nn2, ref_rev, THR, flags, *RATIO)
            np.testing.assert_array_equal(keep, ref_keep)
            np.testing.assert_array_equal(snap[f"match_dj{p}"][:, 1], ref_nn2["j1"])
            assert snap["filt_count"][p] == ref_keep.sum() > 10
    finally:
        b.set_match_gates(None)
        b.set_match_filter()


def test_switched_off_again_it_is_the_single_scale_run(ctx, two_runs, d_frames):
    """The batch that ran multi-scale, switched off, against a batch that never saw a pyramid: two chained runs, every
    view array byte for byte."""
    used, _, _, _ = two_runs
    fresh = yv.Batch(ctx, 2, H, W, K, 2)
    fresh.set_pairs([(0, 1), (2, 0)])
    used.set_pyramid(None)
    snaps = []
    for b in (fresh, used):
        b.run(d_frames.data_ptr(), 2, W, H * W, THR, carry_from=0)
        b.run(d_frames.data_ptr() + 2 * H * W, 2, W, H * W, THR, carry_from=0)
        snaps.append(_snapshot(ctx, b, 2, 2, 0))
    used.set_pyramid(SIZES, QUOTAS)
    fresh.close()
    assert snaps[0]["filt_count"].min() > 20
    _assert_same(snaps[0], snaps[1])


# ---- the benefit under a change of scale ----
ZOOM, ZOOM_KP = 1.4, 500


def test_more_correct_matches_under_a_zoom_and_the_oracles_counts(ctx, oracle, offsets):
    """The KITTI crop `epilines` against its copy shrunk by 1.4 about the centre (the specification's resample on a
    canvas of the crop's size): the matches removeOutliers keeps whose train point lies within 2 px of the query's true
    position, single-scale and with 4 levels at 1.2.  The GPU's counts are the CPU oracle's, and the pyramid's is the
    larger (47 single-scale, 144 with the pyramid)."""
    img = np.load(os.path.join(GOLDEN, "kitti_crops.npz"))["epilines"]
    canvas, small, origin = pr.zoom_out(img, ZOOM)
    d = _device(np.stack([img, canvas]))
    b = yv.Batch(ctx, 2, img.shape[0], img.shape[1], ZOOM_KP, 1)
    b.set_pairs([(0, 1)])
    result = {}
    for name, n_levels in (("single", 1), ("pyramid", 4)):
        sizes = yp.level_sizes(*img.shape, n_levels)
        quotas = yp.level_quotas(ZOOM_KP, sizes)
        b.set_pyramid(sizes, quotas)
        b.run(d.data_ptr(), 2, img.shape[1], img.size, THR)
        ctx.sync()
        v = b.view()
        nf = int(ctx.download(v.filt_count, np.int32, 1)[0])
        got = ctx.download(v.filtered, yv.MATCH_DTYPE, nf)
        kq = pr.oracle_keypoints(oracle, img, sizes, quotas, offsets)[0]
        kt = pr.oracle_keypoints(oracle, canvas, sizes, quotas, offsets)[0]
        want = oracle.remove_outliers(oracle.match(kq, kt), THR)
        result[name] = (pr.correct_matches(got, img.shape, small, origin), len(got),
                        pr.correct_matches(want, img.shape, small, origin), len(want))
        print(f"{name}: GPU {result[name][0]} correct of {result[name][1]} kept, oracle {result[name][2]} of "
              f"{result[name][3]}")
        np.testing.assert_array_equal(got, want)
    b.close()
    for name in result:
        assert result[name][:2] == result[name][2:], name
    assert result["pyramid"][0] > result["single"][0] > 0
