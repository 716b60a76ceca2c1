"""GPU tests of the rotation-steered BRIEF (yv_set_brief_steering, yv_orient, yv_batch_orient_view_get): records, bins
and moments against the numpy specification of tests/steer_reference.py, exact equality everywhere; with steering off
again a batch computes byte for byte what a batch that never had it on does.

The batch's view has no packed-descriptor array: the packed descriptors are what the matcher reads, so they are checked
through `matches` / `filtered`, which equal the oracle's matcher on the records."""

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd.steering import steering_tables
from ya_vo_amd.synth import synth_frame

import steer_reference as sr
from test_gpu_batch_match_filter import (FLAGS, H, K, RATIO, THR, W, _assert_same, _snapshot, d_frames,
                                         frames)  # noqa: F401 (fixtures)
from test_gpu_batch_match_gate import _check_pair as _check_gated_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables(offsets):
    return steering_tables(offsets, 32)


@pytest.fixture(autouse=True)
def _steering_off_afterwards(ctx):
    """The context is the session's: no test leaves steering on."""
    yield
    ctx.set_brief_steering(None)


def _custom_tables(n_bins, seed, extreme=False):
    """Random tables over the whole accepted range; extreme: every component is -15 or 15."""
    rng = np.random.default_rng(seed)
    dirs = rng.integers(-256, 257, (n_bins, 2)).astype(np.int16)
    if extreme:
        off = rng.choice(np.array([-15, 15], np.int8), (n_bins, 256, 4))
    else:
        off = rng.integers(-15, 16, (n_bins, 256, 4)).astype(np.int8)
        off[0, 0], off[-1, -1] = (15, -15, -15, 15), (-15, 15, 15, -15)
    return dirs, off


def _everywhere(rng, Hi, Wi, n):
    """n random positions anywhere in the image, the four corners first."""
    rc = np.stack([rng.integers(0, Hi, n), rng.integers(0, Wi, n)], 1)
    rc[:4] = [(0, 0), (0, Wi - 1), (Hi - 1, 0), (Hi - 1, Wi - 1)]
    return rc[:n]


def _check(ctx, oracle, img, rc, tabs, radius=15):
    """describe and orient of the list rc under (tabs, radius) against the specification -> (records, bin of every
    position)."""
    ctx.set_brief_steering(tabs, radius)
    b = sr.blur(oracle, img)
    rc = np.asarray(rc, np.int64).reshape(-1, 2)
    want, want_k, want_m = sr.describe_records(b, rc, tabs[0], tabs[1], radius)
    got = ctx.describe(img, rc)
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()
    mom, k = ctx.orient(img, rc)
    all_m = sr.moments(b, rc, radius)
    all_k = sr.bins(all_m, tabs[0])
    np.testing.assert_array_equal(mom, all_m)
    np.testing.assert_array_equal(k, all_k)
    # bin[id] belongs to a record
    np.testing.assert_array_equal(k[got["id"]], want_k)
    np.testing.assert_array_equal(mom[got["id"]], want_m)
    return got, k


SHAPES = {"16x16": (16, 16), "17x40": (17, 40), "120x127": (120, 127), "120x128": (120, 128), "200x320": (200, 320),
          "1100x200": (1100, 200)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_describe_and_orient_shapes(ctx, oracle, tables, name):
    """16 x 16: the only keypoint is (8, 8) and every side clamps.  120 x 127 and 120 x 128: the blur pitch is W + 1 and
    2 W, which catches pitch-for-W indexing."""
    Hi, Wi = SHAPES[name]
    rng = np.random.default_rng(Hi * 4096 + Wi)
    img = synth_frame(9, 0, 0, Hi, Wi) if name == "200x320" else rng.integers(0, 256, (Hi, Wi), dtype=np.uint8)
    if name == "16x16":
        r, c = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
        rc = np.stack([r.ravel(), c.ravel()], 1)
    else:
        rc = _everywhere(rng, Hi, Wi, 1500)
        # every class of position: the four corners of checkBoundry and of the kernel's inner region
        rc[4:8] = [(8, 8), (8, Wi - 8), (Hi - 8, 8), (Hi - 8, Wi - 8)]
        if Hi >= 31 and Wi >= 32:
            rc[8:14] = [(15, 15), (15, Wi - 17), (Hi - 16, 15), (Hi - 16, Wi - 17), (14, 15), (Hi - 16, Wi - 16)]
    got, k = _check(ctx, oracle, img, rc, tables)
    if name == "16x16":
        assert len(got) == 1 and (got["x"][0], got["y"][0], got["id"][0]) == (8, 8, 8 * 16 + 8)
    else:
        assert len(got) > 50 and len(np.unique(k)) >= 8


def test_lists(ctx, oracle, tables):
    img = synth_frame(10, 0, 0, 64, 97)
    Hi, Wi = img.shape
    rng = np.random.default_rng(5)
    ctx.set_brief_steering(tables)
    assert len(ctx.describe(img, np.zeros((0, 2), np.int32))) == 0
    mom, k = ctx.orient(img, np.zeros((0, 2), np.int32))
    assert mom.shape == (0, 2) and k.shape == (0,)
    _check(ctx, oracle, img, [(30, 40)], tables)
    _check(ctx, oracle, img, [(0, 96)], tables)  # one position that checkBoundry refuses
    # the capacity, duplicates included
    rc = _everywhere(rng, Hi, Wi, 4096)
    rc[2000:2100] = rc[100:200]
    got, _ = _check(ctx, oracle, img, rc, tables)
    assert len(got) > 2000
    # rows and columns 8, H - 8 and W - 8: the last ones checkBoundry keeps
    edge = [(r, c) for r in (8, Hi - 8) for c in range(8, Wi - 7)]
    edge += [(r, c) for c in (8, Wi - 8) for r in range(8, Hi - 7)]
    got, _ = _check(ctx, oracle, img, edge, tables)
    assert len(got) == len(edge)
    with pytest.raises(yv.YavoError) as e:
        ctx.orient(img, np.zeros((4097, 2), np.int32))
    assert e.value.status == yv.YV_ERR_CAPACITY


def test_constant_image_and_ramp(ctx, oracle, tables):
    rng = np.random.default_rng(6)
    flat = np.full((50, 70), 97, np.uint8)
    rc = _everywhere(rng, 50, 70, 300)
    _, k = _check(ctx, oracle, flat, rc, tables)
    mom, _ = ctx.orient(flat, rc)
    # a flat patch has no centroid: m10 = m01 = 0 and the first bin wins; so has a clamped one
    assert not k.any() and not mom.any()
    # brighter to the left: the centroid points to -column, bin 16 of 32, for every patch the border does not clamp
    ramp = np.tile((250 - 2 * np.arange(110)).astype(np.uint8), (60, 1))
    rc = np.stack([rng.integers(20, 40, 200), rng.integers(20, 90, 200)], 1)
    _, k = _check(ctx, oracle, ramp, rc, tables)
    mom, _ = ctx.orient(ramp, rc)
    assert (k == 16).all() and (mom[:, 0] < 0).all() and not mom[:, 1].any()


@pytest.mark.parametrize("case", ["bins1", "bins64", "custom5", "tie", "extreme"])
def test_tables(ctx, oracle, offsets, case):
    img = synth_frame(12, 0, 0, 90, 131)
    rc = _everywhere(np.random.default_rng(7), 90, 131, 1200)
    if case == "bins1":
        tabs = sr.plain_table(offsets)
    elif case == "bins64":
        tabs = steering_tables(offsets, 64)
    elif case == "custom5":
        tabs = _custom_tables(5, 50)
    elif case == "extreme":
        tabs = _custom_tables(3, 51, extreme=True)
    else:
        # bins 3 and 7 point the same way with different tests: the first index wins every tie
        dirs, off = steering_tables(offsets, 8)
        off = off.copy()
        dirs = dirs.copy()
        dirs[7] = dirs[3]
        off[7] = _custom_tables(1, 52)[1][0]
        tabs = (dirs, off)
    _, k = _check(ctx, oracle, img, rc, tabs)
    if case == "tie":
        assert (k == 3).sum() >= 20 and not (k == 7).any()
    elif case != "bins1":
        assert len(np.unique(k)) >= (32 if case == "bins64" else 2)


@pytest.mark.parametrize("radius", [1, 7, 15])
def test_radius(ctx, oracle, tables, radius):
    img = synth_frame(13, 0, 0, 70, 83)
    rc = _everywhere(np.random.default_rng(8), 70, 83, 800)
    _, k = _check(ctx, oracle, img, rc, tables, radius)
    assert len(np.unique(k)) >= 8


def test_quarter_turn_through_the_abi(ctx, tables):
    """img and np.rot90(img) at positions both sides of checkBoundry keep: equal descriptors, bins shifted by 24."""
    img = synth_frame(21, 0, 0, 120, 160)
    Hi, Wi = img.shape
    rng = np.random.default_rng(9)
    rc = np.stack([rng.integers(8, Hi - 8, 600), rng.integers(8, Wi - 8, 600)], 1)
    rc[:4] = [(8, 8), (8, Wi - 9), (Hi - 9, 8), (Hi - 9, Wi - 9)]
    rc_t = np.stack([Wi - 1 - rc[:, 1], rc[:, 0]], 1)
    ctx.set_brief_steering(tables)
    turned = np.ascontiguousarray(np.rot90(img))
    a, b = ctx.describe(img, rc), ctx.describe(turned, rc_t)
    assert len(a) == len(b) == len(rc)
    np.testing.assert_array_equal(a["id"], b["id"])
    np.testing.assert_array_equal(a["featVec"], b["featVec"])
    _, ka = ctx.orient(img, rc)
    _, kb = ctx.orient(turned, rc_t)
    np.testing.assert_array_equal((ka.astype(np.int32) + 24) % 32, kb)
    ctx.set_brief_steering(None)
    ua, ub = ctx.describe(img, rc), ctx.describe(turned, rc_t)
    assert np.median(sr.hamming(ua["featVec"], ub["featVec"])) >= 100


# ---- the batch ----
def _orient_rows(ctx, b, kp_count, max_kp):
    """The orient view's rows, cut to every slot's keypoints."""
    v = b.orient_view()
    out = []
    for i, n in enumerate(kp_count):
        n = int(n)
        out.append((ctx.download(v.bin + i * max_kp, np.uint8, n),
                    ctx.download(v.moments + i * max_kp * 8, np.int32, 2 * n).reshape(-1, 2)))
    return out


def _check_slot(kps, blurred, orient, tabs, radius=15):
    """One slot's records and orientation against the specification on the view's blurred image."""
    rc = np.stack([kps["x"], kps["y"]], 1).astype(np.int64)
    feat, k, mom = sr.describe(blurred, rc, tabs[0], tabs[1], radius)
    assert kps.tobytes() == sr.records(rc, kps["id"], feat).tobytes()
    np.testing.assert_array_equal(orient[0], k)
    np.testing.assert_array_equal(orient[1], mom)
    return k


def _check_plain_pair(oracle, snap, p, qi, ti):
    m = oracle.match(snap[f"keypoints{qi}"], snap[f"keypoints{ti}"])
    assert snap[f"matches{p}"].tobytes() == m.tobytes()
    assert snap[f"filtered{p}"].tobytes() == oracle.remove_outliers(m, THR).tobytes()


def test_batch_against_the_reference(ctx, oracle, tables, d_frames):
    """L0 R0 L1 with a stereo and a temporal pair: the keypoint set is the unsteered run's, everything the descriptor
    feeds equals the reference on the view's own blurred images and the oracle's matcher on those records."""
    pairs = [(0, 1), (0, 2)]
    b = yv.Batch(ctx, 3, H, W, K, 2)
    b.set_pairs(pairs)
    with pytest.raises(yv.YavoError) as e:
        b.orient_view()  # nothing ran with steering on yet
    assert e.value.status == yv.YV_ERR_INVALID
    b.run(d_frames.data_ptr(), 3, W, H * W, THR)
    off = _snapshot(ctx, b, 3, 2, 0)
    ctx.set_brief_steering(tables)
    with pytest.raises(yv.YavoError):
        b.orient_view()  # the arrays come with the first run
    b.run(d_frames.data_ptr(), 3, W, H * W, THR)
    on = _snapshot(ctx, b, 3, 2, 0)
    same = ("kp_count", "det_", "cand_count", "blurred", "match_count")
    _assert_same(off, on, [k for k in off if k.startswith(same)])
    orient = _orient_rows(ctx, b, on["kp_count"][:3], K)
    for i in range(3):
        for f in ("x", "y", "id"):
            np.testing.assert_array_equal(on[f"keypoints{i}"][f], off[f"keypoints{i}"][f])
        assert len(on[f"keypoints{i}"]) > 300
        k = _check_slot(on[f"keypoints{i}"], on["blurred"][i], orient[i], tables)
        assert len(np.unique(k)) >= 16
        assert (on[f"keypoints{i}"]["featVec"] != off[f"keypoints{i}"]["featVec"]).any()
    for p, (qi, ti) in enumerate(pairs):
        _check_plain_pair(oracle, on, p, qi, ti)
        assert on["filt_count"][p] > 50
    b.close()


def test_batch_envelope_shape(ctx, oracle, tables):
    """1025 x 24: 33 bands of which top-K's band lists are not read, every patch clamps on both sides."""
    import torch
    Hi, Wi, Ki = 1025, 24, 4096
    img = np.random.default_rng(1000 * Hi + Wi).integers(0, 256, (Hi, Wi)).astype(np.uint8)
    d = torch.from_numpy(img).to("cuda:0")
    torch.cuda.synchronize()
    ctx.set_fast_params(40, Ki)
    try:
        ctx.set_brief_steering(tables)
        b = yv.Batch(ctx, 1, Hi, Wi, Ki, 0)
        b.run(d.data_ptr(), 1, Wi, Hi * Wi, THR)
        ctx.sync()
    finally:
        ctx.set_fast_params(40, 2000)
    v = b.view()
    n = int(ctx.download(v.kp_count, np.int32, 1)[0])
    kps = ctx.download(v.keypoints, yv.KEYPOINT_DTYPE, n)
    blurred = ctx.download(v.blurred, np.uint8, Hi * v.blur_pitch).reshape(Hi, v.blur_pitch)[:, :Wi]
    np.testing.assert_array_equal(blurred, sr.blur(oracle, img))
    assert n > 100 and sr.inside_boundary(np.stack([kps["x"], kps["y"]], 1), Hi, Wi).all()
    _check_slot(kps, blurred, _orient_rows(ctx, b, [n], Ki)[0], tables)
    b.close()


def test_batch_with_match_filter_and_gates(ctx, tables, d_frames):
    """Steering under the other opt-in stages: the 2-NN filter and the gates work on the steered descriptors."""
    gates = [(-1, 1, -16, 0), (-4, 4, -8, 8)]
    b = yv.Batch(ctx, 3, H, W, K, 2)
    b.set_pairs([(0, 1), (0, 2)])
    b.set_match_filter(ratio=RATIO, mutual=True)
    b.set_match_gates(gates)
    ctx.set_brief_steering(tables)
    b.run(d_frames.data_ptr(), 3, W, H * W, THR)
    snap = _snapshot(ctx, b, 3, 2, 0)
    orient = _orient_rows(ctx, b, snap["kp_count"][:3], K)
    for i in range(3):
        _check_slot(snap[f"keypoints{i}"], snap["blurred"][i], orient[i], tables)
    for p, (qi, ti) in enumerate([(0, 1), (0, 2)]):
        _, keep = _check_gated_pair(ctx, b, snap, p, qi, ti, gates[p], FLAGS)
        assert 5 <= keep.sum() < len(keep)
    b.close()


def test_batch_carry(ctx, oracle, tables, d_frames):
    """Two chained runs (L0 R0, then L1 R1) with carry_from = 0: the carry slot holds the previous run's image 0 --
    records, bins and moments -- and the temporal pair matches it."""
    carry = 2
    b = yv.Batch(ctx, 2, H, W, K, 2)
    b.set_pairs([(0, 1), (carry, 0)])
    ctx.set_brief_steering(tables)
    b.run(d_frames.data_ptr(), 2, W, H * W, THR, carry_from=0)
    first = _snapshot(ctx, b, 2, 2, 0)
    first_orient = _orient_rows(ctx, b, first["kp_count"], K)
    assert first["kp_count"][carry] == 0
    b.run(d_frames.data_ptr() + 2 * H * W, 2, W, H * W, THR, carry_from=0)
    snap = _snapshot(ctx, b, 2, 2, 0)
    orient = _orient_rows(ctx, b, snap["kp_count"], K)
    assert snap["kp_count"][carry] == first["kp_count"][0] > 300
    assert snap[f"keypoints{carry}"].tobytes() == first["keypoints0"].tobytes()
    np.testing.assert_array_equal(orient[carry][0], first_orient[0][0])
    np.testing.assert_array_equal(orient[carry][1], first_orient[0][1])
    for i in range(2):
        _check_slot(snap[f"keypoints{i}"], snap["blurred"][i], orient[i], tables)
    _check_plain_pair(oracle, snap, 0, 0, 1)
    _check_plain_pair(oracle, snap, 1, carry, 0)
    assert snap["filt_count"][1] > 50
    b.close()


def test_switching_tables_and_off_again(ctx, oracle, offsets, tables, d_frames):
    pairs = [(0, 1), (0, 2)]
    never = yv.Batch(ctx, 3, H, W, K, 2)
    never.set_pairs(pairs)
    never.run(d_frames.data_ptr(), 3, W, H * W, THR)
    want_off = _snapshot(ctx, never, 3, 2, 0)
    never.close()
    b = yv.Batch(ctx, 3, H, W, K, 2)
    b.set_pairs(pairs)
    other = _custom_tables(5, 60)
    seen = []
    for tabs, radius in ((tables, 15), (other, 9)):
        ctx.set_brief_steering(tabs, radius)
        b.run(d_frames.data_ptr(), 3, W, H * W, THR)
        snap = _snapshot(ctx, b, 3, 2, 0)
        orient = _orient_rows(ctx, b, snap["kp_count"][:3], K)
        for i in range(3):
            _check_slot(snap[f"keypoints{i}"], snap["blurred"][i], orient[i], tabs, radius)
        _check_plain_pair(oracle, snap, 0, 0, 1)
        seen.append(snap["keypoints0"]["featVec"].copy())
    assert (seen[0] != seen[1]).any()
    ctx.set_brief_steering(None)
    b.run(d_frames.data_ptr(), 3, W, H * W, THR)
    _assert_same(want_off, _snapshot(ctx, b, 3, 2, 0))
    b.orient_view()  # the arrays stay; they hold the last steered run
    b.close()
