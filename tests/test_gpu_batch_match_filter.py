"""GPU tests of the batch's match filter (yv_batch_set_match_filter): off, it changes nothing; on, every array equals
the numpy brute force of test_gpu_match_knn2.py computed from the batch's own keypoints, and the track builders (match
and LK mode) use exactly the kept matches.

The images are crops of one synthetic field into which a block of its own texture is pasted a second time, so the
keypoints inside the two copies have identical descriptors: ratio-test failures next to clean matches."""
import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import scene
from ya_vo_amd.synth import synth_frame

from test_gpu_match_knn2 import keep_reference, knn2_reference

pytestmark = pytest.mark.gpu

H, W, K = 200, 320, 2000
THR = 20
RATIO = (4, 5)
FLAGS = yv.YV_MATCH_RATIO | yv.YV_MATCH_MUTUAL
T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def _frames():
    """L0, R0, L1, R1: frame k is the crop at (k, 3 k) of the field, its right image 8 columns further."""
    world = synth_frame(77, 0, 0, H + 2, W + 12).copy()
    world[100:180, 170:290] = world[10:90, 20:140]  # repeated texture
    return np.stack([world[k:k + H, c:c + W] for k in (0, 1) for c in (3 * k, 3 * k + 8)])


@pytest.fixture(scope="module")
def frames():
    f = _frames()
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def d_frames(frames):
    import torch
    d = torch.from_numpy(np.array(frames)).to("cuda:0")
    torch.cuda.synchronize()
    return d


def _pose_buffers(n):
    import torch
    d_prior = torch.from_numpy(np.tile(IDENTITY, (n, 1))).to("cuda:0")
    d_pose = torch.zeros((n, 7), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    return d_prior, d_pose


def _snapshot(ctx, b, n_images, n_pairs, n_tracks):
    """Every yv_batch_view array, cut to the entries the run wrote."""
    ctx.sync()
    b.track_sync()
    v = b.view()
    ns = n_images + 1
    s = {"cand_count": ctx.download(v.cand_count, np.uint32, ns), "det_count": ctx.download(v.det_count, np.int32, ns),
         "kp_count": ctx.download(v.kp_count, np.int32, ns),
         "match_count": ctx.download(v.match_count, np.int32, n_pairs),
         "filt_count": ctx.download(v.filt_count, np.int32, n_pairs),
         "match_lim": ctx.download(v.match_lim, np.int32, n_pairs)}
    blur = ctx.download(v.blurred, np.uint8, n_images * H * v.blur_pitch).reshape(n_images, H, v.blur_pitch)
    s["blurred"] = blur[:, :, :W].copy()
    for i in range(ns):
        nd, nk = int(s["det_count"][i]), int(s["kp_count"][i])
        s[f"det_rc{i}"] = ctx.download(v.det_rc + i * K * 8, np.int32, 2 * nd)
        s[f"det_resp{i}"] = ctx.download(v.det_resp + i * K * 4, np.float32, nd)
        s[f"keypoints{i}"] = ctx.download(v.keypoints + i * K * 48, yv.KEYPOINT_DTYPE, nk)
    for p in range(n_pairs):
        nm, nf = int(s["match_count"][p]), int(s["filt_count"][p])
        s[f"matches{p}"] = ctx.download(v.matches + p * K * 100, yv.MATCH_DTYPE, nm)
        s[f"filtered{p}"] = ctx.download(v.filtered + p * K * 100, yv.MATCH_DTYPE, nf)
        s[f"match_dj{p}"] = ctx.download(v.match_dj + p * K * 8, np.int32, 2 * nm).reshape(-1, 2)
    if n_tracks:
        s["edge_count"] = ctx.download(v.edge_count, np.int32, n_tracks)
        s["track_inliers"] = ctx.download(v.track_inliers, np.int32, n_tracks)
        for t in range(n_tracks):
            ne = int(s["edge_count"][t])
            s[f"edge_X{t}"] = ctx.download(v.edge_X + t * K * 24, np.float64, 3 * ne).reshape(-1, 3)
            s[f"edge_uv{t}"] = ctx.download(v.edge_uv + t * K * 16, np.float64, 2 * ne).reshape(-1, 2)
            s[f"edge_query{t}"] = ctx.download(v.edge_query + t * K * 4, np.int32, ne)
            s[f"edge_outlier{t}"] = ctx.download(v.edge_outlier + t * K, np.uint8, ne)
    return s


def _match2(ctx, b, p, nq, nt):
    v = b.match2_view()
    nn2 = ctx.download(v.nn2 + p * K * 16, yv.MATCH2_DTYPE, nq)
    rev = ctx.download(v.rev + p * K * 4, np.int32, nt)
    keep = ctx.download(v.keep + p * K, np.uint8, nq)
    return nn2, rev, keep.astype(bool)


def _check_pair(ctx, b, snap, p, qi, ti, flags=FLAGS, ratio=RATIO):
    """Pair p (query image qi, train image ti) of a run with the filter on, against the brute force."""
    kq, kt = snap[f"keypoints{qi}"], snap[f"keypoints{ti}"]
    ref_nn2, ref_rev = knn2_reference(kq, kt)
    if not flags & yv.YV_MATCH_MUTUAL:
        ref_rev_out = np.full(len(kt), -1, np.int32)  # not computed
    else:
        ref_rev_out = ref_rev
    ref_keep = keep_reference(ref_nn2, ref_rev, THR, flags, *ratio)
    nn2, rev, keep = _match2(ctx, b, p, len(kq), len(kt))
    for f in ("d1", "j1", "d2", "j2"):
        np.testing.assert_array_equal(nn2[f], ref_nn2[f], err_msg=f"pair {p} {f}")
    np.testing.assert_array_equal(rev, ref_rev_out, err_msg=f"pair {p} rev")
    np.testing.assert_array_equal(keep, ref_keep, err_msg=f"pair {p} keep")
    assert snap["match_count"][p] == len(kq) and snap["filt_count"][p] == ref_keep.sum()
    want = snap[f"matches{p}"][ref_keep].copy()
    want["pt1"]["matched"] = 1
    want["pt2"]["matched"] = 1
    np.testing.assert_array_equal(snap[f"filtered{p}"], want, err_msg=f"pair {p} filtered")
    return ref_nn2, ref_keep


def _assert_same(a, b, keys=None):
    assert a.keys() == b.keys()
    for k in (keys or a.keys()):
        assert a[k].tobytes() == b[k].tobytes(), k


def _match_batch(ctx):
    """Images L0 R0 L1 R1; pairs (L1, R1) stereo and (L0, L1) temporal; one track."""
    b = yv.Batch(ctx, 4, H, W, K, 2)
    b.set_pairs([(2, 3), (0, 2)])
    b.set_tracks([(0, 1)], scene.K_KITTI, T_RIGHT)
    return b


def test_view_needs_the_filter_switched_on_once(ctx):
    b = yv.Batch(ctx, 1, H, W, K, 1)
    with pytest.raises(yv.YavoError) as e:
        b.match2_view()
    assert e.value.status == yv.YV_ERR_INVALID
    b.set_match_filter()  # flags = 0: still nothing allocated
    with pytest.raises(yv.YavoError):
        b.match2_view()
    with pytest.raises(yv.YavoError):
        b.set_match_filter(ratio=(5, 4))
    b.set_match_filter(ratio=RATIO)
    assert b.match2_view().keep
    b.close()


def test_filter_off_changes_nothing(ctx, d_frames):
    """A batch whose filter was switched on and off again computes byte for byte what an untouched batch does."""
    d_prior, d_pose = _pose_buffers(1)
    snaps = []
    for toggled in (False, True):
        b = _match_batch(ctx)
        if toggled:
            b.set_match_filter(ratio=RATIO, mutual=True)
            b.set_match_filter()
        b.run(d_frames.data_ptr(), 4, W, H * W, THR)
        b.track(d_prior.data_ptr(), d_pose.data_ptr())
        snaps.append(_snapshot(ctx, b, 4, 2, 1))
        snaps[-1]["pose"] = d_pose.cpu().numpy()
        b.close()
    assert snaps[0]["edge_count"][0] > 0 and snaps[0]["filt_count"].min() > 0
    _assert_same(snaps[0], snaps[1])


@pytest.fixture(scope="module")
def off_on(ctx, d_frames):
    """One batch: a run + track with the filter off, then the same with ratio 4/5 + mutual."""
    d_prior, d_pose = _pose_buffers(1)
    b = _match_batch(ctx)
    out = []
    for on in (False, True):
        b.set_match_filter(ratio=RATIO if on else None, mutual=on)
        b.run(d_frames.data_ptr(), 4, W, H * W, THR)
        b.track(d_prior.data_ptr(), d_pose.data_ptr())
        out.append(_snapshot(ctx, b, 4, 2, 1))
    yield b, out[0], out[1]
    b.close()


def test_filter_on_equals_brute_force(ctx, off_on):
    b, off, on = off_on
    for p, (qi, ti) in enumerate([(2, 3), (0, 2)]):
        nn2, keep = _check_pair(ctx, b, on, p, qi, ti)
        # the repeated texture is there: both outcomes of both tests, and ties
        assert 5 <= keep.sum() <= len(keep) - 5
        assert (nn2["d1"] == nn2["d2"]).sum() >= 5
    # matches, match_dj and match_lim do not change meaning
    keys = [k for k in off if k.startswith(("matches", "match_dj", "match_lim", "match_count", "keypoints", "kp_count"))]
    _assert_same(off, on, keys)
    assert np.all(on["filt_count"] < off["filt_count"])


def _check_edges(off, on, kept_edge):
    """Edges with the filter on = the edges with it off whose matches are kept, same order, same bits."""
    n_off, n_on = int(off["edge_count"][0]), int(on["edge_count"][0])
    assert 0 < n_on < n_off
    assert kept_edge.sum() == n_on
    np.testing.assert_array_equal(on["edge_query0"], off["edge_query0"][kept_edge])
    assert on["edge_X0"].tobytes() == off["edge_X0"][kept_edge].tobytes()
    assert on["edge_uv0"].tobytes() == off["edge_uv0"][kept_edge].tobytes()


def test_track_edges_use_kept_matches_only(ctx, off_on):
    b, off, on = off_on
    _, _, keep_s = _match2(ctx, b, 0, len(on["keypoints2"]), len(on["keypoints3"]))
    _, _, keep_t = _match2(ctx, b, 1, len(on["keypoints0"]), len(on["keypoints2"]))
    q = off["edge_query0"]                 # temporal query i of every edge
    j1 = off["match_dj1"][q, 1]            # its frame-k keypoint, the stereo pair's query
    _check_edges(off, on, keep_t[q] & keep_s[j1])


def test_lk_stereo_points_use_kept_matches_only(ctx, d_frames):
    """LK mode: frame k-1's map points are its stereo matches; with the filter on, the kept ones only (every point is
    tracked on its own, so the surviving edges keep their bits)."""
    d_prior, d_pose = _pose_buffers(1)
    b = yv.Batch(ctx, 4, H, W, K, 2)
    b.set_pairs([(0, 1), (2, 3)])
    b.set_track_lk(2)
    b.set_tracks([(0, 2)], scene.K_KITTI, T_RIGHT)  # {stereo pair of frame 0, image L1}
    snaps = []
    for on in (False, True):
        b.set_match_filter(ratio=RATIO if on else None, mutual=on)
        b.run(d_frames.data_ptr(), 4, W, H * W, THR)
        b.track(d_prior.data_ptr(), d_pose.data_ptr())
        snaps.append(_snapshot(ctx, b, 4, 2, 1))
    off, on = snaps
    _check_pair(ctx, b, on, 0, 0, 1)
    _, _, keep_s = _match2(ctx, b, 0, len(on["keypoints0"]), len(on["keypoints1"]))
    _check_edges(off, on, keep_s[off["edge_query0"]])
    b.close()


def test_two_runs_through_the_carry_slot(ctx, d_frames):
    """Consecutive runs reuse the key buffers: run 2 (temporal pair = carry slot -> L1) still equals the brute force,
    for the ratio test alone (no reverse match) and then for both tests on the same batch."""
    b = yv.Batch(ctx, 2, H, W, K, 2)
    carry = 2
    b.set_pairs([(0, 1), (carry, 0)])
    for flags, kw in ((yv.YV_MATCH_RATIO, dict(ratio=RATIO)), (FLAGS, dict(ratio=RATIO, mutual=True)),
                      (yv.YV_MATCH_RATIO, dict(ratio=RATIO))):
        b.set_match_filter(**kw)
        for k in range(2):
            b.run(d_frames.data_ptr() + 2 * k * H * W, 2, W, H * W, THR, carry_from=0)
            snap = _snapshot(ctx, b, 2, 2, 0)
            _check_pair(ctx, b, snap, 0, 0, 1, flags)
            _, keep = _check_pair(ctx, b, snap, 1, carry, 0, flags)
        assert len(snap[f"keypoints{carry}"]) > 100 and 5 <= keep.sum() < len(keep)
    b.close()
