"""GPU tests of the handles' lifecycle paths (ya_vo_amd/csrc/yavo_host.h HipOwned and its users): the single-image
workspace replaced when the image size changes, the batch's track buffers grown by a later set_tracks, and every kind
of handle created, used and destroyed over and over.  Each test compares a handle that went through such a path with a
fresh one, bit for bit; none of them looks at a number the kernels could change."""
import os

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import scene
from ya_vo_amd.steering import steering_tables
from ya_vo_amd.synth import synth_frame, synth_stereo_batch

from track_chain import IDENTITY

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
# small frames in which the oracle still finds >= 16 keypoints (21 and 28 after the boundary check; 13 at 32 x 64)
H, W = 48, 64
H2, W2 = 40, 80
MAX_KP = 256


def _configured_context():
    """A context of its own with keypoint selection and steering on and the committed BRIEF offsets."""
    offsets = np.fromfile(os.path.join(TESTS, "golden", "brief_offsets_mt19937_42.bin"), np.int8).reshape(256, 4)
    c = yv.Context(0)
    c.set_brief_offsets(offsets)
    c.set_keypoint_select(nms_radius=2, cell=(16, 16), per_cell=8)
    c.set_brief_steering(steering_tables(offsets, 32))
    return c


def _front_end(c, img):
    """detect + describe + orient of img, then the three host matchers that allocate the workspace's filter and gate
    buffers, on img's own keypoints -> every result, in one list."""
    rc, resp, n_cand = c.detect(img, MAX_KP)
    kp = c.describe(img, rc)
    mom, bins = c.orient(img, rc)
    t = kp[::-1].copy()
    nn2, rev = c.match_knn2(kp, t)
    gnn2, grev = c.match_gated(kp, t, (-8, 8, -8, 8))
    kept, keep = c.match_robust(kp, t, 20, (4, 5), True)
    return [rc, resp, np.int64(n_cand), kp, mom, bins, nn2, rev, gnn2, grev, kept, keep]


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_single_image_workspace_replaced(oracle, offsets):
    """One context through images of two sizes and back: the workspace (with its selection, steering, filter and gate
    buffers) is freed and recreated at each change, and every call returns what a fresh context returns."""
    A, B = synth_frame(81, 0, 0, H, W), synth_frame(82, 0, 0, H2, W2)
    for img in (A, B):
        assert len(oracle.brief(img, oracle.fast(img, 2000)[0], offsets)) >= 16
    want = []
    for img in (A, B):
        fresh = _configured_context()
        want.append(_front_end(fresh, img))
        fresh.close()
    assert len(want[0][3]) > 0 and len(want[1][3]) > 0  # keypoints survive the selection: the matchers ran
    c = _configured_context()
    for img, w in ((A, want[0]), (B, want[1]), (A, want[0])):
        _assert_same(_front_end(c, img), w)
    c.close()


# images L0 R0 L1 R1 (4 = the carry slot): temporal and stereo pairs as tests/test_gpu_track.py chains them, and a
# second temporal pair into L1, so three tracks differ
PAIRS = [(4, 0), (0, 1), (0, 2), (2, 3), (4, 2)]
TRACKS = [(1, 0), (3, 2), (3, 4)]     # (stereo pair, temporal pair)
LK_TRACKS = [(1, 2), (3, 0), (1, 0)]  # (stereo pair of frame k-1, image of frame k)


def _two_steps(ctx, d_runs, first_tracks, overlap, lk):
    """Two run + track steps of a new batch, the first with first_tracks tracks and the second with all three ->
    (poses, inlier counts, edge counts) of the second step."""
    import torch
    b = yv.Batch(ctx, 4, H, W, MAX_KP, len(PAIRS))
    b.set_pairs(PAIRS)
    if lk:
        b.set_track_lk(2, win=3, max_level=0)  # the smallest window, one level
    b.set_track_overlap(overlap)
    tracks = LK_TRACKS if lk else TRACKS
    d_prior = torch.from_numpy(np.tile(IDENTITY, (3, 1))).to("cuda:0")
    d_pose = [torch.zeros((3, 7), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    b.set_tracks(tracks[:first_tracks], scene.K_KITTI, T_RIGHT)
    b.run(d_runs[0].data_ptr(), 4, W, H * W, 20, carry_from=2)
    b.track(d_prior.data_ptr(), d_pose[0].data_ptr())
    if first_tracks < 3:
        b.set_tracks(tracks, scene.K_KITTI, T_RIGHT)  # more tracks than the buffers hold: they are replaced
    b.run(d_runs[1].data_ptr(), 4, W, H * W, 20, carry_from=2)
    b.track(d_prior.data_ptr(), d_pose[1].data_ptr())
    ctx.sync()
    b.track_sync()
    v = b.view()
    assert v.n_tracks == 3
    out = (d_pose[1].cpu().numpy(), ctx.download(v.track_inliers, np.int32, 3).copy(),
           ctx.download(v.edge_count, np.int32, 3).copy())
    b.close()
    return out


@pytest.fixture(scope="module")
def stereo_runs():
    """Two runs of two stereo frames each, on the device."""
    import torch
    d = [torch.from_numpy(synth_stereo_batch(91, 2, 2 * r, H, W)).to("cuda:0") for r in range(2)]
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("lk", [False, True], ids=["match", "lk"])
@pytest.mark.parametrize("overlap", [0, 1])
def test_track_buffers_grown(ctx, stereo_runs, overlap, lk):
    """set_tracks with one track, a step, then set_tracks with three (the track group is freed and allocated again), a
    step: the same poses, inlier counts and edge counts as a batch that was given the three tracks at once."""
    want = _two_steps(ctx, stereo_runs, 3, overlap, lk)
    assert want[2].sum() > 0  # some track has edges (17 and 18 in the oracle chain's match tracker at this size)
    got = _two_steps(ctx, stereo_runs, 1, overlap, lk)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def _round(c, d_images):
    """One handle of every kind on context c, one small call on each, all closed again -> the batch's outputs."""
    import torch
    b = yv.Batch(c, 4, H, W, MAX_KP, 2)
    b.set_pairs([(0, 1), (2, 3)])
    b.set_match_filter(ratio=(4, 5), mutual=True)
    b.set_match_gates([(-4, 4, -16, 16), (-4, 4, -16, 16)])
    b.run(d_images.data_ptr(), 4, W, H * W, 20)  # the context's selection and steering: their buffers, too
    c.sync()
    v, o = b.view(), b.orient_view()
    n = c.download(v.kp_count, np.int32, 4).copy()
    out = [n, c.download(v.keypoints, yv.KEYPOINT_DTYPE, 4 * MAX_KP).copy(),
           c.download(v.filt_count, np.int32, 2).copy(), c.download(o.bin, np.uint8, 4 * MAX_KP).copy()]
    lk = yv.Lk(c, 2, H, W, 3, 0)
    lk.build(d_images.data_ptr(), 2, W, H * W)
    lk.level(0, 0)
    es = yv.Essential(c, 1, 64, 100)
    rng = np.random.default_rng(5)
    p1 = torch.from_numpy(rng.uniform(0, 64, (64, 2)).astype(np.float32)).to("cuda:0")
    p2 = torch.from_numpy(rng.uniform(0, 64, (64, 2)).astype(np.float32)).to("cuda:0")
    cnt = torch.tensor([64], dtype=torch.int32, device="cuda:0")
    d_E = torch.zeros(9, dtype=torch.float64, device="cuda:0")
    d_found = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    es.find(p1.data_ptr(), p2.data_ptr(), cnt.data_ptr(), 1, 64, d_E.data_ptr(), d_found.data_ptr())
    c.sync()
    w = scene.ba_window(n_poses=4, n_landmarks=50, obs=2, noise_px=1.0, seed=1)
    ba = yv.BundleAdjuster(c, 4, 50, len(w["ep"]))
    ba.set_problem(4, 1, 50, w["ep"], w["el"], w["meas"], scene.K_KITTI)
    ba.solve(w["poses0"], w["X0"], 2)
    win = yv.BaWindow(ba, 32, 4)
    win.reserve(8)
    for h in (win, ba, es, lk, b):
        h.close()
    return out


def test_create_destroy_in_sequence():
    """Eight rounds of a batch (filter, gates, selection and steering allocated), an Lk, an Essential, a
    BundleAdjuster and a BaWindow: the last round's batch outputs equal the first round's."""
    import torch
    c = _configured_context()
    d_images = torch.from_numpy(synth_stereo_batch(91, 2, 0, H, W)).to("cuda:0")
    torch.cuda.synchronize()
    first = _round(c, d_images)
    assert first[0].min() > 0
    for _ in range(6):
        _round(c, d_images)
    _assert_same(_round(c, d_images), first)
    c.close()
