"""GPU tests of the sub-pixel stereo refinement: yv_stereo_subpix and the batch's refinement stage equal the numpy
specification of tests/stereo_subpix_reference.py entry for entry, yv_triangulate_subpix and the track builders equal
the oracle's triangulation of the refined points bit for bit, the pose LM on the refined edges equals the oracle's in
the kernel's sum mode, and with the refinement off a batch computes byte for byte what it computed before."""
import ctypes

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import map as ymap
from ya_vo_amd import scene
from ya_vo_amd.synth import synth_frame

import stereo_subpix_reference as ssr

pytestmark = pytest.mark.gpu

T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
PARAMS = [(1, 1), (2, 2), (5, 3), (7, 8)]
THR = 20


# ------------------------------------------------------------------------------------------------
# yv_stereo_subpix
# ------------------------------------------------------------------------------------------------
def _strided(img, stride):
    """A view of img with rows `stride` bytes apart in a buffer that ends with the image's last pixel."""
    H, W = img.shape
    flat = np.full((H - 1) * stride + W, 0xA5, np.uint8)
    v = np.lib.stride_tricks.as_strided(flat, (H, W), (stride, 1))
    v[:] = img
    return v


def _noise_pair(H, W, seed):
    """Left noise, right = the left three columns further plus noise of its own: every status occurs."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = (np.roll(L, -3, axis=1) // 4 * 3 + rng.integers(0, 64, (H, W), dtype=np.uint8)).astype(np.uint8)
    return L, R


def _border_matches(H, W, w, s):
    """Every one of the eight footprint conditions touched exactly and crossed by one, around a centre that is inside
    when the image has one (the conditions of both images, rows and columns)."""
    r0, c0 = H // 2, W // 2
    touch = [(w, c0, r0, c0), (H - 1 - w, c0, r0, c0), (r0, w, r0, c0), (r0, W - 1 - w, r0, c0),
             (r0, c0, w, c0), (r0, c0, H - 1 - w, c0), (r0, c0, r0, s + w), (r0, c0, r0, W - 1 - s - w)]
    step = [(-1, 0, 0, 0), (1, 0, 0, 0), (0, -1, 0, 0), (0, 1, 0, 0), (0, 0, -1, 0), (0, 0, 1, 0), (0, 0, 0, -1),
            (0, 0, 0, 1)]
    out = []
    for t, d in zip(touch, step):
        out += [t, tuple(a + b for a, b in zip(t, d))]
    a = np.array(out, np.int64)
    keep = (a[:, [0, 2]] >= 0).all(1) & (a[:, [0, 2]] < H).all(1) & (a[:, [1, 3]] >= 0).all(1) & (a[:, [1, 3]] < W).all(1)
    return a[keep]


def _random_matches(H, W, n, seed):
    """Positions over the whole image, the right keypoint up to 2 rows and 6 columns away."""
    rng = np.random.default_rng(seed)
    rc1 = np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1)
    rc2 = np.clip(rc1 + np.stack([rng.integers(-2, 3, n), rng.integers(-6, 2, n)], 1), 0, [H - 1, W - 1])
    return rc1, rc2


def _check_list(ctx, L, R, rc1, rc2, w, s, stride=None):
    Lg, Rg = (L, R) if stride is None else (_strided(L, stride), _strided(R, stride))
    got = ctx.stereo_subpix(Lg, Rg, ssr.make_matches(rc1, rc2), w, s)
    want = ssr.subpix(L, R, rc1, rc2, w, s)
    for name, g, x in zip(("dcol_q8", "sad", "status"), got, want):
        np.testing.assert_array_equal(g, x, err_msg=name)
    return want


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("shape", [(9, 9), (17, 40), (120, 127), (120, 128), (200, 320)])
@pytest.mark.parametrize("w,s", PARAMS)
def test_list_equals_the_specification(ctx, w, s, shape, pad):
    H, W = shape
    L, R = _noise_pair(H, W, 1000 * H + W)
    rc1, rc2 = _random_matches(H, W, 500, 7 * H + W + w)
    bm = _border_matches(H, W, w, s)
    # the image's corners and last row: the reads next to the end of the buffer
    corners = np.array([(H - 1 - w, W - 1 - w, H - 1 - w, W - 1 - s - w), (w, w, w, s + w),
                        (H - 1 - w, w, H - 1 - w, W - 1 - s - w), (H - 1, W - 1, H - 1, W - 1), (0, 0, 0, 0)], np.int64)
    corners = corners[(corners >= 0).all(1) & (corners[:, [0, 2]] < H).all(1) & (corners[:, [1, 3]] < W).all(1)]
    rc1 = np.concatenate([rc1, bm[:, :2], corners[:, :2]])
    rc2 = np.concatenate([rc2, bm[:, 2:], corners[:, 2:]])
    _, _, st = _check_list(ctx, L, R, rc1, rc2, w, s, stride=W + pad)
    fits = 2 * w + 1 <= H and 2 * (w + s) + 1 <= W
    if fits:
        assert (st != ssr.OUTSIDE).sum() >= len(bm) // 2 and (st == ssr.OUTSIDE).sum() >= len(bm) // 2
        assert (st[500:500 + len(bm)][0::2] != ssr.OUTSIDE).all() and (st[500:500 + len(bm)][1::2] == ssr.OUTSIDE).all()
    else:
        assert (st == ssr.OUTSIDE).all()
    if H >= 100:
        assert {ssr.OK, ssr.EDGE, ssr.OUTSIDE} <= set(np.unique(st).tolist()) or s == 1


@pytest.mark.parametrize("w,s", PARAMS)
def test_rows_that_differ_by_two(ctx, w, s):
    H, W = 60, 97
    L, R = _noise_pair(H, W, 5)
    rng = np.random.default_rng(6)
    rc1 = np.stack([rng.integers(10, H - 10, 300), rng.integers(20, W - 20, 300)], 1)
    for dr in (-2, 2):
        Rs = np.roll(R, dr, axis=0)  # the matching rows are dr further down
        rc2 = rc1 + [dr, -3]
        _, _, st = _check_list(ctx, L, Rs, rc1, rc2, w, s)
        assert (st == ssr.OK).sum() >= 150 or s == 1


@pytest.mark.parametrize("w,s", [(5, 3), (7, 8)])
def test_constant_ramp_and_period_two_images(ctx, w, s):
    H, W = 40, 64
    c = np.arange(W, dtype=np.int64)
    const = np.full((H, W), 77, np.uint8)
    ramp_l = np.broadcast_to((3 * c + 60).astype(np.uint8), (H, W)).copy()
    ramp_r = np.broadcast_to((3 * c).astype(np.uint8), (H, W)).copy()
    per = np.broadcast_to((100 + 50 * (c % 2)).astype(np.uint8), (H, W)).copy()
    rc1, rc2 = _random_matches(H, W, 300, 9)
    dq, sad, st = _check_list(ctx, const, const, rc1, rc2, w, s)
    ins = st != ssr.OUTSIDE
    assert ins.sum() >= 20 and (st[ins] == ssr.OK).all() and (dq == 0).all() and (sad[ins] == 0).all()
    dq, sad, st = _check_list(ctx, const, (const + 10).astype(np.uint8), rc1, rc2, w, s)  # den = 0
    assert (st[ins] == ssr.OK).all() and (dq == 0).all() and (sad[ins] == 10 * (2 * w + 1) ** 2).all()
    for a, b in ((ramp_l, ramp_r), (ramp_r, ramp_l)):
        dq, sad, st = _check_list(ctx, a, b, rc1, rc2, w, s)
        assert (st[ins] == ssr.EDGE).all() and (dq == 0).all()
    dq, sad, st = _check_list(ctx, per, per, rc1, rc2, w, s)
    odd = ((rc1[:, 1] - rc2[:, 1]) % 2 == 1) & ins
    assert odd.sum() >= 5 and (dq[odd] == -256).all() and (dq[ins & ~odd] == 0).all() and (sad[ins] == 0).all()


def test_empty_single_and_full_lists(ctx):
    H, W = 200, 320
    L, R = _noise_pair(H, W, 21)
    e = np.zeros((0, 2), np.int64)
    for got in ctx.stereo_subpix(L, R, ssr.make_matches(e, e), 5, 3):
        assert len(got) == 0
    _check_list(ctx, L, R, [(100, 150)], [(100, 147)], 5, 3)
    rc1, rc2 = _random_matches(H, W, 1500, 22)
    pick = np.random.default_rng(23).integers(0, 1500, 4096)  # 4096 records, most of them more than once
    _, _, st = _check_list(ctx, L, R, rc1[pick], rc2[pick], 5, 3)
    assert (st == ssr.OK).sum() > 500
    with pytest.raises(yv.YavoError) as err:
        ctx.stereo_subpix(L, R, ssr.make_matches(rc1[np.r_[pick, 0]], rc2[np.r_[pick, 0]]), 5, 3)
    assert err.value.status == yv.YV_ERR_CAPACITY


def test_fixture_accuracy_on_the_gpu(ctx):
    """The known-disparity fixture through the kernel: equal to the specification, hence inside its bounds."""
    (left, right), (rc1, rc2, true_c2) = ssr.disparity_pair(33), ssr.disparity_points(33)
    dq, _, st = _check_list(ctx, left, right, rc1, rc2, 5, 3)
    err = np.abs(ssr.refined_column(rc2[:, 1], dq) - true_c2)
    assert (st == ssr.OK).all() and err.max() < 0.25 and err.mean() < 0.12


# ------------------------------------------------------------------------------------------------
# yv_triangulate_subpix
# ------------------------------------------------------------------------------------------------
def test_triangulate_subpix_equals_the_oracle_on_refined_points(ctx, oracle):
    rng = np.random.default_rng(31)
    n = 700
    rc1 = np.stack([rng.integers(0, 376, n), rng.integers(100, 1241, n)], 1)
    rc2 = rc1 - np.stack([np.zeros(n, np.int64), rng.integers(1, 90, n)], 1)
    m = ssr.make_matches(rc1, rc2)
    dq = rng.integers(-8 * 256 - 128, 8 * 256 + 129, n).astype(np.int32)
    dq[:20] = 0
    dq[20:30] = [-2176, 2176, -1, 1, 128, -128, 255, 256, 257, -257]
    # the rectified pose and one a little off it (a larger rotation leaves no pair of rays close enough to accept)
    for Tb in (T_RIGHT, np.array([0.0004, -0.0002, 0.0003, 1, 0.001, -0.54, 0.01])):
        Tb = Tb.copy()
        Tb[:4] /= np.linalg.norm(Tb[:4])
        n_ok, X, ok = ctx.triangulate(IDENTITY, Tb, scene.K_KITTI, m, dcol_q8=dq)
        Xr, okr = ssr.triangulate_refined(oracle, IDENTITY, Tb, scene.K_KITTI, m, dq)
        np.testing.assert_array_equal(ok, okr)
        assert X.tobytes() == Xr.tobytes()
        assert n_ok == okr.sum() and 0 < n_ok < n
        # without refined columns: yv_triangulate, byte for byte (also through a NULL dcol_q8)
        n0, X0, ok0 = ctx.triangulate(IDENTITY, Tb, scene.K_KITTI, m)
        Xn = np.zeros((n, 3))
        okn = np.zeros(n, np.uint8)
        cnt = ctypes.c_int()
        pa, pb, k = np.ascontiguousarray(IDENTITY), np.ascontiguousarray(Tb), np.ascontiguousarray(scene.K_KITTI, np.float64)
        assert ctx.lib.yv_triangulate_subpix(ctx.handle, pa.ctypes.data, pb.ctypes.data, k.ctypes.data, m.ctypes.data,
                                             None, n, Xn.ctypes.data, okn.ctypes.data, ctypes.byref(cnt)) == yv.YV_OK
        assert Xn.tobytes() == X0.tobytes() and np.array_equal(okn.astype(bool), ok0) and cnt.value == n0
        nz, Xz, okz = ctx.triangulate(IDENTITY, Tb, scene.K_KITTI, m, dcol_q8=np.zeros(n, np.int32))
        assert Xz.tobytes() == X0.tobytes() and np.array_equal(okz, ok0)
        assert X.tobytes() != X0.tobytes()


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
H, W, K = 120, 160, 512


def _frames(h, w, seed=77):
    """L0, R0, L1, R1: frame k is the crop at (k, 3 k) of a field with a block of its texture pasted a second time
    (wrong matches with small distances), its right image the mean of the crops 8 and 9 columns further (a disparity
    of 8.5 pixels: the right keypoints sit on either side of it) with noise of its own."""
    world = synth_frame(seed, 0, 0, h + 2, w + 13).copy()
    world[h // 2:h // 2 + h // 3, w // 2:w // 2 + w // 3] = world[5:5 + h // 3, 10:10 + w // 3]
    rng = np.random.default_rng(seed)
    out = []
    for k in (0, 1):
        for c in (3 * k, 3 * k + 8):
            img = world[k:k + h, c:c + w].astype(np.int64)
            if c != 3 * k:
                img = (img + world[k:k + h, c + 1:c + 1 + w] + 1) // 2 + rng.integers(-6, 7, img.shape)
            out.append(np.clip(img, 0, 255).astype(np.uint8))
    return np.stack(out)


@pytest.fixture(scope="module")
def frames():
    f = _frames(H, W)
    f.setflags(write=False)
    return f


def _to_device(a):
    import torch
    d = torch.from_numpy(np.array(a)).to("cuda:0")
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def d_frames(frames):
    return _to_device(frames)


def _pose_buffers(n):
    import torch
    d_prior = torch.from_numpy(np.tile(IDENTITY, (n, 1))).to("cuda:0")
    d_pose = torch.zeros((n, 7), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    return d_prior, d_pose


def _snapshot(ctx, b, n_images, n_pairs, n_tracks, h=H, w=W, k=K):
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
    for i in range(ns):
        nd, nk = int(s["det_count"][i]), int(s["kp_count"][i])
        s[f"det_rc{i}"] = ctx.download(v.det_rc + i * k * 8, np.int32, 2 * nd)
        s[f"keypoints{i}"] = ctx.download(v.keypoints + i * k * 48, yv.KEYPOINT_DTYPE, nk)
    for p in range(n_pairs):
        nm, nf = int(s["match_count"][p]), int(s["filt_count"][p])
        s[f"matches{p}"] = ctx.download(v.matches + p * k * 100, yv.MATCH_DTYPE, nm)
        s[f"filtered{p}"] = ctx.download(v.filtered + p * k * 100, yv.MATCH_DTYPE, nf)
        s[f"match_dj{p}"] = ctx.download(v.match_dj + p * k * 8, np.int32, 2 * nm).reshape(-1, 2)
    if n_tracks:
        s["edge_count"] = ctx.download(v.edge_count, np.int32, n_tracks)
        s["track_inliers"] = ctx.download(v.track_inliers, np.int32, n_tracks)
        for t in range(n_tracks):
            ne = int(s["edge_count"][t])
            s[f"edge_X{t}"] = ctx.download(v.edge_X + t * k * 24, np.float64, 3 * ne).reshape(-1, 3)
            s[f"edge_uv{t}"] = ctx.download(v.edge_uv + t * k * 16, np.float64, 2 * ne).reshape(-1, 2)
            s[f"edge_query{t}"] = ctx.download(v.edge_query + t * k * 4, np.int32, ne)
            s[f"edge_outlier{t}"] = ctx.download(v.edge_outlier + t * k, np.uint8, ne)
    return s


def _assert_same(a, b, keys=None):
    assert a.keys() == b.keys()
    for key in (keys or a.keys()):
        assert a[key].tobytes() == b[key].tobytes(), key


def _subpix_arrays(ctx, b, n_pairs, k=K):
    """The whole view: dcol_q8, sad, status as [n_pairs][max_kp]."""
    v = b.subpix_view()
    return (ctx.download(v.dcol_q8, np.int32, n_pairs * k).reshape(n_pairs, k),
            ctx.download(v.sad, np.int32, n_pairs * k).reshape(n_pairs, k),
            ctx.download(v.status, np.uint8, n_pairs * k).reshape(n_pairs, k))


def _expected_pair(snap, imgs, p, qi, ti, w, s, keep=None, k=K):
    """What the view holds for a marked pair p = (query image qi, train image ti): the specification on the kept
    matches of the view's own match_dj / match_lim (and keep), NONE elsewhere."""
    kq, kt = snap[f"keypoints{qi}"], snap[f"keypoints{ti}"]
    dj = snap[f"match_dj{p}"]
    kept = (dj[:, 0] < snap["match_lim"][p]) & (dj[:, 1] >= 0)
    if keep is not None:
        kept &= keep[:len(kq)]
    dq, sad, st = np.zeros(k, np.int32), np.full(k, -1, np.int32), np.zeros(k, np.uint8)
    i = np.nonzero(kept)[0]
    j = dj[i, 1]
    rc1 = np.stack([kq["x"][i], kq["y"][i]], 1)
    rc2 = np.stack([kt["x"][j], kt["y"][j]], 1)
    dq[i], sad[i], st[i] = ssr.subpix(imgs[qi], imgs[ti], rc1, rc2, w, s)
    return dq, sad, st, kept


def _assert_none(arr, p):
    dq, sad, st = arr
    assert (dq[p] == 0).all() and (sad[p] == -1).all() and (st[p] == ssr.NONE).all(), f"pair {p}"


def _assert_pair(arr, p, want):
    for name, g, x in zip(("dcol_q8", "sad", "status"), arr, want[:3]):
        np.testing.assert_array_equal(g[p], x, err_msg=f"pair {p} {name}")


def _stereo_records(snap, sp, qs, ts, j):
    """MATCH_DTYPE records of the stereo pair sp = (qs, ts) for its query keypoints j."""
    kl, kr = snap[f"keypoints{qs}"], snap[f"keypoints{ts}"]
    jr = snap[f"match_dj{sp}"][j, 1]
    return ssr.make_matches(np.stack([kl["x"][j], kl["y"][j]], 1), np.stack([kr["x"][jr], kr["y"][jr]], 1))


def _match_batch(ctx, n_images=4):
    """Images L0 R0 L1 R1; pairs (L1, R1) stereo, (L0, L1) temporal, (L0, R0) stereo; one track of the first two."""
    b = yv.Batch(ctx, n_images, H, W, K, 4)
    b.set_pairs([(2, 3), (0, 2), (0, 1)])
    b.set_tracks([(0, 1)], scene.K_KITTI, T_RIGHT)
    return b


def test_setting_is_validated_and_the_view_needs_it_switched_on(ctx):
    b = _match_batch(ctx, 6)
    b.set_pairs([(2, 3), (0, 2), (6, 1), (4, 5)])  # pair 2 names the carry slot
    with pytest.raises(yv.YavoError) as e:
        b.subpix_view()
    assert e.value.status == yv.YV_ERR_INVALID
    b.set_stereo_subpix(None)  # off: still nothing allocated
    b.set_stereo_subpix([], half_win=99, search=99)
    with pytest.raises(yv.YavoError):
        b.subpix_view()
    bad = [dict(pairs=[4]), dict(pairs=[-1]), dict(pairs=[0, 0]), dict(pairs=[0, 1, 0]), dict(pairs=[2]),
           dict(pairs=[0], half_win=0), dict(pairs=[0], half_win=8), dict(pairs=[0], search=0),
           dict(pairs=[0], search=9)]
    for kw in bad:
        with pytest.raises(yv.YavoError) as e:
            b.set_stereo_subpix(**kw)
        assert e.value.status == yv.YV_ERR_INVALID, kw
    idx = np.zeros(1, np.int32)
    for flags in (-1, 2, 3):
        assert ctx.lib.yv_batch_set_stereo_subpix(b.handle, idx.ctypes.data, 1, 5, 3, flags) == yv.YV_ERR_INVALID
    assert ctx.lib.yv_batch_set_stereo_subpix(b.handle, idx.ctypes.data, -1, 5, 3, 0) == yv.YV_ERR_INVALID
    with pytest.raises(yv.YavoError):
        b.subpix_view()  # a refused call allocates nothing
    b.set_stereo_subpix([0, 3, 1], half_win=7, search=8, drop_edge=True)
    v = b.subpix_view()
    assert v.dcol_q8 and v.sad and v.status
    _assert_none(_subpix_arrays(ctx, b, 4), slice(None))  # filled with "not attempted"
    b.close()


@pytest.fixture(scope="module")
def off_on(ctx, frames, d_frames):
    """One batch of 6 image slots run on 4 images: a run + track with the refinement off, then with pairs 0 (the
    track's stereo pair) and 3 (images 4, 5: beyond the run) marked at (5, 3)."""
    d_prior, d_pose = _pose_buffers(1)
    b = yv.Batch(ctx, 6, H, W, K, 4)
    b.set_pairs([(2, 3), (0, 2), (0, 1), (4, 5)])
    b.set_tracks([(0, 1)], scene.K_KITTI, T_RIGHT)
    out = []
    for on in (False, True):
        if on:
            b.set_stereo_subpix([0, 3], 5, 3)
        b.run(d_frames.data_ptr(), 4, W, H * W, THR)
        b.track(d_prior.data_ptr(), d_pose.data_ptr())
        out.append(_snapshot(ctx, b, 6, 4, 1))
        out[-1]["pose"] = d_pose.cpu().numpy()
    yield b, out[0], out[1], _subpix_arrays(ctx, b, 4)
    b.close()


def test_view_equals_the_specification(ctx, frames, off_on):
    b, off, on, arr = off_on
    want = _expected_pair(on, frames, 0, 2, 3, 5, 3)
    _assert_pair(arr, 0, want)
    st, kept = want[2], want[3]
    nq = len(on["keypoints2"])
    assert nq >= 100 and kept.sum() >= 50 and (~kept).sum() >= 1       # dropped matches: NONE
    assert (st[:nq][~kept] == ssr.NONE).all() and (st[nq:] == ssr.NONE).all()
    assert (st == ssr.OK).sum() >= 30 and (arr[0][0] != 0).sum() >= 30
    for p in (1, 2, 3):  # unmarked pairs, and the marked pair whose images lie beyond n_images
        _assert_none(arr, p)
    # the run itself does not change
    keys = [key for key in off if key.startswith(("matches", "match_", "filt", "keypoints", "kp_count", "det_"))]
    _assert_same(off, on, keys)


def _check_track(oracle, snap_off, snap_on, arr, drop_edge=False):
    """Match mode, track 0 = (stereo pair 0 = (2, 3), temporal pair 1 = (0, 2)): the edges are the unrefined run's
    (minus the EDGE matches under drop_edge), edge_X the oracle's triangulation of the refined points."""
    q = snap_off["edge_query0"]
    j = snap_off["match_dj1"][q, 1]
    dq, _, st = arr
    sel = st[0][j] != ssr.EDGE if drop_edge else np.ones(len(q), bool)
    m = _stereo_records(snap_off, 0, 2, 3, j[sel])
    X, ok = ssr.triangulate_refined(oracle, IDENTITY, T_RIGHT, scene.K_KITTI, m, dq[0][j[sel]])
    # every refined point still triangulates in front of the camera (the disparities are far from zero): the edge
    # set is the unrefined one
    assert ok.all()
    assert snap_on["edge_count"][0] == sel.sum()
    np.testing.assert_array_equal(snap_on["edge_query0"], q[sel])
    assert snap_on["edge_uv0"].tobytes() == snap_off["edge_uv0"][sel].tobytes()
    assert snap_on["edge_X0"].tobytes() == X.tobytes()
    return sel, st[0][j]


def test_edges_keep_their_set_and_move_to_the_refined_points(ctx, oracle, off_on):
    b, off, on, arr = off_on
    sel, st = _check_track(oracle, off, on, arr)
    assert len(sel) >= 20 and (st == ssr.OK).sum() >= 10
    moved = (on["edge_X0"] != off["edge_X0"]).any(1)
    assert moved.sum() >= 5 and not moved[arr[0][0][off["match_dj1"][off["edge_query0"], 1]] == 0].any()
    # the pose LM on the refined edges, in the kernel's sum mode
    T, out, inl = oracle.pose_lm(on["edge_X0"], on["edge_uv0"], scene.K_KITTI, IDENTITY, yv.track_lm_sum_mode(1))
    assert on["pose"][0].tobytes() == T.tobytes()
    np.testing.assert_array_equal(on["edge_outlier0"].astype(bool), out)
    assert on["track_inliers"][0] == inl


def test_drop_edge_drops_exactly_the_edge_matches(ctx, oracle, frames, d_frames, off_on):
    _, off, _, _ = off_on
    d_prior, d_pose = _pose_buffers(1)
    b = _match_batch(ctx)
    b.set_stereo_subpix([0], 3, 1, drop_edge=True)
    b.run(d_frames.data_ptr(), 4, W, H * W, THR)
    b.track(d_prior.data_ptr(), d_pose.data_ptr())
    on = _snapshot(ctx, b, 4, 3, 1)
    arr = _subpix_arrays(ctx, b, 3)
    _assert_pair(arr, 0, _expected_pair(on, frames, 0, 2, 3, 3, 1))
    off4 = {key: v for key, v in off.items()}  # the same images and pairs 0..2: the unrefined edges
    sel, st = _check_track(oracle, off4, on, arr, drop_edge=True)
    assert (~sel).sum() >= 1 and sel.sum() >= 10 and (st[~sel] == ssr.EDGE).all()
    # a parameter change between two runs, the flag off again: the full edge set at (7, 8), where the footprints of
    # the keypoints next to the left and right border (8 columns off it at the least) are outside
    b.set_stereo_subpix([0], 7, 8)
    b.run(d_frames.data_ptr(), 4, W, H * W, THR)
    b.track(d_prior.data_ptr(), d_pose.data_ptr())
    on2 = _snapshot(ctx, b, 4, 3, 1)
    arr2 = _subpix_arrays(ctx, b, 3)
    _assert_pair(arr2, 0, _expected_pair(on2, frames, 0, 2, 3, 7, 8))
    sel2, _ = _check_track(oracle, off4, on2, arr2)
    assert sel2.all()
    assert (arr2[2][0] == ssr.OUTSIDE).sum() >= 1 and (arr2[2][0] == ssr.EDGE).sum() == 0
    b.close()


def test_set_pairs_clears_it_and_off_is_byte_identical(ctx, d_frames, off_on):
    """After yv_batch_set_pairs, and after switching it off, a batch computes byte for byte what one that never had it
    on computes: every view array and the pose."""
    _, off, _, _ = off_on
    d_prior, d_pose = _pose_buffers(1)
    snaps = []
    for how in ("never", "set_pairs", "off"):
        b = yv.Batch(ctx, 6, H, W, K, 4)
        b.set_pairs([(2, 3), (0, 2), (0, 1), (4, 5)])
        if how != "never":
            b.set_stereo_subpix([0, 2], 5, 3, drop_edge=True)
            b.run(d_frames.data_ptr(), 4, W, H * W, THR)
        if how == "set_pairs":
            b.set_pairs([(2, 3), (0, 2), (0, 1), (4, 5)])
            assert b.subpix_view().status  # the arrays stay
        if how == "off":
            b.set_stereo_subpix(None)
        b.set_tracks([(0, 1)], scene.K_KITTI, T_RIGHT)
        b.run(d_frames.data_ptr(), 4, W, H * W, THR)
        b.track(d_prior.data_ptr(), d_pose.data_ptr())
        snaps.append(_snapshot(ctx, b, 6, 4, 1))
        snaps[-1]["pose"] = d_pose.cpu().numpy()
        b.close()
    assert snaps[0]["edge_count"][0] > 0
    _assert_same(snaps[0], snaps[1])
    _assert_same(snaps[0], snaps[2])
    _assert_same(snaps[0], off)


def test_under_the_match_filter_and_gates(ctx, oracle):
    """200 x 320 images, the 2-NN filter and the stereo gate {-2, 2, -64, 0}: the refinement follows keep."""
    h, w = 200, 320
    fr = _frames(h, w, seed=78)
    d = _to_device(fr)
    d_prior, d_pose = _pose_buffers(1)
    b = yv.Batch(ctx, 4, h, w, K, 2)
    b.set_pairs([(2, 3), (0, 2)])
    b.set_tracks([(0, 1)], scene.K_KITTI, T_RIGHT)
    b.set_match_filter(ratio=(4, 5), mutual=True)
    b.set_match_gates([(-2, 2, -64, 0), (-h, h, -w, w)])
    snaps = []
    for on in (False, True):
        if on:
            b.set_stereo_subpix([0], 5, 3)
        b.run(d.data_ptr(), 4, w, h * w, THR)
        b.track(d_prior.data_ptr(), d_pose.data_ptr())
        snaps.append(_snapshot(ctx, b, 4, 2, 1, h, w))
    off, on = snaps
    arr = _subpix_arrays(ctx, b, 2)
    keep = ctx.download(b.match2_view().keep, np.uint8, K).astype(bool)
    want = _expected_pair(on, fr, 0, 2, 3, 5, 3, keep=keep)
    _assert_pair(arr, 0, want)
    nq = len(on["keypoints2"])
    dj = on["match_dj0"]
    passed = (dj[:, 0] < on["match_lim"][0]) & (dj[:, 1] >= 0)
    assert (passed & ~keep[:nq]).sum() >= 1 and want[3].sum() >= 30  # kept by removeOutliers, dropped by the filter
    assert (arr[2][0][:nq][~keep[:nq]] == ssr.NONE).all()
    _assert_none(arr, 1)
    sel, _ = _check_track(oracle, off, on, arr)
    assert len(sel) >= 10
    b.close()


def test_lk_mode_uses_the_refined_stereo_points(ctx, oracle, frames, d_frames):
    """LK mode: frame k-1's map points triangulate from the refined columns; the flow, and so the edge set, is the
    unrefined run's."""
    d_prior, d_pose = _pose_buffers(1)
    b = yv.Batch(ctx, 4, H, W, K, 2)
    b.set_pairs([(0, 1), (2, 3)])
    b.set_track_lk(2)
    b.set_tracks([(0, 2)], scene.K_KITTI, T_RIGHT)  # {stereo pair of frame 0, image L1}
    snaps = []
    for on in (False, True):
        if on:
            b.set_stereo_subpix([0], 5, 3)
        b.run(d_frames.data_ptr(), 4, W, H * W, THR)
        b.track(d_prior.data_ptr(), d_pose.data_ptr())
        snaps.append(_snapshot(ctx, b, 4, 2, 1))
        snaps[-1]["pose"] = d_pose.cpu().numpy()
    off, on = snaps
    arr = _subpix_arrays(ctx, b, 2)
    _assert_pair(arr, 0, _expected_pair(on, frames, 0, 0, 1, 5, 3))
    _assert_none(arr, 1)
    j = off["edge_query0"]
    assert len(j) >= 10 and on["edge_count"][0] == len(j)
    np.testing.assert_array_equal(on["edge_query0"], j)
    assert on["edge_uv0"].tobytes() == off["edge_uv0"].tobytes()
    X, ok = ssr.triangulate_refined(oracle, IDENTITY, T_RIGHT, scene.K_KITTI, _stereo_records(off, 0, 0, 1, j),
                                    arr[0][0][j])
    assert ok.all() and on["edge_X0"].tobytes() == X.tobytes()
    assert on["edge_X0"].tobytes() != off["edge_X0"].tobytes()
    T, out, inl = oracle.pose_lm(on["edge_X0"], on["edge_uv0"], scene.K_KITTI, IDENTITY, yv.track_lm_sum_mode(1))
    assert on["pose"][0].tobytes() == T.tobytes() and on["track_inliers"][0] == inl
    # DROP_EDGE: the stereo points whose match is EDGE are gone before the flow
    b.set_stereo_subpix([0], 3, 1, drop_edge=True)
    b.run(d_frames.data_ptr(), 4, W, H * W, THR)
    b.track(d_prior.data_ptr(), d_pose.data_ptr())
    dr = _snapshot(ctx, b, 4, 2, 1)
    st = _subpix_arrays(ctx, b, 2)[2][0]
    sel = st[j] != ssr.EDGE
    assert (~sel).sum() >= 1
    np.testing.assert_array_equal(dr["edge_query0"], j[sel])
    b.close()


def test_lk_mode_under_the_match_filter_and_the_refinement(ctx, oracle):
    """LK mode with the 2-NN filter and the refinement both on (the 200 x 320, seed 78 frames of
    test_under_the_match_filter_and_gates): frame k-1's map points are the stereo matches that removeOutliers and the
    filter keep, triangulated from the refined columns."""
    h, w = 200, 320
    fr = _frames(h, w, seed=78)
    d = _to_device(fr)
    d_prior, d_pose = _pose_buffers(1)
    b = yv.Batch(ctx, 4, h, w, K, 2)
    b.set_pairs([(0, 1), (2, 3)])
    b.set_track_lk(2)
    b.set_tracks([(0, 2)], scene.K_KITTI, T_RIGHT)  # {stereo pair of frame 0, image L1}
    b.set_match_filter(ratio=(4, 5), mutual=True)
    b.set_stereo_subpix([0], 5, 3)
    b.run(d.data_ptr(), 4, w, h * w, THR)
    b.track(d_prior.data_ptr(), d_pose.data_ptr())
    snap = _snapshot(ctx, b, 4, 2, 1, h, w)
    pose = d_pose.cpu().numpy()
    arr = _subpix_arrays(ctx, b, 2)
    keep = ctx.download(b.match2_view().keep, np.uint8, K).astype(bool)
    nq = len(snap["keypoints0"])
    dj = snap["match_dj0"]
    passed = (dj[:, 0] < snap["match_lim"][0]) & (dj[:, 1] >= 0)
    j = snap["edge_query0"]
    assert len(j) >= 10 and (passed & ~keep[:nq]).sum() >= 1  # kept by removeOutliers, dropped by the filter
    assert (passed[j] & keep[j]).all()
    X, ok = ssr.triangulate_refined(oracle, IDENTITY, T_RIGHT, scene.K_KITTI, _stereo_records(snap, 0, 0, 1, j),
                                    arr[0][0][j])
    assert ok.all() and snap["edge_X0"].tobytes() == X.tobytes()
    T, out, inl = oracle.pose_lm(snap["edge_X0"], snap["edge_uv0"], scene.K_KITTI, IDENTITY, yv.track_lm_sum_mode(1))
    assert pose[0].tobytes() == T.tobytes() and snap["track_inliers"][0] == inl
    b.close()


@pytest.mark.parametrize("overlap", [0, 1])
def test_through_track_map(ctx, oracle, frames, d_frames, off_on, overlap):
    """yv_batch_track_map (with the asynchronous edge build under overlap): the refined edges, and the map block the
    oracle writes from them."""
    import torch
    _, off, on_ref, arr_ref = off_on
    max_kf = 1
    bb = ymap.block_bytes(max_kf, K)
    d_block = torch.zeros(bb, dtype=torch.uint8, device="cuda:0")
    d_prior, d_pose = _pose_buffers(1)
    b = yv.Batch(ctx, 6, H, W, K, 4)
    b.set_pairs([(2, 3), (0, 2), (0, 1), (4, 5)])
    b.set_tracks([(0, 1)], scene.K_KITTI, T_RIGHT)
    b.set_track_overlap(overlap)
    b.set_stereo_subpix([0, 3], 5, 3)
    for _ in range(2):  # the second run's refinement is ordered after the first track's build
        b.run(d_frames.data_ptr(), 4, W, H * W, THR)
        b.track_map(d_prior.data_ptr(), d_pose.data_ptr(), 1, 1, d_block.data_ptr(), max_kf)
    ctx.sync()
    b.track_sync()
    torch.cuda.synchronize()
    on = _snapshot(ctx, b, 6, 4, 1)
    on["pose"] = d_pose.cpu().numpy()
    _assert_same(on_ref, on)
    for g, x in zip(_subpix_arrays(ctx, b, 4), arr_ref):
        np.testing.assert_array_equal(g, x)
    v = b.view()
    ec = ctx.download(v.edge_count, np.int32, 1)
    eX = ctx.download(v.edge_X, np.float64, K * 3).reshape(1, K, 3)
    eo = ctx.download(v.edge_outlier, np.uint8, K).reshape(1, K)
    ref = oracle.map_chunk(on["pose"], 1, 1, ec, eX, eo, K, max_kf)
    assert d_block.cpu().numpy().tobytes() == np.asarray(ref).tobytes()
    b.close()
