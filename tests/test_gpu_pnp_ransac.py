"""GPU parity of the P3P-RANSAC absolute pose (yv_pnp_ransac, yv_pnp_ransac_batch, the batch's track RANSAC) against the
specification tests/pnp_ransac_reference.py: pose bytes, mask, count and found, bit for bit."""
import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import scene
from ya_vo_amd.synth import synth_frame

import pnp_ransac_reference as ref
from pnp_scenes import IDENTITY, K9, pnp_scene

pytestmark = pytest.mark.gpu

PRIOR = np.array([0.1, -0.2, 0.3, 0.9, 1.0, -2.0, 3.0])  # what a call that finds nothing must hand back


def _same(ctx, X, uv, draws, thr=2.0, min_inliers=12, pose=PRIOR):
    """One host-pointer call against the specification -> the specification's (pose, mask, inliers, found, counts)."""
    want = ref.pnp_ransac(X, uv, K9, draws, thr, min_inliers, pose)
    T, mask, inl, found = ctx.pnp_ransac(X, uv, K9, draws=draws, thr=thr, min_inliers=min_inliers, pose=pose)
    assert (found, inl) == (want[3], want[2])
    np.testing.assert_array_equal(mask, want[1])
    assert T.tobytes() == want[0].tobytes(), (T, want[0])
    return want


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65, 200, 257])
def test_edge_counts(ctx, n):
    # (the small ones exact, so that the fourth edge fits the pose of the other three)
    X, uv, _, clean = pnp_scene(n, seed=n, outlier_frac=0.3 if n >= 63 else 0.0, noise_px=0.3 if n >= 63 else 0.0)
    want = _same(ctx, X, uv, ref.make_draws(64, 1), min_inliers=4)
    assert want[3] == (n >= 4)  # three edges fit every candidate; from four on the clean ones are found
    if n >= 63:
        assert want[2] >= 0.6 * n and not np.any(want[1] & ~clean)


def test_capacity_edge_count(ctx):
    X, uv, _, clean = pnp_scene(4096, seed=7, outlier_frac=0.5)
    want = _same(ctx, X, uv, ref.make_draws(4, 12), min_inliers=4)
    assert want[4].sum() > 0


@pytest.mark.parametrize("iters", [1, 63, 64, 65, 256])
def test_hypothesis_counts(ctx, iters):
    X, uv, _, _ = pnp_scene(200, seed=2, outlier_frac=0.5)
    want = _same(ctx, X, uv, ref.make_draws(iters, 5))
    assert want[3] == (iters > 1)


@pytest.mark.parametrize("frac,iters", [(0.0, 64), (0.5, 64), (0.7, 256)])
@pytest.mark.parametrize("large", [False, True])
def test_outlier_fractions(ctx, frac, iters, large):
    X, uv, _, clean = pnp_scene(200, seed=1, outlier_frac=frac, large=large)
    want = _same(ctx, X, uv, ref.make_draws(iters, 0))
    assert want[3] and not np.any(want[1] & ~clean) and want[2] >= 0.9 * clean.sum()


def _degenerate_scene():
    """40 clean noise-free edges with every degenerate sample planted by hand -> (X, uv, draws, behind)"""
    X, uv, T, _ = pnp_scene(40, seed=3, outlier_frac=0.0, large=True, noise_px=0.0)
    n = len(X)
    X[12] = 2.0 * X[11] - X[10]                      # 10, 11, 12 collinear
    uv[12] = scene.project(T, X[12:13], scene.K_KITTI)[0]
    X[14] = X[13]                                    # 13, 14, 15 coincident
    X[15] = X[13]
    X[18] = X[16]                                    # 16, 17, 18: P1 == P3, b^2 = 0
    behind = np.arange(19, 25)                       # behind the camera, on the same pixels: e = 0 but z < 0
    pc = scene.transform(T, X[behind])
    X[behind] = (scene.quat_to_R(T[:4]).T @ (-pc - T[4:]).T).T
    X[26, 0] = np.nan
    X[27, 2] = np.inf
    uv[28, 1] = np.nan
    uv[29, 0] = -np.inf
    X[30] = [np.inf, np.nan, -np.inf]                # never sampled below, scored by every candidate
    uv[31] = [np.nan, np.inf]
    hand = [(3, 3, 7), (1, 2, 1 + n), (5, 6, 5 + 3 * n),  # a repeated index, also through the modulo
            (10, 11, 12), (12, 10, 11), (13, 14, 15), (16, 17, 18), (16, 18, 17),
            (19, 20, 21), (22, 0, 23), (0, 1, 24),         # behind the camera
            (26, 1, 2), (1, 27, 2), (28, 3, 4), (3, 4, 29), (26, 27, 28)]
    good = [(0, 1, 2), (4, 8, 33), (35, 5, 9), (2 ** 32 - 1, 7, 38)]
    draws = np.array(hand + good, np.uint64).astype(np.uint32)
    return X, uv, draws, behind


def test_degenerate_hypotheses(ctx):
    X, uv, draws, behind = _degenerate_scene()
    want = _same(ctx, X, uv, draws, min_inliers=4)
    nc = want[4]
    assert want[3] and not nc[:3].any() and not nc[5:8].any()  # repeats, coincident and b^2 = 0: no candidate
    assert not want[1][behind].any() and not want[1][26:32].any()
    assert want[2] == 40 - 6 - 6 - 3  # all but the planted edges (behind, non-finite, 14 / 15 / 18 moved off their pixels)
    # each degenerate hypothesis alone: nothing found, the pose handed back
    for h in range(16):
        _same(ctx, X, uv, draws[h:h + 1], min_inliers=4)
    # every edge non-finite
    _same(ctx, np.full((8, 3), np.nan), np.full((8, 2), np.inf), draws, min_inliers=4)


def test_ties_and_min_inliers(ctx):
    X, uv, T, _ = pnp_scene(65, seed=4, outlier_frac=0.0, noise_px=0.0)
    K = [float(k) for k in K9]
    # the same triangle in two orders: the same solutions from other operations, so other pose bytes, and on a
    # noise-free scene both hold every edge: a tie on the count that the first hypothesis wins
    draws = np.array([(9, 3, 40), (3, 9, 40), (40, 3, 9)], np.uint32)
    best = []
    for d in draws:
        c = ref.hypothesis_candidates(X, uv, K, d, 65)
        cnt = [int(ref.inlier_mask(p, X, uv, K9, 2.0).sum()) for _, p in c]
        best.append((max(cnt), np.array(c[int(np.argmax(cnt))][1])))
    assert best[0][0] == best[1][0] == best[2][0] == 65
    assert best[0][1].tobytes() != best[1][1].tobytes()
    want = _same(ctx, X, uv, draws)
    assert want[0].tobytes() == best[0][1].tobytes()
    want = _same(ctx, X, uv, draws[[1, 0, 2]])
    assert want[0].tobytes() == best[1][1].tobytes()
    # min_inliers one above the best count: not found, the pose bytes untouched
    Xo, uvo, _, _ = pnp_scene(65, seed=5, outlier_frac=0.5)
    d = ref.make_draws(64, 2)
    top = _same(ctx, Xo, uvo, d)[2]
    assert top >= 12
    assert _same(ctx, Xo, uvo, d, min_inliers=top)[3]
    want = _same(ctx, Xo, uvo, d, min_inliers=top + 1)
    assert not want[3] and want[0].tobytes() == PRIOR.tobytes()


@pytest.mark.parametrize("sizes,iters", [([200], 64), ([65, 0, 4100], 4), (None, 16)])
def test_batch_equals_single_calls(ctx, sizes, iters):
    import torch
    if sizes is None:  # 70 problems of mixed sizes, empty ones among them
        rng = np.random.default_rng(9)
        sizes = [int(s) for s in rng.choice([0, 0, 1, 3, 4, 17, 63, 64, 65, 130, 257], 70)]
    probs = [pnp_scene(n, seed=20 + i, outlier_frac=0.4) for i, n in enumerate(sizes)]
    draws = ref.make_draws(iters, 4)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    X = np.concatenate([p[0].reshape(-1, 3) for p in probs] + [np.zeros((1, 3))])
    uv = np.concatenate([p[1].reshape(-1, 2) for p in probs] + [np.zeros((1, 2))])
    P = len(sizes)
    pri = np.tile(PRIOR, (P, 1)) + np.arange(P)[:, None]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_off, d_X, d_uv, d_K = dev(off), dev(X), dev(uv), dev(np.tile(K9, (P, 1)))
    d_draws = dev(draws.view(np.int32))
    d_pose = dev(pri)
    d_mask = torch.full((len(X),), 7, dtype=torch.uint8, device="cuda:0")
    d_inl = torch.full((P,), -1, dtype=torch.int32, device="cuda:0")
    d_found = torch.full((P,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.pnp_ransac_batch(P, d_off.data_ptr(), d_X.data_ptr(), d_uv.data_ptr(), d_K.data_ptr(), d_draws.data_ptr(),
                         iters, d_pose.data_ptr(), d_mask.data_ptr(), d_inl.data_ptr(), d_found.data_ptr(),
                         thr=2.0, min_inliers=5)
    ctx.sync()
    pose, mask = d_pose.cpu().numpy(), d_mask.cpu().numpy()
    inl, found = d_inl.cpu().numpy(), d_found.cpu().numpy()
    n_found = 0
    for i, n in enumerate(sizes):
        m = min(n, ref.kMaxEdges)
        Xi, uvi = probs[i][0][:m], probs[i][1][:m]
        if n <= ref.kMaxEdges:
            T, mk, c, f = ctx.pnp_ransac(Xi, uvi, K9, draws=draws, min_inliers=5, pose=pri[i])
        else:  # the batch form solves a longer problem on its first 4096 edges and leaves the mask past them
            T, mk, c, f = ref.pnp_ransac(probs[i][0], probs[i][1], K9, draws, 2.0, 5, pri[i])[:4]
            mk = mk[:m]
            assert np.all(mask[off[i] + m:off[i + 1]] == 7)
        assert (int(found[i]), int(inl[i])) == (int(f), c), i
        np.testing.assert_array_equal(mask[off[i]:off[i] + m].astype(bool), mk)
        assert pose[i].tobytes() == T.tobytes(), i
        n_found += int(f)
    assert mask[-1] == 7 and n_found >= sum(s >= 63 for s in sizes)
    # the specification itself on a few of them
    for i in range(0, P, 9):
        w = ref.pnp_ransac(probs[i][0], probs[i][1], K9, draws, 2.0, 5, pri[i])
        assert pose[i].tobytes() == w[0].tobytes() and int(inl[i]) == w[2]


# ---- the batch tracker: tests/test_gpu_track.py's small fixture, priors 1.2 rad off ----
H, W = 376, 1241
T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
N_FRAMES = 3
FAR = scene.pose(scene.quat_from_axis_angle((0.2, 1.0, 0.1), 1.2), [0.0, 0.0, 0.0])
TRACK_RANSAC = dict(iters=64, thr=2.0, min_inliers=12, seed=0)


@pytest.fixture(scope="module")
def frames():
    return np.stack([im for k in range(N_FRAMES) for im in (synth_frame(51, k, 3 * k), synth_frame(51, k, 3 * k + 8))])


def _track(ctx, frames, overlap, lk, ransac):
    """One run + track of the fixture with the priors FAR -> poses, the edges of every track, the ransac view."""
    import torch
    b = yv.Batch(ctx, 2 * N_FRAMES, H, W, 2000, 2 * N_FRAMES)
    carry = 2 * N_FRAMES
    pairs = []
    for k in range(N_FRAMES):
        pairs.append((carry if k == 0 else 2 * (k - 1), 2 * k))
        pairs.append((2 * k, 2 * k + 1))
    b.set_pairs(pairs)
    if lk:
        b.set_track_lk(2)
        tracks = [(2 * (k - 1) + 1, 2 * k) for k in range(1, N_FRAMES)]
    else:
        tracks = [(2 * k + 1, 2 * k) for k in range(N_FRAMES)]
    b.set_tracks(tracks, scene.K_KITTI, T_RIGHT)
    b.set_track_overlap(overlap)
    if ransac == "on":
        b.set_track_ransac(**TRACK_RANSAC)
    elif ransac == "on-off":
        b.set_track_ransac(**TRACK_RANSAC)
        b.set_track_ransac(0)
    nt = len(tracks)
    d = torch.from_numpy(frames).to("cuda:0")
    d_prior = torch.from_numpy(np.tile(FAR, (nt, 1))).to("cuda:0")
    d_pose = torch.zeros((nt, 7), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    b.run(d.data_ptr(), len(frames), W, H * W, 20)
    b.track(d_prior.data_ptr(), d_pose.data_ptr())
    ctx.sync()
    b.track_sync()
    torch.cuda.synchronize()
    v = b.view()
    cnt = ctx.download(v.edge_count, np.int32, nt)
    edges = []
    for t in range(nt):
        base = t * 2000
        edges.append((ctx.download(v.edge_X + base * 24, np.float64, 3 * cnt[t]).reshape(-1, 3)[:cnt[t]],
                      ctx.download(v.edge_uv + base * 16, np.float64, 2 * cnt[t]).reshape(-1, 2)[:cnt[t]]))
    out = dict(poses=d_pose.cpu().numpy(), edges=edges, nt=nt)
    if ransac == "on":
        rv = b.ransac_view()
        assert rv.n_tracks == nt
        out["r_pose"] = ctx.download(rv.pose, np.float64, 7 * nt).reshape(nt, 7)
        out["r_mask"] = ctx.download(rv.inlier, np.uint8, 2000 * nt).reshape(nt, 2000)
        out["r_inliers"] = ctx.download(rv.inliers, np.int32, nt)
        out["r_found"] = ctx.download(rv.found, np.int32, nt)
    else:
        with pytest.raises(yv.YavoError):
            b.ransac_view()
    b.close()
    return out


@pytest.mark.parametrize("overlap,lk", [(0, False), (2, False), (0, True)])
def test_track_ransac(ctx, oracle, frames, overlap, lk):
    off = _track(ctx, frames, overlap, lk, "off")
    nt = off["nt"]
    mode = yv.track_lm_sum_mode(nt)
    K = scene.K_KITTI
    # off: the existing chain, the LM from the caller's prior over the track's edges, byte for byte; and a mode that
    # was on and is off again leaves nothing behind
    for t, (X, uv) in enumerate(off["edges"]):
        T = oracle.pose_lm(X, uv, K, FAR, mode)[0]
        assert off["poses"][t].tobytes() == np.asarray(T).tobytes(), t
    again = _track(ctx, frames, overlap, lk, "on-off")
    assert again["poses"].tobytes() == off["poses"].tobytes()
    # on: specification RANSAC over the view's edges -> prior -> the oracle's LM
    on = _track(ctx, frames, overlap, lk, "on")
    draws = ref.make_draws(TRACK_RANSAC["iters"], TRACK_RANSAC["seed"])
    n_found = 0
    for t, (X, uv) in enumerate(on["edges"]):
        np.testing.assert_array_equal(X, off["edges"][t][0])
        np.testing.assert_array_equal(uv, off["edges"][t][1])
        prior, mask, inl, found, _ = ref.pnp_ransac(X, uv, K9, draws, 2.0, 12, FAR)
        print(f"track {t}: {len(X)} edges, found {int(found)}, {inl} inliers; gpu {on['r_found'][t]} {on['r_inliers'][t]}")
        assert (int(on["r_found"][t]), int(on["r_inliers"][t])) == (int(found), inl), t
        assert on["r_pose"][t].tobytes() == prior.tobytes(), t
        np.testing.assert_array_equal(on["r_mask"][t][:len(X)].astype(bool), mask)
        T = np.asarray(oracle.pose_lm(X, uv, K, prior, mode)[0])
        assert on["poses"][t].tobytes() == T.tobytes(), t
        if not found:
            assert prior.tobytes() == FAR.tobytes()
        n_found += int(found)
        if found and len(X) >= 100 and not lk:
            # the synthetic motion of tests/test_gpu_track.py, which the LM from a prior 1.2 rad off does not reach
            np.testing.assert_allclose(T[4:], [0.0675, 0.2025, 0.0], atol=2e-3)
            assert abs(abs(T[3]) - 1.0) < 1e-4
    assert n_found >= nt - 1  # (the first match track reads the empty carry slot: no edges, nothing found)


def test_ransac_recovers_what_the_lm_alone_loses(ctx):
    """Large motion, 50 % outliers: yv_pose_lm from the identity keeps fewer than half of the 100 clean edges,
    yv_pnp_ransac -> yv_pose_lm keeps all of them."""
    for seed in range(4):
        X, uv, T, clean = pnp_scene(200, seed, 0.5, True)
        _, out, _ = ctx.pose_lm(X, uv, scene.K_KITTI, IDENTITY)
        assert int((~out[clean]).sum()) < 50
        prior, mask, inl, found = ctx.pnp_ransac(X, uv, K9, seed=0, iters=64, thr=2.0, min_inliers=12)
        assert found and not np.any(mask & ~clean)
        Tl, out, linl = ctx.pose_lm(X, uv, scene.K_KITTI, prior)
        assert int((~out[clean]).sum()) == 100 and linl == 100
        assert np.linalg.norm(Tl[4:] - T[4:]) < 0.02


def test_sequence_frontend_passes_the_mode_through(ctx):
    from ya_vo_amd.sequence import SequenceFrontend
    fe = SequenceFrontend(ctx, 2, scene.K_KITTI, T_RIGHT, ransac=dict(iters=16, thr=2.0, min_inliers=12, seed=3))
    assert fe.batch.ransac_view().n_tracks == 2
    fe.close()
    fe = SequenceFrontend(ctx, 2, scene.K_KITTI, T_RIGHT)  # the default: off
    with pytest.raises(yv.YavoError):
        fe.batch.ransac_view()
    fe.close()
