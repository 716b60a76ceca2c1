"""The match records written beside the next run (overlap mode with the asynchronous edge build and tracks: a key-only
finalize on the run's stream, match_records_kernel on the batch's records stream) against an in-order batch (overlap
off, the fused finalize) fed the same images: the two record lists, the counts, match_dj / match_lim, the edges and the
poses, byte for byte.  The lists and match_dj are filled with a sentinel before the first run, so whole buffers are
compared: slots at and past a pair's count must stay untouched in both.

Images are windows of one noise field (frame k at (+k rows, +3k columns), the right image 8 columns further), so
temporal and stereo pairs have true matches beside the noise ones; every run rotates the frames by one.  Small images
with max_kp 64 and a flat border put every count at the cap, max_kp 300 leaves the counts below it and odd; with
max_kp 301 the lists of the odd pairs are not 16-byte aligned (the records kernel's dword stores)."""
import ctypes

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import scene

pytestmark = pytest.mark.gpu

T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
SENTINEL = 0xA5
SHAPES = [(80, 100), (72, 200)]  # H, W


BORDER = 12  # checkBoundry keeps 8 <= row <= H - 8: behind a flat border this wide every corner survives it


def _frames(H, W, F, seed=7, flat=(), border=0):
    """[2F, H, W]: L_0, R_0, L_1, ...; the images listed in `flat` are constant (no keypoint), `border` pixels around
    every image are flat (every corner then passes checkBoundry: the counts reach max_kp)."""
    field = np.random.default_rng(seed + 1000 * H + W).integers(0, 256, (H + F + 8, W + 3 * F + 16), dtype=np.uint8)
    out = []
    for k in range(F):
        out.append(field[k:k + H, 3 * k:3 * k + W])
        out.append(field[k:k + H, 3 * k + 8:3 * k + 8 + W])
    return np.ascontiguousarray(np.stack(out)), tuple(flat), border


def _run_images(frames, r):
    imgs, flat, border = frames
    F = len(imgs) // 2
    out = np.roll(imgs.reshape(F, 2, *imgs.shape[1:]), -r, axis=0).reshape(imgs.shape).copy()
    if border:
        inner = out[:, border:-border, border:-border].copy()
        out[:] = 128
        out[:, border:-border, border:-border] = inner
    for i in flat:
        out[i] = 128
    return out


def _make_batch(ctx, H, W, F, max_kp, overlap, filt=False, subpix=False):
    b = yv.Batch(ctx, 2 * F, H, W, max_kp, 2 * F)
    carry = 2 * F
    pairs, tracks = [], []
    for k in range(F):
        pairs.append((carry if k == 0 else 2 * (k - 1), 2 * k))  # temporal L_{k-1} -> L_k
        pairs.append((2 * k, 2 * k + 1))                          # stereo L_k -> R_k
        tracks.append((2 * k + 1, 2 * k))
    b.set_pairs(pairs)
    b.set_tracks(tracks, scene.K_KITTI, T_RIGHT)
    if filt:
        b.set_match_filter(ratio=(4, 5), mutual=True)
    if subpix:
        b.set_stereo_subpix([2 * k + 1 for k in range(F)], half_win=3, search=2)
    b.set_track_overlap(overlap)
    v = b.view()
    n = 2 * F * max_kp
    ctx.upload(v.matches, np.full(n * 100, SENTINEL, np.uint8))
    ctx.upload(v.filtered, np.full(n * 100, SENTINEL, np.uint8))
    ctx.upload(v.match_dj, np.full(n * 8, SENTINEL, np.uint8))
    return b


def _lists(ctx, b, F, max_kp):
    v = b.view()
    n = 2 * F
    return {
        "match_count": ctx.download(v.match_count, np.int32, n),
        "filt_count": ctx.download(v.filt_count, np.int32, n),
        "matches": ctx.download(v.matches, np.uint8, n * max_kp * 100),
        "filtered": ctx.download(v.filtered, np.uint8, n * max_kp * 100),
        "match_dj": ctx.download(v.match_dj, np.int32, n * max_kp * 2),
        "match_lim": ctx.download(v.match_lim, np.int32, n),
    }


def _snapshot(ctx, b, d_pose, F, max_kp):
    """Everything a run and its track left, as bytes (after the caller's synchronisation)."""
    s = _lists(ctx, b, F, max_kp)
    v = b.view()
    cnt = ctx.download(v.edge_count, np.int32, F)
    s["edge_count"] = cnt
    s["track_inliers"] = ctx.download(v.track_inliers, np.int32, F)
    for k in range(F):
        c, base = int(cnt[k]), k * max_kp
        s[f"edge_X{k}"] = ctx.download(v.edge_X + base * 24, np.uint8, 24 * c) if c else np.zeros(0, np.uint8)
        s[f"edge_uv{k}"] = ctx.download(v.edge_uv + base * 16, np.uint8, 16 * c) if c else np.zeros(0, np.uint8)
        s[f"edge_query{k}"] = ctx.download(v.edge_query + base * 4, np.int32, c) if c else np.zeros(0, np.int32)
        s[f"edge_outlier{k}"] = ctx.download(v.edge_outlier + base, np.uint8, c) if c else np.zeros(0, np.uint8)
    s["poses"] = d_pose.cpu().numpy().view(np.uint8).copy()
    return s


def _assert_same(got, ref, what):
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert got[k].tobytes() == ref[k].tobytes(), (what, k, int(np.count_nonzero(got[k] != ref[k])))


def _sequence(ctx, H, W, F, max_kp, overlap, runs, *, sync_each, frames=None, carry_from=None, filt=False,
              subpix=False, timing=None):
    """`runs` run + track steps; the snapshots of every run (sync_each) or of the last one only.  timing: the
    enable_timing argument before each run (None: untouched)."""
    import torch
    frames = frames if frames is not None else _frames(H, W, F, border=BORDER if max_kp == 64 else 0)
    carry_from = 2 * (F - 1) if carry_from is None else carry_from
    b = _make_batch(ctx, H, W, F, max_kp, overlap, filt, subpix)
    d_imgs = [torch.from_numpy(_run_images(frames, r)).to("cuda:0") for r in range(runs)]
    d_prior = torch.from_numpy(np.tile(IDENTITY, (F, 1))).to("cuda:0")
    d_pose = [torch.zeros((F, 7), dtype=torch.float64, device="cuda:0") for _ in range(runs)]
    torch.cuda.synchronize()
    snaps = []
    for r in range(runs):
        if timing is not None:
            b.enable_timing(timing[r])
        b.run(d_imgs[r].data_ptr(), 2 * F, W, H * W, 20, carry_from=carry_from)
        b.track(d_prior.data_ptr(), d_pose[r].data_ptr())
        if sync_each or r == runs - 1:
            ctx.sync()
            b.track_sync()
            snaps.append(_snapshot(ctx, b, d_pose[r], F, max_kp))
    b.close()
    return snaps


_REF = {}


def _reference(ctx, H, W, F, max_kp, runs, **kw):
    """The in-order batch's snapshots of every run, computed once per configuration."""
    key = (H, W, F, max_kp, runs, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REF:
        _REF[key] = _sequence(ctx, H, W, F, max_kp, 0, runs, sync_each=True, **kw)
    return _REF[key]


@pytest.mark.parametrize("max_kp", [64, 300, 301])  # 301: a pair's list not 16-B aligned
@pytest.mark.parametrize("H,W", SHAPES)
def test_pipelined_runs_leave_the_in_order_lists(ctx, H, W, max_kp):
    """Three runs, no host synchronisation between run / track / run, then track_sync: the last run's outputs."""
    ref = _reference(ctx, H, W, 3, max_kp, 3)
    nq = ref[-1]["match_count"]
    assert nq.max() <= max_kp and nq.max() > 0
    if max_kp == 64:
        assert np.all(nq == 64), nq  # at the cap
    else:
        assert nq.max() < 300 and np.any(nq % 4 != 0), nq  # below it, no multiple of anything
    got = _sequence(ctx, H, W, 3, max_kp, 1, 3, sync_each=False)
    _assert_same(got[0], ref[-1], "last run")


@pytest.mark.parametrize("max_kp", [64, 300, 301])  # 301: a pair's list not 16-B aligned
@pytest.mark.parametrize("H,W", SHAPES)
def test_every_run_after_track_sync(ctx, H, W, max_kp):
    """track_sync and a download after every run: every run's outputs."""
    ref = _reference(ctx, H, W, 3, max_kp, 3)
    got = _sequence(ctx, H, W, 3, max_kp, 1, 3, sync_each=True)
    for r in range(3):
        _assert_same(got[r], ref[r], f"run {r}")


@pytest.mark.parametrize("overlap", [1, 3])
def test_carry_copy_waits_for_the_records(ctx, overlap):
    """carry_from = a middle image: the next run's carry copy rewrites the carry slot's keypoints, which the records
    of the first temporal pair read.  Two runs back to back (overlap 3: with the LM deferred into the next run)."""
    H, W = SHAPES[0]
    ref = _reference(ctx, H, W, 4, 300, 2, carry_from=2)
    got = _sequence(ctx, H, W, 4, 300, overlap, 2, sync_each=False, carry_from=2)
    _assert_same(got[0], ref[-1], "second run")


def test_empty_query_and_empty_train(ctx):
    """L_1 flat: its pairs as query have nq = 0 (no record), the temporal pair L_0 -> L_1 has no train point (j = -1,
    pt2 zeroed in every record)."""
    H, W = SHAPES[1]
    frames = _frames(H, W, 3, flat=(2,))
    ref = _reference(ctx, H, W, 3, 300, 2, frames=frames)
    assert ref[-1]["match_count"][3] == 0 and ref[-1]["match_count"][4] == 0  # stereo L_1 -> R_1, temporal L_1 -> L_2
    nq = int(ref[-1]["match_count"][2])  # temporal L_0 -> L_1
    assert nq > 0
    dj = ref[-1]["match_dj"].reshape(6, 300, 2)[2, :nq]
    assert np.all(dj[:, 1] == -1)
    rec = ref[-1]["matches"].reshape(6, 300, 100)[2, :nq]
    assert not rec[:, 48:96].any()
    for sync_each in (False, True):
        got = _sequence(ctx, H, W, 3, 300, 1, 2, sync_each=sync_each, frames=frames)
        _assert_same(got[-1], ref[-1], f"sync_each={sync_each}")


@pytest.mark.parametrize("subpix", [False, True])
def test_with_the_match_filter(ctx, subpix):
    """Ratio test + cross-check (the filtering finalize without its record loop), and with the sub-pixel stage behind
    it."""
    H, W = SHAPES[0]
    ref = _reference(ctx, H, W, 3, 300, 3, filt=True, subpix=subpix)
    assert 0 < ref[-1]["filt_count"].sum() < ref[-1]["match_count"].sum()
    got = _sequence(ctx, H, W, 3, 300, 1, 3, sync_each=False, filt=True, subpix=subpix)
    _assert_same(got[0], ref[-1], "last run")
    got = _sequence(ctx, H, W, 3, 300, 1, 3, sync_each=True, filt=True, subpix=subpix)
    for r in range(3):
        _assert_same(got[r], ref[r], f"run {r}")


@pytest.mark.parametrize("sync_each", [True, False])
def test_timing_modes_between_runs(ctx, sync_each):
    """Every-stage timing keeps the fused finalize on the run's stream, detect-only timing and no timing defer the
    lists: one batch switching between them from run to run."""
    H, W = SHAPES[1]
    ref = _reference(ctx, H, W, 3, 64, 4)
    got = _sequence(ctx, H, W, 3, 64, 1, 4, sync_each=sync_each, timing=[True, 2, True, 0])
    if sync_each:
        for r in range(4):
            _assert_same(got[r], ref[r], f"run {r}")
    else:
        _assert_same(got[0], ref[-1], "last run")


def test_records_wait_orders_a_second_stream(ctx):
    """yv_batch_records_wait on a second stream, then a device-side copy of both lists on that stream, with no host
    synchronisation before it."""
    import torch
    H, W = SHAPES[0]
    F, max_kp = 3, 300
    ref = _reference(ctx, H, W, F, max_kp, 3)
    frames = _frames(H, W, F)
    b = _make_batch(ctx, H, W, F, max_kp, 1)
    d_imgs = [torch.from_numpy(_run_images(frames, r)).to("cuda:0") for r in range(3)]
    d_prior = torch.from_numpy(np.tile(IDENTITY, (F, 1))).to("cuda:0")
    d_pose = torch.zeros((F, 7), dtype=torch.float64, device="cuda:0")
    n = 2 * F * max_kp * 100
    copies = [torch.zeros(n, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    s2 = torch.cuda.Stream()
    hip = ctypes.CDLL("libamdhip64.so")
    torch.cuda.synchronize()
    v = b.view()
    for r in range(3):
        b.run(d_imgs[r].data_ptr(), 2 * F, W, H * W, 20, carry_from=2 * (F - 1))
        b.track(d_prior.data_ptr(), d_pose.data_ptr())
    b.records_wait(s2.cuda_stream)
    for dst, src in zip(copies, (v.matches, v.filtered)):
        rc = hip.hipMemcpyAsync(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src), ctypes.c_size_t(n), 3,
                                ctypes.c_void_p(s2.cuda_stream))
        assert rc == 0, f"hipMemcpyAsync {rc}"
    s2.synchronize()
    assert copies[0].cpu().numpy().tobytes() == ref[-1]["matches"].tobytes()
    assert copies[1].cpu().numpy().tobytes() == ref[-1]["filtered"].tobytes()
    ctx.sync()
    b.track_sync()
    b.close()


def test_setters_and_close_right_after_a_run(ctx):
    """set_pairs / set_tracks with a run's records possibly in flight, and a batch closed right after a run: all come
    back clean, and the context serves another batch."""
    import torch
    H, W = SHAPES[0]
    F, max_kp = 3, 300
    ref = _reference(ctx, H, W, F, max_kp, 3)
    frames = _frames(H, W, F)
    d_img = torch.from_numpy(_run_images(frames, 0)).to("cuda:0")
    d_prior = torch.from_numpy(np.tile(IDENTITY, (F, 1))).to("cuda:0")
    d_pose = torch.zeros((F, 7), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    b = _make_batch(ctx, H, W, F, max_kp, 1)
    b.run(d_img.data_ptr(), 2 * F, W, H * W, 20, carry_from=2 * (F - 1))
    b.track(d_prior.data_ptr(), d_pose.data_ptr())
    b.run(d_img.data_ptr(), 2 * F, W, H * W, 20, carry_from=2 * (F - 1))
    b.set_pairs([(0, 1), (6, 0)])            # the records kernel reads the pair list
    b.set_tracks([(0, 1)], scene.K_KITTI, T_RIGHT)
    b.run(d_img.data_ptr(), 2 * F, W, H * W, 20, carry_from=2 * (F - 1))
    b.set_tracks([(0, 1)] * 7, scene.K_KITTI, T_RIGHT)  # grows the track group
    b.run(d_img.data_ptr(), 2 * F, W, H * W, 20, carry_from=2 * (F - 1))
    b.set_track_overlap(0)
    b.set_track_overlap(1)
    b.run(d_img.data_ptr(), 2 * F, W, H * W, 20, carry_from=2 * (F - 1))
    b.close()                                # right after a run
    torch.cuda.synchronize()
    got = _sequence(ctx, H, W, F, max_kp, 1, 3, sync_each=False)
    _assert_same(got[0], ref[-1], "a new batch afterwards")


def test_deferred_equals_fused_at_full_lists(ctx):
    """max_kp 2000, two pairs of ~2000 records each (the workload's record count): the records kernel's grid over
    (pair, chunk) against the fused kernel's loop."""
    H, W, F, max_kp = 240, 320, 1, 2000
    ref = _reference(ctx, H, W, F, max_kp, 2)
    assert ref[-1]["match_count"].min() > 1500, ref[-1]["match_count"]
    got = _sequence(ctx, H, W, F, max_kp, 1, 2, sync_each=False)
    _assert_same(got[0], ref[-1], "second run")
