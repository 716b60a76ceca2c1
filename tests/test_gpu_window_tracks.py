"""GPU parity of the BA window's multi-view mode (SequenceFrontend(multiview=True)): landmarks the temporal matches
follow over several frames enter the window once, observed by every frame of their chain.

  host assembly (window_problem_tracks + yv_ba_set_problem)  ==  the oracle loop of tests/sequence_tracks_chain.py
  device window (yv_ba_window_set_multiview)                 ==  the host assembly

each bit for bit: trajectory, BA logs, every record's X, and the links the device recorded.  Full-size synthetic
frames, as tests/test_gpu_sequence.py; the sizes put chains across add_block calls and across the window's start."""
import numpy as np
import pytest

from sequence_chain import front_end, ground_truth, rmse_translation
from sequence_tracks_chain import sequence_tracks_from_tracks
from track_chain import lm_sum_mode_default
from ya_vo_amd import scene
from ya_vo_amd.sequence import SequenceFrontend, SequenceShard
from ya_vo_amd.synth import synth_sequence

pytestmark = pytest.mark.gpu

T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
SIZES = [(12, 4), (12, 6)]

_frames, _tracks, _oracle, _device = {}, {}, {}, {}


def _sequence(n, blank):
    """[n, 2, H, W]; blank: that stereo frame filled with 128 (no keypoints: its records and the next frame's are
    empty, every chain is cut there)."""
    if (n, blank) not in _frames:
        f = synth_sequence(71, n, stereo=True)
        if blank is not None:
            f = f.copy()
            f[blank] = 128
        _frames[(n, blank)] = f
    return _frames[(n, blank)]


def _oracle_run(oracle, offsets, n, chunk, blank=None):
    """The oracle loop with multi-view windows, computed once per size; the per-frame front end once per sequence and
    pose-LM sum order."""
    if (n, chunk, blank) not in _oracle:
        tk = (n, blank, lm_sum_mode_default(chunk))
        if tk not in _tracks:
            _tracks[tk] = front_end(oracle, _sequence(n, blank), chunk, scene.K_KITTI, T_RIGHT, offsets, threads=8)
        _oracle[(n, chunk, blank)] = sequence_tracks_from_tracks(oracle, _tracks[tk], chunk, scene.K_KITTI)
    return _oracle[(n, chunk, blank)]


def _device_run(ctx, n, chunk, device_window, blank=None):
    """SequenceFrontend(multiview=True) over the sequence -> (trajectory, records, ba_log, links per frame or None)."""
    import torch
    key = (n, chunk, device_window, blank)
    if key not in _device:
        frames = _sequence(n, blank)
        fe = SequenceFrontend(ctx, chunk, scene.K_KITTI, T_RIGHT, device_window=device_window, multiview=True)
        d = torch.from_numpy(frames.reshape(2 * n, *frames.shape[2:])).to("cuda:0")
        for c in range(n // chunk):
            fe.process_chunk(d[2 * c * chunk:2 * (c + 1) * chunk])
        traj = fe.trajectory()
        links = {g: fe.win.read_links(g) for g in range(n)} if device_window else None
        _device[key] = (traj, fe.records, list(fe.ba_log), links)
        fe.close()
    return _device[key]


def _assert_logs_equal(a, b):
    assert [x[:2] for x in a] == [x[:2] for x in b]
    np.testing.assert_array_equal(np.array([x[2:] for x in a]), np.array([x[2:] for x in b]))


def _host_equals_oracle(ctx, oracle, offsets, n, chunk, blank=None):
    traj, rec, log, _ = _device_run(ctx, n, chunk, False, blank)
    ref, ref_rec, ref_log, obs = _oracle_run(oracle, offsets, n, chunk, blank)
    _assert_logs_equal(log, ref_log)
    np.testing.assert_array_equal(traj, ref)
    assert sorted(rec) == sorted(ref_rec)
    for g, r in ref_rec.items():
        np.testing.assert_array_equal(rec[g].edge, r.edge)
        np.testing.assert_array_equal(rec[g].X, r.X)
    return obs


def _parents(records, n):
    """The rule on the host records' indices: the smallest l' of frame g - 1 whose train is the record's query."""
    out = {}
    for g in range(n):
        first = {}
        if g >= 1:
            for l, t in enumerate(records[g - 1].train):
                first.setdefault(int(t), l)
        out[g] = np.array([first.get(int(q), -1) for q in records[g].query], np.int32)
    return out


def _device_equals_host(ctx, n, chunk, blank=None):
    t_dev, r_dev, l_dev, links = _device_run(ctx, n, chunk, True, blank)
    t_host, r_host, l_host, _ = _device_run(ctx, n, chunk, False, blank)
    assert len(l_dev) == n // chunk and l_dev == l_host
    np.testing.assert_array_equal(t_dev, t_host)
    assert sorted(r_dev) == sorted(r_host) == list(range(n))
    parents = _parents(r_host, n)
    for g in r_host:
        np.testing.assert_array_equal(r_dev[g].T_wc, r_host[g].T_wc)
        np.testing.assert_array_equal(r_dev[g].edge, r_host[g].edge)
        np.testing.assert_array_equal(r_dev[g].X, r_host[g].X)
        np.testing.assert_array_equal(r_dev[g].uv_own, r_host[g].uv_own)
        np.testing.assert_array_equal(r_dev[g].uv_prev, r_host[g].uv_prev)
        q, t, p = links[g]
        np.testing.assert_array_equal(q, r_host[g].query)
        np.testing.assert_array_equal(t, r_host[g].train)
        np.testing.assert_array_equal(p, parents[g])
    return parents


@pytest.mark.parametrize("n,chunk", SIZES)
def test_host_multiview_matches_oracle(ctx, oracle, offsets, n, chunk):
    obs = _host_equals_oracle(ctx, oracle, offsets, n, chunk)
    # the windows do hold multi-view landmarks: the test cannot pass on unlinked graphs
    assert len(obs) > 1000 and np.mean(obs >= 3) >= 0.5


@pytest.mark.parametrize("n,chunk", SIZES)
def test_device_window_multiview_equals_host_assembly(ctx, n, chunk):
    parents = _device_equals_host(ctx, n, chunk)
    # chains cross the add_block calls: records of a chunk's first frame have parents in the chunk before
    assert (parents[chunk] >= 0).sum() > 100


def test_blank_stereo_frame_cuts_every_chain(ctx, oracle, offsets):
    n, chunk, blank = 8, 4, 5
    _host_equals_oracle(ctx, oracle, offsets, n, chunk, blank)
    parents = _device_equals_host(ctx, n, chunk, blank)
    _, rec, _, _ = _device_run(ctx, n, chunk, False, blank)
    assert len(rec[blank].edge) == 0 and len(rec[blank + 1].edge) == 0
    assert len(rec[blank + 2].edge) > 100 and (parents[blank + 2] < 0).all()


def test_multiview_trajectory_follows_ground_truth(ctx):
    n, chunk = 12, 6
    traj, _, _, _ = _device_run(ctx, n, chunk, True)
    assert rmse_translation(traj, ground_truth(n, scene.K_KITTI)) < 0.02


def test_multiview_argument_checks(ctx):
    import torch
    n = chunk = 4
    frames = _sequence(12, None)[:n]
    d = torch.from_numpy(np.ascontiguousarray(frames).reshape(2 * n, *frames.shape[2:])).to("cuda:0")
    fe = SequenceFrontend(ctx, chunk, scene.K_KITTI, T_RIGHT, device_window=True, multiview=True)
    try:
        fe.process_chunk(d)
        assert fe._ba_pending
        with pytest.raises(RuntimeError):
            fe.win.set_multiview(False)  # a solve is pending
        fe.win.solve_end()
        fe._ba_pending = False
        fe.win.set_multiview(True)  # the setting it has
        with pytest.raises(RuntimeError):
            fe.win.set_multiview(False)  # frames are recorded with links
        v = fe.batch.view()
        with pytest.raises(RuntimeError):  # the mode is on: a block without match_dj has no links
            fe.win.add_block(fe.d_block.data_ptr(), n, chunk, v.edge_uv, v.edge_query, v.matches, fe.max_kp)
    finally:
        fe.close()
    fe = SequenceFrontend(ctx, chunk, scene.K_KITTI, T_RIGHT, device_window=True)
    try:
        fe.process_chunk(d)
        fe.flush()
        with pytest.raises(RuntimeError):
            fe.win.set_multiview(True)  # frames are recorded without links
        with pytest.raises(RuntimeError):
            fe.win.read_links(0)
    finally:
        fe.close()
    with pytest.raises(ValueError):
        SequenceShard(ctx, 0, 1, 4, 4, scene.K_KITTI, T_RIGHT, multiview=True)
