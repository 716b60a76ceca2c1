"""SequenceFrontend(loop={..., verify=LoopVerifier}): geometric verification of the bag-of-words candidates beside the
sequence loop.  The 24-frame sequence of tests/test_gpu_sequence_bow.py: the four revisits close on their original
frames with the specification's pose and inlier count, bit for bit; every closure is the specification applied to the
specification's candidate list; the candidates and the trajectory are those of the runs without verification."""
import functools

import numpy as np
import pytest

from ya_vo_amd import bow, loop
from ya_vo_amd.sequence import SequenceFrontend

import bow_reference
import bow_scenes
import loop_reference as ref
import loop_scenes as sc

pytestmark = pytest.mark.gpu

CHUNK, EXCLUDE, TOP_K = 4, 8, 4


def _run(ctx, d, with_index, with_verify, ransac=None):
    """-> (trajectory, loop_candidates, loop_closures) of one pass over the sequence"""
    words = bow_scenes.scene(256, 0)[2]
    idx = ver = None
    lp = None
    if with_index:
        idx = bow.BowIndex(ctx, words, None, max_entries=32, max_queries=CHUNK, max_kp=sc.MAX_KP)
        lp = dict(index=idx, every=1, exclude=EXCLUDE, top_k=TOP_K, min_score=0.0)
    if with_verify:
        ver = loop.LoopVerifier(ctx, sc.K, sc.T_RIGHT, max_entries=32, max_problems=CHUNK * TOP_K, max_kp=sc.MAX_KP)
        P = sc.params(3)
        ver.set_params(P.match_thr, P.flags, P.num, P.den, len(P.draws), P.thr_px, P.min_inliers, draws=P.draws)
        lp["verify"] = ver
    fe = SequenceFrontend(ctx, CHUNK, sc.K, sc.T_RIGHT, H=sc.H, W=sc.W, max_kp=sc.MAX_KP, loop=lp, ransac=ransac)
    try:
        for c in range(sc.N_FRAMES // CHUNK):
            fe.process_chunk(d[2 * c * CHUNK:2 * (c + 1) * CHUNK])
            assert fe.loop_candidates == [] and fe.loop_closures == []  # read back at flush, not in the chunk loop
        traj = fe.trajectory()
        if with_verify:
            assert len(ver) == sc.N_FRAMES and ver.entry_frames == idx.entry_frames == list(range(sc.N_FRAMES))
        return traj, list(fe.loop_candidates), list(fe.loop_closures)
    finally:
        fe.close()
        for o in (ver, idx):
            if o is not None:
                o.close()


@functools.lru_cache(maxsize=None)
def _expected():
    """The specification's candidates (tests/bow_reference.py: query, then add, frame by frame) and, for each, the
    specification's verification against the store of the frames before it -> (candidates, closures)"""
    import oracle_bind
    orc = oracle_bind.Oracle()
    words = bow_scenes.scene(256, 0)[2]
    spec, cands = bow_reference.Index(words, None), []
    for f in range(sc.N_FRAMES):
        desc = sc.keypoints(f)[0]["featVec"]
        cands += [(f, e, s) for e, s, _ in spec.query(desc, f, EXCLUDE, TOP_K)[0]]
        spec.add(desc, f)
    store, P, mode = sc.store(sc.N_FRAMES), sc.params(3), loop.lm_sum_mode(CHUNK * TOP_K)
    closures = []
    for f, e, _ in cands:
        r = ref.verify(orc, sc.keypoints(f)[0], store, e, sc.K, P, mode)
        if r.verified:
            closures.append((f, e, r.pose, r.lm_inliers))
    return cands, closures


def _same_closures(got, want):
    assert [(f, g, n) for f, g, _, n in got] == [(f, g, n) for f, g, _, n in want]
    for a, b in zip(got, want):
        assert np.asarray(a[2], np.float64).tobytes() == np.asarray(b[2], np.float64).tobytes(), (a, b)


@pytest.fixture(scope="module")
def d_frames():
    import torch
    d = torch.from_numpy(np.array(sc.frames())).to("cuda:0")
    torch.cuda.synchronize()
    return d


def test_revisits_close_and_nothing_else_changes(ctx, d_frames):
    traj, cands, closures = _run(ctx, d_frames, True, True)
    want_cands, want = _expected()
    assert cands == want_cands  # entry index == frame id here
    _same_closures(closures, want)
    # the four revisits close on their own places, with the table's pose
    table = dict(zip(sc.PROBLEMS, sc.reference(3, loop.lm_sum_mode(CHUNK * TOP_K))))
    for f in range(sc.N_OUT, sc.N_FRAMES):
        mine = [c for c in closures if c[0] == f and c[1] == f - sc.N_OUT]
        assert len(mine) == 1, (f, closures)
        r = table[(f, f - sc.N_OUT)]
        assert mine[0][2].tobytes() == r.pose.tobytes() and mine[0][3] == r.lm_inliers >= 300
    assert all(abs(f - g) >= EXCLUDE for f, g, _, _ in closures)
    # without verify: the same candidates, no closures; without the index: the same trajectory
    traj_i, cands_i, closures_i = _run(ctx, d_frames, True, False)
    assert cands_i == cands and closures_i == []
    np.testing.assert_array_equal(traj_i, traj)
    traj_0, cands_0, closures_0 = _run(ctx, d_frames, False, False)
    assert cands_0 == [] and closures_0 == []
    np.testing.assert_array_equal(traj_0, traj)


def test_track_ransac_beside_the_verification(ctx, d_frames):
    """The batch's track RANSAC (the context's hypothesis workspace, on the LM's stream) and the verification's (the
    object's own) in one front end: the same closures."""
    _, cands, closures = _run(ctx, d_frames, True, True, ransac=dict(iters=64, thr=2.0, min_inliers=12, seed=0))
    want_cands, want = _expected()
    assert cands == want_cands
    _same_closures(closures, want)
