"""SequenceFrontend(loop=...): the bag-of-words index beside the sequence loop.  A short sequence whose last frames return
to its first crops, a few pixels off: the revisits report their original frames as first candidate, nothing inside the
exclusion window is reported, the candidate lists are the specification's over the CPU oracle's descriptors, and the
trajectory is bit-identical to the run without the index."""
import numpy as np
import pytest

from ya_vo_amd import bow
from ya_vo_amd.sequence import SequenceFrontend
from ya_vo_amd.synth import synth_frame

import bow_reference as ref
import bow_scenes

pytestmark = pytest.mark.gpu

H, W, MAX_KP, CHUNK = 120, 320, 400, 4
N_OUT, N_BACK, STEP = 20, 4, 40        # 20 frames STEP columns apart, then the first 4 again, (1, 4) pixels off
EXCLUDE, TOP_K = 8, 4
K = np.array([[300.0, 0, 160.0], [0, 300.0, 60.0], [0, 0, 1.0]])
T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)


def _origin(k):
    return (k, STEP * k) if k < N_OUT else (k - N_OUT + 1, STEP * (k - N_OUT) + 4)


def _frames():
    out = []
    for k in range(N_OUT + N_BACK):
        r, c = _origin(k)
        out += [synth_frame(71, r, c, H, W), synth_frame(71, r, c + 8, H, W)]
    return np.stack(out)


def _run(ctx, d, loop):
    fe = SequenceFrontend(ctx, CHUNK, K, T_RIGHT, H=H, W=W, max_kp=MAX_KP, loop=loop)
    try:
        for c in range((N_OUT + N_BACK) // CHUNK):
            fe.process_chunk(d[2 * c * CHUNK:2 * (c + 1) * CHUNK])
            assert fe.loop_candidates == []  # read back when the front end synchronises, not in the chunk loop
        return fe.trajectory(), list(fe.loop_candidates)
    finally:
        fe.close()


def test_revisits_find_their_frames_and_the_trajectory_is_unchanged(ctx, oracle, offsets):
    import torch
    frames = _frames()
    d = torch.from_numpy(frames).to("cuda:0")
    torch.cuda.synchronize()
    words = bow_scenes.scene(256, 0)[2]
    idx = bow.BowIndex(ctx, words, None, max_entries=32, max_queries=CHUNK, max_kp=MAX_KP)
    try:
        traj, cands = _run(ctx, d, dict(index=idx, every=1, exclude=EXCLUDE, top_k=TOP_K, min_score=0.0))
        assert len(idx) == N_OUT + N_BACK and idx.entry_frames == list(range(N_OUT + N_BACK))
    finally:
        idx.close()
    plain, none = _run(ctx, d, None)
    np.testing.assert_array_equal(traj, plain)
    assert none == []

    # the specification over the oracle's descriptors of the left images: query, then add, frame by frame
    spec, exp = ref.Index(words, None), []
    for f in range(N_OUT + N_BACK):
        desc = bow_scenes.describe(oracle, offsets, frames[2 * f])["featVec"]
        exp += [(f, spec.frames[e], s) for e, s, _ in spec.query(desc, f, EXCLUDE, TOP_K)[0]]
        spec.add(desc, f)
    assert cands == exp
    assert all(abs(f - g) >= EXCLUDE for f, g, _ in cands)
    for f in range(N_OUT, N_OUT + N_BACK):
        mine = [(g, s) for ff, g, s in cands if ff == f]
        assert mine[0][0] == f - N_OUT, (f, mine)  # rank order: the first is the best
        assert all(mine[k][1] >= mine[k + 1][1] for k in range(len(mine) - 1))


def test_min_score_and_every_filter_the_candidates(ctx, oracle, offsets):
    """every = 2 queries and adds the even frames only; min_score keeps the candidates at or above it."""
    import torch
    frames = _frames()
    d = torch.from_numpy(frames).to("cuda:0")
    torch.cuda.synchronize()
    words = bow_scenes.scene(256, 0)[2]
    lo = 0.75
    idx = bow.BowIndex(ctx, words, None, max_entries=32, max_queries=CHUNK, max_kp=MAX_KP)
    try:
        _, cands = _run(ctx, d, dict(index=idx, every=2, exclude=EXCLUDE, top_k=TOP_K, min_score=lo))
        assert idx.entry_frames == list(range(0, N_OUT + N_BACK, 2))
    finally:
        idx.close()
    spec, exp = ref.Index(words, None), []
    for f in range(0, N_OUT + N_BACK, 2):
        desc = bow_scenes.describe(oracle, offsets, frames[2 * f])["featVec"]
        exp += [(f, spec.frames[e], s) for e, s, _ in spec.query(desc, f, EXCLUDE, TOP_K)[0]]
        spec.add(desc, f)
    kept = [c for c in exp if c[2] >= lo]
    assert cands == kept and 0 < len(kept) < len(exp)
    assert (20, 0) in [(f, g) for f, g, _ in cands] and (22, 2) in [(f, g) for f, g, _ in cands]
