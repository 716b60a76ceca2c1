"""CPU tests of the multi-view BA window's host assembly (ya_vo_amd.sequence.window_problem_tracks /
apply_window_tracks, the restatement the device window's multi-view mode is checked against): hand-made records for
each arm of the rule, and the oracle front end's records against tests/sequence_tracks_chain.py, which links by
pixel instead of by keypoint index."""
import numpy as np
import pytest

import sequence_tracks_chain as tchain
from sequence_chain import Rec, front_end, records_from_block
from ya_vo_amd import scene
from ya_vo_amd.sequence import (FrameRecord, apply_window_tracks, frame_records_from_block, window_problem,
                                window_problem_tracks)
from ya_vo_amd.synth import synth_sequence

T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)


def _rec(g, query, train):
    """A frame's record with recognisable numbers: X = (g, l, 0), uv_own = (100 g + l, 1), uv_prev = (100 g + l, 2)."""
    n = len(query)
    l = np.arange(n, dtype=np.float64)
    T = np.array([0, 0, 0, 1, 0.1 * g, 0, 0], np.float64)
    return FrameRecord(T, np.arange(n), np.stack([np.full(n, float(g)), l, np.zeros(n)], 1),
                       np.stack([100.0 * g + l, np.full(n, 2.0)], 1), np.stack([100.0 * g + l, np.full(n, 1.0)], 1),
                       np.array(query, np.int64), np.array(train, np.int64))


def _landmarks(ep, el, meas, X):
    """[(X, [(pose, u, v) in edge order])] per landmark, in landmark order."""
    out = []
    for lm in range(len(X)):
        idx = np.nonzero(el == lm)[0]
        out.append((tuple(X[lm]), [(int(ep[k]), float(meas[k, 0]), float(meas[k, 1])) for k in idx]))
    return out


def test_three_frame_chain():
    # frame 1: records 0, 1 end on keypoints 7, 9 of L_1; frame 2: record 0 starts at 9 (child of (1, 1)) and ends on
    # 4, record 1 starts at 3 (no parent); frame 3: record 0 starts at 4 (child of (2, 0))
    recs = {0: _rec(0, [], []), 1: _rec(1, [5, 6], [7, 9]), 2: _rec(2, [9, 3], [4, 8]), 3: _rec(3, [4], [2])}
    poses, X, ep, el, meas, node_map = window_problem_tracks(recs, [0, 1, 2, 3], 1)
    assert poses.shape == (4, 7) and ep.dtype == np.int32 and el.dtype == np.int32
    # landmarks by (root pose, length, root record): (1, 1, 0), (1, 3, 1), (2, 1, 1)
    assert _landmarks(ep, el, meas, X) == [
        ((1.0, 0.0, 0.0), [(0, 100.0, 2.0), (1, 100.0, 1.0)]),
        ((1.0, 1.0, 0.0), [(0, 101.0, 2.0), (1, 101.0, 1.0), (2, 200.0, 1.0), (3, 300.0, 1.0)]),
        ((2.0, 1.0, 0.0), [(1, 201.0, 2.0), (2, 201.0, 1.0)])]
    assert list(el) == sorted(el)  # landmark-major
    assert [list(m) for m in node_map] == [[], [0, 1], [1, 2], [1]]
    # the write-back gives every node of the chain its landmark's X
    Xn = X + np.array([[10.0, 0, 0], [20.0, 0, 0], [30.0, 0, 0]])
    apply_window_tracks(recs, [0, 1, 2, 3], poses, Xn, node_map)
    np.testing.assert_array_equal(recs[1].X, Xn[[0, 1]])
    np.testing.assert_array_equal(recs[2].X, Xn[[1, 2]])
    np.testing.assert_array_equal(recs[3].X, Xn[[1]])


def test_shared_train_later_record_stays_alone():
    # records 0 and 2 of frame 1 both end on keypoint 7: the child goes to the smaller index, record 2 stays alone
    recs = {0: _rec(0, [], []), 1: _rec(1, [1, 2, 3], [7, 5, 7]), 2: _rec(2, [7], [0])}
    _, X, ep, el, meas, node_map = window_problem_tracks(recs, [0, 1, 2], 1)
    lms = _landmarks(ep, el, meas, X)
    assert [(x, len(e)) for x, e in lms] == [((1.0, 1.0, 0.0), 2), ((1.0, 2.0, 0.0), 2), ((1.0, 0.0, 0.0), 3)]
    assert lms[2][1][-1] == (2, 200.0, 1.0)
    assert [list(m) for m in node_map] == [[], [2, 0, 1], [2]]


def test_chain_cut_by_the_windows_first_frame():
    # the same chain 1 -> 2 -> 3; in the window [1, 2, 3] frame 1 is pose 0 (no nodes) and frame 2 is pose 1, whose
    # nodes are roots whatever they link to
    recs = {0: _rec(0, [], []), 1: _rec(1, [5], [7]), 2: _rec(2, [7], [4]), 3: _rec(3, [4], [2])}
    _, X, ep, el, meas, node_map = window_problem_tracks(recs, [1, 2, 3], 1)
    assert _landmarks(ep, el, meas, X) == [((2.0, 0.0, 0.0), [(0, 200.0, 2.0), (1, 200.0, 1.0), (2, 300.0, 1.0)])]
    assert [list(m) for m in node_map] == [[], [0], [0]]
    _, X4, ep4, el4, _, _ = window_problem_tracks(recs, [0, 1, 2, 3], 1)
    assert len(X4) == 1 and list(ep4) == [0, 1, 2, 3]


def test_frame_without_records_in_mid_window():
    recs = {0: _rec(0, [], []), 1: _rec(1, [5], [7]), 2: _rec(2, [], []), 3: _rec(3, [7], [1]), 4: _rec(4, [1], [6])}
    _, X, ep, el, meas, node_map = window_problem_tracks(recs, [0, 1, 2, 3, 4], 2)
    assert _landmarks(ep, el, meas, X) == [
        ((1.0, 0.0, 0.0), [(0, 100.0, 2.0), (1, 100.0, 1.0)]),
        ((3.0, 0.0, 0.0), [(2, 300.0, 2.0), (3, 300.0, 1.0), (4, 400.0, 1.0)])]
    assert [list(m) for m in node_map] == [[], [0], [], [1], [1]]
    # no records anywhere: an empty problem of the right dtypes
    empty = {g: _rec(g, [], []) for g in range(3)}
    _, X, ep, el, meas, _ = window_problem_tracks(empty, [0, 1, 2], 1)
    assert X.shape == (0, 3) and meas.shape == (0, 2) and ep.dtype == np.int32 and len(ep) == len(el) == 0


def test_no_links_is_the_two_view_graph():
    """Without a link anywhere: window_problem's landmarks, edges and measurements, up to the edge order."""
    recs = {g: _rec(g, [10 * g + l for l in range(3)], [50 + 10 * g + l for l in range(3)]) for g in range(4)}
    recs[0] = _rec(0, [], [])
    a = window_problem_tracks(recs, [0, 1, 2, 3], 2)
    b = window_problem(recs, [0, 1, 2, 3], 2)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])  # same landmarks in the same order
    ea = sorted(zip(a[3].tolist(), a[2].tolist(), map(tuple, a[4].tolist())))
    eb = sorted(zip(b[3].tolist(), b[2].tolist(), map(tuple, b[4].tolist())))
    assert ea == eb and len(ea) == 18


def test_records_without_indices_are_refused():
    recs = {g: _rec(g, [1], [2]) for g in range(3)}
    recs[2].query = recs[2].query[:0]
    with pytest.raises(ValueError):
        window_problem_tracks(recs, [0, 1, 2], 1)


def test_oracle_records_equal_the_pixel_linked_restatement(oracle, offsets):
    """The oracle front end's records for synth_sequence(71, 8): the product's index-linked assembly equals the
    helper's pixel-linked one (ep, el, meas, X, the node map), for windows at the start and in mid-sequence, and a
    solved window writes back the same X."""
    n, chunk, max_kp = 8, 4, 2000
    frames = synth_sequence(71, n, stereo=True)
    off = offsets.reshape(256, 4)
    tracks = front_end(oracle, frames, chunk, scene.K_KITTI, T_RIGHT, off, max_kp, threads=8)
    # the keypoint index of every pixel of L_k, for the match_dj the batch would hand over
    index = []
    for g in range(n):
        kl = oracle.brief(frames[g][0], oracle.fast(frames[g][0], max_kp)[0], off)
        index.append({(int(x), int(y)): j for j, (x, y) in enumerate(zip(kl["x"], kl["y"]))})
    rel = np.zeros((n, 7))
    ec = np.zeros(n, np.int32)
    eX = np.zeros((n, max_kp, 3))
    eo = np.zeros((n, max_kp), np.uint8)
    uv = np.zeros((n, max_kp, 2))
    qq = np.zeros((n, max_kp), np.int32)
    own = np.zeros((n, max_kp, 2), np.int32)
    dj = np.full((n, max_kp, 2), -1, np.int32)
    for k in range(n):
        X, u, q, T, out, o = tracks[k]
        rel[k], ec[k] = T, len(X)
        eX[k, :len(X)], eo[k, :len(X)], uv[k, :len(X)], qq[k, :len(X)], own[k] = X, out, u, q, o
        for i in q:
            dj[k, i, 1] = index[k][(int(o[i, 0]), int(o[i, 1]))]
    block = oracle.map_chunk(rel, 0, 1, ec, eX, eo, max_kp, n)
    placed, _, _ = oracle.map_place(block, 1, len(block), np.array([0, 0, 0, 1, 0, 0, 0], np.float64))
    prod = frame_records_from_block(np.ascontiguousarray(placed), uv, qq, own, dj)
    mine = records_from_block(placed, uv, qq, own)
    assert sum(len(r.edge) for r in prod.values()) > 1000
    for fr, n_fixed in ((list(range(0, 4)), 2), (list(range(2, 8)), 2), (list(range(0, 8)), 1)):
        a = window_problem_tracks(prod, fr, n_fixed)
        b = tchain.assemble_window_tracks(oracle, mine, fr, n_fixed)
        for x, y in zip(a[:5], b[:5]):
            assert x.dtype == y.dtype
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a[5], b[5]):
            np.testing.assert_array_equal(x, y)
        assert np.mean(np.bincount(a[3]) >= 3) >= 0.5  # the records do link
    P, Xo, it, log = oracle.ba_lm(a[0], 1, a[1], a[2], a[3], a[4], scene.K_KITTI, 2)
    p2 = {g: FrameRecord(r.T_wc.copy(), r.edge, r.X.copy(), r.uv_prev, r.uv_own) for g, r in prod.items()}
    m2 = {g: Rec(r.T_wc.copy(), r.edge, r.X.copy(), r.uv_prev, r.uv_own) for g, r in mine.items()}
    apply_window_tracks(p2, fr, P, Xo, a[5])
    tchain.write_back_tracks(oracle, m2, fr, P, Xo, b[5])
    for g in fr:
        np.testing.assert_array_equal(p2[g].T_wc, m2[g].T_wc)
        np.testing.assert_array_equal(p2[g].X, m2[g].X)
