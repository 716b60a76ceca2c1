"""CPU restatement of the sequence front end's multi-view BA window over the oracle -- test infrastructure only.

tests/sequence_chain.py's loop (front_end, records_from_block, the oracle's map block, placement and or_ba_lm) with
the window assembled by the multi-view rule of ya_vo_amd/sequence.py window_problem_tracks, restated by another road:
records are linked by PIXEL, not by keypoint index. The parent of a record of frame k is the first record of frame
k - 1 whose uv_own (the keypoint of L_{k-1} its temporal match ended on) equals this record's uv_prev (the keypoint of
L_{k-1} its own match started from) exactly; keypoints of one image sit on distinct pixels, so this is the relation
train[k-1][l'] == query[k][l] of the product, reached without the indices. Nothing here is imported from the
product.

The rule: nodes are the records of window poses 1 .. P-1; nodes of pose 1 are roots (chains are cut at the window's
start); a chain rooted at pose a with m nodes is one landmark observed by poses a-1 (root's uv_prev), a (root's
uv_own), a+1 (child's uv_own), ...; its X is the root's; landmarks ascend by (a, m, root's record index), edges are
landmark-major; every node of a chain takes the landmark's refined X.
"""
import numpy as np

from sequence_chain import IDENTITY, records_from_block


def link_by_pixel(prev_rec, rec):
    """-> parent [n]: for every record of `rec`, the first record of prev_rec whose uv_own is its uv_prev, or -1."""
    first = {}
    for l, px in enumerate(prev_rec.uv_own):
        first.setdefault((float(px[0]), float(px[1])), l)
    return np.array([first.get((float(p[0]), float(p[1])), -1) for p in rec.uv_prev], np.int64).reshape(-1)


def assemble_window_tracks(orc, records, frames, n_fixed):
    """-> (poses, X, ep, el, meas, node_lm) with node_lm[i][l] = the landmark of record l of pose i."""
    P = len(frames)
    poses = np.array([orc.se3_inverse(records[g].T_wc) for g in frames]).reshape(P, 7)
    # root (pose, record) of every node, walking up frame by frame
    root = [[] for _ in range(P)]
    members = {}
    for i in range(1, P):
        r = records[frames[i]]
        par = link_by_pixel(records[frames[i - 1]], r) if i >= 2 else np.full(len(r.edge), -1, np.int64)
        for l in range(len(r.edge)):
            key = (i, l) if par[l] < 0 else root[i - 1][par[l]]
            root[i].append(key)
            members.setdefault(key, []).append((i, l))
    keys = sorted(members, key=lambda k: (k[0], len(members[k]), k[1]))
    X, ep, el, meas = [], [], [], []
    lm_of = {}
    for lm, (a, l0) in enumerate(keys):
        lm_of[(a, l0)] = lm
        X.append(records[frames[a]].X[l0])
        ep.append(a - 1)
        el.append(lm)
        meas.append(records[frames[a]].uv_prev[l0])
        for i, l in members[(a, l0)]:
            ep.append(i)
            el.append(lm)
            meas.append(records[frames[i]].uv_own[l])
    node_lm = [np.array([lm_of[k] for k in root[i]], np.int64) for i in range(P)]
    return (poses, np.array(X, np.float64).reshape(-1, 3), np.array(ep, np.int32), np.array(el, np.int32),
            np.array(meas, np.float64).reshape(-1, 2), node_lm)


def write_back_tracks(orc, records, frames, poses, X, node_lm):
    for i, g in enumerate(frames):
        records[g].T_wc = orc.se3_inverse(poses[i])
        if len(node_lm[i]):
            records[g].X = X[node_lm[i]].copy()


def sequence_tracks_from_tracks(orc, tracks, chunk, K, n_fixed=2, ba_iters=10, max_kp=2000, ba_mode=0):
    """sequence_chain.sequence_from_tracks with multi-view windows. -> (trajectory, records, ba_log, edges per
    landmark of every window, concatenated)."""
    n_frames = len(tracks)
    records, ba_log, obs = {}, [], []
    base = IDENTITY.copy()
    window = chunk + n_fixed
    for c in range(n_frames // chunk):
        first = c * chunk
        rel = np.zeros((chunk, 7))
        ec = np.zeros(chunk, np.int32)
        eX = np.zeros((chunk, max_kp, 3))
        eo = np.zeros((chunk, max_kp), np.uint8)
        uv = np.zeros((chunk, max_kp, 2))
        qq = np.zeros((chunk, max_kp), np.int32)
        own = np.zeros((chunk, max_kp, 2), np.int32)
        for k in range(chunk):
            X, u, q, T, out, o = tracks[first + k]
            rel[k] = T
            ec[k] = len(X)
            eX[k, :len(X)] = X
            eo[k, :len(X)] = out
            uv[k, :len(X)] = u
            qq[k, :len(X)] = q
            own[k] = o
        block = orc.map_chunk(rel, first, 1, ec, eX, eo, max_kp, chunk)
        placed, base, _ = orc.map_place(block, 1, len(block), base)
        records.update(records_from_block(placed, uv, qq, own))
        last = first + chunk - 1
        fr = list(range(max(0, last - window + 1), last + 1))
        poses, Xw, ep, el, meas, node_lm = assemble_window_tracks(orc, records, fr, n_fixed)
        if len(ep):
            obs.append(np.bincount(el, minlength=len(Xw)))
            P, Xo, it, log = orc.ba_lm(poses, n_fixed, Xw, ep, el, meas, K, ba_iters, mode=ba_mode)
            write_back_tracks(orc, records, fr, P, Xo, node_lm)
            ba_log.append((last, it, float(log[0]), float(log[-1])))
            base = records[last].T_wc.copy()
    traj = np.stack([records[g].T_wc for g in sorted(records)])
    return traj, records, ba_log, (np.concatenate(obs) if obs else np.zeros(0, np.int64))
