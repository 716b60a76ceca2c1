"""The scene of the loop-closure tests: the 24-frame stereo sequence of tests/test_gpu_sequence_bow.py (20 frames 40
columns apart, then the first 4 places again, (1, 4) pixels off), its keypoints from the CPU oracle, the specification's
keyframe store over them and the table of verification problems -- computed once per session."""
import functools
import os

import numpy as np

from ya_vo_amd.synth import synth_frame

import loop_reference as ref

H, W, MAX_KP = 120, 320, 400
N_OUT, N_BACK, STEP = 20, 4, 40
N_FRAMES = N_OUT + N_BACK
K = np.array([[300.0, 0, 160.0], [0, 300.0, 60.0], [0, 0, 1.0]])
T_RIGHT = np.array([0, 0, 0, 1, 0, -0.54, 0], np.float64)
MATCH_THR, MIN_INLIERS = 20, 12

# (query frame, entry): the revisits against their own places, against partially overlapping places, against places
# that share nothing with them
OWN = [(20, 0), (21, 1), (22, 2), (23, 3)]
PARTIAL = [(20, 1), (20, 2), (20, 4)]
NONE = [(20, 10), (23, 15), (21, 12)]
PROBLEMS = OWN + PARTIAL + NONE


def origin(k):
    return (k, STEP * k) if k < N_OUT else (k - N_OUT + 1, STEP * (k - N_OUT) + 4)


def frame_pair(k):
    r, c = origin(k)
    return synth_frame(71, r, c, H, W), synth_frame(71, r, c + 8, H, W)


@functools.lru_cache(maxsize=None)
def frames():
    """uint8 [2 * N_FRAMES, H, W]: L_k, R_k interleaved"""
    out = np.stack([img for k in range(N_FRAMES) for img in frame_pair(k)])
    out.setflags(write=False)
    return out


def params(flags=3):
    return ref.params(MATCH_THR, flags, 4, 5, 64, 0, 2.0, MIN_INLIERS)


@functools.lru_cache(maxsize=None)
def _oracle():
    import oracle_bind
    offsets = np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                       "brief_offsets_mt19937_42.bin"), np.int8).reshape(256, 4)
    return oracle_bind.Oracle(), offsets


@functools.lru_cache(maxsize=None)
def keypoints(k):
    """(left, right) keypoint records of frame k from the oracle's FAST + BRIEF"""
    orc, offsets = _oracle()
    out = []
    for img in frame_pair(k):
        rc, _, _ = orc.fast(img, max_kp=MAX_KP)
        out.append(orc.brief(img, rc, offsets))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def store(n=N_OUT):
    """The specification's store with frames 0 .. n - 1 added in the stereo form"""
    orc, _ = _oracle()
    s = ref.Store()
    for k in range(n):
        kl, kr = keypoints(k)
        s.add_stereo(orc, kl, kr, K, T_RIGHT, k, MATCH_THR)
    return s


@functools.lru_cache(maxsize=None)
def reference(flags, sum_mode):
    """The specification's results of PROBLEMS, one problem each, under params(flags)"""
    orc, _ = _oracle()
    P, s = params(flags), store()
    return [ref.verify(orc, keypoints(f)[0], s, e, K, P, sum_mode) for f, e in PROBLEMS]
