"""Loop closure: the keyframe store and the geometric verification of place-recognition candidates
(include/yavo/yavo_loop.h, csrc/yavo_loop.hip).

A LoopVerifier keeps every keyframe's descriptors, positions and stereo landmarks on the device and turns a candidate
(query keypoints, stored keyframe) into a relative pose with inlier counts: the 2-NN match filter against the keyframe's
descriptors, P3P-RANSAC over the matches that hit a landmark, then the pose LM from the RANSAC pose.  Entry e of the
store is entry e of a ya_vo_amd.bow.BowIndex that was given the same images in the same order, so the candidate rows of
a BowIndex query feed verify_batch as they lie on the device.  Every result equals the specification
(tests/loop_reference.py) bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import List

import numpy as np

from . import KEYPOINT_DTYPE, LOOP_RESULT_DTYPE, _LoopView, _check, _ptr, load_library, ransac_draws

MAX_PROBLEMS = 4096
CAND_STRIDE = 16


def lm_sum_mode(n_problems: int) -> int:
    """The oracle's sum_mode of the LM of a verify call over n_problems problems (yv_loop_lm_sum_mode)."""
    return int(load_library().yv_loop_lm_sum_mode(int(n_problems)))


def _opt(p: int):
    return ctypes.c_void_p(p) if p else None


class LoopVerifier:
    """One yv_loop: the keyframe store and the verification workspace."""

    _close_rank = 1  # before the batches and the context

    def __init__(self, ctx, K, T_right, max_entries: int = 4096, max_problems: int = 64, max_kp: int = 2000):
        self.ctx, self.lib = ctx, ctx.lib
        k = np.ascontiguousarray(K, np.float64).reshape(9)
        t = np.ascontiguousarray(T_right, np.float64).reshape(7)
        h = ctypes.c_void_p()
        _check(self.lib.yv_loop_create(ctx.handle, _ptr(k), _ptr(t), int(max_entries), int(max_problems), int(max_kp),
                                       ctypes.byref(h)), "yv_loop_create")
        self.handle = h
        self.max_entries, self.max_problems, self.max_kp = max_entries, max_problems, max_kp
        self.entry_frames: List[int] = []  # frame id of every entry, in insertion order
        self.min_inliers = 0
        ctx._own(self)

    def close(self) -> None:
        if self.handle:
            self.lib.yv_loop_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = ctypes.c_int()
        _check(self.lib.yv_loop_count(self.handle, ctypes.byref(n)), "yv_loop_count")
        return n.value

    def reset(self) -> None:
        """Empties the store; the parameters stay."""
        _check(self.lib.yv_loop_reset(self.handle), "yv_loop_reset")
        self.entry_frames = []

    def set_params(self, match_thr: int = 20, flags: int = 3, ratio_num: int = 4, ratio_den: int = 5, iters: int = 64,
                   thr_px: float = 2.0, min_inliers: int = 12, seed: int = 0, draws=None) -> None:
        """draws: uint32 [iters][3]; None: ransac_draws(iters, seed)."""
        d = ransac_draws(iters, seed) if draws is None else np.ascontiguousarray(draws, np.uint32).reshape(-1, 3)
        if len(d) != iters:
            raise ValueError("draws must be [iters][3]")
        _check(self.lib.yv_loop_set_params(self.handle, int(match_thr), int(flags), int(ratio_num), int(ratio_den),
                                           int(iters), _ptr(d), float(thr_px), int(min_inliers)), "yv_loop_set_params")
        self.min_inliers = int(min_inliers)

    # ---- host forms ----
    def add(self, kp, X=None, has=None, frame_id: int = 0) -> int:
        """Appends a keyframe (keypoint records, landmarks X [n][3] with flags has [n]; both None: none) -> its entry."""
        k = np.ascontiguousarray(kp, KEYPOINT_DTYPE)
        if (X is None) != (has is None):
            raise ValueError("X and has come together")
        x = h = None
        if X is not None:
            x = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
            h = np.ascontiguousarray(has, np.uint8).reshape(-1)
            if len(x) != len(k) or len(h) != len(k):
                raise ValueError("X / has and the keypoints differ in length")
            if len(k) == 0:
                x, h = np.zeros((1, 3)), np.zeros(1, np.uint8)
        _check(self.lib.yv_loop_add(self.handle, _ptr(k) if len(k) else None, len(k), _ptr(x) if x is not None else None,
                                    _ptr(h) if h is not None else None, int(frame_id)), "yv_loop_add")
        self.entry_frames.append(int(frame_id))
        return len(self.entry_frames) - 1

    def verify(self, q, entries) -> np.ndarray:
        """The query keypoint records against every entry of `entries` -> LOOP_RESULT_DTYPE [len(entries)]."""
        k = np.ascontiguousarray(q, KEYPOINT_DTYPE)
        e = np.ascontiguousarray(entries, np.int32).reshape(-1)
        out = np.zeros(max(len(e), 1), LOOP_RESULT_DTYPE)
        _check(self.lib.yv_loop_verify(self.handle, _ptr(k) if len(k) else None, len(k), _ptr(e) if len(e) else None,
                                       len(e), _ptr(out)), "yv_loop_verify")
        return out[:len(e)]

    # ---- batch forms (asynchronous on `stream`, 0: the context's) ----
    def add_batch(self, batch, left_slots, stereo_pairs, frame_ids, stream: int = 0) -> None:
        s = np.ascontiguousarray(left_slots, np.int32).reshape(-1)
        p = np.ascontiguousarray(stereo_pairs, np.int32).reshape(-1)
        f = np.ascontiguousarray(frame_ids, np.int64).reshape(-1)
        if not len(s) == len(p) == len(f):
            raise ValueError("left_slots, stereo_pairs and frame_ids differ in length")
        n = len(s)
        _check(self.lib.yv_loop_add_batch(self.handle, batch.handle, _ptr(s) if n else None, _ptr(p) if n else None,
                                          _ptr(f) if n else None, n, _opt(stream)), "yv_loop_add_batch")
        self.entry_frames.extend(int(x) for x in f)

    def verify_batch(self, batch, slots, d_cand_entry: int, d_cand_count: int, top_k: int, stream: int = 0) -> None:
        """Query q = slot slots[q] against the first top_k candidates of row q of the device arrays d_cand_entry
        ([nq][16] int32) / d_cand_count ([nq] int32), as BowIndex.candidates_copy writes them."""
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        _check(self.lib.yv_loop_verify_batch(self.handle, batch.handle, _ptr(s) if len(s) else None, len(s),
                                             _opt(d_cand_entry), _opt(d_cand_count), int(top_k), _opt(stream)),
               "yv_loop_verify_batch")

    def results_copy(self, n: int, d_results: int, stream: int = 0) -> None:
        """The last verify call's results 0..n-1 into a device array of the caller's (yv_loop_results_copy)."""
        _check(self.lib.yv_loop_results_copy(self.handle, int(n), _opt(d_results), _opt(stream)),
               "yv_loop_results_copy")

    def view(self) -> _LoopView:
        v = _LoopView()
        _check(self.lib.yv_loop_view_get(self.handle, ctypes.byref(v)), "yv_loop_view_get")
        return v

    def results(self) -> np.ndarray:
        """The last verify call's results read back (synchronises the context's stream)."""
        v = self.view()
        if v.n_problems == 0:
            return np.zeros(0, LOOP_RESULT_DTYPE)
        return self.ctx.download(v.results, LOOP_RESULT_DTYPE, v.n_problems)
