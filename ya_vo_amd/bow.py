"""Place recognition: the bag-of-binary-words keyframe index (include/yavo/yavo_bow.h, csrc/yavo_bow.hip).

A vocabulary is W <= 4096 words of 256 bits with integer idf weights, both made on the host (train_vocabulary,
idf_table) and handed to the device once; BowIndex assigns an image's BRIEF descriptors to their nearest words, builds
its quantised tf-idf vector, scores it against every stored keyframe (an int8 GEMM) and returns the best candidates,
on host keypoint lists or on the slots of a Batch in HBM.  Everything is integer arithmetic plus one correctly rounded
double sqrt and division: the results equal the numpy specification (tests/bow_reference.py) bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import List, Tuple

import numpy as np

from . import KEYPOINT_DTYPE, _BowView, _check, _ptr

MAX_WORDS = 4096
MAX_TOP_K = 16

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _desc(a) -> np.ndarray:
    """descriptors [n][32] uint8 from a keypoint record array or a byte array"""
    a = np.asarray(a)
    if a.dtype == KEYPOINT_DTYPE:
        a = a["featVec"]
    return np.ascontiguousarray(a, np.uint8).reshape(-1, 32)


def _keypoints(a) -> np.ndarray:
    """keypoint records from a record array, or from descriptors [n][32] (positions zero)"""
    a = np.asarray(a)
    if a.dtype == KEYPOINT_DTYPE:
        return np.ascontiguousarray(a)
    d = _desc(a)
    k = np.zeros(len(d), KEYPOINT_DTYPE)
    k["featVec"] = d
    k["id"] = np.arange(len(d))
    return k


def assign_words(desc, words) -> np.ndarray:
    """The word of every descriptor on the host: the first word at minimum Hamming distance -> [n] int32."""
    d, w = _desc(desc), _desc(words)
    out = np.zeros(len(d), np.int32)
    step = max(1, (1 << 22) // max(len(w), 1))  # ~128 MB of xor bytes at a time
    for i in range(0, len(d), step):
        h = _POP8[d[i:i + step, None, :] ^ w[None, :, :]].sum(axis=2)
        out[i:i + step] = np.argmin(h, axis=1)
    return out


def _majority_step(desc_bits: np.ndarray, word_of: np.ndarray, words: np.ndarray) -> np.ndarray:
    """bit b of word k becomes 1 iff 2 * ones_b > count over its descriptors; an empty word keeps its bits"""
    n_words = len(words)
    count = np.bincount(word_of, minlength=n_words).astype(np.int64)
    ones = np.zeros((n_words, 256), np.int64)
    np.add.at(ones, word_of, desc_bits)
    new = np.packbits((2 * ones > count[:, None]).astype(np.uint8), axis=1, bitorder="little")
    out = words.copy()
    out[count > 0] = new[count > 0]
    return out


def train_vocabulary(desc, n_words: int, iters: int, seed: int, assign=None) -> np.ndarray:
    """k-majority over binary descriptors -> words [n_words][32] uint8.  The initial words are the rows
    sort(default_rng(seed).permutation(len(desc))[:n_words]); then `iters` rounds: every descriptor goes to its word
    (first index on ties), bit b of a word becomes 1 iff 2 * ones_b > count, a word without descriptors keeps its bits.
    assign(desc, words) -> [n] words replaces the host assignment (BowIndex.train passes the device's)."""
    d = _desc(desc)
    if not 1 <= n_words <= min(MAX_WORDS, len(d)) or iters < 0:
        raise ValueError("n_words outside 1..min(4096, len(desc)) or iters < 0")
    rows = np.sort(np.random.default_rng(seed).permutation(len(d))[:n_words])
    words = d[rows].copy()
    bits = np.unpackbits(d, axis=1, bitorder="little").astype(np.int64)
    for _ in range(iters):
        w = np.asarray((assign or assign_words)(d, words), np.int64)
        words = _majority_step(bits, w, words)
    return words


def idf_table(word_lists, n_words: int) -> np.ndarray:
    """idf_q8 [n_words] uint16 over N images' word lists: floor(256 * ln(N / df_w) + 0.5), 0 where df_w == 0, clipped
    to 65535."""
    N = len(word_lists)
    df = np.zeros(n_words, np.int64)
    for wl in word_lists:
        df[np.unique(np.asarray(wl, np.int64))] += 1
    out = np.zeros(n_words, np.float64)
    seen = df > 0
    out[seen] = np.floor(256.0 * np.log(N / df[seen]) + 0.5)
    return np.clip(out, 0, 65535).astype(np.uint16)


def save_vocabulary(path: str, words, idf_q8=None) -> None:
    w = _desc(words)
    idf = np.full(len(w), 256, np.uint16) if idf_q8 is None else np.asarray(idf_q8, np.uint16)
    if len(idf) != len(w):
        raise ValueError("words and idf_q8 differ in length")
    np.savez(path, words=w, idf_q8=idf)


def load_vocabulary(path: str) -> Tuple[np.ndarray, np.ndarray]:
    with np.load(path) as z:
        return _desc(z["words"]).copy(), np.asarray(z["idf_q8"], np.uint16).copy()


class BowIndex:
    """One yv_bow: a vocabulary on the device and the keyframe index over it."""

    _close_rank = 1  # before the batches and the context

    def __init__(self, ctx, words, idf_q8=None, max_entries: int = 4096, max_queries: int = 64, max_kp: int = 2000):
        self.ctx, self.lib = ctx, ctx.lib
        w = _desc(words)
        idf = None if idf_q8 is None else np.ascontiguousarray(idf_q8, np.uint16).reshape(-1)
        if idf is not None and len(idf) != len(w):
            raise ValueError("words and idf_q8 differ in length")
        h = ctypes.c_void_p()
        _check(self.lib.yv_bow_create(ctx.handle, len(w), _ptr(w), _ptr(idf) if idf is not None else None,
                                      int(max_entries), int(max_queries), int(max_kp), ctypes.byref(h)),
               "yv_bow_create")
        self.handle = h
        self.n_words, self.max_entries, self.max_queries, self.max_kp = len(w), max_entries, max_queries, max_kp
        self.entry_frames: List[int] = []  # frame id of every entry, in insertion order
        self._last_frames: List[int] = []  # the last query call's frame ids
        ctx._own(self)

    @classmethod
    def train(cls, ctx, desc, n_words: int, iters: int, seed: int, max_kp: int = 4096) -> np.ndarray:
        """train_vocabulary with the assignment step on the device (yv_bow_words over the current words); the
        majority step is numpy.  Equals train_vocabulary(desc, n_words, iters, seed) bit for bit."""
        def assign(d, words):
            idx = cls(ctx, words, None, 1, 1, max_kp)
            try:
                out = np.zeros(len(d), np.int32)
                for i in range(0, len(d), max_kp):
                    out[i:i + max_kp] = idx.words(d[i:i + max_kp])[0]
                return out
            finally:
                idx.close()
        return train_vocabulary(desc, n_words, iters, seed, assign=assign)

    def close(self) -> None:
        if self.handle:
            self.lib.yv_bow_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = ctypes.c_int()
        _check(self.lib.yv_bow_count(self.handle, ctypes.byref(n)), "yv_bow_count")
        return n.value

    def reset(self) -> None:
        _check(self.lib.yv_bow_reset(self.handle), "yv_bow_reset")
        self.entry_frames = []

    # ---- host forms ----
    def words(self, kp) -> Tuple[np.ndarray, np.ndarray]:
        """-> (word [n] int32, dist [n] int32) of a keypoint record array or descriptors [n][32]."""
        k = _keypoints(kp)
        word, dist = np.zeros(max(len(k), 1), np.int32), np.zeros(max(len(k), 1), np.int32)
        _check(self.lib.yv_bow_words(self.handle, _ptr(k) if len(k) else None, len(k), _ptr(word), _ptr(dist)),
               "yv_bow_words")
        return word[:len(k)], dist[:len(k)]

    def vector(self, kp) -> Tuple[np.ndarray, int]:
        """-> (v [n_words] int8, norm2)"""
        k = _keypoints(kp)
        v, n2 = np.zeros(self.n_words, np.int8), ctypes.c_int32()
        _check(self.lib.yv_bow_vector(self.handle, _ptr(k) if len(k) else None, len(k), _ptr(v), ctypes.byref(n2)),
               "yv_bow_vector")
        return v, n2.value

    def add(self, kp, frame_id: int) -> int:
        """Appends the image -> its entry index."""
        k = _keypoints(kp)
        _check(self.lib.yv_bow_add(self.handle, _ptr(k) if len(k) else None, len(k), int(frame_id)), "yv_bow_add")
        self.entry_frames.append(int(frame_id))
        return len(self.entry_frames) - 1

    def query(self, kp, frame_id: int, exclude: int = 0, top_k: int = 4):
        """-> [(entry, entry_frame, score, dot)] in rank order."""
        k = _keypoints(kp)
        e, ef = np.zeros(MAX_TOP_K, np.int32), np.zeros(MAX_TOP_K, np.int64)
        sc, dot, n = np.zeros(MAX_TOP_K, np.float64), np.zeros(MAX_TOP_K, np.int32), ctypes.c_int()
        _check(self.lib.yv_bow_query(self.handle, _ptr(k) if len(k) else None, len(k), int(frame_id), int(exclude),
                                     int(top_k), _ptr(e), _ptr(ef), _ptr(sc), _ptr(dot), ctypes.byref(n)),
               "yv_bow_query")
        self._last_frames = [int(frame_id)]
        return [(int(e[i]), int(ef[i]), float(sc[i]), int(dot[i])) for i in range(n.value)]

    # ---- batch forms (asynchronous on `stream`, 0: the context's) ----
    def add_batch(self, batch, slots, frame_ids, stream: int = 0) -> None:
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        f = np.ascontiguousarray(frame_ids, np.int64).reshape(-1)
        if len(s) != len(f):
            raise ValueError("slots and frame_ids differ in length")
        _check(self.lib.yv_bow_add_batch(self.handle, batch.handle, _ptr(s) if len(s) else None,
                                         _ptr(f) if len(f) else None, len(s),
                                         ctypes.c_void_p(stream) if stream else None), "yv_bow_add_batch")
        self.entry_frames.extend(int(x) for x in f)

    def query_batch(self, batch, slots, frame_ids, exclude: int = 0, top_k: int = 4, stream: int = 0) -> None:
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        f = np.ascontiguousarray(frame_ids, np.int64).reshape(-1)
        if len(s) != len(f):
            raise ValueError("slots and frame_ids differ in length")
        _check(self.lib.yv_bow_query_batch(self.handle, batch.handle, _ptr(s) if len(s) else None,
                                           _ptr(f) if len(f) else None, len(s), int(exclude), int(top_k),
                                           ctypes.c_void_p(stream) if stream else None), "yv_bow_query_batch")
        self._last_frames = [int(x) for x in f]

    def candidates_copy(self, n: int, d_entry: int = 0, d_score: int = 0, d_dot: int = 0, d_count: int = 0,
                        stream: int = 0) -> None:
        """The last query call's candidate rows 0..n-1 into device arrays of the caller's (yv_bow_candidates_copy)."""
        p = [ctypes.c_void_p(x) if x else None for x in (d_entry, d_score, d_dot, d_count, stream)]
        _check(self.lib.yv_bow_candidates_copy(self.handle, int(n), *p), "yv_bow_candidates_copy")

    def view(self) -> _BowView:
        v = _BowView()
        _check(self.lib.yv_bow_view_get(self.handle, ctypes.byref(v)), "yv_bow_view_get")
        return v

    def candidates(self):
        """The last query call's lists read back (synchronises the context's stream): per query
        [(entry, entry_frame, score, dot)] in rank order."""
        v = self.view()
        n = v.n_queries
        if n == 0:
            return []
        ctx = self.ctx
        cnt = ctx.download(v.cand_count, np.int32, n)
        e = ctx.download(v.cand_entry, np.int32, n * MAX_TOP_K).reshape(n, MAX_TOP_K)
        sc = ctx.download(v.cand_score, np.float64, n * MAX_TOP_K).reshape(n, MAX_TOP_K)
        dot = ctx.download(v.cand_dot, np.int32, n * MAX_TOP_K).reshape(n, MAX_TOP_K)
        return [[(int(e[q, k]), self.entry_frames[e[q, k]], float(sc[q, k]), int(dot[q, k]))
                 for k in range(int(cnt[q]))] for q in range(n)]
