"""The specification of the bag-of-binary-words keyframe index (yv_bow_*, ya_vo_amd/csrc/yavo_bow.hip,
ya_vo_amd/bow.py), in numpy, scalar where the order matters.  Everything is integer arithmetic except the score, which
is one correctly rounded IEEE double sqrt and one division: the device's results are compared with these bit for bit.

  vocabulary   W words of 256 bits (1 <= W <= 4096), words[W][32] in featVec's byte / bit order, idf_q8[W] uint16
               (None: every word weighs 256)
  word         (d, w) of a descriptor = the lexicographic minimum of (Hamming(desc, words[w]), w) over w
  vector       c_w = descriptors of the image with word w, t_w = c_w * idf_q8[w], tmax = max t_w,
               v_w = (127 * t_w) // tmax as int8 (all zero for tmax == 0), norm2 = sum v_w^2
  score        dot = sum vq_w * ve_w (int32); score = dot / sqrt(nq2 * ne2) in doubles, 0.0 when a norm is 0
  candidates   entries with |f - frame_id_e| >= x and dot > 0, by (score descending, entry index ascending), the
               first top_k
"""
import numpy as np

MAX_WORDS = 4096
MAX_TOP_K = 16


def _desc(a) -> np.ndarray:
    a = np.ascontiguousarray(a, np.uint8)
    return a.reshape(-1, 32)


def hamming(desc, words) -> np.ndarray:
    """[n][W] Hamming distances of n descriptors and W words ([.][32] uint8 each): popcount(a) + popcount(b) -
    2 popcount(a & b), the last as a product of the 0 / 1 bit matrices (integers below 2^24: exact in float32)."""
    a = np.unpackbits(_desc(desc), axis=1).astype(np.float32)
    b = np.unpackbits(_desc(words), axis=1).astype(np.float32)
    return (a.sum(axis=1)[:, None] + b.sum(axis=1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)


def words_of(desc, words):
    """-> (word [n] int32, dist [n] int32): the first word at minimum distance."""
    d = _desc(desc)
    if len(d) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    h = hamming(d, words)
    w = np.argmin(h, axis=1).astype(np.int32)  # numpy's argmin returns the first minimum
    return w, h[np.arange(len(d)), w].astype(np.int32)


def bow_vector(word, n_words, idf_q8=None):
    """-> (v [n_words] int8, norm2 int): the quantised tf-idf vector of an image whose descriptors have `word`."""
    c = np.bincount(np.asarray(word, np.int64), minlength=n_words).astype(np.int64)
    idf = np.full(n_words, 256, np.int64) if idf_q8 is None else np.asarray(idf_q8, np.uint16).astype(np.int64)
    t = c * idf
    tmax = int(t.max()) if n_words else 0
    if tmax == 0:
        return np.zeros(n_words, np.int8), 0
    v = (127 * t) // tmax
    return v.astype(np.int8), int((v * v).sum())


def score(dot, nq2, ne2) -> float:
    if nq2 == 0 or ne2 == 0:
        return 0.0
    return float(np.float64(dot) / np.sqrt(np.float64(nq2) * np.float64(ne2)))


def dots(vq, ve) -> np.ndarray:
    """[Q][E] int32 dot products of the rows of vq [Q][W] and ve [E][W]."""
    return (np.asarray(vq, np.int64).reshape(len(vq), -1) @ np.asarray(ve, np.int64).reshape(len(ve), -1).T).astype(
        np.int32)


def candidates(dot_row, nq2, ne2, entry_frames, frame_id, exclude, top_k):
    """One query's candidate list -> [(entry, score, dot)], at most top_k, in rank order.  dot_row [E], ne2 [E],
    entry_frames [E] of the E entries in insertion order."""
    assert exclude >= 0 and 1 <= top_k <= MAX_TOP_K
    out = []
    for e in range(len(dot_row)):
        if abs(int(frame_id) - int(entry_frames[e])) < exclude or int(dot_row[e]) <= 0:
            continue
        out.append((e, score(int(dot_row[e]), int(nq2), int(ne2[e])), int(dot_row[e])))
    out.sort(key=lambda c: (-c[1], c[0]))
    return out[:top_k]


class Index:
    """The index as the specification sees it: vectors, norms and frame ids in insertion order."""

    def __init__(self, words, idf_q8=None):
        self.words = _desc(words).copy()
        self.n_words = len(self.words)
        assert 1 <= self.n_words <= MAX_WORDS
        self.idf = None if idf_q8 is None else np.asarray(idf_q8, np.uint16).copy()
        self.vectors, self.norm2, self.frames = [], [], []

    def vector(self, desc):
        w, _ = words_of(desc, self.words)
        return bow_vector(w, self.n_words, self.idf)

    def add(self, desc, frame_id):
        v, n2 = self.vector(desc)
        self.vectors.append(v)
        self.norm2.append(n2)
        self.frames.append(int(frame_id))

    def reset(self):
        self.vectors, self.norm2, self.frames = [], [], []

    def query(self, desc, frame_id, exclude, top_k):
        """-> (candidates, dot row [E] int32, v, norm2)"""
        v, n2 = self.vector(desc)
        E = len(self.vectors)
        row = dots(v[None, :], np.stack(self.vectors))[0] if E else np.zeros(0, np.int32)
        return candidates(row, n2, self.norm2, self.frames, frame_id, exclude, top_k), row, v, n2


def train_vocabulary(desc, n_words, iters, seed):
    """k-majority over binary descriptors -> words [n_words][32] uint8.  The initial words are the rows
    sort(default_rng(seed).permutation(len(desc))[:n_words]); each round assigns every descriptor to its word (above)
    and sets bit b of a word iff 2 * ones_b > count; a word without descriptors keeps its bits."""
    d = _desc(desc)
    assert 1 <= n_words <= min(MAX_WORDS, len(d)) and iters >= 0
    rows = np.sort(np.random.default_rng(seed).permutation(len(d))[:n_words])
    words = d[rows].copy()
    bits = np.unpackbits(d, axis=1, bitorder="little").astype(np.int64)  # [n][256], bit b of byte b >> 3
    for _ in range(iters):
        w, _ = words_of(d, words)
        for k in range(n_words):
            mine = bits[w == k]
            if len(mine) == 0:
                continue
            ones = mine.sum(axis=0)
            words[k] = np.packbits((2 * ones > len(mine)).astype(np.uint8), bitorder="little")
    return words


def idf_table(word_lists, n_words):
    """idf_q8 [n_words] uint16 over N images' word lists: floor(256 * ln(N / df_w) + 0.5), 0 where df_w == 0, clipped
    to 65535 (host only: the device never evaluates a logarithm)."""
    N = len(word_lists)
    df = np.zeros(n_words, np.int64)
    for wl in word_lists:
        df[np.unique(np.asarray(wl, np.int64))] += 1
    out = np.zeros(n_words, np.uint16)
    for w in range(n_words):
        if df[w] > 0:
            out[w] = min(65535, int(np.floor(256.0 * np.log(N / df[w]) + 0.5)))
    return out
