"""CPU tests of the bag-of-binary-words keyframe index: every yv_bow_* symbol and its argument checks, which happen
before the context or the object is looked at (no GPU here), the specification's own properties
(tests/bow_reference.py), the package's host functions against it, and retrieval on the CPU oracle's descriptors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import bow

import bow_reference as ref
import bow_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = yv.YV_ERR_INVALID, yv.YV_ERR_CAPACITY


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(yv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ya_vo_amd", "csrc"), "-j8"], check=True)
    return yv.load_library()


def _p(a):
    return a.ctypes.data


def test_symbols_and_bindings(lib):
    hdr = open(os.path.join(ROOT, "include", "yavo", "yavo_bow.h")).read()
    names = ["yv_bow_create", "yv_bow_destroy", "yv_bow_reset", "yv_bow_count", "yv_bow_words", "yv_bow_vector",
             "yv_bow_add", "yv_bow_query", "yv_bow_add_batch", "yv_bow_query_batch", "yv_bow_view_get",
             "yv_bow_candidates_copy"]
    for name in names:
        assert hasattr(lib, name), name
        assert name in yv.BOW_SIGNATURES and name + "(" in hdr, name
    assert '#include "yavo_bow.h"' in open(os.path.join(ROOT, "include", "yavo", "yavo.h")).read()


def test_view_layout_matches_ctypes(tmp_path):
    fields = [f for f, _ in yv._BowView._fields_]
    src = tmp_path / "probe_bow.c"
    body = " ".join(f'printf("%zu ", offsetof(yv_bow_view, {f}));' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yavo/yavo.h"\n'
                   f'int main(void){{{body} printf("%zu\\n", sizeof(yv_bow_view)); return 0;}}\n')
    exe = tmp_path / "probe_bow"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == [getattr(yv._BowView, f).offset for f in fields] + [ctypes.sizeof(yv._BowView)]


def test_argument_checks_come_before_the_object(lib):
    """With a NULL context / object: YV_ERR_INVALID for every bad argument that needs neither, then what a missing
    object gives (YV_ERR_NODEVICE on a machine without a GPU, YV_ERR_INVALID with one)."""
    none = yv.YV_ERR_NODEVICE if lib.yv_device_count() == 0 else INVALID
    words = np.zeros((4, 32), np.uint8)
    idf = np.zeros(4, np.uint16)
    out = ctypes.c_void_p()

    def create(n_words=4, w=words, max_entries=8, max_queries=2, max_kp=16, o=ctypes.byref(out)):
        return lib.yv_bow_create(None, n_words, _p(w) if w is not None else None, _p(idf), max_entries, max_queries,
                                 max_kp, o)
    assert create() == none
    assert create(w=None) == INVALID and create(o=None) == INVALID
    for bad in (0, -1, 4097):
        assert create(n_words=bad) == INVALID
    assert create(n_words=4096, w=np.zeros((4096, 32), np.uint8)) == none
    for bad in (0, 65537):
        assert create(max_entries=bad) == INVALID
    for bad in (0, 4098):
        assert create(max_queries=bad) == INVALID
    for bad in (0, 4097):
        assert create(max_kp=bad) == INVALID
    assert create(max_entries=65536, max_queries=4097, max_kp=4096) == none
    assert lib.yv_bow_create(None, 4, _p(words), None, 8, 2, 16, ctypes.byref(out)) == none  # idf may be NULL

    lib.yv_bow_destroy(None)
    n = ctypes.c_int()
    assert lib.yv_bow_reset(None) == none
    assert lib.yv_bow_count(None, None) == INVALID and lib.yv_bow_count(None, ctypes.byref(n)) == none

    kp = np.zeros(4, yv.KEYPOINT_DTYPE)
    i32, i64, f64 = np.zeros(16, np.int32), np.zeros(16, np.int64), np.zeros(16, np.float64)
    i8 = np.zeros(4096, np.int8)
    assert lib.yv_bow_words(None, _p(kp), 4, _p(i32), _p(i32)) == none
    assert lib.yv_bow_words(None, None, 0, None, None) == none
    assert lib.yv_bow_words(None, _p(kp), -1, _p(i32), _p(i32)) == INVALID
    assert lib.yv_bow_words(None, None, 4, _p(i32), _p(i32)) == INVALID
    assert lib.yv_bow_words(None, _p(kp), 4, None, _p(i32)) == INVALID
    assert lib.yv_bow_words(None, _p(kp), 4, _p(i32), None) == INVALID

    assert lib.yv_bow_vector(None, _p(kp), 4, _p(i8), _p(i32)) == none
    assert lib.yv_bow_vector(None, None, 0, _p(i8), _p(i32)) == none
    assert lib.yv_bow_vector(None, _p(kp), -1, _p(i8), _p(i32)) == INVALID
    assert lib.yv_bow_vector(None, None, 4, _p(i8), _p(i32)) == INVALID
    assert lib.yv_bow_vector(None, _p(kp), 4, None, _p(i32)) == INVALID
    assert lib.yv_bow_vector(None, _p(kp), 4, _p(i8), None) == INVALID

    assert lib.yv_bow_add(None, _p(kp), 4, 7) == none
    assert lib.yv_bow_add(None, _p(kp), -1, 7) == INVALID and lib.yv_bow_add(None, None, 4, 7) == INVALID

    def query(k=_p(kp), n_kp=4, exclude=0, top_k=4, e=_p(i32), ef=_p(i64), sc=_p(f64), d=_p(i32), no=ctypes.byref(n)):
        return lib.yv_bow_query(None, k, n_kp, 5, exclude, top_k, e, ef, sc, d, no)
    assert query() == none and query(ef=None, d=None) == none and query(top_k=1) == none and query(top_k=16) == none
    assert query(k=None) == INVALID and query(n_kp=-1) == INVALID and query(exclude=-1) == INVALID
    assert query(top_k=0) == INVALID and query(top_k=17) == INVALID
    assert query(e=None) == INVALID and query(sc=None) == INVALID and query(no=None) == INVALID

    slots = np.zeros(2, np.int32)
    fids = np.zeros(2, np.int64)
    assert lib.yv_bow_add_batch(None, None, _p(slots), _p(fids), 2, None) == none
    assert lib.yv_bow_add_batch(None, None, None, None, 0, None) == none
    assert lib.yv_bow_add_batch(None, None, _p(slots), _p(fids), -1, None) == INVALID
    assert lib.yv_bow_add_batch(None, None, None, _p(fids), 2, None) == INVALID
    assert lib.yv_bow_add_batch(None, None, _p(slots), None, 2, None) == INVALID

    def qb(s=_p(slots), f=_p(fids), n_q=2, exclude=0, top_k=4):
        return lib.yv_bow_query_batch(None, None, s, f, n_q, exclude, top_k, None)
    assert qb() == none
    assert qb(s=None) == INVALID and qb(f=None) == INVALID and qb(n_q=-1) == INVALID and qb(exclude=-1) == INVALID
    assert qb(top_k=0) == INVALID and qb(top_k=17) == INVALID

    assert lib.yv_bow_view_get(None, None) == INVALID
    assert lib.yv_bow_view_get(None, ctypes.byref(yv._BowView())) == none
    assert lib.yv_bow_candidates_copy(None, -1, None, None, None, None, None) == INVALID
    assert lib.yv_bow_candidates_copy(None, 1, None, None, None, None, None) == none


# ---- the specification's own properties ----
def _rand_desc(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def _kp(desc):
    k = np.zeros(len(desc), yv.KEYPOINT_DTYPE)
    k["featVec"] = desc
    k["id"] = np.arange(len(desc))
    return k


def test_spec_words_are_the_matcher_with_the_vocabulary_as_train_list(oracle):
    rng = np.random.default_rng(0)
    words = _rand_desc(rng, 100)
    words[40] = words[3]  # duplicate words: the first index wins
    words[77] = words[3]
    desc = _rand_desc(rng, 300)
    desc[:20] = words[rng.integers(0, 100, 20)]  # exact hits, some on the duplicates
    desc[5] = words[77]
    w, d = ref.words_of(desc, words)
    m = oracle.match(_kp(desc), _kp(words))
    np.testing.assert_array_equal(w, m["pt2"]["id"])
    np.testing.assert_array_equal(d, m["distance"])
    assert w[5] == 3 and d[5] == 0
    np.testing.assert_array_equal(bow.assign_words(desc, words), w)


def test_spec_vector_and_score():
    rng = np.random.default_rng(1)
    words = _rand_desc(rng, 17)
    idx = ref.Index(words, rng.integers(0, 2000, 17).astype(np.uint16))
    desc = _rand_desc(rng, 200)
    v, n2 = idx.vector(desc)
    assert v.dtype == np.int8 and v.max() == 127 and v.min() >= 0 and n2 == int((v.astype(np.int64) ** 2).sum())
    assert ref.score(n2, n2, n2) == 1.0  # a vector against itself
    idx.add(desc, 10)
    cands, row, _, _ = idx.query(desc, 10, 0, 4)
    assert cands == [(0, 1.0, n2)] and row[0] == n2
    # no descriptors, and an all-zero idf: the zero vector, norm 0, score 0.0, no candidate
    v0, n0 = idx.vector(np.zeros((0, 32), np.uint8))
    assert not v0.any() and n0 == 0 and ref.score(0, 0, n2) == 0.0
    zero = ref.Index(words, np.zeros(17, np.uint16))
    zero.add(desc, 0)
    assert zero.norm2 == [0] and zero.query(desc, 5, 0, 4)[0] == []


def test_spec_exclusion_and_tie_order():
    rng = np.random.default_rng(2)
    idx = ref.Index(_rand_desc(rng, 64))
    imgs = [_rand_desc(rng, 150) for _ in range(4)]
    for f, i in enumerate([0, 1, 0, 2, 0]):  # entries 0, 2, 4 are the same image
        idx.add(imgs[i], 10 * f)
    c = idx.query(imgs[0], 100, 0, 16)[0]
    assert [e for e, _, _ in c[:3]] == [0, 2, 4] and all(s == 1.0 for _, s, _ in c[:3])  # equal scores: index order
    assert len(c) <= 5 and all(c[k][1] >= c[k + 1][1] for k in range(len(c) - 1))
    assert len(idx.query(imgs[0], 100, 0, 2)[0]) == 2
    # |f - frame_id| >= x: at x = 61 only the entries of frames 0, 10, 20, 30 are left; x = 0 excludes nothing
    assert [e for e, _, _ in idx.query(imgs[0], 100, 61, 16)[0]][:2] == [0, 2]
    assert 4 not in [e for e, _, _ in idx.query(imgs[0], 100, 61, 16)[0]]
    assert idx.query(imgs[0], 40, 0, 1)[0][0][0] == 0 and idx.query(imgs[0], 0, 1, 1)[0][0][0] == 2
    assert idx.query(imgs[0], 100, 101, 16)[0] == []


def test_package_training_equals_the_specification(tmp_path):
    rng = np.random.default_rng(3)
    desc = _rand_desc(rng, 500)
    desc[250:] = desc[:250] ^ (rng.integers(0, 256, (250, 32)) & rng.integers(0, 256, (250, 32))
                               & rng.integers(0, 256, (250, 32))).astype(np.uint8)  # clusters
    for iters in (0, 2):
        np.testing.assert_array_equal(bow.train_vocabulary(desc, 20, iters, 5), ref.train_vocabulary(desc, 20, iters, 5))
    words = ref.train_vocabulary(desc, 20, 1, 5)
    lists = [ref.words_of(desc[i:i + 50], words)[0] for i in range(0, 500, 50)]
    lists.append(np.zeros(0, np.int32))
    idf = ref.idf_table(lists, 21)  # word 20 is never seen: weight 0
    np.testing.assert_array_equal(bow.idf_table(lists, 21), idf)
    assert idf[20] == 0 and idf.dtype == np.uint16
    df3 = sum(1 for wl in lists if 3 in wl)
    assert idf[3] == int(np.floor(256 * np.log(len(lists) / df3) + 0.5))
    bow.save_vocabulary(str(tmp_path / "v.npz"), words, idf[:20])
    w2, i2 = bow.load_vocabulary(str(tmp_path / "v.npz"))
    np.testing.assert_array_equal(w2, words)
    np.testing.assert_array_equal(i2, idf[:20])


def test_retrieval_on_the_cpu_oracle():
    """16 places, 16 revisits (another frame index, 7 pixels further): every revisit ranks its own place first, with
    its score at least 0.2 above the best other place (256 words, iters = 0)."""
    places, revisits, words, idf = bow_scenes.scene(256, 0)
    assert all(300 <= len(p) <= 400 for p in places + revisits)
    idx = ref.Index(words, idf)
    for i, p in enumerate(places):
        idx.add(p["featVec"], i)
    margins = []
    for i, r in enumerate(revisits):
        c = idx.query(r["featVec"], 100 + i, 0, 16)[0]
        assert c[0][0] == i, (i, c[:3])
        margins.append(c[0][1] - max([s for e, s, _ in c if e != i], default=0.0))
    print("smallest margin", min(margins))
    assert min(margins) > 0.2
