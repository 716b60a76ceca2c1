"""The retrieval scene of the bag-of-words tests: 16 places, 16 revisits a few pixels off, and a 256-word vocabulary
trained on other images, all from the CPU oracle (computed once per session)."""
import functools
import os

import numpy as np

from ya_vo_amd.synth import synth_frame

import bow_reference as ref

H, W, MAX_KP = 120, 320, 400
N_PLACES = 16


def place_image(i):
    return synth_frame(1, 0, 400 * i, H, W)


def revisit_image(i):
    return synth_frame(1, 3, 400 * i + 7, H, W)


def train_image(i):
    return synth_frame(7, 0, 400 * i, H, W)


def describe(oracle, offsets, img):
    rc, _, _ = oracle.fast(img, max_kp=MAX_KP)
    return oracle.brief(img, rc, offsets)


@functools.lru_cache(maxsize=None)
def _scene(n_words, iters):
    import oracle_bind
    oracle = oracle_bind.Oracle()
    offsets = np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                       "brief_offsets_mt19937_42.bin"), np.int8).reshape(256, 4)
    places = [describe(oracle, offsets, place_image(i)) for i in range(N_PLACES)]
    revisits = [describe(oracle, offsets, revisit_image(i)) for i in range(N_PLACES)]
    train = np.concatenate([describe(oracle, offsets, train_image(i))["featVec"] for i in range(8)])
    words = ref.train_vocabulary(train, n_words, iters, 0)
    idf = ref.idf_table([ref.words_of(p["featVec"], words)[0] for p in places], n_words)
    return places, revisits, words, idf


def scene(n_words=256, iters=0):
    """-> (places [16] keypoint arrays, revisits [16], words [n_words][32], idf_q8 [n_words])"""
    return _scene(n_words, iters)
