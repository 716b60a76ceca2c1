"""The numpy specification of the scale pyramid (yv_batch_set_pyramid): the level images (a
centre-aligned integer bilinear resample at positions given in closed form, the four-tap blend of section 20's remap),
the mapping of a level's coordinates to level 0 and the merge order.  Written from the text of the specification; the
GPU tests compare the kernels against it byte for byte and record for record."""
import numpy as np

MAX_LEVELS = 8


def src_pos(n_src, n_dst):
    """The source position of every destination index, in 1/32 pixel: int64 [n_dst]."""
    assert 1 <= n_dst <= n_src <= 2 * n_dst
    r = np.arange(n_dst, dtype=np.int64)
    q = ((2 * r + 1) * n_src - n_dst) * 16 // n_dst
    return np.clip(q, 0, (n_src - 1) * 32)


def level_map(Hs, Ws, H, W):
    """The formula's map in section 20's form: int32 [H, W, 2] = (qu, qv), source column and row in 1/32 pixel."""
    qv, qu = np.meshgrid(src_pos(Hs, H), src_pos(Ws, W), indexing="ij")
    return np.stack([qu, qv], -1).astype(np.int32)


def resample(src, H, W):
    """One level step: uint8 [Hs, Ws] -> uint8 [H, W]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    Hs, Ws = src.shape
    qv, qu = src_pos(Hs, H), src_pos(Ws, W)
    iy, ay, ix, ax = (qv >> 5)[:, None], (qv & 31)[:, None], (qu >> 5)[None, :], (qu & 31)[None, :]
    s = src.astype(np.int64)
    # a tap one past the last row or column carries weight 0 (the clamp of the position): read the last one instead
    iy1, ix1 = np.minimum(iy + 1, Hs - 1), np.minimum(ix + 1, Ws - 1)
    assert np.all((iy1 == iy + 1) | (ay == 0)) and np.all((ix1 == ix + 1) | (ax == 0))
    t = (32 - ax) * s[iy, ix] + ax * s[iy, ix1]
    b = (32 - ax) * s[iy1, ix] + ax * s[iy1, ix1]
    return (((32 - ay) * t + ay * b + 512) >> 10).astype(np.uint8)


def resample_slow(src, H, W):
    """resample pixel by pixel, as the specification is written (the vectorised form is checked against it)."""
    Hs, Ws = src.shape
    dst = np.zeros((H, W), np.uint8)

    def tap(r, c):
        return int(src[r, c]) if r < Hs and c < Ws else 0

    for v in range(H):
        qv = min(max(((2 * v + 1) * Hs - H) * 16 // H, 0), (Hs - 1) * 32)
        for u in range(W):
            qu = min(max(((2 * u + 1) * Ws - W) * 16 // W, 0), (Ws - 1) * 32)
            ix, ax, iy, ay = qu >> 5, qu & 31, qv >> 5, qv & 31
            t = (32 - ax) * tap(iy, ix) + ax * tap(iy, ix + 1)
            b = (32 - ax) * tap(iy + 1, ix) + ax * tap(iy + 1, ix + 1)
            dst[v, u] = ((32 - ay) * t + ay * b + 512) >> 10
    return dst


def build_levels(img, sizes):
    """The level images of img over sizes [(H_l, W_l)]: level 0 is img itself, level l the resample of level l - 1."""
    assert tuple(sizes[0]) == img.shape
    levels = [np.ascontiguousarray(img)]
    for h, w in sizes[1:]:
        levels.append(resample(levels[-1], int(h), int(w)))
    return levels


def check_sizes(sizes):
    """The rule the sizes obey: non-increasing, a shrink of at most 2 per level, every side at least 9."""
    assert 1 <= len(sizes) <= MAX_LEVELS
    for l, (h, w) in enumerate(sizes):
        assert h >= 9 and w >= 9
        if l:
            ph, pw = sizes[l - 1]
            assert h <= ph and w <= pw and 2 * h >= ph and 2 * w >= pw


def to_level0(x, n0, nl):
    """A level coordinate on level 0: floor((2 x + 1) n0 / (2 nl))."""
    return (2 * np.asarray(x, np.int64) + 1) * n0 // (2 * nl)


def merge(per_level, sizes):
    """The merged list of the levels' keypoint records (structured arrays with x, y, id, matched, featVec): level 0's
    records as they are, then levels 1.. in level order and each in its own order with x / y mapped to level 0, id =
    the merged index and matched = 0 -> (records, level [n] uint8, level_rc [n, 2] int32)."""
    H0, W0 = sizes[0]
    out, level, rc = [per_level[0].copy()], [np.zeros(len(per_level[0]), np.uint8)], \
        [np.stack([per_level[0]["x"], per_level[0]["y"]], -1).astype(np.int32).reshape(-1, 2)]
    off = len(per_level[0])
    for l in range(1, len(per_level)):
        k = per_level[l].copy()
        rc.append(np.stack([k["x"], k["y"]], -1).astype(np.int32).reshape(-1, 2))
        k["x"] = to_level0(k["x"], H0, sizes[l][0])
        k["y"] = to_level0(k["y"], W0, sizes[l][1])
        k["id"] = off + np.arange(len(k))
        k["matched"] = 0
        out.append(k)
        level.append(np.full(len(k), l, np.uint8))
        off += len(k)
    return np.concatenate(out), np.concatenate(level), np.concatenate(rc)


def zoom_out(img, factor):
    """img shrunk by `factor` about its centre with the specification's resample, centred on a canvas of img's size
    filled with the image's mean -> (canvas, (h, w) of the shrunk copy, (row, col) of its first pixel)."""
    H, W = img.shape
    h, w = int(round(H / factor)), int(round(W / factor))
    small = resample(img, h, w)
    r0, c0 = (H - h) // 2, (W - w) // 2
    canvas = np.full((H, W), int(img.mean()), np.uint8)
    canvas[r0:r0 + h, c0:c0 + w] = small
    return canvas, (h, w), (r0, c0)


def zoom_truth(x, y, shape, small, origin):
    """Where the level-0 pixel (x = row, y = col) of the image lies on zoom_out's canvas (float)."""
    H, W = shape
    h, w = small
    return (np.asarray(x) + 0.5) * h / H - 0.5 + origin[0], (np.asarray(y) + 0.5) * w / W - 0.5 + origin[1]


def oracle_keypoints(orc, img, sizes, quotas, offsets):
    """The merged multi-scale keypoints of img from the CPU oracle (tests/oracle_bind.py): per level FAST with the cut
    at the level's quota and BRIEF on the specification's level image, then merge."""
    per = []
    for lv, q in zip(build_levels(img, sizes), quotas):
        rc, _, _ = orc.fast(lv, int(q))
        per.append(orc.brief(lv, rc, offsets))
    return merge(per, sizes)


def correct_matches(filtered, shape, small, origin, radius=2.0):
    """How many of the kept Matches records (pt1 on the image, pt2 on zoom_out's canvas) lie within `radius` pixels of
    the true position."""
    tx, ty = zoom_truth(filtered["pt1"]["x"], filtered["pt1"]["y"], shape, small, origin)
    return int((np.hypot(filtered["pt2"]["x"] - tx, filtered["pt2"]["y"] - ty) <= radius).sum())
