"""The numpy specification of the rectifier (yv_rectify_*): the map of a camera model in 1/32
pixel, computed in float64 in one stated order, and the integer bilinear remap with a constant zero border.  Written
from the text of the specification; the GPU tests compare the kernels against it entry for entry and byte for byte.

Conventions: u = column, v = row; camera matrices row-major with fx, cx on the first row; a map is int32 [H][W][2] =
(qu, qv), the source column and row in 1/32 pixel, OUTSIDE in either component marking a pixel without a source."""
import numpy as np

OUTSIDE = -2 ** 31  # YV_RECTIFY_OUTSIDE = INT32_MIN


def rectify_matrix(K_new, R):
    """inv(K_new @ R), flattened: the M of model_map (OpenCV's iR)."""
    K_new, R = np.asarray(K_new, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3)
    return np.linalg.inv(K_new @ R).reshape(9)


def model_map(K, dist, M, H, W):
    """The source position (mu, mv) of every destination pixel, float64 [H, W] each; every operation in the
    specification's order (numpy neither contracts nor reassociates)."""
    K = np.asarray(K, np.float64).reshape(9)
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(d) for d in np.asarray(dist, np.float64).reshape(8))
    M = np.asarray(M, np.float64).reshape(9)
    fx, cx, fy, cy = K[0], K[2], K[4], K[5]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        X = (M[0] * u + M[1] * v) + M[2]
        Y = (M[3] * u + M[4] * v) + M[5]
        Wd = (M[6] * u + M[7] * v) + M[8]
        x = X / Wd
        y = Y / Wd
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (2.0 * x) * y
        kr = ((((k3 * r2 + k2) * r2 + k1) * r2) + 1.0) / ((((k6 * r2 + k5) * r2 + k4) * r2) + 1.0)
        xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
        mu = fx * xd + cx
        mv = fy * yd + cy
    return mu, mv


def quantise(mu, mv):
    """(mu, mv) -> int32 [H, W, 2]: rint(m * 32) inside (-65536, 65536), else OUTSIDE (NaN fails both tests); one
    component OUTSIDE makes both."""
    with np.errstate(all="ignore"):
        ok = (mu > -65536.0) & (mu < 65536.0) & (mv > -65536.0) & (mv < 65536.0)
        q = np.stack([np.rint(np.where(ok, mu, 0.0) * 32.0), np.rint(np.where(ok, mv, 0.0) * 32.0)], -1)
    q = q.astype(np.int64)
    q[~ok] = OUTSIDE
    return q.astype(np.int32)


def model_map_q5(K, dist, M, H, W):
    return quantise(*model_map(K, dist, M, H, W))


def remap(src, map_q5):
    """The remap of a uint8 image [Hs, Ws] through int32 map_q5 [H, W, 2] -> uint8 [H, W]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    Hs, Ws = src.shape
    m = np.asarray(map_q5).astype(np.int64)
    qu, qv = m[..., 0], m[..., 1]
    out = (qu == OUTSIDE) | (qv == OUTSIDE)
    ix, ax, iy, ay = qu >> 5, qu & 31, qv >> 5, qv & 31  # arithmetic shifts

    def tap(r, c):
        ins = (r >= 0) & (r < Hs) & (c >= 0) & (c < Ws) & ~out
        return np.where(ins, src[np.clip(r, 0, Hs - 1), np.clip(c, 0, Ws - 1)].astype(np.int64), 0)

    t = (32 - ax) * tap(iy, ix) + ax * tap(iy, ix + 1)
    b = (32 - ax) * tap(iy + 1, ix) + ax * tap(iy + 1, ix + 1)
    d = ((32 - ay) * t + ay * b + 512) >> 10
    return np.where(out, 0, d).astype(np.uint8)


def remap_slow(src, map_q5):
    """remap pixel by pixel, as the specification is written (the vectorised form is checked against it)."""
    Hs, Ws = src.shape
    H, W = map_q5.shape[:2]
    dst = np.zeros((H, W), np.uint8)

    def tap(r, c):
        return int(src[r, c]) if 0 <= r < Hs and 0 <= c < Ws else 0

    for v in range(H):
        for u in range(W):
            qu, qv = int(map_q5[v, u, 0]), int(map_q5[v, u, 1])
            if qu == OUTSIDE or qv == OUTSIDE:
                continue
            ix, ax, iy, ay = qu >> 5, qu & 31, qv >> 5, qv & 31
            t = (32 - ax) * tap(iy, ix) + ax * tap(iy, ix + 1)
            b = (32 - ax) * tap(iy + 1, ix) + ax * tap(iy + 1, ix + 1)
            dst[v, u] = ((32 - ay) * t + ay * b + 512) >> 10
    return dst


# ---- maps the tests share ----
def identity_map(H, W, du=0, dv=0):
    """(32 u + du, 32 v + dv)."""
    v, u = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    return np.stack([32 * u + du, 32 * v + dv], -1).astype(np.int32)


def outside_map(H, W):
    return np.full((H, W, 2), OUTSIDE, np.int32)


def random_map(Hs, Ws, H, W, seed):
    """Uniform q5 in [-64, 32 (Ws + 1)] x [-64, 32 (Hs + 1)]: taps on every border, boxes that span the source."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-64, 32 * (Ws + 1) + 1, (H, W)), rng.integers(-64, 32 * (Hs + 1) + 1, (H, W))],
                    -1).astype(np.int32)


def rotation_map(Hs, Ws, H, W):
    """A 90 degree rotation: destination (u, v) reads source column v, row W - 1 - u (outside the source where the
    shapes do not match): a destination row walks down a source column."""
    v, u = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    return np.stack([32 * v, 32 * (W - 1 - u)], -1).astype(np.int32)


def split_map(Hs, Ws, H, W, seed):
    """Identity on the left half of the destination, random on the right."""
    m = identity_map(H, W)
    m[:, W // 2:] = random_map(Hs, Ws, H, W, seed)[:, W // 2:]
    return m


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _scaled(Hs, Ws, H, W, f_src, f_new):
    """K of a source Hs x Ws and K_new of a destination H x W: the focal lengths of a 512 x 1392 source and a
    376 x 1241 destination, scaled per axis so that other sizes see the same field of view."""
    K = np.array([[f_src * Ws / 1392.0, 0, 0.5 * Ws - 0.3], [0, f_src * Hs / 512.0 * 1.003, 0.5 * Hs + 0.2], [0, 0, 1]])
    Kn = np.array([[f_new * W / 1241.0, 0, 0.5 * W], [0, f_new * H / 376.0, 0.5 * H], [0, 0, 1]])
    return K, Kn


def kitti_raw_model(Hs=512, Ws=1392, H=376, W=1241):
    """A KITTI-raw-like camera (k1 = -0.373, k2 = 0.204, k3 = -0.072, 0.01 rad roll), scaled to the given sizes ->
    (K [9], dist [8], M [9])."""
    K, Kn = _scaled(Hs, Ws, H, W, 984.0, 721.5)
    dist = np.array([-0.373, 0.204, 0.0, 0.0, -0.072, 0.0, 0.0, 0.0])
    return K.reshape(9), dist, rectify_matrix(Kn, _rot(0.0, 0.0, 0.01))


def full_model(Hs, Ws, H, W):
    """All eight coefficients, tangential terms and a rotation about all three axes."""
    K, Kn = _scaled(Hs, Ws, H, W, 984.0, 800.0)
    dist = np.array([-0.31, 0.12, 0.0011, -0.0007, -0.02, 0.05, -0.01, 0.003])
    return K.reshape(9), dist, rectify_matrix(Kn, _rot(0.02, -0.015, 0.03))


def horizon_model(Hs, Ws, H, W):
    """A wide destination (f = 60 at 1241 columns) pitched by 45 degrees: the source's horizon Wd = 0 is a line through
    the destination, Wd is negative beyond it, and the source itself lies on the other side of the centre."""
    K, Kn = _scaled(Hs, Ws, H, W, 984.0, 60.0)
    dist = np.array([-0.1, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    return K.reshape(9), dist, rectify_matrix(Kn, _rot(np.deg2rad(45.0), 0.0, 0.0))


MODELS = {"kitti_raw": kitti_raw_model, "full": full_model, "horizon": horizon_model}
