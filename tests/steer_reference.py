"""The numpy specification of the rotation-steered BRIEF (yv_set_brief_steering): clamped sampling
of the blurred image, the centroid moments over a disc, the bin and the descriptor.  Integer only (int64 throughout), so
every GPU comparison against it is exact equality."""
import numpy as np

from ya_vo_amd import KEYPOINT_DTYPE


def blur(oracle, img):
    """The image the descriptor samples: or_gaussian_blur_u8, the 9 x 9 fixed-point Gaussian."""
    return oracle.blur(np.ascontiguousarray(img, np.uint8))


def sample(b, r, c):
    """S(r, c) = b[clamp(r, 0, H - 1)][clamp(c, 0, W - 1)] as int64."""
    H, W = b.shape
    return b[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)].astype(np.int64)


def disc(radius):
    """(dr, dc) of the pixels with dr^2 + dc^2 <= radius^2."""
    d = np.arange(-radius, radius + 1)
    dr, dc = np.meshgrid(d, d, indexing="ij")
    keep = dr * dr + dc * dc <= radius * radius
    return dr[keep], dc[keep]


def moments(b, rc, radius=15):
    """[n, 2] = (m10, m01) = (sum dc S, sum dr S) over the disc."""
    rc = np.asarray(rc, np.int64).reshape(-1, 2)
    dr, dc = disc(radius)
    s = sample(b, rc[:, 0:1] + dr[None, :], rc[:, 1:2] + dc[None, :])
    return np.stack([(s * dc[None, :]).sum(1), (s * dr[None, :]).sum(1)], 1)


def bins(mom, dirs):
    """The smallest k that maximises m10 dirs[k][0] + m01 dirs[k][1]."""
    d = np.asarray(dirs, np.int64).reshape(-1, 2)
    score = mom[:, 0:1] * d[None, :, 0] + mom[:, 1:2] * d[None, :, 1]
    assert np.abs(score).max(initial=0) < 2 ** 31
    return np.argmax(score, axis=1).astype(np.uint8)  # argmax returns the first maximum


def feat_vec(b, rc, bin_, offsets):
    """[n, 32] uint8: test t of a keypoint in bin k is S(row + o[0], col + o[1]) > S(row + o[2], col + o[3]), o =
    offsets[k][t], into bit t % 8 of byte t / 8."""
    rc = np.asarray(rc, np.int64).reshape(-1, 2)
    o = np.asarray(offsets, np.int64).reshape(-1, 256, 4)[np.asarray(bin_, np.int64)]  # [n, 256, 4]
    r, c = rc[:, 0:1], rc[:, 1:2]
    bits = sample(b, r + o[:, :, 0], c + o[:, :, 1]) > sample(b, r + o[:, :, 2], c + o[:, :, 3])
    return np.packbits(bits, axis=1, bitorder="little").reshape(len(rc), 32)


def describe(b, rc, dirs, offsets, radius=15):
    """-> (featVec [n, 32], bin [n] uint8, moments [n, 2] int64) of every position, no boundary filter."""
    mom = moments(b, rc, radius)
    k = bins(mom, dirs)
    return feat_vec(b, rc, k, offsets), k, mom


def inside_boundary(rc, H, W):
    """checkBoundry: 8 <= row <= H - 8 and 8 <= col <= W - 8."""
    rc = np.asarray(rc, np.int64).reshape(-1, 2)
    return (rc[:, 0] >= 8) & (rc[:, 0] <= H - 8) & (rc[:, 1] >= 8) & (rc[:, 1] <= W - 8)


def records(rc, ids, feat):
    """The 48-byte KeyPoint records: row, col, id, matched = 0, featVec, zero padding."""
    rc = np.asarray(rc, np.int64).reshape(-1, 2)
    k = np.zeros(len(rc), KEYPOINT_DTYPE)
    k["x"], k["y"], k["id"] = rc[:, 0], rc[:, 1], ids
    k["featVec"] = feat
    return k


def describe_records(b, rc, dirs, offsets, radius=15):
    """What yv_describe returns under steering for the list rc of the image blurred to b: the records of the positions
    inside checkBoundry in list order with id = the list index -> (records, bin, moments of the kept ones)."""
    rc = np.asarray(rc, np.int64).reshape(-1, 2)
    keep = inside_boundary(rc, *b.shape)
    feat, k, mom = describe(b, rc[keep], dirs, offsets, radius)
    return records(rc[keep], np.flatnonzero(keep), feat), k, mom


def plain_table(offsets):
    """The one-bin table: the plain offsets, never turned."""
    return np.array([[256, 0]], np.int16), np.asarray(offsets, np.int8).reshape(1, 256, 4)


def hamming(a, b):
    """Bit distance of featVec rows a [n, 32] and b [n, 32]."""
    return np.unpackbits(a ^ b, axis=1).sum(1)


def hamming_matrix(a, b):
    """[n, m] bit distances of every row of a against every row of b."""
    ua, ub = np.unpackbits(a, axis=1).astype(np.int32), np.unpackbits(b, axis=1).astype(np.int32)
    return ua @ (1 - ub).T + (1 - ua) @ ub.T


def rotate_bilinear(img, degrees):
    """img turned by `degrees` about its centre, bilinear, samples clamped to the image -> (uint8 image, a function
    mapping positions [n, 2] (row, col) of img to their positions in the turned image)."""
    H, W = img.shape
    cr, cc = (H - 1) / 2.0, (W - 1) / 2.0
    t = np.deg2rad(degrees)
    c, s = np.cos(t), np.sin(t)
    rr, qq = np.meshgrid(np.arange(H) - cr, np.arange(W) - cc, indexing="ij")
    # the source position of every output pixel: the inverse turn
    sr, sc = c * rr + s * qq + cr, -s * rr + c * qq + cc
    r0, c0 = np.floor(sr).astype(np.int64), np.floor(sc).astype(np.int64)
    fr, fc = sr - r0, sc - c0
    f = img.astype(np.float64)

    def at(r, q):
        return f[np.clip(r, 0, H - 1), np.clip(q, 0, W - 1)]

    out = ((1 - fr) * ((1 - fc) * at(r0, c0) + fc * at(r0, c0 + 1))
           + fr * ((1 - fc) * at(r0 + 1, c0) + fc * at(r0 + 1, c0 + 1)))

    def forward(rc):
        p = np.asarray(rc, np.float64).reshape(-1, 2) - (cr, cc)
        return np.rint(np.stack([c * p[:, 0] - s * p[:, 1] + cr, s * p[:, 0] + c * p[:, 1] + cc], 1)).astype(np.int64)

    return np.clip(np.rint(out), 0, 255).astype(np.uint8), forward


def recall(feat_a, feat_b):
    """The share of rows of feat_a whose nearest row of feat_b (first on ties) is the one of the same index."""
    d = hamming_matrix(feat_a, feat_b)
    return float(np.mean(np.argmin(d, axis=1) == np.arange(len(feat_a))))
