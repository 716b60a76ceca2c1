"""Default tables of the rotation-steered BRIEF (yv_set_brief_steering): the offsets table rotated to n_bins directions.

Bin k stands for the direction theta = 2 pi k / n_bins of the patch's intensity centroid (m10, m01) = (column moment,
row moment).  Its tests are the plain table's tests turned by theta, so a patch that turns with the image keeps its
descriptor.  Only the first quadrant of bins is rounded from float64; every further bin is the exact quarter turn of the
bin n_bins / 4 before it, which makes the descriptors of an image and of its np.rot90 equal bit for bit.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

MAX_BINS = 64
MAX_COMPONENT = 15   # |offsets| bound of yv_set_brief_steering
MAX_DIR = 256        # |dirs| bound


def steering_tables(offsets: np.ndarray, n_bins: int = 32) -> Tuple[np.ndarray, np.ndarray]:
    """offsets [256, 4] int8 {drow1, dcol1, drow2, dcol2} -> (dirs [n_bins, 2] int16 (dcol, drow), offsets
    [n_bins, 256, 4] int8).  n_bins: a multiple of 4 up to 64."""
    n_bins = int(n_bins)
    if n_bins <= 0 or n_bins > MAX_BINS or n_bins % 4 != 0:
        raise ValueError("n_bins must be a multiple of 4 in 4..64")
    pts = np.asarray(offsets, dtype=np.int64).reshape(256, 2, 2)  # [test][point][(drow, dcol)]
    quad = n_bins // 4
    dirs = np.zeros((n_bins, 2), np.int64)
    out = np.zeros((n_bins, 256, 2, 2), np.int64)
    for k in range(quad):
        theta = 2.0 * np.pi * k / n_bins
        c, s = np.cos(theta), np.sin(theta)
        dirs[k] = (np.rint(256.0 * c), np.rint(256.0 * s))
        drow, dcol = pts[..., 0].astype(np.float64), pts[..., 1].astype(np.float64)
        out[k, ..., 0] = np.rint(s * dcol + c * drow)
        out[k, ..., 1] = np.rint(c * dcol - s * drow)
    for k in range(quad, n_bins):
        # the exact quarter turn of bin k - quad: (drow, dcol) -> (dcol, -drow), (dcol, drow) -> (-drow, dcol)
        out[k, ..., 0] = out[k - quad, ..., 1]
        out[k, ..., 1] = -out[k - quad, ..., 0]
        dirs[k] = (-dirs[k - quad, 1], dirs[k - quad, 0])
    if np.abs(out).max() > MAX_COMPONENT or np.abs(dirs).max() > MAX_DIR:
        raise ValueError("a rotated offset leaves the radius-15 patch")
    return dirs.astype(np.int16), out.reshape(n_bins, 256, 4).astype(np.int8)
