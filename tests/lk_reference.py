"""One Newton step of the pyramidal LK tracker (cv::calcOpticalFlowPyrLK's LKTrackerInvoker) on one level image
pair, stated in plain numpy from the published algorithm: integers exact in int64, everything after the window
integers in float64.  Written independently of oracle/yavo_oracle_lk.c (tests/test_oracle_lk.py holds the oracle
against it); it shares no code with it.

What is float32 here on purpose: the window's sub-pixel position.  OpenCV subtracts the half window from the float32
point and takes the fractions a, b in float32, and the four 14-bit weights are cvRound of float32 products; they are
part of the operation's definition (they decide the integers), not of its rounding error.
"""
import numpy as np

W_BITS = 14
FLT_EPSILON = float(np.finfo(np.float32).eps)

# decisions of one point at one level (the values of OR_LK_* in oracle/yavo_oracle.h)
WINDOW_OUTSIDE, MIN_EIG, DET, EPS, MAX_COUNT, ERR_OUTSIDE = 1, 2, 3, 5, 7, 8


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101) for any integer p: ... 2 1 | 0 1 2 .. n-1 | n-2 n-3 ..., period
    2n - 2."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q < n, q, 2 * n - 2 - q)


def scharr(img):
    """(dx, dy) int64 [H, W]: the 3x3 Scharr pair (3, 10, 3) x (-1, 0, 1), REFLECT_101 at the image border."""
    H, W = img.shape
    s = img.astype(np.int64)
    rows, cols = np.arange(H), np.arange(W)
    up, dn = s[reflect101(rows - 1, H)], s[reflect101(rows + 1, H)]
    smooth_v = 3 * up + 10 * s + 3 * dn
    diff_v = dn - up
    lf, rt = reflect101(cols - 1, W), reflect101(cols + 1, W)
    dx = smooth_v[:, rt] - smooth_v[:, lf]
    dy = 3 * diff_v[:, lf] + 10 * diff_v + 3 * diff_v[:, rt]
    return dx, dy


def weights(a, b):
    """The four bilinear weights as 14-bit integers: the first three rounded (to nearest even, cvRound) from float32
    products, the fourth what is left of 2^14."""
    a, b = np.float32(a), np.float32(b)
    one, full = np.float32(1), np.float32(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * full))
    w01 = int(np.rint(a * (one - b) * full))
    w10 = int(np.rint((one - a) * b * full))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n  # int64, arithmetic shift: floor((x + half) / 2^n)


def _window(ix0, iy0, win):
    return (iy0 + np.arange(win + 1))[:, None], (ix0 + np.arange(win + 1))[None, :]


def _bilinear(samples, w):
    """samples [win + 1, win + 1] int64 at the window's integer grid -> the weighted sums [win, win]."""
    return w[0] * samples[:-1, :-1] + w[1] * samples[:-1, 1:] + w[2] * samples[1:, :-1] + w[3] * samples[1:, 1:]


def _image_samples(img, ix0, iy0, win):
    ys, xs = _window(ix0, iy0, win)
    return img.astype(np.int64)[reflect101(ys, img.shape[0]), reflect101(xs, img.shape[1])]


def _deriv_samples(d, ix0, iy0, win):
    """The derivative image is bordered with zeros."""
    H, W = d.shape
    ys, xs = _window(ix0, iy0, win)
    inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    return np.where(inside, d[np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)], 0)


def newton_step(prev, nxt, pt, win, derivs=None):
    """One LK step of the point pt = (x, y) from itself (level 0 is also the top level: the first guess is the point).

    -> dict: outside (the window's corner lies outside [-win, size)), w (weights), I, Ix, Iy, dI (the window integers
    [win, win]; dI = J - I with J sampled at the same position), A11, A12, A22, b1, b2, D, min_eig, step (dx, dy) in
    float64 (None where outside; step is NaN or inf where D is 0)."""
    H, W = prev.shape
    halfw = np.float32((win - 1) * 0.5)
    px, py = np.float32(pt[0]) - halfw, np.float32(pt[1]) - halfw
    fx, fy = np.floor(px), np.floor(py)
    r = dict(outside=True)
    if not (np.isfinite(fx) and np.isfinite(fy) and -win <= fx < W and -win <= fy < H):
        return r
    ix0, iy0 = int(fx), int(fy)
    w = weights(px - np.float32(ix0), py - np.float32(iy0))
    dx, dy = scharr(prev) if derivs is None else derivs
    I = _descale(_bilinear(_image_samples(prev, ix0, iy0, win), w), W_BITS - 5)
    J = _descale(_bilinear(_image_samples(nxt, ix0, iy0, win), w), W_BITS - 5)
    Ix = _descale(_bilinear(_deriv_samples(dx, ix0, iy0, win), w), W_BITS)
    Iy = _descale(_bilinear(_deriv_samples(dy, ix0, iy0, win), w), W_BITS)
    dI = J - I
    scale = 2.0 ** -20
    A11, A12, A22 = (float(np.sum(Ix * Ix)) * scale, float(np.sum(Ix * Iy)) * scale, float(np.sum(Iy * Iy)) * scale)
    b1, b2 = float(np.sum(dI * Ix)) * scale, float(np.sum(dI * Iy)) * scale
    D = A11 * A22 - A12 * A12
    min_eig = (A22 + A11 - np.sqrt((A11 - A22) ** 2 + 4.0 * A12 * A12)) / (2 * win * win)
    with np.errstate(divide="ignore", invalid="ignore"):
        step = (np.float64(A12 * b2 - A22 * b1) / D, np.float64(A12 * b1 - A11 * b2) / D)
    r.update(outside=False, w=w, I=I, Ix=Ix, Iy=Iy, dI=dI, A11=A11, A12=A12, A22=A22, b1=b1, b2=b2, D=D,
             min_eig=min_eig, step=step)
    return r


def decide(r, pt, shape, win, min_eig_thr, eps):
    """What the tracker does with newton_step's r at level 0 = top level, max_count 1: the exit code, the status and
    how far the numbers that decide stand from their thresholds (margin: the smallest distance; inf where none is
    consulted)."""
    if r["outside"]:
        return WINDOW_OUTSIDE, False, np.inf
    margin = abs(r["min_eig"] - min_eig_thr)
    if r["min_eig"] < min_eig_thr:
        return MIN_EIG, False, margin
    margin = min(margin, abs(r["D"] - FLT_EPSILON))
    if r["D"] < FLT_EPSILON:
        return DET, False, margin
    H, W = shape
    halfw = (win - 1) * 0.5
    ex, ey = float(pt[0]) + r["step"][0] - halfw, float(pt[1]) + r["step"][1] - halfw
    # the error window's corner floor(e) must lie in [-win, size): e in [-win, size)
    margin = min(margin, abs(ex + win), abs(ex - W), abs(ey + win), abs(ey - H))
    if not (-win <= ex < W and -win <= ey < H):
        return ERR_OUTSIDE, False, margin
    n2 = r["step"][0] ** 2 + r["step"][1] ** 2
    if eps > 0:
        margin = min(margin, abs(np.sqrt(n2) - eps))
    return (EPS if n2 <= eps * eps else MAX_COUNT), True, margin
