"""Level sizes and keypoint quotas of the scale pyramid (yv_batch_set_pyramid)."""
from typing import List, Sequence, Tuple

MAX_LEVELS = 8
MIN_SIDE = 9


def _side(n0: int, prev: int, level: int, scale: float) -> int:
    # the rounded side, kept inside what a level may be: no larger than the level before, at least half of it
    # (rounded up) and at least the detector's minimum
    want = int(n0 / scale ** level + 0.5)
    return max(MIN_SIDE, (prev + 1) // 2, min(prev, want))


def level_sizes(H: int, W: int, n_levels: int, scale: float = 1.2) -> List[Tuple[int, int]]:
    """(H_l, W_l) of n_levels levels: level 0 is H x W, level l is H / scale^l x W / scale^l rounded, non-increasing
    and never less than half of the level before."""
    if not 1 <= n_levels <= MAX_LEVELS:
        raise ValueError("n_levels must be in 1..8")
    if not scale >= 1.0:
        raise ValueError("scale must be >= 1")
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError("H and W must be at least 9")
    sizes = [(int(H), int(W))]
    for l in range(1, n_levels):
        ph, pw = sizes[-1]
        sizes.append((_side(H, ph, l, scale), _side(W, pw, l, scale)))
    return sizes


def level_quotas(max_kp: int, sizes: Sequence[Tuple[int, int]]) -> List[int]:
    """Keypoint quotas proportional to the levels' areas (rounded down), the remainder to level 0: they sum to
    max_kp."""
    if max_kp < 0:
        raise ValueError("max_kp must not be negative")
    areas = [int(h) * int(w) for h, w in sizes]
    total = sum(areas)
    q = [max_kp * a // total for a in areas]
    q[0] += max_kp - sum(q)
    return q
