"""Scenes of the P3P-RANSAC tests (tests/test_pnp_ransac_abi.py, tests/test_gpu_pnp_ransac.py): ya_vo_amd.scene's
random scenes as they are (small motion: the scene's own pose, <= 0.2 rad and ~0.5 m from the identity) and with the
world moved by 1.2 rad about (0.2, 1, 0.1) and (3, -0.5, 8) m (large motion: the true pose is far from the identity,
the measurements are the same)."""
import numpy as np

from ya_vo_amd import scene

K9 = scene.K_KITTI.reshape(9).copy()
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
BIG_AXIS, BIG_ANGLE, BIG_T = (0.2, 1.0, 0.1), 1.2, np.array([3.0, -0.5, 8.0])


def quat_mul(a, b):
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                     w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def move_world(X, T, axis=BIG_AXIS, angle=BIG_ANGLE, t=BIG_T):
    """X' = M X and T' = T M^-1 for the motion M = (axis, angle, t): T' X' = T X, so the measurements stay."""
    qm = scene.quat_from_axis_angle(axis, angle)
    Rm = scene.quat_to_R(qm)
    Xn = np.ascontiguousarray((Rm @ np.asarray(X).T).T + t)
    qi = np.array([-qm[0], -qm[1], -qm[2], qm[3]])
    ti = -(Rm.T @ t)
    q = quat_mul(T[:4], qi)
    tt = scene.quat_to_R(T[:4]) @ ti + T[4:]
    return Xn, scene.pose(q / np.linalg.norm(q), tt)


def pnp_scene(n=200, seed=0, outlier_frac=0.5, large=True, noise_px=0.3):
    """-> (X [n,3], uv [n,2], T_true [7], clean mask [n] bool)"""
    X, uv, T, out = scene.random_scene(n, seed=seed, noise_px=noise_px, outlier_frac=outlier_frac)
    if large:
        X, T = move_world(X, T)
    return np.ascontiguousarray(X), np.ascontiguousarray(uv), T, ~out


def rot_angle(Ta, Tb):
    """The angle between two poses' rotations (rad)."""
    d = abs(float(np.dot(Ta[:4], Tb[:4])))
    return 2.0 * np.arccos(min(1.0, d))
