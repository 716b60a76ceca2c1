"""ctypes binding of the CPU oracle (oracle/build/liboracle.so) -- test infrastructure only.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg load this; the product path never
does (see oracle/yavo_oracle.h)."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_PATH = os.path.join(ROOT, "oracle", "build", "liboracle.so")

from ya_vo_amd import KEYPOINT_DTYPE, MATCH_DTYPE, DEFAULT_BLUR_KERNEL  # noqa: E402  (record layouts only)

_P = ctypes.c_void_p
_I = ctypes.c_int


def _p(a):
    return a.ctypes.data if a is not None else None


class Oracle:
    def __init__(self, path=ORACLE_PATH):
        lib = ctypes.CDLL(path)
        sig = {
            "or_bresenham_ring": (None, [_I, _I, _P]),
            "or_bresenham_ring_stl": (None, [_I, _I, _P]),
            "or_check_contiguous": (_I, [ctypes.c_uint8, _P, _P, _I, _I]),
            "or_fast_detect": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, ctypes.POINTER(_I), ctypes.POINTER(_I),
                                    _P, _P, _I]),
            "or_harris_response": (ctypes.c_float, [ctypes.c_float, ctypes.c_float, ctypes.c_float]),
            "or_eigen_jacobi_f32": (None, [_P, _I, _P]),
            "or_eigen_selfadjoint2_f32": (None, [ctypes.c_float, ctypes.c_float, ctypes.c_float, _P]),
            "or_set_harris_eigen": (None, [_I]),
            "or_set_libm_flavour": (None, [_I]),
            "or_cube_batch": (None, [_P, _I, _I, _P]),
            "or_std_sort_cut": (_I, [_P, _P, _I, _I, _I, _P]),
            "or_gauss_kernel_fixed": (None, [_I, ctypes.c_double, _I, _P]),
            "or_gaussian_blur_u8": (None, [_P, _I, _I, _I, _P, _I, _P]),
            "or_compute_brief_blurred": (_I, [_P, _I, _I, _P, _P, _I, _P, ctypes.POINTER(_I)]),
            "or_compute_brief": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _P, ctypes.POINTER(_I)]),
            "or_brief_offsets_mt19937": (None, [ctypes.c_uint32, _P]),
            "or_mt19937_new": (ctypes.c_void_p, [ctypes.c_uint32]),
            "or_mt19937_uniform_ints": (None, [ctypes.c_void_p, _I, _I, _I, _P]),
            "or_mt19937_free": (None, [ctypes.c_void_p]),
            "or_hamming": (_I, [_P, _P]),
            "or_match": (_I, [_P, _I, _P, _I, _P]),
            "or_remove_outliers": (_I, [_P, _I, _I, _P, ctypes.POINTER(_I)]),
            "or_parse_calib_string": (_I, [ctypes.c_char_p, _P]),
            "or_cv_svd": (None, [_P, _I, _P, _P, _P]),
            "or_fundamental_8pt": (_I, [_P, _I, _P]),
            "or_f_ransac": (_I, [_P, _I, _P, _I, ctypes.c_double, _P, ctypes.POINTER(_I)]),
            "or_eigen_jacobi_svd": (_I, [_P, _I, _P, _P]),
            "or_triangulate_one": (_I, [_P, _P, _P, _P, _P]),
            "or_triangulate_matches": (_I, [_P, _P, _P, _P, _I, _P, _P]),
            "or_se3_exp": (None, [_P, _P]),
            "or_se3_mul": (None, [_P, _P, _P]),
            "or_se3_inverse": (None, [_P, _P]),
            "or_se3_from_Rt": (None, [_P, _P, _P]),
            "or_se3_act": (None, [_P, _P, _P]),
            "or_quat_to_R": (None, [_P, _P]),
            "or_ksin": (ctypes.c_double, [ctypes.c_double]),
            "or_kcos": (ctypes.c_double, [ctypes.c_double]),
            "or_world2camera": (None, [_P, _I, _P, _P, _P]),
            "or_ldlt6_solve": (_I, [_P, _P, _P, _I]),
            "or_pose_lm": (_I, [_P, _P, _I, _P, _P, _P, _I]),
            "or_pose_gn": (_I, [_P, _P, _I, _P, _P, _I]),
            "or_ldlt6_solve_ex": (_I, [_P, _P, _P, _I, _P]),
            "or_pose_lm_ex": (_I, [_P, _P, _I, _P, _P, _P, _I, _P]),
            "or_pose_gn_ex": (_I, [_P, _P, _I, _P, _P, _I, _P]),
            "or_lm_stats": (None, [_P, _I]),
            "or_pyr_down": (None, [_P, _I, _I, _I, _P]),
            "or_scharr": (None, [_P, _I, _I, _I, _P]),
            "or_lk_pyr": (_I, [_P, _P, _I, _I, _P, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double, _P, _P, _P,
                               _I]),
            "or_lk_pyr_ex": (_I, [_P, _P, _I, _I, _P, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double, _P, _P, _P,
                                  _I, _P]),
            "or_em_subsets": (None, [_I, _I, _P]),
            "or_em_coeff_mat": (None, [_P, _P]),
            "or_em_det_poly": (None, [_P, _P]),
            "or_solve_poly": (_I, [_P, _I, _I, _P]),
            "or_em_kernel": (_I, [_P, _P, _P]),
            "or_solve_poly_ex": (_I, [_P, _I, _I, _P, _P]),
            "or_em_kernel_ex": (_I, [_P, _P, _P, _P]),
            "or_normalize_points": (None, [_P, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _P]),
            "or_find_essential": (_I, [_P, _P, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double, _I, _P, _P, _P]),
            "or_decompose_essential": (None, [_P, _P, _P, _P]),
            "or_recover_pose": (_I, [_P, _P, _P, _I, _P, _P, _P, _P]),
            "or_ldlt_solve": (_I, [_P, _I, _P, _P]),
            "or_ba_lm": (_I, [_P, _I, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P]),
            "or_ba_lm_mode": (_I, [_P, _I, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _I]),
            "or_map_block_bytes": (ctypes.c_int64, [_I, _I]),
            "or_map_chunk": (None, [_P, _I, ctypes.c_int64, _I, _P, _P, _P, _I, _I, _P]),
            "or_map_place": (None, [_P, _I, ctypes.c_int64, _P, _P]),
        }
        for name, (res, args) in sig.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        self.lib = lib

    def ring(self, xc=0, yc=0, stl=False):
        out = np.zeros((16, 2), np.int32)
        (self.lib.or_bresenham_ring_stl if stl else self.lib.or_bresenham_ring)(xc, yc, _p(out))
        return out

    def check_contiguous(self, cent, ring, img, thr=40):
        img = np.ascontiguousarray(img, np.uint8)
        ring = np.ascontiguousarray(ring, np.int32)
        return bool(self.lib.or_check_contiguous(cent, _p(ring), _p(img), img.shape[1], thr))

    def fast(self, img, max_kp=2000, thr=40, mode=1, with_candidates=False):
        img = np.ascontiguousarray(img, np.uint8)
        H, W = img.shape
        rc = np.zeros((max(max_kp, 1), 2), np.int32)
        resp = np.zeros(max(max_kp, 1), np.float32)
        n, nc = _I(), _I()
        cap = (H - 8) * (W - 8) if with_candidates else 0
        ci = np.zeros(max(cap, 1), np.int32) if with_candidates else None
        cr = np.zeros(max(cap, 1), np.float32) if with_candidates else None
        st = self.lib.or_fast_detect(_p(img), H, W, W, thr, max_kp, mode, _p(rc), _p(resp), ctypes.byref(n),
                                     ctypes.byref(nc), _p(ci), _p(cr), cap)
        assert st == 0
        out = (rc[:n.value].copy(), resp[:n.value].copy(), nc.value)
        if with_candidates:
            out = out + (ci[:nc.value].copy(), cr[:nc.value].copy())
        return out

    def harris_response(self, m00, m01, m11):
        return self.lib.or_harris_response(m00, m01, m11)

    def set_libm_flavour(self, flavour):
        """0: the restated pow / sin / cos the GPU kernels share (default); 1: the host C library's, as g2o / Sophus
        call them (process-wide switch of the oracle library)."""
        self.lib.or_set_libm_flavour(int(flavour))

    def cube(self, t, flavour=0):
        """g2o's pow(t, 3) as the oracle evaluates it: correctly rounded (0) or the host C library's pow (1)."""
        t = np.ascontiguousarray(t, np.float64)
        out = np.empty_like(t)
        self.lib.or_cube_batch(_p(t), len(t), int(flavour), _p(out))
        return out

    def set_harris_eigen(self, flavour):
        """cv::eigen flavour of the Harris response: 0 = JacobiImpl_ (default), 1 = HAVE_EIGEN (Eigen 3.4)."""
        self.lib.or_set_harris_eigen(int(flavour))

    def eigen_selfadjoint2(self, m00, m01, m11):
        w = np.zeros(2, np.float32)
        self.lib.or_eigen_selfadjoint2_f32(m00, m01, m11, _p(w))
        return w

    def std_sort_cut(self, idx, resp, W, K=2000):
        """The reference's std::sort(corners, response >) + first K (libstdc++), on scan-ordered candidates."""
        idx = np.ascontiguousarray(idx, np.int32)
        resp = np.ascontiguousarray(resp, np.float32)
        out = np.zeros(max(min(len(idx), K), 1), np.int32)
        m = self.lib.or_std_sort_cut(_p(idx), _p(resp), len(idx), W, K, _p(out))
        return out[:m]

    def eigen_jacobi(self, A):
        A = np.ascontiguousarray(A, np.float32)
        w = np.zeros(A.shape[0], np.float32)
        self.lib.or_eigen_jacobi_f32(_p(A), A.shape[0], _p(w))
        return w

    def gauss_kernel(self, n=9, sigma=2.5, ed=True):
        out = np.zeros(n, np.uint16)
        self.lib.or_gauss_kernel_fixed(n, sigma, 1 if ed else 0, _p(out))
        return out

    def blur(self, img, k=DEFAULT_BLUR_KERNEL):
        img = np.ascontiguousarray(img, np.uint8)
        k = np.ascontiguousarray(k, np.uint16)
        out = np.zeros_like(img)
        self.lib.or_gaussian_blur_u8(_p(img), img.shape[0], img.shape[1], img.shape[1], _p(k), len(k), _p(out))
        return out

    def brief(self, img, rc, offsets, k=DEFAULT_BLUR_KERNEL):
        img = np.ascontiguousarray(img, np.uint8)
        rc = np.ascontiguousarray(rc, np.int32).reshape(-1, 2)
        off = np.ascontiguousarray(offsets, np.int8).reshape(-1)
        k = np.ascontiguousarray(k, np.uint16)
        out = np.zeros(max(len(rc), 1), KEYPOINT_DTYPE)
        m = _I()
        st = self.lib.or_compute_brief(_p(img), img.shape[0], img.shape[1], img.shape[1], _p(k), _p(off), _p(rc),
                                       len(rc), _p(out), ctypes.byref(m))
        assert st == 0
        return out[:m.value].copy()

    def brief_offsets(self, seed):
        out = np.zeros(1024, np.int8)
        self.lib.or_brief_offsets_mt19937(seed, _p(out))
        return out.reshape(256, 4)

    def hamming(self, a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return self.lib.or_hamming(_p(a), _p(b))

    def match(self, q, t):
        q = np.ascontiguousarray(q, KEYPOINT_DTYPE)
        t = np.ascontiguousarray(t, KEYPOINT_DTYPE)
        out = np.zeros(max(len(q), 1), MATCH_DTYPE)
        self.lib.or_match(_p(q), len(q), _p(t), len(t), _p(out))
        return out[:len(q)].copy()

    def remove_outliers(self, m, thr=20):
        m = np.ascontiguousarray(m, MATCH_DTYPE)
        out = np.zeros(max(len(m), 1), MATCH_DTYPE)
        n = _I()
        self.lib.or_remove_outliers(_p(m), len(m), thr, _p(out), ctypes.byref(n))
        return out[:n.value].copy()

    def parse_calib(self, s):
        out = np.zeros(16, np.float64)
        nv = self.lib.or_parse_calib_string(s.encode(), _p(out))
        return out.reshape(4, 4), nv

    # ---- geometry ----
    def cv_svd(self, A):
        A = np.ascontiguousarray(A, np.float64)
        n = A.shape[0]
        w = np.zeros(n)
        u = np.zeros((n, n))
        vt = np.zeros((n, n))
        self.lib.or_cv_svd(_p(A), n, _p(w), _p(u), _p(vt))
        return w, u, vt

    def fundamental(self, pts):
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 4)
        F = np.zeros(9)
        ok = self.lib.or_fundamental_8pt(_p(pts), len(pts), _p(F))
        return bool(ok), F.reshape(3, 3)

    def mt19937(self, seed):
        """A persistent std::mt19937(seed): .uniform_ints(a, b, count) draws uniform_int_distribution<int>(a, b)."""
        lib = self.lib

        class _MT:
            def __init__(self):
                self.h = lib.or_mt19937_new(seed)

            def uniform_ints(self, a, b, count):
                out = np.zeros(count, np.int32)
                lib.or_mt19937_uniform_ints(self.h, a, b, count, _p(out))
                return out

            def __del__(self):
                if self.h:
                    lib.or_mt19937_free(self.h)
                    self.h = None
        return _MT()

    def f_ransac(self, matches, samples, thr=0.1):
        m = np.ascontiguousarray(matches, MATCH_DTYPE)
        smp = np.ascontiguousarray(samples, np.int32).reshape(-1, 8)
        F = np.zeros(9)
        mi = _I()
        ok = self.lib.or_f_ransac(_p(m), len(m), _p(smp), len(smp), thr, _p(F), ctypes.byref(mi))
        return bool(ok), F.reshape(3, 3), mi.value

    def eigen_svd(self, A):
        Acm = np.ascontiguousarray(np.asarray(A, np.float64).T)  # column-major
        n = Acm.shape[0]
        sv = np.zeros(n)
        V = np.zeros(n * n)
        ok = self.lib.or_eigen_jacobi_svd(_p(Acm), n, _p(sv), _p(V))
        return bool(ok), sv, V.reshape(n, n).T

    def triangulate_matches(self, Ta, Tb, K, matches):
        Ta = np.ascontiguousarray(Ta, np.float64)
        Tb = np.ascontiguousarray(Tb, np.float64)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        m = np.ascontiguousarray(matches, MATCH_DTYPE)
        X = np.zeros((max(len(m), 1), 3))
        ok = np.zeros(max(len(m), 1), np.uint8)
        n = self.lib.or_triangulate_matches(_p(Ta), _p(Tb), _p(K), _p(m), len(m), _p(X), _p(ok))
        return n, X[:len(m)], ok[:len(m)].astype(bool)

    def se3_exp(self, a):
        a = np.ascontiguousarray(a, np.float64)
        out = np.zeros(7)
        self.lib.or_se3_exp(_p(a), _p(out))
        return out

    def se3_mul(self, A, B):
        A = np.ascontiguousarray(A, np.float64)
        B = np.ascontiguousarray(B, np.float64)
        out = np.zeros(7)
        self.lib.or_se3_mul(_p(A), _p(B), _p(out))
        return out

    def se3_inverse(self, T):
        T = np.ascontiguousarray(T, np.float64)
        out = np.zeros(7)
        self.lib.or_se3_inverse(_p(T), _p(out))
        return out

    def se3_from_Rt(self, R, t):
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        out = np.zeros(7)
        self.lib.or_se3_from_Rt(_p(R), _p(t), _p(out))
        return out

    def se3_act(self, T, p):
        T = np.ascontiguousarray(T, np.float64)
        p = np.ascontiguousarray(p, np.float64)
        out = np.zeros(3)
        self.lib.or_se3_act(_p(T), _p(p), _p(out))
        return out

    def quat_to_R(self, q):
        q = np.ascontiguousarray(q, np.float64)
        R = np.zeros(9)
        self.lib.or_quat_to_R(_p(q), _p(R))
        return R.reshape(3, 3)

    def world2camera(self, X, T, K):
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        T = np.ascontiguousarray(T, np.float64)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        out = np.zeros_like(X)
        self.lib.or_world2camera(_p(X), len(X), _p(T), _p(K), _p(out))
        return out

    def ldlt6(self, H, b, variant=0):
        H = np.ascontiguousarray(H, np.float64).reshape(36)
        b = np.ascontiguousarray(b, np.float64)
        x = np.zeros(6)
        pos = self.lib.or_ldlt6_solve(_p(H), _p(b), _p(x), variant)
        return bool(pos), x

    def pose_lm(self, X, uv, K, pose, sum_mode=0):
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        T = np.array(pose, np.float64).copy()
        out = np.zeros(max(len(X), 1), np.uint8)
        inl = self.lib.or_pose_lm(_p(X), _p(uv), len(X), _p(K), _p(T), _p(out), sum_mode)
        return T, out[:len(X)].astype(bool), inl

    def pose_gn(self, X, uv, K, pose, sum_mode=0):
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        T = np.array(pose, np.float64).copy()
        it = self.lib.or_pose_gn(_p(X), _p(uv), len(X), _p(K), _p(T), sum_mode)
        return T, it

    LM_TRACE_FIELDS = ("active", "iters", "accepted", "rejected", "not_positive", "chi_nonfinite", "end",
                       "last_rejected", "huber", "literal", "replay", "ldlt_k0", "ldlt_zero_pivot", "ldlt_signs",
                       "ldlt_zeroed", "ldlt_pivoted", "literal_waves")

    def ldlt6_ex(self, H, b, variant=0):
        """-> (positive, x, trace dict: tr (the six transpositions), sign, k0_exit, zero_pivots (at k > 0), zeroed (solve
        entries the > DBL_MIN test set to 0))."""
        H = np.ascontiguousarray(H, np.float64).reshape(36)
        b = np.ascontiguousarray(b, np.float64)
        x = np.zeros(6)
        tr = np.zeros(10, np.int32)
        pos = self.lib.or_ldlt6_solve_ex(_p(H), _p(b), _p(x), variant, _p(tr))
        return bool(pos), x, dict(tr=tuple(int(v) for v in tr[:6]), sign=int(tr[6]), k0_exit=int(tr[7]),
                                  zero_pivots=int(tr[8]), zeroed=int(tr[9]))

    def pose_lm_ex(self, X, uv, K, pose, sum_mode=0):
        """-> (pose, outlier flags, inliers, one trace dict per round with LM_TRACE_FIELDS; oracle/yavo_oracle.h)."""
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        T = np.array(pose, np.float64).copy()
        out = np.zeros(max(len(X), 1), np.uint8)
        tr = np.zeros((4, len(self.LM_TRACE_FIELDS)), np.int32)
        inl = self.lib.or_pose_lm_ex(_p(X), _p(uv), len(X), _p(K), _p(T), _p(out), sum_mode, _p(tr))
        return T, out[:len(X)].astype(bool), inl, [dict(zip(self.LM_TRACE_FIELDS, map(int, r))) for r in tr]

    def pose_gn_ex(self, X, uv, K, pose, sum_mode=0):
        """-> (pose, accepted iterations, trace dict: stop [10] (-1 not run, 0 continued, 1 isnan(dx[0]), 2 cost increase,
        3 |dx| < 1e-6), sign [10], ldlt [10] (bit 1: k == 0 exit, bit 2: zero pivot at k > 0), plane [10] (-1 no point
        with pc_z == 0, else bit 1: one off the optical axis, bit 2: one at the camera centre))."""
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        T = np.array(pose, np.float64).copy()
        tr = np.zeros(40, np.int32)
        it = self.lib.or_pose_gn_ex(_p(X), _p(uv), len(X), _p(K), _p(T), sum_mode, _p(tr))
        return T, it, dict(stop=tr[:10].tolist(), sign=tr[10:20].tolist(), ldlt=tr[20:30].tolist(), plane=tr[30:].tolist())

    # ---- cv::calcOpticalFlowPyrLK ----
    def pyr_down(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        H, W = img.shape
        out = np.zeros(((H + 1) // 2, (W + 1) // 2), np.uint8)
        self.lib.or_pyr_down(_p(img), H, W, W, _p(out))
        return out

    def scharr(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        H, W = img.shape
        out = np.zeros((H, W, 2), np.int16)
        self.lib.or_scharr(_p(img), H, W, W, _p(out))
        return out

    # the exits of one point at one pyramid level (OR_LK_* in oracle/yavo_oracle.h)
    LK_NOT_RUN, LK_WINDOW_OUTSIDE, LK_MIN_EIG, LK_DET, LK_LEFT_IMAGE, LK_EPS, LK_OSCILLATION, LK_MAX_COUNT, \
        LK_ERR_OUTSIDE = range(9)
    LK_TRACE_LEVELS = 8

    def lk(self, prev, nxt, pts, win=11, max_level=3, max_count=30, eps=0.01, min_eig=0.001, sum_mode=0, trace=False):
        """-> (next_pts [n, 2] (x = col, y = row), status [n] bool, err [n], top level used); with trace=True a fifth
        item, the dict {exit [n, 8] (LK_* per pyramid level, LK_NOT_RUN above the top level), steps [n, 8] (Newton
        steps taken)} of or_lk_pyr_ex."""
        prev = np.ascontiguousarray(prev, np.uint8)
        nxt = np.ascontiguousarray(nxt, np.uint8)
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        H, W = prev.shape
        nextp = np.zeros_like(pts)
        status = np.zeros(max(len(pts), 1), np.uint8)
        err = np.zeros(max(len(pts), 1), np.float32)
        args = (_p(prev), _p(nxt), H, W, _p(pts), len(pts), win, max_level, max_count, eps, min_eig, _p(nextp),
                _p(status), _p(err), sum_mode)
        if not trace:
            lv = self.lib.or_lk_pyr(*args)
            return nextp, status[:len(pts)].astype(bool), err[:len(pts)], lv
        tr = np.zeros((max(len(pts), 1), self.LK_TRACE_LEVELS, 2), np.int32)
        lv = self.lib.or_lk_pyr_ex(*args, _p(tr))
        tr = tr[:len(pts)]
        return nextp, status[:len(pts)].astype(bool), err[:len(pts)], lv, dict(exit=tr[:, :, 0].copy(),
                                                                                  steps=tr[:, :, 1].copy())

    # ---- findEssentialMat / recoverPose ----
    def em_subsets(self, count, iters):
        idx = np.zeros((iters, 5), np.int32)
        self.lib.or_em_subsets(count, iters, _p(idx))
        return idx

    def em_kernel(self, q1, q2):
        q1 = np.ascontiguousarray(q1, np.float64).reshape(5, 2)
        q2 = np.ascontiguousarray(q2, np.float64).reshape(5, 2)
        models = np.zeros((10, 9), np.float64)
        n = self.lib.or_em_kernel(_p(q1), _p(q2), _p(models))
        return models[:n].reshape(-1, 3, 3)

    def solve_poly(self, c, max_iters=300):
        c = np.ascontiguousarray(c, np.float64)
        roots = np.zeros((len(c) - 1, 2), np.float64)
        it = self.lib.or_solve_poly(_p(c), len(c) - 1, max_iters, _p(roots))
        return roots[:, 0] + 1j * roots[:, 1], it

    def em_kernel_ex(self, q1, q2):
        """-> (models [10, 9] (zeros past the count), count, trace dict: singular (first singular LU pivot index + 1, or
        0), degree, sweeps, skips, complex, solvez)."""
        q1 = np.ascontiguousarray(q1, np.float64).reshape(5, 2)
        q2 = np.ascontiguousarray(q2, np.float64).reshape(5, 2)
        models = np.zeros((10, 9), np.float64)
        tr = np.zeros(6, np.int32)
        n = self.lib.or_em_kernel_ex(_p(q1), _p(q2), _p(models), _p(tr))
        return models, n, dict(zip(("singular", "degree", "sweeps", "skips", "complex", "solvez"), map(int, tr)))

    def solve_poly_ex(self, c, max_iters=300):
        """-> (roots [n0, 2] (re, im; zeros past the trimmed degree), trace dict: degree, sweeps, skips)."""
        c = np.ascontiguousarray(c, np.float64)
        roots = np.zeros((len(c) - 1, 2), np.float64)
        tr = np.zeros(3, np.int32)
        self.lib.or_solve_poly_ex(_p(c), len(c) - 1, max_iters, _p(roots), _p(tr))
        return roots, dict(zip(("degree", "sweeps", "skips"), map(int, tr)))

    def find_essential(self, pts1, pts2, focal=718.856, pp=(607.1928, 185.2157), prob=0.999, threshold=1.0,
                       max_iters=1000):
        """-> (ok, E [3, 3], mask [n] bool, stats {iters, models, best})."""
        p1 = np.ascontiguousarray(pts1, np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts2, np.float64).reshape(-1, 2)
        n = len(p1)
        E = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        st = np.zeros(3, np.int32)
        ok = self.lib.or_find_essential(_p(p1), _p(p2), n, focal, pp[0], pp[1], prob, threshold, max_iters, _p(E),
                                        _p(mask), _p(st))
        return bool(ok), E.reshape(3, 3), mask[:n].astype(bool), dict(iters=int(st[0]), models=int(st[1]),
                                                                        best=int(st[2]))

    def recover_pose(self, E, pts1, pts2, K):
        """-> (good, R [3, 3], t [3], good per candidate [4])."""
        E = np.ascontiguousarray(E, np.float64).reshape(9)
        p1 = np.ascontiguousarray(pts1, np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts2, np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        R = np.zeros(9, np.float64)
        t = np.zeros(3, np.float64)
        g = np.zeros(4, np.int32)
        good = self.lib.or_recover_pose(_p(E), _p(p1), _p(p2), len(p1), _p(K), _p(R), _p(t), _p(g))
        return good, R.reshape(3, 3), t, g

    # ---- sliding-window BA (BASELINE config 5) ----
    def ldlt_solve(self, H, b):
        H = np.ascontiguousarray(H, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        x = np.zeros_like(b)
        pos = self.lib.or_ldlt_solve(_p(H), len(b), _p(b), _p(x))
        return x, bool(pos)

    def ba_lm(self, poses, n_fixed, X, ep, el, meas, K, max_iters=10, mode=0):
        """-> (poses [P, 7], X [L, 3], iterations, chi2 log). mode 0: the kernel's summation order (bit-exact with
        yv_ba); 1: g2o's own loop orders (BlockSolver::buildSystem / solve, activeRobustChi2, computeScale)."""
        T = np.ascontiguousarray(poses, np.float64).copy()
        Xo = np.ascontiguousarray(X, np.float64).copy()
        ep = np.ascontiguousarray(ep, np.int32)
        el = np.ascontiguousarray(el, np.int32)
        meas = np.ascontiguousarray(meas, np.float64)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        log = np.zeros(max_iters + 1)
        it = self.lib.or_ba_lm_mode(_p(T), len(T), n_fixed, _p(Xo), len(Xo), _p(ep), _p(el), _p(meas), len(ep),
                                    _p(K), max_iters, _p(log), int(mode))
        return T, Xo, it, log[:it + 1]

    # yv_ba_debug_read's buffer order (or_ba_dump[which]); H_pl, W and Dinv exist in the oracle only
    BA_STAGES = ("err", "J_pose", "J_point", "H_pl", "W", "H_pp", "b_p", "H_ll", "b_l", "Dinv", "S", "b_schur", "x_p",
                 "x_l", "poses", "X")

    def ba_lm_trials(self, poses, n_fixed, X, ep, el, meas, K, max_iters=10, mode=0):
        """ba_lm with the trial log (or_ba_trial_log) -> (poses, X, iterations, chi2 log, trials [iterations, 4]); a
        trials row is (q = trials run, trials whose LDLT was not positive, trials with a NaN rho, the stop reason: 0
        none, bits 1 q == 10, 2 rho == 0, 4 non-finite lambda)."""
        trials = np.zeros((max(max_iters, 1), 4), np.int32)
        log_p = ctypes.c_void_p.in_dll(self.lib, "or_ba_trial_log")
        cap = ctypes.c_int.in_dll(self.lib, "or_ba_trial_cap")
        log_p.value, cap.value = trials.ctypes.data, max_iters
        try:
            T, Xo, it, log = self.ba_lm(poses, n_fixed, X, ep, el, meas, K, max_iters, mode)
        finally:
            log_p.value, cap.value = None, 0
        return T, Xo, it, log, trials[:it]

    def ba_dump(self, poses, n_fixed, X, ep, el, meas, K, dump_iter=0, mode=0):
        """The buffers of iteration dump_iter's first damping trial (or_ba_dump; S before its factorisation) as a
        dict by BA_STAGES name; the oracle runs dump_iter + 1 iterations. The solve never writes the H_pp / b_p
        rows of fixed poses: compare the free poses' rows only."""
        P, L, E = len(poses), len(X), len(ep)
        ns = 6 * (P - n_fixed)
        sizes = (2 * E, 12 * E, 6 * E, 18 * E, 18 * E, 36 * P, 6 * P, 9 * L, 3 * L, 9 * L, ns * ns, ns, ns, 3 * L,
                 7 * P, 3 * L)
        bufs = [np.full(max(n, 1), np.nan) for n in sizes]
        slots = (ctypes.c_void_p * 16).in_dll(self.lib, "or_ba_dump")
        which = ctypes.c_int.in_dll(self.lib, "or_ba_dump_iter")
        for i, b in enumerate(bufs):
            slots[i] = b.ctypes.data
        which.value = dump_iter
        try:
            self.ba_lm(poses, n_fixed, X, ep, el, meas, K, dump_iter + 1, mode)
        finally:
            which.value = -1
            for i in range(16):
                slots[i] = None
        return {name: b[:n] for name, b, n in zip(self.BA_STAGES, bufs, sizes)}

    # ---- shared map blocks (include/yavo/yavo_map.h) ----
    def map_block_bytes(self, max_kf, lm_stride):
        return int(self.lib.or_map_block_bytes(max_kf, lm_stride))

    def map_chunk(self, rel, first_frame, kf_every, edge_count, edge_X, edge_outlier, max_kp, max_kf):
        """-> uint8 block. rel [n, 7]; edge_count [n]; edge_X [n, max_kp, 3]; edge_outlier [n, max_kp]."""
        rel = np.ascontiguousarray(rel, np.float64).reshape(-1, 7)
        n = len(rel)
        ec = np.ascontiguousarray(edge_count, np.int32)
        eX = np.ascontiguousarray(edge_X, np.float64).reshape(n, max_kp, 3)
        eo = np.ascontiguousarray(edge_outlier, np.uint8).reshape(n, max_kp)
        out = np.zeros(self.map_block_bytes(max_kf, max_kp), np.uint8)
        self.lib.or_map_chunk(_p(rel), n, first_frame, kf_every, _p(ec), _p(eX), _p(eo), max_kp, max_kf, _p(out))
        return out

    def map_place(self, blocks, world, block_bytes, base):
        """-> (placed blocks, new base, anchors [world, 7]); blocks = world blocks back to back (copied)."""
        b = np.ascontiguousarray(blocks, np.uint8).reshape(-1).copy()
        base = np.ascontiguousarray(base, np.float64).copy()
        anchors = np.zeros((world, 7))
        self.lib.or_map_place(_p(b), world, block_bytes, _p(base), _p(anchors))
        return b, base, anchors
