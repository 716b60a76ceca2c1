// yavo_geom_dev.h -- device functions the geometry kernels (yavo_geom.hip), the pose kernels (yavo_pose.hip) and the
// track kernels (yavo_track.hip) share: the workgroup scan of their compactions, a wave-uniform double in SGPRs and the
// triangulation of one match (Eigen JacobiSVD on the 4x4 DLT system, in registers).  Every floating-point expression is
// written in the reference's operation order; the files are built with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "yavo_se3.h"

namespace yavo {
namespace geom {

using se3::quat_to_R;

constexpr int kNT = 256;          // threads per workgroup of the reduction kernels

// exclusive scan over an NT-thread block; s_tmp >= NT/64 ints
template <int NT = kNT>
__device__ int block_excl_scan_geom(int v, int* s_tmp, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_tmp[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < NT / 64; ++w) {
        if (w < wave) base += s_tmp[w];
        tot += s_tmp[w];
    }
    __syncthreads();
    if (total) *total = tot;
    return base + incl - v;
}

// a wave-uniform double (the value of lane 0) in SGPRs
__device__ __forceinline__ double uni_f64(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// a Jacobi rotation of the SVD below
struct JRot {
    double c, s;
};

__device__ __forceinline__ JRot make_jacobi(double x, double y, double z) {
    JRot r;
    double deno = 2 * fabs(y);
    if (deno < DBL_MIN) {
        r.c = 1; r.s = 0;
        return r;
    }
    double tau = (x - z) / deno;
    double w = sqrt(tau * tau + 1);
    double t = tau > 0 ? 1 / (tau + w) : 1 / (tau - w);
    double sign_t = t > 0 ? 1 : -1;
    double nn = 1 / sqrt(t * t + 1);
    // Eigen's y / |y|: exactly +-1 here (2|y| >= DBL_MIN, and the inputs are finite and scaled to <= 1), so the
    // sign is taken instead of an FP64 division (one of the seven per rotation); the products are unchanged
    r.s = -sign_t * copysign(1.0, y) * fabs(t) * nn;
    r.c = nn;
    return r;
}

// JacobiSVD<MatrixXd>(A 4x4 column-major): sv descending, V column-major.  false on non-finite input.
__device__ inline bool eigen_jacobi_svd4(const double (&Ain)[16], double (&sv)[4], double (&V)[16]) {
    constexpr int n = 4;
    double Wk[16];
    double scale = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        double a = fabs(Ain[i]);
        if (a != a) return false;
        if (a > scale) scale = a;
    }
    if (!isfinite(scale)) return false;
    if (scale == 0) scale = 1;
#pragma unroll
    for (int i = 0; i < 16; ++i) Wk[i] = Ain[i] / scale;
#pragma unroll
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    const double considerAsZero = DBL_MIN, precision = 2 * DBL_EPSILON;
    double maxDiag = 0;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        double a = fabs(Wk[i + i * n]);
        if (a > maxDiag) maxDiag = a;
    }
    bool finished = false;
    int guard = 0;
    while (!finished && guard < 10000) {
        finished = true;
        ++guard;
#pragma unroll
        for (int p = 1; p < n; ++p)
#pragma unroll
            for (int q = 0; q < p; ++q) {
                double threshold = considerAsZero > precision * maxDiag ? considerAsZero : precision * maxDiag;
                if (fabs(Wk[p + q * n]) > threshold || fabs(Wk[q + p * n]) > threshold) {
                    finished = false;
                    // real_2x2_jacobi_svd
                    double m00 = Wk[p + p * n], m01 = Wk[p + q * n], m10 = Wk[q + p * n], m11 = Wk[q + q * n];
                    JRot rot1;
                    double t = m00 + m11;
                    double d = m10 - m01;
                    if (fabs(d) < DBL_MIN) {
                        rot1.s = 0; rot1.c = 1;
                    } else {
                        double u = t / d;
                        double tmp = sqrt(1 + u * u);
                        rot1.s = 1 / tmp;
                        rot1.c = u / tmp;
                    }
                    if (!(rot1.c == 1 && rot1.s == 0)) {
                        double a0 = m00, b0 = m10, a1 = m01, b1 = m11;
                        m00 = rot1.c * a0 + rot1.s * b0;
                        m10 = -rot1.s * a0 + rot1.c * b0;
                        m01 = rot1.c * a1 + rot1.s * b1;
                        m11 = -rot1.s * a1 + rot1.c * b1;
                    }
                    JRot jr = make_jacobi(m00, m01, m11);
                    JRot jl;
                    {
                        const double jtc = jr.c, jts = -jr.s;
                        jl.c = rot1.c * jtc - rot1.s * jts;
                        jl.s = rot1.c * jts + rot1.s * jtc;
                    }
                    // work.applyOnTheLeft(p, q, jl): rows p, q
                    if (!(jl.c == 1 && jl.s == 0)) {
#pragma unroll
                        for (int i = 0; i < n; ++i) {
                            double xi = Wk[p + i * n], yi = Wk[q + i * n];
                            Wk[p + i * n] = jl.c * xi + jl.s * yi;
                            Wk[q + i * n] = -jl.s * xi + jl.c * yi;
                        }
                    }
                    // work.applyOnTheRight(p, q, jr) and V.applyOnTheRight(p, q, jr): rotation by jr^T
                    const double tc = jr.c, ts = -jr.s;
                    if (!(tc == 1 && ts == 0)) {
#pragma unroll
                        for (int i = 0; i < n; ++i) {
                            double xi = Wk[i + p * n], yi = Wk[i + q * n];
                            Wk[i + p * n] = tc * xi + ts * yi;
                            Wk[i + q * n] = -ts * xi + tc * yi;
                        }
#pragma unroll
                        for (int i = 0; i < n; ++i) {
                            double xi = V[i + p * n], yi = V[i + q * n];
                            V[i + p * n] = tc * xi + ts * yi;
                            V[i + q * n] = -ts * xi + tc * yi;
                        }
                    }
                    double aa = fabs(Wk[p + p * n]), bb = fabs(Wk[q + q * n]);
                    double mx = aa > bb ? aa : bb;
                    if (mx > maxDiag) maxDiag = mx;
                }
            }
    }
#pragma unroll
    for (int i = 0; i < n; ++i) sv[i] = fabs(Wk[i + i * n]) * scale;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        int pos = i;
        double mx = sv[i];
#pragma unroll
        for (int k = i + 1; k < n; ++k)
            if (sv[k] > mx) { mx = sv[k]; pos = k; }
        if (mx == 0) break;
        if (pos != i) {
            // swap sv[i] <-> sv[pos] and V columns, static indices only
#pragma unroll
            for (int k = i + 1; k < n; ++k)
                if (k == pos) {
                    double t = sv[i]; sv[i] = sv[k]; sv[k] = t;
#pragma unroll
                    for (int r = 0; r < n; ++r) { t = V[r + k * n]; V[r + k * n] = V[r + i * n]; V[r + i * n] = t; }
                }
        }
    }
    return true;
}

// LoopHandler::triangulation of one match (pixel2camera of both integer pixels, DLT rows, Eigen JacobiSVD);
// returns success (s4/s3 < 1e-2) && Z > 0, the triangulate2View acceptance test (src/LoopHandler.cc:676)
// SUBPIX (yv_stereo_subpix's refinement): the second pixel's column is y2 + dq / 256 (exact in double: |dq| < 2^12 and
// y2 < 2^31 leave the sum inside 53 bits) in place of y2; nothing else changes.
template <bool SUBPIX = false>
__device__ bool triangulate_px(int x1, int y1, int x2, int y2, const double* Ta, const double* Tb,
                               const double* K, double* Xo, int dq = 0) {
    const double K0 = K[0], K2 = K[2], K4 = K[4], K5 = K[5];
    double y2d = (double)y2;
    if constexpr (SUBPIX) y2d = (double)y2 + (double)dq * (1.0 / 256.0);
    const double pa[2] = {((double)x1 - K2) * 1.0 / K0, ((double)y1 - K5) * 1.0 / K4};
    const double pb[2] = {((double)x2 - K2) * 1.0 / K0, (y2d - K5) * 1.0 / K4};
    double A[16];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const double* T = v == 0 ? Ta : Tb;
        const double* pp = v == 0 ? pa : pb;
        double R[9];
        quat_to_R(T, R);
        double mm[12];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            mm[4 * r] = R[3 * r]; mm[4 * r + 1] = R[3 * r + 1]; mm[4 * r + 2] = R[3 * r + 2]; mm[4 * r + 3] = T[4 + r];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            A[(2 * v) + 4 * j] = pp[0] * mm[8 + j] - mm[j];
            A[(2 * v + 1) + 4 * j] = pp[1] * mm[8 + j] - mm[4 + j];
        }
    }
    double sv[4], V[16];
    double X0 = NAN, X1 = NAN, X2 = NAN;
    bool s = false;
    if (eigen_jacobi_svd4(A, sv, V)) {
        X0 = V[0 + 12] / V[3 + 12];
        X1 = V[1 + 12] / V[3 + 12];
        X2 = V[2 + 12] / V[3 + 12];
        s = sv[3] / sv[2] < 1e-2;
    }
    Xo[0] = X0;
    Xo[1] = X1;
    Xo[2] = X2;
    return s && X2 > 0;
}

}  // namespace geom
}  // namespace yavo
