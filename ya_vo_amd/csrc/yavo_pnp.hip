// yavo_pnp.hip -- gfx950 kernels of the P3P-RANSAC absolute pose (yv_pnp_ransac / yv_pnp_ransac_batch and the batch's
// track RANSAC, include/yavo/yavo_geom.h): a pose from 3D-2D edges without a prior, and its inlier mask.  Not a row of the
// reference (it has no solvePnPRansac); the specification is tests/pnp_ransac_reference.py, and every floating-point
// expression here is written in that file's operation order (the file is built with -ffp-contract=off; / and sqrt are
// the correctly rounded ones), so the results equal it bit for bit.
//
//   pnp_hyp_kernel     one lane per hypothesis, 64 per workgroup: its three sampled edges -> Grunert's quartic ->
//                      Durand-Kerner (a fixed number of sweeps: no lane can spin) -> up to 4 poses, one slot per root
//   pnp_count_kernel   one wave per candidate pose (the pose wave-uniform in SGPRs), lanes over the problem's edges:
//                      one ballot + popcount per 64 edges.  Exact integer counts, so any partition of the edges gives
//                      the same totals.  A form with the edges stationary in registers (1024 per workgroup, looping
//                      over the candidates) re-reads no edge but was slower at the bench's shape: 2.12 against
//                      1.45 ms per launch; a problem's edges are 80 KB and stay in L2
//   pnp_select_kernel  one workgroup per problem: the most inliers, then the first candidate in (hypothesis, root)
//                      order; found iff the count reaches min_inliers; the pose, the count and the mask
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "yavo_internal.h"
#include "yavo_edge.h"
#include "yavo_geom_dev.h"
#include "yavo_se3.h"

namespace yavo {
namespace geom {

constexpr int kPnpSweeps = 40;       // Durand-Kerner sweeps (pnp_ransac_reference.kSweeps)
constexpr int kPnpMaxEdges = 4096;   // a problem's first 4096 edges, as the pose LM
constexpr int kPnpHypWG = 64;
constexpr int kPnpNT = 256;          // count and select workgroups

// problem p's edges: [offsets[p], offsets[p + 1]) or, with counts, counts[p] edges from p * stride (the track layout)
struct PnpProblem {
    int64_t e0;
    int n;
};

__device__ __forceinline__ PnpProblem pnp_problem(const int32_t* __restrict__ offsets,
                                                  const int32_t* __restrict__ counts, int stride, int p) {
    PnpProblem r;
    r.e0 = counts ? (int64_t)p * stride : (int64_t)offsets[p];
    int n = counts ? counts[p] : (int)(offsets[p + 1] - r.e0);
    if (counts && n > stride) n = stride;
    if (n > kPnpMaxEdges) n = kPnpMaxEdges;
    r.n = n < 0 ? 0 : n;
    return r;
}

__device__ __forceinline__ double pnp_dot(const double* a, const double* b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

__device__ __forceinline__ double pnp_dist2(const double* A, const double* B) {
    const double dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];
    return dx * dx + dy * dy + dz * dz;
}

// e1 = (B - A) / |B - A|, e3 = (e1 x (C - A)) / |.|, e2 = e3 x e1
__device__ __forceinline__ void pnp_frame(const double* A, const double* B, const double* C, double* e1, double* e2,
                                          double* e3) {
    const double d[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const double n1 = sqrt(pnp_dot(d, d));
    e1[0] = d[0] / n1;
    e1[1] = d[1] / n1;
    e1[2] = d[2] / n1;
    const double g[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    const double c[3] = {e1[1] * g[2] - e1[2] * g[1], e1[2] * g[0] - e1[0] * g[2], e1[0] * g[1] - e1[1] * g[0]};
    const double n3 = sqrt(pnp_dot(c, c));
    e3[0] = c[0] / n3;
    e3[1] = c[1] / n3;
    e3[2] = c[2] / n3;
    e2[0] = e3[1] * e1[2] - e3[2] * e1[1];
    e2[1] = e3[2] * e1[0] - e3[0] * e1[2];
    e2[2] = e3[0] * e1[1] - e3[1] * e1[0];
}

// the largest-diagonal branch of Eigen's quaternion from a rotation matrix with the diagonal index I fixed
template <int I>
__device__ __forceinline__ void pnp_quat_diag(const double* R, double* q) {
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double tr = sqrt(R[4 * I] - R[4 * J] - R[4 * K] + 1.0);
    q[I] = 0.5 * tr;
    tr = 0.5 / tr;
    q[3] = (R[3 * K + J] - R[3 * J + K]) * tr;
    q[J] = (R[3 * J + I] + R[3 * I + J]) * tr;
    q[K] = (R[3 * K + I] + R[3 * I + K]) * tr;
}

// or_se3_from_Rt's quaternion of R (row-major), divided by its norm in or_se3_inverse's summation order
__device__ __forceinline__ void pnp_quat_from_R(const double* R, double* q) {
    double tr = (R[0] + R[4]) + R[8];
    if (tr > 0.0) {
        tr = sqrt(tr + 1.0);
        q[3] = 0.5 * tr;
        tr = 0.5 / tr;
        q[0] = (R[7] - R[5]) * tr;
        q[1] = (R[2] - R[6]) * tr;
        q[2] = (R[3] - R[1]) * tr;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i ? R[4] : R[0])) i = 2;
        if (i == 0) pnp_quat_diag<0>(R, q);
        else if (i == 1) pnp_quat_diag<1>(R, q);
        else pnp_quat_diag<2>(R, q);
    }
    const double len = sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]));
    q[0] = q[0] / len;
    q[1] = q[1] / len;
    q[2] = q[2] / len;
    q[3] = q[3] / len;
}

// Durand-Kerner on x^4 + c[3] x^3 + c[2] x^2 + c[1] x + c[0], complex arithmetic in real operations (the shape of
// yavo_essential.hip's dk_solve): kPnpSweeps Gauss-Seidel sweeps from (0.4 + 0.9i)^k, no data-dependent stop
__device__ __forceinline__ void pnp_dk_quartic(const double* c, double* xr, double* xi) {
    {
        double pr = 1.0, pi = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xr[i] = pr;
            xi[i] = pi;
            const double tr = pr * 0.4 - pi * 0.9, ti = pr * 0.9 + pi * 0.4;
            pr = tr;
            pi = ti;
        }
    }
    for (int sweep = 0; sweep < kPnpSweeps; ++sweep) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double pr = xr[i], pi = xi[i];
            double nr = pr + c[3], ni = pi;
#pragma unroll
            for (int k = 2; k >= 0; --k) {
                const double tr = nr * pr - ni * pi, ti = nr * pi + ni * pr;
                nr = tr + c[k];
                ni = ti;
            }
            double dr = 0.0, di = 0.0;
            bool first = true;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j == i) continue;
                const double sr = pr - xr[j], si = pi - xi[j];
                if (first) {
                    dr = sr;
                    di = si;
                    first = false;
                } else {
                    const double ur = dr * sr - di * si, ui = dr * si + di * sr;
                    dr = ur;
                    di = ui;
                }
            }
            const double t = 1.0 / (dr * dr + di * di);
            const double qr = (nr * dr + ni * di) * t, qi = (ni * dr - nr * di) * t;
            xr[i] = pr - qr;
            xi[i] = pi - qi;
        }
    }
}

// One hypothesis: the edges d[k] % n of (X, uv) -> up to 4 poses at out[root][7]; returns the mask of the roots that
// gave one.  Every test is written !(x > 0), so a NaN falls out.
__device__ int pnp_hypothesis(const double* __restrict__ X, const double* __restrict__ uv, int n, const double* K,
                              const uint32_t* __restrict__ d, double* __restrict__ out) {
    if (n <= 0) return 0;
    const int i0 = (int)(d[0] % (uint32_t)n), i1 = (int)(d[1] % (uint32_t)n), i2 = (int)(d[2] % (uint32_t)n);
    if (i0 == i1 || i0 == i2 || i1 == i2) return 0;
    const int idx[3] = {i0, i1, i2};
    double P[3][3], J[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[k][0] = X[3 * idx[k]];
        P[k][1] = X[3 * idx[k] + 1];
        P[k][2] = X[3 * idx[k] + 2];
        const double x = (uv[2 * idx[k]] - K[2]) / K[0];
        const double y = (uv[2 * idx[k] + 1] - K[5]) / K[4];
        const double nn = sqrt(x * x + y * y + 1.0);
        J[k][0] = x / nn;
        J[k][1] = y / nn;
        J[k][2] = 1.0 / nn;
    }
    const double a2 = pnp_dist2(P[1], P[2]), b2 = pnp_dist2(P[0], P[2]), c2 = pnp_dist2(P[0], P[1]);
    if (!(b2 > 0.0)) return 0;
    const double ca = pnp_dot(J[1], J[2]), cb = pnp_dot(J[0], J[2]), cg = pnp_dot(J[0], J[1]);
    const double q = (a2 - c2) / b2, p = (a2 + c2) / b2;
    const double rab = a2 / b2, rcb = c2 / b2;
    const double ca2 = ca * ca, cb2 = cb * cb, cg2 = cg * cg;
    const double A4 = (q - 1.0) * (q - 1.0) - 4.0 * rcb * ca2;
    const double A3 = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * rcb * ca2 * cb);
    const double A2 = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb2 + 2.0 * ((b2 - c2) / b2) * ca2 - 4.0 * p * ca * cb * cg +
                             2.0 * ((b2 - a2) / b2) * cg2);
    const double A1 = 4.0 * (-q * (1.0 + q) * cb + 2.0 * rab * cg2 * cb - (1.0 - p) * ca * cg);
    const double A0 = (1.0 + q) * (1.0 + q) - 4.0 * rab * cg2;
    if (!(fabs(A4) > 0.0)) return 0;
    const double c[4] = {A0 / A4, A1 / A4, A2 / A4, A3 / A4};
    double re[4], im[4];
    pnp_dk_quartic(c, re, im);
    double w1[3], w2[3], w3[3];
    pnp_frame(P[0], P[1], P[2], w1, w2, w3);
    int mask = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double v = re[r];
        if (!(fabs(im[r]) <= 1e-7 * (1.0 + fabs(v)))) continue;
        if (!(v > 0.0)) continue;
        const double du = 2.0 * (cg - v * ca);
        if (!(fabs(du) > 0.0)) continue;
        const double u = ((q - 1.0) * v * v - 2.0 * q * cb * v + 1.0 + q) / du;
        if (!(u > 0.0)) continue;
        const double ds = 1.0 + v * v - 2.0 * v * cb;
        if (!(ds > 0.0)) continue;
        const double s1 = sqrt(b2 / ds), s2 = u * s1, s3 = v * s1;
        const double Q1[3] = {s1 * J[0][0], s1 * J[0][1], s1 * J[0][2]};
        const double Q2[3] = {s2 * J[1][0], s2 * J[1][1], s2 * J[1][2]};
        const double Q3[3] = {s3 * J[2][0], s3 * J[2][1], s3 * J[2][2]};
        double k1[3], k2[3], k3[3];
        pnp_frame(Q1, Q2, Q3, k1, k2, k3);
        double R[9], T[7];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) R[3 * a + b] = k1[a] * w1[b] + k2[a] * w2[b] + k3[a] * w3[b];
#pragma unroll
        for (int a = 0; a < 3; ++a)
            T[4 + a] = Q1[a] - (R[3 * a] * P[0][0] + R[3 * a + 1] * P[0][1] + R[3 * a + 2] * P[0][2]);
        pnp_quat_from_R(R, T);
        bool fin = true;
#pragma unroll
        for (int a = 0; a < 9; ++a) fin = fin && isfinite(R[a]);
#pragma unroll
        for (int a = 0; a < 7; ++a) fin = fin && isfinite(T[a]);
        if (!fin) continue;
#pragma unroll
        for (int a = 0; a < 7; ++a) out[7 * r + a] = T[a];
        mask |= 1 << r;
    }
    return mask;
}

// what the pose LM's own edge says about pose T: camera-frame z > 0 and |e|^2 < thr^2
__device__ __forceinline__ bool pnp_inlier(const double* T, const double* K, const double* X, const double* m,
                                           double thr2) {
    double pc[3], e[2];
    se3::se3_act(T, X, pc);
    edge::edge_error_pc(pc, K, m, e);
    return pc[2] > 0.0 && e[0] * e[0] + e[1] * e[1] < thr2;
}

__global__ __launch_bounds__(kPnpHypWG) void pnp_hyp_kernel(const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ counts, int stride,
                                                            const double* __restrict__ Xall,
                                                            const double* __restrict__ uvall,
                                                            const double* __restrict__ Kall,
                                                            const uint32_t* __restrict__ draws, int iters,
                                                            double* __restrict__ ws_pose, int32_t* __restrict__ ws_cnt,
                                                            int32_t* __restrict__ ws_valid) {
    const int p = blockIdx.y;
    const int h = blockIdx.x * kPnpHypWG + threadIdx.x;
    if (h >= iters) return;  // no barriers below: lanes leave independently
    const PnpProblem pr = pnp_problem(offsets, counts, stride, p);
    const int64_t slot = (int64_t)p * iters + h;
    double K[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) K[q] = Kall[9 * (int64_t)p + q];
#pragma unroll
    for (int r = 0; r < 4; ++r) ws_cnt[4 * slot + r] = 0;
    ws_valid[slot] = pnp_hypothesis(Xall + 3 * pr.e0, uvall + 2 * pr.e0, pr.n, K, draws + 3 * (int64_t)h,
                                    ws_pose + 28 * slot);
}

__global__ __launch_bounds__(kPnpNT) void pnp_count_kernel(const int32_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ counts, int stride,
                                                           const double* __restrict__ Xall,
                                                           const double* __restrict__ uvall,
                                                           const double* __restrict__ Kall, int iters, double thr,
                                                           const double* __restrict__ ws_pose,
                                                           const int32_t* __restrict__ ws_valid,
                                                           int32_t* __restrict__ ws_cnt) {
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int c = blockIdx.x * (kPnpNT / 64) + (threadIdx.x >> 6);  // this wave's candidate: 4 h + root
    const PnpProblem pr = pnp_problem(offsets, counts, stride, p);
    const int nc = 4 * iters;
    if (c >= nc) return;  // no barriers below: waves leave independently
    if (!((ws_valid[(int64_t)p * iters + (c >> 2)] >> (c & 3)) & 1)) return;  // no pose in this slot (its count stays 0)
    double K[9], T[7];
#pragma unroll
    for (int q = 0; q < 9; ++q) K[q] = uni_f64(Kall[9 * (int64_t)p + q]);
#pragma unroll
    for (int q = 0; q < 7; ++q) T[q] = uni_f64(ws_pose[7 * ((int64_t)p * nc + c) + q]);  // wave-uniform: in SGPRs
    const double* X = Xall + 3 * pr.e0;
    const double* uv = uvall + 2 * pr.e0;
    const double thr2 = thr * thr;
    int cnt = 0;
    for (int k = lane; k < pr.n; k += 64) cnt += __popcll(__ballot(pnp_inlier(T, K, X + 3 * k, uv + 2 * k, thr2)));
    if (lane == 0) ws_cnt[(int64_t)p * nc + c] = cnt;
}

// init (optional, [p][7]): what poses[p] becomes when nothing is found (the track's prior from the caller);
// nullptr leaves poses[p] untouched.  init and poses may be the same buffer.
__global__ __launch_bounds__(kPnpNT) void pnp_select_kernel(const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ counts, int stride,
                                                            const double* __restrict__ Xall,
                                                            const double* __restrict__ uvall,
                                                            const double* __restrict__ Kall, int iters, double thr,
                                                            int min_inliers, const double* __restrict__ ws_pose,
                                                            const int32_t* __restrict__ ws_valid,
                                                            const int32_t* __restrict__ ws_cnt, const double* init,
                                                            double* poses, uint8_t* __restrict__ inlier,
                                                            int32_t* __restrict__ inliers,
                                                            int32_t* __restrict__ found) {
    __shared__ int s_bc[kPnpNT / 64], s_bi[kPnpNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PnpProblem pr = pnp_problem(offsets, counts, stride, p);
    const int nc = 4 * iters;
    // (count, -candidate) lexicographic maximum: candidates in (hypothesis, root) order, strict '>' keeps the first
    int bc = -1, bi = 0x7fffffff;
    for (int c = tid; c < nc; c += kPnpNT) {
        if (!((ws_valid[(int64_t)p * iters + (c >> 2)] >> (c & 3)) & 1)) continue;
        const int v = ws_cnt[(int64_t)p * nc + c];
        if (v > bc) {  // c increases within a thread
            bc = v;
            bi = c;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int oc = __shfl_xor(bc, off, 64), oi = __shfl_xor(bi, off, 64);
        if (oc > bc || (oc == bc && oi < bi)) {
            bc = oc;
            bi = oi;
        }
    }
    if (lane == 0) {
        s_bc[wave] = bc;
        s_bi[wave] = bi;
    }
    __syncthreads();
    bc = s_bc[0];
    bi = s_bi[0];
#pragma unroll
    for (int w = 1; w < kPnpNT / 64; ++w) {
        const int oc = s_bc[w], oi = s_bi[w];
        if (oc > bc || (oc == bc && oi < bi)) {
            bc = oc;
            bi = oi;
        }
    }
    const bool ok = bc >= 0 && bc >= min_inliers;  // the same in every thread
    double T[7], K[9];
    const double* best = ws_pose + 7 * ((int64_t)p * nc + (ok ? bi : 0));
#pragma unroll
    for (int q = 0; q < 7; ++q) T[q] = ok ? best[q] : 0.0;
#pragma unroll
    for (int q = 0; q < 9; ++q) K[q] = Kall[9 * (int64_t)p + q];
    if (tid < 7) {
        if (ok) poses[7 * (int64_t)p + tid] = T[tid];
        else if (init) poses[7 * (int64_t)p + tid] = init[7 * (int64_t)p + tid];
    }
    if (tid == 0) {
        inliers[p] = ok ? bc : 0;
        found[p] = ok ? 1 : 0;
    }
    const double* X = Xall + 3 * pr.e0;
    const double* uv = uvall + 2 * pr.e0;
    const double thr2 = thr * thr;
    for (int i = tid; i < pr.n; i += kPnpNT)
        inlier[pr.e0 + i] = ok && pnp_inlier(T, K, X + 3 * i, uv + 2 * i, thr2) ? 1 : 0;
}

}  // namespace geom

// ------------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------------
namespace {
constexpr size_t pnp_align(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

size_t pnp_ransac_ws_bytes(int n_problems, int iters) {
    const size_t h = (size_t)std::max(n_problems, 1) * (size_t)std::max(iters, 1);
    return pnp_align(h * 28 * sizeof(double)) + pnp_align(h * 4 * sizeof(int32_t)) + h * sizeof(int32_t);
}

void launch_pnp_ransac(const int32_t* offsets, const int32_t* counts, int stride, int n_problems,
                       const double* X, const double* uv, const double* K, const uint32_t* draws, int iters,
                       double thr, int min_inliers, const double* init, double* poses, uint8_t* inlier,
                       int32_t* inliers, int32_t* found, void* ws, hipStream_t s) {
    if (n_problems <= 0 || iters <= 0) return;
    const size_t h = (size_t)n_problems * (size_t)iters;
    char* w = static_cast<char*>(ws);
    double* ws_pose = reinterpret_cast<double*>(w);
    int32_t* ws_cnt = reinterpret_cast<int32_t*>(w + pnp_align(h * 28 * sizeof(double)));
    int32_t* ws_valid =
        reinterpret_cast<int32_t*>(w + pnp_align(h * 28 * sizeof(double)) + pnp_align(h * 4 * sizeof(int32_t)));
    hipLaunchKernelGGL(geom::pnp_hyp_kernel, dim3((iters + geom::kPnpHypWG - 1) / geom::kPnpHypWG, n_problems),
                       dim3(geom::kPnpHypWG), 0, s, offsets, counts, stride, X, uv, K, draws, iters, ws_pose, ws_cnt,
                       ws_valid);
    hipLaunchKernelGGL(geom::pnp_count_kernel, dim3(iters, n_problems), dim3(geom::kPnpNT), 0, s, offsets, counts,
                       stride, X, uv, K, iters, thr, ws_pose, ws_valid, ws_cnt);  // (kPnpNT / 64 = 4 roots per block)
    hipLaunchKernelGGL(geom::pnp_select_kernel, dim3(n_problems), dim3(geom::kPnpNT), 0, s, offsets, counts, stride, X,
                       uv, K, iters, thr, min_inliers, ws_pose, ws_valid, ws_cnt, init, poses, inlier, inliers, found);
}

}  // namespace yavo
