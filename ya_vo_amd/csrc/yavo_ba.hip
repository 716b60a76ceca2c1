// yavo_ba.hip -- gfx950 kernels for the sliding-window bundle adjustment (BASELINE.json config 5):
// g2o's Levenberg-Marquardt over BlockSolver_6_3 with the reference's projection edge (include/Optimizer.hpp:64-126)
// extended to pose-landmark edges, restated like oracle/yavo_oracle_ba.c, expression for expression, in its
// summation orders (built with -ffp-contract=off):
//
//   ba_reduce_kernel      the iteration's linearisation and blocks: H_pp (21) + b_p (6) per free pose in tree4096
//                         order (16 workgroups per pose, each edge's e and J_pose formed on the fly), and one lane per
//                         landmark that linearises its edges -- e, J_pose (the reference's linearizeOplus), J_point =
//                         J_pose[:, :3] R, stored for the later kernels (H_pl = J_pose^T J_point is formed from them
//                         where it is read) -- for H_ll, b_l (sequential over its edges); its last workgroup starts
//                         the iteration's trial loop (device control). (Until round 5 a separate linearisation
//                         kernel stored e / J first: 10.5 us per iteration on a configs[2] window.)
//   ba_schur_kernel       per trial: the reduced pose system S = H_pp + lambda I - sum W H_pl^T and b_schur in tree4096
//                         order (16 workgroups per upper 6 x 6 block or b_schur row), W = H_pl (H_ll + lambda I)^-1
//                         formed per co-visible pair
//   (the reduced system's LDLT and solve run between the two: yavo_ba_ldlt.hip)
//   ba_step_kernel        the trial state: T <- exp(x_p) T, x_l = Dinv (b_l - sum_e H_pl^T x_p), X <- X + x_l (into
//                         the other state buffer), and the trial's chi2 and LM scale x.(lambda x + b) in the
//                         landmark-block order (one lane per landmark); its last workgroup decides the trial (device
//                         control) or leaves both for the host
//   ba_chi2_kernel        the solve's first chi2 in the same order
// The LM control (lambda, rho, accept / reject) runs on the device by default (ba_ctl_*), in the host loop's
// arithmetic; yv_ba_set_control(b, 0) runs it on the host.  The yv_ba C ABI and the host's LM loop are in
// yavo_ba_host.hip, the sliding window that feeds it in yavo_ba_window.hip; kNT, kWG, kWLanes and kTicketGroups, which
// size the host's buffers, are beside BaParams in yavo_internal.h.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "yavo_edge.h"
#include "yavo_internal.h"
#include "yavo_se3.h"

namespace yavo {
namespace ba {

using se3::quat_to_R;
using se3::se3_act;
using se3::se3_exp;
using se3::se3_mul;

using edge::edge_error;
using edge::edge_error_pc;
using edge::edge_jacobian_pc;

// the state (poses, landmarks) the current estimate is in: 0 = P.poses / P.X, 1 = P.poses2 / P.X2
__device__ __forceinline__ int ba_cur(const BaParams& P) { return P.cur ? *P.cur : 0; }

// One edge's linearisation at pose T, point X: the error e = meas - proj(T X), J_pose (the reference's
// linearizeOplus) and J_point = J_pose[:, :3] R. Every reader that needs them forms them with this function, so
// they are the same bits wherever they are formed.
__device__ __forceinline__ void edge_linearize(const double* T, const double* K, const double* X, const double* meas,
                                               double* err, double* Jp, double* Jl) {
    double pc[3];
    se3_act(T, X, pc);
    edge_error_pc(pc, K, meas, err);
    edge_jacobian_pc(pc, K, Jp);
    if (Jl) {
        double R[9];
        quat_to_R(T, R);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                Jl[r * 3 + c] =
                    Jp[r * 6 + 0] * R[0 * 3 + c] + Jp[r * 6 + 1] * R[1 * 3 + c] + Jp[r * 6 + 2] * R[2 * 3 + c];
    }
}

// H_pl(e) = J_pose^T J_point, the expression of the oracle's buildSystem, from the edge's stored Jacobians
__device__ __forceinline__ void hpl_load(const BaParams& P, int64_t e, double* h) {
    double J[12], L[6];
    const double2* jp = reinterpret_cast<const double2*>(P.Jp + 12 * e);
    const double2* jl = reinterpret_cast<const double2*>(P.Jl + 6 * e);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double2 v = jp[i];
        J[2 * i] = v.x;
        J[2 * i + 1] = v.y;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double2 v = jl[i];
        L[2 * i] = v.x;
        L[2 * i + 1] = v.y;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) h[3 * a + c] = J[a] * L[c] + J[6 + a] * L[3 + c];
}

// last-block-done: every workgroup of the launch arrives once; true in the workgroup that arrived last. What the
// last workgroup reads from the others is published write-through (agent-scope atomic stores, or atomics), drained
// (s_waitcnt vmcnt(0) in every storing wave) before the workgroup's barrier and ticket, and read back with agent-scope
// atomic loads: no cache maintenance fences (MI355X guide, Guideline 16's sc1 form). The counter is left at 0 for the
// next launch. Every thread of the workgroup must call it.
__device__ bool ba_last_block(unsigned* ticket) {
    __shared__ unsigned s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = tk == gridDim.x - 1;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = last ? 1u : 0u;
    }
    __syncthreads();
    return s_last != 0;
}

// the same over a large grid: consecutive workgroups in groups of gs = max(16, ceil(grid / 64)), counted per group
// (groups[0 .. 63]); the last of a group counts at *top. Same-address atomics serialise at the cache (a 512-way
// single counter cost ~10 us), so no counter takes more than 64 arrivals.
__device__ bool ba_last_block_h(unsigned* top, unsigned* groups) {
    __shared__ unsigned s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned G = gridDim.x;
        const unsigned gs = max(16u, (G + kTicketGroups - 1) / kTicketGroups);
        const unsigned gi = blockIdx.x / gs, ng = (G + gs - 1) / gs, gsize = min(gs, G - gi * gs);
        bool last = false;
        if (__hip_atomic_fetch_add(&groups[gi], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1) {
            __hip_atomic_store(&groups[gi], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ng - 1) {
                __hip_atomic_store(top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = true;
            }
        }
        s_last = last ? 1u : 0u;
    }
    __syncthreads();
    return s_last != 0;
}

// last of `count` workgroups to arrive at a per-task counter (see ba_last_block)
__device__ bool ba_last_of(unsigned* ticket, unsigned count) {
    __shared__ unsigned s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = tk == count - 1;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = last ? 1u : 0u;
    }
    __syncthreads();
    return s_last != 0;
}

__device__ __forceinline__ double ld_agent(const double* p) {
    return __longlong_as_double(
        __hip_atomic_load(reinterpret_cast<const long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_agent(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<long long*>(p), __double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// an iteration's trial loop starts (after its linearisation); the first one sets lambda = tau max|H_ii|
__device__ void ba_ctl_iter_begin(BaCtl* c, const unsigned long long* maxdiag) {
    if (maxdiag) {
        const double maxd = __longlong_as_double(
            (long long)__hip_atomic_load(maxdiag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        c->lambda = 1e-5 * maxd;
        c->ni = 2;
    }
    c->q = 0;
    c->iter_done = 0;
    c->skip_trial = 0;
}

// tree4096 (the oracle's order for H_pp / b_p, the Schur blocks and b_schur): leaf t sums items k = t mod 4096 in
// ascending k from 0.0, then p[t] += p[t + off], off = 2048 .. 1. A sum runs on kWG workgroups of kWLanes lanes:
// lane u of workgroup g holds leaf g + kWG u. Levels off = 2048 .. kWG add leaves of one residue class mod kWG, so
// each workgroup runs them on its own leaves (off / kWG lanes apart, nv trees at once) and publishes its class totals;
// the last workgroup runs levels kWG / 2 .. 1 over the kWG totals (kWLeaves, kWG, kWLanes: yavo_internal.h).
template <int NV>
__device__ __forceinline__ void wide_local_tree(double* red) {  // red[q * kWLanes + u]; totals end in red[q * kWLanes]
    const int t = threadIdx.x;
    __syncthreads();
    for (int off = kWLanes / 2; off > 0; off >>= 1) {
        for (int idx = t; idx < NV * off; idx += kWLanes) {
            const int q = idx / off, u = idx - q * off;
            red[q * kWLanes + u] = red[q * kWLanes + u] + red[q * kWLanes + u + off];
        }
        __syncthreads();
    }
}

// levels kWG / 2 .. 1 over the class totals part[u * stride], u < kWG (published write-through)
__device__ __forceinline__ double wide_top_tree(const double* part, int stride) {
    double v[kWG];
#pragma unroll
    for (int u = 0; u < kWG; ++u) v[u] = ld_agent(&part[u * stride]);
#pragma unroll
    for (int off = kWG / 2; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < off; ++i) v[i] = v[i] + v[i + off];
    return v[0];
}

__device__ __forceinline__ void atomic_max_abs(unsigned long long* m, double v) {
    if (v > 0.0)  // NaN never, as fmax ignores it
        __hip_atomic_fetch_max(m, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One launch for the iteration's blocks of H and b (kWLanes threads per workgroup):
//  blocks [0, np kWG)  kWG per free pose: 21 upper H_pp entries + 6 b_p entries in tree4096 order over the pose's
//                      edges (a lane's items k = leaf + 4096 m: one per lane up to 4096 edges, all loads in flight),
//                      the 27 local trees at once, class totals published; the pose's last workgroup writes H_pp, b_p
//  blocks beyond:      one lane per landmark: H_ll, b_l sequential over its edges
// first: the largest |diagonal| (free poses and landmarks) into *P.maxdiag (uint64 bits of a non-negative double).
// Device control: the last workgroup starts the iteration's trial loop (lambda on the first iteration).
__global__ __launch_bounds__(kWLanes) void ba_reduce_kernel(BaParams P, Mat3 K, int first) {
    __shared__ double red[27 * kWLanes];
    if (P.gate && *P.gate) return;  // a skipped phase of the device-driven LM
    const int t = threadIdx.x;
    const int cur = ba_cur(P);
    const double* Tc = cur ? P.poses2 : P.poses;
    const double* Xc = cur ? P.X2 : P.X;
    if ((int)blockIdx.x < P.np * kWG) {
        const int j = blockIdx.x / kWG, g = blockIdx.x - j * kWG, p = P.nf + j;
        const int k0 = P.pe_off[p], k1 = P.pe_off[p + 1];
        double T[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) T[i] = Tc[7 * p + i];
        double h[21], gv[6];
#pragma unroll
        for (int i = 0; i < 21; ++i) h[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) gv[i] = 0.0;
        // the pose's edges linearised here (the landmark lanes below store the same bits for the later kernels)
        for (int k = k0 + g + kWG * t; k < k1; k += kWLeaves) {
            const int e = P.pe[k];
            double J[12], ev[2];
            edge_linearize(T, K.v, Xc + 3 * (int64_t)P.el[e], P.meas + 2 * (int64_t)e, ev, J, nullptr);
            int q = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b, ++q) h[q] = h[q] + (J[a] * J[b] + J[6 + a] * J[6 + b]);
#pragma unroll
            for (int a = 0; a < 6; ++a) gv[a] = gv[a] + (J[a] * ev[0] + J[6 + a] * ev[1]);
        }
#pragma unroll
        for (int i = 0; i < 21; ++i) red[i * kWLanes + t] = h[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) red[(21 + i) * kWLanes + t] = gv[i];
        wide_local_tree<27>(red);
        double* part = P.rpart + (int64_t)j * kWG * 27;
        if (t < 27) st_agent(&part[g * 27 + t], red[t * kWLanes]);
        if (ba_last_of(P.rticket + j, kWG) && t < 27) {
            const double v = wide_top_tree(part + t, 27);
            double* H = P.Hpp + 36 * p;
            if (t < 21) {
                int a = 0, q = t;
                while (q >= 6 - a) {
                    q -= 6 - a;
                    ++a;
                }
                const int b = a + q;
                H[6 * a + b] = H[6 * b + a] = v;
                if (first && a == b) atomic_max_abs(P.maxdiag, fabs(v));
            } else {
                P.bp[6 * p + t - 21] = -v;
            }
        }
    } else {
        const int l = (blockIdx.x - P.np * kWG) * kWLanes + t;
        if (l < P.L) {
            double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
            const int k0 = P.le_off[l], k1 = P.le_off[l + 1];
            double X[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) X[c] = Xc[3 * (int64_t)l + c];
            // the landmark's edges two at a time: indices and poses, then both linearised (error, J_pose, J_point:
            // stored for the Schur and step kernels, 16-B stores) and added in edge order
            for (int kb = k0; kb < k1; kb += 2) {
                int eb[2], pb[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) eb[u] = kb + u < k1 ? P.le[kb + u] : 0;
#pragma unroll
                for (int u = 0; u < 2; ++u) pb[u] = kb + u < k1 ? P.ep[eb[u]] : 0;
                double jl[2][6], er[2][2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (kb + u < k1) {
                        double Jp[12];
                        edge_linearize(Tc + 7 * (int64_t)pb[u], K.v, X, P.meas + 2 * (int64_t)eb[u], er[u], Jp, jl[u]);
                        reinterpret_cast<double2*>(P.err)[eb[u]] = make_double2(er[u][0], er[u][1]);
                        double2* jp2 = reinterpret_cast<double2*>(P.Jp + 12 * (int64_t)eb[u]);
#pragma unroll
                        for (int i = 0; i < 6; ++i) jp2[i] = make_double2(Jp[2 * i], Jp[2 * i + 1]);
                        double2* jl2 = reinterpret_cast<double2*>(P.Jl + 6 * (int64_t)eb[u]);
#pragma unroll
                        for (int i = 0; i < 3; ++i) jl2[i] = make_double2(jl[u][2 * i], jl[u][2 * i + 1]);
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (kb + u >= k1) break;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
#pragma unroll
                        for (int b = a; b < 3; ++b)
                            h[3 * a + b] = h[3 * a + b] + (jl[u][a] * jl[u][b] + jl[u][3 + a] * jl[u][3 + b]);
                        g[a] = g[a] + (jl[u][a] * er[u][0] + jl[u][3 + a] * er[u][1]);
                    }
                }
            }
            double m = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = a; b < 3; ++b) {
                    P.Hll[9 * l + 3 * a + b] = h[3 * a + b];
                    P.Hll[9 * l + 3 * b + a] = h[3 * a + b];
                }
                P.bl[3 * l + a] = -g[a];
                m = fmax(m, fabs(h[4 * a]));
            }
            if (first) atomic_max_abs(P.maxdiag, m);
        }
    }
    if (P.ctl && ba_last_block_h(P.ticket + 0, P.ticket + 4) && t == 0)
        ba_ctl_iter_begin(P.ctl, first ? P.maxdiag : nullptr);
}

__device__ __forceinline__ void inv3(const double* a, double* o) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    const double id = 1.0 / det;
    o[0] = c00 * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    o[3] = c01 * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    o[6] = c02 * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
}

// (H_ll + lambda I)^-1 of landmark l, the oracle's expressions (its Dinv)
__device__ __forceinline__ void landmark_dinv(const BaParams& P, int l, double lambda, double* Di) {
    double d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = P.Hll[9 * (int64_t)l + i];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[4 * a] = d[4 * a] + lambda;
    inv3(d, Di);
}

// W_e = H_pl(e) Dinv (6 x 3), the oracle's expression
__device__ __forceinline__ void w_block(const double* h, const double* Di, double* w) {
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            w[3 * a + c] = h[3 * a + 0] * Di[0 * 3 + c] + h[3 * a + 1] * Di[1 * 3 + c] + h[3 * a + 2] * Di[2 * 3 + c];
}

// The Schur complement in the oracle's tree4096 order. Task = an upper block (p1 <= p2) of the free poses, or one
// pose's b_schur; kWG workgroups per task (see wide_local_tree). A lane's items (pair k = leaf + 4096 m) form what the
// oracle's trial step stores: Dinv of the pair's landmark from H_ll + lambda I, H_pl of both edges from their
// Jacobians, W_e1 = H_pl(e1) Dinv -- the same expressions, so the same bits, with no W / Dinv round trip through
// HBM and no trial kernel (216 B read per diagonal pair, 360 B per off-diagonal one). A configs[2] window has at most
// one item per lane, so a block's ~3,700 pairs are spread over 16 CUs with every load in flight at once.
// grid: (nb + np) kWG workgroups; task = blockIdx / kWG, g = blockIdx % kWG.
//  tasks [0, nb): S(a, b) = base - tree4096 over the co-visible pairs k of (W_e1(k)[a] . H_pl(e2(k))[b]); on a
//    diagonal block only a >= b is written, to both mirrored entries (the oracle's loop leaves that value)
//  tasks [nb, nb + np): b_schur(a) = b_p[a] - tree4096 over the pose's edges of W_e[a] . b_l(e)
__global__ __launch_bounds__(kWLanes) void ba_schur_kernel(BaParams P, double lambda) {
    __shared__ double red[36 * kWLanes];
    if (P.gate && *P.gate) return;  // a skipped phase of the device-driven LM
    if (P.lam) lambda = *P.lam;
    const int np = P.np, nb = np * (np + 1) / 2;
    const int task = blockIdx.x / kWG, g = blockIdx.x - task * kWG;
    const int t = threadIdx.x, leaf = g + kWG * t;
    if (task < nb) {
        int blk = task, i1 = 0;
        while (blk >= np - i1) {
            blk -= np - i1;
            ++i1;
        }
        const int i2 = i1 + blk;
        const int p1 = P.nf + i1, p2 = P.nf + i2;
        const int c0 = P.cv_off[p1 * P.P + p2], c1 = P.cv_off[p1 * P.P + p2 + 1];
        if (c1 == c0) {  // no shared landmark: base - (the tree of 0.0 leaves = 0.0)
            if (g == 0)
                for (int q = t; q < 36; q += kWLanes) {
                    const int a = q / 6, b = q % 6;
                    if (i1 == i2 && a < b) continue;
                    const double base = p1 == p2 ? P.Hpp[36 * p1 + 6 * a + b] + (a == b ? lambda : 0.0) : 0.0;
                    const double v = base - 0.0;
                    const int r = 6 * i1 + a, c = 6 * i2 + b, ns = P.ns;
                    P.S[(int64_t)r * ns + c] = v;
                    P.S[(int64_t)c * ns + r] = v;
                }
            return;
        }
        double acc[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) acc[i] = 0.0;
        for (int i = c0 + leaf; i < c1; i += kWLeaves) {
            const int e1 = P.cv_e1[i], e2 = P.cv_e2[i];
            double Di[9], h[18], w[18];
            landmark_dinv(P, P.el[e1], lambda, Di);
            hpl_load(P, e1, h);
            w_block(h, Di, w);  // W_e1 = H_pl(e1) Dinv: the trial kernel's product, formed here
            if (e2 != e1) hpl_load(P, e2, h);
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b < 6; ++b)
                    acc[6 * a + b] = acc[6 * a + b] + (w[3 * a] * h[3 * b] + w[3 * a + 1] * h[3 * b + 1] + w[3 * a + 2] * h[3 * b + 2]);
        }
#pragma unroll
        for (int q = 0; q < 36; ++q) red[q * kWLanes + t] = acc[q];
        wide_local_tree<36>(red);
        double* part = P.spart + (int64_t)task * kWG * 36;
        if (t < 36) st_agent(&part[g * 36 + t], red[t * kWLanes]);
        if (!ba_last_of(P.sticket + task, kWG)) return;
        if (t < 36) {
            const int a = t / 6, b = t % 6;
            if (!(i1 == i2 && a < b)) {
                const double base = p1 == p2 ? P.Hpp[36 * p1 + 6 * a + b] + (a == b ? lambda : 0.0) : 0.0;
                const double v = base - wide_top_tree(part + t, 36);
                const int r = 6 * i1 + a, c = 6 * i2 + b, ns = P.ns;
                P.S[(int64_t)r * ns + c] = v;
                P.S[(int64_t)c * ns + r] = v;
            }
        }
    } else {
        const int j = task - nb, p = P.nf + j;
        const int k0 = P.pe_off[p], k1 = P.pe_off[p + 1];
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = k0 + leaf; i < k1; i += kWLeaves) {
            const int e = P.pe[i], l = P.el[e];
            double Di[9], h[18], w[18];
            landmark_dinv(P, l, lambda, Di);
            hpl_load(P, e, h);
            w_block(h, Di, w);
            const double* gl = P.bl + 3 * l;
            const double g0 = gl[0], g1 = gl[1], g2 = gl[2];
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[a] = acc[a] + (w[3 * a] * g0 + w[3 * a + 1] * g1 + w[3 * a + 2] * g2);
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) red[q * kWLanes + t] = acc[q];
        wide_local_tree<6>(red);
        double* part = P.spart + (int64_t)task * kWG * 36;
        if (t < 6) st_agent(&part[g * 36 + t], red[t * kWLanes]);
        if (!ba_last_of(P.sticket + task, kWG)) return;
        if (t < 6) P.bs[6 * j + t] = P.bp[6 * p + t] - wide_top_tree(part + t, 36);
    }
}

// ---- device-driven LM control (the host loop of yv_ba_solve's host form, operation for operation) ----
__device__ void ba_ctl_init(BaCtl* c, double chi2, double* log, unsigned long long* maxdiag) {
    c->currentChi = chi2;
    log[0] = chi2;
    c->lambda = 0;
    c->ni = 2;
    c->rho = 0;
    c->q = 0;
    c->it = 0;
    c->stop = 0;
    c->iters = 0;
    c->skip_iter = 0;
    c->skip_trial = 1;
    c->suspended = 0;
    c->iter_done = 0;
    *maxdiag = 0;
}

// after a trial: rho, accept (lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), the trial state becomes current) or
// reject (lambda *= ni, ni *= 2); the trial loop ends when !(rho < 0 && q < 10). Then the iteration's end: its chi2
// is logged; stop on q == 10 / rho == 0 / non-finite lambda. A trial loop still running after the one trial slot the
// host enqueued per iteration suspends the solve (every later kernel skips) until the host resumes it.
__device__ void ba_ctl_decide(BaCtl* c, double tempChi, double scale, bool ok2, int* cur, double* log) {
    if (!ok2) tempChi = DBL_MAX;
    double rho = c->currentChi - tempChi;
    scale += 1e-3;
    rho /= scale;
    if (rho > 0 && isfinite(tempChi)) {
        double alpha = 1. - cube_cr(2 * rho - 1);  // pow(2 rho - 1, 3), correctly rounded
        alpha = fmin(alpha, 2. / 3.);
        const double sf = fmax(1. / 3., alpha);
        c->lambda *= sf;
        c->ni = 2;
        c->currentChi = tempChi;
        *cur ^= 1;
    } else {
        c->lambda *= c->ni;
        c->ni *= 2;
    }
    c->rho = rho;
    c->q += 1;
    if (!(rho < 0 && c->q < 10)) {
        c->iter_done = 1;
        c->skip_trial = 1;
    }
    if (!c->iter_done) {
        c->suspended = 1;
        c->skip_iter = 1;
        c->skip_trial = 1;
        return;
    }
    log[c->it + 1] = c->currentChi;
    if (c->q == 10 || c->rho == 0 || !isfinite(c->lambda)) {
        c->stop = 1;
        c->iters = c->it + 1;
        c->skip_iter = 1;
        c->skip_trial = 1;
    } else {
        c->it += 1;
        c->iters = c->it;
    }
}

__global__ void ba_ctl_resume_kernel(BaCtl* c) {
    c->suspended = 0;
    c->skip_iter = 0;
    c->skip_trial = 0;
}

// chi2 and the LM scale in the oracle's landmark-block order (oracle/yavo_oracle_ba.c lblock_total): a workgroup of
// kNT lanes holds one block of 256 landmarks, lane t landmark 256 b + t (0.0 past L). Each workgroup runs the block's
// halving trees in LDS and publishes the totals write-through (P.part[1 + 2 b] chi2, [2 + 2 b] the landmarks' scale
// part; workgroup 0 also the free poses' scale part, tree256 over their items, at [0]); the last workgroup folds the
// block totals into 256 leaves (block b into leaf b mod 256, ascending b), runs the trees over the leaves and then
// decides the trial (device control), starts the solve (trial false), or leaves chi2 / scale in scal[0] / scal[1].
template <bool kTrial>
__device__ __forceinline__ void lblock_reduce(const BaParams& P, double chi, double sl, double sp) {
    __shared__ double red[3][kNT];
    const int t = threadIdx.x;
    red[0][t] = chi;
    red[1][t] = sl;
    red[2][t] = sp;
    __syncthreads();
    for (int off = kNT / 2; off > 0; off >>= 1) {
        if (t < off) {
            red[0][t] = red[0][t] + red[0][t + off];
            if (kTrial) {
                red[1][t] = red[1][t] + red[1][t + off];
                red[2][t] = red[2][t] + red[2][t + off];
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        st_agent(&P.part[1 + 2 * blockIdx.x], red[0][0]);
        if (kTrial) st_agent(&P.part[2 + 2 * blockIdx.x], red[1][0]);
        if (kTrial && blockIdx.x == 0) st_agent(&P.part[0], red[2][0]);
    }
    if (!ba_last_block_h(P.ticket + 1, P.ticket + 4 + kTicketGroups)) return;
    const int nb = (P.L + kNT - 1) / kNT;
    double lc = 0.0, ls = 0.0;
    for (int b = t; b < nb; b += kNT) {
        lc = lc + ld_agent(&P.part[1 + 2 * b]);
        if (kTrial) ls = ls + ld_agent(&P.part[2 + 2 * b]);
    }
    __syncthreads();  // this workgroup's own block trees are read
    red[0][t] = lc;
    red[1][t] = ls;
    __syncthreads();
    for (int off = kNT / 2; off > 0; off >>= 1) {
        if (t < off) {
            red[0][t] = red[0][t] + red[0][t + off];
            if (kTrial) red[1][t] = red[1][t] + red[1][t + off];
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double chi2 = red[0][0];
    if (!kTrial) {
        if (!P.ctl) P.scal[0] = chi2;
        else ba_ctl_init(P.ctl, chi2, P.log, P.maxdiag);
        return;
    }
    const double scale = ld_agent(&P.part[0]) + red[1][0];
    if (!P.ctl) {
        P.scal[0] = chi2;
        P.scal[1] = scale;
    } else {
        ba_ctl_decide(P.ctl, chi2, scale, P.ns > 0 ? P.scal[2] != 0.0 : true, P.cur, P.log);
    }
}

// The trial step in one launch (g2o's back-substitution, oplus, the trial chi2 and the LM scale): every workgroup
// first forms all poses of the trial state in LDS (free: exp(x_p) T, fixed: T); one lane per landmark then runs
// x_l = Dinv (b_l - sum_e H_pl^T x_p) sequentially over its edges, writes X + x_l into the trial state, and sums |e|^2
// of its edges at the trial state and its three scale items x (lambda x + b) (each from 0.0, in order) for
// lblock_reduce, whose last workgroup decides the trial. The trial state is the other buffer: a rejected trial leaves
// the current one untouched (no backup / restore copies); an accepted one flips P.cur. (Until round 5 the per-edge
// |e|^2 and the scale items went through HBM to a separate tree4096 chi2 kernel: 11 us per trial.)
__global__ __launch_bounds__(kNT) void ba_step_kernel(BaParams P, Mat3 K, double lambda) {
    extern __shared__ double sT[];  // [P][7]
    if (P.gate && *P.gate) return;  // a skipped phase of the device-driven LM
    if (P.lam) lambda = *P.lam;
    const int ns = P.ns;
    const int cur = ba_cur(P);
    const double* T0 = cur ? P.poses2 : P.poses;
    const double* X0 = cur ? P.X2 : P.X;
    double* T1 = cur ? P.poses : P.poses2;
    double* X1 = cur ? P.X : P.X2;
    const int t = threadIdx.x;
    for (int p = t; p < P.P; p += kNT) {
        double Tn[7];
        if (p < P.nf) {
#pragma unroll
            for (int i = 0; i < 7; ++i) Tn[i] = T0[7 * p + i];
        } else {
            double dT[7];
            se3_exp(P.xp + 6 * (p - P.nf), dT);
            se3_mul(dT, T0 + 7 * p, Tn);
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) sT[7 * p + i] = Tn[i];
        if (blockIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 7; ++i) T1[7 * p + i] = Tn[i];
        }
    }
    // the free poses' scale items, leaf t = items k = t mod kNT in ascending k (workgroup 0)
    double sp = 0.0;
    if (blockIdx.x == 0)
        for (int k = t; k < ns; k += kNT) {
            const double x = P.xp[k];
            sp = sp + x * (lambda * x + P.bp[6 * P.nf + k]);
        }
    __syncthreads();
    const int l = blockIdx.x * kNT + t;
    double chi = 0.0, sl = 0.0;
    if (l < P.L) {
        const int k0 = P.le_off[l], k1 = P.le_off[l + 1];
        double tv[3] = {P.bl[3 * l], P.bl[3 * l + 1], P.bl[3 * l + 2]};
        double D[9];
        landmark_dinv(P, l, lambda, D);
        // the landmark's edges two at a time: indices and poses, then both edges' Jacobians and x_p loaded before
        // the subtractions (in edge order), one dependent load round per pair of edges
        for (int kb = k0; kb < k1; kb += 2) {
            int eb[2], pb[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) eb[u] = kb + u < k1 ? P.le[kb + u] : 0;
#pragma unroll
            for (int u = 0; u < 2; ++u) pb[u] = kb + u < k1 ? P.ep[eb[u]] : 0;
            double h[2][18], xv[2][6];
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (kb + u < k1 && pb[u] >= P.nf) {
                    hpl_load(P, eb[u], h[u]);
                    const double* xpp = P.xp + 6 * (pb[u] - P.nf);
#pragma unroll
                    for (int a = 0; a < 6; ++a) xv[u][a] = xpp[a];
                }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (kb + u >= k1 || pb[u] < P.nf) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double d = h[u][c] * xv[u][0];
#pragma unroll
                    for (int a = 1; a < 6; ++a) d = d + h[u][3 * a + c] * xv[u][a];
                    tv[c] = tv[c] - d;
                }
            }
        }
        double Xn[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x = D[3 * c] * tv[0] + D[3 * c + 1] * tv[1] + D[3 * c + 2] * tv[2];
            P.xl[3 * l + c] = x;
            sl = sl + x * (lambda * x + P.bl[3 * l + c]);
            Xn[c] = X0[3 * l + c] + x;
            X1[3 * l + c] = Xn[c];
        }
        for (int kb = k0; kb < k1; kb += 2) {
            int eb[2], pb[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) eb[u] = kb + u < k1 ? P.le[kb + u] : 0;
#pragma unroll
            for (int u = 0; u < 2; ++u) pb[u] = kb + u < k1 ? P.ep[eb[u]] : 0;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (kb + u >= k1) break;
                double r[2];
                edge_error(sT + 7 * pb[u], K.v, Xn, P.meas + 2 * eb[u], r);
                chi = chi + (r[0] * r[0] + r[1] * r[1]);
            }
        }
    }
    lblock_reduce<true>(P, chi, sl, sp);
}

// the solve's first chi2 at the current estimate, in the same order: one lane per landmark over its edges. A solve
// starts in state 0 (P.poses / P.X); workgroup 0 also resets *P.cur for the kernels after it (no separate memset)
__global__ __launch_bounds__(kNT) void ba_chi2_kernel(BaParams P, Mat3 K) {
    if (P.gate && *P.gate) return;  // a skipped phase of the device-driven LM
    if (P.cur && blockIdx.x == 0 && threadIdx.x == 0) *P.cur = 0;
    const double* T = P.poses;
    const double* X = P.X;
    const int l = blockIdx.x * kNT + threadIdx.x;
    double chi = 0.0;
    if (l < P.L) {
        const double Xl[3] = {X[3 * l], X[3 * l + 1], X[3 * l + 2]};
        for (int k = P.le_off[l]; k < P.le_off[l + 1]; ++k) {
            const int e = P.le[k];
            double r[2];
            edge_error(T + 7 * P.ep[e], K.v, Xl, P.meas + 2 * e, r);
            chi = chi + (r[0] * r[0] + r[1] * r[1]);
        }
    }
    lblock_reduce<false>(P, chi, 0.0, 0.0);
}

// after the solve: the estimate into P.poses / P.X when it ended in the other buffer
__global__ __launch_bounds__(256) void ba_finish_kernel(BaParams P) {
    if (P.gate && *P.gate) return;  // enqueued with the solve: skipped when it was suspended (the host reruns it)
    if (!P.cur || !*P.cur) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 7 * P.P) P.poses[i] = P.poses2[i];
    if (i < 3 * P.L) P.X[i] = P.X2[i];
}

}  // namespace ba

void launch_ba_ctl_resume(BaCtl* c, hipStream_t s) {
    hipLaunchKernelGGL(ba::ba_ctl_resume_kernel, dim3(1), dim3(1), 0, s, c);
}

void launch_ba_linearize(const BaParams& P, const Mat3& K, int first, hipStream_t s) {
    const int nb = std::max(1, P.np * ba::kWG + (P.L + ba::kWLanes - 1) / ba::kWLanes);
    hipLaunchKernelGGL(ba::ba_reduce_kernel, dim3(nb), dim3(ba::kWLanes), 0, s, P, K, first);
}

void launch_ba_trial(const BaParams& P, const Mat3& K, double lambda, hipStream_t s) {
    const int nb = P.np * (P.np + 1) / 2;
    if (nb > 0)
        hipLaunchKernelGGL(ba::ba_schur_kernel, dim3((nb + P.np) * ba::kWG), dim3(ba::kWLanes), 0, s, P, lambda);
    launch_ba_ldlt(P, s);
    hipLaunchKernelGGL(ba::ba_step_kernel, dim3(std::max(1, (P.L + 255) / 256)), dim3(256),
                       sizeof(double) * 7 * P.P, s, P, K, lambda);
}

void launch_ba_chi2(const BaParams& P, const Mat3& K, hipStream_t s) {
    hipLaunchKernelGGL(ba::ba_chi2_kernel, dim3(std::max(1, (P.L + ba::kNT - 1) / ba::kNT)), dim3(ba::kNT), 0, s, P, K);
}

void launch_ba_finish(const BaParams& P, hipStream_t s) {
    const int n = std::max(7 * P.P, 3 * P.L);
    if (n > 0) hipLaunchKernelGGL(ba::ba_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, s, P);
}

}  // namespace yavo
