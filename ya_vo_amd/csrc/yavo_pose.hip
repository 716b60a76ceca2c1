// yavo_pose.hip -- gfx950 kernels for the pose solvers of the hot path.
//
//   pose_lm_kernel       LoopHandler::optimizePoseOnly + the g2o edge     src/LoopHandler.cc:730-861,
//                        include/Optimizer.hpp:40-135; one workgroup per pose problem: edge terms
//                        (residual, 2x6 Jacobian, Huber weight) per lane, J^T W J / J^T W e / chi2 as
//                        fixed-order tree reductions in LDS, the 6x6 LDLT + LM control on lane 0
//   pose_gn_kernel       bundleAdjustmentGaussNewton                      src/test.cc:172-244
//
// The projection edge is in yavo_edge.h (shared with the bundle adjustment), the two 6x6 LDLT forms in yavo_ldlt6.h,
// the workgroup scan, uni_f64 and kNT in yavo_geom_dev.h (shared with yavo_geom.hip and yavo_track.hip).
// Every floating-point expression is written in the reference's operation order and the file is built
// with -ffp-contract=off, so each kernel matches oracle/yavo_oracle_geom.c bit for bit (sums over edges
// in the oracle's sum_mode 1 = this file's tree order).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <float.h>
#include <stdint.h>
#include <stdlib.h>

#include "yavo_internal.h"
#include "yavo_edge.h"
#include "yavo_geom_dev.h"
#include "yavo_ldlt6.h"
#include "yavo_se3.h"
#include "yavo_xlane.h"

namespace yavo {
namespace geom {

using edge::edge_error;
using edge::edge_error_pc;
using edge::edge_jacobian_pc;
using ldlt6::ldlt6_solve;
using ldlt6::ldlt6_solve_lds;
using se3::k_cos;
using se3::k_sin;
using se3::se3_act;
using se3::se3_exp;
using se3::se3_mul;

// YAVO_LM_PROFILE builds (tools/lm_profile.py) time the pose-LM phases with the shader clock on lane 0
#ifdef YAVO_LM_PROFILE
__device__ unsigned long long g_lm_prof[1024][10];
#define LMP_DECL unsigned long long lmp_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long lmp_t = __builtin_readcyclecounter();
#define LMP_MARK(slot) do { const unsigned long long t_ = __builtin_readcyclecounter(); lmp_acc[slot] += t_ - lmp_t; lmp_t = t_; } while (0)
#define LMP_STORE() do { if (threadIdx.x == 0) for (int q_ = 0; q_ < 10; ++q_) g_lm_prof[blockIdx.x & 1023][q_] = lmp_acc[q_]; } while (0)
#else
#define LMP_DECL
#define LMP_MARK(slot) do {} while (0)
#define LMP_STORE() do {} while (0)
#endif
constexpr int kMaxEdges = 4096;   // edges per pose problem held in LDS

// ------------------------------------------------------------------------------------------------
// pose-only LM (g2o semantics) and GN, one workgroup per problem
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double huber_rho(double e2, double* rho1) {
    const double delta = 1.0, dsqr = delta * delta;
    if (e2 <= dsqr) {
        *rho1 = 1.;
        return e2;
    }
    double sqrte = sqrt(e2);
    *rho1 = delta / sqrte;
    return 2 * sqrte * delta - dsqr;
}

// Tree sum of per-thread partials in the oracle's order (sum_mode log2(NT) - 7): p[t] += p[t + off] for
// off = NT/2 .. 64 (across waves, through LDS), then 32 .. 1 inside wave 0 (shuffles).  part[] holds this
// thread's nv partials; totals land in out[0..nv) (LDS), visible after the trailing barrier.
// red: >= nv * NT/2 doubles of LDS.
template <int NV, int NT = kNT>
__device__ void tree_reduce(double (&part)[NV], double* red, double* out, unsigned long long* t_sync = nullptr) {
    const int tid = threadIdx.x;
    __syncthreads();
#ifdef YAVO_LM_PROFILE
    if (t_sync) *t_sync = __builtin_readcyclecounter();
#endif
#pragma unroll
    for (int off = NT / 2; off >= 128; off >>= 1) {
        if (tid >= off && tid < 2 * off) {
#pragma unroll
            for (int v = 0; v < NV; ++v) red[v * (NT / 2) + (tid - off)] = part[v];
        }
        __syncthreads();
        if (tid < off) {
#pragma unroll
            for (int v = 0; v < NV; ++v) part[v] = part[v] + red[v * (NT / 2) + tid];
        }
        __syncthreads();
    }
    if (tid >= 64 && tid < 128) {
#pragma unroll
        for (int v = 0; v < NV; ++v) red[v * (NT / 2) + (tid - 64)] = part[v];
    }
    __syncthreads();
    if (tid < 64) {
        // wave 0: the NV independent shuffle trees advance together (all NV shuffles of a level are issued
        // before the adds), so one LDS-permute latency is paid per level instead of per value and level
        double x[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) x[v] = part[v] + red[v * (NT / 2) + tid];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            double y[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) y[v] = __shfl_down(x[v], off, 64);
#pragma unroll
            for (int v = 0; v < NV; ++v) x[v] = x[v] + y[v];
        }
        if (tid == 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) out[v] = x[v];
        }
    }
    __syncthreads();
}

// The pose LM's reduction of NV per-thread partials over NT = 64 W threads (oracle sum_mode 4 + log2(W)): the
// halving tree p[l] += p[l + off], off = 32 .. 1, inside each wave, then the W wave totals left to right.
// Inside the wave it runs as a reduce-scatter: at the level with offset off the two lanes l, l ^ off split their
// n live values, each keeping ceil(n / 2) of them (the lane with bit off clear the lower half) and adding its
// partner's copy of those -- one shuffle per kept value instead of one per value, 29 instead of 168 exchanges for
// 28 values. Each value's partials still meet in the tree's pairs and order (the kept sum is own + partner, and
// IEEE addition commutes, so the lane with bit off set computes the lower lane's bits). After the six levels the
// lane pair (l, l ^ 1) holds value v(l) = 14 b5 + 7 b4 + 4 b3 + 2 b2 + b1 (28 values: v < 28 is real, the rest
// are padding slots).
// The exchanges run on the VALU side (yavo_xlane.h): permlane swaps at offsets 32 / 16, DPP below.
template <int N, int OFF>
__device__ __forceinline__ void rs_level(const double* in, double* out, int lane, int& v) {
    constexpr int h = (N + 1) / 2;
    const bool up = (lane & OFF) != 0;
#pragma unroll
    for (int j = 0; j < h; ++j) {
        double lo = in[j];
        double hi = (h + j < N) ? in[h + j] : 0.0;
        if constexpr (OFF >= 16) {
            xl::swap_halves_f64<OFF>(lo, hi);  // {own kept, partner's} in some order: the sum commutes
            out[j] = lo + hi;
        } else {
            const double keep = up ? hi : lo;
            out[j] = keep + xl::xor_row_f64<OFF>(up ? lo : hi);
        }
    }
    if (up) v += h;
}

// flag (optional): read by every thread after the reduction's first barrier and returned (the pass's literal-form
// flag rides on the reduction's barriers instead of a barrier of its own); thread 0 clears it after the last one.
template <int NV, int NT>
__device__ int lm_reduce(double (&part)[NV], double* red /* >= NV * NT / 64 */, double* out,
                         unsigned long long* t_sync = nullptr, int* flag = nullptr) {
    static_assert(NV == 28, "the reduce-scatter schedule is written for 28 values");
    constexpr int W = NT / 64;
    static_assert(W >= 2, "the flag hand-off needs the two barriers of the multi-wave form");
#ifdef YAVO_LM_PROFILE
    if (t_sync) *t_sync = __builtin_readcyclecounter();
#endif
    const int tid = threadIdx.x, lane = tid & 63;
    int v = 0;
    double a14[14], a7[7], a4[4], a2[2], a1[1];
    rs_level<28, 32>(part, a14, lane, v);
    rs_level<14, 16>(a14, a7, lane, v);
    rs_level<7, 8>(a7, a4, lane, v);
    rs_level<4, 4>(a4, a2, lane, v);
    rs_level<2, 2>(a2, a1, lane, v);
    const double tot = a1[0] + xl::xor_row_f64<1>(a1[0]);
    const bool owner = v < NV && (lane & 1) == 0;
    if (owner) red[(tid >> 6) * NV + v] = tot;
    __syncthreads();
    const int f = flag ? *flag : 0;
    if (tid < NV) {
        double q = red[tid];
#pragma unroll
        for (int w = 1; w < W; ++w) q = q + red[w * NV + tid];
        out[tid] = q;
    }
    __syncthreads();
    if (flag && tid == 0 && f) *flag = 0;  // every thread read it before the barrier above; set again next pass
    return f;
}

struct LMShared {
    double T[7], Tbak[7], Tlast[7], K[9];
    double sys[28], x[6], vals[32];  // sys: {H lower packed (21), b (6), chi2} of the current iteration
    double Hf[36];                     // the same H, full symmetric (the LDLT's gather source)
    double lambda, ni, currentChi, tempChi, rho;
    int flag;  // control broadcast from lane 0
    int hub;   // a Huber weight (c2 > delta^2 on a robust edge) was applied in some pass of the current round
    int lit;   // some edge of the current pass had a non-finite operand (lm_pass: the pass is redone literally)
};

constexpr int kLMVals = 28;  // 21 lower-triangle H entries + 6 b + 1 chi2

// The exact short form of one edge's J^T W J lower triangle and -J^T W e (see lm_pass), added to the partials.
__device__ __forceinline__ void lm_accumulate_short(double (&part)[28], const double* J, double w, const double* e) {
    double a[6], b[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        a[r] = J[r] * w;
        b[r] = J[6 + r] * w;
    }
    part[0] = part[0] + a[0] * J[0];
    part[2] = part[2] + b[1] * J[7];
#pragma unroll
    for (int r = 2; r < 6; ++r) {
        part[r * (r + 1) / 2 + 0] = part[r * (r + 1) / 2 + 0] + a[r] * J[0];
        part[r * (r + 1) / 2 + 1] = part[r * (r + 1) / 2 + 1] + b[r] * J[7];
#pragma unroll
        for (int c = 2; c <= r; ++c)
            part[r * (r + 1) / 2 + c] = part[r * (r + 1) / 2 + c] + (a[r] * J[c] + b[r] * J[6 + c]);
    }
    part[21] = part[21] + (-(a[0] * e[0]));
    part[22] = part[22] + (-(b[1] * e[1]));
#pragma unroll
    for (int r = 2; r < 6; ++r) part[21 + r] = part[21 + r] + (-(a[r] * e[0] + b[r] * e[1]));
}

// The literal form of one edge's contributions (rho' Omega with Omega = I spelt out: every product with the literal
// 0.0 / 1.0), added to partials held in a stack array: only the rare pass that meets a non-finite operand runs it
// (lm_pass), so its temporaries do not count against the hot loop's registers.
__device__ __noinline__ void lm_accumulate_literal(double* part, const double* J, double w, const double* e) {
#pragma unroll 1
    for (int r = 0; r < 6; ++r) {
        const double t0 = J[r] * w + J[6 + r] * 0.0;
        const double t1 = J[r] * 0.0 + J[6 + r] * w;
#pragma unroll 1
        for (int c = 0; c <= r; ++c) part[r * (r + 1) / 2 + c] = part[r * (r + 1) / 2 + c] + (t0 * J[c] + t1 * J[6 + c]);
        const double s0 = (w * J[r]) * 1.0 + (w * J[6 + r]) * 0.0;
        const double s1 = (w * J[r]) * 0.0 + (w * J[6 + r]) * 1.0;
        part[21 + r] = part[21 + r] + (-(s0 * e[0] + s1 * e[1]));
    }
}

// One edge at T: its error, robust chi2 and weight, and J.  Returns c2 > delta^2 on a robust edge (a Huber weight).
__device__ __forceinline__ void lm_edge(const double* T, const double* K, const double* xi, const double* mi, int rob,
                                        double* e, double& chi, double& w, double* J, bool& hub) {
    double pc[3];
    se3_act(T, xi, pc);
    edge_error_pc(pc, K, mi, e);
    const double c2 = e[0] * e[0] + e[1] * e[1];
    w = 1.0;
    chi = c2;
    // Huber only past delta: skipped by the whole wave when no lane needs it (a per-lane branch is if-converted
    // into an unconditional sqrt + division)
    hub = rob && c2 > 1.0;
    if (__any(hub)) {
        if (rob) chi = huber_rho(c2, &w);
    }
    edge_jacobian_pc(pc, K, J);
}

// One pass over the active edges at S.T: computeActiveErrors + activeRobustChi2 + buildSystem of g2o's
// BlockSolver (Huber-weighted J^T J lower triangle, -J^T W e, robust chi2), summed in the oracle's tree
// order into S.vals[0..28).  Also records S.Tlast (the estimate the active edges' errors refer to).
//
// g2o forms J^T (rho' Omega) J and -J^T (rho' Omega) e with Omega = I, i.e. products with the literal 0.0 / 1.0 of
// Omega, and J[1] = J[6] = 0 structurally.  With finite operands those products only contribute signed zeros, which
// cannot change a partial sum (a partial that starts at +0.0 never becomes -0.0, and p + (+-0) = p for p != 0), so the
// short form gives bit-identical sums.  A pass in which some edge has a non-finite operand is run again by the whole
// workgroup in the literal form (for every edge: bit-identical to the short form on the finite ones), with the
// partials on the stack; the hot loop carries only the short form (the literal form inside it raised the kernel's
// register demand by ~50 VGPRs).
template <int NT, typename UV>
__device__ __forceinline__ void lm_pass(LMShared& S, const int16_t* s_active, int na, const uint8_t* s_robust,
                                        const double* X, const UV* uv, double* s_red,
                                        unsigned long long* lmp = nullptr) {
    const int tid = threadIdx.x;
    __syncthreads();  // S.T written by lane 0
#ifdef YAVO_LM_PROFILE
    const unsigned long long p0 = __builtin_readcyclecounter();
#endif
    // the estimate and K are wave-uniform: held in SGPRs (16 doubles = 32 VGPRs fewer through the edge loop)
    double T[7], K[9];
#pragma unroll
    for (int q = 0; q < 7; ++q) T[q] = uni_f64(S.T[q]);
#pragma unroll
    for (int q = 0; q < 9; ++q) K[q] = uni_f64(S.K[q]);
    if (tid < 7) S.Tlast[tid] = S.T[tid];
    double part[kLMVals];
#pragma unroll
    for (int v = 0; v < kLMVals; ++v) part[v] = 0.0;
    bool literal = false;
    // the next edge's point / measurement / robust flag are loaded while this one is evaluated (the gathers
    // hit L2: their latency would otherwise be paid once per edge)
    double nx[5] = {0, 0, 0, 0, 0};
    int nrob = 0;
    if (tid < na) {
        const int i = s_active[tid];
        nx[0] = X[3 * i]; nx[1] = X[3 * i + 1]; nx[2] = X[3 * i + 2]; nx[3] = (double)uv[2 * i]; nx[4] = (double)uv[2 * i + 1];
        nrob = s_robust[i];
    }
    for (int a = tid; a < na; a += NT) {
        const double xi[3] = {nx[0], nx[1], nx[2]}, mi[2] = {nx[3], nx[4]};
        const int rob = nrob;
        if (a + NT < na) {
            const int i = s_active[a + NT];
            nx[0] = X[3 * i]; nx[1] = X[3 * i + 1]; nx[2] = X[3 * i + 2]; nx[3] = (double)uv[2 * i]; nx[4] = (double)uv[2 * i + 1];
            nrob = s_robust[i];
        }
        double e[2], J[12], chi, w;
        bool hub;
        lm_edge(T, K, xi, mi, rob, e, chi, w, J, hub);
        if (__any(hub) && (tid & 63) == 0) S.hub = 1;
        part[27] = part[27] + chi;
        const double fin = J[0] + J[2] + J[3] + J[4] + J[5] + J[7] + J[8] + J[9] + J[10] + J[11] + w + e[0] + e[1];
        literal |= !isfinite(fin);
        lm_accumulate_short(part, J, w, e);
    }
    if (literal) S.lit = 1;
#ifdef YAVO_LM_PROFILE
    const unsigned long long p1 = __builtin_readcyclecounter();
    unsigned long long ps = 0;
    const int lit = lm_reduce<kLMVals, NT>(part, s_red, S.vals, &ps, &S.lit);
    if (lmp) {
        const unsigned long long p2 = __builtin_readcyclecounter();
        lmp[0] += p1 - p0;
        lmp[1] += p2 - ps;  // the reduction proper
        lmp[8] += ps - p1;  // waiting at the first barrier for the other waves' edges
        lmp[9] += 1;        // passes (error + system evaluations)
    }
#else
    const int lit = lm_reduce<kLMVals, NT>(part, s_red, S.vals, nullptr, &S.lit);
#endif
    if (lit) {
        // the rare pass: every edge again in the literal form, partials on the stack, in the same order
        double lp[kLMVals];
        for (int v = 0; v < kLMVals; ++v) lp[v] = 0.0;
        for (int a = tid; a < na; a += NT) {
            const int i = s_active[a];
            const double xi[3] = {X[3 * i], X[3 * i + 1], X[3 * i + 2]}, mi[2] = {(double)uv[2 * i], (double)uv[2 * i + 1]};
            double e[2], J[12], chi, w;
            bool hub;
            lm_edge(T, K, xi, mi, s_robust[i], e, chi, w, J, hub);
            lp[27] = lp[27] + chi;
            lm_accumulate_literal(lp, J, w, e);
        }
#pragma unroll
        for (int v = 0; v < kLMVals; ++v) part[v] = lp[v];
        lm_reduce<kLMVals, NT>(part, s_red, S.vals);
    }
}

// Problem p owns edges [offsets[p], offsets[p+1]) (CSR) or, with counts != nullptr, [p*stride, p*stride +
// counts[p]) (the batch's fixed-stride track layout).  The prior is read from priors[p] and the estimate
// written to poses[p] (the two may alias).
// Register budget of the LM.  The 256-thread form (the batch of a step's 2048 tracks, beside top-K and BRIEF): 3 waves
// per SIMD = 168 VGPRs.  With the literal J^T Omega J form out of the edge loop (lm_pass) the hot loop fits without
// spills (the stack partials and the call of the rare literal pass are the kernel's only scratch), and two LM waves
// leave a SIMD 176 registers for BRIEF / top-K beside them instead of 48: 230.1 k -> 233.7 k frames/s, the LM itself
// 2.29 -> 2.12 ms per launch in the step (profiles/r06/c19).  The 512-thread form (one problem of the LoopHandler, the
// sequence's 20-track batches) keeps 2 waves per SIMD = 256: at 168 its single-problem latency rose ~9% (the pose LM
// 54 -> 60 ms of a 200-frame LoopHandler run, profiles/r06/c27).
template <int NT>
struct LMWaves {
    static constexpr int value = NT >= 512 ? 2 : 3;
};
#ifdef YAVO_LM_WPE
#define YAVO_LM_ATTR __attribute__((amdgpu_waves_per_eu(YAVO_LM_WPE)))
#else
#define YAVO_LM_ATTR __attribute__((amdgpu_waves_per_eu(LMWaves<NT>::value)))
#endif
template <int NT>
__device__ __forceinline__ void pose_lm_body(const int32_t* __restrict__ offsets, const int32_t* __restrict__ counts,
                                                      int stride, const double* __restrict__ Xall,
                                                      const double* __restrict__ uvall, const double* __restrict__ Kall,
                                                      const double* priors, double* poses,
                                                      uint8_t* __restrict__ outlier_all, int32_t* __restrict__ inliers,
                                                      int n_prob) {
    constexpr int CAP = kMaxEdges;
    __shared__ uint8_t s_level[CAP], s_out[CAP], s_robust[CAP];
    __shared__ int16_t s_active[CAP];
    __shared__ double s_red[NT > 64 ? kLMVals * (NT / 64) : 1];
    __shared__ LMShared S;
    __shared__ int s_tmp[40];
    LMP_DECL
    // problems blockIdx.x, blockIdx.x + gridDim.x, ...: a grid smaller than the problem count keeps the LM on fewer
    // CUs (launch_lm), every problem is solved exactly as with one workgroup each
    for (int prob = blockIdx.x; prob < n_prob; prob += gridDim.x) {
    const int tid = threadIdx.x;
    const int64_t e0 = counts ? (int64_t)prob * stride : (int64_t)offsets[prob];
    int n = counts ? counts[prob] : (int)(offsets[prob + 1] - e0);
    if (n > CAP) n = CAP;
    const double* X = Xall + 3 * e0;
    const double* uv = uvall + 2 * e0;
    if (tid < 9) S.K[tid] = Kall[9 * prob + tid];
    if (tid < 7) S.T[tid] = priors[7 * prob + tid];
    if (tid == 0) S.lit = 0;
    for (int i = tid; i < n; i += NT) {
        s_level[i] = 0;
        s_out[i] = 0;
        s_robust[i] = 1;
    }
    __syncthreads();
    double prior[7];
    for (int q = 0; q < 7; ++q) prior[q] = S.T[q];
    const double chi2th = 5.991;
    const double tau = 1e-5, goodLower = 1.0 / 3.0, goodUpper = 2.0 / 3.0;
    int outlierCount = 0;
    // Round memoization (exact): every round restarts from the same prior with a fresh LM (src/LoopHandler.cc:817-
    // 819: setEstimate(currentFrame->pose), initializeOptimization(), optimize(10)), so a round whose active edge set
    // and robust kernels equal those of the last executed round replays it operation for operation: its estimate,
    // its edges' errors and hence its classification are the last round's, and it is skipped.  The active set is
    // unchanged iff the last classification moved no edge between levels.  Dropping the Huber kernel after round 2
    // changes nothing either when no pass of the replayed round applied a Huber weight: below delta^2 the kernel's
    // rho = e2 and rho' = 1.0, and every product with 1.0 is exact.
    bool replay = false;
    int hub = 0;

    for (int round = 0; round < 4; ++round) {
        int changed = 0;
        if (!replay) {
            if (tid == 0) S.hub = 0;  // the first pass starts with a barrier: no wave writes S.hub before this store
            if (tid < 7) S.T[tid] = prior[tid];
            // initializeOptimization(): active = level-0 edges in insertion order (block compaction)
            int na = 0;
            for (int base = 0; base < n; base += NT) {
                const int i = base + tid;
                const int f = (i < n && s_level[i] == 0) ? 1 : 0;
                int tot = 0;
                const int off = block_excl_scan_geom<NT>(f, s_tmp, &tot);
                if (f) s_active[na + off] = (int16_t)i;
                na += tot;
            }
            __syncthreads();
            if (na > 0) {
                double lambda = 0, ni = 2;
                // S.vals holds {H, b, chi2} at S.T when `have` (the last trial was accepted: g2o's next
                // computeActiveErrors + buildSystem happen at exactly that estimate, so the trial pass builds the
                // system along with its chi2 and the rebuild is skipped)
                bool have = false;
                for (int it = 0; it < 10; ++it) {
    #ifdef YAVO_LM_PROFILE
                    LMP_MARK(5);
                    if (!have) lm_pass<NT>(S, s_active, na, s_robust, X, uv, s_red, lmp_acc);
                    lmp_t = __builtin_readcyclecounter();
    #else
                    if (!have) lm_pass<NT>(S, s_active, na, s_robust, X, uv, s_red);
    #endif
                    if (tid == 0) {
                        double sys[28];
    #pragma unroll
                        for (int v = 0; v < 28; ++v) sys[v] = S.vals[v];
    #pragma unroll
                        for (int v = 0; v < 28; ++v) S.sys[v] = sys[v];
    #pragma unroll
                        for (int r = 0; r < 6; ++r)
    #pragma unroll
                            for (int c = 0; c <= r; ++c) {
                                S.Hf[r * 6 + c] = sys[r * (r + 1) / 2 + c];
                                S.Hf[c * 6 + r] = sys[r * (r + 1) / 2 + c];
                            }
                        S.currentChi = sys[27];
                        if (it == 0) {
                            double maxDiag = 0;
    #pragma unroll
                            for (int j = 0; j < 6; ++j) {
                                const double d = fabs(sys[j * (j + 1) / 2 + j]);
                                maxDiag = d > maxDiag ? d : maxDiag;
                            }
                            lambda = tau * maxDiag;
                            ni = 2;
                        }
                    }
                    LMP_MARK(7);
                    // trial loop (do ... while (rho < 0 && qmax < 10))
                    int qmax = 0;
                    int f = 0;
                    while (true) {
                        if (tid == 0) {
                            double Tc[7], xs[6];
    #pragma unroll
                            for (int q = 0; q < 7; ++q) Tc[q] = S.T[q];
    #pragma unroll
                            for (int q = 0; q < 7; ++q) S.Tbak[q] = Tc[q];
                            const int ok2 = ldlt6_solve_lds<0>(S.Hf, lambda, S.sys + 21, S.x) ? 1 : 0;
    #pragma unroll
                            for (int q = 0; q < 6; ++q) xs[q] = S.x[q];
                            LMP_MARK(6);
                            double Tn[7], Tnew[7];
                            se3_exp(xs, Tn);
                            se3_mul(Tn, Tc, Tnew);
    #pragma unroll
                            for (int q = 0; q < 7; ++q) S.T[q] = Tnew[q];
                            S.flag = ok2;
                        }
                        LMP_MARK(2);
    #ifdef YAVO_LM_PROFILE
                        lm_pass<NT>(S, s_active, na, s_robust, X, uv, s_red, lmp_acc);
                        lmp_t = __builtin_readcyclecounter();
    #else
                        lm_pass<NT>(S, s_active, na, s_robust, X, uv, s_red);  // errors + system at the trial estimate
    #endif
                        if (tid == 0) {
                            const int ok2 = S.flag;
                            double tempChi = S.vals[27];
                            if (!ok2) tempChi = DBL_MAX;
                            double rho = S.currentChi - tempChi;
                            double scale = 1;
                            if (ok2) {
                                double sc = 0;
                                for (int j = 0; j < 6; ++j) sc += S.x[j] * (lambda * S.x[j] + S.sys[21 + j]);
                                scale = sc + 1e-3;
                            }
                            rho /= scale;
                            int brk = 0, accepted = 0;
                            if (rho > 0 && isfinite(tempChi) && ok2) {
                                double t = 2 * rho - 1;
                                double alpha = 1. - cube_cr(t);  // pow(t, 3), correctly rounded
                                alpha = alpha < goodUpper ? alpha : goodUpper;
                                double sf = goodLower > alpha ? goodLower : alpha;
                                lambda *= sf;
                                ni = 2;
                                S.currentChi = tempChi;
                                accepted = 1;
                            } else {
                                lambda *= ni;
                                ni *= 2;
                                for (int q = 0; q < 7; ++q) S.T[q] = S.Tbak[q];
                                if (!isfinite(lambda)) brk = 1;
                            }
                            qmax++;
                            const bool again = !brk && rho < 0 && qmax < 10;
                            int fl = again ? 1 : 0;
                            if (!again) fl = (qmax == 10 || rho == 0 || !isfinite(lambda)) ? 2 : 0;
                            S.flag = fl | (accepted << 2);
                        }
                        __syncthreads();
                        f = S.flag;
                        __syncthreads();
                        LMP_MARK(3);
                        if ((f & 3) == 1) continue;
                        break;
                    }
                    if ((f & 3) == 2) break;
                    have = (f & 4) != 0;
                }
            }
            __syncthreads();
            // classify: previous outliers are recomputed at the final estimate (e->computeError()); the
            // active edges keep the error of the last computeActiveErrors, i.e. at the last TRIAL estimate
            // Tlast (possibly a rejected one) -- recomputed here from Tlast, bit-identical to the stored value
            double T[7], Tl[7], K[9];
            for (int q = 0; q < 7; ++q) T[q] = uni_f64(S.T[q]);
            for (int q = 0; q < 7; ++q) Tl[q] = uni_f64(S.Tlast[q]);
            for (int q = 0; q < 9; ++q) K[q] = uni_f64(S.K[q]);
            int cnt = 0, chg = 0;
            for (int i = tid; i < n; i += NT) {
                double ee[2];
                const double mi[2] = {(double)uv[2 * i], (double)uv[2 * i + 1]};
                edge_error(s_out[i] ? T : Tl, K, X + 3 * i, mi, ee);
                const double c2 = ee[0] * ee[0] + ee[1] * ee[1];
                const uint8_t lev = c2 > chi2th ? 1 : 0;
                chg |= lev != s_level[i];
                s_out[i] = lev;
                s_level[i] = lev;
                cnt += lev;
                if (round == 2) s_robust[i] = 0;
            }
            int tot = 0;
            block_excl_scan_geom<NT>(cnt, s_tmp, &tot);
            outlierCount = tot;
            hub = S.hub;  // read before the barrier: the next executed round's lane 0 clears S.hub right after it
            changed = __syncthreads_or(chg);
            LMP_MARK(4);
        } else if (round == 2) {  // a replayed round 2 still drops the Huber kernels
            for (int i = tid; i < n; i += NT) s_robust[i] = 0;
            __syncthreads();
        }
        // round + 1 replays the last executed round iff no edge changed level and, across the Huber drop after round 2,
        // no pass of that round applied a Huber weight (`hub` is that round's: replayed rounds run no pass).  Every
        // wave takes the same decision: `changed` comes from the barrier vote and `hub` from a read every wave made
        // before that barrier.
        replay = !changed && (round != 2 || hub == 0);
    }
    if (tid < 7) poses[7 * prob + tid] = S.T[tid];
    for (int i = tid; i < n; i += NT) outlier_all[e0 + i] = s_out[i];
    if (tid == 0) inliers[prob] = n - outlierCount;
    __syncthreads();  // the next problem reinitialises the shared state
    }
    LMP_STORE();
}

template <int NT>
__global__ __launch_bounds__(NT) YAVO_LM_ATTR void pose_lm_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ counts,
                                                      int stride, const double* __restrict__ Xall,
                                                      const double* __restrict__ uvall, const double* __restrict__ Kall,
                                                      const double* priors, double* poses,
                                                      uint8_t* __restrict__ outlier_all, int32_t* __restrict__ inliers,
                                                      int n_prob) {
    pose_lm_body<NT>(offsets, counts, stride, Xall, uvall, Kall, priors, poses, outlier_all, inliers, n_prob);
}

__global__ __launch_bounds__(kNT) void pose_gn_kernel(const int32_t* __restrict__ offsets, const double* __restrict__ Xall,
                                                      const double* __restrict__ uvall, const double* __restrict__ Kall,
                                                      double* __restrict__ poses, int32_t* __restrict__ iters_out) {
    __shared__ double s_red[kLMVals * 128];
    __shared__ double s_vals[32];
    __shared__ double s_T[7];
    __shared__ int s_flag;
    const int prob = blockIdx.x;
    const int tid = threadIdx.x;
    const int e0 = offsets[prob];
    const int n = offsets[prob + 1] - e0;
    const double* X = Xall + 3 * (int64_t)e0;
    const double* uv = uvall + 2 * (int64_t)e0;
    double K[9];
    for (int q = 0; q < 9; ++q) K[q] = Kall[9 * prob + q];
    if (tid < 7) s_T[tid] = poses[7 * prob + tid];
    __syncthreads();
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    double lastCost = 0;
    int acc = 0;
    for (int iter = 0; iter < 10; iter++) {
        double T[7];
        for (int q = 0; q < 7; ++q) T[q] = s_T[q];
        double part[kLMVals];
        for (int v = 0; v < kLMVals; ++v) part[v] = 0.0;
        for (int i = tid; i < n; i += kNT) {
            double pc[3];
            se3_act(T, X + 3 * i, pc);
            double inv_z = 1.0 / pc[2];
            double inv_z2 = inv_z * inv_z;
            double proj0 = fx * pc[0] / pc[2] + cx, proj1 = fy * pc[1] / pc[2] + cy;
            double ee0 = uv[2 * i] - proj0, ee1 = uv[2 * i + 1] - proj1;
            part[27] = part[27] + (ee0 * ee0 + ee1 * ee1);
            double J[12] = {-fx * inv_z, 0, fx * pc[0] * inv_z2, fx * pc[0] * pc[1] * inv_z2,
                            -fx - fx * pc[0] * pc[0] * inv_z2, fx * pc[1] * inv_z,
                            0, -fy * inv_z, fy * pc[1] * inv_z2, fy + fy * pc[1] * pc[1] * inv_z2,
                            -fy * pc[0] * pc[1] * inv_z2, -fy * pc[0] * inv_z};
            int v = 0;
            for (int r = 0; r < 6; ++r) {
                for (int c = 0; c <= r; ++c) {
                    part[v] = part[v] + (J[r] * J[c] + J[6 + r] * J[6 + c]);
                    ++v;
                }
                part[21 + r] = part[21 + r] + ((-J[r]) * ee0 + (-J[6 + r]) * ee1);
            }
        }
        tree_reduce<kLMVals>(part, s_red, s_vals);
        if (tid == 0) {
            double H[36], b[6], dx[6];
            int v = 0;
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c <= r; ++c) {
                    H[r * 6 + c] = s_vals[v];
                    H[c * 6 + r] = s_vals[v];
                    ++v;
                }
            for (int r = 0; r < 6; ++r) b[r] = s_vals[21 + r];
            const double cost = s_vals[27];
            ldlt6_solve<1>(H, b, dx);
            int stop = 0;
            if (isnan(dx[0])) stop = 1;
            else if (iter > 0 && cost >= lastCost) stop = 1;
            else {
                double Tn[7], Tnew[7], Tc[7];
                for (int q = 0; q < 7; ++q) Tc[q] = s_T[q];
                se3_exp(dx, Tn);
                se3_mul(Tn, Tc, Tnew);
                for (int q = 0; q < 7; ++q) s_T[q] = Tnew[q];
                lastCost = cost;
                acc++;
                double q0 = dx[0] * dx[0] + (dx[2] * dx[2] + dx[4] * dx[4]);
                double q1 = dx[1] * dx[1] + (dx[3] * dx[3] + dx[5] * dx[5]);
                if (sqrt(q0 + q1) < 1e-6) stop = 1;
            }
            s_flag = stop;
        }
        __syncthreads();
        const int stop = s_flag;
        __syncthreads();
        if (stop) break;
    }
    if (tid < 7) poses[7 * prob + tid] = s_T[tid];
    if (tid == 0) iters_out[prob] = acc;
}

// Threads per pose-LM workgroup: 256, one wave per SIMD (the LM is latency-bound: 64 / 128 threads measured 2.1 /
// 1.5 ms against 1.0 ms per 256-frame batch).  The summation order follows (yv_lm_sum_mode 6).  Measured and not kept
// (DESIGN.md 4.3, 10): fewer workgroups looping over the problems, LDS padding to one workgroup per CU, and a form
// holding each problem's edges in LDS.
constexpr int kLMThreads = 256;
// A few problems (the host-pointer yv_pose_lm of the LoopHandler, small yv_pose_lm_batch calls, the tracks of a small
// batch such as the sequence front end's 20-frame chunks) leave most CUs idle, so their latency is what counts: 512
// threads, two waves per SIMD of the problem's own CU, halve each thread's edge share (sum order 7,
// yv_pose_lm_sum_mode / yv_track_lm_sum_mode).  Larger batches keep 256 (two problems per CU interleave there).
constexpr int kLMThreadsWide = 512;
constexpr int kLMWideMaxProblems = 256;

template <int NT = kLMThreads, typename... A>
void launch_lm(int n, hipStream_t s, A... args) {
    hipLaunchKernelGGL(pose_lm_kernel<NT>, dim3(n), dim3(NT), 0, s, args..., n);
}

constexpr int lm_mode_of(int nt) { return nt == 512 ? 7 : nt == 256 ? 6 : nt == 128 ? 5 : 4; }

}  // namespace geom

void launch_pose_lm(const int32_t* offsets, int n_problems, const double* X, const double* uv, const double* K,
                    double* poses, uint8_t* outlier, int32_t* inliers, hipStream_t s) {
    if (n_problems <= geom::kLMWideMaxProblems)
        geom::launch_lm<geom::kLMThreadsWide>(n_problems, s, offsets, static_cast<const int32_t*>(nullptr), 0, X, uv, K,
                                              static_cast<const double*>(poses), poses, outlier, inliers);
    else
        geom::launch_lm(n_problems, s, offsets, static_cast<const int32_t*>(nullptr), 0, X, uv, K,
                        static_cast<const double*>(poses), poses, outlier, inliers);
}

void launch_track_pose(int n_tracks, const int32_t* edge_count, int stride, const double* edge_X,
                       const double* edge_uv, const double* K, const double* priors, double* poses,
                       uint8_t* edge_outlier, int32_t* inliers, hipStream_t s) {
    if (n_tracks <= 0) return;
    if (n_tracks <= geom::kLMWideMaxProblems)
        geom::launch_lm<geom::kLMThreadsWide>(n_tracks, s, static_cast<const int32_t*>(nullptr), edge_count, stride,
                                              edge_X, edge_uv, K, priors, poses, edge_outlier, inliers);
    else
        geom::launch_lm(n_tracks, s, static_cast<const int32_t*>(nullptr), edge_count, stride, edge_X, edge_uv, K,
                        priors, poses, edge_outlier, inliers);
}

void launch_pose_gn(const int32_t* offsets, int n_problems, const double* X, const double* uv, const double* K,
                    double* poses, int32_t* iters, hipStream_t s) {
    hipLaunchKernelGGL(geom::pose_gn_kernel, dim3(n_problems), dim3(geom::kNT), 0, s, offsets, X, uv, K, poses, iters);
}

}  // namespace yavo

extern "C" int yv_lm_sum_mode(void) { return yavo::geom::lm_mode_of(yavo::geom::kLMThreads); }

extern "C" int yv_track_lm_sum_mode(int n_tracks) {
    return yavo::geom::lm_mode_of(n_tracks <= yavo::geom::kLMWideMaxProblems ? yavo::geom::kLMThreadsWide
                                                                             : yavo::geom::kLMThreads);
}

extern "C" int yv_pose_lm_sum_mode(int n_problems) {
    return yavo::geom::lm_mode_of(n_problems <= yavo::geom::kLMWideMaxProblems ? yavo::geom::kLMThreadsWide
                                                                               : yavo::geom::kLMThreads);
}

// ------------------------------------------------------------------------------------------------
// test entry point (tests/test_gpu_pose_degenerate.py; like yv_debug_xlane not part of the public headers)
// ------------------------------------------------------------------------------------------------
// The two LDLT forms the pose kernels instantiate, alone, one system a lane: form 0 = ldlt6_solve_lds<0> on (H, lambda)
// with H, b and x in LDS as the LM holds them; form 1 = ldlt6_solve<1> on H with lambda added on the diagonal (the
// GN's private arrays).  x [n][6], positive [n].
namespace yavo {
namespace geom {
template <int FORM>
__global__ __launch_bounds__(64) void debug_ldlt6_kernel(const double* __restrict__ H, const double* __restrict__ lam,
                                                         const double* __restrict__ b, int n, double* __restrict__ x,
                                                         int32_t* __restrict__ positive) {
    const int lane = threadIdx.x;
    const int k = blockIdx.x * 64 + lane;
    if (k >= n) return;  // no barrier below: every lane works on LDS words of its own
    if constexpr (FORM == 0) {
        __shared__ double s_H[64][36], s_b[64][6], s_x[64][6];
        for (int i = 0; i < 36; ++i) s_H[lane][i] = H[36 * (int64_t)k + i];
        for (int i = 0; i < 6; ++i) s_b[lane][i] = b[6 * (int64_t)k + i];
        const bool pos = ldlt6_solve_lds<0>(s_H[lane], lam[k], s_b[lane], s_x[lane]);
        for (int i = 0; i < 6; ++i) x[6 * (int64_t)k + i] = s_x[lane][i];
        positive[k] = pos ? 1 : 0;
    } else {
        double Hd[36], bd[6], xd[6];
        for (int i = 0; i < 36; ++i) Hd[i] = H[36 * (int64_t)k + i];
        for (int i = 0; i < 6; ++i) Hd[i * 7] = Hd[i * 7] + lam[k];
        for (int i = 0; i < 6; ++i) bd[i] = b[6 * (int64_t)k + i];
        const bool pos = ldlt6_solve<1>(Hd, bd, xd);
        for (int i = 0; i < 6; ++i) x[6 * (int64_t)k + i] = xd[i];
        positive[k] = pos ? 1 : 0;
    }
}

// SE3::exp's sin / cos (yavo_se3.h: the polynomial range, the shared reduction past pi/4, the library past 2^20)
__global__ __launch_bounds__(64) void debug_sincos_kernel(const double* __restrict__ x, int n, double* __restrict__ s,
                                                          double* __restrict__ c) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    s[k] = k_sin(x[k]);
    c[k] = k_cos(x[k]);
}
}  // namespace geom
}  // namespace yavo

// x [n] -> s [n], c [n]: host arrays
extern "C" int yv_debug_sincos(const double* x, int n, double* s, double* c) {
    if (!x || !s || !c || n < 0) return -1;
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    double* d = nullptr;
    if (hipMalloc(&d, 3 * N * sizeof(double)) != hipSuccess) return -2;
    bool ok = hipMemcpy(d, x, N * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(yavo::geom::debug_sincos_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, d, n, d + N,
                           d + 2 * N);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(s, d + N, N * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(c, d + 2 * N, N * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    return ok ? 0 : -2;
}

// H [n][36] row-major symmetric, lambda [n], b [n][6], x [n][6], positive [n]: host arrays
extern "C" int yv_debug_ldlt6(int form, const double* H, const double* lambda, const double* b, int n, double* x,
                              int32_t* positive) {
    if ((form != 0 && form != 1) || !H || !lambda || !b || !x || !positive || n < 0) return -1;
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    const size_t nd = N * (36 + 1 + 6 + 6);
    double* d = nullptr;
    int32_t* dp = nullptr;
    if (hipMalloc(&d, nd * sizeof(double)) != hipSuccess) return -2;
    if (hipMalloc(&dp, N * sizeof(int32_t)) != hipSuccess) {
        (void)hipFree(d);
        return -2;
    }
    double *dH = d, *dl = dH + 36 * N, *db = dl + N, *dx = db + 6 * N;
    bool ok = hipMemcpy(dH, H, 36 * N * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dl, lambda, N * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(db, b, 6 * N * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        if (form == 0)
            hipLaunchKernelGGL(yavo::geom::debug_ldlt6_kernel<0>, dim3((n + 63) / 64), dim3(64), 0, nullptr, dH, dl, db, n,
                               dx, dp);
        else
            hipLaunchKernelGGL(yavo::geom::debug_ldlt6_kernel<1>, dim3((n + 63) / 64), dim3(64), 0, nullptr, dH, dl, db, n,
                               dx, dp);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(x, dx, 6 * N * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(positive, dp, N * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    (void)hipFree(dp);
    return ok ? 0 : -2;
}

#ifdef YAVO_LM_PROFILE
// profiling builds only (lib/libyavo_prof.so): per-workgroup pose-LM phase cycle counts of the last launch
extern "C" int yv_debug_lm_prof(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yavo::geom::g_lm_prof), sizeof(unsigned long long) * 1024 * 10) ==
                   hipSuccess ? 0 : -2;
}
#endif
