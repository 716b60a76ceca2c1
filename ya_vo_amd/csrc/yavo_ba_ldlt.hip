// yavo_ba_ldlt.hip -- the bundle adjustment's dense solve (one launch per damping trial, between ba_schur_kernel and
// ba_step_kernel of yavo_ba.hip): Eigen's LDLT (diagonal pivoting) on the reduced pose system P.S x = P.bs, then the
// solve into P.xp and isPositive into P.scal[2], bit-identical to the oracle's or_ldlt_solve.
//
//   ba_ldlt_reg_kernel    one workgroup, the matrix in registers, column pairs handed between waves through LDS
//                         (n <= 128)
//   ba_ldlt_kernel        larger systems: the same steps on S in global memory
// Of the solver they share only BaParams (its gate, S, bs, xp, tr, scal) and kNT.  yv_ba_debug_ldlt runs the launch
// alone on a caller's system; profiling builds keep per-wave phase cycles (yv_debug_ldlt_prof, tools/ldlt_profile.py).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/yavo/yavo.h"
#include "../../include/yavo/yavo_geom.h"
#include "yavo_host.h"
#include "yavo_internal.h"

namespace yavo {
namespace ba {

// Eigen LDLT on the reduced system (n <= kLdltRegN = 128), bit-identical to the oracle's left-looking
// or_ldlt_solve (diagonal pivoting), in one 512-thread workgroup with no workgroup barrier inside the factorisation:
//  1. The pivot sequence. At step k the oracle takes the first position of the largest |L(i, i)|, i >= k, and L(i, i)
//     for i >= k still holds an original diagonal entry (it is only updated at its own step), so the sequence follows
//     from the diagonal alone. Distinct values (the usual case): it is the descending order, by ranks. Any tie or NaN:
//     wave 0 replays the oracle's scan-and-swap step by step.
//  2. Pivoting commutes with the left-looking factorisation: the oracle swaps untouched original entries in the
//     trailing part and the finished rows of L, so its result equals the unpivoted factorisation of P S P^T (S is
//     bitwise symmetric: each Schur entry is stored to both halves from one value).
//  3. The unpivoted factorisation runs right-looking with the matrix in registers, two columns at a time. The oracle
//     forms column k as acc = L(i, k) - L(i, 0) t_0 - L(i, 1) t_1 - ... (t_j = D(j) L(k, j)) and D(k) = L(k, k) -
//     (L(k, 0) t_0 + ...); a term j applied to every such chain (L(i, c) -= L(i, j) t_j(c), t_j(c) = D(j) L(c, j);
//     dot_i += L(i, j) t_j(i)) in ascending j gives the same operations in the same order per entry. Wave w (of 8, two
//     per SIMD) holds the column pairs q = 8 j + w (columns 2q, 2q + 1) of P S P^T, lane l rows l and l + 64. The wave
//     that holds pair q + 1 finalises both its columns as soon as pair q is published: column 2q + 2 from terms 2q,
//     2q + 1 and its division, then column 2q + 3 with term 2q + 2 taken from its own lanes by v_readlane (no LDS
//     round trip inside the pair) -- at raised wave priority, before its share of the bulk update. A published pair
//     is L(., c) in the column store (kept for the solves), t_c(.) in a ring of kLdltRing pair slots and a per-slot
//     flag (workgroup-scope release / acquire). Every wave then applies the pair's two terms to its live pairs'
//     registers (a finalised pair's registers are dead). A slot is rewritten kLdltRing pairs later, which needs every
//     wave to have read it: a wave owns one of any eight consecutive pairs, so none runs more than eight ahead.
//     Wave 0 also runs the forward solve v(i) -= L(i, k) v(k), in the oracle's order.
//     (Round 4 kept the packed triangle in LDS with one workgroup barrier per column step: 139 us per factorisation
//     at n = 120 in the configs[2] sequence; one column per hand-off with four waves: 84 us.)
//  4. The diagonal and backward solves run on wave 0: the vector in registers (two entries per lane), broadcasts by
//     v_readlane, L read by row from the column store (stride 129 doubles: conflict-free by rows and by columns).
constexpr int kLdltRegN = 128;   // n <= 128: lane l holds rows l and l + 64
constexpr int kLdltWaves = 8;    // 512 threads: two waves per SIMD
constexpr int kLdltPairs = 8;    // column pairs per wave: pair 8 j + w holds columns 16 j + 2 w, 16 j + 2 w + 1
constexpr int kLdltLs = 129;     // column stride of the L store (doubles)
constexpr int kLdltRing = 8;     // published pairs in flight

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffff), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// makes one wave's LDS stores visible to its other lanes' later loads (wave-synchronous phases)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// t_c(r) of a ring slot's term h at [h][tq_index(r)] (row order: each wave loads them lane-distributed)
__device__ __forceinline__ int tq_index(int r) { return r; }

#ifdef YAVO_LM_PROFILE
// profiling builds: shader cycles of lane 0 of each wave in the phases of the LDLT, summed over launches
__device__ unsigned long long g_ldlt_prof[kLdltWaves][8];
#define LDP_DECL unsigned long long ldp_t = __builtin_readcyclecounter(), ldp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define LDP_MARK(q) do { const unsigned long long t_ = __builtin_readcyclecounter(); ldp_acc[q] += t_ - ldp_t; ldp_t = t_; } while (0)
#define LDP_STORE() do { if (l == 0) for (int q_ = 0; q_ < 8; ++q_) atomicAdd(&g_ldlt_prof[w][q_], ldp_acc[q_]); } while (0)
#else
#define LDP_DECL
#define LDP_MARK(q) do {} while (0)
#define LDP_STORE() do {} while (0)
#endif

// pair q + 1 = 8 J + w of this wave: both columns finalised and published (read-only on the registers)
#define LDLT_FIN(J)                                                                                            \
    case J: {                                                                                                  \
        constexpr int jl_ = (J) < kLdltPairs / 2 ? (J) : 0;                                                    \
        /* column an: terms ca, cb, then D(an) and the division */                                             \
        double aa0 = 0.0;                                                                                      \
        if ((J) < kLdltPairs / 2) aa0 = (Al[jl_][0] - lka0 * ta_a) - lkb0 * tb_a;                              \
        const double aa1 = (Ah[J][0] - lka1 * ta_a) - lkb1 * tb_a;                                             \
        const bool va = fabs(da) > 0;                                                                          \
        const double La0 = (J) < kLdltPairs / 2 ? (va ? aa0 / da : aa0) : 0.0;                                 \
        const double La1 = va ? aa1 / da : aa1;                                                                \
        const double ua0 = (J) < kLdltPairs / 2 ? da * La0 : 0.0, ua1 = da * La1;                              \
        if ((J) < kLdltPairs / 2) {                                                                            \
            Lc[an * kLdltLs + r0] = La0;                                                                       \
            tqn[tq0] = ua0;                                                                                    \
        }                                                                                                      \
        Lc[an * kLdltLs + r1] = La1;                                                                           \
        tqn[tq1] = ua1;                                                                                        \
        if (l == 0) Dv[an] = da;                                                                               \
        if (bn < n) {                                                                                          \
            /* column bn: terms ca, cb, an (t_an(bn) from row bn's lane), D(bn) = S(bn, bn) - (dot + L t) */   \
            const double ta_b = readlane_f64(bn < 64 ? ua0 : ua1, bn & 63);                                    \
            const double db = dorb - readlane_f64(bn < 64 ? dot0 + La0 * ua0 : dot1 + La1 * ua1, bn & 63);   \
            double ab0 = 0.0;                                                                                  \
            if ((J) < kLdltPairs / 2) ab0 = ((Al[jl_][1] - lka0 * tc_b) - lkb0 * td_b) - La0 * ta_b;           \
            const double ab1 = ((Ah[J][1] - lka1 * tc_b) - lkb1 * td_b) - La1 * ta_b;                          \
            const bool vb = fabs(db) > 0;                                                                      \
            const double Lb0 = (J) < kLdltPairs / 2 ? (vb ? ab0 / db : ab0) : 0.0;                             \
            const double Lb1 = vb ? ab1 / db : ab1;                                                            \
            if ((J) < kLdltPairs / 2) {                                                                        \
                Lc[bn * kLdltLs + r0] = Lb0;                                                                   \
                tqn[kLdltRegN + tq0] = db * Lb0;                                                               \
            }                                                                                                  \
            Lc[bn * kLdltLs + r1] = Lb1;                                                                       \
            tqn[kLdltRegN + tq1] = db * Lb1;                                                                   \
            if (l == 0) Dv[bn] = db;                                                                           \
        }                                                                                                      \
        __hip_atomic_store(&flag[qn & (kLdltRing - 1)], qn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);   \
    } break;

__global__ __launch_bounds__(64 * kLdltWaves) void ba_ldlt_reg_kernel(BaParams P) {
    if (P.gate && *P.gate) return;  // a skipped phase of the device-driven LM
    __shared__ double Lc[kLdltRegN * kLdltLs];       // L(r, c) at Lc[c * 129 + r]
    __shared__ double tq[kLdltRing][2][kLdltRegN];   // pair q's t_2q(.), t_2q+1(.) in slot q % kLdltRing
    __shared__ double Dv[kLdltRegN];                 // D(k)
    __shared__ double dor[kLdltRegN];                // the diagonal of P S P^T
    __shared__ double dg[kLdltRegN];                 // |diagonal|, permuted as the pivots are taken
    __shared__ double dsv[kLdltRegN];                // the diagonal of S
    __shared__ int perm[kLdltRegN];                  // position -> original index: (P S P^T)(i, j) = S(perm[i], perm[j])
    __shared__ int flag[kLdltRing];                  // the pair a slot holds (-1: none yet)
    __shared__ int s_slow;
    const int n = P.ns, t = threadIdx.x, l = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r0 = l, r1 = l + 64;
    LDP_DECL
    // S is read straight from global memory (L2-resident: the Schur kernel just wrote it): its diagonal here, the
    // registers' entries once the permutation is known (round 4 staged all of S in LDS first: ~4 us more)
    if (t < n) {
        const double d = P.S[(int64_t)t * n + t];
        dg[t] = fabs(d);
        dsv[t] = d;
    }
    if (t < kLdltRing) flag[t] = -1;
    if (t == 0) s_slow = 0;
    __syncthreads();
    // 1. ranks by (|d| descending, index ascending); a tie or a NaN sends the sequence to the replay
    if (t < n) {
        const double d = dg[t];
        int rank = 0;
        bool tie = isnan(d);
        int j = 0;
        for (; j + 8 <= n; j += 8) {
            double o[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) o[u] = dg[j + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                rank += o[u] > d;
                tie |= (o[u] == d && j + u != t);
            }
        }
        for (; j < n; ++j) {
            const double o = dg[j];
            rank += o > d;
            tie |= (o == d && j != t);
        }
        perm[rank] = t;  // a permutation when there is no tie
        if (tie) s_slow = 1;
    }
    __syncthreads();
    if (s_slow) {
        if (t < 64) {
            for (int i = t; i < n; i += 64) perm[i] = i;
            wave_lds_sync();
            for (int k = 0; k < n; ++k) {
                double bv = -1.0;
                int bi = n;
                for (int i = k + t; i < n; i += 64) {
                    const double d = dg[i];
                    if (isnan(d)) continue;
                    if (bi == n || d > bv) {
                        bv = d;
                        bi = i;
                    }
                }
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    const double ov = __shfl_xor(bv, m);
                    const int oi = __shfl_xor(bi, m);
                    if (oi < n && (bi == n || ov > bv || (ov == bv && oi < bi))) {
                        bv = ov;
                        bi = oi;
                    }
                }
                if (isnan(dg[k]) || bi == n) bi = k;
                wave_lds_sync();
                if (t == 0 && bi != k) {
                    const double q = dg[k];
                    dg[k] = dg[bi];
                    dg[bi] = q;
                    const int pq = perm[k];
                    perm[k] = perm[bi];
                    perm[bi] = pq;
                }
                wave_lds_sync();
            }
        }
        __syncthreads();
    }
    // the oracle's first step: a zero (or NaN) pivot ends the factorisation with only its own transposition applied
    // to the matrix and none to the vector
    const int big0 = perm[0];
    const double a00 = dsv[big0];
    const bool brk = !(fabs(a00) > 0);
    __syncthreads();
    if (brk) {
        if (t < n) perm[t] = t == 0 ? big0 : (t == big0 ? 0 : t);
        __syncthreads();
    }
    // 2. P S P^T into registers: Al[j][h] = entry (r0, 16 j + 2 w + h) for the columns below 64, Ah[j][h] = (r1, ...);
    // only the strict lower triangle is read (the rest is never used). S is bitwise symmetric, so entry (r, c) is read
    // as S(perm[c], perm[r]): one row of S per load instruction, all 24 loads of a lane in flight together
    double Al[kLdltPairs / 2][2], Ah[kLdltPairs][2];
    const int tq0 = tq_index(r0), tq1 = tq_index(r1);
    {
        const int p0 = r0 < n ? perm[r0] : 0, p1 = r1 < n ? perm[r1] : 0;
#pragma unroll
        for (int j = 0; j < kLdltPairs; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = 16 * j + 2 * w + h;
                const int pc = c < n ? perm[c] : 0;
                const double* row = P.S + (int64_t)pc * n;
                if (j < kLdltPairs / 2) Al[j < kLdltPairs / 2 ? j : 0][h] = (r0 > c && r0 < n) ? row[p0] : 0.0;
                Ah[j][h] = (r1 > c && r1 < n) ? row[p1] : 0.0;
            }
        if (t < n) dor[t] = dsv[perm[t]];
    }
    // the right-hand side, permuted (a zero first pivot: not permuted) -- wave 0 solves
    double v0 = 0.0, v1 = 0.0;
    if (w == 0) {
        v0 = r0 < n ? P.bs[brk ? r0 : perm[r0]] : 0.0;
        v1 = r1 < n ? P.bs[brk ? r1 : perm[r1]] : 0.0;
    }
    __syncthreads();
    int err = 0;
    if (brk) {
        // the solves read P S P^T as it stands
#pragma unroll
        for (int j = 0; j < kLdltPairs; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = 16 * j + 2 * w + h;
                if (c < n) {
                    if (j < kLdltPairs / 2) Lc[c * kLdltLs + r0] = Al[j < kLdltPairs / 2 ? j : 0][h];
                    Lc[c * kLdltLs + r1] = Ah[j][h];
                }
            }
        if (t < n) Dv[t] = dor[t];
        __syncthreads();
        if (w == 0)
            for (int j = 0; j < n; ++j) {
                const double vj = readlane_f64(j < 64 ? v0 : v1, j & 63);
                const double a0 = Lc[j * kLdltLs + r0], a1 = Lc[j * kLdltLs + r1];
                if (r0 > j && r0 < n) v0 = v0 - a0 * vj;
                if (r1 > j && r1 < n) v1 = v1 - a1 * vj;
            }
    } else {
        // 3. pair 0 (wave 0): column 0 with D(0) = a00 (nonzero here); column 1 from term 0 alone, dot_1 = L(1, 0) t_0(1)
        if (w == 0) {
            const double L00 = Al[0][0] / a00, L01 = Ah[0][0] / a00;
            const double u00 = a00 * L00, u01 = a00 * L01;
            Lc[r0] = L00;
            Lc[r1] = L01;
            tq[0][0][tq0] = u00;
            tq[0][0][tq1] = u01;
            if (l == 0) Dv[0] = a00;
            if (n > 1) {
                const double t01 = readlane_f64(u00, 1);
                const double d1 = dor[1] - readlane_f64(L00 * u00, 1);
                const bool v1ok = fabs(d1) > 0;
                const double b0 = Al[0][1] - L00 * t01, b1 = Ah[0][1] - L01 * t01;
                const double L10 = v1ok ? b0 / d1 : b0, L11 = v1ok ? b1 / d1 : b1;
                Lc[kLdltLs + r0] = L10;
                Lc[kLdltLs + r1] = L11;
                tq[0][1][tq0] = d1 * L10;
                tq[0][1][tq1] = d1 * L11;
                if (l == 0) Dv[1] = d1;
            }
            __hip_atomic_store(&flag[0], 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        double dot0 = 0.0, dot1 = 0.0;  // rows r0, r1: L(r, 0) t_0(r) + L(r, 1) t_1(r) + ... (term 0 assigns)
        const int NP = (n + 1) >> 1;
        LDP_MARK(0);
        for (int q = 0; q < NP; ++q) {
            const int s = q & (kLdltRing - 1);
            for (int spin = 0; __hip_atomic_load(&flag[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != q;) {
                if (++spin > (1 << 24)) {  // never expected: a bounded wait, reported as a failed solve
                    err = 1;
                    break;
                }
                // a short sleep between polls leaves the SIMD's issue slots to the wave finalising the pair
                // (60.2 vs 61 us per factorisation, +1% on the sequence leg: profiles/r05/c54)
                __builtin_amdgcn_s_sleep(1);
            }
            if (err) break;
            LDP_MARK(1);
            const int ca = 2 * q, cb = 2 * q + 1;  // this step's terms (cb == n: absent, odd n)
            const bool hb = cb < n;
            const int qn = q + 1, an = 2 * qn, bn = 2 * qn + 1;
            // the loads the critical path needs first: this wave's rows of columns ca, cb and their t values
            const double lka0 = Lc[ca * kLdltLs + r0], lka1 = Lc[ca * kLdltLs + r1];
            const double lkb0 = Lc[cb * kLdltLs + r0], lkb1 = Lc[cb * kLdltLs + r1];
            const double tka0 = tq[s][0][tq0], tka1 = tq[s][0][tq1];
            const double tkb0 = tq[s][1][tq0], tkb1 = tq[s][1][tq1];
            const double dora = dor[an < n ? an : 0], dorb = dor[bn < n ? bn : 0];
            dot0 = ca == 0 ? lka0 * tka0 : dot0 + lka0 * tka0;
            dot1 = ca == 0 ? lka1 * tka1 : dot1 + lka1 * tka1;
            if (hb) {
                dot0 = dot0 + lkb0 * tkb0;
                dot1 = dot1 + lkb1 * tkb1;
            }
            LDP_MARK(2);
            if (qn < NP && (qn & (kLdltWaves - 1)) == w) {  // this wave holds pair q + 1 (wave-uniform; hb holds)
                __builtin_amdgcn_s_setprio(3);
                double* const tqn = &tq[qn & (kLdltRing - 1)][0][0];
                const double ta_a = readlane_f64(an < 64 ? tka0 : tka1, an & 63);  // t_ca(an)
                const double tb_a = readlane_f64(an < 64 ? tkb0 : tkb1, an & 63);  // t_cb(an)
                const double tc_b = readlane_f64(bn < 64 ? tka0 : tka1, bn & 63);  // t_ca(bn)
                const double td_b = readlane_f64(bn < 64 ? tkb0 : tkb1, bn & 63);  // t_cb(bn)
                const double da = dora - readlane_f64(an < 64 ? dot0 : dot1, an & 63);
                switch (qn >> 3) {
                    LDLT_FIN(0) LDLT_FIN(1) LDLT_FIN(2) LDLT_FIN(3) LDLT_FIN(4) LDLT_FIN(5) LDLT_FIN(6) LDLT_FIN(7)
                    default: break;
                }
                __builtin_amdgcn_s_setprio(0);
                LDP_MARK(3);
            }
            // terms ca, cb on this wave's live pairs (pair 8 j + w > q). The t values of a pair's columns c are
            // v_readlane broadcasts of the lane-distributed t_ca(.), t_cb(.) loaded above (lane c & 63 of the half
            // holding c): LDS broadcast loads of them cost eight waves' worth of LDS return bandwidth every step
#pragma unroll
            for (int j = 0; j < kLdltPairs; ++j) {
                if (8 * j + w > q) {
                    const int cl = (16 * j + 2 * w) & 63;  // wave-uniform lane of this pair's first column
                    const double tax = readlane_f64(j < kLdltPairs / 2 ? tka0 : tka1, cl);
                    const double tay = readlane_f64(j < kLdltPairs / 2 ? tka0 : tka1, cl + 1);
                    if (j < kLdltPairs / 2) {
                        double (&a)[2] = Al[j < kLdltPairs / 2 ? j : 0];
                        a[0] = a[0] - lka0 * tax;
                        a[1] = a[1] - lka0 * tay;
                    }
                    Ah[j][0] = Ah[j][0] - lka1 * tax;
                    Ah[j][1] = Ah[j][1] - lka1 * tay;
                    if (hb) {
                        const double tbx = readlane_f64(j < kLdltPairs / 2 ? tkb0 : tkb1, cl);
                        const double tby = readlane_f64(j < kLdltPairs / 2 ? tkb0 : tkb1, cl + 1);
                        if (j < kLdltPairs / 2) {
                            double (&a)[2] = Al[j < kLdltPairs / 2 ? j : 0];
                            a[0] = a[0] - lkb0 * tbx;
                            a[1] = a[1] - lkb0 * tby;
                        }
                        Ah[j][0] = Ah[j][0] - lkb1 * tbx;
                        Ah[j][1] = Ah[j][1] - lkb1 * tby;
                    }
                }
            }
            if (w == 0) {  // the forward solve's terms ca, cb: rows below each
                const double va = readlane_f64(ca < 64 ? v0 : v1, ca & 63);
                if (r0 > ca && r0 < n) v0 = v0 - lka0 * va;
                if (r1 > ca && r1 < n) v1 = v1 - lka1 * va;
                if (hb) {
                    const double vb = readlane_f64(cb < 64 ? v0 : v1, cb & 63);
                    if (r0 > cb && r0 < n) v0 = v0 - lkb0 * vb;
                    if (r1 > cb && r1 < n) v1 = v1 - lkb1 * vb;
                }
            }
            LDP_MARK(4);
        }
    }
    __syncthreads();
    LDP_MARK(5);
    if (w != 0) {
        LDP_STORE();
        return;  // no barrier below
    }
    // 4. diagonal and backward solves on wave 0: lane l holds positions r0 and r1
    const double d0 = r0 < n ? Dv[r0] : 1.0, d1 = r1 < n ? Dv[r1] : 1.0;
    if (r0 < n) v0 = fabs(d0) > DBL_MIN ? v0 / d0 : 0.0;
    if (r1 < n) v1 = fabs(d1) > DBL_MIN ? v1 / d1 : 0.0;
    // backward, v(i) -= L(j, i) v(j) for j descending: while j >= 64 every row below 64 takes the term (v(j) in the
    // upper half), then only rows below j of the lower half; loads four columns ahead
    {
        int j = n - 1;
        for (; j >= 67; j -= 4) {
            double a0[4], a1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a0[u] = Lc[r0 * kLdltLs + j - u];
                a1[u] = Lc[r1 * kLdltLs + j - u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double vj = readlane_f64(v1, (j - u) & 63);
                v0 = v0 - a0[u] * vj;
                if (r1 < j - u) v1 = v1 - a1[u] * vj;
            }
        }
        for (; j >= 64; --j) {
            const double vj = readlane_f64(v1, j & 63);
            v0 = v0 - Lc[r0 * kLdltLs + j] * vj;
            if (r1 < j) v1 = v1 - Lc[r1 * kLdltLs + j] * vj;
        }
        for (; j >= 3; j -= 4) {
            double a0[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a0[u] = Lc[r0 * kLdltLs + j - u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double vj = readlane_f64(v0, j - u);
                if (r0 < j - u) v0 = v0 - a0[u] * vj;
            }
        }
        for (; j >= 0; --j) {
            const double vj = readlane_f64(v0, j);
            if (r0 < j) v0 = v0 - Lc[r0 * kLdltLs + j] * vj;
        }
    }
    if (r0 < n) P.xp[brk ? r0 : perm[r0]] = v0;
    if (r1 < n) P.xp[brk ? r1 : perm[r1]] = v1;
    // isPositive: the oracle's sign state ends in {0, 1} exactly when no D(k) is negative (a zero first pivot: 0)
    const bool neg = !brk && ((r0 < n && d0 < 0) || (r1 < n && d1 < 0));
    const bool any_neg = __ballot(neg) != 0;
    if (l == 0) {
        P.scal[2] = (any_neg || err) ? 0.0 : 1.0;
        P.scal[3] = err ? 1.0 : 0.0;
    }
    LDP_MARK(6);
    LDP_STORE();
}
#undef LDLT_FIN

// larger systems: the same steps on S in global memory
__global__ __launch_bounds__(256) void ba_ldlt_kernel(BaParams P) {
    if (P.gate && *P.gate) return;  // a skipped phase of the device-driven LM
    extern __shared__ double s_dyn[];  // v [n], temp [n]
    __shared__ double s_pv[kNT];
    __shared__ int s_pi[kNT];
    __shared__ int s_sign, s_break;
    const int n = P.ns, t = threadIdx.x;
    double* S = P.S;
    int* tr = P.tr;
    double* v = s_dyn;
    double* temp = s_dyn + n;
#define LL(i, j) S[(int64_t)(i) * n + (j)]
    if (t == 0) {
        s_sign = 0;
        s_break = 0;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        // pivot: the first index of the largest |L(i, i)|, i >= k (sequential strict '>' scan)
        double bv = -1.0;
        int bi = n;
        for (int i = k + t; i < n; i += kNT) {
            const double d = fabs(LL(i, i));
            if (bi == n || d > bv) {
                bv = d;
                bi = i;
            }
        }
        s_pv[t] = bv;
        s_pi[t] = bi;
        __syncthreads();
        for (int off = kNT / 2; off > 0; off >>= 1) {
            if (t < off) {
                const double ov = s_pv[t + off];
                const int oi = s_pi[t + off];
                if (oi < n && (s_pi[t] == n || ov > s_pv[t] || (ov == s_pv[t] && oi < s_pi[t]))) {
                    s_pv[t] = ov;
                    s_pi[t] = oi;
                }
            }
            __syncthreads();
        }
        // the sequential scan starts from bv = |L(k, k)| and only moves on a strict '>': ties keep the first index
        const int big = s_pi[0];
        __syncthreads();
        if (t == 0) tr[k] = big;
        if (k != big) {
            const int s = n - big - 1;
            for (int j = t; j < k; j += kNT) {
                const double q = LL(k, j);
                LL(k, j) = LL(big, j);
                LL(big, j) = q;
            }
            for (int j = t; j < s; j += kNT) {
                const double q = LL(big + 1 + j, k);
                LL(big + 1 + j, k) = LL(big + 1 + j, big);
                LL(big + 1 + j, big) = q;
            }
            if (t == 0) {
                const double q = LL(k, k);
                LL(k, k) = LL(big, big);
                LL(big, big) = q;
            }
            for (int i = k + 1 + t; i < big; i += kNT) {
                const double q = LL(i, k);
                LL(i, k) = LL(big, i);
                LL(big, i) = q;
            }
        }
        __syncthreads();
        if (k > 0) {
            for (int j = t; j < k; j += kNT) temp[j] = LL(j, j) * LL(k, j);
            __syncthreads();
            for (int i = k + 1 + t; i < n; i += kNT) {
                double acc = LL(i, k);
                for (int j = 0; j < k; ++j) acc = acc - LL(i, j) * temp[j];
                LL(i, k) = acc;
            }
            if (t == 0) {
                double dot = LL(k, 0) * temp[0];
                for (int j = 1; j < k; ++j) dot = dot + LL(k, j) * temp[j];
                LL(k, k) -= dot;
            }
            __syncthreads();
        }
        const double akk = LL(k, k);
        const bool valid = fabs(akk) > 0;
        if (k == 0 && !valid) {
            if (t == 0) s_break = 1;
            for (int j = t; j < n; j += kNT) tr[j] = j;
            __syncthreads();
            break;
        }
        if (n - k - 1 > 0 && valid)
            for (int i = k + 1 + t; i < n; i += kNT) LL(i, k) /= akk;
        if (t == 0) {
            int sign = s_sign;
            if (sign == 1) { if (akk < 0) sign = 3; }
            else if (sign == 2) { if (akk > 0) sign = 3; }
            else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
            s_sign = sign;
        }
        __syncthreads();
    }
    if (s_break && t == 0) s_sign = 0;
    for (int i = t; i < n; i += kNT) v[i] = P.bs[i];
    __syncthreads();
    if (t == 0)
        for (int k = 0; k < n; ++k) {
            const double q = v[k];
            v[k] = v[tr[k]];
            v[tr[k]] = q;
        }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double vj = v[j];
        for (int i = j + 1 + t; i < n; i += kNT) v[i] = v[i] - LL(i, j) * vj;
        __syncthreads();
    }
    for (int i = t; i < n; i += kNT) {
        const double d = LL(i, i);
        if (fabs(d) > DBL_MIN) v[i] /= d;
        else v[i] = 0;
    }
    __syncthreads();
    for (int j = n - 1; j >= 0; --j) {
        const double vj = v[j];
        for (int i = t; i < j; i += kNT) v[i] = v[i] - LL(j, i) * vj;
        __syncthreads();
    }
    if (t == 0)
        for (int k = n - 1; k >= 0; --k) {
            const double q = v[k];
            v[k] = v[tr[k]];
            v[tr[k]] = q;
        }
    __syncthreads();
    for (int i = t; i < n; i += kNT) P.xp[i] = v[i];
    if (t == 0) P.scal[2] = (s_sign == 1 || s_sign == 0) ? 1.0 : 0.0;
#undef LL
}

}  // namespace ba

void launch_ba_ldlt(const BaParams& P, hipStream_t s) {
    if (P.ns > 0 && P.ns <= ba::kLdltRegN)
        hipLaunchKernelGGL(ba::ba_ldlt_reg_kernel, dim3(1), dim3(64 * ba::kLdltWaves), 0, s, P);
    else if (P.ns > 0)
        hipLaunchKernelGGL(ba::ba_ldlt_kernel, dim3(1), dim3(256), sizeof(double) * 2 * P.ns, s, P);
}

}  // namespace yavo

#ifdef YAVO_LM_PROFILE
// profiling builds only (lib/libyavo_prof.so): LDLT phase cycles per wave [8][8], summed since the last call (reset)
extern "C" int yv_debug_ldlt_prof(unsigned long long* out) {
    unsigned long long z[yavo::ba::kLdltWaves * 8] = {};
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpyFromSymbol(out, HIP_SYMBOL(yavo::ba::g_ldlt_prof), sizeof z) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(yavo::ba::g_ldlt_prof), z, sizeof z) != hipSuccess)
        return -2;
    return 0;
}
#endif

extern "C" int yv_ba_debug_ldlt(yv_ctx* ctx, const double* S, int n, const double* b, double* x, int* ok) {
    if (!ctx || !S || !b || !x || !ok || n < 1 || n > 6 * yavo::kBaMaxPoses) return YV_ERR_INVALID;
    if (hipSetDevice(yavo::ctx_device(ctx)) != hipSuccess) return YV_ERR_HIP;
    hipStream_t st = yavo::ctx_stream(ctx);
    double *dS = nullptr, *db = nullptr, *dx = nullptr, *ds = nullptr;
    int32_t* dtr = nullptr;
    const size_t nn = (size_t)n * n;
    yavo::HipOwned mem;  // freed on return
    int rc = YV_OK;
    if (mem.alloc(&dS, nn) != YV_OK || mem.alloc(&db, (size_t)n) != YV_OK || mem.alloc(&dx, (size_t)n) != YV_OK ||
        mem.alloc(&ds, 16) != YV_OK || mem.alloc(&dtr, (size_t)n) != YV_OK)
        rc = YV_ERR_HIP;
    double scal[4] = {0, 0, 0, 0};
    if (rc == YV_OK) {
        yavo::BaParams Q{};
        Q.ns = n;
        Q.S = dS;
        Q.bs = db;
        Q.xp = dx;
        Q.scal = ds;
        Q.tr = dtr;
        if (hipMemcpyAsync(dS, S, sizeof(double) * nn, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(db, b, sizeof(double) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemsetAsync(ds, 0, sizeof(double) * 16, st) != hipSuccess)
            rc = YV_ERR_HIP;
        if (rc == YV_OK) {
            yavo::launch_ba_ldlt(Q, st);
            if (hipGetLastError() != hipSuccess ||
                hipMemcpyAsync(x, dx, sizeof(double) * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(scal, ds, sizeof scal, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                rc = YV_ERR_HIP;
        }
    }
    if (rc == YV_OK) *ok = scal[2] != 0.0 ? 1 : 0;
    return rc;
}
