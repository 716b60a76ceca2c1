// yavo_ldlt6.h -- Eigen's 6 x 6 LDLT on one lane, in the two forms the pose kernels (yavo_pose.hip) instantiate:
// ldlt6_solve on a private matrix (the GN) and ldlt6_solve_lds on a system held in LDS (the LM's damped trials).
// The two bodies repeat the column update, the pivot division with Eigen's sign bookkeeping and the three
// substitutions.  Sharing the column update and the substitutions through __forceinline__ helpers was tried and is
// not kept: every pose kernel kept its floating-point instructions, but debug_ldlt6_kernel<0> came out with another
// register allocation and kernel descriptor (98 -> 96 VGPRs), which a move that promises unchanged code generation
// does not allow (profiles/r20/README.md has the figures).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>

namespace yavo {
namespace ldlt6 {

// Eigen::LDLT<Matrix6d> (diagonal pivoting, Eigen's ldlt_inplace + solve) -- variant 0 subtracts the
// GEMV update term by term (the dynamic-size path g2o's LinearSolverDense takes), variant 1 forms the dot
// first (fixed-size path, test.cc's GN).  Fully unrolled: every index is a compile-time constant and the
// pivot swaps are predicated swaps, so the 6x6 factor lives in registers (a runtime-indexed private array
// would go to scratch memory, one dependent round trip per access).
template <int variant>
__device__ bool ldlt6_solve(const double* Hin, const double* b, double* x) {
    double m[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) m[i] = Hin[i];
    constexpr int n = 6;
    int tr[6];
    int sign = 0;
    int found_zero_pivot = 0;
    bool stop = false;
#pragma unroll
    for (int k = 0; k < n; ++k) {
        if (!stop) {
            int big = k;
            double bv = fabs(m[k * 7]);
#pragma unroll
            for (int i = k + 1; i < n; ++i)
                if (fabs(m[i * 7]) > bv) {
                    bv = fabs(m[i * 7]);
                    big = i;
                }
            tr[k] = big;
#pragma unroll
            for (int c = k + 1; c < n; ++c) {
                if (c == big) {
                    // rows/cols k <-> c of the lower triangle (Eigen's ldlt_inplace swap sequence)
#pragma unroll
                    for (int j = 0; j < k; ++j) {
                        const double t = m[k * 6 + j]; m[k * 6 + j] = m[c * 6 + j]; m[c * 6 + j] = t;
                    }
#pragma unroll
                    for (int j = 0; j < n - c - 1; ++j) {
                        const double t = m[(c + 1 + j) * 6 + k]; m[(c + 1 + j) * 6 + k] = m[(c + 1 + j) * 6 + c];
                        m[(c + 1 + j) * 6 + c] = t;
                    }
                    { const double t = m[k * 7]; m[k * 7] = m[c * 7]; m[c * 7] = t; }
#pragma unroll
                    for (int i = k + 1; i < c; ++i) {
                        const double t = m[i * 6 + k]; m[i * 6 + k] = m[c * 6 + i]; m[c * 6 + i] = t;
                    }
                }
            }
            if (k > 0) {
                double temp[6];
#pragma unroll
                for (int j = 0; j < k; ++j) temp[j] = m[j * 7] * m[k * 6 + j];
                double dot = m[k * 6 + 0] * temp[0];
#pragma unroll
                for (int j = 1; j < k; ++j) dot = dot + m[k * 6 + j] * temp[j];
                m[k * 7] -= dot;
#pragma unroll
                for (int i = k + 1; i < n; ++i) {
                    if (variant == 0) {
                        double acc = m[i * 6 + k];
#pragma unroll
                        for (int j = 0; j < k; ++j) acc = acc - m[i * 6 + j] * temp[j];
                        m[i * 6 + k] = acc;
                    } else {
                        double d = m[i * 6 + 0] * temp[0];
#pragma unroll
                        for (int j = 1; j < k; ++j) d = d + m[i * 6 + j] * temp[j];
                        m[i * 6 + k] = m[i * 6 + k] - d;
                    }
                }
            }
            const double akk = m[k * 7];
            const int valid = fabs(akk) > 0;
            if (k == 0 && !valid) {
                sign = 0;
#pragma unroll
                for (int j = 0; j < n; ++j) tr[j] = j;
                stop = true;
            } else {
                if (k + 1 < n && valid) {
#pragma unroll
                    for (int i = k + 1; i < n; ++i) m[i * 6 + k] /= akk;
                }
                if (!(found_zero_pivot && valid) && !valid) found_zero_pivot = 1;
                if (sign == 1) { if (akk < 0) sign = 3; }
                else if (sign == 2) { if (akk > 0) sign = 3; }
                else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
            }
        } else {
            tr[k] = k;
        }
    }
    const bool positive = (sign == 1 || sign == 0);
    double v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = b[i];
    // v = P b: transpositions applied in order, swap(v[k], v[tr[k]]) with tr[k] >= k
#pragma unroll
    for (int k = 0; k < n; ++k) {
#pragma unroll
        for (int c = k + 1; c < n; ++c)
            if (tr[k] == c) { const double t = v[k]; v[k] = v[c]; v[c] = t; }
    }
#pragma unroll
    for (int j = 0; j < n; ++j)
#pragma unroll
        for (int i = j + 1; i < n; ++i) v[i] = v[i] - m[i * 6 + j] * v[j];
#pragma unroll
    for (int i = 0; i < n; ++i) {
        if (fabs(m[i * 7]) > DBL_MIN) v[i] /= m[i * 7];
        else v[i] = 0;
    }
#pragma unroll
    for (int j = n - 1; j >= 0; --j)
#pragma unroll
        for (int i = 0; i < j; ++i) v[i] = v[i] - m[j * 6 + i] * v[j];
#pragma unroll
    for (int k = n - 1; k >= 0; --k) {
#pragma unroll
        for (int c = k + 1; c < n; ++c)
            if (tr[k] == c) { const double t = v[k]; v[k] = v[c]; v[c] = t; }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = v[i];
    return positive;
}

// The same Eigen LDLT for a symmetric system held in LDS (H + lambda I, the LM trial's damped matrix).
// Eigen's pivot at step k is the largest |diagonal| among rows k..5, and those diagonal entries are still
// the original ones (a row's diagonal is only updated at its own step), so the whole transposition
// sequence follows from the six diagonal values alone.  Pivoted LDLT then performs exactly the arithmetic
// of unpivoted LDLT on P H P^T: the permutation is resolved first, P H P^T's lower triangle is gathered
// from LDS, and the factorization runs straight-line in registers.
// Hf the full symmetric 6x6 (row-major), bs the right-hand side, xs the solution (all LDS); P b and P^T v are indexed
// LDS accesses.
template <int variant>
__device__ bool ldlt6_solve_lds(const double* Hf, double lambda, const double* bs, double* xs) {
    constexpr int n = 6;
    double dg[6];
    int id[6];
#pragma unroll
    for (int i = 0; i < n; ++i) {
        dg[i] = Hf[i * 7] + lambda;
        id[i] = i;
    }
#pragma unroll
    for (int k = 0; k < n; ++k) {
        int big = k;
        double bv = fabs(dg[k]);
#pragma unroll
        for (int i = k + 1; i < n; ++i)
            if (fabs(dg[i]) > bv) {
                bv = fabs(dg[i]);
                big = i;
            }
        const double dk = dg[k];
        const int ik = id[k];
#pragma unroll
        for (int c = k + 1; c < n; ++c) {
            const bool sw = c == big;
            dg[k] = sw ? dg[c] : dg[k];
            id[k] = sw ? id[c] : id[k];
            dg[c] = sw ? dk : dg[c];
            id[c] = sw ? ik : id[c];
        }
    }
    const bool zero0 = !(fabs(dg[0]) > 0);  // Eigen's k == 0 early exit: no transposition, no factorization
    if (zero0) {
#pragma unroll
        for (int i = 0; i < n; ++i) {
            id[i] = i;
            dg[i] = Hf[i * 7] + lambda;
        }
    }
    double m[36];
#pragma unroll
    for (int i = 0; i < n; ++i) {
        const double* row = Hf + id[i] * 6;
#pragma unroll
        for (int j = 0; j < i; ++j) m[i * 6 + j] = row[id[j]];
        m[i * 7] = dg[i];
    }
    int sign = 0;
    int found_zero_pivot = 0;
    if (!zero0) {
#pragma unroll
        for (int k = 0; k < n; ++k) {
            if (k > 0) {
                double temp[6];
#pragma unroll
                for (int j = 0; j < k; ++j) temp[j] = m[j * 7] * m[k * 6 + j];
                double dot = m[k * 6 + 0] * temp[0];
#pragma unroll
                for (int j = 1; j < k; ++j) dot = dot + m[k * 6 + j] * temp[j];
                m[k * 7] -= dot;
#pragma unroll
                for (int i = k + 1; i < n; ++i) {
                    if (variant == 0) {
                        double acc = m[i * 6 + k];
#pragma unroll
                        for (int j = 0; j < k; ++j) acc = acc - m[i * 6 + j] * temp[j];
                        m[i * 6 + k] = acc;
                    } else {
                        double d = m[i * 6 + 0] * temp[0];
#pragma unroll
                        for (int j = 1; j < k; ++j) d = d + m[i * 6 + j] * temp[j];
                        m[i * 6 + k] = m[i * 6 + k] - d;
                    }
                }
            }
            const double akk = m[k * 7];
            const int valid = fabs(akk) > 0;
            if (k + 1 < n && valid) {
#pragma unroll
                for (int i = k + 1; i < n; ++i) m[i * 6 + k] /= akk;
            }
            if (!(found_zero_pivot && valid) && !valid) found_zero_pivot = 1;
            if (sign == 1) { if (akk < 0) sign = 3; }
            else if (sign == 2) { if (akk > 0) sign = 3; }
            else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
        }
    }
    const bool positive = (sign == 1 || sign == 0);
    double v[6];
#pragma unroll
    for (int i = 0; i < n; ++i) v[i] = bs[id[i]];  // v = P b
#pragma unroll
    for (int j = 0; j < n; ++j)
#pragma unroll
        for (int i = j + 1; i < n; ++i) v[i] = v[i] - m[i * 6 + j] * v[j];
#pragma unroll
    for (int i = 0; i < n; ++i) {
        if (fabs(m[i * 7]) > DBL_MIN) v[i] /= m[i * 7];
        else v[i] = 0;
    }
#pragma unroll
    for (int j = n - 1; j >= 0; --j)
#pragma unroll
        for (int i = 0; i < j; ++i) v[i] = v[i] - m[j * 6 + i] * v[j];
#pragma unroll
    for (int i = 0; i < n; ++i) xs[id[i]] = v[i];  // x = P^T v
    return positive;
}

}  // namespace ldlt6
}  // namespace yavo
