// yavo_match.hip -- the two brute-force Hamming matchers on the matrix cores (int8 +-1 and FP4) and their dispatch.
//
// Reference functions restated (the reference's file:line):
//   match_kernel        Brief::matchFeatures / hammingDistance  src/BriefDescriptor.cc:139-183
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yavo_internal.h"
#include "yavo_xlane.h"

namespace yavo {

// ------------------------------------------------------------------------------------------------
// Brute-force Hamming matcher on the int8 matrix cores
// ------------------------------------------------------------------------------------------------
// With every descriptor bit b mapped to the int8 value 2b - 1 (+1 / -1), the dot product of two 256-bit
// descriptors is 256 - 2 * Hamming exactly, so a pair's whole distance matrix is an int8 GEMM
// (queries x 256) . (256 x trains) with int32 accumulation: v_mfma_i32_16x16x64_i8 computes a 16 x 16
// distance tile per K-step, four K-steps per tile.  Per query the first minimum (strict <, as
// Brief::matchFeatures) is the maximum of the key (dot << 16) | (0xFFFF - j): larger dot, then smaller j.
// A and B fragments place descriptor element k = 64 s + 16 (lane >> 4) + j in byte j of K-step s of
// their lane, for both operands alike, so the products pair matching bits whatever the hardware's k
// order inside an instruction is.
typedef int mm_v4i __attribute__((ext_vector_type(4)));
constexpr int MM_QT = 8;                  // 16-row query tiles per wave
constexpr int MM_QB = 4 * MM_QT * 16;     // queries per workgroup (4 waves)
constexpr int MM_TC = 128;                // train descriptors per LDS chunk
constexpr int MM_ROW = 17;                // uint4 per expanded train row (16 + 1 pad: conflict-free b128 reads)

// 4 descriptor bits -> 4 bytes of +1 (bit set) / -1 (bit clear), bit i in byte i
__device__ __forceinline__ uint32_t expand_pm1(uint32_t nib) {
    const uint32_t spread = (nib * 0x00204081u) & 0x01010101u;
    return ~(spread * 0xFEu);
}

__device__ __forceinline__ uint4 expand16_pm1(uint32_t bits) {
    return make_uint4(expand_pm1(bits & 0xF), expand_pm1((bits >> 4) & 0xF), expand_pm1((bits >> 8) & 0xF),
                      expand_pm1((bits >> 12) & 0xF));
}

__device__ __forceinline__ int desc_popcount(const Desc& d) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) c += __popc(d.w[w]);
    return c;
}

// Running top-2 of distinct keys: (m1, m2) = the two largest of {m1, m2, x, y}, m1 >= m2 on entry and exit.  The
// larger of m1 and max(x, y) is the new m1; the second is the largest of what is left: min(m1, max(x, y)), m2 and
// min(x, y).  5 VALU per two keys.
__device__ __forceinline__ void top2_push2_i32(int& m1, int& m2, int x, int y) {
    const int hi = max(x, y), lo = min(x, y);
    m2 = max(min(m1, hi), max(m2, lo));
    m1 = max(m1, hi);
}

// Merge of two running pairs over disjoint key sets: the second largest of the union is the smaller head or one of
// the tails.  (A max butterfly on m2 alone would lose the smaller head.)
__device__ __forceinline__ void top2_merge_i32(int& m1, int& m2, int o1, int o2) {
    m2 = max(min(m1, o1), max(m2, o2));
    m1 = max(m1, o1);
}

// the int8 matcher's key -> (distance << 16) | train index
__device__ __forceinline__ uint32_t mm_decode_key(int v) {
    const int dot = v >> 16;
    const uint32_t d = (uint32_t)((256 - dot) >> 1);
    const uint32_t jj = 0xFFFFu - ((uint32_t)v & 0xFFFFu);
    return (d << 16) | jj;
}

// Train lists above 2048 (up to kMaxKp; lists <= 2048 take the FP4 kernel below): the +-1 encoding, dot = 256 -
// 2 Hamming, key = (dot << 16) + 0xFFFF - j formed per element.  TOP2: the keys of one query are distinct (j is in
// the low bits), so the two largest are exactly the nearest and the second nearest train point, ties by index; the
// second goes to match_key2 in the same format (0xFFFFFFFF: no second train point).
template <bool TOP2>
__device__ __forceinline__ void match_body(const Desc* __restrict__ desc, const int32_t* __restrict__ kp_count,
                                           const int32_t* __restrict__ pairs, int max_kp,
                                           uint32_t* __restrict__ match_key, uint32_t* __restrict__ match_key2) {
    __shared__ uint4 s_t[2][MM_TC * MM_ROW];
    const int pair = blockIdx.y;
    const int qi = pairs[2 * pair], ti = pairs[2 * pair + 1];
    const int nq = kp_count[qi], nt = kp_count[ti];
    const int q0 = blockIdx.x * MM_QB;
    if (q0 >= nq) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, g = lane >> 4;
    const Desc* qd = desc + (int64_t)qi * max_kp;
    const uint32_t* tw = reinterpret_cast<const uint32_t*>(desc + (int64_t)ti * max_kp);

    // query fragments: tile qt row (lane & 15) = query q0 + 16 MM_QT wave + 16 qt + (lane & 15)
    mm_v4i A[MM_QT][4];
#pragma unroll
    for (int qt = 0; qt < MM_QT; ++qt) {
        const int q = q0 + 16 * MM_QT * wave + 16 * qt + col;
        const Desc d = qd[q < nq ? q : 0];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t hi_mask = 0u - (uint32_t)(g >> 1);  // blend, not an index: keeps d in registers
            const uint32_t w = d.w[2 * s] ^ ((d.w[2 * s] ^ d.w[2 * s + 1]) & hi_mask);
            const uint32_t bits = (w >> (16 * (g & 1))) & 0xFFFFu;
            const uint4 e = expand16_pm1(bits);
            A[qt][s] = mm_v4i{(int)e.x, (int)e.y, (int)e.z, (int)e.w};
        }
    }
    int best[MM_QT][4];
#pragma unroll
    for (int qt = 0; qt < MM_QT; ++qt)
#pragma unroll
        for (int r = 0; r < 4; ++r) best[qt][r] = INT_MIN;
    int best2[TOP2 ? MM_QT : 1][4];
    if constexpr (TOP2) {
#pragma unroll
        for (int qt = 0; qt < MM_QT; ++qt)
#pragma unroll
            for (int r = 0; r < 4; ++r) best2[qt][r] = INT_MIN;
    }

    // staging: thread -> (train tt = idx >> 4, 16-bit field u = idx & 15), kF fields per thread per chunk
    constexpr int kF = MM_TC * 16 / 256;  // 16-bit fields per thread per chunk
    uint32_t pre[kF];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int k = 0; k < kF; ++k) {
            const int idx = tid + 256 * k, tt = idx >> 4, u = idx & 15;
            const int t = t0 + tt;
            pre[k] = t < nt ? tw[(int64_t)t * 8 + (u >> 1)] : 0u;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int k = 0; k < kF; ++k) {
            const int idx = tid + 256 * k, tt = idx >> 4, u = idx & 15;
            const uint32_t bits = (pre[k] >> (16 * (u & 1))) & 0xFFFFu;
            s_t[buf][tt * MM_ROW + u] = expand16_pm1(bits);
        }
    };
    if (nt > 0) {
        fetch(0);
        store(0);
    }
    int buf = 0;
    for (int t0 = 0; t0 < nt; t0 += MM_TC) {
        const bool more = t0 + MM_TC < nt;
        if (more) fetch(t0 + MM_TC);
        __syncthreads();
        // two 16-column train tiles per pass: four independent MFMA chains, and one v_max3 folds both tiles' keys
        // into the running maximum
#pragma unroll
        for (int tt0 = 0; tt0 < MM_TC; tt0 += 32) {
            if (t0 + tt0 >= nt) break;
            mm_v4i Ba[4], Bb[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint4 va = s_t[buf][(tt0 + col) * MM_ROW + 4 * s + g];
                const uint4 vb = s_t[buf][(tt0 + 16 + col) * MM_ROW + 4 * s + g];
                Ba[s] = mm_v4i{(int)va.x, (int)va.y, (int)va.z, (int)va.w};
                Bb[s] = mm_v4i{(int)vb.x, (int)vb.y, (int)vb.z, (int)vb.w};
            }
            // a column past nt (including the whole second tile at the end of the list) gets -2^30, below every
            // real key and above INT_MIN, so no per-element select and no branch are needed
            const int ja = t0 + tt0 + col, jb = ja + 16;
            {
                // key = (dot << 16) + bias: bias = 0xFFFF - j for a real train column
                const int bias_a = ja < nt ? 0xFFFF - ja : -(1 << 30);
                const int bias_b = jb < nt ? 0xFFFF - jb : -(1 << 30);
#pragma unroll
                for (int qt = 0; qt < MM_QT; qt += 2) {
                    mm_v4i a0 = {0, 0, 0, 0}, b0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[qt][s], Ba[s], a0, 0, 0, 0);
                        b0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[qt][s], Bb[s], b0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[qt + 1][s], Ba[s], a1, 0, 0, 0);
                        b1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[qt + 1][s], Bb[s], b1, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if constexpr (TOP2) {
                            top2_push2_i32(best[qt][r], best2[qt][r], (int)(((uint32_t)a0[r] << 16) + (uint32_t)bias_a),
                                           (int)(((uint32_t)b0[r] << 16) + (uint32_t)bias_b));
                            top2_push2_i32(best[qt + 1][r], best2[qt + 1][r],
                                           (int)(((uint32_t)a1[r] << 16) + (uint32_t)bias_a),
                                           (int)(((uint32_t)b1[r] << 16) + (uint32_t)bias_b));
                            continue;
                        }
                        best[qt][r] = max(best[qt][r], max((int)(((uint32_t)a0[r] << 16) + (uint32_t)bias_a),
                                                           (int)(((uint32_t)b0[r] << 16) + (uint32_t)bias_b)));
                        best[qt + 1][r] = max(best[qt + 1][r],
                                              max((int)(((uint32_t)a1[r] << 16) + (uint32_t)bias_a),
                                                  (int)(((uint32_t)b1[r] << 16) + (uint32_t)bias_b)));
                    }
                }
            }
        }
        if (more) {
            store(buf ^ 1);  // the other buffer: last read before the barrier at the top of this chunk
            buf ^= 1;
        }
    }
    // per query row: max over the 16 lanes (train columns) of its lane group
#pragma unroll
    for (int qt = 0; qt < MM_QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int v = best[qt][r];
            const int q = q0 + 16 * MM_QT * wave + 16 * qt + 4 * g + r;
            if constexpr (TOP2) {
                // the lanes of a butterfly level hold the pairs of disjoint train columns: a pair merge per level
                int v2 = best2[qt][r];
                top2_merge_i32(v, v2, xl::xor_row_i32<8>(v), xl::xor_row_i32<8>(v2));
                top2_merge_i32(v, v2, xl::xor_row_i32<4>(v), xl::xor_row_i32<4>(v2));
                top2_merge_i32(v, v2, xl::xor_row_i32<2>(v), xl::xor_row_i32<2>(v2));
                top2_merge_i32(v, v2, xl::xor_row_i32<1>(v), xl::xor_row_i32<1>(v2));
                if (col == r && q < nq) {
                    // a real key is >= -2^24; a column past the list (-2^30 + ...) and the initial INT_MIN are not
                    match_key[(int64_t)pair * max_kp + q] = v > -(1 << 29) ? mm_decode_key(v) : 0xFFFFFFFFu;
                    match_key2[(int64_t)pair * max_kp + q] = v2 > -(1 << 29) ? mm_decode_key(v2) : 0xFFFFFFFFu;
                }
                continue;
            }
            v = max(v, xl::xor_row_i32<8>(v));  // DPP butterflies inside the 16-lane group (yavo_xlane.h)
            v = max(v, xl::xor_row_i32<4>(v));
            v = max(v, xl::xor_row_i32<2>(v));
            v = max(v, xl::xor_row_i32<1>(v));
            if (col == r && q < nq) {
                uint32_t key = 0xFFFFFFFFu;  // empty train set (nt >= 1 always leaves a real key in the row max)
                if (v != INT_MIN) {
                    const int dot = v >> 16;
                    const uint32_t d = (uint32_t)((256 - dot) >> 1);
                    const uint32_t jj = 0xFFFFu - ((uint32_t)v & 0xFFFFu);
                    key = (d << 16) | jj;
                }
                match_key[(int64_t)pair * max_kp + q] = key;
            }
        }
    }
}

__global__ __launch_bounds__(256) void match_kernel(const Desc* __restrict__ desc, const int32_t* __restrict__ kp_count,
                                                    const int32_t* __restrict__ pairs, int max_kp,
                                                    uint32_t* __restrict__ match_key) {
    match_body<false>(desc, kp_count, pairs, max_kp, match_key, nullptr);
}

__global__ __launch_bounds__(256) void match_top2_kernel(const Desc* __restrict__ desc,
                                                         const int32_t* __restrict__ kp_count,
                                                         const int32_t* __restrict__ pairs, int max_kp,
                                                         uint32_t* __restrict__ match_key,
                                                         uint32_t* __restrict__ match_key2) {
    match_body<true>(desc, kp_count, pairs, max_kp, match_key, match_key2);
}

// ------------------------------------------------------------------------------------------------
// The same matcher on the FP4 matrix cores (train lists <= 2048)
// ------------------------------------------------------------------------------------------------
// v_mfma_scale_f32_32x32x64_f8f6f4 with both operands FP4 (e2m1): every descriptor bit becomes the FP4 value b
// (nibble 0b0010 = 1.0, 0b0000 = 0) and both E8M0 block scales are 2^6, so every product is 4096 * a_k * b_k: exact.
// The accumulator is f32 and every partial sum an integer of magnitude < 2^22 (the chain starts from
// c_j = (2047 - j) - 2048 * popcount(b_j) + 2^21 and adds 4096 * popcount(a & b) <= 2^20), so every sum is exact in
// any order and the chain ends at the int8 kernel's key plus 2^21 exactly:
//   key' = 2048 * (pa - Hamming) + (2047 - j) + 2^21 >= 2^21 - 2^19.
// Every key' is a positive float (a train row past the list starts at 0 and, its staged descriptor being zero, stays
// 0), and positive floats order as their bit patterns, so the running maximum is v_max3_u32 on the raw bits (a float
// max would first canonicalise both MFMA results).
//
// Train descriptors are the A operand (rows), queries B (columns).  A 32 x 32 x 64 tile takes 32 cycles and holds
// the SIMD's vector issue for 8 of them, where the 16 x 16 x 128 form holds 8 of 16 (MI355X_MICROARCH.md), so the
// running maxima and the staging get 24 free issue cycles per MFMA instead of 8 (tools/mfma_fp4_probe.hip: both
// forms alone 0.91-0.96 of the FP4 peak at 3 waves per SIMD, their matcher loops without LDS 0.83-0.84; the kernel
// 1.48 -> 1.43 ms per 4096-pair step, profiles/r06/c12, c14).  With the train list on the rows, a lane's 16
// accumulators are 16 train descriptors of ONE query, so each query tile keeps one running maximum per lane (the two
// lane halves merge at the end), and the chain start C(row) = c_j is four ds_read_b128 of the staged c row per
// 32-train block, shared by every query tile of the wave (no broadcast moves).  Lane (n, h = lane >> 5) of a K-step s
// holds descriptor dword 2 s + h of its train row / query column, for A and B alike; inside a dword the nibble order
// is a fixed permutation of the bits (the same for A and B), so the products pair matching bits.
constexpr int MF_TC = 128;               // train descriptors per LDS chunk
constexpr int MF_ROW = 9;                // uint4 per expanded train row (8 + 1 pad)
constexpr int MF2_QT = 4, MF2_WPE = 3;   // the top-2 instantiation's query tiles per wave and waves per SIMD

// 32 descriptor bits -> 32 FP4 nibbles (1.0 / 0) in four dwords: bit 4i + k lands in bit 1 of nibble i of dword k,
// one mask per dword (and a shift for three of them): 7 VALU per descriptor dword, where spreading each byte
// with two v_mul_u32_u24 took 34
__device__ __forceinline__ uint4 expand32_fp4(uint32_t w) {
    constexpr uint32_t kBit1 = 0x22222222u;
    return make_uint4((w << 1) & kBit1, w & kBit1, (w >> 1) & kBit1, (w >> 2) & kBit1);
}

typedef int mf_v8i __attribute__((ext_vector_type(8)));
typedef float mf_v16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ mf_v16f mfma_fp4_32(const mm_v4i& a, const mm_v4i& b, const mf_v16f& c) {
    // FP4 operands use 4 of the 8 operand registers (the backend narrows them); scales 133 = 2^(133-127) = 64
    const mf_v8i a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, -1, -1, -1, -1);
    const mf_v8i b8 = __builtin_shufflevector(b, b, 0, 1, 2, 3, -1, -1, -1, -1);
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 133, 0, 133);
}

// running maximum of the 16 keys' of one accumulator (positive floats: bit patterns order as the values)
__device__ __forceinline__ uint32_t max16_u32(uint32_t best, const mf_v16f& a) {
    auto u = [&](int i) { return __float_as_uint(a[i]); };
    const uint32_t m0 = max(u(0), max(u(1), u(2))), m1 = max(u(3), max(u(4), u(5)));
    const uint32_t m2 = max(u(6), max(u(7), u(8))), m3 = max(u(9), max(u(10), u(11)));
    const uint32_t m4 = max(u(12), max(u(13), u(14)));
    const uint32_t m5 = max(m0, max(m1, m2)), m6 = max(m3, max(m4, u(15)));
    return max(best, max(m5, m6));
}

// ---- top-2 (the 2-NN mode) ----
// The keys' of one query are distinct (the train index is in the low bits), so the two largest keys' are exactly
// (d1, j1) and (d2, j2): the nearest train point and the nearest of the others, ties by the smaller index.  A row past
// the list and the initial value are 0, below every real key'.  All keys' are non-negative finite floats, whose order
// is that of their bit patterns: heads and tails are compared as u32, and the one median needed is v_med3_f32 on the
// same bits (no NaN, no denormal: it returns one of its operands unchanged).
__device__ __forceinline__ uint32_t umed3_pos(uint32_t a, uint32_t b, uint32_t c) {
    return __float_as_uint(__builtin_amdgcn_fmed3f(__uint_as_float(a), __uint_as_float(b), __uint_as_float(c)));
}

// Three sorted pairs (head >= tail) over disjoint keys -> the top-2 of their union, 4 VALU: the largest is the
// largest head; the second is the median head or the winner's tail, and the other two tails are below their own
// heads, hence below the median head, so the maximum of all three tails may stand for the winner's.
__device__ __forceinline__ void top2_merge3(uint32_t h0, uint32_t l0, uint32_t h1, uint32_t l1, uint32_t h2,
                                            uint32_t l2, uint32_t& m1, uint32_t& m2) {
    m1 = max(h0, max(h1, h2));
    m2 = max(umed3_pos(h0, h1, h2), max(l0, max(l1, l2)));
}

// The running pair and the 16 keys' of one accumulator: five triples give five sorted pairs (max3 + med3 each); with
// the sixteenth key (tail 0) and the running pair that is seven pairs, merged three at a time.  22 VALU per
// accumulator (the chain m2 = med3(m1, m2, x), m1 = max(m1, x) takes 32; the 1-NN maximum 8).
__device__ __forceinline__ void top2_16_u32(uint32_t& m1, uint32_t& m2, const mf_v16f& a) {
    auto u = [&](int i) { return __float_as_uint(a[i]); };
    uint32_t h[5], l[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        h[k] = max(u(3 * k), max(u(3 * k + 1), u(3 * k + 2)));
        l[k] = umed3_pos(u(3 * k), u(3 * k + 1), u(3 * k + 2));
    }
    uint32_t a1, a2, b1, b2;
    top2_merge3(h[0], l[0], h[1], l[1], h[2], l[2], a1, a2);
    top2_merge3(h[3], l[3], h[4], l[4], u(15), 0u, b1, b2);
    top2_merge3(a1, a2, b1, b2, m1, m2, m1, m2);
}

// key' -> (distance << 16) | train index, pa = the query's popcount
__device__ __forceinline__ uint32_t fp4_decode_key(uint32_t bits, int pa) {
    const int iv = (int)__uint_as_float(bits) - (1 << 21);
    const uint32_t d = (uint32_t)(pa - (iv >> 11));
    const uint32_t jj = 2047u - ((uint32_t)iv & 2047u);
    return (d << 16) | jj;
}

template <int QT, int WPE, bool TOP2>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void match_fp4_kernel(
    const Desc* __restrict__ desc, const int32_t* __restrict__ kp_count, const int32_t* __restrict__ pairs, int max_kp,
    uint32_t* __restrict__ match_key, uint32_t* __restrict__ match_key2) {
    constexpr int QB = 4 * QT * 32;  // queries per workgroup
    __shared__ uint4 s_t[2][MF_TC * MF_ROW];
    __shared__ float s_c[2][MF_TC];  // c_j = (2047 - j) - 2048 popcount(b_j) + 2^21, 0 past the list
    const int pair = blockIdx.y;
    const int qi = pairs[2 * pair], ti = pairs[2 * pair + 1];
    const int nq = kp_count[qi], nt = kp_count[ti];
    const int q0 = blockIdx.x * QB;
    if (q0 >= nq) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = lane & 31, h = lane >> 5;
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(desc + (int64_t)qi * max_kp);
    const uint32_t* tw = reinterpret_cast<const uint32_t*>(desc + (int64_t)ti * max_kp);

    // query fragments: tile qt column n = query q0 + 32 QT wave + 32 qt + n; the lane loads only its own four dwords
    // (a whole-descriptor load with a lane-dependent pick went through scratch)
    mm_v4i B[QT][4];
    uint32_t raw[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int q = q0 + 32 * QT * wave + 32 * qt + n;
        const uint32_t* w = qw + (int64_t)(q < nq ? q : 0) * 8 + h;
#pragma unroll
        for (int s = 0; s < 4; ++s) raw[qt][s] = w[2 * s];
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint4 e = expand32_fp4(raw[qt][s]);
            B[qt][s] = mm_v4i{(int)e.x, (int)e.y, (int)e.z, (int)e.w};
        }
    uint32_t best[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) best[qt] = 0u;
    uint32_t best2[TOP2 ? QT : 1];
    if constexpr (TOP2) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) best2[qt] = 0u;
    }

    // staging: thread -> (train tt = idx >> 3, descriptor dword u = idx & 7), kF dwords per thread per chunk; train
    // tt's chain start c_j from the popcounts of its 8 dwords, summed over their 8 consecutive lanes by DPP (waves 0-1
    // re-reading the chunk's descriptors for it stalled the workgroup on those loads at every chunk)
    constexpr int kF = MF_TC * 8 / 256;
    uint32_t pre[kF];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int k = 0; k < kF; ++k) {
            const int idx = tid + 256 * k, tt = idx >> 3, u = idx & 7;
            const int t = t0 + tt;
            pre[k] = t < nt ? tw[(int64_t)t * 8 + u] : 0u;
        }
    };
    auto store = [&](int buf, int t0) {
#pragma unroll
        for (int k = 0; k < kF; ++k) {
            const int idx = tid + 256 * k, tt = idx >> 3, u = idx & 7;
            s_t[buf][tt * MF_ROW + u] = expand32_fp4(pre[k]);
            uint32_t pc = __builtin_popcount(pre[k]);
            pc += xl::dpp<0xB1>(pc);
            pc += xl::dpp<0x4E>(pc);
            pc += xl::dpp<0x141>(pc);
            const int t = t0 + tt;
            if (u == 0) s_c[buf][tt] = t < nt ? (float)((2047 - t) - 2048 * (int)pc + (1 << 21)) : 0.f;
        }
    };
    if (nt > 0) {
        fetch(0);
        store(0, 0);
    }
    int buf = 0;
    for (int t0 = 0; t0 < nt; t0 += MF_TC) {
        const bool more = t0 + MF_TC < nt;
        if (more) fetch(t0 + MF_TC);
        __syncthreads();
#pragma unroll
        for (int tt0 = 0; tt0 < MF_TC; tt0 += 32) {
            if (t0 + tt0 >= nt) break;
            mm_v4i A[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint4 v = s_t[buf][(tt0 + n) * MF_ROW + 2 * s + h];
                A[s] = mm_v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
            }
            // C(row, :) = c of train tt0 + row; accumulator i is row 8 (i >> 2) + 4 h + (i & 3)
            mf_v16f C;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 c4 = *reinterpret_cast<const float4*>(&s_c[buf][tt0 + 8 * k + 4 * h]);
                C[4 * k] = c4.x;
                C[4 * k + 1] = c4.y;
                C[4 * k + 2] = c4.z;
                C[4 * k + 3] = c4.w;
            }
#pragma unroll
            for (int qt = 0; qt < QT; qt += 2) {
                mf_v16f a0 = mfma_fp4_32(A[0], B[qt][0], C);
                mf_v16f a1 = mfma_fp4_32(A[0], B[qt + 1][0], C);
#pragma unroll
                for (int s = 1; s < 4; ++s) {
                    a0 = mfma_fp4_32(A[s], B[qt][s], a0);
                    a1 = mfma_fp4_32(A[s], B[qt + 1][s], a1);
                }
                if constexpr (TOP2) {
                    top2_16_u32(best[qt], best2[qt], a0);
                    top2_16_u32(best[qt + 1], best2[qt + 1], a1);
                } else {
                    best[qt] = max16_u32(best[qt], a0);
                    best[qt + 1] = max16_u32(best[qt + 1], a1);
                }
            }
        }
        if (more) {
            store(buf ^ 1, t0 + MF_TC);  // the other buffer: last read before the barrier at the top of this chunk
            buf ^= 1;
        }
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        uint32_t v = best[qt];
        uint32_t v2 = 0u;
        if constexpr (TOP2) {
            // the other lane half's pair covers the other 16 rows of each train block: the second of the union is the
            // smaller head or one of the tails
            const uint32_t o1 = (uint32_t)__shfl_xor((int)v, 32, 64), o2 = (uint32_t)__shfl_xor((int)best2[qt], 32, 64);
            v2 = max(min(v, o1), max(best2[qt], o2));
            v = max(v, o1);
        } else {
            v = max(v, (uint32_t)__shfl_xor((int)v, 32, 64));  // the other lane half's 16 rows of each train block
        }
        // the query's popcount: its expanded fragments hold one set bit per descriptor bit, half in each lane half
        int pa = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) pa += __popc((uint32_t)B[qt][s][r]);
        pa += __shfl_xor(pa, 32, 64);
        const int q = q0 + 32 * QT * wave + 32 * qt + n;
        if (h == 0 && q < nq) {
            uint32_t key = 0xFFFFFFFFu;  // empty train set
            if (nt > 0) {
                const int iv = (int)__uint_as_float(v) - (1 << 21);
                const uint32_t d = (uint32_t)(pa - (iv >> 11));
                const uint32_t jj = 2047u - ((uint32_t)iv & 2047u);
                key = (d << 16) | jj;
            }
            match_key[(int64_t)pair * max_kp + q] = key;
            // 0 = no second train point (nt < 2): every real key' is >= 2^21 - 2^19
            if constexpr (TOP2) match_key2[(int64_t)pair * max_kp + q] = v2 != 0u ? fp4_decode_key(v2, pa) : 0xFFFFFFFFu;
        }
    }
}

namespace {
template <int QT, int WPE, bool TOP2>
void launch_fp4(const MatchLists& lists, const int32_t* pairs, int n_pairs, uint32_t* match_key, uint32_t* match_key2,
                hipStream_t s) {
    constexpr int QB = 4 * QT * 32;
    dim3 grid((lists.max_kp + QB - 1) / QB, n_pairs);
    hipLaunchKernelGGL((match_fp4_kernel<QT, WPE, TOP2>), grid, dim3(256), 0, s, lists.desc, lists.kp_count, pairs,
                       lists.max_kp, match_key, match_key2);
}
}  // namespace

void launch_match(const MatchLists& lists, const int32_t* pairs, int n_pairs, int max_train, uint32_t* match_key,
                  uint32_t* match_key2, hipStream_t s) {
    if (max_train > 2048) {
        dim3 grid((lists.max_kp + MM_QB - 1) / MM_QB, n_pairs);
        if (match_key2)
            hipLaunchKernelGGL(match_top2_kernel, grid, dim3(256), 0, s, lists.desc, lists.kp_count, pairs,
                               lists.max_kp, match_key, match_key2);
        else
            hipLaunchKernelGGL(match_kernel, grid, dim3(256), 0, s, lists.desc, lists.kp_count, pairs, lists.max_kp,
                               match_key);
        return;
    }
    // FP4, best key only: 4 query tiles of 32 per wave, 3 waves per SIMD (168 VGPRs; 2 tiles at 4 waves per SIMD: 1.60 ms
    // vs 1.43, profiles/r06/c14)
    if (!match_key2) launch_fp4<4, 3, false>(lists, pairs, n_pairs, match_key, nullptr, s);
    else launch_fp4<MF2_QT, MF2_WPE, true>(lists, pairs, n_pairs, match_key, match_key2, s);
}

}  // namespace yavo
