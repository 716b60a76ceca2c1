// yavo_bow.hip -- place recognition: the bag-of-binary-words keyframe index (include/yavo/yavo_bow.h), its four gfx950
// kernels and its C ABI.  Beyond the reference (its notes list ORB features as a to-do; this is what ORB systems put on
// top of them); the specification is tests/bow_reference.py and every result here equals it bit for bit.
//
//   bow_words_kernel    nearest vocabulary word of every descriptor of a list of slots (int8 MFMA, as match_kernel)
//   bow_vector_kernel   word histogram -> quantised tf-idf vector and its squared norm, one workgroup per image
//   bow_score_kernel    [Q][W_pad] . [E][W_pad]^T -> dots[Q][E] in int32 (int8 MFMA)
//   bow_topk_kernel     exclusion window, score and the first top_k by (score desc, entry asc), one wave per query
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "yavo_host.h"
#include "yavo_wave.h"
#include "yavo_xlane.h"

namespace yavo {

constexpr int kBowMaxWords = YV_BOW_MAX_WORDS;
constexpr int kBowTopK = YV_BOW_MAX_TOP_K;
constexpr int kBowRing = 4;  // pinned slot / frame id lists in flight (batch forms)

// ------------------------------------------------------------------------------------------------
// words: the matcher's int8 form with the vocabulary as the train list
// ------------------------------------------------------------------------------------------------
// match_kernel's arithmetic (yavo_match.hip: bit b -> 2 b - 1, dot = 256 - 2 Hamming, key = (dot << 16) | (0xFFFF - w),
// the row maximum is the first word at minimum distance), with two differences in where the operands come from: the
// queries are the descriptors of slot slots[blockIdx.y] wherever that slot lies in the batch (no pair list, no copy of
// the descriptors), and the train list is the vocabulary, the same 32 W bytes for every workgroup (128 KB at W = 4096:
// it stays in L2).  The few helper lines are copies: match_kernel and its object stay as they are.
typedef int bw_v4i __attribute__((ext_vector_type(4)));
constexpr int BW_QT = 8;                  // 16-row query tiles per wave
constexpr int BW_QB = 4 * BW_QT * 16;     // descriptors per workgroup (4 waves)
constexpr int BW_TC = 128;                // words per LDS chunk
constexpr int BW_ROW = 17;                // uint4 per expanded word (16 + 1 pad: conflict-free b128 reads)

// 4 descriptor bits -> 4 bytes of +1 (bit set) / -1 (bit clear), bit i in byte i
__device__ __forceinline__ uint32_t bw_expand_pm1(uint32_t nib) {
    const uint32_t spread = (nib * 0x00204081u) & 0x01010101u;
    return ~(spread * 0xFEu);
}

__device__ __forceinline__ uint4 bw_expand16_pm1(uint32_t bits) {
    return make_uint4(bw_expand_pm1(bits & 0xF), bw_expand_pm1((bits >> 4) & 0xF), bw_expand_pm1((bits >> 8) & 0xF),
                      bw_expand_pm1((bits >> 12) & 0xF));
}

// desc: [slot][src_stride]; kp_count[slot]; out_word / out_dist: [query][out_stride], query = blockIdx.y.  Every slot's
// count is clamped to both strides.  W >= 1.
__global__ __launch_bounds__(256) void bow_words_kernel(const Desc* __restrict__ desc,
                                                        const int32_t* __restrict__ kp_count,
                                                        const int32_t* __restrict__ slots, int src_stride,
                                                        const uint32_t* __restrict__ vocab, int W,
                                                        int32_t* __restrict__ out_word, int32_t* __restrict__ out_dist,
                                                        int out_stride) {
    __shared__ uint4 s_t[2][BW_TC * BW_ROW];
    const int qi = blockIdx.y;
    const int slot = slots[qi];
    const int nq = min(max(kp_count[slot], 0), min(out_stride, src_stride)), nt = W;
    const int q0 = blockIdx.x * BW_QB;
    if (q0 >= nq) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, g = lane >> 4;
    const Desc* qd = desc + (int64_t)slot * src_stride;
    const uint32_t* tw = vocab;

    // descriptor fragments: tile qt row (lane & 15) = descriptor q0 + 16 BW_QT wave + 16 qt + (lane & 15)
    bw_v4i A[BW_QT][4];
#pragma unroll
    for (int qt = 0; qt < BW_QT; ++qt) {
        const int q = q0 + 16 * BW_QT * wave + 16 * qt + col;
        const Desc d = qd[q < nq ? q : 0];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t hi_mask = 0u - (uint32_t)(g >> 1);  // blend, not an index: keeps d in registers
            const uint32_t w = d.w[2 * s] ^ ((d.w[2 * s] ^ d.w[2 * s + 1]) & hi_mask);
            const uint32_t bits = (w >> (16 * (g & 1))) & 0xFFFFu;
            const uint4 e = bw_expand16_pm1(bits);
            A[qt][s] = bw_v4i{(int)e.x, (int)e.y, (int)e.z, (int)e.w};
        }
    }
    int best[BW_QT][4];
#pragma unroll
    for (int qt = 0; qt < BW_QT; ++qt)
#pragma unroll
        for (int r = 0; r < 4; ++r) best[qt][r] = INT_MIN;

    // staging: thread -> (word tt = idx >> 4, 16-bit field u = idx & 15), kF fields per thread per chunk
    constexpr int kF = BW_TC * 16 / 256;
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
            s_t[buf][tt * BW_ROW + u] = bw_expand16_pm1(bits);
        }
    };
    fetch(0);
    store(0);
    int buf = 0;
    for (int t0 = 0; t0 < nt; t0 += BW_TC) {
        const bool more = t0 + BW_TC < nt;
        if (more) fetch(t0 + BW_TC);
        __syncthreads();
#pragma unroll
        for (int tt0 = 0; tt0 < BW_TC; tt0 += 32) {
            if (t0 + tt0 >= nt) break;
            bw_v4i Ba[4], Bb[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint4 va = s_t[buf][(tt0 + col) * BW_ROW + 4 * s + g];
                const uint4 vb = s_t[buf][(tt0 + 16 + col) * BW_ROW + 4 * s + g];
                Ba[s] = bw_v4i{(int)va.x, (int)va.y, (int)va.z, (int)va.w};
                Bb[s] = bw_v4i{(int)vb.x, (int)vb.y, (int)vb.z, (int)vb.w};
            }
            // a column past the vocabulary gets -2^30: below every real key, above INT_MIN
            const int ja = t0 + tt0 + col, jb = ja + 16;
            const int bias_a = ja < nt ? 0xFFFF - ja : -(1 << 30);
            const int bias_b = jb < nt ? 0xFFFF - jb : -(1 << 30);
#pragma unroll
            for (int qt = 0; qt < BW_QT; qt += 2) {
                bw_v4i a0 = {0, 0, 0, 0}, b0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[qt][s], Ba[s], a0, 0, 0, 0);
                    b0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[qt][s], Bb[s], b0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[qt + 1][s], Ba[s], a1, 0, 0, 0);
                    b1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[qt + 1][s], Bb[s], b1, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    best[qt][r] = max(best[qt][r], max((int)(((uint32_t)a0[r] << 16) + (uint32_t)bias_a),
                                                       (int)(((uint32_t)b0[r] << 16) + (uint32_t)bias_b)));
                    best[qt + 1][r] = max(best[qt + 1][r], max((int)(((uint32_t)a1[r] << 16) + (uint32_t)bias_a),
                                                               (int)(((uint32_t)b1[r] << 16) + (uint32_t)bias_b)));
                }
            }
        }
        if (more) {
            store(buf ^ 1);  // the other buffer: last read before the barrier at the top of this chunk
            buf ^= 1;
        }
    }
    // per descriptor row: max over the 16 lanes (word columns) of its lane group
#pragma unroll
    for (int qt = 0; qt < BW_QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int v = best[qt][r];
            const int q = q0 + 16 * BW_QT * wave + 16 * qt + 4 * g + r;
            v = max(v, xl::xor_row_i32<8>(v));
            v = max(v, xl::xor_row_i32<4>(v));
            v = max(v, xl::xor_row_i32<2>(v));
            v = max(v, xl::xor_row_i32<1>(v));
            if (col == r && q < nq) {  // W >= 1: the row maximum is a real key
                const int dot = v >> 16;
                out_dist[(int64_t)qi * out_stride + q] = (256 - dot) >> 1;
                out_word[(int64_t)qi * out_stride + q] = (int)(0xFFFFu - ((uint32_t)v & 0xFFFFu));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// vector: histogram, tf-idf, quantisation, norm
// ------------------------------------------------------------------------------------------------
// One workgroup per image.  The histogram is W int32 counters in LDS; integer LDS atomics commute, so the counts do
// not depend on the order.  t_w = c_w * idf_q8[w] < 2^28, the block maximum, v_w = floor(127 t_w / tmax) in 64 bits
// (127 t_w < 2^35), the row of w_pad bytes (pad bytes zero, written on every call) and the block sum of v_w^2.
constexpr int kBowVecNT = 256;

__global__ __launch_bounds__(kBowVecNT) void bow_vector_kernel(const int32_t* __restrict__ word, int word_stride,
                                                                const int32_t* __restrict__ kp_count,
                                                                const int32_t* __restrict__ slots, int n_words,
                                                                int w_pad, const uint16_t* __restrict__ idf,
                                                                int8_t* __restrict__ out_vec,
                                                                int32_t* __restrict__ out_norm2,
                                                                const int64_t* __restrict__ fids,
                                                                int64_t* __restrict__ out_fid) {
    __shared__ int s_h[kBowMaxWords];
    __shared__ int s_tmp[16];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(kp_count[slots[i]], 0), word_stride);
    for (int w = tid; w < w_pad; w += kBowVecNT) s_h[w] = 0;
    __syncthreads();
    for (int k = tid; k < n; k += kBowVecNT) {
        const int w = word[(int64_t)i * word_stride + k];
        if ((unsigned)w < (unsigned)n_words) atomicAdd(&s_h[w], 1);
    }
    __syncthreads();
    int m = 0;
    for (int w = tid; w < n_words; w += kBowVecNT) {
        const int t = s_h[w] * (idf ? (int)idf[w] : 256);
        s_h[w] = t;
        m = max(m, t);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
    if (lane == 0) s_tmp[wave] = m;
    __syncthreads();
    int tmax = s_tmp[0];
#pragma unroll
    for (int w = 1; w < kBowVecNT / 64; ++w) tmax = max(tmax, s_tmp[w]);
    __syncthreads();  // s_tmp is the scan's scratch next
    int sq = 0;
    uint32_t* row = reinterpret_cast<uint32_t*>(out_vec + (int64_t)i * w_pad);
    for (int d = tid; d < w_pad / 4; d += kBowVecNT) {
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int w = 4 * d + k;  // s_h[w] == 0 for n_words <= w < w_pad
            const int v = tmax > 0 ? (int)((127ull * (unsigned long long)(uint32_t)s_h[w]) / (uint32_t)tmax) : 0;
            packed |= (uint32_t)v << (8 * k);
            sq += v * v;
        }
        row[d] = packed;
    }
    int total = 0;
    (void)block_excl_scan<kBowVecNT>(sq, s_tmp, &total);
    if (tid == 0) {
        out_norm2[i] = total;
        if (out_fid) out_fid[i] = fids[i];
    }
}

// ------------------------------------------------------------------------------------------------
// score: the int8 GEMM
// ------------------------------------------------------------------------------------------------
// dots[q][e] = sum_w qv[q][w] ev[e][w], operand values 0..127, K = w_pad (a multiple of 64) in steps of
// v_mfma_i32_16x16x64_i8.  A workgroup owns 64 queries x 64 entries, a wave 32 x 32 of them as 2 x 2 MFMA tiles.  Lane
// (row = lane & 15, g = lane >> 4) of K-step s holds the 16 bytes at 64 s + 16 g of its row, for A and B alike (so the
// products pair equal w whatever the k order inside the instruction is); accumulator r is row 4 g + r, column lane & 15
// (as match_kernel reads it).  The fragments come straight from global memory as 16-B loads: the rows of the 64 x 64
// block are shared by its four waves through L1, and the whole query matrix stays in L2 across entry blocks.
typedef int bs_v4i __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void bow_score_kernel(const int8_t* __restrict__ qv, int Q,
                                                        const int8_t* __restrict__ ev, int E, int w_pad,
                                                        int32_t* __restrict__ dots, int64_t dots_stride) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.y * 64 + (wave >> 1) * 32, e0 = blockIdx.x * 64 + (wave & 1) * 32;
    if (q0 >= Q || e0 >= E) return;  // no barriers below: waves leave independently
    const uint4* ap[2];
    const uint4* bp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int q = min(q0 + 16 * t + col, Q - 1), e = min(e0 + 16 * t + col, E - 1);  // rows past the end: clamped
        ap[t] = reinterpret_cast<const uint4*>(qv + (int64_t)q * w_pad) + g;
        bp[t] = reinterpret_cast<const uint4*>(ev + (int64_t)e * w_pad) + g;
    }
    bs_v4i acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = bs_v4i{0, 0, 0, 0};
    const int steps = w_pad >> 6;
    for (int s = 0; s < steps; ++s) {
        bs_v4i A[2], B[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint4 va = ap[t][4 * s], vb = bp[t][4 * s];
            A[t] = bs_v4i{(int)va.x, (int)va.y, (int)va.z, (int)va.w};
            B[t] = bs_v4i{(int)vb.x, (int)vb.y, (int)vb.z, (int)vb.w};
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[a], B[b], acc[a][b], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + 16 * a + 4 * g + r, e = e0 + 16 * b + col;
                if (q < Q && e < E) dots[(int64_t)q * dots_stride + e] = acc[a][b][r];
            }
}

// ------------------------------------------------------------------------------------------------
// top-k: exclusion window, score, rank
// ------------------------------------------------------------------------------------------------
// One wave per query.  An entry takes part when |f - frame_id_e| >= exclude and dot > 0 (then both norms are
// positive).  Its score is a positive double, whose order is that of its bit pattern; rank k is the arg-max of
// (score, -entry) over the entries that come after rank k - 1 in that order, so top_k passes over the row find the list
// without storing a score.  All 16 candidate slots are written on every call.
__global__ __launch_bounds__(256) void bow_topk_kernel(const int32_t* __restrict__ dots, int64_t dots_stride, int Q,
                                                       int E, const int32_t* __restrict__ q_norm2,
                                                       const int64_t* __restrict__ q_fid,
                                                       const int32_t* __restrict__ e_norm2,
                                                       const int64_t* __restrict__ e_fid, int64_t exclude, int top_k,
                                                       int32_t* __restrict__ cand_entry,
                                                       double* __restrict__ cand_score,
                                                       int32_t* __restrict__ cand_dot,
                                                       int32_t* __restrict__ cand_count) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;  // no barriers below: waves leave independently
    const double nq2 = (double)q_norm2[q];
    const int64_t f = q_fid[q];
    const int32_t* row = dots + (int64_t)q * dots_stride;
    unsigned long long last_bits = ~0ull;
    int last_e = -1, count = 0;
    for (int k = 0; k < kBowTopK; ++k) {
        unsigned long long bb = 0ull;
        int be = INT_MAX, bd = 0;
        if (k < top_k && k == count) {  // wave-uniform
            for (int e = lane; e < E; e += 64) {
                const int dot = row[e];
                int64_t df = f - e_fid[e];
                if (df < 0) df = -df;
                if (dot <= 0 || df < exclude) continue;
                const double sc = (double)dot / sqrt(nq2 * (double)e_norm2[e]);
                const unsigned long long bits = (unsigned long long)__double_as_longlong(sc);
                const bool after = bits < last_bits || (bits == last_bits && e > last_e);
                if (after && bits > bb) {  // e increases within a lane: the first of equal scores stays
                    bb = bits;
                    be = e;
                    bd = dot;
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long ob = (unsigned long long)__shfl_xor((long long)bb, off, 64);
                const int oe = __shfl_xor(be, off, 64), od = __shfl_xor(bd, off, 64);
                if (ob > bb || (ob == bb && oe < be)) {
                    bb = ob;
                    be = oe;
                    bd = od;
                }
            }
            if (be != INT_MAX) {
                ++count;
                last_bits = bb;
                last_e = be;
            }
        }
        if (lane == 0) {
            const bool found = be != INT_MAX;
            cand_entry[(int64_t)q * kBowTopK + k] = found ? be : -1;
            cand_score[(int64_t)q * kBowTopK + k] = found ? __longlong_as_double((long long)bb) : 0.0;
            cand_dot[(int64_t)q * kBowTopK + k] = found ? bd : 0;
        }
    }
    if (lane == 0) cand_count[q] = count;
}

}  // namespace yavo

// ------------------------------------------------------------------------------------------------
// the object and the C ABI
// ------------------------------------------------------------------------------------------------
struct yv_bow {
    yv_ctx* ctx = nullptr;
    int n_words = 0, w_pad = 0, max_entries = 0, max_queries = 0, max_kp = 0;
    int n_entries = 0, n_queries = 0;
    yavo::HipOwned mem;  // every buffer and event below
    uint32_t* d_words = nullptr;   // [n_words][8]
    uint16_t* d_idf = nullptr;     // [n_words], nullptr: 256 everywhere
    int8_t* vectors = nullptr;     // [max_entries][w_pad]
    int32_t* norm2 = nullptr;      // [max_entries]
    int64_t* frame_id = nullptr;   // [max_entries]
    int32_t* q_word = nullptr;     // [max_queries][max_kp]
    int32_t* q_dist = nullptr;
    int8_t* q_vectors = nullptr;   // [max_queries][w_pad]
    int32_t* q_norm2 = nullptr;    // [max_queries]
    int32_t* dots = nullptr;       // [max_queries][max_entries]
    int32_t* cand_entry = nullptr; // [max_queries][16]
    double* cand_score = nullptr;
    int32_t* cand_dot = nullptr;
    int32_t* cand_count = nullptr; // [max_queries]
    int32_t* d_slots = nullptr;    // [max_queries] the call's slots
    int64_t* d_fids = nullptr;     // [max_queries] the call's frame ids
    // the host-pointer forms' one-slot keypoint list
    yv_keypoint* d_kp = nullptr;   // [max_kp]
    Desc* d_desc = nullptr;        // [max_kp]
    int32_t* d_cnt = nullptr;      // [1]
    // the batch forms' pinned lists: [slots int32 max_queries | frame ids int64 max_queries], reused round robin once
    // the copy that read them has finished
    uint8_t* h_ring[yavo::kBowRing] = {};
    hipEvent_t ev_ring[yavo::kBowRing] = {};
    bool ring_used[yavo::kBowRing] = {};
    int ring_next = 0;
    std::vector<int64_t> h_frame;  // host mirror of frame_id
    int stage_mask = 15;           // yv_debug_bow_stages: which of the four kernels a call launches
};

namespace {

using namespace yavo;

int no_object() { return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE; }

enum BowMode { kWordsOnly, kVectorOnly, kAdd, kQuery };

size_t ring_fid_off(const yv_bow* w) { return ((size_t)w->max_queries * sizeof(int32_t) + 7) & ~(size_t)7; }

// The stages of one call over n slots of a keypoint list set (desc [slot][src_stride], kp_count [slot]) on stream s.
// slots / fids: host, n each.  kAdd appends to the index (the caller has checked the capacity), kQuery fills the query
// arrays, the dot matrix and the candidate lists against the entries enqueued so far.
int bow_run(yv_bow* w, const Desc* desc, const int32_t* kp_count, int src_stride, const int32_t* slots,
            const int64_t* fids, int n, BowMode mode, int64_t exclude, int top_k, hipStream_t s) {
    if (mode == kQuery) w->n_queries = n;
    if (n == 0) return YV_OK;
    const int r = w->ring_next;
    w->ring_next = (r + 1) % kBowRing;
    if (w->ring_used[r]) YV_HIP(hipEventSynchronize(w->ev_ring[r]));
    int32_t* hs = reinterpret_cast<int32_t*>(w->h_ring[r]);
    int64_t* hf = reinterpret_cast<int64_t*>(w->h_ring[r] + ring_fid_off(w));
    for (int i = 0; i < n; ++i) {
        hs[i] = slots[i];
        hf[i] = fids ? fids[i] : 0;
    }
    YV_HIP(hipMemcpyAsync(w->d_slots, hs, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    YV_HIP(hipMemcpyAsync(w->d_fids, hf, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
    YV_HIP(hipEventRecord(w->ev_ring[r], s));
    w->ring_used[r] = true;

    const int span = std::min(src_stride, w->max_kp);
    if (w->stage_mask & 1)
        hipLaunchKernelGGL(bow_words_kernel, dim3((span + BW_QB - 1) / BW_QB, n), dim3(256), 0, s, desc, kp_count,
                           w->d_slots, src_stride, w->d_words, w->n_words, w->q_word, w->q_dist, w->max_kp);
    if (mode == kWordsOnly) return check_launch();
    const int E = w->n_entries;
    if (mode == kAdd) {
        hipLaunchKernelGGL(bow_vector_kernel, dim3(n), dim3(kBowVecNT), 0, s, w->q_word, w->max_kp, kp_count,
                           w->d_slots, w->n_words, w->w_pad, w->d_idf, w->vectors + (size_t)E * w->w_pad,
                           w->norm2 + E, w->d_fids, w->frame_id + E);
        if (check_launch() != YV_OK) return YV_ERR_HIP;
        w->h_frame.insert(w->h_frame.end(), fids, fids + n);
        w->n_entries = E + n;
        return YV_OK;
    }
    if (w->stage_mask & 2)
        hipLaunchKernelGGL(bow_vector_kernel, dim3(n), dim3(kBowVecNT), 0, s, w->q_word, w->max_kp, kp_count,
                           w->d_slots, w->n_words, w->w_pad, w->d_idf, w->q_vectors, w->q_norm2,
                           (const int64_t*)nullptr, (int64_t*)nullptr);
    if (mode == kVectorOnly) return check_launch();
    if (E > 0 && (w->stage_mask & 4))
        hipLaunchKernelGGL(bow_score_kernel, dim3((E + 63) / 64, (n + 63) / 64), dim3(256), 0, s, w->q_vectors, n,
                           w->vectors, E, w->w_pad, w->dots, (int64_t)w->max_entries);
    if (w->stage_mask & 8)
        hipLaunchKernelGGL(bow_topk_kernel, dim3((n + 3) / 4), dim3(256), 0, s, w->dots, (int64_t)w->max_entries, n, E,
                           w->q_norm2, w->d_fids, w->norm2, w->frame_id, exclude, top_k, w->cand_entry,
                           w->cand_score, w->cand_dot, w->cand_count);
    return check_launch();
}

// what the host-pointer forms check before the object
bool host_args_ok(const yv_keypoint* kp, int n) { return n >= 0 && (n == 0 || kp); }

// one host keypoint list into the object's own slot, then bow_run over it
int bow_run_host(yv_bow* w, const yv_keypoint* kp, int n, int64_t frame_id, BowMode mode, int64_t exclude, int top_k,
                 hipStream_t s) {
    yv_ctx* ctx = w->ctx;
    if (n > 0) YV_HIP(stage_h2d(ctx, w->d_kp, kp, sizeof(yv_keypoint) * (size_t)n, s));
    ctx->h_pinned[0] = n;
    YV_HIP(stage_h2d(ctx, w->d_cnt, ctx->h_pinned, sizeof(int32_t), s));
    launch_pack_desc(w->d_kp, w->d_cnt, 1, w->max_kp, w->d_desc, s);
    const int32_t slot0 = 0;
    return bow_run(w, w->d_desc, w->d_cnt, w->max_kp, &slot0, &frame_id, 1, mode, exclude, top_k, s);
}

int batch_args_check(const yv_bow* w, const yv_batch* b, const int32_t* slots, int n) {
    if (b->max_kp > w->max_kp) return YV_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= b->nslots) return YV_ERR_INVALID;
    if (n > w->max_queries) return YV_ERR_CAPACITY;
    return YV_OK;
}

}  // namespace

extern "C" {

int yv_bow_create(yv_ctx* ctx, int n_words, const uint8_t* words, const uint16_t* idf_q8, int max_entries,
                  int max_queries, int max_kp, yv_bow** out) {
    if (!words || !out || n_words < 1 || n_words > kBowMaxWords || max_entries < 1 || max_entries > 65536 ||
        max_queries < 1 || max_queries > 4097 || max_kp < 1 || max_kp > kMaxKp)
        return YV_ERR_INVALID;
    *out = nullptr;
    if (!ctx) return no_object();
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    yv_bow* w = new (std::nothrow) yv_bow;
    if (!w) return YV_ERR_HIP;
    w->ctx = ctx;
    w->n_words = n_words;
    w->w_pad = (n_words + 63) & ~63;
    w->max_entries = max_entries;
    w->max_queries = max_queries;
    w->max_kp = max_kp;
    const size_t nq = (size_t)max_queries, ne = (size_t)max_entries, nk = (size_t)max_kp, wp = (size_t)w->w_pad;
    yavo::HipOwned& m = w->mem;
    bool ok = m.alloc(&w->d_words, 8 * (size_t)n_words) == YV_OK && m.alloc(&w->vectors, ne * wp) == YV_OK &&
              m.alloc(&w->norm2, ne) == YV_OK && m.alloc(&w->frame_id, ne) == YV_OK &&
              m.alloc(&w->q_word, nq * nk) == YV_OK && m.alloc(&w->q_dist, nq * nk) == YV_OK &&
              m.alloc(&w->q_vectors, nq * wp) == YV_OK && m.alloc(&w->q_norm2, nq) == YV_OK &&
              m.alloc(&w->dots, nq * ne) == YV_OK && m.alloc(&w->cand_entry, nq * kBowTopK) == YV_OK &&
              m.alloc(&w->cand_score, nq * kBowTopK) == YV_OK && m.alloc(&w->cand_dot, nq * kBowTopK) == YV_OK &&
              m.alloc(&w->cand_count, nq) == YV_OK && m.alloc(&w->d_slots, nq) == YV_OK &&
              m.alloc(&w->d_fids, nq) == YV_OK && m.alloc(&w->d_kp, nk) == YV_OK && m.alloc(&w->d_desc, nk) == YV_OK &&
              m.alloc(&w->d_cnt, 1) == YV_OK;
    if (ok && idf_q8) ok = m.alloc(&w->d_idf, (size_t)n_words) == YV_OK;
    for (int r = 0; ok && r < kBowRing; ++r)
        ok = m.alloc_host(&w->h_ring[r], ring_fid_off(w) + nq * sizeof(int64_t)) == YV_OK &&
             m.event(&w->ev_ring[r]) == hipSuccess;
    hipStream_t s = ctx->stream;
    // the view's arrays are defined from the start: an empty index, no query
    ok = ok && hipMemsetAsync(w->vectors, 0, ne * wp, s) == hipSuccess &&
         hipMemsetAsync(w->q_vectors, 0, nq * wp, s) == hipSuccess &&
         hipMemsetAsync(w->cand_count, 0, nq * sizeof(int32_t), s) == hipSuccess;
    if (ok) {
        StageScope stage_scope(ctx);
        ok = stage_h2d(ctx, w->d_words, words, 32 * (size_t)n_words, s) == hipSuccess &&
             (!idf_q8 || stage_h2d(ctx, w->d_idf, idf_q8, sizeof(uint16_t) * (size_t)n_words, s) == hipSuccess) &&
             stage_sync(ctx, s) == hipSuccess;
    }
    if (!ok) {
        (void)hipDeviceSynchronize();
        delete w;
        return YV_ERR_HIP;
    }
    *out = w;
    return YV_OK;
}

void yv_bow_destroy(yv_bow* w) {
    if (!w) return;
    if (set_device(w->ctx) == YV_OK) (void)hipDeviceSynchronize();  // a batch form may run on a stream of the caller's
    delete w;
}

int yv_bow_reset(yv_bow* w) {
    if (!w) return no_object();
    w->n_entries = 0;
    w->h_frame.clear();
    return YV_OK;
}

int yv_bow_count(yv_bow* w, int* n_entries) {
    if (!n_entries) return YV_ERR_INVALID;
    if (!w) return no_object();
    *n_entries = w->n_entries;
    return YV_OK;
}

int yv_bow_words(yv_bow* w, const yv_keypoint* kp, int n, int32_t* word, int32_t* dist) {
    if (!host_args_ok(kp, n) || (n > 0 && (!word || !dist))) return YV_ERR_INVALID;
    if (!w) return no_object();
    if (n > w->max_kp) return YV_ERR_CAPACITY;
    if (n == 0) return YV_OK;
    yv_ctx* ctx = w->ctx;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    const int st = bow_run_host(w, kp, n, 0, kWordsOnly, 0, 1, s);
    if (st != YV_OK) return st;
    YV_HIP(stage_d2h(ctx, word, w->q_word, sizeof(int32_t) * (size_t)n, s));
    YV_HIP(stage_d2h(ctx, dist, w->q_dist, sizeof(int32_t) * (size_t)n, s));
    YV_HIP(stage_sync(ctx, s));
    return YV_OK;
}

int yv_bow_vector(yv_bow* w, const yv_keypoint* kp, int n, int8_t* vec, int32_t* norm2) {
    if (!host_args_ok(kp, n) || !vec || !norm2) return YV_ERR_INVALID;
    if (!w) return no_object();
    if (n > w->max_kp) return YV_ERR_CAPACITY;
    yv_ctx* ctx = w->ctx;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    const int st = bow_run_host(w, kp, n, 0, kVectorOnly, 0, 1, s);
    if (st != YV_OK) return st;
    YV_HIP(stage_d2h(ctx, vec, w->q_vectors, (size_t)w->n_words, s));
    YV_HIP(stage_d2h(ctx, norm2, w->q_norm2, sizeof(int32_t), s));
    YV_HIP(stage_sync(ctx, s));
    return YV_OK;
}

int yv_bow_add(yv_bow* w, const yv_keypoint* kp, int n, int64_t frame_id) {
    if (!host_args_ok(kp, n)) return YV_ERR_INVALID;
    if (!w) return no_object();
    if (n > w->max_kp || w->n_entries + 1 > w->max_entries) return YV_ERR_CAPACITY;
    yv_ctx* ctx = w->ctx;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    const int st = bow_run_host(w, kp, n, frame_id, kAdd, 0, 1, s);
    if (st != YV_OK) return st;
    YV_HIP(stage_sync(ctx, s));
    return YV_OK;
}

int yv_bow_query(yv_bow* w, const yv_keypoint* kp, int n, int64_t frame_id, int64_t exclude, int top_k, int32_t* entry,
                 int64_t* entry_frame, double* score, int32_t* dot, int* n_out) {
    if (!host_args_ok(kp, n) || !entry || !score || !n_out || top_k < 1 || top_k > kBowTopK || exclude < 0)
        return YV_ERR_INVALID;
    if (!w) return no_object();
    if (n > w->max_kp) return YV_ERR_CAPACITY;
    yv_ctx* ctx = w->ctx;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    const int st = bow_run_host(w, kp, n, frame_id, kQuery, exclude, top_k, s);
    if (st != YV_OK) return st;
    int32_t e[kBowTopK], d[kBowTopK], cnt = 0;
    double sc[kBowTopK];
    YV_HIP(stage_d2h(ctx, e, w->cand_entry, sizeof(e), s));
    YV_HIP(stage_d2h(ctx, sc, w->cand_score, sizeof(sc), s));
    YV_HIP(stage_d2h(ctx, d, w->cand_dot, sizeof(d), s));
    YV_HIP(stage_d2h(ctx, &cnt, w->cand_count, sizeof(cnt), s));
    YV_HIP(stage_sync(ctx, s));
    cnt = std::min(std::max(cnt, 0), top_k);
    for (int k = 0; k < cnt; ++k) {
        entry[k] = e[k];
        score[k] = sc[k];
        if (dot) dot[k] = d[k];
        if (entry_frame) entry_frame[k] = e[k] >= 0 && (size_t)e[k] < w->h_frame.size() ? w->h_frame[(size_t)e[k]] : -1;
    }
    *n_out = cnt;
    return YV_OK;
}

int yv_bow_add_batch(yv_bow* w, yv_batch* b, const int32_t* slots, const int64_t* frame_ids, int n, void* stream) {
    if (n < 0 || (n > 0 && (!slots || !frame_ids))) return YV_ERR_INVALID;
    if (!w || !b) return no_object();
    const int st = batch_args_check(w, b, slots, n);
    if (st != YV_OK) return st;
    if (w->n_entries + n > w->max_entries) return YV_ERR_CAPACITY;
    if (n == 0) return YV_OK;
    if (set_device(w->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w->ctx->stream;
    return bow_run(w, b->desc, b->kp_count, b->max_kp, slots, frame_ids, n, kAdd, 0, 1, s);
}

int yv_bow_query_batch(yv_bow* w, yv_batch* b, const int32_t* slots, const int64_t* frame_ids, int n, int64_t exclude,
                       int top_k, void* stream) {
    if (n < 0 || (n > 0 && (!slots || !frame_ids)) || top_k < 1 || top_k > kBowTopK || exclude < 0)
        return YV_ERR_INVALID;
    if (!w || !b) return no_object();
    const int st = batch_args_check(w, b, slots, n);
    if (st != YV_OK) return st;
    if (set_device(w->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w->ctx->stream;
    return bow_run(w, b->desc, b->kp_count, b->max_kp, slots, frame_ids, n, kQuery, exclude, top_k, s);
}

int yv_bow_view_get(yv_bow* w, yv_bow_view* v) {
    if (!v) return YV_ERR_INVALID;
    if (!w) return no_object();
    v->n_words = w->n_words;
    v->w_pad = w->w_pad;
    v->max_entries = w->max_entries;
    v->max_queries = w->max_queries;
    v->max_kp = w->max_kp;
    v->n_entries = w->n_entries;
    v->n_queries = w->n_queries;
    v->vectors = w->vectors;
    v->norm2 = w->norm2;
    v->frame_id = w->frame_id;
    v->q_word = w->q_word;
    v->q_dist = w->q_dist;
    v->q_vectors = w->q_vectors;
    v->q_norm2 = w->q_norm2;
    v->dots = w->dots;
    v->cand_entry = w->cand_entry;
    v->cand_score = w->cand_score;
    v->cand_dot = w->cand_dot;
    v->cand_count = w->cand_count;
    return YV_OK;
}

int yv_bow_candidates_copy(yv_bow* w, int n, int32_t* d_entry, double* d_score, int32_t* d_dot, int32_t* d_count,
                           void* stream) {
    if (n < 0) return YV_ERR_INVALID;
    if (!w) return no_object();
    if (n > w->max_queries) return YV_ERR_CAPACITY;
    if (n == 0) return YV_OK;
    if (set_device(w->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w->ctx->stream;
    const size_t rows = (size_t)n * kBowTopK;
    if (d_entry) YV_HIP(hipMemcpyAsync(d_entry, w->cand_entry, rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (d_score) YV_HIP(hipMemcpyAsync(d_score, w->cand_score, rows * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (d_dot) YV_HIP(hipMemcpyAsync(d_dot, w->cand_dot, rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (d_count) YV_HIP(hipMemcpyAsync(d_count, w->cand_count, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return YV_OK;
}

// Measurement entry points (tools/bench_bow.py; like yv_debug_xlane not part of the public headers).
// Which kernels the following query calls launch: bit 0 words, 1 vector, 2 score, 3 top-k (15: all, the default).  A
// call with a stage left out reads what the last full call left in that stage's output.
int yv_debug_bow_stages(yv_bow* w, int mask) {
    if (!w || mask < 0 || mask > 15) return YV_ERR_INVALID;
    w->stage_mask = mask;
    return YV_OK;
}

// launch_match alone on device buffers of the caller's: desc [slots][max_kp] (32 B each), kp_count [slots], pairs
// [n_pairs][2], match_key [n_pairs][max_kp] -- the word kernel's yardstick, a pair list whose train slot is the same
// for every pair.
int yv_debug_match_keys(yv_ctx* ctx, const void* d_desc, const int32_t* d_kp_count, int max_kp, const int32_t* d_pairs,
                        int n_pairs, int max_train, uint32_t* d_match_key, void* stream) {
    if (!ctx || !d_desc || !d_kp_count || !d_pairs || !d_match_key || max_kp < 1 || max_kp > kMaxKp || n_pairs < 1 ||
        n_pairs > 65535 || max_train < 0 || max_train > kMaxKp)
        return YV_ERR_INVALID;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
    const MatchLists lists{static_cast<const Desc*>(d_desc), nullptr, d_kp_count, max_kp};
    launch_match(lists, d_pairs, n_pairs, max_train, d_match_key, nullptr, s);
    return check_launch();
}

}  // extern "C"
