// yavo_topk.hip -- per image: the best max_kp corners in the reference's order, and the checkBoundry compaction that
// hands them to BRIEF band by band.
//
// Reference functions restated (the reference's file:line):
//   topk_kernel         std::sort + top-2000 cut                src/FastDetector.cc:343-368
//                       Brief::checkBoundry                     src/BriefDescriptor.cc:128-136
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yavo_internal.h"
#include "yavo_wave.h"

namespace yavo {

// ------------------------------------------------------------------------------------------------
// top-K selection + sort + checkBoundry compaction (one 1024-thread workgroup per image)
// ------------------------------------------------------------------------------------------------
constexpr int TK_NT = 1024;

// checkBoundry(kp.y=col, kp.x=row, W, H): 8 <= col <= W-8 and 8 <= row <= H-8.
__device__ __forceinline__ bool brief_boundary(int row, int col, int H, int W) {
    return !(col - 8 < 0 || col + 8 > W) && !(row - 8 < 0 || row + 8 > H);
}

// Compacts points 0..K-1 (rc_at(i) -> int2 {row, col}) to those inside checkBoundry, keeping order;
// kp_src[slot] = {row, col, id = input index, 0}.  Chunks of 4 * NT points, 4 consecutive per thread.  The kept
// points are also bucketed by BRIEF band (row / kBandRows): kp_band = {row, col, id, slot} grouped by band,
// band_off[b] = the first entry of band b, band_off[nb] = the count (nb = bands of H rows).  Inside a band the points
// are grouped by the LDS bank of their patch centre in brief_kernel's band layout (bank_classes(nb) classes), which
// deals each 32-lane group of its descriptor waves keypoints of distinct banks (any order inside a class).  A second
// pass recomputes the same flags and slots and places each point after its (band, class) counter.
__host__ __device__ constexpr int bank_classes(int nb) { return nb <= kBandCounters / 32 ? 32 : 1; }

template <int NT, class RcAt>
__device__ void boundary_compact(RcAt rc_at, int K, int H, int W, int32_t* kp_src, int32_t* kp_count,
                                 int32_t* kp_band, int32_t* band_off, int* s_tmp, int* s_band) {
    const int tid = threadIdx.x;
    const int nb = (H + kBandRows - 1) / kBandRows;
    const int C = bank_classes(nb), nbc = nb * C;
    const int LS = brief_lds_stride(W);
    // (band, class) of a point: the dword bank of its centre byte (row - r0 + 8) * LS + col in the band's LDS copy
    auto bucket = [&](int row, int col) -> int {
        const int band = row / kBandRows;
        const int cls = C == 1 ? 0 : ((((row - band * kBandRows + 8) * LS + col) >> 2) & 31);
        return band * C + cls;
    };
    for (int b = tid; b < nbc; b += NT) s_band[b] = 0;
    __syncthreads();
    int base = 0;
    for (int pass = 0; pass < 2; ++pass) {
        base = 0;
        for (int c0 = 0; c0 < K; c0 += 4 * NT) {
            int flags[4];
            int2 rcs[4];
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = c0 + tid * 4 + u;
                flags[u] = 0;
                rcs[u] = make_int2(0, 0);
                if (i < K) {
                    rcs[u] = rc_at(i);
                    flags[u] = brief_boundary(rcs[u].x, rcs[u].y, H, W) ? 1 : 0;
                }
                cnt += flags[u];
            }
            int total = 0;
            int off = base + block_excl_scan<NT>(cnt, s_tmp, &total);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = c0 + tid * 4 + u;
                if (flags[u]) {
                    const int bk = bucket(rcs[u].x, rcs[u].y);
                    if (pass == 0) {
                        reinterpret_cast<int4*>(kp_src)[off] = make_int4(rcs[u].x, rcs[u].y, i, 0);
                        atomicAdd(&s_band[bk], 1);
                    } else {
                        const int pos = atomicAdd(&s_band[bk], 1);
                        reinterpret_cast<int4*>(kp_band)[pos] = make_int4(rcs[u].x, rcs[u].y, i, off);
                    }
                    off++;
                }
            }
            base += total;
        }
        __syncthreads();
        if (pass == 0) {
            // (band, class) counts -> first entries (the second pass's cursors) and the band offsets table
            int acc = 0;
            for (int b0 = 0; b0 < nbc; b0 += NT) {
                const int j = b0 + tid;
                const int c = j < nbc ? s_band[j] : 0;
                int tot = 0;
                const int first = acc + block_excl_scan<NT>(c, s_tmp, &tot);
                if (j < nbc) {
                    s_band[j] = first;
                    if (j % C == 0) band_off[j / C] = first;
                }
                acc += tot;
            }
            if (tid == 0) band_off[nb] = acc;
        }
        __syncthreads();
    }
    if (tid == 0) *kp_count = base;
}

// top-K per image: one workgroup of NT threads per image.  512 threads: same-box A/B in the headline step (r03 c32,
// two runs each) 1024 -> 206.0k fps, 512 -> 209.7k, 256 -> 207.3k; in-step top-K 757 -> 488 us per dispatch (half
// the waves at each of its ~80 workgroup barriers, twice the per-thread work in the sort stages).
constexpr int TK_SEL_NT = 512;
static_assert(TK_SEL_NT >= 256 && TK_SEL_NT % 64 == 0, "the radix-select histogram scan uses the first 256 threads");
template <int NT>
__global__ __launch_bounds__(NT) void topk_kernel(const uint64_t* __restrict__ cand_keys, int64_t cap,
                                                     uint32_t* __restrict__ cand_count, uint32_t* __restrict__ cand_seen,
                                                     int H, int W, int max_kp, int keep, int32_t* __restrict__ det_rc,
                                                     float* __restrict__ det_resp, int32_t* __restrict__ det_count,
                                                     int32_t* __restrict__ kp_src, int32_t* __restrict__ kp_count,
                                                     int32_t* __restrict__ kp_band, int32_t* __restrict__ band_off,
                                                     int32_t* __restrict__ brief_heads) {
    __shared__ uint64_t s_keys[kMaxKp];
    __shared__ uint32_t s_hist[256];
    __shared__ int s_tmp[40];
    __shared__ int s_band[kBandCounters];
    __shared__ uint64_t s_prefix, s_mask;
    __shared__ int s_krem, s_done, s_n;

    const int img = blockIdx.x;
    const int tid = threadIdx.x;
    // the band queue of the brief_kernel that follows on this stream starts empty
    if (img == 0 && tid < kBriefHeads) brief_heads[tid] = 0;
    const uint64_t* keys = cand_keys + (int64_t)img * cap;
    int64_t C64 = (int64_t)cand_count[img];
    if (C64 > cap) C64 = cap;
    const int C = (int)C64;
    const int K = C < keep ? C : keep;
    __syncthreads();
    if (tid == 0) {
        cand_seen[img] = (uint32_t)C;  // corners before the cut, kept for the caller
        cand_count[img] = 0;           // consumed: ready for the next detection into this slot
    }
    int32_t* rc_out = det_rc + (int64_t)img * max_kp * 2;
    float* resp_out = det_resp + (int64_t)img * max_kp;

    if (K == 0) {  // no corners (or max_kp == 0): nothing to select
        const int nb = (H + kBandRows - 1) / kBandRows;
        for (int b = tid; b <= nb; b += NT) band_off[(int64_t)img * (kMaxBands + 1) + b] = 0;
        if (tid == 0) { det_count[img] = 0; kp_count[img] = 0; }
        return;
    }
    uint64_t sel_mask = 0, sel_prefix = ~0ull;  // selection: (key & sel_mask) <= sel_prefix
    if (C > K) {
        if (tid == 0) { s_prefix = 0; s_mask = 0; s_krem = K; s_done = 0; }
        __syncthreads();
        for (int shift = 56; shift >= 0; shift -= 8) {
            // state of the previous pass is read before the barrier that precedes any rewrite of it
            const uint64_t pm = s_mask, pp = s_prefix;
            const int krem = s_krem;
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < C; i += NT) {
                const uint64_t k = keys[i];
                if ((k & pm) == pp) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            // find the bucket holding the krem-th smallest key (256-entry scan by the first 4 waves)
            int h = 0, incl = 0;
            if (tid < 256) {
                h = (int)s_hist[tid];
                incl = wave_incl_scan(h);
                if ((tid & 63) == 63) s_tmp[tid >> 6] = incl;
            }
            __syncthreads();
            if (tid < 256) {
                int base = 0;
                for (int w = 0; w < (tid >> 6); ++w) base += s_tmp[w];
                incl += base;
                if (incl >= krem && incl - h < krem) {
                    const int nk = krem - (incl - h);
                    s_prefix = pp | ((uint64_t)tid << shift);
                    s_mask = pm | (0xFFull << shift);
                    s_krem = nk;
                    s_done = (h == nk);
                }
            }
            __syncthreads();
            if (s_done) break;
        }
        sel_mask = s_mask;
        sel_prefix = s_prefix;
    }
    // collect the K selected keys into LDS (any order), pad to a power of two, bitonic sort
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < C; i += NT) {
        const uint64_t k = keys[i];
        if ((k & sel_mask) <= sel_prefix) {
            const int p = atomicAdd(&s_n, 1);
            if (p < kMaxKp) s_keys[p] = k;
        }
    }
    __syncthreads();
    int P2 = 1;
    while (P2 < K) P2 <<= 1;
    for (int i = K + tid; i < P2; i += NT) s_keys[i] = ~0ull;
    __syncthreads();
    for (int size = 2; size <= P2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P2 >> 1); t += NT) {
                const int i = 2 * t - (t & (stride - 1));
                const int j = i + stride;
                const bool up = ((i & size) == 0);
                const uint64_t a = s_keys[i], b = s_keys[j];
                if ((a > b) == up) { s_keys[i] = b; s_keys[j] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < K; i += NT) {
        const uint64_t k = s_keys[i];
        const uint32_t idx = (uint32_t)k;
        const int row = (int)(idx / (uint32_t)W), col = (int)(idx - (uint32_t)row * (uint32_t)W);
        rc_out[2 * i] = row;
        rc_out[2 * i + 1] = col;
        resp_out[i] = key_resp(k);
    }
    if (tid == 0) det_count[img] = K;
    const uint32_t Wu = (uint32_t)W;
    auto rc_from_lds = [&](int i) -> int2 {
        const uint32_t idx = (uint32_t)s_keys[i];
        const uint32_t row = idx / Wu;
        return make_int2((int)row, (int)(idx - row * Wu));
    };
    boundary_compact<NT>(rc_from_lds, K, H, W, kp_src + (int64_t)img * max_kp * 4, kp_count + img,
                         kp_band + (int64_t)img * max_kp * 4, band_off + (int64_t)img * (kMaxBands + 1), s_tmp, s_band);
}

__global__ __launch_bounds__(TK_NT) void kp_boundary_kernel(const int32_t* __restrict__ det_rc,
                                                            const int32_t* __restrict__ det_count, int H, int W,
                                                            int max_kp, int32_t* __restrict__ kp_src,
                                                            int32_t* __restrict__ kp_count, int32_t* __restrict__ kp_band,
                                                            int32_t* __restrict__ band_off,
                                                            int32_t* __restrict__ brief_heads) {
    __shared__ int s_tmp[40];
    __shared__ int s_band[kBandCounters];
    const int img = blockIdx.x;
    if (img == 0 && threadIdx.x < kBriefHeads) brief_heads[threadIdx.x] = 0;  // as topk_kernel does
    int K = det_count[img];
    if (K > max_kp) K = max_kp;
    const int32_t* rc = det_rc + (int64_t)img * max_kp * 2;
    auto rc_from_global = [&](int i) -> int2 { return make_int2(rc[2 * i], rc[2 * i + 1]); };
    boundary_compact<TK_NT>(rc_from_global, K, H, W, kp_src + (int64_t)img * max_kp * 4, kp_count + img,
                            kp_band + (int64_t)img * max_kp * 4, band_off + (int64_t)img * (kMaxBands + 1), s_tmp,
                            s_band);
}

void launch_topk(const uint64_t* cand_keys, int64_t cap, uint32_t* cand_count, uint32_t* cand_seen, int n_images,
                 int H, int W, int max_kp, int keep, int32_t* det_rc, float* det_resp, int32_t* det_count, int32_t* kp_src,
                 int32_t* kp_count, int32_t* kp_band, int32_t* band_off, int32_t* brief_heads, hipStream_t s) {
    hipLaunchKernelGGL(topk_kernel<TK_SEL_NT>, dim3(n_images), dim3(TK_SEL_NT), 0, s, cand_keys, cap, cand_count,
                       cand_seen, H, W, max_kp, keep, det_rc, det_resp, det_count, kp_src, kp_count, kp_band, band_off,
                       brief_heads);
}

void launch_kp_boundary(const int32_t* det_rc, const int32_t* det_count, int n_images, int H, int W, int max_kp,
                        int32_t* kp_src, int32_t* kp_count, int32_t* kp_band, int32_t* band_off, int32_t* brief_heads,
                        hipStream_t s) {
    hipLaunchKernelGGL(kp_boundary_kernel, dim3(n_images), dim3(TK_NT), 0, s, det_rc, det_count, H, W, max_kp,
                       kp_src, kp_count, kp_band, band_off, brief_heads);
}

}  // namespace yavo
