// yavo_match_gate.hip -- the gated matcher (yv_match_gated / yv_batch_set_match_gates).
//
//   gate_sort_kernel      per slot: the keypoints bucketed by (32-row band, column cell) + the band starts
//   match_gated_kernel    per pair: the best (and second best) train point inside every query's gate
//
// A gate is {drow_lo, drow_hi, dcol_lo, dcol_hi} on train minus query position; the keys written are the ungated
// matcher's, (distance << 16) | train index with 0xFFFFFFFF for "no train point", so match_finalize_kernel and
// everything behind it run unchanged.  No matrix core: a query has tens of candidates, popcounts on the VALU.
#include <hip/hip_runtime.h>

#include "yavo_internal.h"
#include "yavo_wave.h"

namespace yavo {

namespace {

// ------------------------------------------------------------------------------------------------
// Buckets: one 1024-thread workgroup per slot, a counting sort over (band, column cell) in LDS
// ------------------------------------------------------------------------------------------------
// cell = band * col_cells + min(column >> col_shift, col_cells - 1) with band = min(row / kGateBandRows, n_bands - 1):
// consecutive entries of the sorted list are close in the image (one band, neighbouring column cells), and the
// entries of a row range are one contiguous piece of it.  The order inside a cell is whatever the LDS atomics gave:
// the matcher's result does not depend on it, because the key carries the index.
constexpr int GS_NT = 1024;
constexpr int GS_PER = kGateMaxCells / GS_NT;  // cells per thread in the scan
static_assert(kMaxKp <= 4 * GS_NT, "four keypoints per thread");

__global__ __launch_bounds__(GS_NT) void gate_sort_kernel(const yv_keypoint* __restrict__ keypoints,
                                                          const int32_t* __restrict__ kp_count, int max_kp, int n_bands,
                                                          int col_cells, int col_shift, uint2* __restrict__ sorted,
                                                          int32_t* __restrict__ band_start) {
    __shared__ int s_cell[kGateMaxCells];  // counts, then starts
    __shared__ int s_wave[GS_NT / 64];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int n = min(kp_count[slot], min(max_kp, kMaxKp));
    const int n_cells = n_bands * col_cells;  // <= kGateMaxCells
    int32_t* bs = band_start + (int64_t)slot * (n_bands + 1);
    if (n <= 0) {
        for (int b = tid; b <= n_bands; b += GS_NT) bs[b] = 0;
        return;
    }
    for (int c = tid; c < n_cells; c += GS_NT) s_cell[c] = 0;
    __syncthreads();
    const yv_keypoint* kp = keypoints + (int64_t)slot * max_kp;
    int cell[4], rank[4];
    uint32_t pos[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid + u * GS_NT;
        cell[u] = -1;
        if (i < n) {
            const uint32_t r = (uint32_t)kp[i].x & 0xFFFFu, c = (uint32_t)kp[i].y & 0xFFFFu;
            pos[u] = r | (c << 16);
            cell[u] = min((int)(r / kGateBandRows), n_bands - 1) * col_cells + min((int)(c >> col_shift), col_cells - 1);
            rank[u] = atomicAdd(&s_cell[cell[u]], 1);
        }
    }
    __syncthreads();
    int local[GS_PER];
    const int base = cell_excl_scan<GS_NT, GS_PER>(s_cell, n_cells, s_wave, local);
#pragma unroll
    for (int k = 0; k < GS_PER; ++k) {
        const int c = tid * GS_PER + k;
        if (c < n_cells) s_cell[c] = base + local[k];
    }
    __syncthreads();
    uint2* out = sorted + (int64_t)slot * max_kp;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (cell[u] >= 0) out[s_cell[cell[u]] + rank[u]] = make_uint2(pos[u], (uint32_t)(tid + u * GS_NT));  // < n
    for (int b = tid; b < n_bands; b += GS_NT) bs[b] = s_cell[b * col_cells];
    if (tid == 0) bs[n_bands] = n;
}

// ------------------------------------------------------------------------------------------------
// Gated matcher
// ------------------------------------------------------------------------------------------------
// A wave takes GM_Q consecutive queries of the query slot's sorted list, GM_L lanes per query, and works alone (no
// workgroup barrier).  It scans the train slot's entries of the bands its queries' gates can reach, 256 per trip
// (four loads in flight per lane), and appends those inside the bounding box of the wave's gates (ballot + prefix
// count) to its LDS list.  When the list cannot take another trip, or the scan ends, it is consumed in chunks of 64:
// lane e fetches the descriptor of entry e into LDS (the next chunk's fetch is in flight during the walk), then the
// GM_L lanes of a query walk the chunk, each taking every GM_L-th entry, test the query's own gate and keep a running
// minimum (pair of minima) of the key.  The list and the chunk have fixed sizes, so a band holding thousands of
// keypoints only means more chunks.
constexpr int GM_NT = 256;             // 4 waves
// lanes per query: 8 measured 1.27 ms per 2048-frame step, 16 (4 queries per wave) 1.75 ms; with 4 the 1-NN
// instantiation needs 160 VGPRs
constexpr int GM_L = 8;
static_assert(GM_L >= 1 && 64 % GM_L == 0 && GM_L <= 32, "a power of two");
constexpr int GM_Q = 64 / GM_L;        // queries per wave
constexpr int GM_TRIP = 256;           // entries scanned per trip
constexpr int GM_CHUNK = 64;           // descriptors staged per chunk: one per lane
constexpr int GM_LIST = GM_CHUNK + GM_TRIP;  // the list is consumed once it holds more than GM_CHUNK entries

__device__ __forceinline__ int wave_min(int v) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
// LDS written by some lanes of the wave is read by others
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool TOP2>
__global__ __launch_bounds__(GM_NT) __attribute__((amdgpu_waves_per_eu(6, 8))) void match_gated_kernel(
    const Desc* __restrict__ desc, const int32_t* __restrict__ kp_count, const int32_t* __restrict__ pairs, int max_kp,
    int n_bands, const uint2* __restrict__ sorted, const int32_t* __restrict__ band_start,
    const int4* __restrict__ gates, int mirror, uint32_t* __restrict__ match_key, uint32_t* __restrict__ match_key2) {
    __shared__ uint4 s_lo[GM_NT / 64][GM_CHUNK];
    __shared__ uint4 s_hi[GM_NT / 64][GM_CHUNK];
    __shared__ uint2 s_list[GM_NT / 64][GM_LIST];  // {row | column << 16, train index}
    const int pair = blockIdx.y;
    const int qi = pairs[2 * pair], ti = pairs[2 * pair + 1];
    const int nq = min(kp_count[qi], max_kp), nt = min(kp_count[ti], max_kp);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int base = ((int)blockIdx.x * (GM_NT / 64) + wave) * GM_Q;
    if (base >= nq) return;  // the whole wave: waves never meet at a barrier
    int4 g = gates[pair];
    if (mirror) g = make_int4(-g.y, -g.x, -g.w, -g.z);  // query minus train: the swapped pair's gate
    const int sub = lane % GM_L;
    const int qp = base + lane / GM_L;
    const bool active = qp < nq;
    const int64_t qoff = (int64_t)qi * max_kp, toff = (int64_t)ti * max_kp;
    const uint2 qe = sorted[qoff + min(qp, nq - 1)];  // past the list: the last query again, not stored
    const int i = (int)qe.y;
    const int qr = (int)(qe.x & 0xFFFFu), qc = (int)(qe.x >> 16);
    const uint4* dq = reinterpret_cast<const uint4*>(desc + qoff + i);
    const uint4 qa = dq[0], qb = dq[1];
    // this lane's gate as two unsigned range tests
    const int rbase = qr + g.x, cbase = qc + g.z;
    const uint32_t rspan = (uint32_t)(g.y - g.x), cspan = (uint32_t)(g.w - g.z);
    // the box every gate of the wave lies in
    const int r0 = wave_min(qr) + g.x, r1 = wave_max(qr) + g.y;
    const int c0 = wave_min(qc) + g.z, c1 = wave_max(qc) + g.w;
    uint32_t m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
    int p_lo = 0, p_hi = 0;
    const int max_row = n_bands * kGateBandRows - 1;
    if (nt > 0 && r1 >= 0 && r0 <= max_row) {
        const int32_t* bs = band_start + (int64_t)ti * (n_bands + 1);
        p_lo = bs[max(r0, 0) / kGateBandRows];
        p_hi = min(bs[min(r1, max_row) / kGateBandRows + 1], nt);
    }
    uint4* lo = s_lo[wave];
    uint4* hi = s_hi[wave];
    uint2* list = s_list[wave];
    const uint2* tsorted = sorted + toff;
    const Desc* tdesc = desc + toff;
    int cnt = 0;
    for (int p0 = p_lo; p0 < p_hi; p0 += GM_TRIP) {
        uint2 te[GM_TRIP / 64];
#pragma unroll
        for (int u = 0; u < GM_TRIP / 64; ++u) te[u] = tsorted[min(p0 + u * 64 + lane, p_hi - 1)];
#pragma unroll
        for (int u = 0; u < GM_TRIP / 64; ++u) {
            const int tr = (int)(te[u].x & 0xFFFFu), tc = (int)(te[u].x >> 16);
            const bool in = p0 + u * 64 + lane < p_hi && tr >= r0 && tr <= r1 && tc >= c0 && tc <= c1;
            const uint64_t mask = __ballot(in);
            if (in) list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = te[u];  // < cnt + 64 <= GM_LIST
            cnt += __popcll(mask);
        }
        cnt = __builtin_amdgcn_readfirstlane(cnt);  // the same in every lane: scalar loop control below
        if (cnt <= GM_CHUNK && p0 + GM_TRIP < p_hi) continue;  // room for another trip
        wave_sync_lds();
        // chunk c's descriptors travel through registers: fetched while chunk c - 1 is walked
        uint4 fa = make_uint4(0, 0, 0, 0), fb = fa;
        if (lane < cnt) {
            const uint4* dt = reinterpret_cast<const uint4*>(tdesc + list[lane].y);
            fa = dt[0];
            fb = dt[1];
        }
        for (int cb = 0; cb < cnt; cb += GM_CHUNK) {
            lo[lane] = fa;
            hi[lane] = fb;
            wave_sync_lds();
            if (cb + GM_CHUNK + lane < cnt) {
                const uint4* dt = reinterpret_cast<const uint4*>(tdesc + list[cb + GM_CHUNK + lane].y);
                fa = dt[0];
                fb = dt[1];
            }
            const int m = min(cnt - cb, GM_CHUNK);
            // branch-free steps, two in flight: entry e < GM_CHUNK always (k is a multiple of GM_L), and one past
            // the chunk's m entries is stale LDS that never passes
#pragma unroll 2
            for (int k = 0; k < m; k += GM_L) {
                const int e = k + sub;
                const uint4 a = lo[e], b = hi[e];
                const uint2 mt = list[cb + e];
                const int tr = (int)(mt.x & 0xFFFFu), tc = (int)(mt.x >> 16);
                const bool pass = (e < m) & ((uint32_t)(tr - rbase) <= rspan) & ((uint32_t)(tc - cbase) <= cspan);
                const int d = __popc(qa.x ^ a.x) + __popc(qa.y ^ a.y) + __popc(qa.z ^ a.z) + __popc(qa.w ^ a.w) +
                              __popc(qb.x ^ b.x) + __popc(qb.y ^ b.y) + __popc(qb.z ^ b.z) + __popc(qb.w ^ b.w);
                const uint32_t key = pass ? ((uint32_t)d << 16) | mt.y : 0xFFFFFFFFu;
                if constexpr (TOP2) m2 = min(m2, max(m1, key));  // the keys of a query's candidates are distinct
                m1 = min(m1, key);
            }
            wave_sync_lds();  // the walk's reads before the next chunk's (and the next trip's) writes
        }
        cnt = 0;
    }
    // the GM_L lanes of a query hold disjoint candidate sets
#pragma unroll
    for (int off = 1; off < GM_L; off <<= 1) {
        const uint32_t o1 = (uint32_t)__shfl_xor((int)m1, off, 64);
        if constexpr (TOP2) {
            const uint32_t o2 = (uint32_t)__shfl_xor((int)m2, off, 64);
            m2 = min(max(m1, o1), min(m2, o2));
        }
        m1 = min(m1, o1);
    }
    if (active && sub == 0) {
        match_key[(int64_t)pair * max_kp + i] = m1;
        if constexpr (TOP2) match_key2[(int64_t)pair * max_kp + i] = m2;
    }
}

}  // namespace

void launch_gate_sort(const yv_keypoint* keypoints, const int32_t* kp_count, int n_slots, int max_kp, int n_bands,
                      int col_cells, int col_shift, uint2* sorted, int32_t* band_start, hipStream_t s) {
    hipLaunchKernelGGL(gate_sort_kernel, dim3(n_slots), dim3(GS_NT), 0, s, keypoints, kp_count, max_kp, n_bands,
                       col_cells, col_shift, sorted, band_start);
}

void launch_match_gated(const MatchLists& lists, const int32_t* pairs, int n_pairs, int n_bands, const uint2* sorted,
                        const int32_t* band_start, const int32_t* gates, bool mirror, uint32_t* match_key,
                        uint32_t* match_key2, hipStream_t s) {
    constexpr int per_block = (GM_NT / 64) * GM_Q;
    dim3 grid((lists.max_kp + per_block - 1) / per_block, n_pairs);
    const int4* g = reinterpret_cast<const int4*>(gates);
    const auto kernel = match_key2 ? match_gated_kernel<true> : match_gated_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(GM_NT), 0, s, lists.desc, lists.kp_count, pairs, lists.max_kp, n_bands,
                       sorted, band_start, g, mirror ? 1 : 0, match_key, match_key2);
}

}  // namespace yavo
