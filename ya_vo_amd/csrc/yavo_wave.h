// yavo_wave.h -- the wave and workgroup prefix sums of the front end (detect, top-K, finalize, the two counting
// sorts, PNG inflate).  Only these: block_excl_scan_geom (yavo_geom_dev.h) and the wave_min / wave_max / wave_sum of
// yavo_match_gate.hip and yavo_steer.hip are other algorithms, and moving a kernel onto another one is a speed change.
#pragma once

#include <hip/hip_runtime.h>

namespace yavo {

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// Inclusive scan across one 64-lane wave, all in DPP (no LDS permutes): Hillis-Steele inside each 16-lane row
// (row_shr 1, 2, 4, 8; lanes without a source add the `old` 0), then row_bcast:15 adds row 0's total to row 1 and
// row 2's to row 3, and row_bcast:31 adds rows 0-1's total to rows 2 and 3 (GFX9 DPP).
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

// Exclusive scan over the whole block (blockDim.x = NT, multiple of 64, <= 1024).  s_tmp >= 16 ints.
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* s_tmp, int* total) {
    const int lane = lane_id();
    const int wave = (int)threadIdx.x >> 6;
    constexpr int NW = NT / 64;
    int incl = wave_incl_scan(v);
    if (lane == 63) s_tmp[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        int w = lane < NW ? s_tmp[lane] : 0;
        int wi = wave_incl_scan(w);
        if (lane < NW) s_tmp[lane] = wi - w;  // exclusive wave offsets
        if (lane == NW - 1) s_tmp[NW] = wi;
    }
    __syncthreads();
    int res = s_tmp[wave] + incl - v;
    if (total) *total = s_tmp[NW];
    __syncthreads();
    return res;
}

// The counting sorts' exclusive scan over the n_cells <= NT * PER counters s_cell (blockDim.x = NT): PER consecutive
// cells per thread, then the threads' sums, the waves' totals through s_wave (NT / 64 ints).  Cell threadIdx.x * PER + k
// starts at the returned base + local[k].  The barrier comes after every read of s_cell, so the caller may put the
// starts over the counts at once.
template <int NT, int PER>
__device__ __forceinline__ int cell_excl_scan(const int* s_cell, int n_cells, int* s_wave, int (&local)[PER]) {
    static_assert(NT % 64 == 0, "whole waves");
    const int tid = threadIdx.x;
    int sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = tid * PER + k;
        local[k] = sum;
        sum += c < n_cells ? s_cell[c] : 0;
    }
    int incl = sum;
    const int lane = tid & 63, wave = tid >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();  // every count is read, every wave total written
    int base = incl - sum;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    return base;
}

}  // namespace yavo
