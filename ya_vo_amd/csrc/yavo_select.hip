// yavo_select.hip -- keypoint selection between the detect kernel and top-K (yv_set_keypoint_select, DESIGN.md
// section 17): non-maximum suppression among the FAST corners and per-cell quotas, exact on the 64-bit key the cut
// itself uses.
//
//   select_bucket_kernel   per image: the candidate keys counting-sorted by a grid of cells + the cells' starts
//   select_nms_kernel      per 32 x 64 tile: the corners no corner within the radius beats, appended to the output
//   select_quota_kernel    per corner: its rank among its cell's corners, appended when rank < per_cell
//
// A key is (~ord(response)) << 32 | row * W + col: smaller is better, keys of one image are distinct.  Every kernel
// writes a list in whatever order its atomics give; top-K's result does not depend on the order of its input.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "yavo_internal.h"
#include "yavo_wave.h"

namespace yavo {

namespace {

// ------------------------------------------------------------------------------------------------
// Buckets: one 1024-thread workgroup per image, a counting sort over the cells in LDS
// ------------------------------------------------------------------------------------------------
// Two passes over the image's keys (count, then scatter): the list has no bound a register array could hold, and a
// pass is one coalesced read.  The order inside a cell is whatever the LDS atomics gave.
constexpr int SB_NT = 1024;
constexpr int SB_PER = kSelMaxCells / SB_NT;  // cells per thread in the scan
static_assert(kSelMaxCells % SB_NT == 0, "whole cells per thread");

__device__ __forceinline__ int cell_of(uint64_t key, uint32_t W, uint32_t cell_rows, uint32_t cell_cols, int cells_x,
                                       int n_cells) {
    const uint32_t idx = (uint32_t)key;
    const uint32_t row = idx / W, col = idx - row * W;
    return min((int)(row / cell_rows) * cells_x + (int)(col / cell_cols), n_cells - 1);  // in range for row < H
}

// count[img] keys of src -> dst cell by cell, starts[img][0 .. n_cells] (the last entry is the list's length).
// seen != nullptr: src is the detect kernel's list, and the kernel does for it what topk_kernel does (seen = the
// corners before any filter, count = 0 for the next detection).  zero[img] = 0: the counter the kernel that follows
// appends under.
__global__ __launch_bounds__(SB_NT) void select_bucket_kernel(const uint64_t* __restrict__ src, int64_t cap,
                                                              uint32_t* __restrict__ count,
                                                              uint32_t* __restrict__ seen, uint32_t* __restrict__ zero,
                                                              int W, int cell_rows, int cell_cols, int cells_x,
                                                              int n_cells, uint64_t* __restrict__ dst,
                                                              int32_t* __restrict__ starts) {
    __shared__ int s_cell[kSelMaxCells];  // counts, then starts, then cursors
    __shared__ int s_wave[SB_NT / 64];
    const int img = blockIdx.x, tid = threadIdx.x;
    const uint64_t* in = src + (int64_t)img * cap;
    uint64_t* out = dst + (int64_t)img * cap;
    int32_t* st = starts + (int64_t)img * (kSelMaxCells + 1);
    int64_t n64 = (int64_t)count[img];
    if (n64 > cap) n64 = cap;
    const int n = (int)n64;
    for (int c = tid; c < n_cells; c += SB_NT) s_cell[c] = 0;
    __syncthreads();  // every thread has read count[img]
    if (tid == 0) {
        if (seen) {
            seen[img] = (uint32_t)n;
            count[img] = 0;
        }
        zero[img] = 0;
    }
    for (int i = tid; i < n; i += SB_NT)
        atomicAdd(&s_cell[cell_of(in[i], (uint32_t)W, (uint32_t)cell_rows, (uint32_t)cell_cols, cells_x, n_cells)], 1);
    __syncthreads();
    int local[SB_PER];
    const int base = cell_excl_scan<SB_NT, SB_PER>(s_cell, n_cells, s_wave, local);
#pragma unroll
    for (int k = 0; k < SB_PER; ++k) {
        const int c = tid * SB_PER + k;
        if (c < n_cells) {
            s_cell[c] = base + local[k];
            st[c] = base + local[k];
        }
    }
    if (tid == 0) st[n_cells] = n;
    __syncthreads();
    for (int i = tid; i < n; i += SB_NT) {
        const uint64_t k = in[i];
        const int p =
            atomicAdd(&s_cell[cell_of(k, (uint32_t)W, (uint32_t)cell_rows, (uint32_t)cell_cols, cells_x, n_cells)], 1);
        out[p] = k;  // p < n <= cap: the cursors of all cells together advance n times
    }
}

// keep ? key : nothing appended to out under *counter: ballot + prefix count, one atomic per wave.  Called by whole
// waves.
__device__ __forceinline__ void wave_append(bool keep, uint64_t key, uint64_t* __restrict__ out,
                                            uint32_t* __restrict__ counter, int lane) {
    const uint64_t mask = __ballot(keep);
    if (mask == 0) return;  // the same in every lane
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (keep) out[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = key;  // < the input's length <= cap
}

// ------------------------------------------------------------------------------------------------
// Suppression: one wave per tile
// ------------------------------------------------------------------------------------------------
// The wave writes the upper key half (~ord(response): smaller is better, kNone = no corner) of every corner of its
// tile and of the r-pixel ring around it into a dense LDS map -- the corners of the 3 x 3 tiles around its own, three
// contiguous pieces of the bucketed list -- and each corner of the tile then walks its (2r + 1)^2 window.  The
// row-major position breaks ties between equal responses, and inside a window that is the walk's own order: a
// neighbour before the centre wins on <=, one after it on <.  A corner whose upper half is kNone itself (response
// bits 0xFFFFFFFF; a host list can hold it) is told from an empty pixel by one bit per pixel in s_has.
// The map is the launch's dynamic LDS, (32 + 2r) x (64 + 2r) words + the bits: 9.0 KB at r = 1, 15.5 KB at r = 8.  The
// kernel is a chain of dependent global reads per tile (starts, keys, the append's atomic), so what it needs is tiles
// in flight per CU, and the map's size is what limits them.
constexpr int SN_NT = 64;
constexpr int SN_LOADS = 4;  // keys per lane in flight while the map is filled
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kSelTileRows >= kSelMaxRadius && kSelTileCols >= kSelMaxRadius, "the ring lies in the adjacent tiles");
__host__ __device__ constexpr int nms_map_words(int r) { return (kSelTileRows + 2 * r) * (kSelTileCols + 2 * r); }
__host__ __device__ constexpr int nms_lds_words(int r) { return nms_map_words(r) + (nms_map_words(r) + 31) / 32; }

__global__ __launch_bounds__(SN_NT) void select_nms_kernel(const uint64_t* __restrict__ sorted, int64_t cap,
                                                           const int32_t* __restrict__ starts, int W, int tiles_x,
                                                           int tiles_y, int r, uint64_t* __restrict__ dst,
                                                           uint32_t* __restrict__ dst_count) {
    extern __shared__ uint32_t s_nms[];  // nms_lds_words(r)
    const int img = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x;  // images on x: no 65535 limit
    const int32_t* st = starts + (int64_t)img * (kSelMaxCells + 1);
    const uint64_t* in = sorted + (int64_t)img * cap;
    uint64_t* out = dst + (int64_t)img * cap;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int r0 = ty * kSelTileRows - r, c0 = tx * kSelTileCols - r;  // the map's first row and column
    const int mh = kSelTileRows + 2 * r, mw = kSelTileCols + 2 * r;
    const int n_map = mh * mw;
    uint32_t* s_map = s_nms;
    uint32_t* s_has = s_nms + n_map;
    const uint32_t Wu = (uint32_t)W;
    // tiles tx - 1 .. tx + 1 of a tile row follow each other in the list: three pieces, their bounds read together
    // with the tile's own (eight independent loads in flight, before the map is cleared)
    const int own_lo = st[tile], own_hi = st[tile + 1];
    int lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int y = ty - 1 + d;
        const bool ok = y >= 0 && y < tiles_y;
        const int yy = ok ? y : ty;
        lo[d] = st[yy * tiles_x + max(tx - 1, 0)];
        hi[d] = ok ? st[yy * tiles_x + min(tx + 1, tiles_x - 1) + 1] : lo[d];  // no such tile row: an empty piece
    }
    if (own_lo >= own_hi) return;  // the whole workgroup: an empty tile
    for (int i = lane; i < n_map; i += SN_NT) s_map[i] = kNone;
    for (int i = lane; i < (n_map + 31) / 32; i += SN_NT) s_has[i] = 0;
    __syncthreads();
    // the three pieces as one index space, SN_LOADS keys per lane in flight: the usual tile (a few hundred corners in
    // its 3 x 3 neighbourhood) is one round trip to memory, not one per 64 keys and piece
    const int n0 = hi[0] - lo[0], n01 = n0 + hi[1] - lo[1], total = n01 + hi[2] - lo[2];  // total >= own_hi - own_lo > 0
    for (int b = 0; b < total; b += SN_LOADS * SN_NT) {
        uint64_t k[SN_LOADS];
#pragma unroll
        for (int u = 0; u < SN_LOADS; ++u) {
            const int j = min(b + u * SN_NT + lane, total - 1);  // past the end: the last key again, not placed
            k[u] = in[j < n0 ? lo[0] + j : (j < n01 ? lo[1] + (j - n0) : lo[2] + (j - n01))];
        }
#pragma unroll
        for (int u = 0; u < SN_LOADS; ++u) {
            const uint32_t idx = (uint32_t)k[u], kh = (uint32_t)(k[u] >> 32);
            const uint32_t row = idx / Wu, col = idx - row * Wu;
            const int mr = (int)row - r0, mc = (int)col - c0;
            if (b + u * SN_NT + lane < total && (uint32_t)mr < (uint32_t)mh && (uint32_t)mc < (uint32_t)mw) {
                const int m = mr * mw + mc;  // < n_map; positions are distinct: one writer per entry
                s_map[m] = kh;
                if (kh == kNone) atomicOr(&s_has[m >> 5], 1u << (m & 31));
            }
        }
    }
    __syncthreads();
    for (int b = own_lo; b < own_hi; b += SN_NT) {  // the same trips in every lane
        const int i = b + lane;
        bool keep = false;
        uint64_t k = 0;
        if (i < own_hi) {
            k = in[i];
            const uint32_t idx = (uint32_t)k, kh = (uint32_t)(k >> 32);
            const uint32_t row = idx / Wu, col = idx - row * Wu;
            const int mr = (int)row - r0, mc = (int)col - c0;
            keep = true;
            // a corner of this tile has r <= mr < r + kSelTileRows and r <= mc < r + kSelTileCols: its window lies
            // inside the map (anything else is no corner of an H x W image and passes unexamined)
            const bool inside = mr >= r && mr < r + kSelTileRows && mc >= r && mc < r + kSelTileCols;
            for (int dr = -r; inside && keep && dr <= r; ++dr) {
                const int m0 = (mr + dr) * mw + mc;
                for (int dc = -r; dc <= r; ++dc) {
                    const uint32_t v = s_map[m0 + dc];
                    const bool before = dr < 0 || (dr == 0 && dc < 0);
                    if (v < kh) keep = false;
                    else if (v == kh && before && (kh != kNone || ((s_has[(m0 + dc) >> 5] >> ((m0 + dc) & 31)) & 1u)))
                        keep = false;
                }
            }
        }
        wave_append(keep, k, out, dst_count + img, lane);
    }
}

// ------------------------------------------------------------------------------------------------
// Quota: one thread per corner of the cell-bucketed list
// ------------------------------------------------------------------------------------------------
// A corner's rank is the number of corners of its cell with a smaller key; it stays iff rank < q.  A cell holding no
// more than q corners is not ranked.  A cell of m > q corners costs m reads per corner, from L2.
constexpr int SQ_NT = 256;

__global__ __launch_bounds__(SQ_NT) void select_quota_kernel(const uint64_t* __restrict__ sorted, int64_t cap,
                                                             const int32_t* __restrict__ starts, int W, int cell_rows,
                                                             int cell_cols, int cells_x, int n_cells, int q,
                                                             uint64_t* __restrict__ dst,
                                                             uint32_t* __restrict__ dst_count) {
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int32_t* st = starts + (int64_t)img * (kSelMaxCells + 1);
    const int n = st[n_cells];
    const uint64_t* in = sorted + (int64_t)img * cap;
    uint64_t* out = dst + (int64_t)img * cap;
    for (int b = (int)blockIdx.y * SQ_NT; b < n; b += (int)gridDim.y * SQ_NT) {  // the same trips in every lane
        const int i = b + tid;
        bool keep = false;
        uint64_t k = 0;
        if (i < n) {
            k = in[i];
            const int c = cell_of(k, (uint32_t)W, (uint32_t)cell_rows, (uint32_t)cell_cols, cells_x, n_cells);
            const int lo = st[c], hi = st[c + 1];
            int rank = 0;
            if (hi - lo > q)
                for (int j = lo; j < hi && rank < q; ++j) rank += in[j] < k ? 1 : 0;
            keep = rank < q;
        }
        wave_append(keep, k, out, dst_count + img, lane);
    }
}

}  // namespace

static_assert(((kBandRows * kMaxBands + kSelTileRows - 1) / kSelTileRows) *
                      ((kMaxWidth + kSelTileCols - 1) / kSelTileCols) <= kSelMaxCells,
              "the tiles of every accepted H x W fit the LDS counter table");

uint32_t* launch_select(uint64_t* cand_keys, int64_t cap, uint32_t* cand_count, uint32_t* cand_seen, int n_images,
                        int H, int W, int nms_radius, int cell_rows, int cell_cols, int per_cell, uint64_t* scratch,
                        int32_t* starts, uint32_t* counts, hipStream_t s) {
    uint32_t* cnt_nms = counts;
    uint32_t* cnt_quota = counts + n_images;
    uint32_t* src_count = cand_count;
    uint32_t* seen = cand_seen;  // the first bucket pass consumes the detect kernel's list
    if (nms_radius > 0) {
        const int tiles_x = (W + kSelTileCols - 1) / kSelTileCols, tiles_y = (H + kSelTileRows - 1) / kSelTileRows;
        const int n_tiles = tiles_x * tiles_y;
        hipLaunchKernelGGL(select_bucket_kernel, dim3(n_images), dim3(SB_NT), 0, s, cand_keys, cap, src_count, seen,
                           cnt_nms, W, kSelTileRows, kSelTileCols, tiles_x, n_tiles, scratch, starts);
        hipLaunchKernelGGL(select_nms_kernel, dim3(n_images, n_tiles), dim3(SN_NT),
                           sizeof(uint32_t) * (size_t)nms_lds_words(nms_radius), s, scratch, cap, starts, W,
                           tiles_x, tiles_y, nms_radius, cand_keys, cnt_nms);
        src_count = cnt_nms;
        seen = nullptr;
    }
    if (per_cell > 0) {
        const int cells_x = (W + cell_cols - 1) / cell_cols, cells_y = (H + cell_rows - 1) / cell_rows;
        const int n_cells = cells_x * cells_y;  // <= kSelMaxCells: checked by the caller
        hipLaunchKernelGGL(select_bucket_kernel, dim3(n_images), dim3(SB_NT), 0, s, cand_keys, cap, src_count, seen,
                           cnt_quota, W, cell_rows, cell_cols, cells_x, n_cells, scratch, starts);
        // blocks per image: the list's length is not known here; a few images get enough blocks for a long list
        const int64_t full = (cap + SQ_NT - 1) / SQ_NT;
        const int blocks = (int)std::min<int64_t>(full, n_images >= 64 ? 8 : 256);
        hipLaunchKernelGGL(select_quota_kernel, dim3(n_images, blocks), dim3(SQ_NT), 0, s, scratch, cap, starts, W,
                           cell_rows, cell_cols, cells_x, n_cells, per_cell, cand_keys, cnt_quota);
        src_count = cnt_quota;
    }
    return src_count;
}

}  // namespace yavo
