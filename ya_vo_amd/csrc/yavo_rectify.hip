// yavo_rectify.hip -- lens undistortion and rectification (yv_rectify_*): the map of a camera
// model in 1/32 pixel (rectify_model_kernel, float64 in the specification's order) or a caller's map, and the integer
// bilinear remap of a batch of images through it with a constant zero border.  The map is shared by every image of
// its camera, so the remap kernels read it once and reuse it over a group of images.
//
// A destination image is cut into 16 x 256 tiles.  rectify_prepare_kernel writes the map in the form the remap
// kernels read and, per tile, the bounding box of the source taps of its pixels.  A tile whose box fits the LDS
// budget is remapped by rectify_tile_kernel, which stages the box per image with aligned dword loads and gathers the
// taps from LDS; every other tile by rectify_direct_kernel, which gathers them from global memory.
//
// No read leaves the source: a tap is read only after its row and column were tested to lie inside [0, Hs) x [0, Ws)
// (direct), or comes out of the staged box, which holds in-source taps only and is filled by rect_dword: a dword load
// is issued only after its four bytes were tested to lie inside [image, image + (Hs - 1) * stride + Ws), a dword that
// fails the test is assembled from the box's own bytes.  No write leaves the destination rows: every store, a byte or
// an aligned dword (store_row), covers pixels (x, y) with x < W and y < H only.
#include "yavo_host.h"

#include "../../include/yavo/yavo_io.h"

namespace yavo {
namespace rect {

constexpr int kTileW = 256, kTileH = 16;   // destination tile: 64 lanes x 4 pixels wide, 4 waves x 4 rows high
constexpr int kNT = 256;
constexpr int kRows = kTileH / (kNT / 64);  // rows of a tile per wave
constexpr int kGroup = 8;                   // images per workgroup: the map is read once per group
constexpr int kLdsBytes = 16384;            // a staged box; the tile kernel's registers allow 4 workgroups per CU
constexpr int kMaxBoxRows = 64;             // the fill takes one wave pass per box row, however narrow the box is
constexpr int kOutside = INT32_MIN;

// One destination tile of one map: the bounding box of the taps of its live pixels (bw = bh = 0: none).  A live pixel
// has a tap in the source, so its taps lie in [-1, Ws] x [-1, Hs]: the box holds in-source positions and, where the
// tile reaches the edge of the source, the line of zero taps next to it.
struct Tile {
    int32_t x0, y0, bw, bh, fits, pad[3];
};

// bytes between two rows of a staged box: its width plus the up to 3 bytes before its first column in the row's
// first aligned dword, in whole dwords
__host__ __device__ constexpr int box_pitch(int bw) { return ((bw + 6) >> 2) * 4; }

struct Model {
    double fx, cx, fy, cy, d[8], M[9];
};

__global__ __launch_bounds__(kNT) void rectify_model_kernel(Model m, int H, int W, int32_t* __restrict__ map) {
    const int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const double u = (double)(int)(i % W), v = (double)(int)(i / W);
    const double k1 = m.d[0], k2 = m.d[1], p1 = m.d[2], p2 = m.d[3], k3 = m.d[4], k4 = m.d[5], k5 = m.d[6],
                 k6 = m.d[7];
    const double X = (m.M[0] * u + m.M[1] * v) + m.M[2];
    const double Y = (m.M[3] * u + m.M[4] * v) + m.M[5];
    const double Wd = (m.M[6] * u + m.M[7] * v) + m.M[8];
    const double x = X / Wd, y = Y / Wd;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
    const double kr = ((((k3 * r2 + k2) * r2 + k1) * r2) + 1.0) / ((((k6 * r2 + k5) * r2 + k4) * r2) + 1.0);
    const double xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
    const double mu = m.fx * xd + m.cx, mv = m.fy * yd + m.cy;
    // NaN fails both comparisons
    const bool ok = mu > -65536.0 && mu < 65536.0 && mv > -65536.0 && mv < 65536.0;
    map[2 * i] = ok ? (int32_t)rint(mu * 32.0) : kOutside;
    map[2 * i + 1] = ok ? (int32_t)rint(mv * 32.0) : kOutside;
}

// the pixels of thread t in tile (tx, ty): columns x0 + k, k < 4, of the rows y0 + 4 j, j < kRows
__device__ __forceinline__ int px_x0(int tx) { return tx * kTileW + 4 * (threadIdx.x & 63); }
__device__ __forceinline__ int px_y0(int ty) { return ty * kTileH + (threadIdx.x >> 6); }

// One workgroup per tile: pack = the map with (OUTSIDE, OUTSIDE) for the entries that are OUTSIDE in either component
// or have all four taps outside the source; the tile's record.
__global__ __launch_bounds__(kNT) void rectify_prepare_kernel(const int32_t* __restrict__ map, int Hs, int Ws, int H,
                                                              int W, int tiles_x, int2* __restrict__ pack,
                                                              Tile* __restrict__ tiles) {
    __shared__ int box[4];  // min col, min row, max col, max row
    if (threadIdx.x == 0) {
        box[0] = box[1] = INT32_MAX;
        box[2] = box[3] = INT32_MIN;
    }
    __syncthreads();
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int xb = px_x0(tx), yb = px_y0(ty);
    int lo_c = INT32_MAX, lo_r = INT32_MAX, hi_c = INT32_MIN, hi_r = INT32_MIN;
    for (int j = 0; j < kRows; ++j) {
        const int y = yb + 4 * j;
        for (int k = 0; k < 4; ++k) {
            const int x = xb + k;
            if (x >= W || y >= H) continue;
            const int64_t i = (int64_t)y * W + x;
            int qu = map[2 * i], qv = map[2 * i + 1];
            bool keep = qu != kOutside && qv != kOutside;
            if (keep) {
                const int ix = qu >> 5, iy = qv >> 5;
                // the in-source columns of {ix, ix + 1} and rows of {iy, iy + 1}
                const int c0 = ix < 0 ? ix + 1 : ix, c1 = ix + 1 >= Ws ? ix : ix + 1;
                const int r0 = iy < 0 ? iy + 1 : iy, r1 = iy + 1 >= Hs ? iy : iy + 1;
                keep = c0 >= 0 && c0 < Ws && c1 >= c0 && r0 >= 0 && r0 < Hs && r1 >= r0;
                if (keep) {
                    lo_c = min(lo_c, ix);
                    hi_c = max(hi_c, ix + 1);
                    lo_r = min(lo_r, iy);
                    hi_r = max(hi_r, iy + 1);
                }
            }
            pack[i] = keep ? make_int2(qu, qv) : make_int2(kOutside, kOutside);
        }
    }
    if (hi_c != INT32_MIN) {
        atomicMin(&box[0], lo_c);
        atomicMin(&box[1], lo_r);
        atomicMax(&box[2], hi_c);
        atomicMax(&box[3], hi_r);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Tile t{};
        if (box[2] != INT32_MIN) {
            t.x0 = box[0];
            t.y0 = box[1];
            t.bw = box[2] - box[0] + 1;
            t.bh = box[3] - box[1] + 1;
        }
        t.fits = t.bh <= kMaxBoxRows && (int64_t)box_pitch(t.bw) * t.bh <= kLdsBytes;
        tiles[blockIdx.x] = t;
    }
}

struct Run {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_pitch, dst_pitch;
    int src_stride, dst_stride, Hs, Ws, H, W;
    int map, n_maps, n_img, group;  // the map's images are map + k n_maps, k < n_img; `group` of them per workgroup
    int tiles_x;
    const int2* pack;     // the map's
    const Tile* tiles;    // the map's
    const int32_t* list;  // the tiles of this launch (nullptr: every tile)
};

// ((32 - ay) * t + ay * b + 512) >> 10 with t = (32 - ax) * p00 + ax * p01 and b the same on the lower row, written
// as 32 p + a (q - p): the same integers with a multiplication less per line
__device__ __forceinline__ uint32_t blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t ax,
                                          uint32_t ay) {
    const int t = (int)(p00 << 5) + (int)ax * ((int)p01 - (int)p00);
    const int b = (int)(p10 << 5) + (int)ax * ((int)p11 - (int)p10);
    return (uint32_t)((t << 5) + (int)ay * (b - t) + 512) >> 10;
}

// The image loops keep a pixel's two map words in registers and derive the rest per image: without this the compiler
// hoists every derived address and every inside test out of the loop (64 wave masks, 160 VGPRs).
__device__ __forceinline__ void keep_in_loop(int& a, int& b) { asm volatile("" : "+v"(a), "+v"(b)); }

// Row y of a tile, by the whole wave: lane l holds the pixels x .. x + 3 (x = the tile's first column + 4 l) as the
// bytes of v, p is the address of pixel x, the pixels below W exist.  Whatever p's alignment (the same for every lane),
// the row goes out as aligned dwords: with p & 3 = sh != 0 a lane stores the dword at p + 4 - sh, its last sh pixels
// and the next lane's first 4 - sh; what no whole dword covers (the tile's first and last bytes, the row's tail) as
// bytes.
__device__ __forceinline__ void store_row(uint8_t* p, int x, int W, uint32_t v) {
    const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(p) & 3u;
    if (sh == 0) {
        if (x + 3 < W) {
            *reinterpret_cast<uint32_t*>(p) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < W) p[k] = (uint8_t)(v >> (8 * k));
        }
        return;
    }
    const int lane = threadIdx.x & 63, lead = 4 - (int)sh;
    const uint32_t next = (uint32_t)__shfl_down((int)v, 1);
    const uint32_t d = __builtin_amdgcn_alignbyte(next, v, (uint32_t)lead);  // the pixels x + lead .. x + lead + 3
    const bool own = lane < 63 && x + lead + 3 < W;  // this lane's dword
    const bool prev = lane > 0 && x + lead - 1 < W;  // the previous lane's, which holds this lane's first pixels
    if (own) *reinterpret_cast<uint32_t*>(p + lead) = d;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (x + k < W && (k < lead ? !prev : !own)) p[k] = (uint8_t)(v >> (8 * k));
}

// The complete path: the taps straight from global memory, each behind its inside test.
__global__ __launch_bounds__(kNT) void rectify_direct_kernel(Run a) {
    const int tile = a.list ? a.list[blockIdx.x] : (int)blockIdx.x;
    const int xb = px_x0(tile % a.tiles_x), yb = px_y0(tile / a.tiles_x);
    int2 e[kRows][4];
#pragma unroll
    for (int j = 0; j < kRows; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = xb + k, y = yb + 4 * j;
            e[j][k] = x < a.W && y < a.H ? a.pack[(int64_t)y * a.W + x] : make_int2(kOutside, kOutside);
        }
    const int first = blockIdx.y * a.group, last = min(a.n_img, first + a.group);
    for (int n = first; n < last; ++n) {
        const int64_t img = (int64_t)a.map + (int64_t)n * a.n_maps;
        const uint8_t* __restrict__ src = a.src + img * a.src_pitch;
        uint8_t* __restrict__ dst = a.dst + img * a.dst_pitch;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int y = yb + 4 * j;
            if (y >= a.H) continue;
            uint32_t out = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int qu = e[j][k].x, qv = e[j][k].y;
                keep_in_loop(qu, qv);
                if (qu == kOutside) continue;
                const int ix = qu >> 5, iy = qv >> 5;
                const bool c0 = (unsigned)ix < (unsigned)a.Ws, c1 = (unsigned)(ix + 1) < (unsigned)a.Ws;
                const bool r0 = (unsigned)iy < (unsigned)a.Hs, r1 = (unsigned)(iy + 1) < (unsigned)a.Hs;
                const uint8_t* p = src + (int64_t)iy * a.src_stride + ix;  // formed, not read
                uint32_t p00, p01, p10, p11;
                if (c0 && c1 && r0 && r1) {  // nearly every pixel of a camera's map
                    p00 = p[0];
                    p01 = p[1];
                    p10 = p[a.src_stride];
                    p11 = p[a.src_stride + 1];
                } else {
                    p00 = r0 && c0 ? p[0] : 0u;
                    p01 = r0 && c1 ? p[1] : 0u;
                    p10 = r1 && c0 ? p[a.src_stride] : 0u;
                    p11 = r1 && c1 ? p[a.src_stride + 1] : 0u;
                }
                out |= blend(p00, p01, p10, p11, (uint32_t)(qu & 31), (uint32_t)(qv & 31)) << (8 * k);
            }
            store_row(dst + (int64_t)y * a.dst_stride + xb, xb, a.W, out);
        }
    }
}

// The dword at address p (4-byte aligned) for the box row [lo, hi): zero when it holds none of the row's bytes; one
// aligned load when all four bytes are inside [img, img_end); byte loads of the row's bytes otherwise.  (The discipline
// of subpix_dword, yavo_stereo_subpix.hip.)
__device__ __forceinline__ uint32_t rect_dword(uintptr_t p, uintptr_t lo, uintptr_t hi, uintptr_t img,
                                               uintptr_t img_end) {
    if (p + 4 <= lo || p >= hi) return 0u;
    if (p >= img && p + 4 <= img_end) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uintptr_t q = p + b;
        if (q >= lo && q < hi) v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(q)) << (8 * b);
    }
    return v;
}

// mask of the bytes of the dword at p that lie inside [lo, hi)
__device__ __forceinline__ uint32_t keep_mask(uintptr_t p, uintptr_t lo, uintptr_t hi) {
    const intptr_t below = (intptr_t)(lo - p), above = (intptr_t)(p + 4 - hi);
    const int nlo = (int)min((intptr_t)4, max((intptr_t)0, below));
    const int nhi = (int)min((intptr_t)4, max((intptr_t)0, above));
    return (nlo >= 4 ? 0u : 0xFFFFFFFFu << (8 * nlo)) & (nhi >= 4 ? 0u : 0xFFFFFFFFu >> (8 * nhi));
}

constexpr int kFillRows = 8;  // box rows of a wave whose loads are in flight together
constexpr int kFillDw = 128;  // dwords of a box row the batched fill covers: two per lane (v[][2] below)

// Row j of a tile's box in one image.  The addresses are formed and not read: row -1 and column -1 lie before the
// image.
struct BoxRow {
    uintptr_t al;   // the aligned dword that holds the row's first byte
    uintptr_t lo, hi;  // the row's in-source bytes
    int ndw;        // dwords from al that hold the row: <= pitch / 4
    bool in_row;    // a source row (not the zero row above or below the source)
    bool whole;     // and every one of its dwords lies inside the image
};
__device__ __forceinline__ BoxRow box_row(const Tile& t, int j, uintptr_t base, uintptr_t img_end, int stride, int Hs,
                                          int cx0, int cx1) {
    const int r = t.y0 + j;
    const uintptr_t row = base + (uintptr_t)((int64_t)r * stride), beg = row + (uintptr_t)(intptr_t)t.x0;
    BoxRow b;
    b.al = beg & ~(uintptr_t)3;
    b.lo = row + (uintptr_t)cx0;
    b.hi = row + (uintptr_t)cx1;
    b.ndw = (int)((beg & 3) + (uintptr_t)t.bw + 3) >> 2;
    b.in_row = (unsigned)r < (unsigned)Hs;
    b.whole = b.in_row && b.al >= base && b.al + 4 * (uintptr_t)b.ndw <= img_end;
    return b;
}

// The hot path, for the tiles whose box fits: per image the box goes to LDS, zeros where it lies outside the source,
// and the four taps of a pixel come out of it with no test.  Box row j is stored at lds + j * pitch from the aligned
// dword that holds its first byte, so the byte of column c sits at sh + c - x0 with sh = the address of the row's first
// byte & 3: one value for the whole image when the source stride is a multiple of 4 (kRowShift = false), else
// (a0 + row * stride) & 3.  A lane's 4 pixels and its neighbours' lie about 4 bytes apart.
template <bool kRowShift>
__global__ __launch_bounds__(kNT) void rectify_tile_kernel(Run a) {
    __shared__ uint32_t lds[kLdsBytes / 4];
    const int tile = a.list[blockIdx.x];
    const Tile t = a.tiles[tile];
    const int xb = px_x0(tile % a.tiles_x), yb = px_y0(tile / a.tiles_x);
    const int pitch = box_pitch(t.bw), lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the fill's row arithmetic is scalar
    // per pixel, what does not depend on the image: rel = the tap (iy, ix)'s byte in a box whose rows start aligned
    // (0 for a pixel without a source: it reads the box's first bytes and drops them); meta = ax | ay << 5 |
    // live << 14 | (iy & 3) << 16
    int rel[kRows][4];
    uint32_t meta[kRows][4];
#pragma unroll
    for (int j = 0; j < kRows; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = xb + k, y = yb + 4 * j;
            const int2 e = x < a.W && y < a.H ? a.pack[(int64_t)y * a.W + x] : make_int2(kOutside, kOutside);
            rel[j][k] = 0;
            meta[j][k] = 0;
            if (e.x != kOutside) {
                const int ix = e.x >> 5, iy = e.y >> 5;
                rel[j][k] = (iy - t.y0) * pitch + (ix - t.x0);
                meta[j][k] = (uint32_t)(e.x & 31) | (uint32_t)(e.y & 31) << 5 | 1u << 14 | (uint32_t)(iy & 3) << 16;
            }
        }
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(lds);
    const int64_t span = (int64_t)(a.Hs - 1) * a.src_stride + a.Ws;
    const int cx0 = max(t.x0, 0), cx1 = min(t.x0 + t.bw, a.Ws);  // the box's in-source columns [cx0, cx1)
    const bool edge = t.x0 < 0 || t.x0 + t.bw > a.Ws;            // a zero column on one side at least
    const int first = blockIdx.y * a.group, last = min(a.n_img, first + a.group);
    for (int n = first; n < last; ++n) {
        const int64_t img = (int64_t)a.map + (int64_t)n * a.n_maps;
        const uint8_t* __restrict__ imgp = a.src + img * a.src_pitch;  // loads through it are global, not flat
        const uintptr_t base = reinterpret_cast<uintptr_t>(imgp);
        const uintptr_t img_end = base + (uintptr_t)span;
        uint8_t* __restrict__ dst = a.dst + img * a.dst_pitch;
        if (n != first) __syncthreads();  // the previous image's taps are read
        // The fill.  A wave owns the box rows wave, wave + 4, ...  Where the box has no zero row or column, a row is
        // at most kFillDw dwords and pitch / 4 dwords from every row's first lie inside the image (all boxes but those
        // at the image's first and last bytes), the loads of kFillRows of a wave's rows are issued together: one
        // memory latency per batch, not per row.  Every other box goes dword by dword.
        const int pd = pitch >> 2;
        const int64_t off0 = (int64_t)t.y0 * a.src_stride + t.x0;  // the box's first byte in the image
        const uintptr_t al_top = (base + (uintptr_t)off0) & ~(uintptr_t)3;
        const uintptr_t al_bot = (base + (uintptr_t)(off0 + (int64_t)(t.bh - 1) * a.src_stride)) & ~(uintptr_t)3;
        // a row between the first and the last: its first dword starts after row - 4 >= base, its pd dwords end before
        // row + Ws + 6 <= the last row's end when a row is at least 8 bytes long
        const bool fast = t.bh > 0 && pd <= kFillDw && !edge && t.y0 >= 0 && t.y0 + t.bh <= a.Hs && a.src_stride >= 8 &&
                          al_top >= base && al_bot + 4 * (uintptr_t)pd <= img_end;
        if (fast) {
            const bool m0 = lane < pd, m1 = lane + 64 < pd;
            for (int jb = wave; jb < t.bh; jb += (kNT / 64) * kFillRows) {
                uint32_t v[kFillRows][2];
#pragma unroll
                for (int i = 0; i < kFillRows; ++i) {
                    const int j = jb + (kNT / 64) * i;
                    if (j >= t.bh) continue;
                    const int64_t off = off0 + (int64_t)j * a.src_stride;
                    const uint32_t* __restrict__ rowp =
                        reinterpret_cast<const uint32_t*>(imgp + (off - (int64_t)((base + (uintptr_t)off) & 3)));
                    v[i][0] = m0 ? rowp[lane] : 0u;
                    v[i][1] = m1 ? rowp[lane + 64] : 0u;
                }
#pragma unroll
                for (int i = 0; i < kFillRows; ++i) {
                    const int j = jb + (kNT / 64) * i;
                    if (j >= t.bh) continue;
                    if (m0) lds[j * pd + lane] = v[i][0];
                    if (m1) lds[j * pd + lane + 64] = v[i][1];
                }
            }
        } else {
            for (int j = wave; j < t.bh; j += kNT / 64) {
                const BoxRow br = box_row(t, j, base, img_end, a.src_stride, a.Hs, cx0, cx1);
                for (int k = lane; k < br.ndw; k += 64) {
                    const uintptr_t p = br.al + 4 * (uintptr_t)k;
                    uint32_t x = 0;
                    if (br.whole) x = *reinterpret_cast<const uint32_t*>(imgp + (intptr_t)(p - base));
                    else if (br.in_row) x = rect_dword(p, br.lo, br.hi, base, img_end);
                    if (edge) x &= keep_mask(p, br.lo, br.hi);
                    lds[j * (pitch >> 2) + k] = x;
                }
            }
        }
        __syncthreads();
        const uint32_t a0 = (uint32_t)(base + (uintptr_t)(intptr_t)t.x0) & 3u, s4 = (uint32_t)a.src_stride & 3u;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int y = yb + 4 * j;
            if (y >= a.H) continue;
            uint32_t out = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int m_ = (int)meta[j][k], rl = rel[j][k];
                keep_in_loop(m_, rl);
                const uint32_t m = (uint32_t)m_;
                int o0, o1;
                if constexpr (kRowShift) {
                    const uint32_t sh0 = (a0 + ((m >> 16) & 3u) * s4) & 3u, sh1 = (sh0 + s4) & 3u;
                    o0 = rl + (int)sh0;
                    o1 = rl + pitch + (int)sh1;
                } else {
                    o0 = rl + (int)a0;
                    o1 = o0 + pitch;
                }
                const uint32_t v = blend(lb[o0], lb[o0 + 1], lb[o1], lb[o1 + 1], m & 31u, (m >> 5) & 31u);
                out |= ((m >> 14) & 1u ? v : 0u) << (8 * k);
            }
            store_row(dst + (int64_t)y * a.dst_stride + xb, xb, a.W, out);
        }
    }
}

}  // namespace rect
}  // namespace yavo

using yavo::rect::Tile;

struct yv_rectify {
    yv_ctx* ctx = nullptr;
    int n_maps = 0, Hs = 0, Ws = 0, H = 0, W = 0;
    int tiles_x = 0, n_tiles = 0;
    yavo::HipOwned mem;
    int32_t* d_map = nullptr;     // [n_maps][H][W][2] as set or computed (yv_rectify_map_read)
    int2* d_pack = nullptr;       // [n_maps][H][W] the kernels' form
    Tile* d_tiles = nullptr;      // [n_maps][n_tiles]
    int32_t* d_lds = nullptr;     // [n_maps][n_tiles] the tiles of the tile kernel, n_lds[map] of them
    int32_t* d_direct = nullptr;  // [n_maps][n_tiles] the direct kernel's
    std::vector<int> n_lds, n_direct;
    std::vector<uint8_t> is_set;
    bool force_direct = false;
};

namespace {

constexpr int kMaxSize = 8192, kMaxMaps = 16;

bool size_ok(int v) { return v >= 1 && v <= kMaxSize; }

// the map's int32 form is on the device (written on the context's stream or by a blocking copy): the kernels' form,
// the tile records and the two tile lists
int finish_map(yv_rectify* r, int m) {
    hipStream_t s = r->ctx->stream;
    const size_t px = (size_t)r->H * r->W, t0 = (size_t)m * r->n_tiles;
    hipLaunchKernelGGL(yavo::rect::rectify_prepare_kernel, dim3(r->n_tiles), dim3(yavo::rect::kNT), 0, s,
                       r->d_map + 2 * px * m, r->Hs, r->Ws, r->H, r->W, r->tiles_x, r->d_pack + px * m,
                       r->d_tiles + t0);
    if (yavo::check_launch() != YV_OK) return YV_ERR_HIP;
    std::vector<Tile> tiles((size_t)r->n_tiles);
    YV_HIP(hipMemcpyAsync(tiles.data(), r->d_tiles + t0, sizeof(Tile) * tiles.size(), hipMemcpyDeviceToHost, s));
    YV_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> lds, direct;
    for (int t = 0; t < r->n_tiles; ++t) (tiles[t].fits ? lds : direct).push_back(t);
    if (!lds.empty()) YV_HIP(hipMemcpy(r->d_lds + t0, lds.data(), sizeof(int32_t) * lds.size(), hipMemcpyHostToDevice));
    if (!direct.empty())
        YV_HIP(hipMemcpy(r->d_direct + t0, direct.data(), sizeof(int32_t) * direct.size(), hipMemcpyHostToDevice));
    r->n_lds[m] = (int)lds.size();
    r->n_direct[m] = (int)direct.size();
    r->is_set[m] = 1;
    return YV_OK;
}

}  // namespace

extern "C" {

int yv_rectify_create(yv_ctx* ctx, int n_maps, int src_H, int src_W, int dst_H, int dst_W, yv_rectify** out) {
    if (!out || !size_ok(src_H) || !size_ok(src_W) || !size_ok(dst_H) || !size_ok(dst_W) || n_maps < 1 ||
        n_maps > kMaxMaps)
        return YV_ERR_INVALID;
    *out = nullptr;
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    if (yavo::set_device(ctx) != YV_OK) return YV_ERR_HIP;
    yv_rectify* r = new (std::nothrow) yv_rectify();
    if (!r) return YV_ERR_INVALID;
    r->ctx = ctx;
    r->n_maps = n_maps;
    r->Hs = src_H;
    r->Ws = src_W;
    r->H = dst_H;
    r->W = dst_W;
    r->tiles_x = (dst_W + yavo::rect::kTileW - 1) / yavo::rect::kTileW;
    r->n_tiles = r->tiles_x * ((dst_H + yavo::rect::kTileH - 1) / yavo::rect::kTileH);
    r->n_lds.assign((size_t)n_maps, 0);
    r->n_direct.assign((size_t)n_maps, 0);
    r->is_set.assign((size_t)n_maps, 0);
    const size_t px = (size_t)dst_H * dst_W * n_maps, nt = (size_t)r->n_tiles * n_maps;
    if (r->mem.alloc(&r->d_map, 2 * px) != YV_OK || r->mem.alloc(&r->d_pack, px) != YV_OK ||
        r->mem.alloc(&r->d_tiles, nt) != YV_OK || r->mem.alloc(&r->d_lds, nt) != YV_OK ||
        r->mem.alloc(&r->d_direct, nt) != YV_OK) {
        delete r;
        return YV_ERR_HIP;
    }
    *out = r;
    return YV_OK;
}

void yv_rectify_destroy(yv_rectify* r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    (void)hipDeviceSynchronize();  // a run in flight, on any stream, reads the maps
    delete r;
}

int yv_rectify_set_model(yv_rectify* r, int map, const double K[9], const double dist[8], const double M[9]) {
    if (!r || !K || !dist || !M || map < 0 || map >= r->n_maps) return YV_ERR_INVALID;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i]) || !std::isfinite(M[i]) || (i < 8 && !std::isfinite(dist[i]))) return YV_ERR_INVALID;
    if (yavo::set_device(r->ctx) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipDeviceSynchronize());  // a run in flight, on any stream, reads the map
    yavo::rect::Model m;
    m.fx = K[0];
    m.cx = K[2];
    m.fy = K[4];
    m.cy = K[5];
    std::memcpy(m.d, dist, sizeof(m.d));
    std::memcpy(m.M, M, sizeof(m.M));
    const size_t px = (size_t)r->H * r->W;
    hipLaunchKernelGGL(yavo::rect::rectify_model_kernel, dim3((unsigned)((px + yavo::rect::kNT - 1) / yavo::rect::kNT)),
                       dim3(yavo::rect::kNT), 0, r->ctx->stream, m, r->H, r->W, r->d_map + 2 * px * map);
    if (yavo::check_launch() != YV_OK) return YV_ERR_HIP;
    return finish_map(r, map);
}

int yv_rectify_set_map(yv_rectify* r, int map, const int32_t* map_q5) {
    if (!r || !map_q5 || map < 0 || map >= r->n_maps) return YV_ERR_INVALID;
    if (yavo::set_device(r->ctx) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipDeviceSynchronize());  // a run in flight, on any stream, reads the map
    const size_t px = (size_t)r->H * r->W;
    YV_HIP(hipMemcpy(r->d_map + 2 * px * map, map_q5, sizeof(int32_t) * 2 * px, hipMemcpyHostToDevice));
    return finish_map(r, map);
}

int yv_rectify_map_read(yv_rectify* r, int map, int32_t* map_q5) {
    if (!r || !map_q5 || map < 0 || map >= r->n_maps || !r->is_set[map]) return YV_ERR_INVALID;
    if (yavo::set_device(r->ctx) != YV_OK) return YV_ERR_HIP;
    const size_t px = (size_t)r->H * r->W;
    YV_HIP(hipMemcpy(map_q5, r->d_map + 2 * px * map, sizeof(int32_t) * 2 * px, hipMemcpyDeviceToHost));
    return YV_OK;
}

int yv_rectify_run(yv_rectify* r, const uint8_t* d_src, int src_stride, int64_t src_pitch, uint8_t* d_dst,
                   int dst_stride, int64_t dst_pitch, int n_images, void* stream) {
    if (!r || n_images < 0 || src_stride < r->Ws || dst_stride < r->W || (n_images > 0 && (!d_src || !d_dst)))
        return YV_ERR_INVALID;
    for (int m = 0; m < r->n_maps && m < n_images; ++m)
        if (!r->is_set[m]) return YV_ERR_INVALID;
    if (n_images == 0) return YV_OK;
    if (yavo::set_device(r->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->ctx->stream;
    const size_t px = (size_t)r->H * r->W;
    for (int m = 0; m < r->n_maps && m < n_images; ++m) {
        yavo::rect::Run a;
        a.src = d_src;
        a.dst = d_dst;
        a.src_pitch = src_pitch;
        a.dst_pitch = dst_pitch;
        a.src_stride = src_stride;
        a.dst_stride = dst_stride;
        a.Hs = r->Hs;
        a.Ws = r->Ws;
        a.H = r->H;
        a.W = r->W;
        a.map = m;
        a.n_maps = r->n_maps;
        a.n_img = (n_images - m + r->n_maps - 1) / r->n_maps;
        a.group = std::max(yavo::rect::kGroup, (a.n_img + 65534) / 65535);  // grid.y <= 65535
        a.tiles_x = r->tiles_x;
        a.pack = r->d_pack + px * m;
        a.tiles = r->d_tiles + (size_t)m * r->n_tiles;
        const unsigned groups = (unsigned)((a.n_img + a.group - 1) / a.group);
        const int n_lds = r->force_direct ? 0 : r->n_lds[m];
        const int n_direct = r->force_direct ? r->n_tiles : r->n_direct[m];
        if (n_lds > 0) {
            a.list = r->d_lds + (size_t)m * r->n_tiles;
            if (src_stride & 3)
                hipLaunchKernelGGL(yavo::rect::rectify_tile_kernel<true>, dim3((unsigned)n_lds, groups),
                                   dim3(yavo::rect::kNT), 0, s, a);
            else
                hipLaunchKernelGGL(yavo::rect::rectify_tile_kernel<false>, dim3((unsigned)n_lds, groups),
                                   dim3(yavo::rect::kNT), 0, s, a);
        }
        if (n_direct > 0) {
            a.list = r->force_direct ? nullptr : r->d_direct + (size_t)m * r->n_tiles;
            hipLaunchKernelGGL(yavo::rect::rectify_direct_kernel, dim3((unsigned)n_direct, groups),
                               dim3(yavo::rect::kNT), 0, s, a);
        }
    }
    return yavo::check_launch();
}

int yv_rectify_image(yv_ctx* ctx, const uint8_t* src, int src_H, int src_W, int src_stride, const int32_t* map_q5,
                     uint8_t* dst, int dst_H, int dst_W, int dst_stride) {
    if (!src || !map_q5 || !dst || !size_ok(src_H) || !size_ok(src_W) || !size_ok(dst_H) || !size_ok(dst_W) ||
        src_stride < src_W || dst_stride < dst_W)
        return YV_ERR_INVALID;
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    yv_rectify* r = nullptr;
    int st = yv_rectify_create(ctx, 1, src_H, src_W, dst_H, dst_W, &r);
    if (st != YV_OK) return st;
    uint8_t *d_s = nullptr, *d_d = nullptr;
    const auto body = [&]() -> int {
        const int rc = yv_rectify_set_map(r, 0, map_q5);
        if (rc != YV_OK) return rc;
        if (r->mem.alloc(&d_s, (size_t)src_H * src_W) != YV_OK || r->mem.alloc(&d_d, (size_t)dst_H * dst_W) != YV_OK)
            return YV_ERR_HIP;
        YV_HIP(hipMemcpy2D(d_s, (size_t)src_W, src, (size_t)src_stride, (size_t)src_W, (size_t)src_H,
                           hipMemcpyHostToDevice));
        const int rr = yv_rectify_run(r, d_s, src_W, (int64_t)src_H * src_W, d_d, dst_W, (int64_t)dst_H * dst_W, 1,
                                      nullptr);
        if (rr != YV_OK) return rr;
        YV_HIP(hipStreamSynchronize(ctx->stream));
        // the destination's rows only: the bytes between them stay the caller's
        YV_HIP(hipMemcpy2D(dst, (size_t)dst_stride, d_d, (size_t)dst_W, (size_t)dst_W, (size_t)dst_H,
                           hipMemcpyDeviceToHost));
        return YV_OK;
    };
    st = body();
    yv_rectify_destroy(r);
    return st;
}

int yv_rectify_debug_tiles(yv_rectify* r, int map, int32_t* n_lds, int32_t* n_direct) {
    if (!r || !n_lds || !n_direct || map < 0 || map >= r->n_maps || !r->is_set[map]) return YV_ERR_INVALID;
    *n_lds = r->n_lds[map];
    *n_direct = r->n_direct[map];
    return YV_OK;
}

int yv_rectify_debug_force_direct(yv_rectify* r, int on) {
    if (!r) return YV_ERR_INVALID;
    r->force_direct = on != 0;
    return YV_OK;
}

}  // extern "C"
