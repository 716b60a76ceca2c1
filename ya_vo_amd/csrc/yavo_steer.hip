// yavo_steer.hip -- rotation-steered BRIEF (yv_set_brief_steering): the keypoint's orientation
// bin from the intensity centroid of its blurred patch, then the 256 tests of that bin's rotated pattern.  Integer
// only.  Every sample is S(r, c) = blurred[clamp(r, 0, H - 1)][clamp(c, 0, W - 1)]: no padding column, no column W,
// no row H, nothing out of bounds.  brief_kernel (yavo_brief.hip) stays the path with steering off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "yavo_internal.h"
#include "yavo_xlane.h"

namespace yavo {

namespace {

// One wave per keypoint, ST_KPW keypoints per wave one after the other.  The wave keeps the keypoint's patch, rows
// -15 .. 15 and columns -15 .. 16 around it, in its own LDS slice of 31 rows x kSteerPatchStride bytes: no other wave
// touches the slice, so the kernel has no workgroup barrier.
constexpr int ST_NT = 256;
constexpr int ST_NW = ST_NT / 64;
constexpr int ST_KPW = 8;
constexpr int ST_KPB = ST_NW * ST_KPW;  // keypoints per workgroup
constexpr int ST_ROWS = 2 * kSteerMaxRadius + 1;
constexpr int ST_LS = kSteerPatchStride;
constexpr int ST_SLICE = ST_ROWS * ST_LS;
// an inner keypoint's rows come as aligned dwords from the first one that holds column -15: 9 cover 32 columns at any
// of the four byte phases
constexpr int ST_ROW_DW = 9;
static_assert(4 * ST_ROW_DW <= ST_LS && ST_LS % 4 == 0 && ST_SLICE % 4 == 0, "dword rows inside the slice");
static_assert(kSteerMaxRadius == 15, "the patch is 31 rows of 32 columns: 16 cells per lane");
static_assert(kSteerMaxBins <= 64, "lanes are bins");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the wave's total / maximum of v in every lane: DPP butterflies inside the 16-lane rows, then the four rows' values
__device__ __forceinline__ int wave_sum(int v) {
    v += xl::xor_row_i32<1>(v);
    v += xl::xor_row_i32<2>(v);
    v += xl::xor_row_i32<4>(v);
    v += xl::xor_row_i32<8>(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

__device__ __forceinline__ int wave_max(int v) {
    v = max(v, xl::xor_row_i32<1>(v));
    v = max(v, xl::xor_row_i32<2>(v));
    v = max(v, xl::xor_row_i32<4>(v));
    v = max(v, xl::xor_row_i32<8>(v));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// w[k] for a lane's own k (0 outside 0 .. 7): the words are wave-uniform, the index is not
__device__ __forceinline__ uint32_t pick8(const uint32_t (&w)[8], int k) {
    uint32_t r = 0u;
#pragma unroll
    for (int q = 0; q < 8; ++q) r = k == q ? w[q] : r;
    return r;
}

// The wave's LDS accesses execute in order; the fence keeps the compiler from moving one lane's reads above another
// lane's writes of the same slice.
__device__ __forceinline__ void slice_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// src: kDescribe ? kp_src [image][max_kp] int4 {row, col, id, -} : positions [image][max_kp] int2 {row, col}; count
// [image].  Keypoint i of image blockIdx.y writes bin[i], moments[i] = (m10, m01) and, kDescribe, keypoints[i] and
// desc[i].  taddr: steer_pack_offsets' form of the offsets table.
template <bool kDescribe>
__global__ __launch_bounds__(ST_NT) void brief_steer_kernel(const uint8_t* __restrict__ blur, int H, int W,
                                                            const int32_t* __restrict__ src,
                                                            const int32_t* __restrict__ count, int max_kp, int n_bins,
                                                            int radius, const int16_t* __restrict__ dirs,
                                                            const uint32_t* __restrict__ taddr,
                                                            yv_keypoint* __restrict__ keypoints,
                                                            Desc* __restrict__ desc, uint8_t* __restrict__ o_bin,
                                                            int32_t* __restrict__ o_mom) {
    __shared__ __attribute__((aligned(16))) uint8_t s_patch[ST_NW * ST_SLICE];
    const int img = blockIdx.y;
    const int n = min(count[img], max_kp);
    const int first = (int)blockIdx.x * ST_KPB;
    if (first >= n) return;
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    uint8_t* sp = s_patch + wave * ST_SLICE;
    const int bp = blur_pitch(W);
    const uint8_t* b = blur + (int64_t)img * H * bp;
    constexpr int kSrcInts = kDescribe ? 4 : 2;
    const int32_t* kp = src + (int64_t)img * max_kp * kSrcInts;
    const int64_t out0 = (int64_t)img * max_kp;
    // lanes are bins
    int dx = 0, dy = 0;
    if (lane < n_bins) {
        dx = dirs[2 * lane];
        dy = dirs[2 * lane + 1];
    }
    // the patch as 16 cells per lane: column pc (dc = pc - 15) of rows 2 u + half, u = 0 .. 15 (row 31 does not exist;
    // column 31, dc = 16, lies outside every disc and is there for the tests' row of 32 only)
    const int pc = lane & 31, half = lane >> 5;
    const int dcl = pc - kSteerMaxRadius;
    const int lim = radius * radius - dcl * dcl;  // the disc: dr^2 <= lim

    for (int j = 0; j < ST_KPW; ++j) {
        const int i = first + wave + ST_NW * j;
        if (i >= n) break;  // wave-uniform
        const int row = __builtin_amdgcn_readfirstlane(kp[(int64_t)i * kSrcInts]);
        const int col = __builtin_amdgcn_readfirstlane(kp[(int64_t)i * kSrcInts + 1]);
        // 1. the clamped patch.  sh: the byte phase of column -15 inside its row in the slice
        int sh = 0;
        if (row >= 15 && row + 15 <= H - 1 && col >= 15 && col + 16 <= W - 1) {
            // at least 16 pixels from every border: rows of aligned dwords.  The last one starts at a column <= col +
            // 17 <= W < the pitch, a multiple of 4: inside the row's pitch.
            const int c0 = (col - 15) & ~3;
            sh = (col - 15) & 3;
            const uint8_t* p = b + (int64_t)(row - 15) * bp + c0;
            uint32_t v[5];
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int k = lane + 64 * u, r = k / ST_ROW_DW, q = k - r * ST_ROW_DW;
                v[u] = k < ST_ROWS * ST_ROW_DW ? *reinterpret_cast<const uint32_t*>(p + (int64_t)r * bp + 4 * q) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int k = lane + 64 * u, r = k / ST_ROW_DW, q = k - r * ST_ROW_DW;
                if (k < ST_ROWS * ST_ROW_DW) *reinterpret_cast<uint32_t*>(sp + r * ST_LS + 4 * q) = v[u];
            }
        } else {
            const int cc = clampi(col + dcl, 0, W - 1);
#pragma unroll 4
            for (int u = 0; u < 16; ++u) {
                const int r = 2 * u + half;
                if (r < ST_ROWS) sp[r * ST_LS + pc] = b[(int64_t)clampi(row + r - 15, 0, H - 1) * bp + cc];
            }
        }
        slice_sync();
        // 2. the moments over the disc dr^2 + dc^2 <= radius^2
        int sv = 0, sdr = 0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = 2 * u + half, dr = r - 15;
            if (r < ST_ROWS && dr * dr <= lim) {
                const int v = sp[r * ST_LS + pc + sh];
                sv += v;
                sdr += dr * v;
            }
        }
        const int m10 = wave_sum(dcl * sv), m01 = wave_sum(sdr);
        // 3. the bin: the smallest k that maximises m10 dirs[k][0] + m01 dirs[k][1] (|score| < 2^31 by the ranges
        // yv_set_brief_steering accepts)
        const int score = lane < n_bins ? m10 * dx + m01 * dy : INT_MIN;
        const int best = wave_max(score);
        const uint64_t at = __ballot(lane < n_bins && score == best);
        const int bin = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(at));
        if (lane == 0) {
            o_bin[out0 + i] = (uint8_t)bin;
            reinterpret_cast<int2*>(o_mom)[out0 + i] = make_int2(m10, m01);
        }
        if constexpr (kDescribe) {
            // 4. lane l takes tests 64 g + l: the ballot is word g of the descriptor
            const uint32_t* ta = taddr + bin * 256;
            uint32_t w[8];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t a = ta[64 * g + lane];
                const uint32_t p1 = sp[(a & 0xFFFFu) + sh], p2 = sp[(a >> 16) + sh];
                const uint64_t m = __ballot(p1 > p2);
                w[2 * g] = (uint32_t)m;
                w[2 * g + 1] = (uint32_t)(m >> 32);
            }
            // 5. the packed descriptor by lanes 0 .. 7; the 48-B record {row, col, id, matched = 0, featVec[32], 3 zero
            // bytes} as its 12 dwords by lanes 0 .. 11: featVec starts at byte 13, so dword d >= 3 is the last byte
            // of word d - 4 and the first three of word d - 3
            if (lane < 8) desc[out0 + i].w[lane] = pick8(w, lane);
            if (lane < 12) {
                uint32_t v = (pick8(w, lane - 4) >> 24) | (pick8(w, lane - 3) << 8);
                if (lane == 0) v = (uint32_t)row;
                if (lane == 1) v = (uint32_t)col;
                if (lane == 2) v = (uint32_t)kp[(int64_t)i * kSrcInts + 2];
                reinterpret_cast<uint32_t*>(keypoints + out0 + i)[lane] = v;
            }
        }
        slice_sync();  // the next keypoint's patch overwrites the slice
    }
}

}  // namespace

void steer_pack_offsets(const int8_t* offsets, int n_tests, uint32_t* out) {
    for (int t = 0; t < n_tests; ++t) {
        const int8_t* o = offsets + 4 * (size_t)t;
        const uint32_t a1 = (uint32_t)((o[0] + kSteerMaxRadius) * ST_LS + o[1] + kSteerMaxRadius);
        const uint32_t a2 = (uint32_t)((o[2] + kSteerMaxRadius) * ST_LS + o[3] + kSteerMaxRadius);
        out[t] = a1 | (a2 << 16);
    }
}

void launch_brief_steer(const uint8_t* blur, int n_images, int H, int W, const SteerTables& t, const int32_t* kp_src,
                        const int32_t* kp_count, int max_kp, yv_keypoint* keypoints, Desc* desc, uint8_t* bin,
                        int32_t* moments, hipStream_t s) {
    const dim3 grid((max_kp + ST_KPB - 1) / ST_KPB, n_images);
    hipLaunchKernelGGL(brief_steer_kernel<true>, grid, dim3(ST_NT), 0, s, blur, H, W, kp_src, kp_count, max_kp,
                       t.n_bins, t.radius, t.dirs, t.taddr, keypoints, desc, bin, moments);
}

void launch_orient(const uint8_t* blur, int H, int W, const SteerTables& t, const int32_t* rc, const int32_t* count,
                   int max_kp, uint8_t* bin, int32_t* moments, hipStream_t s) {
    const dim3 grid((max_kp + ST_KPB - 1) / ST_KPB, 1);
    hipLaunchKernelGGL(brief_steer_kernel<false>, grid, dim3(ST_NT), 0, s, blur, H, W, rc, count, max_kp, t.n_bins,
                       t.radius, t.dirs, t.taddr, static_cast<yv_keypoint*>(nullptr), static_cast<Desc*>(nullptr), bin,
                       moments);
}

}  // namespace yavo
