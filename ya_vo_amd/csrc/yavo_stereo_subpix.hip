// yavo_stereo_subpix.hip -- sub-pixel stereo disparity (yv_stereo_subpix / yv_batch_set_stereo_subpix, DESIGN.md
// section 19): around a descriptor match, the SAD of the (2w + 1)^2 window of the raw left image against the right
// image at the column shifts -s..s, the first minimum in the order 0, -1, +1, ..., and the vertex of the parabola
// through it in 1/256 pixel.  All integer.
//
// One 16-lane DPP row per match, four matches per wave: lane l < 2w + 1 owns window row l.  It loads its <= 15 left
// and <= 31 right bytes as aligned dwords, shifts them into place with v_alignbyte and accumulates the 2s + 1 <= 17
// sums with v_sad_u8 (four byte differences per instruction).  The sums sit in 17 registers at fixed positions (shift
// k in register k + 8), so no register array is indexed at run time.  The rows are added with four DPP butterflies
// (yavo_xlane.h); no LDS, no barrier.
//
// No read leaves the image: a match is attempted only if its two footprints lie inside [0, H) x [0, W), every byte
// load reads a footprint byte, and every dword load is issued only after its four bytes were tested to lie inside
// [image, image + (H - 1) * stride + W) (subpix_dword); a dword that fails the test is assembled from the footprint
// bytes it holds.
#include "yavo_internal.h"
#include "yavo_xlane.h"

namespace yavo {
namespace subpix {

constexpr int SP_NT = 256;             // 4 waves = 16 matches per workgroup
constexpr int SP_PER_WG = SP_NT / 16;

// The dword at address p (4-byte aligned) restricted to the bytes inside [lo, hi) (the lane's footprint bytes): zero
// when the dword holds none; one aligned load when all four bytes are inside [img, img_end); byte loads of the
// footprint bytes otherwise.  Bytes outside [lo, hi) of a whole-dword load are whatever the image holds there: the
// callers mask or never use them.
__device__ __forceinline__ uint32_t subpix_dword(uintptr_t p, uintptr_t lo, uintptr_t hi, uintptr_t img,
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

// mask of the bytes [4 j, 4 j + 4) that lie below n
__device__ __forceinline__ uint32_t byte_mask(int j, int n) {
    const int k = n - 4 * j;
    return k >= 4 ? 0xFFFFFFFFu : (k <= 0 ? 0u : (0xFFFFFFFFu >> (8 * (4 - k))));
}

struct Result {
    int dcol, sad, status;
};

// The refinement of one match by the 16 lanes of a DPP row (all 16 call it, with the same arguments; `row_lane` is
// the lane's index in the row).  img_l / img_r: first byte of the two images.
__device__ __forceinline__ Result subpix_match(const uint8_t* __restrict__ img_l, const uint8_t* __restrict__ img_r,
                                               int H, int W, int stride, int r, int c, int r2, int c2, int w, int s,
                                               int row_lane) {
    Result res{0, -1, kSubpixOutside};
    const bool inside = r - w >= 0 && r + w < H && c - w >= 0 && c + w < W && r2 - w >= 0 && r2 + w < H &&
                        c2 - s - w >= 0 && c2 + s + w < W;
    if (!inside) return res;  // uniform over the row
    const int n = 2 * w + 1;
    const int64_t span = (int64_t)(H - 1) * stride + W;
    uint32_t Lb[4] = {0u, 0u, 0u, 0u};
    uint32_t Rb[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (row_lane < n) {
        // left: bytes [0, n) of the row from column c - w
        {
            const uintptr_t base = reinterpret_cast<uintptr_t>(img_l);
            const uintptr_t a = base + (uintptr_t)((int64_t)(r - w + row_lane) * stride + (c - w));
            const uintptr_t a0 = a & ~(uintptr_t)3;
            const uint32_t sh = (uint32_t)(a & 3);
            uint32_t A[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) A[k] = subpix_dword(a0 + 4 * k, a, a + n, base, base + (uintptr_t)span);
#pragma unroll
            for (int j = 0; j < 4; ++j) Lb[j] = __builtin_amdgcn_alignbyte(A[j + 1], A[j], sh) & byte_mask(j, n);
        }
        // right: the row from the virtual column c2 - 8 - w (shift k starts at byte k + 8 whatever s is), of which
        // only the footprint columns [c2 - s - w, c2 + s + w] are loaded; the virtual start may lie before the image
        // and is never dereferenced
        {
            const uintptr_t base = reinterpret_cast<uintptr_t>(img_r);
            const int64_t row_off = (int64_t)(r2 - w + row_lane) * stride;
            const uintptr_t lo = base + (uintptr_t)(row_off + (c2 - s - w));
            const uintptr_t hi = lo + (uintptr_t)(2 * s + n);
            const intptr_t v = (intptr_t)base + (intptr_t)(row_off + (c2 - kSubpixMaxSearch - w));
            const uintptr_t v0 = (uintptr_t)v & ~(uintptr_t)3;
            const uint32_t sh = (uint32_t)((uintptr_t)v & 3);
            uint32_t A[10];
#pragma unroll
            for (int k = 0; k < 9; ++k) A[k] = subpix_dword(v0 + 4 * k, lo, hi, base, base + (uintptr_t)span);
            A[9] = 0u;  // bytes 33.. of the virtual row: past shift +8's last column
#pragma unroll
            for (int j = 0; j < 9; ++j) Rb[j] = __builtin_amdgcn_alignbyte(A[j + 1], A[j], sh);
        }
    }
    // S[k + 8] = this lane's row of SAD_k; lanes >= n hold zeros on both sides
    uint32_t S[17];
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        S[i] = 0u;
        const int k = i - kSubpixMaxSearch;
        if (k >= -s && k <= s) {  // uniform
            uint32_t acc = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (4 * j < n) {  // uniform
                    // bytes [i + 4 j, i + 4 j + 4) of the virtual row
                    const int d = (i + 4 * j) >> 2, sh = (i + 4 * j) & 3;
                    const uint32_t hi = d + 1 < 9 ? Rb[d + 1] : 0u;
                    const uint32_t rv = __builtin_amdgcn_alignbyte(hi, Rb[d], (uint32_t)sh) & byte_mask(j, n);
                    acc = __builtin_amdgcn_sad_u8(Lb[j], rv, acc);
                }
            }
            acc += (uint32_t)xl::xor_row_i32<1>((int)acc);
            acc += (uint32_t)xl::xor_row_i32<2>((int)acc);
            acc += (uint32_t)xl::xor_row_i32<4>((int)acc);
            acc += (uint32_t)xl::xor_row_i32<8>((int)acc);
            S[i] = acc;
        }
    }
    // the first minimum in the order 0, -1, +1, -2, +2, ...
    int best = (int)S[kSubpixMaxSearch], kb = 0;
#pragma unroll
    for (int d = 1; d <= kSubpixMaxSearch; ++d) {
        if (d <= s) {
            const int lo = (int)S[kSubpixMaxSearch - d], hi = (int)S[kSubpixMaxSearch + d];
            if (lo < best) { best = lo; kb = -d; }
            if (hi < best) { best = hi; kb = d; }
        }
    }
    if (kb == s || kb == -s) {
        res.sad = best;
        res.status = kSubpixEdge;
        return res;
    }
    int a = 0, cc = 0;
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        if (i == kb + kSubpixMaxSearch - 1) a = (int)S[i];
        if (i == kb + kSubpixMaxSearch + 1) cc = (int)S[i];
    }
    const int den = a + cc - 2 * best;
    int frac = 0;
    if (den != 0) {
        const int num = 256 * (a - cc) + den, d2 = 2 * den;
        frac = num / d2;
        if (num % d2 < 0) --frac;  // floor
    }
    res.dcol = 256 * kb + frac;
    res.sad = best;
    res.status = kSubpixOk;
    return res;
}

__global__ __launch_bounds__(SP_NT) void subpix_list_kernel(const uint8_t* __restrict__ left,
                                                            const uint8_t* __restrict__ right, int H, int W, int stride,
                                                            const yv_match* __restrict__ m, int n, int w, int s,
                                                            int32_t* __restrict__ dcol_q8, int32_t* __restrict__ sad,
                                                            uint8_t* __restrict__ status) {
    const int i = blockIdx.x * SP_PER_WG + (threadIdx.x >> 4), row_lane = threadIdx.x & 15;
    if (i >= n) return;  // uniform over the row
    const Result r = subpix_match(left, right, H, W, stride, m[i].pt1.x, m[i].pt1.y, m[i].pt2.x, m[i].pt2.y, w, s,
                                  row_lane);
    if (row_lane == 0) {
        dcol_q8[i] = r.dcol;
        sad[i] = r.sad;
        status[i] = (uint8_t)r.status;
    }
}

// grid (ceil(max_kp / SP_PER_WG), n_marked): the workgroups of one pair are neighbours in launch order, so its two
// images stay in L2 while it runs
template <bool KEEP>
__global__ __launch_bounds__(SP_NT) void subpix_batch_kernel(
    const uint8_t* __restrict__ images, int n_images, int H, int W, int stride, int64_t pitch,
    const int32_t* __restrict__ marked, const int32_t* __restrict__ pairs, const yv_keypoint* __restrict__ keypoints,
    const int32_t* __restrict__ kp_count, const int2* __restrict__ match_dj, const int32_t* __restrict__ match_lim,
    const uint8_t* __restrict__ keep, int max_kp, int w, int s, int32_t* __restrict__ dcol_q8,
    int32_t* __restrict__ sad, uint8_t* __restrict__ status) {
    const int i = blockIdx.x * SP_PER_WG + (threadIdx.x >> 4), row_lane = threadIdx.x & 15;
    if (i >= max_kp) return;  // uniform over the row
    const int p = marked[blockIdx.y];
    const int qs = pairs[2 * p], ts = pairs[2 * p + 1];
    const int64_t o = (int64_t)p * max_kp + i;
    Result r{0, -1, kSubpixNone};
    if (qs < n_images && ts < n_images && i < kp_count[qs]) {
        const int2 a = match_dj[o];
        bool k = a.x < match_lim[p] && a.y >= 0;
        if constexpr (KEEP) k = k && keep[o] != 0;
        if (k) {
            const yv_keypoint* kl = keypoints + (int64_t)qs * max_kp + i;
            const yv_keypoint* kr = keypoints + (int64_t)ts * max_kp + a.y;
            r = subpix_match(images + (int64_t)qs * pitch, images + (int64_t)ts * pitch, H, W, stride, kl->x, kl->y,
                             kr->x, kr->y, w, s, row_lane);
        }
    }
    if (row_lane == 0) {
        dcol_q8[o] = r.dcol;
        sad[o] = r.sad;
        status[o] = (uint8_t)r.status;
    }
}

}  // namespace subpix

void launch_subpix_list(const uint8_t* left, const uint8_t* right, int H, int W, int stride, const yv_match* m, int n,
                        int half_win, int search, const SubpixOut& out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(subpix::subpix_list_kernel, dim3((n + subpix::SP_PER_WG - 1) / subpix::SP_PER_WG),
                       dim3(subpix::SP_NT), 0, s, left, right, H, W, stride, m, n, half_win, search, out.dcol_q8,
                       out.sad, out.status);
}

void launch_subpix_batch(const uint8_t* images, int n_images, int H, int W, int stride, int64_t pitch,
                         const int32_t* marked, int n_marked, const int32_t* pairs, const yv_keypoint* keypoints,
                         const int32_t* kp_count, const int2* match_dj, const int32_t* match_lim,
                         const uint8_t* keep, int max_kp, int half_win, int search, const SubpixOut& out,
                         hipStream_t s) {
    if (n_marked <= 0) return;
    const dim3 grid((max_kp + subpix::SP_PER_WG - 1) / subpix::SP_PER_WG, n_marked);
    if (keep)
        hipLaunchKernelGGL((subpix::subpix_batch_kernel<true>), grid, dim3(subpix::SP_NT), 0, s, images, n_images, H, W,
                           stride, pitch, marked, pairs, keypoints, kp_count, match_dj, match_lim, keep, max_kp,
                           half_win, search, out.dcol_q8, out.sad, out.status);
    else
        hipLaunchKernelGGL((subpix::subpix_batch_kernel<false>), grid, dim3(subpix::SP_NT), 0, s, images, n_images, H,
                           W, stride, pitch, marked, pairs, keypoints, kp_count, match_dj, match_lim, keep, max_kp,
                           half_win, search, out.dcol_q8, out.sad, out.status);
}

}  // namespace yavo
