// yavo_pyramid.hip -- the opt-in scale pyramid of the front end (yv_batch_set_pyramid): the level
// images (pyr_level_kernel: the integer bilinear resample of section 20's remap at positions given in closed form), the
// merge of the levels' keypoints into the base batch's slots (pyr_merge_kernel), and the host side: the batch's level
// workspaces, the three front stages of a multi-scale yv_batch_run and the host-pointer forms.
//
// A destination level is cut into kTileH x kTileW tiles, one workgroup each.  A tile's taps lie in a box of at most
// 2 kTileH + 1 rows and 2 kTileW + 1 columns of the source (the shrink per level is at most 2), which the workgroup
// stages in LDS with aligned dword loads; the four taps of a pixel come out of LDS.
//
// No read leaves the source: the box holds in-source positions only, and a dword load is issued only after its four
// bytes were tested to lie inside [image, image + (Hs - 1) * stride + Ws); a dword that fails the test is assembled from
// the box row's own bytes.  A destination is the library's own: rows dst_stride bytes apart with dst_stride a multiple
// of 4 and a 4-byte aligned first pixel; the columns [W, dst_stride) of a row are written as zero.
#include "yavo_host.h"

namespace yavo {
namespace pyr {

constexpr int kTileW = 128, kTileH = 16;  // destination tile: 32 lanes x 4 pixels wide, 8 half-waves x 2 rows high
constexpr int kNT = 256;
constexpr int kBoxH = 2 * kTileH + 1, kBoxW = 2 * kTileW + 1;
// bytes between two rows of the staged box: its width plus the up to 3 bytes before its first column in the row's
// first aligned dword, in whole dwords
__host__ __device__ constexpr int box_pitch(int bw) { return ((bw + 6) >> 2) * 4; }
constexpr int kLdsBytes = kBoxH * box_pitch(kBoxW);

// The source position of destination index r, in 1/32 pixel (n_src >= n_dst, so the numerator is positive; at most
// (2 * 8191 + 1) * 8192 * 16 < 2^32).
__host__ __device__ inline int src_pos(int r, int n_src, int n_dst) {
    const uint32_t num = ((uint32_t)(2 * r + 1) * (uint32_t)n_src - (uint32_t)n_dst) * 16u;
    const uint32_t q = num / (uint32_t)n_dst, top = (uint32_t)(n_src - 1) * 32u;
    return (int)(q < top ? q : top);
}

// section 20's blend: ((32 - ay) * t + ay * b + 512) >> 10 with t = (32 - ax) * p00 + ax * p01, b the lower row's
__device__ __forceinline__ uint32_t blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t ax,
                                          uint32_t ay) {
    const int t = (int)(p00 << 5) + (int)ax * ((int)p01 - (int)p00);
    const int b = (int)(p10 << 5) + (int)ax * ((int)p11 - (int)p10);
    return (uint32_t)((t << 5) + (int)ay * (b - t) + 512) >> 10;
}

struct LevelArgs {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_pitch, dst_pitch;  // bytes between images
    int src_stride, dst_stride, Hs, Ws, H, W;
    int tiles_x;
};

// grid (tiles, images)
__global__ __launch_bounds__(kNT) void pyr_level_kernel(LevelArgs a) {
    __shared__ uint32_t lds[kLdsBytes / 4];
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int xb = tx * kTileW, yb = ty * kTileH;
    const int x1 = min(xb + kTileW, a.W) - 1, y1 = min(yb + kTileH, a.H) - 1;  // the tile's last live pixel
    // the box of the tile's taps, inside the source (positions grow with the index)
    const int bx0 = src_pos(xb, a.Ws, a.W) >> 5, by0 = src_pos(yb, a.Hs, a.H) >> 5;
    const int bw = min(min((src_pos(x1, a.Ws, a.W) >> 5) + 1, a.Ws - 1) - bx0 + 1, kBoxW);
    const int bh = min(min((src_pos(y1, a.Hs, a.H) >> 5) + 1, a.Hs - 1) - by0 + 1, kBoxH);
    const int pitch = box_pitch(bw), pd = pitch >> 2;
    const uint8_t* __restrict__ img = a.src + (int64_t)blockIdx.y * a.src_pitch;
    const uintptr_t base = reinterpret_cast<uintptr_t>(img);
    const uintptr_t img_end = base + (uintptr_t)((int64_t)(a.Hs - 1) * a.src_stride + a.Ws);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // A wave owns the box rows wave, wave + 4, ...  Where pd dwords from every row's first aligned dword lie inside the
    // image (every box but those at the image's first and last bytes), the loads of all of a wave's rows are issued
    // together: one memory latency per tile, not per row.  Every other box goes dword by dword.
    const int64_t off0 = (int64_t)by0 * a.src_stride + bx0;
    const uintptr_t al_top = (base + (uintptr_t)off0) & ~(uintptr_t)3;
    const uintptr_t al_bot = (base + (uintptr_t)(off0 + (int64_t)(bh - 1) * a.src_stride)) & ~(uintptr_t)3;
    const bool fast = al_top >= base && al_bot + 4 * (uintptr_t)pd <= img_end;
    if (fast) {
        constexpr int kRows = (kBoxH + kNT / 64 - 1) / (kNT / 64);
        const bool m0 = lane < pd, m1 = lane + 64 < pd;
        uint32_t v[kRows][2];
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            const int j = wave + (kNT / 64) * i;
            if (j >= bh) continue;
            const int64_t off = off0 + (int64_t)j * a.src_stride;
            const uint32_t* __restrict__ rowp =
                reinterpret_cast<const uint32_t*>(img + (off - (int64_t)((base + (uintptr_t)off) & 3)));
            v[i][0] = m0 ? rowp[lane] : 0u;
            v[i][1] = m1 ? rowp[lane + 64] : 0u;
        }
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            const int j = wave + (kNT / 64) * i;
            if (j >= bh) continue;
            if (m0) lds[j * pd + lane] = v[i][0];
            if (m1) lds[j * pd + lane + 64] = v[i][1];
        }
    }
    for (int j = fast ? bh : wave; j < bh; j += kNT / 64) {
        const uintptr_t lo = base + (uintptr_t)((int64_t)(by0 + j) * a.src_stride + bx0), hi = lo + (uintptr_t)bw;
        const uintptr_t al = lo & ~(uintptr_t)3;
        const int ndw = (int)((lo & 3) + (uintptr_t)bw + 3) >> 2;  // <= pd
        for (int k = lane; k < ndw; k += 64) {
            const uintptr_t p = al + 4 * (uintptr_t)k;
            uint32_t v = 0;
            if (p >= base && p + 4 <= img_end) {
                v = *reinterpret_cast<const uint32_t*>(img + (intptr_t)(p - base));
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uintptr_t q = p + b;
                    if (q >= lo && q < hi) v |= (uint32_t)img[(intptr_t)(q - base)] << (8 * b);
                }
            }
            lds[j * pd + k] = v;
        }
    }
    __syncthreads();
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(lds);
    const uint32_t a0 = (uint32_t)(base + (uintptr_t)bx0) & 3u, s4 = (uint32_t)a.src_stride & 3u;
    const int x = xb + 4 * (threadIdx.x & 31);
    // the columns' taps: byte offsets in a box row that starts aligned, and the weights
    int c0[4], c1[4];
    uint32_t ax[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = x + k < a.W ? src_pos(x + k, a.Ws, a.W) : bx0 << 5;
        const int ix = q >> 5;
        ax[k] = (uint32_t)q & 31u;
        c0[k] = min(ix - bx0, bw - 1);
        c1[k] = min(min(ix + 1, a.Ws - 1) - bx0, bw - 1);
    }
    uint8_t* __restrict__ dst = a.dst + (int64_t)blockIdx.y * a.dst_pitch;
#pragma unroll
    for (int j = 0; j < kTileH / (kNT / 32); ++j) {
        const int y = yb + (int)(threadIdx.x >> 5) + (kNT / 32) * j;
        if (y >= a.H || x >= a.dst_stride) continue;
        const int q = src_pos(y, a.Hs, a.H);
        const int iy = q >> 5, r0 = min(iy - by0, bh - 1), r1 = min(min(iy + 1, a.Hs - 1) - by0, bh - 1);
        const uint32_t ay = (uint32_t)q & 31u;
        // a box row's first byte sits (its address & 3) bytes into the row's first dword
        const int o0 = r0 * pitch + (int)((a0 + (uint32_t)(by0 + r0) * s4) & 3u);
        const int o1 = r1 * pitch + (int)((a0 + (uint32_t)(by0 + r1) * s4) & 3u);
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t v = blend(lb[o0 + c0[k]], lb[o0 + c1[k]], lb[o1 + c0[k]], lb[o1 + c1[k]], ax[k], ay);
            out |= (x + k < a.W ? v : 0u) << (8 * k);
        }
        // dst_stride is a multiple of 4 and x is: the dword lies inside the row
        *reinterpret_cast<uint32_t*>(dst + (int64_t)y * a.dst_stride + x) = out;
    }
}

constexpr int kMaxLevels = 8;
constexpr int kMergeNT = 512;

struct MergeLevel {
    const yv_keypoint* kp;   // [slot][max_kp]
    const Desc* desc;
    const int32_t* count;    // [slot]
    const uint8_t* bin;      // steering only
    const int32_t* mom;
    int H, W;
};
struct MergeArgs {
    int n_levels, max_kp, steer;
    MergeLevel lv[kMaxLevels];  // lv[0]: the base batch's own arrays, which are the output as well
    yv_keypoint* kp;
    Desc* desc;
    int32_t* kp_count;
    uint8_t* bin;
    int32_t* mom;
    int32_t* count0;  // [slot] level 0's keypoints
    uint8_t* level;   // [slot][max_kp]
    int32_t* level_rc;
};

// One workgroup per image.  Level l's records go to [off_l, off_l + n_l) with off_l the sum of the counts of the levels
// before it, read before the slot's count is rewritten (the barrier).
__global__ __launch_bounds__(kMergeNT) void pyr_merge_kernel(MergeArgs a) {
    const int img = blockIdx.x, tid = threadIdx.x;
    const int64_t slot = (int64_t)img * a.max_kp;
    int n[kMaxLevels], off = 0;
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l) n[l] = l < a.n_levels ? a.lv[l].count[img] : 0;
    __syncthreads();
    const int n0 = min(n[0], a.max_kp);
    for (int i = tid; i < n0; i += kMergeNT) {
        const yv_keypoint k = a.kp[slot + i];
        a.level[slot + i] = 0;
        a.level_rc[2 * (slot + i)] = k.x;
        a.level_rc[2 * (slot + i) + 1] = k.y;
    }
    off = n0;
#pragma unroll
    for (int l = 1; l < kMaxLevels; ++l) {
        if (l >= a.n_levels) break;
        const MergeLevel& L = a.lv[l];
        const int nl = min(n[l], a.max_kp - off);
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(L.kp + slot);
        for (int i = tid; i < nl; i += kMergeNT) {
            uint32_t w[12];
#pragma unroll
            for (int d = 0; d < 12; ++d) w[d] = src[12 * i + d];
            const int xl = (int)w[0], yl = (int)w[1];
            w[0] = (uint32_t)((2 * xl + 1) * a.lv[0].H / (2 * L.H));
            w[1] = (uint32_t)((2 * yl + 1) * a.lv[0].W / (2 * L.W));
            w[2] = (uint32_t)(off + i);
            w[3] &= 0xFFFFFF00u;  // matched = 0 (byte 12; the descriptor starts at byte 13)
            uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(a.kp + slot + off + i);
#pragma unroll
            for (int d = 0; d < 12; ++d) out[d] = w[d];
            a.desc[slot + off + i] = L.desc[slot + i];
            a.level[slot + off + i] = (uint8_t)l;
            a.level_rc[2 * (slot + off + i)] = xl;
            a.level_rc[2 * (slot + off + i) + 1] = yl;
            if (a.steer) {
                a.bin[slot + off + i] = L.bin[slot + i];
                a.mom[2 * (slot + off + i)] = L.mom[2 * (slot + i)];
                a.mom[2 * (slot + off + i) + 1] = L.mom[2 * (slot + i) + 1];
            }
        }
        off += nl;
    }
    if (tid == 0) {
        a.count0[img] = n0;
        a.kp_count[img] = off;
    }
}

// rows of a level image the library allocates: 64-B aligned
inline int level_stride(int W) { return (W + 63) & ~63; }

void launch_level(const uint8_t* src, int n_images, int Hs, int Ws, int src_stride, int64_t src_pitch, uint8_t* dst,
                  int H, int W, int dst_stride, int64_t dst_pitch, hipStream_t s) {
    LevelArgs a;
    a.src = src;
    a.dst = dst;
    a.src_pitch = src_pitch;
    a.dst_pitch = dst_pitch;
    a.src_stride = src_stride;
    a.dst_stride = dst_stride;
    a.Hs = Hs;
    a.Ws = Ws;
    a.H = H;
    a.W = W;
    a.tiles_x = (W + kTileW - 1) / kTileW;
    const unsigned tiles = (unsigned)(a.tiles_x * ((H + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(pyr_level_kernel, dim3(tiles, (unsigned)n_images), dim3(kNT), 0, s, a);
}

}  // namespace pyr

// The argument checks of the pyramid's entry points, in the order the header states: H x W and max_kp are the batch's
// (the host-pointer form: the image's and kMaxKp).
int pyramid_args_check(int H, int W, int max_kp, int n_levels, const int32_t* hw, const int32_t* keep) {
    if (n_levels > pyr::kMaxLevels || !hw || !keep) return YV_ERR_INVALID;
    int64_t total = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int h = hw[2 * l], w = hw[2 * l + 1];
        if (h < 9 || w < 9 || keep[l] < 0) return YV_ERR_INVALID;
        if (l == 0 && (h != H || w != W)) return YV_ERR_INVALID;
        if (l > 0) {
            const int ph = hw[2 * l - 2], pw = hw[2 * l - 1];
            if (h > ph || w > pw || 2 * (int64_t)h < ph || 2 * (int64_t)w < pw) return YV_ERR_INVALID;
        }
        total += keep[l];
    }
    if (total > max_kp) return YV_ERR_CAPACITY;
    for (int l = 0; l < n_levels; ++l)
        if (hw[2 * l + 1] > kMaxWidth || hw[2 * l] > kBandRows * kMaxBands) return YV_ERR_CAPACITY;
    return YV_OK;
}

namespace {

void pyramid_release(yv_batch* b) {
    for (int l = 0; l < pyr::kMaxLevels; ++l) {
        if (b->pyr[l].ws) batch_free(b->pyr[l].ws);
        b->pyr[l] = yv_batch::PyrLevel{};
    }
    b->pyr_levels = 0;
}

}  // namespace

void pyramid_free(yv_batch* b) { pyramid_release(b); }

int pyramid_prepare(yv_batch* b) {
    const bool steer = steer_on(b->ctx);
    for (int l = 1; l < b->pyr_levels; ++l) {
        yv_batch* w = b->pyr[l].ws;
        const int sel = prepare_select(w, w->H, w->W);
        if (sel != YV_OK) return sel;
        if (steer && ensure_steer(w) != YV_OK) return YV_ERR_HIP;
    }
    return YV_OK;
}

int pyramid_carry(yv_batch* b, size_t from, hipStream_t s) {
    const size_t nk = (size_t)b->max_kp, dst = (size_t)b->max_images;
    YV_HIP(hipMemcpyAsync(b->pyr_level + dst * nk, b->pyr_level + from * nk, nk, hipMemcpyDeviceToDevice, s));
    YV_HIP(hipMemcpyAsync(b->pyr_rc + dst * nk * 2, b->pyr_rc + from * nk * 2, nk * 2 * sizeof(int32_t),
                          hipMemcpyDeviceToDevice, s));
    YV_HIP(hipMemcpyAsync(b->pyr_count0 + dst, b->pyr_count0 + from, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return YV_OK;
}

void pyramid_detect(yv_batch* b, const uint8_t* d_images, int n_images, int stride, int64_t image_pitch,
                    hipStream_t s) {
    const yv_ctx* ctx = b->ctx;
    const uint8_t* src = d_images;
    int Hs = b->H, Ws = b->W, ss = stride;
    int64_t sp = image_pitch;
    for (int l = 1; l < b->pyr_levels; ++l) {
        const yv_batch::PyrLevel& L = b->pyr[l];
        yv_batch* w = L.ws;
        const int64_t pitch = (int64_t)L.stride * L.H;
        pyr::launch_level(src, n_images, Hs, Ws, ss, sp, L.img, L.H, L.W, L.stride, pitch, s);
        launch_detect_blur(L.img, n_images, L.H, L.W, L.stride, pitch, ctx->fast_thr, ctx->harris_eigen, w->cand_keys,
                           w->cap, w->cand_count, ctx->k9, w->blur, s);
        src = L.img;
        Hs = L.H;
        Ws = L.W;
        ss = L.stride;
        sp = pitch;
    }
}

void pyramid_topk(yv_batch* b, int n_images, hipStream_t s) {
    for (int l = 1; l < b->pyr_levels; ++l)
        launch_select_topk(b->pyr[l].ws, n_images, std::min(b->ctx->max_corners, b->pyr[l].keep), s);
}

void pyramid_describe_merge(yv_batch* b, int n_images, hipStream_t s) {
    yv_ctx* ctx = b->ctx;
    pyr::MergeArgs a{};
    a.n_levels = b->pyr_levels;
    a.max_kp = b->max_kp;
    a.steer = steer_on(ctx) ? 1 : 0;
    a.lv[0] = {b->keypoints, b->desc, b->kp_count, b->steer_bin, b->steer_mom, b->H, b->W};
    for (int l = 1; l < b->pyr_levels; ++l) {
        yv_batch* w = b->pyr[l].ws;
        launch_describe(w, n_images, brief_workers(ctx, w->W), s);
        a.lv[l] = {w->keypoints, w->desc, w->kp_count, w->steer_bin, w->steer_mom, w->H, w->W};
    }
    a.kp = b->keypoints;
    a.desc = b->desc;
    a.kp_count = b->kp_count;
    a.bin = b->steer_bin;
    a.mom = b->steer_mom;
    a.count0 = b->pyr_count0;
    a.level = b->pyr_level;
    a.level_rc = b->pyr_rc;
    hipLaunchKernelGGL(pyr::pyr_merge_kernel, dim3((unsigned)n_images), dim3(pyr::kMergeNT), 0, s, a);
}

}  // namespace yavo

using namespace yavo;

extern "C" {

int yv_batch_set_pyramid(yv_batch* b, int n_levels, const int32_t* level_hw, const int32_t* level_keep) {
    if (n_levels <= 1) {
        if (!b) return YV_ERR_INVALID;
        b->pyr_on = false;
        return YV_OK;
    }
    // without a batch, what can be checked without one
    int st = pyramid_args_check(b ? b->H : (level_hw ? level_hw[0] : 0), b ? b->W : (level_hw ? level_hw[1] : 0),
                                b ? b->max_kp : kMaxKp, n_levels, level_hw, level_keep);
    if (st != YV_OK) return st;
    if (!b) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    // a run in flight, on any stream, uses the level workspaces
    YV_HIP(hipDeviceSynchronize());
    b->pyr_on = false;
    if (!b->pyr_level) {
        const size_t n = (size_t)b->nslots * (size_t)b->max_kp;
        int rc = YV_OK;
        rc |= b->mem.alloc(&b->pyr_level, n);
        rc |= b->mem.alloc(&b->pyr_rc, 2 * n);
        rc |= b->mem.alloc(&b->pyr_count0, (size_t)b->nslots);
        if (rc != YV_OK) {  // a retry starts clean
            b->mem.release(b->pyr_level, b->pyr_rc, b->pyr_count0);
            return YV_ERR_HIP;
        }
        YV_HIP(hipMemset(b->pyr_level, 0, n));
        YV_HIP(hipMemset(b->pyr_rc, 0, 2 * n * sizeof(int32_t)));
        YV_HIP(hipMemset(b->pyr_count0, 0, (size_t)b->nslots * sizeof(int32_t)));
    }
    bool same = b->pyr_levels == n_levels;
    for (int l = 0; same && l < n_levels; ++l)
        same = b->pyr[l].H == level_hw[2 * l] && b->pyr[l].W == level_hw[2 * l + 1];
    if (!same) {
        pyramid_release(b);
        for (int l = 0; l < n_levels; ++l) {
            yv_batch::PyrLevel& L = b->pyr[l];
            L.H = level_hw[2 * l];
            L.W = level_hw[2 * l + 1];
            if (l == 0) continue;
            L.stride = pyr::level_stride(L.W);
            st = yv_batch_create(b->ctx, b->max_images, L.H, L.W, b->max_kp, 0, &L.ws);
            if (st == YV_OK && L.ws->mem.alloc(&L.img, (size_t)b->max_images * (size_t)L.stride * (size_t)L.H) != YV_OK)
                st = YV_ERR_HIP;
            if (st != YV_OK) {
                pyramid_release(b);
                return st;
            }
        }
        b->pyr_levels = n_levels;
    }
    for (int l = 0; l < n_levels; ++l) b->pyr[l].keep = level_keep[l];
    b->pyr_on = true;
    return YV_OK;
}

int yv_batch_pyramid_view_get(yv_batch* b, yv_batch_pyramid_view* v) {
    if (!b || !v || !b->pyr_level || b->pyr_levels < 2) return YV_ERR_INVALID;
    std::memset(v, 0, sizeof(*v));
    v->n_levels = b->pyr_levels;
    v->level = b->pyr_level;
    v->level_rc = b->pyr_rc;
    for (int l = 0; l < b->pyr_levels; ++l) {
        const yv_batch::PyrLevel& L = b->pyr[l];
        const yv_batch* w = l ? L.ws : b;
        v->H[l] = L.H;
        v->W[l] = L.W;
        v->keep[l] = L.keep;
        v->image[l] = L.img;  // level 0: NULL, the run's own images
        v->stride[l] = L.stride;
        v->pitch[l] = (int64_t)L.stride * L.H;
        v->kp_count[l] = l ? w->kp_count : b->pyr_count0;
        v->det_count[l] = w->det_count;
        v->keypoints[l] = w->keypoints;
    }
    return YV_OK;
}

int yv_pyramid_image(yv_ctx* ctx, const uint8_t* src, int src_H, int src_W, int src_stride, int dst_H, int dst_W,
                     uint8_t* dst, int dst_stride) {
    if (!src || !dst || dst_H < 1 || dst_W < 1 || src_H > 8192 || src_W > 8192 || dst_H > src_H || dst_W > src_W ||
        2 * dst_H < src_H || 2 * dst_W < src_W || src_stride < src_W || dst_stride < dst_W)
        return YV_ERR_INVALID;
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    HipOwned mem;
    uint8_t *d_s = nullptr, *d_d = nullptr;
    const int ds = pyr::level_stride(dst_W);
    // the source as the caller holds it, stride and all: the kernel's reads are bounded by the rows, not the stride
    const size_t src_bytes = (size_t)src_stride * (size_t)(src_H - 1) + (size_t)src_W;
    if (mem.alloc(&d_s, src_bytes) != YV_OK || mem.alloc(&d_d, (size_t)ds * dst_H) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipMemcpy(d_s, src, src_bytes, hipMemcpyHostToDevice));
    pyr::launch_level(d_s, 1, src_H, src_W, src_stride, 0, d_d, dst_H, dst_W, ds, 0, ctx->stream);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipStreamSynchronize(ctx->stream));
    // the destination's rows only: the bytes between them stay the caller's
    YV_HIP(hipMemcpy2D(dst, (size_t)dst_stride, d_d, (size_t)ds, (size_t)dst_W, (size_t)dst_H, hipMemcpyDeviceToHost));
    return YV_OK;
}

int yv_detect_describe_pyramid(yv_ctx* ctx, const uint8_t* img, int H, int W, int stride, int n_levels,
                               const int32_t* level_hw, const int32_t* level_keep, yv_keypoint* out, uint8_t* level,
                               int32_t* level_rc, int* n_out) {
    if (!img || !n_out || n_levels < 1 || H < 9 || W < 9 || stride < W) return YV_ERR_INVALID;
    int st = pyramid_args_check(H, W, kMaxKp, n_levels, level_hw, level_keep);
    if (st != YV_OK) return st;
    int total = 0;
    for (int l = 0; l < n_levels; ++l) total += level_keep[l];
    if (total > 0 && (!out || !level || !level_rc)) return YV_ERR_INVALID;
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    *n_out = 0;
    if (total == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    yv_batch* b = nullptr;
    st = yv_batch_create(ctx, 1, H, W, total, 0, &b);
    if (st != YV_OK) return st;
    const auto body = [&]() -> int {
        int rc = yv_batch_set_pyramid(b, n_levels, level_hw, level_keep);
        if (rc != YV_OK) return rc;
        YV_HIP(hipMemcpy2D(b->staging, (size_t)W, img, (size_t)stride, (size_t)W, (size_t)H, hipMemcpyHostToDevice));
        rc = yv_batch_run(b, b->staging, 1, W, (int64_t)H * W, 0, -1, nullptr);
        if (rc != YV_OK) return rc;
        YV_HIP(hipStreamSynchronize(ctx->stream));
        int32_t n = 0;
        YV_HIP(hipMemcpy(&n, b->kp_count, sizeof(n), hipMemcpyDeviceToHost));
        n = std::min(std::max(n, 0), total);
        if (n > 0) {
            YV_HIP(hipMemcpy(out, b->keypoints, sizeof(yv_keypoint) * (size_t)n, hipMemcpyDeviceToHost));
            if (b->pyr_on) {
                YV_HIP(hipMemcpy(level, b->pyr_level, (size_t)n, hipMemcpyDeviceToHost));
                YV_HIP(hipMemcpy(level_rc, b->pyr_rc, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost));
            } else {  // one level: every keypoint is level 0's, at its own position
                for (int i = 0; i < n; ++i) {
                    level[i] = 0;
                    level_rc[2 * i] = out[i].x;
                    level_rc[2 * i + 1] = out[i].y;
                }
            }
        }
        *n_out = n;
        return YV_OK;
    };
    st = body();
    yv_batch_destroy(b);
    return st;
}

}  // extern "C"
