// yavo_brief.hip -- BRIEF descriptors and KeyPoint records of the kept keypoints, band by band.
//
// Reference functions restated (the reference's file:line):
//   brief_kernel        Brief::computeBrief                     src/BriefDescriptor.cc:86-124
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "yavo_internal.h"
#include "yavo_wave.h"

namespace yavo {

// ------------------------------------------------------------------------------------------------
// BRIEF
// ------------------------------------------------------------------------------------------------

// Persistent workers over the (32-row band, image) items: a band's keypoints (rows [r0, r0 + 32)) read their 17 x 17
// patches from an LDS copy of the blurred rows [r0 - 8, r0 + 41) with row stride LS = brief_lds_stride(W) >= W + 1.
// The reference samples getPixelVal at the linear index (row + dr) * W + (col + dc) (src/BriefDescriptor.cc:
// 100-118, src/Image.cc:15-17).  checkBoundry keeps 8 <= row <= H - 8 and 8 <= col <= W - 8, and |dr|, |dc| <= 8
// (yv_set_brief_offsets), so a sample is pixel (row + dr, col + dc) except (a) col + dc == W, which wraps to the
// first pixel of the next row, and (b) any index past the image end (row + dr == H, or row + dr == H - 1 at
// col + dc == W), which the reference reads out of bounds (UB; both paths read 0).  The band therefore holds in
// LDS column W of each row the next row's first pixel, and zero rows past the image: every sample is then
// s_band[(row + dr - (r0 - 8)) * LS + col + dc] with no test.  Lanes = keypoints: a wave takes 64 keypoints and
// one quarter (64) of the tests, whose sample offsets are wave-uniform scalars (loff).
constexpr int BR_BAND = kBandRows;
constexpr int BR_ROWS = BR_BAND + 17;  // rows r0-8 .. r0+40 (the last one for the wrap of col + 8 == W)
// 16 waves share one staged band: the ~61 KB band limits a CU to 2 workgroups, so the workgroup is as wide as
// the 64-VGPR budget of 8 waves per SIMD allows
constexpr int BR_NT = 1024;
constexpr int BR_NW = BR_NT / 64;
// the band's keypoint records are loaded as 4 per thread (kq below): a band may hold every keypoint of the image.
// (A loop over any further records would lift this bound but takes the kernel from 46 to 64 VGPRs, and at <= 48 one
// BRIEF wave per SIMD still fits beside the side stream's two pose-LM waves: 2 x 232 of 512.)
static_assert(4 * BR_NT >= kMaxKp, "brief_kernel loads at most 4 * BR_NT band records");

// The band queue.  The items (logical blocks lb = image * bands + band) are cut into eight contiguous ranges, the ones
// xcd_swizzle gives the eight XCD labels: label x owns [first, first + len).  heads[x] counts the items taken from
// range x.  A worker takes from its own label's range (neighbouring bands, and their 17 shared rows, meet in one L2)
// and, once that is exhausted, from the next labels' ranges in turn; -1 when every head has failed.  `at` (0 .. 7) is
// the number of ranges this worker has found exhausted: a head only grows, so they stay exhausted.  One returning
// atomic per item, no waiting on another workgroup.
__device__ __forceinline__ int brief_take(int32_t* heads, int label, int total, int& at) {
    const int q = total >> 3, r = total & 7;
    while (at < kBriefHeads) {
        const int x = (label + at) & 7;
        const int len = q + (x < r ? 1 : 0);
        if (len > 0) {
            const int v = atomicAdd(&heads[x], 1);
            if (v < len) return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + v;
        }
        ++at;
    }
    return -1;
}

#ifdef YAVO_LM_PROFILE
constexpr int kBriefProfSlots = 16384;
__device__ unsigned long long g_brief_prof[kBriefProfSlots][6];
// brief_kernel, per worker (lane 0): cycles summed over its bands in [0] staging (boundary barrier to staged band),
// [1] descriptors, and in the high half of [5] the hand-over (the wave's last descriptor store to the boundary
// barrier passed, with the first dequeue); [2], [3] the worker's life in s_memrealtime ticks; the low halves of [4],
// [5] its HW_ID / XCC_ID, the high half of [4] the bands it took (0 in a build of the one-band-per-workgroup revision,
// whose slots tools/brief_profile.py still reads)
#define BP_DECL unsigned long long bp_acc[3] = {0, 0, 0}; unsigned long long bp_t = __builtin_readcyclecounter(); \
    unsigned long long bp_bands = 0; const unsigned long long bp_rt0 = __builtin_amdgcn_s_memrealtime();
#define BP_MARK(k) do { const unsigned long long t_ = __builtin_readcyclecounter(); bp_acc[k] += t_ - bp_t; bp_t = t_; } while (0)
#define BP_BAND() do { ++bp_bands; } while (0)
#define BP_STORE() do { \
        if (threadIdx.x == 0 && blockIdx.x < kBriefProfSlots) { \
            g_brief_prof[blockIdx.x][0] = bp_acc[0]; g_brief_prof[blockIdx.x][1] = bp_acc[1]; \
            g_brief_prof[blockIdx.x][2] = bp_rt0; \
            g_brief_prof[blockIdx.x][3] = __builtin_amdgcn_s_memrealtime(); \
            g_brief_prof[blockIdx.x][4] = (unsigned long long)__builtin_amdgcn_s_getreg(0xF804) | (bp_bands << 32); \
            g_brief_prof[blockIdx.x][5] = (unsigned long long)__builtin_amdgcn_s_getreg(0xF814) | (bp_acc[2] << 32); \
        } \
    } while (0)
#else
#define BP_DECL
#define BP_MARK(k) do {} while (0)
#define BP_BAND() do {} while (0)
#define BP_STORE() do {} while (0)
#endif

// amdgpu_waves_per_eu(8, 8): two 16-wave workers on a CU are 8 waves per SIMD, which the SIMD's 800 scalar registers
// allow only up to 96 per wave.  The band loop's scalars took 104: every CU then ran its two workers one after the other
// (tools/brief_profile.py: 1.00 resident, BRIEF alone 1.55 ms against the one-band workgroups' 1.38).  With the bound
// the compiler keeps 78 and moves 21 into lanes of one VGPR, once per band.
__global__ __launch_bounds__(BR_NT) __attribute__((amdgpu_waves_per_eu(8, 8))) void brief_kernel(
                                                    const uint8_t* __restrict__ blur, int H, int W,
                                                    const int32_t* __restrict__ kp_src,
                                                    const int32_t* __restrict__ kp_band,
                                                    const int32_t* __restrict__ band_off, int max_kp,
                                                    yv_keypoint* __restrict__ keypoints, Desc* __restrict__ desc,
                                                    const int2* __restrict__ loff, int32_t* __restrict__ heads,
                                                    int total) {
    // All of the workgroup's LDS is dynamic, from a 16-B aligned base: static __shared__ variables would precede the
    // dynamic region unpadded (16,388 B of them put the band at 4 mod 16), and the band's 16-B LDS-DMA and zero-word
    // stores then run off their natural alignment.  Layout: the band (BR_ROWS * LS bytes, LS a multiple of 16), this
    // band's keypoints packed (index << 16) | (col << 5) | (row - r0) (index < 4096, col < 2048, 32-row band), the
    // next item {lb, lo, count} (brief_lds_bytes sizes the region).
    extern __shared__ __attribute__((aligned(16))) uint8_t s_band[];
    uint32_t* s_list = reinterpret_cast<uint32_t*>(s_band + BR_ROWS * brief_lds_stride(W));
    int* s_next = reinterpret_cast<int*>(s_list + kMaxKp);
    BP_DECL
    const int nbands = (H + BR_BAND - 1) / BR_BAND;
    const int tid = threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int label = (int)blockIdx.x & 7;
    // What does not depend on the band.  A band is rows rb .. rb + BR_ROWS - 1 (rb = r0 - 8) of the pitched blurred
    // image as 16-B words, LS bytes per row (LS <= the pitch: inside the row); column W of row r is patched with pixel
    // (r + 1, 0) (0 past the image), rows outside [0, H) are zero.  The first 4 x BR_NT words come by LDS-DMA, word
    // k = tid + u BR_NT = (band row j, 16-B column q) by this thread: pk[u] = the word's byte offset from the band's
    // first row in the image (17 bits) | j << 17 | (q holds column W) << 23 | (k < nw) << 24.
    const int bp = blur_pitch(W), LS = brief_lds_stride(W);
    const int wpr = LS >> 4;              // 16-B words per LDS row
    const int nw = BR_ROWS * wpr;
    const int kw_fix = W >> 4;
    uint4* s4 = reinterpret_cast<uint4*>(s_band);
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    uint32_t pk[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = tid + u * BR_NT;
        const int j = k / wpr, q = k - j * wpr;
        pk[u] = k < nw ? (uint32_t)(j * bp + 16 * q) | ((uint32_t)j << 17) | (q == kw_fix ? 1u << 23 : 0u) | (1u << 24)
                       : 0u;
    }
    // The next item is fetched a band ahead by lane 0 of the last wave (the one with the fewest descriptor items): the
    // dequeue and the item's band_off pair, left in s_next for everyone to read after the band's closing barrier.
    // s_next is read between that barrier and the staging barrier and written after the staging barrier only.
    auto fetch_next = [&]() {
        int at = s_next[3];  // the exhausted ranges so far, kept in LDS: one lane's value, no register across the loop
        const int nl = brief_take(heads, label, total, at);
        s_next[3] = at;
        int nlo = 0, nn = 0;
        if (nl >= 0) {
            const int ni = nl / nbands;
            const int32_t* bo = band_off + (int64_t)ni * (kMaxBands + 1) + (nl - ni * nbands);
            nlo = bo[0];
            nn = bo[1] - nlo;
        }
        s_next[0] = nl;
        s_next[1] = nlo;
        s_next[2] = nn;
    };
    if (tid == BR_NT - 64) {
        s_next[3] = 0;
        fetch_next();
    }
    __syncthreads();
    int lb = __builtin_amdgcn_readfirstlane(s_next[0]);
    int klo = __builtin_amdgcn_readfirstlane(s_next[1]);
    int nbk = __builtin_amdgcn_readfirstlane(s_next[2]);
    BP_MARK(2);
    while (lb >= 0) {
        // (the thread index and the packed words are opaque here: otherwise every value derived from them is kept in
        // a register of its own across the loop, 59 VGPRs where the budget beside the pose LM is 40)
        int t = tid;
        asm volatile("" : "+v"(t), "+v"(pk[0]), "+v"(pk[1]), "+v"(pk[2]), "+v"(pk[3]));
        const int img = lb / nbands;
        const int band = lb - img * nbands;
        const int r0 = band * BR_BAND, rb = r0 - 8;
        const int4* src = reinterpret_cast<const int4*>(kp_src) + (int64_t)img * max_kp;
        // An empty band (known a band ahead) stages nothing: the LDS keeps an earlier band's pixels, zero rows,
        // column-W bytes and list, and the next band with keypoints rewrites every word of the band and its own list
        // entries below.
        if (nbk > 0) {
            // this band's keypoints, bucketed by top-K (kp_band {row, col, id, slot}, band_off): its own ~K / bands
            // records, not the image's whole list.
            // Every global load of the band is issued at once after the closing barrier of the band before: the
            // band's keypoint records (<= 4096 = 4 per thread), then the band itself by LDS-DMA
            // (global_load_lds_dwordx4: word k of the band lands at s4[k] with no VGPR destination; the LDS address
            // is the wave's base + 16 x lane, and word k = tid + u BR_NT is lane-linear).  Staging the band through
            // registers held 16 VGPRs per thread across the loads: the kernel took 46, and beside two pose-LM waves
            // on a SIMD (2 x 168 of 512 registers) a 16-wave BRIEF workgroup fits only at <= 40.
            // the zero words first: an LDS store issued while LDS-DMA loads are in flight waits for them all (and
            // before the record loads, from a zero made here: its four registers are then free again)
            uint32_t z = 0u;
            asm volatile("" : "+v"(z));
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = rb + (int)((pk[u] >> 17) & 63u);
                if ((pk[u] >> 24) != 0u && (r < 0 || r >= H)) s4[t + u * BR_NT] = make_uint4(z, z, z, z);
            }
            const int4* kb = reinterpret_cast<const int4*>(kp_band) + (int64_t)img * max_kp + klo;
            int4 kq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = u * BR_NT + t;
                kq[u] = kb[j < nbk ? j : 0];
            }
            const uint8_t* b = blur + (int64_t)img * H * bp;
            const int64_t boff = (int64_t)rb * bp;
            uint32_t nx[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = rb + (int)((pk[u] >> 17) & 63u);
                nx[u] = 0u;
                if ((pk[u] >> 24) != 0u && r >= 0 && r < H) {
                    __builtin_amdgcn_global_load_lds(b + (boff + (int64_t)(pk[u] & 0x1FFFFu)),
                                                     (lds_ptr_t)(s4 + (t & ~63) + u * BR_NT), 16, 0, 0);
                    if ((pk[u] & (1u << 23)) != 0u && r + 1 < H) nx[u] = (uint32_t)b[(int64_t)(r + 1) * bp];
                }
            }
            // every load is in flight: one wait for all of them (consumed earlier, the records were waited for one
            // by one)
            __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
            for (int u = 0; u < 4; ++u) asm volatile("" : "+v"(kq[u].x), "+v"(kq[u].y), "+v"(kq[u].w), "+v"(nx[u]));
            // 1. this band's keypoints (any order: each keypoint's outputs go to its own slot)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = u * BR_NT + t;
                if (j < nbk)
                    s_list[j] = ((uint32_t)kq[u].w << 16) | ((uint32_t)kq[u].y << 5) | (uint32_t)(kq[u].x - r0);
            }
            // 2. column W of each row: the byte after the row's last pixel takes the next row's first pixel, written
            // by the lane whose LDS-DMA word holds it, after its own loads have landed
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = rb + (int)((pk[u] >> 17) & 63u);
                if ((pk[u] >> 24) != 0u && (pk[u] & (1u << 23)) != 0u && r >= 0 && r < H)
                    s_band[16 * (t + u * BR_NT) + (W & 15)] = (uint8_t)nx[u];
            }
            // wide images (W > 1320): the rest of the band, word by word through registers
            const int sh_fix = 8 * (W & 3), dw_fix = (W >> 2) & 3;
            int wprw = wpr;  // (opaque: the division's reciprocal is formed here, not held across the band loop)
            asm volatile("" : "+s"(wprw));
            for (int k = t + 4 * BR_NT; k < nw; k += BR_NT) {
                const int j = k / wprw, q = k - j * wprw;
                const int r = rb + j;
                uint4 w = make_uint4(0, 0, 0, 0);
                if (r >= 0 && r < H) {
                    w = reinterpret_cast<const uint4*>(b + (int64_t)r * bp)[q];
                    if (q == kw_fix) {
                        const uint32_t nxx = r + 1 < H ? (uint32_t)b[(int64_t)(r + 1) * bp] : 0u;
                        const uint32_t m = ~(0xFFu << sh_fix);
                        if (dw_fix == 0) w.x = (w.x & m) | (nxx << sh_fix);
                        else if (dw_fix == 1) w.y = (w.y & m) | (nxx << sh_fix);
                        else if (dw_fix == 2) w.z = (w.z & m) | (nxx << sh_fix);
                        else w.w = (w.w & m) | (nxx << sh_fix);
                    }
                }
                s4[k] = w;
            }
        }
        __syncthreads();
        BP_MARK(0);
        BP_BAND();
        // the next item's dequeue and band_off pair travel while this band's descriptors are computed
        if (tid == BR_NT - 64) fetch_next();
        const int nb = nbk;
        if (nb > 0) {
            int ln = lane;
            asm volatile("" : "+v"(ln));
            // 3. descriptors, lanes = keypoints: wave item = (block of 64 keypoints, group g of 64 tests).  The tests'
            // offsets are wave-uniform (loff, scalar loads), so a test costs each lane two LDS byte reads, two address adds,
            // a subtraction and one v_alignbit that shifts the result bit in: 4 VALU per test and keypoint, against ~110
            // VALU of per-keypoint ballot / emit work per wave in the lanes = tests form.
            uint8_t* rec_b = reinterpret_cast<uint8_t*>(keypoints + (int64_t)img * max_kp);
            Desc* d_base = desc + (int64_t)img * max_kp;
            // s_list is grouped by the bank of the patch centre (boundary_compact's classes, ~G entries each): lane kd of the
            // dealt order takes entry (kd % 32) * G + kd / 32, so the 32 lanes of a group take entries G apart, about one per
            // class -- distinct banks for every test's uniform offset, up to a carry -- where neighbouring entries share one
            const int G = (nb + 31) >> 5;
            const int nitems = ((32 * G + 63) >> 6) * 4;
            // the item index in an SGPR (wave: readfirstlane above): loff then comes by scalar loads
            for (int item = wave; item < nitems; item += BR_NW) {
                const int g = item & 3, kd = (item >> 2) * 64 + ln;
                const int k = (kd & 31) * G + (kd >> 5);
                const bool act = (kd >> 5) < G && k < nb;
                const uint32_t e = s_list[act ? k : nb - 1];
                const int i = (int)(e >> 16), row = r0 + (int)(e & 31u), col = (int)((e >> 5) & 2047u);
                const int id = (act && g == 0) ? src[i].z : 0;
                const int la = (row - rb) * LS + col;
                const int2* lo = loff + 64 * g;
                uint32_t w[2] = {0u, 0u};
                // tests 64g + 63 down to 64g: w[h] = (w[h] << 1) | (p1 > p2), so bit j of w[h] is test 64g + 32h + j; eight
                // tests (16 LDS reads in flight) per iteration keep the lane within the 64 VGPRs of 8 waves per SIMD
#pragma unroll 1
                for (int c = 7; c >= 0; --c) {
                    const int2* oc = lo + 8 * c;
                    uint32_t acc = w[c >> 2];
#pragma unroll
                    for (int j = 7; j >= 0; --j) {
                        const int2 o = oc[j];
                        const uint32_t p1 = s_band[la + o.x], p2 = s_band[la + o.y];
                        acc = __builtin_amdgcn_alignbit(acc, p2 - p1, 31);  // p2 - p1 < 0 iff p1 > p2
                    }
                    if (c >= 4) w[1] = acc;
                    else w[0] = acc;
                }
                if (act) {
                    reinterpret_cast<uint2*>(d_base + i)[g] = make_uint2(w[0], w[1]);
                    // the 48-B record {row, col, id, matched = 0, featVec[32], 3 pad bytes}: featVec bytes 8g .. 8g + 7 at
                    // record byte 13 + 8g (byte, short, dword, byte: the natural alignments of 13 + 8g ...)
                    uint8_t* r = rec_b + (int64_t)i * 48;
                    if (g == 0) {
                        reinterpret_cast<int32_t*>(r)[0] = row;
                        reinterpret_cast<int32_t*>(r)[1] = col;
                        reinterpret_cast<int32_t*>(r)[2] = id;
                        r[12] = 0;
                    }
                    r[13 + 8 * g] = (uint8_t)w[0];
                    *reinterpret_cast<uint16_t*>(r + 14 + 8 * g) = (uint16_t)(w[0] >> 8);
                    *reinterpret_cast<uint32_t*>(r + 16 + 8 * g) = (w[0] >> 24) | (w[1] << 8);
                    r[20 + 8 * g] = (uint8_t)(w[1] >> 24);
                    if (g == 3) {
                        r[45] = 0;
                        *reinterpret_cast<uint16_t*>(r + 46) = 0;
                    }
                }
                // (id's load counts as consumed on every path: otherwise the closing barrier's LDS read, which may reuse
                // its register, waits for every outstanding store of the wave as well)
                asm volatile("" ::"v"(id));
            }
        }
        BP_MARK(1);
        // the band's closing barrier: every wave is done reading the band and the list, and s_next is written.  It
        // orders LDS accesses only (__syncthreads() would also wait for this band's descriptor and record stores to
        // complete, ~2 us that the one-band workgroup never waited: they drain while the next band's loads travel)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        lb = __builtin_amdgcn_readfirstlane(s_next[0]);
        klo = __builtin_amdgcn_readfirstlane(s_next[1]);
        nbk = __builtin_amdgcn_readfirstlane(s_next[2]);
        BP_MARK(2);
    }
    BP_STORE();
}

// the 256 tests' sample offsets in the band's LDS layout: loff[t] = {dr1 * LS + dc1, dr2 * LS + dc2}
__global__ void brief_loff_kernel(const int8_t* __restrict__ offsets, int LS, int2* __restrict__ loff) {
    const int t = threadIdx.x;
    const int8_t* o = offsets + 4 * t;
    loff[t] = make_int2((int)o[0] * LS + (int)o[1], (int)o[2] * LS + (int)o[3]);
}

void launch_brief(const uint8_t* blur, int n_images, int H, int W, const int8_t* offsets, const int32_t* kp_src,
                  const int32_t* kp_band, const int32_t* band_off, int max_kp, yv_keypoint* keypoints, Desc* desc,
                  int32_t* loff, bool new_loff, int32_t* heads, int max_workers, hipStream_t s) {
    const int total = ((H + BR_BAND - 1) / BR_BAND) * n_images;
    dim3 grid(std::max(1, std::min(max_workers, total)));
    const size_t lds = brief_lds_bytes(W);
    int2* lo = reinterpret_cast<int2*>(loff);
    if (new_loff) hipLaunchKernelGGL(brief_loff_kernel, dim3(1), dim3(256), 0, s, offsets, brief_lds_stride(W), lo);
    hipLaunchKernelGGL(brief_kernel, grid, dim3(BR_NT), lds, s, blur, H, W, kp_src, kp_band, band_off, max_kp,
                       keypoints, desc, lo, heads, total);
}

__global__ void pack_desc_kernel(const yv_keypoint* __restrict__ keypoints, const int32_t* __restrict__ kp_count,
                                 int max_kp, Desc* __restrict__ desc) {
    const int slot = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kp_count[slot] || i >= max_kp) return;
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(keypoints + (int64_t)slot * max_kp + i);
    Desc d;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        d.w[q] = (uint32_t)rec[13 + 4 * q] | ((uint32_t)rec[14 + 4 * q] << 8) | ((uint32_t)rec[15 + 4 * q] << 16) |
                 ((uint32_t)rec[16 + 4 * q] << 24);
    }
    desc[(int64_t)slot * max_kp + i] = d;
}

void launch_pack_desc(const yv_keypoint* keypoints, const int32_t* kp_count, int n_slots, int max_kp, Desc* desc,
                      hipStream_t s) {
    dim3 grid((max_kp + 255) / 256, n_slots);
    hipLaunchKernelGGL(pack_desc_kernel, grid, dim3(256), 0, s, keypoints, kp_count, max_kp, desc);
}

}  // namespace yavo

#ifdef YAVO_LM_PROFILE
extern "C" int yv_debug_brief_prof(unsigned long long* out /* [16384][6] */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yavo::g_brief_prof), sizeof(unsigned long long) * 16384 * 6) ==
                   hipSuccess ? 0 : -2;
}
#endif
