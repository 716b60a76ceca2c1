// yavo_detect.hip -- gfx950 (CDNA4) kernels of the detect stage: FAST-12 + Harris, and the 9x9 blur fused into the same
// tile on the int8 matrix cores or on its own.
//
// Built with -ffp-contract=off: the Harris eigen solve and response must round operation-for-operation
// like the reference's x86-64 build (no FMA contraction), see DESIGN.md "Float parity".
//
// Reference functions restated (the reference's file:line):
//   detect_kernel       FastDetector::getFastFeatures loop      src/FastDetector.cc:298-335
//                       checkInBetween / checkContiguousPixels  src/FastDetector.cc:135-161
//                       preComputeHarris + Harris response      src/FastDetector.cc:164-214, 244-273
//   blur9_kernel        cv::GaussianBlur(9x9, 2.5) call         src/BriefDescriptor.cc:90
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yavo_internal.h"
#include "yavo_wave.h"

namespace yavo {

// ------------------------------------------------------------------------------------------------
// FAST-12 + Harris
// ------------------------------------------------------------------------------------------------
// Ring order of FastDetector::getBresenhamCirclePoints (src/FastDetector.cc:50-112) as (drow, dcol);
// pinned by tests/test_oracle_fast.py against the reference's testBresenham.png fixture.
#define YV_RING_DR {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1}
#define YV_RING_DC {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3}

// OpenCV lapack.cpp hypot<float>: a*sqrt(1+(b/a)^2) (used by JacobiImpl_).
__device__ __forceinline__ float cv_hypotf(float a, float b) {
    a = fabsf(a);
    b = fabsf(b);
    if (a > b) {
        b /= a;
        return a * sqrtf(1.0f + b * b);
    }
    if (b > 0.0f) {
        a /= b;
        return b * sqrtf(1.0f + a * a);
    }
    return 0.0f;
}

// cv::eigen in an OpenCV built with HAVE_EIGEN: Eigen 3.4 SelfAdjointEigenSolver<MatrixXf> on the 2x2 (oracle
// or_eigen_selfadjoint2_f32 states the derivation): scale by the largest |entry|, implicit Wilkinson-shift QR steps
// until (e / FLT_EPSILON)^2 <= |d0| + |d1| (or |e| < FLT_MIN), at most 60; ascending sort, scale back.  Returns
// (w0 >= w1).  Every float operation in the oracle's order (-ffp-contract=off, IEEE div / sqrt).
__device__ __forceinline__ float eig_hypotf(float x, float y) {
    x = fabsf(x);
    y = fabsf(y);
    if (isinf(x) || isinf(y)) return __builtin_inff();
    if (isnan(x) || isnan(y)) return __builtin_nanf("");
    const float p = x > y ? x : y;
    if (p == 0.0f) return 0.0f;
    const float qp = (y < x ? y : x) / p;
    return p * sqrtf(1.0f + qp * qp);
}

__device__ void eig_selfadjoint2(float m00, float m01, float m11, float& w0, float& w1) {
    float scale = fabsf(m00);
    if (fabsf(m01) > scale) scale = fabsf(m01);
    if (fabsf(m11) > scale) scale = fabsf(m11);
    if (scale == 0.0f) scale = 1.0f;
    float d0 = m00 / scale, d1 = m11 / scale, e = m01 / scale;
    int iter = 0, ok = 1;
    while (true) {
        if (fabsf(e) < 1.17549435082228750797e-38f) {
            e = 0.0f;
        } else {
            const float se = 8388608.0f * e;
            if (se * se <= (fabsf(d0) + fabsf(d1))) e = 0.0f;
        }
        if (e == 0.0f) break;
        if (++iter > 60) { ok = 0; break; }
        const float td = (d0 - d1) * 0.5f;
        float mu = d1;
        if (td == 0.0f) {
            mu -= fabsf(e);
        } else {
            const float e2 = e * e;
            const float h = eig_hypotf(td, e);
            if (e2 == 0.0f) mu -= e / ((td + (td > 0.0f ? h : -h)) / e);
            else mu -= e2 / (td + (td > 0.0f ? h : -h));
        }
        const float x = d0 - mu, z = e;
        float c, sn;
        if (x == 0.0f) {  // makeGivens(x, z) with z != 0
            c = 0.0f;
            sn = z < 0.0f ? 1.0f : -1.0f;
        } else if (fabsf(x) > fabsf(z)) {
            const float t = z / x;
            float u = sqrtf(1.0f + t * t);
            if (x < 0.0f) u = -u;
            c = 1.0f / u;
            sn = -t * c;
        } else {
            const float t = x / z;
            float u = sqrtf(1.0f + t * t);
            if (z < 0.0f) u = -u;
            sn = -1.0f / u;
            c = -t * sn;
        }
        const float sdk = sn * d0 + c * e;
        const float dkp1 = sn * e + c * d1;
        const float nd0 = c * (c * d0 - sn * e) - sn * (c * e - sn * d1);
        const float nd1 = sn * sdk + c * dkp1;
        const float ne = c * sdk - sn * dkp1;
        d0 = nd0;
        d1 = nd1;
        e = ne;
    }
    if (ok && d1 < d0) { const float t = d0; d0 = d1; d1 = t; }
    d0 *= scale;
    d1 *= scale;
    w0 = d1;
    w1 = d0;
}

// cv::eigen on the 2x2 float structure tensor (eig = 0: JacobiImpl_<float>(n=2): one rotation unless
// |m01| <= FLT_EPSILON, then a descending sort; eig = 1: the HAVE_EIGEN solver above), followed by the response
// expression of src/FastDetector.cc:270 evaluated in double and rounded to float.
__device__ __forceinline__ float harris_response(float a, float b, float d, int eig) {
    float w0 = a, w1 = d;
    if (eig == 1) {
        eig_selfadjoint2(a, b, d, w0, w1);
    } else if (!(fabsf(b) <= 1.1920928955078125e-07f)) {
        const float p = b;
        const float y = (float)((double)(w1 - w0) * 0.5);
        float t = fabsf(y) + cv_hypotf(p, y);
        float s = cv_hypotf(p, t);
        // c = t / s is only used to rotate off-diagonal entries, none remain for n = 2
        s = p / s;
        t = (p / t) * p;
        if (y < 0.0f) { s = -s; t = -t; }
        w0 -= t;
        w1 += t;
    }
    if (eig != 1 && w0 < w1) { float tmp = w0; w0 = w1; w1 = tmp; }
    const float prod = w0 * w1;
    const float sum = w1 + w0;
    const double sq = (double)sum * (double)sum;
    const double r = (double)prod - 0.04 * sq;
    return (float)r;
}

struct K9 {
    uint32_t k[9];  // the taps (blur9_kernel)
    // detect_kernel<true>'s band table: byte i of kh[j][m] is tap 4m + i - j (0 outside 0..8), the four taps a dword of
    // either matrix-core tap operand holds
    uint32_t kh[4][3];
    // the matrix-core passes take pixels and the bytes of h as b - 128, so the sums are offset by hbias = 128 * (sum of
    // the taps)
    int hbias;
};

static K9 make_k9(const uint16_t* k9) {
    K9 kw = {};
    uint32_t sum = 0;
    for (int i = 0; i < 9; ++i) {
        kw.k[i] = k9[i];
        sum += k9[i];
    }
    auto tap = [&](int t) -> uint32_t { return (t >= 0 && t <= 8) ? (uint32_t)k9[t] : 0u; };
    for (int j = 0; j < 4; ++j)
        for (int m = 0; m < 3; ++m)
            for (int i = 0; i < 4; ++i) kw.kh[j][m] |= tap(4 * m + i - j) << (8 * i);
    kw.hbias = (int)(128 * sum);
    return kw;
}

__device__ __forceinline__ int reflect101(int p, int len) {
    // cv::borderInterpolate(BORDER_REFLECT_101); callers clamp p to [-(len-1), 2*len-2]
    if (p < 0) p = -p;
    if (p >= len) p = 2 * len - p - 2;
    return p;
}

// Fused per-tile detector: FAST-12 candidate test + Harris response (src/FastDetector.cc:298-335) and, with kBlur
// (the fused matrix-core blur), the 9x9 fixed-point Gaussian of the same tile (src/BriefDescriptor.cc:90), so the
// image is read from HBM once.  One 256-thread workgroup per 64 x 56 output tile, the tile plus a 4-pixel halo staged
// in LDS (BORDER_REFLECT_101 values outside the image: the blur needs them, no FAST candidate ever reads them).
// Candidates are staged in LDS and appended with ONE global atomic per workgroup.
// YAVO_LM_PROFILE builds (tools/det_profile.py): detect phase cycles of lane 0 of every workgroup, summed (five
// phases; g_det_prof keeps six slots, the last 0, so that the tool also reads a build of an earlier revision)
#ifdef YAVO_LM_PROFILE
constexpr int kDetProfSlots = 131072;
__device__ unsigned long long g_det_prof[kDetProfSlots][6];
#define DP_DECL unsigned long long dp_acc[6] = {0, 0, 0, 0, 0, 0}; unsigned long long dp_t = __builtin_readcyclecounter();
#define DP_MARK(k) do { const unsigned long long t_ = __builtin_readcyclecounter(); dp_acc[k] += t_ - dp_t; dp_t = t_; } while (0)
#define DP_STORE() do { \
        const unsigned slot_ = blockIdx.x; \
        if (threadIdx.x == 0 && slot_ < kDetProfSlots) for (int q_ = 0; q_ < 6; ++q_) g_det_prof[slot_][q_] = dp_acc[q_]; \
    } while (0)
#else
#define DP_DECL
#define DP_MARK(k) do {} while (0)
#define DP_STORE() do {} while (0)
#endif
constexpr int FT_W = kFastTileW;        // 64 output columns per tile (one wave-row)
constexpr int FT_H = kFastTileH;        // 56 output rows per tile
constexpr int FT_R = 4;                 // halo: blur radius 4 (ring radius 3, Sobel + 3x3 window radius 2)
constexpr int FT_LW = FT_W + 2 * FT_R;  // 72 bytes per LDS row
constexpr int FT_LH = FT_H + 2 * FT_R;  // 64 LDS rows
constexpr int kBandM = 19;              // dwords per row of the band table (detect_kernel's s_band)
constexpr int kBlurStageDw = FT_LH * (FT_W / 4);  // the blur's output staging: 4 row blocks of 16 rows, 16 dwords each

// detect_kernel<true>'s 9x9 blur of the staged tile, both passes on the int8 matrix cores with h never leaving
// registers (every tap <= 127 and the taps sum to 256: launch_detect_blur's dispatch).  Wave cb takes column block cb
// and leaves the tile's output bytes in `stage`; after a barrier blur_store_rows writes them out.
__device__ __forceinline__ void blur_tile_mfma(const uint8_t* tile, const uint32_t* s_band, uint32_t* stage, int hbias,
                                               int lane, int cb) {
    // Horizontal: the 64 x 64 h of the tile (all 64 LDS rows, the 64 output columns) is 4 x 4 blocks of 16 x 16,
    // block (rb, cb) = A (tile rows 16 rb .., LDS columns 16 cb .. 16 cb + 63, as p - 128) x B (the banded taps:
    // B[k][n] = tap(k - n)), one v_mfma_i32_16x16x64_i8 each, wave cb taking COLUMN block cb.  Exact: products and
    // sums are integers far inside i32.  A lane (n, g) of K-block g holds bytes 16 g .. 16 g + 15 of its row /
    // column for A and B alike (the pairing is by K index, the same for both); B's dword jj is kh[n & 3][4 g + jj -
    // (n >> 2)] (0 outside 0 .. 2), read from s_band.  LDS columns past 71 (cb = 3) meet zero taps.  The
    // accumulators start at 0, so acc = h - 128 * 256 with h = sum_t tap(t) p[x + t] <= 65280: a signed 16-bit
    // value whose low byte is h's and whose high byte is h's high byte - 128, already the int8 the next MFMA wants.
    // Output lane (n, g) holds acc[rb][i] = h(LDS row 16 rb + 4 g + i, column 16 cb + n): 16 rows of one column,
    // the four lane groups of a column all 64.
    typedef int dt_v4i __attribute__((ext_vector_type(4)));
    const int nn = lane & 15, g = lane >> 4;
    const uint32_t* band = &s_band[(nn & 3) * kBandM + 3 - (nn >> 2)];  // band[M + (n >> 2)] = kh[n & 3][M]
    const dt_v4i B = {(int)band[4 * g], (int)band[4 * g + 1], (int)band[4 * g + 2], (int)band[4 * g + 3]};
    const dt_v4i Z = {0, 0, 0, 0};
    const uint8_t* arow = &tile[nn * FT_LW + 16 * cb + 16 * g];
    // Vertical: out(r, x) = sum_t tap(t) h(r + t, x) over the same K = 64 LDS rows, so those accumulators ARE an
    // MFMA operand once split into bytes, h = 256 hi + lo (each byte as b - 128, like the pixels): K slot (g, j)
    // of lane (n, g) is LDS row 16 (j >> 2) + 4 g + (j & 3) -- dword rb holds the four bytes of acc[rb][0 .. 3].
    // K need not be in row order, the tap operand only has to use the same labelling.
    dt_v4i Hlo, Hhi;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const uint2 lo = *reinterpret_cast<const uint2*>(arow + 16 * rb * FT_LW);
        const uint2 hi = *reinterpret_cast<const uint2*>(arow + 16 * rb * FT_LW + 8);
        const dt_v4i A = {(int)(lo.x ^ 0x80808080u), (int)(lo.y ^ 0x80808080u), (int)(hi.x ^ 0x80808080u),
                          (int)(hi.y ^ 0x80808080u)};
        const dt_v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, Z, 0, 0, 0);
        // bytes 0 and 1 of the four accumulators, transposed: {lo0, lo1, hi0, hi1}, {lo2, lo3, hi2, hi3}
        const uint32_t p01 = __builtin_amdgcn_perm((uint32_t)acc[1], (uint32_t)acc[0], 0x05010400u);
        const uint32_t p23 = __builtin_amdgcn_perm((uint32_t)acc[3], (uint32_t)acc[2], 0x05010400u);
        Hlo[rb] = (int)(__builtin_amdgcn_perm(p23, p01, 0x05040100u) ^ 0x80808080u);
        Hhi[rb] = (int)__builtin_amdgcn_perm(p23, p01, 0x07060302u);
    }
    // The product is taken transposed, D[column][row] = H^T x T^T with H as A: lane (x, g) ends with output row
    // 16 ob + x, columns 16 cb + 4 g .. + 3 as one dword.  The tap operand of output-row block ob: byte j of lane
    // (x, g) is tap(row(g, j) - (16 ob + x)), so dword jj is the four taps from 16 (jj - ob) + 4 g - x
    // = kh[x & 3][4 (jj - ob) + g - (x >> 2)], non-zero only for jj - ob in {0, 1}: two registers from s_band serve
    // every ob.  Output row r reads LDS rows r .. r + 8 (all inside the 64 for the 56 stored rows), so every stored
    // row sees all nine taps: sum = 256 (vh + 128 * 256) + (vl + 128 * 256), and the start value of vl carries
    // both terms and 2^15, the rounding term of (sum + 2^15) >> 16.  The output byte is byte 2 (sum < 2^24).
    const int T0 = (int)band[g], T1 = (int)band[g + 4];
    const int cv = 257 * hbias + (1 << 15);
    const dt_v4i Cv = {cv, cv, cv, cv};
    // The bytes go through the LDS the pretest list no longer needs, so that the global stores are whole 64-B row
    // segments: row R's 16 dwords at stage[16 R ..], the 16-B column groups XORed with (R >> 2) & 3 so that the
    // 64 lanes of a store instruction (16 rows x 4 dwords) hit 64 different banks.
    uint32_t* ostage = &stage[nn * 16 + ((4 * cb) ^ (nn & 12)) + g];
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
        dt_v4i T = {0, 0, 0, 0};
        T[ob] = T0;
        if (ob < 3) T[ob + 1] = T1;
        const dt_v4i vl = __builtin_amdgcn_mfma_i32_16x16x64_i8(Hlo, T, Cv, 0, 0, 0);
        const dt_v4i vh = __builtin_amdgcn_mfma_i32_16x16x64_i8(Hhi, T, Z, 0, 0, 0);
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ((uint32_t)vh[i] << 8) + (uint32_t)vl[i];
        // two v_perm pick the byte 2s pairwise, one v_perm joins the pairs
        ostage[ob * 16 * 16] = __builtin_amdgcn_perm(__builtin_amdgcn_perm(v[3], v[2], 0x0c0c0602u),
                                                     __builtin_amdgcn_perm(v[1], v[0], 0x0c0c0602u), 0x05040100u);
    }
}

// The staged rows to the pitched blurred image: 4 lanes per row, 16 B each; rows past the tile (the upper half of
// ob = 3) and past the image are not stored, columns past W land in the row padding.
__device__ __forceinline__ void blur_store_rows(const uint32_t* stage, uint8_t* __restrict__ blur, int img, int H, int W,
                                                int r0, int c0, int tid) {
    if (tid < FT_H * 4) {
        const int R = tid >> 2, q = tid & 3;
        const int bp = blur_pitch(W);
        if (r0 + R < H)
            *reinterpret_cast<uint4*>(blur + ((int64_t)img * H + r0 + R) * bp + c0 + 16 * (q ^ ((R >> 2) & 3))) =
                *reinterpret_cast<const uint4*>(&stage[R * 16 + 4 * q]);
    }
}

template <bool kBlur>
__global__ __launch_bounds__(256) void detect_kernel(const uint8_t* __restrict__ imgs, int H, int W, int stride,
                                                     int64_t pitch, int thr, int eig, uint64_t* __restrict__ cand_keys,
                                                     int64_t cap, uint32_t* __restrict__ cand_count, K9 kw,
                                                     uint8_t* __restrict__ blur) {
    __shared__ __align__(16) uint8_t tile[FT_LH * FT_LW];
    // the pretest survivors (phases 1-2) share LDS with the blur's output bytes on their way to 64-B row stores, which
    // are written from the barrier after phase 2 on
    constexpr int kPreDw = FT_W * FT_H / 2;
    static_assert(kBlurStageDw <= kPreDw, "the blur's output staging must fit in the pretest list");
    __shared__ __align__(16) uint32_t s_share[kPreDw];
    uint16_t* s_pre = reinterpret_cast<uint16_t*>(s_share);
    __shared__ uint16_t s_pos[FT_W * FT_H];
    __shared__ uint32_t s_n, s_npre, s_base;
    // kh[r][M] at r * kBandM + M + 3 for M in -3 .. 15 (0 outside 0 .. 2): the banded tap operands, read with no test
    __shared__ uint32_t s_band[4 * kBandM];
    DP_DECL
    // 1-D grid, XCD-aware: an image's tiles (and the halo rows neighbouring tiles share) stay in one XCD's L2
    const int ntx = (W + FT_W - 1) / FT_W, nty = (H + FT_H - 1) / FT_H;
    const int lb = xcd_swizzle((int)blockIdx.x, (int)gridDim.x);
    const int img = lb / (ntx * nty), tyx = lb - img * (ntx * nty);
    const int r0 = (tyx / ntx) * FT_H, c0 = (tyx % ntx) * FT_W;
    const uint8_t* src = imgs + (int64_t)img * pitch;
    const int tid = threadIdx.x;
    const int lane = lane_id();
    const int wave = tid >> 6;
    if (tid == 0) {
        s_n = 0;
        s_npre = 0;
    }
    if (kBlur && tid < 4 * kBandM) {
        const int r = tid / kBandM, M = tid - kBandM * r - 3;
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < 3; ++m)
                if (r == j && M == m) v = kw.kh[j][m];
        s_band[tid] = v;
    }

    // stage (FT_H + 8) x (FT_W + 8) = 64 x 72 bytes, one LDS dword per load: 5 per thread, all in flight before the
    // LDS writes.  Interior tiles (every source byte inside the image): each LDS dword is one unaligned dword load
    // (the hardware's unaligned mode splits it), no alignment arithmetic in VALU.  Border tiles (36% of a KITTI
    // image's 140 tiles): REFLECT_101 rows are whole source rows, so a dword whose 4 columns are inside the image is
    // still one dword load from the reflected row; only the dwords that cross the left / right edge gather their
    // 4 reflected columns byte by byte.
    {
        constexpr int kDw = FT_LW / 4;               // 18 LDS dwords per row
        constexpr int kSlots = FT_LH * kDw;          // 1152
        constexpr int kPer = (kSlots + 255) / 256;   // 5
        const bool interior = (c0 >= FT_R) && (c0 + FT_W + FT_R <= W) && (r0 >= FT_R) && (r0 + FT_H + FT_R < H);
        uint32_t v[kPer];
        if (interior) {
            // one wave-uniform base (SGPRs) and a 32-bit lane offset: slot t + 256 is 14 rows and 4 dwords on, or 15
            // rows and 14 dwords back when the dword index wraps past 18 (256 = 14 * 18 + 4), so one division for
            // the first slot and a compare + select + add for each further one (the same slots as the division form)
            const uint8_t* base = src + (int64_t)(r0 - FT_R) * stride + (c0 - FT_R);
            const int lr0 = tid / kDw, j0 = tid - lr0 * kDw;
            uint32_t off = (uint32_t)(lr0 * stride + 4 * j0);
            int j = j0;
            const uint32_t step = (uint32_t)(14 * stride + 16), wrap = (uint32_t)(15 * stride - 56);
            const uint32_t last = (uint32_t)((kSlots - 1) / kDw * stride + 4 * ((kSlots - 1) % kDw));
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                // slots past the tile (t >= kSlots, last pass only) read the last slot again; their store is skipped
                const uint32_t o = (256 * u + 255 >= kSlots && tid + 256 * u >= kSlots) ? last : off;
                __builtin_memcpy(&v[u], base + o, 4);
                const bool c = j + 4 >= kDw;
                off += c ? wrap : step;
                j += c ? 4 - kDw : 4;
            }
        } else {
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int t = min(tid + 256 * u, kSlots - 1);
                const int lr = t / kDw, j = t - lr * kDw;
                const int r = reflect101(min(max(r0 - FT_R + lr, -(H - 1)), 2 * H - 2), H);
                const uint8_t* row = src + (int64_t)r * stride;
                const int cc = c0 - FT_R + 4 * j;
                if (cc >= 0 && cc + 4 <= W) {
                    __builtin_memcpy(&v[u], row + cc, 4);
                } else {
                    uint32_t w = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        w |= (uint32_t)row[reflect101(min(max(cc + b, -(W - 1)), 2 * W - 2), W)] << (8 * b);
                    v[u] = w;
                }
            }
        }
        uint32_t* tile32 = reinterpret_cast<uint32_t*>(tile);
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int t = tid + 256 * u;
            if (t < kSlots) tile32[t] = v[u];
        }
    }
    __syncthreads();
    DP_MARK(0);

    constexpr int ring_dr[16] = YV_RING_DR;
    constexpr int ring_dc[16] = YV_RING_DC;
    const uint32_t neg_thr = (uint32_t)(-thr);
    // checkInBetween(cent, p) <=> cent > p - thr && cent < p + thr <=> |cent - p| - thr < 0: v_sad_u8 gives
    // |cent - p| + (-thr) in one instruction; its sign bit is "similar"
    // phase 1: the reference's pretest on ring pixels 0, 7 and (4 | 12) (src/FastDetector.cc:304-317) for
    // every pixel; each lane keeps a mask of its passing rows and the survivors are compacted into s_pre
    // once per wave (one scan, one LDS atomic)
    const int tx = lane;
    const int ty = __builtin_amdgcn_readfirstlane(wave);  // wave-uniform: the row bookkeeping below stays scalar
    const int c = c0 + tx;
    constexpr int kRowIters = FT_H / 4;
    // pixel (r, c) is tested iff 4 <= r < H - 4 and 4 <= c < W - 4: rows are wave-uniform, so the row test is one
    // scalar mask over the row iterations and the column test one compare
    uint32_t row_ok = 0;
#pragma unroll
    for (int u = 0; u < kRowIters; ++u) row_ok |= (uint32_t)((unsigned)(r0 + ty + 4 * u - 4) < (unsigned)(H - 8)) << u;
    // The reference's corner test is pre && run12 with pre = diff0 && diff7 && (diff4 || diff12)
    // (src/FastDetector.cc:304-317) and run12 = 12 consecutive "different" ring pixels without wrap
    // (checkContiguousPixels).  Any such run covers ring indices 4..11, so run12 implies diff7 and diff4, and
    // pre && run12 == diff0 && run12.  Phase 1 therefore filters on diff0 && diff4 && diff8 && diff11 (left, bottom,
    // right and top of the ring: a necessary condition, ~7% survivors against the pretest's ~18%) and phase 2
    // evaluates run12 exactly; the corner set is the reference's.
    // "similar" is the sign bit of sad(c, p) - thr, so the filter holds iff the sign bit of d0 | d4 | d8 | d11 is
    // clear; the sign bits are shifted into nmask (bit u = filtered out) with v_alignbit.  Every LDS read is one base
    // register (the 7 x 7 window's top-left of row iteration 0) plus a constant non-negative offset, so the
    // addresses cost no VALU.
    uint32_t nmask = 0;
    const uint8_t* wbase = &tile[(ty + FT_R - 3) * FT_LW + tx + FT_R - 3];
#pragma unroll
    for (int u = kRowIters - 1; u >= 0; --u) {
        const uint8_t* t0 = wbase + 4 * u * FT_LW;
        const uint32_t cent = t0[3 * FT_LW + 3];
        auto d = [&](int k) {
            return __builtin_amdgcn_sad_u8(cent, (uint32_t)t0[(ring_dr[k] + 3) * FT_LW + ring_dc[k] + 3], neg_thr);
        };
        const uint32_t v = (d(0) | d(4)) | (d(8) | d(11));
        nmask = __builtin_amdgcn_alignbit(nmask, v, 31);  // (nmask << 1) | (v >> 31)
    }
    uint32_t pmask = (unsigned)(c - 4) < (unsigned)(W - 8) ? (~nmask & row_ok) : 0u;
    {
        // survivors (~1 per lane) compacted into s_pre: a loop over the set bits, not one masked store per row
        const int cnt = __popc(pmask);
        const int incl = wave_incl_scan(cnt);
        const int total = __shfl(incl, 63, 64);
        uint32_t base = 0;
        if (lane == 0 && total > 0) base = atomicAdd(&s_npre, (uint32_t)total);
        base = __shfl(base, 0, 64);
        uint32_t off = base + (uint32_t)(incl - cnt);
        while (pmask) {
            const int u = __builtin_ctz(pmask);
            s_pre[off++] = (uint16_t)((ty + 4 * u) * FT_W + tx);
            pmask &= pmask - 1;
        }
    }
    __syncthreads();
    DP_MARK(1);
    // phase 2: the full 16-pixel test (>= 12 consecutive "different" ring pixels, no wrap:
    // checkContiguousPixels) densely over the pretest survivors; corners are staged in s_pos
    const uint32_t npre = s_npre;
    for (uint32_t i0 = 0; i0 < npre; i0 += 256) {  // uniform trip count: the ballots below see whole waves
        const uint32_t i = i0 + tid;
        bool cand = false;
        int pos = 0;
        if (i < npre) {
            pos = s_pre[i];
            // the 7 x 7 window's top-left: every ring read is this base plus a constant non-negative offset
            const uint8_t* t0 = &tile[((pos >> 6) + FT_R - 3) * FT_LW + (pos & 63) + FT_R - 3];
            const uint32_t cent = t0[3 * FT_LW + 3];
            // similar bits in reverse ring order (bit 15 - k for ring pixel k), one v_alignbit each; a run of
            // 12 consecutive bits without wrap is the same test in either order
            uint32_t sim = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                sim = __builtin_amdgcn_alignbit(
                    sim, __builtin_amdgcn_sad_u8(cent, (uint32_t)t0[(ring_dr[k] + 3) * FT_LW + ring_dc[k] + 3], neg_thr),
                    31);
            const uint32_t mask = ~sim & 0xFFFFu;  // "different" ring pixels
            const uint32_t a2 = mask & (mask >> 1);
            const uint32_t a4 = a2 & (a2 >> 2);
            const uint32_t a8 = a4 & (a4 >> 4);
            const uint32_t a12 = a8 & (a4 >> 8);
            cand = a12 != 0u;
        }
        const uint64_t bal = __ballot(cand);
        if (bal == 0) continue;
        const int leader = __ffsll((long long)bal) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&s_n, (uint32_t)__popcll(bal));
        base = __shfl(base, leader, 64);
        if (cand) s_pos[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)pos;
    }
    __syncthreads();
    DP_MARK(2);
    const uint32_t n = s_n;
    // Harris response of every staged corner, one lane per corner (no divergence across FAST lanes);
    // consecutive lanes write consecutive keys from `base`, the tile's range in the image's candidate list
    auto harris = [&](uint32_t base) {
        uint64_t* out = cand_keys + (int64_t)img * cap + base;
        for (uint32_t i = tid; i < n; i += 256) {
            const int pos = s_pos[i];
            const int prr = pos >> 6, ptx = pos & 63;
            // the 5 x 5 patch's top-left: every read is this base plus a constant non-negative offset
            const uint8_t* t0 = &tile[(prr + FT_R - 2) * FT_LW + ptx + FT_R - 2];
            // Sobel Ix / Iy (3x3 correlation) at the 3x3 window around the corner, from the 5x5 patch.
            int sxx = 0, sxy = 0, syy = 0;
#pragma unroll
            for (int ii = -1; ii <= 1; ++ii) {
#pragma unroll
                for (int j = -1; j <= 1; ++j) {
                    const uint8_t* q = t0 + (ii + 2) * FT_LW + j + 2;
                    const int pmm = q[-FT_LW - 1], pm0 = q[-FT_LW], pmp = q[-FT_LW + 1];
                    const int p0m = q[-1], p0p = q[1];
                    const int ppm = q[FT_LW - 1], pp0 = q[FT_LW], ppp = q[FT_LW + 1];
                    const int gx = (pmp - pmm) + 2 * (p0p - p0m) + (ppp - ppm);
                    const int gy = (ppm - pmm) + 2 * (pp0 - pm0) + (ppp - pmp);
                    sxx += gx * gx;
                    sxy += gx * gy;
                    syy += gy * gy;
                }
            }
            // all partial sums are integers < 2^24: exact in float, as in the reference
            const float resp = harris_response((float)sxx, (float)sxy, (float)syy, eig);
            out[i] = make_key(resp, (uint32_t)((r0 + prr) * W + (c0 + ptx)));  // cap >= every pixel: in range
        }
    };
    // One global atomic per workgroup reserves the output range of this tile's corners; it is issued first and its
    // latency hides behind the blur.  The barrier publishes s_base and the blur's staged rows.
    if (tid == 0 && n > 0) s_base = atomicAdd(&cand_count[img], n);
    if constexpr (kBlur) blur_tile_mfma(tile, s_band, s_share, kw.hbias, lane, ty);
    __syncthreads();
    if constexpr (kBlur) blur_store_rows(s_share, blur, img, H, W, r0, c0, tid);
    DP_MARK(3);
    if (n > 0) harris(s_base);
    DP_MARK(4);
    DP_STORE();
}

void launch_fast_harris(const uint8_t* imgs, int n_images, int H, int W, int stride, int64_t pitch,
                        int thr, int eig, uint64_t* cand_keys, int64_t cap, uint32_t* cand_count, hipStream_t s) {
    dim3 grid(((W + FT_W - 1) / FT_W) * ((H + FT_H - 1) / FT_H) * n_images);
    K9 kw = {};
    hipLaunchKernelGGL(detect_kernel<false>, grid, dim3(256), 0, s, imgs, H, W, stride, pitch, thr, eig, cand_keys,
                       cap, cand_count, kw, (uint8_t*)nullptr);
}

void launch_detect_blur(const uint8_t* imgs, int n_images, int H, int W, int stride, int64_t pitch, int thr,
                        int eig, uint64_t* cand_keys, int64_t cap, uint32_t* cand_count, const uint16_t* k9_host,
                        uint8_t* blur, hipStream_t s) {
    // the fused blur takes the taps as int8 (yv_set_blur_kernel has checked that they sum to 256); a tap above 127
    // takes the detector without blur and the stand-alone blur, which reads the image a second time
    uint32_t max_tap = 0;
    for (int i = 0; i < 9; ++i) max_tap = k9_host[i] > max_tap ? k9_host[i] : max_tap;
    if (max_tap > 127) {
        launch_fast_harris(imgs, n_images, H, W, stride, pitch, thr, eig, cand_keys, cap, cand_count, s);
        launch_blur9(imgs, n_images, H, W, stride, pitch, k9_host, blur, s);
        return;
    }
    dim3 grid(((W + FT_W - 1) / FT_W) * ((H + FT_H - 1) / FT_H) * n_images);
    const K9 kw = make_k9(k9_host);
    hipLaunchKernelGGL(detect_kernel<true>, grid, dim3(256), 0, s, imgs, H, W, stride, pitch, thr, eig, cand_keys, cap,
                       cand_count, kw, blur);
}

// ------------------------------------------------------------------------------------------------
// 9x9 fixed-point Gaussian blur (OpenCV GaussianBlurFixedPoint<uint8_t, ufixedpoint16>)
// ------------------------------------------------------------------------------------------------
constexpr int BL_W = 64, BL_H = 32, BL_R = 4;
constexpr int BL_LW = BL_W + 2 * BL_R;  // 72
constexpr int BL_LH = BL_H + 2 * BL_R;  // 40

__global__ __launch_bounds__(256) void blur9_kernel(const uint8_t* __restrict__ imgs, int H, int W, int stride,
                                                    int64_t pitch, K9 kw, uint8_t* __restrict__ blur) {
    __shared__ uint8_t tin[BL_LH * BL_LW];
    __shared__ uint32_t th[BL_LH * BL_W];
    const int img = blockIdx.z;
    const int r0 = blockIdx.y * BL_H, c0 = blockIdx.x * BL_W;
    const uint8_t* src = imgs + (int64_t)img * pitch;
    const int tid = threadIdx.x;
    for (int i = tid; i < BL_LH * BL_LW; i += 256) {
        const int lr = i / BL_LW, lc = i - lr * BL_LW;
        const int r = reflect101(min(max(r0 - BL_R + lr, -(H - 1)), 2 * H - 2), H);
        const int c = reflect101(min(max(c0 - BL_R + lc, -(W - 1)), 2 * W - 2), W);
        tin[i] = src[(int64_t)r * stride + c];
    }
    __syncthreads();
    // horizontal: exact u32 sums (<= 255 * 256)
    for (int i = tid; i < BL_LH * BL_W; i += 256) {
        const int lr = i >> 6, lc = i & 63;
        const uint8_t* q = &tin[lr * BL_LW + lc];
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) acc += kw.k[j] * (uint32_t)q[j];
        th[i] = acc;
    }
    __syncthreads();
    const int tx = tid & 63, ty = tid >> 6;
    const int c = c0 + tx;
    for (int rr = ty; rr < BL_H; rr += 4) {
        const int r = r0 + rr;
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) acc += kw.k[i] * th[(rr + i) * BL_W + tx];
        uint32_t v = (acc + (1u << 15)) >> 16;
        if (r < H && c < W) blur[(int64_t)img * blur_image_bytes(H, W) + (int64_t)r * blur_pitch(W) + c] = (uint8_t)(v > 255u ? 255u : v);
    }
}

void launch_blur9(const uint8_t* imgs, int n_images, int H, int W, int stride, int64_t pitch,
                  const uint16_t* k9_host, uint8_t* blur, hipStream_t s) {
    const K9 kw = make_k9(k9_host);
    // the image index is blockIdx.z, which ends at 65,535: a larger batch goes in slices
    constexpr int kMaxGridZ = 65535;
    for (int i0 = 0; i0 < n_images; i0 += kMaxGridZ) {
        const int n = n_images - i0 < kMaxGridZ ? n_images - i0 : kMaxGridZ;
        dim3 grid((W + BL_W - 1) / BL_W, (H + BL_H - 1) / BL_H, n);
        hipLaunchKernelGGL(blur9_kernel, grid, dim3(256), 0, s, imgs + (int64_t)i0 * pitch, H, W, stride, pitch, kw,
                           blur + (int64_t)i0 * blur_image_bytes(H, W));
    }
}

}  // namespace yavo

#ifdef YAVO_LM_PROFILE
extern "C" int yv_debug_det_prof(unsigned long long* out /* [131072][6] */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yavo::g_det_prof), sizeof(unsigned long long) * 131072 * 6) ==
                   hipSuccess ? 0 : -2;
}
#endif
