// yavo_ba_window.hip -- the sliding BA window of the chained stereo front end, assembled on the device
// (ya_vo_amd/sequence.py window_problem / apply_window / frame_records_from_block, restated): frame records in HBM, the
// graph's index arrays from per-frame counts (every landmark is seen by its own frame and the one before), no host
// round trip.  The multi-view mode (landmarks followed over several frames enter the window once; its kernels are
// yavo_ba_window_tracks.hip's) is switched here.  The yv_ba_window C ABI (include/yavo/yavo_geom.h); the solve itself
// is the yv_ba's (yavo_host.h: ba_ensure_schur, ba_solve_enqueue, ba_solve_wait of yavo_ba_host.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/yavo/yavo.h"
#include "../../include/yavo/yavo_geom.h"
#include "../../include/yavo/yavo_map.h"
#include "yavo_host.h"
#include "yavo_internal.h"
#include "yavo_se3.h"

using yavo::ba_ensure_schur;
using yavo::ba_solve_enqueue;
using yavo::ba_solve_wait;
using yavo::se3::se3_inverse;

namespace {

constexpr int kWinMaxPoses = 128;

// one workgroup per keyframe of a placed block: its T_wc, landmarks and their two observations into the records
__global__ __launch_bounds__(256) void win_add_kernel(const uint8_t* __restrict__ block, const double* __restrict__ edge_uv,
                                                      const int32_t* __restrict__ edge_query,
                                                      const uint8_t* __restrict__ matches, int max_kp, int64_t g0,
                                                      int64_t cap, int max_lm, double* __restrict__ T, int32_t* __restrict__ cnt,
                                                      int32_t* __restrict__ edge, double* __restrict__ X,
                                                      double* __restrict__ uvo, double* __restrict__ uvp,
                                                      int64_t* __restrict__ info) {
    const yv_map_header* h = reinterpret_cast<const yv_map_header*>(block);
    const int j = blockIdx.x;
    if (j == 0 && threadIdx.x == 0) info[0] = h->n_kf;
    if (j >= h->n_kf) return;
    const yv_keyframe* kf = reinterpret_cast<const yv_keyframe*>(block + sizeof(yv_map_header)) + j;
    const int64_t lmo = ((int64_t)sizeof(yv_map_header) + (int64_t)h->max_kf * (int64_t)sizeof(yv_keyframe) + 255) & ~255ll;
    const yv_landmark* lm = reinterpret_cast<const yv_landmark*>(block + lmo) + (int64_t)j * h->lm_stride;
    const int64_t g = kf->frame_id, s = g - g0;
    const int64_t k64 = g - h->first_frame;
    if (s < 0 || s >= cap || k64 < 0 || k64 >= h->n_frames) return;  // not a frame of the reserved range
    const int k = (int)k64;
    const int n = min(kf->n_landmarks, max_lm);
    if (threadIdx.x < 7) T[s * 7 + threadIdx.x] = kf->T[threadIdx.x];
    if (threadIdx.x == 0) {
        cnt[s] = n;
        info[1 + 2 * j] = g;
        info[2 + 2 * j] = n;
    }
    for (int l = threadIdx.x; l < n; l += 256) {
        const int e = (int)(lm[l].id & 0xFFFF);
        const int64_t o = s * max_lm + l;
        edge[o] = e;
        X[3 * o] = lm[l].X[0];
        X[3 * o + 1] = lm[l].X[1];
        X[3 * o + 2] = lm[l].X[2];
        const int64_t ke = (int64_t)k * max_kp + e;
        uvp[2 * o] = edge_uv[2 * ke];
        uvp[2 * o + 1] = edge_uv[2 * ke + 1];
        const int q = edge_query[ke];
        const uint8_t* rec = matches + ((int64_t)(2 * k) * max_kp + q) * 100;  // the temporal pair's Matches
        int32_t px[2];
        __builtin_memcpy(px, rec + 48, 8);  // Matches::pt2 {x, y}
        uvo[2 * o] = (double)px[0];
        uvo[2 * o + 1] = (double)px[1];
    }
}

// one workgroup per exported frame: the record's T_wc and landmarks as a map block of a sequence shard (yavo_map.h
// placed = 2: the shard's own T_wc / X_w, placed after the shards before it by yv_map_place)
__global__ __launch_bounds__(256) void win_export_kernel(const double* __restrict__ T, const int32_t* __restrict__ cnt,
                                                         const int32_t* __restrict__ edge, const double* __restrict__ X,
                                                         int64_t s_first, int n, int64_t s_chunk, int64_t id0,
                                                         int max_lm, int max_kf, int lm_stride, uint8_t* __restrict__ block) {
    yv_map_header* h = reinterpret_cast<yv_map_header*>(block);
    const int j = blockIdx.x;
    if (j == 0 && threadIdx.x == 0) {
        for (int i = 0; i < 7; ++i) h->chunk[i] = T[7 * s_chunk + i];
        h->first_frame = id0;
        h->n_frames = n;
        h->n_kf = n;
        h->kf_every = 1;
        h->lm_stride = lm_stride;
        h->max_kf = max_kf;
        h->placed = 2;
        for (int i = 0; i < 5; ++i) h->pad[i] = 0.0;
    }
    if (j >= n) return;
    const int64_t s = s_first + j, g = id0 + j;
    yv_keyframe* kf = reinterpret_cast<yv_keyframe*>(block + sizeof(yv_map_header)) + j;
    const int64_t lmo = ((int64_t)sizeof(yv_map_header) + (int64_t)max_kf * (int64_t)sizeof(yv_keyframe) + 255) & ~255ll;
    yv_landmark* lm = reinterpret_cast<yv_landmark*>(block + lmo) + (int64_t)j * lm_stride;
    const int c = min(max(cnt[s], 0), lm_stride);
    if (threadIdx.x < 7) kf->T[threadIdx.x] = T[7 * s + threadIdx.x];
    if (threadIdx.x == 0) {
        kf->frame_id = g;
        kf->n_landmarks = c;
        kf->pad = 0;
    }
    for (int l = threadIdx.x; l < c; l += 256) {
        const int64_t o = s * max_lm + l;
        lm[l].id = (g << 16) | (int64_t)edge[o];
        lm[l].X[0] = X[3 * o];
        lm[l].X[1] = X[3 * o + 1];
        lm[l].X[2] = X[3 * o + 2];
    }
}

struct WinFrames {
    int P;
    int64_t s0;                   // store index of the window's first frame
    int32_t c[kWinMaxPoses];      // landmarks owned by pose i (0 for the first pose)
    int32_t base[kWinMaxPoses];   // their first landmark index
    int32_t pe0[kWinMaxPoses];    // pe_off of pose i
    int32_t row[kWinMaxPoses];    // first co-visibility entry of row p1 = i
};

// the graph of window_problem: poses (T_cw = inverse T_wc), landmarks, edges (own frame, then the frame before),
// edges per pose / landmark and the co-visibility lists, each entry written by its landmark's thread
__global__ __launch_bounds__(256) void win_build_kernel(WinFrames F, int L, int max_lm, const double* __restrict__ T,
                                                        const double* __restrict__ Xs, const double* __restrict__ uvo,
                                                        const double* __restrict__ uvp, double* __restrict__ poses,
                                                        double* __restrict__ X, int32_t* __restrict__ ep,
                                                        int32_t* __restrict__ el, double* __restrict__ meas,
                                                        int32_t* __restrict__ le_off, int32_t* __restrict__ le,
                                                        int32_t* __restrict__ pe, int32_t* __restrict__ cv1,
                                                        int32_t* __restrict__ cv2, int32_t* __restrict__ pe_off,
                                                        int32_t* __restrict__ cv_off) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = F.P;
    if (t < n) se3_inverse(T + (F.s0 + t) * 7, poses + 7 * t);
    if (t == 0) le_off[L] = 2 * L;
    // the offsets (closed form in the counts): pose p's edges start at pe0[p]; the co-visibility lists of row p1 hold
    // (p1, p1): c[p1] + c[p1 + 1] entries and (p1, p1 + 1): c[p1 + 1], after F.row[p1]
    if (t <= n) pe_off[t] = t < n ? F.pe0[t] : 2 * L;
    for (int i = t; i <= n * n; i += gridDim.x * 256) {
        if (i == 0) {
            cv_off[0] = 0;
            continue;
        }
        const int p1 = (i - 1) / n, p2 = (i - 1) - p1 * n;
        const int cn = p1 + 1 < n ? F.c[p1 + 1] : 0;
        cv_off[i] = F.row[p1] + (p2 >= p1 ? F.c[p1] + cn : 0) + (p2 >= p1 + 1 ? cn : 0);
    }
    if (t >= L) return;
    int i = 1;  // the owning pose: base[i] <= t < base[i] + c[i]
    while (i + 1 < F.P && t >= F.base[i + 1]) ++i;
    while (F.c[i] == 0 || t >= F.base[i] + F.c[i]) ++i;
    const int j = t - F.base[i];
    const int64_t o = (F.s0 + i) * max_lm + j;
    X[3 * t] = Xs[3 * o];
    X[3 * t + 1] = Xs[3 * o + 1];
    X[3 * t + 2] = Xs[3 * o + 2];
    const int own = 2 * F.base[i] + j, prev = 2 * F.base[i] + F.c[i] + j;
    ep[own] = i;
    ep[prev] = i - 1;
    el[own] = t;
    el[prev] = t;
    meas[2 * own] = uvo[2 * o];
    meas[2 * own + 1] = uvo[2 * o + 1];
    meas[2 * prev] = uvp[2 * o];
    meas[2 * prev + 1] = uvp[2 * o + 1];
    le_off[t] = 2 * t;
    le[2 * t] = own;
    le[2 * t + 1] = prev;
    // pose i: its own edges first; pose i - 1: its own edges, then frame i's prev edges
    pe[F.pe0[i] + j] = own;
    pe[F.pe0[i - 1] + F.c[i - 1] + j] = prev;
    // (i, i): frame i's (own, own) first, frame i + 1's (prev, prev) after; (i - 1, i - 1) likewise;
    // (i - 1, i): frame i's (prev, own)
    cv1[F.row[i] + j] = own;
    cv2[F.row[i] + j] = own;
    const int r = F.row[i - 1] + F.c[i - 1];
    cv1[r + j] = prev;
    cv2[r + j] = prev;
    cv1[r + F.c[i] + j] = prev;
    cv2[r + F.c[i] + j] = own;
}

// apply_window: T_wc = inverse(T_cw) for every window frame, refined landmarks back to their frames, the anchor
__global__ __launch_bounds__(256) void win_scatter_kernel(WinFrames F, int L, int max_lm, const double* __restrict__ poses,
                                                          const double* __restrict__ X, double* __restrict__ T,
                                                          double* __restrict__ Xs, double* __restrict__ anchor,
                                                          const int* gate) {
    if (gate && *gate) return;  // enqueued with the solve: skipped when it was suspended (solve_end reruns it)
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < F.P) {
        double o[7];
        se3_inverse(poses + 7 * t, o);
        for (int k = 0; k < 7; ++k) T[(F.s0 + t) * 7 + k] = o[k];
        if (anchor && t == F.P - 1)
            for (int k = 0; k < 7; ++k) anchor[k] = o[k];
    }
    if (t >= L) return;
    int i = 1;
    while (i + 1 < F.P && t >= F.base[i + 1]) ++i;
    while (F.c[i] == 0 || t >= F.base[i] + F.c[i]) ++i;
    const int64_t o = (F.s0 + i) * max_lm + (t - F.base[i]);
    Xs[3 * o] = X[3 * t];
    Xs[3 * o + 1] = X[3 * t + 1];
    Xs[3 * o + 2] = X[3 * t + 2];
}

__global__ void win_anchor_kernel(const double* __restrict__ T, double* __restrict__ anchor) {
    if (threadIdx.x < 7) anchor[threadIdx.x] = T[threadIdx.x];
}

}  // namespace

struct yv_ba_window {
    yv_ba* ba = nullptr;
    int max_lm = 0, max_kf = 0;
    int64_t g0 = -1, cap = 0;  // store index 0 = frame g0; frames [g0, g0 + cap) fit
    int64_t hint = 0;          // yv_ba_window_reserve: frames the store is first sized for
    double *d_T = nullptr, *d_X = nullptr, *d_uvo = nullptr, *d_uvp = nullptr;
    int32_t *d_cnt = nullptr, *d_edge = nullptr;
    int64_t* d_info = nullptr;  // [1 + 3 max_kf]: n_kf, (frame, count) per keyframe of the last block, then (multi-view)
                                // the keyframes' root counts
    int64_t* h_info = nullptr;  // pinned copy
    yavo::HipOwned mem;         // the store, d_info / h_info and the event
    hipEvent_t added = nullptr;
    bool add_pending = false;
    std::vector<int32_t> h_cnt;  // per store index, -1 = not recorded
    // a solve enqueued by yv_ba_window_solve_begin, collected by yv_ba_window_solve_end
    bool solving = false;
    int solve_kind = 0;  // 1: the LM runs; 2: nothing to solve (only the anchor kernel)
    int solve_iters = 0, solve_nb = 0, solve_L = 0;
    double* solve_anchor = nullptr;
    WinFrames solve_F{};
    // the multi-view mode (yv_ba_window_set_multiview): the records' query / train / parent and each frame's table
    // train keypoint -> record in the store, the parentless records per frame on the host, the graph build's workspace
    bool multiview = false, recorded = false;
    int32_t *d_query = nullptr, *d_train = nullptr, *d_parent = nullptr, *d_tab = nullptr;
    std::vector<int32_t> h_root;
    yavo::WinTracks tracks{};
    yavo::WinTracks solve_W{};
};

namespace {

// the multi-view arrays of a store of `cap` frames, the first c0 frames copied over
int win_reserve_links(yv_ba_window* w, int64_t cap, int64_t c0, hipStream_t st) {
    const int64_t M = w->max_lm;
    int32_t* a[4] = {nullptr, nullptr, nullptr, nullptr};
    int32_t** old[4] = {&w->d_query, &w->d_train, &w->d_parent, &w->d_tab};
    bool ok = true;
    for (int i = 0; i < 4 && ok; ++i) ok = w->mem.alloc(&a[i], (size_t)(M * cap)) == YV_OK;
    for (int i = 0; i < 4 && ok && c0 > 0 && *old[i]; ++i)
        ok = hipMemcpyAsync(a[i], *old[i], sizeof(int32_t) * M * c0, hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (ok && c0 > 0) ok = hipStreamSynchronize(st) == hipSuccess;
    if (!ok) {
        w->mem.release(a[0], a[1], a[2], a[3]);
        return YV_ERR_HIP;
    }
    w->mem.release(w->d_query, w->d_train, w->d_parent, w->d_tab);
    for (int i = 0; i < 4; ++i) *old[i] = a[i];
    return YV_OK;
}

// the store covers frames [g0, end): grown by doubling, the recorded frames copied over (stream-ordered)
int win_reserve(yv_ba_window* w, int64_t first, int64_t end, hipStream_t st) {
    if (w->g0 < 0) w->g0 = first;
    if (first < w->g0) return YV_ERR_INVALID;
    if (end - w->g0 <= w->cap) return YV_OK;
    int64_t cap = std::max<int64_t>(std::max<int64_t>(64, w->hint), w->cap);
    while (cap < end - w->g0) cap *= 2;
    const int64_t M = w->max_lm;
    double *T = nullptr, *X = nullptr, *uvo = nullptr, *uvp = nullptr;
    int32_t *cnt = nullptr, *edge = nullptr;
    if (w->mem.alloc(&T, (size_t)(7 * cap)) != YV_OK || w->mem.alloc(&X, (size_t)(3 * M * cap)) != YV_OK ||
        w->mem.alloc(&uvo, (size_t)(2 * M * cap)) != YV_OK || w->mem.alloc(&uvp, (size_t)(2 * M * cap)) != YV_OK ||
        w->mem.alloc(&cnt, (size_t)cap) != YV_OK || w->mem.alloc(&edge, (size_t)(M * cap)) != YV_OK) {
        w->mem.release(T, X, uvo, uvp, cnt, edge);
        return YV_ERR_HIP;
    }
    const int64_t c0 = w->cap;
    bool ok = true;
    if (c0 > 0) {
        ok = hipMemcpyAsync(T, w->d_T, sizeof(double) * 7 * c0, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(X, w->d_X, sizeof(double) * 3 * M * c0, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(uvo, w->d_uvo, sizeof(double) * 2 * M * c0, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(uvp, w->d_uvp, sizeof(double) * 2 * M * c0, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(cnt, w->d_cnt, sizeof(int32_t) * c0, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(edge, w->d_edge, sizeof(int32_t) * M * c0, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (ok && w->multiview) ok = win_reserve_links(w, cap, c0, st) == YV_OK;
    w->mem.release(w->d_T, w->d_X, w->d_uvo, w->d_uvp, w->d_cnt, w->d_edge);
    w->d_T = T;
    w->d_X = X;
    w->d_uvo = uvo;
    w->d_uvp = uvp;
    w->d_cnt = cnt;
    w->d_edge = edge;
    w->cap = cap;
    w->h_cnt.resize((size_t)cap, -1);
    w->h_root.resize((size_t)cap, 0);
    return ok ? YV_OK : YV_ERR_HIP;
}

// the last add's keyframe counts are on the host
int win_collect(yv_ba_window* w) {
    if (!w->add_pending) return YV_OK;
    if (hipEventSynchronize(w->added) != hipSuccess) return YV_ERR_HIP;
    w->add_pending = false;
    const int64_t n = std::min<int64_t>(w->h_info[0], w->max_kf);
    for (int64_t j = 0; j < n; ++j) {
        const int64_t s = w->h_info[1 + 2 * j] - w->g0;
        if (s >= 0 && s < w->cap) {
            w->h_cnt[(size_t)s] = (int32_t)w->h_info[2 + 2 * j];
            if (w->multiview) w->h_root[(size_t)s] = (int32_t)w->h_info[1 + 2 * (int64_t)w->max_kf + j];
        }
    }
    return YV_OK;
}

}  // namespace

extern "C" int yv_ba_window_create(yv_ba* ba, int max_lm, int max_kf, yv_ba_window** out) {
    if (!out) return YV_ERR_INVALID;
    *out = nullptr;
    if (!ba || max_lm < 1 || max_lm > 65536 || max_kf < 1) return YV_ERR_INVALID;
    if (hipSetDevice(ba->dev) != hipSuccess) return YV_ERR_HIP;
    yv_ba_window* w = new yv_ba_window();
    w->ba = ba;
    w->max_lm = max_lm;
    w->max_kf = max_kf;
    if (w->mem.alloc(&w->d_info, 1 + 3 * (size_t)max_kf) != YV_OK ||
        w->mem.alloc_host(&w->h_info, 1 + 3 * (size_t)max_kf) != YV_OK ||
        w->mem.event(&w->added) != hipSuccess) {
        yv_ba_window_destroy(w);
        return YV_ERR_HIP;
    }
    *out = w;
    return YV_OK;
}

extern "C" void yv_ba_window_destroy(yv_ba_window* w) {
    if (!w) return;
    (void)hipSetDevice(w->ba->dev);
    if (w->added) (void)hipEventSynchronize(w->added);
    (void)hipStreamSynchronize(w->ba->st);
    delete w;
}

extern "C" int yv_ba_window_reserve(yv_ba_window* w, int64_t n_frames) {
    if (!w || n_frames < 0 || n_frames > (int64_t)1 << 24 || w->solving) return YV_ERR_INVALID;
    w->hint = n_frames;
    if (n_frames <= w->cap) return YV_OK;
    if (hipSetDevice(w->ba->dev) != hipSuccess) return YV_ERR_HIP;
    if (w->g0 < 0) {
        // nothing recorded yet: allocate the store now, not at the first add_block, which runs inside the caller's
        // frame loop (the store is ~150 MB per 1000 frames at 2000 landmark slots); its origin stays unset
        w->g0 = 0;
        const int rc = win_reserve(w, 0, n_frames, yavo::ctx_stream(w->ba->ctx));
        w->g0 = -1;
        return rc;
    }
    return win_reserve(w, w->g0, w->g0 + n_frames, yavo::ctx_stream(w->ba->ctx));
}

extern "C" int yv_ba_window_set_multiview(yv_ba_window* w, int on) {
    if (!w || w->solving) return YV_ERR_INVALID;
    const bool want = on != 0;
    if (want == w->multiview) return YV_OK;
    if (w->recorded) return YV_ERR_INVALID;  // the recorded frames have no links (or links nothing would follow)
    if (!want) {
        w->multiview = false;
        return YV_OK;
    }
    if (hipSetDevice(w->ba->dev) != hipSuccess) return YV_ERR_HIP;
    yavo::WinTracks& t = w->tracks;
    if (!t.up) {
        const size_t nodes = (size_t)kWinMaxPoses * (size_t)w->max_lm, cls = (size_t)kWinMaxPoses * kWinMaxPoses;
        if (w->mem.alloc(&t.up, nodes) != YV_OK || w->mem.alloc(&t.len, nodes) != YV_OK ||
            w->mem.alloc(&t.rank, nodes) != YV_OK || w->mem.alloc(&t.lmk, nodes) != YV_OK ||
            w->mem.alloc(&t.cnt, cls) != YV_OK || w->mem.alloc(&t.rp, cls) != YV_OK ||
            w->mem.alloc(&t.lbase, cls) != YV_OK || w->mem.alloc(&t.ebase, cls) != YV_OK ||
            w->mem.alloc(&t.rtot, (size_t)kWinMaxPoses) != YV_OK || w->mem.alloc(&t.A, cls + kWinMaxPoses) != YV_OK) {
            w->mem.release(t.up, t.len, t.rank, t.lmk, t.cnt, t.rp, t.lbase, t.ebase, t.rtot, t.A);
            return YV_ERR_HIP;
        }
        t.max_lm = w->max_lm;
    }
    // a store reserved before the switch gains its link arrays now (nothing is recorded in it yet)
    if (w->cap > 0 && !w->d_query && win_reserve_links(w, w->cap, 0, yavo::ctx_stream(w->ba->ctx)) != YV_OK)
        return YV_ERR_HIP;
    w->multiview = true;
    return YV_OK;
}

extern "C" int yv_ba_window_add_block(yv_ba_window* w, const void* d_block, int64_t first_frame, int n_frames,
                                      const double* d_edge_uv, const int32_t* d_edge_query, const void* d_matches,
                                      int max_kp, void* stream) {
    return yv_ba_window_add_block_linked(w, d_block, first_frame, n_frames, d_edge_uv, d_edge_query, d_matches, max_kp,
                                         nullptr, 0, stream);
}

extern "C" int yv_ba_window_add_block_linked(yv_ba_window* w, const void* d_block, int64_t first_frame, int n_frames,
                                             const double* d_edge_uv, const int32_t* d_edge_query,
                                             const void* d_matches, int max_kp, const int32_t* d_match_dj,
                                             int64_t dj_stride, void* stream) {
    if (!w || !d_block || !d_edge_uv || !d_edge_query || !d_matches || n_frames < 1 || first_frame < 0 ||
        max_kp < 1 || max_kp > 65536 || w->solving)  // a pending solve reads the store: collect it first
        return YV_ERR_INVALID;
    // multi-view: the links need the temporal pairs' match_dj, and every train keypoint a slot of the frame's table
    if (w->multiview && (!d_match_dj || dj_stride < max_kp || max_kp > w->max_lm)) return YV_ERR_INVALID;
    if (hipSetDevice(w->ba->dev) != hipSuccess) return YV_ERR_HIP;
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : yavo::ctx_stream(w->ba->ctx);
    if (win_collect(w) != YV_OK) return YV_ERR_HIP;  // one block in flight: its info buffer is reused
    const int rc = win_reserve(w, first_frame, first_frame + n_frames, st);
    if (rc != YV_OK) return rc;
    hipLaunchKernelGGL(win_add_kernel, dim3(w->max_kf), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(d_block),
                       d_edge_uv, d_edge_query, reinterpret_cast<const uint8_t*>(d_matches), max_kp, w->g0, w->cap,
                       w->max_lm,
                       w->d_T, w->d_cnt, w->d_edge, w->d_X, w->d_uvo, w->d_uvp, w->d_info);
    if (hipGetLastError() != hipSuccess) return YV_ERR_HIP;
    w->recorded = true;
    if (w->multiview) {
        const int64_t sc = first_frame - 1 - w->g0;
        const int64_t carry = sc >= 0 && w->h_cnt[(size_t)sc] >= 0 ? first_frame - 1 : -1;
        if (yavo::win_tracks_add(d_block, d_edge_query, d_match_dj, dj_stride, max_kp, carry, w->g0, w->cap, w->max_lm,
                                 w->max_kf, w->d_query, w->d_train, w->d_tab, w->d_parent,
                                 w->d_info + 1 + 2 * (int64_t)w->max_kf, st) != YV_OK)
            return YV_ERR_HIP;
    }
    if (hipMemcpyAsync(w->h_info, w->d_info, sizeof(int64_t) * (1 + (w->multiview ? 3 : 2) * (size_t)w->max_kf),
                       hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipEventRecord(w->added, st) != hipSuccess)
        return YV_ERR_HIP;
    w->add_pending = true;
    return YV_OK;
}

extern "C" int yv_ba_window_solve_begin(yv_ba_window* w, int64_t first, int n, int n_fixed, const double K[9],
                                        int max_iters, double* d_anchor) {
    if (!w || !K || n < 1 || n > kWinMaxPoses || n_fixed < 0 || max_iters < 0 || w->solving) return YV_ERR_INVALID;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return YV_ERR_INVALID;
    yv_ba* b = w->ba;
    if (hipSetDevice(b->dev) != hipSuccess || win_collect(w) != YV_OK) return YV_ERR_HIP;
    if (first < w->g0 || first + n > w->g0 + w->cap) return YV_ERR_INVALID;
    WinFrames F{};
    F.P = n;
    F.s0 = first - w->g0;
    int L = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t c = w->h_cnt[(size_t)(F.s0 + i)];
        if (c < 0) return YV_ERR_INVALID;  // frame not recorded
        F.c[i] = i == 0 ? 0 : c;           // the first frame's predecessor is outside the window
        F.base[i] = L;
        L += F.c[i];
    }
    hipStream_t st = b->st;
    if (n <= n_fixed || L == 0) {  // nothing to solve: the anchor is the last frame's pose as recorded
        if (d_anchor) {
            hipLaunchKernelGGL(win_anchor_kernel, dim3(1), dim3(64), 0, st, w->d_T + (F.s0 + n - 1) * 7, d_anchor);
            if (hipGetLastError() != hipSuccess) return YV_ERR_HIP;
        }
        w->solving = true;
        w->solve_kind = 2;
        return YV_OK;
    }
    // multi-view: the nodes are the L records counted above; a landmark per root -- every record of pose 1 (chains
    // are cut at the window's start) and the parentless records after it -- and an edge per node and per root.  The
    // co-visibility entries, sum (m + 1)(m + 2) / 2 over the chains, depend on the chains' lengths, which stay on the
    // device: a node of pose i adds at most i + 1 (its chain starts at pose 0 at the earliest), a root one more
    const bool mv = w->multiview;
    const int N = L;
    int64_t nc = 3 * (int64_t)L;
    if (mv) {
        L = F.c[1];
        nc = 0;
        for (int i = 1; i < n; ++i) {
            if (i >= 2) L += std::min(w->h_root[(size_t)(F.s0 + i)], F.c[i]);
            nc += (int64_t)F.c[i] * (i + 1);
        }
        nc += L;
        if (nc > INT32_MAX) return YV_ERR_CAPACITY;
    }
    const int E = mv ? N + L : 2 * L;
    if (n > b->max_poses || L > b->max_landmarks || E > b->max_edges) return YV_ERR_CAPACITY;
    // per pose: its edges start (own edges of frame p, then the prev edges of frame p + 1); per row p1 of the
    // co-visibility buckets: (p1, p1) = c[p1] + c[p1 + 1] entries, (p1, p1 + 1) = c[p1 + 1]. win_build_kernel writes
    // pe_off / cv_off from these (until c59 the host wrote them and copied them over: two copies per solve)
    int32_t acc = 0, racc = 0;
    for (int p = 0; p < n; ++p) {
        const int32_t cn = p + 1 < n ? F.c[p + 1] : 0;
        F.pe0[p] = acc;
        acc += F.c[p] + cn;
        F.row[p] = racc;
        racc += F.c[p] + 2 * cn;
    }
    if (nc > b->cv_cap) {
        if (hipStreamSynchronize(st) != hipSuccess) return YV_ERR_HIP;
        b->mem.release(b->d_cv_e1, b->d_cv_e2);
        b->cv_cap = 0;
        // multi-view: sized once for this window length with every slot of every frame taken, so that the frame loop
        // allocates when the window grows to its full length and never after
        const int64_t want = mv ? std::max<int64_t>(nc, (int64_t)w->max_lm * ((int64_t)n * (n + 1) / 2 + n)) : nc;
        if (b->mem.alloc(&b->d_cv_e1, want) != YV_OK || b->mem.alloc(&b->d_cv_e2, want) != YV_OK) return YV_ERR_HIP;
        b->cv_cap = want;
    }
    b->ready = false;
    yavo::BaParams& Q = b->P;
    const int nb = (std::max(L, n) + 255) / 256;
    yavo::WinTracks W = w->tracks;
    if (mv) {
        W.P = n;
        W.s0 = F.s0;
        if (yavo::win_tracks_build(W, L, E, w->d_cnt, w->d_parent, w->d_T, w->d_X, w->d_uvo, w->d_uvp, Q.poses, Q.X,
                                   b->d_ep, b->d_el, b->d_meas, b->d_le_off, b->d_le, b->d_pe_off, b->d_pe, b->d_cv_off,
                                   b->d_cv_e1, b->d_cv_e2, st) != YV_OK)
            return YV_ERR_HIP;
    } else {
        hipLaunchKernelGGL(win_build_kernel, dim3(nb), dim3(256), 0, st, F, L, w->max_lm, w->d_T, w->d_X, w->d_uvo,
                           w->d_uvp, Q.poses, Q.X, b->d_ep, b->d_el, b->d_meas, b->d_le_off, b->d_le, b->d_pe,
                           b->d_cv_e1, b->d_cv_e2, b->d_pe_off, b->d_cv_off);
        if (hipGetLastError() != hipSuccess) return YV_ERR_HIP;
    }
    Q.P = n;
    Q.nf = n_fixed;
    Q.np = n - n_fixed;
    Q.ns = 6 * Q.np;
    if (ba_ensure_schur(b, Q.np, st) != YV_OK) return YV_ERR_HIP;
    Q.L = L;
    Q.E = E;
    Q.ep = b->d_ep;
    Q.el = b->d_el;
    Q.meas = b->d_meas;
    Q.pe_off = b->d_pe_off;
    Q.pe = b->d_pe;
    Q.le_off = b->d_le_off;
    Q.le = b->d_le;
    Q.cv_off = b->d_cv_off;
    Q.cv_e1 = b->d_cv_e1;
    Q.cv_e2 = b->d_cv_e2;
    std::memcpy(b->K.v, K, sizeof b->K.v);
    b->ready = true;
    const int rc = ba_solve_enqueue(b, nullptr, nullptr, max_iters);
    if (rc != YV_OK) return rc;
    // the write-back in the same submission (skipped on the device if the solve suspends; _end reruns it then)
    if (mv) {
        if (yavo::win_tracks_scatter(W, w->d_cnt, Q.poses, Q.X, w->d_T, w->d_X, d_anchor,
                                     static_cast<const int*>(&b->d_ctl->suspended), st) != YV_OK)
            return YV_ERR_HIP;
    } else {
        hipLaunchKernelGGL(win_scatter_kernel, dim3(nb), dim3(256), 0, st, F, L, w->max_lm, Q.poses, Q.X, w->d_T,
                           w->d_X, d_anchor, static_cast<const int*>(&b->d_ctl->suspended));
        if (hipGetLastError() != hipSuccess) return YV_ERR_HIP;
    }
    w->solving = true;
    w->solve_kind = 1;
    w->solve_iters = max_iters;
    w->solve_nb = nb;
    w->solve_L = L;
    w->solve_anchor = d_anchor;
    w->solve_F = F;
    w->solve_W = W;
    return YV_OK;
}

extern "C" int yv_ba_window_solve_end(yv_ba_window* w, double* chi2_log, int* iters, int* solved) {
    if (!w || !w->solving) return YV_ERR_INVALID;
    yv_ba* b = w->ba;
    if (hipSetDevice(b->dev) != hipSuccess) return YV_ERR_HIP;
    hipStream_t st = b->st;
    const int kind = w->solve_kind;
    w->solving = false;
    w->solve_kind = 0;
    if (iters) *iters = 0;
    if (solved) *solved = 0;
    if (kind == 2) return hipStreamSynchronize(st) == hipSuccess ? YV_OK : YV_ERR_HIP;
    int it = 0;
    const int rc = ba_solve_wait(b, nullptr, nullptr, w->solve_iters, chi2_log, &it);
    if (rc != YV_OK) return rc;
    if (b->resumed) {  // the write-back enqueued by _begin was skipped: the solve finished only now
        yavo::BaParams& Q = b->P;
        if (w->multiview) {
            if (yavo::win_tracks_scatter(w->solve_W, w->d_cnt, Q.poses, Q.X, w->d_T, w->d_X, w->solve_anchor, nullptr,
                                         st) != YV_OK)
                return YV_ERR_HIP;
        } else {
            hipLaunchKernelGGL(win_scatter_kernel, dim3(w->solve_nb), dim3(256), 0, st, w->solve_F, w->solve_L,
                               w->max_lm, Q.poses, Q.X, w->d_T, w->d_X, w->solve_anchor,
                               static_cast<const int*>(nullptr));
        }
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return YV_ERR_HIP;
    }
    if (iters) *iters = it;
    if (solved) *solved = 1;
    return YV_OK;
}

extern "C" int yv_ba_window_solve(yv_ba_window* w, int64_t first, int n, int n_fixed, const double K[9], int max_iters,
                                  double* d_anchor, double* chi2_log, int* iters, int* solved) {
    const int rc = yv_ba_window_solve_begin(w, first, n, n_fixed, K, max_iters, d_anchor);
    if (rc != YV_OK) return rc;
    return yv_ba_window_solve_end(w, chi2_log, iters, solved);
}

extern "C" int yv_ba_window_read(yv_ba_window* w, int64_t frame, double* T_wc, int* n, int32_t* edge, double* X,
                                 double* uv_own, double* uv_prev, int cap) {
    if (!w || !n || w->solving) return YV_ERR_INVALID;
    if (hipSetDevice(w->ba->dev) != hipSuccess || win_collect(w) != YV_OK) return YV_ERR_HIP;
    const int64_t s = frame - w->g0;
    if (w->g0 < 0 || s < 0 || s >= w->cap || w->h_cnt[(size_t)s] < 0) return YV_ERR_INVALID;
    hipStream_t st = w->ba->st;
    const int m = w->h_cnt[(size_t)s];
    *n = m;
    if (hipStreamSynchronize(yavo::ctx_stream(w->ba->ctx)) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return YV_ERR_HIP;
    const int k = std::min(m, cap);
    const int64_t o = s * w->max_lm;
    if ((T_wc && hipMemcpy(T_wc, w->d_T + 7 * s, sizeof(double) * 7, hipMemcpyDeviceToHost) != hipSuccess) ||
        (edge && k && hipMemcpy(edge, w->d_edge + o, sizeof(int32_t) * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (X && k && hipMemcpy(X, w->d_X + 3 * o, sizeof(double) * 3 * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (uv_own && k && hipMemcpy(uv_own, w->d_uvo + 2 * o, sizeof(double) * 2 * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (uv_prev && k && hipMemcpy(uv_prev, w->d_uvp + 2 * o, sizeof(double) * 2 * k, hipMemcpyDeviceToHost) != hipSuccess))
        return YV_ERR_HIP;
    return YV_OK;
}

extern "C" int yv_ba_window_read_links(yv_ba_window* w, int64_t frame, int32_t* query, int32_t* train,
                                       int32_t* parent, int cap) {
    if (!w || w->solving || !w->multiview || cap < 0) return YV_ERR_INVALID;
    if (hipSetDevice(w->ba->dev) != hipSuccess || win_collect(w) != YV_OK) return YV_ERR_HIP;
    const int64_t s = frame - w->g0;
    if (w->g0 < 0 || s < 0 || s >= w->cap || w->h_cnt[(size_t)s] < 0) return YV_ERR_INVALID;
    if (hipStreamSynchronize(yavo::ctx_stream(w->ba->ctx)) != hipSuccess) return YV_ERR_HIP;
    const int k = std::min(w->h_cnt[(size_t)s], cap);
    const int64_t o = s * w->max_lm;
    if ((query && k && hipMemcpy(query, w->d_query + o, sizeof(int32_t) * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (train && k && hipMemcpy(train, w->d_train + o, sizeof(int32_t) * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (parent && k && hipMemcpy(parent, w->d_parent + o, sizeof(int32_t) * k, hipMemcpyDeviceToHost) != hipSuccess))
        return YV_ERR_HIP;
    return YV_OK;
}

extern "C" int yv_ba_window_export_block(yv_ba_window* w, int64_t first, int n, int64_t chunk_frame,
                                         int64_t frame_id_offset, void* d_block, int max_kf, int lm_stride,
                                         void* stream) {
    if (!w || !d_block || n < 0 || n > max_kf || max_kf < 1 || lm_stride < w->max_lm || w->solving ||
        frame_id_offset < 0 || first + frame_id_offset < 0 || first + frame_id_offset + n > ((int64_t)1 << 47))
        return YV_ERR_INVALID;
    if (hipSetDevice(w->ba->dev) != hipSuccess || win_collect(w) != YV_OK) return YV_ERR_HIP;
    if ((n > 0 && (first < w->g0 || first + n > w->g0 + w->cap)) || chunk_frame < w->g0 ||
        chunk_frame >= w->g0 + w->cap)
        return YV_ERR_INVALID;
    for (int64_t g = first; g < first + n; ++g)
        if (w->h_cnt[(size_t)(g - w->g0)] < 0) return YV_ERR_INVALID;  // not recorded
    if (w->h_cnt[(size_t)(chunk_frame - w->g0)] < 0) return YV_ERR_INVALID;
    // the records' last writers (add_block on its stream, the window write-back on the BA stream) are finished
    if (hipStreamSynchronize(yavo::ctx_stream(w->ba->ctx)) != hipSuccess ||
        hipStreamSynchronize(w->ba->st) != hipSuccess)
        return YV_ERR_HIP;
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : yavo::ctx_stream(w->ba->ctx);
    hipLaunchKernelGGL(win_export_kernel, dim3(std::max(n, 1)), dim3(256), 0, st, w->d_T, w->d_cnt,
                       w->d_edge, w->d_X, first - w->g0, n, chunk_frame - w->g0, first + frame_id_offset, w->max_lm,
                       max_kf, lm_stride, static_cast<uint8_t*>(d_block));
    return hipGetLastError() == hipSuccess ? YV_OK : YV_ERR_HIP;
}

extern "C" int yv_ba_window_trajectory(yv_ba_window* w, int64_t first, int n, double* T_wc) {
    if (!w || !T_wc || n < 0 || w->solving) return YV_ERR_INVALID;
    if (hipSetDevice(w->ba->dev) != hipSuccess || win_collect(w) != YV_OK) return YV_ERR_HIP;
    if (n == 0) return YV_OK;
    if (first < w->g0 || first + n > w->g0 + w->cap) return YV_ERR_INVALID;
    if (hipStreamSynchronize(yavo::ctx_stream(w->ba->ctx)) != hipSuccess ||
        hipStreamSynchronize(w->ba->st) != hipSuccess ||
        hipMemcpy(T_wc, w->d_T + 7 * (first - w->g0), sizeof(double) * 7 * n, hipMemcpyDeviceToHost) != hipSuccess)
        return YV_ERR_HIP;
    return YV_OK;
}
