// yavo_host.h -- what the host side of the C ABI shares between its translation units (yavo_api.hip, yavo_batch.hip,
// yavo_batch_track.hip, yavo_geom_host.hip, yavo_ba_host.hip, yavo_ba_window.hip and the ABI parts of yavo_lk.hip,
// yavo_essential.hip, yavo_ba_ldlt.hip): error handling, the owner of what the HIP runtime hands out, the context, the
// batch and the bundle adjustment's workspace, and the context's two host staging mechanisms.  Host code only: nothing
// here is passed to a kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/yavo/yavo.h"
#include "yavo_internal.h"

#define YV_HIP(call)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            std::fprintf(stderr, "yavo: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), \
                         __FILE__, __LINE__);                                                  \
            return YV_ERR_HIP;                                                                 \
        }                                                                                      \
    } while (0)

namespace yavo {

inline int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        std::fprintf(stderr, "yavo: kernel launch failed: %s\n", hipGetErrorString(e));
        return YV_ERR_HIP;
    }
    return YV_OK;
}

inline bool finite_pose(const double* p) {
    for (int i = 0; i < 7; ++i)
        if (!std::isfinite(p[i])) return false;  // NaN or +-inf
    return true;
}

// Owns what the HIP runtime hands out to one handle: device memory, pinned host memory, events and streams.  The handle
// keeps its raw pointers (the kernel-argument structs stay plain data) and this owner beside them, so a buffer added
// to a handle needs no line in any destroy function.  It never synchronises: whoever clears or destroys it has
// drained the work that uses what it holds.
class HipOwned {
public:
    HipOwned() = default;
    HipOwned(const HipOwned&) = delete;
    HipOwned& operator=(const HipOwned&) = delete;
    ~HipOwned() { clear(); }

    // `count` elements of device memory (0: 1); *p == nullptr on failure
    template <class T>
    int alloc(T** p, size_t count) {
        return take(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(T), false, 0);
    }
    int alloc(void** p, size_t bytes) { return take(p, std::max<size_t>(bytes, 1), false, 0); }
    // the same of pinned host memory (hipHostMalloc's flags)
    template <class T>
    int alloc_host(T** p, size_t count, unsigned flags = hipHostMallocDefault) {
        return take(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(T), true, flags);
    }
    // a new event; *e == nullptr on failure
    hipError_t event(hipEvent_t* e, unsigned flags = hipEventDisableTiming) {
        *e = nullptr;
        const hipError_t rc = hipEventCreateWithFlags(e, flags);
        if (rc == hipSuccess) events_.push_back(*e);
        else *e = nullptr;
        return rc;
    }
    // a stream the caller created (plain, with a priority or with a CU mask)
    void adopt(hipStream_t s) { streams_.push_back(s); }
    // frees the allocations p... now and forgets them; each p becomes nullptr (a null p is skipped)
    template <class... T>
    void release(T*&... p) {
        (drop(p), ...);
    }
    // gives everything back: events, streams, memory
    void clear() {
        for (hipEvent_t e : events_) (void)hipEventDestroy(e);
        for (hipStream_t s : streams_) (void)hipStreamDestroy(s);
        for (const Mem& m : mem_) give_back(m);
        events_.clear();
        streams_.clear();
        mem_.clear();
    }

private:
    struct Mem {
        void* p;
        bool host;
    };
    static void give_back(const Mem& m) {
        if (m.host) (void)hipHostFree(m.p);
        else (void)hipFree(m.p);
    }
    int take(void** p, size_t bytes, bool host, unsigned flags) {
        *p = nullptr;
        const hipError_t e = host ? hipHostMalloc(p, bytes, flags) : hipMalloc(p, bytes);
        if (e != hipSuccess) {
            std::fprintf(stderr, "yavo: %s(%zu B) failed: %s\n", host ? "hipHostMalloc" : "hipMalloc", bytes,
                         hipGetErrorString(e));
            *p = nullptr;
            return YV_ERR_HIP;
        }
        mem_.push_back({*p, host});
        return YV_OK;
    }
    template <class T>
    void drop(T*& p) {
        for (size_t i = 0; i < mem_.size(); ++i)
            if (p && mem_[i].p == static_cast<const void*>(p)) {
                give_back(mem_[i]);
                mem_.erase(mem_.begin() + (ptrdiff_t)i);
                p = nullptr;
                return;
            }
    }
    std::vector<Mem> mem_;
    std::vector<hipEvent_t> events_;
    std::vector<hipStream_t> streams_;
};

}  // namespace yavo

using yavo::Desc;

struct yv_ctx {
    int device = 0;
    yavo::HipOwned mem;  // every buffer and stream below (the caches are handles of their own)
    hipStream_t stream = nullptr;
    int fast_thr = 40;         // include/FastDetector.hpp:35
    int harris_eigen = 0;      // cv::eigen flavour of the Harris response (yv_set_harris_eigen)
    int max_corners = 2000;    // include/FastDetector.hpp:36
    uint16_t k9[9] = {12, 22, 31, 41, 44, 41, 31, 22, 12};  // cv::GaussianBlur 9x9, sigma 2.5, 8U
    int8_t* d_offsets = nullptr;                              // [256*4]
    int offsets_version = 0;                                  // bumped by yv_set_brief_offsets
    yv_batch* single = nullptr;                               // workspace of the host-pointer API
    int32_t* h_pinned = nullptr;                              // small pinned scratch for counts
    void* scratch = nullptr;                                  // device arena of the geometry host calls
    size_t scratch_cap = 0;
    uint8_t* scratch_h = nullptr;                             // its pinned host mirror (same offsets)
    uint8_t* scratch_hd = nullptr;                            // the mirror's address for kernels (zero-copy regions)
    void* fr_ws = nullptr;                                    // yv_f_ransac_batch's hypothesis workspace
    size_t fr_ws_cap = 0;
    void* pnp_ws = nullptr;                                   // yv_pnp_ransac_batch's hypothesis workspace
    size_t pnp_ws_cap = 0;
    // yv_calc_optical_flow_pyr_lk's pyramid workspace, kept between calls (creating and destroying it per call
    // costs two hipMalloc / hipFree pairs and a device-wide synchronisation per tracked frame)
    yv_lk* lk_cache = nullptr;
    // its two image slots (device, with a pinned host copy of what each holds): a call whose prev image is the previous
    // call's next image (the tracking loop's consecutive frames) finds it and its pyramid already there
    uint8_t* lk_img_d = nullptr;
    uint8_t* lk_img_h = nullptr;
    int lk_last = -1;  // the slot holding the previous call's next image (-1: none)
    // the host findEssentialMat / recoverPose calls' workspace (yv_essential_create is ~10 hipMallocs, its destroy a
    // device synchronisation: per call they cost more than the solve), grown on demand
    yv_essential* ess_cache = nullptr;
    int lk_key[4] = {0, 0, 0, 0};  // H, W, win, max_level
    // Pinned staging of the host-pointer entry points.  The caller's buffers are pageable: a hipMemcpyAsync from or to
    // pageable memory is synchronous and goes through the runtime's own staging (~250 us per call, even for a
    // 4-byte count, and serialised across threads).  Uploads are copied into this buffer and DMA'd from it;
    // downloads land in it and are copied out after the call's stream synchronisation (stage_sync).
    uint8_t* h_stage = nullptr;
    size_t h_stage_cap = 0, h_stage_off = 0;
    struct PendingD2H {
        void* dst;
        const void* src;
        size_t bytes;
    };
    std::vector<PendingD2H> pending;
    hipStream_t side = nullptr;  // yv_side_stream: a stream on a hardware queue of its own, made on first use
    int cus = 0;                 // the device's CU count (0: not asked yet), see brief_workers
    int brief_cap = 0;           // yv_debug_set_brief_workers: a cap on brief_kernel's workers (0: none)
    // keypoint selection before the cut (yv_set_keypoint_select): all off = the reference's cut
    int sel_radius = 0, sel_rows = 0, sel_cols = 0, sel_q = 0;
    // rotation-steered BRIEF (yv_set_brief_steering): 0 bins = off, the unsteered brief_kernel.  The device tables are
    // allocated by the first call that switches it on and read by the kernel as they are: a batch keeps no form of
    // its own of them, so a new table holds for every later launch
    int steer_bins = 0, steer_radius = 0;
    int16_t* d_steer_dirs = nullptr;   // [kSteerMaxBins][2]
    uint32_t* d_steer_addr = nullptr;  // [kSteerMaxBins][256] steer_pack_offsets
};

// Track edge buffers in flight: the build of track i + kEdgeBufs waits for the pose LM of track i (side stream), so
// an LM deferred into the next run (overlap modes 2-4) does not hold up the next build.
constexpr int kEdgeBufs = 3;

namespace yavo {

// the map block a track's LM is followed by (yv_batch_track_map)
struct MapArgs {
    int64_t first_frame = 0;
    int kf_every = 1, max_kf = 1;
    void* block = nullptr;
};

}  // namespace yavo

struct yv_batch {
    yv_ctx* ctx = nullptr;
    int max_images = 0, H = 0, W = 0, max_kp = 0, max_pairs = 0, n_pairs = 0;
    int64_t cap = 0;
    int nslots = 0;
    yavo::HipOwned mem;        // what lives as long as the batch: every buffer, event and stream but the track group
    yavo::HipOwned track_mem;  // the track group, replaced as a whole when yv_batch_set_tracks grows it: tracks,
                               // track_K, T_right, edge_*, track_inliers and the lk_* buffers
    uint64_t* cand_keys = nullptr;
    uint32_t* cand_count = nullptr;
    uint32_t* cand_seen = nullptr;
    int32_t* det_rc = nullptr;
    float* det_resp = nullptr;
    int32_t* det_count = nullptr;
    int32_t* kp_src = nullptr;
    int32_t* kp_count = nullptr;
    int32_t* kp_count_build = nullptr;  // the asynchronous edge build's copy of the run's counts (top-K rewrites them)
    int32_t* kp_band = nullptr;     // [slot][max_kp] int4 {row, col, id, slot}: the kept keypoints by BRIEF band
    int32_t* band_off = nullptr;    // [slot][kMaxBands + 1]
    int32_t* brief_loff = nullptr;  // [256][2] BRIEF test offsets in the band's LDS layout (launch_brief)
    int32_t* brief_heads = nullptr; // [8] brief_kernel's band queue heads: zeroed by top-K / kp_boundary_kernel
    int loff_version = -1;          // the ctx offsets_version brief_loff was formed from (-1: never)
    bool counts_copied = false;     // this run's finalize wrote kp_count_build (the asynchronous build's copy)
    yv_keypoint* keypoints = nullptr;
    Desc* desc = nullptr;
    uint8_t* blur = nullptr;
    int32_t* pairs = nullptr;
    uint32_t* match_key = nullptr;
    yv_match* matches = nullptr;
    int32_t* match_count = nullptr;
    yv_match* filtered = nullptr;
    int32_t* filt_count = nullptr;
    int2* match_dj = nullptr;       // [max_pairs][max_kp] {distance, train index}
    int32_t* match_lim = nullptr;   // [max_pairs] removeOutliers limit
    // the match filter (yv_batch_set_match_filter): allocated by the first call that switches it on
    int match_flags = 0, ratio_num = 0, ratio_den = 1;
    int run_flags = 0;              // the filter of the last yv_batch_run (0: the tracks read no keep array)
    bool m2_alloc = false;
    uint32_t* match_key2 = nullptr; // [max_pairs][max_kp] second-best keys
    uint32_t* rev_key = nullptr;    // [max_pairs][max_kp] the swapped pairs' keys
    int32_t* pairs_rev = nullptr;   // [max_pairs][2] {train image, query image}
    int4* nn2 = nullptr;            // [max_pairs][max_kp] {d1, j1, d2, j2}
    int32_t* rev = nullptr;         // [max_pairs][max_kp]
    uint8_t* keep = nullptr;        // [max_pairs][max_kp]
    // the match gates (yv_batch_set_match_gates): allocated by the first call that sets gates
    bool gated = false, gate_alloc = false;
    int gate_bands = 0;             // bands of kGateBandRows rows in gate_band's tables
    int gate_cols = 0, gate_shift = 0;  // column cells per band, of (1 << gate_shift) columns
    int32_t* gates = nullptr;       // [max_pairs][4] {drow_lo, drow_hi, dcol_lo, dcol_hi}
    uint2* gate_sorted = nullptr;   // [slot][max_kp] {row | column << 16, keypoint index} by (band, column cell)
    int32_t* gate_band = nullptr;   // [slot][gate_bands + 1] band starts
    // keypoint selection (yv_set_keypoint_select): allocated by the first run or call with selection on
    bool sel_alloc = false;
    uint64_t* sel_keys = nullptr;   // [max_images][cap] the bucketed candidate lists
    int32_t* sel_starts = nullptr;  // [max_images][kSelMaxCells + 1] the buckets' starts
    uint32_t* sel_counts = nullptr; // [3][max_images] filtered counts after suppression / quota, top-K's unused "seen"
    // the keypoints' orientation (yv_set_brief_steering): allocated by the first run or call with steering on
    bool steer_alloc = false;
    uint8_t* steer_bin = nullptr;   // [slot][max_kp]
    int32_t* steer_mom = nullptr;   // [slot][max_kp][2] (m10, m01)
    // the sub-pixel stereo refinement (yv_batch_set_stereo_subpix): allocated by the first call that switches it on
    bool subpix_on = false, subpix_alloc = false;
    int subpix_n = 0, subpix_win = 0, subpix_search = 0, subpix_flags = 0;
    int32_t* subpix_pairs = nullptr;  // [max_pairs] the marked pairs
    int32_t* subpix_dcol = nullptr;   // [max_pairs][max_kp] dcol_q8, by query keypoint
    int32_t* subpix_sad = nullptr;    // [max_pairs][max_kp]
    uint8_t* subpix_status = nullptr; // [max_pairs][max_kp]
    // the scale pyramid (yv_batch_set_pyramid): the sidecar is allocated by the first call that switches it on, a
    // level's workspace (a batch of that level's size, which owns the level's images) while the sizes stay the same
    struct PyrLevel {
        int H = 0, W = 0, keep = 0, stride = 0;
        uint8_t* img = nullptr;     // [max_images][H][stride] (level 0: the run's images)
        yv_batch* ws = nullptr;     // levels >= 1
    };
    bool pyr_on = false;
    int pyr_levels = 0;
    PyrLevel pyr[8];
    uint8_t* pyr_level = nullptr;   // [slot][max_kp] the level of every merged keypoint
    int32_t* pyr_rc = nullptr;      // [slot][max_kp][2] its position on its own level
    int32_t* pyr_count0 = nullptr;  // [slot] level 0's keypoints
    uint8_t* staging = nullptr;  // one H x W input image (host-pointer API)
    std::vector<int32_t> h_pairs;   // host copy of the pairs (track validation)
    // tracks (PnP over the matches)
    int n_tracks = 0, max_tracks = 0;
    int32_t* tracks = nullptr;      // [max_tracks][2] {stereo pair, temporal pair}
    double* track_K = nullptr;      // [max_tracks][9]
    double* T_right = nullptr;      // [7]
    // edge / LM buffers, kEdgeBufs of each ([kEdgeBufs][...], buffer k: edge_slice): track i builds into and its LM
    // reads buffer i % kEdgeBufs; with the LM on the side stream the build of track i + kEdgeBufs waits for the LM of
    // track i (ev_lm)
    double* edge_X = nullptr;       // [kEdgeBufs][max_tracks][max_kp][3]
    double* edge_uv = nullptr;      // [kEdgeBufs][max_tracks][max_kp][2]
    int32_t* edge_query = nullptr;  // [kEdgeBufs][max_tracks][max_kp]
    int32_t* edge_count = nullptr;  // [kEdgeBufs][max_tracks]
    uint8_t* edge_outlier = nullptr;   // [kEdgeBufs][max_tracks][max_kp]
    int32_t* track_inliers = nullptr;  // [kEdgeBufs][max_tracks]
    // LK tracking mode (yv_batch_set_track_lk): tracks are {stereo pair of frame k-1, image index of frame k}
    int lk_step = 0;                // > 0: LK mode, LK images are the run's images 0, lk_step, 2 lk_step, ...
    yv_lk* lk = nullptr;
    int lk_max_count = 30;
    double lk_eps = 0.01, lk_min_eig = 1e-3;
    int32_t* lk_sp = nullptr;       // [max_tracks] stereo pair per track
    int32_t* lk_pairs = nullptr;    // [max_tracks][2] LK slots (prev, next)
    double* lk_X = nullptr;         // [max_tracks][max_kp][3]
    float* lk_pts = nullptr;        // [max_tracks][max_kp][2]
    float* lk_next = nullptr;
    float* lk_err = nullptr;
    uint8_t* lk_status = nullptr;
    int32_t* lk_q = nullptr;
    int32_t* lk_count = nullptr;
    // lk_X / lk_pts / lk_q / lk_count come in two sets: with the asynchronous build (overlap mode) the LK stage of
    // track i reads set i & 1 on bstream while track i + 1's stereo points fill the other one on the run's stream
    int lk_set = 0;
    hipEvent_t ev_lk[2] = {};
    bool lk_ev_pending[2] = {false, false};
    // track RANSAC (yv_batch_set_track_ransac): 0 iterations = off.  Its outputs come kEdgeBufs times like the edge
    // buffers (buffer k: ransac_slice), so a view or a deferred LM of track i still reads its own while track i + 1's
    // RANSAC runs; the hypothesis workspace is one, every RANSAC runs in order on the LM's stream.  Sized for max_tracks
    // by ensure_ransac (the call that switches the mode on, or the yv_batch_set_tracks that grows the tracks)
    int ransac_iters = 0, ransac_min = 0, ransac_tracks = 0, ransac_iters_cap = 0;
    double ransac_thr = 0;
    uint32_t* ransac_draws = nullptr;  // [ransac_iters_cap][3]
    void* ransac_ws = nullptr;
    double* ransac_pose = nullptr;     // [kEdgeBufs][ransac_tracks][7] the LM's priors
    uint8_t* ransac_inlier = nullptr;  // [kEdgeBufs][ransac_tracks][max_kp]
    int32_t* ransac_inliers = nullptr; // [kEdgeBufs][ransac_tracks]
    int32_t* ransac_found = nullptr;   // [kEdgeBufs][ransac_tracks]
    const uint8_t* run_images = nullptr;  // the last yv_batch_run's images (LK reads them)
    int run_n = 0, run_stride = 0;
    int64_t run_pitch = 0;
    int tbuf = 0;                   // buffer of the last yv_batch_track
    int track_calls = 0;
    bool overlap = false;           // LM on the side stream
    int overlap_mode = 0;           // 1: LM after the edge build; 2 / 3 / 4: after the next run's detect / describe / top-K
    struct DeferredLM {              // overlap modes 2 / 3: an LM launch waiting for the next yv_batch_run
        bool active = false;
        int k = 0, run = -1;
        const double* priors = nullptr;
        double* poses = nullptr;
        hipEvent_t* ev = nullptr;   // stage timing events of the run the track belongs to
        bool has_map = false;
        yavo::MapArgs map;
    } deferred;
    hipEvent_t ev_defer = nullptr;
    hipStream_t side = nullptr;
    // edge build beside the next run (YAVO_BUILD_ASYNC, default on with the overlap, match tracker only): the
    // build runs on `bstream` after the run's finalize (ev_fin); the next run's top-K, which rewrites the keypoint
    // counts the build reads, waits for ev_built
    hipStream_t bstream = nullptr;
    bool build_async = false, build_pending = false;
    hipEvent_t ev_fin = nullptr, ev_built = nullptr;
    // match records beside the next run (pipelined mode, see yv_batch_run): the finalize on the run's stream writes
    // the keys' results and match_pos only (ev_keys), match_records_kernel writes the two lists on `rstream`
    // (ev_records); the next writer of the keypoints it reads waits for it (join_records)
    hipStream_t rstream = nullptr;
    hipEvent_t ev_keys = nullptr, ev_records = nullptr;
    bool records_pending = false;
    int32_t* match_pos = nullptr;   // [max_pairs][max_kp] position in the filtered list, -1: dropped (on first use)
    hipEvent_t ev_edges[kEdgeBufs] = {}, ev_lm[kEdgeBufs] = {};
    bool lm_pending[kEdgeBufs] = {};
    hipEvent_t ev_map = nullptr;    // after the last yv_batch_track_map's block (yv_batch_map_wait)
    bool map_written = false;
    hipEvent_t ev_map_release = nullptr;  // the block's readers (yv_batch_map_release): the next block write waits
    bool map_release_pending = false;
    // stage timing: events 0..5 bracket the run's stages, 6..8 the track's
    int timing = 0;  // 0 off, 1 every stage, 2 detect only
    std::vector<hipEvent_t> events;  // kEvPerRun per recorded run
    std::vector<uint8_t> tracked;    // run r was followed by a timed yv_batch_track
    int runs_recorded = 0;
    int last_run = -1;
    int pending_carry = -1;  // image whose keypoints enter the carry slot at the start of the next run
};

namespace yavo {

inline int set_device(yv_ctx* ctx) {
    YV_HIP(hipSetDevice(ctx->device));
    return YV_OK;
}

inline bool select_on(const yv_ctx* ctx) { return ctx->sel_radius > 0 || ctx->sel_q > 0; }
inline bool steer_on(const yv_ctx* ctx) { return ctx->steer_bins > 0; }

// ---- the context (yavo_api.hip) ----
// brief_kernel's worker limit for images W wide
int brief_workers(yv_ctx* ctx, int W);
// match_records_kernel's one-wave workgroups: two per SIMD
int records_workgroups(yv_ctx* ctx);
// A stream on a hardware queue of its own (see yv_side_stream): a CU mask with every CU enabled, or a plain
// non-blocking stream where the runtime refuses the mask.  nullptr on failure; the caller owns the stream.
hipStream_t make_queue_stream(yv_ctx* ctx);

// Pinned staging of the host-pointer entry points (yv_ctx::h_stage): uploads are copied into the staging buffer and
// DMA'd from it, downloads land in it and reach the caller's buffers in stage_sync.
hipError_t stage_sync(yv_ctx* ctx, hipStream_t s);
uint8_t* stage_alloc(yv_ctx* ctx, size_t bytes, hipStream_t s);
hipError_t stage_h2d(yv_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s);
hipError_t stage_h2d_2d(yv_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                        size_t height, hipStream_t s);
hipError_t stage_d2h(yv_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s);

// Drops the downloads of a call that returns before its stage_sync (an error path): they must not be copied into
// buffers the caller no longer expects to be written.  The staging offset is kept, so nothing still in flight is
// overwritten before the next stage_sync.
struct StageScope {
    yv_ctx* ctx;
    explicit StageScope(yv_ctx* c) : ctx(c) {}
    ~StageScope() { ctx->pending.clear(); }
};

// Carves 256-B aligned sub-buffers out of the context's device arena (grown on demand, outside any
// timed loop: the host-pointer calls are synchronous anyway).  The arena has a pinned host mirror with the same
// offsets: a call's inputs are copied into the mirror (`in`), one DMA moves the range they span (`upload`), and its
// outputs come back in one DMA of the range they span (`download`, then `finish` after the stream drained).  A
// host-pointer call is then two copies however many buffers it has (round 3: one staged copy per buffer, ~10 per
// LoopHandler frame).
//
// Regions added with add_host live in the pinned mirror itself and kernels address them there (zero-copy over PCIe):
// read-once inputs and the small outputs, which then need no DMA at all (a host call's outputs are a few hundred
// bytes to a few tens of KB; a DMA costs a copy-engine round trip each way).  Inputs the kernels read many times stay
// device regions.
struct Arena {
    yv_ctx* ctx;
    size_t need = 0;
    struct Req {
        void** p;
        size_t bytes;
        bool host;
    };
    std::vector<Req> reqs;
    size_t in_lo = SIZE_MAX, in_hi = 0, out_lo = SIZE_MAX, out_hi = 0;
    struct Out {
        void* dst;
        size_t off, bytes;
    };
    std::vector<Out> outs;
    std::vector<std::pair<size_t, size_t>> host_spans;  // [off, off + bytes) of every add_host region
    template <class T>
    void add(T** p, size_t count) {
        reqs.push_back({reinterpret_cast<void**>(p), count * sizeof(T), false});
        need += (count * sizeof(T) + 255) & ~(size_t)255;
    }
    template <class T>
    void add_host(T** p, size_t count) {
        reqs.push_back({reinterpret_cast<void**>(p), count * sizeof(T), true});
        need += (count * sizeof(T) + 255) & ~(size_t)255;
    }
    // places the regions added so far, after growing the arena and its mirror when they do not fit
    int commit();
    bool is_host(const void* p) const;
    size_t off_of(const void* p) const;
    void in(const void* dev, const void* src, size_t bytes);
    // a pitched host image into a packed device image
    void in_2d(const void* dev, const uint8_t* src, size_t spitch, size_t width, size_t height);
    void out(void* dst, const void* dev, size_t bytes);
    hipError_t upload(hipStream_t s);
    // one DMA over the span of the device outputs, unless a host region (written in place by the kernel) lies inside
    // it: then one DMA per device output, so the span's stale device bytes never land on those host results
    hipError_t download(hipStream_t s);
    // after the stream drained: the outputs into the caller's buffers
    void finish();
    // download, wait, finish
    hipError_t fetch(hipStream_t s);
};

// ---- the batch (yavo_batch.hip), as the single-image workspace of the host-pointer front end uses it ----
// One match stage over the batch's first n_pairs pairs (the defaults: the single-image workspace's plain match).
struct MatchStage {
    int n_pairs = 1;
    int max_train = 0, max_train_rev = 0;  // bounds of the train lists' lengths, forward and over the swapped pairs
                                           // (ungated: <= 2048 selects the FP4 matcher)
    bool top2 = false;                     // second-best keys and the filtering finalize (ensure_match2 has passed)
    bool with_rev = false;                 // top2 only: the swapped pairs as well
    bool gated = false;                    // inside the pairs' gates (ensure_gates has passed, b->gates is set)
    int thr = 0;                           // removeOutliers' threshold
    int flags = 0, num = 0, den = 1;       // top2 only: the filter's tests
    int32_t* kp_count_copy = nullptr;      // optional: the finalize copies kp_count[0, n_slots) there
    int n_slots = 0;
    bool defer_records = false;            // the record lists on b->rstream after the finalize (kp_count_copy is set,
                                           // b->match_pos and b->rstream exist)
};

void batch_free(yv_batch* b);  // no drain of the context's stream: yv_batch_destroy's part
bool match_filter_args_ok(int flags, int num, int den);
bool gate_ok(const int32_t* g);
bool select_fits(const yv_ctx* ctx, int H, int W);
// the opt-in stages' device buffers, on first use
int ensure_match2(yv_batch* b);
int ensure_gates(yv_batch* b, int max_row, int max_col);
int ensure_steer(yv_batch* b);
int prepare_select(yv_batch* b, int H, int W);
void launch_select_topk(yv_batch* b, int n_images, int keep, hipStream_t s);
void launch_describe(yv_batch* b, int n_images, int max_workers, hipStream_t s);
int match_stage(yv_batch* b, MatchStage st, hipStream_t s, int run);

// ---- the scale pyramid (yavo_pyramid.hip), as yv_batch_run drives it: the levels >= 1 of a run with the pyramid on ----
void pyramid_free(yv_batch* b);   // the level workspaces (batch_free's part)
int pyramid_prepare(yv_batch* b);  // the levels' selection preflight and steering arrays, before any copy or launch
int pyramid_carry(yv_batch* b, size_t from, hipStream_t s);  // slot `from`'s sidecar into the carry slot
// stage 0: level images and the levels' detect; stage 1: their selection and cut; stage 2: their BRIEF and the merge
void pyramid_detect(yv_batch* b, const uint8_t* d_images, int n_images, int stride, int64_t image_pitch,
                    hipStream_t s);
void pyramid_topk(yv_batch* b, int n_images, hipStream_t s);
void pyramid_describe_merge(yv_batch* b, int n_images, hipStream_t s);

// ---- the track half of the batch (yavo_batch_track.hip), as yv_batch_run and the view need it ----
constexpr int kEvPerRun = 9;  // stage timing events per recorded run (yv_batch::events)
// the next writer of what an asynchronous edge build reads is ordered after it on stream s
int join_build(yv_batch* b, hipStream_t s);
// the same for the deferred match records, which read the keypoints
int join_records(yv_batch* b, hipStream_t s);
// drains the records stream (before the host rewrites or frees what match_records_kernel reads or writes)
int drain_records(yv_batch* b);
// the deferred LM of the previous track, ordered after the work issued on s so far (the stage it waits for)
int launch_deferred_after(yv_batch* b, hipStream_t s);
// edge buffer k of kEdgeBufs (every pointer null while no tracks were set)
struct EdgeSlice {
    double* X;
    double* uv;
    int32_t* query;
    int32_t* count;
    uint8_t* outlier;
    int32_t* inliers;
};
EdgeSlice edge_slice(const yv_batch* b, int k);

}  // namespace yavo

// ---- bundle adjustment (yavo_ba_host.hip), as the sliding window (yavo_ba_window.hip) needs it ----
struct yv_ba {
    yv_ctx* ctx = nullptr;
    int dev = 0;
    hipStream_t st = nullptr;
    hipStream_t ctx_st = nullptr;  // the context's stream (yv_ba_set_stream(b, NULL) returns to it)
    int max_poses = 0, max_landmarks = 0, max_edges = 0;
    int64_t cv_cap = 0;
    yavo::BaParams P;
    yavo::Mat3 K{};
    yavo::HipOwned mem;  // every d_* / h_* buffer below and P's
    int32_t *d_ep = nullptr, *d_el = nullptr, *d_pe_off = nullptr, *d_pe = nullptr, *d_le_off = nullptr,
            *d_le = nullptr, *d_cv_off = nullptr, *d_cv_e1 = nullptr, *d_cv_e2 = nullptr;
    double* d_meas = nullptr;
    int* d_cur = nullptr;          // the state the estimate is in (BaParams::cur)
    unsigned* d_ticket = nullptr;  // last-workgroup counters [kBaTickets]
    int64_t schur_cap = 0;         // Schur tasks P.spart / P.sticket hold
    unsigned long long* d_maxdiag = nullptr;
    double* h_scal = nullptr;  // pinned [4]
    yavo::BaCtl* d_ctl = nullptr;  // the device-driven LM's control block
    yavo::BaCtl* h_ctl = nullptr;  // pinned copy
    double* h_log = nullptr;       // pinned copy of d_log [log_cap]
    bool resumed = false;          // the last ba_solve_wait resumed a suspended solve
    int resumes = 0;               // suspended trial loops resumed since creation (yv_ba_debug_resumes)
    double* d_log = nullptr;       // [log_cap] chi2 per iteration
    int log_cap = 0;
    int device_control = 1;        // yv_ba_set_control
    bool ready = false;
};

namespace yavo {

// the global-memory LDLT keeps 2 x 6 np doubles in dynamic LDS beside ~3 KB of its own: 6 x 640 rows fit 64 KB
constexpr int kBaMaxPoses = 640;

// the tree4096 class totals and per-sum counters of np free poses: P.spart / P.sticket for the Schur tasks (nb upper
// blocks + np b_schur rows), P.rpart / P.rticket for the pose reduce; grown on demand
int ba_ensure_schur(yv_ba* b, int np, hipStream_t st);
// The LM of yv_ba_solve with its control on the device, in two halves (see yavo_ba_host.hip).  poses / landmarks: host
// in / out; both nullptr: the problem's poses and landmarks are already in P.poses / P.X on the device and stay there.
int ba_solve_enqueue(yv_ba* b, const double* poses, const double* landmarks, int max_iters);
int ba_solve_wait(yv_ba* b, double* poses, double* landmarks, int max_iters, double* chi2_log, int* iters);

// ---- the window's multi-view mode (yavo_ba_window_tracks.hip), as yavo_ba_window.hip drives it ----
// One window's nodes and tables: node (i, l) = record l of window pose i >= 1, id = i * max_lm + l.
struct WinTracks {
    int P = 0;        // window poses
    int max_lm = 0;
    int64_t s0 = 0;   // store index of the window's first frame
    int32_t *up = nullptr, *len = nullptr, *rank = nullptr, *lmk = nullptr;  // [kWinMaxPoses * max_lm] per node:
                                                                             // root id; at roots the chain length
                                                                             // and the rank in its class; landmark
    int32_t *cnt = nullptr, *rp = nullptr, *lbase = nullptr, *ebase = nullptr;  // [P][P] per class (s, e)
    int32_t *rtot = nullptr, *A = nullptr;                                      // [P], [P + 1][P]
};
// the records win_add_kernel just wrote gain query / train / parent and their frame its train -> record table;
// d_roots[j] = records of keyframe j without a parent.  carry_frame: first_frame - 1 where recorded, else -1
int win_tracks_add(const void* d_block, const int32_t* d_edge_query, const int32_t* d_match_dj, int64_t dj_stride,
                   int max_kp, int64_t carry_frame, int64_t g0, int64_t cap, int max_lm, int max_kf, int32_t* d_query,
                   int32_t* d_train, int32_t* d_tab, int32_t* d_parent, int64_t* d_roots, hipStream_t st);
// the multi-view graph of the window (L landmarks, E edges, as the host counted them) into the yv_ba's arrays
int win_tracks_build(const WinTracks& W, int L, int E, const int32_t* d_cnt, const int32_t* d_parent, const double* d_T,
                     const double* d_Xs, const double* d_uvo, const double* d_uvp, double* poses, double* X,
                     int32_t* ep, int32_t* el, double* meas, int32_t* le_off, int32_t* le, int32_t* pe_off, int32_t* pe,
                     int32_t* cv_off, int32_t* cv1, int32_t* cv2, hipStream_t st);
int win_tracks_scatter(const WinTracks& W, const int32_t* d_cnt, const double* poses, const double* X, double* d_T,
                       double* d_Xs, double* d_anchor, const int* gate, hipStream_t st);

}  // namespace yavo
