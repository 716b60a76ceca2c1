// yavo_batch.hip -- the batched device pipeline of the C ABI (include/yavo/yavo.h): yv_batch_* up to the run and the
// view, the buffers, the match stage and the opt-in stages behind it, which the host-pointer front end (yavo_api.hip)
// runs on its single-image workspace as well.  The tracks (yv_batch_set_tracks, yv_batch_track and what follows a run's
// matches) are in yavo_batch_track.hip.  Host code only; kernels live in the stage files (yavo_detect.hip .. yavo_match_finalize.hip
// and the opt-in stages').
#include "yavo_host.h"

using namespace yavo;

namespace {

constexpr int kMaxTimedRuns = 4096;

// the swapped pair list of the reverse match
int upload_pairs_rev(yv_batch* b) {
    if (!b->m2_alloc || b->n_pairs <= 0) return YV_OK;
    std::vector<int32_t> r(b->h_pairs.size());
    for (size_t i = 0; i + 1 < r.size(); i += 2) {
        r[i] = b->h_pairs[i + 1];
        r[i + 1] = b->h_pairs[i];
    }
    YV_HIP(hipMemcpyAsync(b->pairs_rev, r.data(), sizeof(int32_t) * r.size(), hipMemcpyHostToDevice, b->ctx->stream));
    YV_HIP(hipStreamSynchronize(b->ctx->stream));
    return YV_OK;
}

int record_stage(yv_batch* b, hipStream_t s, int run, int stage) {
    if (!b->timing || run < 0) return YV_OK;
    if (b->timing == 2 && stage > 1) return YV_OK;  // detect-only: the two events around the detect kernel
    YV_HIP(hipEventRecord(b->events[(size_t)run * kEvPerRun + stage], s));
    return YV_OK;
}

yavo::MatchLists match_lists(const yv_batch* b) { return {b->desc, b->keypoints, b->kp_count, b->max_kp}; }

// (deferred: the finalize leaves the two lists to launch_match_records)
yavo::MatchRecords match_records(const yv_batch* b, bool deferred) {
    return {b->matches,  b->match_count, b->filtered, b->filt_count,
            b->match_dj, b->match_lim,   deferred ? b->match_pos : nullptr};
}

// the deferred records' filtered positions, on first use
int ensure_match_pos(yv_batch* b) {
    if (b->match_pos) return YV_OK;
    return b->mem.alloc(&b->match_pos, (size_t)std::max(b->max_pairs, 1) * (size_t)b->max_kp);
}

static_assert(YV_SUBPIX_NONE == yavo::kSubpixNone && YV_SUBPIX_OK == yavo::kSubpixOk &&
                  YV_SUBPIX_OUTSIDE == yavo::kSubpixOutside && YV_SUBPIX_EDGE == yavo::kSubpixEdge,
              "yavo.h / yavo_internal.h");

// the stereo refinement's arrays everywhere "not attempted" (dcol_q8 0, sad -1, status NONE), on s
int subpix_fill_none(yv_batch* b, hipStream_t s) {
    const size_t n = (size_t)std::max(b->max_pairs, 1) * (size_t)b->max_kp;
    YV_HIP(hipMemsetAsync(b->subpix_dcol, 0, n * sizeof(int32_t), s));
    YV_HIP(hipMemsetAsync(b->subpix_sad, 0xFF, n * sizeof(int32_t), s));
    YV_HIP(hipMemsetAsync(b->subpix_status, YV_SUBPIX_NONE, n, s));
    return YV_OK;
}

// the stereo refinement's device buffers, on first use
int ensure_subpix(yv_batch* b) {
    if (b->subpix_alloc) return YV_OK;
    const size_t nk = (size_t)b->max_kp, np = (size_t)std::max(b->max_pairs, 1);
    int rc = YV_OK;
    rc |= b->mem.alloc(&b->subpix_pairs, np);
    rc |= b->mem.alloc(&b->subpix_dcol, np * nk);
    rc |= b->mem.alloc(&b->subpix_sad, np * nk);
    rc |= b->mem.alloc(&b->subpix_status, np * nk);
    if (rc != YV_OK) {  // a retry starts clean
        b->mem.release(b->subpix_pairs, b->subpix_dcol, b->subpix_sad, b->subpix_status);
        return YV_ERR_HIP;
    }
    b->subpix_alloc = true;
    return YV_OK;
}

}  // namespace

namespace yavo {

void batch_free(yv_batch* b) {
    if (!b) return;
    if (b->bstream) (void)hipStreamSynchronize(b->bstream);
    if (b->side) (void)hipStreamSynchronize(b->side);
    if (b->rstream) (void)hipStreamSynchronize(b->rstream);  // (the owner destroys streams before it frees memory)
    if (b->lk) yv_lk_destroy(b->lk);
    pyramid_free(b);
    delete b;
}

static_assert(YV_MATCH_RATIO == yavo::kMatchRatio && YV_MATCH_MUTUAL == yavo::kMatchMutual, "yavo.h / yavo_internal.h");
static_assert(sizeof(yv_match2) == sizeof(int4), "nn2 is written as int4 {d1, j1, d2, j2}");

// 0 <= flags <= 3 and, with the ratio test, 0 < num <= den <= 32768 (d * den and d * num stay far inside int64, and
// num <= den makes a tie d1 == d2 fail)
bool match_filter_args_ok(int flags, int num, int den) {
    if (flags < 0 || flags > (YV_MATCH_RATIO | YV_MATCH_MUTUAL)) return false;
    if ((flags & YV_MATCH_RATIO) && !(num > 0 && num <= den && den <= 32768)) return false;
    return true;
}

// the match filter's device buffers, on first use
int ensure_match2(yv_batch* b) {
    if (b->m2_alloc) return YV_OK;
    const size_t nk = (size_t)b->max_kp, np = (size_t)std::max(b->max_pairs, 1);
    int rc = YV_OK;
    rc |= b->mem.alloc(&b->match_key2, np * nk);
    rc |= b->mem.alloc(&b->rev_key, np * nk);
    rc |= b->mem.alloc(&b->pairs_rev, np * 2);
    rc |= b->mem.alloc(&b->nn2, np * nk);
    rc |= b->mem.alloc(&b->rev, np * nk);
    rc |= b->mem.alloc(&b->keep, np * nk);
    if (rc != YV_OK) {  // a retry starts clean
        b->mem.release(b->match_key2, b->rev_key, b->pairs_rev, b->nn2, b->rev, b->keep);
        return YV_ERR_HIP;
    }
    hipStream_t s = b->ctx->stream;
    YV_HIP(hipMemsetAsync(b->match_key2, 0xFF, np * nk * sizeof(uint32_t), s));
    YV_HIP(hipMemsetAsync(b->rev_key, 0xFF, np * nk * sizeof(uint32_t), s));
    YV_HIP(hipMemsetAsync(b->nn2, 0, np * nk * sizeof(int4), s));
    YV_HIP(hipMemsetAsync(b->rev, 0xFF, np * nk * sizeof(int32_t), s));
    YV_HIP(hipMemsetAsync(b->keep, 0, np * nk, s));
    YV_HIP(hipStreamSynchronize(s));
    b->m2_alloc = true;
    return upload_pairs_rev(b);
}

// {drow_lo, drow_hi, dcol_lo, dcol_hi}: lo <= hi, every bound inside [-65535, 65535]
bool gate_ok(const int32_t* g) {
    for (int k = 0; k < 4; ++k)
        if (g[k] < -yavo::kGateMaxCoord || g[k] > yavo::kGateMaxCoord) return false;
    return g[0] <= g[1] && g[2] <= g[3];
}

// the gated matcher's device buffers, on first use (pairs_rev is the match filter's: the reverse launch needs both).
// The buckets cover max_row + 1 rows and max_col + 1 columns: the widest column cells that keep n_bands * col_cells
// inside kGateMaxCells, 64 columns at the least.
int ensure_gates(yv_batch* b, int max_row, int max_col) {
    if (b->gate_alloc) return YV_OK;
    const int n_bands = max_row / yavo::kGateBandRows + 1;
    int shift = 6;
    while (n_bands * ((max_col >> shift) + 1) > yavo::kGateMaxCells && shift < 16) ++shift;
    if (n_bands * ((max_col >> shift) + 1) > yavo::kGateMaxCells) return YV_ERR_CAPACITY;
    const size_t nk = (size_t)b->max_kp, np = (size_t)std::max(b->max_pairs, 1), ns = (size_t)b->nslots;
    int rc = YV_OK;
    rc |= b->mem.alloc(&b->gates, np * 4);
    rc |= b->mem.alloc(&b->gate_sorted, ns * nk);
    rc |= b->mem.alloc(&b->gate_band, ns * (size_t)(n_bands + 1));
    if (rc != YV_OK) {  // a retry starts clean
        b->mem.release(b->gates, b->gate_sorted, b->gate_band);
        return YV_ERR_HIP;
    }
    b->gate_bands = n_bands;
    b->gate_cols = (max_col >> shift) + 1;
    b->gate_shift = shift;
    b->gate_alloc = true;
    return YV_OK;
}

// the quota's cells of an H x W image fit the bucket kernel's counter table
bool select_fits(const yv_ctx* ctx, int H, int W) {
    if (ctx->sel_q <= 0) return true;
    const int64_t cy = (H + ctx->sel_rows - 1) / ctx->sel_rows, cx = (W + ctx->sel_cols - 1) / ctx->sel_cols;
    return cy * cx <= yavo::kSelMaxCells;
}

// the selection's device buffers, on first use
int ensure_select(yv_batch* b) {
    if (b->sel_alloc) return YV_OK;
    const size_t ni = (size_t)b->max_images;
    int rc = YV_OK;
    rc |= b->mem.alloc(&b->sel_keys, ni * (size_t)b->cap);
    rc |= b->mem.alloc(&b->sel_starts, ni * (size_t)(yavo::kSelMaxCells + 1));
    rc |= b->mem.alloc(&b->sel_counts, 3 * ni);
    if (rc != YV_OK) {  // a retry starts clean
        b->mem.release(b->sel_keys, b->sel_starts, b->sel_counts);
        return YV_ERR_HIP;
    }
    b->sel_alloc = true;
    return YV_OK;
}

// launch_topk over the detect kernel's lists, behind the context's selection when one is on (select_fits and
// ensure_select have passed)
void launch_select_topk(yv_batch* b, int n_images, int keep, hipStream_t s) {
    const yv_ctx* ctx = b->ctx;
    uint32_t* count = b->cand_count;
    uint32_t* seen = b->cand_seen;
    if (select_on(ctx)) {
        count = yavo::launch_select(b->cand_keys, b->cap, b->cand_count, b->cand_seen, n_images, b->H, b->W,
                                    ctx->sel_radius, ctx->sel_rows, ctx->sel_cols, ctx->sel_q, b->sel_keys,
                                    b->sel_starts, b->sel_counts, s);
        seen = b->sel_counts + 2 * (size_t)b->max_images;  // the corners before the filter are in cand_seen already
    }
    yavo::launch_topk(b->cand_keys, b->cap, count, seen, n_images, b->H, b->W, b->max_kp, keep, b->det_rc, b->det_resp,
                      b->det_count, b->kp_src, b->kp_count, b->kp_band, b->band_off, b->brief_heads, s);
}

// ---- rotation-steered BRIEF (yv_set_brief_steering) ----
// the orientation arrays, on first use (zeroed: the carry slot's rows are read before a keypoint was ever carried)
int ensure_steer(yv_batch* b) {
    if (b->steer_alloc) return YV_OK;
    const size_t n = (size_t)b->nslots * (size_t)b->max_kp;
    int rc = YV_OK;
    rc |= b->mem.alloc(&b->steer_bin, n);
    rc |= b->mem.alloc(&b->steer_mom, 2 * n);
    if (rc != YV_OK) {  // a retry starts clean
        b->mem.release(b->steer_bin, b->steer_mom);
        return YV_ERR_HIP;
    }
    hipStream_t s = b->ctx->stream;
    YV_HIP(hipMemsetAsync(b->steer_bin, 0, n, s));
    YV_HIP(hipMemsetAsync(b->steer_mom, 0, 2 * n * sizeof(int32_t), s));
    YV_HIP(hipStreamSynchronize(s));
    b->steer_alloc = true;
    return YV_OK;
}

// The descriptor stage of n_images images on s: launch_brief, or the steered kernel while steering is on (ensure_steer
// has passed).
void launch_describe(yv_batch* b, int n_images, int max_workers, hipStream_t s) {
    yv_ctx* ctx = b->ctx;
    if (steer_on(ctx)) {
        const yavo::SteerTables t{ctx->steer_bins, ctx->steer_radius, ctx->d_steer_dirs, ctx->d_steer_addr};
        yavo::launch_brief_steer(b->blur, n_images, b->H, b->W, t, b->kp_src, b->kp_count, b->max_kp, b->keypoints,
                                 b->desc, b->steer_bin, b->steer_mom, s);
        return;
    }
    // the tests' LDS offsets depend on the offsets table and W only: formed again only when the table changed (a
    // 256-thread launch in the step waited ~15-50 us for a CU behind the side stream's LM, profiles/r06/c17)
    const bool new_loff = b->loff_version != ctx->offsets_version;
    b->loff_version = ctx->offsets_version;
    yavo::launch_brief(b->blur, n_images, b->H, b->W, ctx->d_offsets, b->kp_src, b->kp_band, b->band_off, b->max_kp,
                       b->keypoints, b->desc, b->brief_loff, new_loff, b->brief_heads, max_workers, s);
}

// The selection's preflight of a run on H x W images, before any copy or launch: a refused run leaves the batch as it
// was.
int prepare_select(yv_batch* b, int H, int W) {
    if (!select_on(b->ctx)) return YV_OK;
    if (!select_fits(b->ctx, H, W)) return YV_ERR_CAPACITY;
    return ensure_select(b);
}

// The key buffers ([max_pairs][max_kp], 0xFFFFFFFF = no key) hold keys between the stage's matcher and its finalize
// only; outside a stage every entry is 0xFFFFFFFF:
// - yv_batch_create fills match_key, ensure_match2 fills match_key2 and rev_key (and the swapped pair list pairs_rev).
// - A matcher stores a key for every query of every pair, [0, nq): the forward one into match_key (top2: and
//   match_key2), the one over the swapped pairs, whose queries are the train points, into rev_key [0, nt).
// - The finalize reads and resets match_key [0, nq); the filtering one also match_key2 [0, nq) and rev_key [0, nt),
//   whether or not the swapped pairs ran (it then reads "no query" for every train point).
// So a stage with top2 ends in the filtering finalize and one without in the plain one, and no stage sees the keys of
// an earlier one, however the lists' lengths changed.  Stage event 4 separates matcher and finalize (run < 0: none).
int match_stage(yv_batch* b, MatchStage st, hipStream_t s, int run) {
    const yavo::MatchLists lists = match_lists(b);
    uint32_t* key2 = st.top2 ? b->match_key2 : nullptr;
    if (st.gated) {
        yavo::launch_gate_sort(b->keypoints, b->kp_count, b->nslots, b->max_kp, b->gate_bands, b->gate_cols,
                               b->gate_shift, b->gate_sorted, b->gate_band, s);
        yavo::launch_match_gated(lists, b->pairs, st.n_pairs, b->gate_bands, b->gate_sorted, b->gate_band, b->gates,
                                 false, b->match_key, key2, s);
        if (st.with_rev)
            yavo::launch_match_gated(lists, b->pairs_rev, st.n_pairs, b->gate_bands, b->gate_sorted, b->gate_band,
                                     b->gates, true, b->rev_key, nullptr, s);
    } else {
        yavo::launch_match(lists, b->pairs, st.n_pairs, st.max_train, b->match_key, key2, s);
        if (st.with_rev) yavo::launch_match(lists, b->pairs_rev, st.n_pairs, st.max_train_rev, b->rev_key, nullptr, s);
    }
    const int rc = record_stage(b, s, run, 4);
    const yavo::FinalizeRobust rb{b->match_key2, b->rev_key, st.flags, st.num, st.den, b->nn2, b->rev, b->keep};
    const yavo::MatchRecords out = match_records(b, st.defer_records);
    yavo::launch_match_finalize(b->match_key, lists, b->pairs, st.n_pairs, st.thr, out, st.top2 ? &rb : nullptr, s,
                                st.kp_count_copy, st.n_slots);
    if (st.defer_records) {
        // the lists beside whatever follows on s; they read the finalize's copy of the counts (the next run's top-K
        // rewrites kp_count) and the keypoints, whose next writer joins (join_records)
        YV_HIP(hipEventRecord(b->ev_keys, s));
        YV_HIP(hipStreamWaitEvent(b->rstream, b->ev_keys, 0));
        yavo::launch_match_records({lists.desc, lists.keypoints, st.kp_count_copy, lists.max_kp}, b->pairs, st.n_pairs,
                                   out, records_workgroups(b->ctx), b->rstream);
        YV_HIP(hipEventRecord(b->ev_records, b->rstream));
        b->records_pending = true;
    }
    return rc;
}

}  // namespace yavo

extern "C" {

// ------------------------------------------------------------------------------------------------
// batches
// ------------------------------------------------------------------------------------------------
int yv_batch_create(yv_ctx* ctx, int max_images, int H, int W, int max_kp, int max_pairs, yv_batch** out) {
    if (!ctx || !out || max_images <= 0 || H < 9 || W < 9 || max_kp <= 0 || max_kp > yavo::kMaxKp ||
        max_pairs < 0 || (int64_t)H * W >= (1ll << 31))
        return YV_ERR_INVALID;
    if (W > yavo::kMaxWidth) return YV_ERR_CAPACITY;  // BRIEF stages 49 image rows in LDS
    if (H > yavo::kBandRows * yavo::kMaxBands) return YV_ERR_CAPACITY;  // top-K's band lists
    *out = nullptr;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    yv_batch* b = new (std::nothrow) yv_batch();
    if (!b) return YV_ERR_INVALID;
    b->ctx = ctx;
    b->max_images = max_images;
    b->H = H;
    b->W = W;
    b->max_kp = max_kp;
    b->max_pairs = max_pairs;
    b->nslots = max_images + 1;
    b->cap = (int64_t)(H - 8) * (W - 8);  // every pixel FAST can test: no candidate is ever dropped
    const size_t ns = (size_t)b->nslots, nk = (size_t)max_kp, np = (size_t)std::max(max_pairs, 1);
    int rc = YV_OK;
    rc |= b->mem.alloc(&b->cand_keys, (size_t)max_images * (size_t)b->cap);
    rc |= b->mem.alloc(&b->cand_count, ns);
    rc |= b->mem.alloc(&b->cand_seen, ns);
    rc |= b->mem.alloc(&b->det_rc, ns * nk * 2);
    rc |= b->mem.alloc(&b->det_resp, ns * nk);
    rc |= b->mem.alloc(&b->det_count, ns);
    rc |= b->mem.alloc(&b->kp_src, ns * nk * 4);
    rc |= b->mem.alloc(&b->kp_count, ns);
    rc |= b->mem.alloc(&b->kp_count_build, ns);
    rc |= b->mem.alloc(&b->kp_band, ns * nk * 4);
    rc |= b->mem.alloc(&b->band_off, ns * (size_t)(yavo::kMaxBands + 1));
    rc |= b->mem.alloc(&b->brief_loff, 512);
    rc |= b->mem.alloc(&b->brief_heads, (size_t)yavo::kBriefHeads);
    rc |= b->mem.alloc(&b->keypoints, ns * nk);
    rc |= b->mem.alloc(&b->desc, ns * nk);
    rc |= b->mem.alloc(&b->blur, (size_t)max_images * (size_t)yavo::blur_image_bytes(H, W));
    rc |= b->mem.alloc(&b->pairs, np * 2);
    rc |= b->mem.alloc(&b->match_key, np * nk);
    rc |= b->mem.alloc(&b->matches, np * nk);
    rc |= b->mem.alloc(&b->match_count, np);
    rc |= b->mem.alloc(&b->filtered, np * nk);
    rc |= b->mem.alloc(&b->filt_count, np);
    rc |= b->mem.alloc(&b->match_dj, np * nk);
    rc |= b->mem.alloc(&b->match_lim, np);
    rc |= b->mem.alloc(&b->staging, (size_t)H * W);
    if (rc != YV_OK) {
        batch_free(b);
        return YV_ERR_HIP;
    }
    hipStream_t s = ctx->stream;
    bool ok = hipMemsetAsync(b->cand_count, 0, ns * sizeof(uint32_t), s) == hipSuccess &&
              hipMemsetAsync(b->cand_seen, 0, ns * sizeof(uint32_t), s) == hipSuccess &&
              hipMemsetAsync(b->kp_count, 0, ns * sizeof(int32_t), s) == hipSuccess &&
              hipMemsetAsync(b->det_count, 0, ns * sizeof(int32_t), s) == hipSuccess &&
              hipMemsetAsync(b->match_key, 0xFF, np * nk * sizeof(uint32_t), s) == hipSuccess &&
              hipMemsetAsync(b->keypoints, 0, ns * nk * sizeof(yv_keypoint), s) == hipSuccess &&
              hipMemsetAsync(b->match_count, 0, np * sizeof(int32_t), s) == hipSuccess &&
              hipMemsetAsync(b->filt_count, 0, np * sizeof(int32_t), s) == hipSuccess &&
              hipMemsetAsync(b->match_lim, 0, np * sizeof(int32_t), s) == hipSuccess &&
              hipStreamSynchronize(s) == hipSuccess;
    if (!ok) {
        batch_free(b);
        return YV_ERR_HIP;
    }
    *out = b;
    return YV_OK;
}

void yv_batch_destroy(yv_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    batch_free(b);
}

int yv_batch_set_pairs(yv_batch* b, const int32_t* pairs, int n_pairs) {
    if (!b || n_pairs < 0 || n_pairs > b->max_pairs || (n_pairs > 0 && !pairs)) return YV_ERR_INVALID;
    for (int i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || pairs[i] > b->max_images) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    if (b->bstream) YV_HIP(hipStreamSynchronize(b->bstream));  // an edge build in flight reads pairs
    b->build_pending = false;
    if (drain_records(b) != YV_OK) return YV_ERR_HIP;  // and so do deferred match records
    if (n_pairs > 0) {
        YV_HIP(hipMemcpyAsync(b->pairs, pairs, sizeof(int32_t) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice,
                              b->ctx->stream));
        YV_HIP(hipStreamSynchronize(b->ctx->stream));
    }
    b->h_pairs.assign(pairs, pairs + 2 * (size_t)n_pairs);
    b->n_pairs = n_pairs;
    b->n_tracks = 0;  // tracks refer to pair indices: set them again
    b->gated = false;  // and so do the gates
    b->subpix_on = false;  // and the pairs marked for the stereo refinement
    return upload_pairs_rev(b);
}

int yv_batch_set_stereo_subpix(yv_batch* b, const int32_t* pair_idx, int n, int half_win, int search, int flags) {
    if (!b || n < 0) return YV_ERR_INVALID;
    if (!pair_idx || n == 0) {
        b->subpix_on = false;
        return YV_OK;
    }
    if (half_win < 1 || half_win > yavo::kSubpixMaxWin || search < 1 || search > yavo::kSubpixMaxSearch || flags < 0 ||
        flags > YV_SUBPIX_DROP_EDGE || n > b->n_pairs)
        return YV_ERR_INVALID;
    std::vector<uint8_t> seen((size_t)b->n_pairs, 0);
    for (int i = 0; i < n; ++i) {
        const int p = pair_idx[i];
        if (p < 0 || p >= b->n_pairs || seen[p]) return YV_ERR_INVALID;
        if (b->h_pairs[2 * p] >= b->max_images || b->h_pairs[2 * p + 1] >= b->max_images) return YV_ERR_INVALID;
        seen[p] = 1;
    }
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    const int rc = ensure_subpix(b);
    if (rc != YV_OK) return rc;
    // a run or an edge build in flight, on the context's stream, the batch's or one of the caller's, reads the list
    // and the arrays: wait for the device
    hipStream_t s = b->ctx->stream;
    YV_HIP(hipDeviceSynchronize());
    b->build_pending = false;
    YV_HIP(hipMemcpyAsync(b->subpix_pairs, pair_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    if (subpix_fill_none(b, s) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipStreamSynchronize(s));
    b->subpix_n = n;
    b->subpix_win = half_win;
    b->subpix_search = search;
    b->subpix_flags = flags;
    b->subpix_on = true;
    return YV_OK;
}

int yv_batch_subpix_view_get(yv_batch* b, yv_batch_subpix_view* v) {
    if (!b || !v || !b->subpix_alloc) return YV_ERR_INVALID;
    v->dcol_q8 = b->subpix_dcol;
    v->sad = b->subpix_sad;
    v->status = b->subpix_status;
    return YV_OK;
}

int yv_batch_set_match_gates(yv_batch* b, const int32_t* gates, int n_pairs) {
    if (!b) return YV_ERR_INVALID;
    if (!gates || n_pairs == 0) {
        b->gated = false;
        return YV_OK;
    }
    if (n_pairs != b->n_pairs) return YV_ERR_INVALID;
    for (int p = 0; p < n_pairs; ++p)
        if (!gate_ok(gates + 4 * p)) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    const int rc = ensure_gates(b, b->H - 1, b->W - 1);
    if (rc != YV_OK) return rc;
    // a run in flight reads the table
    YV_HIP(hipStreamSynchronize(b->ctx->stream));
    YV_HIP(hipMemcpyAsync(b->gates, gates, sizeof(int32_t) * 4 * (size_t)n_pairs, hipMemcpyHostToDevice,
                          b->ctx->stream));
    YV_HIP(hipStreamSynchronize(b->ctx->stream));
    b->gated = true;
    return YV_OK;
}

int yv_batch_set_match_filter(yv_batch* b, int flags, int ratio_num, int ratio_den) {
    if (!match_filter_args_ok(flags, ratio_num, ratio_den) || !b) return YV_ERR_INVALID;
    if (flags != 0) {
        if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
        const int rc = ensure_match2(b);
        if (rc != YV_OK) return rc;
    }
    b->match_flags = flags;
    b->ratio_num = (flags & YV_MATCH_RATIO) ? ratio_num : 0;
    b->ratio_den = (flags & YV_MATCH_RATIO) ? ratio_den : 1;
    return YV_OK;
}

int yv_batch_match2_view_get(yv_batch* b, yv_batch_match2_view* v) {
    if (!b || !v || !b->m2_alloc) return YV_ERR_INVALID;
    v->nn2 = reinterpret_cast<const yv_match2*>(b->nn2);
    v->rev = b->rev;
    v->keep = b->keep;
    return YV_OK;
}

int yv_batch_orient_view_get(yv_batch* b, yv_batch_orient_view* v) {
    if (!b || !v || !b->steer_alloc) return YV_ERR_INVALID;
    v->bin = b->steer_bin;
    v->moments = b->steer_mom;
    return YV_OK;
}

int yv_batch_enable_timing(yv_batch* b, int on) {
    if (!b) return YV_ERR_INVALID;
    if (on && b->events.empty()) {
        if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
        b->events.resize((size_t)kMaxTimedRuns * kEvPerRun);
        for (auto& e : b->events) YV_HIP(b->mem.event(&e, hipEventDefault));
        b->tracked.assign(kMaxTimedRuns, 0);
    }
    b->timing = on == 2 ? 2 : (on != 0 ? 1 : 0);
    b->runs_recorded = 0;
    b->last_run = -1;
    std::fill(b->tracked.begin(), b->tracked.end(), 0);
    return YV_OK;
}

int yv_batch_stage_times(yv_batch* b, float* ms, int* n_runs) {
    if (!b || !ms) return YV_ERR_INVALID;
    for (int i = 0; i < 8; ++i) ms[i] = 0.f;
    const int runs = std::min(b->runs_recorded, kMaxTimedRuns);
    if (n_runs) *n_runs = runs;
    if (runs == 0) return YV_OK;
    for (int r = 0; r < runs; ++r) {
        const hipEvent_t* ev = &b->events[(size_t)r * kEvPerRun];
        if (b->timing == 2) {
            float t = 0.f;
            YV_HIP(hipEventSynchronize(ev[1]));
            YV_HIP(hipEventElapsedTime(&t, ev[0], ev[1]));
            ms[0] += t;
            continue;
        }
        YV_HIP(hipEventSynchronize(ev[b->tracked[r] ? 8 : 5]));
        for (int st = 0; st < 5; ++st) {
            float t = 0.f;
            YV_HIP(hipEventElapsedTime(&t, ev[st], ev[st + 1]));
            ms[st] += t;
        }
        if (b->tracked[r])
            for (int st = 5; st < 7; ++st) {
                float t = 0.f;
                YV_HIP(hipEventElapsedTime(&t, ev[st + 1], ev[st + 2]));
                ms[st] += t;
            }
    }
    return YV_OK;
}

int yv_batch_run(yv_batch* b, const uint8_t* d_images, int n_images, int stride, int64_t image_pitch, int match_thr,
                 int carry_from, void* stream) {
    if (!b || !d_images || n_images <= 0 || n_images > b->max_images || stride < b->W ||
        image_pitch < (int64_t)stride * (b->H - 1) + b->W || carry_from >= n_images)
        return YV_ERR_INVALID;
    yv_ctx* ctx = b->ctx;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
    const int H = b->H, W = b->W, K = b->max_kp;
    const bool pyr = b->pyr_on;  // levels -> per-level stages -> merge in place of stages 0-2 (yv_batch_set_pyramid)
    const int keep = std::min(ctx->max_corners, pyr ? b->pyr[0].keep : K);
    const int sel = prepare_select(b, H, W);
    if (sel != YV_OK) return sel;
    const bool steer = steer_on(ctx);
    if (steer && ensure_steer(b) != YV_OK) return YV_ERR_HIP;
    if (pyr) {
        const int pp = pyramid_prepare(b);
        if (pp != YV_OK) return pp;
    }
    const bool defer_records = b->rstream && b->n_tracks > 0 && b->timing != 1;  // (with copy_counts below)
    if (defer_records && ensure_match_pos(b) != YV_OK) return YV_ERR_HIP;
    if (b->pending_carry >= 0 && (join_build(b, s) != YV_OK || join_records(b, s) != YV_OK)) return YV_ERR_HIP;
    if (b->pending_carry >= 0) {
        const size_t c = (size_t)b->pending_carry, dst = (size_t)b->max_images, nk = (size_t)K;
        YV_HIP(hipMemcpyAsync(b->keypoints + dst * nk, b->keypoints + c * nk, nk * sizeof(yv_keypoint),
                              hipMemcpyDeviceToDevice, s));
        YV_HIP(hipMemcpyAsync(b->desc + dst * nk, b->desc + c * nk, nk * sizeof(Desc), hipMemcpyDeviceToDevice, s));
        YV_HIP(hipMemcpyAsync(b->kp_count + dst, b->kp_count + c, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        if (steer) {  // the carried keypoints' orientation with them
            YV_HIP(hipMemcpyAsync(b->steer_bin + dst * nk, b->steer_bin + c * nk, nk, hipMemcpyDeviceToDevice, s));
            YV_HIP(hipMemcpyAsync(b->steer_mom + dst * nk * 2, b->steer_mom + c * nk * 2, nk * 2 * sizeof(int32_t),
                                  hipMemcpyDeviceToDevice, s));
        }
        if (pyr && pyramid_carry(b, c, s) != YV_OK) return YV_ERR_HIP;  // and their levels
        b->pending_carry = -1;
    }
    int run = -1;
    if (b->timing && b->runs_recorded < kMaxTimedRuns) run = b->runs_recorded++;
    b->last_run = run;
    int rc = YV_OK;
    rc |= record_stage(b, s, run, 0);
    yavo::launch_detect_blur(d_images, n_images, H, W, stride, image_pitch, ctx->fast_thr, ctx->harris_eigen, b->cand_keys, b->cap,
                             b->cand_count, ctx->k9, b->blur, s);
    if (pyr) pyramid_detect(b, d_images, n_images, stride, image_pitch, s);
    rc |= record_stage(b, s, run, 1);
    if (b->overlap_mode == 2) rc |= launch_deferred_after(b, s);
    launch_select_topk(b, n_images, keep, s);
    if (pyr) pyramid_topk(b, n_images, s);
    rc |= record_stage(b, s, run, 2);
    if (b->overlap_mode == 4) rc |= launch_deferred_after(b, s);  // after top-K
    // the previous track's build (beside detect and top-K) reads keypoints / matches: BRIEF and finalize rewrite them
    // (its keypoint counts are a copy, kp_count_build, so top-K need not wait)
    rc |= join_build(b, s);
    rc |= join_records(b, s);  // and the previous run's deferred match records read keypoints
    launch_describe(b, n_images, brief_workers(ctx, W), s);
    if (pyr) pyramid_describe_merge(b, n_images, s);
    rc |= record_stage(b, s, run, 3);
    if (b->overlap_mode == 3) rc |= launch_deferred_after(b, s);  // after describe
    b->run_flags = b->n_pairs > 0 ? b->match_flags : 0;
    // the asynchronous edge build reads a copy of the keypoint counts (the next run's top-K rewrites them):
    // the finalize kernel writes it, where a separate device copy waited ~50 us for a CU at the end of the step
    const bool copy_counts = b->n_pairs > 0 && b->overlap && b->build_async && b->lk_step == 0;
    // In that pipelined mode with tracks, nothing later in the step reads the two lists of Matches records (the build
    // and the sub-pixel stage read match_dj / match_lim / keep): they are written on the records stream beside the next
    // run's detect.  The every-stage timing keeps the fused finalize, so its finalize stage stays the whole finalize.
    const bool defer = copy_counts && defer_records;
    if (b->n_pairs > 0) {
        // with the match filter: top-2 forward, the swapped pairs for the cross-check, then the filtering finalize
        MatchStage st;
        st.n_pairs = b->n_pairs;
        st.max_train = st.max_train_rev = K;
        st.top2 = b->run_flags != 0;
        st.with_rev = st.top2 && (b->match_flags & YV_MATCH_MUTUAL) != 0;
        st.gated = b->gated;
        st.thr = match_thr;
        st.flags = b->match_flags;
        st.num = b->ratio_num;
        st.den = b->ratio_den;
        st.kp_count_copy = copy_counts ? b->kp_count_build : nullptr;
        st.n_slots = b->nslots;
        st.defer_records = defer;
        rc |= match_stage(b, st, s, run);
        // the stereo refinement of the marked pairs, on the finalize's match_dj / match_lim / keep and the raw images
        if (b->subpix_on)
            yavo::launch_subpix_batch(d_images, n_images, H, W, stride, image_pitch, b->subpix_pairs, b->subpix_n,
                                      b->pairs, b->keypoints, b->kp_count, b->match_dj, b->match_lim,
                                      b->run_flags ? b->keep : nullptr, K, b->subpix_win, b->subpix_search,
                                      yavo::SubpixOut{b->subpix_dcol, b->subpix_sad, b->subpix_status}, s);
    } else {
        rc |= record_stage(b, s, run, 4);
    }
    b->counts_copied = copy_counts;
    rc |= record_stage(b, s, run, 5);
    if (rc != YV_OK) return YV_ERR_HIP;
    // The carry slot keeps this run's frame k-1 (the query of its first temporal pair) until the next run
    // starts, so yv_batch_track and the view still see it; the copy of image carry_from is deferred.
    b->pending_carry = carry_from;
    b->run_images = d_images;
    b->run_n = n_images;
    b->run_stride = stride;
    b->run_pitch = image_pitch;
    return check_launch();
}

int yv_batch_view_get(yv_batch* b, yv_batch_view* v) {
    if (!b || !v) return YV_ERR_INVALID;
    v->max_images = b->max_images;
    v->max_kp = b->max_kp;
    v->max_pairs = b->max_pairs;
    v->H = b->H;
    v->W = b->W;
    v->cand_cap = b->cap;
    v->cand_count = b->cand_seen;
    v->det_count = b->det_count;
    v->det_rc = b->det_rc;
    v->det_resp = b->det_resp;
    v->kp_count = b->kp_count;
    v->keypoints = b->keypoints;
    v->blurred = b->blur;
    v->blur_pitch = yavo::blur_pitch(b->W);
    v->match_count = b->match_count;
    v->matches = b->matches;
    v->filt_count = b->filt_count;
    v->filtered = b->filtered;
    v->match_dj = reinterpret_cast<const int32_t*>(b->match_dj);
    v->match_lim = b->match_lim;
    v->n_tracks = b->n_tracks;
    const EdgeSlice e = edge_slice(b, b->tbuf);
    v->edge_count = e.count;
    v->edge_X = e.X;
    v->edge_uv = e.uv;
    v->edge_query = e.query;
    v->edge_outlier = e.outlier;
    v->track_inliers = e.inliers;
    return YV_OK;
}

}  // extern "C"
