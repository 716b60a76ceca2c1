// yavo_batch_track.hip -- the track half of the batch (include/yavo/yavo.h, yavo_map.h): what follows a run's matches.
// yv_batch_set_tracks and the track group's buffers, yv_batch_track (the edge build from the matches or through LK,
// then the pose LM and the map block) and the streams and events that let them overlap the next run: the build
// stream, the side stream of the LM, the LM deferred into the next run.  Host code only; the kernels are in
// yavo_track.hip, yavo_pose.hip, yavo_lk.hip and yavo_map.hip.
#include "yavo_host.h"

#include <cstdlib>

#include "../../include/yavo/yavo_map.h"

using namespace yavo;

namespace yavo {

// (what an asynchronous edge build reads: keypoint counts, keypoints, match lists, pairs, tracks)
int join_build(yv_batch* b, hipStream_t s) {
    if (!b->build_pending) return YV_OK;
    YV_HIP(hipStreamWaitEvent(s, b->ev_built, 0));
    b->build_pending = false;
    return YV_OK;
}

// (what the deferred match records read: the counts' copy, keypoints, match_dj, match_pos, pairs)
int join_records(yv_batch* b, hipStream_t s) {
    if (!b->records_pending) return YV_OK;
    YV_HIP(hipStreamWaitEvent(s, b->ev_records, 0));
    b->records_pending = false;
    return YV_OK;
}

int drain_records(yv_batch* b) {
    if (b->rstream) YV_HIP(hipStreamSynchronize(b->rstream));
    b->records_pending = false;
    return YV_OK;
}

EdgeSlice edge_slice(const yv_batch* b, int k) {
    if (!b->edge_X) return {};
    const size_t nt = (size_t)b->max_tracks, nk = (size_t)b->max_kp;
    return {b->edge_X + k * nt * nk * 3, b->edge_uv + k * nt * nk * 2,  b->edge_query + k * nt * nk,
            b->edge_count + k * nt,      b->edge_outlier + k * nt * nk, b->track_inliers + k * nt};
}

}  // namespace yavo

namespace {

// What the track kernels read of the last run.  keep while that run filtered its matches, the refinement's arrays
// while it is on: otherwise null, the unfiltered / unrefined kernels.
TrackSrc track_src(const yv_batch* b) {
    const bool sub = b->subpix_on;
    return {b->pairs, b->keypoints, b->kp_count, b->match_dj, b->match_lim, b->max_kp, b->track_K, b->T_right,
            b->run_flags ? b->keep : nullptr, sub ? b->subpix_dcol : nullptr, sub ? b->subpix_status : nullptr,
            sub && (b->subpix_flags & YV_SUBPIX_DROP_EDGE) != 0};
}

// buffer k of the track RANSAC's outputs
struct RansacSlice {
    double* pose;
    uint8_t* inlier;
    int32_t* inliers;
    int32_t* found;
};

RansacSlice ransac_slice(const yv_batch* b, int k) {
    const size_t nt = (size_t)b->ransac_tracks, nk = (size_t)b->max_kp;
    return {b->ransac_pose + k * nt * 7, b->ransac_inlier + k * nt * nk, b->ransac_inliers + k * nt,
            b->ransac_found + k * nt};
}

// The track RANSAC's buffers for max_tracks tracks and ransac_iters hypotheses (a no-op while the mode is off, no tracks
// were set or they already fit).  The caller has drained the streams a track runs on.
int ensure_ransac(yv_batch* b) {
    if (b->ransac_iters == 0 || b->max_tracks == 0) return YV_OK;
    if (b->max_tracks > 65535) return YV_ERR_CAPACITY;  // a track per workgroup row of the grid
    if (b->ransac_tracks >= b->max_tracks && b->ransac_iters_cap >= b->ransac_iters) return YV_OK;
    b->mem.release(b->ransac_ws, b->ransac_pose, b->ransac_inlier, b->ransac_inliers, b->ransac_found);
    b->ransac_tracks = 0;
    const size_t nt = (size_t)b->max_tracks, nk = (size_t)b->max_kp;
    const int cap = std::max(b->ransac_iters_cap, b->ransac_iters);
    int rc = YV_OK;
    rc |= b->mem.alloc(&b->ransac_ws, yavo::pnp_ransac_ws_bytes(b->max_tracks, cap));
    rc |= b->mem.alloc(&b->ransac_pose, kEdgeBufs * nt * 7);
    rc |= b->mem.alloc(&b->ransac_inlier, kEdgeBufs * nt * nk);
    rc |= b->mem.alloc(&b->ransac_inliers, kEdgeBufs * nt);
    rc |= b->mem.alloc(&b->ransac_found, kEdgeBufs * nt);
    if (rc != YV_OK) return YV_ERR_HIP;
    hipStream_t s = b->ctx->stream;
    YV_HIP(hipMemsetAsync(b->ransac_pose, 0, sizeof(double) * kEdgeBufs * nt * 7, s));
    YV_HIP(hipMemsetAsync(b->ransac_inlier, 0, kEdgeBufs * nt * nk, s));
    YV_HIP(hipMemsetAsync(b->ransac_inliers, 0, sizeof(int32_t) * kEdgeBufs * nt, s));
    YV_HIP(hipMemsetAsync(b->ransac_found, 0, sizeof(int32_t) * kEdgeBufs * nt, s));
    YV_HIP(hipStreamSynchronize(s));
    b->ransac_tracks = b->max_tracks;
    b->ransac_iters_cap = cap;
    return YV_OK;
}

// The pose LM (and the map block) of one track. Overlap: on the side stream after the edge build (ev_edges[k]);
// otherwise on `s`, in order.
int launch_lm(yv_batch* b, const yv_batch::DeferredLM& L, hipStream_t s) {
    const int k = L.k;
    const EdgeSlice e = edge_slice(b, k);
    hipStream_t ls = s;
    if (b->overlap) {
        // the LM reads only this track's edge buffer, priors and poses: it runs on the side stream beside the
        // next batch's image kernels (which overwrite keypoints / matches, already consumed by the build)
        YV_HIP(hipStreamWaitEvent(b->side, b->ev_edges[k], 0));
        ls = b->side;
    }
    if (L.ev) YV_HIP(hipEventRecord(L.ev[7], ls));
    const double* priors = L.priors;
    if (b->ransac_iters > 0) {
        // the track RANSAC on the LM's stream, over the same edge buffer and after the same waits: whatever orders the
        // LM against the build before it and the build kEdgeBufs tracks later (ev_lm[k], recorded below) orders this
        // too.  It reads the caller's priors here, where the LM would, and the LM reads buffer k's priors after it
        const RansacSlice r = ransac_slice(b, k);
        yavo::launch_pnp_ransac(nullptr, e.count, b->max_kp, b->n_tracks, e.X, e.uv, b->track_K,
                                b->ransac_draws, b->ransac_iters, b->ransac_thr, b->ransac_min, L.priors, r.pose,
                                r.inlier, r.inliers, r.found, b->ransac_ws, ls);
        priors = r.pose;
    }
    yavo::launch_track_pose(b->n_tracks, e.count, b->max_kp, e.X, e.uv, b->track_K, priors, L.poses, e.outlier,
                            e.inliers, ls);
    if (L.ev) {
        YV_HIP(hipEventRecord(L.ev[8], ls));
        b->tracked[L.run] = 1;
    }
    if (L.has_map) {
        // the chunk's map block, after the LM on its stream: the build that next rewrites this edge buffer waits
        // for ev_lm[k], recorded below, so it also waits for these reads. The block itself is rewritten only
        // after its last reader released it (the all-gather of the previous chunk, yv_batch_map_release).
        if (b->map_release_pending) {
            YV_HIP(hipStreamWaitEvent(ls, b->ev_map_release, 0));
            b->map_release_pending = false;
        }
        yavo::launch_map_chunk(L.poses, b->n_tracks, L.map.first_frame, L.map.kf_every, e.count, e.X, e.outlier,
                               b->max_kp, L.map.max_kf, L.map.block, ls);
        if (!b->ev_map) YV_HIP(b->mem.event(&b->ev_map));
        YV_HIP(hipEventRecord(b->ev_map, ls));
        b->map_written = true;
    }
    if (b->overlap) {
        YV_HIP(hipEventRecord(b->ev_lm[k], ls));
        b->lm_pending[k] = true;
    }
    return YV_OK;
}

// Launch a deferred LM now (its inputs are complete once ev_edges was recorded).
int flush_deferred(yv_batch* b) {
    if (!b->deferred.active) return YV_OK;
    b->deferred.active = false;
    return launch_lm(b, b->deferred, b->ctx->stream);
}

int batch_track(yv_batch* b, const double* d_priors, double* d_poses, void* stream, const MapArgs* map) {
    if (!b || (b->n_tracks > 0 && (!d_priors || !d_poses))) return YV_ERR_INVALID;
    if (b->n_tracks == 0) return YV_OK;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : b->ctx->stream;
    if (flush_deferred(b) != YV_OK) return YV_ERR_HIP;  // two tracks without a run between them
    const int k = b->track_calls++ % kEdgeBufs;
    const size_t nt = (size_t)b->max_tracks, nk = (size_t)b->max_kp;
    const EdgeSlice e = edge_slice(b, k);
    const EdgeOut edges{e.X, e.uv, e.query, e.count};
    const int run = b->last_run;
    const bool timed = b->timing == 1 && run >= 0 && !b->tracked[run];
    hipEvent_t* ev = timed ? &b->events[(size_t)run * kEvPerRun] : nullptr;
    const hipStream_t s_run = s;
    TrackSrc src = track_src(b);
    PointsOut lk_pts{};
    int lk_j = 0;
    if (b->lk_step > 0) {
        // LK: frame k-1's stereo map points from this run's keypoints / matches, on the run's stream (the next run
        // rewrites them), into the point set the LK stage two tracks ago has finished reading
        if (!b->run_images || b->run_n < b->lk_step) return YV_ERR_INVALID;
        lk_j = b->lk_set;
        b->lk_set ^= 1;
        lk_pts = {b->lk_X + (size_t)lk_j * nt * nk * 3, b->lk_pts + (size_t)lk_j * nt * nk * 2,
                  b->lk_q + (size_t)lk_j * nt * nk, b->lk_count + (size_t)lk_j * nt};
        if (b->lk_ev_pending[lk_j]) YV_HIP(hipStreamWaitEvent(s_run, b->ev_lk[lk_j], 0));
        b->lk_ev_pending[lk_j] = false;
        yavo::launch_stereo_points(b->lk_sp, b->n_tracks, src, lk_pts, s_run);
    }
    if (b->overlap && b->build_async) {
        // the build (match: edges from the run's matches; LK: pyramids, flow, edges) waits for the run on s and
        // leaves s free for the next run's detect; the match build reads a copy of the keypoint counts
        if (b->lk_step == 0) {
            if (!b->counts_copied)
                YV_HIP(hipMemcpyAsync(b->kp_count_build, b->kp_count, sizeof(int32_t) * (size_t)b->nslots,
                                      hipMemcpyDeviceToDevice, s_run));
            src.kp_count = b->kp_count_build;
        }
        YV_HIP(hipEventRecord(b->ev_fin, s_run));
        YV_HIP(hipStreamWaitEvent(b->bstream, b->ev_fin, 0));
        s = b->bstream;
    }
    // buffer k was last read by the LM kEdgeBufs tracks ago (side stream): the build must not overwrite it early
    if (b->lm_pending[k]) YV_HIP(hipStreamWaitEvent(s, b->ev_lm[k], 0));
    if (timed) YV_HIP(hipEventRecord(ev[6], s));
    if (b->lk_step > 0) {
        // trackLastFrame: frame k-1's stereo map points -> calcOpticalFlowPyrLK into frame k -> edges
        const int n_lk = (b->run_n + b->lk_step - 1) / b->lk_step;
        int rc = yv_lk_build(b->lk, b->run_images, n_lk, b->run_stride, b->run_pitch * b->lk_step, s);
        if (rc != YV_OK) return rc;
        rc = yv_lk_track_batch(b->lk, b->lk_pairs, b->n_tracks, lk_pts.pts, lk_pts.count, b->max_kp, b->lk_max_count,
                               b->lk_eps, b->lk_min_eig, b->lk_next, b->lk_status, b->lk_err, s);
        if (rc != YV_OK) return rc;
        yavo::launch_lk_edges(b->n_tracks, lk_pts, b->lk_next, b->lk_status, b->max_kp, edges, s);
        if (s != s_run) {
            if (!b->ev_lk[lk_j]) YV_HIP(b->mem.event(&b->ev_lk[lk_j]));
            YV_HIP(hipEventRecord(b->ev_lk[lk_j], s));
            b->lk_ev_pending[lk_j] = true;
        }
    } else {
        yavo::launch_track_build(b->tracks, b->n_tracks, src, edges, s);
    }
    if (b->overlap) YV_HIP(hipEventRecord(b->ev_edges[k], s));
    if (s != s_run && b->lk_step == 0) {  // (the LK stage reads nothing the next run writes: no join)
        YV_HIP(hipEventRecord(b->ev_built, s));
        b->build_pending = true;
    }
    yv_batch::DeferredLM L;
    L.active = true;
    L.k = k;
    L.run = timed ? run : -1;
    L.priors = d_priors;
    L.poses = d_poses;
    L.ev = ev;
    if (map) {
        L.has_map = true;
        L.map = *map;
    }
    b->tbuf = k;
    if (b->overlap_mode >= 2) {
        // launched by the next yv_batch_run after its detect (2) / describe (3) stage, or by a flush
        b->deferred = L;
        return check_launch();
    }
    const int rc = launch_lm(b, L, s);
    if (rc != YV_OK) return rc;
    return check_launch();
}

}  // namespace

int yavo::launch_deferred_after(yv_batch* b, hipStream_t s) {
    if (!b->deferred.active) return YV_OK;
    if (!b->ev_defer) YV_HIP(b->mem.event(&b->ev_defer));
    YV_HIP(hipEventRecord(b->ev_defer, s));
    YV_HIP(hipStreamWaitEvent(b->side, b->ev_defer, 0));
    b->deferred.active = false;
    return launch_lm(b, b->deferred, s) == YV_OK ? YV_OK : YV_ERR_HIP;
}

extern "C" {

int yv_batch_set_tracks(yv_batch* b, const int32_t* tracks, int n_tracks, const double K[9], const double T_right[7]) {
    if (!b || n_tracks < 0 || (n_tracks > 0 && (!tracks || !K || !T_right))) return YV_ERR_INVALID;
    for (int t = 0; t < n_tracks; ++t) {
        const int sp = tracks[2 * t], tp = tracks[2 * t + 1];
        if (sp < 0 || sp >= b->n_pairs) return YV_ERR_INVALID;
        if (b->lk_step > 0) {
            // LK mode: {stereo pair of frame k-1, image of frame k}, both LK images (multiples of the step)
            const int prev = b->h_pairs[2 * sp];
            if (prev % b->lk_step || prev >= b->max_images || tp < 0 || tp >= b->max_images || tp % b->lk_step)
                return YV_ERR_INVALID;
        } else {
            if (tp < 0 || tp >= b->n_pairs) return YV_ERR_INVALID;
            if (b->h_pairs[2 * sp] != b->h_pairs[2 * tp + 1]) return YV_ERR_INVALID;  // stereo query = temporal train
        }
    }
    for (int i = 0; i < 9 && n_tracks > 0; ++i)
        if (!std::isfinite(K[i])) return YV_ERR_INVALID;
    if (n_tracks > 0 && !finite_pose(T_right)) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = b->ctx->stream;
    if (b->bstream) YV_HIP(hipStreamSynchronize(b->bstream));  // a build in flight reads tracks / K
    b->build_pending = false;
    if (drain_records(b) != YV_OK) return YV_ERR_HIP;  // (as every call that drains the build)
    if (b->side) YV_HIP(hipStreamSynchronize(b->side));  // an LM in flight reads tracks / K
    if (n_tracks > b->max_tracks) {
        YV_HIP(hipStreamSynchronize(s));
        if (b->side) YV_HIP(hipStreamSynchronize(b->side));
        b->track_mem.clear();
        b->max_tracks = 0;
        b->n_tracks = 0;
        const size_t nt = (size_t)n_tracks, nk = (size_t)b->max_kp;
        int rc = YV_OK;
        rc |= b->track_mem.alloc(&b->tracks, 2 * nt);
        rc |= b->track_mem.alloc(&b->track_K, 9 * nt);
        rc |= b->track_mem.alloc(&b->T_right, 7);
        rc |= b->track_mem.alloc(&b->edge_X, kEdgeBufs * 3 * nt * nk);
        rc |= b->track_mem.alloc(&b->edge_uv, kEdgeBufs * 2 * nt * nk);
        rc |= b->track_mem.alloc(&b->edge_query, kEdgeBufs * nt * nk);
        rc |= b->track_mem.alloc(&b->edge_count, kEdgeBufs * nt);
        rc |= b->track_mem.alloc(&b->edge_outlier, kEdgeBufs * nt * nk);
        rc |= b->track_mem.alloc(&b->track_inliers, kEdgeBufs * nt);
        rc |= b->track_mem.alloc(&b->lk_sp, nt);
        rc |= b->track_mem.alloc(&b->lk_pairs, 2 * nt);
        rc |= b->track_mem.alloc(&b->lk_X, 2 * 3 * nt * nk);
        rc |= b->track_mem.alloc(&b->lk_pts, 2 * 2 * nt * nk);
        rc |= b->track_mem.alloc(&b->lk_next, 2 * nt * nk);
        rc |= b->track_mem.alloc(&b->lk_err, nt * nk);
        rc |= b->track_mem.alloc(&b->lk_status, nt * nk);
        rc |= b->track_mem.alloc(&b->lk_q, 2 * nt * nk);
        rc |= b->track_mem.alloc(&b->lk_count, 2 * nt);
        b->lk_ev_pending[0] = b->lk_ev_pending[1] = false;
        if (rc != YV_OK) return YV_ERR_HIP;
        b->max_tracks = n_tracks;
        rc = ensure_ransac(b);  // (the streams a track runs on were drained above)
        if (rc != YV_OK) return rc;
    }
    if (n_tracks > 0) {
        std::vector<double> Ks(9 * (size_t)n_tracks);
        for (int t = 0; t < n_tracks; ++t) std::memcpy(&Ks[9 * (size_t)t], K, 9 * sizeof(double));
        YV_HIP(hipMemcpyAsync(b->tracks, tracks, 2 * sizeof(int32_t) * (size_t)n_tracks, hipMemcpyHostToDevice, s));
        YV_HIP(hipMemcpyAsync(b->track_K, Ks.data(), Ks.size() * sizeof(double), hipMemcpyHostToDevice, s));
        YV_HIP(hipMemcpyAsync(b->T_right, T_right, 7 * sizeof(double), hipMemcpyHostToDevice, s));
        YV_HIP(hipMemsetAsync(b->edge_count, 0, kEdgeBufs * sizeof(int32_t) * (size_t)b->max_tracks, s));
        if (b->lk_step > 0) {
            std::vector<int32_t> sp(n_tracks), lp(2 * (size_t)n_tracks);
            for (int t = 0; t < n_tracks; ++t) {
                sp[t] = tracks[2 * t];
                lp[2 * t] = b->h_pairs[2 * sp[t]] / b->lk_step;
                lp[2 * t + 1] = tracks[2 * t + 1] / b->lk_step;
            }
            YV_HIP(hipMemcpyAsync(b->lk_sp, sp.data(), sizeof(int32_t) * sp.size(), hipMemcpyHostToDevice, s));
            YV_HIP(hipMemcpyAsync(b->lk_pairs, lp.data(), sizeof(int32_t) * lp.size(), hipMemcpyHostToDevice, s));
        }
        YV_HIP(hipStreamSynchronize(s));
    }
    b->n_tracks = n_tracks;
    return YV_OK;
}

int yv_batch_track(yv_batch* b, const double* d_priors, double* d_poses, void* stream) {
    return batch_track(b, d_priors, d_poses, stream, nullptr);
}

int yv_batch_track_map(yv_batch* b, const double* d_priors, double* d_poses, int64_t first_frame, int kf_every,
                       void* d_block, int max_kf, void* stream) {
    if (!b || !d_block || kf_every < 1 || max_kf < 1 || first_frame < 0) return YV_ERR_INVALID;
    const MapArgs m{first_frame, kf_every, max_kf, d_block};
    return batch_track(b, d_priors, d_poses, stream, &m);
}

int yv_batch_map_wait(yv_batch* b, void* stream) {
    if (!b || !stream) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    if (flush_deferred(b) != YV_OK) return YV_ERR_HIP;  // the block is written after the LM
    if (!b->map_written) return YV_OK;
    YV_HIP(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), b->ev_map, 0));
    return YV_OK;
}

int yv_batch_map_release(yv_batch* b, void* stream) {
    if (!b || !stream) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    if (!b->ev_map_release) YV_HIP(b->mem.event(&b->ev_map_release));
    YV_HIP(hipEventRecord(b->ev_map_release, reinterpret_cast<hipStream_t>(stream)));
    b->map_release_pending = true;
    return YV_OK;
}

int yv_batch_set_track_overlap(yv_batch* b, int on) {
    if (!b || on < 0 || on > 4) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    if (flush_deferred(b) != YV_OK) return YV_ERR_HIP;
    if (on && !b->side) {
        // lowest priority: the LM fills the CUs the next batch's detect / describe / match leave idle
        int least = 0, greatest = 0;
        YV_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        YV_HIP(hipStreamCreateWithPriority(&b->side, hipStreamNonBlocking, least));
        b->mem.adopt(b->side);
        for (int k = 0; k < kEdgeBufs; ++k) {
            YV_HIP(b->mem.event(&b->ev_edges[k]));
            YV_HIP(b->mem.event(&b->ev_lm[k]));
        }
        // the build stream at the default priority (the highest and the lowest measured the same)
        YV_HIP(hipStreamCreateWithFlags(&b->bstream, hipStreamNonBlocking));
        b->mem.adopt(b->bstream);
        YV_HIP(b->mem.event(&b->ev_fin));
        YV_HIP(b->mem.event(&b->ev_built));
        // the records stream on a hardware queue of its own: a fifth plain stream would share one of the four queues,
        // and on the context stream's the records would run in order after all (see yv_side_stream)
        b->rstream = make_queue_stream(b->ctx);
        if (!b->rstream) return YV_ERR_HIP;
        b->mem.adopt(b->rstream);
        YV_HIP(b->mem.event(&b->ev_keys));
        YV_HIP(b->mem.event(&b->ev_records));
    }
    if (!on && b->bstream) YV_HIP(hipStreamSynchronize(b->bstream));
    if (!on) b->build_pending = false;
    if (!on && drain_records(b) != YV_OK) return YV_ERR_HIP;
    {
        const char* e = std::getenv("YAVO_BUILD_ASYNC");
        b->build_async = on != 0 && !(e && e[0] == '0');
    }
    if (!on && b->side) YV_HIP(hipStreamSynchronize(b->side));
    b->overlap = on != 0;
    b->overlap_mode = on;
    return YV_OK;
}

int yv_batch_track_sync(yv_batch* b) {
    if (!b) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    if (flush_deferred(b) != YV_OK) return YV_ERR_HIP;
    if (b->bstream) YV_HIP(hipStreamSynchronize(b->bstream));
    if (b->side) YV_HIP(hipStreamSynchronize(b->side));
    return drain_records(b);  // the last run's match and filtered lists are complete
}

int yv_batch_records_wait(yv_batch* b, void* stream) {
    if (!b || !stream) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    // (the flag stays: the next writer of the keypoints still joins on its own stream)
    if (b->records_pending) YV_HIP(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), b->ev_records, 0));
    return YV_OK;
}

int yv_batch_set_track_ransac(yv_batch* b, int iters, double thr, int min_inliers, const uint32_t* draws) {
    if (!b || iters < 0) return YV_ERR_INVALID;
    if (iters > 0 && (iters > yavo::kPnpMaxIters || min_inliers < 4 || !std::isfinite(thr) || !(thr > 0) || !draws))
        return YV_ERR_INVALID;
    if (iters == 0 && b->ransac_iters == 0) return YV_OK;  // off stays off: nothing to wait for
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    // a deferred LM belongs to the mode it was issued in; a track in flight, on whichever stream the caller named,
    // reads the draws and the workspace
    if (flush_deferred(b) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipDeviceSynchronize());
    if (iters == 0) {
        b->ransac_iters = 0;
        return YV_OK;
    }
    if (!b->ransac_draws && b->mem.alloc(&b->ransac_draws, 3 * (size_t)yavo::kPnpMaxIters) != YV_OK)
        return YV_ERR_HIP;
    YV_HIP(hipMemcpyAsync(b->ransac_draws, draws, sizeof(uint32_t) * 3 * (size_t)iters, hipMemcpyHostToDevice,
                          b->ctx->stream));
    YV_HIP(hipStreamSynchronize(b->ctx->stream));
    b->ransac_iters = iters;
    b->ransac_thr = thr;
    b->ransac_min = min_inliers;
    const int rc = ensure_ransac(b);
    if (rc != YV_OK) b->ransac_iters = 0;
    return rc;
}

int yv_batch_ransac_view_get(yv_batch* b, yv_batch_ransac_view* v) {
    if (!b || !v || b->ransac_iters == 0 || b->ransac_tracks == 0) return YV_ERR_INVALID;
    const RansacSlice r = ransac_slice(b, b->tbuf);
    v->n_tracks = b->n_tracks;
    v->pose = r.pose;
    v->inlier = r.inlier;
    v->inliers = r.inliers;
    v->found = r.found;
    return YV_OK;
}

int yv_batch_set_track_lk(yv_batch* b, int image_step, int win, int max_level, int max_count, double eps,
                          double min_eig) {
    if (!b || image_step < 0 || (image_step > 0 && (win < 3 || win > 22 || max_level < 0))) return YV_ERR_INVALID;
    if (set_device(b->ctx) != YV_OK) return YV_ERR_HIP;
    if (flush_deferred(b) != YV_OK) return YV_ERR_HIP;
    if (b->side) YV_HIP(hipStreamSynchronize(b->side));
    if (b->bstream) YV_HIP(hipStreamSynchronize(b->bstream));  // an edge build in flight (as its siblings drain)
    b->build_pending = false;
    if (drain_records(b) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipStreamSynchronize(b->ctx->stream));
    if (b->lk) {
        yv_lk_destroy(b->lk);
        b->lk = nullptr;
    }
    b->lk_step = image_step;
    b->n_tracks = 0;  // tracks change meaning with the mode: set them again
    if (image_step == 0) return YV_OK;
    const int slots = (b->max_images + image_step - 1) / image_step;
    const int rc = yv_lk_create(b->ctx, slots, b->H, b->W, win, max_level, &b->lk);
    if (rc != YV_OK) {
        b->lk_step = 0;
        return rc;
    }
    b->lk_max_count = max_count;
    b->lk_eps = eps;
    b->lk_min_eig = min_eig;
    return YV_OK;
}

}  // extern "C"
