// yavo_geom_host.hip -- the geometry entry points of the C ABI (include/yavo/yavo_geom.h) on host pointers (through
// the context's arena, yavo_host.h) and on device buffers.  Host code only; kernels live in yavo_geom.hip.
#include "yavo_host.h"

using namespace yavo;

extern "C" {

int yv_f_ransac(yv_ctx* ctx, const yv_match* m, int n, const int32_t* samples, int iters, double thr, double F[9],
                int* max_inliers, int* found) {
    if (!ctx || !F || !max_inliers || !found || n < 0 || iters < 0 || (n > 0 && !m) || (iters > 0 && !samples))
        return YV_ERR_INVALID;
    if (n > yavo::kMaxKp) return YV_ERR_CAPACITY;
    *found = 0;
    if (n < 8) return YV_OK;  // "Not enough matches": false, F untouched (src/3DHandler.cc:154-156)
    for (int i = 0; i < 8 * iters; ++i)
        if (samples[i] < 0 || samples[i] >= n) return YV_ERR_INVALID;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    Arena a{ctx};
    yv_match* dm;
    int32_t *dcnt, *dsmp, *dmax, *dfound;
    double* dF;
    uint8_t* dws;
    a.add(&dm, (size_t)n);  // every hypothesis' count reads the whole list: on the device
    a.add(&dws, yavo::f_ransac_ws_bytes(1, iters));
    a.add_host(&dcnt, 1);
    a.add_host(&dsmp, (size_t)std::max(8 * iters, 1));
    a.add_host(&dF, 9);
    a.add_host(&dmax, 1);
    a.add_host(&dfound, 1);
    if (a.commit() != YV_OK) return YV_ERR_HIP;
    a.in(dm, m, sizeof(yv_match) * (size_t)n);
    a.in(dcnt, &n, sizeof(int32_t));
    if (iters > 0) a.in(dsmp, samples, sizeof(int32_t) * 8 * (size_t)iters);
    a.in(dF, F, sizeof(double) * 9);  // untouched if iters == 0
    YV_HIP(a.upload(s));
    yavo::launch_f_ransac(dm, n, dcnt, 1, dsmp, 8 * (int64_t)iters, iters, thr, dF, dmax, dfound, dws, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    a.out(F, dF, sizeof(double) * 9);
    a.out(max_inliers, dmax, sizeof(int32_t));
    a.out(found, dfound, sizeof(int32_t));
    YV_HIP(a.fetch(s));
    return YV_OK;
}

int yv_triangulate(yv_ctx* ctx, const double pose_a[7], const double pose_b[7], const double K[9], const yv_match* m,
                   int n, double* Xw, uint8_t* ok, int* n_ok) {
    return yv_triangulate_subpix(ctx, pose_a, pose_b, K, m, nullptr, n, Xw, ok, n_ok);
}

int yv_triangulate_subpix(yv_ctx* ctx, const double pose_a[7], const double pose_b[7], const double K[9],
                          const yv_match* m, const int32_t* dcol_q8, int n, double* Xw, uint8_t* ok, int* n_ok) {
    if (!ctx || !pose_a || !pose_b || !K || !n_ok || n < 0 || (n > 0 && (!m || !Xw || !ok))) return YV_ERR_INVALID;
    *n_ok = 0;
    if (n == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    Arena a{ctx};
    yv_match* dm;
    double *dposes, *dK, *dX;
    uint8_t* dok;
    int32_t* ddq = nullptr;
    // every record, pose and output is read or written once: all in the pinned mirror, no DMA
    a.add_host(&dm, (size_t)n);
    if (dcol_q8) a.add_host(&ddq, (size_t)n);
    a.add_host(&dposes, 14);
    a.add_host(&dK, 9);
    a.add_host(&dX, 3 * (size_t)n);
    a.add_host(&dok, (size_t)n);
    if (a.commit() != YV_OK) return YV_ERR_HIP;
    a.in(dm, m, sizeof(yv_match) * (size_t)n);
    a.in(dposes, pose_a, sizeof(double) * 7);
    a.in(dposes + 7, pose_b, sizeof(double) * 7);
    a.in(dK, K, sizeof(double) * 9);
    if (dcol_q8) a.in(ddq, dcol_q8, sizeof(int32_t) * (size_t)n);
    yavo::launch_triangulate(dm, n, dposes, dK, dX, dok, nullptr, s, ddq);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    a.out(Xw, dX, sizeof(double) * 3 * (size_t)n);
    a.out(ok, dok, (size_t)n);
    YV_HIP(a.fetch(s));
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += ok[i] ? 1 : 0;
    *n_ok = cnt;
    return YV_OK;
}

int yv_world2camera(yv_ctx* ctx, const double* X, int n, const double pose[7], const double K[9], double* out) {
    if (!ctx || !pose || !K || n < 0 || (n > 0 && (!X || !out))) return YV_ERR_INVALID;
    if (n == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    Arena a{ctx};
    double *dX, *dT, *dK, *dO;
    // one read and one write per point: all in the pinned mirror, no DMA
    a.add_host(&dX, 3 * (size_t)n);
    a.add_host(&dT, 7);
    a.add_host(&dK, 9);
    a.add_host(&dO, 3 * (size_t)n);
    if (a.commit() != YV_OK) return YV_ERR_HIP;
    a.in(dX, X, sizeof(double) * 3 * (size_t)n);
    a.in(dT, pose, sizeof(double) * 7);
    a.in(dK, K, sizeof(double) * 9);
    yavo::launch_world2camera(dX, n, dT, dK, dO, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    a.out(out, dO, sizeof(double) * 3 * (size_t)n);
    YV_HIP(a.fetch(s));
    return YV_OK;
}

static int pose_single(yv_ctx* ctx, const double* X, const double* uv, int n, const double* K, double* pose,
                       uint8_t* outlier, int* result, bool lm) {
    if (!ctx || !K || !pose || !result || n < 0 || (n > 0 && (!X || !uv)) || (lm && n > 0 && !outlier))
        return YV_ERR_INVALID;
    if (n > 4096) return YV_ERR_CAPACITY;
    if (!finite_pose(pose)) return YV_ERR_INVALID;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    Arena a{ctx};
    int32_t *doff, *dres;
    double *dX, *duv, *dK, *dP;
    uint8_t* dout;
    a.add(&dX, 3 * (size_t)std::max(n, 1));  // read by every pass: on the device
    a.add(&duv, 2 * (size_t)std::max(n, 1));
    a.add_host(&doff, 2);                      // read once, or written once: in the pinned mirror
    a.add_host(&dK, 9);
    a.add_host(&dP, 7);
    a.add_host(&dout, (size_t)std::max(n, 1));
    a.add_host(&dres, 1);
    if (a.commit() != YV_OK) return YV_ERR_HIP;
    const int32_t off2[2] = {0, n};
    a.in(doff, off2, 2 * sizeof(int32_t));
    if (n > 0) {
        a.in(dX, X, sizeof(double) * 3 * (size_t)n);
        a.in(duv, uv, sizeof(double) * 2 * (size_t)n);
    }
    a.in(dK, K, sizeof(double) * 9);
    a.in(dP, pose, sizeof(double) * 7);
    YV_HIP(a.upload(s));
    if (lm) yavo::launch_pose_lm(doff, 1, dX, duv, dK, dP, dout, dres, s);
    else yavo::launch_pose_gn(doff, 1, dX, duv, dK, dP, dres, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    a.out(pose, dP, sizeof(double) * 7);
    if (lm && n > 0) a.out(outlier, dout, (size_t)n);
    a.out(result, dres, sizeof(int32_t));
    YV_HIP(a.fetch(s));
    return YV_OK;
}

int yv_pose_lm(yv_ctx* ctx, const double* X, const double* uv, int n, const double K[9], double pose[7],
               uint8_t* outlier, int* inliers) {
    return pose_single(ctx, X, uv, n, K, pose, outlier, inliers, true);
}

int yv_pose_gn(yv_ctx* ctx, const double* X, const double* uv, int n, const double K[9], double pose[7],
               int* iterations) {
    return pose_single(ctx, X, uv, n, K, pose, nullptr, iterations, false);
}

int yv_pose_lm_batch(yv_ctx* ctx, int n_problems, const int32_t* d_offsets, const double* d_X, const double* d_uv,
                     const double* d_K, double* d_poses, uint8_t* d_outlier, int32_t* d_inliers, void* stream) {
    if (!ctx || n_problems < 0 || (n_problems > 0 && (!d_offsets || !d_X || !d_uv || !d_K || !d_poses || !d_outlier ||
                                                      !d_inliers)))
        return YV_ERR_INVALID;
    if (n_problems == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
    yavo::launch_pose_lm(d_offsets, n_problems, d_X, d_uv, d_K, d_poses, d_outlier, d_inliers, s);
    return check_launch();
}

int yv_pose_gn_batch(yv_ctx* ctx, int n_problems, const int32_t* d_offsets, const double* d_X, const double* d_uv,
                     const double* d_K, double* d_poses, int32_t* d_iterations, void* stream) {
    if (!ctx || n_problems < 0 ||
        (n_problems > 0 && (!d_offsets || !d_X || !d_uv || !d_K || !d_poses || !d_iterations)))
        return YV_ERR_INVALID;
    if (n_problems == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
    yavo::launch_pose_gn(d_offsets, n_problems, d_X, d_uv, d_K, d_poses, d_iterations, s);
    return check_launch();
}

int yv_f_ransac_batch(yv_ctx* ctx, const yv_match* d_matches, int64_t list_stride, const int32_t* d_counts, int n_lists,
                      const int32_t* d_samples, int64_t sample_stride, int iters, double thr, double* d_F,
                      int32_t* d_max_inliers, int32_t* d_found, void* stream) {
    if (!ctx || n_lists < 0 || iters < 0 ||
        (n_lists > 0 && (!d_matches || !d_counts || !d_samples || !d_F || !d_max_inliers || !d_found)))
        return YV_ERR_INVALID;
    if (n_lists == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
    const size_t need = yavo::f_ransac_ws_bytes(n_lists, iters);
    if (need > ctx->fr_ws_cap) {  // grown outside any timed loop; earlier launches that use it have finished
        YV_HIP(hipDeviceSynchronize());
        ctx->mem.release(ctx->fr_ws);
        ctx->fr_ws_cap = 0;
        if (ctx->mem.alloc(&ctx->fr_ws, need) != YV_OK) return YV_ERR_HIP;
        ctx->fr_ws_cap = need;
    }
    yavo::launch_f_ransac(d_matches, list_stride, d_counts, n_lists, d_samples, sample_stride, iters, thr, d_F,
                          d_max_inliers, d_found, ctx->fr_ws, s);
    return check_launch();
}

// what both P3P-RANSAC entry points check before they look at the context
static int pnp_args_check(int iters, double thr, int min_inliers) {
    if (iters < 1 || iters > yavo::kPnpMaxIters || min_inliers < 4 || !std::isfinite(thr) || !(thr > 0))
        return YV_ERR_INVALID;
    return YV_OK;
}

int yv_pnp_ransac(yv_ctx* ctx, const double* X, const double* uv, int n, const double K[9], const uint32_t* draws,
                  int iters, double thr, int min_inliers, double pose[7], uint8_t* inlier, int* inliers, int* found) {
    if (!K || !draws || !pose || !inliers || !found || n < 0 || (n > 0 && (!X || !uv || !inlier)))
        return YV_ERR_INVALID;
    if (pnp_args_check(iters, thr, min_inliers) != YV_OK) return YV_ERR_INVALID;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return YV_ERR_INVALID;
    if (n > 4096) return YV_ERR_CAPACITY;
    if (!ctx) return YV_ERR_INVALID;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    Arena a{ctx};
    int32_t *doff, *dinl, *dfound;
    uint32_t* ddraws;
    double *dX, *duv, *dK, *dP;
    uint8_t *dmask, *dws;
    a.add(&dX, 3 * (size_t)std::max(n, 1));  // read by every candidate's count: on the device
    a.add(&duv, 2 * (size_t)std::max(n, 1));
    a.add(&dws, yavo::pnp_ransac_ws_bytes(1, iters));
    a.add_host(&doff, 2);  // read once, or written once: in the pinned mirror
    a.add_host(&ddraws, 3 * (size_t)iters);
    a.add_host(&dK, 9);
    a.add_host(&dP, 7);
    a.add_host(&dmask, (size_t)std::max(n, 1));
    a.add_host(&dinl, 1);
    a.add_host(&dfound, 1);
    if (a.commit() != YV_OK) return YV_ERR_HIP;
    const int32_t off2[2] = {0, n};
    a.in(doff, off2, 2 * sizeof(int32_t));
    if (n > 0) {
        a.in(dX, X, sizeof(double) * 3 * (size_t)n);
        a.in(duv, uv, sizeof(double) * 2 * (size_t)n);
    }
    a.in(ddraws, draws, sizeof(uint32_t) * 3 * (size_t)iters);
    a.in(dK, K, sizeof(double) * 9);
    a.in(dP, pose, sizeof(double) * 7);  // untouched when nothing is found
    YV_HIP(a.upload(s));
    yavo::launch_pnp_ransac(doff, nullptr, 0, 1, dX, duv, dK, ddraws, iters, thr, min_inliers, nullptr, dP, dmask,
                            dinl, dfound, dws, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    a.out(pose, dP, sizeof(double) * 7);
    if (n > 0) a.out(inlier, dmask, (size_t)n);
    a.out(inliers, dinl, sizeof(int32_t));
    a.out(found, dfound, sizeof(int32_t));
    YV_HIP(a.fetch(s));
    return YV_OK;
}

int yv_pnp_ransac_batch(yv_ctx* ctx, int n_problems, const int32_t* d_offsets, const double* d_X, const double* d_uv,
                        const double* d_K, const uint32_t* d_draws, int iters, double thr, int min_inliers,
                        double* d_poses, uint8_t* d_inlier, int32_t* d_inliers, int32_t* d_found, void* stream) {
    if (n_problems < 0 || (n_problems > 0 && (!d_offsets || !d_X || !d_uv || !d_K || !d_draws || !d_poses ||
                                              !d_inlier || !d_inliers || !d_found)))
        return YV_ERR_INVALID;
    if (pnp_args_check(iters, thr, min_inliers) != YV_OK) return YV_ERR_INVALID;
    if (n_problems > 65535) return YV_ERR_CAPACITY;
    if (!ctx) return YV_ERR_INVALID;
    if (n_problems == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
    const size_t need = yavo::pnp_ransac_ws_bytes(n_problems, iters);
    if (need > ctx->pnp_ws_cap) {  // grown outside any timed loop; earlier launches that use it have finished
        YV_HIP(hipDeviceSynchronize());
        ctx->mem.release(ctx->pnp_ws);
        ctx->pnp_ws_cap = 0;
        if (ctx->mem.alloc(&ctx->pnp_ws, need) != YV_OK) return YV_ERR_HIP;
        ctx->pnp_ws_cap = need;
    }
    yavo::launch_pnp_ransac(d_offsets, nullptr, 0, n_problems, d_X, d_uv, d_K, d_draws, iters, thr, min_inliers,
                            nullptr, d_poses, d_inlier, d_inliers, d_found, ctx->pnp_ws, s);
    return check_launch();
}

// Test entry point (tests/test_gpu_pose_degenerate.py; like yv_debug_xlane not part of the public headers): the batch's
// track LM alone (launch_track_pose: the fixed-stride layout, track t owns d_counts[t] edges from t * stride) on device
// buffers; d_priors [n][7] is read, d_poses [n][7] written.
int yv_debug_track_pose(yv_ctx* ctx, int n_tracks, const int32_t* d_counts, int stride, const double* d_X,
                        const double* d_uv, const double* d_K, const double* d_priors, double* d_poses,
                        uint8_t* d_outlier, int32_t* d_inliers, void* stream) {
    if (!ctx || n_tracks <= 0 || stride < 0 || !d_counts || !d_X || !d_uv || !d_K || !d_priors || !d_poses ||
        !d_outlier || !d_inliers)
        return YV_ERR_INVALID;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
    yavo::launch_track_pose(n_tracks, d_counts, stride, d_X, d_uv, d_K, d_priors, d_poses, d_outlier, d_inliers, s);
    return check_launch();
}

}  // extern "C"
