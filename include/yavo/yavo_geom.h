/*
 * yavo_geom.h -- geometry rows of the hot path behind the same C ABI as yavo.h.
 *
 * Poses are Sophus::SE3d (T_cw, world -> camera) in SE3d::data() layout:
 *     pose[7] = {qx, qy, qz, qw, tx, ty, tz}
 * so a reference Frame::pose (include/Frame.hpp:13) crosses as pose.data().  K is the row-major 3x3
 * intrinsic matrix (Camera::K, include/Utils.hpp:30-70).  Image measurements are the reference's
 * KeyPoint convention (x = row, y = column).  Conventions and errors as in yavo.h.
 */
#ifndef YAVO_GEOM_H
#define YAVO_GEOM_H

#include <stdint.h>

#include "yavo_types.h"

#ifdef __cplusplus
extern "C" {
#endif

struct yv_ctx;

/* _3DHandler::getFRANSAC (src/3DHandler.cc:145-195; include/3DHandler.hpp:58): `iters` hypotheses, each the
 * normalised 8-point F (getFundamentalMatrix, :50-142) of samples[8*h .. 8*h+7] (indices into m, drawn with
 * replacement -- the reference draws them from std::random_device), inliers |p2^T F p1| < thr in raw
 * (row, col, 1) pixels; the first hypothesis with the most inliers wins.  *found = 0 (F untouched) when
 * n < 8 (the reference returns false).  n <= 4096. */
int yv_f_ransac(struct yv_ctx* ctx, const yv_match* m, int n, const int32_t* samples, int iters, double thr,
                double F[9], int* max_inliers, int* found);

/* triangulate2View's per-match work (src/LoopHandler.cc:658-726): pixel2camera of pt1 / pt2 (:908-915),
 * LoopHandler::triangulation with the two poses (:867-885, DLT + SVD, success iff s4/s3 < 1e-2), accepted iff
 * success and Z > 0.  Xw [n][3], ok [n], *n_ok = accepted count. */
int yv_triangulate(struct yv_ctx* ctx, const double pose_a[7], const double pose_b[7], const double K[9],
                   const yv_match* m, int n, double* Xw, uint8_t* ok, int* n_ok);

/* yv_triangulate from refined right columns (yv_stereo_subpix, yavo.h): record i's pt2 enters pixel2camera with the
 * column (double)pt2.y + (double)dcol_q8[i] * (1.0 / 256.0) in place of (double)pt2.y, everything else operation for
 * operation as in yv_triangulate.  dcol_q8 == NULL is exactly yv_triangulate. */
int yv_triangulate_subpix(struct yv_ctx* ctx, const double pose_a[7], const double pose_b[7], const double K[9],
                          const yv_match* m, const int32_t* dcol_q8, int n, double* Xw, uint8_t* ok, int* n_ok);

/* Frame::world2Camera (src/Frame.cc:16-28): out[i] = K [R|t] [X_i; 1] (unnormalised). */
int yv_world2camera(struct yv_ctx* ctx, const double* X, int n, const double pose[7], const double K[9],
                    double* out);

/* LoopHandler::optimizePoseOnly (src/LoopHandler.cc:730-861) with the g2o edge of include/Optimizer.hpp:40-135:
 * pose-only Levenberg-Marquardt from the prior `pose`, 4 rounds x optimize(10), Huber(1) kernel (removed after
 * round 3), chi2 > 5.991 -> outlier.  X [n][3] world points, uv [n][2] measurements (kp.x, kp.y).  pose is
 * updated in place; outlier [n] = final flags; *inliers = n - outliers.  n <= 4096 (YV_ERR_CAPACITY past it); a prior
 * with a NaN or infinite entry is YV_ERR_INVALID (yv_pose_gn the same). */
int yv_pose_lm(struct yv_ctx* ctx, const double* X, const double* uv, int n, const double K[9], double pose[7],
               uint8_t* outlier, int* inliers);

/* bundleAdjustmentGaussNewton (src/test.cc:172-244): 10 Gauss-Newton iterations, stop on cost increase or
 * |dx| < 1e-6.  *iterations = accepted updates. */
int yv_pose_gn(struct yv_ctx* ctx, const double* X, const double* uv, int n, const double K[9], double pose[7],
               int* iterations);

/* Batched device-pointer forms (asynchronous on `stream`, NULL = context stream).  Problem p owns edges
 * [d_offsets[p], d_offsets[p+1]) of d_X [][3] / d_uv [][2]; d_K [p][9]; d_poses [p][7] in/out.
 * yv_pose_lm_batch solves a problem of more than 4096 edges on its first 4096 alone (no error: the call does not see
 * the offsets): the pose and d_outlier flags are those of that shorter problem, d_inliers[p] = 4096 - its outliers,
 * and the problem's d_outlier bytes past the first 4096 are left untouched.  Priors, points and measurements are not
 * checked: non-finite ones give the reference's result on them (usually the prior back, or a NaN pose). */
int yv_pose_lm_batch(struct yv_ctx* ctx, int n_problems, const int32_t* d_offsets, const double* d_X,
                     const double* d_uv, const double* d_K, double* d_poses, uint8_t* d_outlier,
                     int32_t* d_inliers, void* stream);
/* The order in which the pose-LM kernel sums over edges, as the oracle's sum_mode (oracle/yavo_oracle.h:
 * 4 / 5 / 6 / 7 = 64- / 128- / 256- / 512-thread workgroups). yv_lm_sum_mode: the track LM of a batch of more than
 * 256 tracks (256 threads). yv_track_lm_sum_mode(n): the track LM of a batch of n tracks (yv_batch_create's
 * n_tracks; 512 threads up to 256 tracks, 256 above). yv_pose_lm_sum_mode(n): yv_pose_lm (n = 1) and
 * yv_pose_lm_batch with n problems (the same rule: with few problems the call's latency is set by one problem per
 * CU). Results are bit-identical to the oracle in that order and within 1e-9 of the reference's sequential order. */
int yv_lm_sum_mode(void);
int yv_track_lm_sum_mode(int n_tracks);
int yv_pose_lm_sum_mode(int n_problems);
int yv_pose_gn_batch(struct yv_ctx* ctx, int n_problems, const int32_t* d_offsets, const double* d_X,
                     const double* d_uv, const double* d_K, double* d_poses, int32_t* d_iterations, void* stream);
/* F-RANSAC over n_lists match lists: list l = d_matches + l*list_stride, d_counts[l] entries, samples
 * d_samples + l*sample_stride ([iters][8]).  The hypothesis F / inlier-count workspace belongs to the context
 * (one per yv_ctx), so calls on one context must be serialised even when they name different streams: run
 * concurrent F-RANSAC batches on separate contexts (the LoopHandler's side lane does).  Growing the workspace
 * synchronises the device. */
int yv_f_ransac_batch(struct yv_ctx* ctx, const yv_match* d_matches, int64_t list_stride, const int32_t* d_counts,
                      int n_lists, const int32_t* d_samples, int64_t sample_stride, int iters, double thr,
                      double* d_F, int32_t* d_max_inliers, int32_t* d_found, void* stream);

/* ---- P3P-RANSAC absolute pose (opt-in, beyond the reference: it has no solvePnPRansac) ----
 * A pose from 3D-2D edges without a prior, and its inlier mask: `iters` hypotheses, hypothesis h from the edges
 * draws[3 h + k] % n (two equal indices: no candidate), Grunert's P3P (up to 4 poses each), an edge an inlier of a pose
 * iff its camera-frame z > 0 and the pose LM's edge error e has e0^2 + e1^2 < thr^2 (pixels); the pose with the most
 * inliers wins, ties to the lowest hypothesis, then the lowest root.  *found = 1 iff that count >= min_inliers; otherwise
 * pose is left untouched, inlier [n] is zero and *inliers = 0.  X, uv, K and pose as in yv_pose_lm, so the pose feeds it
 * as the prior.  Bit-identical to tests/pnp_ransac_reference.py, which fixes the order of every operation.
 * n <= 4096 (YV_ERR_CAPACITY past it), 1 <= iters <= 1024, min_inliers >= 4 (three points fit every candidate), thr
 * finite and > 0, K finite: anything else is YV_ERR_INVALID, checked before the context. */
int yv_pnp_ransac(struct yv_ctx* ctx, const double* X, const double* uv, int n, const double K[9],
                  const uint32_t* draws, int iters, double thr, int min_inliers, double pose[7], uint8_t* inlier,
                  int* inliers, int* found);
/* The batched device-pointer form in yv_pose_lm_batch's layout (d_poses [p][7] in / out feeds it directly as priors;
 * d_inlier by edge like d_outlier; d_draws [iters][3] serves every problem).  A problem of more than 4096 edges is
 * solved on its first 4096 and its d_inlier bytes past them are left untouched.  n_problems <= 65535.  The hypothesis
 * workspace belongs to the context: calls on one context must be serialised (as yv_f_ransac_batch); growing it
 * synchronises the device. */
int yv_pnp_ransac_batch(struct yv_ctx* ctx, int n_problems, const int32_t* d_offsets, const double* d_X,
                        const double* d_uv, const double* d_K, const uint32_t* d_draws, int iters, double thr,
                        int min_inliers, double* d_poses, uint8_t* d_inlier, int32_t* d_inliers, int32_t* d_found,
                        void* stream);

/* ---- cv::calcOpticalFlowPyrLK (src/LoopHandler.cc:372-375) ---------------------------
 * Restates OpenCV's pyramidal LK (flags 0: no initial flow) -- pyrDown pyramid (levels stop when the next one
 * would be <= win), Scharr derivatives, 14-bit bilinear windows, minEig test, Newton steps with the eps^2 and
 * oscillation tests, the level-0 error.  Points are cv::Point2f (x = column, y = row).  Window sums use the
 * GPU order of oracle/yavo_oracle_lk.c (sum_mode 1).
 * Any float is a valid point coordinate.  A point with a coordinate that is NaN, infinite or beyond +-2^31 is
 * rejected like one whose window lies outside the image, as OpenCV's x86 build does (cvFloor gives INT_MIN there):
 * status 0, err 0, next point = the input (NaN stays NaN), and nothing is read at it.
 * Any H, W >= 1 is a valid image size, also below the window: image pixels are REFLECT_101 at any distance
 * (cv::borderInterpolate's period 2 len - 2). */
typedef struct yv_lk yv_lk;
/* Workspace for up to max_images H x W images: pyramids and derivatives.  3 <= win <= 22, 0 <= max_level <= 7;
 * anything else is YV_ERR_INVALID. */
int yv_lk_create(struct yv_ctx* ctx, int max_images, int H, int W, int win, int max_level, yv_lk** out);
void yv_lk_destroy(yv_lk* lk);
/* Levels actually used (buildOpticalFlowPyramid's return value). */
int yv_lk_levels(const yv_lk* lk);
/* Pyramids + derivatives of n_images device images (image i at d_images + i*image_pitch, rows `stride`
 * apart).  The images must stay valid until the last yv_lk_track_batch that reads them has completed. */
int yv_lk_build(yv_lk* lk, const uint8_t* d_images, int n_images, int stride, int64_t image_pitch, void* stream);
/* Level `level` (0 .. yv_lk_levels) of image `image` of the last yv_lk_build, as cv::buildOpticalFlowPyramid
 * would hand it over without derivatives interleaved: the level image (*d_img, rows *img_stride bytes apart;
 * level 0 is the caller's image; valid until the next yv_lk_build / yv_lk_destroy, after the build's stream work)
 * and its Scharr derivatives (*d_deriv, (dx, dy) int16 pairs, rows *deriv_stride pairs apart; computed on the
 * context stream and complete on return, valid until the next yv_lk_level), size *H x *W.  The tracker itself
 * computes derivatives inside its windows and keeps no derivative pyramid. */
int yv_lk_level(yv_lk* lk, int image, int level, const uint8_t** d_img, int* img_stride, const int16_t** d_deriv,
                int* deriv_stride, int* H, int* W);
/* Track d_counts[p] points of pair p (prev image d_pairs[2p], next image d_pairs[2p+1], indices into the
 * last yv_lk_build): points d_pts + 2*(p*pts_stride + i); results at the same positions of d_next / d_status /
 * d_err.  max_count, eps, min_eig: TermCriteria(COUNT+EPS, max_count, eps) and minEigThreshold. */
int yv_lk_track_batch(yv_lk* lk, const int32_t* d_pairs, int n_pairs, const float* d_pts, const int32_t* d_counts,
                      int pts_stride, int max_count, double eps, double min_eig, float* d_next, uint8_t* d_status,
                      float* d_err, void* stream);
/* Host-pointer drop-in for cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err,
 * Size(win, win), max_level, TermCriteria(COUNT+EPS, max_count, eps), 0, min_eig); n <= 65536. */
int yv_calc_optical_flow_pyr_lk(struct yv_ctx* ctx, const uint8_t* prev, const uint8_t* next, int H, int W,
                                int stride, const float* prev_pts, int n, int win, int max_level, int max_count,
                                double eps, double min_eig, float* next_pts, uint8_t* status, float* err);

/* ---- cv::findEssentialMat (RANSAC) + cv::recoverPose ----
 * Replaces, at the reference's (re)initialisation (src/LoopHandler.cc:239,256 and :581,598):
 *     E = cv::findEssentialMat(currFeatures, prevFeatures, 718.8560, cv::Point2d(607.1928, 185.2157), cv::RANSAC,
 *                              0.999, 1.0, mask);
 *     cv::recoverPose(E, currFramePts, lastFramePts, K, R, t);
 * Points are (x, y) pixel pairs exactly as the reference builds them (cv::Point2f(kp.x, kp.y), i.e. x = row,
 * y = column, used literally with pp and K).  The classic OpenCV path is restated (oracle/yavo_oracle_essential.c):
 * RANSAC with cv::RNG((uint64)-1) subsets, the five-point solver, float Sampson errors, maxIters 1000; recoverPose
 * with distance threshold 50 and no input mask (as the reference calls it).  A workspace serves up to max_pairs
 * lists of up to max_points correspondences. */
typedef struct yv_essential yv_essential;
int yv_essential_create(struct yv_ctx* ctx, int max_pairs, int max_points, int max_iters, yv_essential** out);
void yv_essential_destroy(yv_essential* es);
/* List p: d_pts1 / d_pts2 + 2*(p*pts_stride + i), i < d_counts[p] (5 <= n <= max_points to run; fewer -> not
 * found).  Outputs: d_E [p][9] (row-major; 0 when not found), d_mask + p*pts_stride (inliers of E; may be NULL),
 * d_found [p], d_stats [p][3] = {RANSAC iterations, models scored, best inlier count} (may be NULL). */
int yv_find_essential_batch(yv_essential* es, const float* d_pts1, const float* d_pts2, const int32_t* d_counts,
                            int n_pairs, int pts_stride, double focal, double ppx, double ppy, double prob,
                            double threshold, double* d_E, uint8_t* d_mask, int32_t* d_found, int32_t* d_stats,
                            void* stream);
/* recoverPose(E_p, pts1_p, pts2_p, K, R_p, t_p): d_R [p][9], d_t [p][3], d_good [p] = cheirality count (may be
 * NULL).  Lists as in yv_find_essential_batch. */
int yv_recover_pose_batch(yv_essential* es, const double* d_E, const float* d_pts1, const float* d_pts2,
                          const int32_t* d_counts, int n_pairs, int pts_stride, const double K[9], double* d_R,
                          double* d_t, int32_t* d_good, void* stream);
/* Host-pointer drop-ins for one list (n <= 65536): *found = 0 leaves E zero. */
int yv_find_essential(struct yv_ctx* ctx, const float* pts1, const float* pts2, int n, double focal, double ppx,
                      double ppy, double prob, double threshold, double E[9], uint8_t* mask, int* found);
int yv_recover_pose(struct yv_ctx* ctx, const double E[9], const float* pts1, const float* pts2, int n,
                    const double K[9], double R[9], double t[3], int* good);

/* ---- sliding-window bundle adjustment (BASELINE.json config 5) ----
 * The reference's Optimizer (src/Optimizer.cc:17-60 partialBA, include/Optimizer.hpp:64-126 edge / vertex) widened
 * to a keyframe window: poses (VertexPose, T_cw, SE3d::data()) and landmarks (3-vectors) joined by projection edges
 * e = meas - (K (T X)).xy / z with the reference's pose Jacobian, solved by g2o's Levenberg-Marquardt over
 * BlockSolver_6_3 (Schur complement on the landmarks, dense LDLT on the poses).  The first n_fixed poses are held
 * fixed.  Restated in oracle/yavo_oracle_ba.c (or_ba_lm); results are bit-identical to it. */
typedef struct yv_ba yv_ba;
/* max_poses <= 640: the reduced pose system (6 max_poses <= 3840 rows) is factorised by one workgroup whose two
 * vectors sit in LDS (16 B per row of a 64 KB workgroup allocation).  Device memory besides the problem arrays: the
 * tree4096 Schur partials of np free poses, (np (np + 1) / 2 + np) x 4.6 KB (24 MB at np = 100, 0.95 GB at 640),
 * allocated by the first problem that needs them. */
int yv_ba_create(struct yv_ctx* ctx, int max_poses, int max_landmarks, int max_edges, yv_ba** out);
void yv_ba_destroy(yv_ba* ba);
/* The graph: edge e joins pose edge_pose[e] and landmark edge_landmark[e] with measurement meas[e][2] (pixels, x
 * along K's first row); K row-major.  Host arrays, copied; the block structure (edges per pose / landmark, landmarks
 * shared by each pose pair) is built here, once per graph, as g2o's initializeOptimization does. */
int yv_ba_set_problem(yv_ba* ba, int n_poses, int n_fixed, int n_landmarks, const int32_t* edge_pose,
                      const int32_t* edge_landmark, const double* meas, int n_edges, const double K[9]);
/* optimize(max_iters) from poses [n_poses][7] / landmarks [n_landmarks][3] (host, in / out).  chi2_log
 * [max_iters + 1] (may be NULL): chi2 before the first iteration and after each; *iters = iterations run (may be
 * NULL; an iteration whose 10 damping trials all fail ends the run). */
int yv_ba_solve(yv_ba* ba, double* poses, double* landmarks, int max_iters, double* chi2_log, int* iters);
/* Run the BA's uploads, kernels and read-backs on `stream` (a hipStream_t of the same device; NULL = the context's
 * stream), e.g. beside the next frame batch on the context stream. Waits for the BA's previous stream first. */
int yv_ba_set_stream(yv_ba* ba, void* stream);
/* Where the LM's control runs: 1 (default) on the device -- the host enqueues every iteration without waiting and
 * one-lane kernels carry lambda / rho / accept / stop in a device control block (one read-back per solve); 0 on the
 * host (one read-back per damping trial).  Both give the same results bit for bit. */
int yv_ba_set_control(yv_ba* ba, int on_device);
/* Diagnostics: copy `count` doubles of workspace buffer `which` (0 err, 1 J_pose, 2 J_point, 3 H_pl, 4 W, 5 H_pp,
 * 6 b_p, 7 H_ll, 8 b_l, 9 D^-1, 10 S (as assembled for n <= 120; LDLT-factorised in place above), 11 b_schur, 12 x_p, 13 x_l, 14 poses, 15 landmarks)
 * as the last yv_ba_solve left it. */
int yv_ba_debug_read(yv_ba* ba, int which, double* dst, int64_t count);
/* Diagnostics: the reduced-system solver of yv_ba_solve on its own -- Eigen LDLT with diagonal pivoting of the
 * symmetric n x n S (row-major, bitwise symmetric as the Schur kernel writes it), then x = S^-1 b as
 * or_ldlt_solve computes it; *ok = its isPositive flag.  The same kernels the solve launches (n <= 128: the
 * register form, above: the global-memory form); 1 <= n <= 3840 (the solve's own limit, 6 x 640 poses). */
int yv_ba_debug_ldlt(yv_ctx* ctx, const double* S, int n, const double* b, double* x, int* ok);
/* Diagnostics: how many suspended trial loops (an iteration whose first damping trial was rejected) the device LM of
 * this yv_ba has resumed from the host since it was created (tests use it to show the resume path ran). */
int yv_ba_debug_resumes(yv_ba* ba);

/* ---- the sliding BA window of the chained stereo front end, on the device (BASELINE configs[2]) ----
 * The window LoopHandler's loop would hand Optimizer (src/LoopHandler.cc:60-165, src/Optimizer.cc:17-70), as
 * ya_vo_amd/sequence.py assembles it: frame records (T_wc, landmarks X_w, and each landmark's two observations --
 * its own frame's keypoint of the temporal match and the PnP measurement in the frame before) kept in HBM, the graph
 * built from per-frame counts, solved by the yv_ba it is tied to, written back; nothing crosses to the host but the
 * counts and the chi2 log.  Results are bit-identical to the host assembly + yv_ba_set_problem / yv_ba_solve. */
typedef struct yv_ba_window yv_ba_window;
/* max_lm: landmark slots per frame (the batch's max_kp); max_kf: keyframes per added block */
int yv_ba_window_create(yv_ba* ba, int max_lm, int max_kf, yv_ba_window** out);
void yv_ba_window_destroy(yv_ba_window* w);
/* size the record store for n_frames frames from the first recorded one, allocated by this call (it grows by doubling
 * from 64 otherwise, and each growth allocates, copies and synchronises the device inside the frame loop) */
int yv_ba_window_reserve(yv_ba_window* w, int64_t n_frames);
/* record the frames [first_frame, first_frame + n_frames) of a placed map block (yv_map_place; every frame a
 * keyframe) on `stream` (NULL: the context's): T_wc, landmarks, uv_prev = edge_uv[k][e], uv_own =
 * matches[2 k][edge_query[k][e]].pt2 with e = landmark id & 0xFFFF and k the frame's track (device pointers of
 * the batch: edge_uv [n][max_kp][2] f64, edge_query [n][max_kp] i32, matches [2 n][max_kp] yv_match, temporal
 * pairs at even indices) */
int yv_ba_window_add_block(yv_ba_window* w, const void* d_block, int64_t first_frame, int n_frames,
                           const double* d_edge_uv, const int32_t* d_edge_query, const void* d_matches, int max_kp,
                           void* stream);
/* BA over the recorded frames [first, first + n) (n <= 128), the first n_fixed held fixed, on the yv_ba's stream;
 * refined T_wc / X written back to the records, d_anchor (7 doubles, device, may be NULL) = the last frame's T_wc.
 * *solved = 0 when there is nothing to solve (n <= n_fixed or no landmark): the records stay, the anchor is set. */
int yv_ba_window_solve(yv_ba_window* w, int64_t first, int n, int n_fixed, const double K[9], int max_iters,
                       double* d_anchor, double* chi2_log, int* iters, int* solved);
/* yv_ba_window_solve in two halves, so the host can enqueue other work (the next chunk's front end on the context
 * stream) while the solve runs: _begin builds the graph and enqueues every LM iteration on the yv_ba's stream and
 * returns; _end waits, resumes a suspended trial loop if needed, writes the records back and returns the log.
 * Between the two, the window's add_block / read / trajectory and a second _begin return YV_ERR_INVALID, and the
 * yv_ba must not be used by anything else. */
int yv_ba_window_solve_begin(yv_ba_window* w, int64_t first, int n, int n_fixed, const double K[9], int max_iters,
                             double* d_anchor);
int yv_ba_window_solve_end(yv_ba_window* w, double* chi2_log, int* iters, int* solved);
/* one frame's record (host, blocking): T_wc[7], *n landmarks, up to cap of edge ids / X [3] / uv_own [2] /
 * uv_prev [2] (any may be NULL) */
int yv_ba_window_read(yv_ba_window* w, int64_t frame, double* T_wc, int* n, int32_t* edge, double* X, double* uv_own,
                      double* uv_prev, int cap);
/* T_wc [n][7] of the recorded frames [first, first + n) (host, blocking) */
int yv_ba_window_trajectory(yv_ba_window* w, int64_t first, int n, double* T_wc);
/* The recorded frames [first, first + n) as one map block (yavo_map.h, placed = 2) of a sequence shard, written on
 * `stream` (NULL: the context's) after the records' writers finished (host wait): keyframe j = frame first + j with
 * frame_id first + j + frame_id_offset, its T_wc and landmarks (ptID = frame_id << 16 | edge, X_w) as recorded, i.e.
 * relative to the shard's first frame; header C = T_wc of chunk_frame (the shard's last frame), n_frames = n_kf = n.
 * yv_map_place then places the gathered shards after each other (A_{r+1} = A_r C_r): T_wc = A_r T, X_w = A_r X.
 * d_block holds yv_map_block_bytes(max_kf, lm_stride) bytes; n <= max_kf, lm_stride >= the window's max_lm.  The
 * sequence's frame-sharded form (ya_vo_amd.sequence.SequenceShard). */
int yv_ba_window_export_block(yv_ba_window* w, int64_t first, int n, int64_t chunk_frame, int64_t frame_id_offset,
                              void* d_block, int max_kf, int lm_stride, void* stream);
/* ---- the window's multi-view mode (off by default; ya_vo_amd/sequence.py window_problem_tracks) ----
 * A landmark the temporal matches follow over several frames enters the window once, observed by every frame of its
 * chain, instead of once per frame with two observations.  Record l of frame k carries query = edge_query[k][e] (its
 * keypoint in L_{k-1}) and train = match_dj[2 k][query][1] (in L_k); its parent is the record of frame k-1 with the
 * smallest index whose train is this query, within the window and not at the window's second pose (chains are cut at
 * the window's start).  A chain rooted at window pose a with m records is one landmark with m + 1 edges in pose order
 * (a-1: the root's uv_prev; a .. a+m-1: the records' uv_own) and the root's X; landmarks ascend by (a, m, root's
 * index), edges are landmark-major; every record of a chain takes the landmark's refined X.  Results are
 * bit-identical to the host assembly + yv_ba_set_problem / yv_ba_solve.  The co-visibility lists are sized for a full
 * window (max_lm (n (n + 1) / 2 + n) entries for n poses) when the window first reaches a length, never after.
 * YV_ERR_INVALID while a solve is pending, or when frames were recorded with the other setting. */
int yv_ba_window_set_multiview(yv_ba_window* w, int on);
/* yv_ba_window_add_block that also records the links: d_match_dj = the batch's match_dj ([pairs][dj_stride][2] i32
 * {distance, train index}, temporal pairs at even indices), dj_stride >= max_kp.  With the mode on it is the only
 * way to add (NULL d_match_dj, or max_kp above the window's max_lm: YV_ERR_INVALID); with it off the two extra
 * arguments are ignored. */
int yv_ba_window_add_block_linked(yv_ba_window* w, const void* d_block, int64_t first_frame, int n_frames,
                                  const double* d_edge_uv, const int32_t* d_edge_query, const void* d_matches,
                                  int max_kp, const int32_t* d_match_dj, int64_t dj_stride, void* stream);
/* one frame's links (host, blocking, multi-view only): up to cap of query / train / parent (-1: none; any may be
 * NULL), in the record order of yv_ba_window_read */
int yv_ba_window_read_links(yv_ba_window* w, int64_t frame, int32_t* query, int32_t* train, int32_t* parent, int cap);

#ifdef __cplusplus
}
#endif
#endif /* YAVO_GEOM_H */
