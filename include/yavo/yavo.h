/*
 * yavo.h -- C ABI of the MI355X-native YA_VO front end (libyavo.so, gfx950).
 *
 * Drop-in boundary for the reference's per-frame hot path.  Each host-pointer entry point replaces one
 * reference member function (cited below) with the same argument meaning; results are bit-identical
 * to the reference's integer arithmetic (FAST indices, BRIEF bits, Hamming matches) and follow the
 * reference's float arithmetic operation-for-operation where it has one.
 *
 * Conventions:
 *   - plain C, no exceptions cross the boundary; every call returns YV_OK (0) or a negative status;
 *   - caller-allocated output buffers, capacities passed in, counts returned through out-pointers;
 *   - one yv_ctx per thread and per GPU (not thread-shared); all work is issued on the ctx's HIP stream
 *     unless a stream is passed explicitly;
 *   - coordinates follow the reference: x / rc[2i] = ROW, y / rc[2i+1] = COLUMN.
 *
 * There is no CPU fallback: without a usable gfx950 device every compute entry point returns
 * YV_ERR_NODEVICE.
 */
#ifndef YAVO_H
#define YAVO_H

#include <stddef.h>
#include <stdint.h>

#include "yavo_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YV_OK 0
#define YV_ERR_INVALID (-1)   /* bad argument (null pointer, bad size, capacity too small) */
#define YV_ERR_HIP (-2)       /* HIP runtime error */
#define YV_ERR_NODEVICE (-3)  /* no usable GPU */
#define YV_ERR_CAPACITY (-4)  /* request exceeds the batch / context capacity */

#define YV_ABI_VERSION 2

typedef struct yv_ctx yv_ctx;
typedef struct yv_batch yv_batch;

/* ---- library / context ------------------------------------------------------------------------ */
int yv_abi_version(void);
const char* yv_status_string(int status);
/* Number of visible HIP devices (0 when none); never fails. */
int yv_device_count(void);
/* Create a context on `device`: a HIP stream, default parameters (FAST threshold 40, 2000 corners,
 * the 9x9/sigma 2.5 fixed-point blur kernel, an all-zero BRIEF offset table until set). */
int yv_create(int device, yv_ctx** out);
void yv_destroy(yv_ctx* ctx);
/* The stream all yv_* calls on this context use (hipStream_t as void*). */
void* yv_stream(yv_ctx* ctx);
/* A second stream of the context on a hardware queue of its own (never the context stream's), made on first use and
 * kept until yv_destroy: work issued on it overlaps the context stream's (the sequence's BA windows). */
void* yv_side_stream(yv_ctx* ctx);
/* Block until all work queued on the context stream has finished. */
int yv_sync(yv_ctx* ctx);
/* Synchronous copies between host memory and device memory (e.g. a yv_batch_view array) on the
 * context stream. */
int yv_download(yv_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
int yv_upload(yv_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
/* Device memory on the context's GPU and pinned host memory, for callers without a HIP toolchain of their own (the C++
 * LoopHandler's GPU-decode look-ahead): the batch / decoder entry points take device pointers. */
int yv_device_alloc(yv_ctx* ctx, size_t bytes, void** out);
void yv_device_free(yv_ctx* ctx, void* p);
int yv_host_alloc(yv_ctx* ctx, size_t bytes, void** out);
void yv_host_free(yv_ctx* ctx, void* p);

/* FastDetector constructor constants (include/FastDetector.hpp:32-38): intensityThreshold (40) and
 * fastCornerNumThreshold (2000). */
int yv_set_fast_params(yv_ctx* ctx, int intensity_threshold, int max_corners);
/* Which cv::eigen the Harris response (src/FastDetector.cc:265) restates -- the reference's OpenCV build decides:
 * 0 (default) = OpenCV's JacobiImpl_<float> (built without Eigen), 1 = HAVE_EIGEN's
 * Eigen::SelfAdjointEigenSolver<MatrixXf> (Eigen 3.4).  Both are bit-exact against the oracle's restatements; they
 * differ from each other in the last bits of most responses. */
#define YV_HARRIS_EIGEN_JACOBI 0
#define YV_HARRIS_EIGEN_EIGEN3 1
int yv_set_harris_eigen(yv_ctx* ctx, int flavour);
/* Brief offsets table (src/BriefDescriptor.cc:4-20): 256 rows of {drow1, dcol1, drow2, dcol2},
 * each in [-8, 8]. */
int yv_set_brief_offsets(yv_ctx* ctx, const int8_t* offsets /* [256*4] */);
/* 9-tap fixed-point Gaussian (8 fractional bits, sum 256) used in place of cv::GaussianBlur
 * (src/BriefDescriptor.cc:90).  Default = OpenCV's bit-exact 9 / 2.5 kernel {12,22,31,41,44,...}.
 * Each tap must be <= 255 (YV_ERR_INVALID otherwise). */
int yv_set_blur_kernel(yv_ctx* ctx, const uint16_t* k9);

/* ---- host-pointer drop-in entry points (synchronous) --------------------------------------------- */
/* FastDetector::getFastFeatures (src/FastDetector.cc:277-369; include/FastDetector.hpp:48).
 * img: H x W u8, row stride `stride` bytes.  Writes up to max_kp (row, col) pairs into rc[2*max_kp] in
 * response-descending order (ties: row-major index ascending) and their Harris responses into resp
 * (may be NULL).  *n = number written, *n_candidates (may be NULL) = corners before the top-K cut. */
int yv_detect(yv_ctx* ctx, const uint8_t* img, int H, int W, int stride, int max_kp, int32_t* rc,
              float* resp, int* n, int* n_candidates);
/* Brief::computeBrief (src/BriefDescriptor.cc:86-124; include/BriefDescriptor.hpp:61): blur, keep the
 * points inside checkBoundry (:128-136), emit KeyPoint records (id = input index).  out capacity n. */
int yv_describe(yv_ctx* ctx, const uint8_t* img, int H, int W, int stride, const int32_t* rc, int n,
                yv_keypoint* out, int* n_out);
/* Brief::matchFeatures (src/BriefDescriptor.cc:163-183; include/BriefDescriptor.hpp:62): for every
 * query the first train point at minimum Hamming distance.  out capacity nq. */
int yv_match_features(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, yv_match* out);
/* Brief::removeOutliers (src/BriefDescriptor.cc:213-231; include/BriefDescriptor.hpp:64). */
int yv_filter_matches(yv_ctx* ctx, const yv_match* in, int n, int thr, yv_match* out, int* n_out);

/* ---- 2-NN matching: Lowe's ratio test and the mutual cross-check (beyond the reference; exact, all integer) ---- */
/* With d(i, j) the Hamming distance of query i and train point j:
 *   (d1, j1)(i) = the lexicographic minimum of (d(i, j), j) over j -- what yv_match_features returns;
 *   (d2, j2)(i) = the same minimum over j != j1(i): d2 >= d1, and on d2 == d1 j2 is the next tied index;
 *   nt < 2: d2 = INT32_MAX, j2 = -1; nt == 0: also d1 = INT32_MAX, j1 = -1;
 *   i1(j)       = the smallest query index that minimises d(i, j) (-1 for nq == 0).
 * YV_MATCH_RATIO keeps a query iff (int64)d1 * ratio_den < (int64)d2 * ratio_num (0 < num <= den <= 32768: an exact
 * tie d1 == d2 never passes); YV_MATCH_MUTUAL iff j1(i) >= 0 and i1(j1(i)) == i.  Both are applied on top of
 * removeOutliers' limit, which stays the one over all queries of the pair. */
#define YV_MATCH_RATIO 1
#define YV_MATCH_MUTUAL 2
typedef struct yv_match2 { int32_t d1, j1, d2, j2; } yv_match2; /* 16 B */
/* The two nearest train points of every query (out capacity nq) and, with rev != NULL (capacity nt), every train
 * point's best query i1(j).  YV_ERR_CAPACITY for nq or nt above 4096.  Both calls check their arguments before the
 * context; on a machine without a GPU (where no context can exist) a NULL context then yields YV_ERR_NODEVICE. */
int yv_match_knn2(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, yv_match2* out,
                  int32_t* rev);
/* yv_match_features + yv_filter_matches(thr) + the tests selected by flags, in query order with matched = true (flags
 * = 0: exactly those two calls).  out capacity nq; keep (may be NULL, capacity nq) = one byte per query.
 * YV_ERR_INVALID for flags outside 0..3 or, with YV_MATCH_RATIO, a ratio outside 0 < num <= den <= 32768. */
int yv_match_robust(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, int thr, int flags,
                    int ratio_num, int ratio_den, yv_match* out, int* n_out, uint8_t* keep);

/* ---- gated matching: only train points inside a window around the query (beyond the reference; exact) ---- */
/* A gate is {drow_lo, drow_hi, dcol_lo, dcol_hi} (yv_keypoint: x = row, y = column).  Train point j is a candidate
 * of query i iff drow_lo <= t[j].x - q[i].x <= drow_hi and dcol_lo <= t[j].y - q[i].y <= dcol_hi, and (d1, j1),
 * (d2, j2) and i1(j) above are taken over the candidates only (i1(j) over the queries j is a candidate of): no
 * candidate gives d1 = INT32_MAX, j1 = -1, fewer than two d2 = INT32_MAX, j2 = -1, no such query i1 = -1.  A rectified
 * stereo pair (left = query) is {-r, r, -max_disparity, 0}, a temporal pair a window {-h, h, -w, w}.
 * yv_match_knn2 under a gate: out capacity nq, rev (may be NULL) capacity nt.  YV_ERR_INVALID for a NULL gate, q, t
 * or out, a negative count, a gate with lo > hi or a bound outside [-65535, 65535], or a keypoint with x or y outside
 * [0, 65535]; YV_ERR_CAPACITY for nq or nt above 4096; all checked before the context, as in yv_match_knn2. */
int yv_match_gated(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, const int32_t gate[4],
                   yv_match2* out, int32_t* rev);

/* ---- keypoint selection: non-maximum suppression and per-cell quotas (beyond the reference; exact) ---- */
/* Every FAST corner has the key (~ord(response)) << 32 | row * W + col the cut ranks by: a smaller key is better
 * (higher response first, then the smaller row-major index), and the keys of one image are distinct.  Before the cut:
 *   nms_radius = r in 0..8 (0: off): a corner survives iff no other corner of the image with |drow| <= r and
 *     |dcol| <= r has a smaller key.  Simultaneous (a suppressed corner still suppresses), among corners only;
 *   per_cell = q in 0..4096 (0: off; cell_rows, cell_cols in [8, 8192], ignored for q = 0): cells are anchored at pixel
 *     (0, 0), cell(p) = (row / cell_rows, col / cell_cols); of each cell's survivors the q with the smallest keys stay.
 * What remains goes through the cut unchanged: the best min(max_corners, max_kp) in key order, then checkBoundry and
 * BRIEF as before; n_candidates / the view's cand_count keep counting the corners before selection and cut.  The
 * setting lives on the context: yv_detect, yv_select_corners and every yv_batch_run of the context's batches follow it
 * from the next call on.  All off (the default) launches exactly the reference's cut.  With q > 0 an H x W image may
 * have at most 8192 cells, ceil(H / cell_rows) * ceil(W / cell_cols) <= 8192: those three calls return
 * YV_ERR_CAPACITY otherwise, before any copy or launch (a batch is left exactly as it was).  The extra device
 * buffers (one more candidate list per image + counters) are allocated by the first run or call with selection on.
 * YV_ERR_INVALID for r outside 0..8, q outside 0..4096 or, with q > 0, a cell side outside [8, 8192], all checked
 * before the context; then for a NULL context. */
int yv_set_keypoint_select(yv_ctx* ctx, int nms_radius, int cell_rows, int cell_cols, int per_cell);
/* Selection + cut of a host list: n corners rc[2 * i ..] = (row, col) of an H x W image with responses resp[i], under
 * the context's selection and keep = min(max_corners, max_kp), in key order into out_rc / out_resp (capacity max_kp;
 * out_resp may be NULL), *n_out = number written.  Positions must be distinct (not checked).  Responses are compared
 * through the key, so any bit pattern is ordered; -0.0 and 0.0 differ.  Checked before the context: YV_ERR_INVALID
 * for a NULL rc, resp, out_rc or n_out, n < 0, max_kp < 0, H < 9, W < 9 or a position outside [0, H) x [0, W);
 * YV_ERR_CAPACITY for n > (H - 8) * (W - 8); then, as in yv_match_knn2, YV_ERR_NODEVICE for a NULL context on a
 * machine without a GPU. */
int yv_select_corners(yv_ctx* ctx, int H, int W, const int32_t* rc, const float* resp, int n, int max_kp,
                      int32_t* out_rc, float* out_resp, int* n_out);

/* ---- rotation-steered BRIEF from the intensity centroid (beyond the reference; exact, all integer) ---- */
/* With b the blurred image the descriptor samples and S(r, c) = b[clamp(r, 0, H - 1)][clamp(c, 0, W - 1)] (under
 * steering every read is clamped: no column W, no row H, no wrap), a keypoint at (row, col) has the moments
 *   m10 = sum dc * S(row + dr, col + dc),  m01 = sum dr * S(row + dr, col + dc)  over the disc dr^2 + dc^2 <= radius^2,
 * the bin = the smallest k that maximises m10 * dirs[k][0] + m01 * dirs[k][1] (a flat patch: bin 0), and test t
 * compares S(row + o[0], col + o[1]) > S(row + o[2], col + o[3]) with o = offsets[bin][t]; bit t is bit t % 8 of
 * featVec[t / 8] as before, and the record is otherwise unchanged.  The keypoint set (checkBoundry, the cut, kp_count,
 * the order, id) does not change.  n_bins = 0 (the default) switches steering off, radius and the tables are then
 * ignored and yv_describe / yv_batch_run launch exactly the unsteered descriptor; n_bins in 1..64 switches it on with
 * radius in 1..15, |dirs| <= 256 and |offsets| <= 15 in every component (every score then fits in int32).  The tables
 * are copied at the call; the setting lives on the context: yv_describe and every yv_batch_run of the context's
 * batches follow it from the next call on (ya_vo_amd/steering.py builds the default tables: the offsets table rotated
 * to n_bins directions).  YV_ERR_INVALID for n_bins outside 0..64 and, with n_bins > 0, a NULL table, a radius outside
 * 1..15 or a component out of range, all checked before the context; then for a NULL context. */
int yv_set_brief_steering(yv_ctx* ctx, int n_bins, int radius, const int16_t* dirs /* [n_bins][2] = (dcol, drow) */,
                          const int8_t* offsets /* [n_bins][256][4] = {drow1, dcol1, drow2, dcol2} */);
/* Moments (m10, m01) and bin of n positions rc[2 * i ..] = (row, col), anywhere inside the H x W image, under the
 * context's steering: blurs as yv_describe does, applies no boundary filter.  yv_describe's records carry id = the
 * input index, so bin[id] belongs to a record of the same list.  Checked before the context: YV_ERR_INVALID for a
 * NULL img, rc, moments or bin with n > 0, n < 0, H < 9, W < 9, stride < W or a position outside the image;
 * YV_ERR_CAPACITY for n > 4096; then YV_ERR_INVALID for a NULL context or with steering off. */
int yv_orient(yv_ctx* ctx, const uint8_t* img, int H, int W, int stride, const int32_t* rc, int n,
              int32_t* moments /* [n][2] = (m10, m01) */, uint8_t* bin /* [n] */);

/* ---- sub-pixel stereo disparity: a SAD search and a parabola (beyond the reference; exact, all integer) ---- */
/* With L and R the raw (unblurred) images of a rectified pair, a match of the left keypoint (r, c) and the right
 * keypoint (r2, c2) (x = row, y = column; the rows may differ), a half window w in 1..7 and a search range s in 1..8:
 *   inside iff r - w >= 0, r + w < H, c - w >= 0, c + w < W, r2 - w >= 0, r2 + w < H, c2 - s - w >= 0 and
 *     c2 + s + w < W; otherwise status YV_SUBPIX_OUTSIDE, dcol_q8 = 0, sad = -1 and nothing is read (no clamp, no wrap);
 *   SAD_k = sum over dr, dc in [-w, w] of |L(r + dr, c + dc) - R(r2 + dr, c2 + k + dc)| for k in -s..s, and k* the
 *     first minimum in the order 0, -1, +1, -2, +2, ..., -s, +s;
 *   |k*| = s: status YV_SUBPIX_EDGE, dcol_q8 = 0, sad = SAD_k* (the minimum is not bracketed);
 *   otherwise a = SAD_(k*-1), b = SAD_k*, c = SAD_(k*+1), den = a + c - 2 b (>= |a - c|), frac = 0 for den = 0, else
 *     floor((256 (a - c) + den) / (2 den)) (the parabola's vertex in 1/256 pixel, rounded half up, |frac| <= 128):
 *     status YV_SUBPIX_OK, dcol_q8 = 256 k* + frac, sad = b.
 * The refined right column is (double)c2 + (double)dcol_q8 * (1.0 / 256.0), exact in double. */
#define YV_SUBPIX_NONE 0     /* not attempted (batches only): dcol_q8 = 0, sad = -1 */
#define YV_SUBPIX_OK 1
#define YV_SUBPIX_OUTSIDE 2
#define YV_SUBPIX_EDGE 3
#define YV_SUBPIX_DROP_EDGE 1 /* yv_batch_set_stereo_subpix flag: the tracks drop the YV_SUBPIX_EDGE matches */
/* The refinement of n match records (pt1 = the left keypoint, pt2 = the right one; every record is attempted) on two
 * H x W host images with rows `stride` bytes apart; dcol_q8, sad and status have capacity n.  Checked before the
 * context: YV_ERR_INVALID for a NULL left, right, m, dcol_q8, sad or status with n > 0, n < 0, H < 9, W < 9,
 * stride < W, half_win outside 1..7, search outside 1..8 or a keypoint outside the image; YV_ERR_CAPACITY for n > 4096;
 * then, as in yv_match_knn2, YV_ERR_NODEVICE for a NULL context on a machine without a GPU. */
int yv_stereo_subpix(yv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W, int stride,
                     const yv_match* m, int n, int half_win, int search, int32_t* dcol_q8, int32_t* sad,
                     uint8_t* status);

/* ---- batched device pipeline (inputs resident in HBM) ---------------------------------------------- */
/* A batch owns device workspace for up to max_images images of H x W and max_pairs match pairs.  Slot
 * index max_images is the "carry" slot: it holds the keypoints / descriptors of one image of the
 * previous run (see yv_batch_run's carry_from), so consecutive runs chain frame k-1 -> k.  YV_ERR_CAPACITY for
 * W > 2048 (BRIEF stages 49 image rows in LDS) or H > 8192 (top-K's per-band keypoint lists). */
int yv_batch_create(yv_ctx* ctx, int max_images, int H, int W, int max_kp, int max_pairs,
                    yv_batch** out);
void yv_batch_destroy(yv_batch* b);
/* Match pairs (query image, train image) for subsequent runs; indices in [0, max_images] (max_images =
 * carry slot).  Copied to the device once. */
int yv_batch_set_pairs(yv_batch* b, const int32_t* pairs /* [2*n_pairs] */, int n_pairs);
/* Run detect -> describe -> match -> removeOutliers for n_images device images
 *   image i at d_images + i*image_pitch, rows `stride` bytes apart,
 * then copy image carry_from's keypoints into the carry slot (carry_from < 0: no copy).  Asynchronous
 * on `stream` (NULL = the context stream).  match_thr is removeOutliers' threshold (20 in
 * src/LoopHandler.cc:192,537). */
int yv_batch_run(yv_batch* b, const uint8_t* d_images, int n_images, int stride, int64_t image_pitch,
                 int match_thr, int carry_from, void* stream);
/* The match filter of the following runs: flags = 0 (the default) is the reference's behaviour, YV_MATCH_RATIO and /
 * or YV_MATCH_MUTUAL add the tests above.  With a filter on, yv_batch_run runs the top-2 matcher, the matcher on the
 * swapped pairs (YV_MATCH_MUTUAL only) and a finalize that writes `matches`, `match_dj` and `match_lim` as before,
 * `filtered` / `filt_count` with the kept records only, and the arrays of yv_batch_match2_view; yv_batch_track,
 * yv_batch_track_map and the LK mode then use only kept matches.  The extra device buffers are allocated by the
 * first call with flags != 0.  Same argument checks as yv_match_robust. */
int yv_batch_set_match_filter(yv_batch* b, int flags, int ratio_num, int ratio_den);
typedef struct yv_batch_match2_view {
    const yv_match2* nn2;             /* [max_pairs][max_kp] */
    const int32_t* rev;               /* [max_pairs][max_kp]: i1(j); -1 everywhere without YV_MATCH_MUTUAL */
    const uint8_t* keep;              /* [max_pairs][max_kp] */
} yv_batch_match2_view;
/* Device views of the filter's arrays (the last run with a filter on); YV_ERR_INVALID before the filter was ever
 * switched on. */
int yv_batch_match2_view_get(yv_batch* b, yv_batch_match2_view* v);
typedef struct yv_batch_orient_view {
    const uint8_t* bin;               /* [max_images + 1][max_kp], keypoint order */
    const int32_t* moments;           /* [max_images + 1][max_kp][2] = (m10, m01) */
} yv_batch_orient_view;
/* Device views of the orientation of every keypoint of the last run with steering on (yv_set_brief_steering), the
 * carry slot's rows copied with its keypoints.  The two arrays are allocated by the first run with steering on:
 * YV_ERR_INVALID before it. */
int yv_batch_orient_view_get(yv_batch* b, yv_batch_orient_view* v);
/* The gates of the following runs, one per pair of yv_batch_set_pairs (gates[4 * p ..] as in yv_match_gated); gates
 * == NULL or n_pairs == 0 switches gating off (the default).  With gates set, yv_batch_run replaces its matcher
 * launches (forward, top-2 and swapped pairs alike) by the gated matcher; removeOutliers, the match filter, the
 * tracks and every view array work as before, on the gated (d1, j1), (d2, j2) and i1: a query without a candidate
 * has distance INT32_MAX, train index -1 and is never kept.  yv_batch_set_pairs clears the gates.  The device
 * buffers are allocated by the first call that sets gates.  YV_ERR_INVALID for a NULL batch, n_pairs different from
 * the batch's pair count, or a gate yv_match_gated would reject. */
int yv_batch_set_match_gates(yv_batch* b, const int32_t* gates /* [4 * n_pairs] */, int n_pairs);
/* The stereo pairs (indices into yv_batch_set_pairs' list; query = left image, train = right image) whose matches the
 * following runs refine as yv_stereo_subpix does, on the raw images passed to the run; pair_idx == NULL or n == 0
 * switches it off (the default; the other arguments are then ignored).  With it on, yv_batch_run launches the
 * refinement right after the match stage's finalize (inside stage 4 of yv_batch_stage_times) for every match of a
 * marked pair that removeOutliers keeps (distance < limit, train index >= 0), that the match filter, when on, keeps,
 * and whose two slots are images of the run (index < n_images); every other entry of the arrays below is
 * YV_SUBPIX_NONE.  yv_batch_track, yv_batch_track_map and the LK mode then triangulate a match with status
 * YV_SUBPIX_OK from its refined right column and every other match from its integer column, exactly as before; with
 * flags = YV_SUBPIX_DROP_EDGE a YV_SUBPIX_EDGE match counts as not kept there.  Without it the edge set (edge_count,
 * edge_query, edge_uv) is the unrefined run's and only edge_X moves, as long as every refined point still passes
 * triangulate2View's test (s4 / s3 < 1e-2 and Z > 0), which is applied to the refined point: a match whose refined
 * point fails it is no edge, one whose integer point failed it and whose refined point passes is.  A call waits for the
 * device (a run or a track in flight on any stream reads the list and the arrays).  yv_batch_set_pairs switches it
 * off.  The device
 * arrays are allocated by the first call that switches it on; every call that switches it on fills them with
 * YV_SUBPIX_NONE.  YV_ERR_INVALID for a NULL batch, n < 0, an index outside the pair list, a duplicate, a pair that
 * names the carry slot, half_win outside 1..7, search outside 1..8 or flags outside 0..1. */
int yv_batch_set_stereo_subpix(yv_batch* b, const int32_t* pair_idx /* [n] */, int n, int half_win, int search,
                               int flags);
typedef struct yv_batch_subpix_view {
    const int32_t* dcol_q8;           /* [max_pairs][max_kp], by query keypoint index */
    const int32_t* sad;               /* [max_pairs][max_kp] */
    const uint8_t* status;            /* [max_pairs][max_kp] YV_SUBPIX_* */
} yv_batch_subpix_view;
/* Device views of the refinement's arrays (the last run with it on); YV_ERR_INVALID before it was ever switched on. */
int yv_batch_subpix_view_get(yv_batch* b, yv_batch_subpix_view* v);
/* ---- scale pyramid: multi-scale keypoints merged into the batch's slots (beyond the reference; exact, all integer) ---- */
/* n_levels in 2..8 levels of sizes level_hw[2 * l ..] = (H_l, W_l): level 0 is the batch's H x W, the sizes do not grow
 * and shrink by at most 2 per level (2 H_l >= H_(l-1), 2 W_l >= W_(l-1)), and every size is one yv_batch_create accepts.
 * Level l is the integer bilinear resample of level l - 1, centre-aligned: the source position of destination row r, in
 * 1/32 pixel, is qv = clamp(floor(((2 r + 1) H_(l-1) - H_l) * 16 / H_l), 0, (H_(l-1) - 1) * 32), of column c the same
 * with W; the pixel is yv_rectify_image's four-tap blend at (qu, qv) (yavo_io.h), whose taps all lie inside the source.
 * Every level runs detect, the context's keypoint selection, the cut at min(level_keep[l], max_corners) and BRIEF
 * (steered when the context's steering is on) on its own image and its own blur, exactly as yv_detect + yv_describe
 * with max_kp = level_keep[l] do on that image.  The keypoints of levels 1 .. L - 1 are then appended to their image's
 * slot behind level 0's, in level order and inside a level in that level's keypoint order: featVec and the internal
 * descriptor copied, matched = 0, id = the index in the merged list, x = floor((2 x_l + 1) H_0 / (2 H_l)), y the same
 * with W; with steering the bin and the moments travel with the record.  kp_count becomes the merged count; det_count,
 * det_rc, det_resp and cand_count of yv_batch_view stay level 0's.  From the match stage on a run works on the merged
 * slots unchanged.  n_levels <= 1 switches the pyramid off (the default; the arrays are then ignored) and yv_batch_run
 * launches exactly what it launched before.  In yv_batch_stage_times the level images and the levels' detect count in
 * stage 0, their selection and cut in stage 1, their BRIEF and the merge in stage 2.  The level workspaces are allocated by the first call that switches it on
 * and kept while the sizes stay the same; a call that switches it on waits for the device.
 * Checked in this order, before the batch is looked at where the batch is not needed: YV_ERR_INVALID for a NULL array
 * with n_levels > 1, n_levels > 8, a side below 9, a negative quota, a level 0 that differs from the batch, a level
 * larger than the one before it or less than half of it; YV_ERR_CAPACITY for a sum of the quotas above max_kp or a
 * level with W > 2048 or H > 8192; then YV_ERR_INVALID for a NULL batch. */
#define YV_PYRAMID_MAX_LEVELS 8
int yv_batch_set_pyramid(yv_batch* b, int n_levels, const int32_t* level_hw /* [n_levels][2] */,
                         const int32_t* level_keep /* [n_levels] */);
typedef struct yv_batch_pyramid_view {
    int n_levels;
    int H[YV_PYRAMID_MAX_LEVELS], W[YV_PYRAMID_MAX_LEVELS], keep[YV_PYRAMID_MAX_LEVELS];
    /* level l's images: image i at image[l] + i * pitch[l], rows stride[l] bytes apart (level 0: NULL, the run's own) */
    const uint8_t* image[YV_PYRAMID_MAX_LEVELS];
    int stride[YV_PYRAMID_MAX_LEVELS];
    int64_t pitch[YV_PYRAMID_MAX_LEVELS];
    const int32_t* kp_count[YV_PYRAMID_MAX_LEVELS];    /* [max_images + 1] the level's keypoints per image */
    const int32_t* det_count[YV_PYRAMID_MAX_LEVELS];   /* [max_images + 1] the level's corners after its cut */
    /* [max_images + 1][max_kp] the level's own records (level 0: the head of the merged slot) */
    const yv_keypoint* keypoints[YV_PYRAMID_MAX_LEVELS];
    const uint8_t* level;             /* [max_images + 1][max_kp] the level of every merged keypoint */
    const int32_t* level_rc;          /* [max_images + 1][max_kp][2] its (row, col) on its own level */
} yv_batch_pyramid_view;
/* Device views of the last run with the pyramid on; the carry slot's level / level_rc rows (and kp_count[0]) are copied
 * with its keypoints.  YV_ERR_INVALID before the pyramid was ever switched on. */
int yv_batch_pyramid_view_get(yv_batch* b, yv_batch_pyramid_view* v);
/* The host-pointer form for one image: the merged list of a one-image batch with max_kp = the sum of the quotas
 * (at most 4096) into out / level / level_rc (capacity: that sum), *n_out = the merged count.  n_levels = 1 is the
 * single-scale detect + describe with the cut at level_keep[0].  The argument checks of yv_batch_set_pyramid with the
 * image's H x W as the batch's, and YV_ERR_INVALID for a NULL img or n_out, n_levels < 1, H < 9, W < 9 or stride < W,
 * all before the context; then, as in yv_match_knn2, YV_ERR_NODEVICE for a NULL context on a machine without a GPU. */
int yv_detect_describe_pyramid(yv_ctx* ctx, const uint8_t* img, int H, int W, int stride, int n_levels,
                               const int32_t* level_hw, const int32_t* level_keep, yv_keypoint* out, uint8_t* level,
                               int32_t* level_rc /* [n][2] */, int* n_out);
/* One level step on host pointers: dst (dst_H x dst_W, rows dst_stride bytes apart; the bytes between the rows stay
 * the caller's) = the resample above of src.  YV_ERR_INVALID for a NULL src or dst, a size outside
 * 1 <= dst <= src <= min(2 dst, 8192) per axis or a stride below its width, checked before the context. */
int yv_pyramid_image(yv_ctx* ctx, const uint8_t* src, int src_H, int src_W, int src_stride, int dst_H, int dst_W,
                     uint8_t* dst, int dst_stride);

/* Tracking (PnP) over the last run's matches: track t = {stereo_pair, temporal_pair} (pair indices of
 * yv_batch_set_pairs) where the stereo pair's query image (frame k left) is the temporal pair's train
 * image.  Each frame-(k-1) keypoint kept by removeOutliers in the temporal pair whose frame-k keypoint is
 * itself kept in the stereo pair becomes one pose edge: X = LoopHandler::triangulation of the stereo match
 * (src/LoopHandler.cc:867-885, left camera = world, right camera pose T_right; accepted iff success and
 * Z > 0 as in triangulate2View :658-726), measurement = the frame-(k-1) keypoint (x, y).  The pose of
 * frame k-1 in frame k's camera is then LoopHandler::optimizePoseOnly (:730-861) from the prior.  K and
 * T_right are copied once; tracks are validated against the pairs (YV_ERR_INVALID otherwise), and a NaN or infinite
 * entry of K or T_right is YV_ERR_INVALID as well. */
int yv_batch_set_tracks(yv_batch* b, const int32_t* tracks /* [2*n_tracks] */, int n_tracks, const double K[9],
                        const double T_right[7]);
/* Build the track edges and solve every track's pose in one launch each (asynchronous on `stream`, NULL =
 * context stream).  d_priors [n_tracks][7] in, d_poses [n_tracks][7] out (may alias d_priors). */
int yv_batch_track(yv_batch* b, const double* d_priors, double* d_poses, void* stream);
/* Overlap mode: the pose LM of each yv_batch_track runs on a stream of the batch, ordered after that call's
 * edge build only, so it executes beside the next yv_batch_run's kernels (edge buffers rotate over three
 * copies; the build of track i + 3 waits for the LM of track i).  With the match tracker the edge build itself
 * also runs on a stream of the batch, after the run's matches, beside the next run's detect; the next run's
 * top-K waits for it (environment YAVO_BUILD_ASYNC=0 keeps it on the call's stream).  d_priors / d_poses / the
 * track views are then complete only after yv_batch_track_sync (or a device-wide synchronization).  on = 2 / 3 / 4 defer each
 * LM further: it is launched by the next yv_batch_run once that run's detect (2) / describe (3) / top-K (4) stage is issued
 * (so it runs beside the later, less occupancy-sensitive stages), or by yv_batch_track_sync /
 * yv_batch_map_wait / the next yv_batch_track, whichever comes first.
 * With the match tracker, tracks set and the asynchronous edge build, a run's two lists of Matches records
 * (yv_batch_view matches / filtered) are also written on a stream of the batch, beside the next run's detect: nothing
 * in the step reads them.  They are then complete after yv_batch_track_sync, or on a stream that called
 * yv_batch_records_wait after the run, and no longer after a synchronization of the run's stream alone.  The counts,
 * match_dj, match_lim and every other view are written on the run's stream as before.  (Every-stage timing,
 * yv_batch_enable_timing(b, 1), keeps the lists on the run's stream.) */
int yv_batch_set_track_overlap(yv_batch* b, int on);
int yv_batch_track_sync(yv_batch* b);
/* `stream` waits for the last run's lists of Matches records where they are written beside the next run (overlap
 * mode, above); otherwise a no-op: the lists are then ordered on the run's stream. */
int yv_batch_records_wait(yv_batch* b, void* stream);
/* LK tracking mode, the reference's trackLastFrame (src/LoopHandler.cc:298-454): with image_step > 0 a track
 * is {stereo pair of frame k-1, image index of frame k}.  Frame k-1's map points are its left keypoints whose
 * stereo match survives removeOutliers and triangulates; they are tracked into frame k by
 * calcOpticalFlowPyrLK(win, max_level, TermCriteria(COUNT+EPS, max_count, eps), flags 0, min_eig) on the last
 * run's images 0, image_step, 2 image_step, ... (both images of a track must be among them), and every point
 * with status 1 becomes an edge at cv::Point2i(next.y, next.x) (truncation).  image_step = 0: match mode.
 * Clears the tracks (set them again).  Declared in yavo_geom.h: the LK workspace API it uses. */
int yv_batch_set_track_lk(yv_batch* b, int image_step, int win, int max_level, int max_count, double eps,
                          double min_eig);
/* ---- track RANSAC: a P3P-RANSAC pose as each track's LM prior (opt-in, beyond the reference; off by default) ----
 * With iters > 0 every following yv_batch_track runs yv_pnp_ransac_batch (yavo_geom.h: `iters` hypotheses from
 * draws [iters][3], host, copied; threshold thr pixels; min_inliers) over each track's edges on the LM's stream just
 * before the LM, in every overlap mode and in LK mode.  The LM's prior of a track is the RANSAC pose where one was found
 * and the caller's d_priors entry otherwise; the LM itself is unchanged.  iters = 0 switches it off (the other arguments
 * are ignored): not one launch or allocation more than before.  The arguments are checked as yv_pnp_ransac's
 * (YV_ERR_INVALID); a call that changes the mode waits for the device (a track in flight reads the draws). */
int yv_batch_set_track_ransac(yv_batch* b, int iters /* 0 = off */, double thr, int min_inliers,
                              const uint32_t* draws);
typedef struct yv_batch_ransac_view {
    int n_tracks;
    const double* pose;               /* [n_tracks][7] the LM's priors: the RANSAC pose, or the caller's prior */
    const uint8_t* inlier;            /* [n_tracks][max_kp] by edge, zero where nothing was found */
    const int32_t* inliers;           /* [n_tracks] */
    const int32_t* found;             /* [n_tracks] */
} yv_batch_ransac_view;
/* Device views of the last yv_batch_track's RANSAC (complete when its LM is); YV_ERR_INVALID while the mode is off or
 * no tracks are set. */
int yv_batch_ransac_view_get(yv_batch* b, yv_batch_ransac_view* v);
/* Per-stage device time of the runs since the last reset, when timing is enabled (HIP events recorded
 * on the run stream around every stage).  Stages: 0 detect (FAST + Harris + blur, one fused kernel),
 * 1 top-K + checkBoundry, 2 BRIEF, 3 match (with a match filter: both matcher launches), 4 Matches records +
 * removeOutliers (+ carry copies, + the match filter's tests), 5 track edges (stereo triangulation), 6 track poses (LM).  ms[i] = summed milliseconds, *n_runs = runs
 * accumulated (stages 5-6 summed over the runs followed by yv_batch_track).  on = 2: events around the
 * detect kernel only (ms[0]; the other stages read 0) -- two events per run instead of nine. */
int yv_batch_enable_timing(yv_batch* b, int on);
int yv_batch_stage_times(yv_batch* b, float* ms /* [8] */, int* n_runs);
#define YV_NUM_STAGES 7

/* Device views of the batch results (valid until the next run / destroy).  All arrays are indexed
 * [slot][...] with the per-slot strides given. */
typedef struct yv_batch_view {
    int max_images, max_kp, max_pairs, H, W;
    int64_t cand_cap;                 /* candidate capacity per image = (H-8)*(W-8) */
    const uint32_t* cand_count;       /* [max_images+1]: FAST corners before the cut */
    const int32_t* det_count;         /* [max_images+1]: min(corners, max_kp) */
    const int32_t* det_rc;            /* [max_images+1][max_kp][2] (row, col), response order */
    const float* det_resp;            /* [max_images+1][max_kp] */
    const int32_t* kp_count;          /* [max_images+1]: keypoints that passed checkBoundry */
    const yv_keypoint* keypoints;     /* [max_images+1][max_kp] */
    const uint8_t* blurred;           /* [max_images][H][blur_pitch] (row pitch: the last field) */
    const int32_t* match_count;       /* [max_pairs]: = kp_count of the query image */
    const yv_match* matches;          /* [max_pairs][max_kp] */
    const int32_t* filt_count;        /* [max_pairs] */
    const yv_match* filtered;         /* [max_pairs][max_kp] */
    /* per-query {distance, train keypoint index (-1: empty train)} and the removeOutliers limit
     * (kept iff distance < limit) of every pair */
    const int32_t* match_dj;          /* [max_pairs][max_kp][2] */
    const int32_t* match_lim;         /* [max_pairs] */
    /* tracks (yv_batch_set_tracks / yv_batch_track): the buffers of the last yv_batch_track call */
    int n_tracks;
    const int32_t* edge_count;        /* [n_tracks] */
    const double* edge_X;             /* [n_tracks][max_kp][3] */
    const double* edge_uv;            /* [n_tracks][max_kp][2] */
    const int32_t* edge_query;        /* [n_tracks][max_kp]: temporal query keypoint index */
    const uint8_t* edge_outlier;      /* [n_tracks][max_kp] */
    const int32_t* track_inliers;     /* [n_tracks] */
    int blur_pitch;                   /* row pitch of `blurred` in bytes (128-B aligned, >= W + 1) */
} yv_batch_view;
int yv_batch_view_get(yv_batch* b, yv_batch_view* view);

#ifdef __cplusplus
}
#endif

#include "yavo_geom.h"
#include "yavo_bow.h"
#include "yavo_loop.h"

#endif /* YAVO_H */
