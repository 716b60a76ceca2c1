/*
 * yavo_loop.h -- loop closure: a keyframe store and the geometric verification of place-recognition candidates on the
 * GPU (beyond the reference; exact).
 *
 * A keyframe (entry) is n <= max_kp left keypoints: a descriptor (32 B) and a position (x = row, y = column) each, and
 * optionally a landmark X[3] (double, in the keyframe's left camera frame) with a flag `has`.  An entry's index is its
 * insertion order: entry e of the store is entry e of a yv_bow when the caller adds the same images to both in the same
 * order.  The general add takes X and has from the caller; the batch add takes them from a stereo pair of the batch's
 * last run: keypoint j of the left slot has a landmark iff the stereo leg of the track builders holds for it (its
 * stereo match is below the pair's removeOutliers limit, passes the batch's match filter and sub-pixel refinement as
 * yv_batch_track reads them, and triangulates with Z > 0 between the identity and T_right), and X is that point.  X is
 * stored as zero where has is 0.
 *
 * Verification of a query keypoint list q against entry e, under yv_loop_set_params, composes operations the library
 * already specifies and adds no floating-point expression of its own (tests/loop_reference.py):
 *
 *   1. keep[i], j1[i] = yv_match_robust(q, the entry's keypoints, match_thr, flags, ratio_num, ratio_den);
 *   2. edges, in query order: every i with keep[i] and has[j1[i]]: X = X_e[j1[i]], uv = ((double)q[i].x, (double)q[i].y),
 *      edge_query = i, edge_train = j1[i]; n_kept = the kept queries, n_edges = the edges;
 *   3. yv_pnp_ransac over the edges (K, draws, thr_px, min_inliers) -> found, ransac_inliers, the inlier mask;
 *   4. only if found: yv_pose_lm over all edges from the RANSAC pose as prior -> pose, outlier flags, lm_inliers, summed
 *      in the oracle's sum_mode yv_loop_lm_sum_mode(n_problems);
 *   5. verified = found && lm_inliers >= min_inliers.
 *
 * Where no pose is found lm_inliers = 0, pose is the identity {0,0,0,1,0,0,0} and both masks are zero.  pose maps
 * keyframe-camera coordinates to the query's camera.
 *
 * The batch form reads the candidate rows of a yv_bow query (d_cand_entry [nq][16], d_cand_count [nq]) from device
 * memory: problem v = top_k * q + k for k < top_k is skipped when k >= count[q], the entry is negative or the entry is
 * not below the store's count at the call.  A skipped problem has entry = -1, every count 0, verified = 0 and the
 * identity pose.  The grid is the static nq x top_k: the host never learns the counts.
 *
 * Argument checks come first, before the context or the object is looked at: YV_ERR_INVALID for a NULL required
 * pointer, max_entries outside 1..65536, max_problems outside 1..4096, max_kp outside 1..4096, top_k outside 1..16,
 * n < 0, non-finite K / T_right, flags / ratio as yv_match_robust, iters / thr_px / min_inliers as yv_pnp_ransac; then
 * YV_ERR_INVALID for a NULL context or object -- YV_ERR_NODEVICE instead on a machine without a GPU; then what needs
 * the object: YV_ERR_INVALID for a slot or stereo pair outside the batch, a stereo pair whose query slot is not the
 * left slot given, a batch whose max_kp exceeds the object's, or a verify before yv_loop_set_params; YV_ERR_CAPACITY
 * for n > max_kp (host forms), nq * top_k > max_problems (n > max_problems in the host form) and an add beyond
 * max_entries, which leaves the store as it was.
 *
 * A context or batch without a yv_loop launches and allocates nothing new.
 */
#ifndef YAVO_LOOP_H
#define YAVO_LOOP_H

#include <stdint.h>

#include "yavo_types.h"

#ifdef __cplusplus
extern "C" {
#endif

struct yv_ctx;
struct yv_batch;
typedef struct yv_loop yv_loop;

#define YV_LOOP_MAX_PROBLEMS 4096
#define YV_LOOP_CAND_STRIDE 16  /* the row length of a candidate array (YV_BOW_MAX_TOP_K) */

typedef struct yv_loop_result { /* 80 B */
    int32_t entry;          /* the entry verified against, -1: the problem was skipped */
    int32_t n_kept;         /* queries the match filter kept */
    int32_t n_edges;        /* of those, the ones whose train keypoint has a landmark */
    int32_t ransac_inliers; /* 0 where nothing was found */
    int32_t lm_inliers;     /* 0 where nothing was found */
    int32_t verified;       /* found && lm_inliers >= min_inliers */
    double pose[7];         /* qx qy qz qw tx ty tz, keyframe camera -> query camera; identity where nothing was found */
} yv_loop_result;

int yv_loop_create(struct yv_ctx* ctx, const double K[9], const double T_right[7], int max_entries /* 1..65536 */,
                   int max_problems /* 1..4096 */, int max_kp /* 1..4096 */, yv_loop** out);
void yv_loop_destroy(yv_loop* loop);
/* empties the store, keeps the parameters */
int yv_loop_reset(yv_loop* loop);
int yv_loop_count(yv_loop* loop, int* n_entries);
/* The verification's parameters (draws: [iters][3] uint32, copied).  Synchronous on the context's stream. */
int yv_loop_set_params(yv_loop* loop, int match_thr, int flags, int ratio_num, int ratio_den, int iters,
                       const uint32_t* draws, double thr_px, int min_inliers);
/* the LM's edge-sum order (the oracle's sum_mode) of a verify call over n_problems problems */
int yv_loop_lm_sum_mode(int n_problems);

/* ---- host-pointer forms (synchronous, on the context's stream) ---- */
/* appends the keyframe as entry yv_loop_count(); X [n][3] and has [n] may both be NULL (no landmarks) */
int yv_loop_add(yv_loop* loop, const yv_keypoint* kp, int n, const double* X, const uint8_t* has, int64_t frame_id);
/* the query list q against entries[0..n): results[p] is problem p; an entry outside the store is a skipped problem */
int yv_loop_verify(yv_loop* loop, const yv_keypoint* q, int nq, const int32_t* entries, int n, yv_loop_result* results);

/* ---- batch forms: read the batch's slots in HBM, asynchronous on `stream` (NULL: the context's); the caller orders
 * them after the run that filled the slots and before the next one.  The host arrays are copied at the call. ---- */
/* left slot left_slots[i] with the landmarks of stereo pair stereo_pairs[i] (an index into the batch's pairs, whose
 * query slot is left_slots[i]) becomes entry count + i with frame id frame_ids[i] */
int yv_loop_add_batch(yv_loop* loop, struct yv_batch* batch, const int32_t* left_slots, const int32_t* stereo_pairs,
                      const int64_t* frame_ids, int n, void* stream);
/* query q = slot slots[q]; its candidates are row q of d_cand_entry ([nq][16]) / d_cand_count ([nq]), device arrays
 * laid out as yv_bow_candidates_copy writes them; the results are the view's rows 0..nq * top_k - 1 */
int yv_loop_verify_batch(yv_loop* loop, struct yv_batch* batch, const int32_t* slots, int nq,
                         const int32_t* d_cand_entry, const int32_t* d_cand_count, int top_k, void* stream);

typedef struct yv_loop_view {
    int max_entries, max_problems, max_kp;
    int n_entries;                  /* entries whose add was enqueued so far */
    int n_problems;                 /* problems of the last verify call */
    /* the store */
    const uint8_t* desc;            /* [max_entries][max_kp][32] */
    const int32_t* pos;             /* [max_entries][max_kp][2] = (x = row, y = column) */
    const double* X;                /* [max_entries][max_kp][3], zero where has is 0 */
    const uint8_t* has;             /* [max_entries][max_kp], zero past the entry's count */
    const int32_t* kp_count;        /* [max_entries] */
    const int64_t* frame_id;        /* [max_entries] */
    /* the last verify call */
    const yv_loop_result* results;  /* [max_problems] */
    const double* edge_X;           /* [max_problems][max_kp][3] */
    const double* edge_uv;          /* [max_problems][max_kp][2] */
    const int32_t* edge_query;      /* [max_problems][max_kp] */
    const int32_t* edge_train;      /* [max_problems][max_kp] */
    const uint8_t* ransac_inlier;   /* [max_problems][max_kp] */
    const uint8_t* lm_outlier;      /* [max_problems][max_kp] */
    const int32_t* edge_count;      /* [max_problems] */
} yv_loop_view;
/* Device views (valid until yv_loop_destroy; complete once the stream of the call that wrote them has drained). */
int yv_loop_view_get(yv_loop* loop, yv_loop_view* view);
/* The last verify call's results 0..n-1 copied device to device, asynchronously on `stream` (NULL: the context's),
 * into the caller's d_results ([n] yv_loop_result), like yv_bow_candidates_copy. */
int yv_loop_results_copy(yv_loop* loop, int n, yv_loop_result* d_results, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YAVO_LOOP_H */
