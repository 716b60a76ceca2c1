/*
 * yavo_bow.h -- place recognition: a bag-of-binary-words keyframe index on the GPU (beyond the reference; exact).
 *
 * A vocabulary is W words of 256 bits, 1 <= W <= 4096: words[W][32] in featVec's byte / bit order, and idf_q8[W]
 * (uint16; NULL: every word weighs 256).  Both tables come from the host (ya_vo_amd/bow.py trains them); the device
 * never evaluates a logarithm.  With integer tf-idf vectors everything below is integer arithmetic plus one correctly
 * rounded double sqrt and one division, and is bit-exact against tests/bow_reference.py:
 *
 *   word of a descriptor   (d, w) = the lexicographic minimum of (Hamming(desc, words[w]), w) over w: what
 *                          yv_match_features returns with the vocabulary as the train list (first index on ties);
 *   vector of an image     c_w = its descriptors with word w, t_w = c_w * idf_q8[w] (int32), tmax = max t_w,
 *                          v_w = (127 * t_w) / tmax (floor) as int8, all zero when tmax == 0 (n == 0 included),
 *                          norm2 = sum v_w^2 (< 2^27);
 *   score of q against e   dot = sum vq_w * ve_w (int32, exact); score = (double)dot / sqrt((double)nq2 * (double)ne2),
 *                          0.0 when either norm is 0;
 *   candidates of a query  with frame id f, exclusion window x >= 0 and top_k in 1..16: the entries with
 *                          |f - frame_id_e| >= x and dot > 0, ranked by (score descending, entry index ascending),
 *                          the first top_k.  An entry's index is its insertion order.
 *
 * The entry count is host state: an add knows its n, so a query sees every entry whose add was enqueued before it.
 * A context or batch without a yv_bow launches and allocates nothing new.
 *
 * Argument checks come first, before the context or the object is looked at: YV_ERR_INVALID for a NULL required
 * pointer, n_words outside 1..4096, max_entries outside 1..65536, max_queries outside 1..4097, max_kp outside 1..4096,
 * top_k outside 1..16, exclude < 0 or n < 0; then YV_ERR_INVALID for a NULL context or object -- YV_ERR_NODEVICE
 * instead on a machine without a GPU (where none can exist), as in yv_match_knn2; then what needs the object:
 * YV_ERR_INVALID for a slot outside the batch or a batch whose max_kp exceeds the object's, YV_ERR_CAPACITY for
 * n > max_kp (host forms), n > max_queries (batch forms) and an add beyond max_entries, which leaves the index as it was.
 */
#ifndef YAVO_BOW_H
#define YAVO_BOW_H

#include <stdint.h>

#include "yavo_types.h"

#ifdef __cplusplus
extern "C" {
#endif

struct yv_ctx;
struct yv_batch;
typedef struct yv_bow yv_bow;

#define YV_BOW_MAX_WORDS 4096
#define YV_BOW_MAX_TOP_K 16

int yv_bow_create(struct yv_ctx* ctx, int n_words, const uint8_t* words /* [n_words][32] */,
                  const uint16_t* idf_q8 /* [n_words], may be NULL */, int max_entries /* 1..65536 */,
                  int max_queries /* 1..4097 */, int max_kp /* 1..4096 */, yv_bow** out);
void yv_bow_destroy(yv_bow* bow);
/* empties the index, keeps the vocabulary */
int yv_bow_reset(yv_bow* bow);
int yv_bow_count(yv_bow* bow, int* n_entries);

/* ---- host-pointer forms (synchronous, on the context's stream) ---- */
/* nearest word and its distance of each of n keypoints' descriptors (word, dist: capacity n) */
int yv_bow_words(yv_bow* bow, const yv_keypoint* kp, int n, int32_t* word, int32_t* dist);
/* the image's vector (vec: n_words int8) and its squared norm */
int yv_bow_vector(yv_bow* bow, const yv_keypoint* kp, int n, int8_t* vec, int32_t* norm2);
/* appends the image as entry yv_bow_count() */
int yv_bow_add(yv_bow* bow, const yv_keypoint* kp, int n, int64_t frame_id);
/* the image's candidates: entry / entry_frame / score / dot have capacity top_k (entry_frame and dot may be NULL),
 * *n_out = candidates written */
int yv_bow_query(yv_bow* bow, const yv_keypoint* kp, int n, int64_t frame_id, int64_t exclude, int top_k,
                 int32_t* entry, int64_t* entry_frame, double* score, int32_t* dot, int* n_out);

/* ---- batch forms: read the descriptors of the batch's slots in HBM (no copy of them), asynchronous on `stream`
 * (NULL: the context's); the caller orders them after the run that filled the slots and before the next one.  slots
 * and frame_ids are host arrays of n, copied at the call. ---- */
/* slot slots[i] becomes entry count + i with frame id frame_ids[i] */
int yv_bow_add_batch(yv_bow* bow, struct yv_batch* batch, const int32_t* slots, const int64_t* frame_ids, int n,
                     void* stream);
/* query i = slot slots[i] with frame id frame_ids[i]; the results are the view's q_* / dots / cand_* rows 0..n-1 */
int yv_bow_query_batch(yv_bow* bow, struct yv_batch* batch, const int32_t* slots, const int64_t* frame_ids, int n,
                       int64_t exclude, int top_k, void* stream);

typedef struct yv_bow_view {
    int n_words, w_pad;               /* w_pad: n_words rounded up to 64, the vectors' row length */
    int max_entries, max_queries, max_kp;
    int n_entries;                    /* entries whose add was enqueued so far */
    int n_queries;                    /* queries of the last query call */
    /* the index */
    const int8_t* vectors;            /* [max_entries][w_pad], pad bytes zero */
    const int32_t* norm2;             /* [max_entries] */
    const int64_t* frame_id;          /* [max_entries] */
    /* the last query call (q_word / q_dist: the last query or add call, which share the word stage's output) */
    const int32_t* q_word;            /* [max_queries][max_kp] */
    const int32_t* q_dist;            /* [max_queries][max_kp] */
    const int8_t* q_vectors;          /* [max_queries][w_pad] */
    const int32_t* q_norm2;           /* [max_queries] */
    const int32_t* dots;              /* [max_queries][max_entries], columns 0..n_entries-1 of the call */
    const int32_t* cand_entry;        /* [max_queries][16], -1 past cand_count */
    const double* cand_score;         /* [max_queries][16], 0 past cand_count */
    const int32_t* cand_dot;          /* [max_queries][16], 0 past cand_count */
    const int32_t* cand_count;        /* [max_queries] */
} yv_bow_view;
/* Device views (valid until yv_bow_destroy; complete once the stream of the call that wrote them has drained). */
int yv_bow_view_get(yv_bow* bow, yv_bow_view* view);
/* The last query call's candidate rows 0..n-1 copied device to device, asynchronously on `stream` (NULL: the
 * context's), into the caller's d_entry / d_score / d_dot ([n][16]) and d_count ([n]); any may be NULL.  A caller that
 * issues several query calls before it synchronises keeps each call's lists this way. */
int yv_bow_candidates_copy(yv_bow* bow, int n, int32_t* d_entry, double* d_score, int32_t* d_dot, int32_t* d_count,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YAVO_BOW_H */
