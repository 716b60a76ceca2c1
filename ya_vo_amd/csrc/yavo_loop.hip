// yavo_loop.hip -- loop closure: the keyframe store and the geometric verification of place-recognition candidates
// (include/yavo/yavo_loop.h).
//
// Verification composes stages the library already has, each called as it is: the matrix-core matcher with second-best
// keys and the reverse direction (launch_match), the filtering finalize without record lists (launch_match_finalize,
// match_pos set), P3P-RANSAC (launch_pnp_ransac, on a hypothesis workspace of the object's own) and the track layout's
// pose LM (launch_track_pose); the batch add takes its landmarks from launch_stereo_points.  What this file adds is
// glue: gathers and integer tests, no floating-point expression.
//
//   loop_store_kernel   batch add: a slot's descriptors, positions and count into entry e, the stereo points scattered
//                       by keypoint index into X[e] / has[e] (both rows written whole)
//   loop_stage_kernel   verify: the query slots into the staging slots behind the entries, so that one MatchLists
//                       serves launch_match with pairs (staging slot, entry)
//   loop_pairs_kernel   the (staging, entry) and swapped pair lists from the candidate rows; a skipped problem gets the
//                       empty slot on both sides, so the matcher and the finalize touch none of its keys
//   loop_edges_kernel   keep + match_dj + has -> compacted edges in query order, one workgroup per problem
//   loop_gate_kernel    after the RANSAC: the LM's edge count (0 where nothing was found, so the LM does no work there)
//                       and zeroed outlier flags where it will not run
//   loop_result_kernel  yv_loop_result per problem
//
// Slots of desc / pos / kp_count: [0, max_entries) the entries, [max_entries, max_entries + max_problems) staging, then
// one slot that is always empty.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yavo_host.h"
#include "yavo_wave.h"

namespace yavo {

constexpr int kLoopNT = 256;
constexpr int kLoopAddChunk = 256;  // entries per launch group of a batch add (its stereo points' staging)
constexpr int kLoopRing = 4;        // pinned host lists in flight (batch forms)
constexpr int kLoopCandStride = YV_LOOP_CAND_STRIDE;

// one keypoint list's descriptors (32 B each, as two 16-B words) and positions
__device__ __forceinline__ void loop_copy_list(const Desc* __restrict__ sd, const yv_keypoint* __restrict__ sk, int n,
                                               Desc* __restrict__ dd, int2* __restrict__ dp) {
    const uint4* s4 = reinterpret_cast<const uint4*>(sd);
    uint4* d4 = reinterpret_cast<uint4*>(dd);
    for (int k = (int)threadIdx.x; k < 2 * n; k += kLoopNT) d4[k] = s4[k];
    for (int j = (int)threadIdx.x; j < n; j += kLoopNT) dp[j] = make_int2(sk[j].x, sk[j].y);
}

// Entry e0 + t = slot slots[t] of the batch (lists of b_max_kp) with the stereo points of track t (pts_*, rows of
// b_max_kp: X, the keypoint index of each, their count).
__global__ __launch_bounds__(kLoopNT) void loop_store_kernel(
    const Desc* __restrict__ b_desc, const yv_keypoint* __restrict__ b_kp, const int32_t* __restrict__ b_count,
    int b_max_kp, const int32_t* __restrict__ slots, const int64_t* __restrict__ fids,
    const double* __restrict__ pts_X, const int32_t* __restrict__ pts_q, const int32_t* __restrict__ pts_count,
    int e0, int max_kp, Desc* __restrict__ desc, int2* __restrict__ pos, int32_t* __restrict__ kp_count,
    double* __restrict__ X, uint8_t* __restrict__ has, int64_t* __restrict__ frame_id) {
    __shared__ int s_idx[kMaxKp];  // keypoint -> its stereo point, -1: none
    const int t = blockIdx.x, tid = threadIdx.x, e = e0 + t, slot = slots[t];
    const int n = min(max(b_count[slot], 0), b_max_kp);
    loop_copy_list(b_desc + (int64_t)slot * b_max_kp, b_kp + (int64_t)slot * b_max_kp, n, desc + (int64_t)e * max_kp,
                   pos + (int64_t)e * max_kp);
    for (int j = tid; j < max_kp; j += kLoopNT) s_idx[j] = -1;
    __syncthreads();
    const int np = min(max(pts_count[t], 0), b_max_kp);
    const int64_t prow = (int64_t)t * b_max_kp;
    for (int c = tid; c < np; c += kLoopNT) {
        const int j = pts_q[prow + c];
        if (j >= 0 && j < n) s_idx[j] = c;
    }
    __syncthreads();
    const int64_t row = (int64_t)e * max_kp;
    for (int j = tid; j < max_kp; j += kLoopNT) has[row + j] = s_idx[j] >= 0 ? 1 : 0;
    for (int k = tid; k < 3 * max_kp; k += kLoopNT) {
        const int j = k / 3, c = s_idx[j];
        X[3 * row + k] = c >= 0 ? pts_X[3 * (prow + c) + (k - 3 * j)] : 0.0;
    }
    if (tid == 0) {
        kp_count[e] = n;
        frame_id[e] = fids[t];
    }
}

__global__ __launch_bounds__(kLoopNT) void loop_stage_kernel(const Desc* __restrict__ b_desc,
                                                             const yv_keypoint* __restrict__ b_kp,
                                                             const int32_t* __restrict__ b_count, int b_max_kp,
                                                             const int32_t* __restrict__ slots, int s0, int max_kp,
                                                             Desc* __restrict__ desc, int2* __restrict__ pos,
                                                             int32_t* __restrict__ kp_count) {
    const int q = blockIdx.x, slot = slots[q];
    const int n = min(max(b_count[slot], 0), b_max_kp);
    loop_copy_list(b_desc + (int64_t)slot * b_max_kp, b_kp + (int64_t)slot * b_max_kp, n,
                   desc + (int64_t)(s0 + q) * max_kp, pos + (int64_t)(s0 + q) * max_kp);
    if (threadIdx.x == 0) kp_count[s0 + q] = n;
}

// Problem v: top_k > 0: candidate k = v % top_k of query q = v / top_k (rows of kLoopCandStride, cand_count[q] valid);
// top_k == 0 (the host form): entry cand_entry[v] against the one query in staging slot s0.
__global__ __launch_bounds__(kLoopNT) void loop_pairs_kernel(const int32_t* __restrict__ cand_entry,
                                                             const int32_t* __restrict__ cand_count, int top_k,
                                                             int n_problems, int n_entries, int s0, int empty_slot,
                                                             int32_t* __restrict__ pairs, int32_t* __restrict__ pairs_rev,
                                                             int32_t* __restrict__ prob_entry) {
    const int v = blockIdx.x * kLoopNT + threadIdx.x;
    if (v >= n_problems) return;
    int q = 0, e;
    bool ok = true;
    if (top_k > 0) {
        q = v / top_k;
        const int k = v - q * top_k;
        e = cand_entry[q * kLoopCandStride + k];
        ok = k < cand_count[q];
    } else {
        e = cand_entry[v];
    }
    ok = ok && e >= 0 && e < n_entries;
    const int qs = ok ? s0 + q : empty_slot, ts = ok ? e : empty_slot;
    pairs[2 * v] = qs;
    pairs[2 * v + 1] = ts;
    pairs_rev[2 * v] = ts;
    pairs_rev[2 * v + 1] = qs;
    prob_entry[v] = ok ? e : -1;
}

__global__ __launch_bounds__(kLoopNT) void loop_edges_kernel(
    const int32_t* __restrict__ prob_entry, const int32_t* __restrict__ pairs, const int32_t* __restrict__ kp_count,
    const int2* __restrict__ pos, const double* __restrict__ X, const uint8_t* __restrict__ has,
    const uint8_t* __restrict__ keep, const int2* __restrict__ match_dj, int max_kp, double* __restrict__ edge_X,
    double* __restrict__ edge_uv, int32_t* __restrict__ edge_query, int32_t* __restrict__ edge_train,
    int32_t* __restrict__ edge_count) {
    __shared__ int s_tmp[40];
    const int v = blockIdx.x, tid = threadIdx.x;
    const int e = prob_entry[v], qs = pairs[2 * v];
    const int nq = e >= 0 ? min(kp_count[qs], max_kp) : 0;
    const int64_t row = (int64_t)v * max_kp, erow = (int64_t)max(e, 0) * max_kp, qrow = (int64_t)qs * max_kp;
    int ne = 0;
    for (int base = 0; base < nq; base += kLoopNT) {
        const int i = base + tid;
        int j = -1;
        bool good = false;
        if (i < nq && keep[row + i]) {
            j = match_dj[row + i].y;
            good = j >= 0 && j < max_kp && has[erow + j] != 0;
        }
        int tot = 0;
        const int off = block_excl_scan<kLoopNT>(good ? 1 : 0, s_tmp, &tot);
        if (good) {
            const int64_t o = row + ne + off;
            const int2 p = pos[qrow + i];
            edge_X[3 * o] = X[3 * (erow + j)];
            edge_X[3 * o + 1] = X[3 * (erow + j) + 1];
            edge_X[3 * o + 2] = X[3 * (erow + j) + 2];
            edge_uv[2 * o] = (double)p.x;
            edge_uv[2 * o + 1] = (double)p.y;
            edge_query[o] = i;
            edge_train[o] = j;
        }
        ne += tot;
    }
    if (tid == 0) edge_count[v] = ne;
}

__global__ __launch_bounds__(kLoopNT) void loop_gate_kernel(const int32_t* __restrict__ found,
                                                            const int32_t* __restrict__ edge_count, int max_kp,
                                                            int32_t* __restrict__ lm_count,
                                                            uint8_t* __restrict__ lm_outlier) {
    const int v = blockIdx.x;
    const int ne = min(edge_count[v], max_kp);
    const bool f = found[v] != 0;
    if (threadIdx.x == 0) lm_count[v] = f ? ne : 0;
    if (!f)
        for (int i = (int)threadIdx.x; i < ne; i += kLoopNT) lm_outlier[(int64_t)v * max_kp + i] = 0;
}

__global__ __launch_bounds__(kLoopNT) void loop_result_kernel(
    const int32_t* __restrict__ prob_entry, const int32_t* __restrict__ filt_count,
    const int32_t* __restrict__ edge_count, const int32_t* __restrict__ ransac_inliers,
    const int32_t* __restrict__ found, const int32_t* __restrict__ lm_inliers, const double* __restrict__ poses,
    int min_inliers, int n_problems, yv_loop_result* __restrict__ results) {
    const int v = blockIdx.x * kLoopNT + threadIdx.x;
    if (v >= n_problems) return;
    const int e = prob_entry[v];
    const bool f = e >= 0 && found[v] != 0;
    yv_loop_result r;
    r.entry = e;
    r.n_kept = e >= 0 ? filt_count[v] : 0;
    r.n_edges = e >= 0 ? edge_count[v] : 0;
    r.ransac_inliers = f ? ransac_inliers[v] : 0;
    r.lm_inliers = f ? lm_inliers[v] : 0;
    r.verified = f && r.lm_inliers >= min_inliers ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) r.pose[k] = f ? poses[7 * (int64_t)v + k] : (k == 3 ? 1.0 : 0.0);
    results[v] = r;
}

}  // namespace yavo

// ------------------------------------------------------------------------------------------------
// the object and the C ABI
// ------------------------------------------------------------------------------------------------
struct yv_loop {
    yv_ctx* ctx = nullptr;
    int max_entries = 0, max_problems = 0, max_kp = 0;
    int n_entries = 0, n_problems = 0;
    double K[9] = {}, T_right[7] = {};
    // yv_loop_set_params
    bool params = false;
    int match_thr = 0, flags = 0, num = 0, den = 1, iters = 0, min_inliers = 0;
    double thr_px = 0;
    yavo::HipOwned mem;  // every buffer and event below
    // the slots: entries, staging, the empty one
    Desc* desc = nullptr;          // [slots][max_kp]
    int2* pos = nullptr;           // [slots][max_kp]
    int32_t* kp_count = nullptr;   // [slots]
    double* X = nullptr;           // [max_entries][max_kp][3]
    uint8_t* has = nullptr;        // [max_entries][max_kp]
    int64_t* frame_id = nullptr;   // [max_entries]
    // a verify call's problems
    int32_t* pairs = nullptr;      // [max_problems][2] {staging slot, entry}
    int32_t* pairs_rev = nullptr;  // [max_problems][2]
    int32_t* prob_entry = nullptr; // [max_problems] -1: skipped
    uint32_t* match_key = nullptr; // [max_problems][max_kp], 0xFFFFFFFF between calls (as match_key2, rev_key)
    uint32_t* match_key2 = nullptr;
    uint32_t* rev_key = nullptr;
    int4* nn2 = nullptr;           // [max_problems][max_kp]
    int32_t* rev = nullptr;
    uint8_t* keep = nullptr;
    int2* match_dj = nullptr;
    int32_t* match_pos = nullptr;
    int32_t* match_lim = nullptr;  // [max_problems]
    int32_t* match_count = nullptr;
    int32_t* filt_count = nullptr;
    double* edge_X = nullptr;      // [max_problems][max_kp][3]
    double* edge_uv = nullptr;     // [max_problems][max_kp][2]
    int32_t* edge_query = nullptr; // [max_problems][max_kp]
    int32_t* edge_train = nullptr;
    int32_t* edge_count = nullptr; // [max_problems]
    int32_t* lm_count = nullptr;   // [max_problems] edge_count where a pose was found, else 0
    double* ransac_pose = nullptr; // [max_problems][7]
    uint8_t* ransac_inlier = nullptr;  // [max_problems][max_kp]
    int32_t* ransac_inliers = nullptr; // [max_problems]
    int32_t* found = nullptr;
    double* poses = nullptr;       // [max_problems][7]
    uint8_t* lm_outlier = nullptr; // [max_problems][max_kp]
    int32_t* lm_inliers = nullptr; // [max_problems]
    yv_loop_result* results = nullptr;  // [max_problems]
    double* d_K = nullptr;         // [max(max_problems, kLoopAddChunk)][9] K, once per problem / added entry
    double* d_T_right = nullptr;   // [7]
    double* d_identity = nullptr;  // [max_problems][7] the RANSAC's pose where nothing is found
    uint32_t* d_draws = nullptr;   // [kPnpMaxIters][3]
    void* pnp_ws = nullptr;        // pnp_ransac_ws_bytes(max_problems, iters): the object's own (the context's serves the
    size_t pnp_ws_cap = 0;         // batch's track RANSAC, which may run beside a verify call on another stream)
    // a batch add's stereo points, kLoopAddChunk tracks at a time
    double* pts_X = nullptr;       // [kLoopAddChunk][max_kp][3]
    float* pts_pt = nullptr;       // [kLoopAddChunk][max_kp][2]
    int32_t* pts_q = nullptr;      // [kLoopAddChunk][max_kp]
    int32_t* pts_count = nullptr;  // [kLoopAddChunk]
    int32_t* d_slots = nullptr;    // [max(max_problems, kLoopAddChunk)] the call's slots (host form: its entries)
    int32_t* d_sp = nullptr;       // [kLoopAddChunk] the add's stereo pairs
    int64_t* d_fids = nullptr;     // [kLoopAddChunk] the add's frame ids
    // the batch forms' pinned lists [slots | stereo pairs | frame ids], reused round robin once their copy has finished
    uint8_t* h_ring[yavo::kLoopRing] = {};
    hipEvent_t ev_ring[yavo::kLoopRing] = {};
    bool ring_used[yavo::kLoopRing] = {};
    int ring_next = 0;
    int stage_mask = 255;          // yv_debug_loop_stages: which stages a verify call launches
};

namespace {

using namespace yavo;

int no_object() { return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE; }

int list_cap(const yv_loop* w) { return std::max(w->max_problems, kLoopAddChunk); }
int staging0(const yv_loop* w) { return w->max_entries; }
int empty_slot(const yv_loop* w) { return w->max_entries + w->max_problems; }

bool params_ok(int flags, int num, int den, int iters, const uint32_t* draws, double thr_px, int min_inliers) {
    return match_filter_args_ok(flags, num, den) && draws && iters >= 1 && iters <= kPnpMaxIters && min_inliers >= 4 &&
           std::isfinite(thr_px) && thr_px > 0;
}

bool host_list_ok(const yv_keypoint* kp, int n) { return n >= 0 && (n == 0 || kp); }

// the next pinned list buffer, once the copies of its last use have finished
int ring_take(yv_loop* w, uint8_t** h, int* r_out) {
    const int r = w->ring_next;
    w->ring_next = (r + 1) % kLoopRing;
    if (w->ring_used[r]) YV_HIP(hipEventSynchronize(w->ev_ring[r]));
    *h = w->h_ring[r];
    *r_out = r;
    return YV_OK;
}

int ring_done(yv_loop* w, int r, hipStream_t s) {
    YV_HIP(hipEventRecord(w->ev_ring[r], s));
    w->ring_used[r] = true;
    return YV_OK;
}

// Everything of a verify call after the queries are staged and the candidate rows are on the device: n problems on s.
int verify_problems(yv_loop* w, const int32_t* d_cand_entry, const int32_t* d_cand_count, int top_k, int n,
                    hipStream_t s) {
    const int blocks = (n + kLoopNT - 1) / kLoopNT;
    const int mask = w->stage_mask;
    if (mask & 1)
        hipLaunchKernelGGL(loop_pairs_kernel, dim3(blocks), dim3(kLoopNT), 0, s, d_cand_entry, d_cand_count, top_k, n,
                           w->n_entries, staging0(w), empty_slot(w), w->pairs, w->pairs_rev, w->prob_entry);
    const MatchLists lists{w->desc, nullptr, w->kp_count, w->max_kp};
    if (mask & 2) {
        launch_match(lists, w->pairs, n, w->max_kp, w->match_key, w->match_key2, s);
        if (w->flags & kMatchMutual) launch_match(lists, w->pairs_rev, n, w->max_kp, w->rev_key, nullptr, s);
    }
    const bool ratio = (w->flags & kMatchRatio) != 0;
    const FinalizeRobust rb{w->match_key2, w->rev_key, w->flags, ratio ? w->num : 0, ratio ? w->den : 1, w->nn2, w->rev,
                            w->keep};
    // no record lists (match_pos set): matches / filtered stay null
    const MatchRecords out{nullptr, w->match_count, nullptr, w->filt_count, w->match_dj, w->match_lim, w->match_pos};
    if (mask & 4) launch_match_finalize(w->match_key, lists, w->pairs, n, w->match_thr, out, &rb, s);
    if (mask & 8)
        hipLaunchKernelGGL(loop_edges_kernel, dim3(n), dim3(kLoopNT), 0, s, w->prob_entry, w->pairs, w->kp_count,
                           w->pos, w->X, w->has, w->keep, w->match_dj, w->max_kp, w->edge_X, w->edge_uv, w->edge_query,
                           w->edge_train, w->edge_count);
    if (mask & 16)
        launch_pnp_ransac(nullptr, w->edge_count, w->max_kp, n, w->edge_X, w->edge_uv, w->d_K, w->d_draws, w->iters,
                          w->thr_px, w->min_inliers, w->d_identity, w->ransac_pose, w->ransac_inlier,
                          w->ransac_inliers, w->found, w->pnp_ws, s);
    if (mask & 32)
        hipLaunchKernelGGL(loop_gate_kernel, dim3(n), dim3(kLoopNT), 0, s, w->found, w->edge_count, w->max_kp,
                           w->lm_count, w->lm_outlier);
    if (mask & 64)
        launch_track_pose(n, w->lm_count, w->max_kp, w->edge_X, w->edge_uv, w->d_K, w->ransac_pose, w->poses,
                          w->lm_outlier, w->lm_inliers, s);
    if (mask & 128)
        hipLaunchKernelGGL(loop_result_kernel, dim3(blocks), dim3(kLoopNT), 0, s, w->prob_entry, w->filt_count,
                           w->edge_count, w->ransac_inliers, w->found, w->lm_inliers, w->poses, w->min_inliers, n,
                           w->results);
    w->n_problems = n;
    return check_launch();
}

}  // namespace

extern "C" {

int yv_loop_create(yv_ctx* ctx, const double K[9], const double T_right[7], int max_entries, int max_problems,
                   int max_kp, yv_loop** out) {
    if (!K || !T_right || !out || max_entries < 1 || max_entries > 65536 || max_problems < 1 ||
        max_problems > YV_LOOP_MAX_PROBLEMS || max_kp < 1 || max_kp > kMaxKp)
        return YV_ERR_INVALID;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return YV_ERR_INVALID;
    if (!finite_pose(T_right)) return YV_ERR_INVALID;
    *out = nullptr;
    if (!ctx) return no_object();
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    yv_loop* w = new (std::nothrow) yv_loop;
    if (!w) return YV_ERR_HIP;
    w->ctx = ctx;
    w->max_entries = max_entries;
    w->max_problems = max_problems;
    w->max_kp = max_kp;
    std::memcpy(w->K, K, sizeof(w->K));
    std::memcpy(w->T_right, T_right, sizeof(w->T_right));
    const size_t ne = (size_t)max_entries, np = (size_t)max_problems, nk = (size_t)max_kp;
    const size_t ns = ne + np + 1, nl = (size_t)list_cap(w), na = (size_t)kLoopAddChunk;
    yavo::HipOwned& m = w->mem;
    int rc = YV_OK;
    rc |= m.alloc(&w->desc, ns * nk);
    rc |= m.alloc(&w->pos, ns * nk);
    rc |= m.alloc(&w->kp_count, ns);
    rc |= m.alloc(&w->X, ne * nk * 3);
    rc |= m.alloc(&w->has, ne * nk);
    rc |= m.alloc(&w->frame_id, ne);
    rc |= m.alloc(&w->pairs, np * 2);
    rc |= m.alloc(&w->pairs_rev, np * 2);
    rc |= m.alloc(&w->prob_entry, np);
    rc |= m.alloc(&w->match_key, np * nk);
    rc |= m.alloc(&w->match_key2, np * nk);
    rc |= m.alloc(&w->rev_key, np * nk);
    rc |= m.alloc(&w->nn2, np * nk);
    rc |= m.alloc(&w->rev, np * nk);
    rc |= m.alloc(&w->keep, np * nk);
    rc |= m.alloc(&w->match_dj, np * nk);
    rc |= m.alloc(&w->match_pos, np * nk);
    rc |= m.alloc(&w->match_lim, np);
    rc |= m.alloc(&w->match_count, np);
    rc |= m.alloc(&w->filt_count, np);
    rc |= m.alloc(&w->edge_X, np * nk * 3);
    rc |= m.alloc(&w->edge_uv, np * nk * 2);
    rc |= m.alloc(&w->edge_query, np * nk);
    rc |= m.alloc(&w->edge_train, np * nk);
    rc |= m.alloc(&w->edge_count, np);
    rc |= m.alloc(&w->lm_count, np);
    rc |= m.alloc(&w->ransac_pose, np * 7);
    rc |= m.alloc(&w->ransac_inlier, np * nk);
    rc |= m.alloc(&w->ransac_inliers, np);
    rc |= m.alloc(&w->found, np);
    rc |= m.alloc(&w->poses, np * 7);
    rc |= m.alloc(&w->lm_outlier, np * nk);
    rc |= m.alloc(&w->lm_inliers, np);
    rc |= m.alloc(&w->results, np);
    rc |= m.alloc(&w->d_K, nl * 9);
    rc |= m.alloc(&w->d_T_right, 7);
    rc |= m.alloc(&w->d_identity, np * 7);
    rc |= m.alloc(&w->d_draws, 3 * (size_t)kPnpMaxIters);
    rc |= m.alloc(&w->pts_X, na * nk * 3);
    rc |= m.alloc(&w->pts_pt, na * nk * 2);
    rc |= m.alloc(&w->pts_q, na * nk);
    rc |= m.alloc(&w->pts_count, na);
    rc |= m.alloc(&w->d_slots, nl);
    rc |= m.alloc(&w->d_sp, na);
    rc |= m.alloc(&w->d_fids, na);
    bool ok = rc == YV_OK;
    for (int r = 0; ok && r < kLoopRing; ++r)
        ok = m.alloc_host(&w->h_ring[r], nl * 16) == YV_OK && m.event(&w->ev_ring[r]) == hipSuccess;
    hipStream_t s = ctx->stream;
    // the key buffers as the finalize leaves them, every count zero (the empty slot's for good), the view's arrays
    // defined from the start
    ok = ok && hipMemsetAsync(w->match_key, 0xFF, np * nk * sizeof(uint32_t), s) == hipSuccess &&
         hipMemsetAsync(w->match_key2, 0xFF, np * nk * sizeof(uint32_t), s) == hipSuccess &&
         hipMemsetAsync(w->rev_key, 0xFF, np * nk * sizeof(uint32_t), s) == hipSuccess &&
         hipMemsetAsync(w->kp_count, 0, ns * sizeof(int32_t), s) == hipSuccess &&
         hipMemsetAsync(w->has, 0, ne * nk, s) == hipSuccess &&
         hipMemsetAsync(w->frame_id, 0, ne * sizeof(int64_t), s) == hipSuccess &&
         hipMemsetAsync(w->edge_count, 0, np * sizeof(int32_t), s) == hipSuccess &&
         hipMemsetAsync(w->ransac_inlier, 0, np * nk, s) == hipSuccess &&
         hipMemsetAsync(w->lm_outlier, 0, np * nk, s) == hipSuccess &&
         hipMemsetAsync(w->results, 0, np * sizeof(yv_loop_result), s) == hipSuccess;
    if (ok) {
        std::vector<double> hk(nl * 9), hi(np * 7, 0.0);
        for (size_t p = 0; p < nl; ++p) std::memcpy(&hk[9 * p], K, 9 * sizeof(double));
        for (size_t p = 0; p < np; ++p) hi[7 * p + 3] = 1.0;
        StageScope stage_scope(ctx);
        ok = stage_h2d(ctx, w->d_K, hk.data(), hk.size() * sizeof(double), s) == hipSuccess &&
             stage_h2d(ctx, w->d_identity, hi.data(), hi.size() * sizeof(double), s) == hipSuccess &&
             stage_h2d(ctx, w->d_T_right, T_right, 7 * sizeof(double), s) == hipSuccess &&
             stage_sync(ctx, s) == hipSuccess;
    }
    if (!ok) {
        (void)hipDeviceSynchronize();
        delete w;
        return YV_ERR_HIP;
    }
    *out = w;
    return YV_OK;
}

void yv_loop_destroy(yv_loop* w) {
    if (!w) return;
    if (set_device(w->ctx) == YV_OK) (void)hipDeviceSynchronize();  // a batch form may run on a stream of the caller's
    delete w;
}

int yv_loop_reset(yv_loop* w) {
    if (!w) return no_object();
    w->n_entries = 0;
    return YV_OK;
}

int yv_loop_count(yv_loop* w, int* n_entries) {
    if (!n_entries) return YV_ERR_INVALID;
    if (!w) return no_object();
    *n_entries = w->n_entries;
    return YV_OK;
}

int yv_loop_set_params(yv_loop* w, int match_thr, int flags, int ratio_num, int ratio_den, int iters,
                       const uint32_t* draws, double thr_px, int min_inliers) {
    if (!params_ok(flags, ratio_num, ratio_den, iters, draws, thr_px, min_inliers)) return YV_ERR_INVALID;
    if (!w) return no_object();
    yv_ctx* ctx = w->ctx;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    const size_t need = pnp_ransac_ws_bytes(w->max_problems, iters);
    if (need > w->pnp_ws_cap) {  // outside any timed loop; earlier launches that use it have finished
        YV_HIP(hipDeviceSynchronize());
        w->mem.release(w->pnp_ws);
        w->pnp_ws_cap = 0;
        if (w->mem.alloc(&w->pnp_ws, need) != YV_OK) return YV_ERR_HIP;
        w->pnp_ws_cap = need;
    }
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    YV_HIP(stage_h2d(ctx, w->d_draws, draws, sizeof(uint32_t) * 3 * (size_t)iters, s));
    YV_HIP(stage_sync(ctx, s));
    w->match_thr = match_thr;
    w->flags = flags;
    w->num = ratio_num;
    w->den = ratio_den;
    w->iters = iters;
    w->thr_px = thr_px;
    w->min_inliers = min_inliers;
    w->params = true;
    return YV_OK;
}

int yv_loop_lm_sum_mode(int n_problems) { return yv_track_lm_sum_mode(n_problems); }

int yv_loop_add(yv_loop* w, const yv_keypoint* kp, int n, const double* X, const uint8_t* has, int64_t frame_id) {
    if (!host_list_ok(kp, n) || ((X == nullptr) != (has == nullptr))) return YV_ERR_INVALID;
    if (!w) return no_object();
    if (n > w->max_kp || w->n_entries + 1 > w->max_entries) return YV_ERR_CAPACITY;
    yv_ctx* ctx = w->ctx;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    const size_t nk = (size_t)w->max_kp, e = (size_t)w->n_entries;
    std::vector<Desc> hd((size_t)std::max(n, 1));
    std::vector<int2> hp((size_t)std::max(n, 1));
    std::vector<double> hx(3 * nk, 0.0);
    std::vector<uint8_t> hh(nk, 0);
    for (int j = 0; j < n; ++j) {
        std::memcpy(&hd[(size_t)j], kp[j].featVec, sizeof(Desc));
        hp[(size_t)j] = make_int2(kp[j].x, kp[j].y);
        if (has && has[j]) {
            hh[(size_t)j] = 1;
            std::memcpy(&hx[3 * (size_t)j], X + 3 * (size_t)j, 3 * sizeof(double));
        }
    }
    if (n > 0) {
        YV_HIP(stage_h2d(ctx, w->desc + e * nk, hd.data(), sizeof(Desc) * (size_t)n, s));
        YV_HIP(stage_h2d(ctx, w->pos + e * nk, hp.data(), sizeof(int2) * (size_t)n, s));
    }
    YV_HIP(stage_h2d(ctx, w->X + 3 * e * nk, hx.data(), sizeof(double) * 3 * nk, s));
    YV_HIP(stage_h2d(ctx, w->has + e * nk, hh.data(), nk, s));
    const int32_t cnt = n;
    YV_HIP(stage_h2d(ctx, w->kp_count + e, &cnt, sizeof(cnt), s));
    YV_HIP(stage_h2d(ctx, w->frame_id + e, &frame_id, sizeof(frame_id), s));
    YV_HIP(stage_sync(ctx, s));
    w->n_entries = (int)e + 1;
    return YV_OK;
}

int yv_loop_verify(yv_loop* w, const yv_keypoint* q, int nq, const int32_t* entries, int n, yv_loop_result* results) {
    if (!host_list_ok(q, nq) || n < 0 || (n > 0 && (!entries || !results))) return YV_ERR_INVALID;
    if (!w) return no_object();
    if (!w->params) return YV_ERR_INVALID;
    if (nq > w->max_kp || n > w->max_problems) return YV_ERR_CAPACITY;
    if (n == 0) {
        w->n_problems = 0;
        return YV_OK;
    }
    yv_ctx* ctx = w->ctx;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    const size_t nk = (size_t)w->max_kp, s0 = (size_t)staging0(w);
    std::vector<Desc> hd((size_t)std::max(nq, 1));
    std::vector<int2> hp((size_t)std::max(nq, 1));
    for (int i = 0; i < nq; ++i) {
        std::memcpy(&hd[(size_t)i], q[i].featVec, sizeof(Desc));
        hp[(size_t)i] = make_int2(q[i].x, q[i].y);
    }
    if (nq > 0) {
        YV_HIP(stage_h2d(ctx, w->desc + s0 * nk, hd.data(), sizeof(Desc) * (size_t)nq, s));
        YV_HIP(stage_h2d(ctx, w->pos + s0 * nk, hp.data(), sizeof(int2) * (size_t)nq, s));
    }
    const int32_t cnt = nq;
    YV_HIP(stage_h2d(ctx, w->kp_count + s0, &cnt, sizeof(cnt), s));
    YV_HIP(stage_h2d(ctx, w->d_slots, entries, sizeof(int32_t) * (size_t)n, s));
    const int st = verify_problems(w, w->d_slots, nullptr, 0, n, s);
    if (st != YV_OK) return st;
    YV_HIP(stage_d2h(ctx, results, w->results, sizeof(yv_loop_result) * (size_t)n, s));
    YV_HIP(stage_sync(ctx, s));
    return YV_OK;
}

int yv_loop_add_batch(yv_loop* w, yv_batch* b, const int32_t* left_slots, const int32_t* stereo_pairs,
                      const int64_t* frame_ids, int n, void* stream) {
    if (n < 0 || (n > 0 && (!left_slots || !stereo_pairs || !frame_ids))) return YV_ERR_INVALID;
    if (!w || !b) return no_object();
    if (b->max_kp > w->max_kp) return YV_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const int sp = stereo_pairs[i];
        if (left_slots[i] < 0 || left_slots[i] >= b->nslots || sp < 0 || sp >= b->n_pairs ||
            (size_t)(2 * sp + 1) >= b->h_pairs.size() || b->h_pairs[2 * (size_t)sp] != left_slots[i])
            return YV_ERR_INVALID;
    }
    if (w->n_entries + n > w->max_entries) return YV_ERR_CAPACITY;
    if (n == 0) return YV_OK;
    if (set_device(w->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w->ctx->stream;
    // the batch's stereo leg as yv_batch_track reads it, with the object's own K and T_right
    const bool sub = b->subpix_on;
    const TrackSrc src{b->pairs,
                       b->keypoints,
                       b->kp_count,
                       b->match_dj,
                       b->match_lim,
                       b->max_kp,
                       w->d_K,
                       w->d_T_right,
                       b->run_flags ? b->keep : nullptr,
                       sub ? b->subpix_dcol : nullptr,
                       sub ? b->subpix_status : nullptr,
                       sub && (b->subpix_flags & YV_SUBPIX_DROP_EDGE) != 0};
    const PointsOut pts{w->pts_X, w->pts_pt, w->pts_q, w->pts_count};
    const size_t nl = (size_t)list_cap(w);
    for (int i0 = 0; i0 < n; i0 += kLoopAddChunk) {
        const int m = std::min(kLoopAddChunk, n - i0);
        uint8_t* h = nullptr;
        int r = 0;
        if (ring_take(w, &h, &r) != YV_OK) return YV_ERR_HIP;
        int32_t* hs = reinterpret_cast<int32_t*>(h);
        int32_t* hsp = reinterpret_cast<int32_t*>(h + 4 * nl);
        int64_t* hf = reinterpret_cast<int64_t*>(h + 8 * nl);
        for (int i = 0; i < m; ++i) {
            hs[i] = left_slots[i0 + i];
            hsp[i] = stereo_pairs[i0 + i];
            hf[i] = frame_ids[i0 + i];
        }
        YV_HIP(hipMemcpyAsync(w->d_slots, hs, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, s));
        YV_HIP(hipMemcpyAsync(w->d_sp, hsp, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, s));
        YV_HIP(hipMemcpyAsync(w->d_fids, hf, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, s));
        if (ring_done(w, r, s) != YV_OK) return YV_ERR_HIP;
        launch_stereo_points(w->d_sp, m, src, pts, s);
        hipLaunchKernelGGL(loop_store_kernel, dim3(m), dim3(kLoopNT), 0, s, b->desc, b->keypoints, b->kp_count,
                           b->max_kp, w->d_slots, w->d_fids, w->pts_X, w->pts_q, w->pts_count, w->n_entries, w->max_kp,
                           w->desc, w->pos, w->kp_count, w->X, w->has, w->frame_id);
        if (check_launch() != YV_OK) return YV_ERR_HIP;
        w->n_entries += m;
    }
    return YV_OK;
}

int yv_loop_verify_batch(yv_loop* w, yv_batch* b, const int32_t* slots, int nq, const int32_t* d_cand_entry,
                         const int32_t* d_cand_count, int top_k, void* stream) {
    if (nq < 0 || (nq > 0 && (!slots || !d_cand_entry || !d_cand_count)) || top_k < 1 || top_k > kLoopCandStride)
        return YV_ERR_INVALID;
    if (!w || !b) return no_object();
    if (b->max_kp > w->max_kp || !w->params) return YV_ERR_INVALID;
    for (int i = 0; i < nq; ++i)
        if (slots[i] < 0 || slots[i] >= b->nslots) return YV_ERR_INVALID;
    if ((int64_t)nq * top_k > w->max_problems) return YV_ERR_CAPACITY;
    if (nq == 0) {
        w->n_problems = 0;
        return YV_OK;
    }
    if (set_device(w->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w->ctx->stream;
    uint8_t* h = nullptr;
    int r = 0;
    if (ring_take(w, &h, &r) != YV_OK) return YV_ERR_HIP;
    int32_t* hs = reinterpret_cast<int32_t*>(h);
    for (int i = 0; i < nq; ++i) hs[i] = slots[i];
    YV_HIP(hipMemcpyAsync(w->d_slots, hs, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    if (ring_done(w, r, s) != YV_OK) return YV_ERR_HIP;
    if (w->stage_mask & 1)
        hipLaunchKernelGGL(loop_stage_kernel, dim3(nq), dim3(kLoopNT), 0, s, b->desc, b->keypoints, b->kp_count,
                           b->max_kp, w->d_slots, staging0(w), w->max_kp, w->desc, w->pos, w->kp_count);
    return verify_problems(w, d_cand_entry, d_cand_count, top_k, nq * top_k, s);
}

int yv_loop_view_get(yv_loop* w, yv_loop_view* v) {
    if (!v) return YV_ERR_INVALID;
    if (!w) return no_object();
    v->max_entries = w->max_entries;
    v->max_problems = w->max_problems;
    v->max_kp = w->max_kp;
    v->n_entries = w->n_entries;
    v->n_problems = w->n_problems;
    v->desc = reinterpret_cast<const uint8_t*>(w->desc);
    v->pos = reinterpret_cast<const int32_t*>(w->pos);
    v->X = w->X;
    v->has = w->has;
    v->kp_count = w->kp_count;
    v->frame_id = w->frame_id;
    v->results = w->results;
    v->edge_X = w->edge_X;
    v->edge_uv = w->edge_uv;
    v->edge_query = w->edge_query;
    v->edge_train = w->edge_train;
    v->ransac_inlier = w->ransac_inlier;
    v->lm_outlier = w->lm_outlier;
    v->edge_count = w->edge_count;
    return YV_OK;
}

int yv_loop_results_copy(yv_loop* w, int n, yv_loop_result* d_results, void* stream) {
    if (n < 0 || (n > 0 && !d_results)) return YV_ERR_INVALID;
    if (!w) return no_object();
    if (n > w->max_problems) return YV_ERR_CAPACITY;
    if (n == 0) return YV_OK;
    if (set_device(w->ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w->ctx->stream;
    YV_HIP(hipMemcpyAsync(d_results, w->results, sizeof(yv_loop_result) * (size_t)n, hipMemcpyDeviceToDevice, s));
    return YV_OK;
}

// Measurement entry points (tools/bench_loop.py; like yv_debug_xlane not part of the public headers).
// Which stages the following verify calls launch: bit 0 stage + pairs, 1 the matcher (both directions), 2 the finalize,
// 3 edges, 4 the RANSAC, 5 gate, 6 the LM, 7 result (255: all, the default).  A call with a stage left out reads what
// the last full call left in that stage's output.
int yv_debug_loop_stages(yv_loop* w, int mask) {
    if (!w || mask < 0 || mask > 255) return YV_ERR_INVALID;
    w->stage_mask = mask;
    return YV_OK;
}

// launch_match alone with second-best keys on device buffers of the caller's: desc [slots][max_kp] (32 B each),
// kp_count [slots], pairs [n_pairs][2], match_key / match_key2 [n_pairs][max_kp] (match_key2 NULL: best keys only) --
// the yardstick of a verify call's matcher.
int yv_debug_loop_match(yv_ctx* ctx, const void* d_desc, const int32_t* d_kp_count, int max_kp, const int32_t* d_pairs,
                        int n_pairs, int max_train, uint32_t* d_match_key, uint32_t* d_match_key2, void* stream) {
    if (!ctx || !d_desc || !d_kp_count || !d_pairs || !d_match_key || max_kp < 1 || max_kp > kMaxKp || n_pairs < 1 ||
        n_pairs > 65535 || max_train < 0 || max_train > kMaxKp)
        return YV_ERR_INVALID;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
    const MatchLists lists{static_cast<const Desc*>(d_desc), nullptr, d_kp_count, max_kp};
    launch_match(lists, d_pairs, n_pairs, max_train, d_match_key, d_match_key2, s);
    return check_launch();
}

}  // extern "C"
