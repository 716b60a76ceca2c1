// yavo_ba_window_tracks.hip -- the multi-view mode of the sliding BA window (yv_ba_window_set_multiview): the kernels
// that link a frame's records to the records of the frame before (query / train keypoint indices of the temporal
// match) and build the window graph over the chains (ya_vo_amd/sequence.py window_problem_tracks, restated).  The
// window itself, its store and the C ABI are yavo_ba_window.hip's; this file holds what only the mode needs.
//
// The graph.  Node (i, l) = record l of window pose i >= 1, id = i * max_lm + l.  A chain rooted at pose a with m
// nodes is one landmark seen by poses s = a - 1 .. e = a + m - 1; landmarks ascend by (a, m, root's l), edges are
// landmark-major in pose order.  With cnt[s][e] the landmarks per pose range ("class") and r a landmark's stable rank
// in its class, every index array yv_ba_set_problem would build from that edge list is closed-form:
//   landmark  = lbase[s][e] + r                       lbase: classes before in (s, e) order
//   its edges = ebase[s][e] + r (e - s + 1) + (p - s) for pose p
//   its place in the list of a pose pair (p1 <= p2) -- the landmarks with s <= p1 and e >= p2, ascending --
//             = A[s][p2] + RP[s][e] - RP[s][p2] + r   A[s][p2] = sum_{s' < s, e' >= p2} cnt, RP[s][x] = sum_{e' < x} cnt[s][e']
//     which does not depend on p1; pose p's edge list is the pair (p, p).
// No atomic decides an order: the two integer atomics (min of l per train keypoint, max of the depth per chain) give
// the same value in any order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yavo/yavo.h"
#include "../../include/yavo/yavo_map.h"
#include "yavo_host.h"
#include "yavo_internal.h"
#include "yavo_se3.h"
#include "yavo_wave.h"

using yavo::WinTracks;
using yavo::se3::se3_inverse;

namespace {

constexpr int kNone = 0x7fffffff;

// ---- add: one workgroup per keyframe of the block win_add_kernel just recorded ----

// query / train of every record and the frame's table train keypoint -> smallest record index
__global__ __launch_bounds__(256) void wint_record_kernel(const uint8_t* __restrict__ block,
                                                          const int32_t* __restrict__ edge_query,
                                                          const int32_t* __restrict__ match_dj, int64_t dj_stride,
                                                          int max_kp, int64_t g0, int64_t cap, int max_lm,
                                                          int32_t* __restrict__ query, int32_t* __restrict__ train,
                                                          int32_t* __restrict__ tab) {
    const yv_map_header* h = reinterpret_cast<const yv_map_header*>(block);
    const int j = blockIdx.x;
    if (j >= h->n_kf) return;
    const yv_keyframe* kf = reinterpret_cast<const yv_keyframe*>(block + sizeof(yv_map_header)) + j;
    const int64_t lmo = ((int64_t)sizeof(yv_map_header) + (int64_t)h->max_kf * (int64_t)sizeof(yv_keyframe) + 255) & ~255ll;
    const yv_landmark* lm = reinterpret_cast<const yv_landmark*>(block + lmo) + (int64_t)j * h->lm_stride;
    const int64_t s = kf->frame_id - g0, k64 = kf->frame_id - h->first_frame;
    if (s < 0 || s >= cap || k64 < 0 || k64 >= h->n_frames) return;
    const int n = min(kf->n_landmarks, max_lm);
    int32_t* t = tab + s * max_lm;
    for (int x = threadIdx.x; x < max_lm; x += 256) t[x] = kNone;
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += 256) {
        const int e = (int)(lm[l].id & 0xFFFF);
        const int q = edge_query[k64 * max_kp + e];
        const int tr = match_dj[((2 * k64) * dj_stride + q) * 2 + 1];  // the temporal pair's {distance, train}
        query[s * max_lm + l] = q;
        train[s * max_lm + l] = tr;
        if (tr >= 0 && tr < max_lm) atomicMin(&t[tr], l);
    }
}

// parent of every record (the record of the frame before whose train keypoint is this record's query, the smallest
// index where several share it; -1 without one) and the frame's root count, beside the counts win_add_kernel left
__global__ __launch_bounds__(256) void wint_link_kernel(const uint8_t* __restrict__ block, int64_t carry_frame,
                                                        int64_t g0, int64_t cap, int max_lm,
                                                        const int32_t* __restrict__ query,
                                                        const int32_t* __restrict__ tab, int32_t* __restrict__ parent,
                                                        int64_t* __restrict__ roots) {
    __shared__ int s_roots;
    const yv_map_header* h = reinterpret_cast<const yv_map_header*>(block);
    const int j = blockIdx.x;
    if (j >= h->n_kf) return;
    const yv_keyframe* kfs = reinterpret_cast<const yv_keyframe*>(block + sizeof(yv_map_header));
    const int64_t g = kfs[j].frame_id, s = g - g0, k64 = g - h->first_frame;
    if (s < 0 || s >= cap || k64 < 0 || k64 >= h->n_frames) return;
    // the frame before is recorded: by this block, or (the block's first frame) by an earlier one
    bool prev = s >= 1 && g - 1 == carry_frame;
    for (int i = 0; i < h->n_kf && !prev; ++i) {
        const int64_t k2 = kfs[i].frame_id - h->first_frame;
        prev = s >= 1 && kfs[i].frame_id == g - 1 && k2 >= 0 && k2 < h->n_frames;
    }
    const int n = min(kfs[j].n_landmarks, max_lm);
    if (threadIdx.x == 0) s_roots = 0;
    __syncthreads();
    int mine = 0;
    for (int l = threadIdx.x; l < n; l += 256) {
        const int q = query[s * max_lm + l];
        int p = -1;
        if (prev && q >= 0 && q < max_lm) {
            const int v = tab[(s - 1) * max_lm + q];
            p = v == kNone ? -1 : v;
        }
        parent[s * max_lm + l] = p;
        mine += p < 0;
    }
    if (mine) atomicAdd(&s_roots, mine);
    __syncthreads();
    if (threadIdx.x == 0) roots[j] = s_roots;
}

// ---- graph build: grid (tiles of 256 records, window poses 1 .. P-1) unless noted ----

// every node points at its parent (itself: a root; all of pose 1 are roots), chain lengths and class counts cleared,
// the poses as T_cw
__global__ __launch_bounds__(256) void wint_init_kernel(WinTracks W, const int32_t* __restrict__ cnt_f,
                                                        const int32_t* __restrict__ parent, const double* __restrict__ T,
                                                        double* __restrict__ poses) {
    const int i = blockIdx.y + 1, l = blockIdx.x * 256 + threadIdx.x;
    const int flat = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    if (flat < W.P) se3_inverse(T + (W.s0 + flat) * 7, poses + 7 * flat);
    for (int x = flat; x < W.P * W.P; x += gridDim.x * gridDim.y * 256) W.cnt[x] = 0;
    if (l >= cnt_f[W.s0 + i]) return;
    const int id = i * W.max_lm + l;
    const int p = i >= 2 ? parent[(W.s0 + i) * W.max_lm + l] : -1;
    W.up[id] = p < 0 ? id : id - W.max_lm - l + p;
    W.len[id] = 0;
}

// one round of pointer doubling, in place: up[] always names an ancestor, a racing read only a further one, so after
// k rounds every node is at least min(2^k, depth) steps up, and at the root after ceil(log2(depth)) rounds.  The last
// round leaves the chain's length (deepest node's depth + 1) at the root.
__global__ __launch_bounds__(256) void wint_jump_kernel(WinTracks W, const int32_t* __restrict__ cnt_f, int last) {
    const int i = blockIdx.y + 1, l = blockIdx.x * 256 + threadIdx.x;
    if (l >= cnt_f[W.s0 + i]) return;
    const int id = i * W.max_lm + l;
    const int u = __hip_atomic_load(&W.up[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int r = __hip_atomic_load(&W.up[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r != u) __hip_atomic_store(&W.up[id], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (last) atomicMax(&W.len[r], i - r / W.max_lm + 1);
}

// one wave per pose a: the roots' stable rank among the roots of the same chain length (a counting sort's rank, the
// running counts per length in LDS), and the class counts cnt[a - 1][a + m - 1]
__global__ __launch_bounds__(64) void wint_rank_kernel(WinTracks W, const int32_t* __restrict__ cnt_f) {
    __shared__ int s_run[128];
    const int a = blockIdx.x + 1, lane = threadIdx.x;
    const int n = cnt_f[W.s0 + a];
    s_run[lane] = 0;
    s_run[lane + 64] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int l0 = 0; l0 < n; l0 += 64) {
        const int l = l0 + lane, id = a * W.max_lm + l;
        int key = -1;
        if (l < n && W.up[id] == id) key = W.len[id];  // 1 .. P - a
        unsigned long long todo = __ballot(key >= 0);
        while (todo) {  // one turn per distinct length among the 64
            const int k = __shfl(key, __ffsll((long long)todo) - 1, 64);
            const unsigned long long same = __ballot(key == k);
            const int base = s_run[k & 127];
            if (key == k) W.rank[id] = base + __popcll(same & below);
            __syncthreads();
            if (lane == 0) s_run[k & 127] = base + __popcll(same);
            __syncthreads();
            todo &= ~same;
        }
    }
    for (int m = 1 + lane; a + m - 1 < W.P; m += 64) W.cnt[(a - 1) * W.P + a + m - 1] = s_run[m & 127];
}

// one workgroup: everything that is a prefix sum of cnt -- RP, lbase, ebase, A -- and with them pe_off and cv_off.
// Thread t owns row s = t (then column p2 = t); the row bases come from one block scan each.
__global__ __launch_bounds__(256) void wint_tables_kernel(WinTracks W, int32_t* __restrict__ pe_off,
                                                          int32_t* __restrict__ cv_off) {
    __shared__ int s_tmp[16];
    const int P = W.P, t = threadIdx.x;
    int row_l = 0, row_e = 0;
    if (t < P)
        for (int e = 0; e < P; ++e) {
            const int c = W.cnt[t * P + e];
            W.rp[t * P + e] = row_l;
            W.ebase[t * P + e] = row_e;
            row_l += c;
            row_e += c * (e - t + 1);
        }
    const int base_l = yavo::block_excl_scan<256>(row_l, s_tmp, nullptr);
    const int base_e = yavo::block_excl_scan<256>(row_e, s_tmp, nullptr);
    if (t < P)
        for (int e = 0; e < P; ++e) {
            W.lbase[t * P + e] = base_l + W.rp[t * P + e];
            W.ebase[t * P + e] += base_e;
        }
    if (t < P) W.rtot[t] = row_l;
    __syncthreads();  // rp and rtot of every row
    // column p2 = t: A[s][p2] for s = 0 .. P, the landmarks of rows before s that reach p2
    if (t < P) {
        int acc = 0;
        for (int s = 0; s <= P; ++s) {
            W.A[s * P + t] = acc;
            if (s < P) acc += W.rtot[s] - W.rp[s * P + t];
        }
    }
    __syncthreads();
    // the list of the pair (p1, p2), p1 <= p2, holds A[p1 + 1][p2] landmarks; pose p's edges are the pair (p, p)
    const int deg = t < P ? W.A[(t + 1) * P + t] : 0;
    int row_c = 0;
    if (t < P)
        for (int p2 = t; p2 < P; ++p2) row_c += W.A[(t + 1) * P + p2];
    const int pe0 = yavo::block_excl_scan<256>(deg, s_tmp, nullptr);
    int cv0 = yavo::block_excl_scan<256>(row_c, s_tmp, nullptr);
    if (t < P) {
        pe_off[t] = pe0;
        if (t == P - 1) pe_off[P] = pe0 + deg;
        if (t == 0) cv_off[0] = 0;
        for (int p2 = 0; p2 < P; ++p2) {
            if (p2 >= t) cv0 += W.A[(t + 1) * P + p2];
            cv_off[1 + t * P + p2] = cv0;
        }
    }
}

// every node writes its edge and that edge's entries in the pose, landmark and pose-pair lists; a root also the edge
// of the pose before it, the landmark's X and its le_off
__global__ __launch_bounds__(256) void wint_write_kernel(WinTracks W, int L, int E, const int32_t* __restrict__ cnt_f,
                                                         const double* __restrict__ Xs, const double* __restrict__ uvo,
                                                         const double* __restrict__ uvp, double* __restrict__ X,
                                                         int32_t* __restrict__ ep, int32_t* __restrict__ el,
                                                         double* __restrict__ meas, int32_t* __restrict__ le_off,
                                                         int32_t* __restrict__ le, const int32_t* __restrict__ pe_off,
                                                         int32_t* __restrict__ pe, const int32_t* __restrict__ cv_off,
                                                         int32_t* __restrict__ cv1, int32_t* __restrict__ cv2) {
    const int i = blockIdx.y + 1, l = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) le_off[L] = E;
    if (l >= cnt_f[W.s0 + i]) return;
    const int P = W.P, id = i * W.max_lm + l;
    const int R = W.up[id];
    const int a = R / W.max_lm, m = W.len[R], r = W.rank[R];
    const int s = a - 1, e = a + m - 1, cls = s * P + e;
    const int lam = W.lbase[cls] + r;
    const int eb = W.ebase[cls] + r * (m + 1);
    const int in_row = W.rp[cls] + r;  // + A[s][p2] - RP[s][p2]: the landmark's place in a list (., p2)
    W.lmk[id] = lam;
    const int64_t o = (W.s0 + i) * W.max_lm + l;
    const int k = eb + (i - s);
    ep[k] = i;
    el[k] = lam;
    meas[2 * k] = uvo[2 * o];
    meas[2 * k + 1] = uvo[2 * o + 1];
    le[k] = k;
    const int at = W.A[s * P + i] + in_row - W.rp[s * P + i];
    pe[pe_off[i] + at] = k;
    for (int p1 = s; p1 <= i; ++p1) {
        const int c = cv_off[p1 * P + i] + at;
        cv1[c] = eb + (p1 - s);
        cv2[c] = k;
    }
    if (id != R) return;
    X[3 * lam] = Xs[3 * o];
    X[3 * lam + 1] = Xs[3 * o + 1];
    X[3 * lam + 2] = Xs[3 * o + 2];
    le_off[lam] = eb;
    ep[eb] = s;
    el[eb] = lam;
    meas[2 * eb] = uvp[2 * o];
    meas[2 * eb + 1] = uvp[2 * o + 1];
    le[eb] = eb;
    const int at0 = W.A[s * P + s] + in_row - W.rp[s * P + s];
    pe[pe_off[s] + at0] = eb;
    const int c0 = cv_off[s * P + s] + at0;
    cv1[c0] = eb;
    cv2[c0] = eb;
}

// apply_window_tracks: T_wc = inverse(T_cw), every node its landmark's refined X, the anchor
__global__ __launch_bounds__(256) void wint_scatter_kernel(WinTracks W, const int32_t* __restrict__ cnt_f,
                                                           const double* __restrict__ poses, const double* __restrict__ X,
                                                           double* __restrict__ T, double* __restrict__ Xs,
                                                           double* __restrict__ anchor, const int* gate) {
    if (gate && *gate) return;  // enqueued with the solve: skipped when it was suspended (solve_end reruns it)
    const int i = blockIdx.y + 1, l = blockIdx.x * 256 + threadIdx.x;
    const int flat = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    if (flat < W.P) {
        double o[7];
        se3_inverse(poses + 7 * flat, o);
        for (int k = 0; k < 7; ++k) T[(W.s0 + flat) * 7 + k] = o[k];
        if (anchor && flat == W.P - 1)
            for (int k = 0; k < 7; ++k) anchor[k] = o[k];
    }
    if (l >= cnt_f[W.s0 + i]) return;
    const int lam = W.lmk[i * W.max_lm + l];
    const int64_t o = (W.s0 + i) * W.max_lm + l;
    Xs[3 * o] = X[3 * lam];
    Xs[3 * o + 1] = X[3 * lam + 1];
    Xs[3 * o + 2] = X[3 * lam + 2];
}

dim3 node_grid(const WinTracks& W) { return dim3((W.max_lm + 255) / 256, W.P - 1); }

}  // namespace

namespace yavo {

int win_tracks_add(const void* d_block, const int32_t* d_edge_query, const int32_t* d_match_dj, int64_t dj_stride,
                   int max_kp, int64_t carry_frame, int64_t g0, int64_t cap, int max_lm, int max_kf, int32_t* d_query,
                   int32_t* d_train, int32_t* d_tab, int32_t* d_parent, int64_t* d_roots, hipStream_t st) {
    const uint8_t* blk = static_cast<const uint8_t*>(d_block);
    hipLaunchKernelGGL(wint_record_kernel, dim3(max_kf), dim3(256), 0, st, blk, d_edge_query, d_match_dj, dj_stride,
                       max_kp, g0, cap, max_lm, d_query, d_train, d_tab);
    hipLaunchKernelGGL(wint_link_kernel, dim3(max_kf), dim3(256), 0, st, blk, carry_frame, g0, cap, max_lm, d_query,
                       d_tab, d_parent, d_roots);
    return hipGetLastError() == hipSuccess ? YV_OK : YV_ERR_HIP;
}

int win_tracks_build(const WinTracks& W, int L, int E, const int32_t* d_cnt, const int32_t* d_parent, const double* d_T,
                     const double* d_Xs, const double* d_uvo, const double* d_uvp, double* poses, double* X,
                     int32_t* ep, int32_t* el, double* meas, int32_t* le_off, int32_t* le, int32_t* pe_off, int32_t* pe,
                     int32_t* cv_off, int32_t* cv1, int32_t* cv2, hipStream_t st) {
    const dim3 g = node_grid(W);
    hipLaunchKernelGGL(wint_init_kernel, g, dim3(256), 0, st, W, d_cnt, d_parent, d_T, poses);
    // the deepest node of a P-pose window is P - 2 steps below its root (pose P - 1 under pose 1)
    int rounds = 1;
    while ((1 << rounds) < W.P - 2) ++rounds;
    for (int r = 0; r < rounds; ++r)
        hipLaunchKernelGGL(wint_jump_kernel, g, dim3(256), 0, st, W, d_cnt, r == rounds - 1 ? 1 : 0);
    hipLaunchKernelGGL(wint_rank_kernel, dim3(W.P - 1), dim3(64), 0, st, W, d_cnt);
    hipLaunchKernelGGL(wint_tables_kernel, dim3(1), dim3(256), 0, st, W, pe_off, cv_off);
    hipLaunchKernelGGL(wint_write_kernel, g, dim3(256), 0, st, W, L, E, d_cnt, d_Xs, d_uvo, d_uvp, X, ep, el, meas,
                       le_off, le, pe_off, pe, cv_off, cv1, cv2);
    return hipGetLastError() == hipSuccess ? YV_OK : YV_ERR_HIP;
}

int win_tracks_scatter(const WinTracks& W, const int32_t* d_cnt, const double* poses, const double* X, double* d_T,
                       double* d_Xs, double* d_anchor, const int* gate, hipStream_t st) {
    hipLaunchKernelGGL(wint_scatter_kernel, node_grid(W), dim3(256), 0, st, W, d_cnt, poses, X, d_T, d_Xs, d_anchor,
                       gate);
    return hipGetLastError() == hipSuccess ? YV_OK : YV_ERR_HIP;
}

}  // namespace yavo
