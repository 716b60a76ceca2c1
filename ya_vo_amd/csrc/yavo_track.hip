// yavo_track.hip -- gfx950 kernels of the track composition: a run's stereo and temporal matches into the PnP edges
// that the per-frame pose LM (yavo_pose.hip, launch_track_pose) solves.
//
//   track_build_kernel    match mode: temporal match -> stereo match -> triangulated point, one edge each
//   stereo_points_kernel  LK mode (trackLastFrame, src/LoopHandler.cc:298-454): frame k-1's stereo map points
//   lk_edges_kernel       LK mode: the points that calcOpticalFlowPyrLK followed into frame k, as edges
//
// They share stereo_leg (whether a left keypoint's stereo match counts, and its point), the camera preamble and the
// compaction.  Built with -ffp-contract=off: the triangulation (yavo_geom_dev.h) matches the oracle bit for bit.
#include <type_traits>

#include "yavo_internal.h"
#include "yavo_geom_dev.h"

namespace yavo {
namespace geom {

// K of track t, Ta = identity (the left camera is the world) and Tb = T_right, in LDS
struct StereoRig {
    double K[9], Ta[7], Tb[7];
};

__device__ __forceinline__ void load_rig(StereoRig& rig, const TrackSrc& src, int t) {
    const int tid = threadIdx.x;
    if (tid < 9) rig.K[tid] = src.K[9 * t + tid];
    if (tid < 7) {
        rig.Ta[tid] = tid == 3 ? 1.0 : 0.0;
        rig.Tb[tid] = src.T_right[tid];
    }
    __syncthreads();
}

// A stereo pair as the stereo leg reads it, formed once per workgroup: its row of the [pair][max_kp] arrays, its
// removeOutliers limit, its left and right keypoints
struct StereoPair {
    int64_t row;
    int lim;
    const yv_keypoint *kl, *kr;
};

__device__ __forceinline__ StereoPair stereo_pair(const TrackSrc& src, int sp) {
    return {(int64_t)sp * src.max_kp, src.match_lim[sp], src.keypoints + (int64_t)src.pairs[2 * sp] * src.max_kp,
            src.keypoints + (int64_t)src.pairs[2 * sp + 1] * src.max_kp};
}

// The stereo leg: whether left keypoint j's match in stereo pair p counts (kept by removeOutliers, with right-image
// keypoint r) and, if so, X = triangulate(kp_left[j], kp_right[r]) with the left camera as world (pose identity) and
// the right camera at T_right; true iff triangulation succeeds and Z > 0 (triangulate2View,
// src/LoopHandler.cc:658-726).
// KEEP (the match filter is on): the match counts only if keep[sp][j].
// SUBPIX (the stereo refinement is on): it triangulates from its refined right column (sub_dcol[sp][j], zero unless
// its status is OK) and, with drop_edge, does not count when its status is EDGE.
template <bool KEEP, bool SUBPIX>
__device__ __forceinline__ bool stereo_leg(const TrackSrc& src, const StereoPair& p, const StereoRig& rig, int j,
                                           double* X) {
    const int2 b = src.match_dj[p.row + j];
    bool ks = true;
    if constexpr (KEEP) ks = src.keep[p.row + j] != 0;
    int dq = 0;
    if constexpr (SUBPIX) {
        dq = src.sub_dcol[p.row + j];
        if (src.drop_edge && src.sub_status[p.row + j] == kSubpixEdge) ks = false;
    }
    if (!(b.x < p.lim && b.y >= 0 && ks)) return false;
    return triangulate_px<SUBPIX>(p.kl[j].x, p.kl[j].y, p.kr[b.y].x, p.kr[b.y].y, rig.Ta, rig.Tb, rig.K, X, dq);
}

// One pass of a compaction in lane order: a good lane's edge index is e = ne + (the good lanes before it); it writes
// its point X there and `rest(e)` the kernel's other outputs.  Returns the pass's number of good lanes.
template <int NT, class Rest>
__device__ __forceinline__ int compact_pass(bool good, int ne, const double* X, double* Xo, int* s_tmp, Rest rest) {
    int tot = 0;
    const int off = block_excl_scan_geom<NT>(good ? 1 : 0, s_tmp, &tot);
    if (good) {
        const int e = ne + off;
        Xo[3 * e] = X[0];
        Xo[3 * e + 1] = X[1];
        Xo[3 * e + 2] = X[2];
        rest(e);
    }
    return tot;
}

// Track edges of the batched frontend: track t = {stereo pair sp, temporal pair tp} with
// pairs[sp].query == pairs[tp].train (frame k's left image).  For temporal query i (frame k-1 keypoint)
// kept by removeOutliers with best train keypoint j of frame k, and j's stereo leg: X = its point,
// uv = (kp_{k-1}[i].x, kp_{k-1}[i].y) (the reference's measurement, src/LoopHandler.cc:786).  Edges keep temporal
// query order.  One workgroup per track.
// KEEP: a temporal match i counts only if keep[tp][i]; KEEP and SUBPIX in the stereo leg: see there.
template <int NT, bool KEEP, bool SUBPIX>
__global__ __launch_bounds__(NT) void track_build_kernel(const int32_t* __restrict__ tracks, const TrackSrc src,
                                                         const EdgeOut out) {
    __shared__ int s_tmp[40];
    __shared__ StereoRig rig;
    const int t = blockIdx.x, tid = threadIdx.x;
    const int sp = tracks[2 * t], tp = tracks[2 * t + 1];
    const int qt = src.pairs[2 * tp];  // frame k-1 left
    load_rig(rig, src, t);
    const int nq = src.kp_count[qt];
    const StereoPair stereo = stereo_pair(src, sp);
    const int lim_t = src.match_lim[tp];
    const int2* dj_t = src.match_dj + (int64_t)tp * src.max_kp;
    const yv_keypoint* kq = src.keypoints + (int64_t)qt * src.max_kp;
    double* Xo = out.X + 3 * (int64_t)t * src.max_kp;
    double* uvo = out.uv + 2 * (int64_t)t * src.max_kp;
    int32_t* qo = out.query + (int64_t)t * src.max_kp;
    int ne = 0;
    for (int base = 0; base < nq; base += NT) {
        const int i = base + tid;
        bool good = false;
        double X[3];
        if (i < nq) {
            const int2 a = dj_t[i];
            bool kt = true;
            if constexpr (KEEP) kt = src.keep[(int64_t)tp * src.max_kp + i] != 0;
            if (a.x < lim_t && a.y >= 0 && kt) good = stereo_leg<KEEP, SUBPIX>(src, stereo, rig, a.y, X);
        }
        ne += compact_pass<NT>(good, ne, X, Xo, s_tmp, [&](int e) {
            uvo[2 * e] = (double)kq[i].x;
            uvo[2 * e + 1] = (double)kq[i].y;
            qo[e] = i;
        });
    }
    if (tid == 0) out.count[t] = ne;
}

// LK tracking mode (the reference's trackLastFrame, src/LoopHandler.cc:298-454).  Map points of frame k-1: its
// left keypoints whose stereo leg (pair sp) holds.  Compacted in keypoint order: X, the LK start point (x = column,
// y = row as cv::Point2f, :344) and the keypoint index.  One workgroup per track.
template <int NT, bool KEEP, bool SUBPIX>
__global__ __launch_bounds__(NT) void stereo_points_kernel(const int32_t* __restrict__ stereo_pairs,
                                                           const TrackSrc src, const PointsOut out) {
    __shared__ int s_tmp[40];
    __shared__ StereoRig rig;
    const int t = blockIdx.x, tid = threadIdx.x;
    const int sp = stereo_pairs[t];
    load_rig(rig, src, t);
    const int nq = src.kp_count[src.pairs[2 * sp]];
    const StereoPair stereo = stereo_pair(src, sp);
    const yv_keypoint* kl = stereo.kl;
    double* Xo = out.X + 3 * (int64_t)t * src.max_kp;
    float* po = out.pts + 2 * (int64_t)t * src.max_kp;
    int32_t* qo = out.query + (int64_t)t * src.max_kp;
    int ne = 0;
    for (int base = 0; base < nq; base += NT) {
        const int j = base + tid;
        bool good = false;
        double X[3];
        if (j < nq) good = stereo_leg<KEEP, SUBPIX>(src, stereo, rig, j, X);
        ne += compact_pass<NT>(good, ne, X, Xo, s_tmp, [&](int e) {
            po[2 * e] = (float)kl[j].y;      // cv::Point2i(kp.y, kp.x) -> Point2f: x = column
            po[2 * e + 1] = (float)kl[j].x;  // y = row
            qo[e] = j;
        });
    }
    if (tid == 0) out.count[t] = ne;
}

// Pose edges from the LK result: points with status 1 become features at cv::Point2i(next.y, next.x), i.e. the
// float coordinates truncated toward zero (src/LoopHandler.cc:395), measurement (kp.x, kp.y) = (row, col).
__global__ __launch_bounds__(kNT) void lk_edges_kernel(const PointsOut pts, const float* __restrict__ next,
                                                       const uint8_t* __restrict__ status, int max_kp,
                                                       const EdgeOut out) {
    __shared__ int s_tmp[40];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int n = pts.count[t];
    const int64_t b = (int64_t)t * max_kp;
    int ne = 0;
    for (int base = 0; base < n; base += kNT) {
        const int i = base + tid;
        const bool good = i < n && status[b + i];
        ne += compact_pass<kNT>(good, ne, pts.X + 3 * (b + i), out.X + 3 * b, s_tmp, [&](int e) {
            out.uv[2 * (b + e)] = (double)(int)next[2 * (b + i) + 1];  // kp.x = (int) row
            out.uv[2 * (b + e) + 1] = (double)(int)next[2 * (b + i)];  // kp.y = (int) column
            out.query[b + e] = pts.query[b + i];
        });
    }
    if (tid == 0) out.count[t] = ne;
}

// f(KEEP, SUBPIX) as std::bool_constant values: the instantiation for what src carries
template <class F>
void with_variant(const TrackSrc& src, F f) {
    auto with_keep = [&](auto keep) { src.sub_dcol ? f(keep, std::true_type{}) : f(keep, std::false_type{}); };
    src.keep ? with_keep(std::true_type{}) : with_keep(std::false_type{});
}

}  // namespace geom

// The builders run 1024 threads: about one (query) keypoint per thread (the FP64 triangulations are latency-bound;
// 256 / 512 were measured)
void launch_track_build(const int32_t* tracks, int n_tracks, const TrackSrc& src, const EdgeOut& out, hipStream_t s) {
    if (n_tracks <= 0) return;
    geom::with_variant(src, [&](auto keep, auto sub) {
        hipLaunchKernelGGL((geom::track_build_kernel<1024, decltype(keep)::value, decltype(sub)::value>),
                           dim3(n_tracks), dim3(1024), 0, s, tracks, src, out);
    });
}

void launch_stereo_points(const int32_t* stereo_pairs, int n_tracks, const TrackSrc& src, const PointsOut& out,
                          hipStream_t s) {
    if (n_tracks <= 0) return;
    geom::with_variant(src, [&](auto keep, auto sub) {
        hipLaunchKernelGGL((geom::stereo_points_kernel<1024, decltype(keep)::value, decltype(sub)::value>),
                           dim3(n_tracks), dim3(1024), 0, s, stereo_pairs, src, out);
    });
}

void launch_lk_edges(int n_tracks, const PointsOut& pts, const float* next, const uint8_t* status, int max_kp,
                     const EdgeOut& out, hipStream_t s) {
    if (n_tracks <= 0) return;
    hipLaunchKernelGGL(geom::lk_edges_kernel, dim3(n_tracks), dim3(geom::kNT), 0, s, pts, next, status, max_kp, out);
}

}  // namespace yavo
