// yavo_internal.h -- the launch interface: the kernels' launchers, constants and kernel-argument structs, shared between
// the kernel translation units and the host side of the C ABI (yavo_host.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yavo/yavo_types.h"

struct yv_ctx;

namespace yavo {

// pow(t, 3) of g2o's LM step scaling (alpha = 1 - pow(2 rho - 1, 3)), correctly rounded: t^2 = p + e1 and p t = q + e2
// exactly (fma), t^3 = q + (e2 + e1 t) rounded once (oracle/yavo_oracle.h or_cube, the same operations).
__host__ __device__ inline double cube_cr(double t) {
    const double p = t * t, e1 = fma(t, t, -p);
    const double q = p * t, e2 = fma(p, t, -q);
    return q + (e2 + e1 * t);
}

constexpr int kMaxKp = 4096;     // per-image keypoint capacity supported by the top-K / scan kernels
constexpr int kMaxWidth = 2048;  // image width limit (BRIEF keeps 49 rows of the blurred image in LDS)
// BRIEF's row bands: 32 image rows per workgroup.  top-K buckets each image's kept keypoints by band
// (kp_band[image][max_kp] int4 {row, col, id, slot}, band b at [band_off[image][b], band_off[image][b + 1])), so a
// BRIEF workgroup reads its band's keypoints only; H <= kBandRows * kMaxBands.
constexpr int kBandRows = 32;
constexpr int kMaxBands = 256;
constexpr int kBandCounters = 1024;  // top-K's (band, bank class) counters: 32 classes up to 32 bands, else 1
constexpr int kFastTileW = 64;     // FAST / blur output tile: one wave per tile row
constexpr int kFastTileH = 56;
// The blurred image (detect's second output, BRIEF's input) is stored with a 128-B aligned row pitch, so the
// detect tiles write whole 64-B row segments with dword stores (a row stride of W = 1241 put every segment across
// two cache lines, stored byte by byte).  Columns [W, pitch) are padding no reader uses; pitch >= W + 1
// (brief_lds_stride(W) <= pitch: BRIEF stages whole 16-B words of a row).
__host__ __device__ constexpr int blur_pitch(int W) { return (W + 1 + 127) & ~127; }
// BRIEF's LDS band row stride: >= W + 1 (column W holds the next row's first pixel, see brief_kernel), 16-B rows
__host__ __device__ constexpr int brief_lds_stride(int W) { return (W + 1 + 15) & ~15; }
// brief_kernel's LDS region: the band (49 rows), the band's keypoint list, the next band's index / lo / count
__host__ __device__ constexpr size_t brief_lds_bytes(int W) {
    return (size_t)(kBandRows + 17) * brief_lds_stride(W) + sizeof(uint32_t) * kMaxKp + 16;
}
// brief_kernel is a grid of persistent workers that take (band, image) items from a queue with kBriefHeads heads, one
// per XCD label (blockIdx % 8): as many workers per CU as LDS regions fit the CU's 160 KiB (2 up to W = 1327)
constexpr int kBriefHeads = 8;
inline int brief_workers_per_cu(int W) { return brief_lds_bytes(W) <= 80 * 1024 ? 2 : 1; }
// Blurred images are laid out [image][H][blur_pitch(W)].
__host__ __device__ constexpr int64_t blur_image_bytes(int H, int W) { return (int64_t)H * blur_pitch(W); }
// XCD-aware block order (MI355X: 8 XCDs, each with its own L2; blocks are observed to round-robin over them by
// linear id): the bijective remap turns linear block b into a logical index so that every XCD runs one contiguous
// range of logical blocks -- neighbouring tiles (and their shared halo rows) stay in one L2.  Pure speed.
__device__ __forceinline__ int xcd_swizzle(int b, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7, xcd = b & 7, slot = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

struct Desc {                      // 256-bit BRIEF descriptor, test j -> bit j (LSB-first bytes)
    uint32_t w[8];
};
struct Mat3 {                      // a row-major 3 x 3 (a camera's K) as a kernel argument: recoverPose, the BA
    double v[9];
};

// ---- detect (yavo_detect.hip) ----
// FAST-12 candidate test + Harris response, appends (response, index) keys per image.  eig: the cv::eigen
// flavour (0 = JacobiImpl_, 1 = HAVE_EIGEN's SelfAdjointEigenSolver).
void launch_fast_harris(const uint8_t* imgs, int n_images, int H, int W, int stride, int64_t pitch,
                        int thr, int eig, uint64_t* cand_keys, int64_t cap, uint32_t* cand_count,
                        hipStream_t s);
// FAST + Harris + 9x9 blur (k9_host: 9 taps that sum to 256).  Taps <= 127: one fused kernel over the same LDS tile,
// the blur on the int8 matrix cores (the image is read once).  A tap above 127: launch_fast_harris, then launch_blur9
// on the same stream.
void launch_detect_blur(const uint8_t* imgs, int n_images, int H, int W, int stride, int64_t pitch, int thr,
                        int eig, uint64_t* cand_keys, int64_t cap, uint32_t* cand_count, const uint16_t* k9_host,
                        uint8_t* blur, hipStream_t s);
// 9-tap separable fixed-point Gaussian, BORDER_REFLECT_101; output [image][H][blur_pitch(W)].
void launch_blur9(const uint8_t* imgs, int n_images, int H, int W, int stride, int64_t pitch,
                  const uint16_t* k9_host, uint8_t* blur, hipStream_t s);
// The key detect writes, select filters and top-K reads.  Order-preserving: ascending key == (response descending,
// row-major index ascending).
__device__ __forceinline__ uint64_t make_key(float resp, uint32_t idx) {
    if (resp == 0.0f) resp = 0.0f;  // -0 and +0 compare equal in the reference's sort
    uint32_t u = __float_as_uint(resp);
    uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)(~ord) << 32) | (uint64_t)idx;
}
__device__ __forceinline__ float key_resp(uint64_t key) {
    uint32_t ord = ~(uint32_t)(key >> 32);
    uint32_t u = (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord;
    return __uint_as_float(u);
}

// ---- keypoint selection (yavo_select.hip) ----
// Keypoint selection (yv_set_keypoint_select, yavo_select.hip): the filter between the detect kernel and launch_topk.
// Suppression buckets the corners by tiles of kSelTileRows x kSelTileCols pixels, the quota by the caller's cells; both
// grids have at most kSelMaxCells cells (the tiles of every accepted H x W do, the cells are the caller's to check).
constexpr int kSelMaxCells = 8192;
constexpr int kSelTileRows = 32, kSelTileCols = 64;
constexpr int kSelMaxRadius = 8;
constexpr int kSelMaxPerCell = 4096;
constexpr int kSelMinCell = 8, kSelMaxCell = 8192;
// Filters cand_keys[img][0 .. cand_count[img]) in place (nms_radius > 0: suppression; per_cell > 0: the quota) and does
// launch_topk's bookkeeping for the detect kernel's list (cand_seen = corners before the filter, cand_count = 0).
// scratch: n_images lists of cap keys; starts: [n_images][kSelMaxCells + 1]; counts: [2][n_images].  Returns the array
// (inside counts) holding the filtered lists' lengths: launch_topk's cand_count, which resets it.
uint32_t* launch_select(uint64_t* cand_keys, int64_t cap, uint32_t* cand_count, uint32_t* cand_seen, int n_images,
                        int H, int W, int nms_radius, int cell_rows, int cell_cols, int per_cell, uint64_t* scratch,
                        int32_t* starts, uint32_t* counts, hipStream_t s);

// ---- top-K (yavo_topk.hip) ----
// Per-image top-K (response desc, index asc) + checkBoundry compaction.
// cand_count is copied to cand_seen and reset to 0 after it is read (ready for the next detection).
// brief_heads: the kBriefHeads queue heads of the launch_brief that follows on s, zeroed here (no launch of their own).
void launch_topk(const uint64_t* cand_keys, int64_t cap, uint32_t* cand_count, uint32_t* cand_seen, int n_images,
                 int H, int W, int max_kp, int keep, int32_t* det_rc, float* det_resp, int32_t* det_count,
                 int32_t* kp_src, int32_t* kp_count, int32_t* kp_band, int32_t* band_off, int32_t* brief_heads,
                 hipStream_t s);
// checkBoundry compaction of externally supplied points (det_rc / det_count already on the device).
void launch_kp_boundary(const int32_t* det_rc, const int32_t* det_count, int n_images, int H, int W,
                        int max_kp, int32_t* kp_src, int32_t* kp_count, int32_t* kp_band, int32_t* band_off,
                        int32_t* brief_heads, hipStream_t s);

// ---- BRIEF (yavo_brief.hip, yavo_steer.hip) ----
// BRIEF: writes KeyPoint records + packed descriptors.  loff: a 2 KB device scratch of the caller holding the tests'
// LDS offsets for this W, formed on stream s first when new_loff (the offsets table or W changed since it was formed).
// heads: the band queue's kBriefHeads heads, zero on entry (launch_topk / launch_kp_boundary on s); the grid is
// min(max_workers, bands x images) workers.
void launch_brief(const uint8_t* blur, int n_images, int H, int W, const int8_t* offsets,
                  const int32_t* kp_src, const int32_t* kp_band, const int32_t* band_off, int max_kp,
                  yv_keypoint* keypoints, Desc* desc, int32_t* loff, bool new_loff, int32_t* heads, int max_workers,
                  hipStream_t s);
// Pack KeyPoint records -> descriptors (host-supplied keypoints).
void launch_pack_desc(const yv_keypoint* keypoints, const int32_t* kp_count, int n_slots, int max_kp,
                      Desc* desc, hipStream_t s);
// Rotation-steered BRIEF (yv_set_brief_steering, yavo_steer.hip): launch_brief's replacement while steering is on.
// Every sample is the blurred image clamped to [0, H - 1] x [0, W - 1].  The kernel keeps a keypoint's patch in LDS as
// 2 kSteerMaxRadius + 1 rows of kSteerPatchStride bytes; the offsets table reaches it as one dword per test, the two
// samples' byte addresses in that patch (steer_pack_offsets: a1 | a2 << 16 of {drow1, dcol1, drow2, dcol2}).
constexpr int kSteerMaxBins = 64;
constexpr int kSteerMaxRadius = 15;   // of the moments' disc and of every offset component
constexpr int kSteerMaxDir = 256;     // |dirs| component bound: 2 * 577,320 * 256 < 2^31
constexpr int kSteerPatchStride = 40;
struct SteerTables {
    int n_bins, radius;
    const int16_t* dirs;    // [n_bins][2] = (dcol, drow), device
    const uint32_t* taddr;  // [n_bins][256], device
};
void steer_pack_offsets(const int8_t* offsets, int n_tests, uint32_t* out);  // host
// Records + packed descriptors of kp_src[image][0 .. kp_count[image]) in keypoint order, as launch_brief writes them,
// and per keypoint bin[image][max_kp] and moments[image][max_kp][2] = (m10, m01).  Reads no band list, no queue head.
void launch_brief_steer(const uint8_t* blur, int n_images, int H, int W, const SteerTables& t, const int32_t* kp_src,
                        const int32_t* kp_count, int max_kp, yv_keypoint* keypoints, Desc* desc, uint8_t* bin,
                        int32_t* moments, hipStream_t s);
// bin and moments alone of rc[0 .. min(*count, max_kp)) = {row, col}, any position of one H x W image
void launch_orient(const uint8_t* blur, int H, int W, const SteerTables& t, const int32_t* rc, const int32_t* count,
                   int max_kp, uint8_t* bin, int32_t* moments, hipStream_t s);

// ---- matchers (yavo_match.hip, yavo_match_gate.hip) ----
// The keypoint lists a matcher reads: slot i holds kp_count[i] points at desc / keypoints[i * max_kp].
struct MatchLists {
    const Desc* desc;
    const yv_keypoint* keypoints;
    const int32_t* kp_count;
    int max_kp;
};
// Brute-force Hamming NN: match_key[pair][q] = min over t of (dist << 16 | t).  max_train bounds every train
// list's length (<= 2048: the FP4 matcher, otherwise the int8 +-1 form).  match_key2 != nullptr: also every query's
// second-best key there (same format, 0xFFFFFFFF: no second train point), exact, first index on ties.
void launch_match(const MatchLists& lists, const int32_t* pairs, int n_pairs, int max_train, uint32_t* match_key,
                  uint32_t* match_key2, hipStream_t s);
// The gated matcher (yv_match_gated / yv_batch_set_match_gates, yavo_match_gate.hip).  Per slot, the keypoints
// bucketed by cell = (band of kGateBandRows rows, column >> col_shift): sorted[slot][max_kp] = {row | column << 16,
// keypoint index} cell by cell, band_start[slot][n_bands + 1] = first entry of every band.  n_bands * kGateBandRows
// covers every row, col_cells << col_shift every column, n_bands * col_cells <= kGateMaxCells; rows and columns are
// 16-bit.
constexpr int kGateBandRows = 32;
constexpr int kGateMaxCells = 8192;
constexpr int kGateMaxCoord = 65535;
void launch_gate_sort(const yv_keypoint* keypoints, const int32_t* kp_count, int n_slots, int max_kp, int n_bands,
                      int col_cells, int col_shift, uint2* sorted, int32_t* band_start, hipStream_t s);
// launch_match over the train points inside each pair's gate: gates[pair] = {drow_lo, drow_hi, dcol_lo, dcol_hi} on
// train minus query position; mirror: the gate of the swapped pair list.  Writes a key for every query of every pair,
// 0xFFFFFFFF where the gate holds no (second) train point.
void launch_match_gated(const MatchLists& lists, const int32_t* pairs, int n_pairs, int n_bands, const uint2* sorted,
                        const int32_t* band_start, const int32_t* gates, bool mirror, uint32_t* match_key,
                        uint32_t* match_key2, hipStream_t s);

// ---- match records (yavo_match_finalize.hip) ----
// The finalize's outputs per pair: all records and the kept ones ([pair][max_kp]) with their counts, every query's
// {distance, train index} and the removeOutliers limit.  match_pos != nullptr defers the two record lists: the finalize
// then writes every query's position in the filtered list there ([pair][max_kp], -1: dropped) and leaves the lists to
// launch_match_records.
struct MatchRecords {
    yv_match* matches;
    int32_t* match_count;
    yv_match* filtered;
    int32_t* filt_count;
    int2* match_dj;
    int32_t* match_lim;
    int32_t* match_pos;
};
// The 2-NN match filter (yv_batch_set_match_filter; the values of YV_MATCH_RATIO / YV_MATCH_MUTUAL).
constexpr int kMatchRatio = 1, kMatchMutual = 2;
// ROBUST (the 2-NN match filter): also consumes the second-best keys and the reverse direction's keys (rev_key[pair][j]
// = train point j's best query, from the matcher run on the swapped pair), and keeps a query iff
//   d1 < lim  &&  (no YV_MATCH_RATIO || d1 * den < d2 * num in int64)  &&  (no YV_MATCH_MUTUAL || i1(j1) == i).
// matches / match_dj / match_lim are written as without it; filtered / filt_count hold the kept records only; nn2 =
// {d1, j1, d2, j2}, rev = i1(j) (-1: not computed or no query), keep = one byte per query.
struct FinalizeRobust {
    uint32_t* match_key2;
    uint32_t* rev_key;
    int flags, num, den;
    int4* nn2;
    int32_t* rev;
    uint8_t* keep;
};
// Matches records (matchFeatures) + removeOutliers per pair.  match_key entries are reset to 0xFFFFFFFF after they are
// read (ready for the next match).  rb != nullptr: with the filter, which consumes (and resets) rb->match_key2 and
// rb->rev_key as well (untouched 0xFFFFFFFF entries read as "no query").  kp_count_copy: + kp_count[0, n_slots) -> copy.
void launch_match_finalize(uint32_t* match_key, const MatchLists& lists, const int32_t* pairs, int n_pairs, int thr,
                           const MatchRecords& out, const FinalizeRobust* rb, hipStream_t s,
                           int32_t* kp_count_copy = nullptr, int n_slots = 0);
// The record lists of a finalize that deferred them (out.match_pos set), byte for byte what the fused finalize writes:
// from out.match_dj / out.match_pos, the pairs and the keypoints; lists.kp_count may be a copy of that run's counts.
// At most max_workgroups one-wave workgroups walk the lists.
void launch_match_records(const MatchLists& lists, const int32_t* pairs, int n_pairs, const MatchRecords& out,
                          int max_workgroups, hipStream_t s);
// removeOutliers on externally supplied Matches records (one list).
void launch_filter_records(const yv_match* in, int n, int thr, yv_match* out, int32_t* out_count,
                           hipStream_t s);

// ---- stereo refinement (yavo_stereo_subpix.hip) ----
// Sub-pixel stereo refinement (yv_stereo_subpix / yv_batch_set_stereo_subpix, yavo_stereo_subpix.hip; the values of
// YV_SUBPIX_*).  Images are read inside [image, image + (H - 1) * stride + W) only.
constexpr int kSubpixNone = 0, kSubpixOk = 1, kSubpixOutside = 2, kSubpixEdge = 3;
constexpr int kSubpixMaxWin = 7, kSubpixMaxSearch = 8;
struct SubpixOut {
    int32_t* dcol_q8;
    int32_t* sad;
    uint8_t* status;
};
// every record of m[0, n): pt1 in `left`, pt2 in `right`
void launch_subpix_list(const uint8_t* left, const uint8_t* right, int H, int W, int stride, const yv_match* m, int n,
                        int half_win, int search, const SubpixOut& out, hipStream_t s);
// the kept matches of the pairs marked[0, n_marked) (indices into pairs) of a run on n_images images (image i at
// images + i * pitch): out[pair][query] for every query in [0, max_kp), kSubpixNone where nothing is attempted
void launch_subpix_batch(const uint8_t* images, int n_images, int H, int W, int stride, int64_t pitch,
                         const int32_t* marked, int n_marked, const int32_t* pairs, const yv_keypoint* keypoints,
                         const int32_t* kp_count, const int2* match_dj, const int32_t* match_lim,
                         const uint8_t* keep, int max_kp, int half_win, int search, const SubpixOut& out,
                         hipStream_t s);

// ---- geometry (yavo_geom.hip): F-RANSAC, triangulation, world2Camera ----
// device workspace of launch_f_ransac: [n_lists][iters] hypotheses' F and inlier counts
size_t f_ransac_ws_bytes(int n_lists, int iters);
void launch_f_ransac(const yv_match* matches, int64_t list_stride, const int32_t* counts, int n_lists,
                     const int32_t* samples, int64_t sample_stride, int iters, double thr, double* F_out,
                     int32_t* max_inliers, int32_t* found, void* ws, hipStream_t s);
// dcol_q8 (optional, [n]): record i's right column is pt2.y + dcol_q8[i] / 256 (yv_triangulate_subpix)
void launch_triangulate(const yv_match* m, int n, const double* poses2, const double* K, double* Xw, uint8_t* ok,
                        int32_t* n_ok, hipStream_t s, const int32_t* dcol_q8 = nullptr);
void launch_world2camera(const double* X, int n, const double* T, const double* K, double* out, hipStream_t s);

// ---- pose-only LM and GN (yavo_pose.hip) ----
void launch_pose_lm(const int32_t* offsets, int n_problems, const double* X, const double* uv, const double* K,
                    double* poses, uint8_t* outlier, int32_t* inliers, hipStream_t s);
void launch_pose_gn(const int32_t* offsets, int n_problems, const double* X, const double* uv, const double* K,
                    double* poses, int32_t* iters, hipStream_t s);
void launch_track_pose(int n_tracks, const int32_t* edge_count, int stride, const double* edge_X,
                       const double* edge_uv, const double* K, const double* priors, double* poses,
                       uint8_t* edge_outlier, int32_t* inliers, hipStream_t s);

// ---- P3P-RANSAC absolute pose (yavo_pnp.hip) ----
constexpr int kPnpMaxIters = 1024;  // hypotheses per problem (4 candidate poses each)
// device workspace of launch_pnp_ransac: [n_problems][iters] hypotheses' 4 poses, inlier counts and root masks
size_t pnp_ransac_ws_bytes(int n_problems, int iters);
// Problem p's edges as the pose LM addresses them: [offsets[p], offsets[p + 1]), or with counts (the track layout)
// counts[p] edges from p * stride; the first 4096.
// draws [iters][3] serves every problem.  init (optional [p][7]): poses[p] where nothing is found; nullptr leaves it.
void launch_pnp_ransac(const int32_t* offsets, const int32_t* counts, int stride, int n_problems,
                       const double* X, const double* uv, const double* K, const uint32_t* draws, int iters,
                       double thr, int min_inliers, const double* init, double* poses, uint8_t* inlier,
                       int32_t* inliers, int32_t* found, void* ws, hipStream_t s);

// ---- track composition (yavo_track.hip): a run's stereo and temporal matches into the pose LM's edges ----
// What the track kernels read: the run's pair list, keypoints ([slot][max_kp]) and match records ([pair][max_kp]), the
// tracks' K ([n_tracks][9]) and the right camera's pose T_right ([7]).  The rest is optional, [pair][max_kp]:
// keep (the match filter's): a match counts only if its query's byte is set;
// sub_dcol / sub_status (the stereo refinement's dcol_q8 and status, both or neither): a stereo match triangulates from
// its refined right column and, with drop_edge, does not count when its status is kSubpixEdge.
struct TrackSrc {
    const int32_t* pairs;
    const yv_keypoint* keypoints;
    const int32_t* kp_count;
    const int2* match_dj;
    const int32_t* match_lim;
    int max_kp;
    const double* K;
    const double* T_right;
    const uint8_t* keep;
    const int32_t* sub_dcol;
    const uint8_t* sub_status;
    bool drop_edge;
};
// What they write, track t at t * max_kp: the pose LM's edges ...
struct EdgeOut {
    double* X;       // [n_tracks][max_kp][3]
    double* uv;      // [n_tracks][max_kp][2]
    int32_t* query;  // [n_tracks][max_kp]
    int32_t* count;  // [n_tracks]
};
// ... and LK mode's map points (pts: cv::Point2f, x = column)
struct PointsOut {
    double* X;
    float* pts;
    int32_t* query;
    int32_t* count;
};
void launch_track_build(const int32_t* tracks, int n_tracks, const TrackSrc& src, const EdgeOut& out, hipStream_t s);
void launch_stereo_points(const int32_t* stereo_pairs, int n_tracks, const TrackSrc& src, const PointsOut& out,
                          hipStream_t s);
// edges of the points `pts` that LK tracked to `next` with `status` set (both [n_tracks][max_kp])
void launch_lk_edges(int n_tracks, const PointsOut& pts, const float* next, const uint8_t* status, int max_kp,
                     const EdgeOut& out, hipStream_t s);

// ---- Lucas-Kanade (yavo_lk.hip) ----
// cv::calcOpticalFlowPyrLK workspace view (yavo_lk.hip).  Level 0 is the caller's image; levels >= 1 live in
// `pyr` ([image][pyr_pitch], level l at off[l], row stride ps[l] = w[l] rounded up to 64 bytes: every pyrDown store
// is a whole aligned dword of full cache lines).  The tracker computes Scharr derivatives inside its windows; `der`
// is one level's (dx, dy) int16 image for yv_lk_level only (ds[l] pixels per row = w[l] rounded up to 16).
constexpr int kLkMaxLevels = 8;
struct LkParams {
    int levels = 0, win = 11, max_count = 30;
    double eps2 = 1e-4, min_eig = 1e-3;
    int h[kLkMaxLevels] = {}, w[kLkMaxLevels] = {};
    int ps[kLkMaxLevels] = {}, ds[kLkMaxLevels] = {};
    int64_t off[kLkMaxLevels] = {};
    const uint8_t* img0 = nullptr;
    int stride0 = 0;
    int64_t pitch0 = 0;
    uint8_t* pyr = nullptr;
    int64_t pyr_pitch = 0;
    int16_t* der = nullptr;
    int64_t der_pitch = 0;  // int16 elements of `der`
};
void launch_lk_pyramid(const LkParams& P, int n_images, hipStream_t s);
void launch_lk_derivs(const LkParams& P, int image, int level, int16_t* der, hipStream_t s);
void launch_lk_track(const LkParams& P, const int32_t* pairs, int n_pairs, const float* pts, const int32_t* counts,
                     int pts_stride, int max_pts, float* next_pts, uint8_t* status, float* err, hipStream_t s);

// ---- essential matrix (yavo_essential.hip) ----
// cv::findEssentialMat (RANSAC) + cv::recoverPose (yavo_essential.hip).  Workspace of a yv_essential.
// RANSAC iterations evaluated per round: 64, or 1024 (>= findEssentialMat's 1000) for workspaces of at most kEssWidePairs
// lists, where the chip is otherwise idle: a list that needs all its iterations (the LoopHandler's re-initialisation
// lists, one image translation apart, never reach the 0.999 confidence early) then takes one round instead of four
// dependent ones, and a list that converges early costs the same one round (the sequential selection ignores the
// iterations past niters, so the result is the same)
constexpr int kEssChunk = 64;
constexpr int kEssChunkWide = 1024;
constexpr int kEssWidePairs = 8;
inline int ess_chunk_for(int max_pairs) { return max_pairs <= kEssWidePairs ? kEssChunkWide : kEssChunk; }
struct EssParams {
    int max_pairs = 0, max_points = 0, max_iters = 0;
    int chunk = kEssChunk;     // iterations per round (ess_chunk_for)
    double* m1 = nullptr;      // [max_pairs][max_points][2] normalised points1
    double* m2 = nullptr;      // [max_pairs][max_points][2] normalised points2
    int32_t* idx = nullptr;    // [max_pairs][max_iters][5] getSubset draws
    double* models = nullptr;  // [max_pairs][chunk][10][9]
    int32_t* nmod = nullptr;   // [max_pairs][chunk]
    int32_t* good = nullptr;   // [max_pairs][chunk][10]
    int32_t* state = nullptr;  // [max_pairs][8]: niters, max_good, iterations run, models, found, n, -, -
    double* best = nullptr;    // [max_pairs][9]
    double* cand = nullptr;    // [max_pairs][4][12] recoverPose candidates P1..P4
    int32_t* cgood = nullptr;  // [max_pairs][4]
    // cv::RNG((uint64)-1)'s states after 1 .. rng_len draws (list-independent: every list's round 0 starts there), for
    // the parallel subset draws of wide rounds (ess_subsets_par_kernel); null for narrow rounds
    uint64_t* rng_tab = nullptr;
    int rng_len = 0;
};
struct EssRun {
    double focal, ppx, ppy, prob, threshold;
    int max_iters;
};
void launch_find_essential(const EssParams& P, const EssRun& r, const float* pts1, const float* pts2,
                           const int32_t* counts, int n_pairs, int pts_stride, double* E, uint8_t* mask,
                           int32_t* found, int32_t* stats, hipStream_t s);
// test entry point behind yv_debug_ess_models (below the kernels in yavo_essential.hip): the model kernel of the workspace's form on n_sets given
// five-point subsets q1 / q2 [n_sets][5][2]; models [n_sets][10][9] (zeros past a subset's count), nmod [n_sets]
int launch_debug_ess_models(const EssParams& P, const double* q1, const double* q2, int n_sets, double* models,
                            int32_t* nmod, hipStream_t s);
void launch_recover_pose(const EssParams& P, const double* E, const float* pts1, const float* pts2,
                         const int32_t* counts, int n_pairs, int pts_stride, const Mat3& K, double* R, double* t,
                         int32_t* good, hipStream_t s);

// ---- bundle adjustment (yavo_ba.hip, yavo_ba_ldlt.hip; the host side: yavo_ba_host.hip, yavo_ba_window.hip) ----
namespace ba {
// what the kernels and the host's buffer sizes share
constexpr int kNT = 256;             // lanes of a landmark-block workgroup (ba_step_kernel, ba_chi2_kernel)
constexpr int kTicketGroups = 64;    // counters of a large grid's last-workgroup ticket (ba_last_block_h)
constexpr int kWLeaves = 4096;       // leaves of a tree4096 sum (yavo_ba.hip wide_local_tree)
// 16 workgroups of 256 lanes per sum (32 x 128 until c49: the reduce kernel 19.4 -> 17.3 us, the Schur kernel the same;
// 8 x 512: Schur 33 us, profiles/r05/c49)
constexpr int kWG = 16;
constexpr int kWLanes = kWLeaves / kWG;  // 256
}  // namespace ba
// sliding-window BA: the device graph, workspace and estimate of a yv_ba
struct BaParams {
    int P = 0, nf = 0, np = 0, ns = 0, L = 0, E = 0;
    const int32_t* ep = nullptr;      // [E]
    const int32_t* el = nullptr;      // [E]
    const double* meas = nullptr;     // [E][2]
    const int32_t* pe_off = nullptr;  // [P + 1] edges per pose (edge order)
    const int32_t* pe = nullptr;      // [E]
    const int32_t* le_off = nullptr;  // [L + 1] edges per landmark (edge order)
    const int32_t* le = nullptr;      // [E]
    const int32_t* cv_off = nullptr;  // [P * P + 1] per pose pair (p1 <= p2): shared landmarks ascending
    const int32_t* cv_e1 = nullptr;   // the p1 edge of each
    const int32_t* cv_e2 = nullptr;   // the p2 edge of each
    double* poses = nullptr;          // [P][7]
    double* X = nullptr;              // [L][3]
    double* err = nullptr;            // [E][2]
    double* Jp = nullptr;             // [E][12]
    double* Jl = nullptr;             // [E][6]
    double* Hpp = nullptr;            // [P][36]
    double* bp = nullptr;             // [P][6]
    double* Hll = nullptr;            // [L][9]
    double* bl = nullptr;             // [L][3]
    double* S = nullptr;              // [ns][ns]
    double* bs = nullptr;             // [ns]
    double* xp = nullptr;             // [ns]
    double* xl = nullptr;             // [L][3]
    int32_t* tr = nullptr;            // [ns] LDLT transpositions
    double* scal = nullptr;           // [4]: chi2, scale, LDLT ok
    // device-driven LM (yv_ba_solve): a kernel returns at once when *gate != 0 (its phase is skipped), and the trial
    // kernels read lambda from *lam; both nullptr under host control
    const int* gate = nullptr;
    const double* lam = nullptr;
    // the trial state: ba_step_kernel writes the trial estimate into the other buffer (poses2 / X2 when *cur == 0),
    // an accepted trial flips *cur; ba_finish_kernel leaves the result in poses / X
    double* poses2 = nullptr;          // [P][7]
    double* X2 = nullptr;              // [L][3]
    int* cur = nullptr;
    struct BaCtl* ctl = nullptr;        // device control block (nullptr: host control)
    double* log = nullptr;             // [max_iters + 1] chi2 per iteration (device control)
    unsigned long long* maxdiag = nullptr;
    unsigned* ticket = nullptr;        // [kBaTickets] last-workgroup counters (0 between launches)
    double* part = nullptr;            // [1 + 2 blocks]: the free poses' scale part, then per block of 256
                                       // landmarks its chi2 and scale totals (ba_step_kernel)
    double* spart = nullptr;           // [Schur task][kWG][36] tree4096 class totals of the Schur workgroups
    unsigned* sticket = nullptr;       // [Schur task] last-workgroup counters (0 between launches)
    double* rpart = nullptr;           // [free pose][kWG][27] class totals of the H_pp / b_p reduce
    unsigned* rticket = nullptr;       // [free pose] last-workgroup counters
};
// The device-side Levenberg-Marquardt control of one solve (g2o OptimizationAlgorithmLevenberg::solve, the
// host loop's arithmetic): written by the last workgroups of ba_reduce_kernel / ba_chi2_kernel, read by the gates.
struct BaCtl {
    double currentChi, lambda, ni, rho;
    int q, it, stop, iters;
    int skip_iter, skip_trial, suspended, iter_done;
};
// linearise + the H / b blocks (first: the largest diagonal into *P.maxdiag; device control: the iteration begins)
void launch_ba_linearize(const BaParams& P, const Mat3& K, int first, hipStream_t s);
// one damping trial: Dinv / W, Schur, LDLT, step into the trial state, chi2 + scale (device control: the decision)
void launch_ba_trial(const BaParams& P, const Mat3& K, double lambda, hipStream_t s);
// the solve's first chi2 (device control: the control block's initialisation)
void launch_ba_chi2(const BaParams& P, const Mat3& K, hipStream_t s);
void launch_ba_finish(const BaParams& P, hipStream_t s);
void launch_ba_ctl_resume(BaCtl* c, hipStream_t s);
// Eigen's LDLT on the reduced pose system P.S x = P.bs into P.xp, P.scal[2] = isPositive (yavo_ba_ldlt.hip; part of
// launch_ba_trial, alone behind yv_ba_debug_ldlt)
void launch_ba_ldlt(const BaParams& P, hipStream_t s);

// ---- map (yavo_map.hip) ----
// the shared map (yavo_map.hip): one chunk's block after its pose LM
void launch_map_chunk(const double* rel, int n, int64_t first_frame, int kf_every, const int32_t* edge_count,
                      const double* edge_X, const uint8_t* edge_outlier, int max_kp, int max_kf, void* block,
                      hipStream_t s);

// ---- PNG (yavo_inflate.hip) ----
// PNG decoding on the GPU (yavo_inflate.hip): per-image status codes and the two kernels
enum : int32_t {
    kPngOk = 0, kPngErrHeader = 1, kPngErrBlock = 2, kPngErrCode = 3, kPngErrOverrun = 4, kPngErrShort = 5,
    kPngErrFilter = 6, kPngErrCrc = 7, kPngErrAdler = 8,
    kPngErrFile = 9  // missing, unreadable, truncated or not an 8-bit grey PNG of the decoder's size (host side)
};
// one IDAT payload of a PNG file staged on the device: len bytes from src to dst (byte offsets in the staging buffers);
// the chunk's type is the 4 bytes before src, its CRC the 4 after src + len; img = the payload's image in the call
struct PngPiece {
    int64_t src, dst;
    int32_t len, img;
};
// gather + chunk CRCs: crc_bad[img] = 1 when a payload's CRC-32 (type + data) differs from the stored one
void launch_png_gather(const uint8_t* src, uint8_t* dst, const PngPiece* pieces, int n, int32_t* crc_bad, hipStream_t s);
// inflate: reads and clears crc_bad; adler[i] = the zlib trailer of image i
void launch_png_inflate(const uint8_t* src, const int64_t* off, const int32_t* len, int n, uint8_t* out,
                        int64_t out_pitch, uint32_t out_len, int32_t* status, int32_t* crc_bad, uint32_t* adler,
                        hipStream_t s);
// unfilter + the Adler-32 of the inflated bytes against adler[i]; failed images are zero-filled and counted in
// *bad_total
void launch_png_unfilter(const uint8_t* raw, int64_t raw_pitch, int n, int H, int W, uint8_t* dst, int64_t dst_pitch,
                         int dst_stride, int32_t* status, const uint32_t* adler, uint32_t* bad_total, hipStream_t s);

// ---- context (yavo_api.hip) ----
// the context's device / stream for the host-side modules that do not see yv_ctx (yavo_io.hip); defined with the
// context, beside yv_create in yavo_api.hip
int ctx_device(struct ::yv_ctx* ctx);
hipStream_t ctx_stream(struct ::yv_ctx* ctx);

}  // namespace yavo
