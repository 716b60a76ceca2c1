// yavo_match_finalize.hip -- the matchers' keys into Matches records, and removeOutliers.
//
// Reference functions restated (the reference's file:line):
//   match_finalize      Matches records + removeOutliers        src/BriefDescriptor.cc:163-231
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yavo_internal.h"
#include "yavo_wave.h"

namespace yavo {

// ------------------------------------------------------------------------------------------------
// Matches records + removeOutliers (one 1024-thread workgroup per pair)
// ------------------------------------------------------------------------------------------------
constexpr int FZ_NT = 1024;
constexpr int REC_DW = 25;  // 100-B Matches record = 25 dwords

__device__ __forceinline__ int block_min_int(int v, int* s_tmp) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    const int wave = (int)threadIdx.x >> 6;
    if (lane_id() == 0) s_tmp[wave] = v;
    __syncthreads();
    int r = s_tmp[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = min(r, s_tmp[w]);
    __syncthreads();
    return r;
}

// removeOutliers limit: max(2*min_dist, thr) with the reference's int wrap-around.
__device__ __forceinline__ int outlier_limit(int min_d, int thr) {
    const int twice = (int)((uint32_t)min_d * 2u);
    return twice > thr ? twice : thr;
}

// The 100-B Matches record, dword by dword, for the fused finalize and the records kernel alike.  Dword f of the record
// of query i matched to train j (< 0: none) is the query keypoint's dword f (f < 12) or the train keypoint's dword
// record_train_dword(f), fixed by record_dword.  record_src is that dword's address, always valid (train 0 when j < 0).
__device__ __forceinline__ int record_train_dword(int f) { return min(f - 12, 2); }
__device__ __forceinline__ const uint32_t* record_src(const uint32_t* qrec, const uint32_t* trec, int i, int j, int f) {
    return f < 12 ? qrec + (int64_t)i * 12 + f : trec + (int64_t)max(j, 0) * 12 + record_train_dword(f);
}
__device__ __forceinline__ uint32_t record_dword(uint32_t x, int f, int j, int dist) {
    if (f == 11) x &= 0xFFu;                        // featVec[31]; the 3 pad bytes are always written as 0
    else if (f >= 12 && (f >= 15 || j < 0)) x = 0;  // pt2: x, y, id of the train keypoint only
    if (f == 24) x = (uint32_t)dist;
    return x;
}
// the same dword in the filtered list: matched = true on both copies
__device__ __forceinline__ uint32_t record_dword_kept(uint32_t x, int f) {
    return (f == 3 || f == 15) ? (x & ~0xFFu) | 1u : x;
}

// ROBUST: the 2-NN match filter over rb (FinalizeRobust, yavo_internal.h).  RECORDS: the two record lists as well;
// without them every query's position in the filtered list (-1: dropped) goes to match_pos for match_records_kernel.
template <bool ROBUST, bool RECORDS>
__global__ __launch_bounds__(FZ_NT) void match_finalize_kernel(
    uint32_t* __restrict__ match_key, const yv_keypoint* __restrict__ keypoints,
    const int32_t* __restrict__ kp_count, const int32_t* __restrict__ pairs, int max_kp, int thr,
    yv_match* __restrict__ matches, int32_t* __restrict__ match_count, yv_match* __restrict__ filtered,
    int32_t* __restrict__ filt_count, int2* __restrict__ match_dj, int32_t* __restrict__ match_lim,
    int32_t* __restrict__ match_pos, int32_t* __restrict__ kp_count_copy, int n_slots, FinalizeRobust rb) {
    __shared__ int s_dist[kMaxKp];
    // the edge build's copy of the run's keypoint counts (the last writer of kp_count, top-K, ran before this kernel)
    if (kp_count_copy && blockIdx.x == 0)
        for (int i = (int)threadIdx.x; i < n_slots; i += FZ_NT) kp_count_copy[i] = kp_count[i];
    __shared__ int s_j[kMaxKp];
    __shared__ int s_pos[kMaxKp];
    __shared__ int s_tmp[40];
    const int pair = blockIdx.x;
    const int tid = threadIdx.x;
    const int qi = pairs[2 * pair], ti = pairs[2 * pair + 1];
    const int nq = kp_count[qi];
    uint32_t* keys = match_key + (int64_t)pair * max_kp;
    int local_min = 0x7fffffff;
    for (int i = tid; i < nq; i += FZ_NT) {
        const uint32_t k = keys[i];
        keys[i] = 0xFFFFFFFFu;  // consumed: ready for the next match into this pair slot
        const int d = (k == 0xFFFFFFFFu) ? 0x7fffffff : (int)(k >> 16);
        s_dist[i] = d;
        s_j[i] = (k == 0xFFFFFFFFu) ? -1 : (int)(k & 0xFFFFu);
        local_min = min(local_min, d);
        if constexpr (ROBUST) {
            uint32_t* keys2 = rb.match_key2 + (int64_t)pair * max_kp;
            const uint32_t k2 = keys2[i];
            keys2[i] = 0xFFFFFFFFu;
            const int j1 = s_j[i];
            const int d2 = (k2 == 0xFFFFFFFFu) ? 0x7fffffff : (int)(k2 >> 16);
            const int j2 = (k2 == 0xFFFFFFFFu) ? -1 : (int)(k2 & 0xFFFFu);
            rb.nn2[(int64_t)pair * max_kp + i] = make_int4(d, j1, d2, j2);
            bool ok = true;
            if (rb.flags & kMatchRatio) ok = (int64_t)d * rb.den < (int64_t)d2 * rb.num;
            if (rb.flags & kMatchMutual) {
                // the reverse keys are reset only after the barrier of the block minimum below
                const uint32_t rk = j1 >= 0 ? rb.rev_key[(int64_t)pair * max_kp + j1] : 0xFFFFFFFFu;
                ok = ok && rk != 0xFFFFFFFFu && (int)(rk & 0xFFFFu) == i;
            }
            s_pos[i] = ok ? 1 : 0;
        }
    }
    const int min_d = block_min_int(local_min, s_tmp);
    const int lim = outlier_limit(min_d, thr);
    if constexpr (ROBUST) {
        const int nt = kp_count[ti];
        uint32_t* rkeys = rb.rev_key + (int64_t)pair * max_kp;
        for (int j = tid; j < nt; j += FZ_NT) {
            const uint32_t rk = rkeys[j];
            rkeys[j] = 0xFFFFFFFFu;
            rb.rev[(int64_t)pair * max_kp + j] = (rk == 0xFFFFFFFFu) ? -1 : (int)(rk & 0xFFFFu);
        }
    }
    int flags[4], cnt = 0;
    int2* dj = match_dj + (int64_t)pair * max_kp;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid * 4 + u;
        flags[u] = (i < nq && s_dist[i] < lim) ? 1 : 0;
        if constexpr (ROBUST) {
            if (i < nq) {
                flags[u] &= s_pos[i];  // ratio / mutual, written before the block minimum's barrier
                rb.keep[(int64_t)pair * max_kp + i] = (uint8_t)flags[u];
            }
        }
        cnt += flags[u];
        if (i < nq) dj[i] = make_int2(s_dist[i], s_j[i]);
    }
    int total = 0;
    int off = block_excl_scan<FZ_NT>(cnt, s_tmp, &total);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid * 4 + u;
        if constexpr (RECORDS) {
            if (i < nq) s_pos[i] = flags[u] ? off : -1;
        } else {
            if (i < nq) match_pos[(int64_t)pair * max_kp + i] = flags[u] ? off : -1;
        }
        off += flags[u];
    }
    if constexpr (RECORDS) {
        __syncthreads();
        const uint32_t* qrec = reinterpret_cast<const uint32_t*>(keypoints + (int64_t)qi * max_kp);
        const uint32_t* trec = reinterpret_cast<const uint32_t*>(keypoints + (int64_t)ti * max_kp);
        uint32_t* out_all = reinterpret_cast<uint32_t*>(matches + (int64_t)pair * max_kp);
        uint32_t* out_f = reinterpret_cast<uint32_t*>(filtered + (int64_t)pair * max_kp);
        const int ndw = nq * REC_DW;
        // Branch-free record assembly: every lane issues one load per record dword from an address that is always
        // valid (record_src; the value is then selected), FZ_U dwords per thread with every load in flight before the
        // stores.  A wave's 64 consecutive dwords span ~2.5 records, so per-field branches ran all three paths with a
        // load wait in each (0.83 -> 0.67 ms per 2048-frame step, profiles/r03/c54).
        constexpr int FZ_U = 4;
        for (int dw0 = tid; dw0 < ndw; dw0 += FZ_U * FZ_NT) {
            uint32_t v[FZ_U];
            int ii[FZ_U], ff[FZ_U];
#pragma unroll
            for (int u = 0; u < FZ_U; ++u) {
                const int dw = min(dw0 + u * FZ_NT, ndw - 1);
                const int i = dw / REC_DW, f = dw - i * REC_DW;
                v[u] = *record_src(qrec, trec, i, s_j[i], f);
                ii[u] = i;
                ff[u] = f;
            }
#pragma unroll
            for (int u = 0; u < FZ_U; ++u) {
                const int dw = dw0 + u * FZ_NT;
                if (dw >= ndw) break;
                const int i = ii[u], f = ff[u];
                const uint32_t x = record_dword(v[u], f, s_j[i], s_dist[i]);
                out_all[dw] = x;
                const int p = s_pos[i];
                if (p >= 0) out_f[(int64_t)p * REC_DW + f] = record_dword_kept(x, f);
            }
        }
    }
    if (tid == 0) {
        match_count[pair] = nq;
        filt_count[pair] = total;
        match_lim[pair] = lim;
    }
}

// The record loop of match_finalize_kernel as a kernel of its own, for a finalize that ran without RECORDS: the query's
// {distance, train index} and filtered position come from match_dj / match_pos.  Slots >= nq stay untouched, as in the
// fused kernel.  It runs beside the next run's detect, which is bound by VALU issue and stretches by about what this
// kernel issues, so it works record by record: a wave takes MR_NT consecutive queries of a pair, every lane loads its
// query keypoint (three 16-B loads) and three dwords of its train keypoint and lays the record out in the wave's LDS
// image, which the wave then stores as it lies in memory (16-B stores where the destination is aligned).  The kept
// records of the group are consecutive in the filtered list (match_pos is a running count), so they go the same way.
// One wave per workgroup: the image is the wave's own.  A fixed grid walks the (pair, group) space.  The lists are
// stored non-temporally: nothing in the step reads them, and 1.6 GB of them per 2048-frame step otherwise pass through
// the L2 that detect's tiles share their halo rows in (detect beside it 3.60 -> 3.45 ms, profiles/r18).
constexpr int MR_NT = 64;
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(MR_NT) void match_records_kernel(
    const int2* __restrict__ match_dj, const int32_t* __restrict__ match_pos,
    const yv_keypoint* __restrict__ keypoints, const int32_t* __restrict__ kp_count,
    const int32_t* __restrict__ pairs, int n_pairs, int max_kp, yv_match* __restrict__ matches,
    yv_match* __restrict__ filtered) {
    static_assert(sizeof(yv_keypoint) == 48 && sizeof(yv_match) == 4 * REC_DW, "record layout");
    __shared__ __attribute__((aligned(16))) uint32_t s_rec[MR_NT * REC_DW];
    const int lane = threadIdx.x;
    const int groups = (max_kp + MR_NT - 1) / MR_NT;  // per pair
    for (int c = blockIdx.x; c < n_pairs * groups; c += gridDim.x) {
        const int pair = c / groups, i0 = (c - pair * groups) * MR_NT;
        const int qi = pairs[2 * pair], ti = pairs[2 * pair + 1];
        const int nq = min(kp_count[qi], max_kp);
        if (i0 >= nq) continue;
        const int n = min(MR_NT, nq - i0);     // records of this group
        const int i = min(i0 + lane, nq - 1);  // (idle lanes: a valid query, nothing of theirs is stored)
        const int2 d = match_dj[(int64_t)pair * max_kp + i];
        const int p = lane < n ? match_pos[(int64_t)pair * max_kp + i] : -1;
        uint32_t q[12], t[3];
        const uint4* q4 = reinterpret_cast<const uint4*>(keypoints + (int64_t)qi * max_kp + i);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint4 w = q4[k];
            q[4 * k] = w.x, q[4 * k + 1] = w.y, q[4 * k + 2] = w.z, q[4 * k + 3] = w.w;
        }
        const uint32_t* tr = reinterpret_cast<const uint32_t*>(keypoints + (int64_t)ti * max_kp + max(d.y, 0));
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = tr[k];
#pragma unroll
        for (int f = 0; f < REC_DW; ++f)
            s_rec[lane * REC_DW + f] = record_dword(f < 12 ? q[f] : t[record_train_dword(f)], f, d.y, d.x);
        __syncthreads();
        uint32_t* out_all = reinterpret_cast<uint32_t*>(matches + (int64_t)pair * max_kp + i0);
        const int ndw = n * REC_DW;
        if ((reinterpret_cast<uintptr_t>(out_all) & 15) == 0) {
            for (int k = lane; 4 * k < ndw; k += MR_NT) {
                if (4 * k + 4 <= ndw) {
                    const uint4 w = reinterpret_cast<const uint4*>(s_rec)[k];
                    __builtin_nontemporal_store(v4u{w.x, w.y, w.z, w.w}, reinterpret_cast<v4u*>(out_all) + k);
                } else {  // the last, partial quad
                    for (int e = 4 * k; e < ndw; ++e) out_all[e] = s_rec[e];
                }
            }
        } else {  // max_kp * 100 no multiple of 16
            for (int k = lane; k < ndw; k += MR_NT) __builtin_nontemporal_store(s_rec[k], out_all + k);
        }
        __syncthreads();
        const uint64_t kept = __ballot(p >= 0);  // wave-uniform
        if (kept != 0) {
            const int p0 = __shfl(p, __ffsll((unsigned long long)kept) - 1);
            if (p >= 0) {
#pragma unroll
                for (int f = 0; f < REC_DW; ++f)
                    s_rec[(p - p0) * REC_DW + f] = record_dword_kept(
                        record_dword(f < 12 ? q[f] : t[record_train_dword(f)], f, d.y, d.x), f);
            }
            __syncthreads();
            uint32_t* out_f = reinterpret_cast<uint32_t*>(filtered + (int64_t)pair * max_kp + p0);
            const int nf = __popcll(kept) * REC_DW;
            for (int k = lane; k < nf; k += MR_NT) __builtin_nontemporal_store(s_rec[k], out_f + k);
            __syncthreads();
        }
    }
}

void launch_match_finalize(uint32_t* match_key, const MatchLists& lists, const int32_t* pairs, int n_pairs, int thr,
                           const MatchRecords& out, const FinalizeRobust* rb, hipStream_t s, int32_t* kp_count_copy,
                           int n_slots) {
    const bool rec = out.match_pos == nullptr;
    const auto kernel = !rb ? (rec ? match_finalize_kernel<false, true> : match_finalize_kernel<false, false>)
                            : (rec ? match_finalize_kernel<true, true> : match_finalize_kernel<true, false>);
    hipLaunchKernelGGL(kernel, dim3(n_pairs), dim3(FZ_NT), 0, s, match_key, lists.keypoints, lists.kp_count, pairs,
                       lists.max_kp, thr, out.matches, out.match_count, out.filtered, out.filt_count, out.match_dj,
                       out.match_lim, out.match_pos, kp_count_copy, n_slots, rb ? *rb : FinalizeRobust{});
}

void launch_match_records(const MatchLists& lists, const int32_t* pairs, int n_pairs, const MatchRecords& out,
                          int max_workgroups, hipStream_t s) {
    const int64_t groups = (int64_t)n_pairs * ((lists.max_kp + MR_NT - 1) / MR_NT);
    const int grid = (int)std::min<int64_t>(groups, std::max(max_workgroups, 1));
    hipLaunchKernelGGL(match_records_kernel, dim3(grid), dim3(MR_NT), 0, s, out.match_dj, out.match_pos,
                       lists.keypoints, lists.kp_count, pairs, n_pairs, lists.max_kp, out.matches, out.filtered);
}

// removeOutliers over a caller-supplied Matches list (n <= kMaxKp), one workgroup.
__global__ __launch_bounds__(FZ_NT) void filter_records_kernel(const yv_match* __restrict__ in, int n, int thr,
                                                               yv_match* __restrict__ out,
                                                               int32_t* __restrict__ out_count) {
    __shared__ int s_pos[kMaxKp];
    __shared__ int s_tmp[40];
    const int tid = threadIdx.x;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(in);
    int local_min = 0x7fffffff;
    for (int i = tid; i < n; i += FZ_NT) local_min = min(local_min, (int)src[(int64_t)i * REC_DW + 24]);
    const int min_d = block_min_int(local_min, s_tmp);
    const int lim = outlier_limit(min_d, thr);
    int flags[4], cnt = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid * 4 + u;
        flags[u] = (i < n && (int)src[(int64_t)i * REC_DW + 24] < lim) ? 1 : 0;
        cnt += flags[u];
    }
    int total = 0;
    int off = block_excl_scan<FZ_NT>(cnt, s_tmp, &total);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid * 4 + u;
        if (i < n) s_pos[i] = flags[u] ? off : -1;
        off += flags[u];
    }
    __syncthreads();
    uint32_t* dst = reinterpret_cast<uint32_t*>(out);
    for (int dw = tid; dw < n * REC_DW; dw += FZ_NT) {
        const int i = dw / REC_DW;
        const int f = dw - i * REC_DW;
        const int p = s_pos[i];
        if (p < 0) continue;
        uint32_t v = src[dw];
        if (f == 3 || f == 15) v = (v & ~0xFFu) | 1u;
        dst[(int64_t)p * REC_DW + f] = v;
    }
    if (tid == 0) *out_count = total;
}

void launch_filter_records(const yv_match* in, int n, int thr, yv_match* out, int32_t* out_count, hipStream_t s) {
    hipLaunchKernelGGL(filter_records_kernel, dim3(1), dim3(FZ_NT), 0, s, in, n, thr, out, out_count);
}

}  // namespace yavo
