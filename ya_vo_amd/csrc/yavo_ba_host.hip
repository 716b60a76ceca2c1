// yavo_ba_host.hip -- the host side of the bundle adjustment: the yv_ba C ABI (include/yavo/yavo_geom.h) over the
// kernels of yavo_ba.hip and yavo_ba_ldlt.hip -- the workspace, the problem's graph (edges per pose / landmark, the
// co-visibility lists), and g2o's Levenberg-Marquardt loop in its two forms: the control on the device (default;
// ba_solve_enqueue / ba_solve_wait, which the sliding window of yavo_ba_window.hip calls as well) or on the host
// (yv_ba_set_control(b, 0)).  struct yv_ba is in yavo_host.h.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/yavo/yavo.h"
#include "../../include/yavo/yavo_geom.h"
#include "yavo_host.h"
#include "yavo_internal.h"

using yavo::ba_ensure_schur;
using yavo::ba_solve_enqueue;
using yavo::ba_solve_wait;
using yavo::kBaMaxPoses;

namespace {

// [0] reduce, [1] chi2 (the last-workgroup tops); [4, 68) the reduce's groups, [68, 132) chi2's
constexpr int kBaTickets = 4 + 2 * yavo::ba::kTicketGroups;

}  // namespace

// the tree4096 class totals and per-sum counters of np free poses: P.spart / P.sticket for the Schur tasks (nb upper
// blocks + np b_schur rows), P.rpart / P.rticket for the pose reduce; grown on demand
int yavo::ba_ensure_schur(yv_ba* b, int np, hipStream_t st) {
    const int64_t tasks = (int64_t)np * (np + 1) / 2 + np;
    if (tasks <= b->schur_cap) return YV_OK;
    if (hipStreamSynchronize(st) != hipSuccess) return YV_ERR_HIP;
    yavo::BaParams& Q = b->P;
    b->mem.release(Q.spart, Q.sticket, Q.rpart, Q.rticket);
    b->schur_cap = 0;
    if (b->mem.alloc(&Q.spart, (size_t)tasks * yavo::ba::kWG * 36) != YV_OK ||
        b->mem.alloc(&Q.sticket, (size_t)tasks) != YV_OK ||
        b->mem.alloc(&Q.rpart, (size_t)np * yavo::ba::kWG * 27) != YV_OK ||
        b->mem.alloc(&Q.rticket, (size_t)np) != YV_OK ||
        hipMemsetAsync(Q.sticket, 0, sizeof(unsigned) * tasks, st) != hipSuccess ||
        hipMemsetAsync(Q.rticket, 0, sizeof(unsigned) * (np > 0 ? np : 1), st) != hipSuccess)
        return YV_ERR_HIP;
    b->schur_cap = tasks;
    return YV_OK;
}

namespace {

// the last-workgroup counters return to 0 at the end of every launch that uses them; a launch that never finished
// (an error, a fault) could leave one non-zero, and every later solve would then skip that launch's last-workgroup
// work silently -- so a new problem, and every failed enqueue, starts from zeroed counters (a few hundred bytes)
int ba_reset_tickets(yv_ba* b, hipStream_t st) {
    const yavo::BaParams& Q = b->P;
    if (hipMemsetAsync(b->d_ticket, 0, kBaTickets * sizeof(unsigned), st) != hipSuccess) return YV_ERR_HIP;
    if (b->schur_cap > 0 && (hipMemsetAsync(Q.sticket, 0, sizeof(unsigned) * b->schur_cap, st) != hipSuccess ||
                             hipMemsetAsync(Q.rticket, 0, sizeof(unsigned) * std::max(1, Q.np), st) != hipSuccess))
        return YV_ERR_HIP;
    return YV_OK;
}

int ba_sync_scal(yv_ba* b, int n) {
    if (hipMemcpyAsync(b->h_scal, b->P.scal, sizeof(double) * n, hipMemcpyDeviceToHost, b->st) != hipSuccess ||
        hipStreamSynchronize(b->st) != hipSuccess)
        return YV_ERR_HIP;
    return YV_OK;
}

}  // namespace

extern "C" int yv_ba_create(yv_ctx* ctx, int max_poses, int max_landmarks, int max_edges, yv_ba** out) {
    if (!out) return YV_ERR_INVALID;
    *out = nullptr;
    // the reduced pose system (6 max_poses)^2 doubles is factorised by one workgroup with its vectors in LDS
    if (!ctx || max_poses < 1 || max_poses > kBaMaxPoses || max_landmarks < 0 || max_edges < 0) return YV_ERR_INVALID;
    yv_ba* b = new yv_ba();
    b->ctx = ctx;
    b->dev = yavo::ctx_device(ctx);
    b->st = yavo::ctx_stream(ctx);
    b->ctx_st = b->st;
    b->max_poses = max_poses;
    b->max_landmarks = max_landmarks;
    b->max_edges = max_edges;
    if (hipSetDevice(b->dev) != hipSuccess) {
        delete b;
        return YV_ERR_HIP;
    }
    const size_t P = max_poses, L = max_landmarks, E = max_edges, ns = 6 * P;
    yavo::BaParams& Q = b->P;
    int rc = YV_OK;
    rc |= b->mem.alloc(&b->d_ep, E);
    rc |= b->mem.alloc(&b->d_el, E);
    rc |= b->mem.alloc(&b->d_meas, 2 * E);
    rc |= b->mem.alloc(&b->d_pe_off, P + 1);
    rc |= b->mem.alloc(&b->d_pe, E);
    rc |= b->mem.alloc(&b->d_le_off, L + 1);
    rc |= b->mem.alloc(&b->d_le, E);
    rc |= b->mem.alloc(&b->d_cv_off, P * P + 1);
    rc |= b->mem.alloc(&Q.poses, 7 * P);
    rc |= b->mem.alloc(&Q.X, 3 * L);
    rc |= b->mem.alloc(&Q.poses2, 7 * P);
    rc |= b->mem.alloc(&Q.X2, 3 * L);
    rc |= b->mem.alloc(&b->d_cur, 1);
    rc |= b->mem.alloc(&b->d_ticket, kBaTickets);
    rc |= b->mem.alloc(&Q.part, 1 + 2 * std::max<size_t>(1, (L + yavo::ba::kNT - 1) / yavo::ba::kNT));
    rc |= b->mem.alloc(&Q.err, 2 * E);
    rc |= b->mem.alloc(&Q.Jp, 12 * E);
    rc |= b->mem.alloc(&Q.Jl, 6 * E);
    rc |= b->mem.alloc(&Q.Hpp, 36 * P);
    rc |= b->mem.alloc(&Q.bp, 6 * P);
    rc |= b->mem.alloc(&Q.Hll, 9 * L);
    rc |= b->mem.alloc(&Q.bl, 3 * L);
    rc |= b->mem.alloc(&Q.S, ns * ns);
    rc |= b->mem.alloc(&Q.bs, ns);
    rc |= b->mem.alloc(&Q.xp, ns);
    rc |= b->mem.alloc(&Q.xl, 3 * L);
    rc |= b->mem.alloc(&Q.tr, ns);
    rc |= b->mem.alloc(&Q.scal, 16);
    rc |= b->mem.alloc(&b->d_maxdiag, 1);
    rc |= b->mem.alloc(&b->d_ctl, 1);
    if (rc == YV_OK) rc = b->mem.alloc_host(&b->h_scal, 4);
    if (rc == YV_OK) rc = b->mem.alloc_host(&b->h_ctl, 1);
    if (rc == YV_OK) rc = b->mem.alloc_host(&b->h_log, 65);
    // sized up front where that is small, so a solve loop's first iterations do not allocate (each growth
    // synchronises the stream and frees device memory, which synchronises the device): the Schur partials of up to 64
    // free poses, the window graph's co-visibility lists (3 per landmark) and a 64-iteration chi2 log
    if (rc == YV_OK && max_poses <= 64) rc |= ba_ensure_schur(b, max_poses, b->st);
    if (rc == YV_OK && max_landmarks > 0) {
        rc |= b->mem.alloc(&b->d_cv_e1, 3 * L);
        rc |= b->mem.alloc(&b->d_cv_e2, 3 * L);
        if (rc == YV_OK) b->cv_cap = 3 * (int64_t)L;
    }
    if (rc == YV_OK) {
        rc |= b->mem.alloc(&b->d_log, 65);
        if (rc == YV_OK) b->log_cap = 65;
    }
    if (rc == YV_OK && (hipMemsetAsync(b->d_ticket, 0, kBaTickets * sizeof(unsigned), b->st) != hipSuccess ||
                        hipMemsetAsync(b->d_cur, 0, sizeof(int), b->st) != hipSuccess ||
                        hipStreamSynchronize(b->st) != hipSuccess))
        rc = YV_ERR_HIP;
    if (rc != YV_OK) {
        yv_ba_destroy(b);
        return YV_ERR_HIP;
    }
    Q.cur = b->d_cur;
    Q.ticket = b->d_ticket;
    Q.maxdiag = b->d_maxdiag;
    *out = b;
    return YV_OK;
}

extern "C" void yv_ba_destroy(yv_ba* b) {
    if (!b) return;
    (void)hipSetDevice(b->dev);
    (void)hipStreamSynchronize(b->st);
    delete b;
}

extern "C" int yv_ba_set_stream(yv_ba* b, void* stream) {
    if (!b) return YV_ERR_INVALID;
    if (hipSetDevice(b->dev) != hipSuccess || hipStreamSynchronize(b->st) != hipSuccess) return YV_ERR_HIP;
    b->st = stream ? reinterpret_cast<hipStream_t>(stream) : b->ctx_st;
    return YV_OK;
}

extern "C" int yv_ba_set_problem(yv_ba* b, int n_poses, int n_fixed, int n_landmarks, const int32_t* edge_pose,
                                 const int32_t* edge_landmark, const double* meas, int n_edges, const double K[9]) {
    if (!b || !K || n_poses < 1 || n_poses > b->max_poses || n_fixed < 0 || n_fixed > n_poses || n_landmarks < 0 ||
        n_landmarks > b->max_landmarks || n_edges < 0 || n_edges > b->max_edges ||
        (n_edges > 0 && (!edge_pose || !edge_landmark || !meas)))
        return YV_ERR_INVALID;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return YV_ERR_INVALID;
    for (int e = 0; e < n_edges; ++e)
        if (edge_pose[e] < 0 || edge_pose[e] >= n_poses || edge_landmark[e] < 0 || edge_landmark[e] >= n_landmarks)
            return YV_ERR_INVALID;
    if (hipSetDevice(b->dev) != hipSuccess) return YV_ERR_HIP;
    b->ready = false;
    const int P = n_poses, L = n_landmarks, E = n_edges;
    // edges per pose / per landmark in edge order; co-visibility per pose pair (p1 <= p2), landmarks ascending
    std::vector<int32_t> pe_off(P + 1, 0), le_off(L + 1, 0), pe(std::max(E, 1)), le(std::max(E, 1));
    for (int e = 0; e < E; ++e) {
        pe_off[edge_pose[e] + 1]++;
        le_off[edge_landmark[e] + 1]++;
    }
    for (int p = 0; p < P; ++p) pe_off[p + 1] += pe_off[p];
    for (int l = 0; l < L; ++l) le_off[l + 1] += le_off[l];
    {
        std::vector<int32_t> fp(pe_off.begin(), pe_off.end() - 1), fl(le_off.begin(), le_off.end() - 1);
        for (int e = 0; e < E; ++e) {
            pe[fp[edge_pose[e]]++] = e;
            le[fl[edge_landmark[e]]++] = e;
        }
    }
    const int64_t NB = (int64_t)P * P;
    std::vector<int32_t> cv_off(NB + 1, 0);
    for (int l = 0; l < L; ++l)
        for (int a = le_off[l]; a < le_off[l + 1]; ++a)
            for (int c = le_off[l]; c < le_off[l + 1]; ++c) {
                const int p1 = edge_pose[le[a]], p2 = edge_pose[le[c]];
                if (p1 <= p2) cv_off[(int64_t)p1 * P + p2 + 1]++;
            }
    int64_t nc = 0;
    for (int64_t i = 0; i < NB; ++i) {
        nc += cv_off[i + 1];
        if (nc > INT32_MAX) return YV_ERR_CAPACITY;
        cv_off[i + 1] = (int32_t)nc;
    }
    std::vector<int32_t> cv_e1(std::max<int64_t>(nc, 1)), cv_e2(std::max<int64_t>(nc, 1));
    {
        std::vector<int32_t> fill(cv_off.begin(), cv_off.end() - 1);
        for (int l = 0; l < L; ++l)
            for (int a = le_off[l]; a < le_off[l + 1]; ++a)
                for (int c = le_off[l]; c < le_off[l + 1]; ++c) {
                    const int p1 = edge_pose[le[a]], p2 = edge_pose[le[c]];
                    if (p1 > p2) continue;
                    const int32_t k = fill[(int64_t)p1 * P + p2]++;
                    cv_e1[k] = le[a];
                    cv_e2[k] = le[c];
                }
    }
    if (nc > b->cv_cap) {
        b->mem.release(b->d_cv_e1, b->d_cv_e2);
        b->cv_cap = 0;
        if (b->mem.alloc(&b->d_cv_e1, nc) != YV_OK || b->mem.alloc(&b->d_cv_e2, nc) != YV_OK) return YV_ERR_HIP;
        b->cv_cap = nc;
    }
    auto h2d = [&](void* d, const void* h, size_t bytes) {
        return bytes == 0 || hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, b->st) == hipSuccess;
    };
    bool ok = h2d(b->d_ep, edge_pose, sizeof(int32_t) * E) && h2d(b->d_el, edge_landmark, sizeof(int32_t) * E) &&
              h2d(b->d_meas, meas, sizeof(double) * 2 * E) && h2d(b->d_pe_off, pe_off.data(), 4 * (P + 1)) &&
              h2d(b->d_pe, pe.data(), 4 * (size_t)E) && h2d(b->d_le_off, le_off.data(), 4 * (size_t)(L + 1)) &&
              h2d(b->d_le, le.data(), 4 * (size_t)E) && h2d(b->d_cv_off, cv_off.data(), 4 * (size_t)(NB + 1)) &&
              h2d(b->d_cv_e1, cv_e1.data(), 4 * (size_t)nc) && h2d(b->d_cv_e2, cv_e2.data(), 4 * (size_t)nc);
    // the pageable sources die with this call
    if (!ok || hipStreamSynchronize(b->st) != hipSuccess) return YV_ERR_HIP;
    yavo::BaParams& Q = b->P;
    Q.P = P;
    Q.nf = n_fixed;
    Q.np = P - n_fixed;
    Q.ns = 6 * Q.np;
    if (ba_ensure_schur(b, Q.np, b->st) != YV_OK || ba_reset_tickets(b, b->st) != YV_OK) return YV_ERR_HIP;
    Q.L = L;
    Q.E = E;
    Q.ep = b->d_ep;
    Q.el = b->d_el;
    Q.meas = b->d_meas;
    Q.pe_off = b->d_pe_off;
    Q.pe = b->d_pe;
    Q.le_off = b->d_le_off;
    Q.le = b->d_le;
    Q.cv_off = b->d_cv_off;
    Q.cv_e1 = b->d_cv_e1;
    Q.cv_e2 = b->d_cv_e2;
    std::memcpy(b->K.v, K, sizeof b->K.v);
    b->ready = true;
    return YV_OK;
}

namespace {

// The LM of yv_ba_solve with its control on the device (default): the host enqueues every iteration's kernels
// without waiting -- linearise + H / b (whose last workgroup begins the iteration), one damping trial (Dinv / W,
// Schur, LDLT, step into the trial state, chi2 + scale, whose last workgroup decides and ends the iteration) -- and
// the control block (lambda, ni, currentChi, stop / accept) gates the kernels. g2o's trial loop usually accepts its
// first trial; an iteration that needs more suspends the solve (every later kernel skips) and the host resumes it.
// One read-back per solve, plus one per suspended trial loop.
// poses / landmarks: host in / out; both nullptr: the problem's poses and landmarks are already in Q.poses / Q.X on
// the device (yv_ba_window_solve) and stay there.
//
// the kernels' arguments under the control block: Pc for the first chi2, Pit gated per iteration (the linearisation),
// Ptr gated per trial, its lambda read from the block
struct BaGated {
    yavo::BaParams Pc, Pit, Ptr;
};
BaGated ba_gated(const yv_ba* b) {
    yavo::BaCtl* c = b->d_ctl;
    BaGated g;
    g.Pc = b->P;
    g.Pc.ctl = c;
    g.Pc.log = b->d_log;
    g.Pit = g.Ptr = g.Pc;
    g.Pit.gate = &c->skip_iter;
    g.Ptr.gate = &c->skip_trial;
    g.Ptr.lam = &c->lambda;
    return g;
}

// the enqueue half: chi2 at the start, then every iteration with one trial slot, then the control block's read-back
// (asynchronous: ba_solve_wait collects it)
int ba_solve_enqueue_(yv_ba* b, const double* poses, const double* landmarks, int max_iters) {
    yavo::BaParams& Q = b->P;
    const size_t pb = sizeof(double) * 7 * Q.P, xb = sizeof(double) * 3 * Q.L;
    hipStream_t st = b->st;
    if (max_iters + 1 > b->log_cap) {
        if (hipStreamSynchronize(st) != hipSuccess) return YV_ERR_HIP;
        b->mem.release(b->d_log);
        b->log_cap = 0;
        if (b->mem.alloc(&b->d_log, (size_t)max_iters + 1) != YV_OK) return YV_ERR_HIP;
        b->mem.release(b->h_log);
        if (b->mem.alloc_host(&b->h_log, (size_t)max_iters + 1) != YV_OK) return YV_ERR_HIP;
        b->log_cap = max_iters + 1;
    }
    yavo::BaCtl* c = b->d_ctl;
    const BaGated g = ba_gated(b);  // after d_log is final
    // (*Q.cur is reset by the first kernel, ba_chi2_kernel)
    if (poses && (hipMemcpyAsync(Q.poses, poses, pb, hipMemcpyHostToDevice, st) != hipSuccess ||
                  (xb && hipMemcpyAsync(Q.X, landmarks, xb, hipMemcpyHostToDevice, st) != hipSuccess)))
        return YV_ERR_HIP;
    yavo::launch_ba_chi2(g.Pc, b->K, st);
    for (int it = 0; it < max_iters; ++it) {
        yavo::launch_ba_linearize(g.Pit, b->K, it == 0 ? 1 : 0, st);
        yavo::launch_ba_trial(g.Ptr, b->K, 0.0, st);
    }
    // the end of the solve in the same submission (skipped on the device when it was suspended; ba_solve_wait then
    // resumes it and reruns these), so an unsuspended solve is collected with one wait
    yavo::BaParams Pf = Q;
    Pf.gate = &c->suspended;
    yavo::launch_ba_finish(Pf, st);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(b->h_log, b->d_log, sizeof(double) * (max_iters + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(b->h_ctl, c, sizeof(yavo::BaCtl), hipMemcpyDeviceToHost, st) != hipSuccess)
        return YV_ERR_HIP;
    return YV_OK;
}

}  // namespace

int yavo::ba_solve_enqueue(yv_ba* b, const double* poses, const double* landmarks, int max_iters) {
    const int rc = ba_solve_enqueue_(b, poses, landmarks, max_iters);
    if (rc != YV_OK) (void)ba_reset_tickets(b, b->st);
    return rc;
}

// the collecting half: waits for the control block, resumes a suspended trial loop (one read-back each) until the
// solve ends, then the estimate into Q.poses / Q.X (host copies when poses != nullptr) and the chi2 log
int yavo::ba_solve_wait(yv_ba* b, double* poses, double* landmarks, int max_iters, double* chi2_log, int* iters) {
    yavo::BaParams& Q = b->P;
    const size_t pb = sizeof(double) * 7 * Q.P, xb = sizeof(double) * 3 * Q.L;
    hipStream_t st = b->st;
    yavo::BaCtl* c = b->d_ctl;
    const BaGated g = ba_gated(b);
    b->resumed = false;
    for (;;) {
        if (hipStreamSynchronize(st) != hipSuccess) return YV_ERR_HIP;
        if (!b->h_ctl->suspended) break;
        b->resumed = true;
        ++b->resumes;
        yavo::launch_ba_ctl_resume(c, st);  // the suspended iteration's trial loop continues at its trial q
        const int first = b->h_ctl->it;
        for (int it = first; it < max_iters; ++it) {
            if (it != first) yavo::launch_ba_linearize(g.Pit, b->K, 0, st);
            yavo::launch_ba_trial(g.Ptr, b->K, 0.0, st);
        }
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(b->h_ctl, c, sizeof(yavo::BaCtl), hipMemcpyDeviceToHost, st) != hipSuccess)
            return YV_ERR_HIP;
    }
    const int n_it = max_iters > 0 ? b->h_ctl->iters : 0;
    if (b->resumed) {
        yavo::launch_ba_finish(Q, st);
        if (hipMemcpyAsync(b->h_log, b->d_log, sizeof(double) * (max_iters + 1), hipMemcpyDeviceToHost, st) !=
            hipSuccess)
            return YV_ERR_HIP;
    }
    if (poses && (hipMemcpyAsync(poses, Q.poses, pb, hipMemcpyDeviceToHost, st) != hipSuccess ||
                  (xb && hipMemcpyAsync(landmarks, Q.X, xb, hipMemcpyDeviceToHost, st) != hipSuccess)))
        return YV_ERR_HIP;
    if ((b->resumed || poses) && hipStreamSynchronize(st) != hipSuccess) return YV_ERR_HIP;
    if (chi2_log) std::memcpy(chi2_log, b->h_log, sizeof(double) * (n_it + 1));
    if (iters) *iters = n_it;
    return YV_OK;
}

namespace {

int ba_solve_device(yv_ba* b, double* poses, double* landmarks, int max_iters, double* chi2_log, int* iters) {
    const int rc = ba_solve_enqueue(b, poses, landmarks, max_iters);
    if (rc != YV_OK) return rc;
    return ba_solve_wait(b, poses, landmarks, max_iters, chi2_log, iters);
}

}  // namespace

extern "C" int yv_ba_set_control(yv_ba* b, int on_device) {
    if (!b || on_device < 0 || on_device > 1) return YV_ERR_INVALID;
    b->device_control = on_device;
    return YV_OK;
}

// g2o OptimizationAlgorithmLevenberg::solve, as or_ba_lm: the host runs the damping control on the device's chi2
// and scale (bit-identical double arithmetic), the device everything per edge / landmark / pose
extern "C" int yv_ba_solve(yv_ba* b, double* poses, double* landmarks, int max_iters, double* chi2_log, int* iters) {
    if (!b || !b->ready || !poses || (b->P.L > 0 && !landmarks) || max_iters < 0) return YV_ERR_INVALID;
    if (hipSetDevice(b->dev) != hipSuccess) return YV_ERR_HIP;
    if (b->device_control) return ba_solve_device(b, poses, landmarks, max_iters, chi2_log, iters);
    yavo::BaParams& Q = b->P;
    const size_t pb = sizeof(double) * 7 * Q.P, xb = sizeof(double) * 3 * Q.L;
    hipStream_t st = b->st;
    int cur = 0;  // the state the estimate is in (the device's *Q.cur, which the host sets)
    if (hipMemsetAsync(b->d_cur, 0, sizeof(int), st) != hipSuccess ||
        hipMemcpyAsync(Q.poses, poses, pb, hipMemcpyHostToDevice, st) != hipSuccess ||
        (xb && hipMemcpyAsync(Q.X, landmarks, xb, hipMemcpyHostToDevice, st) != hipSuccess))
        return YV_ERR_HIP;
    yavo::launch_ba_chi2(Q, b->K, st);
    if (ba_sync_scal(b, 1) != YV_OK) return YV_ERR_HIP;
    double currentChi = b->h_scal[0];
    if (chi2_log) chi2_log[0] = currentChi;
    double lambda = 0, ni = 2;
    int it;
    for (it = 0; it < max_iters; ++it) {
        if (it == 0 && hipMemsetAsync(b->d_maxdiag, 0, sizeof(unsigned long long), st) != hipSuccess) return YV_ERR_HIP;
        yavo::launch_ba_linearize(Q, b->K, it == 0 ? 1 : 0, st);
        if (it == 0) {
            unsigned long long bits = 0;
            if (hipMemcpyAsync(&bits, b->d_maxdiag, sizeof bits, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return YV_ERR_HIP;
            double maxd;
            std::memcpy(&maxd, &bits, sizeof maxd);
            lambda = 1e-5 * maxd;
            ni = 2;
        }
        double rho = 0;
        int q = 0;
        do {
            yavo::launch_ba_trial(Q, b->K, lambda, st);
            if (hipGetLastError() != hipSuccess || ba_sync_scal(b, 3) != YV_OK) return YV_ERR_HIP;
            double tempChi = b->h_scal[0];
            const bool ok2 = Q.ns > 0 ? b->h_scal[2] != 0.0 : true;
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = b->h_scal[1];
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - yavo::cube_cr(2 * rho - 1);  // pow(2 rho - 1, 3), correctly rounded
                alpha = fmin(alpha, 2. / 3.);
                const double sf = fmax(1. / 3., alpha);
                lambda *= sf;
                ni = 2;
                currentChi = tempChi;
                cur ^= 1;  // the trial state becomes the estimate
                if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->d_cur), cur, 1, st) != hipSuccess)
                    return YV_ERR_HIP;
            } else {
                lambda *= ni;
                ni *= 2;
            }
            q++;
        } while (rho < 0 && q < 10);
        if (chi2_log) chi2_log[it + 1] = currentChi;
        if (q == 10 || rho == 0 || !std::isfinite(lambda)) {
            ++it;
            break;
        }
    }
    yavo::launch_ba_finish(Q, st);
    if (hipMemcpyAsync(poses, Q.poses, pb, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (xb && hipMemcpyAsync(landmarks, Q.X, xb, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return YV_ERR_HIP;
    if (iters) *iters = it;
    return YV_OK;
}

// diagnostics: copy one of the workspace's device buffers (as left by the last yv_ba_solve) to the host
extern "C" int yv_ba_debug_resumes(yv_ba* b) { return b ? b->resumes : -1; }

extern "C" int yv_ba_debug_read(yv_ba* b, int which, double* dst, int64_t count) {
    if (!b || !b->ready || !dst || count < 0) return YV_ERR_INVALID;
    const yavo::BaParams& Q = b->P;
    // which = 3 (H_pl), 4 (W) and 9 (Dinv) are no longer stored (formed where they are read): YV_ERR_INVALID
    if (which == 3 || which == 4 || which == 9) return YV_ERR_INVALID;
    double* const bufs[] = {Q.err, Q.Jp, Q.Jl, nullptr, nullptr, Q.Hpp, Q.bp, Q.Hll, Q.bl, nullptr, Q.S, Q.bs, Q.xp, Q.xl,
                            Q.poses, Q.X, Q.scal};
    const int64_t sizes[] = {2LL * Q.E, 12LL * Q.E, 6LL * Q.E, 18LL * Q.E, 18LL * Q.E, 36LL * Q.P, 6LL * Q.P,
                             9LL * Q.L, 3LL * Q.L, 9LL * Q.L, (int64_t)Q.ns * Q.ns, Q.ns, Q.ns, 3LL * Q.L,
                             7LL * Q.P, 3LL * Q.L, 16};
    if (which < 0 || which >= (int)(sizeof sizes / sizeof sizes[0]) || count > sizes[which]) return YV_ERR_INVALID;
    if (hipSetDevice(b->dev) != hipSuccess || hipStreamSynchronize(b->st) != hipSuccess) return YV_ERR_HIP;
    if (count && hipMemcpy(dst, bufs[which], sizeof(double) * count, hipMemcpyDeviceToHost) != hipSuccess)
        return YV_ERR_HIP;
    return YV_OK;
}
