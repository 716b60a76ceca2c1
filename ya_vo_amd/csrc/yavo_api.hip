// yavo_api.hip -- the context's part of the C ABI of libyavo.so (include/yavo/yavo.h): create / destroy / setters,
// streams, upload / download / alloc, the two host staging mechanisms (yavo_host.h), the single-image workspace and the
// host-pointer drop-in entry points.  Host code only; kernels live in the stage files.  No CPU fallback exists: every
// compute path runs the gfx950 kernels.
#include "yavo_host.h"

using namespace yavo;

namespace {

// ---- pinned staging of the host-pointer entry points (yv_ctx::h_stage) ----
bool in_pinned_scratch(const yv_ctx* ctx, const void* p) {
    const char* c = static_cast<const char*>(p);
    const char* b = reinterpret_cast<const char*>(ctx->h_pinned);
    return ctx->h_pinned && c >= b && c < b + 64 * sizeof(int32_t);
}

}  // namespace

namespace yavo {

int ctx_device(yv_ctx* ctx) { return ctx->device; }
hipStream_t ctx_stream(yv_ctx* ctx) { return ctx->stream; }

// the downloads of the call land in the caller's buffers once the stream has drained
hipError_t stage_sync(yv_ctx* ctx, hipStream_t s) {
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        ctx->pending.clear();
        return e;
    }
    for (const auto& d : ctx->pending) std::memcpy(d.dst, d.src, d.bytes);
    ctx->pending.clear();
    ctx->h_stage_off = 0;
    return hipSuccess;
}

// `bytes` of the staging buffer for this call (64-B aligned); grows it after draining the stream when full
uint8_t* stage_alloc(yv_ctx* ctx, size_t bytes, hipStream_t s) {
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (ctx->h_stage_off + need > ctx->h_stage_cap) {
        if (ctx->h_stage_off > 0 && stage_sync(ctx, s) != hipSuccess) return nullptr;
        if (need > ctx->h_stage_cap) {
            ctx->mem.release(ctx->h_stage);
            ctx->h_stage_cap = 0;
            const size_t cap = std::max(need, (size_t)4 << 20);
            if (ctx->mem.alloc_host(&ctx->h_stage, cap) != YV_OK) return nullptr;
            ctx->h_stage_cap = cap;
        }
    }
    uint8_t* p = ctx->h_stage + ctx->h_stage_off;
    ctx->h_stage_off += need;
    return p;
}

hipError_t stage_h2d(yv_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    if (in_pinned_scratch(ctx, src)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    uint8_t* p = stage_alloc(ctx, bytes, s);
    if (!p) return hipErrorOutOfMemory;
    std::memcpy(p, src, bytes);
    return hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
}

// a pitched host image (rows of `width` bytes, `spitch` apart) into a pitched device image
hipError_t stage_h2d_2d(yv_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                        size_t height, hipStream_t s) {
    if (width == 0 || height == 0) return hipSuccess;
    uint8_t* p = stage_alloc(ctx, width * height, s);
    if (!p) return hipErrorOutOfMemory;
    const uint8_t* q = static_cast<const uint8_t*>(src);
    if (spitch == width) std::memcpy(p, q, width * height);
    else
        for (size_t r = 0; r < height; ++r) std::memcpy(p + r * width, q + r * spitch, width);
    // a packed destination takes one linear DMA: hipMemcpy2DAsync moves a 376-row image as row-sized transfers at
    // ~0.2 GB/s (2.6 ms per KITTI frame in the r03 LoopHandler trace)
    if (dpitch == width) return hipMemcpyAsync(dst, p, width * height, hipMemcpyHostToDevice, s);
    return hipMemcpy2DAsync(dst, dpitch, p, width, width, height, hipMemcpyHostToDevice, s);
}

hipError_t stage_d2h(yv_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    if (in_pinned_scratch(ctx, dst)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
    uint8_t* p = stage_alloc(ctx, bytes, s);
    if (!p) return hipErrorOutOfMemory;
    ctx->pending.push_back({dst, p, bytes});
    return hipMemcpyAsync(p, src, bytes, hipMemcpyDeviceToHost, s);
}

// ---- the geometry host calls' arena (struct Arena, yavo_host.h) ----
int Arena::commit() {
    if (need > ctx->scratch_cap) {
        ctx->mem.release(ctx->scratch, ctx->scratch_h);
        ctx->scratch_cap = 0;
        size_t cap = std::max(need, (size_t)1 << 20);
        if (ctx->mem.alloc(&ctx->scratch, cap) != YV_OK) return YV_ERR_HIP;
        void* hd = nullptr;
        // coherent (fine-grained) host memory: kernels read and write the host regions uncached, so nothing of a
        // previous call can be stale in the GPU's caches
        if (ctx->mem.alloc_host(&ctx->scratch_h, cap, hipHostMallocMapped | hipHostMallocCoherent) != YV_OK ||
            hipHostGetDevicePointer(&hd, ctx->scratch_h, 0) != hipSuccess) {
            ctx->mem.release(ctx->scratch_h);
            return YV_ERR_HIP;
        }
        ctx->scratch_hd = static_cast<uint8_t*>(hd);
        ctx->scratch_cap = cap;
    }
    char* base = reinterpret_cast<char*>(ctx->scratch);
    size_t off = 0;
    host_spans.clear();
    for (auto& r : reqs) {
        *r.p = r.host ? static_cast<void*>(ctx->scratch_hd + off) : static_cast<void*>(base + off);
        if (r.host) host_spans.push_back({off, off + r.bytes});
        off += (r.bytes + 255) & ~(size_t)255;
    }
    return YV_OK;
}

bool Arena::is_host(const void* p) const {
    const uint8_t* q = static_cast<const uint8_t*>(p);
    return q >= ctx->scratch_hd && q < ctx->scratch_hd + ctx->scratch_cap;
}

size_t Arena::off_of(const void* p) const {
    return is_host(p) ? (size_t)(static_cast<const uint8_t*>(p) - ctx->scratch_hd)
                      : (size_t)(static_cast<const char*>(p) - static_cast<const char*>(ctx->scratch));
}

void Arena::in(const void* dev, const void* src, size_t bytes) {
    if (!bytes) return;
    const size_t o = off_of(dev);
    std::memcpy(ctx->scratch_h + o, src, bytes);
    if (is_host(dev)) return;  // read by the kernel where it is
    in_lo = std::min(in_lo, o);
    in_hi = std::max(in_hi, o + bytes);
}

void Arena::in_2d(const void* dev, const uint8_t* src, size_t spitch, size_t width, size_t height) {
    if (!width || !height) return;
    const size_t o = off_of(dev);
    uint8_t* p = ctx->scratch_h + o;
    if (spitch == width) std::memcpy(p, src, width * height);
    else
        for (size_t r = 0; r < height; ++r) std::memcpy(p + r * width, src + r * spitch, width);
    in_lo = std::min(in_lo, o);
    in_hi = std::max(in_hi, o + width * height);
}

void Arena::out(void* dst, const void* dev, size_t bytes) {
    if (!bytes) return;
    const size_t o = off_of(dev);
    outs.push_back({dst, o, bytes});
    if (is_host(dev)) return;  // written by the kernel where it is
    out_lo = std::min(out_lo, o);
    out_hi = std::max(out_hi, o + bytes);
}

hipError_t Arena::upload(hipStream_t s) {
    if (in_hi <= in_lo) return hipSuccess;
    return hipMemcpyAsync(static_cast<char*>(ctx->scratch) + in_lo, ctx->scratch_h + in_lo, in_hi - in_lo,
                          hipMemcpyHostToDevice, s);
}

hipError_t Arena::download(hipStream_t s) {
    if (out_hi <= out_lo) return hipSuccess;
    bool split = false;
    for (const auto& h : host_spans) split |= h.first < out_hi && h.second > out_lo;
    if (!split)
        return hipMemcpyAsync(ctx->scratch_h + out_lo, static_cast<char*>(ctx->scratch) + out_lo,
                              out_hi - out_lo, hipMemcpyDeviceToHost, s);
    for (const auto& o : outs) {
        bool host = false;
        for (const auto& h : host_spans) host |= o.off >= h.first && o.off < h.second;
        if (host) continue;
        hipError_t e = hipMemcpyAsync(ctx->scratch_h + o.off, static_cast<char*>(ctx->scratch) + o.off, o.bytes,
                                      hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void Arena::finish() {
    for (const auto& o : outs) std::memcpy(o.dst, ctx->scratch_h + o.off, o.bytes);
}

hipError_t Arena::fetch(hipStream_t s) {
    hipError_t e = download(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) finish();
    return e;
}

// the device's CU count (256 when the runtime does not tell)
static int ctx_cus(yv_ctx* ctx) {
    if (ctx->cus <= 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0) {
            (void)hipGetLastError();
            cus = 256;
        }
        ctx->cus = cus;
    }
    return ctx->cus;
}

// brief_kernel's worker limit: two LDS regions of <= 80 KiB per CU (one where a wider band's region is larger),
// under the test cap of yv_debug_set_brief_workers
int brief_workers(yv_ctx* ctx, int W) {
    const int w = ctx_cus(ctx) * yavo::brief_workers_per_cu(W);
    return ctx->brief_cap > 0 ? std::min(w, ctx->brief_cap) : w;
}

int records_workgroups(yv_ctx* ctx) { return ctx_cus(ctx) * 8; }

hipStream_t make_queue_stream(yv_ctx* ctx) {
    const int cus = ctx_cus(ctx);
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
    for (int c = 0; c < cus; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
    hipStream_t s = nullptr;
    if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
        s = nullptr;
        (void)hipGetLastError();
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
    }
    return s;
}

}  // namespace yavo

namespace {

// The host-pointer entry points share one single-image workspace per context.
int ensure_single(yv_ctx* ctx, int H, int W) {
    if (ctx->single && ctx->single->H == H && ctx->single->W == W) return YV_OK;
    if (ctx->single) {
        batch_free(ctx->single);
        ctx->single = nullptr;
    }
    yv_batch* b = nullptr;
    int rc = yv_batch_create(ctx, 1, H, W, yavo::kMaxKp, 1, &b);
    if (rc != YV_OK) return rc;
    const int32_t pair[2] = {0, 1};  // query = slot 0, train = slot 1 (the carry slot)
    rc = yv_batch_set_pairs(b, pair, 1);
    if (rc != YV_OK) {
        batch_free(b);
        return rc;
    }
    ctx->single = b;
    return YV_OK;
}

// ---- keypoint selection (yv_set_keypoint_select) ----
bool select_args_ok(int nms_radius, int cell_rows, int cell_cols, int per_cell) {
    if (nms_radius < 0 || nms_radius > yavo::kSelMaxRadius || per_cell < 0 || per_cell > yavo::kSelMaxPerCell)
        return false;
    if (per_cell > 0 && (cell_rows < yavo::kSelMinCell || cell_rows > yavo::kSelMaxCell ||
                         cell_cols < yavo::kSelMinCell || cell_cols > yavo::kSelMaxCell))
        return false;
    return true;
}

// One pair of host keypoint lists through the single-image workspace (the matcher does not look at the image size:
// whatever workspace exists, or a minimal one): the buffers the stage needs, the query list into slot 0, the train list
// into slot 1 (the carry slot), their counts and packed descriptors, the gate if any, then the stage.
int match_single_pair(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, MatchStage st,
                      const int32_t* gate, hipStream_t s) {
    int rc = ctx->single ? YV_OK : ensure_single(ctx, 16, 16);
    if (rc == YV_OK && st.top2) rc = ensure_match2(ctx->single);
    // the gated positions come from the caller: all 16 bits
    if (rc == YV_OK && gate) rc = ensure_gates(ctx->single, yavo::kGateMaxCoord, yavo::kGateMaxCoord);
    if (rc != YV_OK) return rc;
    yv_batch* b = ctx->single;
    YV_HIP(stage_h2d(ctx, b->keypoints, q, sizeof(yv_keypoint) * (size_t)nq, s));
    if (nt > 0) YV_HIP(stage_h2d(ctx, b->keypoints + (size_t)b->max_kp, t, sizeof(yv_keypoint) * (size_t)nt, s));
    ctx->h_pinned[0] = nq;
    ctx->h_pinned[1] = nt;
    YV_HIP(stage_h2d(ctx, b->kp_count, ctx->h_pinned, 2 * sizeof(int32_t), s));
    if (gate) YV_HIP(stage_h2d(ctx, b->gates, gate, 4 * sizeof(int32_t), s));
    yavo::launch_pack_desc(b->keypoints, b->kp_count, 2, b->max_kp, b->desc, s);
    st.max_train = nt;
    st.max_train_rev = nq;
    st.gated = gate != nullptr;
    (void)match_stage(b, st, s, -1);
    return check_launch();
}

// yv_match_knn2's / yv_match_gated's results of the single pair
int download_nn2(yv_ctx* ctx, yv_match2* out, int nq, int32_t* rev, int nt, hipStream_t s) {
    YV_HIP(stage_d2h(ctx, out, ctx->single->nn2, sizeof(yv_match2) * (size_t)nq, s));
    if (rev && nt > 0) YV_HIP(stage_d2h(ctx, rev, ctx->single->rev, sizeof(int32_t) * (size_t)nt, s));
    YV_HIP(stage_sync(ctx, s));
    return YV_OK;
}

// One array of a counted download: `elem` bytes per counted element from the device's `src` to the caller's `dst`
// (nullptr: not wanted).
struct CountedArray {
    void* dst;
    const void* src;
    size_t elem;
};

// The tail of a host-pointer call: the device's count into the pinned *h_count and a drain (which also lands whatever
// the caller staged before), then, when the count is positive, that many elements of a and b and a second drain.
int download_counted(yv_ctx* ctx, int32_t* h_count, const void* d_count, CountedArray a, CountedArray b,
                     hipStream_t s) {
    YV_HIP(stage_d2h(ctx, h_count, d_count, sizeof(int32_t), s));
    YV_HIP(stage_sync(ctx, s));
    const size_t k = *h_count > 0 ? (size_t)*h_count : 0;
    if (k == 0) return YV_OK;
    if (a.dst) YV_HIP(stage_d2h(ctx, a.dst, a.src, a.elem * k, s));
    if (b.dst) YV_HIP(stage_d2h(ctx, b.dst, b.src, b.elem * k, s));
    YV_HIP(stage_sync(ctx, s));
    return YV_OK;
}

}  // namespace

extern "C" {

int yv_abi_version(void) { return YV_ABI_VERSION; }

const char* yv_status_string(int status) {
    switch (status) {
        case YV_OK: return "ok";
        case YV_ERR_INVALID: return "invalid argument";
        case YV_ERR_HIP: return "HIP runtime error";
        case YV_ERR_NODEVICE: return "no usable GPU";
        case YV_ERR_CAPACITY: return "capacity exceeded";
        default: return "unknown status";
    }
}

int yv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int yv_create(int device, yv_ctx** out) {
    if (!out) return YV_ERR_INVALID;
    *out = nullptr;
    int n = yv_device_count();
    if (n <= 0) return YV_ERR_NODEVICE;
    if (device < 0 || device >= n) return YV_ERR_INVALID;
    yv_ctx* ctx = new (std::nothrow) yv_ctx();
    if (!ctx) return YV_ERR_INVALID;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return YV_ERR_HIP;
    }
    ctx->mem.adopt(ctx->stream);
    if (ctx->mem.alloc(&ctx->d_offsets, 1024) != YV_OK || hipMemset(ctx->d_offsets, 0, 1024) != hipSuccess ||
        ctx->mem.alloc_host(&ctx->h_pinned, 64) != YV_OK) {
        yv_destroy(ctx);
        return YV_ERR_HIP;
    }
    *out = ctx;
    return YV_OK;
}

void yv_destroy(yv_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->lk_cache) yv_lk_destroy(ctx->lk_cache);
    if (ctx->ess_cache) yv_essential_destroy(ctx->ess_cache);
    batch_free(ctx->single);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side);
    delete ctx;
}

void* yv_stream(yv_ctx* ctx) { return ctx ? reinterpret_cast<void*>(ctx->stream) : nullptr; }

// HIP binds each new stream to one of a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default), reusing the least
// used one once they are all taken, so two streams can end up on one queue and run in order: work meant to overlap
// then serialises (the sequence's BA stream against the context stream measured 0.067 vs 0.097 s for 1000 frames, one
// fresh stream in four, profiles/r06/c5, c6).  A stream with an explicit CU mask gets a queue of its own (the mask is
// a property of the queue); with every CU enabled it is an ordinary stream that never shares the context's queue.
void* yv_side_stream(yv_ctx* ctx) {
    if (!ctx) return nullptr;
    if (ctx->side) return reinterpret_cast<void*>(ctx->side);
    if (set_device(ctx) != YV_OK) return nullptr;
    ctx->side = make_queue_stream(ctx);
    if (ctx->side) ctx->mem.adopt(ctx->side);
    return reinterpret_cast<void*>(ctx->side);
}

int yv_sync(yv_ctx* ctx) {
    if (!ctx) return YV_ERR_INVALID;
    YV_HIP(hipStreamSynchronize(ctx->stream));
    return YV_OK;
}

int yv_download(yv_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes) {
    if (!ctx || (bytes > 0 && (!host_dst || !dev_src))) return YV_ERR_INVALID;
    if (bytes == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    YV_HIP(hipStreamSynchronize(ctx->stream));
    return YV_OK;
}

int yv_upload(yv_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes) {
    if (!ctx || (bytes > 0 && (!host_src || !dev_dst))) return YV_ERR_INVALID;
    if (bytes == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    YV_HIP(hipStreamSynchronize(ctx->stream));
    return YV_OK;
}

int yv_device_alloc(yv_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return YV_ERR_INVALID;
    *out = nullptr;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipMalloc(out, bytes ? bytes : 1));
    return YV_OK;
}

void yv_device_free(yv_ctx* ctx, void* p) {
    if (!ctx || !p) return;
    (void)set_device(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(p);
}

int yv_host_alloc(yv_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return YV_ERR_INVALID;
    *out = nullptr;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipHostMalloc(out, bytes ? bytes : 1));
    return YV_OK;
}

void yv_host_free(yv_ctx* ctx, void* p) {
    if (!ctx || !p) return;
    (void)set_device(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipHostFree(p);
}

int yv_set_fast_params(yv_ctx* ctx, int intensity_threshold, int max_corners) {
    if (!ctx || intensity_threshold < 0 || intensity_threshold > 255 || max_corners < 0 ||
        max_corners > yavo::kMaxKp)
        return YV_ERR_INVALID;
    ctx->fast_thr = intensity_threshold;
    ctx->max_corners = max_corners;
    return YV_OK;
}

int yv_set_keypoint_select(yv_ctx* ctx, int nms_radius, int cell_rows, int cell_cols, int per_cell) {
    if (!select_args_ok(nms_radius, cell_rows, cell_cols, per_cell) || !ctx) return YV_ERR_INVALID;
    ctx->sel_radius = nms_radius;
    ctx->sel_q = per_cell;
    ctx->sel_rows = per_cell > 0 ? cell_rows : 0;
    ctx->sel_cols = per_cell > 0 ? cell_cols : 0;
    return YV_OK;
}

int yv_set_harris_eigen(yv_ctx* ctx, int flavour) {
    if (!ctx || flavour < 0 || flavour > 1) return YV_ERR_INVALID;
    ctx->harris_eigen = flavour;
    return YV_OK;
}

int yv_set_brief_offsets(yv_ctx* ctx, const int8_t* offsets) {
    if (!ctx || !offsets) return YV_ERR_INVALID;
    for (int i = 0; i < 1024; ++i)
        if (offsets[i] < -8 || offsets[i] > 8) return YV_ERR_INVALID;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    YV_HIP(hipMemcpyAsync(ctx->d_offsets, offsets, 1024, hipMemcpyHostToDevice, ctx->stream));
    YV_HIP(hipStreamSynchronize(ctx->stream));
    ++ctx->offsets_version;
    return YV_OK;
}

int yv_set_brief_steering(yv_ctx* ctx, int n_bins, int radius, const int16_t* dirs, const int8_t* offsets) {
    if (n_bins < 0 || n_bins > yavo::kSteerMaxBins) return YV_ERR_INVALID;
    if (n_bins > 0) {
        if (!dirs || !offsets || radius < 1 || radius > yavo::kSteerMaxRadius) return YV_ERR_INVALID;
        for (int i = 0; i < 2 * n_bins; ++i)
            if (dirs[i] < -yavo::kSteerMaxDir || dirs[i] > yavo::kSteerMaxDir) return YV_ERR_INVALID;
        for (int i = 0; i < 1024 * n_bins; ++i)
            if (offsets[i] < -yavo::kSteerMaxRadius || offsets[i] > yavo::kSteerMaxRadius) return YV_ERR_INVALID;
    }
    if (!ctx) return YV_ERR_INVALID;
    if (n_bins == 0) {
        ctx->steer_bins = 0;
        return YV_OK;
    }
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    if (!ctx->d_steer_dirs && ctx->mem.alloc(&ctx->d_steer_dirs, 2 * (size_t)yavo::kSteerMaxBins) != YV_OK) return YV_ERR_HIP;
    if (!ctx->d_steer_addr && ctx->mem.alloc(&ctx->d_steer_addr, 256 * (size_t)yavo::kSteerMaxBins) != YV_OK) return YV_ERR_HIP;
    std::vector<uint32_t> addr(256 * (size_t)n_bins);
    yavo::steer_pack_offsets(offsets, 256 * n_bins, addr.data());
    // a run in flight reads the tables
    YV_HIP(hipStreamSynchronize(ctx->stream));
    YV_HIP(hipMemcpyAsync(ctx->d_steer_dirs, dirs, sizeof(int16_t) * 2 * (size_t)n_bins, hipMemcpyHostToDevice,
                          ctx->stream));
    YV_HIP(hipMemcpyAsync(ctx->d_steer_addr, addr.data(), sizeof(uint32_t) * addr.size(), hipMemcpyHostToDevice,
                          ctx->stream));
    YV_HIP(hipStreamSynchronize(ctx->stream));
    ctx->steer_bins = n_bins;
    ctx->steer_radius = radius;
    return YV_OK;
}

int yv_set_blur_kernel(yv_ctx* ctx, const uint16_t* k9) {
    if (!ctx || !k9) return YV_ERR_INVALID;
    uint32_t sum = 0;
    for (int i = 0; i < 9; ++i) {
        if (k9[i] > 255u) return YV_ERR_INVALID;  // the ABI's documented bound (yavo.h)
        sum += k9[i];
    }
    if (sum != 256u) return YV_ERR_INVALID;  // 8 fractional bits: the kernel must sum to 1.0
    std::memcpy(ctx->k9, k9, sizeof(ctx->k9));
    return YV_OK;
}

// ------------------------------------------------------------------------------------------------
// host-pointer drop-in entry points
// ------------------------------------------------------------------------------------------------
static int upload_image(yv_batch* b, const uint8_t* img, int stride, hipStream_t s) {
    YV_HIP(stage_h2d_2d(b->ctx, b->staging, (size_t)b->W, img, (size_t)stride, (size_t)b->W, (size_t)b->H, s));
    return YV_OK;
}

int yv_detect(yv_ctx* ctx, const uint8_t* img, int H, int W, int stride, int max_kp, int32_t* rc, float* resp,
              int* n, int* n_candidates) {
    if (!ctx || !img || !rc || !n || H < 9 || W < 9 || stride < W || max_kp < 0) return YV_ERR_INVALID;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    int st = ensure_single(ctx, H, W);
    if (st != YV_OK) return st;
    yv_batch* b = ctx->single;
    hipStream_t s = ctx->stream;
    const int keep = std::min(std::min(ctx->max_corners, max_kp), b->max_kp);
    st = prepare_select(b, H, W);
    if (st != YV_OK) return st;
    if (upload_image(b, img, stride, s) != YV_OK) return YV_ERR_HIP;
    yavo::launch_fast_harris(b->staging, 1, H, W, W, (int64_t)H * W, ctx->fast_thr, ctx->harris_eigen, b->cand_keys, b->cap,
                             b->cand_count, s);
    launch_select_topk(b, 1, keep, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    YV_HIP(stage_d2h(ctx, ctx->h_pinned + 1, b->cand_seen, sizeof(uint32_t), s));  // lands with the count
    st = download_counted(ctx, ctx->h_pinned, b->det_count, {rc, b->det_rc, 2 * sizeof(int32_t)},
                          {resp, b->det_resp, sizeof(float)}, s);
    if (st != YV_OK) return st;
    *n = ctx->h_pinned[0];
    if (n_candidates) *n_candidates = ctx->h_pinned[1];
    return YV_OK;
}

int yv_select_corners(yv_ctx* ctx, int H, int W, const int32_t* rc, const float* resp, int n, int max_kp,
                      int32_t* out_rc, float* out_resp, int* n_out) {
    if (!rc || !resp || !out_rc || !n_out || n < 0 || max_kp < 0 || H < 9 || W < 9) return YV_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (rc[2 * i] < 0 || rc[2 * i] >= H || rc[2 * i + 1] < 0 || rc[2 * i + 1] >= W) return YV_ERR_INVALID;
    if ((int64_t)n > (int64_t)(H - 8) * (W - 8)) return YV_ERR_CAPACITY;
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    if (!select_fits(ctx, H, W)) return YV_ERR_CAPACITY;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    int st = ensure_single(ctx, H, W);
    if (st != YV_OK) return st;
    yv_batch* b = ctx->single;
    st = prepare_select(b, H, W);  // the cells fit (tested above, before the device was touched)
    if (st != YV_OK) return st;
    hipStream_t s = ctx->stream;
    const int keep = std::min(std::min(ctx->max_corners, max_kp), b->max_kp);
    // the detect kernel's key, from the response's bits as they are: (~ord) << 32 | row * W + col
    if (n > 0) {
        uint64_t* keys = reinterpret_cast<uint64_t*>(stage_alloc(ctx, sizeof(uint64_t) * (size_t)n, s));
        if (!keys) return YV_ERR_HIP;
        for (int i = 0; i < n; ++i) {
            uint32_t u;
            std::memcpy(&u, resp + i, sizeof(u));
            const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            keys[i] = ((uint64_t)(~ord) << 32) | (uint64_t)((uint32_t)rc[2 * i] * (uint32_t)W + (uint32_t)rc[2 * i + 1]);
        }
        YV_HIP(hipMemcpyAsync(b->cand_keys, keys, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, s));
    }
    ctx->h_pinned[0] = n;
    YV_HIP(stage_h2d(ctx, b->cand_count, ctx->h_pinned, sizeof(uint32_t), s));
    launch_select_topk(b, 1, keep, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    st = download_counted(ctx, ctx->h_pinned + 1, b->det_count, {out_rc, b->det_rc, 2 * sizeof(int32_t)},
                          {out_resp, b->det_resp, sizeof(float)}, s);
    if (st != YV_OK) return st;
    *n_out = ctx->h_pinned[1];
    return YV_OK;
}

int yv_describe(yv_ctx* ctx, const uint8_t* img, int H, int W, int stride, const int32_t* rc, int n, yv_keypoint* out,
                int* n_out) {
    if (!ctx || !img || !out || !n_out || H < 9 || W < 9 || stride < W || n < 0 || (n > 0 && !rc)) return YV_ERR_INVALID;
    if (n > yavo::kMaxKp) return YV_ERR_CAPACITY;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    int st = ensure_single(ctx, H, W);
    if (st != YV_OK) return st;
    yv_batch* b = ctx->single;
    hipStream_t s = ctx->stream;
    if (steer_on(ctx) && ensure_steer(b) != YV_OK) return YV_ERR_HIP;
    if (upload_image(b, img, stride, s) != YV_OK) return YV_ERR_HIP;
    ctx->h_pinned[0] = n;
    if (n > 0) YV_HIP(stage_h2d(ctx, b->det_rc, rc, sizeof(int32_t) * 2 * (size_t)n, s));
    YV_HIP(stage_h2d(ctx, b->det_count, ctx->h_pinned, sizeof(int32_t), s));
    yavo::launch_blur9(b->staging, 1, H, W, W, (int64_t)H * W, ctx->k9, b->blur, s);
    yavo::launch_kp_boundary(b->det_rc, b->det_count, 1, H, W, b->max_kp, b->kp_src, b->kp_count, b->kp_band,
                             b->band_off, b->brief_heads, s);
    launch_describe(b, 1, brief_workers(ctx, W), s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    st = download_counted(ctx, ctx->h_pinned + 2, b->kp_count, {out, b->keypoints, sizeof(yv_keypoint)}, {}, s);
    if (st != YV_OK) return st;
    *n_out = ctx->h_pinned[2];
    return YV_OK;
}

int yv_orient(yv_ctx* ctx, const uint8_t* img, int H, int W, int stride, const int32_t* rc, int n, int32_t* moments,
              uint8_t* bin) {
    if (n < 0 || H < 9 || W < 9 || stride < W || (n > 0 && (!img || !rc || !moments || !bin))) return YV_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (rc[2 * i] < 0 || rc[2 * i] >= H || rc[2 * i + 1] < 0 || rc[2 * i + 1] >= W) return YV_ERR_INVALID;
    if (n > yavo::kMaxKp) return YV_ERR_CAPACITY;
    if (!ctx || !steer_on(ctx)) return YV_ERR_INVALID;
    if (n == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    int st = ensure_single(ctx, H, W);
    if (st != YV_OK) return st;
    yv_batch* b = ctx->single;
    hipStream_t s = ctx->stream;
    if (ensure_steer(b) != YV_OK) return YV_ERR_HIP;
    if (upload_image(b, img, stride, s) != YV_OK) return YV_ERR_HIP;
    ctx->h_pinned[0] = n;
    YV_HIP(stage_h2d(ctx, b->det_rc, rc, sizeof(int32_t) * 2 * (size_t)n, s));
    YV_HIP(stage_h2d(ctx, b->det_count, ctx->h_pinned, sizeof(int32_t), s));
    yavo::launch_blur9(b->staging, 1, H, W, W, (int64_t)H * W, ctx->k9, b->blur, s);
    const yavo::SteerTables t{ctx->steer_bins, ctx->steer_radius, ctx->d_steer_dirs, ctx->d_steer_addr};
    yavo::launch_orient(b->blur, H, W, t, b->det_rc, b->det_count, b->max_kp, b->steer_bin, b->steer_mom, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    YV_HIP(stage_d2h(ctx, moments, b->steer_mom, sizeof(int32_t) * 2 * (size_t)n, s));
    YV_HIP(stage_d2h(ctx, bin, b->steer_bin, (size_t)n, s));
    YV_HIP(stage_sync(ctx, s));
    return YV_OK;
}

int yv_match_features(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, yv_match* out) {
    if (!ctx || nq < 0 || nt < 0 || (nq > 0 && (!q || !out)) || (nt > 0 && !t)) return YV_ERR_INVALID;
    if (nq > yavo::kMaxKp || nt > yavo::kMaxKp) return YV_ERR_CAPACITY;
    if (nq == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    const int st = match_single_pair(ctx, q, nq, t, nt, MatchStage{}, nullptr, s);
    if (st != YV_OK) return st;
    YV_HIP(stage_d2h(ctx, out, ctx->single->matches, sizeof(yv_match) * (size_t)nq, s));
    YV_HIP(stage_sync(ctx, s));
    return YV_OK;
}

int yv_filter_matches(yv_ctx* ctx, const yv_match* in, int n, int thr, yv_match* out, int* n_out) {
    if (!ctx || !n_out || n < 0 || (n > 0 && (!in || !out))) return YV_ERR_INVALID;
    if (n > yavo::kMaxKp) return YV_ERR_CAPACITY;
    *n_out = 0;
    if (n == 0) return YV_OK;  // reference: minmax_element on an empty list is dereferenced (UB)
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    int st = ctx->single ? YV_OK : ensure_single(ctx, 16, 16);
    if (st != YV_OK) return st;
    yv_batch* b = ctx->single;
    hipStream_t s = ctx->stream;
    YV_HIP(stage_h2d(ctx, b->matches, in, sizeof(yv_match) * (size_t)n, s));
    yavo::launch_filter_records(b->matches, n, thr, b->filtered, b->filt_count, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    st = download_counted(ctx, ctx->h_pinned, b->filt_count, {out, b->filtered, sizeof(yv_match)}, {}, s);
    if (st != YV_OK) return st;
    *n_out = ctx->h_pinned[0];
    return YV_OK;
}

int yv_match_knn2(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, yv_match2* out,
                  int32_t* rev) {
    if (nq < 0 || nt < 0 || (nq > 0 && (!q || !out)) || (nt > 0 && !t)) return YV_ERR_INVALID;
    if (nq > yavo::kMaxKp || nt > yavo::kMaxKp) return YV_ERR_CAPACITY;
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    if (nq == 0) {
        if (rev)
            for (int j = 0; j < nt; ++j) rev[j] = -1;  // no query
        return YV_OK;
    }
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    MatchStage stage;
    stage.top2 = true;
    stage.with_rev = rev != nullptr;
    const int st = match_single_pair(ctx, q, nq, t, nt, stage, nullptr, s);
    return st != YV_OK ? st : download_nn2(ctx, out, nq, rev, nt, s);
}

int yv_match_gated(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, const int32_t gate[4],
                   yv_match2* out, int32_t* rev) {
    if (!gate || !q || !t || !out || nq < 0 || nt < 0 || !gate_ok(gate)) return YV_ERR_INVALID;
    if (nq > yavo::kMaxKp || nt > yavo::kMaxKp) return YV_ERR_CAPACITY;
    for (int i = 0; i < nq; ++i)
        if (q[i].x < 0 || q[i].x > yavo::kGateMaxCoord || q[i].y < 0 || q[i].y > yavo::kGateMaxCoord)
            return YV_ERR_INVALID;
    for (int j = 0; j < nt; ++j)
        if (t[j].x < 0 || t[j].x > yavo::kGateMaxCoord || t[j].y < 0 || t[j].y > yavo::kGateMaxCoord)
            return YV_ERR_INVALID;
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    if (nq == 0) {
        if (rev)
            for (int j = 0; j < nt; ++j) rev[j] = -1;  // no query
        return YV_OK;
    }
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    MatchStage stage;
    stage.top2 = true;
    stage.with_rev = rev != nullptr;
    const int st = match_single_pair(ctx, q, nq, t, nt, stage, gate, s);
    return st != YV_OK ? st : download_nn2(ctx, out, nq, rev, nt, s);
}

int yv_match_robust(yv_ctx* ctx, const yv_keypoint* q, int nq, const yv_keypoint* t, int nt, int thr, int flags,
                    int ratio_num, int ratio_den, yv_match* out, int* n_out, uint8_t* keep) {
    if (!match_filter_args_ok(flags, ratio_num, ratio_den) || !n_out || nq < 0 || nt < 0 ||
        (nq > 0 && (!q || !out)) || (nt > 0 && !t))
        return YV_ERR_INVALID;
    if (nq > yavo::kMaxKp || nt > yavo::kMaxKp) return YV_ERR_CAPACITY;
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    *n_out = 0;
    if (nq == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    const bool ratio = (flags & YV_MATCH_RATIO) != 0;
    MatchStage stage;
    stage.top2 = true;
    stage.with_rev = (flags & YV_MATCH_MUTUAL) != 0;
    stage.thr = thr;
    stage.flags = flags;
    stage.num = ratio ? ratio_num : 0;
    stage.den = ratio ? ratio_den : 1;
    int st = match_single_pair(ctx, q, nq, t, nt, stage, nullptr, s);
    if (st != YV_OK) return st;
    const yv_batch* b = ctx->single;
    if (keep) YV_HIP(stage_d2h(ctx, keep, b->keep, (size_t)nq, s));  // lands with the count
    st = download_counted(ctx, ctx->h_pinned, b->filt_count, {out, b->filtered, sizeof(yv_match)}, {}, s);
    if (st != YV_OK) return st;
    *n_out = ctx->h_pinned[0];
    return YV_OK;
}

int yv_stereo_subpix(yv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W, int stride,
                     const yv_match* m, int n, int half_win, int search, int32_t* dcol_q8, int32_t* sad,
                     uint8_t* status) {
    if (n < 0 || H < 9 || W < 9 || stride < W || half_win < 1 || half_win > yavo::kSubpixMaxWin || search < 1 ||
        search > yavo::kSubpixMaxSearch || (n > 0 && (!left || !right || !m || !dcol_q8 || !sad || !status)))
        return YV_ERR_INVALID;
    if (n > yavo::kMaxKp) return YV_ERR_CAPACITY;
    for (int i = 0; i < n; ++i) {
        const yv_keypoint &a = m[i].pt1, &b = m[i].pt2;
        if (a.x < 0 || a.x >= H || a.y < 0 || a.y >= W || b.x < 0 || b.x >= H || b.y < 0 || b.y >= W)
            return YV_ERR_INVALID;
    }
    if (!ctx) return yv_device_count() > 0 ? YV_ERR_INVALID : YV_ERR_NODEVICE;
    if (n == 0) return YV_OK;
    if (set_device(ctx) != YV_OK) return YV_ERR_HIP;
    StageScope stage_scope(ctx);
    hipStream_t s = ctx->stream;
    // the images keep the caller's stride and end with their last pixel, (H - 1) * stride + W bytes: the kernel's bound
    const size_t span = (size_t)(H - 1) * (size_t)stride + (size_t)W;
    Arena a{ctx};
    uint8_t *dl, *dr, *dst;
    yv_match* dm;
    int32_t *ddq, *dsad;
    a.add(&dl, span);
    a.add(&dr, span);
    a.add(&dm, (size_t)n);
    a.add_host(&ddq, (size_t)n);
    a.add_host(&dsad, (size_t)n);
    a.add_host(&dst, (size_t)n);
    if (a.commit() != YV_OK) return YV_ERR_HIP;
    a.in(dl, left, span);
    a.in(dr, right, span);
    a.in(dm, m, sizeof(yv_match) * (size_t)n);
    YV_HIP(a.upload(s));
    yavo::launch_subpix_list(dl, dr, H, W, stride, dm, n, half_win, search, yavo::SubpixOut{ddq, dsad, dst}, s);
    if (check_launch() != YV_OK) return YV_ERR_HIP;
    a.out(dcol_q8, ddq, sizeof(int32_t) * (size_t)n);
    a.out(sad, dsad, sizeof(int32_t) * (size_t)n);
    a.out(status, dst, (size_t)n);
    YV_HIP(a.fetch(s));
    return YV_OK;
}

// Test entry point (tests/test_gpu_brief_persistent.py; like yv_debug_xlane not part of the public headers): caps the
// number of brief_kernel's workers for the context's later launches, so that few workers walk many bands; 0 restores
// the default (two per CU).
int yv_debug_set_brief_workers(yv_ctx* ctx, int n) {
    if (!ctx || n < 0) return YV_ERR_INVALID;
    ctx->brief_cap = n;
    return YV_OK;
}

}  // extern "C"
