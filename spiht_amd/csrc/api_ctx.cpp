// Host side of libspiht_hip.so (include/spiht_hip.h), the context: status texts, the context -- create / destroy, scratch,
// timing, the device-side error word, options, colour model -- events and resident tickets, the diagnostic entry points, the
// page-locked host pool and the device-memory helpers.
#include "api_internal.h"

thread_local std::string g_hip_err;

static const char *STAGE_NAMES[ST_COUNT] = {"h2d", "d2h", "absmax", "pyramid", "encode_lists", "decode_lists",
                                            "dwt_level1", "dwt_rest", "idwt_rest", "idwt_level1", "memset", "gather"};

// memory at p goes back to the allocator: what is remembered about arrays there is void (option "pads_persist")
static void forget_pads(spiht_ctx *ctx, const void *p) {
    auto &v = ctx->pads_zeroed;
    v.erase(std::remove_if(v.begin(), v.end(), [&](const spiht_ctx::PadKey &k) { return k.p == p; }), v.end());
}

int ensure(spiht_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return SPIHT_OK;
    if (b.p) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        forget_pads(ctx, b.p);
        HIPCHK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        want = bytes;
        e = hipMalloc(&b.p, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            g_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e);
            b.p = nullptr;
            return SPIHT_ERR_NOMEM;
        }
    }
    b.cap = want;
    return SPIHT_OK;
}

static void drain_timing(spiht_ctx *ctx) {
    if (ctx->pending.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &r : ctx->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            ctx->ms[r.stage] += ms;
            ctx->launches[r.stage] += 1;
        }
        ctx->pool.push_back(r.a);
        ctx->pool.push_back(r.b);
    }
    ctx->pending.clear();
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------

extern "C" const char *spiht_strerror(int s) {
    switch (s) {
    case SPIHT_OK: return "ok";
    case SPIHT_ERR_LL: return "assertion failed: ll_h > 1 && ll_w > 1";
    case SPIHT_ERR_EMPTY: return "empty coefficient array";
    case SPIHT_ERR_SHAPE: return "offspring of the ll_h x ll_w root block fall outside the array (index out of bounds)";
    case SPIHT_ERR_CAPACITY: return "output buffer too small";
    case SPIHT_ERR_HIP: return "HIP runtime error";
    case SPIHT_ERR_ARG: return "invalid argument";
    case SPIHT_ERR_MAGNITUDE: return "coefficient magnitude >= 2^30 is outside the supported range";
    case SPIHT_ERR_INTERNAL: return "internal list capacity guard tripped";
    case SPIHT_ERR_TOO_LARGE: return "array or stream too large (c*h*w must be < 2^30, stream < 2^32 bits, a picture at most 65535 planes)";
    case SPIHT_ERR_NOMEM: return "out of device memory";
    case SPIHT_ERR_BUSY: return "the stream's ring is full: take a result first";
    case SPIHT_ERR_TIMEOUT: return "the step did not complete within the time given";
    case SPIHT_ERR_IDLE: return "nothing is submitted";
    default: return "unknown status";
    }
}
extern "C" const char *spiht_last_hip_error(void) { return g_hip_err.c_str(); }
extern "C" int spiht_abi_version(void) { return 2; }  // 2: round 3 (pipeline, occupancy words, options, geometry_mode, every wavelet / mode)

extern "C" int spiht_ctx_create(int device, spiht_ctx **out) { return spiht_ctx_create_priority(device, 0, out); }

// priority > 0: the context's stream is created with the device's highest stream priority -- its workgroups are placed
// before those of normal streams when both wait for room on the CUs (the list-coding contexts of a pipelined schedule)
extern "C" int spiht_ctx_create_priority(int device, int priority, spiht_ctx **out) {
    if (!out) return SPIHT_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        g_hip_err = "no such HIP device";
        return SPIHT_ERR_HIP;
    }
    HIPCHK(hipSetDevice(device));
    spiht_ctx *ctx = new spiht_ctx();
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        ctx->num_cu = prop.multiProcessorCount;
        ctx->tilectr.lds_per_cu = (int32_t)std::min<size_t>(prop.maxSharedMemoryPerMultiProcessor, (size_t)1 << 30);
    }
    ctx->tilectr.num_cu = ctx->num_cu;
    hipError_t e;
    if (priority > 0) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        e = hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest);
    } else {
        e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    }
    if (e != hipSuccess) {
        g_hip_err = std::string("hipStreamCreate: ") + hipGetErrorString(e);
        delete ctx;
        return SPIHT_ERR_HIP;
    }
    // `(max as f32).log2() as u8` with THIS host's libm (what Rust's f32::log2 lowers to on linux-gnu):
    // thresh[k] = smallest float below 2^k whose truncated log2f already reads k
    for (int k = 0; k < 32; k++) {
        float t = ldexpf(1.0f, k);
        if (k >= 1) {
            float m = nextafterf(t, 0.0f);
            int guard = 0;
            while (guard++ < 64 && m >= 1.0f && (int)log2f(m) == k) { t = m; m = nextafterf(m, 0.0f); }
        }
        ctx->log2_thresh[k] = t;
    }
    for (int s = 0; s < ST_COUNT; s++) { ctx->ms[s] = 0; ctx->launches[s] = 0; }
    int rc = ensure(ctx, ctx->err, 8192);  // (one error word; the rest is for diagnostic builds)
    if (rc != SPIHT_OK) { spiht_ctx_destroy(ctx); return rc; }
    (void)hipMemset(ctx->err.p, 0, 8192);
    rc = ensure(ctx, ctx->tilebuf, TILECTR_WORDS * sizeof(uint32_t));
    if (rc != SPIHT_OK) { spiht_ctx_destroy(ctx); return rc; }
    (void)hipMemset(ctx->tilebuf.p, 0, TILECTR_WORDS * sizeof(uint32_t));
    ctx->tilectr.dev = (uint32_t *)ctx->tilebuf.p;
    *out = ctx;
    return SPIHT_OK;
}

extern "C" void spiht_ctx_destroy(spiht_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    DevBuf *bufs[] = {&ctx->widebuf, &ctx->filt, &ctx->exttmp, &ctx->l1flags, &ctx->x, &ctx->dmsb, &ctx->lmsb, &ctx->maxabs, &ctx->out, &ctx->nbits, &ctx->maxn, &ctx->err,
                      &ctx->lists, &ctx->coeffs, &ctx->a0, &ctx->a1, &ctx->data, &ctx->nbytes, &ctx->rec, &ctx->mults,
                      &ctx->img, &ctx->trace, &ctx->meta, &ctx->recz, &ctx->lspcnt, &ctx->himg, &ctx->hrec, &ctx->tilebuf,
                      &ctx->pix, &ctx->hpix8, &ctx->rdpart, &ctx->tilescr, &ctx->allocscr, &ctx->layerscr, &ctx->tsettab};
    for (DevBuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (TableStage &s : ctx->tstages) {
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.host) (void)hipHostFree(s.host);
    }
    for (auto &r : ctx->pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : ctx->pool) (void)hipEventDestroy(e);
    if (ctx->copy_in) (void)hipStreamDestroy(ctx->copy_in);
    if (ctx->copy_out) (void)hipStreamDestroy(ctx->copy_out);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// Waits for the context's stream and reports (then clears) what the device-side guards of the calls queued before it
// recorded and no call has reported yet (take_err: the one place of that rule).
extern "C" int spiht_ctx_synchronize(spiht_ctx *ctx) {
    if (!ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    return take_err(ctx);
}
extern "C" int spiht_ctx_wait_on(spiht_ctx *ctx, spiht_ctx *other) {
    if (!ctx || !other || ctx->device != other->device) return SPIHT_ERR_ARG;
    if (ctx == other) return SPIHT_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e1 = hipEventRecord(ev, other->stream);
    hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(ctx->stream, ev, 0) : e1;
    (void)hipEventDestroy(ev);  // released once the wait has been satisfied
    HIPCHK(e2);
    return SPIHT_OK;
}
extern "C" int spiht_ctx_set_timing(spiht_ctx *ctx, int enabled) {
    if (!ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    drain_timing(ctx);
    ctx->timing = enabled != 0;
    return SPIHT_OK;
}
extern "C" int spiht_ctx_reset_timing(spiht_ctx *ctx) {
    if (!ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    drain_timing(ctx);
    for (int s = 0; s < ST_COUNT; s++) { ctx->ms[s] = 0; ctx->launches[s] = 0; }
    return SPIHT_OK;
}
extern "C" int spiht_ctx_num_stages(void) { return ST_COUNT; }
extern "C" const char *spiht_ctx_stage_name(int s) { return (s >= 0 && s < ST_COUNT) ? STAGE_NAMES[s] : ""; }
extern "C" int spiht_ctx_get_timing(spiht_ctx *ctx, int stage, double *ms, uint64_t *launches) {
    if (!ctx || stage < 0 || stage >= ST_COUNT) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    drain_timing(ctx);
    if (ms) *ms = ctx->ms[stage];
    if (launches) *launches = ctx->launches[stage];
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// device-side error word
// ------------------------------------------------------------------------------------------------
static int clear_err(spiht_ctx *ctx) {
    HIPCHK(hipMemsetAsync(ctx->err.p, 0, 4, ctx->stream));
    return SPIHT_OK;
}
static int read_err(spiht_ctx *ctx) {
    uint32_t e = 0;
    HIPCHK(hipMemcpyAsync(&e, ctx->err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (e & 2u) return SPIHT_ERR_MAGNITUDE;
    if (e & 4u) return SPIHT_ERR_CAPACITY;
    if (e & 1u) {
        g_hip_err = "device error word 0x" + [](uint32_t v) { char b[16]; snprintf(b, sizeof b, "%x", v); return std::string(b); }(e);
        return SPIHT_ERR_INTERNAL;
    }
    return SPIHT_OK;
}
// The latched error: waits for the stream and, when the word is set, returns its status, clears the word and stops trusting
// what the decoder left behind (a guard tripped: its lists may not describe what it wrote).  An error is reported once,
// by the first call that waits for the stream: spiht_ctx_synchronize(), or a synchronous single call -- those look before
// their own work (what an earlier batched call left belongs to the caller: the single call does not run) and after it.
int take_err(spiht_ctx *ctx) {
    const int st = read_err(ctx);  // includes the stream synchronize
    if (st == SPIHT_OK || st == SPIHT_ERR_HIP) return st;
    ctx->recz_clean = false;
    ctx->last_dec_valid = false;
    (void)clear_err(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    return st;
}

// The context's mutex for a SEQUENCE of calls (it is recursive: the calls inside take it again).  What needs it: a
// setting that is state of the context and must hold for exactly the calls of one caller -- the colour model
// (spiht_ctx_set_color3 ... image calls ... clear): without it another thread's call on the same context could run
// between the set and the clear and be coded in the wrong colour model.  Unlock from the thread that locked.
extern "C" int spiht_ctx_lock(spiht_ctx *ctx) {
    if (!ctx) return SPIHT_ERR_ARG;
    ctx->mu.lock();
    return SPIHT_OK;
}
extern "C" int spiht_ctx_unlock(spiht_ctx *ctx) {
    if (!ctx) return SPIHT_ERR_ARG;
    ctx->mu.unlock();
    return SPIHT_OK;
}

// Switches of this library's own making (nothing of the reference): "l1_flags" (default 1) the list decoder flags the occupied level-1 tiles for the inverse transform of the image-level
// decode calls.  Results are the same bits whatever the setting.  Unknown name / value: SPIHT_ERR_ARG.
extern "C" int spiht_ctx_set_option(spiht_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name || value < 0) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const bool b01 = value == 0 || value == 1;
    if (!strcmp(name, "l1_flags") && b01) ctx->opt_l1_flags = value != 0;
    else if (!strcmp(name, "idwt_groups") && value <= 8) ctx->tilectr.wg_per_cu = (int32_t)value;
    else if (!strcmp(name, "wide_encode") && value <= 3) ctx->opt_wide_encode = (int)value;
    else if (!strcmp(name, "wide_groups") && value <= 256) ctx->opt_wide_g = (int)value;
    else if (!strcmp(name, "wide_solo") && value <= (1 << 30)) ctx->opt_wide_solo = (int)value;
    else if (!strcmp(name, "pads_persist") && b01) ctx->opt_pads_persist = value != 0;
    else if (!strcmp(name, "meta_chunk") && value <= 65535) ctx->opt_meta_chunk = value;
    else return SPIHT_ERR_ARG;
    return SPIHT_OK;
}
extern "C" int spiht_ctx_get_option(spiht_ctx *ctx, const char *name, int64_t *value) {
    if (!ctx || !name || !value) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!strcmp(name, "l1_flags")) *value = ctx->opt_l1_flags;
    else if (!strcmp(name, "idwt_groups")) *value = ctx->tilectr.wg_per_cu;
    else if (!strcmp(name, "wide_encode")) *value = ctx->opt_wide_encode;
    else if (!strcmp(name, "wide_groups")) *value = ctx->opt_wide_g;
    else if (!strcmp(name, "wide_solo")) *value = ctx->opt_wide_solo;
    else if (!strcmp(name, "pads_persist")) *value = ctx->opt_pads_persist;
    else if (!strcmp(name, "meta_chunk")) *value = ctx->opt_meta_chunk;
    else if (!strcmp(name, "num_cu")) *value = ctx->num_cu;                    // (read-only: what the device reports)
    else if (!strcmp(name, "lds_per_cu")) *value = ctx->tilectr.lds_per_cu;
    else return SPIHT_ERR_ARG;
    return SPIHT_OK;
}

// The last encode call of this context that ran the several-CUs-per-image encoder: how many images (groups of workgroups)
// it had and how many of those groups gave up for lack of residency and were coded by the single-workgroup kernel behind
// it instead (csrc/encode_wide.hip).  Waits for the context's stream.  No such call yet: 0, 0.
extern "C" int spiht_ctx_wide_stats(spiht_ctx *ctx, uint32_t *groups, uint32_t *gave_up) {
    if (!ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int n = ctx->widebuf.p ? ctx->wide_last_groups : 0;
    std::vector<WideCtl> h((size_t)n);
    if (n) HIPCHK(hipMemcpy(h.data(), ctx->widebuf.p, (size_t)n * sizeof(WideCtl), hipMemcpyDeviceToHost));
    uint32_t gu = 0;
    for (const WideCtl &c : h) gu += (c.bad & 2u) ? 1u : 0u;
    if (groups) *groups = (uint32_t)n;
    if (gave_up) *gave_up = gu;
    return SPIHT_OK;
}

// Width of the list decoder's workgroups on this context.  12 wavefronts (default) walk one stream fastest; 8 take 4 %
// longer alone but leave the HBM-bound kernels that share the CUs with the decoder more room -- the setting of the
// list-coding contexts of the pipelined schedule (csrc/pipeline.cpp).  Same output either way.
extern "C" int spiht_ctx_set_decoder_waves(spiht_ctx *ctx, int waves) {
    if (!ctx || (waves != 8 && waves != 12)) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->dec_waves = waves;
    return SPIHT_OK;
}

// Colour model of the coded picture, fused into the transform: while set, every image-level entry point of
// this context takes and returns pixels in the caller's colour model (RGB) and codes them in the other one -- level 1 of the
// forward transform converts on its loads (w = M_f * spow(A_f * u, p_f) per pixel), level 1 of the inverse transform on its
// stores (A_i, M_i, p_i: the way back) -- for 3-channel float64 images.  A_f == NULL clears it.  Row-major 3x3 host arrays.
extern "C" int spiht_ctx_set_color3(spiht_ctx *ctx, const double *A_f, const double *M_f, double p_f, const double *A_i,
                                    const double *M_i, double p_i) {
    if (!ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!A_f) { ctx->color_on = false; return SPIHT_OK; }
    if (!M_f || !A_i || !M_i) return SPIHT_ERR_ARG;
    for (int i = 0; i < 9; i++) {
        ctx->col_fwd.A[i] = A_f[i]; ctx->col_fwd.M[i] = M_f[i];
        ctx->col_inv.A[i] = A_i[i]; ctx->col_inv.M[i] = M_i[i];
    }
    ctx->col_fwd.p = p_f;
    ctx->col_inv.p = p_i;
    ctx->color_on = true;
    return SPIHT_OK;
}

// what spiht_ctx_set_color3 last set (on == 0: nothing is set and the arrays are left alone); any output pointer may be NULL
extern "C" int spiht_ctx_get_color3(spiht_ctx *ctx, int *on, double *A_f, double *M_f, double *p_f, double *A_i, double *M_i,
                                    double *p_i) {
    if (!ctx || !on) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *on = ctx->color_on ? 1 : 0;
    if (!ctx->color_on) return SPIHT_OK;
    if (A_f) memcpy(A_f, ctx->col_fwd.A, 72);
    if (M_f) memcpy(M_f, ctx->col_fwd.M, 72);
    if (A_i) memcpy(A_i, ctx->col_inv.A, 72);
    if (M_i) memcpy(M_i, ctx->col_inv.M, 72);
    if (p_f) *p_f = ctx->col_fwd.p;
    if (p_i) *p_i = ctx->col_inv.p;
    return SPIHT_OK;
}

// Colour model change of B three-channel float64 images [B,3,npix] on the device: per pixel w = M * spow(A * u, p) with
// spow(x, p) = sign(x)|x|^p (the RGB <-> IPT shape; A, M row-major 3x3 host arrays).  d_out may equal d_in.
extern "C" int spiht_color3_batch_f64(spiht_ctx *ctx, const double *d_in, double *d_out, int64_t B, int64_t npix,
                                      const double *A, const double *M, double p) {
    if (!ctx || !d_in || !d_out || !A || !M || B < 0 || npix < 1 || B > 65535) return SPIHT_ERR_ARG;
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LAUNCHCHK(spiht_launch_color3(d_in, d_out, (int)B, (size_t)npix, A, M, p, ctx->stream));
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// events: ordering between contexts at a finer grain than spiht_ctx_wait_on
// ------------------------------------------------------------------------------------------------
struct spiht_event {
    int device;
    hipEvent_t ev;
};

// the context's HIP stream (a hipStream_t), for callers that put their own work (e.g. an RCCL collective) in order
// with the library's
extern "C" int spiht_ctx_stream(spiht_ctx *ctx, void **stream) {
    if (!ctx || !stream) return SPIHT_ERR_ARG;
    *stream = (void *)ctx->stream;
    return SPIHT_OK;
}

extern "C" int spiht_event_create(spiht_ctx *ctx, spiht_event **out) {
    if (!ctx || !out) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    spiht_event *e = new spiht_event;
    e->device = ctx->device;
    hipError_t r = hipEventCreateWithFlags(&e->ev, hipEventDisableTiming);
    if (r != hipSuccess) {
        delete e;
        g_hip_err = std::string("hipEventCreateWithFlags: ") + hipGetErrorString(r);
        return SPIHT_ERR_HIP;
    }
    *out = e;
    return SPIHT_OK;
}
extern "C" void spiht_event_destroy(spiht_event *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipEventDestroy(e->ev);
    delete e;
}
// marks the point reached by the work queued on ctx so far
extern "C" int spiht_event_record(spiht_event *e, spiht_ctx *ctx) {
    if (!e || !ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventRecord(e->ev, ctx->stream));
    return SPIHT_OK;
}
// work queued on ctx after this call starts only when the recorded point has been reached
extern "C" int spiht_ctx_wait_event(spiht_ctx *ctx, spiht_event *e) {
    if (!e || !ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamWaitEvent(ctx->stream, e->ev, 0));
    return SPIHT_OK;
}

// Placement between two contexts' kernels without a timer.  The large levels of the inverse transform run as persistent
// workgroups (a fixed number per CU) that count themselves in as they start; a ticket says what that count will read once
// every such launch queued on `ctx` SO FAR has all its workgroups on the CUs ...
extern "C" int spiht_ctx_resident_ticket(spiht_ctx *ctx, const void **d_counter, uint32_t *target) {
    if (!ctx || !d_counter || !target) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *d_counter = ctx->tilectr.dev ? (const void *)(ctx->tilectr.dev + TILECTR_STARTED) : nullptr;
    *target = ctx->tilectr.started;
    return SPIHT_OK;
}
// ... and this queues, on another context's stream, a one-wavefront kernel that waits for that count (at most timeout_us
// microseconds, <= 10 000: it must not hold its stream for ever if the launch it waits for never comes): the work queued
// behind it starts when those workgroups are resident.  d_counter NULL: nothing to wait for.
extern "C" int spiht_ctx_wait_resident(spiht_ctx *ctx, const void *d_counter, uint32_t target, uint32_t timeout_us) {
    if (!ctx || timeout_us > 10000u) return SPIHT_ERR_ARG;
    if (!d_counter) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LAUNCHCHK(spiht_launch_gate((const uint32_t *)d_counter, target, (uint64_t)timeout_us * 2400u, ctx->stream));  // (s_memtime: shader clocks)
    return SPIHT_OK;
}

#ifdef SPIHT_DIAG  // diagnostics of tools/corun*.py, not part of the product library (tools/build_variant.sh diag -DSPIHT_DIAG)
// diagnostic: copy the device error/debug words (64 x uint32) to the host
// diagnostic, not part of the ABI header: occupy the GPU with `blocks` idle workgroups for `ticks` clock ticks
extern "C" int spiht_debug_spin(spiht_ctx *ctx, int blocks, int threads, uint64_t ticks, uint32_t lds_bytes) {
    if (!ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LAUNCHCHK(spiht_launch_spin(blocks, threads, ticks, lds_bytes, (uint32_t *)ctx->err.p + 8, ctx->stream));
    return SPIHT_OK;
}

// diagnostic: ... with workgroups that do one kind of work (pyramid.hip: k_spin_kind)
extern "C" int spiht_debug_spin_kind(spiht_ctx *ctx, int blocks, int threads, uint64_t ticks, uint32_t lds_bytes, int mode) {
    if (!ctx) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LAUNCHCHK(spiht_launch_spin_kind(blocks, threads, ticks, lds_bytes, (uint32_t *)ctx->err.p + 8, mode, ctx->stream));
    return SPIHT_OK;
}

extern "C" int spiht_debug_words(spiht_ctx *ctx, uint32_t *out64) {
    if (!ctx || !out64) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(out64, ctx->err.p, 256, hipMemcpyDeviceToHost));
    return SPIHT_OK;
}
extern "C" int spiht_debug_words_ext(spiht_ctx *ctx, uint32_t *out2048) {
    if (!ctx || !out2048) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(out2048, ctx->err.p, 8192, hipMemcpyDeviceToHost));
    return SPIHT_OK;
}
#endif  // SPIHT_DIAG

// ------------------------------------------------------------------------------------------------
// page-locked host memory for the arrays the drop-in calls RETURN (spiht_wrapper.py:192-216 returns a new ndarray): a
// device -> host copy into such memory is one DMA at the link's speed; into fresh pageable memory it is staged copies
// plus a page fault per 4 KB (measured on a 1080p RGB picture, 49.8 MB: 4.2 ms against 1 ms).  Pooled, because pinning
// is what costs: a freed buffer waits for the next request of about its size.
// ------------------------------------------------------------------------------------------------
namespace {
struct HostPool {
    std::mutex mu;
    struct Buf { void *p; size_t cap; };
    std::vector<Buf> free_list;            // oldest first
    std::vector<Buf> live;                 // handed out
    size_t pooled = 0, out = 0;
    static constexpr size_t kMaxPooled = (size_t)1 << 30, kMaxOut = (size_t)4 << 30;
};
HostPool g_host_pool;
bool g_host_pool_exiting = false;  // process exit: buffers are left to the system (the HIP runtime may be gone already)
}  // namespace

// bytes of page-locked host memory (usable from every device).  SPIHT_ERR_NOMEM when the allocation fails or more than
// 4 GiB are handed out already: the caller then takes ordinary memory (the calls accept any host pointer).
extern "C" int spiht_host_alloc(uint64_t bytes, void **h_ptr) {
    if (!h_ptr || bytes == 0) return SPIHT_ERR_ARG;
    *h_ptr = nullptr;
    HostPool &hp = g_host_pool;
    static const int registered = atexit([] { g_host_pool_exiting = true; });
    (void)registered;
    std::lock_guard<std::mutex> lk(hp.mu);
    if (hp.out + bytes > HostPool::kMaxOut) return SPIHT_ERR_NOMEM;
    int best = -1;
    for (size_t i = 0; i < hp.free_list.size(); i++)
        if (hp.free_list[i].cap >= bytes && hp.free_list[i].cap <= bytes + bytes / 4 + 4096 &&
            (best < 0 || hp.free_list[i].cap < hp.free_list[(size_t)best].cap)) best = (int)i;
    HostPool::Buf b;
    if (best >= 0) {
        b = hp.free_list[(size_t)best];
        hp.free_list.erase(hp.free_list.begin() + best);
        hp.pooled -= b.cap;
    } else {
        b.cap = (size_t)bytes;
        if (hipHostMalloc(&b.p, b.cap, hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            // (room may be what is missing: the pool gives its buffers back and the request is tried once more)
            for (auto &f : hp.free_list) (void)hipHostFree(f.p);
            hp.free_list.clear();
            hp.pooled = 0;
            if (hipHostMalloc(&b.p, b.cap, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return SPIHT_ERR_NOMEM; }
        }
    }
    hp.live.push_back(b);
    hp.out += b.cap;
    *h_ptr = b.p;
    return SPIHT_OK;
}
extern "C" int spiht_host_free(void *h_ptr) {
    if (!h_ptr) return SPIHT_OK;
    HostPool &hp = g_host_pool;
    std::lock_guard<std::mutex> lk(hp.mu);
    for (size_t i = 0; i < hp.live.size(); i++) {
        if (hp.live[i].p != h_ptr) continue;
        const HostPool::Buf b = hp.live[i];
        hp.live.erase(hp.live.begin() + (long)i);
        hp.out -= b.cap;
        hp.free_list.push_back(b);
        hp.pooled += b.cap;
        while (!g_host_pool_exiting && (hp.pooled > HostPool::kMaxPooled || hp.free_list.size() > 8)) {  // the oldest goes back to the system
            (void)hipHostFree(hp.free_list.front().p);
            hp.pooled -= hp.free_list.front().cap;
            hp.free_list.erase(hp.free_list.begin());
        }
        return SPIHT_OK;
    }
    return SPIHT_ERR_ARG;  // not one of ours
}

// ------------------------------------------------------------------------------------------------
// device memory helpers
// ------------------------------------------------------------------------------------------------
extern "C" int spiht_dev_alloc(spiht_ctx *ctx, uint64_t bytes, void **d_ptr) {
    if (!ctx || !d_ptr) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 4);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return SPIHT_ERR_NOMEM;
    }
    return SPIHT_OK;
}
extern "C" int spiht_dev_free(spiht_ctx *ctx, void *d_ptr) {
    if (!ctx) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        forget_pads(ctx, d_ptr);
    }
    HIPCHK(hipFree(d_ptr));
    return SPIHT_OK;
}
extern "C" int spiht_dev_upload(spiht_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes) {
    if (!ctx || (!d_dst && bytes) || (!h_src && bytes)) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_dev_download(spiht_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes) {
    if (!ctx || (!h_dst && bytes) || (!d_src && bytes)) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_dev_copy(spiht_ctx *ctx, void *d_dst, const void *d_src, uint64_t bytes) {
    if (!ctx || (!d_dst && bytes) || (!d_src && bytes)) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_dev_memset(spiht_ctx *ctx, void *d_dst, int value, uint64_t bytes) {
    if (!ctx || (!d_dst && bytes)) return SPIHT_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemsetAsync(d_dst, value, bytes, ctx->stream));
    return SPIHT_OK;
}
