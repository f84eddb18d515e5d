// Host-fed streams behind the C ABI (include/spiht_hip.h: spiht_hstream_*): batches of host pictures encoded, or batches of
// host streams decoded, with the transfers overlapped.  The coding is the batched call of api_image.cpp with the stream's element
// on the caller's context; what is new here is the schedule over three queues -- copies in, the context's stream, copies out --
// ordered with events, and a ring of slots (hstream_ring.h) whose staging is page-locked on both sides:
//
//     copy-in :  U(i+1)                      U(i+2)
//     context :  [U(i) done]  C(i)  P(i)     [U(i+1) done]  C(i+1)  P(i+1)
//     copy-out:  D(i-1)                      D(i)
//
// U = upload of a step's input, C = the batched encode (decode: spiht_tile_unpack, then the batched decode), P = spiht_tile_pack
// and the download of the n lengths and start planes (encode only, on the context's stream), D = download: decode, of the
// pictures, queued at the submit behind a wait for C(i); encode, of exactly the packed bytes, queued by spiht_hstream_next once
// it has seen P(i) done and knows the lengths -- with no wait in front of it, so that it never stands behind a later step.  The host never waits except in _next and _destroy, and there
// by polling an event for a bounded time.  A slot's buffers are reused only after its result was taken, i.e. after every
// queue is through with them: no event is needed for the reuse.  The two copy streams are the context's (api_internal.h): every
// host-fed stream on a context shares them, so that a context never has more than three HIP streams.
// The reference codes one host picture per call (spiht_wrapper.py:142-216); this replaces a loop over such calls.
#include "api_internal.h"
#include "hstream_ring.h"

#include <time.h>

#include <chrono>
#include <new>

struct HsSlot {
    // page-locked staging (spiht_host_alloc)
    char *h_in = nullptr;    // encoder: pictures.  decoder: packed bytes | lens | max_n
    char *h_out = nullptr;   // encoder: packed bytes | lens | max_n.  decoder: pictures
    // device
    char *d_pic = nullptr;       // the step's pictures (in or out)
    uint8_t *d_slots = nullptr;  // B stream slots
    uint8_t *d_packed = nullptr; // the streams as one run
    uint32_t *d_lens = nullptr;
    uint64_t *d_n64 = nullptr;   // encoder: nbits.  decoder: nbytes
    uint8_t *d_maxn = nullptr;
    hipEvent_t ev_up = nullptr, ev_done = nullptr, ev_out = nullptr, ev_bytes = nullptr;
    // the step it holds
    int64_t n = 0;
    bool bytes_queued = false;  // encoder: _next has queued the download of the packed bytes
    uint64_t total = 0;         // ... and their number
    bool to_device = false;     // decoder: the pictures went to the caller's device destination
    hipEvent_t last = nullptr;  // the event behind everything queued for the step so far
};

struct spiht_hstream {
    spiht_ctx *ctx = nullptr;
    int dir = SPIHT_HS_ENCODE;
    PicElem el = EL_F64;  // the staged pictures' element (el_of_hs of _create's elem)
    int64_t B = 0, c = 0, H = 0, W = 0;
    int wavelet = 0, mode = 0, level = -1;
    double q = 1.0;
    std::vector<double> mults;
    uint64_t max_bits = 0;
    uint64_t slot_bytes = 0;     // stream slot per picture (a multiple of 4)
    bool strided = false;
    int64_t st[4] = {0, 0, 0, 0};  // byte strides of the staged pictures, the dense ones included
    int64_t pic_h = 0, pic_w = 0;  // the staged pictures' size: H x W, a float64 decoder's rec_H x rec_W
    uint64_t pic_bytes = 0;        // what B of them span
    hipStream_t s_in = nullptr, s_out = nullptr;
    HsRing ring;
    HsSlot slot[HsRing::MAX_DEPTH];
    int poisoned = SPIHT_OK;
    bool counted = false;  // among the users of the context's copy streams
    const double *mp() const { return mults.empty() ? nullptr : mults.data(); }
    const int64_t *strides() const { return strided ? st : nullptr; }
    uint64_t span(int64_t n) const {  // bytes from the first sample of n staged pictures to one past the last
        return (uint64_t)el_size(el) + (uint64_t)(n - 1) * st[0] + (uint64_t)(c - 1) * st[1] + (uint64_t)(pic_h - 1) * st[2] +
               (uint64_t)(pic_w - 1) * st[3];
    }
    // the parts of a slot's stream staging: packed bytes | lens (uint32 [B]) | max_n (uint8 [B])
    uint64_t off_lens() const { return (uint64_t)B * slot_bytes; }
    uint64_t off_maxn() const { return off_lens() + (uint64_t)B * 4; }
    uint64_t stream_staging() const { return off_maxn() + (uint64_t)B; }
};

#pragma GCC visibility push(hidden)

namespace {

// a HIP call that fails latches: the stream's state is void from there on
#define HS_HIP(s, expr)                                                        \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) {                                                \
            g_hip_err = std::string(#expr) + ": " + hipGetErrorString(_e);     \
            (s)->poisoned = SPIHT_ERR_HIP;                                     \
            return SPIHT_ERR_HIP;                                              \
        }                                                                      \
    } while (0)
#define HS_CHK(s, expr)                                                        \
    do {                                                                       \
        int _s = (expr);                                                       \
        if (_s != SPIHT_OK) {                                                  \
            (s)->poisoned = _s;                                                \
            return _s;                                                         \
        }                                                                      \
    } while (0)

typedef std::chrono::steady_clock hs_clock;

// Polls ev until it has been reached or `deadline` has passed: SPIHT_OK, SPIHT_ERR_TIMEOUT, or SPIHT_ERR_HIP.  At least one look.
int poll_event(hipEvent_t ev, hs_clock::time_point deadline) {
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return SPIHT_OK;
        if (e != hipErrorNotReady) {
            g_hip_err = std::string("hipEventQuery: ") + hipGetErrorString(e);
            return SPIHT_ERR_HIP;
        }
        (void)hipGetLastError();
        if (hs_clock::now() >= deadline) return SPIHT_ERR_TIMEOUT;
        struct timespec ts = {0, 50 * 1000};  // 50 us: far below a step, far above the cost of a query
        (void)nanosleep(&ts, nullptr);
    }
}

void free_slot_buffers(HsSlot &k) {
    if (k.h_in) (void)spiht_host_free(k.h_in);
    if (k.h_out) (void)spiht_host_free(k.h_out);
    void *dev[] = {k.d_pic, k.d_slots, k.d_packed, k.d_lens, k.d_n64, k.d_maxn};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    k.h_in = k.h_out = k.d_pic = nullptr;
    k.d_slots = k.d_packed = k.d_maxn = nullptr;
    k.d_lens = nullptr;
    k.d_n64 = nullptr;
}

// the events and the buffers (with abandon: the buffers stay with the process, a transfer may still be using them)
int hstream_free(spiht_hstream *s, bool abandon_buffers) {
    if (!s) return SPIHT_OK;
    if (s->ctx) (void)hipSetDevice(s->ctx->device);
    for (int i = 0; i < HsRing::MAX_DEPTH; i++) {
        HsSlot &k = s->slot[i];
        if (!abandon_buffers) free_slot_buffers(k);
        hipEvent_t evs[] = {k.ev_up, k.ev_done, k.ev_out, k.ev_bytes};
        for (hipEvent_t e : evs)
            if (e) (void)hipEventDestroy(e);
    }
    // the copy streams go with the context's last host-fed stream (work still queued on them: the runtime destroys them behind it)
    if (s->ctx && s->counted) {
        std::lock_guard<std::recursive_mutex> lk(s->ctx->mu);
        if (--s->ctx->copy_users == 0) {
            if (s->ctx->copy_in) (void)hipStreamDestroy(s->ctx->copy_in);
            if (s->ctx->copy_out) (void)hipStreamDestroy(s->ctx->copy_out);
            s->ctx->copy_in = s->ctx->copy_out = nullptr;
        }
    }
    delete s;
    return SPIHT_OK;
}

int dev_alloc(void **p, uint64_t bytes) {
    hipError_t e = hipMalloc(p, bytes ? bytes : 4);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e);
        *p = nullptr;
        return SPIHT_ERR_NOMEM;
    }
    return SPIHT_OK;
}

int alloc_slot(spiht_hstream *s, HsSlot &k) {
    const bool enc = s->dir == SPIHT_HS_ENCODE;
    CHK(spiht_host_alloc(enc ? s->pic_bytes : s->stream_staging(), (void **)&k.h_in));
    CHK(spiht_host_alloc(enc ? s->stream_staging() : s->pic_bytes, (void **)&k.h_out));
    CHK(dev_alloc((void **)&k.d_pic, s->pic_bytes));
    CHK(dev_alloc((void **)&k.d_slots, (uint64_t)s->B * s->slot_bytes));
    CHK(dev_alloc((void **)&k.d_packed, (uint64_t)s->B * s->slot_bytes));
    CHK(dev_alloc((void **)&k.d_lens, (uint64_t)s->B * 4));
    CHK(dev_alloc((void **)&k.d_n64, (uint64_t)s->B * 8));
    CHK(dev_alloc((void **)&k.d_maxn, (uint64_t)s->B));
    hipEvent_t *evs[] = {&k.ev_up, &k.ev_done, &k.ev_out, &k.ev_bytes};
    for (hipEvent_t *e : evs) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return SPIHT_OK;
}

// the batched encode: n pictures at d_pic (float64: a dense array; else a view) -> slots, bit counts, start planes
int queue_encode(spiht_hstream *s, HsSlot &k) {
    if (s->el == EL_F64)
        return encode_image_batch(s->ctx, dense_pic(k.d_pic, EL_F64), k.n, s->c, s->H, s->W, s->wavelet, s->mode, s->level, s->q,
                                  s->mp(), s->max_bits, k.d_slots, s->slot_bytes, k.d_n64, k.d_maxn, nullptr);
    return encode_image_batch_view(s->el, s->ctx, k.d_pic, s->strides(), k.n, s->c, s->H, s->W, s->wavelet, s->mode, s->level, s->q,
                                   s->mp(), s->max_bits, k.d_slots, s->slot_bytes, k.d_n64, k.d_maxn, nullptr);
}

// the batched decode of the stream's element: n slots of `stride` bytes -> pictures at d_dst
int queue_decode(spiht_hstream *s, HsSlot &k, uint64_t stride, void *d_dst) {
    if (s->el == EL_F64)
        return decode_image_batch(s->ctx, k.d_slots, stride, k.d_n64, k.d_maxn, k.n, s->c, s->H, s->W, s->wavelet, s->mode, s->level,
                                  s->q, s->mp(), dense_pic(d_dst, EL_F64, true), nullptr);
    return decode_image_batch_view(s->el, s->ctx, k.d_slots, stride, k.d_n64, k.d_maxn, k.n, s->c, s->H, s->W, s->wavelet, s->mode,
                                   s->level, s->q, s->mp(), d_dst, s->strides(), nullptr);
}

int submit_encode(spiht_hstream *s, HsSlot &k) {
    spiht_ctx *ctx = s->ctx;
    HS_HIP(s, hipMemcpyAsync(k.d_pic, k.h_in, s->span(k.n), hipMemcpyHostToDevice, s->s_in));
    HS_HIP(s, hipEventRecord(k.ev_up, s->s_in));
    {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);  // the wait, the coding and the event stand together in the context's queue
        HS_HIP(s, hipStreamWaitEvent(ctx->stream, k.ev_up, 0));
        HS_CHK(s, queue_encode(s, k));
        HS_CHK(s, spiht_tile_pack(ctx, k.d_slots, s->slot_bytes, k.d_n64, k.n, k.d_packed, (uint64_t)s->B * s->slot_bytes, k.d_lens));
        // The lengths and start planes come down on the context's stream, right behind the pack: a few bytes.  Nothing of an
        // encode step is queued on the copy-out stream here.  That stream is in order: a wait for THIS step's event on it would
        // stand in front of the packed bytes of every EARLIER step, which _next queues there later -- _next(i) would then return
        // only when every step in flight had been coded, and the ring would drain on every call.
        HS_HIP(s, hipMemcpyAsync(k.h_out + s->off_lens(), k.d_lens, (size_t)k.n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HS_HIP(s, hipMemcpyAsync(k.h_out + s->off_maxn(), k.d_maxn, (size_t)k.n, hipMemcpyDeviceToHost, ctx->stream));
        HS_HIP(s, hipEventRecord(k.ev_done, ctx->stream));
    }
    k.last = k.ev_done;
    return SPIHT_OK;
}

int submit_decode(spiht_hstream *s, HsSlot &k, void *d_dst) {
    spiht_ctx *ctx = s->ctx;
    const uint32_t *lens = (const uint32_t *)(k.h_in + s->off_lens());
    uint64_t total = 0, longest = 0;
    for (int64_t b = 0; b < k.n; b++) {  // (refused before anything is queued: the stream stays as it was)
        if (lens[b] > s->slot_bytes) return SPIHT_ERR_ARG;
        total += lens[b];
        longest = std::max<uint64_t>(longest, lens[b]);
    }
    const uint64_t stride = std::max<uint64_t>(4, (longest + 3) & ~(uint64_t)3);  // <= slot_bytes, itself a multiple of 4
    if (total) HS_HIP(s, hipMemcpyAsync(k.d_packed, k.h_in, total, hipMemcpyHostToDevice, s->s_in));
    HS_HIP(s, hipMemcpyAsync(k.d_lens, k.h_in + s->off_lens(), (size_t)k.n * 4, hipMemcpyHostToDevice, s->s_in));
    HS_HIP(s, hipMemcpyAsync(k.d_maxn, k.h_in + s->off_maxn(), (size_t)k.n, hipMemcpyHostToDevice, s->s_in));
    HS_HIP(s, hipEventRecord(k.ev_up, s->s_in));
    {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        HS_HIP(s, hipStreamWaitEvent(ctx->stream, k.ev_up, 0));
        HS_CHK(s, spiht_tile_unpack(ctx, k.d_packed, total, k.d_lens, k.n, k.d_slots, stride, k.d_n64));
        HS_CHK(s, queue_decode(s, k, stride, d_dst ? d_dst : k.d_pic));
        HS_HIP(s, hipEventRecord(k.ev_done, ctx->stream));
    }
    k.to_device = d_dst != nullptr;
    k.last = k.ev_done;
    if (!d_dst) {
        HS_HIP(s, hipStreamWaitEvent(s->s_out, k.ev_done, 0));
        HS_HIP(s, hipMemcpyAsync(k.h_out, k.d_pic, s->span(k.n), hipMemcpyDeviceToHost, s->s_out));
        HS_HIP(s, hipEventRecord(k.ev_out, s->s_out));
        k.last = k.ev_out;
    }
    return SPIHT_OK;
}

}  // namespace

#pragma GCC visibility pop

extern "C" int spiht_hstream_create(spiht_ctx *ctx, int direction, int elem, int64_t B, int depth, int64_t c, int64_t H, int64_t W,
                                    int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                    uint64_t max_bits, const int64_t *strides, spiht_hstream **out) {
    if (!out) return SPIHT_ERR_ARG;
    *out = nullptr;
    if (!ctx || (direction != SPIHT_HS_ENCODE && direction != SPIHT_HS_DECODE) || elem < SPIHT_HS_F64 ||
        elem > SPIHT_HS_BF16 || !HsRing::depth_ok(depth) || B < 1 || c < 1 || H < 1 || W < 1)
        return SPIHT_ERR_ARG;
    if (c > 65535 || B > 65535) return SPIHT_ERR_TOO_LARGE;
    if (elem == SPIHT_HS_F64 && strides) return SPIHT_ERR_ARG;
    spiht_hstream *s = new (std::nothrow) spiht_hstream();
    if (!s) return SPIHT_ERR_NOMEM;
    s->ctx = ctx;
    s->dir = direction; s->el = el_of_hs(elem);
    s->B = B; s->c = c; s->H = H; s->W = W;
    s->wavelet = wavelet; s->mode = mode; s->level = level; s->q = q_scale;
    if (channel_mults) s->mults.assign(channel_mults, channel_mults + c);
    s->max_bits = max_bits;
    s->ring = HsRing(depth);
    int64_t ll_h = 0, ll_w = 0, enc_h = 0, enc_w = 0, rec_H = 0, rec_W = 0;
    int st = spiht_geometry_mode(H, W, wavelet, mode, level, nullptr, &ll_h, &ll_w, &enc_h, &enc_w, &rec_H, &rec_W);
    if (st == SPIHT_OK)
        st = spiht_encode_bound(c, enc_h, enc_w, ll_h, ll_w, 0x3FFFFFFFu, max_bits == SPIHT_MAX_BITS_UNLIMITED ? 0 : max_bits, &s->slot_bytes);
    if (st == SPIHT_OK && s->el != EL_F64 && strides) st = check_view(s->el, B, c, H, W, strides, direction == SPIHT_HS_DECODE);
    if (st != SPIHT_OK) { delete s; return st; }
    s->slot_bytes = std::max<uint64_t>(4, (s->slot_bytes + 3) & ~(uint64_t)3);
    if (s->slot_bytes > ((uint64_t)1 << 29)) { delete s; return SPIHT_ERR_TOO_LARGE; }  // (spiht_tile_pack's limit)
    const bool rec = direction == SPIHT_HS_DECODE && s->el == EL_F64;
    s->pic_h = rec ? rec_H : H;
    s->pic_w = rec ? rec_W : W;
    s->strided = strides != nullptr;
    if (strides) memcpy(s->st, strides, sizeof(s->st));
    else { s->st[3] = el_size(s->el); s->st[2] = s->pic_w * s->st[3]; s->st[1] = s->pic_h * s->st[2]; s->st[0] = c * s->st[1]; }
    s->pic_bytes = s->span(B);
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    // the two copy streams are the context's: shared by every host-fed stream on it, gone with the last of them
    ctx->copy_users++;
    s->counted = true;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess && !ctx->copy_in) e = hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking);
    if (e == hipSuccess && !ctx->copy_out) e = hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking);
    s->s_in = ctx->copy_in;
    s->s_out = ctx->copy_out;
    if (e != hipSuccess) {
        g_hip_err = std::string("hipStreamCreate: ") + hipGetErrorString(e);
        (void)hstream_free(s, false);
        return SPIHT_ERR_HIP;
    }
    for (int i = 0; i < depth; i++)
        if ((st = alloc_slot(s, s->slot[i])) != SPIHT_OK) {  // (the pool refuses, or the device is full: nothing stays allocated)
            (void)hstream_free(s, false);
            return st;
        }
    *out = s;
    return SPIHT_OK;
}

extern "C" int spiht_hstream_destroy(spiht_hstream *s) {
    if (!s) return SPIHT_OK;
    (void)hipSetDevice(s->ctx->device);
    // what is queued: the last event of every submitted step, oldest first, all within one bound
    const hs_clock::time_point deadline = hs_clock::now() + std::chrono::milliseconds(SPIHT_HS_DESTROY_MS);
    int st = SPIHT_OK;
    for (uint64_t t = s->ring.taken; t < s->ring.issued && st == SPIHT_OK; t++) {
        HsSlot &k = s->slot[t % (uint64_t)s->ring.depth];
        if (k.last) st = poll_event(k.last, deadline);
    }
    (void)hstream_free(s, st != SPIHT_OK || s->poisoned != SPIHT_OK);
    return st == SPIHT_OK ? SPIHT_OK : SPIHT_ERR_TIMEOUT;
}

extern "C" int spiht_hstream_info(spiht_hstream *s, uint64_t *slot_bytes, uint64_t *pic_bytes, int64_t *rec_H, int64_t *rec_W) {
    if (!s) return SPIHT_ERR_ARG;
    if (slot_bytes) *slot_bytes = s->slot_bytes;
    if (pic_bytes) *pic_bytes = s->pic_bytes;
    if (rec_H) *rec_H = s->pic_h;
    if (rec_W) *rec_W = s->pic_w;
    return SPIHT_OK;
}

extern "C" int spiht_hstream_pending(spiht_hstream *s, int *steps) {
    if (!s || !steps) return SPIHT_ERR_ARG;
    *steps = s->ring.in_flight();
    return SPIHT_OK;
}

extern "C" int spiht_hstream_input(spiht_hstream *s, void **h_ptr) {
    if (!s || !h_ptr) return SPIHT_ERR_ARG;
    if (s->poisoned != SPIHT_OK) return s->poisoned;
    const int i = s->ring.acquire();
    if (i < 0) return SPIHT_ERR_BUSY;
    *h_ptr = s->slot[i].h_in;
    return SPIHT_OK;
}

extern "C" int spiht_hstream_decode_input(spiht_hstream *s, uint8_t **h_packed, uint32_t **h_lens, uint8_t **h_max_n) {
    if (!s || s->dir != SPIHT_HS_DECODE) return SPIHT_ERR_ARG;
    void *p = nullptr;
    CHK(spiht_hstream_input(s, &p));
    if (h_packed) *h_packed = (uint8_t *)p;
    if (h_lens) *h_lens = (uint32_t *)((char *)p + s->off_lens());
    if (h_max_n) *h_max_n = (uint8_t *)p + s->off_maxn();
    return SPIHT_OK;
}

extern "C" int spiht_hstream_submit(spiht_hstream *s, int64_t n, void *d_dst) {
    if (!s) return SPIHT_ERR_ARG;
    if (s->poisoned != SPIHT_OK) return s->poisoned;
    const int i = s->ring.handed_slot();
    if (i < 0) return s->ring.full() ? SPIHT_ERR_BUSY : SPIHT_ERR_ARG;
    if (n < 1 || n > s->B || (d_dst && s->dir == SPIHT_HS_ENCODE) || (d_dst && (uintptr_t)d_dst % (uintptr_t)el_size(s->el)))
        return SPIHT_ERR_ARG;
    HsSlot &k = s->slot[i];
    k.n = n;
    k.bytes_queued = false;
    k.total = 0;
    k.to_device = false;
    k.last = nullptr;
    if (hipSetDevice(s->ctx->device) != hipSuccess) { s->poisoned = SPIHT_ERR_HIP; g_hip_err = "hipSetDevice"; return SPIHT_ERR_HIP; }
    // (a HIP call that fails half-way latches; part of the step may be queued then, with no event to wait for: _destroy leaves
    // the buffers of a latched stream to the process, as it does when its time runs out)
    CHK(s->dir == SPIHT_HS_ENCODE ? submit_encode(s, k) : submit_decode(s, k, d_dst));
    (void)s->ring.submit();
    return SPIHT_OK;
}

extern "C" int spiht_hstream_next(spiht_hstream *s, int timeout_ms, spiht_hstream_result *out) {
    if (!s || !out || timeout_ms < 0) return SPIHT_ERR_ARG;
    if (s->poisoned != SPIHT_OK) return s->poisoned;
    const int i = s->ring.oldest();
    if (i < 0) return SPIHT_ERR_IDLE;
    HsSlot &k = s->slot[i];
    const hs_clock::time_point deadline = hs_clock::now() + std::chrono::milliseconds(timeout_ms);
    HS_HIP(s, hipSetDevice(s->ctx->device));
    int st;
    if (s->dir == SPIHT_HS_ENCODE && !k.bytes_queued) {
        // the lengths first; then exactly the bytes they add up to, on the copy-out stream -- the pack is through, so the copy needs
        // no wait in front of it and runs beside the coding of the steps behind
        st = poll_event(k.ev_done, deadline);
        if (st == SPIHT_ERR_TIMEOUT) return st;
        HS_CHK(s, st);
        const uint32_t *lens = (const uint32_t *)(k.h_out + s->off_lens());
        uint64_t total = 0;
        for (int64_t b = 0; b < k.n; b++) total += lens[b];
        if (total > (uint64_t)s->B * s->slot_bytes) { s->poisoned = SPIHT_ERR_INTERNAL; return SPIHT_ERR_INTERNAL; }
        if (total) HS_HIP(s, hipMemcpyAsync(k.h_out, k.d_packed, total, hipMemcpyDeviceToHost, s->s_out));
        HS_HIP(s, hipEventRecord(k.ev_bytes, s->s_out));
        k.total = total;
        k.bytes_queued = true;
        k.last = k.ev_bytes;
    }
    st = poll_event(k.last, deadline);
    if (st == SPIHT_ERR_TIMEOUT) return st;
    HS_CHK(s, st);
    memset(out, 0, sizeof(*out));
    out->n = k.n;
    out->step = s->ring.taken;
    if (s->dir == SPIHT_HS_ENCODE) {
        out->nbytes = k.total;
        out->bytes = (const uint8_t *)k.h_out;
        out->lens = (const uint32_t *)(k.h_out + s->off_lens());
        out->max_n = (const uint8_t *)k.h_out + s->off_maxn();
    } else {
        out->nbytes = s->span(k.n);
        out->pictures = k.to_device ? nullptr : (void *)k.h_out;
    }
    (void)s->ring.take();
    return SPIHT_OK;
}
