// What the files of the host side (api_*.cpp and hoststream.cpp: the C ABI of libspiht_hip.so, include/spiht_hip.h) share: the
// status macros, the context and its scratch, the geometry and the pictures of an image call, and the helpers that cross files.
// Nothing declared here is exported: the whole header has hidden visibility.
#pragma once
#include "../../include/spiht_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "alloc.h"
#include "common.h"
#include "floatpx.h"
#include "rd.h"
#include "tiles.h"
#include "tileset.h"

#pragma GCC visibility push(hidden)

extern thread_local std::string g_hip_err;  // what spiht_last_hip_error() reports: one per thread, whichever file set it (api_ctx.cpp)

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            g_hip_err = std::string(#expr) + ": " + hipGetErrorString(_e);                 \
            return SPIHT_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)
#define LAUNCHCHK(expr)                                                                    \
    do {                                                                                   \
        int _e = (expr);                                                                   \
        if (_e != 0) {                                                                     \
            g_hip_err = std::string(#expr) + ": launch error " + std::to_string(_e);       \
            return SPIHT_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)
#define CHK(expr)                      \
    do {                               \
        int _s = (expr);               \
        if (_s != SPIHT_OK) return _s; \
    } while (0)

enum Stage {
    ST_H2D = 0, ST_D2H, ST_ABSMAX, ST_PYRAMID, ST_ENC_LISTS, ST_DEC_LISTS, ST_DWT_L1, ST_DWT_REST, ST_IDWT_REST,
    ST_IDWT_L1, ST_MEMSET, ST_GATHER, ST_COUNT
};

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct spiht_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::recursive_mutex mu;  // recursive: the host-array entry points call the batched ones
    // host-fed streams (hoststream.cpp): the copy-in and the copy-out stream beside `stream`, made for the first spiht_hstream of
    // the context, shared by all of them and given back with the last -- three HIP streams per context however many host-fed
    // streams it carries, and one when it carries none
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    int copy_users = 0;
    int num_cu = 256;
    float log2_thresh[32];
    // grow-only scratch
    DevBuf x, dmsb, lmsb, maxabs, out, nbits, maxn, err, lists, coeffs, a0, a1, data, nbytes, rec, mults, img;
    DevBuf trace, meta;  // decode_with_metadata
    DevBuf tilebuf;      // tile counters of the persistent inverse-transform kernel
    TileCtr tilectr = {nullptr, {0, 0, 0, 0, 0, 0, 0, 0}, 0, 0, 0, 0};
    DevBuf himg, hrec;   // host-array image entry points: pixels in / out, coefficient array in
    DevBuf pix;          // 8- / 16-bit pixels: the dense float64 picture of the routes that convert in a pass of their own
    DevBuf hpix8;        // 8- / 16-bit host-array entry points: the picture's bytes on the device
    std::vector<double> mults_host;  // what ctx->mults holds (uploaded again only when the scales change)
    // colour model of the coded picture (spiht_ctx_set_color3): applied inside level 1 of the transforms of 3-channel images
    bool color_on = false;
    Color3 col_fwd, col_inv;
    int dec_waves = 12;  // wavefronts per decoder workgroup (spiht_ctx_set_decoder_waves)
    // spiht_ctx_set_option
    bool opt_l1_flags = true;   // the decoder flags the occupied level-1 tiles for the inverse transform
    bool opt_pads_persist = false;  // coefficient arrays this context has filled keep their zero padding (see dwt_forward)
    struct PadKey { const void *p; int planes; int64_t H, W; int F, L, mode; };
    std::vector<PadKey> pads_zeroed;  // arrays whose padding strips this context has zeroed (opt_pads_persist)
    DevBuf l1flags;             // L1Flags words of the fused decode path
    DevBuf exttmp;              // intermediates of the two-pass forward level (extension modes that compute their samples)
    DevBuf widebuf;             // control blocks and scan descriptors of the several-CUs-per-image encoder (encode_wide.hip)
    int opt_wide_solo = 24576;  // list entries up to which a plane stays with workgroup 0 (4 k ... 64 k measured the same)
    int opt_wide_g = 0;         // workgroups per image of that encoder (0: by the size of the image)
    int opt_wide_encode = 1;    // few images per call: one image on several CUs (2: whatever the image's size -- tests)
    int64_t opt_meta_chunk = 0; // batched decode_with_metadata: images per chunk at most (0: by the scratch bound)
    int wide_per_cu = -1;       // workgroups of k_encode_wide a CU holds (occupancy query, once; 0: unknown -> one)
    std::vector<WideCtl> wide_forced;  // opt_wide_encode == 3 (tests): control blocks that say "gave up" before the launch
    int wide_last_groups = 0;   // groups of the last several-CUs-per-image launch (spiht_ctx_wide_stats)
    DevBuf filt;                // the filters of wavelet `filt_wavelet` on the device, for the two-pass levels (any length)
    int filt_wavelet = -1;
    // decoder output of the fused image path: kept all-zero between calls (k_unscatter), so no per-call zero-fill
    DevBuf recz, lspcnt;
    DevBuf rdpart;              // per-workgroup partial sums of the rate-distortion reductions (rd.hip)
    DevBuf tilescr;             // tiled pictures (tiles.hip): byte lengths and offsets of the streams pack / unpack move
    DevBuf allocscr;            // rate allocation across tiles (alloc.hip): the tiles' hulls
    DevBuf layerscr;            // quality layers (layers.hip): the pieces' offsets in the run, the table's running maximum
    DevBuf tsettab;             // picture sets (tileset.hip): the tables of the call queued last; the next call's copy is behind its kernel
    std::vector<TableStage> tstages;  // ... and the page-locked stages the tables are copied from, one per call in flight
    bool recz_clean = false;
    // spiht_decode_lists_batch_i32 -> spiht_unscatter_lists_batch_i32: the launch whose scatter can still be undone
    DecArgs last_dec;
    bool last_dec_valid = false;
    // timing
    bool timing = false;
    struct Rec { int stage; hipEvent_t a, b; };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    double ms[ST_COUNT];
    uint64_t launches[ST_COUNT];
};

// ---- api_ctx.cpp -----------------------------------------------------------------------------------------------------------
int ensure(spiht_ctx *ctx, DevBuf &b, size_t bytes);  // grows b to at least `bytes` (waits for the stream when it must free)
int take_err(spiht_ctx *ctx);                          // the latched device-side error: waits, reports it once, clears it

struct StageTimer {
    spiht_ctx *ctx;
    int stage;
    hipEvent_t a = nullptr, b = nullptr;
    StageTimer(spiht_ctx *c, int s) : ctx(c), stage(s) {
        if (!ctx->timing) return;
        auto get = [&]() {
            hipEvent_t e = nullptr;
            if (!ctx->pool.empty()) { e = ctx->pool.back(); ctx->pool.pop_back(); }
            else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
            return e;
        };
        a = get();
        b = get();
        if (a) (void)hipEventRecord(a, ctx->stream);
    }
    ~StageTimer() {
        if (!ctx->timing || !a || !b) return;
        (void)hipEventRecord(b, ctx->stream);
        ctx->pending.push_back({stage, a, b});
    }
};

// ---- api_coder.cpp: the list coder on device-resident arrays; everything queues work on ctx->stream ---------------------------
int make_geom(int64_t c, int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, Geom *g);
uint64_t bound_bits(const Geom &g, uint32_t max_abs);
// Encode B device-resident coefficient arrays.  max_bits already validated.
int encode_device(spiht_ctx *ctx, const Geom &g, const int32_t *d_x, int B, uint64_t max_bits_in, uint8_t *d_out,
                  uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_maxn, bool have_maxabs = false);
int decode_device(spiht_ctx *ctx, const Geom &g, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                  const uint8_t *d_maxn, int B, int32_t *d_out, uint32_t *d_tr_ent = nullptr, uint8_t *d_tr_act = nullptr,
                  uint64_t tr_stride = 0, bool zero_out = true, DecArgs *args_out = nullptr, const L1Flags *fl = nullptr);
// The result of a single encode (ctx->out, ctx->nbits, ctx->maxn) to the host; waits
int read_encoded(spiht_ctx *ctx, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n);
// One host stream for the decoder: its bytes into ctx->data, a slot of *slot bytes whose last word is zeroed first (the
// bytes past the stream in it), its length and magnitude into ctx->nbytes / ctx->maxn; waits, and returns the error an
// earlier batched call has latched, if any (take_err)
int stage_stream(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, uint64_t *slot);

// fn(b0, nb) over a batch of B images of c planes, in chunks of at most 65535 planes (a launch's grid.y / slot limit)
template <class Fn> static int batch_chunks(int64_t B, int64_t c, Fn fn) {
    const int chunk = (int)std::max<int64_t>(1, 65535 / c);
    for (int64_t b0 = 0; b0 < B; b0 += chunk) CHK(fn(b0, (int)std::min<int64_t>(chunk, B - b0)));
    return SPIHT_OK;
}

// ---- api_dwt.cpp: the geometry of an image, the pictures of a call, the two transform drivers ---------------------------------
struct ImgGeom {
    int L;
    int64_t hs[SPIHT_MAX_LEVELS + 1], ws[SPIHT_MAX_LEVELS + 1];      // band sizes, [0] = image
    int64_t offh[SPIHT_MAX_LEVELS + 1], offw[SPIHT_MAX_LEVELS + 1];  // detail block offsets per level
    int64_t ll_h, ll_w, enc_h, enc_w, rec_H, rec_W;
    bool per;  // periodization: ceil(n / 2) coefficients per level and 2 n samples back (the rule below with a two-tap filter)
    int l0;    // levels dropped below level 1 of this geometry (reduced_geometry; 0: level 1 is the picture's own)
};
int img_geometry(int64_t H, int64_t W, int F_real, int level, ImgGeom *g, int mode = SPIHT_MODE_REFLECT);
// ... of a stream (ig) and of its picture at 1/2^reduce size (pig); refuses a reduce outside 0 .. L
int reduced_open(int64_t H, int64_t W, int wavelet, int mode, int level, int reduce, ImgGeom *ig, ImgGeom *pig);
// Geometry of the L1Flags words of an image geometry (common.h): false when they do not apply
bool l1flags_geometry(const ImgGeom &ig, int F, L1Flags *fl);
int check_img_args(int wavelet, int mode, int64_t B, int64_t c, int64_t H, int64_t W);

// ---- the pictures of an image call -------------------------------------------------------------------------------------------
// The element of a picture, said once.  Float64 and float32 pictures are transformed in their own precision (EL_F32: the
// single-precision transform).  8- and 16-bit samples are k / 255, k / 65535.  A float kind (floatpx.h: float pixels in or
// out) is widened exactly on the load and rounded once on the store; everything between is the float64 path.
enum PicElem { EL_F64, EL_F32, EL_U8, EL_U16, EL_FLT_F32, EL_FLT_F16, EL_FLT_BF16, EL_NONE };
static inline int el_size(PicElem el) {
    static const int bytes[] = {8, 4, 1, 2, 4, 2, 2, 0};
    return bytes[el];
}
// the float kind as the kernels want it (PxView.kind; 0: no float kind), and back (EL_NONE: not a kind -- view_pic refuses it)
static inline int el_flt_kind(PicElem el) { return el >= EL_FLT_F32 && el <= EL_FLT_BF16 ? el - EL_FLT_F32 + SPIHT_FLT_F32 : 0; }
static inline PicElem el_of_kind(int kind) { return flt_itemsize(kind) ? (PicElem)(EL_FLT_F32 + kind - SPIHT_FLT_F32) : EL_NONE; }
static inline PicElem el_of_hs(int elem) {  // the element of a host-fed stream: SPIHT_HS_F64 .. SPIHT_HS_BF16, checked by the caller
    static const PicElem els[] = {EL_F64, EL_U8, EL_U16, EL_FLT_F32, EL_FLT_F16, EL_FLT_BF16};
    return els[elem];
}

// A batch of pictures [B, c, h, w] at p: a dense array, or (strided) a view by byte strides that view_pic has checked.  The
// extern "C" entry points make one; everything behind them passes it on.
struct Pic {
    PicElem el = EL_F64;
    bool strided = false;  // a view by the strides of px (else dense: the inverse transform's output is [B, c, rec_H, rec_W])
    char *p = nullptr;     // the first picture
    bool out = false;      // the call writes the pixels (else it reads them)
    PxView px = {};        // a view's strides and extents (the rest of it: see view())
    int es() const { return el_size(el); }
    // the view as the strided kernels and the conversion passes take it
    PxView view() const {
        PxView v = px;
        v.es = es();
        v.kind = el_flt_kind(el);
        if (out) v.out = (uint8_t *)p;
        else v.in = (const uint8_t *)p;
        return v;
    }
    // the four byte strides of its pictures as [B, c, h, w]: the view's own, or the dense ones.  The only place that asks which.
    void strides(int64_t c, int64_t h, int64_t w, int64_t st[4]) const {
        if (strided) {
            st[0] = px.sb; st[1] = px.sc; st[2] = px.sh; st[3] = px.sw;
        } else {
            st[3] = es(); st[2] = w * st[3]; st[1] = h * st[2]; st[0] = c * st[1];
        }
    }
    // bytes from the first sample to one past the last of B pictures [c, h, w]; what the host calls transfer
    uint64_t bytes(int64_t B, int64_t c, int64_t h, int64_t w) const {
        int64_t st[4];
        strides(c, h, w, st);
        return (uint64_t)es() + (uint64_t)(B - 1) * st[0] + (uint64_t)(c - 1) * st[1] + (uint64_t)(h - 1) * st[2] + (uint64_t)(w - 1) * st[3];
    }
    // the pictures from b0 on
    Pic at(int64_t b0, int64_t c, int64_t h, int64_t w) const {
        int64_t st[4];
        strides(c, h, w, st);
        Pic v = *this;
        v.p += b0 * st[0];
        return v;
    }
    // the same pictures at another address (a copy of their bytes)
    Pic on(void *base) const {
        Pic v = *this;
        v.p = (char *)base;
        return v;
    }
};
static inline Pic dense_pic(const void *p, PicElem el, bool out = false) {
    Pic v;
    v.el = el;
    v.p = (char *)p;
    v.out = out;
    return v;
}
// The one builder of a strided picture: B pictures [c, h, w] of element el at p, by n byte strides -- n == 4: (sb, sc, sh, sw);
// n == 3: (sc, sh, sw) of one picture; nullptr: dense CHW.  Strides are non-negative and, as the base, multiples of the element
// size; a view that is written must not overlap itself.  What differs between the entry points is said by rules:
//   PIC_NULL_FIRST  a NULL p is SPIHT_ERR_ARG before anything else (else p is not looked at: the shared code refuses it later)
//   PIC_IMG_ARGS    check_img_args(wavelet, mode, B, c, h, w) runs before the view is looked at
//   PIC_EMPTY_OK    an empty batch (B == 0) is checked as one picture
enum { PIC_NULL_FIRST = 1, PIC_IMG_ARGS = 2, PIC_EMPTY_OK = 4 };
int view_pic(Pic *v, const void *p, PicElem el, bool out, const int64_t *strides, int n, int64_t B, int64_t c, int64_t h,
             int64_t w, int rules = 0, int wavelet = 0, int mode = 0);
// spiht_check_view_*: would view_pic take these four strides of B pictures [c, H, W] of element el (output: as a view that is written)
int check_view(PicElem el, int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output);

// The set-up of an image call on B pictures [c, H, W].  open(): the arguments and the geometry (coded: the coefficient
// array's Geom for the list coder too); false ends the call with *st -- an error, or SPIHT_OK for an empty batch, whose
// geometry is not looked at.  enter(): the context's lock, its device and the channel scales (nullptr: none uploaded).
// chunks(): batch_chunks over the call's batch.
struct ImgCall {
    spiht_ctx *ctx = nullptr;
    int64_t B = 0, c = 0;
    int F = 0;
    ImgGeom ig;
    ImgGeom pig;  // the geometry the pictures are made with: ig, or its reduced form (reduce())
    double q = 0; // ... and the quantisation scale that goes with it (reduce())
    Geom g;
    const double *d_mults = nullptr;
    std::unique_lock<std::recursive_mutex> lk;

    bool open(int *st, spiht_ctx *ctx_, int64_t B_, int64_t c_, int64_t H, int64_t W, int wavelet, int mode, int level, bool coded);
    // pictures of 1/2^k size (0: the call as it always was); before anything is queued
    bool reduce(int *st, int k, double q_scale);
    int enter(const double *channel_mults);
    template <class Fn> int chunks(Fn fn) const { return batch_chunks(B, c, fn); }
    // B pictures of the call as they lie in memory: a view, and every picture that is read, has the picture's own size; a
    // dense array that is written holds what the inverse transform makes (rec_H x rec_W)
    void extents(const Pic &v, int64_t *h, int64_t *w) const {
        const ImgGeom &vg = v.out ? pig : ig;
        const bool rec = v.out && !v.strided;
        *h = rec ? vg.rec_H : vg.hs[0];
        *w = rec ? vg.rec_W : vg.ws[0];
    }
    uint64_t bytes(const Pic &v, int64_t nb) const {
        int64_t h, w;
        extents(v, &h, &w);
        return v.bytes(nb, c, h, w);
    }
    Pic at(const Pic &v, int64_t b0) const {
        int64_t h, w;
        extents(v, &h, &w);
        return v.at(b0, c, h, w);
    }
};

// the transform drivers: pictures -> quantised packed array [planes, enc_h, enc_w], and back (levels l_hi .. l_lo: all of them)
int dwt_forward(spiht_ctx *ctx, const Pic &in, int planes, int c, const ImgGeom &ig, int wavelet, int mode, double q,
                const double *d_mults, int32_t *d_coeffs, uint32_t *d_maxabs = nullptr);
int dwt_inverse(spiht_ctx *ctx, const int32_t *d_rec, int planes, int c, const ImgGeom &ig, int wavelet, double q,
                const double *d_mults, const Pic &out, int l_hi = -1, int l_lo = 1, const double *d_a_in = nullptr,
                const uint32_t *d_flags = nullptr, const uint32_t *d_rows = nullptr);

// ---- api_image.cpp: what a host-fed stream queues -- the batched coded calls on a picture, and on a view of element el -----------
int encode_image_batch(spiht_ctx *ctx, const Pic &in, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                       double q_scale, const double *channel_mults, uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride,
                       uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs);
int decode_image_batch(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes, const uint8_t *d_max_n,
                       int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                       const double *channel_mults, const Pic &out, int32_t *d_rec, int reduce = 0);
int encode_image_batch_view(PicElem el, spiht_ctx *ctx, const void *d_img, const int64_t *strides, int64_t B, int64_t c, int64_t H,
                            int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                            uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n,
                            int32_t *d_coeffs);
int decode_image_batch_view(PicElem el, spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                            const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                            double q_scale, const double *channel_mults, void *d_img_out, const int64_t *out_strides,
                            int32_t *d_rec);

#pragma GCC visibility pop
