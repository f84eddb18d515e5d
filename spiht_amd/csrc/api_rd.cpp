// C ABI of libspiht_hip.so (include/spiht_hip.h), rate-distortion: the error sums of decoded arrays and pictures against the
// original (rd.hip) -- K decodes -> K small rows, all in HBM -- and the rate allocation across the tiles of a tiled picture
// (alloc.hip, roi.hip): the error sums of the tiles' prefixes (api_tiles.cpp cuts them), plain or weighted, and the cut of equal slope.
#include "api_internal.h"

extern "C" int spiht_sqerr_i32(spiht_ctx *ctx, const int32_t *d_x, const int32_t *d_y, int64_t K, int64_t c, int64_t h, int64_t w,
                               uint64_t *d_out) {
    if (!ctx || !d_x || !d_y || !d_out || K < 1 || K > 65535 || c < 1 || h < 1 || w < 1) return SPIHT_ERR_ARG;
    if (c > 65535 || h >= (1 << 28) || w >= (1 << 28) || (__int128)c * h * w >= (1 << 28)) return SPIHT_ERR_TOO_LARGE;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t hw = (uint32_t)(h * w);
    CHK(ensure(ctx, ctx->rdpart, (size_t)K * c * rd_tiles(hw, RD_TILE_I32) * 16));
    LAUNCHCHK(spiht_launch_sqerr_i32(d_x, d_y, (int)K, (int)c, hw, (uint64_t *)ctx->rdpart.p, d_out, ctx->stream));
    return SPIHT_OK;
}
// the checks the pixel-domain sums share: K as above, a picture of fewer than 2^30 samples per channel (the 64-bit sums),
// K * c within a grid's x extent
static int sse_args(spiht_ctx *ctx, const void *d_pic, const void *d_dec, int64_t K, int64_t c, int64_t H, int64_t W,
                    const void *d_out) {
    if (!ctx || !d_pic || !d_dec || !d_out || K < 1 || K > 65535 || c < 1 || H < 1 || W < 1) return SPIHT_ERR_ARG;
    if (c > 65535 || H >= (1 << 30) || W >= (1 << 30) || H * W >= (1 << 30)) return SPIHT_ERR_TOO_LARGE;
    if (K * c > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;  // (the second launch: one workgroup / thread per (k, channel))
    return SPIHT_OK;
}
extern "C" int spiht_sse_f64(spiht_ctx *ctx, const double *d_pic, const double *d_dec, int64_t K, int64_t c, int64_t H, int64_t W,
                             int64_t rec_h, int64_t rec_w, double *d_out) {
    CHK(sse_args(ctx, d_pic, d_dec, K, c, H, W, d_out));
    if (rec_h < H || rec_w < W) return SPIHT_ERR_ARG;
    if (rec_h >= (1 << 30) || rec_w >= (1 << 30)) return SPIHT_ERR_TOO_LARGE;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->rdpart, (size_t)K * c * rd_tiles(H, RD_TILE_ROWS) * 8));
    LAUNCHCHK(spiht_launch_sse_f64(d_pic, d_dec, (int)K, (int)c, (int)H, (int)W, (int)rec_h, (int)rec_w, (double *)ctx->rdpart.p,
                                   d_out, ctx->stream));
    return SPIHT_OK;
}
// strides: (sc, sh, sw) of the original in bytes, NULL = dense CHW; d_dec: dense [K, c, H, W] of the same element
static int sse_view(PicElem el, spiht_ctx *ctx, const void *d_pic, const int64_t *strides, const void *d_dec, int64_t K, int64_t c,
                  int64_t H, int64_t W, uint64_t *d_out) {
    CHK(sse_args(ctx, d_pic, d_dec, K, c, H, W, d_out));
    if ((uintptr_t)d_dec % (uintptr_t)el_size(el) != 0) return SPIHT_ERR_ARG;
    Pic pic;
    CHK(view_pic(&pic, d_pic, el, false, strides, 3, 1, c, H, W));
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->rdpart, (size_t)K * c * rd_tiles((uint64_t)H * W, RD_TILE_PX) * 8));
    const PxView px = pic.view();
    LAUNCHCHK(spiht_launch_sse_px(&px, d_dec, (int)K, (uint64_t *)ctx->rdpart.p, d_out, ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_sse_u8(spiht_ctx *ctx, const uint8_t *d_pic, const int64_t *strides, const uint8_t *d_dec, int64_t K,
                            int64_t c, int64_t H, int64_t W, uint64_t *d_out) {
    return sse_view(EL_U8, ctx, d_pic, strides, d_dec, K, c, H, W, d_out);
}
extern "C" int spiht_sse_u16(spiht_ctx *ctx, const uint16_t *d_pic, const int64_t *strides, const uint16_t *d_dec, int64_t K,
                             int64_t c, int64_t H, int64_t W, uint64_t *d_out) {
    return sse_view(EL_U16, ctx, d_pic, strides, d_dec, K, c, H, W, d_out);
}

// ---- rate allocation across tiles ----
// el: the element of the ORIGINAL tiles d_tiles [N * T, c, th, tw]; the decodes d_dec [G, N * T, c, rh, rw] are of the same
// element, but float64 beside a float kind (float pixels in: the decodes and the sums are float64) -> d_out [G][N * T].
// weighted: every term times d_w [N or 1][H][W] (roi.hip)
static int sse_tiles(PicElem el, spiht_ctx *ctx, const void *d_tiles, const void *d_dec, int64_t G, int64_t N, int64_t c, int64_t H,
                     int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, void *d_out, bool weighted = false,
                     const uint8_t *d_w = nullptr, uint64_t w_stride = 0) {
    const int kind = el_flt_kind(el), es = kind ? 8 : el_size(el);
    if (!ctx || !d_tiles || !d_dec || !d_out || G < 1 || G > 65535 || N < 1 || c < 1) return SPIHT_ERR_ARG;
    if (weighted && !d_w) return SPIHT_ERR_ARG;
    if (el == EL_NONE) return SPIHT_ERR_ARG;  // (not a float kind)
    if ((uintptr_t)d_tiles % el_size(el) || (uintptr_t)d_dec % es || (uintptr_t)d_out % 8) return SPIHT_ERR_ARG;
    int64_t gy, gx;
    CHK(spiht_tile_grid(H, W, th, tw, &gy, &gx));
    if (rh < th || rw < tw) return SPIHT_ERR_ARG;
    if (weighted && w_stride != 0 && w_stride < (uint64_t)H * (uint64_t)W) return SPIHT_ERR_ARG;
    // the exact 64-bit sum of a weighted tile: 255 * 65535^2 * 2^24 < 2^64
    if (weighted && es != 8 && (__int128)c * th * tw > ((__int128)1 << 24)) return SPIHT_ERR_ARG;
    if (c > 65535 || th * tw >= (1 << 30) || rh >= (1 << 30) || rw >= (1 << 30) || al_chunks(th) > 65535) return SPIHT_ERR_TOO_LARGE;
    if (es != 8 && (__int128)c * th * tw >= ((__int128)1 << 32)) return SPIHT_ERR_TOO_LARGE;  // the exact 64-bit sum of a tile
    if ((__int128)G * N * gy * gx > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    TileSseArgs a;
    a.tiles = d_tiles; a.dec = d_dec; a.out = d_out;
    a.c = (int32_t)c; a.H = (int32_t)H; a.W = (int32_t)W; a.th = (int32_t)th; a.tw = (int32_t)tw; a.rh = (int32_t)rh;
    a.rw = (int32_t)rw; a.gx = (int32_t)gx;
    a.T = (uint32_t)(gy * gx); a.NT = (uint32_t)(N * gy * gx); a.chunks = al_chunks(th);
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->rdpart, (size_t)G * a.NT * c * a.chunks * 8));
    a.part = ctx->rdpart.p;
    if (weighted) {
        TileSseWArgs q;
        q.a = a; q.w = d_w; q.w_stride = w_stride;
        if (kind) LAUNCHCHK(spiht_launch_sse_tiles_w_flt(&q, kind, G, ctx->stream));
        else LAUNCHCHK(spiht_launch_sse_tiles_w(&q, es, G, ctx->stream));
    } else {
        if (kind) LAUNCHCHK(spiht_launch_sse_tiles_flt(&a, kind, G, ctx->stream));
        else LAUNCHCHK(spiht_launch_sse_tiles(&a, es, G, ctx->stream));
    }
    return SPIHT_OK;
}
extern "C" int spiht_sse_tiles_f64(spiht_ctx *ctx, const double *d_tiles, const double *d_dec, int64_t G, int64_t N, int64_t c,
                                   int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, double *d_out) {
    return sse_tiles(EL_F64, ctx, d_tiles, d_dec, G, N, c, H, W, th, tw, rh, rw, d_out);
}
extern "C" int spiht_sse_tiles_u8(spiht_ctx *ctx, const uint8_t *d_tiles, const uint8_t *d_dec, int64_t G, int64_t N, int64_t c,
                                  int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, uint64_t *d_out) {
    return sse_tiles(EL_U8, ctx, d_tiles, d_dec, G, N, c, H, W, th, tw, rh, rw, d_out);
}
extern "C" int spiht_sse_tiles_u16(spiht_ctx *ctx, const uint16_t *d_tiles, const uint16_t *d_dec, int64_t G, int64_t N, int64_t c,
                                   int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, uint64_t *d_out) {
    return sse_tiles(EL_U16, ctx, d_tiles, d_dec, G, N, c, H, W, th, tw, rh, rw, d_out);
}
extern "C" int spiht_sse_tiles_w_f64(spiht_ctx *ctx, const double *d_tiles, const double *d_dec, int64_t G, int64_t N, int64_t c,
                                     int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, double *d_out,
                                     const uint8_t *d_w, uint64_t w_stride) {
    return sse_tiles(EL_F64, ctx, d_tiles, d_dec, G, N, c, H, W, th, tw, rh, rw, d_out, true, d_w, w_stride);
}
extern "C" int spiht_sse_tiles_w_u8(spiht_ctx *ctx, const uint8_t *d_tiles, const uint8_t *d_dec, int64_t G, int64_t N, int64_t c,
                                    int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, uint64_t *d_out,
                                    const uint8_t *d_w, uint64_t w_stride) {
    return sse_tiles(EL_U8, ctx, d_tiles, d_dec, G, N, c, H, W, th, tw, rh, rw, d_out, true, d_w, w_stride);
}
extern "C" int spiht_sse_tiles_w_u16(spiht_ctx *ctx, const uint16_t *d_tiles, const uint16_t *d_dec, int64_t G, int64_t N, int64_t c,
                                     int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, uint64_t *d_out,
                                     const uint8_t *d_w, uint64_t w_stride) {
    return sse_tiles(EL_U16, ctx, d_tiles, d_dec, G, N, c, H, W, th, tw, rh, rw, d_out, true, d_w, w_stride);
}
// float pixels in: the original tiles of a float kind, widened on the load; the decodes float64 -- the bits of the _f64 calls
// on the widened tiles
extern "C" int spiht_sse_tiles_flt(spiht_ctx *ctx, int kind, const void *d_tiles, const double *d_dec, int64_t G, int64_t N,
                                   int64_t c, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, double *d_out) {
    return sse_tiles(el_of_kind(kind), ctx, d_tiles, d_dec, G, N, c, H, W, th, tw, rh, rw, d_out);
}
extern "C" int spiht_sse_tiles_w_flt(spiht_ctx *ctx, int kind, const void *d_tiles, const double *d_dec, int64_t G, int64_t N,
                                     int64_t c, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, double *d_out,
                                     const uint8_t *d_w, uint64_t w_stride) {
    return sse_tiles(el_of_kind(kind), ctx, d_tiles, d_dec, G, N, c, H, W, th, tw, rh, rw, d_out, true, d_w, w_stride);
}
// both cuts: at the budget (d_target NULL), or at a target squared error per picture under that budget
static int tile_allocate(spiht_ctx *ctx, const uint64_t *d_nbits, const void *d_D, int kind, int64_t K, int64_t N, int64_t T,
                         uint64_t budget_bytes, const double *d_target, uint64_t *d_nbits_out, double *d_lambda, double *d_dist,
                         uint32_t *d_met) {
    if (!ctx || !d_nbits || !d_D || !d_nbits_out || (kind != 0 && kind != 1) || K < 1 || K > 255 || N < 0 || T < 1)
        return SPIHT_ERR_ARG;
    if ((uintptr_t)d_nbits % 8 || (uintptr_t)d_D % 8 || (uintptr_t)d_nbits_out % 8 || (uintptr_t)d_lambda % 8) return SPIHT_ERR_ARG;
    if ((uintptr_t)d_target % 8 || (uintptr_t)d_dist % 8 || (uintptr_t)d_met % 4) return SPIHT_ERR_ARG;
    if ((__int128)N * T > 0x7FFFFFFF || budget_bytes > ((uint64_t)1 << 60)) return SPIHT_ERR_TOO_LARGE;
    if (N == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->allocscr, al_scratch_bytes((uint64_t)N * T, (uint64_t)K)));
    LAUNCHCHK(spiht_launch_tile_allocate(d_nbits, d_D, kind, (int)K, N, T, budget_bytes, d_target, ctx->allocscr.p, d_nbits_out,
                                         d_lambda, d_dist, d_met, ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_tile_allocate(spiht_ctx *ctx, const uint64_t *d_nbits, const void *d_D, int kind, int64_t K, int64_t N,
                                   int64_t T, uint64_t budget_bytes, uint64_t *d_nbits_out, double *d_lambda) {
    return tile_allocate(ctx, d_nbits, d_D, kind, K, N, T, budget_bytes, nullptr, d_nbits_out, d_lambda, nullptr, nullptr);
}
extern "C" int spiht_tile_allocate_target(spiht_ctx *ctx, const uint64_t *d_nbits, const void *d_D, int kind, int64_t K, int64_t N,
                                          int64_t T, uint64_t budget_bytes, const double *d_target, uint64_t *d_nbits_out,
                                          double *d_lambda, double *d_dist, uint32_t *d_met) {
    if (!d_target) return SPIHT_ERR_ARG;
    return tile_allocate(ctx, d_nbits, d_D, kind, K, N, T, budget_bytes, d_target, d_nbits_out, d_lambda, d_dist, d_met);
}
