// C ABI of libspiht_hip.so (include/spiht_hip.h), tiled pictures (tiles.hip, overlap.hip, layers.hip): one picture <-> a dense
// batch of equal tiles -- the grid, the cut (with a margin: overlapping tiles), paste, mosaic (reduced tiles) and blend into a
// window -- T stream slots <-> one run of bytes, the quality layers of a tiled picture, the cut and the paste of a picture set
// (tileset.hip) and its resized crops (resample.hip).  Copies, the cross-fade and the resample; the
// transforms and the coder see the tiles as an ordinary batch.  As in api_image.cpp, a family of views by byte strides has one
// body, <family>_view, that takes the element; _f32s and the strided _f32 mosaic are views of EL_FLT_F32 (4-byte copies).
#include "api_internal.h"
#include "resample.h"

extern "C" int spiht_tile_grid(int64_t H, int64_t W, int64_t th, int64_t tw, int64_t *gy, int64_t *gx) {
    if (H < 1 || W < 1 || th < 8 || tw < 8) return SPIHT_ERR_ARG;
    if (H >= (1 << 30) || W >= (1 << 30) || th > (1 << 24) || tw > (1 << 24)) return SPIHT_ERR_TOO_LARGE;
    if (gy) *gy = (H + th - 1) / th;
    if (gx) *gx = (W + tw - 1) / tw;
    return SPIHT_OK;
}
// in: the picture batch (dense_pic, or tile_cut_view's checked view)
// overlap: NULL, or the margin m of spiht_tile_cut_overlap_* (k_tile_cut_overlap; 0 <= m, 2 m <= min(th, tw)): d_tiles is then
// [N * T, c, th + 2m, tw + 2m]
static int tile_cut(spiht_ctx *ctx, const Pic &in, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th, int64_t tw,
                    void *d_tiles, const int64_t *overlap = nullptr) {
    const int es = in.es();
    if (!ctx || !in.p || !d_tiles || N < 0 || c < 1 || (uintptr_t)in.p % es || (uintptr_t)d_tiles % es) return SPIHT_ERR_ARG;
    int64_t gy, gx;
    CHK(spiht_tile_grid(H, W, th, tw, &gy, &gx));
    if (overlap && (*overlap < 0 || 2 * *overlap > std::min(th, tw))) return SPIHT_ERR_ARG;
    if (c > 65535 || (__int128)N * gy * gx > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    if (N == 0) return SPIHT_OK;
    TileCutArgs a;
    a.in = (const uint8_t *)in.p;
    int64_t st[4];
    in.strides(c, H, W, st);
    a.sb = st[0]; a.sc = st[1]; a.sh = st[2]; a.sw = st[3];
    a.out = (uint8_t *)d_tiles;
    a.c = (int32_t)c; a.H = (int32_t)H; a.W = (int32_t)W; a.th = (int32_t)th; a.tw = (int32_t)tw;
    a.gy = (int32_t)gy; a.gx = (int32_t)gx; a.rows = 0;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    if (overlap) {
        const TileCutOverlapArgs q = {a, (int32_t)*overlap};
        LAUNCHCHK(spiht_launch_tile_cut_overlap(&q, es, N * gy * gx, ctx->stream));
        return SPIHT_OK;
    }
    LAUNCHCHK(spiht_launch_tile_cut(&a, es, N * gy * gx, ctx->stream));
    return SPIHT_OK;
}
// the strided cuts, plain and with a margin: the view of N pictures [c, H, W] (an empty batch is checked as one picture; a NULL
// picture is tile_cut's to refuse)
static int tile_cut_view(PicElem el, spiht_ctx *ctx, const void *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                         int64_t W, int64_t th, int64_t tw, void *d_tiles, const int64_t *overlap = nullptr) {
    if (N < 0 || c < 1 || H < 1 || W < 1) return SPIHT_ERR_ARG;
    Pic pic;
    CHK(view_pic(&pic, d_img, el, false, strides, 4, N, c, H, W, PIC_EMPTY_OK));
    return tile_cut(ctx, pic, N, c, H, W, th, tw, d_tiles, overlap);
}
extern "C" int spiht_tile_cut_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                                 int64_t W, int64_t th, int64_t tw, uint8_t *d_tiles) {
    return tile_cut_view(EL_U8, ctx, d_img, strides, N, c, H, W, th, tw, d_tiles);
}
extern "C" int spiht_tile_cut_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                                  int64_t W, int64_t th, int64_t tw, uint16_t *d_tiles) {
    return tile_cut_view(EL_U16, ctx, d_img, strides, N, c, H, W, th, tw, d_tiles);
}
extern "C" int spiht_tile_cut_f32s(spiht_ctx *ctx, const float *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                                   int64_t W, int64_t th, int64_t tw, float *d_tiles) {
    return tile_cut_view(EL_FLT_F32, ctx, d_img, strides, N, c, H, W, th, tw, d_tiles);
}
extern "C" int spiht_tile_cut_f32(spiht_ctx *ctx, const float *d_img, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th,
                                  int64_t tw, float *d_tiles) {
    return tile_cut(ctx, dense_pic(d_img, EL_F32), N, c, H, W, th, tw, d_tiles);
}
extern "C" int spiht_tile_cut_f64(spiht_ctx *ctx, const double *d_img, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th,
                                  int64_t tw, double *d_tiles) {
    return tile_cut(ctx, dense_pic(d_img, EL_F64), N, c, H, W, th, tw, d_tiles);
}
extern "C" int spiht_tile_cut_overlap_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t N, int64_t c,
                                         int64_t H, int64_t W, int64_t th, int64_t tw, int64_t m, uint8_t *d_tiles) {
    return tile_cut_view(EL_U8, ctx, d_img, strides, N, c, H, W, th, tw, d_tiles, &m);
}
extern "C" int spiht_tile_cut_overlap_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t N, int64_t c,
                                          int64_t H, int64_t W, int64_t th, int64_t tw, int64_t m, uint16_t *d_tiles) {
    return tile_cut_view(EL_U16, ctx, d_img, strides, N, c, H, W, th, tw, d_tiles, &m);
}
extern "C" int spiht_tile_cut_overlap_f32s(spiht_ctx *ctx, const float *d_img, const int64_t *strides, int64_t N, int64_t c,
                                           int64_t H, int64_t W, int64_t th, int64_t tw, int64_t m, float *d_tiles) {
    return tile_cut_view(EL_FLT_F32, ctx, d_img, strides, N, c, H, W, th, tw, d_tiles, &m);
}
extern "C" int spiht_tile_cut_overlap_f32(spiht_ctx *ctx, const float *d_img, int64_t N, int64_t c, int64_t H, int64_t W,
                                          int64_t th, int64_t tw, int64_t m, float *d_tiles) {
    return tile_cut(ctx, dense_pic(d_img, EL_F32), N, c, H, W, th, tw, d_tiles, &m);
}
extern "C" int spiht_tile_cut_overlap_f64(spiht_ctx *ctx, const double *d_img, int64_t N, int64_t c, int64_t H, int64_t W,
                                          int64_t th, int64_t tw, int64_t m, double *d_tiles) {
    return tile_cut(ctx, dense_pic(d_img, EL_F64), N, c, H, W, th, tw, d_tiles, &m);
}

// overlapping tiles: the tiles (lo, hi) with weight at position P of an axis of g tiles of t with margin m: the two of a seam's
// zone, else the one that owns P (m == 0: always that one)
static void blend_axis_tiles(int64_t P, int64_t g, int64_t t, int64_t m, int64_t *lo, int64_t *hi) {
    const int64_t k = (P + m) / t;
    if (k >= 1 && k < g && P + m - k * t < 2 * m) {
        *lo = k - 1; *hi = k;
    } else {
        *lo = *hi = P / t;
    }
}
// What paste, mosaic and blend ask of a window [y0, y0 + wh) x [x0, x0 + ww) and the sub-grid [i0, i1) x [j0, j1) of tiles it is
// made from: the sub-grid lies in the gy x gx grid, the window in the H x W picture, and the sub-grid holds every tile with
// weight in the window -- with margin m == 0 (paste, mosaic) the tiles the window meets; c and the tile count fit a launch.
static int check_window(int64_t c, int64_t gy, int64_t gx, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t m, int64_t i0,
                        int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww) {
    if (i0 < 0 || i1 <= i0 || i1 > gy || j0 < 0 || j1 <= j0 || j1 > gx) return SPIHT_ERR_ARG;
    if (y0 < 0 || x0 < 0 || wh < 1 || ww < 1 || y0 + wh > H || x0 + ww > W) return SPIHT_ERR_ARG;
    int64_t lo, hi, unused;
    blend_axis_tiles(y0, gy, th, m, &lo, &unused);
    blend_axis_tiles(y0 + wh - 1, gy, th, m, &unused, &hi);
    if (lo < i0 || hi >= i1) return SPIHT_ERR_ARG;
    blend_axis_tiles(x0, gx, tw, m, &lo, &unused);
    blend_axis_tiles(x0 + ww - 1, gx, tw, m, &unused, &hi);
    if (lo < j0 || hi >= j1) return SPIHT_ERR_ARG;
    if (c > 65535 || (__int128)(i1 - i0) * (j1 - j0) > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    return SPIHT_OK;
}
// the window's strides into the arguments of its kernel
template <class Args> static void window_strides(const Pic &out, int64_t c, int64_t wh, int64_t ww, Args *a) {
    int64_t st[4];
    out.strides(c, wh, ww, st);
    a->sc = st[1]; a->sh = st[2]; a->sw = st[3];
}
// the view of a strided window [c, wh, ww]
static int window_view(Pic *pic, void *d_out, PicElem el, const int64_t *out_strides, int64_t c, int64_t wh, int64_t ww) {
    if (c < 1 || wh < 1 || ww < 1) return SPIHT_ERR_ARG;
    return view_pic(pic, d_out, el, true, out_strides, 3, 1, c, wh, ww);
}

// out: the window (dense_pic, or window_view's checked view of [c, wh, ww])
static int tile_paste(spiht_ctx *ctx, const void *d_tiles, const Pic &out, int64_t c, int64_t rh, int64_t rw, int64_t H,
                      int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                      int64_t wh, int64_t ww) {
    const int es = out.es();
    if (!ctx || !d_tiles || !out.p || c < 1 || (uintptr_t)d_tiles % es || (uintptr_t)out.p % es) return SPIHT_ERR_ARG;
    int64_t gy, gx;
    CHK(spiht_tile_grid(H, W, th, tw, &gy, &gx));
    if (rh < th || rw < tw || rh > th + (1 << 24) || rw > tw + (1 << 24)) return SPIHT_ERR_ARG;
    CHK(check_window(c, gy, gx, H, W, th, tw, 0, i0, i1, j0, j1, y0, x0, wh, ww));
    TilePasteArgs a;
    a.tiles = (const uint8_t *)d_tiles;
    a.out = (uint8_t *)out.p;
    window_strides(out, c, wh, ww, &a);
    a.c = (int32_t)c; a.rh = (int32_t)rh; a.rw = (int32_t)rw; a.th = (int32_t)th; a.tw = (int32_t)tw;
    a.i0 = (int32_t)i0; a.j0 = (int32_t)j0; a.nj = (int32_t)(j1 - j0);
    a.y0 = (int32_t)y0; a.x0 = (int32_t)x0; a.wh = (int32_t)wh; a.ww = (int32_t)ww; a.rows = 0;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LAUNCHCHK(spiht_launch_tile_paste(&a, es, (i1 - i0) * (j1 - j0), ctx->stream));
    return SPIHT_OK;
}
static int tile_paste_view(PicElem el, spiht_ctx *ctx, const void *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                           int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                           int64_t wh, int64_t ww, void *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, el, out_strides, c, wh, ww));
    return tile_paste(ctx, d_tiles, pic, c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_paste_u8(spiht_ctx *ctx, const uint8_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                   int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                                   int64_t wh, int64_t ww, uint8_t *d_out, const int64_t *out_strides) {
    return tile_paste_view(EL_U8, ctx, d_tiles, c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww, d_out, out_strides);
}
extern "C" int spiht_tile_paste_u16(spiht_ctx *ctx, const uint16_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H,
                                    int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                                    int64_t x0, int64_t wh, int64_t ww, uint16_t *d_out, const int64_t *out_strides) {
    return tile_paste_view(EL_U16, ctx, d_tiles, c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww, d_out, out_strides);
}
extern "C" int spiht_tile_paste_f32s(spiht_ctx *ctx, const float *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                     int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                                     int64_t wh, int64_t ww, float *d_out, const int64_t *out_strides) {
    return tile_paste_view(EL_FLT_F32, ctx, d_tiles, c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww, d_out, out_strides);
}
extern "C" int spiht_tile_paste_f32(spiht_ctx *ctx, const float *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                    int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                                    int64_t wh, int64_t ww, float *d_out) {
    return tile_paste(ctx, d_tiles, dense_pic(d_out, EL_F32, true), c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_paste_f64(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                    int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                                    int64_t wh, int64_t ww, double *d_out) {
    return tile_paste(ctx, d_tiles, dense_pic(d_out, EL_F64, true), c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}

// tiled pictures at reduced resolution: the geometry (no device) and the assembly of reduced tiles (k_tile_mosaic)
extern "C" int spiht_tile_reduced_grid(int64_t H, int64_t W, int64_t th, int64_t tw, int wavelet, int mode, int level, int reduce,
                                       int *level_used, int64_t *thk, int64_t *twk, int64_t *Hk, int64_t *Wk, int64_t *gy,
                                       int64_t *gx, int64_t *rec_h, int64_t *rec_w, int64_t *pic_h, int64_t *pic_w,
                                       int64_t *off_y, int64_t *off_x) {
    int64_t ty, tx;
    CHK(spiht_tile_grid(H, W, th, tw, &ty, &tx));
    // the reduced decode of one tile: refuses a reduce outside 0 .. L
    CHK(spiht_reduced_shape(th, tw, wavelet, mode, level, reduce, level_used, rec_h, rec_w, pic_h, pic_w, off_y, off_x, nullptr,
                            nullptr));
    const int64_t m = ((int64_t)1 << reduce) - 1;
    if ((th & m) || (tw & m)) return SPIHT_ERR_ARG;  // a seam between two reduced samples
    if (thk) *thk = th >> reduce;
    if (twk) *twk = tw >> reduce;
    if (Hk) *Hk = (H + m) >> reduce;
    if (Wk) *Wk = (W + m) >> reduce;
    if (gy) *gy = ty;
    if (gx) *gx = tx;
    return SPIHT_OK;
}
// out: the window (dense_pic of float64, or window_view's checked view of [c, wh, ww]); H, W, th, tw: the picture and the tile
// being assembled (the reduced ones)
static int tile_mosaic(spiht_ctx *ctx, const void *d_tiles, const Pic &out, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                       int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1,
                       int64_t y0, int64_t x0, int64_t wh, int64_t ww) {
    const int es = out.es();
    if (!ctx || !d_tiles || !out.p || c < 1 || (uintptr_t)d_tiles % es || (uintptr_t)out.p % es) return SPIHT_ERR_ARG;
    if (H < 1 || W < 1 || th < 1 || tw < 1 || oy < 0 || ox < 0) return SPIHT_ERR_ARG;
    if (H >= (1 << 30) || W >= (1 << 30) || th > (1 << 24) || tw > (1 << 24)) return SPIHT_ERR_TOO_LARGE;
    if (oy > (1 << 24) || ox > (1 << 24) || rh < oy + th || rw < ox + tw || rh > th + (1 << 25) || rw > tw + (1 << 25))
        return SPIHT_ERR_ARG;
    CHK(check_window(c, (H + th - 1) / th, (W + tw - 1) / tw, H, W, th, tw, 0, i0, i1, j0, j1, y0, x0, wh, ww));
    TileMosaicArgs a;
    a.tiles = (const uint8_t *)d_tiles;
    a.out = (uint8_t *)out.p;
    window_strides(out, c, wh, ww, &a);
    a.c = (int32_t)c; a.rh = (int32_t)rh; a.rw = (int32_t)rw; a.oy = (int32_t)oy; a.ox = (int32_t)ox;
    a.th = (int32_t)th; a.tw = (int32_t)tw; a.i0 = (int32_t)i0; a.j0 = (int32_t)j0; a.nj = (int32_t)(j1 - j0);
    a.y0 = (int32_t)y0; a.x0 = (int32_t)x0; a.wh = (int32_t)wh; a.ww = (int32_t)ww; a.rows = 0;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LAUNCHCHK(spiht_launch_tile_mosaic(&a, es, ctx->stream));
    return SPIHT_OK;
}
static int tile_mosaic_view(PicElem el, spiht_ctx *ctx, const void *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy, int64_t ox,
                            int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                            int64_t x0, int64_t wh, int64_t ww, void *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, el, out_strides, c, wh, ww));
    return tile_mosaic(ctx, d_tiles, pic, c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_mosaic_u8(spiht_ctx *ctx, const uint8_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                                    int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0,
                                    int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww, uint8_t *d_out,
                                    const int64_t *out_strides) {
    return tile_mosaic_view(EL_U8, ctx, d_tiles, c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww, d_out, out_strides);
}
extern "C" int spiht_tile_mosaic_u16(spiht_ctx *ctx, const uint16_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                                     int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0,
                                     int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww, uint16_t *d_out,
                                     const int64_t *out_strides) {
    return tile_mosaic_view(EL_U16, ctx, d_tiles, c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww, d_out, out_strides);
}
extern "C" int spiht_tile_mosaic_f32(spiht_ctx *ctx, const float *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                                     int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0,
                                     int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww, float *d_out,
                                     const int64_t *out_strides) {
    return tile_mosaic_view(EL_FLT_F32, ctx, d_tiles, c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww, d_out,
                            out_strides);
}
extern "C" int spiht_tile_mosaic_f64(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                                     int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0,
                                     int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww, double *d_out) {
    if (c < 1 || wh < 1 || ww < 1) return SPIHT_ERR_ARG;
    return tile_mosaic(ctx, d_tiles, dense_pic(d_out, EL_F64, true), c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh,
                       ww);
}

// overlapping tiles: the cross-fade of the float64 decodes of a sub-grid into a window (k_tile_blend); into a float kind, rounded
// at the store
// out: the window (dense_pic of float64, or window_view's checked view of [c, wh, ww])
static int tile_blend(spiht_ctx *ctx, const double *d_tiles, const Pic &out, int64_t c, int64_t rh, int64_t rw, int64_t H,
                      int64_t W, int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                      int64_t x0, int64_t wh, int64_t ww) {
    const int es = out.es();
    if (!ctx || !d_tiles || !out.p || c < 1 || (uintptr_t)d_tiles % 8 || (uintptr_t)out.p % es) return SPIHT_ERR_ARG;
    int64_t gy, gx;
    CHK(spiht_tile_grid(H, W, th, tw, &gy, &gx));
    if (m < 0 || 2 * m > std::min(th, tw)) return SPIHT_ERR_ARG;
    if (rh < th + 2 * m || rw < tw + 2 * m || rh > th + (1 << 25) || rw > tw + (1 << 25)) return SPIHT_ERR_ARG;
    CHK(check_window(c, gy, gx, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww));
    TileBlendArgs a;
    a.tiles = d_tiles;
    a.out = (uint8_t *)out.p;
    window_strides(out, c, wh, ww, &a);
    a.c = (int32_t)c; a.rh = (int32_t)rh; a.rw = (int32_t)rw; a.th = (int32_t)th; a.tw = (int32_t)tw; a.m = (int32_t)m;
    a.gy = (int32_t)gy; a.gx = (int32_t)gx; a.i0 = (int32_t)i0; a.j0 = (int32_t)j0; a.nj = (int32_t)(j1 - j0);
    a.y0 = (int32_t)y0; a.x0 = (int32_t)x0; a.wh = (int32_t)wh; a.ww = (int32_t)ww; a.rows = 0;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    if (el_flt_kind(out.el)) LAUNCHCHK(spiht_launch_tile_blend_flt(&a, el_flt_kind(out.el), ctx->stream));
    else LAUNCHCHK(spiht_launch_tile_blend(&a, es, ctx->stream));
    return SPIHT_OK;
}
static int tile_blend_view(PicElem el, spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                           int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                           int64_t wh, int64_t ww, void *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, el, out_strides, c, wh, ww));
    return tile_blend(ctx, d_tiles, pic, c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_blend_u8(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                   int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                                   int64_t x0, int64_t wh, int64_t ww, uint8_t *d_out, const int64_t *out_strides) {
    return tile_blend_view(EL_U8, ctx, d_tiles, c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww, d_out, out_strides);
}
extern "C" int spiht_tile_blend_u16(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                    int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                                    int64_t x0, int64_t wh, int64_t ww, uint16_t *d_out, const int64_t *out_strides) {
    return tile_blend_view(EL_U16, ctx, d_tiles, c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww, d_out, out_strides);
}
extern "C" int spiht_tile_blend_flt(spiht_ctx *ctx, int kind, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H,
                                    int64_t W, int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1,
                                    int64_t y0, int64_t x0, int64_t wh, int64_t ww, void *d_out, const int64_t *out_strides) {
    return tile_blend_view(el_of_kind(kind), ctx, d_tiles, c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww, d_out,
                           out_strides);
}
extern "C" int spiht_tile_blend_f64(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                    int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                                    int64_t x0, int64_t wh, int64_t ww, double *d_out) {
    if (c < 1 || wh < 1 || ww < 1) return SPIHT_ERR_ARG;
    return tile_blend(ctx, d_tiles, dense_pic(d_out, EL_F64, true), c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh,
                      ww);
}

// T stream slots <-> one run of bytes.  The checks pack, unpack and the prefixes share; the scratch: uint64 [T] byte lengths
// (pack), uint64 [T] offsets
static int tile_streams_args(spiht_ctx *ctx, const void *a, const void *b, const void *d, const void *e, uint64_t slot_stride, int64_t T) {
    if (!ctx || !a || !b || !d || !e || T < 0 || slot_stride == 0 || slot_stride % 4) return SPIHT_ERR_ARG;
    if (T > 0x7FFFFFFF || slot_stride > ((uint64_t)1 << 29)) return SPIHT_ERR_TOO_LARGE;
    return SPIHT_OK;
}
extern "C" int spiht_tile_pack(spiht_ctx *ctx, const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_nbits, int64_t T,
                               uint8_t *d_packed, uint64_t packed_cap, uint32_t *d_lens) {
    CHK(tile_streams_args(ctx, d_slots, d_nbits, d_packed, d_lens, slot_stride, T));
    if (T == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->tilescr, (size_t)T * 16));
    uint64_t *d_nbytes = (uint64_t *)ctx->tilescr.p, *d_off = d_nbytes + T;
    CHK(spiht_nbits_to_nbytes(ctx, d_nbits, T, d_nbytes));
    LAUNCHCHK(spiht_launch_tile_pack(d_slots, slot_stride, d_nbytes, T, d_off, d_packed, packed_cap, d_lens, ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_tile_unpack(spiht_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint32_t *d_lens, int64_t T,
                                 uint8_t *d_slots, uint64_t slot_stride, uint64_t *d_nbytes) {
    CHK(tile_streams_args(ctx, d_packed, d_lens, d_slots, d_nbytes, slot_stride, T));
    if (T == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->tilescr, (size_t)T * 16));
    LAUNCHCHK(spiht_launch_tile_unpack(d_packed, packed_bytes, d_lens, T, (uint64_t *)ctx->tilescr.p + T, d_slots, slot_stride,
                                       d_nbytes, ctx->stream));
    return SPIHT_OK;
}

// prefixes of every stream, for the rate allocation across tiles (alloc.hip; the sums and the cut: api_rd.cpp)
extern "C" int spiht_tile_prefix_slots(spiht_ctx *ctx, const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_nbits,
                                       int64_t NT, int64_t K, int64_t k0, int64_t G, uint8_t *d_out, uint64_t out_stride,
                                       uint64_t *d_nbytes, const uint8_t *d_max_n, uint8_t *d_max_n_out) {
    CHK(tile_streams_args(ctx, d_slots, d_nbits, d_out, d_nbytes, slot_stride, NT));
    if (out_stride == 0 || out_stride % 4 || (uintptr_t)d_slots % 4 || (uintptr_t)d_out % 4 || (uintptr_t)d_nbits % 8 ||
        (uintptr_t)d_nbytes % 8)
        return SPIHT_ERR_ARG;
    if (K < 1 || K > 255 || k0 < 0 || G < 1 || k0 + G > K + 1 || !d_max_n != !d_max_n_out) return SPIHT_ERR_ARG;
    if (out_stride > ((uint64_t)1 << 29) || G * NT > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    if (NT == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LAUNCHCHK(spiht_launch_tile_prefix_slots(d_slots, slot_stride, d_nbits, NT, (int)K, (int)k0, (int)G, d_out, out_stride, d_nbytes,
                                             d_max_n, d_max_n_out, ctx->stream));
    return SPIHT_OK;
}
// ------------------------------------------------------------------------------------------------
// quality layers of a tiled picture (layers.hip): the tiles' streams in layer-major order and back
// ------------------------------------------------------------------------------------------------
static int layer_args(spiht_ctx *ctx, const void *a, const void *b, const void *d, const void *e, const void *f, uint64_t slot_stride,
                      int64_t Q, int64_t N, int64_t T) {
    if (!ctx || !a || !b || !d || !e || !f || slot_stride == 0 || slot_stride % 4) return SPIHT_ERR_ARG;
    if (Q < 1 || Q > 255 || N < 0 || T < 1) return SPIHT_ERR_ARG;
    if (slot_stride > ((uint64_t)1 << 29) || (__int128)N * Q * T > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    return SPIHT_OK;
}
extern "C" int spiht_layer_pack(spiht_ctx *ctx, const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_cum_bits, int64_t Q,
                                int64_t N, int64_t T, uint8_t *d_packed, uint64_t packed_cap, uint32_t *d_cum, uint64_t *d_pic_bytes) {
    CHK(layer_args(ctx, d_slots, d_cum_bits, d_packed, d_cum, d_pic_bytes, slot_stride, Q, N, T));
    if ((uintptr_t)d_cum_bits % 8 || (uintptr_t)d_cum % 4 || (uintptr_t)d_pic_bytes % 8) return SPIHT_ERR_ARG;
    if (N == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->layerscr, (size_t)(N * Q * T) * 8));
    LAUNCHCHK(spiht_launch_layer_pack(d_slots, slot_stride, d_cum_bits, Q, N, T, (uint64_t *)ctx->layerscr.p, d_packed, packed_cap,
                                      d_cum, d_pic_bytes, ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_layer_unpack(spiht_ctx *ctx, const uint8_t *d_layers, uint64_t layers_bytes, const uint32_t *d_cum, int64_t Q,
                                  int64_t T, int64_t upto, const int32_t *d_sel, int64_t S, uint8_t *d_slots, uint64_t slot_stride,
                                  uint64_t *d_nbytes) {
    CHK(layer_args(ctx, d_layers, d_cum, d_slots, d_nbytes, d_nbytes, slot_stride, Q, 1, T));
    if (upto < 1 || upto > Q || S < 0 || (!d_sel && S > T)) return SPIHT_ERR_ARG;
    if ((uintptr_t)d_cum % 4 || (uintptr_t)d_sel % 4 || (uintptr_t)d_nbytes % 8) return SPIHT_ERR_ARG;
    if (S > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    if (S == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->layerscr, (size_t)(upto * T) * 12));
    uint64_t *d_off = (uint64_t *)ctx->layerscr.p;
    LAUNCHCHK(spiht_launch_layer_unpack(d_layers, layers_bytes, d_cum, T, upto, d_sel, S, d_off, (uint32_t *)(d_off + upto * T), d_slots,
                                        slot_stride, d_nbytes, ctx->stream));
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// picture sets (tileset.hip): pictures of different sizes as one tile batch, one tile batch into many windows
// ------------------------------------------------------------------------------------------------
static PicElem el_of_es(int es) {  // a copy moves elements of a size: any element of that size has its rules of a view
    switch (es) {
    case 1: return EL_U8;
    case 2: return EL_U16;
    case 4: return EL_FLT_F32;
    case 8: return EL_F64;
    default: return EL_NONE;
    }
}
static size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
// The tables of one call, `bytes` at h, into ctx->tsettab by a copy on the context's stream.  The copy reads a page-locked stage
// that belongs to this call until the copy is done (the stage's event): the next call takes another stage, so two calls queued
// back to back each see their own tables.  The device side needs no such care: the next copy is queued behind this call's
// kernel.  No wait unless all TS_MAX_STAGES copies are still in flight; called with the context's lock held.
static int upload_tables(spiht_ctx *ctx, const void *h, size_t bytes) {
    CHK(ensure(ctx, ctx->tsettab, bytes));
    int k = -1;
    for (size_t i = 0; i < ctx->tstages.size() && k < 0; i++) {
        if (hipEventQuery(ctx->tstages[i].copied) == hipSuccess) k = (int)i;
        else (void)hipGetLastError();  // (not ready: no error of ours)
    }
    if (k < 0 && ctx->tstages.size() < TS_MAX_STAGES) {
        TableStage s;
        HIPCHK(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
        ctx->tstages.push_back(s);
        k = (int)ctx->tstages.size() - 1;
    }
    if (k < 0) {
        k = 0;
        HIPCHK(hipEventSynchronize(ctx->tstages[0].copied));
    }
    TableStage &s = ctx->tstages[k];
    if (s.cap < bytes) {  // (its last copy is done: nothing reads it)
        if (s.host) HIPCHK(hipHostFree(s.host));
        s.host = nullptr;
        s.cap = 0;
        HIPCHK(hipHostMalloc(&s.host, bytes + bytes / 4 + 4096, hipHostMallocDefault));
        s.cap = bytes + bytes / 4 + 4096;
    }
    memcpy(s.host, h, bytes);
    HIPCHK(hipMemcpyAsync(ctx->tsettab.p, s.host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipEventRecord(s.copied, ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_tile_cut_set(spiht_ctx *ctx, int es, int64_t P, int64_t c, int64_t th, int64_t tw, const spiht_tileset_pic *pics,
                                  void *d_tiles) {
    const PicElem el = el_of_es(es);
    if (!ctx || el == EL_NONE || !pics || !d_tiles || P < 1 || c < 1 || (uintptr_t)d_tiles % es) return SPIHT_ERR_ARG;
    if (c > 65535 || P > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    // the whole table is checked before anything is queued
    int64_t NT = 0;
    for (int64_t p = 0; p < P; p++) {
        const spiht_tileset_pic &q = pics[p];
        int64_t gy, gx;
        if (!q.d_img) return SPIHT_ERR_ARG;
        CHK(spiht_tile_grid(q.H, q.W, th, tw, &gy, &gx));
        const int64_t st[3] = {q.sc, q.sh, q.sw};
        Pic v;
        CHK(view_pic(&v, q.d_img, el, false, st, 3, 1, c, q.H, q.W));
        NT += gy * gx;
        if (NT > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    }
    const size_t tab = align16((size_t)P * sizeof(TileSetPic)), bytes = tab + align16((size_t)NT * 4);
    std::vector<char> h(bytes, 0);
    TileSetPic *rows = (TileSetPic *)h.data();
    uint32_t *pic_of_tile = (uint32_t *)(h.data() + tab);
    uint32_t tile0 = 0;
    for (int64_t p = 0; p < P; p++) {
        const spiht_tileset_pic &q = pics[p];
        const int64_t gy = (q.H + th - 1) / th, gx = (q.W + tw - 1) / tw;
        rows[p] = {(const uint8_t *)q.d_img, q.sc, q.sh, q.sw, (int32_t)q.H, (int32_t)q.W, (int32_t)gx, tile0};
        std::fill(pic_of_tile + tile0, pic_of_tile + tile0 + gy * gx, (uint32_t)p);
        tile0 += (uint32_t)(gy * gx);
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(upload_tables(ctx, h.data(), bytes));
    TileSetCutArgs a;
    a.pics = (const TileSetPic *)ctx->tsettab.p;
    a.pic_of_tile = (const uint32_t *)((const char *)ctx->tsettab.p + tab);
    a.out = (uint8_t *)d_tiles;
    a.c = (int32_t)c; a.th = (int32_t)th; a.tw = (int32_t)tw; a.rows = 0;
    LAUNCHCHK(spiht_launch_tile_cut_set(&a, es, NT, ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_tile_paste_set(spiht_ctx *ctx, int es, int64_t B, int64_t c, int64_t rh, int64_t rw, int64_t th, int64_t tw,
                                    const spiht_tileset_item *items, const void *d_tiles, int64_t S) {
    const PicElem el = el_of_es(es);
    if (!ctx || el == EL_NONE || !items || !d_tiles || B < 1 || c < 1 || S < 0 || (uintptr_t)d_tiles % es) return SPIHT_ERR_ARG;
    if (c > 65535 || B > 0x7FFFFFFF || S > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    // the whole table is checked before anything is queued
    int64_t sum = 0, n = 1, nrows = 1;
    int strided = 0;
    for (int64_t b = 0; b < B; b++) {
        const spiht_tileset_item &q = items[b];
        int64_t gy, gx;
        if (!q.d_out) return SPIHT_ERR_ARG;
        CHK(spiht_tile_grid(q.H, q.W, th, tw, &gy, &gx));
        if (rh < th || rw < tw || rh > th + (1 << 24) || rw > tw + (1 << 24)) return SPIHT_ERR_ARG;
        CHK(check_window(c, gy, gx, q.H, q.W, th, tw, 0, q.i0, q.i1, q.j0, q.j1, q.y0, q.x0, q.wh, q.ww));
        const int64_t st[3] = {q.sc, q.sh, q.sw};
        Pic v;
        CHK(window_view(&v, q.d_out, el, st, c, q.wh, q.ww));
        sum += (q.i1 - q.i0) * (q.j1 - q.j0);
        if (sum > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
        n = std::max(n, std::min(tw, q.ww));
        nrows = std::max(nrows, std::min(th, q.wh));
        strided |= q.sw != es;
    }
    if (sum != S) return SPIHT_ERR_ARG;
    const size_t tab = align16((size_t)B * sizeof(TileSetItem)), bytes = tab + align16((size_t)S * 4);
    std::vector<char> h(bytes, 0);
    TileSetItem *rows = (TileSetItem *)h.data();
    uint32_t *item_of_tile = (uint32_t *)(h.data() + tab);
    uint32_t s0 = 0;
    for (int64_t b = 0; b < B; b++) {
        const spiht_tileset_item &q = items[b];
        const int64_t cnt = (q.i1 - q.i0) * (q.j1 - q.j0);
        rows[b] = {(uint8_t *)q.d_out, q.sc, q.sh, q.sw, (int32_t)q.i0, (int32_t)q.j0, (int32_t)(q.j1 - q.j0), s0,
                   (int32_t)q.y0, (int32_t)q.x0, (int32_t)q.wh, (int32_t)q.ww};
        std::fill(item_of_tile + s0, item_of_tile + s0 + cnt, (uint32_t)b);
        s0 += (uint32_t)cnt;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(upload_tables(ctx, h.data(), bytes));
    TileSetPasteArgs a;
    a.items = (const TileSetItem *)ctx->tsettab.p;
    a.item_of_tile = (const uint32_t *)((const char *)ctx->tsettab.p + tab);
    a.tiles = (const uint8_t *)d_tiles;
    a.c = (int32_t)c; a.rh = (int32_t)rh; a.rw = (int32_t)rw; a.th = (int32_t)th; a.tw = (int32_t)tw; a.rows = 0;
    LAUNCHCHK(spiht_launch_tile_paste_set(&a, es, S, n, nrows, strided, ctx->stream));
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// resized crops (resample.hip): boxes of the pictures of a set, resampled to one size straight from the decoded tiles
// ------------------------------------------------------------------------------------------------
// One axis table of n outputs at `off` of the caller's blob (resample.h: start, count, weights), K taps wide, for a box side of
// `side` samples: it lies in the blob, every run of taps lies in the box and has 1 .. K <= RS_MAX_TAPS taps.  rows: the table
// of the rows -- the taps of RS_ROWS consecutive outputs span at most the RS_SPAN source rows a workgroup holds
static int check_axis_table(const uint8_t *tables, uint64_t table_bytes, int64_t off, int64_t K, int64_t n, int64_t side, bool rows) {
    if (off < 0 || off % 8 || K < 1 || K > RS_MAX_TAPS) return SPIHT_ERR_ARG;
    if ((uint64_t)off > table_bytes || rs_table_bytes(n, K) > table_bytes - (uint64_t)off) return SPIHT_ERR_ARG;
    const int32_t *start = (const int32_t *)(tables + off), *count = start + n;
    for (int64_t i = 0; i < n; i++)
        if (count[i] < 1 || count[i] > K || start[i] < 0 || (int64_t)start[i] + count[i] > side) return SPIHT_ERR_ARG;
    for (int64_t r0 = 0; rows && r0 < n; r0 += RS_ROWS) {
        int64_t lo = start[r0], hi = lo + count[r0];
        for (int64_t r = r0 + 1; r < std::min<int64_t>(n, r0 + RS_ROWS); r++) {
            lo = std::min<int64_t>(lo, start[r]);
            hi = std::max<int64_t>(hi, (int64_t)start[r] + count[r]);
        }
        if (hi - lo > RS_SPAN) return SPIHT_ERR_ARG;
    }
    return SPIHT_OK;
}
// The rule's table of one axis (spiht_amd/resample.py: axis_table, flip_table), written in the layout above: host arithmetic
// only, every operation and its order the rule's -- float64, nothing fused --, so that a caller need not build B tables in
// numpy for every call.  tests/test_resample_cpu.py holds it to axis_table bit for bit.
extern "C" int spiht_resample_axis_table(int64_t n_in, int64_t n_out, int flip, void *table, uint64_t cap, int64_t *K,
                                         uint64_t *bytes) {
#pragma clang fp contract(off)
    if (n_in < 1 || n_out < 1 || !K || !bytes) return SPIHT_ERR_ARG;
    if (n_in >= (1 << 30) || n_out > (1 << 24)) return SPIHT_ERR_TOO_LARGE;
    const double scale = (double)n_in / (double)n_out, support = scale > 1.0 ? scale : 1.0, inv = 1.0 / support;
    auto run = [&](int64_t i, int64_t *start, int64_t *stop) {  // the taps of output i, and its centre
        const double center = scale * ((double)i + 0.5);
        *start = std::max<int64_t>(0, (int64_t)(center - support + 0.5));
        *stop = std::min<int64_t>(n_in, (int64_t)(center + support + 0.5));
        return center;
    };
    int64_t k_max = 0, a, b;
    for (int64_t i = 0; i < n_out; i++) {
        run(i, &a, &b);
        k_max = std::max(k_max, b - a);
    }
    *K = k_max;
    *bytes = rs_table_bytes(n_out, k_max);
    if (!table) return SPIHT_OK;  // (a question: K and the bytes)
    if (cap < *bytes || (uintptr_t)table % 8) return SPIHT_ERR_ARG;
    int32_t *start = (int32_t *)table, *count = start + n_out;
    double *w = (double *)(count + n_out);
    for (int64_t x = 0; x < n_out; x++, w += k_max) {
        const double center = run(flip ? n_out - 1 - x : x, &a, &b);
        start[x] = (int32_t)a;
        count[x] = (int32_t)(b - a);
        double total = 0.0;
        for (int64_t j = a; j < b; j++) {
            const double d = fabs(((double)j - center + 0.5) * inv), v = 1.0 - d;
            w[j - a] = v > 0.0 ? v : 0.0;
            total = j == a ? w[0] : total + w[j - a];  // in ascending j
        }
        for (int64_t k = 0; k < k_max; k++) w[k] = k < b - a ? w[k] / total : 0.0;
    }
    return SPIHT_OK;
}
extern "C" int spiht_tile_resample_set(spiht_ctx *ctx, int elem, int64_t B, int64_t c, int64_t rh, int64_t rw, int64_t th, int64_t tw,
                                       int64_t oh, int64_t ow, const spiht_tileset_item *items, const int64_t *item_tables,
                                       const void *tables, uint64_t table_bytes, const double *mean, const double *std,
                                       const double *d_tiles, int64_t S) {
    if (!ctx || elem < SPIHT_HS_F64 || elem > SPIHT_HS_BF16 || !items || !item_tables || !tables || !d_tiles) return SPIHT_ERR_ARG;
    if (B < 1 || c < 1 || oh < 1 || ow < 1 || S < 0 || (uintptr_t)d_tiles % 8 || (uintptr_t)tables % 8 || !mean != !std) return SPIHT_ERR_ARG;
    const PicElem el = el_of_hs(elem);
    if (mean && (el == EL_U8 || el == EL_U16)) return SPIHT_ERR_ARG;  // (8 / 16 bits are clipped to [0, 1]: no normalisation)
    if (c > 65535 || B > 65535 || S > 0x7FFFFFFF || oh > (1 << 24) || ow > (1 << 24) || table_bytes > ((uint64_t)1 << 31)) return SPIHT_ERR_TOO_LARGE;
    if (((oh + RS_ROWS - 1) / RS_ROWS) * ((ow + RS_COLS - 1) / RS_COLS) > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    for (int64_t ch = 0; mean && ch < c; ch++)
        if (std[ch] == 0.0) return SPIHT_ERR_ARG;
    // the rows and the tables are checked completely before anything is queued
    int64_t sum = 0;
    for (int64_t b = 0; b < B; b++) {
        const spiht_tileset_item &q = items[b];
        const int64_t *t = item_tables + 4 * b;
        int64_t gy, gx;
        if (!q.d_out) return SPIHT_ERR_ARG;
        CHK(spiht_tile_grid(q.H, q.W, th, tw, &gy, &gx));
        if (rh < th || rw < tw || rh > th + (1 << 24) || rw > tw + (1 << 24)) return SPIHT_ERR_ARG;
        CHK(check_window(c, gy, gx, q.H, q.W, th, tw, 0, q.i0, q.i1, q.j0, q.j1, q.y0, q.x0, q.wh, q.ww));
        const int64_t st[3] = {q.sc, q.sh, q.sw};
        Pic v;
        CHK(window_view(&v, q.d_out, el, st, c, oh, ow));
        CHK(check_axis_table((const uint8_t *)tables, table_bytes, t[0], t[1], ow, q.ww, false));
        CHK(check_axis_table((const uint8_t *)tables, table_bytes, t[2], t[3], oh, q.wh, true));
        sum += (q.i1 - q.i0) * (q.j1 - q.j0);
        if (sum > 0x7FFFFFFF) return SPIHT_ERR_TOO_LARGE;
    }
    if (sum != S) return SPIHT_ERR_ARG;
    // one blob: the items' rows, mean and std, the tables
    const size_t tab = align16((size_t)B * sizeof(ResampleItem)), norm = mean ? align16((size_t)c * 16) : 0;
    const size_t bytes = tab + norm + align16((size_t)table_bytes);
    std::vector<char> h(bytes, 0);
    ResampleItem *rows = (ResampleItem *)h.data();
    uint32_t s0 = 0;
    for (int64_t b = 0; b < B; b++) {
        const spiht_tileset_item &q = items[b];
        const int64_t *t = item_tables + 4 * b;
        rows[b] = {(uint8_t *)q.d_out, q.sc, q.sh, q.sw, (int32_t)q.i0, (int32_t)q.j0, (int32_t)(q.j1 - q.j0), s0,
                   (int32_t)q.y0, (int32_t)q.x0, (int32_t)q.wh, (int32_t)q.ww,
                   (uint32_t)(tab + norm + t[0]), (uint32_t)(tab + norm + t[2]), (int32_t)t[1], (int32_t)t[3]};
        s0 += (uint32_t)((q.i1 - q.i0) * (q.j1 - q.j0));
    }
    if (mean) {
        memcpy(h.data() + tab, mean, (size_t)c * 8);
        memcpy(h.data() + tab + (size_t)c * 8, std, (size_t)c * 8);
    }
    memcpy(h.data() + tab + norm, tables, (size_t)table_bytes);
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(upload_tables(ctx, h.data(), bytes));
    ResampleArgs a;
    a.items = (const ResampleItem *)ctx->tsettab.p;
    a.tables = (const uint8_t *)ctx->tsettab.p;
    a.mean = mean ? (const double *)((const char *)ctx->tsettab.p + tab) : nullptr;
    a.std = mean ? a.mean + c : nullptr;
    a.tiles = d_tiles;
    a.c = (int32_t)c; a.rh = (int32_t)rh; a.rw = (int32_t)rw; a.th = (int32_t)th; a.tw = (int32_t)tw;
    a.oh = (int32_t)oh; a.ow = (int32_t)ow; a.ncol = 0;
    LAUNCHCHK(spiht_launch_tile_resample_set(&a, el_size(el), el_flt_kind(el), B, ctx->stream));
    return SPIHT_OK;
}
