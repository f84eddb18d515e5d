// C ABI of libspiht_hip.so (include/spiht_hip.h), the image calls built on the transform drivers of api_dwt.cpp: transform and
// quantise, the inverse in one piece and in two parts, the coded calls on device batches and on host arrays, their
// reduced-resolution forms, the float conversions on their own, and transform + pyramid.
// A call family whose pictures come as a view by byte strides has ONE body, <family>_view, that takes the element (PicElem),
// builds the view by that family's rules and goes on as the dense calls do; its exports only name the element: _u8 EL_U8,
// _u16 EL_U16, _flt el_of_kind(kind) (no such kind: EL_NONE, which view_pic refuses where the family looks at the view).  A
// float kind goes the float64 path behind its exact widening -- NOT the single-precision transform of the *_f32 calls.
#include "api_internal.h"

static int dwt_quant_batch(spiht_ctx *ctx, const Pic &in, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                           int level, double q_scale, const double *channel_mults, int32_t *d_coeffs) {
    if (!ctx || !in.p || !d_coeffs) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, B, c, H, W, wavelet, mode, level, false)) return st;
    CHK(k.enter(channel_mults));
    return k.chunks([&](int64_t b0, int nb) -> int {
        return dwt_forward(ctx, k.at(in, b0), nb * (int)c, (int)c, k.ig, wavelet, mode, q_scale, k.d_mults,
                           d_coeffs + (size_t)b0 * c * k.ig.enc_h * k.ig.enc_w);
    });
}
extern "C" int spiht_dwt_quant_batch_f64(spiht_ctx *ctx, const double *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                                         int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                         int32_t *d_coeffs) {
    return dwt_quant_batch(ctx, dense_pic(d_img, EL_F64), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs);
}
extern "C" int spiht_dwt_quant_batch_f32(spiht_ctx *ctx, const float *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                                         int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                         int32_t *d_coeffs) {
    return dwt_quant_batch(ctx, dense_pic(d_img, EL_F32), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs);
}

static int dequant_idwt_batch(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B, int64_t c, int64_t H,
                              int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                              const Pic &out, int reduce = 0) {
    if (!ctx || !d_rec || !out.p) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, B, c, H, W, wavelet, mode, level, false) || !k.reduce(&st, reduce, q_scale)) return st;
    CHK(k.enter(channel_mults));
    L1Flags fl;
    const bool flagged = d_flags && reduce == 0 && !(ctx->color_on && c == 3) && l1flags_geometry(k.ig, k.F, &fl);
    return k.chunks([&](int64_t b0, int nb) -> int {
        return dwt_inverse(ctx, d_rec + (size_t)b0 * c * k.ig.enc_h * k.ig.enc_w, nb * (int)c, (int)c, k.pig, wavelet, k.q,
                           k.d_mults, k.at(out, b0), -1, 1, nullptr, flagged ? d_flags + (size_t)b0 * c * fl.gy * fl.gx : nullptr);
    });
}
extern "C" int spiht_dequant_idwt_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H,
                                            int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, double *d_img_out) {
    return dequant_idwt_batch(ctx, d_rec, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                              dense_pic(d_img_out, EL_F64, true));
}
extern "C" int spiht_dequant_idwt_flags_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B,
                                                  int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                  double q_scale, const double *channel_mults, double *d_img_out) {
    return dequant_idwt_batch(ctx, d_rec, d_flags, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                              dense_pic(d_img_out, EL_F64, true));
}
static int dequant_idwt_flags_view(PicElem el, spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B, int64_t c,
                                   int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                   const double *channel_mults, void *d_img_out, const int64_t *out_strides) {
    Pic out;
    CHK(view_pic(&out, d_img_out, el, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST));
    return dequant_idwt_batch(ctx, d_rec, d_flags, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out);
}
extern "C" int spiht_dequant_idwt_flags_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B,
                                                 int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                 const double *channel_mults, uint8_t *d_img_out, const int64_t *out_strides) {
    return dequant_idwt_flags_view(EL_U8, ctx, d_rec, d_flags, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_img_out,
                                   out_strides);
}
extern "C" int spiht_dequant_idwt_flags_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B,
                                                  int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                  const double *channel_mults, uint16_t *d_img_out, const int64_t *out_strides) {
    return dequant_idwt_flags_view(EL_U16, ctx, d_rec, d_flags, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_img_out,
                                   out_strides);
}
extern "C" int spiht_dequant_idwt_flags_batch_flt(spiht_ctx *ctx, int kind, const int32_t *d_rec, const uint32_t *d_flags,
                                                  int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                  double q_scale, const double *channel_mults, void *d_img_out,
                                                  const int64_t *out_strides) {
    return dequant_idwt_flags_view(el_of_kind(kind), ctx, d_rec, d_flags, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                                   d_img_out, out_strides);
}

// The inverse transform in two parts, so that a pipelined caller can queue the coarse levels (a quarter of the bytes,
// six small launches at 1080p) where no list decoder shares the GPU and only level 1 beside it (csrc/pipeline.cpp):
//   coarse (no `out` pictures): levels level..2 -> d_approx [B*c, 2*hs[2]-F+2, 2*ws[2]-F+2] (float64), the approximation
//   level 1 starts from
//   level1: d_rec + d_approx -> pixels.  With fewer than two levels the coarse part does nothing and d_approx is not read.
static int idwt_part(spiht_ctx *ctx, const int32_t *d_rec, double *d_approx, int64_t B, int64_t c, int64_t H, int64_t W,
                     int wavelet, int mode, int level, double q_scale, const double *channel_mults, const Pic &out,
                     const uint32_t *d_flags = nullptr, const uint32_t *d_rows = nullptr) {
    if (!ctx || !d_rec || (!d_approx && !out.p)) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, B, c, H, W, wavelet, mode, level, false)) return st;
    const ImgGeom &ig = k.ig;
    if (ig.per) return SPIHT_ERR_ARG;  // (the two-part inverse is a schedule experiment of the tiled kernels)
    const bool coarse = !out.p;
    if (coarse && ig.L < 2) return SPIHT_OK;
    if (!coarse && ig.L >= 2 && !d_approx) return SPIHT_ERR_ARG;
    CHK(k.enter(channel_mults));
    const int F = k.F;
    const size_t a_plane = ig.L >= 2 ? (size_t)(2 * ig.hs[2] - F + 2) * (size_t)(2 * ig.ws[2] - F + 2) : 0;
    L1Flags fl;
    const bool flagged = d_flags && !(ctx->color_on && c == 3) && l1flags_geometry(ig, F, &fl);
    return k.chunks([&](int64_t b0, int nb) -> int {
        const int32_t *rec = d_rec + (size_t)b0 * c * ig.enc_h * ig.enc_w;
        double *ap = d_approx ? d_approx + (size_t)b0 * c * a_plane : nullptr;
        if (coarse)
            return dwt_inverse(ctx, rec, nb * (int)c, (int)c, ig, wavelet, q_scale, k.d_mults, dense_pic(ap, EL_F64, true), ig.L, 2,
                               nullptr);
        const size_t w0 = flagged ? (size_t)b0 * c * fl.gy * fl.gx : 0;  // (the chunk's words, and its row words)
        return dwt_inverse(ctx, rec, nb * (int)c, (int)c, ig, wavelet, q_scale, k.d_mults, k.at(out, b0), std::min(ig.L, 1), 1,
                           ig.L >= 2 ? ap : nullptr, flagged ? d_flags + w0 : nullptr, flagged && d_rows ? d_rows + w0 : nullptr);
    });
}
extern "C" int spiht_idwt_coarse_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                           int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                           double *d_approx) {
    return idwt_part(ctx, d_rec, d_approx, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, Pic());  // (no d_approx: refused)
}
extern "C" int spiht_idwt_level1_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, double *d_img_out) {
    return spiht_idwt_level1_flags_batch_f64(ctx, d_rec, d_approx, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                                             d_img_out);
}
// ... reading the decoder's occupancy words of the level-1 tiles (spiht_decode_lists_flags_batch_i32; NULL: reads everything)
extern "C" int spiht_idwt_level1_flags_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                                 int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                 double q_scale, const double *channel_mults, double *d_img_out) {
    return spiht_idwt_level1_rows_batch_f64(ctx, d_rec, d_approx, d_flags, nullptr, B, c, H, W, wavelet, mode, level, q_scale,
                                            channel_mults, d_img_out);
}
// ... and its row words (spiht_decode_lists_rows_batch_i32; NULL: a set word means every row)
extern "C" int spiht_idwt_level1_rows_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                                const uint32_t *d_rows, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                                int mode, int level, double q_scale, const double *channel_mults, double *d_img_out) {
    if (!d_img_out) return SPIHT_ERR_ARG;
    return idwt_part(ctx, d_rec, const_cast<double *>(d_approx), B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                     dense_pic(d_img_out, EL_F64, true), d_flags, d_rows);
}
static int idwt_level1_rows_view(PicElem el, spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                 const uint32_t *d_rows, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                 double q_scale, const double *channel_mults, void *d_img_out, const int64_t *out_strides) {
    Pic out;
    CHK(view_pic(&out, d_img_out, el, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST));
    return idwt_part(ctx, d_rec, const_cast<double *>(d_approx), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out,
                     d_flags, d_rows);
}
extern "C" int spiht_idwt_level1_rows_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                               const uint32_t *d_rows, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                               int mode, int level, double q_scale, const double *channel_mults, uint8_t *d_img_out,
                                               const int64_t *out_strides) {
    return idwt_level1_rows_view(EL_U8, ctx, d_rec, d_approx, d_flags, d_rows, B, c, H, W, wavelet, mode, level, q_scale,
                                 channel_mults, d_img_out, out_strides);
}
extern "C" int spiht_idwt_level1_rows_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                                const uint32_t *d_rows, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                                int mode, int level, double q_scale, const double *channel_mults,
                                                uint16_t *d_img_out, const int64_t *out_strides) {
    return idwt_level1_rows_view(EL_U16, ctx, d_rec, d_approx, d_flags, d_rows, B, c, H, W, wavelet, mode, level, q_scale,
                                 channel_mults, d_img_out, out_strides);
}
extern "C" int spiht_idwt_level1_flags_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                                int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                double q_scale, const double *channel_mults, uint8_t *d_img_out,
                                                const int64_t *out_strides) {
    return idwt_level1_rows_view(EL_U8, ctx, d_rec, d_approx, d_flags, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                                  d_img_out, out_strides);
}
extern "C" int spiht_idwt_level1_flags_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                                 int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                 double q_scale, const double *channel_mults, uint16_t *d_img_out,
                                                 const int64_t *out_strides) {
    return idwt_level1_rows_view(EL_U16, ctx, d_rec, d_approx, d_flags, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                                  d_img_out, out_strides);
}

// the coded calls on device batches: pictures -> streams and back
int encode_image_batch(spiht_ctx *ctx, const Pic &in, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                       double q_scale, const double *channel_mults, uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride,
                       uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs) {
    if (!ctx || !in.p || !d_out || !d_nbits || !d_max_n) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, B, c, H, W, wavelet, mode, level, true)) return st;
    CHK(k.enter(channel_mults));
    const Geom &g = k.g;
    return k.chunks([&](int64_t b0, int nb) -> int {
        int32_t *co = d_coeffs ? d_coeffs + (size_t)b0 * g.n : nullptr;
        if (!co) {
            CHK(ensure(ctx, ctx->coeffs, (size_t)nb * g.n * 4));
            co = (int32_t *)ctx->coeffs.p;
        }
        CHK(ensure(ctx, ctx->maxabs, (size_t)nb * 4));
        HIPCHK(hipMemsetAsync(ctx->maxabs.p, 0, (size_t)nb * 4, ctx->stream));
        CHK(dwt_forward(ctx, k.at(in, b0), nb * (int)c, (int)c, k.ig, wavelet, mode, q_scale, k.d_mults, co,
                        (uint32_t *)ctx->maxabs.p));
        return encode_device(ctx, g, co, nb, max_bits, d_out + (size_t)b0 * slot_stride, slot_stride, d_nbits + b0, d_max_n + b0,
                             true);
    });  // asynchronous: errors surface in spiht_ctx_synchronize()
}
extern "C" int spiht_encode_image_batch_f64(spiht_ctx *ctx, const double *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                                            int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                            uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride, uint64_t *d_nbits,
                                            uint8_t *d_max_n, int32_t *d_coeffs) {
    return encode_image_batch(ctx, dense_pic(d_img, EL_F64), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits,
                              d_out, slot_stride, d_nbits, d_max_n, d_coeffs);
}
extern "C" int spiht_encode_image_batch_f32(spiht_ctx *ctx, const float *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                                            int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                            uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride, uint64_t *d_nbits,
                                            uint8_t *d_max_n, int32_t *d_coeffs) {
    return encode_image_batch(ctx, dense_pic(d_img, EL_F32), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits,
                              d_out, slot_stride, d_nbits, d_max_n, d_coeffs);
}
int encode_image_batch_view(PicElem el, spiht_ctx *ctx, const void *d_img, const int64_t *strides, int64_t B, int64_t c, int64_t H,
                            int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                            uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n,
                            int32_t *d_coeffs) {
    Pic in;
    CHK(view_pic(&in, d_img, el, false, strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return encode_image_batch(ctx, in, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, d_out, slot_stride,
                              d_nbits, d_max_n, d_coeffs);
}
extern "C" int spiht_encode_image_batch_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                                           uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs) {
    return encode_image_batch_view(EL_U8, ctx, d_img, strides, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits,
                                   d_out, slot_stride, d_nbits, d_max_n, d_coeffs);
}
extern "C" int spiht_encode_image_batch_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                            int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                                            uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs) {
    return encode_image_batch_view(EL_U16, ctx, d_img, strides, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits,
                                   d_out, slot_stride, d_nbits, d_max_n, d_coeffs);
}
extern "C" int spiht_encode_image_batch_flt(spiht_ctx *ctx, int kind, const void *d_img, const int64_t *strides, int64_t B,
                                            int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                                            uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs) {
    return encode_image_batch_view(el_of_kind(kind), ctx, d_img, strides, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                                   max_bits, d_out, slot_stride, d_nbits, d_max_n, d_coeffs);
}

int decode_image_batch(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes, const uint8_t *d_max_n,
                       int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                       const double *channel_mults, const Pic &out, int32_t *d_rec, int reduce) {
    if (!ctx || !d_data || !d_nbytes || !d_max_n || !out.p) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, B, c, H, W, wavelet, mode, level, true) || !k.reduce(&st, reduce, q_scale)) return st;
    CHK(k.enter(channel_mults));
    const Geom &g = k.g;
    return k.chunks([&](int64_t b0, int nb) -> int {
        int32_t *rec = d_rec ? d_rec + (size_t)b0 * g.n : nullptr;
        // the decoder tells the inverse transform which level-1 tiles hold anything (common.h: L1Flags)
        L1Flags fl;
        // (a reduced decode never reaches the stream's level 1: it asks for no words and passes none)
        const bool flagged = ctx->opt_l1_flags && reduce == 0 && !(ctx->color_on && c == 3) && l1flags_geometry(k.ig, k.F, &fl);
        if (flagged) {
            const size_t nw = (size_t)nb * c * fl.gy * fl.gx;  // words, and as many row words behind them: one buffer, one fill
            CHK(ensure(ctx, ctx->l1flags, 2 * nw * 4));
            fl.p = (uint32_t *)ctx->l1flags.p;
            fl.rows = fl.p + nw;
        }
        if (rec) {
            CHK(decode_device(ctx, g, d_data + (size_t)b0 * slot_stride, slot_stride, d_nbytes + b0, d_max_n + b0, nb, rec,
                              nullptr, nullptr, 0, true, nullptr, flagged ? &fl : nullptr));
            return dwt_inverse(ctx, rec, nb * (int)c, (int)c, k.pig, wavelet, k.q, k.d_mults, k.at(out, b0), -1, 1, nullptr,
                               flagged ? fl.p : nullptr, flagged ? fl.rows : nullptr);
        }
        // Internal coefficient array: it is all zero on entry and is left all zero -- after the inverse transform the
        // cells the decoder wrote are cleared again through its own LSP lists (about 1 % of the array) instead of
        // zero-filling 26 MB per 1080p image before every decode.
        const size_t old_cap = ctx->recz.cap;  // (the allocator may hand back the same address for a larger buffer)
        CHK(ensure(ctx, ctx->recz, (size_t)nb * g.n * 4));
        if (ctx->recz.cap != old_cap || !ctx->recz_clean) {
            StageTimer t(ctx, ST_MEMSET);
            HIPCHK(hipMemsetAsync(ctx->recz.p, 0, ctx->recz.cap, ctx->stream));
            ctx->recz_clean = true;
        }
        rec = (int32_t *)ctx->recz.p;
        DecArgs da;
        CHK(decode_device(ctx, g, d_data + (size_t)b0 * slot_stride, slot_stride, d_nbytes + b0, d_max_n + b0, nb, rec, nullptr,
                          nullptr, 0, false, &da, flagged ? &fl : nullptr));
        // (a reduced inverse reads a corner of the array only; the decoder wrote all over it: its whole LSP is cleared)
        CHK(dwt_inverse(ctx, rec, nb * (int)c, (int)c, k.pig, wavelet, k.q, k.d_mults, k.at(out, b0), -1, 1, nullptr,
                        flagged ? fl.p : nullptr, flagged ? fl.rows : nullptr));
        if (da.nslots >= nb) {
            StageTimer t(ctx, ST_MEMSET);
            LAUNCHCHK(spiht_launch_unscatter(&da, ctx->stream));
        } else {
            ctx->recz_clean = false;  // slots were reused inside the launch: the lists of earlier images are gone
        }
        return SPIHT_OK;
    });  // asynchronous: errors surface in spiht_ctx_synchronize()
}
extern "C" int spiht_decode_image_batch_f64(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                            const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                            int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, double *d_img_out, int32_t *d_rec) {
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, dense_pic(d_img_out, EL_F64, true), d_rec);
}
int decode_image_batch_view(PicElem el, spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                            const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                            double q_scale, const double *channel_mults, void *d_img_out, const int64_t *out_strides,
                            int32_t *d_rec) {
    Pic out;
    CHK(view_pic(&out, d_img_out, el, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, out, d_rec);
}
extern "C" int spiht_decode_image_batch_u8(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                           const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                           int mode, int level, double q_scale, const double *channel_mults, uint8_t *d_img_out,
                                           const int64_t *out_strides, int32_t *d_rec) {
    return decode_image_batch_view(EL_U8, ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                                   channel_mults, d_img_out, out_strides, d_rec);
}
extern "C" int spiht_decode_image_batch_u16(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                            const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                            int mode, int level, double q_scale, const double *channel_mults, uint16_t *d_img_out,
                                            const int64_t *out_strides, int32_t *d_rec) {
    return decode_image_batch_view(EL_U16, ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                                   channel_mults, d_img_out, out_strides, d_rec);
}
extern "C" int spiht_decode_image_batch_flt(spiht_ctx *ctx, int kind, const uint8_t *d_data, uint64_t slot_stride,
                                            const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H,
                                            int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, void *d_img_out, const int64_t *out_strides,
                                            int32_t *d_rec) {
    return decode_image_batch_view(el_of_kind(kind), ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level,
                                   q_scale, channel_mults, d_img_out, out_strides, d_rec);
}

// ------------------------------------------------------------------------------------------------
// the drop-in calls on host arrays: encode_image / decode_image / decode_from_rec_arr of the reference's wrapper
// (spiht_wrapper.py:142-216, 259-281) as one C call each.  Pixels, stream and coefficient array live in the
// context's grow-only device buffers -- no allocation per call after the first of a given size.
// ------------------------------------------------------------------------------------------------
// (a view: only the bytes its strides span are uploaded)
static int encode_image_host(spiht_ctx *ctx, const Pic &img, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                             double q_scale, const double *channel_mults, uint64_t max_bits, uint8_t *out, uint64_t out_cap,
                             uint64_t *out_nbits, uint8_t *max_n) {
    if (!ctx || !img.p || !out_nbits || !max_n || (!out && out_cap)) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, 1, c, H, W, wavelet, mode, level, true)) return st;
    CHK(k.enter(nullptr));  // (the channel scales: the batch call's)
    uint64_t bits = bound_bits(k.g, 0x3FFFFFFFu);
    if (max_bits != 0) bits = std::min(bits, max_bits);
    if (bits >= 0xFFFFFF00ull * 8ull) return SPIHT_ERR_TOO_LARGE;
    const uint64_t slot = std::max<uint64_t>(4, ((bits + 7) / 8 + 3) & ~3ull);
    const size_t img_bytes = (size_t)k.bytes(img, 1);
    DevBuf &hb = img.strided ? ctx->hpix8 : ctx->himg;
    CHK(ensure(ctx, hb, img_bytes));
    CHK(ensure(ctx, ctx->out, slot));
    CHK(ensure(ctx, ctx->nbits, 8));
    CHK(ensure(ctx, ctx->maxn, 4));
    CHK(take_err(ctx));
    {
        StageTimer t(ctx, ST_H2D);
        HIPCHK(hipMemcpyAsync(hb.p, img.p, img_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    CHK(encode_image_batch(ctx, img.on(hb.p), 1, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits,
                           (uint8_t *)ctx->out.p, slot, (uint64_t *)ctx->nbits.p, (uint8_t *)ctx->maxn.p, nullptr));
    return read_encoded(ctx, out, out_cap, out_nbits, max_n);
}
extern "C" int spiht_encode_image_host_f64(spiht_ctx *ctx, const double *img, int64_t c, int64_t H, int64_t W, int wavelet,
                                           int mode, int level, double q_scale, const double *channel_mults, uint64_t max_bits,
                                           uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n) {
    return encode_image_host(ctx, dense_pic(img, EL_F64), c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out,
                             out_cap, out_nbits, max_n);
}
extern "C" int spiht_encode_image_host_f32(spiht_ctx *ctx, const float *img, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                                           int level, double q_scale, const double *channel_mults, uint64_t max_bits, uint8_t *out,
                                           uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n) {
    return encode_image_host(ctx, dense_pic(img, EL_F32), c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out,
                             out_cap, out_nbits, max_n);
}
static int encode_image_host_view(PicElem el, spiht_ctx *ctx, const void *img, const int64_t *strides, int64_t c, int64_t H,
                                  int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                  uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n) {
    Pic in;
    CHK(view_pic(&in, img, el, false, strides, 3, 1, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return encode_image_host(ctx, in, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out, out_cap, out_nbits,
                             max_n);
}
extern "C" int spiht_encode_image_host_u8(spiht_ctx *ctx, const uint8_t *img, const int64_t *strides, int64_t c, int64_t H,
                                          int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                          uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n) {
    return encode_image_host_view(EL_U8, ctx, img, strides, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out,
                                  out_cap, out_nbits, max_n);
}
extern "C" int spiht_encode_image_host_u16(spiht_ctx *ctx, const uint16_t *img, const int64_t *strides, int64_t c, int64_t H,
                                           int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                           uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n) {
    return encode_image_host_view(EL_U16, ctx, img, strides, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out,
                                  out_cap, out_nbits, max_n);
}
extern "C" int spiht_encode_image_host_flt(spiht_ctx *ctx, int kind, const void *img, const int64_t *strides, int64_t c, int64_t H,
                                           int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                           uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n) {
    return encode_image_host_view(el_of_kind(kind), ctx, img, strides, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                                  max_bits, out, out_cap, out_nbits, max_n);
}

// the copy back of a host decode into a view is of c * h * w samples: only the two dense layouts, CHW and HWC
static int dense_chw_or_hwc(const Pic &v) {
    const int64_t es = v.es(), c = v.px.c, h = v.px.h, w = v.px.w;
    const bool chw = v.px.sw == es && v.px.sh == w * es && v.px.sc == h * w * es;
    const bool hwc = v.px.sc == es && v.px.sw == c * es && v.px.sh == w * c * es;
    return chw || hwc ? SPIHT_OK : SPIHT_ERR_ARG;
}
static int decode_image_host(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H, int64_t W,
                             int wavelet, int mode, int level, double q_scale, const double *channel_mults, const Pic &img_out,
                             int reduce = 0) {
    if (!ctx || !img_out.p || (!data && nbytes)) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, 1, c, H, W, wavelet, mode, level, false) || !k.reduce(&st, reduce, q_scale)) return st;
    if (n > 30) return SPIHT_ERR_MAGNITUDE;
    if (nbytes * 8 >= 0xFFFFFF00ull) return SPIHT_ERR_TOO_LARGE;
    CHK(k.enter(nullptr));  // (the channel scales: the batch call's)
    const size_t out_bytes = (size_t)k.bytes(img_out, 1);  // (a reduced picture: only its bytes come back)
    DevBuf &hb = img_out.strided ? ctx->hpix8 : ctx->himg;
    CHK(ensure(ctx, hb, out_bytes));
    uint64_t slot;
    CHK(stage_stream(ctx, data, nbytes, n, &slot));
    CHK(decode_image_batch(ctx, (const uint8_t *)ctx->data.p, slot, (const uint64_t *)ctx->nbytes.p, (const uint8_t *)ctx->maxn.p, 1,
                           c, H, W, wavelet, mode, level, q_scale, channel_mults, img_out.on(hb.p), nullptr, reduce));
    CHK(take_err(ctx));
    {
        StageTimer t(ctx, ST_D2H);
        HIPCHK(hipMemcpyAsync(img_out.p, hb.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_decode_image_host_f64(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, double *img_out) {
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                             dense_pic(img_out, EL_F64, true));
}
static int decode_image_host_view(PicElem el, spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H,
                                  int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                  void *img_out, const int64_t *strides) {
    Pic out;
    CHK(view_pic(&out, img_out, el, true, strides, 3, 1, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    CHK(dense_chw_or_hwc(out));
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, out);
}
extern "C" int spiht_decode_image_host_u8(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                          int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                          const double *channel_mults, uint8_t *img_out, const int64_t *strides) {
    return decode_image_host_view(EL_U8, ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, img_out,
                                  strides);
}
extern "C" int spiht_decode_image_host_u16(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, uint16_t *img_out, const int64_t *strides) {
    return decode_image_host_view(EL_U16, ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, img_out,
                                  strides);
}
extern "C" int spiht_decode_image_host_flt(spiht_ctx *ctx, int kind, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, void *img_out, const int64_t *strides) {
    return decode_image_host_view(el_of_kind(kind), ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                                  img_out, strides);
}

extern "C" int spiht_dequant_idwt_host_f64(spiht_ctx *ctx, const int32_t *rec, int64_t c, int64_t H, int64_t W, int wavelet,
                                           int mode, int level, double q_scale, const double *channel_mults, double *img_out) {
    if (!ctx || !rec || !img_out) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, 1, c, H, W, wavelet, mode, level, false)) return st;
    CHK(k.enter(nullptr));  // (the channel scales: the batch call's)
    const ImgGeom &ig = k.ig;
    const size_t rec_bytes = (size_t)c * ig.enc_h * ig.enc_w * 4, out_bytes = (size_t)c * ig.rec_H * ig.rec_W * 8;
    CHK(ensure(ctx, ctx->hrec, rec_bytes));
    CHK(ensure(ctx, ctx->himg, out_bytes));
    {
        StageTimer t(ctx, ST_H2D);
        HIPCHK(hipMemcpyAsync(ctx->hrec.p, rec, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    CHK(spiht_dequant_idwt_batch_f64(ctx, (const int32_t *)ctx->hrec.p, 1, c, H, W, wavelet, mode, level, q_scale,
                                     channel_mults, (double *)ctx->himg.p));
    {
        StageTimer t(ctx, ST_D2H);
        HIPCHK(hipMemcpyAsync(img_out, ctx->himg.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// reduced-resolution decode: the picture at 1/2^reduce size straight from the coefficient array or the stream
// (include/spiht_hip.h).  The calls above with a reduced geometry behind them (api_dwt.cpp: reduced_geometry / reduced_q):
// levels L .. reduce + 1 of the inverse transform run, nothing below.  The list decoder is the same: it parses every bit.
// ------------------------------------------------------------------------------------------------
// the view of a reduced call: B pictures [c, hs[reduce], ws[reduce]] by n strides
static int reduced_pic(void *p, PicElem el, const int64_t *strides, int n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                       int mode, int level, int reduce, Pic *out) {
    if (!p) return SPIHT_ERR_ARG;
    CHK(check_img_args(wavelet, mode, B, c, H, W));
    ImgGeom ig, pig;
    CHK(reduced_open(H, W, wavelet, mode, level, reduce, &ig, &pig));
    return view_pic(out, p, el, true, strides, n, B, c, pig.hs[0], pig.ws[0]);
}

extern "C" int spiht_dequant_idwt_reduced_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H,
                                                    int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, double *d_img_out, int reduce) {
    return dequant_idwt_batch(ctx, d_rec, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                              dense_pic(d_img_out, EL_F64, true), reduce);
}
static int dequant_idwt_reduced_view(PicElem el, spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                     int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                     void *d_img_out, const int64_t *out_strides, int reduce) {
    Pic out;
    CHK(reduced_pic(d_img_out, el, out_strides, 4, B, c, H, W, wavelet, mode, level, reduce, &out));
    return dequant_idwt_batch(ctx, d_rec, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out, reduce);
}
extern "C" int spiht_dequant_idwt_reduced_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                                   int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                                   uint8_t *d_img_out, const int64_t *out_strides, int reduce) {
    return dequant_idwt_reduced_view(EL_U8, ctx, d_rec, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_img_out,
                                     out_strides, reduce);
}
extern "C" int spiht_dequant_idwt_reduced_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H,
                                                    int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, uint16_t *d_img_out,
                                                    const int64_t *out_strides, int reduce) {
    return dequant_idwt_reduced_view(EL_U16, ctx, d_rec, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_img_out,
                                     out_strides, reduce);
}
extern "C" int spiht_dequant_idwt_reduced_batch_flt(spiht_ctx *ctx, int kind, const int32_t *d_rec, int64_t B, int64_t c,
                                                    int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, void *d_img_out,
                                                    const int64_t *out_strides, int reduce) {
    return dequant_idwt_reduced_view(el_of_kind(kind), ctx, d_rec, B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                                     d_img_out, out_strides, reduce);
}

extern "C" int spiht_decode_image_reduced_batch_f64(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                    const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                    int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, double *d_img_out, int32_t *d_rec, int reduce) {
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, dense_pic(d_img_out, EL_F64, true), d_rec, reduce);
}
static int decode_image_reduced_view(PicElem el, spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                     const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                                     int level, double q_scale, const double *channel_mults, void *d_img_out,
                                     const int64_t *out_strides, int32_t *d_rec, int reduce) {
    Pic out;
    CHK(reduced_pic(d_img_out, el, out_strides, 4, B, c, H, W, wavelet, mode, level, reduce, &out));
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, out, d_rec, reduce);
}
extern "C" int spiht_decode_image_reduced_batch_u8(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                   const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                   int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                   const double *channel_mults, uint8_t *d_img_out,
                                                   const int64_t *out_strides, int32_t *d_rec, int reduce) {
    return decode_image_reduced_view(EL_U8, ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                                     channel_mults, d_img_out, out_strides, d_rec, reduce);
}
extern "C" int spiht_decode_image_reduced_batch_u16(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                    const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                    int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, uint16_t *d_img_out,
                                                    const int64_t *out_strides, int32_t *d_rec, int reduce) {
    return decode_image_reduced_view(EL_U16, ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                                     channel_mults, d_img_out, out_strides, d_rec, reduce);
}
extern "C" int spiht_decode_image_reduced_batch_flt(spiht_ctx *ctx, int kind, const uint8_t *d_data, uint64_t slot_stride,
                                                    const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                    int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, void *d_img_out,
                                                    const int64_t *out_strides, int32_t *d_rec, int reduce) {
    return decode_image_reduced_view(el_of_kind(kind), ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level,
                                     q_scale, channel_mults, d_img_out, out_strides, d_rec, reduce);
}

extern "C" int spiht_decode_image_reduced_host_f64(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                                   int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                   const double *channel_mults, double *img_out, int reduce) {
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                             dense_pic(img_out, EL_F64, true), reduce);
}
static int decode_image_reduced_host_view(PicElem el, spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                          int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                          const double *channel_mults, void *img_out, const int64_t *strides, int reduce) {
    Pic out;
    CHK(reduced_pic(img_out, el, strides, 3, 1, c, H, W, wavelet, mode, level, reduce, &out));
    CHK(dense_chw_or_hwc(out));
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, out, reduce);
}
extern "C" int spiht_decode_image_reduced_host_u8(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                                  int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                  const double *channel_mults, uint8_t *img_out, const int64_t *strides,
                                                  int reduce) {
    return decode_image_reduced_host_view(EL_U8, ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, img_out,
                                          strides, reduce);
}
extern "C" int spiht_decode_image_reduced_host_u16(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                                   int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                   const double *channel_mults, uint16_t *img_out, const int64_t *strides,
                                                   int reduce) {
    return decode_image_reduced_host_view(EL_U16, ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, img_out,
                                          strides, reduce);
}
extern "C" int spiht_decode_image_reduced_host_flt(spiht_ctx *ctx, int kind, const uint8_t *data, uint64_t nbytes, uint8_t n,
                                                   int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                   double q_scale, const double *channel_mults, void *img_out,
                                                   const int64_t *strides, int reduce) {
    return decode_image_reduced_host_view(el_of_kind(kind), ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale,
                                          channel_mults, img_out, strides, reduce);
}

// float pixels: the conversion passes of the routes without a fused form (dwt_inverse: conv8; dwt_forward: k_px_to_f64), alone
extern "C" int spiht_convert_batch_flt(spiht_ctx *ctx, int kind, const double *d_in, int64_t B, int64_t c, int64_t rec_h,
                                       int64_t rec_w, int64_t H, int64_t W, void *d_out, const int64_t *out_strides) {
    if (!ctx || !d_in || !d_out || B < 0 || c < 1 || H < 1 || W < 1 || rec_h < H || rec_w < W) return SPIHT_ERR_ARG;
    if (rec_h > (1 << 24) || rec_w > (1 << 24) || (__int128)B * c >= ((__int128)1 << 31)) return SPIHT_ERR_TOO_LARGE;
    Pic out;
    CHK(view_pic(&out, d_out, el_of_kind(kind), true, out_strides, 4, B, c, H, W, PIC_EMPTY_OK));
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    const PxView px = out.view();
    LAUNCHCHK(spiht_launch_f64_to_px(d_in, (int)rec_h, (int)rec_w, &px, B, ctx->stream));
    return SPIHT_OK;
}
extern "C" int spiht_widen_batch_flt(spiht_ctx *ctx, int kind, const void *d_in, const int64_t *strides, int64_t B, int64_t c,
                                     int64_t H, int64_t W, double *d_out) {
    if (!ctx || !d_in || !d_out || B < 0 || c < 1 || H < 1 || W < 1) return SPIHT_ERR_ARG;
    if (H > (1 << 24) || W > (1 << 24) || (__int128)B * c >= ((__int128)1 << 31)) return SPIHT_ERR_TOO_LARGE;
    Pic in;
    CHK(view_pic(&in, d_in, el_of_kind(kind), false, strides, 4, B, c, H, W, PIC_EMPTY_OK));
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    const PxView px = in.view();
    LAUNCHCHK(spiht_launch_px_to_f64(&px, B, d_out, ctx->stream));
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// the two halves of each direction on their own, so a caller can run the HBM-bound half of one batch on one
// context while another context list-codes a different batch (bench.py)
// ------------------------------------------------------------------------------------------------
static int dwt_pyramid_batch(spiht_ctx *ctx, const Pic &in, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                             int level, double q_scale, const double *channel_mults, int32_t *d_coeffs, uint8_t *d_dmsb,
                             uint8_t *d_lmsb, uint32_t *d_maxabs) {
    if (!ctx || !in.p || !d_coeffs || !d_maxabs || (!d_dmsb) != (!d_lmsb)) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    if (!k.open(&st, ctx, B, c, H, W, wavelet, mode, level, true)) return st;
    CHK(k.enter(channel_mults));
    const Geom &g = k.g;
    HIPCHK(hipMemsetAsync(d_maxabs, 0, (size_t)B * 4, ctx->stream));
    return k.chunks([&](int64_t b0, int nb) -> int {
        int32_t *co = d_coeffs + (size_t)b0 * g.n;
        CHK(dwt_forward(ctx, k.at(in, b0), nb * (int)c, (int)c, k.ig, wavelet, mode, q_scale, k.d_mults, co, d_maxabs + b0));
        if (!d_dmsb) return SPIHT_OK;  // transform + max|coefficient| only: the pyramid is queued elsewhere (spiht_pyramid_batch_i32)
        StageTimer t(ctx, ST_PYRAMID);
        LAUNCHCHK(spiht_launch_pyramid(&g, nb, co, d_dmsb + (size_t)b0 * g.n, d_lmsb + (size_t)b0 * g.n, ctx->stream));
        return SPIHT_OK;
    });
}
extern "C" int spiht_dwt_pyramid_batch_f64(spiht_ctx *ctx, const double *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                                           int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                           int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb, uint32_t *d_maxabs) {
    return dwt_pyramid_batch(ctx, dense_pic(d_img, EL_F64), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs,
                             d_dmsb, d_lmsb, d_maxabs);
}
static int dwt_pyramid_view(PicElem el, spiht_ctx *ctx, const void *d_img, const int64_t *strides, int64_t B, int64_t c, int64_t H,
                            int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                            int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb, uint32_t *d_maxabs) {
    Pic in;
    CHK(view_pic(&in, d_img, el, false, strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return dwt_pyramid_batch(ctx, in, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs, d_dmsb, d_lmsb,
                             d_maxabs);
}
extern "C" int spiht_dwt_pyramid_batch_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                          int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                          const double *channel_mults, int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb,
                                          uint32_t *d_maxabs) {
    return dwt_pyramid_view(EL_U8, ctx, d_img, strides, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs, d_dmsb,
                            d_lmsb, d_maxabs);
}
extern "C" int spiht_dwt_pyramid_batch_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb,
                                           uint32_t *d_maxabs) {
    return dwt_pyramid_view(EL_U16, ctx, d_img, strides, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs, d_dmsb,
                            d_lmsb, d_maxabs);
}
extern "C" int spiht_dwt_pyramid_batch_flt(spiht_ctx *ctx, int kind, const void *d_img, const int64_t *strides, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb,
                                           uint32_t *d_maxabs) {
    return dwt_pyramid_view(el_of_kind(kind), ctx, d_img, strides, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs,
                            d_dmsb, d_lmsb, d_maxabs);
}
