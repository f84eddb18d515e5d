// C ABI of libspiht_hip.so (include/spiht_hip.h), the transform side: wavelet and mode ids, the geometry of an image and of its
// reduced forms with the calls that report them, the check of a view by byte strides, the forward and inverse transform drivers
// and the set-up of an image call (ImgCall).  The image calls built on these are api_image.cpp; the rest of the host side is
// api_tiles.cpp, api_rd.cpp, api_ctx.cpp (context), api_coder.cpp (int32 calls), api_comm.cpp (RCCL) and hoststream.cpp.
#include "api_internal.h"
#include "wavelets.h"

static int dwt_max_level(int64_t len, int F) {  // pywt common.c dwt_max_level
    if (F <= 1 || len < F - 1) return 0;
    int64_t q = len / (F - 1);
    int l = 0;
    while (q > 1) { q >>= 1; l++; }
    return l;
}

// mode: only periodization changes the geometry (pywt.dwt_coeff_len); the level count follows the real filter length whatever
// the mode (pywt.dwt_max_level knows none)
int img_geometry(int64_t H, int64_t W, int F_real, int level, ImgGeom *g, int mode) {
    if (H < 1 || W < 1) return SPIHT_ERR_ARG;
    int L = level;
    if (L < 0) L = std::min(dwt_max_level(H, F_real), dwt_max_level(W, F_real));
    if (L > SPIHT_MAX_LEVELS) return SPIHT_ERR_ARG;
    g->per = mode == SPIHT_MODE_PERIODIZATION;
    g->l0 = 0;
    const int F = g->per ? 2 : F_real;
    g->L = L;
    g->hs[0] = H;
    g->ws[0] = W;
    for (int l = 1; l <= L; l++) {
        g->hs[l] = (g->hs[l - 1] + F - 1) / 2;
        g->ws[l] = (g->ws[l - 1] + F - 1) / 2;
    }
    g->ll_h = g->hs[L];
    g->ll_w = g->ws[L];
    int64_t ah = g->ll_h, aw = g->ll_w;
    for (int l = L; l >= 1; l--) {
        g->offh[l] = ah;
        g->offw[l] = aw;
        ah += g->hs[l];
        aw += g->ws[l];
    }
    g->enc_h = ah;
    g->enc_w = aw;
    int64_t rh = g->ll_h, rw = g->ll_w;
    for (int l = L; l >= 1; l--) {
        rh = 2 * g->hs[l] - F + 2;
        rw = 2 * g->ws[l] - F + 2;
    }
    g->rec_H = rh;
    g->rec_W = rw;
    return SPIHT_OK;
}

// Reduced-resolution decode: the geometry that makes the picture of pyramid level k (hs[k] x ws[k], 1/2^k size) out of
// the SAME packed array.  The top-left corner of the array is itself the packed array of that picture at L - k levels --
// same root block, same detail blocks at the same offsets -- so the geometry is ig with its k finest levels dropped and
// the levels renumbered; enc_h / enc_w stay the full array's (they are the strides the kernels address it with).  The
// inverse transform run on it stops at level k + 1 of the stream: that level is "level 1" to everything that makes a
// picture (integer store, colour change, conversion pass).  rec_H x rec_W: what waverec2 returns for coeffs[:L - k + 1],
// the root block itself for k == L.  F: the length rule's filter length (2 under periodization).
static int reduced_geometry(const ImgGeom &ig, int F_real, int k, ImgGeom *r) {
    if (k < 0 || k > ig.L) return SPIHT_ERR_ARG;
    const int F = ig.per ? 2 : F_real;
    *r = ig;
    r->L = ig.L - k;
    r->l0 = ig.l0 + k;
    for (int l = 0; l <= r->L; l++) {
        r->hs[l] = ig.hs[l + k]; r->ws[l] = ig.ws[l + k];
        r->offh[l] = ig.offh[l + k]; r->offw[l] = ig.offw[l + k];  // ([0] is never read)
    }
    r->rec_H = r->L ? 2 * r->hs[1] - F + 2 : ig.ll_h;
    r->rec_W = r->L ? 2 * r->ws[1] - F + 2 : ig.ll_w;
    return SPIHT_OK;
}
// The quantisation scale of a reduced decode.  The approximation band carries a DC gain of 2 per level; R_k takes it out:
// waverec2(coeffs[:L - k + 1]) * 2^-k.  Dividing by q * 2^k instead of q scales every dequantised value by exactly 2^-k, and
// IEEE division, products and sums commute with a power of two (no subnormals in reach: |rec| >= 1, k <= SPIHT_MAX_LEVELS,
// q an ordinary number) -- so no kernel multiplies by a gain: the levels run as they are with this q.
static int reduced_q(double q, int k, double *qk) {
    *qk = k ? ldexp(q, k) : q;
    if (k && !(std::isfinite(*qk) && std::isfinite(q))) return SPIHT_ERR_ARG;  // (q * 2^k overflows)
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// wavelet and mode ids, the geometry as the callers see it
// ------------------------------------------------------------------------------------------------

extern "C" int spiht_wavelet_id(const char *name) {
    if (!name) return -1;
    for (int i = 0; i < SPIHT_NWAVELETS; i++)
        if (!strcmp(SPIHT_WAVELETS[i].name, name)) return i;
    if (!strcmp(name, "db1")) return spiht_wavelet_id("haar");
    return -1;
}
// filter length of a wavelet of the table (pywt.Wavelet(name).dec_len); < 0: no such id
extern "C" int spiht_wavelet_taps(int wavelet) {
    return (wavelet >= 0 && wavelet < SPIHT_NWAVELETS) ? SPIHT_WAVELETS[wavelet].F : -1;
}
extern "C" int spiht_mode_id(const char *name) {
    if (!name) return -1;
    static const char *names[] = {"reflect", "symmetric", "periodic", "zero", "constant", "smooth", "antisymmetric", "antireflect",
                                  "periodization"};
    for (int i = 0; i < 9; i++)
        if (!strcmp(names[i], name)) return i;
    return -1;
}

extern "C" int spiht_geometry(int64_t H, int64_t W, int wavelet, int level, int *level_used, int64_t *ll_h,
                              int64_t *ll_w, int64_t *enc_h, int64_t *enc_w, int64_t *rec_H, int64_t *rec_W) {
    return spiht_geometry_mode(H, W, wavelet, SPIHT_MODE_REFLECT, level, level_used, ll_h, ll_w, enc_h, enc_w, rec_H, rec_W);
}
extern "C" int spiht_geometry_mode(int64_t H, int64_t W, int wavelet, int mode, int level, int *level_used, int64_t *ll_h,
                                   int64_t *ll_w, int64_t *enc_h, int64_t *enc_w, int64_t *rec_H, int64_t *rec_W) {
    if (wavelet < 0 || wavelet >= SPIHT_NWAVELETS || mode < 0 || mode > SPIHT_MODE_PERIODIZATION) return SPIHT_ERR_ARG;
    ImgGeom ig;
    CHK(img_geometry(H, W, SPIHT_WAVELETS[wavelet].F, level, &ig, mode));
    if (level_used) *level_used = ig.L;
    if (ll_h) *ll_h = ig.ll_h;
    if (ll_w) *ll_w = ig.ll_w;
    if (enc_h) *enc_h = ig.enc_h;
    if (enc_w) *enc_w = ig.enc_w;
    if (rec_H) *rec_H = ig.rec_H;
    if (rec_W) *rec_W = ig.rec_W;
    return SPIHT_OK;
}
// the approximation level 1 of the two-part inverse starts from (spiht_idwt_coarse_batch_f64); 0 x 0 with fewer than two levels
extern "C" int spiht_idwt_approx_shape(int64_t H, int64_t W, int wavelet, int level, int64_t *a_h, int64_t *a_w) {
    if (wavelet < 0 || wavelet >= SPIHT_NWAVELETS || !a_h || !a_w) return SPIHT_ERR_ARG;
    ImgGeom ig;
    const int F = SPIHT_WAVELETS[wavelet].F;
    CHK(img_geometry(H, W, F, level, &ig));
    *a_h = ig.L >= 2 ? 2 * ig.hs[2] - F + 2 : 0;
    *a_w = ig.L >= 2 ? 2 * ig.ws[2] - F + 2 : 0;
    return SPIHT_OK;
}
int reduced_open(int64_t H, int64_t W, int wavelet, int mode, int level, int reduce, ImgGeom *ig, ImgGeom *pig) {
    if (wavelet < 0 || wavelet >= SPIHT_NWAVELETS || mode < 0 || mode > SPIHT_MODE_PERIODIZATION) return SPIHT_ERR_ARG;
    CHK(img_geometry(H, W, SPIHT_WAVELETS[wavelet].F, level, ig, mode));
    return reduced_geometry(*ig, SPIHT_WAVELETS[wavelet].F, reduce, pig);
}
extern "C" int spiht_reduced_shape(int64_t H, int64_t W, int wavelet, int mode, int level, int reduce, int *level_used,
                                   int64_t *rec_h, int64_t *rec_w, int64_t *pic_h, int64_t *pic_w, int64_t *off_y,
                                   int64_t *off_x, int64_t *in_h, int64_t *in_w) {
    ImgGeom ig, pig;
    CHK(reduced_open(H, W, wavelet, mode, level, reduce, &ig, &pig));
    const int64_t ih = (H + ((int64_t)1 << reduce) - 1) >> reduce, iw = (W + ((int64_t)1 << reduce) - 1) >> reduce;
    if (level_used) *level_used = ig.L;
    if (rec_h) *rec_h = pig.rec_H;
    if (rec_w) *rec_w = pig.rec_W;
    if (pic_h) *pic_h = pig.hs[0];
    if (pic_w) *pic_w = pig.ws[0];
    if (off_y) *off_y = ig.per ? 0 : (pig.hs[0] - ih) / 2;
    if (off_x) *off_x = ig.per ? 0 : (pig.ws[0] - iw) / 2;
    if (in_h) *in_h = ih;
    if (in_w) *in_w = iw;
    return SPIHT_OK;
}

static int upload_mults(spiht_ctx *ctx, const double *channel_mults, int64_t c, const double **d_mults) {
    *d_mults = nullptr;
    if (!channel_mults) return SPIHT_OK;
    // the same scales as last time (every call of a codec object): nothing to upload, nothing to wait for
    if (ctx->mults.p && ctx->mults_host.size() == (size_t)c && !memcmp(ctx->mults_host.data(), channel_mults, (size_t)c * 8)) {
        *d_mults = (const double *)ctx->mults.p;
        return SPIHT_OK;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));  // queued kernels still read the old scales
    ctx->mults_host.clear();
    CHK(ensure(ctx, ctx->mults, (size_t)c * 8));
    HIPCHK(hipMemcpyAsync(ctx->mults.p, channel_mults, (size_t)c * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // caller's array may be a temporary
    ctx->mults_host.assign(channel_mults, channel_mults + c);
    *d_mults = (const double *)ctx->mults.p;
    return SPIHT_OK;
}

// The wavelet's filters on the device for the two-pass levels: dec_lo, dec_hi, rec_lo, rec_hi (F doubles each), then dec_lo,
// dec_hi as the single-precision transform has them (F floats each).  Uploaded when the wavelet changes.
static int upload_filters(spiht_ctx *ctx, int wavelet, const double **d_filt) {
    const WaveletDef &wv = SPIHT_WAVELETS[wavelet];
    const size_t F = (size_t)wv.F, bytes = 4 * F * 8 + 2 * F * 4;
    if (ctx->filt_wavelet != wavelet || !ctx->filt.p) {
        HIPCHK(hipStreamSynchronize(ctx->stream));  // queued kernels still read the old filters
        ctx->filt_wavelet = -1;
        CHK(ensure(ctx, ctx->filt, bytes));
        std::vector<char> h(bytes);
        memcpy(h.data(), wv.dec_lo, F * 8);
        memcpy(h.data() + F * 8, wv.dec_hi, F * 8);
        memcpy(h.data() + 2 * F * 8, wv.rec_lo, F * 8);
        memcpy(h.data() + 3 * F * 8, wv.rec_hi, F * 8);
        memcpy(h.data() + 4 * F * 8, wv.dec_lo_f, F * 4);
        memcpy(h.data() + 4 * F * 8 + F * 4, wv.dec_hi_f, F * 4);
        HIPCHK(hipMemcpyAsync(ctx->filt.p, h.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));  // (h is a temporary)
        ctx->filt_wavelet = wavelet;
    }
    *d_filt = (const double *)ctx->filt.p;
    return SPIHT_OK;
}

// ---- the pictures of an image call (api_internal.h: Pic) ------------------------------------------------------------------------
int check_img_args(int wavelet, int mode, int64_t B, int64_t c, int64_t H, int64_t W) {
    if (wavelet < 0 || wavelet >= SPIHT_NWAVELETS || mode < 0 || mode > SPIHT_MODE_PERIODIZATION) return SPIHT_ERR_ARG;
    if (B < 0 || c < 1 || H < 1 || W < 1) return SPIHT_ERR_ARG;
    if (H > (1 << 24) || W > (1 << 24)) return SPIHT_ERR_TOO_LARGE;
    // one picture is never split: batch_chunks hands all its c planes to one launch, and the launchers put the planes of a
    // launch into grid.y / grid.z (k_dwt_edge, k_zero_pads, k_pyr_ll, k_ll_to_pic), which end at 65535
    if (c > 65535) return SPIHT_ERR_TOO_LARGE;
    return SPIHT_OK;
}

// the one builder of a view by strides (api_internal.h); a float kind obeys the rules of the integer kinds, read or written
int view_pic(Pic *v, const void *p, PicElem el, bool out, const int64_t *strides, int n, int64_t B, int64_t c, int64_t h,
             int64_t w, int rules, int wavelet, int mode) {
    if ((rules & PIC_NULL_FIRST) && !p) return SPIHT_ERR_ARG;
    if (rules & PIC_IMG_ARGS) CHK(check_img_args(wavelet, mode, B, c, h, w));
    if (rules & PIC_EMPTY_OK) B = std::max<int64_t>(B, 1);
    const int es = el_size(el);
    if (es < 1) return SPIHT_ERR_ARG;
    int64_t st[4] = {c * h * w * es, h * w * es, w * es, es};
    if (strides)
        for (int i = 0; i < n; i++) st[4 - n + i] = strides[i];
    if (n == 3) st[0] = 0;  // (one picture: no batch stride)
    const int64_t ext[4] = {B, c, h, w};
    __int128 span = es;
    if ((uintptr_t)p % (uintptr_t)es != 0) return SPIHT_ERR_ARG;
    for (int i = 0; i < 4; i++) {
        if (st[i] < 0 || st[i] % es != 0) return SPIHT_ERR_ARG;
        if (ext[i] > 1) span += (__int128)(ext[i] - 1) * st[i];
    }
    if (span >= ((__int128)1 << 62)) return SPIHT_ERR_ARG;
    if (out) {  // sorted by stride, every dimension longer than 1 must step past the last byte all the smaller ones reach
        int idx[4] = {0, 1, 2, 3};
        std::sort(idx, idx + 4, [&](int x, int y) { return st[x] < st[y]; });
        int64_t reach = 0;
        for (int k = 0; k < 4; k++) {
            const int i = idx[k];
            if (ext[i] <= 1) continue;
            if (st[i] < reach + es) return SPIHT_ERR_ARG;
            reach += (ext[i] - 1) * st[i];
        }
    }
    *v = dense_pic(p, el, out);
    v->strided = true;
    v->px.sb = st[0]; v->px.sc = st[1]; v->px.sh = st[2]; v->px.sw = st[3];
    v->px.c = (int32_t)c; v->px.h = (int32_t)h; v->px.w = (int32_t)w;
    return SPIHT_OK;
}
// (a view that is read obeys the same rules without the overlap check)
int check_view(PicElem el, int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output) {
    if (B < 1 || c < 1 || H < 1 || W < 1 || !strides) return SPIHT_ERR_ARG;
    Pic v;
    return view_pic(&v, nullptr, el, output != 0, strides, 4, B, c, H, W);
}
extern "C" int spiht_check_view_u8(int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output) {
    return check_view(EL_U8, B, c, H, W, strides, output);
}
extern "C" int spiht_check_view_u16(int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output) {
    return check_view(EL_U16, B, c, H, W, strides, output);
}
extern "C" int spiht_check_view_flt(int kind, int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output) {
    return check_view(el_of_kind(kind), B, c, H, W, strides, output);
}

// pictures `in` (planes / c of them) -> quantised packed array [planes, enc_h, enc_w].  The rules of the pixel formats:
// float32 pixels are transformed in single precision, as PyWavelets does for float32 / float16 input (every level's input
// must then be at least as long as the filter: SPIHT_ERR_ARG otherwise), at a level >= 1 and without the colour model.
// 8- and 16-bit pixels need a level >= 1 (no entry point gets here with level 0: SPIHT refuses that geometry -- the root block's
// offspring fall outside the array -- before anything is transformed, on the float64 path as well); the tiled level 1
// reads them itself, the two-pass levels get their float64 form from a conversion pass first.  Float pixels in (EL_FLT_*) go
// the integer kinds' way in everything: the same view, the same two routes; their conversion is the exact widening.
int dwt_forward(spiht_ctx *ctx, const Pic &in, int planes, int c, const ImgGeom &ig, int wavelet, int mode, double q,
                const double *d_mults, int32_t *d_coeffs, uint32_t *d_maxabs) {
    const WaveletDef &wv = SPIHT_WAVELETS[wavelet];
    const size_t plane_out = (size_t)ig.enc_h * ig.enc_w;
    const bool f32 = in.el == EL_F32;
    bool strided = in.strided, color = ctx->color_on && c == 3;  // (strided: level 1 reads the view itself)
    if ((f32 || strided) && ig.L == 0) return SPIHT_ERR_ARG;
    if (color && f32) return SPIHT_ERR_ARG;  // the colour model change is float64 (as colour-science's)
    // the plain two-pass level: the modes that compute their extension, periodization, and filters longer than the tiled
    // kernels take (db11.., sym11.., coif4.., dmey)
    const bool twopass = mode >= SPIHT_MODE_SMOOTH || wv.F > SPIHT_MAX_TAPS;
    const double *d_img = strided ? nullptr : (const double *)in.p;
    if (strided && twopass) {  // no strided form of the two-pass level: the float64 picture as a pass of its own
        StageTimer t(ctx, ST_DWT_L1);
        CHK(ensure(ctx, ctx->pix, (size_t)planes * ig.hs[0] * ig.ws[0] * 8));
        const PxView px = in.view();
        LAUNCHCHK(spiht_launch_px_to_f64(&px, planes / c, (double *)ctx->pix.p, ctx->stream));
        d_img = (const double *)ctx->pix.p;
        strided = false;
    }
    const double *d_filt = nullptr;
    if (twopass && ig.L > 0) CHK(upload_filters(ctx, wavelet, &d_filt));
    if (color && twopass && ig.L > 0) {
        // the two-pass level has no colour form: the colour model change as a pass of its own in front of it
        const size_t npix = (size_t)ig.hs[0] * ig.ws[0];
        CHK(ensure(ctx, ctx->img, (size_t)planes * npix * 8));
        LAUNCHCHK(spiht_launch_color3(d_img, (double *)ctx->img.p, planes / 3, npix, ctx->col_fwd.A, ctx->col_fwd.M, ctx->col_fwd.p,
                                      ctx->stream));
        d_img = (const double *)ctx->img.p;
        color = false;
    }
    if (ig.L == 0) {
        StageTimer t(ctx, ST_DWT_REST);
        if (color) {  // no transform level to carry the colour model change: a pass of its own
            CHK(ensure(ctx, ctx->a0, (size_t)planes * plane_out * 8));
            LAUNCHCHK(spiht_launch_color3(d_img, (double *)ctx->a0.p, planes / 3, plane_out, ctx->col_fwd.A, ctx->col_fwd.M,
                                          ctx->col_fwd.p, ctx->stream));
            d_img = (const double *)ctx->a0.p;
        }
        LAUNCHCHK(spiht_launch_quant_plain(d_img, d_coeffs, plane_out, planes, c, d_mults, q, d_maxabs, ctx->stream));
        return SPIHT_OK;
    }
    // zero padding cells of coeffs_to_array (thin strips; every other cell is written by a band).  The transform writes
    // band cells only, so an array it has filled once for this geometry still has its zeros the next time -- PROVIDED
    // nobody else writes into it: a caller that owns its arrays says so (option "pads_persist": the pipeline's
    // double-buffered arrays; beside a list decoder this launch of thin strips took 0.74 instead of 0.12 ms per step).
    bool pads_known = false;
    // (the mode belongs to the key: periodization packs the bands by another length rule, i.e. other strips)
    const spiht_ctx::PadKey key = {d_coeffs, planes, ig.hs[0], ig.ws[0], wv.F, ig.L, mode == SPIHT_MODE_PERIODIZATION ? 1 : 0};
    if (ctx->opt_pads_persist)
        for (const auto &k : ctx->pads_zeroed)
            pads_known = pads_known || (k.p == key.p && k.planes == key.planes && k.H == key.H && k.W == key.W && k.F == key.F && k.L == key.L &&
                                        k.mode == key.mode);
    if (!pads_known) {
        StageTimer t(ctx, ST_MEMSET);
        LAUNCHCHK(spiht_launch_zero_pads(ig.L, ig.hs, ig.ws, ig.offh, ig.offw, (int)ig.enc_h, (int)ig.enc_w, d_coeffs, planes,
                                         ctx->stream));
        // (an array seen with another geometry before has other strips: forget it -- whether or not this call may rely
        // on the promise, so that a later one that does never finds a record older than the array's last layout)
        auto &v = ctx->pads_zeroed;
        v.erase(std::remove_if(v.begin(), v.end(), [&](const spiht_ctx::PadKey &k) { return k.p == key.p; }), v.end());
        if (ctx->opt_pads_persist) {
            if (v.size() >= 8) v.erase(v.begin());
            v.push_back(key);
        }
    }
    if (ig.L >= 2) {
        CHK(ensure(ctx, ctx->a0, (size_t)planes * ig.hs[1] * ig.ws[1] * 8));
        if (ig.L >= 3) CHK(ensure(ctx, ctx->a1, (size_t)planes * ig.hs[2] * ig.ws[2] * 8));
    }
    for (int l = 1; l <= ig.L; l++) {  // (d_img: the level's input)
        DwtKArgs a;
        memset(&a, 0, sizeof(a));
        a.c = c;
        a.F = wv.F;
        a.mode = mode;
        a.in_h = (int32_t)ig.hs[l - 1]; a.in_w = (int32_t)ig.ws[l - 1];
        a.out_h = (int32_t)ig.hs[l]; a.out_w = (int32_t)ig.ws[l];
        a.off_h = (int32_t)ig.offh[l]; a.off_w = (int32_t)ig.offw[l];
        a.enc_h = (int32_t)ig.enc_h; a.enc_w = (int32_t)ig.enc_w;
        a.last = (l == ig.L) ? 1 : 0;
        a.f32 = f32 ? 1 : 0;
        a.in = d_img;
        a.ll_out = a.last ? nullptr : (double *)((l & 1) ? ctx->a0.p : ctx->a1.p);
        a.coeffs = d_coeffs;
        a.mults = d_mults;
        a.maxabs = d_maxabs;
        a.q = q;
        if (color && l == 1) { a.color = 1; a.col = ctx->col_fwd; }
        if (strided && l == 1) a.px = in.view();  // (the launcher takes the kernels of its pixel kind)
        const int Fc = std::min(wv.F, SPIHT_MAX_TAPS);  // (a longer filter goes by the device copy: two-pass level)
        memcpy(a.lo, wv.dec_lo, sizeof(double) * Fc);
        memcpy(a.hi, wv.dec_hi, sizeof(double) * Fc);
        memcpy(a.lo_f, wv.dec_lo_f, sizeof(float) * Fc);
        memcpy(a.hi_f, wv.dec_hi_f, sizeof(float) * Fc);
        if (twopass) {
            // smooth / antisymmetric / antireflect / periodization / long filters: two plain passes through an intermediate (dwt_plain.hip:
            // k_dwt_axis_ext), a few planes at a time so that the intermediates stay under a gigabyte; in the pixels' precision
            StageTimer t(ctx, l == 1 ? ST_DWT_L1 : ST_DWT_REST);
            const size_t esz = f32 ? 4 : 8;
            const size_t n_t = (size_t)a.out_h * a.in_w, n_b = (size_t)a.out_h * a.out_w;  // elements per plane
            const size_t per_plane = (2 * n_t + 4 * n_b) * esz;
            int pc = (int)std::max<size_t>(1, ((size_t)1 << 30) / per_plane);
            pc = std::max(c, pc / c * c);  // whole images: the max|coefficient| word and the channel scale go by plane / c, plane % c
            CHK(ensure(ctx, ctx->exttmp, per_plane * (size_t)std::min(pc, planes)));
            for (int p0 = 0; p0 < planes; p0 += pc) {
                const int np = std::min(pc, planes - p0);
                DwtKArgs b = a;
                b.in = (const double *)((const char *)a.in + (size_t)p0 * a.in_h * a.in_w * esz);
                if (b.ll_out) b.ll_out = (double *)((char *)a.ll_out + (size_t)p0 * n_b * esz);
                b.coeffs = a.coeffs + (size_t)p0 * a.enc_h * a.enc_w;
                if (b.maxabs) b.maxabs = a.maxabs + p0 / c;
                char *base = (char *)ctx->exttmp.p;
                void *t_lo = base, *t_hi = base + (size_t)np * n_t * esz;
                char *bb = base + 2 * (size_t)np * n_t * esz;
                LAUNCHCHK(spiht_launch_dwt_level_ext(&b, np, t_lo, t_hi, bb, bb + (size_t)np * n_b * esz, bb + 2 * (size_t)np * n_b * esz,
                                                     bb + 3 * (size_t)np * n_b * esz, d_filt, ctx->stream));
            }
        } else {
            StageTimer t(ctx, l == 1 ? ST_DWT_L1 : ST_DWT_REST);
            LAUNCHCHK(spiht_launch_dwt_level(&a, planes, ctx->stream));
        }
        d_img = a.ll_out;
    }
    return SPIHT_OK;
}

// Geometry of the L1Flags words of an image geometry (common.h): false when they do not apply (fewer than two levels: the
// level-1 approximation then comes out of the packed array too; a filter whose halo exceeds a tile)
bool l1flags_geometry(const ImgGeom &ig, int F, L1Flags *fl) {
    memset(fl, 0, sizeof(*fl));
    if (ig.per) return false;  // (periodization runs the plain two-pass inverse: no tiles)
    if (ig.L < 2 || F / 2 - 1 > IW_TH / 2 || F / 2 - 1 > IW_TW / 2) return false;
    fl->off_h = (int32_t)ig.offh[1]; fl->off_w = (int32_t)ig.offw[1];
    fl->band_h = (int32_t)ig.hs[1]; fl->band_w = (int32_t)ig.ws[1];
    fl->hf1 = F / 2 - 1;
    fl->gx = (int32_t)((2 * ig.ws[1] - F + 2 + IW_TW - 1) / IW_TW);
    fl->gy = (int32_t)((2 * ig.hs[1] - F + 2 + IW_TH - 1) / IW_TH);
    return fl->gx > 0 && fl->gy > 0;
}
// Size, in 32-bit words per image, of the occupancy words the decoder leaves for the inverse transform's level 1
// (common.h: L1Flags): 0 when they do not apply to this geometry (fewer than two levels).
extern "C" int spiht_l1_flags_words(int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, uint64_t *words_per_image) {
    if (!words_per_image || wavelet < 0 || wavelet >= SPIHT_NWAVELETS || c < 1 || mode < 0 || mode > SPIHT_MODE_PERIODIZATION)
        return SPIHT_ERR_ARG;
    ImgGeom ig;
    CHK(img_geometry(H, W, SPIHT_WAVELETS[wavelet].F, level, &ig, mode));
    L1Flags fl;
    *words_per_image = l1flags_geometry(ig, SPIHT_WAVELETS[wavelet].F, &fl) ? (uint64_t)c * fl.gy * fl.gx : 0;
    return SPIHT_OK;
}

// packed int32 array -> pixels [planes, rec_H, rec_W]
// l_hi .. l_lo: the levels to run, coarsest first (ig.L .. 1 = all).  A run that stops above level 1 leaves its last
// approximation in d_out ([planes, 2*hs[l_lo]-F+2, 2*ws[l_lo]-F+2]); a run that starts below ig.L takes that array as d_a_in.
// d_flags: L1Flags words [planes, gy, gx] the decoder of d_rec left (nullptr: every level-1 tile reads its detail bands)
// d_rows: their row words (nullptr: a tile whose word is set reads every row)
// 8- / 16-bit output (l_lo == 1, a level >= 1: see dwt_forward): cropped to the picture's size; the tiled level 1 writes it
// itself, the two-pass level goes through a conversion pass behind it.
// A reduced geometry (reduced_geometry: ig.l0 = k levels dropped) runs the same way: its level 1 is level k + 1 of the
// stream and makes the picture of that size -- integer store, crop, colour change, conversion pass; also as the coarsest
// level (l == ig.L) -- and q is the caller's q * 2^k (reduced_q).  No d_flags then: the words belong to the stream's level 1.
int dwt_inverse(spiht_ctx *ctx, const int32_t *d_rec, int planes, int c, const ImgGeom &ig, int wavelet, double q,
                const double *d_mults, const Pic &out, int l_hi, int l_lo, const double *d_a_in, const uint32_t *d_flags,
                const uint32_t *d_rows) {
    const WaveletDef &wv = SPIHT_WAVELETS[wavelet];
    const int F = wv.F;
    if (l_hi < 0) l_hi = ig.L;
    const bool strided = out.strided;  // (level 1 writes the view itself, or a conversion pass behind it does)
    if (strided && (l_lo != 1 || (ig.L == 0 && ig.l0 == 0))) return SPIHT_ERR_ARG;
    double *d_out = strided ? nullptr : (double *)out.p;
    const bool color = ctx->color_on && c == 3;
    if (ig.L == 0 && ig.l0 > 0) {  // a reduced decode down to the root block: the window of the array, as the picture
        StageTimer t(ctx, ST_IDWT_REST);
        LlPicArgs a;
        memset(&a, 0, sizeof(a));
        a.rec = d_rec;
        a.enc_h = (int32_t)ig.enc_h; a.enc_w = (int32_t)ig.enc_w; a.ll_h = (int32_t)ig.ll_h; a.ll_w = (int32_t)ig.ll_w;
        a.c = c; a.mults = d_mults; a.q = q; a.out = d_out;
        if (color) { a.color = 1; a.col = ctx->col_inv; }
        if (strided) a.px = out.view();
        LAUNCHCHK(spiht_launch_ll_to_pic(&a, planes, ctx->stream));
        return SPIHT_OK;
    }
    if (ig.L == 0) {
        StageTimer t(ctx, ST_IDWT_REST);
        LAUNCHCHK(spiht_launch_dequant_plain(d_rec, d_out, (size_t)ig.enc_h * ig.enc_w, planes, c, d_mults, q, ctx->stream));
        if (color)
            LAUNCHCHK(spiht_launch_color3(d_out, d_out, planes / 3, (size_t)ig.enc_h * ig.enc_w, ctx->col_inv.A, ctx->col_inv.M,
                                          ctx->col_inv.p, ctx->stream));
        return SPIHT_OK;
    }
    // intermediate approximations ping-pong between a0/a1; sizes 2*band-F+2
    size_t maxa = 0;
    const int Fg = ig.per ? 2 : F;  // (the length rule's filter length: periodization gives back 2 n samples)
    for (int l = l_hi; l > l_lo; l--) maxa = std::max(maxa, (size_t)(2 * ig.hs[l] - Fg + 2) * (size_t)(2 * ig.ws[l] - Fg + 2));
    if (maxa) {
        CHK(ensure(ctx, ctx->a0, maxa * planes * 8));
        CHK(ensure(ctx, ctx->a1, maxa * planes * 8));
    }
    const double *a_in = d_a_in;
    int64_t ah = ig.ll_h, aw = ig.ll_w;
    if (l_hi < ig.L) { ah = 2 * ig.hs[l_hi + 1] - Fg + 2; aw = 2 * ig.ws[l_hi + 1] - Fg + 2; }
    for (int l = l_hi; l >= l_lo; l--) {
        IdwtKArgs a;
        memset(&a, 0, sizeof(a));
        a.c = c;
        a.F = F;
        a.band_h = (int32_t)ig.hs[l]; a.band_w = (int32_t)ig.ws[l];
        a.out_h = (int32_t)(2 * ig.hs[l] - F + 2); a.out_w = (int32_t)(2 * ig.ws[l] - F + 2);
        a.a_h = (int32_t)ah; a.a_w = (int32_t)aw;
        // waverec2 trim rule: the running approximation may be exactly one longer than the band
        if (!((ah == ig.hs[l] || ah == ig.hs[l] + 1) && (aw == ig.ws[l] || aw == ig.ws[l] + 1))) return SPIHT_ERR_ARG;
        if (ig.per) { a.out_h = (int32_t)(2 * ig.hs[l]); a.out_w = (int32_t)(2 * ig.ws[l]); }
        a.off_h = (int32_t)ig.offh[l]; a.off_w = (int32_t)ig.offw[l];
        a.enc_h = (int32_t)ig.enc_h; a.enc_w = (int32_t)ig.enc_w;
        a.first = (l == ig.L) ? 1 : 0;
        a.a_in = a_in;
        a.rec = d_rec;
        a.out = (l == l_lo) ? d_out : (double *)((l & 1) ? ctx->a1.p : ctx->a0.p);
        a.mults = d_mults;
        a.q = q;
        if (color && l == 1) { a.color = 1; a.col = ctx->col_inv; }
        if (l == 1 && !a.first && !a.color) { a.flags = d_flags; a.rows = d_flags ? d_rows : nullptr; }
        memcpy(a.lo, wv.rec_lo, sizeof(double) * std::min(F, SPIHT_MAX_TAPS));
        memcpy(a.hi, wv.rec_hi, sizeof(double) * std::min(F, SPIHT_MAX_TAPS));
        const bool conv8 = strided && l == 1 && (ig.per || F > SPIHT_MAX_TAPS);  // a view's output through a pass of its own
        if (conv8) {
            CHK(ensure(ctx, ctx->pix, (size_t)planes * a.out_h * a.out_w * 8));
            a.out = (double *)ctx->pix.p;
        }
        if (ig.per || F > SPIHT_MAX_TAPS) {
            // periodization / a filter longer than the tiled kernels take: two plain passes through an intermediate (dwt_plain.hip:
            // k_idwt_axis_per), a few planes at a time; the colour model of the picture as a pass of its own behind level 1
            const double *d_filt;
            CHK(upload_filters(ctx, wavelet, &d_filt));
            StageTimer t(ctx, l + ig.l0 == 1 ? ST_IDWT_L1 : ST_IDWT_REST);
            a.color = 0;
            const size_t per_plane = (size_t)2 * a.band_h * a.out_w * 8;
            int pc = (int)std::max<size_t>(1, ((size_t)1 << 30) / per_plane);
            pc = std::max(c, pc / c * c);
            CHK(ensure(ctx, ctx->exttmp, per_plane * (size_t)std::min(pc, planes)));
            for (int p0 = 0; p0 < planes; p0 += pc) {
                const int np = std::min(pc, planes - p0);
                IdwtKArgs b = a;
                if (b.a_in) b.a_in = a.a_in + (size_t)p0 * a.a_h * a.a_w;
                b.rec = a.rec + (size_t)p0 * a.enc_h * a.enc_w;
                b.out = a.out + (size_t)p0 * a.out_h * a.out_w;
                double *t_lo = (double *)ctx->exttmp.p, *t_hi = t_lo + (size_t)np * a.band_h * a.out_w;
                LAUNCHCHK(spiht_launch_idwt_level_per(&b, np, t_lo, t_hi, d_filt, ig.per ? 1 : 0, ctx->stream));
            }
            if (color && l == 1)
                LAUNCHCHK(spiht_launch_color3(a.out, a.out, planes / 3, (size_t)a.out_h * a.out_w, ctx->col_inv.A, ctx->col_inv.M,
                                              ctx->col_inv.p, ctx->stream));
            if (conv8) {
                const PxView px = out.view();
                LAUNCHCHK(spiht_launch_f64_to_px(a.out, a.out_h, a.out_w, &px, planes / c, ctx->stream));
            }
        } else {
            if (strided && l == 1) a.px = out.view();  // (the launcher takes the kernels of its pixel kind)
            StageTimer t(ctx, l + ig.l0 == 1 ? ST_IDWT_L1 : ST_IDWT_REST);
            LAUNCHCHK(spiht_launch_idwt_level(&a, planes, ctx->stream, ctx->tilectr.dev ? &ctx->tilectr : nullptr));
        }
        a_in = a.out;
        ah = a.out_h;
        aw = a.out_w;
    }
    return SPIHT_OK;
}

// ImgCall (api_internal.h): the set-up of an image call
bool ImgCall::open(int *st, spiht_ctx *ctx_, int64_t B_, int64_t c_, int64_t H, int64_t W, int wavelet, int mode, int level, bool coded) {
    ctx = ctx_; B = B_; c = c_;
    *st = check_img_args(wavelet, mode, B, c, H, W);
    if (*st != SPIHT_OK || B == 0) return false;
    F = SPIHT_WAVELETS[wavelet].F;
    *st = img_geometry(H, W, F, level, &ig, mode);
    if (*st == SPIHT_OK && coded) *st = make_geom(c, ig.enc_h, ig.enc_w, ig.ll_h, ig.ll_w, &g);
    pig = ig;
    return *st == SPIHT_OK;
}
bool ImgCall::reduce(int *st, int k, double q_scale) {
    q = q_scale;
    if (k == 0) return true;
    *st = reduced_geometry(ig, F, k, &pig);
    if (*st == SPIHT_OK) *st = reduced_q(q_scale, k, &q);
    return *st == SPIHT_OK;
}
int ImgCall::enter(const double *channel_mults) {
    lk = std::unique_lock<std::recursive_mutex>(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    return upload_mults(ctx, channel_mults, c, &d_mults);
}

