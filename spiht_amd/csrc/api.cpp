// C ABI of libspiht_hip.so (include/spiht_hip.h), the image calls: wavelets and the geometry of an image, the forward and
// inverse transform drivers, and every image call -- batched, reduced, on host arrays -- for every pixel format; the
// rate-distortion reductions; tiled pictures.  The rest of the host side is api_ctx.cpp (context), api_coder.cpp (int32 calls)
// and api_comm.cpp (RCCL); api_internal.h holds what the four files share.
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
static int img_geometry(int64_t H, int64_t W, int F_real, int level, ImgGeom *g, int mode = SPIHT_MODE_REFLECT) {
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
// image path
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

extern "C" int spiht_geometry_mode(int64_t H, int64_t W, int wavelet, int mode, int level, int *level_used, int64_t *ll_h,
                                   int64_t *ll_w, int64_t *enc_h, int64_t *enc_w, int64_t *rec_H, int64_t *rec_W);
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

// pixels [planes,H,W] -> quantised packed array [planes,enc_h,enc_w]
// f32: d_img holds float pixels and the transform runs in single precision, as PyWavelets does for float32 / float16
// input (every level's input must then be at least as long as the filter: SPIHT_ERR_ARG otherwise)
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
static int check_img_args(int wavelet, int mode, int64_t B, int64_t c, int64_t H, int64_t W) {
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
extern "C" int spiht_check_view_u8(int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output) {
    if (B < 1 || c < 1 || H < 1 || W < 1 || !strides) return SPIHT_ERR_ARG;
    Pic v;
    return view_pic(&v, nullptr, EL_U8, output != 0, strides, 4, B, c, H, W);
}
extern "C" int spiht_check_view_u16(int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output) {
    if (B < 1 || c < 1 || H < 1 || W < 1 || !strides) return SPIHT_ERR_ARG;
    Pic v;
    return view_pic(&v, nullptr, EL_U16, output != 0, strides, 4, B, c, H, W);
}

// pictures `in` (planes / c of them) -> quantised packed array [planes, enc_h, enc_w].  The rules of the pixel formats:
// float32 pixels are transformed in single precision, as PyWavelets does for float32 / float16 input (every level's input
// must then be at least as long as the filter: SPIHT_ERR_ARG otherwise), at a level >= 1 and without the colour model.
// 8- and 16-bit pixels need a level >= 1 (no entry point gets here with level 0: SPIHT refuses that geometry -- the root block's
// offspring fall outside the array -- before anything is transformed, on the float64 path as well); the tiled level 1
// reads them itself, the two-pass levels get their float64 form from a conversion pass first.  Float pixels in (EL_FLT_*) go
// the integer kinds' way in everything: the same view, the same two routes; their conversion is the exact widening.
static int dwt_forward(spiht_ctx *ctx, const Pic &in, int planes, int c, const ImgGeom &ig, int wavelet, int mode,
                       double q, const double *d_mults, int32_t *d_coeffs, uint32_t *d_maxabs = nullptr) {
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

// packed int32 array -> pixels [planes, rec_H, rec_W]
// l_hi .. l_lo: the levels to run, coarsest first (ig.L .. 1 = all).  A run that stops above level 1 leaves its last
// approximation in d_out ([planes, 2*hs[l_lo]-F+2, 2*ws[l_lo]-F+2]); a run that starts below ig.L takes that array as
// d_a_in.
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

// d_flags: L1Flags words [planes, gy, gx] the decoder of d_rec left (nullptr: every level-1 tile reads its detail bands)
// 8- / 16-bit output (l_lo == 1, a level >= 1: see dwt_forward): cropped to the picture's size; the tiled level 1 writes it
// itself, the two-pass level goes through a conversion pass behind it.
// A reduced geometry (reduced_geometry: ig.l0 = k levels dropped) runs the same way: its level 1 is level k + 1 of the
// stream and makes the picture of that size -- integer store, crop, colour change, conversion pass; also as the coarsest
// level (l == ig.L) -- and q is the caller's q * 2^k (reduced_q).  No d_flags then: the words belong to the stream's level 1.
static int dwt_inverse(spiht_ctx *ctx, const int32_t *d_rec, int planes, int c, const ImgGeom &ig, int wavelet, double q,
                       const double *d_mults, const Pic &out, int l_hi = -1, int l_lo = 1, const double *d_a_in = nullptr,
                       const uint32_t *d_flags = nullptr) {
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
        if (l == 1 && !a.first && !a.color) a.flags = d_flags;
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
extern "C" int spiht_dequant_idwt_flags_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B,
                                                 int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                 double q_scale, const double *channel_mults, uint8_t *d_img_out,
                                                 const int64_t *out_strides) {
    Pic out;
    CHK(view_pic(&out, d_img_out, EL_U8, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST));
    return dequant_idwt_batch(ctx, d_rec, d_flags, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out);
}
extern "C" int spiht_dequant_idwt_flags_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B,
                                                  int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                  double q_scale, const double *channel_mults, uint16_t *d_img_out,
                                                  const int64_t *out_strides) {
    Pic out;
    CHK(view_pic(&out, d_img_out, EL_U16, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST));
    return dequant_idwt_batch(ctx, d_rec, d_flags, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out);
}

// The inverse transform in two parts, so that a pipelined caller can queue the coarse levels (a quarter of the bytes,
// six small launches at 1080p) where no list decoder shares the GPU and only level 1 beside it (csrc/pipeline.cpp):
//   coarse (no `out` pictures): levels level..2 -> d_approx [B*c, 2*hs[2]-F+2, 2*ws[2]-F+2] (float64), the approximation
//   level 1 starts from
//   level1: d_rec + d_approx -> pixels.  With fewer than two levels the coarse part does nothing and d_approx is not read.
static int idwt_part(spiht_ctx *ctx, const int32_t *d_rec, double *d_approx, int64_t B, int64_t c, int64_t H, int64_t W,
                     int wavelet, int mode, int level, double q_scale, const double *channel_mults, const Pic &out,
                     const uint32_t *d_flags = nullptr) {
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
        return dwt_inverse(ctx, rec, nb * (int)c, (int)c, ig, wavelet, q_scale, k.d_mults, k.at(out, b0), std::min(ig.L, 1), 1,
                           ig.L >= 2 ? ap : nullptr, flagged ? d_flags + (size_t)b0 * c * fl.gy * fl.gx : nullptr);
    });
}
extern "C" int spiht_idwt_coarse_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                           int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                           double *d_approx) {
    if (!d_approx) return SPIHT_ERR_ARG;
    return idwt_part(ctx, d_rec, d_approx, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, Pic());
}
extern "C" int spiht_idwt_level1_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, double *d_img_out) {
    if (!d_img_out) return SPIHT_ERR_ARG;
    return idwt_part(ctx, d_rec, const_cast<double *>(d_approx), B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                     dense_pic(d_img_out, EL_F64, true));
}

// ... reading the decoder's occupancy words of the level-1 tiles (spiht_decode_lists_flags_batch_i32; NULL: reads everything)
extern "C" int spiht_idwt_level1_flags_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                                 int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                 double q_scale, const double *channel_mults, double *d_img_out) {
    if (!d_img_out) return SPIHT_ERR_ARG;
    return idwt_part(ctx, d_rec, const_cast<double *>(d_approx), B, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                     dense_pic(d_img_out, EL_F64, true), d_flags);
}
extern "C" int spiht_idwt_level1_flags_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                                int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                double q_scale, const double *channel_mults, uint8_t *d_img_out,
                                                const int64_t *out_strides) {
    Pic out;
    CHK(view_pic(&out, d_img_out, EL_U8, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST));
    return idwt_part(ctx, d_rec, const_cast<double *>(d_approx), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out,
                     d_flags);
}
extern "C" int spiht_idwt_level1_flags_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                                 int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                 double q_scale, const double *channel_mults, uint16_t *d_img_out,
                                                 const int64_t *out_strides) {
    Pic out;
    CHK(view_pic(&out, d_img_out, EL_U16, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST));
    return idwt_part(ctx, d_rec, const_cast<double *>(d_approx), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out,
                     d_flags);
}

extern "C" int spiht_idwt_approx_shape(int64_t H, int64_t W, int wavelet, int level, int64_t *a_h, int64_t *a_w) {
    if (wavelet < 0 || wavelet >= SPIHT_NWAVELETS || !a_h || !a_w) return SPIHT_ERR_ARG;
    ImgGeom ig;
    const int F = SPIHT_WAVELETS[wavelet].F;
    CHK(img_geometry(H, W, F, level, &ig));
    *a_h = ig.L >= 2 ? 2 * ig.hs[2] - F + 2 : 0;
    *a_w = ig.L >= 2 ? 2 * ig.ws[2] - F + 2 : 0;
    return SPIHT_OK;
}

static int encode_image_batch(spiht_ctx *ctx, const Pic &in, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                              int level, double q_scale, const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                              uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs) {
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
extern "C" int spiht_encode_image_batch_f64(spiht_ctx *ctx, const double *d_img, int64_t B, int64_t c, int64_t H,
                                            int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                                            uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n,
                                            int32_t *d_coeffs) {
    return encode_image_batch(ctx, dense_pic(d_img, EL_F64), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits,
                              d_out, slot_stride, d_nbits, d_max_n, d_coeffs);
}
extern "C" int spiht_encode_image_batch_f32(spiht_ctx *ctx, const float *d_img, int64_t B, int64_t c, int64_t H,
                                            int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                                            uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n,
                                            int32_t *d_coeffs) {
    return encode_image_batch(ctx, dense_pic(d_img, EL_F32), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits,
                              d_out, slot_stride, d_nbits, d_max_n, d_coeffs);
}
extern "C" int spiht_encode_image_batch_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                                           uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs) {
    Pic in;
    CHK(view_pic(&in, d_img, EL_U8, false, strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return encode_image_batch(ctx, in, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, d_out, slot_stride,
                              d_nbits, d_max_n, d_coeffs);
}
extern "C" int spiht_encode_image_batch_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                            int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                                            uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs) {
    Pic in;
    CHK(view_pic(&in, d_img, EL_U16, false, strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return encode_image_batch(ctx, in, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, d_out, slot_stride,
                              d_nbits, d_max_n, d_coeffs);
}

static int decode_image_batch(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                              const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                              double q_scale, const double *channel_mults, const Pic &out, int32_t *d_rec, int reduce = 0) {
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
            CHK(ensure(ctx, ctx->l1flags, (size_t)nb * c * fl.gy * fl.gx * 4));
            fl.p = (uint32_t *)ctx->l1flags.p;
        }
        if (rec) {
            CHK(decode_device(ctx, g, d_data + (size_t)b0 * slot_stride, slot_stride, d_nbytes + b0, d_max_n + b0, nb, rec,
                              nullptr, nullptr, 0, true, nullptr, flagged ? &fl : nullptr));
            return dwt_inverse(ctx, rec, nb * (int)c, (int)c, k.pig, wavelet, k.q, k.d_mults, k.at(out, b0), -1, 1, nullptr,
                               flagged ? fl.p : nullptr);
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
                        flagged ? fl.p : nullptr));
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
                              channel_mults,
                              dense_pic(d_img_out, EL_F64, true), d_rec);
}
extern "C" int spiht_decode_image_batch_u8(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                           const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, uint8_t *d_img_out, const int64_t *out_strides,
                                           int32_t *d_rec) {
    Pic out;
    CHK(view_pic(&out, d_img_out, EL_U8, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, out, d_rec);
}
extern "C" int spiht_decode_image_batch_u16(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                            const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                            int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, uint16_t *d_img_out, const int64_t *out_strides,
                                            int32_t *d_rec) {
    Pic out;
    CHK(view_pic(&out, d_img_out, EL_U16, true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, out, d_rec);
}

// ------------------------------------------------------------------------------------------------
// the drop-in calls on host arrays: encode_image / decode_image / decode_from_rec_arr of the reference's wrapper
// (spiht_wrapper.py:142-216, 259-281) as one C call each.  Pixels, stream and coefficient array live in the
// context's grow-only device buffers -- no allocation per call after the first of a given size.
// ------------------------------------------------------------------------------------------------
// (an 8- / 16-bit picture: only the bytes its strides span are uploaded)
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
                                           int mode, int level, double q_scale, const double *channel_mults,
                                           uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits,
                                           uint8_t *max_n) {
    return encode_image_host(ctx, dense_pic(img, EL_F64), c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out,
                             out_cap, out_nbits, max_n);
}
extern "C" int spiht_encode_image_host_f32(spiht_ctx *ctx, const float *img, int64_t c, int64_t H, int64_t W, int wavelet,
                                           int mode, int level, double q_scale, const double *channel_mults,
                                           uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits,
                                           uint8_t *max_n) {
    return encode_image_host(ctx, dense_pic(img, EL_F32), c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out,
                             out_cap, out_nbits, max_n);
}
extern "C" int spiht_encode_image_host_u8(spiht_ctx *ctx, const uint8_t *img, const int64_t *strides, int64_t c, int64_t H,
                                          int64_t W, int wavelet, int mode, int level, double q_scale,
                                          const double *channel_mults, uint64_t max_bits, uint8_t *out, uint64_t out_cap,
                                          uint64_t *out_nbits, uint8_t *max_n) {
    Pic in;
    CHK(view_pic(&in, img, EL_U8, false, strides, 3, 1, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return encode_image_host(ctx, in, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out, out_cap, out_nbits,
                             max_n);
}
extern "C" int spiht_encode_image_host_u16(spiht_ctx *ctx, const uint16_t *img, const int64_t *strides, int64_t c, int64_t H,
                                           int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, uint64_t max_bits, uint8_t *out, uint64_t out_cap,
                                           uint64_t *out_nbits, uint8_t *max_n) {
    Pic in;
    CHK(view_pic(&in, img, EL_U16, false, strides, 3, 1, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return encode_image_host(ctx, in, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out, out_cap, out_nbits,
                             max_n);
}

// the copy back of a host decode into a view is of c * h * w samples: only the two dense layouts, CHW and HWC
static int dense_chw_or_hwc(const Pic &v) {
    const int64_t es = v.es(), c = v.px.c, h = v.px.h, w = v.px.w;
    const bool chw = v.px.sw == es && v.px.sh == w * es && v.px.sc == h * w * es;
    const bool hwc = v.px.sc == es && v.px.sw == c * es && v.px.sh == w * c * es;
    return chw || hwc ? SPIHT_OK : SPIHT_ERR_ARG;
}
// (a view: a dense one, see above)
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
    CHK(decode_image_batch(ctx, (const uint8_t *)ctx->data.p, slot, (const uint64_t *)ctx->nbytes.p,
                           (const uint8_t *)ctx->maxn.p, 1,
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
extern "C" int spiht_decode_image_host_u8(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                          int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                          const double *channel_mults, uint8_t *img_out, const int64_t *strides) {
    Pic out;
    CHK(view_pic(&out, img_out, EL_U8, true, strides, 3, 1, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    CHK(dense_chw_or_hwc(out));
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, out);
}
extern "C" int spiht_decode_image_host_u16(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, uint16_t *img_out, const int64_t *strides) {
    Pic out;
    CHK(view_pic(&out, img_out, EL_U16, true, strides, 3, 1, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    CHK(dense_chw_or_hwc(out));
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, out);
}

extern "C" int spiht_dequant_idwt_host_f64(spiht_ctx *ctx, const int32_t *rec, int64_t c, int64_t H, int64_t W, int wavelet,
                                           int mode, int level, double q_scale, const double *channel_mults,
                                           double *img_out) {
    if (!ctx || !rec || !img_out) return SPIHT_ERR_ARG;
    CHK(check_img_args(wavelet, mode, 1, c, H, W));
    ImgGeom ig;
    CHK(img_geometry(H, W, SPIHT_WAVELETS[wavelet].F, level, &ig, mode));
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
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
// (include/spiht_hip.h).  The calls above with a reduced geometry behind them (reduced_geometry / reduced_q): levels
// L .. reduce + 1 of the inverse transform run, nothing below.  The list decoder is the same: it parses every bit.
// ------------------------------------------------------------------------------------------------
static int reduced_open(int64_t H, int64_t W, int wavelet, int mode, int level, int reduce, ImgGeom *ig, ImgGeom *pig) {
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
extern "C" int spiht_dequant_idwt_reduced_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H,
                                                   int64_t W, int wavelet, int mode, int level, double q_scale,
                                                   const double *channel_mults, uint8_t *d_img_out,
                                                   const int64_t *out_strides, int reduce) {
    Pic out;
    CHK(reduced_pic(d_img_out, EL_U8, out_strides, 4, B, c, H, W, wavelet, mode, level, reduce, &out));
    return dequant_idwt_batch(ctx, d_rec, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out, reduce);
}
extern "C" int spiht_dequant_idwt_reduced_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H,
                                                    int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, uint16_t *d_img_out,
                                                    const int64_t *out_strides, int reduce) {
    Pic out;
    CHK(reduced_pic(d_img_out, EL_U16, out_strides, 4, B, c, H, W, wavelet, mode, level, reduce, &out));
    return dequant_idwt_batch(ctx, d_rec, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out, reduce);
}

extern "C" int spiht_decode_image_reduced_batch_f64(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                    const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                    int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, double *d_img_out, int32_t *d_rec,
                                                    int reduce) {
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults,
                              dense_pic(d_img_out, EL_F64, true), d_rec, reduce);
}
extern "C" int spiht_decode_image_reduced_batch_u8(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                   const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                   int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                   const double *channel_mults, uint8_t *d_img_out,
                                                   const int64_t *out_strides, int32_t *d_rec, int reduce) {
    Pic out;
    CHK(reduced_pic(d_img_out, EL_U8, out_strides, 4, B, c, H, W, wavelet, mode, level, reduce, &out));
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, out, d_rec, reduce);
}
extern "C" int spiht_decode_image_reduced_batch_u16(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                    const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                    int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, uint16_t *d_img_out,
                                                    const int64_t *out_strides, int32_t *d_rec, int reduce) {
    Pic out;
    CHK(reduced_pic(d_img_out, EL_U16, out_strides, 4, B, c, H, W, wavelet, mode, level, reduce, &out));
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, out, d_rec, reduce);
}

extern "C" int spiht_decode_image_reduced_host_f64(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                                   int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                   const double *channel_mults, double *img_out, int reduce) {
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults,
                             dense_pic(img_out, EL_F64, true), reduce);
}
extern "C" int spiht_decode_image_reduced_host_u8(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                                  int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                  const double *channel_mults, uint8_t *img_out, const int64_t *strides,
                                                  int reduce) {
    Pic out;
    CHK(reduced_pic(img_out, EL_U8, strides, 3, 1, c, H, W, wavelet, mode, level, reduce, &out));
    CHK(dense_chw_or_hwc(out));
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, out, reduce);
}
extern "C" int spiht_decode_image_reduced_host_u16(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                                   int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                   const double *channel_mults, uint16_t *img_out, const int64_t *strides,
                                                   int reduce) {
    Pic out;
    CHK(reduced_pic(img_out, EL_U16, strides, 3, 1, c, H, W, wavelet, mode, level, reduce, &out));
    CHK(dense_chw_or_hwc(out));
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, out, reduce);
}

// ------------------------------------------------------------------------------------------------
// float pixels out (include/spiht_hip.h, *_flt): the *_u16 decode calls with the element of a float kind.  The view's rules
// are view_pic's with 4 or 2 bytes per sample; level 1 of the tiled inverse stores the kind (dwt_inv.hip, PX_FLT), the routes
// without a fused form convert in a pass of their own (dwt_inverse: conv8), which spiht_convert_batch_flt runs alone.
// ------------------------------------------------------------------------------------------------
extern "C" int spiht_check_view_flt(int kind, int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output) {
    if (B < 1 || c < 1 || H < 1 || W < 1 || !strides) return SPIHT_ERR_ARG;
    Pic v;
    // (a view that is read obeys the same rules without the overlap check)
    return view_pic(&v, nullptr, el_of_kind(kind), output != 0, strides, 4, B, c, H, W);
}
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
extern "C" int spiht_decode_image_batch_flt(spiht_ctx *ctx, int kind, const uint8_t *d_data, uint64_t slot_stride,
                                            const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H,
                                            int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, void *d_img_out, const int64_t *out_strides,
                                            int32_t *d_rec) {
    Pic out;
    CHK(view_pic(&out, d_img_out, el_of_kind(kind), true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet,
                 mode));
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, out, d_rec);
}
extern "C" int spiht_decode_image_host_flt(spiht_ctx *ctx, int kind, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, void *img_out, const int64_t *strides) {
    Pic out;
    CHK(view_pic(&out, img_out, el_of_kind(kind), true, strides, 3, 1, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    CHK(dense_chw_or_hwc(out));
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, out);
}
extern "C" int spiht_dequant_idwt_flags_batch_flt(spiht_ctx *ctx, int kind, const int32_t *d_rec, const uint32_t *d_flags,
                                                  int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                  double q_scale, const double *channel_mults, void *d_img_out,
                                                  const int64_t *out_strides) {
    Pic out;
    CHK(view_pic(&out, d_img_out, el_of_kind(kind), true, out_strides, 4, B, c, H, W, PIC_NULL_FIRST));
    return dequant_idwt_batch(ctx, d_rec, d_flags, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out);
}
extern "C" int spiht_dequant_idwt_reduced_batch_flt(spiht_ctx *ctx, int kind, const int32_t *d_rec, int64_t B, int64_t c,
                                                    int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, void *d_img_out,
                                                    const int64_t *out_strides, int reduce) {
    Pic out;
    CHK(reduced_pic(d_img_out, el_of_kind(kind), out_strides, 4, B, c, H, W, wavelet, mode, level, reduce, &out));
    return dequant_idwt_batch(ctx, d_rec, nullptr, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, out, reduce);
}
extern "C" int spiht_decode_image_reduced_batch_flt(spiht_ctx *ctx, int kind, const uint8_t *d_data, uint64_t slot_stride,
                                                    const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                    int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                                    const double *channel_mults, void *d_img_out,
                                                    const int64_t *out_strides, int32_t *d_rec, int reduce) {
    Pic out;
    CHK(reduced_pic(d_img_out, el_of_kind(kind), out_strides, 4, B, c, H, W, wavelet, mode, level, reduce, &out));
    return decode_image_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level, q_scale,
                              channel_mults, out, d_rec, reduce);
}
extern "C" int spiht_decode_image_reduced_host_flt(spiht_ctx *ctx, int kind, const uint8_t *data, uint64_t nbytes, uint8_t n,
                                                   int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                                                   double q_scale, const double *channel_mults, void *img_out,
                                                   const int64_t *strides, int reduce) {
    Pic out;
    CHK(reduced_pic(img_out, el_of_kind(kind), strides, 3, 1, c, H, W, wavelet, mode, level, reduce, &out));
    CHK(dense_chw_or_hwc(out));
    return decode_image_host(ctx, data, nbytes, n, c, H, W, wavelet, mode, level, q_scale, channel_mults, out, reduce);
}

// ------------------------------------------------------------------------------------------------
// float pixels in (include/spiht_hip.h, *_flt): the *_u16 encode calls with the element of a float kind.  Every sample is
// widened exactly on the loads of forward level 1 (dwt_fwd.hip, PX_FLT: flt_load_value), and everything behind that is the
// float64 path -- NOT the single-precision transform of the *_f32 calls.  The routes without a fused form widen in a pass of
// their own (dwt_forward: k_px_to_f64), which spiht_widen_batch_flt runs alone.
// ------------------------------------------------------------------------------------------------
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
extern "C" int spiht_encode_image_batch_flt(spiht_ctx *ctx, int kind, const void *d_img, const int64_t *strides, int64_t B,
                                            int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                            const double *channel_mults, uint64_t max_bits, uint8_t *d_out,
                                            uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs) {
    Pic in;
    CHK(view_pic(&in, d_img, el_of_kind(kind), false, strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return encode_image_batch(ctx, in, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, d_out, slot_stride,
                              d_nbits, d_max_n, d_coeffs);
}
extern "C" int spiht_encode_image_host_flt(spiht_ctx *ctx, int kind, const void *img, const int64_t *strides, int64_t c, int64_t H,
                                           int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, uint64_t max_bits, uint8_t *out, uint64_t out_cap,
                                           uint64_t *out_nbits, uint8_t *max_n) {
    Pic in;
    CHK(view_pic(&in, img, el_of_kind(kind), false, strides, 3, 1, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return encode_image_host(ctx, in, c, H, W, wavelet, mode, level, q_scale, channel_mults, max_bits, out, out_cap, out_nbits,
                             max_n);
}

// ------------------------------------------------------------------------------------------------
// rate-distortion reductions (rd.hip): K decoded arrays / pictures against the original -> K small rows, all in HBM
// ------------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------------
// tiled pictures (tiles.hip): one picture <-> a dense batch of equal tiles, T stream slots <-> one run of bytes
// ------------------------------------------------------------------------------------------------
extern "C" int spiht_tile_grid(int64_t H, int64_t W, int64_t th, int64_t tw, int64_t *gy, int64_t *gx) {
    if (H < 1 || W < 1 || th < 8 || tw < 8) return SPIHT_ERR_ARG;
    if (H >= (1 << 30) || W >= (1 << 30) || th > (1 << 24) || tw > (1 << 24)) return SPIHT_ERR_TOO_LARGE;
    if (gy) *gy = (H + th - 1) / th;
    if (gx) *gx = (W + tw - 1) / tw;
    return SPIHT_OK;
}
// in: the picture batch (dense_pic, or view_pic's checked view)
// overlap: NULL, or the margin m of spiht_tile_cut_overlap_* (k_tile_cut_overlap; 0 <= m, 2 m <= min(th, tw))
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
// the view of the strided cuts: N pictures [c, H, W] (an empty batch is checked as one picture; a NULL picture is tile_cut's to refuse)
static int cut_view(Pic *pic, const void *d_img, PicElem el, const int64_t *strides, int64_t N, int64_t c, int64_t H, int64_t W) {
    if (N < 0 || c < 1 || H < 1 || W < 1) return SPIHT_ERR_ARG;
    return view_pic(pic, d_img, el, false, strides, 4, N, c, H, W, PIC_EMPTY_OK);
}
extern "C" int spiht_tile_cut_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                                 int64_t W, int64_t th, int64_t tw, uint8_t *d_tiles) {
    Pic pic;
    CHK(cut_view(&pic, d_img, EL_U8, strides, N, c, H, W));
    return tile_cut(ctx, pic, N, c, H, W, th, tw, d_tiles);
}
extern "C" int spiht_tile_cut_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                                  int64_t W, int64_t th, int64_t tw, uint16_t *d_tiles) {
    Pic pic;
    CHK(cut_view(&pic, d_img, EL_U16, strides, N, c, H, W));
    return tile_cut(ctx, pic, N, c, H, W, th, tw, d_tiles);
}
extern "C" int spiht_tile_cut_f32(spiht_ctx *ctx, const float *d_img, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th,
                                  int64_t tw, float *d_tiles) {
    return tile_cut(ctx, dense_pic(d_img, EL_F32), N, c, H, W, th, tw, d_tiles);
}
extern "C" int spiht_tile_cut_f64(spiht_ctx *ctx, const double *d_img, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th,
                                  int64_t tw, double *d_tiles) {
    return tile_cut(ctx, dense_pic(d_img, EL_F64), N, c, H, W, th, tw, d_tiles);
}
// ... from a float32 view by byte strides (float pixels in: the 16-bit kinds go through the *_u16 copies, as bit patterns)
extern "C" int spiht_tile_cut_f32s(spiht_ctx *ctx, const float *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                                   int64_t W, int64_t th, int64_t tw, float *d_tiles) {
    Pic pic;
    CHK(cut_view(&pic, d_img, EL_FLT_F32, strides, N, c, H, W));
    return tile_cut(ctx, pic, N, c, H, W, th, tw, d_tiles);
}
// ... with a margin of m samples around every tile (overlap.hip): d_tiles is [N * T, c, th + 2m, tw + 2m]
extern "C" int spiht_tile_cut_overlap_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t N, int64_t c,
                                         int64_t H, int64_t W, int64_t th, int64_t tw, int64_t m, uint8_t *d_tiles) {
    Pic pic;
    CHK(cut_view(&pic, d_img, EL_U8, strides, N, c, H, W));
    return tile_cut(ctx, pic, N, c, H, W, th, tw, d_tiles, &m);
}
extern "C" int spiht_tile_cut_overlap_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t N, int64_t c,
                                          int64_t H, int64_t W, int64_t th, int64_t tw, int64_t m, uint16_t *d_tiles) {
    Pic pic;
    CHK(cut_view(&pic, d_img, EL_U16, strides, N, c, H, W));
    return tile_cut(ctx, pic, N, c, H, W, th, tw, d_tiles, &m);
}
extern "C" int spiht_tile_cut_overlap_f32s(spiht_ctx *ctx, const float *d_img, const int64_t *strides, int64_t N, int64_t c,
                                           int64_t H, int64_t W, int64_t th, int64_t tw, int64_t m, float *d_tiles) {
    Pic pic;
    CHK(cut_view(&pic, d_img, EL_FLT_F32, strides, N, c, H, W));
    return tile_cut(ctx, pic, N, c, H, W, th, tw, d_tiles, &m);
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
extern "C" int spiht_tile_paste_u8(spiht_ctx *ctx, const uint8_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                   int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                                   int64_t wh, int64_t ww, uint8_t *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, EL_U8, out_strides, c, wh, ww));
    return tile_paste(ctx, d_tiles, pic, c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_paste_u16(spiht_ctx *ctx, const uint16_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H,
                                    int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                                    int64_t x0, int64_t wh, int64_t ww, uint16_t *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, EL_U16, out_strides, c, wh, ww));
    return tile_paste(ctx, d_tiles, pic, c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
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
extern "C" int spiht_tile_mosaic_u8(spiht_ctx *ctx, const uint8_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                                    int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0,
                                    int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww, uint8_t *d_out,
                                    const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, EL_U8, out_strides, c, wh, ww));
    return tile_mosaic(ctx, d_tiles, pic, c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_mosaic_u16(spiht_ctx *ctx, const uint16_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                                     int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0,
                                     int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww, uint16_t *d_out,
                                     const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, EL_U16, out_strides, c, wh, ww));
    return tile_mosaic(ctx, d_tiles, pic, c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_mosaic_f64(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                                     int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0,
                                     int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww, double *d_out) {
    if (c < 1 || wh < 1 || ww < 1) return SPIHT_ERR_ARG;
    return tile_mosaic(ctx, d_tiles, dense_pic(d_out, EL_F64, true), c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh,
                       ww);
}

// overlapping tiles: the cross-fade of the float64 decodes of a sub-grid into a window (k_tile_blend)
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
extern "C" int spiht_tile_blend_u8(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                   int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                                   int64_t x0, int64_t wh, int64_t ww, uint8_t *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, EL_U8, out_strides, c, wh, ww));
    return tile_blend(ctx, d_tiles, pic, c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_blend_u16(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                    int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                                    int64_t x0, int64_t wh, int64_t ww, uint16_t *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, EL_U16, out_strides, c, wh, ww));
    return tile_blend(ctx, d_tiles, pic, c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_blend_f64(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                    int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                                    int64_t x0, int64_t wh, int64_t ww, double *d_out) {
    if (c < 1 || wh < 1 || ww < 1) return SPIHT_ERR_ARG;
    return tile_blend(ctx, d_tiles, dense_pic(d_out, EL_F64, true), c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh,
                      ww);
}

// float pixels out: the blend rounded to a float kind at the store; float32 tile batches pasted / assembled by strides (a copy
// of 4-byte elements -- the 16-bit kinds go through the *_u16 copies)
extern "C" int spiht_tile_blend_flt(spiht_ctx *ctx, int kind, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H,
                                    int64_t W, int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1,
                                    int64_t y0, int64_t x0, int64_t wh, int64_t ww, void *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, el_of_kind(kind), out_strides, c, wh, ww));
    return tile_blend(ctx, d_tiles, pic, c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_paste_f32s(spiht_ctx *ctx, const float *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                                     int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                                     int64_t wh, int64_t ww, float *d_out, const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, EL_FLT_F32, out_strides, c, wh, ww));
    return tile_paste(ctx, d_tiles, pic, c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}
extern "C" int spiht_tile_mosaic_f32(spiht_ctx *ctx, const float *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy,
                                     int64_t ox, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0,
                                     int64_t j1, int64_t y0, int64_t x0, int64_t wh, int64_t ww, float *d_out,
                                     const int64_t *out_strides) {
    Pic pic;
    CHK(window_view(&pic, d_out, EL_FLT_F32, out_strides, c, wh, ww));
    return tile_mosaic(ctx, d_tiles, pic, c, rh, rw, oy, ox, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww);
}

// the checks pack and unpack share; the scratch: uint64 [T] byte lengths (pack), uint64 [T] offsets
static int tile_streams_args(spiht_ctx *ctx, const void *a, const void *b, const void *d, const void *e, uint64_t slot_stride,
                             int64_t T) {
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

// ------------------------------------------------------------------------------------------------
// rate allocation across tiles (alloc.hip): prefixes of every tile's stream, their error sums, the cut of equal slope
// ------------------------------------------------------------------------------------------------
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
    if (!d_img) return SPIHT_ERR_ARG;
    return dwt_pyramid_batch(ctx, dense_pic(d_img, EL_F64), B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs,
                             d_dmsb, d_lmsb, d_maxabs);
}
extern "C" int spiht_dwt_pyramid_batch_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                          int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                          const double *channel_mults, int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb,
                                          uint32_t *d_maxabs) {
    Pic in;
    CHK(view_pic(&in, d_img, EL_U8, false, strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return dwt_pyramid_batch(ctx, in, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs, d_dmsb, d_lmsb,
                             d_maxabs);
}
extern "C" int spiht_dwt_pyramid_batch_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb,
                                           uint32_t *d_maxabs) {
    Pic in;
    CHK(view_pic(&in, d_img, EL_U16, false, strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return dwt_pyramid_batch(ctx, in, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs, d_dmsb, d_lmsb,
                             d_maxabs);
}
extern "C" int spiht_dwt_pyramid_batch_flt(spiht_ctx *ctx, int kind, const void *d_img, const int64_t *strides, int64_t B, int64_t c,
                                           int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                           const double *channel_mults, int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb,
                                           uint32_t *d_maxabs) {
    Pic in;
    CHK(view_pic(&in, d_img, el_of_kind(kind), false, strides, 4, B, c, H, W, PIC_NULL_FIRST | PIC_IMG_ARGS, wavelet, mode));
    return dwt_pyramid_batch(ctx, in, B, c, H, W, wavelet, mode, level, q_scale, channel_mults, d_coeffs, d_dmsb, d_lmsb,
                             d_maxabs);
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
