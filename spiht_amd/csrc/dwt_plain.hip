// The plain passes around the DWT (gfx950), one thread per sample and nobody's headline: the colour model change alone, the two-pass
// levels, the pad strips, quantise / dequantise, pixel conversions, the root block as a picture (dwt_device.h: the whole picture).
#include "dwt_device.h"

// Stand-alone colour model change of a batch of 3-channel float64 images [B,3,npix]; in place allowed.  The checker of
// the fused kernels, and the path of images that have no transform level.
__global__ __launch_bounds__(256) void k_color3(const double *__restrict__ in, double *__restrict__ out, size_t npix, Color3 c) {
    __shared__ SpowLds s_pw;
    spow_lds_fill(s_pw, threadIdx.x);
    __syncthreads();
    const size_t img = (size_t)blockIdx.y * 3 * npix;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < npix; t += (size_t)gridDim.x * 256) {
        double w0, w1, w2;
        color3_px(c, s_pw, in[img + t], in[img + npix + t], in[img + 2 * npix + t], w0, w1, w2);
        out[img + t] = w0;
        out[img + npix + t] = w1;
        out[img + 2 * npix + t] = w2;
    }
}
extern "C" int spiht_launch_color3(const double *d_in, double *d_out, int B, size_t npix, const double *A, const double *M,
                                   double p, hipStream_t st) {
    Color3 c;
    for (int i = 0; i < 9; i++) { c.A[i] = A[i]; c.M[i] = M[i]; }
    c.p = p;
    const unsigned gx = (unsigned)((npix + 1023) / 1024 < 1 ? 1 : (npix + 1023) / 1024);
    hipLaunchKernelGGL(k_color3, dim3(gx, (unsigned)B), dim3(256), 0, st, d_in, d_out, npix, c);
    return (int)hipGetLastError();
}

// ---- forward level for the extension modes that COMPUTE the extended sample (smooth, antisymmetric, antireflect) ----------
// PyWavelets' modes beyond the five index maps (the reference passes SpihtSettings.mode through, spiht_wrapper.py:163).
// A sample outside the signal is a function of the samples at the edge, and along axis -1 pywt extends the INTERMEDIATE
// (axis -2 already filtered) rows -- which is not the filtered extension of the pixels in the last bits -- so these modes
// run as two plain passes, one thread per output, through a float64 intermediate in memory: correctness first, no tiling
// (a path nobody's headline runs on; the tiled kernel of dwt_fwd.hip serves the index-map modes).  Summation order as pywt's
// downsampling_convolution: taps ascending, except that on the right overhang of an input at least as long as the filter
// the taps that read the extension come first, nearest first -- smooth, like constant, keeps ascending order there too.
template <typename T>
__device__ __forceinline__ T ext_value(const T *x, int N, size_t sx, int i, int mode) {
    if (mode == 8) {  // periodization: the signal, made even by repeating its last sample, continued periodically
        const int Np = N + (N & 1);
        int m = i % Np;
        if (m < 0) m += Np;
        return x[(size_t)(m < N ? m : N - 1) * sx];
    }
    if (i >= 0 && i < N) return x[(size_t)i * sx];
    if (mode < 5) {  // the index maps (filters longer than the tiled kernels take come through here too)
        const int m = ext_index(i, N, mode);
        return m < 0 ? (T)0 : x[(size_t)m * sx];
    }
    if (mode == 5) {  // smooth: the straight line through the two samples at the edge
        if (N < 2) return x[0];
        if (i < 0) return x[0] + (T)(-i) * (x[0] - x[sx]);
        return x[(size_t)(N - 1) * sx] + (T)(i - N + 1) * (x[(size_t)(N - 1) * sx] - x[(size_t)(N - 2) * sx]);
    }
    if (mode == 6) {  // antisymmetric: half-sample mirror image, every other block of N samples negated
        const int P = 2 * N;
        int m = i % P;
        if (m < 0) m += P;
        const int blk = (i - m) / N + (m >= N ? 1 : 0);
        const T v = x[(size_t)(m < N ? m : P - 1 - m) * sx];
        return (blk & 1) ? -v : v;
    }
    // antireflect: whole-sample mirror image through the edge VALUE; the value a block ends on is the next block's edge
    if (N < 2) return x[0];
    const bool left = i < 0;
    int d = left ? -i : i - N + 1;
    T e = left ? x[0] : x[(size_t)(N - 1) * sx];
    bool away = true;  // the first block walks away from the edge it started at and subtracts; the next one comes back and adds
    for (;;) {
        const int k = d <= N - 1 ? d : N - 1;
        const bool from_left = left ? away : !away;
        const T dlt = from_left ? x[(size_t)k * sx] - x[0] : x[(size_t)(N - 1 - k) * sx] - x[(size_t)(N - 1) * sx];
        const T v = away ? e - dlt : e + dlt;
        if (d <= N - 1) return v;
        e = v;
        d -= N - 1;
        away = !away;
    }
}

// one analysis pass along one axis: out position o of line `line` of plane `plane`.  n_lines lines of length N, element
// stride sx, line stride sl; outputs: lo / hi [plane][L][n_lines] laid out with the same strides roles (so, sol).
// T = float: the single-precision transform PyWavelets runs on float32 / float16 pixels (its own filter values).
struct DwtAxisArgs {
    int32_t F, mode, N, L, n_lines, planes;
    int32_t i0, pad;             // output o reads the window that ends at sample 2 o + i0: 1, or F / 2 under periodization
    size_t sx, sl, plane_in;     // input: element stride along the axis, stride between lines, plane stride
    size_t so, sol, plane_out;   // output alike
    const void *in;
    void *lo, *hi;
    const double *flo, *fhi;     // device: dec_lo, dec_hi (any length: the whole PyWavelets table goes through this path)
    const float *flo_f, *fhi_f;  // ... as the single-precision transform has them
};
template <typename T>
__global__ __launch_bounds__(256) void k_dwt_axis_ext(DwtAxisArgs a) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_plane = (size_t)a.L * a.n_lines;
    if (t >= per_plane * (size_t)a.planes) return;
    const int plane = (int)(t / per_plane);
    const size_t r = t - (size_t)plane * per_plane;
    // consecutive threads along the contiguous direction of the output
    int o, line;
    if (a.so == 1) { line = (int)(r / a.L); o = (int)(r - (size_t)line * a.L); }
    else { o = (int)(r / a.n_lines); line = (int)(r - (size_t)o * a.n_lines); }
    const T *x = reinterpret_cast<const T *>(a.in) + (size_t)plane * a.plane_in + (size_t)line * a.sl;
    const int i = 2 * o + a.i0;
    const int jb = (i >= a.N && a.mode != 5 && a.mode != 4) ? i - a.N : -1;  // (smooth and constant: ascending throughout)
    T sa = 0, sd = 0;
    for (int s2 = 0; s2 < a.F; s2++) {
        const int j = s2 <= jb ? jb - s2 : s2;
        const T v = ext_value<T>(x, a.N, a.sx, i - j, a.mode);
        const T fl = sizeof(T) == 4 ? (T)a.flo_f[j] : (T)a.flo[j], fh = sizeof(T) == 4 ? (T)a.fhi_f[j] : (T)a.fhi[j];
        sa += fl * v;
        sd += fh * v;
    }
    const size_t oo = (size_t)plane * a.plane_out + (size_t)line * a.sol + (size_t)o * a.so;
    reinterpret_cast<T *>(a.lo)[oo] = sa;
    reinterpret_cast<T *>(a.hi)[oo] = sd;
}
// quantise + pack the four sub-bands of a level computed by the two passes: aa / ad from the low rows, da / dd from the high rows
struct DwtPackArgs {
    int32_t c, out_h, out_w, off_h, off_w, enc_h, enc_w, last, planes, pad;
    const void *aa, *ad, *da, *dd;   // [planes, out_h, out_w]
    void *ll_out;
    int32_t *coeffs;
    const double *mults;
    uint32_t *maxabs;
    double q;
};
template <typename T>
__global__ __launch_bounds__(256) void k_dwt_pack_ext(DwtPackArgs a) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)a.out_h * a.out_w;
    uint32_t amax = 0;
    int img = -1;
    if (t < per * (size_t)a.planes) {
        const int plane = (int)(t / per);
        const size_t r = t - (size_t)plane * per;
        const int oh = (int)(r / a.out_w), ow = (int)(r - (size_t)oh * a.out_w);
        const bool has_m = a.mults != nullptr;
        const double mk = has_m ? a.mults[plane % a.c] : 1.0;
        const float qf = (float)a.q;
        auto qz = [&](T v) -> int32_t {  // the wrapper's arithmetic in the array's precision (spiht_wrapper.py:167-172, :9-11)
            if (sizeof(T) == 4) return quant_f32((float)v, mk, a.q, qf, has_m);
            return quant((double)v, mk, a.q, has_m);
        };
        int32_t *co = a.coeffs + (size_t)plane * a.enc_h * a.enc_w;
        const T *aa = reinterpret_cast<const T *>(a.aa), *ad = reinterpret_cast<const T *>(a.ad);
        const T *da = reinterpret_cast<const T *>(a.da), *dd = reinterpret_cast<const T *>(a.dd);
        const int32_t qad = qz(ad[t]), qda = qz(da[t]), qdd = qz(dd[t]);
        if (a.last) {
            const int32_t qaa = qz(aa[t]);
            co[(size_t)oh * a.enc_w + ow] = qaa;
            amax = iabs_u(qaa);
        } else {
            reinterpret_cast<T *>(a.ll_out)[t] = aa[t];
        }
        co[(size_t)oh * a.enc_w + a.off_w + ow] = qad;
        co[(size_t)(a.off_h + oh) * a.enc_w + ow] = qda;
        co[(size_t)(a.off_h + oh) * a.enc_w + a.off_w + ow] = qdd;
        amax = max(amax, max(iabs_u(qad), max(iabs_u(qda), iabs_u(qdd))));
        img = plane / a.c;
    }
    if (a.maxabs != nullptr) wave_raise_max(a.maxabs, img, amax);
}
// tmp: 6 arrays of planes*out_h*in_w (2) and planes*out_h*out_w (4) elements (float when a->f32), carved by the caller
// d_filt: the wavelet's filters on the device -- dec_lo, dec_hi, rec_lo, rec_hi (F doubles each), then dec_lo, dec_hi as the
// single-precision transform has them (F floats each)
extern "C" int spiht_launch_dwt_level_ext(const DwtKArgs *a, int planes, void *t_lo, void *t_hi, void *b_aa, void *b_ad,
                                          void *b_da, void *b_dd, const double *d_filt, hipStream_t st) {
    DwtAxisArgs x;
    memset(&x, 0, sizeof(x));
    x.F = a->F; x.mode = a->mode; x.planes = planes;
    x.i0 = a->mode == 8 ? a->F / 2 : 1;
    x.flo = d_filt; x.fhi = d_filt + a->F;
    x.flo_f = reinterpret_cast<const float *>(d_filt + 4 * (size_t)a->F); x.fhi_f = x.flo_f + a->F;
    const bool f32 = a->f32 != 0;
    auto axis = [&](size_t n) {
        if (f32) hipLaunchKernelGGL(k_dwt_axis_ext<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x);
        else hipLaunchKernelGGL(k_dwt_axis_ext<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x);
    };
    // axis -2: lines = columns
    x.N = a->in_h; x.L = a->out_h; x.n_lines = a->in_w;
    x.sx = (size_t)a->in_w; x.sl = 1; x.plane_in = (size_t)a->in_h * a->in_w;
    x.so = (size_t)a->in_w; x.sol = 1; x.plane_out = (size_t)a->out_h * a->in_w;
    x.in = a->in; x.lo = t_lo; x.hi = t_hi;
    axis((size_t)planes * x.L * x.n_lines);
    // axis -1 on the low rows, then on the high rows: lines = rows
    x.N = a->in_w; x.L = a->out_w; x.n_lines = a->out_h;
    x.sx = 1; x.sl = (size_t)a->in_w; x.plane_in = (size_t)a->out_h * a->in_w;
    x.so = 1; x.sol = (size_t)a->out_w; x.plane_out = (size_t)a->out_h * a->out_w;
    const size_t n = (size_t)planes * x.L * x.n_lines;
    x.in = t_lo; x.lo = b_aa; x.hi = b_ad;
    axis(n);
    x.in = t_hi; x.lo = b_da; x.hi = b_dd;
    axis(n);
    DwtPackArgs p;
    memset(&p, 0, sizeof(p));
    p.c = a->c; p.out_h = a->out_h; p.out_w = a->out_w; p.off_h = a->off_h; p.off_w = a->off_w; p.enc_h = a->enc_h; p.enc_w = a->enc_w;
    p.last = a->last; p.planes = planes;
    p.aa = b_aa; p.ad = b_ad; p.da = b_da; p.dd = b_dd;
    p.ll_out = a->ll_out; p.coeffs = a->coeffs; p.mults = a->mults; p.maxabs = a->maxabs; p.q = a->q;
    if (f32) hipLaunchKernelGGL(k_dwt_pack_ext<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_dwt_pack_ext<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    return (int)hipGetLastError();
}

// ---- inverse level under periodization (pywt upsampling_convolution_valid_sf_periodization) ---------------------------------
// 2 L samples back from L + L coefficients: x[n] = sum_k rec[n - 2k + F/2 - 1] c[k mod L], i.e. with p = (n + F/2 - 1) & 1 and
// i = (n + F/2 - 1 - p) / 2 the terms j = 0 .. F/2-1: tap 2j + p against c[(i - j) mod L]; pywt adds every product straight
// into the output sample, the approximation's first, then the detail's; where the window hangs over the right end (i >= L)
// the terms beyond it come first, nearest first -- and sample 0 of a filter with an even number of tap pairs is summed
// like the odd half of the last window (jb = F/4 - 1).  One thread per output sample, two passes (axis -1, then axis -2)
// through an intermediate: the plain form of a mode nobody's headline runs on.
struct IdwtPerArgs {
    int32_t F, L, n_lines, planes;     // L coefficients per line, n_lines lines
    int32_t per, n_out;                // periodization (2 L samples) or the plain synthesis (2 L - F + 2 samples: filters longer than
                                       // the tiled kernels take)
    const double *flo_d, *fhi_d;       // device: rec_lo, rec_hi
    size_t si, so;                     // element stride along the axis: inputs, output
    size_t sla, sld, slo;              // stride between lines: approximation input, detail input, output
    size_t plane_a, plane_d, plane_out;
    const double *ca, *cd;             // float inputs ...
    const int32_t *qa, *qd;            // ... or quantised ones (dequantised on the fly, (v / m) / q as the wrapper does)
    int32_t a_is_q, d_is_q, c, has_m;
    const double *mults;
    double q;
    double *out;
};
__global__ __launch_bounds__(256) void k_idwt_axis_per(IdwtPerArgs a) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_plane = (size_t)a.n_out * a.n_lines;
    if (t >= per_plane * (size_t)a.planes) return;
    const int plane = (int)(t / per_plane);
    const size_t r = t - (size_t)plane * per_plane;
    int n, line;  // consecutive threads along the contiguous direction of the output
    if (a.so == 1) { line = (int)(r / (size_t)a.n_out); n = (int)(r - (size_t)line * a.n_out); }
    else { n = (int)(r / a.n_lines); line = (int)(r - (size_t)n * a.n_lines); }
    const int HF = a.F / 2;
    const bool has_m = a.has_m != 0;
    const double mk = has_m ? a.mults[plane % a.c] : 1.0;
    const size_t ba = (size_t)plane * a.plane_a + (size_t)line * a.sla, bd = (size_t)plane * a.plane_d + (size_t)line * a.sld;
    auto va = [&](int k) -> double { return a.a_is_q ? dequant(a.qa[ba + (size_t)k * a.si], mk, a.q, has_m) : a.ca[ba + (size_t)k * a.si]; };
    auto vd = [&](int k) -> double { return a.d_is_q ? dequant(a.qd[bd + (size_t)k * a.si], mk, a.q, has_m) : a.cd[bd + (size_t)k * a.si]; };
    double res;
    if (a.per) {
        const int s0 = HF - 1, p = (n + s0) & 1, i = (n + s0 - p) / 2;
        int jb = i >= a.L ? i - a.L : -1;
        if (n == 0 && (HF & 1) == 0) jb = a.F / 4 - 1;
        double acc = 0.0;
#pragma unroll 1
        for (int pass = 0; pass < 2; pass++) {
            const double *f = pass ? a.fhi_d : a.flo_d;
            for (int s2 = 0; s2 < HF; s2++) {
                const int j = s2 <= jb ? jb - s2 : s2;
                int k = (i - j) % a.L;
                if (k < 0) k += a.L;
                acc += f[2 * j + p] * (pass ? vd(k) : va(k));
            }
        }
        res = acc;
    } else {
        // upsampling_convolution_valid_sf: sample n = 2 (i - (F/2 - 1)) + p; the approximation's sum and the detail's sum kept
        // apart, each over j ascending (tap 2j + p against coefficient i - j, those inside the band), then added
        const int p = n & 1, i = n / 2 + HF - 1;
        double sa = 0.0, sd = 0.0;
        for (int j = 0; j < HF; j++) {
            const int k = i - j;
            if (k < 0 || k >= a.L) continue;
            sa += a.flo_d[2 * j + p] * va(k);
            sd += a.fhi_d[2 * j + p] * vd(k);
        }
        res = (0.0 + sa) + sd;
    }
    a.out[(size_t)plane * a.plane_out + (size_t)line * a.slo + (size_t)n * a.so] = res;
}
// t_lo, t_hi: planes * band_h * out_w doubles each (out_w = 2 band_w, out_h = 2 band_h)
// per: periodization (a->out_h / out_w = 2 x band) or the plain synthesis for a filter of any length (2 x band - F + 2);
// d_filt: the wavelet's filters on the device (see spiht_launch_dwt_level_ext)
extern "C" int spiht_launch_idwt_level_per(const IdwtKArgs *a, int planes, double *t_lo, double *t_hi, const double *d_filt, int per,
                                           hipStream_t st) {
    IdwtPerArgs x;
    memset(&x, 0, sizeof(x));
    x.F = a->F; x.planes = planes; x.c = a->c; x.has_m = a->mults != nullptr; x.mults = a->mults; x.q = a->q;
    x.per = per;
    x.flo_d = d_filt + 2 * (size_t)a->F; x.fhi_d = d_filt + 3 * (size_t)a->F;
    const size_t enc_plane = (size_t)a->enc_h * a->enc_w;
    // axis -1 (PyWavelets' idwtn takes the last axis first): band_h lines of band_w coefficients -> out_w samples
    x.L = a->band_w; x.n_lines = a->band_h; x.n_out = a->out_w;
    x.si = 1; x.so = 1; x.slo = (size_t)a->out_w; x.plane_out = (size_t)a->band_h * a->out_w;
    const size_t n1 = (size_t)planes * x.n_out * x.n_lines;
    // (aa, ad) -> low rows: the approximation comes out of the packed array (coarsest level) or from the level before, whose
    // array may be one sample longer than the band in either direction (waverec2 drops it)
    if (a->first) { x.a_is_q = 1; x.qa = a->rec; x.plane_a = enc_plane; x.sla = (size_t)a->enc_w; }
    else { x.a_is_q = 0; x.ca = a->a_in; x.plane_a = (size_t)a->a_h * a->a_w; x.sla = (size_t)a->a_w; }
    x.d_is_q = 1; x.qd = a->rec + a->off_w; x.plane_d = enc_plane; x.sld = (size_t)a->enc_w;
    x.out = t_lo;
    hipLaunchKernelGGL(k_idwt_axis_per, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, x);
    // (da, dd) -> high rows
    x.a_is_q = 1; x.qa = a->rec + (size_t)a->off_h * a->enc_w; x.plane_a = enc_plane; x.sla = (size_t)a->enc_w;
    x.qd = a->rec + (size_t)a->off_h * a->enc_w + a->off_w;
    x.out = t_hi;
    hipLaunchKernelGGL(k_idwt_axis_per, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, x);
    // axis -2: out_w lines (columns) of band_h coefficients -> out_h samples
    x.L = a->band_h; x.n_lines = a->out_w; x.n_out = a->out_h;
    x.si = (size_t)a->out_w; x.sla = 1; x.sld = 1; x.plane_a = x.plane_d = (size_t)a->band_h * a->out_w;
    x.so = (size_t)a->out_w; x.slo = 1; x.plane_out = (size_t)a->out_h * a->out_w;
    x.a_is_q = 0; x.d_is_q = 0; x.ca = t_lo; x.cd = t_hi;
    x.out = a->out;
    const size_t n2 = (size_t)planes * x.n_out * x.n_lines;
    hipLaunchKernelGGL(k_idwt_axis_per, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, x);
    return (int)hipGetLastError();
}

// zero the padding cells of coeffs_to_array: per level the strip below 'ad' and the strip right of 'da'.
// grid: (blocks, nrects, planes)
struct PadRects {
    int32_t n;
    int32_t enc_h, enc_w, pad;
    int32_t r0[2 * SPIHT_MAX_LEVELS], r1[2 * SPIHT_MAX_LEVELS], c0[2 * SPIHT_MAX_LEVELS], c1[2 * SPIHT_MAX_LEVELS];
};
__global__ __launch_bounds__(256) void k_zero_pads(PadRects pr, int32_t *coeffs) {
    const int rc = blockIdx.y;
    const int r0 = pr.r0[rc], r1 = pr.r1[rc], c0 = pr.c0[rc], c1 = pr.c1[rc];
    const int w = c1 - c0, cells = (r1 - r0) * w;
    int32_t *co = coeffs + (size_t)blockIdx.z * pr.enc_h * pr.enc_w;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < cells; t += gridDim.x * blockDim.x) {
        int r = t / w, cidx = t - r * w;
        co[(size_t)(r0 + r) * pr.enc_w + c0 + cidx] = 0;
    }
}

// level 0 of the API (no decomposition): quantise the image itself. grid-stride.
__global__ __launch_bounds__(256) void k_quant_plain(const double *in, int32_t *out, size_t n_per_plane, int planes, int c,
                                                     const double *mults, double q, uint32_t *maxabs) {
    size_t total = n_per_plane * (size_t)planes;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t0 = (size_t)blockIdx.x * blockDim.x; t0 < total; t0 += stride) {  // (t0: the same in every lane of a wavefront's block)
        const size_t t = t0 + threadIdx.x;
        int img = -1;
        uint32_t av = 0;
        if (t < total) {
            int plane = (int)(t / n_per_plane);
            bool has_m = mults != nullptr;
            int32_t v = quant(in[t], has_m ? mults[plane % c] : 1.0, q, has_m);
            out[t] = v;
            img = plane / c;
            av = iabs_u(v);
        }
        if (maxabs != nullptr) wave_raise_max(maxabs, img, av);
    }
}
__global__ __launch_bounds__(256) void k_dequant_plain(const int32_t *in, double *out, size_t n_per_plane, int planes, int c,
                                                       const double *mults, double q) {
    size_t total = n_per_plane * (size_t)planes;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        int plane = (int)(t / n_per_plane);
        double v = (double)in[t];
        if (mults != nullptr) v = v / mults[plane % c];
        out[t] = v / q;
    }
}

// pad strips of coeffs_to_array for `L` levels: hs/ws band sizes and offh/offw block offsets (index 1..L)
extern "C" int spiht_launch_zero_pads(int L, const int64_t *hs, const int64_t *ws, const int64_t *offh, const int64_t *offw,
                                      int enc_h, int enc_w, int32_t *coeffs, int planes, hipStream_t st) {
    PadRects pr;
    pr.n = 0; pr.enc_h = enc_h; pr.enc_w = enc_w; pr.pad = 0;
    for (int l = 1; l <= L; l++) {
        if (offh[l] > hs[l]) {  // below 'ad'
            pr.r0[pr.n] = (int)hs[l]; pr.r1[pr.n] = (int)offh[l]; pr.c0[pr.n] = (int)offw[l]; pr.c1[pr.n] = (int)(offw[l] + ws[l]);
            pr.n++;
        }
        if (offw[l] > ws[l]) {  // right of 'da'
            pr.r0[pr.n] = (int)offh[l]; pr.r1[pr.n] = (int)(offh[l] + hs[l]); pr.c0[pr.n] = (int)ws[l]; pr.c1[pr.n] = (int)offw[l];
            pr.n++;
        }
    }
    if (pr.n == 0) return 0;
    hipLaunchKernelGGL(k_zero_pads, dim3(8, pr.n, planes), dim3(256), 0, st, pr, coeffs);
    return (int)hipGetLastError();
}
extern "C" int spiht_launch_quant_plain(const double *in, int32_t *out, size_t n_per_plane, int planes, int c,
                                        const double *mults, double q, uint32_t *maxabs, hipStream_t st) {
    hipLaunchKernelGGL(k_quant_plain, dim3(1024), dim3(256), 0, st, in, out, n_per_plane, planes, c, mults, q, maxabs);
    return (int)hipGetLastError();
}
extern "C" int spiht_launch_dequant_plain(const int32_t *in, double *out, size_t n_per_plane, int planes, int c,
                                          const double *mults, double q, hipStream_t st) {
    hipLaunchKernelGGL(k_dequant_plain, dim3(1024), dim3(256), 0, st, in, out, n_per_plane, planes, c, mults, q);
    return (int)hipGetLastError();
}

// ---- 8- and 16-bit pixels to and from dense float64, for the routes whose level 1 has no integer form ------------------------
// (level 0, the two-pass levels, the colour model change in front of a two-pass level).  One thread per sample, the same
// conversions as the fused kernels (px_value / PX_STORE); the kind is the view's element size, or its float kind (both ways:
// k_px_to_f64<PX_FLT> is the exact widening of float pixels in, spiht_widen_batch_flt runs it alone).
template <int PX>
__global__ __launch_bounds__(256) void k_px_to_f64(PxView px, double *__restrict__ out, int64_t n) {  // out [B*c, h, w]
    const int64_t hw = (int64_t)px.h * px.w;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const int64_t p = t / hw, r = t - p * hw, y = r / px.w, x = r - y * px.w;
        const int64_t o = (p / px.c) * px.sb + (p % px.c) * px.sc + y * px.sh + x * px.sw;
        out[t] = px_value<PX>(px_load<PX>(px.in + o, px.kind), px.kind);
    }
}
template <int PX>
__global__ __launch_bounds__(256) void k_f64_to_px(const double *__restrict__ in, int rec_h, int rec_w, PxView px, int64_t n) {
    const int64_t hw = (int64_t)px.h * px.w;  // n = B*c*h*w: the cropped picture
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const int64_t p = t / hw, r = t - p * hw, y = r / px.w, x = r - y * px.w;
        const int64_t o = (p / px.c) * px.sb + (p % px.c) * px.sc + y * px.sh + x * px.sw;
        PX_STORE(PX, px.out, o, in[(p * rec_h + y) * rec_w + x], px.kind);
    }
}
static unsigned pass_grid(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 8192); }
extern "C" int spiht_launch_px_to_f64(const PxView *px, int64_t B, double *out, hipStream_t st) {
    const int64_t n = B * px->c * (int64_t)px->h * px->w;
    if (n <= 0) return 0;
    with_px(px_kind_of(*px), [&](auto PX) {  // (a view is never float64: no such instantiation)
        if constexpr (PX != PX_F64) hipLaunchKernelGGL(k_px_to_f64<PX>, dim3(pass_grid(n)), dim3(256), 0, st, *px, out, n);
    });
    return (int)hipGetLastError();
}
extern "C" int spiht_launch_f64_to_px(const double *in, int rec_h, int rec_w, const PxView *px, int64_t B, hipStream_t st) {
    const int64_t n = B * px->c * (int64_t)px->h * px->w;
    if (n <= 0) return 0;
    with_px(px_kind_of(*px), [&](auto PX) {
        if constexpr (PX != PX_F64) hipLaunchKernelGGL(k_f64_to_px<PX>, dim3(pass_grid(n)), dim3(256), 0, st, in, rec_h, rec_w, *px, n);
    });
    return (int)hipGetLastError();
}

// ---- reduced-resolution decode that stops at the root block (reduce == level): no synthesis level runs at all ------------
// The picture is the root block itself: the ll_h x ll_w window in the top-left corner of the packed int32 array, dequantised
// ((r / m) / q, the statement of every other kernel here; q already carries the 2^level of the approximation band's gain),
// through the colour model change for a three-channel picture (color3_px: the bits of k_color3 on the dequantised planes),
// stored as float64 [units, ll_h, ll_w] or through the strided 8- / 16-bit view, cropped to it.  One thread per pixel (per
// three-channel pixel with colour), plain vector stores.  grid: (tiles of 256 pixels, plane) -- (.., image) with colour.
template <int PX>
__global__ __launch_bounds__(256) void k_ll_to_pic(LlPicArgs a) {
    __shared__ SpowLds s_pw;
    if (a.color) {  // (kernel-uniform)
        spow_lds_fill(s_pw, threadIdx.x);
        __syncthreads();
    }
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= a.ll_h * a.ll_w) return;
    const int y = t / a.ll_w, x = t - y * a.ll_w;
    const bool has_m = a.mults != nullptr;
    const size_t cpl = (size_t)a.enc_h * a.enc_w, opl = (size_t)a.ll_h * a.ll_w;
    const size_t ro = (size_t)y * a.enc_w + x;
    const int nch = a.color ? 3 : 1;
    const int plane0 = (int)blockIdx.y * nch;
    double v[3] = {0.0, 0.0, 0.0};
    for (int ch = 0; ch < nch; ch++) {
        const int plane = plane0 + ch;
        v[ch] = dequant(a.rec[(size_t)plane * cpl + ro], has_m ? a.mults[plane % a.c] : 1.0, a.q, has_m);
    }
    if (a.color) {
        double w0, w1, w2;
        color3_px(a.col, s_pw, v[0], v[1], v[2], w0, w1, w2);
        v[0] = w0; v[1] = w1; v[2] = w2;
    }
    if (PX) {
        if (y >= a.px.h || x >= a.px.w) return;
        for (int ch = 0; ch < nch; ch++) {
            const int plane = plane0 + ch;
            uint8_t *p = a.px.out + (int64_t)(plane / a.c) * a.px.sb + (int64_t)(plane % a.c) * a.px.sc;
            PX_STORE(PX, p, (int64_t)y * a.px.sh + (int64_t)x * a.px.sw, v[ch], a.px.kind);
        }
    } else {
        for (int ch = 0; ch < nch; ch++) a.out[(size_t)(plane0 + ch) * opl + t] = v[ch];
    }
}
// planes: B*c of the launch (at most 65535); a->color: c == 3 and col set; a->px.out set: an 8- / 16-bit picture
extern "C" int spiht_launch_ll_to_pic(const LlPicArgs *a, int planes, hipStream_t st) {
    const int64_t npix = (int64_t)a->ll_h * a->ll_w;
    const int units = a->color ? planes / 3 : planes;
    if (npix <= 0 || units <= 0) return 0;
    if (npix >= (1ll << 31) - 256 || units > 65535) return -1;
    const dim3 grid((unsigned)((npix + 255) / 256), (unsigned)units);
    with_px(a->px.out == nullptr ? PX_F64 : px_kind_of(a->px), [&](auto PX) { hipLaunchKernelGGL(k_ll_to_pic<PX>, grid, dim3(256), 0, st, *a); });
    return (int)hipGetLastError();
}
