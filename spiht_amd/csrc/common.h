// Shared host/device definitions for libspiht_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SPIHT_MAX_LEVELS 32
#define SPIHT_MAX_TAPS 20

// Exact unsigned division by an invariant divisor d >= 2 (Granlund-Montgomery round-up form):
//   q = (t + ((n - t) >> 1)) >> sh,  t = mulhi(m, n)
struct FastDiv {
    uint32_t m, sh, d, pad;
};

static inline FastDiv fastdiv_make(uint32_t d) {
    FastDiv f;
    f.d = d;
    f.pad = 0;
    if (d < 2) { f.m = 0; f.sh = 0; return f; }  // callers never divide by < 2
    uint32_t l = 0;
    while ((1ull << l) < d) l++;  // ceil(log2 d)
    uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    f.m = (uint32_t)m;
    f.sh = l - 1;
    return f;
}

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv &f) {
    uint32_t t = __umulhi(f.m, n);
    return (t + ((n - t) >> 1)) >> f.sh;
}
#endif

// The same for any divisor d >= 1 (the general Granlund-Montgomery form: two shifts, so that d == 1 needs no case of its own):
//   q = (t + ((n - t) >> s1)) >> s2,  t = mulhi(m, n);  exact for every 32-bit n
struct FastDivU {
    uint32_t m, s1, s2, d;
};

static inline FastDivU fastdivu_make(uint32_t d) {
    FastDivU f;
    if (d < 1) d = 1;
    f.d = d;
    uint32_t l = 0;
    while ((1ull << l) < d) l++;  // ceil(log2 d), 0 ... 32
    f.m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    f.s1 = l < 1 ? l : 1;
    f.s2 = l < 1 ? 0 : l - 1;
    return f;
}
static inline uint32_t fastdivu_host(uint32_t n, const FastDivU &f) {  // what fdivu computes, on the host (tools/fastdiv_check.cpp)
    const uint32_t t = (uint32_t)(((uint64_t)f.m * n) >> 32);
    return (t + ((n - t) >> f.s1)) >> f.s2;
}

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t fdivu(uint32_t n, const FastDivU &f) {
    const uint32_t t = __umulhi(f.m, n);
    return (t + ((n - t) >> f.s1)) >> f.s2;
}
#endif

// Geometry of one coefficient array [c,h,w] with an ll_h x ll_w root block.
struct Geom {
    int32_t c, h, w, ll_h, ll_w;
    uint32_t hw;  // h*w
    uint32_t n;   // c*h*w  (< 2^30)
    uint32_t pad;
    FastDiv div_w, div_hw;
};

// List entry: bit 31 = type A (1) / type B (0) for LIS entries; bit 30 = "leaf": a type-A entry whose node
// has no offspring (the reference still queues it when its parent's B entry fires; it emits a 0 in every
// plane and can never fire, encoder_decoder.rs:229-239); low 30 bits = linear index k*hw + i*w + j.  The rules on these
// entries -- tree geometry, tokens, appends -- stand once, in list_coder.h (device code: both encoders, the decoder's tree).
#define ENT_A 0x80000000u
#define ENT_LEAF 0x40000000u
#define ENT_IDX 0x3FFFFFFFu

// Per-slot scratch of the list coder.  A "slot" serves one image at a time.
struct ListCaps {
    uint32_t lip, lsp, lis;  // capacities in entries
    uint32_t pad;
};

// One image on several CUs (encode_wide.hip): per group of workgroups a control block and the descriptors of the chunk scan.
struct WideCtl {          // zero-filled before every launch
    uint32_t bar_count, bar_gen;  // the group's barrier: arrivals (monotonic), released epoch
    uint32_t go;          // workgroup 0 has handed over: st[] is valid
    uint32_t bad;         // 1: a list capacity exceeded; 2: a wait ran out of time -- the group's workgroups were not all
                          // resident (other kernels held the CUs): everyone leaves, k_encode codes the image again
    uint32_t st[12];      // n, lip_len, lsp_len, lis_len, bitpos lo / hi, LIP buffer, LIS buffer, done
    uint32_t tot[8];      // totals of the pass just finished, two sets (pass number & 1)
    uint32_t bad_at;      // ~(pass number) of the first pass in which a capacity was exceeded (atomicMax), 0: none
    uint32_t pad[3];
};
struct WideArgs {
    WideCtl *ctl;         // [groups]
    uint64_t *desc;       // [groups][2][maxchunks][4] words [pass number | count]: aggregates, inclusive prefixes; zero-filled
    uint32_t maxchunks;
    uint32_t G;           // workgroups per image
    uint32_t solo;        // entries on the three lists together up to which a plane is coded by workgroup 0 alone
    uint32_t pad;
};

struct EncArgs {
    Geom g;
    ListCaps caps;
    int32_t B;
    int32_t nslots;
    const int32_t *x;        // [B, n]
    const uint8_t *dmsb;     // [B, n]
    const uint8_t *lmsb;     // [B, n]
    const uint32_t *maxabs;  // [B]
    uint64_t max_bits;       // already mapped: 0 -> unlimited
    uint8_t *out;            // [B, slot_stride]
    uint64_t slot_stride;    // bytes, multiple of 4
    uint64_t *out_nbits;     // [B]
    uint8_t *out_maxn;       // [B]
    // scratch, per slot
    uint32_t *lip0, *lip1, *lsp, *lis0, *lis1, *lis2;
    uint32_t *err;           // device error word
    const WideCtl *redo;     // k_encode behind k_encode_wide: codes only the images whose group gave up (bad & 2); else null
    float log2_thresh[32];   // log2_thresh[k]: smallest float m < 2^k with (u8)log2f(m) == k (host libm), or 2^k
};

// Tile of the inverse level-1 kernels (dwt_inv.hip), in output positions; in band positions half of it.
#define IW_TH 24    // output rows per tile (two halves, one per half of the workgroup; a multiple of 4)
#define IW_TW 128   // output cols per tile, one thread per column per half

// Which tiles of the inverse transform's level 1 have anything but zeros in their detail bands: the list decoder knows
// every cell it writes, so it sets one word per (plane, tile) whose staged band region -- the tile's IW_TH/2 x IW_TW/2
// band positions plus the halo of F/2 - 1 rows / columns behind them -- contains a decoded cell of a level-1 band; the
// inverse level-1 kernel then does not read the three int32 detail bands of a tile whose word is still zero (at 0.5 bpp
// nearly all of them).  Conservative by construction: a set word only means "read".  p == nullptr: no flags.
// Two granularities: the word says "this tile stages a cell" (0/1: callers make and read such words, and they stay), bit r of
// the row word "staged band row r of this tile holds one" -- a few hundred scattered cells set 40 % of the words, 4 % of the rows.
struct L1Flags {
    uint32_t *p;              // [planes, gy, gx] (planes = B*c of the launch), zero-filled before the decoder runs
    uint32_t *rows;           // [planes, gy, gx] or null (not wanted): bit r, 0 <= r < IW_TH/2 + hf1, of a tile's word: its staged
                              // band row r holds a decoded cell, in some staged column of some of the three bands; zero-filled likewise
    int32_t off_h, off_w;     // offsets of the level-1 detail bands in the packed array
    int32_t band_h, band_w;   // their size
    int32_t hf1;              // F/2 - 1: band rows / columns of halo a tile stages beyond its own
    int32_t gx, gy;           // tiles per plane
    int32_t pad;
};

struct DecArgs {
    Geom g;
    ListCaps caps;
    int32_t B;
    int32_t nslots;
    const uint8_t *data;      // [B, slot_stride]
    uint64_t slot_stride;     // bytes, multiple of 4
    const uint64_t *nbytes;   // [B]
    const uint8_t *max_n;     // [B]
    int32_t *out;             // [B, n], zero-filled before launch
    uint32_t *lip0, *lip1, *lsp_idx, *lis0, *lis1, *lis2;
    int32_t *lsp_val;
    uint32_t *err;
    uint32_t *lsp_count;      // [nslots] or null: final LSP length of the image a slot decoded (k_unscatter)
    L1Flags fl;               // occupancy of the inverse transform's level-1 tiles (fl.p null: not wanted)
    // decode_with_metadata only (k_decode<true>): one trace record per stream position 0..nbits (the last one is
    // the operation that was waiting for a bit when the stream ended)
    uint32_t *tr_ent;         // [B, tr_stride]  entry: node index | filter << 28 (| ENT_A / ENT_LEAF, ignored)
    uint8_t *tr_act;          // [B, tr_stride]  action 0..6 | plane << 3;  TR_NONE where no operation starts
    uint64_t tr_stride;       // records per image (>= 8*nbytes + 1)
};

// decode_with_metadata: list entries also carry the filter (encoder_decoder.rs:457-462) in bits 28-29, because
// on trees with duplicated nodes (odd ll_h / ll_w) the same node is reached under two different filters; the
// index is then limited to 28 bits.
#define ENT_IDX_META 0x0FFFFFFFu
#define ENT_FILT_SHIFT 28
#define TR_NONE 0xFFu

// k_meta_rows / k_meta_fold (metadata.hip)
struct MetaArgs {
    Geom g;
    int32_t level;            // number of detail levels (Slices.other_slices.len())
    int32_t pad;
    uint64_t rows;            // 8*nbytes + 1
    const uint32_t *tr_ent;   // [rows]
    const uint8_t *tr_act;    // [rows]
    const uint8_t *data;      // stream bytes
    const int32_t *slices;    // device: top {start_i,end_i,start_j,end_j}, then [level][3][4]
    int32_t *meta;            // [rows, 8]
    const uint32_t *skey;     // sorted node index per record (fold)
    const uint32_t *spos;     // record position, sorted by (node index, position)
};

// The batched form (k_meta_keys_batch / k_meta_rows_batch / k_meta_fold_batch, metadata.hip): a chunk of nb images whose
// traces lie at b * tr_stride.  The slices travel by value (the call stays asynchronous and never reads the caller's host
// arrays later); only the levels the tree reaches are read, and a tree has at most META_MAX_GEN generations (n < 2^28).
#define META_MAX_GEN 32
struct MetaBatchArgs {
    Geom g;
    int32_t level;            // number of detail levels (Slices.other_slices.len())
    int32_t nb;               // images in the chunk
    uint32_t tr_stride;       // records per image (8 * slot_stride + 1 or more); nb * tr_stride <= 2^31
    uint32_t pad0;
    FastDiv div_tr;           // record index -> image
    uint64_t slot_stride;     // bytes per stream slot
    uint64_t meta_rows;       // rows per image of meta (>= tr_stride)
    uint32_t key_none;        // nb * n: the sort key of positions without an operation (keys b * n + node below it)
    uint32_t pad;
    const uint32_t *tr_ent;   // [nb, tr_stride]
    const uint8_t *tr_act;    // [nb, tr_stride]
    const uint8_t *data;      // [nb, slot_stride] stream bytes
    const uint64_t *nbytes;   // [nb] valid bytes per slot (more than slot_stride: the decoder reads none)
    int32_t *meta;            // [nb, meta_rows, 8]
    const uint32_t *skey;     // sorted keys b * n + node (fold)
    const uint32_t *spos;     // record index b * tr_stride + position, sorted by (image, node, position)
    int32_t slices[4 + 12 * META_MAX_GEN];  // top {start_i,end_i,start_j,end_j}, then [generation - 1][3][4]
};

struct PyrArgs {
    Geom g;
    int32_t B;
    int32_t round;            // 1..: index-doubling depth handled by this launch
    const int32_t *x;
    uint8_t *dmsb, *lmsb;
    uint32_t *maxabs;
};

// Colour model change fused into level 1 of the transform (dwt_device.h: color3_px): per pixel w = M * spow(A * u, p), spow(x, p) =
// sign(x)|x|^p -- the shape of RGB <-> IPT (spiht/color_models.py:6-13 -> colour-science; here the published matrices)
struct Color3 {
    double A[9], M[9], p;
};

// 8- and 16-bit pixels at level 1 of the transforms (dwt_fwd.hip, dwt_inv.hip: the PX_U8 / PX_U16 kernels): a [B, c, h, w] uint8 or uint16
// view given by BYTE strides (both kinds: the pointers stay byte pointers, a 16-bit sample is read / written at its byte
// address, which is even -- the entry points check base and strides).  With D = 255 (es == 1) or 65535 (es == 2):
// Forward: sample k is loaded as the double k / D (IEEE division: exactly numpy's P / D).  Inverse: a value v is
// stored as (uintN)(clip(v, 0, 1) * D), truncated, and only for y < h, x < w (the picture's own size: the level's
// output is one longer where h / w is odd).  Plane index p = b*c + ch; its base b*sb + ch*sc is formed in 64 bits.
struct PxView {
    const uint8_t *in;     // forward: the pixels read
    uint8_t *out;          // inverse: the pixels written
    int64_t sb, sc, sh, sw;
    int32_t c, h, w;
    int32_t es;            // element size in bytes: 1 or 2 (the launchers pick the kernels' pixel kind from it); a float kind: 4 or 2
    int32_t kind;          // 0: integer pixels.  floatpx.h: 1 float32, 2 float16, 3 bfloat16.  Inverse: the value is stored rounded
    int32_t pad;           // once to the kind, no clip and no scale, through the same strides and the same crop.  Forward: the
                           // sample is loaded as the double of the same value (exact), through the same strides
};

// One forward DWT level (dwt_fwd.hip)
struct DwtKArgs {
    int32_t c;             // channels (plane index = b*c + k)
    int32_t F, mode;
    int32_t in_h, in_w, out_h, out_w;
    int32_t off_h, off_w, enc_h, enc_w;
    int32_t last;          // coarsest level: LL is quantised into the packed array too
    int32_t planes;        // B*c (set by the launcher)
    int32_t f32;           // single-precision level (k_dwt_level_f32): `in` / `ll_out` then point to float arrays
    int32_t ov_h, ov_w;    // first output row / column that hangs over the bottom / right end of the input far enough for
                           // PyWavelets' overhang order to differ from ascending order; out_h / out_w: none (launcher)
    const double *in;      // [planes, in_h, in_w]
    double *ll_out;        // [planes, out_h, out_w]
    int32_t *coeffs;       // [planes, enc_h, enc_w]
    const double *mults;   // device [c] or null
    uint32_t *maxabs;      // device [B] or null: atomicMax of |quantised coefficient| per image
    double q;
    double lo[SPIHT_MAX_TAPS], hi[SPIHT_MAX_TAPS];  // dec_lo, dec_hi
    float lo_f[SPIHT_MAX_TAPS], hi_f[SPIHT_MAX_TAPS];  // ... as PyWavelets' single-precision transform has them (f32 levels)
    int32_t color, pad2;   // level 1 of a 3-channel image with the colour model change on its loads (k_dwt1_color)
    Color3 col;
    PxView px;             // level 1 of an 8- / 16-bit picture: the kernels' integer instantiations read it instead of `in`
    // Launch-time constants of the tiled kernel k_dwt_level (set by its launcher, dwt_fwd.hip: dwt_set_launch_consts)
    FastDivU dv_gx, dv_gy, dv_c;  // tile -> (bx, by, plane), plane -> (image, channel) without a division in the kernel
    uint32_t gx, gy, nt;   // tiles per row, per column, in all
    int32_t narrow;        // every plane the kernel touches spans less than 2^30 bytes: 32-bit offsets into plane descriptors
    uint32_t in_pb;        // narrow: bytes per input plane (float64 input), per row, per column; an 8- / 16-bit view: its span and
    uint32_t in_rb, in_cb; // its byte strides sh and sw
    uint32_t co_pb, co_rb; // ... per plane and row of `coeffs`
    uint32_t ll_pb, ll_rb; // ... of `ll_out`
    uint32_t pad3;
};

// Whether k_dwt_level may address with 32-bit offsets (DwtKArgs::narrow): each plane it reads or writes -- the input (float64
// in_h x in_w, or the byte span of an 8- / 16-bit view), the packed array, the approximation -- stays under 2^30 bytes, so that
// the sum of a row offset and a column offset, either of which may be an out-of-range mark (2^31 for a row, 2^30 for a column),
// neither wraps nor lands inside the plane.  Larger pictures take the 64-bit addressing.
static inline bool dwt_narrow_ok(int64_t in_h, int64_t in_w, int64_t out_h, int64_t out_w, int64_t enc_h, int64_t enc_w, int px_es,
                                 int64_t px_sh, int64_t px_sw) {
    const int64_t lim = (int64_t)1 << 30;
    if (in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || enc_h < 1 || enc_w < 1) return false;
    if (in_h >= lim || in_w >= lim || out_h >= lim / 16 || out_w >= lim / 16 || enc_h >= lim || enc_w >= lim) return false;  // (no overflow below)
    if (px_es) {
        if (px_sh < 0 || px_sw < 0 || px_sh >= lim || px_sw >= lim) return false;
        if ((in_h - 1) * px_sh + (in_w - 1) * px_sw + px_es >= lim) return false;
    } else if (in_h * in_w * 8 >= lim) return false;
    if (enc_h * enc_w * 4 >= lim) return false;
    if (out_h * out_w * 8 >= lim) return false;
    // a tile's rows below the last output row (at most DW_TH - 1 <= 64 of them) are addressed and dropped by the range check:
    // their offsets, and an out-of-range mark advanced over a tile's rows, stay below 2^32
    if ((out_h + 64) * enc_w * 4 >= 2 * lim || (out_h + 64) * out_w * 8 >= 2 * lim) return false;
    return true;
}

// One inverse DWT level (dwt_inv.hip)
// Tile hand-out of the persistent inverse-transform kernel (k_idwt_level_pf): one counter per XCD in device memory,
// never reset -- the launcher knows how many numbers a launch draws from each (tiles + 2 per workgroup) and hands the
// kernel the counter values it starts from (all arithmetic modulo 2^32).
struct TileCtr {
    uint32_t *dev;      // 8 counters, 32 words apart (a memory line each), and a ninth (word 8 * 32): persistent workgroups
                        // that have started, ever; zero when allocated
    uint32_t base[8];   // host-side: value of each counter before the next launch
    int32_t wg_per_cu;  // persistent workgroups per CU of the next launches (0: the kernel's default, IWP_WG)
    int32_t num_cu;     // of the context's device
    int32_t lds_per_cu; // bytes of LDS a CU has (hipDeviceProp_t::maxSharedMemoryPerMultiProcessor)
    uint32_t started;   // host-side: what the ninth counter reads once every launch queued so far has all its workgroups on the CUs
};
#define TILECTR_WORDS (9 * 32)
#define TILECTR_STARTED (8 * 32)
struct TileBase { uint32_t v[8]; };

struct IdwtKArgs {
    int32_t c;
    int32_t F;
    int32_t band_h, band_w;    // detail band size (= approximation size used)
    int32_t out_h, out_w;      // 2*band - F + 2
    int32_t a_h, a_w;          // stored size of the incoming approximation (>= band; trim rule)
    int32_t off_h, off_w, enc_h, enc_w;
    int32_t first;             // coarsest level: approximation comes from rec[0:band_h, 0:band_w]
    int32_t planes;            // B*c (set by the launcher)
    const double *a_in;        // [planes, a_h, a_w]
    const int32_t *rec;        // [planes, enc_h, enc_w]
    const uint32_t *flags;     // [planes, gy, gx] or null: L1Flags words of this level's tiles (level 1 only)
    const uint32_t *rows;      // [planes, gy, gx] or null: their row words (with flags only; null: a set word means every row)
    double *out;               // [planes, out_h, out_w]
    const double *mults;
    double q;
    double lo[SPIHT_MAX_TAPS], hi[SPIHT_MAX_TAPS];  // rec_lo, rec_hi
    int32_t color, pad2;       // level 1 of a 3-channel image with the colour model change on its stores (k_idwt1_color)
    Color3 col;
    PxView px;                 // level 1 into an 8- / 16-bit picture: the kernels' integer instantiations write it instead of `out`
};

// The root block as a picture (dwt_plain.hip: k_ll_to_pic): a reduced-resolution decode that runs no synthesis level
struct LlPicArgs {
    const int32_t *rec;    // [planes, enc_h, enc_w]
    int32_t enc_h, enc_w, ll_h, ll_w;
    int32_t c, color;
    const double *mults;   // device [c] or null
    double q;
    double *out;           // float64 pictures [planes, ll_h, ll_w] (PX_F64)
    PxView px;             // integer pictures
    Color3 col;
};

// The launchers of pyramid.hip, encode.hip, encode_wide.hip, decode.hip (built twice: 12 and 8 wavefronts), dwt_fwd.hip, dwt_inv.hip, dwt_plain.hip and
// metadata.hip, as the host side (api.cpp, api_*.cpp) calls them: declared here so that the compiler holds every definition to its callers.
extern "C" {
int spiht_launch_absmax(const int32_t *d_x, int B, uint32_t n, uint32_t *d_maxabs, hipStream_t st);
int spiht_launch_pyramid(const Geom *g, int B, const int32_t *d_x, uint8_t *d_dmsb, uint8_t *d_lmsb, hipStream_t st);
int spiht_launch_encode(const EncArgs *a, hipStream_t st);
int spiht_launch_encode_wide(const EncArgs *a, const WideArgs *w, int groups, hipStream_t st);
int spiht_wide_groups_per_cu(void);
int spiht_launch_decode(const DecArgs *a, hipStream_t st);
int spiht_launch_decode_w8(const DecArgs *a, hipStream_t st);  // the 8-wavefront build of decode.hip
int spiht_launch_unscatter(const DecArgs *a, hipStream_t st);
int spiht_meta_sort_temp_bytes(uint64_t rows, size_t *bytes);
int spiht_launch_metadata(const MetaArgs *a, uint32_t *keys_in, uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out,
                          void *temp, size_t temp_bytes, hipStream_t st);
int spiht_launch_budget_fold(const MetaArgs *a, uint32_t *keys_in, uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out,
                             void *temp, size_t temp_bytes, const uint64_t *d_budgets, int K, int32_t *d_out, hipStream_t st);
int spiht_meta_batch_sort_temp_bytes(const MetaBatchArgs *a, size_t *bytes);
int spiht_launch_metadata_batch(const MetaBatchArgs *a, uint32_t *keys_in, uint32_t *vals_in, uint32_t *keys_out,
                                uint32_t *vals_out, void *temp, size_t temp_bytes, hipStream_t st);
int spiht_launch_nbits_to_nbytes(const uint64_t *d_nbits, int B, uint64_t *d_nbytes, hipStream_t st);
int spiht_launch_color3(const double *d_in, double *d_out, int B, size_t npix, const double *A, const double *M, double p,
                        hipStream_t st);
int spiht_launch_dwt_level(const DwtKArgs *a, int planes, hipStream_t st);
int spiht_launch_dwt_level_ext(const DwtKArgs *a, int planes, void *t_lo, void *t_hi, void *b_aa, void *b_ad, void *b_da,
                               void *b_dd, const double *d_filt, hipStream_t st);
int spiht_launch_idwt_level_per(const IdwtKArgs *a, int planes, double *t_lo, double *t_hi, const double *d_filt, int per,
                                hipStream_t st);
int spiht_launch_idwt_level(const IdwtKArgs *a, int planes, hipStream_t st, TileCtr *tc);
int spiht_launch_px_to_f64(const PxView *px, int64_t B, double *out, hipStream_t st);
int spiht_launch_f64_to_px(const double *in, int rec_h, int rec_w, const PxView *px, int64_t B, hipStream_t st);
int spiht_launch_quant_plain(const double *in, int32_t *out, size_t n_per_plane, int planes, int c, const double *mults,
                             double q, uint32_t *maxabs, hipStream_t st);
int spiht_launch_zero_pads(int L, const int64_t *hs, const int64_t *ws, const int64_t *offh, const int64_t *offw, int enc_h,
                           int enc_w, int32_t *coeffs, int planes, hipStream_t st);
int spiht_launch_ll_to_pic(const LlPicArgs *a, int planes, hipStream_t st);
int spiht_launch_dequant_plain(const int32_t *in, double *out, size_t n_per_plane, int planes, int c,
                               const double *mults, double q, hipStream_t st);
int spiht_launch_gate(const uint32_t *counter, uint32_t target, uint64_t ticks, hipStream_t st);
int spiht_launch_spin(int blocks, int threads, uint64_t ticks, uint32_t lds_bytes, uint32_t *sink, hipStream_t st);  // (SPIHT_DIAG builds)
int spiht_launch_spin_kind(int blocks, int threads, uint64_t ticks, uint32_t lds_bytes, uint32_t *sink, int mode, hipStream_t st);
}
