/*
 * spiht_hip.h -- C ABI of libspiht_hip.so, the MI355X (gfx950) SPIHT hot path.
 *
 * This is the drop-in boundary: the entry points are what the reference's
 * extension module `spiht.spiht` (PyO3, /root/reference/src/lib.rs) exposes,
 * re-expressed with plain pointers and sizes, plus batched / fused forms so the
 * DWT output never has to leave HBM.  No torch types, no C++ types.
 *
 * Every function returns an int status (SPIHT_OK = 0) and never aborts.
 * Host pointers unless a parameter says "device".
 */
#ifndef SPIHT_HIP_H
#define SPIHT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SPIHT_OK = 0,
    SPIHT_ERR_LL = 1,        /* ll_h <= 1 || ll_w <= 1: the reference asserts (encoder_decoder.rs:160-161, 310-311) */
    SPIHT_ERR_EMPTY = 2,     /* empty array: the reference unwrap()s None (encoder_decoder.rs:165) */
    SPIHT_ERR_SHAPE = 3,     /* LL offspring fall outside [h,w]: the reference panics on an out-of-bounds index */
    SPIHT_ERR_CAPACITY = 4,  /* caller's output buffer too small; *out_nbits holds the size needed */
    SPIHT_ERR_HIP = 5,       /* a HIP runtime call failed; see spiht_last_hip_error() */
    SPIHT_ERR_ARG = 6,       /* null pointer / negative size / unknown wavelet or mode */
    SPIHT_ERR_MAGNITUDE = 7, /* max|x| >= 2^30: outside the range the reference handles */
    SPIHT_ERR_INTERNAL = 8,  /* device-side list overflow guard tripped (a bug, never expected) */
    SPIHT_ERR_TOO_LARGE = 9, /* c*h*w >= 2^30, stream >= 2^32 bits, or a picture of more than 65535 planes */
    SPIHT_ERR_NOMEM = 10
};

/* signal extension modes of the DWT (pywt names) */
enum { SPIHT_MODE_REFLECT = 0, SPIHT_MODE_SYMMETRIC = 1, SPIHT_MODE_PERIODIC = 2, SPIHT_MODE_ZERO = 3,
       SPIHT_MODE_CONSTANT = 4,
       /* the modes whose extended samples are computed, not picked: a slower two-pass forward transform */
       SPIHT_MODE_SMOOTH = 5, SPIHT_MODE_ANTISYMMETRIC = 6, SPIHT_MODE_ANTIREFLECT = 7,
       /* another length rule: ceil(n / 2) coefficients per level, 2 n samples back (spiht_geometry_mode); two-pass in both
        * directions */
       SPIHT_MODE_PERIODIZATION = 8 };

#define SPIHT_MAX_BITS_UNLIMITED 0xFFFFFFFFFFFFFFFFull

typedef struct spiht_ctx spiht_ctx;

const char *spiht_strerror(int status);
const char *spiht_last_hip_error(void);
/* ABI version of this header; bumped on any signature change and on every round that adds entry points (now 2).  The
 * 8-bit and 16-bit pixel entry points (*_u8, *_u16) and the float pixel ones (*_flt) are additions only -- no existing
 * signature changed -- and the version stays at 2. */
int spiht_abi_version(void);

/* One context per (process, GPU): device id, streams, scratch.  Thread-safe per context
 * (calls on one context are serialised by an internal mutex); no globals survive a call. */
int spiht_ctx_create(int device, spiht_ctx **out);
/* priority > 0: the context's stream gets the device's highest stream priority (its workgroups are placed first when
 * kernels of several contexts wait for room on the CUs); 0: as spiht_ctx_create. */
int spiht_ctx_create_priority(int device, int priority, spiht_ctx **out);
void spiht_ctx_destroy(spiht_ctx *ctx);
/* Block until everything queued on the context's stream has finished.  Returns (and clears) what the device-side guards of
 * the asynchronous calls queued before it recorded: SPIHT_ERR_MAGNITUDE, SPIHT_ERR_CAPACITY or SPIHT_ERR_INTERNAL.
 * The rule for that latched error: it is reported exactly once, by the first call on the context that waits for its
 * stream.  Those calls are spiht_ctx_synchronize() and the calls that take or return host arrays: spiht_encode_i32,
 * spiht_decode_i32, spiht_decode_with_metadata_i32, spiht_decode_budgets_i32, spiht_decode_budgets_dev_i32 (it waits while
 * it uploads the stream), spiht_encode_image_host_f64 / _f32 / _u8 / _u16, spiht_decode_image_host_f64 / _u8 / _u16 / _flt,
 * spiht_decode_image_reduced_host_f64 / _u8 / _u16 / _flt.  (spiht_pipeline_synchronize reports for the pipeline's contexts.)
 * Such a call looks at the error before it starts its own work: it returns the earlier call's status without running, and
 * the same call made again works normally.  Outputs of the images that tripped no guard are valid either way. */
int spiht_ctx_synchronize(spiht_ctx *ctx);
/* Order across contexts without blocking the host: everything queued on `ctx` after this call waits (on the
 * device) for everything queued on `other` before it.  Lets one context's stream encode step i+1 while another
 * decodes step i. */
int spiht_ctx_wait_on(spiht_ctx *ctx, spiht_ctx *other);
/* Finer-grained ordering: an event marks the point a context's queue has reached (spiht_event_record); work queued on
 * another context after spiht_ctx_wait_event starts only once that point has been passed.  Neither call blocks the host. */
typedef struct spiht_event spiht_event;
int spiht_event_create(spiht_ctx *ctx, spiht_event **out);
void spiht_event_destroy(spiht_event *ev);
int spiht_event_record(spiht_event *ev, spiht_ctx *ctx);
int spiht_ctx_wait_event(spiht_ctx *ctx, spiht_event *ev);
/* Placement between two contexts' kernels without a timer (csrc/pipeline.cpp: the list decoder of a batch is launched
 * behind the persistent workgroups of the previous batch's inverse level 1).  The large levels of the inverse transform run
 * as persistent workgroups -- a fixed number per CU, each too large for one more than that number to fit -- that count
 * themselves in as they start.  _resident_ticket: where that count lives and what it will read once every such launch
 * queued on ctx SO FAR has all its workgroups on the CUs (*d_counter NULL: the context has no such counter).
 * _wait_resident: queues on ctx's stream a one-wavefront kernel that waits for the count to reach target, at most
 * timeout_us microseconds (<= 10 000; it never holds its stream for ever): what is queued behind it starts when those
 * workgroups are resident. */
int spiht_ctx_resident_ticket(spiht_ctx *ctx, const void **d_counter, uint32_t *target);
int spiht_ctx_wait_resident(spiht_ctx *ctx, const void *d_counter, uint32_t target, uint32_t timeout_us);
/* The context's HIP stream (*stream is a hipStream_t) so a caller can queue its own work -- e.g. the RCCL gather of
 * the streams between encode and decode -- in order with the library's. */
int spiht_ctx_stream(spiht_ctx *ctx, void **stream);
/* Stage timing: when enabled, HIP events bracket each kernel group of the next calls
 * (on the context's own stream); spiht_ctx_get_timing returns accumulated ms and launches. */
int spiht_ctx_set_timing(spiht_ctx *ctx, int enabled);
int spiht_ctx_reset_timing(spiht_ctx *ctx);
int spiht_ctx_num_stages(void);
const char *spiht_ctx_stage_name(int stage);
int spiht_ctx_get_timing(spiht_ctx *ctx, int stage, double *ms, uint64_t *launches);

/* ---------------------------------------------------------------------------------------
 * L2 boundary, single image, host buffers.
 * ------------------------------------------------------------------------------------- */

/* Replaces `encode(x, ll_h, ll_w, max_bits) -> (bytes, max_n)`  (src/lib.rs:24-32, which calls
 * encoder_decoder.rs:155-303 and packs bits LSB-first, lib.rs:29).
 * x: int32 [c,h,w] with element strides (any strides, as PyReadonlyArray3 allows).
 * max_bits: 0 behaves as "never reached" exactly like the reference (encoder_decoder.rs:196).
 * out/out_cap: caller-owned byte buffer; on SPIHT_ERR_CAPACITY *out_nbits is the bit count needed. */
int spiht_encode_i32(spiht_ctx *ctx, const int32_t *x, int64_t c, int64_t h, int64_t w, int64_t stride_c,
                     int64_t stride_h, int64_t stride_w, int64_t ll_h, int64_t ll_w, uint64_t max_bits,
                     uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n);

/* Upper bound, in bytes, of the stream spiht_encode_i32 can produce for this geometry when the largest
 * magnitude is max_abs (pass 0x3FFFFFFF if unknown).  Used by bindings to size `out`. */
int spiht_encode_bound(int64_t c, int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, uint32_t max_abs,
                       uint64_t max_bits, uint64_t *bound_bytes);

/* Replaces `decode(data_u8, n, c, h, w, ll_h, ll_w) -> ndarray[int32,(c,h,w)]`  (src/lib.rs:35-42 ->
 * encoder_decoder.rs:307-454).  All 8*nbytes bits are data (lib.rs:38).  out: c*h*w int32, C-contiguous,
 * fully written (zeros where nothing was decoded). */
int spiht_decode_i32(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t h,
                     int64_t w, int64_t ll_h, int64_t ll_w, int32_t *out);

/* Replaces `decode_with_metadata(data_u8, n, c, h, w, ll_h, ll_w, top_slice, other_slices)
 *           -> (ndarray[int32,(c,h,w)], ndarray[int32,(8*nbytes+1, 8)])`
 * (src/lib.rs:47-56 -> encoder_decoder.rs:631-841, Slices::from_vec :482-527).
 * top_slice: {start_i, end_i, start_j, end_j} of the LL block; other_slices: [level][3][4], coarsest level
 * first, per level the three filters in the caller's order (the reference wrapper passes da, ad, dd,
 * spiht_wrapper.py:240), each {start_i, end_i, start_j, end_j}.  level = other_slices.len().
 * meta: (8*nbytes + 1) rows of 8 int32 {action 0..6, local_h, local_w, channel, filter 0..3, depth, n, value of
 * the coefficient before the bit is read} (doc comment :616-630); row t describes the operation that reads
 * stream bit t, row 8*nbytes the operation left waiting when the stream ended, rows of bits that were never
 * reached are zero.
 * Errors: SPIHT_ERR_SHAPE when the tree is deeper than `level` (the reference indexes other_slices out of
 * bounds -> panic, :603), when a slice is empty or reversed (end <= start, usize underflow) or c*h*w >= 2^28. */
int spiht_decode_with_metadata_i32(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                   int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, const int64_t *top_slice,
                                   const int64_t *other_slices, int64_t level, int32_t *out, int32_t *meta);

/* ---------------------------------------------------------------------------------------
 * Batched, device-resident forms (new; the reference codes one image per call).
 * All pointers below are DEVICE pointers (hipMalloc'd by anyone, e.g. a torch tensor's data_ptr()).
 * Work is queued on the context's stream; call spiht_ctx_synchronize() before reading results.
 * ------------------------------------------------------------------------------------- */

/* B images of identical geometry. d_x: int32 [B,c,h,w] contiguous.
 * d_out: B slots of slot_stride bytes (multiple of 4, >= ceil(min(max_bits,bound)/8) rounded up to 4);
 * bytes past ceil(nbits/8) in a slot are zeroed.  d_nbits: uint64 [B].  d_max_n: uint8 [B]. */
int spiht_encode_batch_i32(spiht_ctx *ctx, const int32_t *d_x, int64_t B, int64_t c, int64_t h, int64_t w,
                           int64_t ll_h, int64_t ll_w, uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride,
                           uint64_t *d_nbits, uint8_t *d_max_n);

/* d_data: B slots of slot_stride bytes (multiple of 4); d_nbytes: uint64 [B] valid bytes per slot
 * (all 8*nbytes bits are data); d_max_n: uint8 [B]; d_out: int32 [B,c,h,w], fully written. */
int spiht_decode_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                           const uint8_t *d_max_n, int64_t B, int64_t c, int64_t h, int64_t w, int64_t ll_h,
                           int64_t ll_w, int32_t *d_out);

/* decode_with_metadata of B streams at once (spiht_decode_with_metadata_i32 per stream, in one queue of work).
 * d_data / slot_stride / d_nbytes / d_max_n: device, as in spiht_decode_batch_i32; top_slice / other_slices / level: HOST
 * arrays, as in spiht_decode_with_metadata_i32 (read during the call only).  d_meta: device int32 [B, meta_rows, 8],
 * meta_rows >= 8 * slot_stride + 1: rows [0, 8 * nbytes[b] + 1) of image b are what spiht_decode_with_metadata_i32 returns
 * for that stream, every later row is zero.  d_out: device int32 [B, c, h, w] receiving the decoded arrays, or NULL.
 * Host-side errors as the single call (SPIHT_ERR_SHAPE: tree deeper than `level`, a reversed slice; SPIHT_ERR_TOO_LARGE:
 * c*h*w >= 2^28 or slot_stride >= 2^28), SPIHT_ERR_ARG for NULL pointers, slot_stride % 4 or meta_rows too small; B == 0
 * does nothing.  max_n > 30 and nbytes > slot_stride are reported by spiht_ctx_synchronize().  Asynchronous.
 * The images go in chunks; the context's scratch for a chunk -- the trace and the sort buffers, 21 bytes per record of
 * (8 * slot_stride + 1) per image, plus rocPRIM's temporary for sorting them -- stays within 2 GiB (one image that needs
 * more goes alone), whatever B is; with d_out NULL also a chunk's coefficient arrays.  Option "meta_chunk" (0: by that
 * bound) caps the images per chunk. */
int spiht_decode_with_metadata_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                         const uint8_t *d_max_n, int64_t B, int64_t c, int64_t h, int64_t w, int64_t ll_h,
                                         int64_t ll_w, const int64_t *top_slice, const int64_t *other_slices, int64_t level,
                                         int32_t *d_out, int32_t *d_meta, uint64_t meta_rows);

/* ---------------------------------------------------------------------------------------
 * Fused image path: pixels -> DWT -> quantise -> SPIHT and back, everything in HBM.
 * Mirrors spiht_wrapper.encode_image / decode_image (wrapper:142-216) without colour conversion.
 * ------------------------------------------------------------------------------------- */

/* Geometry of the packed coefficient array for an H x W image (wrapper:92-139, pywt.wavedecn_shapes).
 * level < 0 means "None" (pywt's maximum useful level).  Any out pointer may be NULL. */
/* Every discrete wavelet of PyWavelets, 106 names (the reference hands SpihtSettings.wavelet to pywt as it is,
 * spiht_wrapper.py:163, :276): haar, db1-38, sym2-20, coif1-17, bior / rbio 1.1 ... 6.8, dmey (csrc/wavelets.h, generated
 * from PyWavelets by tools/gen_wavelets.py).  Filters of up to 20 taps run in the tiled level kernels; longer ones (up to
 * 102 taps) in the plain two-pass levels, their filters read from device memory.  Ids are positions in that table:
 * bior2.2 = 0, bior4.4 = 1, bior6.8 = 2, haar = 3. */
int spiht_wavelet_id(const char *name);           /* < 0 if unknown */
int spiht_wavelet_taps(int wavelet);              /* filter length (pywt dec_len); < 0: no such id */
int spiht_mode_id(const char *name);              /* the pywt names of the nine modes above; <0 if unknown */
int spiht_geometry(int64_t H, int64_t W, int wavelet, int level, int *level_used, int64_t *ll_h, int64_t *ll_w,
                   int64_t *enc_h, int64_t *enc_w, int64_t *rec_H, int64_t *rec_W);
/* ... for an extension mode: periodization has its own sizes (pywt.dwt_coeff_len), every other mode those above */
int spiht_geometry_mode(int64_t H, int64_t W, int wavelet, int mode, int level, int *level_used, int64_t *ll_h, int64_t *ll_w,
                        int64_t *enc_h, int64_t *enc_w, int64_t *rec_H, int64_t *rec_W);

/* Every image call below -- batched or host, any pixel format, forward, inverse, fused, two-part, reduced -- takes at most
 * 65535 planes per picture: c > 65535 is SPIHT_ERR_TOO_LARGE before anything is queued and before the geometry is looked
 * at.  A batch is cut into launches of at most 65535 planes between pictures, never inside one, and a launch carries its
 * planes in grid.y / grid.z.  spiht_encode_batch_i32 has the same limit and the same status; spiht_pyramid_batch_i32
 * takes at most 65535 planes in the whole call (SPIHT_ERR_ARG beyond).
 *
 * d_img: float64 [B,c,H,W] (device).  channel_mults: HOST array of c doubles or NULL
 * (SpihtSettings.per_channel_quant_scales); q_scale: SpihtSettings.quantization_scale.
 * Outputs as spiht_encode_batch_i32.  d_coeffs: optional device int32 [B,c,enc_h,enc_w] that receives the
 * quantised coefficient array handed to the coder (NULL to keep it in scratch). */
int spiht_encode_image_batch_f64(spiht_ctx *ctx, const double *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                                 int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                 uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride, uint64_t *d_nbits,
                                 uint8_t *d_max_n, int32_t *d_coeffs);

/* Inverse: streams -> float64 [B,c,rec_H,rec_W] (rec_H/rec_W from spiht_geometry; may exceed H/W by one on
 * odd axes exactly as pywt.waverec2 does).  d_rec: optional device int32 [B,c,enc_h,enc_w] receiving the
 * decoded coefficient array. */
int spiht_decode_image_batch_f64(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                 const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H,
                                 int64_t W, int wavelet, int mode, int level, double q_scale,
                                 const double *channel_mults, double *d_img_out, int32_t *d_rec);

/* ---- 8-bit pixels (*_u8) ----------------------------------------------------------------------------------------
 * A uint8 picture batch [B, c, H, W] is described by byte strides (sb, sc, sh, sw) (one picture: (sc, sh, sw)); NULL
 * means dense CHW.  That covers planar CHW, interleaved HWC (sc = 1, sw = c) and, with c = 3 and sw = 4, an RGBA buffer
 * whose alpha byte is never read and never written.  Strides are non-negative; an OUTPUT view must not overlap itself:
 * sorted by stride, every dimension longer than one must step past the largest offset the smaller ones reach.  Anything
 * else: SPIHT_ERR_ARG before anything is queued.
 *   encode: sample k is coded as the double k / 255.0 (exactly numpy's P / 255), then the float64 path, colour model
 *           change included -- the streams equal spiht_encode_image_batch_f64's of P / 255.
 *   decode: the float64 result v is stored as (uint8)(clip(v, 0, 1) * 255.0), truncated, CROPPED to H x W (the float64
 *           decode's rec_H x rec_W is one longer on an odd axis); NaN is stored as 0.
 * Level 1 of the transforms reads / writes the bytes itself; level 0 and the two-pass levels convert through a float64
 * pass of their own.
 *
 * 16-bit pixels (*_u16): the same rules for a uint16 batch (native byte order) with 65535 in place of 255 -- sample k is
 * coded as the double k / 65535.0, a result v is stored as (uint16)(clip(v, 0, 1) * 65535.0), truncated, NaN as 0.  The
 * strides are still BYTE strides (numpy's .strides as they are); in addition every stride must be a multiple of 2 and
 * the base pointer 2-byte aligned, and the overlap rule of an output view counts the sample's two bytes: every dimension
 * longer than one must step past the last byte the smaller ones reach.  Interleaved HWC is sc = 2, sw = 2c; a 16-bit
 * RGBA buffer is c = 3, sw = 8.  A stream does not record the pixel format it came from: any stream decodes into any
 * format.  Each *_u16 call below is its *_u8 sibling in everything else: statuses, asynchrony, chunking. */
/* The rule above on its own (no device work, no context): SPIHT_OK or SPIHT_ERR_ARG for the strides[4] of a [B, c, H, W]
 * view that is read (output 0) or written (output 1). */
int spiht_check_view_u8(int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output);
int spiht_check_view_u16(int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output);
int spiht_encode_image_batch_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                const double *channel_mults, uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride,
                                uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs);
int spiht_encode_image_batch_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t B, int64_t c,
                                 int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                 const double *channel_mults, uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride,
                                 uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs);
int spiht_decode_image_batch_u8(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H,
                                int64_t W, int wavelet, int mode, int level, double q_scale,
                                const double *channel_mults, uint8_t *d_img_out, const int64_t *out_strides,
                                int32_t *d_rec);
int spiht_decode_image_batch_u16(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                 const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H,
                                 int64_t W, int wavelet, int mode, int level, double q_scale,
                                 const double *channel_mults, uint16_t *d_img_out, const int64_t *out_strides,
                                 int32_t *d_rec);

/* DWT halves on their own (device pointers), for parity tests and profiling:
 * forward: float64 [B,c,H,W] -> int32 [B,c,enc_h,enc_w] (quantised, zero padded)  (wrapper:163-172)
 * inverse: int32 [B,c,enc_h,enc_w] -> float64 [B,c,rec_H,rec_W]                   (wrapper:259-276) */
int spiht_dwt_quant_batch_f64(spiht_ctx *ctx, const double *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                              int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                              int32_t *d_coeffs);
int spiht_dequant_idwt_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                 int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                 double *d_img_out);

/* Single-precision forms of the two encode-side entry points: d_img float32 [B,c,H,W].  PyWavelets transforms
 * float32 (and float16) pixels in float32 and the reference wrapper quantises the float32 array in float32
 * (`pywt.wavedec2` dtype rule, spiht_wrapper.py:163-172) -- so a float32 image does not give the stream its float64
 * copy gives; these reproduce the float32 result, including pywt's order of additions at the right / bottom edge.
 * (Levels above pywt's dwt_max_level -- inputs shorter than the filter -- are coded as PyWavelets codes them, in either
 * precision: it only warns, spiht_wrapper.py:163.)  SPIHT_ERR_ARG for level == 0.
 * The decode side is float64 in the reference whatever the pixels were. */
int spiht_dwt_quant_batch_f32(spiht_ctx *ctx, const float *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                              int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                              int32_t *d_coeffs);
int spiht_encode_image_batch_f32(spiht_ctx *ctx, const float *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                                 int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                 uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride, uint64_t *d_nbits,
                                 uint8_t *d_max_n, int32_t *d_coeffs);

/* Significance pyramid on its own (device pointers), for parity tests and profiling:
 * d_x int32 [B,c,h,w] -> d_dmsb, d_lmsb uint8 [B,c,h,w] (1 + msb of the D / L set maxima of the node with
 * that index, 0 = empty/zero; only nodes with offspring are written) and d_maxabs uint32 [B] (NULL: not computed). */
int spiht_pyramid_batch_i32(spiht_ctx *ctx, const int32_t *d_x, int64_t B, int64_t c, int64_t h, int64_t w,
                            int64_t ll_h, int64_t ll_w, uint8_t *d_dmsb, uint8_t *d_lmsb, uint32_t *d_maxabs);

/* The two halves of each direction on their own (device pointers, asynchronous).  The transform + pyramid half is
 * HBM-bound, the list-coding half is latency-bound and leaves the HBM idle, so a caller that keeps several batches in
 * flight runs them on two contexts ordered with events (bench.py):
 *   spiht_dwt_pyramid_batch_f64   pixels -> coefficients + D/L pyramid + max|coef|   (front half of encode_image);
 *                                 with d_dmsb = d_lmsb = NULL the pyramid is left out and can be queued on another
 *                                 context with spiht_pyramid_batch_i32(..., d_maxabs = NULL) (NULL: max|coef| is
 *                                 already known, no pass over the coefficients for it)
 *   spiht_encode_lists_batch_i32  coefficients + pyramid -> streams                  (back half; = k_encode)
 *   spiht_decode_lists_batch_i32  streams -> coefficients; d_out must be ZERO-FILLED by the caller (spiht_dev_memset)
 *   spiht_dequant_idwt_batch_f64  coefficients -> pixels                             (above)
 *   spiht_unscatter_lists_batch_i32  after the inverse transform has read d_out: puts back the zeros in exactly the
 *                                 cells the context's last spiht_decode_lists_batch_i32 wrote (through the decoder's
 *                                 lists), so the array is zero again for the next decode without a full zero-fill;
 *                                 falls back to the zero-fill when another list-coding call on the context came in
 *                                 between.  (The reference allocates a fresh zero array per call,
 *                                 encoder_decoder.rs:308; this keeps one array zero instead.)
 * Results are identical to the fused entry points. */
int spiht_dwt_pyramid_batch_f64(spiht_ctx *ctx, const double *d_img, int64_t B, int64_t c, int64_t H, int64_t W,
                                int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb, uint32_t *d_maxabs);
/* ... of 8-bit / 16-bit pictures (strides[4] as spiht_encode_image_batch_u8 / _u16) */
int spiht_dwt_pyramid_batch_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t B, int64_t c, int64_t H,
                               int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                               int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb, uint32_t *d_maxabs);
int spiht_dwt_pyramid_batch_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t B, int64_t c, int64_t H,
                                int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb, uint32_t *d_maxabs);
int spiht_encode_lists_batch_i32(spiht_ctx *ctx, const int32_t *d_x, const uint8_t *d_dmsb, const uint8_t *d_lmsb,
                                 const uint32_t *d_maxabs, int64_t B, int64_t c, int64_t h, int64_t w, int64_t ll_h,
                                 int64_t ll_w, uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride,
                                 uint64_t *d_nbits, uint8_t *d_max_n);
int spiht_decode_lists_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                 const uint8_t *d_max_n, int64_t B, int64_t c, int64_t h, int64_t w, int64_t ll_h,
                                 int64_t ll_w, int32_t *d_out_zeroed);
int spiht_unscatter_lists_batch_i32(spiht_ctx *ctx, int32_t *d_out, int64_t B, int64_t c, int64_t h, int64_t w);
/* Occupancy of the inverse transform's level-1 tiles, handed from the list decoder to the inverse transform.  The
 * reference's decoder fills a dense array and waverec2 reads all of it (spiht_wrapper.py:248-276); at the metric's bit
 * rates nearly every cell of the level-1 detail bands -- three quarters of the array -- is zero, and the decoder knows
 * every cell it writes: it sets one 32-bit word per (plane, inverse-transform tile) whose staged band region holds a
 * decoded cell, and level 1 of the inverse transform does not read the detail bands of a tile whose word is zero (zeros go
 * through the same arithmetic: the same bits).  The image-level decode calls do this internally (option "l1_flags");
 * the split calls take the words explicitly:
 *   spiht_l1_flags_words                 words per image for this geometry (0: not applicable -- fewer than two levels,
 *                                        periodization)
 *   spiht_decode_lists_flags_batch_i32   spiht_decode_lists_batch_i32 for the arrays of H x W images + the words
 *                                        (zero-filled by the call; d_flags NULL: no flags)
 *   spiht_dequant_idwt_flags_batch_f64   spiht_dequant_idwt_batch_f64 reading them (d_flags NULL: reads everything) */
int spiht_l1_flags_words(int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, uint64_t *words_per_image);
int spiht_decode_lists_flags_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                       const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                       int mode, int level, int32_t *d_out_zeroed, uint32_t *d_flags);
/* Row words: a second array of the same size and geometry as the words (spiht_l1_flags_words x B, [planes, gy, gx]).  Bit r
 * of a tile's row word, 0 <= r < 12 + F/2 - 1, is set when band row r of the region that tile stages (its 12 band rows and
 * the F/2 - 1 halo rows behind them, every staged column, any of the three level-1 detail bands) holds a decoded cell.  A few
 * hundred scattered cells per plane set 40 % of the words but under 5 % of the rows; spiht_idwt_level1_rows_batch_* neither
 * reads nor filters the detail rows whose bit is clear (same bits: a clear row is +0.0 throughout, and y + 0.0 == y).  The
 * words themselves stay 0 / 1.  d_rows is zero-filled by the call -- in one fill with the words when d_rows == d_flags +
 * the words' count, so lay them out as one buffer.  d_rows NULL: spiht_decode_lists_flags_batch_i32; ignored without d_flags.
 * Additions only: the version stays at 2. */
int spiht_decode_lists_rows_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                      const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                      int mode, int level, int32_t *d_out_zeroed, uint32_t *d_flags, uint32_t *d_rows);
int spiht_dequant_idwt_flags_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B, int64_t c,
                                       int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                       const double *channel_mults, double *d_img_out);
/* ... into 8-bit / 16-bit pictures (out_strides[4] and the crop as spiht_decode_image_batch_u8 / _u16) */
int spiht_dequant_idwt_flags_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B, int64_t c,
                                      int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                      const double *channel_mults, uint8_t *d_img_out, const int64_t *out_strides);
int spiht_dequant_idwt_flags_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, const uint32_t *d_flags, int64_t B, int64_t c,
                                       int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                       const double *channel_mults, uint16_t *d_img_out, const int64_t *out_strides);
/* Switches of this library's own making; the results are the same bits whatever they are set to.  "l1_flags" (default 1):
 * the occupancy words above inside the image-level decode calls; "pads_persist" (default 0): the caller promises that a
 * coefficient array this context's forward transform has filled is not written by anyone else before the same context
 * fills it again with the same geometry -- the zero padding of coeffs_to_array is then written once per array instead
 * of once per call (a caller that recycles its arrays, e.g. the pipelined schedule).  Those two: value 0 / 1.
 * "wide_encode" (default 1): an encode call of few images (at most half as many as the device has CUs, each of 2^18
 * coefficients or more) codes each image on a group of workgroups, one per CU, instead of one workgroup -- the latency of a
 * single call (csrc/encode_wide.hip); 0: always one workgroup per image; 2: groups whatever the size of the image
 * (tests); 3: as 2, and every group finds itself "given up" (tests of the fallback below).  "wide_groups" (default 0 = by
 * image size, 2 ... 64): workgroups per image of that path, 0 ... 256; "wide_solo" (default 24576): list entries up to
 * which a bit plane is still coded by the group's first workgroup alone.  The workgroups of a group wait for one another
 * and should all be resident: the library keeps a launch within what the device holds of that kernel and queues such
 * launches of one process one at a time per device; when other work holds the CUs all the same (another process, a long
 * kernel of the caller's), a group gives up after a bounded wait (tens of milliseconds) and the image is coded by one
 * workgroup instead, queued behind on the same stream -- same bits, never an error (spiht_ctx_wide_stats tells).
 * "idwt_groups" (default 0 = 4): persistent workgroups per CU of the large inverse-transform levels; 3 leaves a list
 * decoder's workgroup room beside them (the pipelined schedule sets it around its own calls).  "meta_chunk" (default 0 =
 * by the scratch bound, up to 65535): images per chunk of spiht_decode_with_metadata_batch_i32. */
int spiht_ctx_set_option(spiht_ctx *ctx, const char *name, int64_t value);
int spiht_ctx_get_option(spiht_ctx *ctx, const char *name, int64_t *value);
/* The last encode call of this context that took the several-CUs-per-image path: its images (groups) and how many of them
 * gave up for lack of residency and were coded by the single-workgroup kernel instead.  Waits for the context's stream. */
int spiht_ctx_wide_stats(spiht_ctx *ctx, uint32_t *groups, uint32_t *gave_up);

/* The inverse transform (spiht_dequant_idwt_batch_f64) in two parts, for the same kind of schedule: the coarse levels
 * (level .. 2: a quarter of the bytes) into d_approx [B*c, 2*hs[2]-F+2, 2*ws[2]-F+2] float64 -- the approximation level 1
 * starts from; spiht_idwt_approx_shape gives its size -- and level 1 from d_rec + d_approx to the pixels.  With fewer than
 * two levels the coarse call does nothing and level 1 does everything.  Same bits as the one-call form. */
int spiht_idwt_coarse_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                double *d_approx);
int spiht_idwt_level1_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, int64_t B, int64_t c,
                                int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                const double *channel_mults, double *d_img_out);
int spiht_idwt_approx_shape(int64_t H, int64_t W, int wavelet, int level, int64_t *a_h, int64_t *a_w);
/* ... level 1 reading the decoder's occupancy words (spiht_decode_lists_flags_batch_i32; d_flags NULL: reads everything) */
int spiht_idwt_level1_flags_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                      int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                      const double *channel_mults, double *d_img_out);
/* ... into 8-bit / 16-bit pictures (out_strides[4] and the crop as spiht_decode_image_batch_u8 / _u16) */
int spiht_idwt_level1_flags_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                     int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                     const double *channel_mults, uint8_t *d_img_out, const int64_t *out_strides);
int spiht_idwt_level1_flags_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                      int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                      const double *channel_mults, uint16_t *d_img_out, const int64_t *out_strides);
/* ... and the decoder's row words (spiht_decode_lists_rows_batch_i32): per tile the mask of staged detail rows to read and to
 * filter is its row word; d_rows NULL: the _flags_ call (a set word: every row); ignored without d_flags.  The same pictures,
 * bit for bit, whatever bits are set beyond the rows that hold a cell. */
int spiht_idwt_level1_rows_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                     const uint32_t *d_rows, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                                     int level, double q_scale, const double *channel_mults, double *d_img_out);
int spiht_idwt_level1_rows_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                    const uint32_t *d_rows, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                                    int level, double q_scale, const double *channel_mults, uint8_t *d_img_out,
                                    const int64_t *out_strides);
int spiht_idwt_level1_rows_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, const double *d_approx, const uint32_t *d_flags,
                                     const uint32_t *d_rows, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                                     int level, double q_scale, const double *channel_mults, uint16_t *d_img_out,
                                     const int64_t *out_strides);

/* Colour model change on the device (the reference converts on the host through colour-science, color_models.py:6-13,
 * called from spiht_wrapper.py:158-160 and :278-279): B three-channel float64 images [B,3,npix]; per pixel
 * w = M * spow(A * u, p) with spow(x, p) = sign(x)|x|^p -- RGB -> IPT is (XYZ->LMS * RGB->XYZ, 0.43, LMS->IPT), the way
 * back the inverses with 1/0.43.  A, M: row-major 3x3 host arrays.  d_out may equal d_in.  Asynchronous. */
int spiht_color3_batch_f64(spiht_ctx *ctx, const double *d_in, double *d_out, int64_t B, int64_t npix, const double *A,
                           const double *M, double p);
/* The colour model of the coded picture as a property of the context (spiht_wrapper.py:158-160, :278-279: RGB -> model
 * before the transform, model -> RGB after the inverse transform), fused into the transform: while set, every image-level
 * entry point of the context takes and returns RGB pixels of 3-channel float64 images and codes them in the other model --
 * the forward level-1 kernel converts on its loads (w = M_f * spow(A_f * u, p_f)), the inverse level-1 kernel on its
 * stores (A_i, M_i, p_i); the converted picture never exists in memory.  Same bits as spiht_color3_batch_f64 followed by
 * the plain transform.  A_f == NULL clears the setting.  Images with other channel counts are coded as they are. */
int spiht_ctx_set_color3(spiht_ctx *ctx, const double *A_f, const double *M_f, double p_f, const double *A_i,
                         const double *M_i, double p_i);
/* ... and what is set at the moment (*on == 0: nothing, the arrays are left alone; output pointers other than `on` may be
 * NULL) -- for code that borrows a context and puts the caller's setting back (csrc/pipeline.cpp). */
int spiht_ctx_get_color3(spiht_ctx *ctx, int *on, double *A_f, double *M_f, double *p_f, double *A_i, double *M_i, double *p_i);

/* Progressive decoding of one stream to K bit budgets from ONE walk (the reference decodes a prefix per frame,
 * make_gif.py:46-61: `decode(original_bytes[:byte_len], ...)`, i.e. K walks).  budgets_bits: host array,
 * ascending (else SPIHT_ERR_ARG); out[k] = what spiht_decode_i32 returns for the first budgets_bits[k] bits of the
 * stream (8 x a byte length for a byte prefix; a budget past the end means the whole stream) -- bit-exact, duplicated
 * tree nodes included.  The walk records which list entry every stream position belongs to (as decode_with_metadata,
 * src/encoder_decoder.rs:631-841), the records are sorted by node, and one thread per node replays the node's operations
 * once, leaving its value in every budget it passes.
 *   spiht_decode_budgets_i32      out: host int32 [K, c, h, w]; synchronous
 *   spiht_decode_budgets_dev_i32  d_out: device int32 [K, c, h, w] (zero-filled by the call); asynchronous apart from
 *                                 the upload of the stream (feeds spiht_dequant_idwt_batch_f64 with B = K) */
int spiht_decode_budgets_i32(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t h, int64_t w,
                             int64_t ll_h, int64_t ll_w, const uint64_t *budgets_bits, int64_t K, int32_t *out);
int spiht_decode_budgets_dev_i32(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t h,
                                 int64_t w, int64_t ll_h, int64_t ll_w, const uint64_t *budgets_bits, int64_t K, int32_t *d_out);

/* The context's (recursive) mutex held across a SEQUENCE of calls by one thread: spiht_ctx_set_color3 is state of the
 * context, so set / image calls / clear must not interleave with another thread's calls on the same context (those
 * would be coded in the wrong colour model, silently).  spiht_amd.color_models.fused brackets its block with these.
 * Unlock from the thread that locked.  (The reference's colour step is a pure function of the pixel array,
 * spiht_wrapper.py:158-160 -- there is no shared state to protect there.) */
int spiht_ctx_lock(spiht_ctx *ctx);
int spiht_ctx_unlock(spiht_ctx *ctx);

/* Wavefronts per workgroup of the list decoder on this context: 12 (default; the shortest walk of one stream) or 8
 * (4 % slower alone, a lighter neighbour for HBM-bound kernels running beside it on other contexts -- what the
 * pipelined schedule uses for its list-coding contexts).  Output identical.  Other values: SPIHT_ERR_ARG.
 * Replaces nothing in the reference (src/encoder_decoder.rs:307-454 is one thread); a scheduling knob of this library. */
int spiht_ctx_set_decoder_waves(spiht_ctx *ctx, int waves);

/* d_nbytes[b] = ceil(d_nbits[b] / 8) for b < B (device arrays): turns the encoder's bit counts into the byte
 * counts the decoder takes, without a host round trip. */
int spiht_nbits_to_nbytes(spiht_ctx *ctx, const uint64_t *d_nbits, int64_t B, uint64_t *d_nbytes);

/* The drop-in calls on HOST arrays, one C call each (what spiht_amd.encode_image / decode_image / decode_from_rec_arr
 * bind): replace encode_image (spiht_wrapper.py:142-189: wavedec2 -> coeffs_to_array -> channel scales -> quantize ->
 * spiht.encode), decode_image (:192-216, :259-276: spiht.decode -> dequantize -> waverec2) and decode_from_rec_arr
 * (:259-276) without the colour step.  img: [c,H,W] C-contiguous; out / out_cap as in spiht_encode_i32; img_out:
 * float64 [c, rec_H, rec_W] (spiht_geometry).  Pixels, coefficients and stream stay in the context's grow-only device
 * buffers: no device allocation per call once a size has been seen.  Synchronous. */
int spiht_encode_image_host_f64(spiht_ctx *ctx, const double *img, int64_t c, int64_t H, int64_t W, int wavelet,
                                int mode, int level, double q_scale, const double *channel_mults, uint64_t max_bits,
                                uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n);
int spiht_encode_image_host_f32(spiht_ctx *ctx, const float *img, int64_t c, int64_t H, int64_t W, int wavelet,
                                int mode, int level, double q_scale, const double *channel_mults, uint64_t max_bits,
                                uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n);
int spiht_decode_image_host_f64(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H,
                                int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                double *img_out);
int spiht_dequant_idwt_host_f64(spiht_ctx *ctx, const int32_t *rec, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                                int level, double q_scale, const double *channel_mults, double *img_out);
/* 8-bit and 16-bit pixels on the host (see the *_u8 / *_u16 batch calls): strides[3] = (sc, sh, sw) in bytes, NULL =
 * dense CHW.  Encode uploads only the bytes the strides span (an RGBA buffer's first three channels need no host copy).  Decode writes
 * img_out cropped to c x H x W, which must be dense CHW or dense HWC (anything else: SPIHT_ERR_ARG). */
int spiht_encode_image_host_u8(spiht_ctx *ctx, const uint8_t *img, const int64_t *strides, int64_t c, int64_t H, int64_t W,
                               int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                               uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n);
int spiht_encode_image_host_u16(spiht_ctx *ctx, const uint16_t *img, const int64_t *strides, int64_t c, int64_t H, int64_t W,
                                int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n);
int spiht_decode_image_host_u8(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H,
                               int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                               uint8_t *img_out, const int64_t *strides);
int spiht_decode_image_host_u16(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H,
                                int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                uint16_t *img_out, const int64_t *strides);

/* ---------------------------------------------------------------------------------------
 * Reduced-resolution decode: the picture at 1/2^reduce size straight from a stream (what JPEG 2000 calls resolution
 * levels).  The coefficient array is a Mallat pyramid, and pywt.waverec2 passes through the picture at 1/2, 1/4, ... size
 * on its way up: a reduced decode runs levels L .. reduce + 1 of the inverse transform and nothing below, 0 <= reduce <= L
 * (L: the levels used; anything else: SPIHT_ERR_ARG before anything is queued).  With hs[l], ws[l] the band sizes of the
 * geometry (hs[0] = H), F the filter length (2 under periodization) and D = (rec / channel_mults) / q_scale:
 *   float64   R = pywt.waverec2(coeffs[:L - reduce + 1], wavelet, mode) * 2^-reduce, uncropped as the full-size calls:
 *             [c, 2 hs[reduce+1] - F + 2, 2 ws[reduce+1] - F + 2]; reduce == L: D[:, :ll_h, :ll_w] * 2^-L.  The factor
 *             takes out the approximation band's DC gain of 2 per level; it is applied as q_scale * 2^reduce, which is
 *             exact (a q_scale for which that overflows: SPIHT_ERR_ARG).  reduce == 0: the full-size call in every bit.
 *   colour    with spiht_ctx_set_color3 set, the model -> RGB change per pixel of R (three channels)
 *   8/16-bit  (uintN)(clip(R, 0, 1) * 255 or 65535) cropped to [c, hs[reduce], ws[reduce]]: the rule of the *_u8 / *_u16
 *             calls one pyramid level up; strides are those of that picture
 * R is PyWavelets' approximation band: it carries a rim of extension samples, hs[reduce] >= ceil(H / 2^reduce).
 * The list decoder parses every bit whatever the resolution; what is saved is the inverse transform's fine levels, their
 * HBM traffic and the bytes of the picture. */
/* Sizes of a reduced decode; pure arithmetic, no device.  rec_h x rec_w: the float64 picture; pic_h x pic_w: the integer
 * picture (hs[reduce] x ws[reduce]); in_h x in_w = ceil(H / 2^reduce) x ceil(W / 2^reduce), the size a 2^reduce-fold
 * downsampling of the picture has, and off_y, off_x where that window lies centred in either picture:
 * (pic - in) / 2, rounded down; 0 under periodization.  Output pointers may be NULL. */
int spiht_reduced_shape(int64_t H, int64_t W, int wavelet, int mode, int level, int reduce, int *level_used, int64_t *rec_h,
                        int64_t *rec_w, int64_t *pic_h, int64_t *pic_w, int64_t *off_y, int64_t *off_x, int64_t *in_h,
                        int64_t *in_w);
/* spiht_dequant_idwt_batch_f64 / spiht_dequant_idwt_flags_batch_u8 / _u16 (without occupancy words: they belong to level 1)
 * at reduced size: device coefficient arrays [B, c, enc_h, enc_w] -> pictures.  Asynchronous. */
int spiht_dequant_idwt_reduced_batch_f64(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                         int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                         double *d_img_out, int reduce);
int spiht_dequant_idwt_reduced_batch_u8(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                        int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                        uint8_t *d_img_out, const int64_t *out_strides, int reduce);
int spiht_dequant_idwt_reduced_batch_u16(spiht_ctx *ctx, const int32_t *d_rec, int64_t B, int64_t c, int64_t H, int64_t W,
                                         int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                         uint16_t *d_img_out, const int64_t *out_strides, int reduce);
/* spiht_decode_image_batch_f64 / _u8 / _u16 at reduced size: streams in device slots -> pictures.  Asynchronous as those;
 * the internal coefficient array is left all zero, as after a full-size call. */
int spiht_decode_image_reduced_batch_f64(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                         const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                         int mode, int level, double q_scale, const double *channel_mults, double *d_img_out,
                                         int32_t *d_rec, int reduce);
int spiht_decode_image_reduced_batch_u8(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                        const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                        int mode, int level, double q_scale, const double *channel_mults, uint8_t *d_img_out,
                                        const int64_t *out_strides, int32_t *d_rec, int reduce);
int spiht_decode_image_reduced_batch_u16(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                         const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet,
                                         int mode, int level, double q_scale, const double *channel_mults, uint16_t *d_img_out,
                                         const int64_t *out_strides, int32_t *d_rec, int reduce);
/* spiht_decode_image_host_f64 / _u8 / _u16 at reduced size: one stream in a host array -> one picture in a host array of the
 * reduced size (img_out: float64 [c, rec_h, rec_w]; integer [c, pic_h, pic_w], dense CHW or HWC): only the reduced
 * picture's bytes cross the link.  Synchronous. */
int spiht_decode_image_reduced_host_f64(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H,
                                        int64_t W, int wavelet, int mode, int level, double q_scale,
                                        const double *channel_mults, double *img_out, int reduce);
int spiht_decode_image_reduced_host_u8(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H,
                                       int64_t W, int wavelet, int mode, int level, double q_scale,
                                       const double *channel_mults, uint8_t *img_out, const int64_t *strides, int reduce);
int spiht_decode_image_reduced_host_u16(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H,
                                        int64_t W, int wavelet, int mode, int level, double q_scale,
                                        const double *channel_mults, uint16_t *img_out, const int64_t *strides, int reduce);

/* ---------------------------------------------------------------------------------------
 * Rate-distortion reductions: how far K decoded versions of one picture are from the original, computed where they lie.
 * A SPIHT stream decodes at any prefix; spiht_decode_budgets_dev_i32 + spiht_dequant_idwt_batch_* give the K coefficient
 * arrays and pictures of K prefixes in HBM, and these calls turn them into K small rows -- nothing but those rows has to
 * cross the link (spiht_amd/rd.py builds the curve and the cut to a target quality on them).  Additions only: the ABI
 * version stays at 2.  All pointers are DEVICE pointers; asynchronous on the context's stream like the *_batch_* calls;
 * argument errors are returned before anything is queued.  1 <= K <= 65535, c <= 65535, K*c < 2^31 (SPIHT_ERR_ARG /
 * _TOO_LARGE).  The per-workgroup partial sums live in a grow-only buffer of the context.
 *   spiht_sqerr_i32  d_x int32 [c, h, w], d_y int32 [K, c, h, w], dense; c*h*w < 2^28 (SPIHT_ERR_TOO_LARGE).
 *                    d_out uint64 [K][2] = (lo, hi) of E[k] = sum (x - y[k])^2 as an exact 128-bit unsigned integer.
 *   spiht_sse_f64    d_pic float64 [c, H, W], d_dec float64 [K, c, rec_h, rec_w] (uncropped, as the decode calls return
 *                    them; rec_h >= H and rec_w >= W, else SPIHT_ERR_ARG).  d_out double [K][c]: S[k, ch] = the sum over
 *                    the H x W window of (p - d) * (p - d), every term rounded and then added (no fused multiply-add), in
 *                    an order fixed by (H, W) alone: the same bits from call to call, for any K and wherever a picture
 *                    lies in d_dec.  H*W < 2^30.
 *   spiht_sse_u8 / _u16  d_pic: the original by byte strides[3] = (sc, sh, sw) (NULL: dense CHW), under the rules of
 *                    spiht_check_view_u8 / _u16 for a view that is read; d_dec uint8 / uint16 [K, c, H, W] dense.
 *                    d_out uint64 [K][c], exact (65535^2 * 2^30 < 2^63: H*W < 2^30). */
int spiht_sqerr_i32(spiht_ctx *ctx, const int32_t *d_x, const int32_t *d_y, int64_t K, int64_t c, int64_t h, int64_t w,
                    uint64_t *d_out);
int spiht_sse_f64(spiht_ctx *ctx, const double *d_pic, const double *d_dec, int64_t K, int64_t c, int64_t H, int64_t W,
                  int64_t rec_h, int64_t rec_w, double *d_out);
int spiht_sse_u8(spiht_ctx *ctx, const uint8_t *d_pic, const int64_t *strides, const uint8_t *d_dec, int64_t K, int64_t c,
                 int64_t H, int64_t W, uint64_t *d_out);
int spiht_sse_u16(spiht_ctx *ctx, const uint16_t *d_pic, const int64_t *strides, const uint16_t *d_dec, int64_t K, int64_t c,
                  int64_t H, int64_t W, uint64_t *d_out);

/* ---------------------------------------------------------------------------------------
 * Tiled pictures (csrc/tiles.hip): one picture as gy x gx equal tiles of th x tw, every tile coded as a picture of its own by
 * the batched calls above -- so a tile's stream is exactly what the single-image encode gives for the tile's pixels.  Tiles
 * are in row-major order; tile (i, j) covers rows i*th .. i*th+th-1 and columns j*tw .. j*tw+tw-1 of the picture EXTENDED BY
 * EDGE REPLICATION to (gy*th) x (gx*tw): numpy's np.pad(P, mode="edge").  One tile shape per picture, th, tw >= 8.
 * Additions only: the ABI version stays at 2; the next change of an EXISTING signature bumps it.
 * All pointers of the four copy calls are DEVICE pointers; they are asynchronous on the context's stream like the *_batch_*
 * calls, argument errors are returned before anything is queued, and no byte outside the stated output is written.
 *   spiht_tile_grid    gy = ceil(H / th), gx = ceil(W / tw); T = gy * gx.  Pure arithmetic, no device.  SPIHT_ERR_ARG for
 *                      H, W < 1 or th, tw < 8; SPIHT_ERR_TOO_LARGE for H, W >= 2^30 or th, tw > 2^24.
 *   spiht_tile_cut_*   d_img: N pictures [N, c, H, W] -> d_tiles: dense [N * T, c, th, tw] of the same element type (picture n's
 *                      tiles at rows [n*T, (n+1)*T)).  _u8 / _u16: strides[4] = (sb, sc, sh, sw) in bytes under the rules of
 *                      spiht_check_view_u8 / _u16 for a view that is read (NULL: dense CHW), so HWC and RGBA views are cut as
 *                      they lie; _f32 / _f64: dense CHW.  N * T < 2^31, c <= 65535.
 *   spiht_tile_paste_* d_tiles: dense [(i1-i0) * (j1-j0), c, rh, rw], the tiles of the sub-grid [i0, i1) x [j0, j1) in
 *                      row-major order, rh >= th, rw >= tw (the float64 decode's rec_H x rec_W is one longer on an odd axis;
 *                      the integer decodes are cropped already) -> d_out: the window [c, wh, ww] of the H x W picture whose
 *                      first sample is picture sample (y0, x0).  Every output sample comes from the one tile that owns it;
 *                      rows / columns >= th / tw of a tile and the replicated padding are never read into the window.  The
 *                      window must lie in the picture and the sub-grid must hold every tile it meets (SPIHT_ERR_ARG).
 *                      _u8 / _u16: out_strides[3] = (sc, sh, sw) in bytes under the rule for a view that is WRITTEN (NULL:
 *                      dense CHW): what lies between the view's samples -- an RGBA buffer's alpha -- is not written.
 *   spiht_tile_pack    T stream slots (slot_stride apart, as the batched encode calls leave them) + d_nbits [T] -> d_packed:
 *                      the streams' bytes one behind the other, stream t ceil(nbits[t] / 8) bytes long (the rounding of
 *                      spiht_nbits_to_nbytes), and d_lens: uint32 [T], those lengths.  An exclusive scan of the lengths on the
 *                      device, then the gather.  Nothing is written at or past d_packed + packed_cap (T * slot_stride always
 *                      suffices; the table tells the host what the run needs).  A zero-length stream and T = 1 are ordinary.
 *   spiht_tile_unpack  the inverse: d_packed (packed_bytes long) + d_lens [T] -> T slots, every byte of a slot past its
 *                      stream's end zero, and d_nbytes: uint64 [T] -- what the batched decode calls take.  A length is taken
 *                      as at most slot_stride; bytes a table claims past packed_bytes read as zero.
 * slot_stride: a multiple of 4, at most 2^29. */
int spiht_tile_grid(int64_t H, int64_t W, int64_t th, int64_t tw, int64_t *gy, int64_t *gx);
int spiht_tile_cut_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H, int64_t W,
                      int64_t th, int64_t tw, uint8_t *d_tiles);
int spiht_tile_cut_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H, int64_t W,
                       int64_t th, int64_t tw, uint16_t *d_tiles);
int spiht_tile_cut_f32(spiht_ctx *ctx, const float *d_img, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th, int64_t tw,
                       float *d_tiles);
int spiht_tile_cut_f64(spiht_ctx *ctx, const double *d_img, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th, int64_t tw,
                       double *d_tiles);
int spiht_tile_paste_u8(spiht_ctx *ctx, const uint8_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                        int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0, int64_t wh,
                        int64_t ww, uint8_t *d_out, const int64_t *out_strides);
int spiht_tile_paste_u16(spiht_ctx *ctx, const uint16_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                         int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                         int64_t wh, int64_t ww, uint16_t *d_out, const int64_t *out_strides);
int spiht_tile_paste_f32(spiht_ctx *ctx, const float *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W, int64_t th,
                         int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0, int64_t wh,
                         int64_t ww, float *d_out);
int spiht_tile_paste_f64(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                         int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                         int64_t wh, int64_t ww, double *d_out);
int spiht_tile_pack(spiht_ctx *ctx, const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_nbits, int64_t T,
                    uint8_t *d_packed, uint64_t packed_cap, uint32_t *d_lens);
int spiht_tile_unpack(spiht_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint32_t *d_lens, int64_t T,
                      uint8_t *d_slots, uint64_t slot_stride, uint64_t *d_nbytes);

/* ---------------------------------------------------------------------------------------
 * Tiled pictures at reduced resolution: the tiles decoded by spiht_decode_image_reduced_batch_* at 1/2^reduce size, assembled
 * into the picture at 1/2^reduce size.  reduce = k is allowed when 0 <= k <= L (the tile codec's levels) and 2^k divides th
 * and tw, so that the seams between tiles fall on whole reduced samples.  With thk = th >> k, twk = tw >> k,
 * Hk = ceil(H / 2^k), Wk = ceil(W / 2^k), sample (Y, X) of the reduced picture [c, Hk, Wk] is sample
 * (off_y + Y - i thk, off_x + X - j twk) of the reduced decode of tile (i, j) = (Y / thk, X / twk): that decode's centred
 * window (spiht_reduced_shape of a th x tw picture; in_h x in_w = thk x twk).  Additions only: the ABI version stays at 2.
 *   spiht_tile_reduced_grid  the geometry, pure arithmetic, no device: level_used = L; thk, twk, Hk, Wk; gy, gx (the grid of
 *                      the full picture, which is the reduced one's); rec_h x rec_w, the float64 reduced tile, pic_h x pic_w,
 *                      the 8- / 16-bit one; off_y, off_x, the origin of the tile's own samples in either.  level: -1 for the
 *                      default of a th x tw picture.  Every output pointer may be NULL.  SPIHT_ERR_ARG for what
 *                      spiht_tile_grid or spiht_reduced_shape refuse and for a tile side that 2^reduce does not divide.
 *   spiht_tile_mosaic_*  spiht_tile_paste_* with a source origin, for tiles of any side >= 1.  d_tiles: dense
 *                      [(i1-i0) * (j1-j0), c, rh, rw], the tiles of the sub-grid in row-major order; tile (i, j) gives its
 *                      samples [oy, oy + th) x [ox, ox + tw): oy, ox >= 0, rh >= oy + th, rw >= ox + tw.  H, W, th, tw are
 *                      the sizes of the picture and the tile BEING ASSEMBLED (the reduced ones: Hk, Wk, thk, twk), th, tw >= 1.
 *                      The rules for the window (y0, x0, wh, ww), the sub-grid and the output view (out_strides) are
 *                      spiht_tile_paste_*'s; asynchronous on the context's stream; argument errors are returned before anything
 *                      is queued; no byte outside the stated output is written.  With oy = ox = 0 and th, tw >= 8 the output
 *                      is spiht_tile_paste_*'s. */
int spiht_tile_reduced_grid(int64_t H, int64_t W, int64_t th, int64_t tw, int wavelet, int mode, int level, int reduce,
                            int *level_used, int64_t *thk, int64_t *twk, int64_t *Hk, int64_t *Wk, int64_t *gy, int64_t *gx,
                            int64_t *rec_h, int64_t *rec_w, int64_t *pic_h, int64_t *pic_w, int64_t *off_y, int64_t *off_x);
int spiht_tile_mosaic_u8(spiht_ctx *ctx, const uint8_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy, int64_t ox,
                         int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                         int64_t x0, int64_t wh, int64_t ww, uint8_t *d_out, const int64_t *out_strides);
int spiht_tile_mosaic_u16(spiht_ctx *ctx, const uint16_t *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy, int64_t ox,
                          int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                          int64_t x0, int64_t wh, int64_t ww, uint16_t *d_out, const int64_t *out_strides);
int spiht_tile_mosaic_f64(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy, int64_t ox,
                          int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                          int64_t x0, int64_t wh, int64_t ww, double *d_out);

/* ---------------------------------------------------------------------------------------
 * Rate allocation across the tiles of a picture (csrc/alloc.hip; the rule is spiht_amd/alloc.py).  The tiles are coded past
 * their share of the budget; K prefixes of every tile's stream are decoded and measured; every tile is cut where one more
 * byte buys the same drop in distortion, and spiht_tile_pack takes the cut lengths.  Additions only: the ABI version stays
 * at 2.  All pointers are DEVICE pointers; asynchronous on the context's stream; argument errors are returned before anything
 * is queued; no byte outside the stated outputs is written.  1 <= K <= 255, N * T < 2^31, strides multiples of 4 below 2^29.
 *   spiht_tile_prefix_slots  the NT slots a batched encode left (slot_stride, d_nbits) -> G * NT slots of out_stride bytes for
 *                      the candidates k0 .. k0 + G - 1 (k0 + G <= K + 1): slot (k - k0) * NT + t holds the first
 *                      R_t[k] = ceil(n_t k / K) bytes of slot t, n_t = ceil(nbits[t] / 8), and zeros behind them;
 *                      d_nbytes uint64 [G * NT]: those lengths.  d_max_n [NT] -> d_max_n_out [G * NT], the start planes
 *                      repeated for the batched decode (both NULL: not wanted).  d_slots and d_out 4-byte aligned.
 *   spiht_sse_tiles_*  d_tiles [N * T, c, th, tw], the cut tiles (spiht_tile_cut_*); d_dec [G, N * T, c, rh, rw] of the same
 *                      element type, rh >= th, rw >= tw -> d_out [G][N * T]: the sum over all channels of the squared error
 *                      over the tile's VALID extent, its first min(th, H - i th) rows and min(tw, W - j tw) columns; rows and
 *                      columns past it are never read.  _f64: double; every term (p - d) * (p - d) rounded, then added, in an
 *                      order fixed by (c, th, tw) and the extent alone: the same bits for any G and grouping.  _u8 / _u16:
 *                      uint64, exact (c th tw < 2^32).  1 <= G <= 65535, c <= 65535, th tw < 2^30, G * N * T < 2^31.
 *   spiht_tile_allocate  d_nbits [N * T] (the full streams), d_D [K + 1][N * T] (kind 0: float64, 1: uint64, converted with one
 *                      rounding), budget_bytes for each picture -> d_nbits_out uint64 [N * T] = 8 * the bytes alloc.allocate
 *                      gives, d_lambda double [N] (may be NULL) = its lambda*.  One workgroup per picture; the hulls live in
 *                      a grow-only buffer of the context. */
int spiht_tile_prefix_slots(spiht_ctx *ctx, const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_nbits, int64_t NT,
                            int64_t K, int64_t k0, int64_t G, uint8_t *d_out, uint64_t out_stride, uint64_t *d_nbytes,
                            const uint8_t *d_max_n, uint8_t *d_max_n_out);
int spiht_sse_tiles_f64(spiht_ctx *ctx, const double *d_tiles, const double *d_dec, int64_t G, int64_t N, int64_t c, int64_t H,
                        int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, double *d_out);
int spiht_sse_tiles_u8(spiht_ctx *ctx, const uint8_t *d_tiles, const uint8_t *d_dec, int64_t G, int64_t N, int64_t c, int64_t H,
                       int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, uint64_t *d_out);
int spiht_sse_tiles_u16(spiht_ctx *ctx, const uint16_t *d_tiles, const uint16_t *d_dec, int64_t G, int64_t N, int64_t c, int64_t H,
                        int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, uint64_t *d_out);
int spiht_tile_allocate(spiht_ctx *ctx, const uint64_t *d_nbits, const void *d_D, int kind, int64_t K, int64_t N, int64_t T,
                        uint64_t budget_bytes, uint64_t *d_nbits_out, double *d_lambda);

/* ---------------------------------------------------------------------------------------
 * A target quality across tiles (csrc/alloc.hip: k_tile_allocate_target; the rule is alloc.allocate_target).  Addition only:
 * the ABI version stays at 2.
 *   spiht_tile_allocate_target  the arguments, checks and limits of spiht_tile_allocate, and d_target double [N]: per picture
 *                      the squared error of the whole picture to reach (NULL: SPIHT_ERR_ARG, before anything is queued).
 *                      -> d_nbits_out uint64 [N * T] = 8 * the bytes alloc.allocate_target gives: every tile at the hull vertex
 *                      of the steepest common slope at which the total error (a float64 sum in the fixed order of
 *                      alloc.total_distortion) is at or below the target, if those bytes fit budget_bytes; else the cut of
 *                      spiht_tile_allocate at budget_bytes.  d_lambda double [N]: that slope, or lambda* of the budget;
 *                      d_dist double [N]: the total error reached, NaN in the budget branch; d_met uint32 [N]: 1 if the target
 *                      was reached within the budget, else 0.  The three may be NULL.  One launch, one workgroup per picture. */
int spiht_tile_allocate_target(spiht_ctx *ctx, const uint64_t *d_nbits, const void *d_D, int kind, int64_t K, int64_t N, int64_t T,
                               uint64_t budget_bytes, const double *d_target /* [N] squared errors */, uint64_t *d_nbits_out,
                               double *d_lambda, double *d_dist, uint32_t *d_met);

/* ---------------------------------------------------------------------------------------
 * Region of interest (csrc/roi.hip; the rule is spiht_amd/alloc.py).  A weight map steers the allocation above: the table
 * spiht_tile_allocate cuts by holds the squared error WEIGHTED per pixel position.  Additions only: the ABI version stays at 2.
 *   spiht_sse_tiles_w_*  the arguments, checks and limits of spiht_sse_tiles_*, then d_w uint8 [N or 1][H][W], the weights in
 *                      PICTURE coordinates, the same for every channel and candidate, at any byte address; w_stride: bytes
 *                      from one picture's map to the next, 0 = one map for all N pictures, else >= H * W.  -> d_out [G][N * T]:
 *                      the sum over the channels and the tile's valid extent of w[i th + y][j tw + x] * (p - d)^2, tile (i, j).
 *                      No byte outside the map is read: nothing past a tile's valid extent, nothing for the padding of edge tiles.
 *                      _f64: double; every term double(w) * ((p - d) * (p - d)), the subtraction, the square and the product
 *                      rounded once each, added in the order of spiht_sse_tiles_f64 -- a map of ones gives its bits, and the
 *                      bits do not depend on G or the grouping.  _u8 / _u16: uint64, exact; c * th * tw <= 2^24
 *                      (255 * 65535^2 * 2^24 < 2^64), else SPIHT_ERR_ARG.  d_w NULL or 0 < w_stride < H * W: SPIHT_ERR_ARG.
 *                      Asynchronous on the context's stream; argument errors are returned before anything is queued. */
int spiht_sse_tiles_w_f64(spiht_ctx *ctx, const double *d_tiles, const double *d_dec, int64_t G, int64_t N, int64_t c, int64_t H,
                          int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, double *d_out, const uint8_t *d_w,
                          uint64_t w_stride);
int spiht_sse_tiles_w_u8(spiht_ctx *ctx, const uint8_t *d_tiles, const uint8_t *d_dec, int64_t G, int64_t N, int64_t c, int64_t H,
                         int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, uint64_t *d_out, const uint8_t *d_w,
                         uint64_t w_stride);
int spiht_sse_tiles_w_u16(spiht_ctx *ctx, const uint16_t *d_tiles, const uint16_t *d_dec, int64_t G, int64_t N, int64_t c, int64_t H,
                          int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, uint64_t *d_out, const uint8_t *d_w,
                          uint64_t w_stride);

/* ---------------------------------------------------------------------------------------
 * Quality layers of a tiled picture (csrc/layers.hip; the rule is spiht_amd/alloc.py, allocate_layers).  The allocation is
 * run at Q growing budgets on one table of distortions; the lengths nest, and the run stores for every tile the bytes between
 * consecutive allocations, layer-major: layer q is, for t = 0 .. T-1, bytes [B(q-1, t), B(q, t)) of tile t's stream, B(-1) = 0.
 * The run through layer q is the whole picture at budget q.  Additions only: the ABI version stays at 2.  All pointers are
 * DEVICE pointers; asynchronous on the context's stream; argument errors are returned before anything is queued; no byte
 * outside the stated outputs is written.  1 <= Q <= 255, N * Q * T < 2^31, slot_stride a multiple of 4, at most 2^29.
 *   spiht_layer_pack   the N * T slots a batched encode left + d_cum_bits uint64 [Q][N * T], row q what the q-th
 *                      spiht_tile_allocate wrote (bits) -> d_cum uint32 [N][Q][T]: B(q, t) = max over q' <= q of
 *                      min(ceil(bits / 8), slot_stride) -- total: a table that does not nest still gives a valid run;
 *                      d_packed: picture n's run behind picture n - 1's, inside a picture layer-major, then tile;
 *                      d_pic_bytes uint64 [N]: the runs' lengths.  Nothing is written at or past d_packed + packed_cap
 *                      (N * T * slot_stride always suffices).  The pieces' offsets live in a grow-only buffer of the context.
 *   spiht_layer_unpack d_layers (layers_bytes long): one picture's run or a prefix of it; d_cum uint32 [Q][T] its table ->
 *                      S slots of slot_stride bytes: slot s receives tile d_sel[s] (an entry outside [0, T) is clamped), or
 *                      tile s when d_sel is NULL (then S <= T): its pieces of the layers 0 .. upto - 1 one behind the other,
 *                      then zeros up to slot_stride; d_nbytes uint64 [S] = min(cum[upto-1][t], slot_stride).  1 <= upto <= Q.
 *                      Bytes the table claims past layers_bytes read as zero; a table that falls in q is taken as its running
 *                      maximum. */
int spiht_layer_pack(spiht_ctx *ctx, const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_cum_bits, int64_t Q, int64_t N,
                     int64_t T, uint8_t *d_packed, uint64_t packed_cap, uint32_t *d_cum, uint64_t *d_pic_bytes);
int spiht_layer_unpack(spiht_ctx *ctx, const uint8_t *d_layers, uint64_t layers_bytes, const uint32_t *d_cum, int64_t Q, int64_t T,
                       int64_t upto, const int32_t *d_sel, int64_t S, uint8_t *d_slots, uint64_t slot_stride, uint64_t *d_nbytes);

/* ---------------------------------------------------------------------------------------
 * Overlapping tiles, cross-faded at the seams (csrc/overlap.hip; the rule is spiht_amd/overlap.py).  Every tile is coded with a
 * margin of m samples of its neighbours (0 <= m, 2 m <= min(th, tw)), and the decoder blends the decoded tiles over the 2m
 * samples around each seam.  Additions only: the ABI version stays at 2.  All pointers are DEVICE pointers; asynchronous on the
 * context's stream; argument errors are returned before anything is queued; no byte outside the stated outputs is written.
 *   spiht_tile_cut_overlap_*  the arguments, checks and limits of spiht_tile_cut_*, and m -> d_tiles: dense
 *                      [N * T, c, th + 2m, tw + 2m]; coded tile (i, j)'s sample (y, x) is the picture's at row
 *                      clamp(i th - m + y, 0, H - 1), column clamp(j tw - m + x, 0, W - 1) (np.pad(mode="edge") on all four
 *                      sides).  m = 0 gives the bytes of spiht_tile_cut_*.  m < 0 or 2 m > min(th, tw): SPIHT_ERR_ARG.
 *   spiht_tile_blend_*  d_tiles: float64, dense [(i1-i0) * (j1-j0), c, rh, rw], the decodes of the coded tiles of the sub-grid
 *                      in row-major order, rh >= th + 2m, rw >= tw + 2m (tile (i, j)'s own samples at (m, m)) -> the window
 *                      [c, wh, ww] at (y0, x0) of the H x W picture: _f64 dense float64; _u8 / _u16 by out_strides (bytes
 *                      (sc, sh, sw); NULL = dense CHW; what lies between a view's samples is not written).  Along an axis
 *                      (core t, g tiles) position P lies in the zone of the seam s = k t, 1 <= k < g, when s - m <= P < s + m;
 *                      there u = P - (s - m), tile k weighs a = 2u + 1 and tile k - 1 b = 4m - a, and tile k's sample index of
 *                      P is P - k t + m; elsewhere tile P / t has the whole weight.  In float64, every operation rounded once
 *                      (no fma), the division IEEE's: columns first, r = (bx L + ax R) / (4m) in a column zone, else the one
 *                      tile's sample; then rows, out = (by r_top + ay r_bottom) / (4m) in a row zone, else r.  _u8 / _u16:
 *                      out through the decoders' conversion (clip to [0, 1], times 255 / 65535, truncated, NaN -> 0).
 *                      SPIHT_ERR_ARG: m < 0 or 2 m > min(th, tw), a window that is empty or leaves the picture, a sub-grid
 *                      that is not inside the grid or misses a tile with weight in the window, rh / rw too small. */
int spiht_tile_cut_overlap_u8(spiht_ctx *ctx, const uint8_t *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                              int64_t W, int64_t th, int64_t tw, int64_t m, uint8_t *d_tiles);
int spiht_tile_cut_overlap_u16(spiht_ctx *ctx, const uint16_t *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                               int64_t W, int64_t th, int64_t tw, int64_t m, uint16_t *d_tiles);
int spiht_tile_cut_overlap_f32(spiht_ctx *ctx, const float *d_img, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th,
                               int64_t tw, int64_t m, float *d_tiles);
int spiht_tile_cut_overlap_f64(spiht_ctx *ctx, const double *d_img, int64_t N, int64_t c, int64_t H, int64_t W, int64_t th,
                               int64_t tw, int64_t m, double *d_tiles);
int spiht_tile_blend_u8(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W, int64_t th,
                        int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0, int64_t wh,
                        int64_t ww, uint8_t *d_out, const int64_t *out_strides);
int spiht_tile_blend_u16(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W, int64_t th,
                         int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0, int64_t wh,
                         int64_t ww, uint16_t *d_out, const int64_t *out_strides);
int spiht_tile_blend_f64(spiht_ctx *ctx, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W, int64_t th,
                         int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0, int64_t wh,
                         int64_t ww, double *d_out);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, every rank codes its own images (the reference's encode / decode
 * are pure functions of one image, src/lib.rs:24-42 -- nothing is exchanged while coding); the ONE exchange of the
 * path is the gather of the finished streams.  It runs on RCCL (ncclAllGather over xGMI), inside this library, on
 * the context's stream; librccl is loaded on first use.
 * ------------------------------------------------------------------------------------- */
typedef struct spiht_comm spiht_comm;
#define SPIHT_COMM_ID_BYTES 128
/* Rank 0 makes the job's id (ncclGetUniqueId) and hands its 128 bytes to every rank by any host channel
 * (spiht_amd/dist.py: a TCP exchange on MASTER_ADDR). */
int spiht_comm_unique_id(uint8_t *id128);
/* Collective over all ranks: joins the communicator of `world` ranks as `rank`, on the context's GPU. */
int spiht_comm_create(spiht_ctx *ctx, const uint8_t *id128, int world, int rank, spiht_comm **out);
void spiht_comm_destroy(spiht_comm *comm);
int spiht_comm_info(spiht_comm *comm, int *world, int *rank, int *rccl_version);
/* All-gather of B stream slots (slot_stride bytes each), bit counts and start planes per rank: rank r's rows land in
 * rows [r*B, (r+1)*B) of d_all_* (sizes world*B) on every rank.  Device pointers; queued on the context's stream
 * after the encoder kernels queued before it -- the host does not block (spiht_ctx_synchronize to wait). */
int spiht_gather_streams(spiht_ctx *ctx, spiht_comm *comm, const uint8_t *d_slots, const uint64_t *d_nbits,
                         const uint8_t *d_max_n, int64_t B, uint64_t slot_stride, uint8_t *d_all_slots,
                         uint64_t *d_all_nbits, uint8_t *d_all_max_n);
/* The RCCL shared library this process uses: the soname that was loaded, or every candidate tried with the loader's
 * reason when none could be ("" before the first spiht_comm_* call).  For the job's log line. */
const char *spiht_rccl_library(void);
/* spiht_pipeline_submit with the gather of a multi-GPU job in it (see the pipeline section below) */
typedef struct spiht_pipeline spiht_pipeline;
int spiht_pipeline_submit_gather(spiht_pipeline *p, const double *d_img, uint8_t *d_out, uint64_t *d_nbits, uint8_t *d_max_n,
                                 double *d_img_out, spiht_comm *comm, uint8_t *d_all_slots, uint64_t *d_all_nbits,
                                 uint8_t *d_all_max_n, int rank);
/* Where rank r's rows start in the gathered arrays, in bytes from each array's start (rank-major: rows [r*B, (r+1)*B)).
 * Pure arithmetic, no device: callable anywhere. */
int spiht_gather_row_offsets(int rank, int world, int64_t B, uint64_t slot_stride, uint64_t *off_slots, uint64_t *off_nbits,
                             uint64_t *off_max_n);
/* Host-side job control over the same communicator (both block): every rank has arrived and its context's queue is
 * empty; *value becomes the maximum over ranks. */
int spiht_comm_barrier(spiht_ctx *ctx, spiht_comm *comm);
int spiht_comm_allreduce_max_f64(spiht_ctx *ctx, spiht_comm *comm, double *value);

/* ---------------------------------------------------------------------------------------
 * The pipelined round trip (csrc/pipeline.cpp): B images per step, pixels -> streams -> pixels, consecutive steps
 * software-pipelined over three contexts the pipeline owns -- the HBM-bound passes of steps i+1 / i-1 on one, the list
 * coder of step i on another -- ordered with events; no call blocks the host except _synchronize.  This is the schedule
 * the throughput metric is measured on (bench.py); it replaces a caller's loop over the reference's one-image calls
 * (spiht_wrapper.py:142-216).  All image / stream pointers are DEVICE pointers as in the batched calls above and must stay
 * valid until the step that uses them has completed (d_out / d_nbits / d_max_n may be the same for every step: a step's
 * decoder has read them before the next step's encoder writes them).
 *   create        geometry and settings as spiht_encode_image_batch_f64; max_bits 0 = unlimited
 *   info          stream slot size in bytes (spiht_encode_bound) and the decoded picture size
 *   set_color3    colour model of the coded picture (as spiht_ctx_set_color3) for every step; kept by the pipeline
 *   submit        queue one step; the decoded pictures of step i are complete after submit of step i+1 has been followed
 *                 by _synchronize -- or after _flush + waiting
 *   submit_gather the same in a multi-GPU job: the streams are all-gathered (spiht_gather_streams) between encoder and
 *                 decoder on the list-coding stream, and the decoder reads rows [rank*B, (rank+1)*B) of the gathered buffers
 *   flush         queue the inverse transform of the last submitted step
 *   synchronize   flush, then wait for everything; returns the first latched device error
 *   contexts      the three contexts (stage timing: spiht_ctx_set_timing / _get_timing) */
typedef struct spiht_pipeline spiht_pipeline;
int spiht_pipeline_create(int device, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level,
                          double q_scale, const double *channel_mults, uint64_t max_bits, spiht_pipeline **out);
/* ... the HBM-bound passes on the caller's context h_ctx (on `device`; not destroyed with the pipeline): a process has few
 * hardware queues for its HIP streams, a caller that holds a context already should not add a fourth stream.  Nothing of
 * the pipeline's stays on h_ctx between calls: while submit / flush queue work they hold its mutex and have the pipeline's
 * colour model and options on it, and put back what the caller had set.  A call that fails half-way leaves the pipeline
 * unusable: every later call returns that first error (destroy it). */
int spiht_pipeline_create_on(spiht_ctx *h_ctx, int device, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                             int level, double q_scale, const double *channel_mults, uint64_t max_bits, spiht_pipeline **out);
void spiht_pipeline_destroy(spiht_pipeline *p);
int spiht_pipeline_info(spiht_pipeline *p, uint64_t *slot_stride, int64_t *rec_H, int64_t *rec_W);
int spiht_pipeline_set_color3(spiht_pipeline *p, const double *A_f, const double *M_f, double p_f, const double *A_i,
                              const double *M_i, double p_i);
int spiht_pipeline_submit(spiht_pipeline *p, const double *d_img, uint8_t *d_out, uint64_t *d_nbits, uint8_t *d_max_n,
                          double *d_img_out);
/* ... with 8-bit or 16-bit pictures in and out (the *_u8 / *_u16 batch calls: strides[4] in bytes, NULL = dense CHW; the
 * output cropped to H x W).  Every step keeps its own output form: float64, 8-bit and 16-bit steps may alternate on one pipeline. */
int spiht_pipeline_submit_u8(spiht_pipeline *p, const uint8_t *d_img, const int64_t *in_strides, uint8_t *d_out,
                             uint64_t *d_nbits, uint8_t *d_max_n, uint8_t *d_img_out, const int64_t *out_strides);
int spiht_pipeline_submit_u16(spiht_pipeline *p, const uint16_t *d_img, const int64_t *in_strides, uint8_t *d_out,
                              uint64_t *d_nbits, uint8_t *d_max_n, uint16_t *d_img_out, const int64_t *out_strides);
int spiht_pipeline_flush(spiht_pipeline *p);
int spiht_pipeline_synchronize(spiht_pipeline *p);
int spiht_pipeline_contexts(spiht_pipeline *p, spiht_ctx **h, spiht_ctx **l0, spiht_ctx **l1);

/* Thin device-memory helpers so a host language without a HIP binding can drive the batched API. */
/* Page-locked host memory for the arrays the host-array calls RETURN (decode_image gives back a new array,
 * spiht_wrapper.py:192-216): a device -> host copy into it is one DMA at the link's speed, into fresh pageable memory
 * several times slower (page faults + staging).  Pooled inside the library (pinning is what costs); at most 4 GiB are
 * handed out -- beyond that, or when the system refuses, SPIHT_ERR_NOMEM and the caller takes ordinary memory: every
 * host-array call accepts any host pointer.  Not tied to a context or device. */
int spiht_host_alloc(uint64_t bytes, void **h_ptr);
int spiht_host_free(void *h_ptr);
int spiht_dev_alloc(spiht_ctx *ctx, uint64_t bytes, void **d_ptr);
int spiht_dev_free(spiht_ctx *ctx, void *d_ptr);
int spiht_dev_upload(spiht_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int spiht_dev_download(spiht_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);
int spiht_dev_memset(spiht_ctx *ctx, void *d_dst, int value, uint64_t bytes);
int spiht_dev_copy(spiht_ctx *ctx, void *d_dst, const void *d_src, uint64_t bytes); /* device to device, asynchronous */

/* ---------------------------------------------------------------------------------------
 * Float pixels out (*_flt): a decode into float32, float16 or bfloat16 pictures.
 *
 *   kind   1 float32, 2 float16, 3 bfloat16 (anything else: SPIHT_ERR_ARG)
 *
 * Each call is its *_u16 sibling with a leading `kind` behind the context (in front of everything, where there is none) and
 * a void picture pointer: the same view by BYTE strides (non-negative multiples of the element size, 4 or 2; the base
 * aligned to the element; a view that is written does not overlap itself; NULL: dense CHW), the same crop to the picture's
 * own [c, H, W] (the reduced forms: to [c, hs[reduce], ws[reduce]]), the same statuses, asynchrony and chunking; refusals
 * happen before any launch.  What is stored differs: sample v of the float64 picture the *_f64 sibling makes, rounded ONCE
 * to the kind, to nearest, ties to even -- no clip, no scale; overflow gives +-inf, subnormals of the kind are kept, the sign
 * of zero is kept, NaN gives a NaN.  (Once: float64 -> float32 -> float16 rounds twice and differs on a few dozen samples of
 * a small bior2.2 picture, whose decoded samples lie a hair off the ties of the narrow kinds.)  The rule in integer
 * arithmetic: spiht_amd/floatpx.py on the host, csrc/floatpx.h on the device.  A stream does not record the pixel format it
 * was coded from: streams of float64, float32, 8-bit and 16-bit pictures all decode into the float kinds.
 * Level 1 of the tiled inverse transform stores the kind itself (one pixel kind of the kernels, PX_FLT, for the three); the
 * routes without a fused form -- periodization, filters longer than SPIHT_MAX_TAPS -- convert in a pass of their own over
 * the float64 result, which is what spiht_convert_batch_flt runs alone:
 *   spiht_convert_batch_flt  d_in: dense float64 [B, c, rec_h, rec_w] on the device -> the view [B, c, H, W] of the kind at
 *                            d_out (H <= rec_h, W <= rec_w: the crop).  Asynchronous.
 * Tiles: a tile batch of a 16-bit kind is pasted and assembled by the *_u16 copies, one of float32 by spiht_tile_paste_f32
 * and spiht_tile_mosaic_f32 (dense), or by the strided copies below; overlapping tiles are decoded as float64, blended in
 * float64 and rounded at the store (spiht_tile_blend_flt: spiht_tile_blend_u16's arguments). */
int spiht_check_view_flt(int kind, int64_t B, int64_t c, int64_t H, int64_t W, const int64_t *strides, int output);
int spiht_convert_batch_flt(spiht_ctx *ctx, int kind, const double *d_in, int64_t B, int64_t c, int64_t rec_h, int64_t rec_w,
                            int64_t H, int64_t W, void *d_out, const int64_t *out_strides);
int spiht_decode_image_batch_flt(spiht_ctx *ctx, int kind, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                                 const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H, int64_t W, int wavelet, int mode,
                                 int level, double q_scale, const double *channel_mults, void *d_img_out,
                                 const int64_t *out_strides, int32_t *d_rec);
int spiht_decode_image_host_flt(spiht_ctx *ctx, int kind, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t H,
                                int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                void *img_out, const int64_t *strides);
int spiht_dequant_idwt_flags_batch_flt(spiht_ctx *ctx, int kind, const int32_t *d_rec, const uint32_t *d_flags, int64_t B,
                                       int64_t c, int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                       const double *channel_mults, void *d_img_out, const int64_t *out_strides);
int spiht_dequant_idwt_reduced_batch_flt(spiht_ctx *ctx, int kind, const int32_t *d_rec, int64_t B, int64_t c, int64_t H,
                                         int64_t W, int wavelet, int mode, int level, double q_scale,
                                         const double *channel_mults, void *d_img_out, const int64_t *out_strides, int reduce);
int spiht_decode_image_reduced_batch_flt(spiht_ctx *ctx, int kind, const uint8_t *d_data, uint64_t slot_stride,
                                         const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c, int64_t H,
                                         int64_t W, int wavelet, int mode, int level, double q_scale,
                                         const double *channel_mults, void *d_img_out, const int64_t *out_strides,
                                         int32_t *d_rec, int reduce);
int spiht_decode_image_reduced_host_flt(spiht_ctx *ctx, int kind, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                        int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                        const double *channel_mults, void *img_out, const int64_t *strides, int reduce);
/* float32 tile batches by strides (spiht_tile_paste_u16 / spiht_tile_mosaic_u16 with 4-byte elements: out_strides[3] in bytes,
 * multiples of 4; NULL: dense CHW) */
int spiht_tile_paste_f32s(spiht_ctx *ctx, const float *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                          int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0, int64_t x0,
                          int64_t wh, int64_t ww, float *d_out, const int64_t *out_strides);
int spiht_tile_mosaic_f32(spiht_ctx *ctx, const float *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t oy, int64_t ox,
                          int64_t H, int64_t W, int64_t th, int64_t tw, int64_t i0, int64_t i1, int64_t j0, int64_t j1,
                          int64_t y0, int64_t x0, int64_t wh, int64_t ww, float *d_out, const int64_t *out_strides);
int spiht_tile_blend_flt(spiht_ctx *ctx, int kind, const double *d_tiles, int64_t c, int64_t rh, int64_t rw, int64_t H, int64_t W,
                         int64_t th, int64_t tw, int64_t m, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int64_t y0,
                         int64_t x0, int64_t wh, int64_t ww, void *d_out, const int64_t *out_strides);

/* ---------------------------------------------------------------------------------------
 * Float pixels in (*_flt, the encode side): float32, float16 or bfloat16 pictures coded as they lie, by the float64 codec.
 *
 * Each call is its *_u16 sibling with `kind` (as above) behind the context and a void picture pointer: the same view by BYTE
 * strides (non-negative multiples of the element size, 4 or 2; the base aligned to the element; NULL: dense CHW), the same
 * statuses, asynchrony and chunking at 65535 planes; refusals (spiht_check_view_flt(kind, .., 0), an unaligned base, an
 * unknown kind) happen before any launch.  Every sample is WIDENED EXACTLY to float64 on the loads of forward level 1 --
 * float32 by the hardware's conversion, float16 as half -> float -> double, bfloat16 as the upper half of a float32; nothing
 * is scaled and nothing is clipped, subnormals of every kind keep their value -- and everything behind the loads is the
 * float64 path.  So every call returns, field by field and bit for bit, what its *_f64 sibling returns for the widened
 * picture (spiht_amd/floatpx.py: to_float64; csrc/floatpx.h: flt_load_value), with every feature of the float64 codec: the
 * colour model, every mode and wavelet, tiles, allocation, region of interest, target PSNR, layers, overlap.
 * This is NOT spiht_encode_image_*_f32: a float32 picture given to the *_f32 calls keeps the reference's single-precision
 * transform (and its limits: dense CHW, no colour model); the same picture given to the *_flt calls is transformed in
 * float64.  The two streams differ as soon as the quantiser step is fine enough to see float32's rounding.
 * Non-finite samples are outside the contract of the encode calls, as they are for the *_f64 calls; the widening pass alone
 * is specified on them (infinities stay, a NaN gives a NaN).
 * Level 1 of the tiled forward transform loads the kind itself (one pixel kind of the kernels, PX_FLT, for the three; all loads
 * of a thread first, then the widenings); the routes without a fused form -- the modes that compute their extension,
 * periodization, filters longer than SPIHT_MAX_TAPS -- widen in a pass of their own in front, which is what
 * spiht_widen_batch_flt runs alone (the mirror of spiht_convert_batch_flt):
 *   spiht_widen_batch_flt    the view [B, c, H, W] of the kind at d_in (strides[4] in bytes; NULL: dense) -> dense float64
 *                            [B, c, H, W] at d_out on the device.  Asynchronous.
 * Error sums of the allocation: spiht_sse_tiles_flt / spiht_sse_tiles_w_flt are spiht_sse_tiles_f64 / _w_f64 with ORIGINAL
 * tiles of the kind (d_tiles aligned to the element), widened on the load; the decodes stay float64, the partition and the
 * order of additions are the same, so the sums are the bits of the _f64 calls on the widened tiles.
 * Tiles: a picture of a 16-bit kind is cut by the *_u16 copies, as bit patterns; one of float32 by the strided copies
 * spiht_tile_cut_f32s / spiht_tile_cut_overlap_f32s (spiht_tile_cut_u16 / spiht_tile_cut_overlap_u16 with 4-byte elements;
 * the dense *_f32 calls are unchanged). */
int spiht_widen_batch_flt(spiht_ctx *ctx, int kind, const void *d_in, const int64_t *strides, int64_t B, int64_t c, int64_t H,
                          int64_t W, double *d_out);
int spiht_encode_image_batch_flt(spiht_ctx *ctx, int kind, const void *d_img, const int64_t *strides, int64_t B, int64_t c,
                                 int64_t H, int64_t W, int wavelet, int mode, int level, double q_scale,
                                 const double *channel_mults, uint64_t max_bits, uint8_t *d_out, uint64_t slot_stride,
                                 uint64_t *d_nbits, uint8_t *d_max_n, int32_t *d_coeffs);
int spiht_encode_image_host_flt(spiht_ctx *ctx, int kind, const void *img, const int64_t *strides, int64_t c, int64_t H, int64_t W,
                                int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                uint64_t max_bits, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n);
int spiht_dwt_pyramid_batch_flt(spiht_ctx *ctx, int kind, const void *d_img, const int64_t *strides, int64_t B, int64_t c, int64_t H,
                                int64_t W, int wavelet, int mode, int level, double q_scale, const double *channel_mults,
                                int32_t *d_coeffs, uint8_t *d_dmsb, uint8_t *d_lmsb, uint32_t *d_maxabs);
int spiht_sse_tiles_flt(spiht_ctx *ctx, int kind, const void *d_tiles, const double *d_dec, int64_t G, int64_t N, int64_t c,
                        int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, double *d_out);
int spiht_sse_tiles_w_flt(spiht_ctx *ctx, int kind, const void *d_tiles, const double *d_dec, int64_t G, int64_t N, int64_t c,
                          int64_t H, int64_t W, int64_t th, int64_t tw, int64_t rh, int64_t rw, double *d_out, const uint8_t *d_w,
                          uint64_t w_stride);
int spiht_tile_cut_f32s(spiht_ctx *ctx, const float *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H, int64_t W,
                        int64_t th, int64_t tw, float *d_tiles);
int spiht_tile_cut_overlap_f32s(spiht_ctx *ctx, const float *d_img, const int64_t *strides, int64_t N, int64_t c, int64_t H,
                                int64_t W, int64_t th, int64_t tw, int64_t m, float *d_tiles);

/* How the tiled forward transform kernel addresses a level (host only, no device call): 1 when every plane the level reads or
 * writes -- its float64 input in_h x in_w (px_es == 0) or the byte span of an 8- / 16-bit or float view with element size px_es
 * (1, 2 or 4) and
 * byte strides px_sh, px_sw; the packed array enc_h x enc_w; the approximation out_h x out_w -- is under 2^30 bytes, so that the
 * kernel may use 32-bit offsets into per-plane buffer descriptors; 0: 64-bit addresses.  The results are the same bits. */
int spiht_dwt_addr32(int64_t in_h, int64_t in_w, int64_t out_h, int64_t out_w, int64_t enc_h, int64_t enc_w, int px_es,
                     int64_t px_sh, int64_t px_sw);

/* ---------------------------------------------------------------------------------------
 * Host-fed streams (csrc/hoststream.cpp): batches of HOST pictures encoded, or batches of HOST streams decoded, with the
 * transfers overlapped -- step i+1's upload, step i's coding and step i-1's download run at the same time.  The reference's
 * interface is host arrays in and out, one picture per call (spiht_wrapper.py:142-216); this is the schedule for a caller
 * with a folder of pictures or a loader with thousands of streams.  One-directional: a stream encodes or it decodes.
 * Additions only: the ABI version stays at 2.
 *
 * A stream lives on a caller's context, which must outlive it.  The first one gives the context two more HIP streams,
 * one for the copies in and one for the copies out; every later host-fed stream on the context shares them and the last
 * one destroyed takes them along, so a context carries three HIP streams in all however many encoders and decoders it
 * feeds (a process has four hardware queues, and two HIP streams on one queue run one after the other).  No graphs, no
 * threads, no new context; it is driven by the caller's thread.
 * It holds a ring of `depth` slots (2 .. 4), each with page-locked input staging and page-locked output staging from the pool behind spiht_host_alloc, its device buffers and its events.  The coding is the
 * batched entry point of the stream's element -- spiht_encode_image_batch_f64 / _u8 / _u16 / _flt or its decode sibling --
 * so every wavelet, mode, level, channel scale and the context's colour model (spiht_ctx_set_color3: the setting at the
 * moment of _submit) mean what they mean there, and the bits are those calls' bits.
 *
 *   elem      SPIHT_HS_F64, _U8, _U16, or a float kind of the *_flt calls: SPIHT_HS_FLT32, _FLT16, _BF16
 *   strides   the view [B, c, H, W] of the staged pictures in BYTES, as the batched calls take it (NULL: dense CHW); float64
 *             pictures are dense.  An encoder reads the view, a decoder writes it (the rules of spiht_check_view_*).
 *             A float64 decoder's pictures are dense [n, c, rec_H, rec_W], uncropped as spiht_decode_image_batch_f64 leaves
 *             them; every other element's are cropped to H x W as its batch call crops them.
 *   max_bits  encoder: the budget per picture (0 or SPIHT_MAX_BITS_UNLIMITED: none).  decoder: the longest stream it takes,
 *             in bits (0: the bound of the geometry).  Either way it sizes the staging: slot_bytes per picture
 *             (spiht_hstream_info).
 *
 * Encode step:
 *   _input(s, &h)    the next slot's page-locked picture buffer (B pictures by `strides`), to be filled by the caller -- a
 *                    decoder library can write straight into it.  Asked again before the submit: the same buffer.
 *   _submit(s, n, 0) 1 <= n <= B pictures of it.  Queues, without waiting for anything: the upload on the copy-in stream; on
 *                    the context's stream, behind an event, the batched encode, spiht_tile_pack of the n streams into one
 *                    run and the download of the n lengths and start planes; an event.
 *   _next(s, ms, &o) the OLDEST submitted step: waits for that event, queues the download of exactly the packed bytes on
 *                    the copy-out stream -- with no wait in front of it: it never stands behind a later step -- and waits
 *                    for it.
 *                    o.bytes: the n streams one behind the other, o.nbytes of them; o.lens[n]; o.max_n[n].
 * Decode step:
 *   _input(s, &h)    page-locked room for a step's input; spiht_hstream_decode_input gives its three parts: packed bytes
 *                    (B * slot_bytes), lens uint32 [B], max_n uint8 [B].  (*h is the packed bytes.)
 *   _submit(s, n, d) the n streams of lens[0 .. n), one behind the other.  Queues the upload of exactly those bytes,
 *                    spiht_tile_unpack into slots (of the longest stream's size, rounded up to 4), the batched decode, and
 *                    the download of the pictures.  d != NULL: a DEVICE destination for the pictures (the view by `strides`,
 *                    or dense) -- they stay in HBM and nothing is downloaded; d must stay valid until _next has returned
 *                    the step.  (An encoder takes d == NULL only.)
 *   _next(s, ms, &o) o.pictures: the n pictures in the slot's page-locked output (NULL with a device destination, which is
 *                    complete when _next returns), o.nbytes the bytes they span.
 * What _next hands out is valid until _input hands that slot out again -- after `depth` - 1 further steps at the earliest.
 *
 * No call waits without bound.  _input and _submit never block: with no free slot they return SPIHT_ERR_BUSY and change
 * nothing (_submit without an _input before it: SPIHT_ERR_BUSY when the ring is full, else SPIHT_ERR_ARG).  _next polls the
 * step's event for at most timeout_ms milliseconds (0: one look), then returns SPIHT_ERR_TIMEOUT and leaves the stream as it
 * was -- the same call made again goes on waiting; with nothing submitted it returns SPIHT_ERR_IDLE at once.  Results leave
 * in the order of submission.  A failed HIP call latches: every later call returns that first status (destroy the stream).
 * The device-side guards of the batched calls (SPIHT_ERR_MAGNITUDE ...) stay the context's: spiht_ctx_synchronize reports
 * them, as for every batched call.  The first step of a stream may wait while the context's scratch grows to the batch's
 * size; later steps do not.  _destroy waits for what is queued, at most SPIHT_HS_DESTROY_MS, then frees; when that time runs
 * out it gives its events back but leaves the buffers to the process (a transfer may still be writing them) and
 * returns SPIHT_ERR_TIMEOUT.  Calls on one stream come from one thread at a time.
 * Page-locked footprint: depth * (one batch of pictures + B * slot_bytes + 5 B) bytes; when the pool refuses (4 GiB handed
 * out, or the system says no) _create fails with SPIHT_ERR_NOMEM and nothing is left allocated. */
enum { SPIHT_ERR_BUSY = 11,    /* a host-fed stream's ring is full: take a result (spiht_hstream_next) first */
       SPIHT_ERR_TIMEOUT = 12, /* the step did not complete within the time given; the call may be made again */
       SPIHT_ERR_IDLE = 13 };  /* spiht_hstream_next with nothing submitted */
enum { SPIHT_HS_ENCODE = 0, SPIHT_HS_DECODE = 1 };
enum { SPIHT_HS_F64 = 0, SPIHT_HS_U8 = 1, SPIHT_HS_U16 = 2,
       SPIHT_HS_FLT32 = 3, SPIHT_HS_FLT16 = 4, SPIHT_HS_BF16 = 5 /* the float kinds 1, 2, 3 of the *_flt calls */ };
#define SPIHT_HS_DESTROY_MS 10000
typedef struct spiht_hstream spiht_hstream;
typedef struct spiht_hstream_result {
    int64_t n;              /* pictures of the step */
    uint64_t nbytes;        /* encoder: bytes at `bytes`; decoder: bytes the n pictures span at `pictures` */
    const uint8_t *bytes;   /* encoder: the n streams, one behind the other */
    const uint32_t *lens;   /* encoder: their n lengths in bytes */
    const uint8_t *max_n;   /* encoder: their n start planes */
    void *pictures;         /* decoder: the n pictures (NULL: they went to the device destination of the submit) */
    uint64_t step;          /* the step's number, from 0 in the order of submission */
} spiht_hstream_result;
int spiht_hstream_create(spiht_ctx *ctx, int direction, int elem, int64_t B, int depth, int64_t c, int64_t H, int64_t W,
                         int wavelet, int mode, int level, double q_scale, const double *channel_mults, uint64_t max_bits,
                         const int64_t *strides, spiht_hstream **out);
int spiht_hstream_destroy(spiht_hstream *s);
/* slot_bytes: the stream slot per picture; pic_bytes: bytes one step's B pictures span in the staging; rec_H x rec_W: the
 * size of a decoder's pictures (float64: spiht_geometry's; else H x W).  Output pointers may be NULL. */
int spiht_hstream_info(spiht_hstream *s, uint64_t *slot_bytes, uint64_t *pic_bytes, int64_t *rec_H, int64_t *rec_W);
int spiht_hstream_input(spiht_hstream *s, void **h_ptr);
int spiht_hstream_decode_input(spiht_hstream *s, uint8_t **h_packed, uint32_t **h_lens, uint8_t **h_max_n);
int spiht_hstream_submit(spiht_hstream *s, int64_t n, void *d_dst);
int spiht_hstream_next(spiht_hstream *s, int timeout_ms, spiht_hstream_result *out);
/* steps submitted and not yet taken (0 .. depth) */
int spiht_hstream_pending(spiht_hstream *s, int *steps);

/* ---------------------------------------------------------------------------------------
 * Picture sets (csrc/tileset.hip): pictures of DIFFERENT sizes as one dense tile batch, and one dense batch of decoded tiles
 * into many windows of many pictures -- the cut and the paste of the tiled pictures above, for a whole set in one launch.  All
 * tiles of a set have one shape th x tw, so the tiles of pictures of any sizes share one batch of the batched calls; the
 * grid of every picture, the order of its tiles and the edge replication are those of spiht_tile_grid and spiht_tile_cut_*.
 * One call per kernel, by the element's size es = 1, 2, 4 or 8 bytes and not by the pixel type: both are copies.
 * Additions only: the ABI version stays at 2.
 * The tables (pics, items) are HOST memory, one plain row per picture (item); every other pointer, those inside the rows
 * included, is a DEVICE pointer.  The tables are checked completely before anything is queued -- argument errors are returned
 * before anything is queued --, then copied to device memory of the library's own on the context's stream: the caller may free
 * or rewrite them as soon as the call returns, and calls queued back to back without a synchronisation each see their own.
 * The calls are asynchronous on the context's stream like the *_batch_* calls, and no byte outside the stated output is written.
 *   spiht_tile_cut_set    pics: P >= 1 rows.  Picture p is [c, H, W] at d_img by the byte strides (sc, sh, sw), under the rules
 *                         of spiht_check_view_* for a view that is read (non-negative multiples of es, the base aligned to es)
 *                         -> d_tiles: dense [NT, c, th, tw], NT the sum of the pictures' gy * gx; picture p's tiles lie at
 *                         rows [tile0_p, tile0_p + T_p), tile0_p the sum of the tile counts in front of it, in row-major
 *                         order.  H, W >= 1, th, tw >= 8 and the limits of spiht_tile_grid; NT < 2^31, c <= 65535.
 *   spiht_tile_paste_set  items: B >= 1 rows.  d_tiles: dense [S, c, rh, rw], rh >= th, rw >= tw; item b owns the tiles
 *                         [s0_b, s0_b + (i1-i0) * (j1-j0)), s0_b the sum of the sub-grid sizes in front of it: the sub-grid
 *                         [i0, i1) x [j0, j1) of its H x W picture in row-major order.  -> d_out of item b: the window
 *                         [c, wh, ww] of that picture whose first sample is picture sample (y0, x0), by the byte strides
 *                         (sc, sh, sw) under the rule for a view that is WRITTEN.  Every output sample comes from the one
 *                         tile that owns it; a tile that does not meet its item's window gives nothing; rows / columns >= th /
 *                         tw of a tile are never read.  Every window must lie in its picture and every sub-grid must hold the
 *                         tiles its window meets; S must be the sum of the sub-grid sizes (SPIHT_ERR_ARG); S < 2^31,
 *                         c <= 65535.  The views of two DIFFERENT items may overlap: which of the two is left is not said. */
typedef struct spiht_tileset_pic {
    const void *d_img;      /* device: the picture's first sample */
    int64_t sc, sh, sw;     /* bytes */
    int64_t H, W;
} spiht_tileset_pic;
typedef struct spiht_tileset_item {
    void *d_out;            /* device: the window's first sample */
    int64_t sc, sh, sw;     /* bytes */
    int64_t H, W;           /* the picture the window lies in */
    int64_t i0, i1, j0, j1; /* the sub-grid of its tiles in the batch */
    int64_t y0, x0, wh, ww; /* the window */
} spiht_tileset_item;
int spiht_tile_cut_set(spiht_ctx *ctx, int es, int64_t P, int64_t c, int64_t th, int64_t tw, const spiht_tileset_pic *pics,
                       void *d_tiles);
int spiht_tile_paste_set(spiht_ctx *ctx, int es, int64_t B, int64_t c, int64_t rh, int64_t rw, int64_t th, int64_t tw,
                         const spiht_tileset_item *items, const void *d_tiles, int64_t S);

/* ---------------------------------------------------------------------------------------
 * Resized crops (csrc/resample.hip): a box of any size of each of B pictures of a set, resampled to ONE size [c, oh, ow] straight
 * from the dense batch of the decoded float64 tiles -- the paste above with arithmetic: the antialiased triangle filter
 * ("bilinear, antialias"), a mirror left to right, (v - mean) / std per channel and ONE rounding to the output's element.  The
 * rule is spiht_amd/resample.py: resize_rule.  Additions only: the ABI version stays at 2.
 * The weights are the CALLER's (resample.py: axis_table, the mirror applied by reversing the rows of the column table): the
 * kernel computes none, it multiplies and adds in the rule's order -- columns first, then rows; acc = s[start] * w[0], then
 * acc = acc + s[start + k] * w[k], every product and sum rounded on its own -- normalises with IEEE's division and converts.
 *   elem         the output's element, SPIHT_HS_F64 .. SPIHT_HS_BF16: float64; 8 / 16 bits by the decoder's conversion (clip to
 *                [0, 1], times 255 / 65535, truncate); a float kind rounded once, to nearest even (the *_flt calls' rule)
 *   items        B >= 1 HOST rows as spiht_tile_paste_set takes them, read the same way: item b is the box (y0, x0, wh, ww) of
 *                its H x W picture, made from the sub-grid [i0, i1) x [j0, j1) of tiles; d_out and (sc, sh, sw) are the view
 *                of its OUTPUT [c, oh, ow], under the rule for a view that is written.  Samples outside the box never
 *                contribute, and what lies between a view's samples is not written.
 *   item_tables  HOST, int64 [B][4]: the byte offset in `tables` of item b's column table and its K, then of its row table and
 *                its K.  A table of an axis with n outputs (ow, oh) lies at a multiple of 8 bytes: int32 start[n], int32
 *                count[n], float64 weights[n][K]; output i is made from the box's samples start[i] .. start[i] + count[i] - 1
 *                of the axis.  Tables may be shared between items.
 *   tables       HOST, table_bytes bytes, 8-byte aligned
 *   mean, std    HOST, float64 [c] each, or both NULL; not with 8 / 16 bits; std != 0
 *   d_tiles      DEVICE, dense float64 [S, c, rh, rw], rh >= th, rw >= tw, S the sum of the sub-grid sizes, as for the paste
 * SPIHT_ERR_ARG, before anything is queued: what spiht_tile_paste_set refuses of an item; B, c, oh or ow < 1; an output
 * misaligned for its element or overlapping itself; a table that leaves `tables`, lies at no multiple of 8 or has K < 1 or
 * K > 33 (the taps of a box side of at most 16 output sides); a count < 1 or > K; a run of taps that leaves the box; a row table
 * whose 8 consecutive outputs (from a multiple of 8) span more than 145 box rows (what a workgroup holds: 16 * 7 + 33); mean
 * without std.  B, c <= 65535 (SPIHT_ERR_TOO_LARGE).  Rows, tables, mean and std are copied to device memory of the library's
 * own on the context's stream, as the tables of the calls above: they may be dropped when the call returns, and calls queued
 * back to back each see their own.  Asynchronous on the context's stream. */
/* HOST only, no device: the rule's table of one axis of n_in samples resampled to n_out (resample.py: axis_table; flip != 0: its
 * rows reversed, flip_table), written at `table` (8-byte aligned, cap bytes) in the layout above, bit for bit numpy's.  *K and
 * *bytes are set whenever the sizes are valid; table == NULL only asks for them; cap < *bytes: SPIHT_ERR_ARG, nothing written. */
int spiht_resample_axis_table(int64_t n_in, int64_t n_out, int flip, void *table, uint64_t cap, int64_t *K, uint64_t *bytes);
int spiht_tile_resample_set(spiht_ctx *ctx, int elem, int64_t B, int64_t c, int64_t rh, int64_t rw, int64_t th, int64_t tw,
                            int64_t oh, int64_t ow, const spiht_tileset_item *items, const int64_t *item_tables,
                            const void *tables, uint64_t table_bytes, const double *mean, const double *std,
                            const double *d_tiles, int64_t S);

#ifdef __cplusplus
}
#endif
#endif /* SPIHT_HIP_H */
