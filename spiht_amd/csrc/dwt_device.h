// 2-D separable DWT / inverse DWT for the SPIHT image path (gfx950), float64 (level 1 also from / into 8- and 16-bit pixels).
//
// Replaces the PyWavelets calls of the reference wrapper
//   encode: pywt.wavedec2 -> coeffs_to_array -> channel_mults*arr -> quantize   (spiht_wrapper.py:163-172)
//   decode: rec/channel_mults -> dequantize -> array_to_coeffs -> waverec2       (spiht_wrapper.py:259-276)
// One launch per decomposition level, both axes fused:
//   forward: a workgroup owns a TH x TW tile of output positions of all four sub-bands.  The axis -2
//            filter runs straight from global memory: thread = input column, and the whole column segment
//            the tile needs is loaded into registers FIRST (2*TH+F-2 independent 8-byte loads per lane in
//            flight, consecutive lanes -> consecutive addresses), then filtered; the low/high intermediates
//            go to LDS split by column parity so that the axis -1 filter reads them with unit stride.  LL
//            is written as float64 (input of the next level); the three detail bands are written already
//            quantised (int32, truncation toward zero) into their place in the zero-padded Mallat array --
//            coeffs_to_array and the two quantise passes of the wrapper cost no extra HBM traffic -- and
//            max|coefficient| (encoder_decoder.rs:165) is folded into the same pass.
//   inverse: band tiles are dequantised on load ((rec / m_k) / q as the wrapper does) into LDS; thread =
//            output column: axis -1 synthesis of one band row at a time feeds a register window of the
//            last F/2 rows, from which the axis -2 synthesis emits two output rows -- no LDS round trip for
//            the intermediate, stores are 512 B per wave.
// Arithmetic follows the published pywt definitions in the same summation order as oracle/dwt_oracle.c
// (ascending tap / band index, separate multiply and add: the three units are compiled with -ffp-contract=off),
// so GPU and oracle agree bit for bit and both agree with pywt to a few ulp.
// HBM-bound: per level, 8 B per input sample + 8 B (LL) + 3*4 B (details) per output position.
// This header: what the three units share.  dwt_fwd.hip holds the tiled forward kernels, dwt_inv.hip the tiled inverse ones (each
// takes minutes to compile: side by side), dwt_plain.hip the one-thread-per-sample passes (seconds).
#pragma once
#include "common.h"
#include "floatpx.h"
#include "list_coder.h"  // iabs_u
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#ifndef DW_TH
#define DW_TH 12      // output rows per tile.  Level 1 of 256 1080p images: 12 rows 3.8-3.95 ms, 16 rows 4.05-4.2, 14: 4.1,
#endif                // 10: 4.4, 20: 4.5, 24: 4.2 (25.9 KB of LDS per workgroup at 12 rows: six workgroups per CU)
#define DW32_TH 16    // ... of the single-precision kernel (12 rows: 3.9 instead of 2.85 ms)
#ifndef DW_TW
#define DW_TW 64      // output cols per tile
#endif
#define DW_BLOCK 256
#ifndef DWF_STRAY
#define DWF_STRAY 1    // k_dwt_level: the few input columns beyond the last full wavefront as (column, output row) items (dwt_tile)
#endif
#ifndef DWF_BLOCK
#define DWF_BLOCK 192  // threads of a forward-transform workgroup (k_dwt_level); 132 input columns: 128 threads hold one each, the
                       // other four are the third wavefront's items (DWF_STRAY).  Three
                       // wavefronts instead of four: beside a list-decoder workgroup (192 of a SIMD's 512 registers) FIVE of these
                       // workgroups fit a CU instead of four -- level 1 inside the pipelined step 6.3 instead of 6.55 ms, the step
                       // 16.4 instead of 16.7; alone 4.2 instead of 4.05 ms (round 4)
#endif

// Workgroups are dealt round-robin over the 8 XCDs (block b and b+8 share an L2).  Remap the linear block id so
// that each XCD walks one contiguous range of tiles: neighbouring tiles (shared halo columns/rows on the read
// side, shared partial cache lines on the write side) then meet in the same L2.  Speed only, never correctness.
__device__ __forceinline__ void xcd_tile_at(uint32_t L, uint32_t gx, uint32_t gy, uint32_t gz, uint32_t &bx, uint32_t &by,
                                            uint32_t &bz) {
    const uint32_t nt = gx * gy * gz;
    const uint32_t q = nt >> 3, r = nt & 7u, x = L & 7u, j = L >> 3;
    const uint32_t T = x * q + (x < r ? x : r) + j;
    bx = T % gx;
    const uint32_t t2 = T / gx;
    by = t2 % gy;
    bz = t2 / gy;
}

__device__ __forceinline__ void xcd_tile(uint32_t gx, uint32_t gy, uint32_t gz, uint32_t &bx, uint32_t &by, uint32_t &bz) {
    xcd_tile_at(blockIdx.x, gx, gy, gz, bx, by, bz);
}

// max |coefficient| of an image, raised by every tile of the image: an atomic on one word, and read-modify-writes of one
// memory line are served one after the other (11.5 ns each, measured: with one atomic per wavefront a 16-image launch
// of level 1 took 1.6 ms for its 141 000 atomics, six times what its bytes take, and 256 images were as much
// atomic-bound as HBM-bound).  So: one atomic per workgroup (the wavefronts meet in an LDS word first), and none when
// the word already holds as much (a cached look; measured against no look and a look the atomics' coherence point answers,
// DESIGN.md 6; a stale answer only costs a spare atomic).  `s_m` must have been zeroed before an earlier barrier.
// The cached look relies on this: the word is only ever RAISED between two zero-fills (hipMemsetAsync in front of every
// transform, api.cpp), and a zero-fill is a kernel / copy of its own on the same stream -- the caches that could hold the
// word (the CU's vector L1, and the per-XCD L2 for lines another XCD wrote) are invalidated at the kernel boundary in
// front of this launch, so a look can return an OLD value of this launch's epoch (lower: a spare atomic) but never one
// from before the zero-fill (higher: a lost maximum).  tests/test_gpu_dwt.py::test_maxabs_small_batch_after_large_batch
// runs exactly the case that would show it: large magnitudes, then small ones, same context and buffer.
// The wavefront's maximum, in its lane 63, by data-parallel-primitive moves inside the vector unit (six ds_bpermute round
// trips, with their address arithmetic, were 64 instructions): neighbours, pairs, mirrored halves and rows leave every lane
// of a row of 16 with the row's maximum; lane 15 of each row is then handed to the next row, lane 31 to the upper half.
// All 64 lanes must be active.
#define DPP_MAX_STEP(v, ctrl, rows) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rows, 0xF, false))
__device__ __forceinline__ uint32_t wave_max_lane63(uint32_t v) {
    DPP_MAX_STEP(v, 0xB1, 0xF);   // quad_perm [1,0,3,2]
    DPP_MAX_STEP(v, 0x4E, 0xF);   // quad_perm [2,3,0,1]
    DPP_MAX_STEP(v, 0x141, 0xF);  // row_half_mirror
    DPP_MAX_STEP(v, 0x140, 0xF);  // row_mirror
    DPP_MAX_STEP(v, 0x142, 0xA);  // row_bcast:15 into rows 1 and 3 (a row left out takes 0: no change)
    DPP_MAX_STEP(v, 0x143, 0xC);  // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ void block_raise_max(uint32_t *p, uint32_t v, uint32_t *s_m) {
    v = wave_max_lane63(v);
    if ((threadIdx.x & 63) == 63 && v) atomicMax(s_m, v);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t m = *s_m;
        if (m > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(p, m);
    }
}

// The same for kernels whose threads are a flat index over planes (a wavefront may straddle two images): one atomic per
// wavefront when all its lanes belong to one image, per lane otherwise.  img < 0: the lane has nothing to report.  All lanes
// of the wavefront call it.  (One atomic per THREAD on one word per image made the two-pass forward level 17 ms per 1080p
// picture: six million atomics on the same address.)
__device__ __forceinline__ void wave_raise_max(uint32_t *maxabs, int img, uint32_t v) {
    const int any = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane(img, __builtin_ctzll(__ballot(img >= 0) | (1ull << 63))));
    if (__ballot(img >= 0) == 0) return;
    if (__all(img < 0 || img == any)) {
        for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
        if ((threadIdx.x & 63) == 0 && v > __hip_atomic_load(&maxabs[any], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&maxabs[any], v);
    } else if (img >= 0 && v) {
        atomicMax(&maxabs[img], v);
    }
}

// i mod P for P > 0, in [0, P).  An index within one period either side of [0, P) -- every index a tile asks for when the
// picture is at least as long as the filter -- takes an add or a subtract; the software division runs only for the rest
// (pictures shorter than the filter, the unused rows of a tile far below a short picture).
__device__ __forceinline__ int ext_mod(int i, int P) {
    int m = i < 0 ? i + P : i;
    if (m >= P) m -= P;
    if ((unsigned)m >= (unsigned)P) {
        m = i % P; if (m < 0) m += P;
    }
    return m;
}
__device__ __forceinline__ int ext_index(int i, int N, int mode) {
    if (i >= 0 && i < N) return i;
    switch (mode) {
    case 0: {  // reflect (whole-sample symmetric)
        if (N == 1) return 0;
        int P = 2 * (N - 1);
        int m = ext_mod(i, P);
        return m < N ? m : P - m;
    }
    case 1: {  // symmetric (half-sample)
        int P = 2 * N;
        int m = ext_mod(i, P);
        return m < N ? m : P - 1 - m;
    }
    case 2: {  // periodic
        return ext_mod(i, N);
    }
    case 4: return i < 0 ? 0 : N - 1;  // constant
    default: return -1;                 // zero
    }
}

__device__ __forceinline__ int32_t quant(double v, double m, double q, bool has_m) {
    if (has_m) v = m * v;
    v = v * q;
    return (int32_t)v;
}
__device__ __forceinline__ double dequant(int32_t r, double m, double q, bool has_m) {
    double v = (double)r;
    if (has_m) v = v / m;
    return v / q;
}

// 8-bit pixels (common.h: PxView): k -> the double k / 255.0, numpy's P / 255 in every bit.  Not a division (a dozen float64
// instructions; 28 of them per thread and tile cost level 1 of 256 1080p pictures about 0.4 ms) and not k * (1/255) alone
// (24 of the 256 quotients differ): the product corrected once by its exact residual, which gives the correctly rounded
// quotient for all 256 k (tests/test_u8_cpu.py proves the algorithm for all of them).
// v -> (uint8)(clip(v, 0, 1) * 255.0) truncated, NaN -> 0 (fmax / fmin return the number of a NaN pair)
__device__ __forceinline__ double px8_value(uint8_t k) {
    const double x = (double)k, r = 1.0 / 255.0;
    const double q = x * r;
    return fma(fma(-q, 255.0, x), r, q);
}
__device__ __forceinline__ uint8_t px8_store_value(double v) {
    const double c = fmin(fmax(v, 0.0), 1.0);
    const double s = c * 255.0;
    return (uint8_t)(uint32_t)s;
}
// 16-bit pixels: the same rules with 65535 for 255.  k * (1/65535) alone misses 88 of the 65536 quotients; the corrected
// product gives all of them (tests/test_u16_cpu.py proves it), and (uint16)((k / 65535.0) * 65535.0) is k for every k.
__device__ __forceinline__ double px16_value(uint16_t k) {
    const double x = (double)k, r = 1.0 / 65535.0;
    const double q = x * r;
    return fma(fma(-q, 65535.0, x), r, q);
}
__device__ __forceinline__ uint16_t px16_store_value(double v) {
    const double c = fmin(fmax(v, 0.0), 1.0);
    const double s = c * 65535.0;
    return (uint16_t)(uint32_t)s;
}
// The pixel kind of a level-1 kernel (template parameter PX): PX_F64 reads / writes the dense float64 planes a.in / a.out,
// the integer kinds the strided view a.px (common.h: PxView; byte strides, so a sample's address is formed in bytes for
// both) -- the value of an integer kind is its element size.  PX_FLT: float32 / float16 / bfloat16 samples (floatpx.h)
// through the same view, stored by the inverse kernels (rounded once) and loaded by the forward ones (widened exactly);
// which of the three is the view's `kind`, uniform over the launch, so the one instantiation serves them all (every kind
// multiplies the level-1 kernels by the wavelet instantiations).
enum PxKind : int { PX_F64 = 0, PX_U8 = 1, PX_U16 = 2, PX_FLT = 3 };
// the pixel kind of a launch into / out of the view px
static inline int px_kind_of(const PxView &px) { return px.kind ? PX_FLT : px.es == 2 ? PX_U16 : PX_U8; }
// The one place where a run-time kind becomes a template parameter: f(std::integral_constant<int, PX>{}), which a launcher's generic
// lambda takes as `auto PX`.  f is instantiated for all four kinds: a kernel without a float64 form goes under `if constexpr`.
template <typename Fn> static inline void with_px(int px, Fn &&f) {
    switch (px) {
    case PX_FLT: f(std::integral_constant<int, PX_FLT>{}); break;
    case PX_U16: f(std::integral_constant<int, PX_U16>{}); break;
    case PX_U8: f(std::integral_constant<int, PX_U8>{}); break;
    default: f(std::integral_constant<int, PX_F64>{}); break;
    }
}
// bit j set = tap j of lo / hi is non-zero (the LOM / HIM of the tiled kernels of both directions)
static inline void tap_masks(const double *lo, const double *hi, int F, uint32_t &lom, uint32_t &him) {
    lom = him = 0;
    for (int j = 0; j < F; j++) {
        if (lo[j] != 0.0) lom |= 1u << j;
        if (hi[j] != 0.0) him |= 1u << j;
    }
}
// a float sample at its byte address: 4 bytes of float32, else the 2 of float16 / bfloat16
__device__ __forceinline__ void flt_store(uint8_t *p, double v, int kind) {
    const uint32_t b = flt_store_value(v, kind);
    if (kind == SPIHT_FLT_F32) *reinterpret_cast<uint32_t *>(p) = b;
    else *reinterpret_cast<uint16_t *>(p) = (uint16_t)b;
}
// (kind: the view's, read by PX_FLT alone -- 4 bytes of float32, else the 2 of float16 / bfloat16; widened exactly, floatpx.h)
template <int PX> __device__ __forceinline__ uint32_t px_load(const uint8_t *p, int kind = 0) {  // the raw sample, not yet converted
    if constexpr (PX == PX_FLT) return kind == SPIHT_FLT_F32 ? *reinterpret_cast<const uint32_t *>(p) : (uint32_t)*reinterpret_cast<const uint16_t *>(p);
    else if constexpr (PX == PX_U16) return *reinterpret_cast<const uint16_t *>(p);
    else return *p;
}
template <int PX> __device__ __forceinline__ double px_value(uint32_t raw, int kind = 0) {
    if constexpr (PX == PX_FLT) return flt_load_value(raw, kind);
    else if constexpr (PX == PX_U16) return px16_value((uint16_t)raw);
    else return px8_value((uint8_t)raw);
}
// p[o] = the stored form of v.  The 8-bit statement is the one the kernels held before there was a second integer kind,
// as a statement of its own: their instruction order stays what it was.
// (kind: the view's, read by PX_FLT alone)
#define PX_STORE(PX, p, o, v, kind)                                                         \
    do {                                                                                    \
        if constexpr ((PX) == PX_FLT) flt_store((p) + (o), v, kind);                        \
        else if constexpr ((PX) == PX_U16) *reinterpret_cast<uint16_t *>((p) + (o)) = px16_store_value(v); \
        else (p)[o] = px8_store_value(v);                                                   \
    } while (0)

// ---- plane descriptors and LDS barrier of the tiled forward kernel and the persistent inverse kernel -----------------
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// a barrier that waits for LDS traffic only: __syncthreads() would wait for the global loads in flight as well
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#define BUF_OOB 0x80000000u  // an offset no plane reaches (the launcher checks): dropped by the descriptor's range check
// Buffer descriptor of `bytes` bytes at p.  p and bytes are workgroup-uniform, but a value that went through a VALU
// division is a VGPR to the instruction selector, and a descriptor in VGPRs costs a waterfall loop per memory
// instruction: its words are read back as scalars here, once.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const void *p, uint32_t bytes) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, (int)__builtin_amdgcn_readfirstlane(bytes),
                                             0x00020000);
}

// the single-precision quantiser (k_dwt_level_f32, and the two-pass level on float32 arrays)
__device__ __forceinline__ int32_t quant_f32(float v, double m, double q, float qf, bool has_m) {
    if (has_m) return (int32_t)((m * (double)v) * q);  // channel_mults[:,None,None] * arr is float64 (wrapper:167-170)
    return (int32_t)(v * qf);                          // arr * q_scale stays float32 (wrapper:9-11)
}

// ---- colour ---------------------------------------------------------------------------------------------------------
#define SPOW_FN __device__ __forceinline__
#define SPOW_FMA(a, b, c) fma((a), (b), (c))
#define SPOW_RINT(a) rint(a)
#define SPOW_LDEXP(a, n) ldexp((a), (n))
#define SPOW_TABLE_QUAL __device__ const
#include "spow_tables.h"
#include "spow.h"

// the three tables of the power function, copied to LDS by every kernel that converts colours (per-lane table reads)
struct SpowLds {
    double inv[SPOW_N], log2c[SPOW_N], exp2t[SPOW_N];
};
__device__ __forceinline__ void spow_lds_fill(SpowLds &t, int tid) {  // needs a barrier before the first use
    if (tid < SPOW_N) { t.inv[tid] = SPOW_INV[tid]; t.log2c[tid] = SPOW_LOG2C[tid]; t.exp2t[tid] = SPOW_EXP2[tid]; }
}

// One pixel of the colour model change.  Shared by the stand-alone kernel (k_color3) and the fused level-1 kernels, and
// every unit that includes this is compiled without multiply-add contraction: the three produce the same bits.  Every operation
// here and in spow.h is a correctly rounded IEEE one in a fixed order, so the device gives, bit for bit, what the same header
// gives on the host inside the same sums: tests/test_gpu_colour.py holds k_color3 to that (tests/colour_cases.py: color3_rule),
// and tests/test_colour_cases.py holds the host build to 60-digit arithmetic.  (The CPU checker, oracle/color_oracle.c, is an
// arithmetic of its own with the C library's pow(): the device is held to it within a tolerance besides,
// tests/test_gpu_image.py.)  numpy's dot order.
__device__ __forceinline__ void color3_px(const Color3 &c, const SpowLds &t, double u0, double u1, double u2, double &w0,
                                          double &w1, double &w2) {
    double v[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double x = (u0 * c.A[3 * r] + u1 * c.A[3 * r + 1]) + u2 * c.A[3 * r + 2];
#ifdef SPIHT_COLOR_POW   // diagnostic: the device library's pow() (<= 1 ulp, about 250 float64 instruction slots per call)
        const double m = pow(fabs(x), c.p);
        v[r] = x < 0.0 ? -m : (x > 0.0 ? m : 0.0);
#else
        v[r] = spow_signed(x, c.p, t.inv, t.log2c, t.exp2t);
#endif
    }
    w0 = (v[0] * c.M[0] + v[1] * c.M[1]) + v[2] * c.M[2];
    w1 = (v[0] * c.M[3] + v[1] * c.M[4]) + v[2] * c.M[5];
    w2 = (v[0] * c.M[6] + v[1] * c.M[7]) + v[2] * c.M[8];
}
