// Float pixels out (include/spiht_hip.h, *_flt): a float64 sample as float32, float16 or bfloat16, rounded ONCE to nearest,
// ties to even -- the rule of spiht_amd/floatpx.py, which the tests hold this header to.  No clip, no scale: overflow gives
// +-inf, subnormals of the target are kept, the sign of zero is kept, NaN gives a NaN.
//
// float32 is the hardware's conversion.  The two 16-bit kinds must not go through it as it is: float64 -> float32 -> float16
// rounds twice, and is wrong a few dozen times per small picture (bior2.2's dyadic taps put decoded samples a hair off the ties
// of the narrow types).  They go through float32 rounded TO ODD instead -- the truncated value with its last bit set when
// anything was cut off -- which a second rounding to nearest even cannot be misled by, as long as it drops two bits or more:
// 24 significand bits against 11 and 8.  The sticky bit survives float32's subnormal range (the smallest subnormal stands for
// "something, below every tie of the 16-bit kinds"), and float32's largest finite value stands for everything above it, which
// both 16-bit kinds round to infinity.  Round to odd from the hardware's round to nearest: convert, convert back, and where
// the two differ step back one pattern if the conversion went away from zero, then set the last bit (-ffp-contract and the
// absence of fast-math keep the comparison honest).  float16 is then the hardware's float32 -> float16 conversion, bfloat16
// the usual nearest-even on the float32 bits.  All of this holds only while float32 and float16 denormals are not flushed:
// the library is built that way (no -fgpu-flush-denormals-to-zero, no fast-math), and the conversion test's subnormal inputs
// fail if it is not.
#pragma once
#include <stdint.h>

#define SPIHT_FLT_F32 1
#define SPIHT_FLT_F16 2
#define SPIHT_FLT_BF16 3

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLT_HD __host__ __device__ __forceinline__
#else
#define FLT_HD inline
#endif

// bytes per sample of a kind; 0: not a kind
FLT_HD int flt_itemsize(int kind) { return kind == SPIHT_FLT_F32 ? 4 : (kind == SPIHT_FLT_F16 || kind == SPIHT_FLT_BF16) ? 2 : 0; }

// the bits of v as a float32 rounded to odd (a NaN stays one)
FLT_HD uint32_t flt_f32_round_odd(double v) {
    const float f = (float)v;  // to nearest even
    const double d = (double)f;
    uint32_t b = __builtin_bit_cast(uint32_t, f);
    if (d != v) {  // inexact
        if (__builtin_fabs(d) > __builtin_fabs(v)) b -= 1u;  // it went away from zero: one pattern back is the truncation
        b |= 1u;
    }
    return b;
}

// the bit pattern of v in the kind (in the low 16 bits for the two 16-bit kinds).  `kind` is uniform wherever this is called.
FLT_HD uint32_t flt_store_value(double v, int kind) {
    if (kind == SPIHT_FLT_F32) return __builtin_bit_cast(uint32_t, (float)v);
    const uint32_t b = flt_f32_round_odd(v);
    if (kind == SPIHT_FLT_F16) return __builtin_bit_cast(uint16_t, (_Float16)__builtin_bit_cast(float, b));
    if (v != v) return (b >> 16) | 0x40u;                 // NaN: the quiet one of its sign (the rounding below could carry out of it)
    return (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;        // nearest even on the float32 bits; a carry runs up to infinity by itself
}

// Float pixels in (include/spiht_hip.h, the encode side of *_flt): the bit pattern of a sample of the kind (in the low 16 bits
// for the two 16-bit kinds) as the double of the same value -- the rule of spiht_amd/floatpx.py: to_float64.  Every step is
// exact: float32 -> float64 is the hardware's conversion, float16 goes half -> float -> double (each type holds every value
// of the one before it), and a bfloat16 is the upper half of the float32 of the same value.  Subnormals keep their value (no
// flush, see above), the sign of zero is kept, infinities stay, a NaN gives a NaN.  `kind` is uniform wherever this is called.
FLT_HD double flt_load_value(uint32_t raw, int kind) {
    if (kind == SPIHT_FLT_F32) return (double)__builtin_bit_cast(float, raw);
    if (kind == SPIHT_FLT_F16) return (double)(float)__builtin_bit_cast(_Float16, (uint16_t)raw);
    return (double)__builtin_bit_cast(float, raw << 16);
}
