"""Float pixels in: what tests/test_floatin_cpu.py and tests/test_gpu_floatin.py share -- the picture generator, the bit views,
and the oracle's streams of a picture in double and in single precision.  No device and no library needed."""
import functools

import numpy as np

KINDS = ("float32", "float16", "bfloat16")
LOW_BITS = {"float32": 8, "float16": 4, "bfloat16": 3}  # the low mantissa bits whose every value a picture holds


def bits(a):
    """an array of a kind as unsigned integers: equality of these is equality of every bit (-0.0 is not 0.0)"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def widen(a, kind):
    from spiht_amd import floatpx
    return floatpx.to_float64(a, kind)


@functools.lru_cache(maxsize=None)
def _float_image(kind, seed, c, H, W):
    from spiht_amd import floatpx
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    planes = []
    for ch in range(c):
        fy, fx = rng.uniform(0.6, 1.7, 2)
        py, px = rng.uniform(0.0, 2 * np.pi, 2)
        smooth = 0.4 + 0.45 * np.sin(2 * np.pi * fy * y / max(H, 8) + py) * np.sin(2 * np.pi * fx * x / max(W, 8) + px)
        steps = 0.2 * (((y // 13).astype(np.int64) + (x // 19).astype(np.int64) + ch) % 2)
        planes.append(smooth + steps + rng.normal(0.0, 0.01, (H, W)))
    P = floatpx.convert(np.stack(planes), kind)
    v = floatpx.to_float64(P, kind)
    assert np.isfinite(v).all()
    if c * H * W >= 8192:  # what a picture of some size shows: every value of the low bits ...
        n = LOW_BITS[kind]
        assert len(np.unique(bits(P) & ((1 << n) - 1))) == 1 << n
    if c >= 3 and H * W >= 57 * 83:  # ... and samples on both sides of [0, 1]
        assert (v < 0).sum() >= 20 and (v > 1).sum() >= 20, (v.min(), v.max(), (v < 0).sum(), (v > 1).sum())
    P.setflags(write=False)
    return P


def float_image(kind, seed, c, H, W):
    """A picture [c, H, W] of the kind (float32, float16, or uint16 bit patterns of bfloat16): a smooth pattern of amplitude
    0.45 around 0.4, plus steps of 0.2, plus N(0, 0.01) noise, each sample rounded once to the kind (floatpx.convert) -- so
    that some samples lie below 0 and some above 1 (nothing may clip them) and the low mantissa bits of the kind take every
    value (a conversion that drops them shows).  Read-only, computed once per argument tuple."""
    return _float_image(kind, int(seed), int(c), int(H), int(W))


def clear_last_bit(P):
    """the picture with the last mantissa bit of every sample cleared: what a conversion one bit short would read"""
    P = np.ascontiguousarray(P)
    return (bits(P) & ~bits(P).dtype.type(1)).view(P.dtype)


def oracle_stream(O, img64, wavelet, mode, level, q, max_bits):
    """the oracle's double-precision path of a float64 picture -> (quantised array, bytes, max_n)"""
    g = O.geometry(img64.shape[1], img64.shape[2], wavelet, level, mode)
    co = O.quantize(O.wavedec2_array(img64, wavelet, mode, level)[0], q, None)
    data, n, _ = O.encode_nbits(co, g["ll_h"], g["ll_w"], max_bits)
    return co, data, n


def oracle_stream_f32(O, img32, wavelet, mode, level, q, max_bits):
    """the oracle's single-precision path of a float32 picture (what encode_image does with it)"""
    g = O.geometry(img32.shape[1], img32.shape[2], wavelet, level, mode)
    co = O.quantize_f32(O.wavedec2_array_f32(img32, wavelet, mode, level)[0], q, None)
    data, n, _ = O.encode_nbits(co, g["ll_h"], g["ll_w"], max_bits)
    return co, data, n
