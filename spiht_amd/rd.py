"""Rate-distortion curve of a stream, and the cut of a stream to a target quality.

A SPIHT stream decodes at any prefix; this module says how good a prefix is.  rd_curve evaluates K prefixes of one
stream without bringing a picture back: the stream is walked once per group of prefixes (spiht_decode_budgets_dev_i32), the
K coefficient arrays are compared with the encoder's own quantised array (spiht_sqerr_i32, exact), inverse-transformed in
one batched launch and compared with the original picture (spiht_sse_f64 / _u8 / _u16), all in HBM; K small rows come
back.  cut_to_psnr / cut_to_sqerr search the prefix lengths on that curve, `points` lengths per walk.

The reference has nothing of the kind (its make_gif.py decodes a prefix per frame and looks at it).
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Any, List

import numpy as np

from . import _lib, px
from .spiht_wrapper import EncodingResult, SpihtSettings, _check_version, _int_picture

PEAK = {None: 1.0, px.U8.storage: int(px.U8.peak), px.U16.storage: int(px.U16.peak)}  # by dtype; None: float pixels


@dataclass
class RDCurve:
    """The curve at K prefixes of one stream, rows in the order the lengths were given.
    byte_lengths -- as given; bits -- 8 * min(length, len(stream)), the bits the decoder reads; coef_sqerr -- sum (X - X_k)^2
    over the quantised coefficient arrays, Python ints (exact); sse -- [K][c] per channel over the h x w picture: float64
    for float pixels, Python ints (exact) for 8- / 16-bit pixels; mse -- sum_ch sse / (c h w); psnr -- 10 log10(peak^2 / mse)
    in dB with peak 1.0, 255 or 65535, inf where mse is 0; bpp -- bits / (h w)."""
    byte_lengths: List[int]
    bits: List[int]
    coef_sqerr: List[int]
    sse: Any
    mse: List[float]
    psnr: List[float]
    bpp: List[float]


# ---- host arithmetic (no device) ---------------------------------------------------------------------------------------

def _points_arg(points):
    if isinstance(points, bool) or not isinstance(points, (int, np.integer)):
        raise TypeError("points must be an integer, not %s" % type(points).__name__)
    if points < 1:
        raise ValueError("points = %d: at least one length per curve" % points)
    return int(points)


def _lengths_arg(byte_lengths):
    lens = []
    for k in byte_lengths:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError("a byte length must be an integer, not %s" % type(k).__name__)
        if k < 0:
            raise ValueError("byte length %d is negative" % k)
        lens.append(int(k))
    return lens


def _target_arg(target, name):
    target = float(target)
    if math.isnan(target):
        raise ValueError("%s is NaN" % name)
    return target


def default_lengths(n, points):
    """`points` byte lengths evenly spaced over 1 .. n, strictly ascending, the last one n; fewer when n < points (every
    length once); [0] for an empty stream"""
    points = _points_arg(points)
    if n <= 0:
        return [0]
    return sorted({-(-n * i // points) for i in range(1, points + 1)})


def group_size(c, enc_h, enc_w, rec_h, rec_w, max_bytes):
    """budgets per group: as many as keep K_g c (enc_h enc_w 4 + rec_h rec_w 8) bytes within max_bytes, at least one"""
    per = c * (enc_h * enc_w * 4 + rec_h * rec_w * 8)
    return max(1, int(max_bytes) // per)


def psnr_of(mse, peak):
    """10 log10(peak^2 / mse) in dB; inf for mse == 0"""
    return math.inf if mse == 0 else 10.0 * math.log10(float(peak) * float(peak) / mse)


def curve_from_sums(byte_lengths, n, coef_sqerr, sse, c, h, w, peak):
    """RDCurve from the rows the device returns; sse: [K][c] floats or Python ints.  The channel sums are added in channel
    order; integer sums are divided as integers (one rounding)."""
    bits = [8 * min(k, n) for k in byte_lengths]
    mse = []
    for row in sse:
        total = row[0]
        for v in row[1:]:
            total = total + v
        mse.append(total / (c * h * w))
    return RDCurve(list(byte_lengths), bits, [int(e) for e in coef_sqerr], sse, [float(m) for m in mse],
                   [psnr_of(m, peak) for m in mse], [b / (h * w) for b in bits])


def search_rounds_bound(n, points):
    """rounds search_cut needs at most after its first look at the whole stream: ceil(log(n + 1) / log(points + 1)),
    in integers"""
    t = 0
    while (points + 1) ** t < n + 1:
        t += 1
    return t


def search_cut(n, points, evaluate, passes):
    """The search of cut_to_psnr / cut_to_sqerr on lengths 0 .. n.  evaluate(lengths) -> one value per length (one curve
    call); passes(value) -> bool.  Returns (L, value at L, met).
    The whole stream is looked at first: if it does not pass, (n, value, False).  Otherwise, with the invariant "hi passes,
    lo fails or is -1", each round evaluates at most `points` lengths evenly spaced inside (lo, hi), moves hi to the
    smallest that passes and lo to the largest evaluated length below it, until hi - lo == 1.  A round leaves at most
    floor(m / (points + 1)) of its m unknown lengths, so there are at most search_rounds_bound(n, points) rounds.
    What holds for L: it passes, and L == 0 or L - 1 was evaluated and fails -- a crossing; the smallest passing length
    only if the values are monotone in the length."""
    points = _points_arg(points)
    value = evaluate([n])[0]
    if not passes(value):
        return n, value, False
    lo, hi = -1, n
    while hi - lo > 1:
        gap = hi - lo
        p = min(points, gap - 1)
        cand = [lo + i * gap // (p + 1) for i in range(1, p + 1)]
        for length, v in zip(cand, evaluate(cand)):
            if passes(v):
                hi, value = length, v
                break
            lo = length
    return hi, value, True


# ---- the curve on the device -------------------------------------------------------------------------------------------

def _prefix(result, length):
    return EncodingResult(result.encoded_bytes[:length], result.h, result.w, result.c, result.max_n, result.level,
                          result._encoding_version)


def _picture(codec, image, elem):
    """the checks on `image`: one picture of the codec's geometry, float (px.F64) or of the integer element"""
    if not elem.integer:
        if codec.pixel_dtype != np.float64:
            raise ValueError("rd_curve takes the pictures of a float64 codec")
        image = np.ascontiguousarray(image, dtype=np.float64)
    else:
        image = np.ascontiguousarray(_int_picture(image, codec.settings, elem.storage, "rd_curve_" + elem.suffix))
    if image.shape != (codec.c, codec.H, codec.W):
        raise ValueError("a picture of shape %s, the codec's are %s" % (image.shape, (codec.c, codec.H, codec.W)))
    return image


def codec_rd_curve(codec, image, result=None, byte_lengths=None, points=32, max_bytes=2 ** 31, elem=px.F64, kept=None):
    """BatchCodec.rd_curve / rd_curve_u8 / rd_curve_u16 (elem px.F64 / px.U8 / px.U16); returns (RDCurve, result).
    kept: a list, empty at first, in which the picture and X stay on the device from one call to the next of the same
    picture and stream (the rounds of a search: codec_cut, which frees them)"""
    from .batch import DeviceArray
    points = _points_arg(points)
    if byte_lengths is not None:
        byte_lengths = _lengths_arg(byte_lengths)
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, (int, np.integer)) or max_bytes < 0:
        raise ValueError("max_bytes must be a non-negative integer")
    image = _picture(codec, image, elem)
    view = (None,) if elem.view else ()  # the integer calls take a view: dense here, no strides
    if result is not None:
        _check_version(result)
        if (result.c, result.h, result.w, result.level) != (codec.c, codec.H, codec.W, codec.level):
            raise ValueError("the stream is not of the codec's geometry")
    ctx, L, g, c, H, W = codec.ctx, codec.L, codec.geom, codec.c, codec.H, codec.W
    vp = C.c_void_p
    q = float(codec.settings.quantization_scale)
    held = []

    def dev(shape, dt):
        held.append(DeviceArray(ctx, shape, dt))
        return held[-1]

    try:
        fresh = not kept
        if fresh:
            d_pic = DeviceArray(ctx, image.shape, image.dtype)
            d_x = DeviceArray(ctx, (c, g["enc_h"], g["enc_w"]), np.int32)
            (held if kept is None else kept).extend((d_pic, d_x))
            d_pic.upload(image)
            elem.check_aligned(d_pic.ptr)
        else:
            d_pic, d_x = kept
        if not fresh:
            pass  # the picture and X are there from an earlier round
        elif result is None:
            # a batch of one: X is the array the encoder handed to the list coder
            d_out, d_nbits, d_maxn = dev((1, codec.slot_stride), np.uint8), dev((1,), np.uint64), dev((1,), np.uint8)
            codec._encode_device(elem, d_pic.ptr, 1, d_out.ptr, d_nbits.ptr, d_maxn.ptr, None, d_x.ptr)
            ctx.synchronize()
            nbits = int(d_nbits.download()[0])
            result = EncodingResult(d_out.download()[0, :(nbits + 7) // 8].tobytes(), H, W, c, int(d_maxn.download()[0]),
                                    codec.level)
        else:
            # the forward transform of the picture with the codec's settings (the pyramid left out)
            d_maxabs = dev((1,), np.uint32)
            with codec._color():
                _lib.check(elem.entry(L, "spiht_dwt_pyramid_batch_")(ctx.handle, vp(d_pic.ptr), *view, 1, c, H, W, codec.wid, codec.mid,
                                                                     codec._lv, q, codec._mults_p, vp(d_x.ptr), None, None,
                                                                     vp(d_maxabs.ptr)))
        n = len(result.encoded_bytes)
        lens = default_lengths(n, points) if byte_lengths is None else byte_lengths
        K = len(lens)
        if K == 0:
            return curve_from_sums([], n, [], [], c, H, W, elem.peak), result
        # one row per distinct number of bits read, ascending (what the walk wants); the caller's rows point into them
        uniq = sorted({min(k, n) for k in lens})
        row = {k: i for i, k in enumerate(uniq)}
        U = len(uniq)
        rec_h, rec_w = (H, W) if elem.integer else (g["rec_h"], g["rec_w"])
        Kg = min(U, group_size(c, g["enc_h"], g["enc_w"], g["rec_h"], g["rec_w"], max_bytes), 65535)
        d_rec = dev((Kg, c, g["enc_h"], g["enc_w"]), np.int32)
        d_dec = dev((Kg, c, rec_h, rec_w), image.dtype)
        d_e = dev((U, 2), np.uint64)
        d_s = dev((U, c), np.uint64 if elem.integer else np.float64)
        data = np.frombuffer(result.encoded_bytes[:uniq[-1]], dtype=np.uint8)
        for k0 in range(0, U, Kg):
            kg = min(Kg, U - k0)
            bud = np.ascontiguousarray([8 * k for k in uniq[k0:k0 + kg]], dtype=np.uint64)
            _lib.check(L.spiht_decode_budgets_dev_i32(
                ctx.handle, vp(data.ctypes.data if data.size else 0), data.size, int(result.max_n), c, g["enc_h"], g["enc_w"],
                g["ll_h"], g["ll_w"], vp(bud.ctypes.data), kg, vp(d_rec.ptr)))
            _lib.check(L.spiht_sqerr_i32(ctx.handle, vp(d_x.ptr), vp(d_rec.ptr), kg, c, g["enc_h"], g["enc_w"],
                                         vp(d_e.ptr + 16 * k0)))
            idwt = (kg, c, H, W, codec.wid, codec.mid, codec._lv, q, codec._mults_p, vp(d_dec.ptr))
            sse = elem.entry(L, "spiht_sse_")
            with codec._color():
                if elem.integer:  # (the flags form with no flags; both pictures dense)
                    _lib.check(elem.entry(L, "spiht_dequant_idwt_flags_batch_")(ctx.handle, vp(d_rec.ptr), None, *idwt, *view))
                    _lib.check(sse(ctx.handle, vp(d_pic.ptr), *view, vp(d_dec.ptr), kg, c, H, W, vp(d_s.ptr + 8 * c * k0)))
                else:
                    _lib.check(L.spiht_dequant_idwt_batch_f64(ctx.handle, vp(d_rec.ptr), *idwt))
                    _lib.check(sse(ctx.handle, vp(d_pic.ptr), vp(d_dec.ptr), kg, c, H, W, rec_h, rec_w, vp(d_s.ptr + 8 * c * k0)))
        ctx.synchronize()
        e, s = d_e.download(), d_s.download()
    finally:
        for d in held:
            d.free()
    coef = [int(e[row[min(k, n)], 0]) | (int(e[row[min(k, n)], 1]) << 64) for k in lens]
    if elem.integer:
        sse_rows = sums = [[int(v) for v in s[row[min(k, n)]]] for k in lens]
    else:
        sse_rows = np.ascontiguousarray(s[[row[min(k, n)] for k in lens]])
        sums = [[float(v) for v in r] for r in sse_rows]
    curve = curve_from_sums(lens, n, coef, sums, c, H, W, elem.peak)
    curve.sse = sse_rows
    return curve, result


def codec_cut(codec, image, result, points, elem, field, passes):
    """the search on one field of the curve -> (EncodingResult of the cut stream, the field's value there, met)"""
    points = _points_arg(points)
    kept = []  # the picture and X on the device, uploaded and transformed once for all rounds

    def evaluate(lengths):
        curve, _ = codec_rd_curve(codec, image, result, lengths, points, elem=elem, kept=kept)
        return getattr(curve, field)

    try:
        length, value, met = search_cut(len(result.encoded_bytes), points, evaluate, passes)
    finally:
        for d in kept:
            d.free()
    return _prefix(result, length), value, met


# ---- module level, beside encode_image: the codec is built from the picture's shape --------------------------------------

def _codec(image, settings, level, max_bits=None):
    from .batch import BatchCodec
    if getattr(image, "ndim", None) != 3:
        raise ValueError('image ndim must be 3: c,h,w')
    c, h, w = image.shape
    return BatchCodec(c, h, w, settings, level, max_bits)


def _curve_args(byte_lengths, points):
    """the host checks, before a context is asked for"""
    _points_arg(points)
    if byte_lengths is not None:
        _lengths_arg(byte_lengths)


def rd_curve(image, spiht_settings: SpihtSettings = SpihtSettings(), level=None, result=None, byte_lengths=None, points=32,
             max_bits=None, max_bytes=2 ** 31):
    """RDCurve of the float picture (c, h, w): of `result`, a stream of it, or of the stream encode_image(image,
    spiht_settings, level, max_bits) gives (BatchCodec.rd_curve)"""
    _curve_args(byte_lengths, points)
    return _codec(image, spiht_settings, level, max_bits).rd_curve(image, result, byte_lengths, points, max_bytes)


def rd_curve_u8(image, spiht_settings: SpihtSettings = SpihtSettings(), level=None, result=None, byte_lengths=None, points=32,
                max_bits=None, max_bytes=2 ** 31):
    """rd_curve of a uint8 picture (c, h, w): distances between 8-bit pictures, as decode_image_u8 returns them"""
    _curve_args(byte_lengths, points)
    return _codec(image, spiht_settings, level, max_bits).rd_curve_u8(image, result, byte_lengths, points, max_bytes)


def rd_curve_u16(image, spiht_settings: SpihtSettings = SpihtSettings(), level=None, result=None, byte_lengths=None, points=32,
                 max_bits=None, max_bytes=2 ** 31):
    """rd_curve of a uint16 picture (c, h, w)"""
    _curve_args(byte_lengths, points)
    return _codec(image, spiht_settings, level, max_bits).rd_curve_u16(image, result, byte_lengths, points, max_bytes)


def _cut_module(method, image, result, target_db, spiht_settings, points):
    _target_arg(target_db, "target_db")
    _points_arg(points)
    _check_version(result)
    codec = _codec(image, spiht_settings, result.level)
    return getattr(codec, method)(image, result, target_db, points)


def cut_to_psnr(image, result, target_db, spiht_settings: SpihtSettings = SpihtSettings(), points=32):
    """(EncodingResult, psnr, met): a prefix of `result`, a stream of the float picture `image`, that reaches target_db
    (BatchCodec.cut_to_psnr)"""
    return _cut_module("cut_to_psnr", image, result, target_db, spiht_settings, points)


def cut_to_psnr_u8(image, result, target_db, spiht_settings: SpihtSettings = SpihtSettings(), points=32):
    return _cut_module("cut_to_psnr_u8", image, result, target_db, spiht_settings, points)


def cut_to_psnr_u16(image, result, target_db, spiht_settings: SpihtSettings = SpihtSettings(), points=32):
    return _cut_module("cut_to_psnr_u16", image, result, target_db, spiht_settings, points)
