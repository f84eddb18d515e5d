"""Counterpart of the reference's public Python API (/root/reference/spiht/spiht_wrapper.py).

Same names, defaults, field order and exceptions:
    SpihtSettings, EncodingResult, ENCODER_DECODER_VERSION, encode_image, decode_image,
    decode_rec_array, decode_from_rec_arr, get_slices_and_h_w, quantize, dequantize
What differs is where the arithmetic runs: the multilevel DWT (pywt.wavedec2/waverec2 in the reference),
the Mallat packing, the per-channel scaling, the quantisation and the SPIHT coder all execute as HIP kernels
on the MI355X through libspiht_hip.so; the pixel array is uploaded once and only the bitstream comes back.
"""
import ctypes as C
from dataclasses import asdict, dataclass
from typing import Any, List, Optional, Tuple, Union

import numpy as np

from . import _lib, color_models, floatpx, px
from . import spiht as spiht_rs
from .floatpx import check_float_view  # noqa: F401  (the float kinds' view rule, beside check_u8_view / check_u16_view)
from .px import _check_aligned, _check_int_view, _is_dtype  # noqa: F401  (the rules by dtype; px.Elem has them by element)


def quantize(arr, q_scale=10.):
    """wrapper:9-11 (host helper kept for API parity; the hot path quantises inside the DWT kernel)"""
    arr = arr * q_scale
    return arr.astype(np.int32)


def dequantize(arr, q_scale=10.):
    """wrapper:13-14"""
    return arr / q_scale


ENCODER_DECODER_VERSION = "0.0.2"


@dataclass
class SpihtSettings:
    """Parameters that are not particular to a single image (wrapper:20-63): field order is API
    (demonstrate.py:23-29 passes them positionally)."""
    wavelet: str = 'bior2.2'
    quantization_scale: float = 50.0
    mode: str = 'reflect'
    color_model: Optional[str] = None
    per_channel_quant_scales: Optional[List[float]] = None


@dataclass
class EncodingResult:
    """wrapper:65-89.  h, w, c are IMAGE dims; level may be None."""
    encoded_bytes: bytes
    h: int
    w: int
    c: int
    max_n: int
    level: Optional[int]
    _encoding_version: str = ENCODER_DECODER_VERSION

    def to_dict(self):
        return {f"encoding_result_{k}": v for k, v in asdict(self).items()}

    @staticmethod
    def from_dict(d):
        d = {k.removeprefix('encoding_result_'): v for k, v in d.items() if k.startswith('encoding_result_')}
        return EncodingResult(**d)


def _wavelet_mode_ids(spiht_settings):
    L = _lib.lib()
    wid = L.spiht_wavelet_id(str(spiht_settings.wavelet).encode())
    if wid < 0:
        # pywt.Wavelet(name) raises this ValueError for a name it does not know (spiht_wrapper.py:163 reaches it through
        # wavedec2); all 106 discrete wavelets of PyWavelets are known here (csrc/wavelets.h)
        raise ValueError("Unknown wavelet name '%s', check wavelist() for the list of available builtin wavelets." % spiht_settings.wavelet)
    mid = L.spiht_mode_id(str(spiht_settings.mode).encode())
    if mid < 0:
        # pywt.Modes.from_object raises ValueError("Unknown mode name '...'.") (reached from spiht_wrapper.py:163)
        raise ValueError("Unknown mode name '%s'." % spiht_settings.mode)
    return wid, mid


def _geometry(h, w, wid, level, mid=0):
    """sizes of the packed coefficient array; mid: the extension mode's id (periodization has its own length rule)"""
    L = _lib.lib()
    lv = C.c_int()
    v = [C.c_int64() for _ in range(6)]
    if level is not None and level < 0:
        raise ValueError("Level value of %d is too low . Minimum level is 0." % level)
    _lib.check(L.spiht_geometry_mode(int(h), int(w), wid, int(mid), -1 if level is None else int(level), C.byref(lv),
                                     *[C.byref(t) for t in v]))
    return dict(level=lv.value, ll_h=v[0].value, ll_w=v[1].value, enc_h=v[2].value, enc_w=v[3].value,
                rec_h=v[4].value, rec_w=v[5].value)


def _filter_len(wavelet):
    """pywt.Wavelet(name).dec_len, from the library's table"""
    L = _lib.lib()
    return L.spiht_wavelet_taps(L.spiht_wavelet_id(str(wavelet).encode()))


def get_slices_and_h_w(h: int, w: int, spiht_settings: SpihtSettings, level: Optional[int]):
    """wrapper:92-139: the pywt.coeffs_to_array slices of a (1,h,w) wavedec2, the height and the width of the
    packed coefficient array.  Closed form len' = (len + F - 1)//2 instead of pywt.wavedecn_shapes."""
    wid, mid = _wavelet_mode_ids(spiht_settings)
    g = _geometry(h, w, wid, level, mid)
    hs, ws = _band_sizes(h, w, spiht_settings.wavelet, g["level"], spiht_settings.mode)
    start_h, start_w = hs[-1], ws[-1]
    slices: List[Any] = [(slice(None), slice(start_h), slice(start_w))]
    for lv in range(g["level"], 0, -1):
        dh, dw = hs[lv], ws[lv]
        slices.append({
            "ad": (slice(None), slice(0, dh), slice(start_w, start_w + dw)),
            "da": (slice(None), slice(start_h, start_h + dh), slice(0, dw)),
            "dd": (slice(None), slice(start_h, start_h + dh), slice(start_w, start_w + dw)),
        })
        start_h += dh
        start_w += dw
    return slices, start_h, start_w


def _mults_arg(per_channel_quant_scales, c):
    if per_channel_quant_scales is None:
        return None, None
    m = np.ascontiguousarray(np.array(per_channel_quant_scales), dtype=np.float64)
    if m.ndim != 1 or m.shape[0] != c:
        # numpy broadcasting of channel_mults[:,None,None] * coeffs_arr fails the same way (wrapper:167-170)
        raise ValueError("operands could not be broadcast together with shapes (%d,1,1) (%d,...)" % (m.shape[0], c))
    return m, C.c_void_p(m.ctypes.data)


def encode_image(image: np.ndarray, spiht_settings: SpihtSettings = SpihtSettings(), level: Optional[int] = None,
                 max_bits: Optional[int] = None):
    """wrapper:142-189.  image: (C,H,W) floating point pixels.  Returns EncodingResult."""
    if image.ndim != 3:
        raise ValueError('image ndim must be 3: c,h,w')
    c, h, w = image.shape

    # wrapper:158-160: the colour model change happens on the GPU, inside level 1 of the transform (color_models.fused)
    color_model = spiht_settings.color_model
    if color_model is not None:
        if color_model not in color_models.SUPPORTED_MODELS:
            color_models.convert(image, 'RGB', color_model)  # raises the reference's ValueError
        if c != 3:
            raise ValueError("colour conversion needs 3 channels")
        if image.dtype in (np.float32, np.float16):
            image = image.astype(np.float64)  # colour-science computes in float64; so does the transform that follows

    wid, mid = _wavelet_mode_ids(spiht_settings)
    g = _geometry(h, w, wid, level, mid)
    mults, mults_p = _mults_arg(spiht_settings.per_channel_quant_scales, c)

    if max_bits == None:  # noqa: E711  (as the reference)
        max_bits = 99999999999999999
    max_bits = spiht_rs._as_usize(max_bits, "max_bits")

    ctx = _lib.default_context()
    L = _lib.lib()
    # PyWavelets' dtype rule (_check_dtype): float32 and float16 pixels are transformed in single precision (and then
    # quantised in single precision, wrapper:163-172), everything else in double
    f32 = image.dtype in (np.float32, np.float16)
    img = np.ascontiguousarray(image, dtype=np.float32 if f32 else np.float64)
    if f32 and g["level"] == 0:
        raise ValueError("float32 pixels with level 0 are not supported; pass float64 pixels")
    return _encode_host(ctx, L.spiht_encode_image_host_f32 if f32 else L.spiht_encode_image_host_f64, (C.c_void_p(img.ctypes.data),),
                        (c, h, w), g, wid, mid, level, spiht_settings, mults_p, max_bits)


def _encode_host(ctx, fn, pixels, chw, g, wid, mid, level, spiht_settings, mults_p, max_bits):
    """the tail of encode_image / encode_image_u8 / encode_image_u16: one C call fn(ctx, *pixels, c, h, w, ...) -- upload, DWT + quantise +
    pyramid + list coder, stream back (the context keeps its device buffers) -- into a buffer of the stream's bound"""
    c, h, w = chw
    bound = C.c_uint64()
    _lib.check(_lib.lib().spiht_encode_bound(c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"], 0x3FFFFFFF, max_bits,
                                             C.byref(bound)))
    out = np.empty(max(int(bound.value), 4), dtype=np.uint8)
    nbits, mn = C.c_uint64(), C.c_uint8()
    with color_models.fused(ctx, spiht_settings.color_model):
        _lib.check(fn(ctx.handle, *pixels, c, h, w, wid, mid, -1 if level is None else int(level),
                      float(spiht_settings.quantization_scale), mults_p, max_bits, C.c_void_p(out.ctypes.data), out.size,
                      C.byref(nbits), C.byref(mn)))
    out = out[:(int(nbits.value) + 7) // 8]
    return EncodingResult(out.tobytes(), h, w, c, int(mn.value), level)


def decode_image(encoding_result: EncodingResult, spiht_settings: SpihtSettings,
                 return_metadata: bool = False) -> Union[np.ndarray, Tuple[np.ndarray, np.ndarray]]:
    """wrapper:192-216"""
    if return_metadata:
        d = decode_rec_array(encoding_result, spiht_settings, return_metadata)
        spiht_metadata = d.pop("spiht_metadata", None)
        image = decode_from_rec_arr(**d, spiht_settings=spiht_settings)
        return image, spiht_metadata
    # decode_rec_array + decode_from_rec_arr (wrapper:218-281) as one C call: the coefficient array never leaves HBM
    return _decode_image_px(encoding_result, spiht_settings, px.F64)


def _check_version(encoding_result):
    if encoding_result._encoding_version != ENCODER_DECODER_VERSION:
        raise ValueError(encoding_result._encoding_version)


def _decode_args(encoding_result, spiht_settings):
    """the checks decode_image, decode_image_u8 and decode_image_u16 share, in their order -> (geometry, the arrays the pointers point into --
    kept by the caller until the call --, the arguments of the C call from the stream to the channel scales)"""
    h, w, c, level = encoding_result.h, encoding_result.w, encoding_result.c, encoding_result.level
    wid, mid = _wavelet_mode_ids(spiht_settings)
    g = _geometry(h, w, wid, level, mid)
    buf = spiht_rs._as_u8_vec(encoding_result.encoded_bytes)
    n = spiht_rs._as_usize(encoding_result.max_n, "n")
    if n > 255:
        raise OverflowError("out of range integral type conversion attempted")
    mults, mults_p = _mults_arg(spiht_settings.per_channel_quant_scales, c)
    return g, (buf, mults), (C.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, n, c, h, w, wid, mid, -1 if level is None else int(level),
               float(spiht_settings.quantization_scale), mults_p)


def check_u8_view(shape, strides, output):
    """The library's rule for an 8-bit view (include/spiht_hip.h, *_u8; spiht_check_view_u8): byte strides of a (B, c, h, w)
    or (c, h, w) `shape` are non-negative, and a view that is written does not overlap itself -- sorted by stride, every
    dimension longer than one steps past the largest offset the smaller ones reach.  Raises ValueError.  No device needed."""
    _check_int_view(8, shape, strides, output)


def check_u16_view(shape, strides, output):
    """The library's rule for a 16-bit view (include/spiht_hip.h, *_u16; spiht_check_view_u16): as check_u8_view, the strides
    still in BYTES (numpy's .strides as they are) and all of them even; the overlap rule counts a sample's two bytes."""
    _check_int_view(16, shape, strides, output)


def _int_picture(image, spiht_settings, dtype, name):
    """checks of encode_image_u8 / encode_image_u16: a (c, h, w) array of `dtype` (or (h, w, c) given as such a view);
    negative strides and the other byte order are copied into a native contiguous array"""
    if not _is_dtype(image, dtype):
        raise ValueError("%s takes a %s array, not %s" % (name, np.dtype(dtype).name, getattr(image, "dtype", type(image)),))
    if image.ndim != 3:
        raise ValueError('image ndim must be 3: c,h,w')
    if spiht_settings.color_model is not None:
        if spiht_settings.color_model not in color_models.SUPPORTED_MODELS:
            color_models.convert(np.zeros((3, 1, 1)), 'RGB', spiht_settings.color_model)  # the reference's ValueError
        if image.shape[0] != 3:
            raise ValueError("colour conversion needs 3 channels")
    if any(st < 0 for st in image.strides) or not image.dtype.isnative:
        image = np.ascontiguousarray(image, dtype=np.dtype(dtype).newbyteorder("="))
    return image


def _encode_image_px(image, spiht_settings, level, max_bits, channels_last, elem, name):
    """the encode calls of the elements that come as a view: the picture goes as it lies, by its own strides"""
    if _is_dtype(image, elem.storage) and image.ndim == 3 and channels_last:
        image = image.transpose(2, 0, 1)
    image = _int_picture(image, spiht_settings, elem.storage, name)
    c, h, w = image.shape
    wid, mid = _wavelet_mode_ids(spiht_settings)
    g = _geometry(h, w, wid, level, mid)
    mults, mults_p = _mults_arg(spiht_settings.per_channel_quant_scales, c)
    if max_bits == None:  # noqa: E711  (as encode_image)
        max_bits = 99999999999999999
    max_bits = spiht_rs._as_usize(max_bits, "max_bits")
    strides = np.array(image.strides, dtype=np.int64)
    elem.check_view(image.shape, strides, False)
    elem.check_aligned(image.ctypes.data)
    return _encode_host(_lib.default_context(), elem.entry(_lib.lib(), "spiht_encode_image_host_"),
                        (C.c_void_p(image.ctypes.data), C.c_void_p(strides.ctypes.data)), (c, h, w), g, wid, mid, level,
                        spiht_settings, mults_p, max_bits)


def _decode_image_px(encoding_result, spiht_settings, elem, channels_last=False, reduce=None, crop=False):
    """every decode call that returns a picture: float64 pictures are the uncropped rec_h x rec_w of the inverse transform,
    dense; a view element's are cropped to the picture (reduce: to the band) and written by strides.  reduce=None: the
    full-size entry point"""
    _check_version(encoding_result)
    er = encoding_result
    rs = None if reduce is None else reduced_shape(er.h, er.w, spiht_settings, er.level, reduce)
    if spiht_settings.color_model is not None and er.c != 3:
        raise ValueError("colour conversion needs 3 channels")
    g, keep, args = _decode_args(er, spiht_settings)
    if elem.view:
        h, w = (er.h, er.w) if rs is None else (rs["pic_h"], rs["pic_w"])
    else:
        h, w = (g if rs is None else rs)["rec_h"], (g if rs is None else rs)["rec_w"]
    c, es = er.c, elem.itemsize
    out = _lib.result_array((h, w, c) if channels_last else (c, h, w), elem.storage)
    view = ()
    if elem.view:
        strides = np.array(elem.channels_last_strides((c, h, w)) if channels_last else (h * w * es, w * es, es), dtype=np.int64)
        view = (C.c_void_p(strides.ctypes.data),)
    stem, tail = ("spiht_decode_image_host_", ()) if reduce is None else ("spiht_decode_image_reduced_host_", (int(reduce),))
    ctx = _lib.default_context()
    with color_models.fused(ctx, spiht_settings.color_model):  # wrapper:278-279, inside the last level of the inverse transform
        _lib.check(elem.entry(_lib.lib(), stem)(ctx.handle, *args, C.c_void_p(out.ctypes.data), *view, *tail))
    return _crop_window(out, rs, crop, channels_last)


def encode_image_u8(image: np.ndarray, spiht_settings: SpihtSettings = SpihtSettings(), level: Optional[int] = None,
                    max_bits: Optional[int] = None, channels_last: bool = False):
    """8-bit pixels: the EncodingResult of encode_image(image / 255.0, ...), field by field, with the conversion done on the
    device (only the bytes cross the link).  image: uint8 (c, h, w), or (h, w, c) with channels_last -- any strides (an
    RGBA buffer's rgba[..., :3] view goes as it is)."""
    return _encode_image_px(image, spiht_settings, level, max_bits, channels_last, px.U8, "encode_image_u8")


def decode_image_u8(encoding_result: EncodingResult, spiht_settings: SpihtSettings, channels_last: bool = False) -> np.ndarray:
    """8-bit pixels: (np.clip(decode_image(r, s), 0, 1) * 255).astype(np.uint8) cropped to the encoded picture's h x w, with
    the conversion done on the device.  Returns a new uint8 array (c, h, w), or (h, w, c) with channels_last."""
    return _decode_image_px(encoding_result, spiht_settings, px.U8, channels_last)


def encode_image_u16(image: np.ndarray, spiht_settings: SpihtSettings = SpihtSettings(), level: Optional[int] = None,
                     max_bits: Optional[int] = None, channels_last: bool = False):
    """16-bit pixels: the EncodingResult of encode_image(image / 65535.0, ...), field by field, with the conversion done on
    the device (two bytes per sample cross the link).  image: uint16 (c, h, w), or (h, w, c) with channels_last -- any
    non-negative strides (a 16-bit RGBA buffer's rgba[..., :3] view goes as it is); the other byte order is copied."""
    return _encode_image_px(image, spiht_settings, level, max_bits, channels_last, px.U16, "encode_image_u16")


def decode_image_u16(encoding_result: EncodingResult, spiht_settings: SpihtSettings, channels_last: bool = False) -> np.ndarray:
    """16-bit pixels: (np.clip(decode_image(r, s), 0, 1) * 65535).astype(np.uint16) cropped to the encoded picture's h x w,
    with the conversion done on the device.  Returns a new uint16 array (c, h, w), or (h, w, c) with channels_last.  The
    stream may come from any pixel format."""
    return _decode_image_px(encoding_result, spiht_settings, px.U16, channels_last)


def encode_image_float(image: np.ndarray, spiht_settings: SpihtSettings = SpihtSettings(), level: Optional[int] = None,
                       max_bits: Optional[int] = None, dtype=None, channels_last: bool = False):
    """Float pixels in: the EncodingResult of encode_image(floatpx.to_float64(image, kind), ...), field by field -- every
    sample widened EXACTLY to float64 on the device (nothing scaled, nothing clipped, subnormals kept), then the float64
    codec with all it has (colour model, every mode and wavelet) -- so that 4 or 2 bytes per sample cross the link.
    This is NOT encode_image(image): a float32 array given to encode_image keeps the reference's single-precision
    transform; given to this call it is transformed in float64.
    image: float32 or float16 (c, h, w), or (h, w, c) with channels_last -- any non-negative strides (a four-sample buffer's
    [..., :3] view goes as it is; a negative stride or the other byte order is copied first); for bfloat16 the uint16 bit
    patterns with dtype="bfloat16" or torch.bfloat16 (floatpx.kind_arg).  The kind is inferred from a float32 / float16
    array.  Non-finite samples are outside the contract, as they are for encode_image."""
    elem = px.of_kind_id(floatpx.input_kind(image, dtype, "encode_image_float"))
    return _encode_image_px(image, spiht_settings, level, max_bits, channels_last, elem, "encode_image_float")


def decode_image_float(encoding_result: EncodingResult, spiht_settings: SpihtSettings, dtype=np.float32,
                       channels_last: bool = False) -> np.ndarray:
    """Float pixels out: floatpx.convert(decode_image(r, s)[:, :h, :w], dtype) in every bit -- each float64 sample rounded ONCE
    to the kind (nearest, ties to even; no clip, no scale: what lies outside [0, 1] stays, overflow gives inf), cropped to the
    encoded picture's h x w -- with the conversion done on the device, so that 4 or 2 bytes per sample cross the link.
    dtype: np.float32, np.float16, "bfloat16", or a torch dtype (floatpx.kind_arg).  Returns a new array (c, h, w), or
    (h, w, c) with channels_last: float32, float16, or for bfloat16 the uint16 bit patterns (numpy has no such type) --

        torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)

    The stream may come from any pixel format."""
    return _decode_image_px(encoding_result, spiht_settings, px.of_kind(dtype), channels_last)


def reduced_shape(h: int, w: int, spiht_settings: SpihtSettings, level: Optional[int], reduce: int):
    """Sizes of a reduced-resolution decode of an h x w picture coded with `level` levels (None: as encode_image picks
    it), `reduce` pyramid levels below full size (spiht_reduced_shape; no device needed).  Returns a dict:
    level -- the levels L the stream has; rec_h, rec_w -- the float64 picture decode_image_reduced returns; pic_h, pic_w --
    the 8- / 16-bit picture (the band size hs[reduce], ws[reduce]); in_h, in_w -- ceil(h / 2^reduce), ceil(w / 2^reduce),
    the size of the picture downsampled 2^reduce-fold; off_y, off_x -- where that window lies in either picture (crop=True).
    ValueError unless 0 <= reduce <= L."""
    wid, mid = _wavelet_mode_ids(spiht_settings)
    if level is not None and level < 0:
        raise ValueError("Level value of %d is too low . Minimum level is 0." % level)
    g = _geometry(h, w, wid, level, mid)
    reduce = _reduce_arg(reduce, g["level"])
    lv = C.c_int()
    v = [C.c_int64() for _ in range(8)]
    _lib.check(_lib.lib().spiht_reduced_shape(int(h), int(w), wid, mid, -1 if level is None else int(level), reduce,
                                              C.byref(lv), *[C.byref(t) for t in v]))
    names = ("rec_h", "rec_w", "pic_h", "pic_w", "off_y", "off_x", "in_h", "in_w")
    return dict(level=lv.value, **{k: t.value for k, t in zip(names, v)})


def _reduce_arg(reduce, levels):
    if isinstance(reduce, bool) or not isinstance(reduce, (int, np.integer)):
        raise TypeError("reduce must be an integer, not %s" % type(reduce).__name__)
    if not 0 <= reduce <= levels:
        raise ValueError("reduce = %d: a stream of %d levels decodes at reduce 0 .. %d" % (reduce, levels, levels))
    return int(reduce)


def _crop_window(picture, rs, crop, channels_last=False):
    """crop=True: the centred in_h x in_w window of a reduced picture, or of a batch of them (a view)"""
    if not crop:
        return picture
    ys, xs = slice(rs["off_y"], rs["off_y"] + rs["in_h"]), slice(rs["off_x"], rs["off_x"] + rs["in_w"])
    return picture[..., ys, xs, :] if channels_last else picture[..., ys, xs]


def decode_image_reduced(encoding_result: EncodingResult, spiht_settings: SpihtSettings, reduce: int,
                         crop: bool = False) -> np.ndarray:
    """The picture at 1/2^reduce size straight from the stream, 0 <= reduce <= L (the stream's levels; ValueError
    otherwise): levels L .. reduce + 1 of the inverse transform run on the GPU and nothing below, and only the small picture
    comes back.  Returns float64 (c, rec_h, rec_w) (reduced_shape):

        pywt.waverec2(coeffs[:L - reduce + 1], wavelet, mode) * 2 ** -reduce

    of the dequantised coefficients -- PyWavelets' approximation band with the DC gain of 2 per level taken out --,
    uncropped as decode_image's; for reduce == L the root block itself; with a colour model, changed back to RGB per pixel.
    reduce=0 is decode_image(encoding_result, spiht_settings) in every bit.

    The band carries a rim of extension samples (its size is hs[reduce] >= ceil(h / 2^reduce); with bior4.4 the rim
    approaches four samples a side).  crop=True returns the centred ceil(h / 2^reduce) x ceil(w / 2^reduce) window of it, as
    a view: offset (hs[reduce] - ceil(h / 2^reduce)) // 2 per axis, 0 under periodization.  That window is the downsampled
    picture to within a sample: the sampling phase of an even-length filter is not an integer."""
    return _decode_image_px(encoding_result, spiht_settings, px.F64, False, reduce, crop)


def decode_image_reduced_u8(encoding_result: EncodingResult, spiht_settings: SpihtSettings, reduce: int, crop: bool = False,
                            channels_last: bool = False) -> np.ndarray:
    """8-bit pixels at 1/2^reduce size: (np.clip(decode_image_reduced(r, s, reduce), 0, 1) * 255).astype(np.uint8) cropped to
    the band size (c, pic_h, pic_w) (reduced_shape) -- the rule of decode_image_u8 one pyramid level up --, converted on the
    device; (pic_h, pic_w, c) with channels_last.  crop=True: the centred window, as decode_image_reduced."""
    return _decode_image_px(encoding_result, spiht_settings, px.U8, channels_last, reduce, crop)


def decode_image_reduced_u16(encoding_result: EncodingResult, spiht_settings: SpihtSettings, reduce: int, crop: bool = False,
                             channels_last: bool = False) -> np.ndarray:
    """16-bit pixels at 1/2^reduce size: as decode_image_reduced_u8 with 65535 for 255."""
    return _decode_image_px(encoding_result, spiht_settings, px.U16, channels_last, reduce, crop)


def decode_image_reduced_float(encoding_result: EncodingResult, spiht_settings: SpihtSettings, reduce: int, dtype=np.float32,
                               crop: bool = False, channels_last: bool = False) -> np.ndarray:
    """Float pixels at 1/2^reduce size: floatpx.convert(decode_image_reduced(r, s, reduce), dtype) cropped to the band size
    (c, pic_h, pic_w) (reduced_shape), as the integer forms are -- the rule of decode_image_float one pyramid level up --,
    converted on the device; (pic_h, pic_w, c) with channels_last.  crop=True: the centred window, as decode_image_reduced."""
    return _decode_image_px(encoding_result, spiht_settings, px.of_kind(dtype), channels_last, reduce, crop)


def _band_sizes(h, w, wavelet, levels, mode="reflect"):
    """band heights / widths per level, [0] = the image: len' = (len + F - 1) // 2 (pywt.dwt_coeff_len), under periodization
    ceil(len / 2) -- the same rule with a two-tap filter"""
    F = 2 if str(mode) == "periodization" else _filter_len(wavelet)
    hs, ws = [int(h)], [int(w)]
    for _ in range(levels):
        hs.append((hs[-1] + F - 1) // 2)
        ws.append((ws[-1] + F - 1) // 2)
    return hs, ws


def _metadata_boxes(h, w, spiht_settings, g):
    """The boxes of the sub-bands inside the packed array of an h x w picture of geometry g (_geometry), as (start, end)
    pairs per axis: the root block, then per level (coarsest first) the filters in the order the reference hands them
    over, 'da', 'ad', 'dd' (wrapper:240) -> (top_slice, other_slices) of decode_with_metadata.  (The reference reads them
    off pywt's slice objects, whose `start` is None on the approximation side -- which PyO3 refuses, wrapper:242-245; here
    they come from the band sizes, so every start is a number.)"""
    hs, ws = _band_sizes(h, w, spiht_settings.wavelet, g["level"], spiht_settings.mode)
    top_box = [(0, g["ll_h"]), (0, g["ll_w"])]
    level_boxes = []
    row0, col0 = g["ll_h"], g["ll_w"]  # where the detail blocks of the level start
    for lv in range(g["level"], 0, -1):
        rows, cols = (row0, row0 + hs[lv]), (col0, col0 + ws[lv])
        level_boxes.append([[rows, (0, ws[lv])],     # 'da': below the approximation
                            [(0, hs[lv]), cols],     # 'ad': right of it
                            [rows, cols]])           # 'dd': diagonal
        row0, col0 = rows[1], cols[1]
    return top_box, level_boxes


def decode_rec_array(encoding_result: EncodingResult, spiht_settings: SpihtSettings, return_metadata: bool = False):
    """wrapper:218-257: stream -> int32 coefficient array (+ the coder's per-bit metadata)."""
    if encoding_result._encoding_version != ENCODER_DECODER_VERSION:
        raise ValueError(encoding_result._encoding_version)
    er = encoding_result
    wid, mid = _wavelet_mode_ids(spiht_settings)
    g = _geometry(er.h, er.w, wid, er.level, mid)
    slices, enc_h, enc_w = get_slices_and_h_w(er.h, er.w, spiht_settings, er.level)  # (returned to the caller, as the reference does)
    spiht_metadata = None
    if not return_metadata:
        rec_arr = spiht_rs.decode(er.encoded_bytes, er.max_n, er.c, enc_h, enc_w, g["ll_h"], g["ll_w"])
    else:
        top_box, level_boxes = _metadata_boxes(er.h, er.w, spiht_settings, g)
        rec_arr, spiht_metadata = spiht_rs.decode_with_metadata(er.encoded_bytes, er.max_n, er.c, enc_h, enc_w, g["ll_h"],
                                                                g["ll_w"], top_box, level_boxes)
    return dict(rec_arr=rec_arr, slices=slices, spiht_metadata=spiht_metadata, h=er.h, w=er.w, level=er.level)


def decode_from_rec_arr(rec_arr: np.ndarray, h: int, w: int, level, spiht_settings: SpihtSettings, slices=None):
    """wrapper:259-281: (rec / channel_mults) / q -> inverse DWT -> colour back.  Runs on the GPU."""
    wid, mid = _wavelet_mode_ids(spiht_settings)
    g = _geometry(h, w, wid, level, mid)
    rec = np.ascontiguousarray(rec_arr, dtype=np.int32)
    if rec.ndim != 3 or rec.shape[1] != g["enc_h"] or rec.shape[2] != g["enc_w"]:
        raise ValueError("rec_arr shape %s does not match the coefficient array (c,%d,%d)"
                         % (rec.shape, g["enc_h"], g["enc_w"]))
    c = rec.shape[0]
    mults, mults_p = _mults_arg(spiht_settings.per_channel_quant_scales, c)
    ctx = _lib.default_context()
    L = _lib.lib()
    out = _lib.result_array((c, g["rec_h"], g["rec_w"]), np.float64)
    if spiht_settings.color_model is not None and c != 3:
        raise ValueError("colour conversion needs 3 channels")
    with color_models.fused(ctx, spiht_settings.color_model):
        _lib.check(L.spiht_dequant_idwt_host_f64(ctx.handle, C.c_void_p(rec.ctypes.data), c, h, w, wid, mid,
                                                 -1 if level is None else int(level),
                                                 float(spiht_settings.quantization_scale), mults_p, C.c_void_p(out.ctypes.data)))
    return out
