"""Batched, device-resident image codec: the form the throughput metric is measured on.

The reference codes one image per call (spiht_wrapper.encode_image / decode_image).  Here B images of one
geometry are transformed, quantised and coded in one queue of HIP kernels; pixels, coefficient arrays and
bitstreams stay in HBM between the stages.  Device buffers may come from this module (hipMalloc through the
C ABI) or from anyone else (e.g. a torch tensor's data_ptr()) -- the C ABI takes plain pointers.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, color_models, floatpx, px
from . import spiht as spiht_rs
from .spiht_wrapper import (EncodingResult, SpihtSettings, _crop_window, _geometry, _metadata_boxes, _mults_arg,
                            _wavelet_mode_ids, reduced_shape)


class DeviceArray:
    """A hipMalloc'd buffer with a shape and dtype (no arithmetic: storage only)."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.ptr = ctx.alloc(max(self.nbytes, 4))

    def upload(self, arr, offset_bytes=0):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert offset_bytes + arr.nbytes <= self.nbytes
        self.ctx.upload(self.ptr + offset_bytes, arr)

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if out.nbytes:
            self.ctx.download(out, self.ptr)
        return out

    def zero(self):
        self.ctx.memset(self.ptr, 0, self.nbytes)

    def free(self):
        if self.ptr:
            self.ctx.free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BatchCodec:
    """encode/decode B images [B,c,H,W] (float64) at a fixed bit budget.

    settings / level / max_bits have the meaning of spiht_wrapper.encode_image, settings.color_model included: pixels
    go in and come out as RGB, the change to and from the coded colour model happens inside level 1 of the transforms
    (color_models.fused; 3-channel float64 images)."""

    def __init__(self, c, H, W, settings=None, level=None, max_bits=None, ctx=None, pixel_dtype=np.float64):
        # pixel_dtype float32: the encoder side runs PyWavelets' single-precision arithmetic (what the reference does
        # with float32 / float16 pixels); decoded images are float64 either way, as in the reference
        self.pixel_dtype = np.dtype(np.float32 if np.dtype(pixel_dtype) in (np.float32, np.float16) else np.float64)
        self.settings = settings if settings is not None else SpihtSettings()
        self.c, self.H, self.W, self.level = int(c), int(H), int(W), level
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.L = _lib.lib()
        self.wid, self.mid = _wavelet_mode_ids(self.settings)
        self.geom = _geometry(H, W, self.wid, level, self.mid)
        self.max_bits = 99999999999999999 if max_bits is None else int(max_bits)
        self.mults, self._mults_p = _mults_arg(self.settings.per_channel_quant_scales, self.c)
        bound = C.c_uint64()
        _lib.check(self.L.spiht_encode_bound(self.c, self.geom["enc_h"], self.geom["enc_w"], self.geom["ll_h"],
                                             self.geom["ll_w"], 0x3FFFFFFF, self.max_bits, C.byref(bound)))
        self.slot_stride = max(int(bound.value), 4)
        self._lv = -1 if level is None else int(level)
        self._meta_slices = None   # decode_with_metadata_device: the sub-band boxes (host int64 arrays) and their level count
        self._rec_scratch = None   # ... its coefficient arrays when the caller gives none
        if self.settings.color_model not in (None, "RGB"):
            if self.settings.color_model not in color_models.SUPPORTED_MODELS:
                raise ValueError(f'{self.settings.color_model} is not a supported color model. '
                                 f'Supported models are {color_models.SUPPORTED_MODELS}')
            if self.c != 3:
                raise ValueError("colour conversion needs 3 channels")
            if self.pixel_dtype != np.float64:
                raise ValueError("colour conversion on the device takes float64 pixels")

    def _color(self):
        return color_models.fused(self.ctx, self.settings.color_model)

    # ---- raw device-pointer API (ints) -------------------------------------------------------
    # One implementation by the element type (px.Elem); the public names pick it.  The checks of a view -- its strides, its
    # base -- come before anything of the codec but c, H, W is read: they need no context.
    def _encode_device(self, elem, d_img, B, d_out, d_nbits, d_max_n, strides=None, d_coeffs=None):
        view = ()  # the elements that come as a view take the strides behind the address
        if elem.view:
            st, st_p = elem.strides_arg((int(B), self.c, self.H, self.W), strides, False)
            elem.check_aligned(d_img)
            view = (st_p,)
        args = (C.c_void_p(d_img), *view, int(B), self.c, self.H, self.W, self.wid, self.mid, self._lv,
                float(self.settings.quantization_scale), self._mults_p, self.max_bits, C.c_void_p(d_out), self.slot_stride,
                C.c_void_p(d_nbits), C.c_void_p(d_max_n), C.c_void_p(d_coeffs) if d_coeffs else None)
        with self._color():
            _lib.check(elem.entry(self.L, "spiht_encode_image_batch_")(self.ctx.handle, *args))

    def _decode_device(self, elem, d_data, d_nbytes, d_max_n, B, d_img_out, strides=None, d_rec=None, slot_stride=None, reduce=None):
        """reduce=None: the full-size entry point; otherwise the *_reduced_* one, whose pictures are reduced_shape(reduce)'s"""
        stem, h, w, tail = "spiht_decode_image_batch_", self.H, self.W, ()
        if reduce is not None:
            rs = self.reduced_shape(reduce)
            stem, h, w, tail = "spiht_decode_image_reduced_batch_", rs["pic_h"], rs["pic_w"], (int(reduce),)
        view = ()
        if elem.view:
            st, st_p = elem.strides_arg((int(B), self.c, h, w), strides, True)
            elem.check_aligned(d_img_out)
            view = (st_p,)
        args = (C.c_void_p(d_data), self.slot_stride if slot_stride is None else int(slot_stride), C.c_void_p(d_nbytes),
                C.c_void_p(d_max_n), int(B), self.c, self.H, self.W, self.wid, self.mid, self._lv,
                float(self.settings.quantization_scale), self._mults_p, C.c_void_p(d_img_out), *view,
                C.c_void_p(d_rec) if d_rec else None, *tail)
        with self._color():
            _lib.check(elem.entry(self.L, stem)(self.ctx.handle, *args))

    def encode_device(self, d_img, B, d_out, d_nbits, d_max_n, d_coeffs=None):
        self._encode_device(px.of_dtype(self.pixel_dtype), d_img, B, d_out, d_nbits, d_max_n, None, d_coeffs)

    def decode_device(self, d_data, d_nbytes, d_max_n, B, d_img_out, d_rec=None, slot_stride=None):
        self._decode_device(px.F64, d_data, d_nbytes, d_max_n, B, d_img_out, None, d_rec, slot_stride)

    def decode_with_metadata_device(self, d_data, d_nbytes, d_max_n, B, d_meta, meta_rows, d_img_out=None, d_rec=None,
                                    slot_stride=None):
        """decode_image(..., return_metadata=True) of B device-resident streams (the slots, nbytes and max_n of
        encode_device + nbits_to_nbytes): the metadata tables into d_meta, int32 [B, meta_rows, 8] with meta_rows >=
        8 * slot_stride + 1 (image b's rows past 8 * nbytes[b] + 1 are zero); the decoded coefficient arrays into d_rec
        (int32 [B, c, enc_h, enc_w]) when given, and the pictures, float64 [B, c, H', W'], into d_img_out when given.
        Queued on the codec's context (spiht_decode_with_metadata_batch_i32, then spiht_dequant_idwt_batch_f64)."""
        g = self.geom
        B = int(B)
        if self._meta_slices is None:
            top, other = _metadata_boxes(self.H, self.W, self.settings, g)
            self._meta_slices = spiht_rs._metadata_args(self.c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"], top, other)[5:]
        topv, oth, level = self._meta_slices
        rec = d_rec
        if rec is None and d_img_out is not None:
            need = B * self.c * g["enc_h"] * g["enc_w"] * 4
            if self._rec_scratch is None or self._rec_scratch.nbytes < need:
                if self._rec_scratch is not None:
                    self._rec_scratch.free()
                self._rec_scratch = DeviceArray(self.ctx, (B, self.c, g["enc_h"], g["enc_w"]), np.int32)
            rec = self._rec_scratch.ptr
        _lib.check(self.L.spiht_decode_with_metadata_batch_i32(
            self.ctx.handle, C.c_void_p(d_data), self.slot_stride if slot_stride is None else int(slot_stride),
            C.c_void_p(d_nbytes), C.c_void_p(d_max_n), B, self.c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"],
            C.c_void_p(topv.ctypes.data), C.c_void_p(oth.ctypes.data), level, C.c_void_p(rec) if rec else None,
            C.c_void_p(d_meta), int(meta_rows)))
        if d_img_out is not None and B > 0:
            with self._color():
                _lib.check(self.L.spiht_dequant_idwt_batch_f64(
                    self.ctx.handle, C.c_void_p(rec), B, self.c, self.H, self.W, self.wid, self.mid, self._lv,
                    float(self.settings.quantization_scale), self._mults_p, C.c_void_p(d_img_out)))

    # ---- 8- and 16-bit pixels (include/spiht_hip.h, *_u8 / *_u16): whatever pixel_dtype says, the float64 arithmetic on
    # k / 255 (k / 65535).  One implementation by the element type; the public names pick it. -------------------------------
    def _encode_pixels(self, elem, name, images, channels_last):
        """host pictures [B, c, H, W] (or [B, H, W, c]) of a view element -> EncodingResults"""
        images = np.asarray(images)
        if not px._is_dtype(images, elem.storage) or images.ndim != 4:
            raise ValueError("%s takes a %s array [B, c, H, W]" % (name, elem.storage.name))
        if channels_last:
            images = images.transpose(0, 3, 1, 2)
        images = np.ascontiguousarray(images, dtype=elem.storage)
        if images.shape[1:] != (self.c, self.H, self.W):
            raise ValueError("%s: pictures of shape %s, the codec's are %s" % (name, images.shape[1:], (self.c, self.H, self.W)))
        return self._encode_host(elem, images)

    def _decode_pixels(self, elem, results, channels_last=False, reduce=None, crop=False):
        """EncodingResults -> host pictures [B, c, h, w] (or [B, h, w, c]) of the element: the uncropped float64 ones, or a view
        element's, cropped to the picture (reduce: to the band); crop: the centred window of a reduced decode"""
        rs = None if reduce is None else self.reduced_shape(reduce)
        if not elem.view:
            g = self.geom if rs is None else rs
            h, w = g["rec_h"], g["rec_w"]
        else:
            h, w = (self.H, self.W) if rs is None else (rs["pic_h"], rs["pic_w"])
        shape = (len(results), self.c, h, w)
        out = self._decode_host(elem, results, (h, w, self.c) if channels_last else shape[1:],
                                elem.channels_last_strides(shape) if channels_last else None, reduce)
        return _crop_window(out, rs, crop, channels_last)

    def encode_device_u8(self, d_img, B, d_out, d_nbits, d_max_n, strides=None):
        """d_img: uint8 [B, c, H, W] on the device, laid out by `strides` (bytes; None: dense CHW)"""
        self._encode_device(px.U8, d_img, B, d_out, d_nbits, d_max_n, strides)

    def decode_device_u8(self, d_data, d_nbytes, d_max_n, B, d_img_out, strides=None, d_rec=None, slot_stride=None):
        """-> uint8 [B, c, H, W] on the device, cropped to H x W, laid out by `strides` (bytes; None: dense CHW; the bytes
        between the view's elements -- an RGBA buffer's alpha, row padding -- are not written)"""
        self._decode_device(px.U8, d_data, d_nbytes, d_max_n, B, d_img_out, strides, d_rec, slot_stride)

    def encode_u8(self, images, channels_last=False):
        """images: uint8 [B, c, H, W] (or [B, H, W, c] with channels_last) -> list of EncodingResult (those of
        encode(images / 255.0))"""
        return self._encode_pixels(px.U8, "encode_u8", images, channels_last)

    def decode_u8(self, results, channels_last=False):
        """list of EncodingResult (same geometry) -> uint8 [B, c, H, W] (or [B, H, W, c]), cropped to H x W"""
        return self._decode_pixels(px.U8, results, channels_last)

    def encode_device_u16(self, d_img, B, d_out, d_nbits, d_max_n, strides=None):
        """d_img: uint16 [B, c, H, W] on the device (native byte order, even address), laid out by `strides` (BYTES, all
        even; None: dense CHW)"""
        self._encode_device(px.U16, d_img, B, d_out, d_nbits, d_max_n, strides)

    def decode_device_u16(self, d_data, d_nbytes, d_max_n, B, d_img_out, strides=None, d_rec=None, slot_stride=None):
        """-> uint16 [B, c, H, W] on the device, cropped to H x W, laid out by `strides` (BYTES, all even; None: dense CHW;
        what lies between the view's elements -- a 16-bit RGBA buffer's alpha, row padding -- is not written)"""
        self._decode_device(px.U16, d_data, d_nbytes, d_max_n, B, d_img_out, strides, d_rec, slot_stride)

    def encode_u16(self, images, channels_last=False):
        """images: uint16 [B, c, H, W] (or [B, H, W, c] with channels_last) -> list of EncodingResult (those of
        encode(images / 65535.0))"""
        return self._encode_pixels(px.U16, "encode_u16", images, channels_last)

    def decode_u16(self, results, channels_last=False):
        """list of EncodingResult (same geometry) -> uint16 [B, c, H, W] (or [B, H, W, c]), cropped to H x W"""
        return self._decode_pixels(px.U16, results, channels_last)

    # ---- float pixels out (include/spiht_hip.h, *_flt; spiht_amd/floatpx.py): float32, float16 or bfloat16 pictures, each
    # sample of the float64 decode rounded once to the kind.  dtype: what floatpx.kind_arg takes. -----------------------------
    def decode_device_float(self, d_data, d_nbytes, d_max_n, B, d_img_out, dtype, strides=None, d_rec=None, slot_stride=None):
        """-> pictures of the kind `dtype` [B, c, H, W] on the device, cropped to H x W: floatpx.convert of what decode_device
        makes, laid out by `strides` (BYTES, multiples of the element size, as the base; None: dense CHW; what lies between the
        view's elements -- a fourth channel, row padding -- is not written)"""
        self._decode_device(px.of_kind_id(dtype), d_data, d_nbytes, d_max_n, B, d_img_out, strides, d_rec, slot_stride)

    def decode_float(self, results, dtype=np.float32, channels_last=False):
        """list of EncodingResult (same geometry) -> [B, c, H, W] (or [B, H, W, c]) of the kind `dtype`, cropped to H x W:
        spiht_wrapper.decode_image_float of each (float32, float16, or uint16 bit patterns for bfloat16)"""
        return self._decode_pixels(px.of_kind(dtype), results, channels_last)

    def decode_reduced_device_float(self, d_data, d_nbytes, d_max_n, B, d_img_out, reduce, dtype, strides=None, d_rec=None,
                                    slot_stride=None):
        """-> pictures of the kind `dtype` [B, c, pic_h, pic_w] on the device (reduced_shape), laid out by `strides` (BYTES,
        multiples of the element size; None: dense CHW): floatpx.convert of decode_reduced_device's, cropped to the band"""
        self._decode_device(px.of_kind_id(dtype), d_data, d_nbytes, d_max_n, B, d_img_out, strides, d_rec, slot_stride, reduce)

    def decode_reduced_float(self, results, reduce, dtype=np.float32, crop=False, channels_last=False):
        """list of EncodingResult -> [B, c, pic_h, pic_w] (or [B, pic_h, pic_w, c]) of the kind `dtype`:
        decode_image_reduced_float of each"""
        return self._decode_pixels(px.of_kind(dtype), results, channels_last, reduce, crop)

    # ---- float pixels in (include/spiht_hip.h, the encode side of *_flt): float32, float16 or bfloat16 pictures, each sample
    # widened exactly on the loads of level 1; whatever pixel_dtype says, the float64 arithmetic -- what encode() of a float64
    # codec gives for floatpx.to_float64 of the pictures.  NOT the single-precision transform of a pixel_dtype=float32 codec.
    def encode_device_float(self, d_img, B, d_out, d_nbits, d_max_n, dtype, strides=None, d_coeffs=None):
        """d_img: pictures of the kind `dtype` [B, c, H, W] on the device, laid out by `strides` (BYTES, non-negative multiples
        of the element size, as the base; None: dense CHW)"""
        self._encode_device(px.of_kind_id(dtype), d_img, B, d_out, d_nbits, d_max_n, strides, d_coeffs)

    def encode_float(self, images, dtype=None, channels_last=False):
        """images: [B, c, H, W] (or [B, H, W, c] with channels_last) float32 or float16, or uint16 bit patterns with
        dtype="bfloat16" -> list of EncodingResult: spiht_wrapper.encode_image_float of each"""
        images = np.asarray(images)
        elem = px.of_kind_id(floatpx.input_kind(images, dtype, "encode_float"))
        return self._encode_pixels(elem, "encode_float", images, channels_last)

    # ---- reduced-resolution decode (include/spiht_hip.h, *_reduced_*): pictures at 1/2^reduce size, 0 <= reduce <= L.
    # What spiht_wrapper.decode_image_reduced* return, for B streams in one queue of kernels. ------------------------------
    def reduced_shape(self, reduce):
        """spiht_wrapper.reduced_shape of the codec's pictures"""
        return reduced_shape(self.H, self.W, self.settings, self.level, reduce)

    def decode_reduced_device(self, d_data, d_nbytes, d_max_n, B, d_img_out, reduce, d_rec=None, slot_stride=None):
        """decode_device at 1/2^reduce size -> float64 [B, c, rec_h, rec_w] on the device (reduced_shape)"""
        self._decode_device(px.F64, d_data, d_nbytes, d_max_n, B, d_img_out, None, d_rec, slot_stride, reduce)

    def decode_reduced_device_u8(self, d_data, d_nbytes, d_max_n, B, d_img_out, reduce, strides=None, d_rec=None,
                                 slot_stride=None):
        """-> uint8 [B, c, pic_h, pic_w] on the device (reduced_shape), laid out by `strides` (bytes; None: dense CHW; what
        lies between the view's elements is not written)"""
        self._decode_device(px.U8, d_data, d_nbytes, d_max_n, B, d_img_out, strides, d_rec, slot_stride, reduce)

    def decode_reduced_device_u16(self, d_data, d_nbytes, d_max_n, B, d_img_out, reduce, strides=None, d_rec=None,
                                  slot_stride=None):
        """-> uint16 [B, c, pic_h, pic_w] on the device, laid out by `strides` (BYTES, all even; None: dense CHW)"""
        self._decode_device(px.U16, d_data, d_nbytes, d_max_n, B, d_img_out, strides, d_rec, slot_stride, reduce)

    def decode_reduced(self, results, reduce, crop=False):
        """list of EncodingResult (same geometry) -> float64 [B, c, rec_h, rec_w]: decode_image_reduced of each; crop=True:
        the centred in_h x in_w window (a view)"""
        return self._decode_pixels(px.F64, results, False, reduce, crop)

    def decode_reduced_u8(self, results, reduce, crop=False, channels_last=False):
        """list of EncodingResult -> uint8 [B, c, pic_h, pic_w] (or [B, pic_h, pic_w, c]): decode_image_reduced_u8 of each"""
        return self._decode_pixels(px.U8, results, channels_last, reduce, crop)

    def decode_reduced_u16(self, results, reduce, crop=False, channels_last=False):
        """list of EncodingResult -> uint16 [B, c, pic_h, pic_w] (or [B, pic_h, pic_w, c]): decode_image_reduced_u16 of each"""
        return self._decode_pixels(px.U16, results, channels_last, reduce, crop)

    # ---- rate-distortion curve and cut (spiht_amd/rd.py; include/spiht_hip.h: spiht_sqerr_i32, spiht_sse_*) ---------------
    def rd_curve(self, image, result=None, byte_lengths=None, points=32, max_bytes=2 ** 31):
        """How good the prefixes of one stream are -> rd.RDCurve, rows in the order of byte_lengths.  image: one float
        picture (c, H, W) of the codec's geometry.  result: a stream of it (X, the array the coefficient error is taken
        against, is then the forward transform of `image` with the codec's settings); None: the picture is encoded first,
        with the codec's max_bits, and X is the encoder's own quantised array.  byte_lengths: prefix lengths (None: `points`
        lengths evenly spaced over 1 .. len(stream), the full length among them); a length past the end means the whole
        stream, as in decode_prefixes.
        Everything stays in HBM: the picture goes up once; per group of lengths the stream is walked once
        (spiht_decode_budgets_dev_i32), the arrays are compared (spiht_sqerr_i32), inverse-transformed in one batched launch
        and compared with the picture (spiht_sse_f64); the K rows come back.  A group holds as many lengths as keep
        K_g c (enc_h enc_w 4 + rec_h rec_w 8) bytes within max_bytes, at least one; the numbers do not depend on it."""
        from . import rd
        return rd.codec_rd_curve(self, image, result, byte_lengths, points, max_bytes, px.F64)[0]

    def rd_curve_u8(self, image, result=None, byte_lengths=None, points=32, max_bytes=2 ** 31):
        """rd_curve of a uint8 picture (c, H, W): the distances are those between 8-bit pictures (decode_image_u8 of the
        prefix against `image`), exact integers; peak 255"""
        from . import rd
        return rd.codec_rd_curve(self, image, result, byte_lengths, points, max_bytes, px.U8)[0]

    def rd_curve_u16(self, image, result=None, byte_lengths=None, points=32, max_bytes=2 ** 31):
        """rd_curve of a uint16 picture (c, H, W); peak 65535"""
        from . import rd
        return rd.codec_rd_curve(self, image, result, byte_lengths, points, max_bytes, px.U16)[0]

    def _cut_to_psnr(self, image, result, target_db, points, elem):
        from . import rd
        target = rd._target_arg(target_db, "target_db")
        return rd.codec_cut(self, image, result, points, elem, "psnr", lambda v: v >= target)

    def cut_to_psnr(self, image, result, target_db, points=32):
        """A prefix of `result` (a stream of the float picture `image`) that reaches target_db -> (EncodingResult, psnr, met).
        If the whole stream stays below the target: the whole stream, met False.  Otherwise the returned length L satisfies
        psnr(L) >= target_db and (L == 0 or psnr(L - 1) < target_db).  That is a crossing, not the shortest such prefix
        there is: PSNR over prefixes need not be monotone (the filters are biorthogonal, the integer formats clip), and the
        search -- at most `points` lengths per round, evenly spaced between a length that fails and one that passes, one
        rd_curve call per round, at most ceil(log(n + 1) / log(points + 1)) rounds after the look at the whole stream --
        ends at one place where the curve crosses the target."""
        return self._cut_to_psnr(image, result, target_db, points, px.F64)

    def cut_to_psnr_u8(self, image, result, target_db, points=32):
        """cut_to_psnr on the 8-bit curve (rd_curve_u8)"""
        return self._cut_to_psnr(image, result, target_db, points, px.U8)

    def cut_to_psnr_u16(self, image, result, target_db, points=32):
        """cut_to_psnr on the 16-bit curve (rd_curve_u16)"""
        return self._cut_to_psnr(image, result, target_db, points, px.U16)

    def cut_to_sqerr(self, image, result, max_sqerr, points=32):
        """A prefix of `result` whose coefficient error E = sum (X - X_L)^2 is at most max_sqerr -> (EncodingResult, E, met);
        the whole stream with met False when even that is above it.  The arithmetic is exact (128-bit sums, Python ints),
        and the returned length L satisfies E(L) <= max_sqerr and (L == 0 or E(L - 1) > max_sqerr).  Where E does not
        increase with the length that is the shortest such prefix.  E falls almost everywhere, but not everywhere: the
        decoder puts a coefficient found significant at plane n at 1.5 * 2^n, and a first refinement bit of 0 moves it to
        2^n -- away from a true value above 1.25 * 2^n -- so a prefix that ends in a refinement pass can be a little worse
        than the one a byte shorter (the CPU oracle shows 32 such steps among the 3521 prefixes of one 37 x 53 test
        picture's full stream).  A target inside such a step gets a crossing, as in cut_to_psnr."""
        from . import rd
        if isinstance(max_sqerr, float) and math.isnan(max_sqerr):
            raise ValueError("max_sqerr is NaN")
        return rd.codec_cut(self, image, result, points, px.F64, "coef_sqerr", lambda v: v <= max_sqerr)

    def nbits_to_nbytes(self, d_nbits, B, d_nbytes):
        _lib.check(self.L.spiht_nbits_to_nbytes(self.ctx.handle, C.c_void_p(d_nbits), int(B), C.c_void_p(d_nbytes)))

    # ---- host convenience ---------------------------------------------------------------------
    def encode(self, images):
        """images: float array [B,c,H,W] -> list of EncodingResult"""
        images = np.ascontiguousarray(images, dtype=self.pixel_dtype)
        assert images.shape[1:] == (self.c, self.H, self.W)
        return self._encode_host(px.of_dtype(self.pixel_dtype), images)

    def decode(self, results):
        """list of EncodingResult (same geometry) -> float64 [B,c,H',W']"""
        return self._decode_pixels(px.F64, results)

    def decode_with_metadata(self, results):
        """list of EncodingResult (same geometry) -> (float64 [B,c,H',W'], [metadata_b]): the pictures of decode(results)
        and, per stream, the table decode_image(results[b], settings, return_metadata=True) returns, int32
        (8 * len(results[b].encoded_bytes) + 1, 8) -- from one batched call"""
        B = len(results)
        g = self.geom
        if B == 0:
            return np.zeros((0, self.c, g["rec_h"], g["rec_w"])), []
        stride, d_in = self._streams_on_device(results)
        meta_rows = 8 * stride + 1
        d_img = DeviceArray(self.ctx, (B, self.c, g["rec_h"], g["rec_w"]), np.float64)
        d_meta = DeviceArray(self.ctx, (B, meta_rows, 8), np.int32)
        try:
            self.decode_with_metadata_device(*(d.ptr for d in d_in), B, d_meta.ptr, meta_rows, d_img_out=d_img.ptr,
                                             slot_stride=stride)
            self.ctx.synchronize()
            images, meta = d_img.download(), d_meta.download()
        finally:
            for d in d_in + (d_img, d_meta):
                d.free()
        return images, [meta[b, :8 * len(r.encoded_bytes) + 1] for b, r in enumerate(results)]

    def _encode_host(self, elem, images):
        """host pictures [B, c, H, W] of the element, dense -> their device copy -> _encode_device -> EncodingResults"""
        B = images.shape[0]
        ctx = self.ctx
        d_img = DeviceArray(ctx, images.shape, images.dtype)
        d_out = DeviceArray(ctx, (B, self.slot_stride), np.uint8)
        d_nbits = DeviceArray(ctx, (B,), np.uint64)
        d_maxn = DeviceArray(ctx, (B,), np.uint8)
        try:
            d_img.upload(images)
            self._encode_device(elem, d_img.ptr, B, d_out.ptr, d_nbits.ptr, d_maxn.ptr)
            ctx.synchronize()
            out, nbits, maxn = d_out.download(), d_nbits.download(), d_maxn.download()
        finally:
            for d in (d_img, d_out, d_nbits, d_maxn):
                d.free()
        return [EncodingResult(out[b, :(int(nbits[b]) + 7) // 8].tobytes(), self.H, self.W, self.c, int(maxn[b]),
                               self.level) for b in range(B)]

    def _decode_host(self, elem, results, shape, strides, reduce):
        """the streams of `results` on the device, in slots of the longest one's size -> _decode_device into pictures of the
        element, `shape` each as the host sees them, laid out by `strides` -> host array [B, *shape]"""
        B = len(results)
        stride, (d_data, d_nbytes, d_maxn) = self._streams_on_device(results)
        d_img = DeviceArray(self.ctx, (B,) + tuple(shape), elem.storage)
        try:
            self._decode_device(elem, d_data.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_img.ptr, strides, None, stride, reduce)
            self.ctx.synchronize()
            return d_img.download()
        finally:
            for d in (d_data, d_nbytes, d_maxn, d_img):
                d.free()

    def _streams_on_device(self, results):
        """the streams of `results` on the device, in slots of the longest one's size -> (slot_stride, (d_data, d_nbytes,
        d_max_n)) -- DeviceArrays the caller frees"""
        B = len(results)
        stride = max(4, (max(len(r.encoded_bytes) for r in results) + 3) & ~3)
        data = np.zeros((B, stride), dtype=np.uint8)
        for b, r in enumerate(results):
            data[b, :len(r.encoded_bytes)] = np.frombuffer(r.encoded_bytes, np.uint8)
        d = (DeviceArray(self.ctx, data.shape, np.uint8), DeviceArray(self.ctx, (B,), np.uint64),
             DeviceArray(self.ctx, (B,), np.uint8))
        d[0].upload(data)
        d[1].upload(np.array([len(r.encoded_bytes) for r in results], dtype=np.uint64))
        d[2].upload(np.array([r.max_n for r in results], dtype=np.uint8))
        return stride, d

    def decode_prefixes(self, result, byte_lengths, one_walk=True, reduce=0):
        """Progressive decoding (the pattern of the reference's make_gif.py:46-61): the pictures of the
        prefixes `result.encoded_bytes[:k]` for every k in byte_lengths -> float64 [K,c,H',W'] (in the order given).
        one_walk (default): the stream is walked ONCE, to the longest prefix, and every tree node replays its operations
        into the K coefficient arrays (spiht_decode_budgets_dev_i32); then one batched inverse transform.
        one_walk=False: K streams in one batch, every prefix decoded by its own workgroup (K walks on K CUs).
        reduce: the pictures at 1/2^reduce size (decode_reduced: float64 [K,c,rec_h,rec_w]) -- preview frames at thumbnail
        size; the walk is the same, the inverse transform of the K arrays stops `reduce` levels early."""
        lens = [int(k) for k in byte_lengths]
        rs = self.reduced_shape(reduce) if reduce else None
        if not one_walk or not lens:
            pre = [EncodingResult(result.encoded_bytes[:k], result.h, result.w, result.c, result.max_n, result.level) for k in lens]
            if reduce:
                return self.decode_reduced(pre, reduce) if pre else np.zeros((0, self.c, rs["rec_h"], rs["rec_w"]))
            return self.decode(pre)
        g = self.geom
        K = len(lens)
        order = np.argsort(np.asarray(lens), kind="stable")
        total = len(result.encoded_bytes)
        bud = np.ascontiguousarray([8 * min(lens[i], total) for i in order], dtype=np.uint64)
        data = np.frombuffer(result.encoded_bytes[:max(min(k, total) for k in lens)], dtype=np.uint8)
        d_rec = DeviceArray(self.ctx, (K, self.c, g["enc_h"], g["enc_w"]), np.int32)
        d_img = DeviceArray(self.ctx, (K, self.c) + ((rs["rec_h"], rs["rec_w"]) if reduce else (g["rec_h"], g["rec_w"])), np.float64)
        try:
            _lib.check(self.L.spiht_decode_budgets_dev_i32(
                self.ctx.handle, C.c_void_p(data.ctypes.data if data.size else 0), data.size, int(result.max_n), self.c,
                g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"], C.c_void_p(bud.ctypes.data), K, C.c_void_p(d_rec.ptr)))
            idwt_args = (self.ctx.handle, C.c_void_p(d_rec.ptr), K, self.c, self.H, self.W, self.wid, self.mid, self._lv,
                         float(self.settings.quantization_scale), self._mults_p, C.c_void_p(d_img.ptr))
            with self._color():
                if reduce:
                    _lib.check(self.L.spiht_dequant_idwt_reduced_batch_f64(*idwt_args, int(reduce)))
                else:
                    _lib.check(self.L.spiht_dequant_idwt_batch_f64(*idwt_args))
            self.ctx.synchronize()
            out = d_img.download()
        finally:
            d_rec.free()
            d_img.free()
        inv = np.empty(K, dtype=np.int64)
        inv[order] = np.arange(K)
        return out[inv]


class Pipeline:
    """The pipelined round trip as the C ABI offers it (include/spiht_hip.h: spiht_pipeline_*, csrc/pipeline.cpp): consecutive
    batches software-pipelined over three contexts -- the HBM-bound passes (transform + pyramid of step i+1, inverse transform
    of step i-1) on one, the list coding of step i on the two others in turn --, queued by the library itself: what a caller
    in any host language gets, and what bench.py times.  `codec` gives geometry and settings; its context runs the HBM-bound
    passes unless own_context is set."""

    def __init__(self, codec, B, own_context=False):
        """own_context: the HBM-bound passes on a context of the pipeline's own instead of the codec's (one more HIP stream;
        a process has few hardware queues for them)"""
        self.codec, self.B = codec, int(B)
        self.L = codec.L
        h = C.c_void_p()
        args = (codec.ctx.device, self.B, codec.c, codec.H, codec.W, codec.wid, codec.mid, codec._lv,
                float(codec.settings.quantization_scale), codec._mults_p, 0 if codec.max_bits >= 2 ** 63 else codec.max_bits, C.byref(h))
        if own_context:
            _lib.check(self.L.spiht_pipeline_create(*args))
        else:
            _lib.check(self.L.spiht_pipeline_create_on(codec.ctx.handle, *args))
        self.handle = h
        ss = C.c_uint64()
        _lib.check(self.L.spiht_pipeline_info(self.handle, C.byref(ss), None, None))
        assert ss.value == codec.slot_stride or codec.max_bits >= 2 ** 63, (ss.value, codec.slot_stride)
        self.slot_stride = int(ss.value)
        cm = codec.settings.color_model
        if cm not in (None, "RGB"):
            Af, Mf, pf = color_models._params("RGB", cm)
            Ai, Mi, pi = color_models._params(cm, "RGB")
            vp = C.c_void_p
            _lib.check(self.L.spiht_pipeline_set_color3(self.handle, vp(Af.ctypes.data), vp(Mf.ctypes.data), pf, vp(Ai.ctypes.data),
                                                        vp(Mi.ctypes.data), pi))

    def contexts(self):
        """[H, L0, L1] as borrowed Context objects (stage timing)"""
        hs = [C.c_void_p() for _ in range(3)]
        _lib.check(self.L.spiht_pipeline_contexts(self.handle, *[C.byref(x) for x in hs]))
        return [_lib.Context.borrowed(x, self.codec.ctx.device) for x in hs]

    def submit(self, d_img, d_out, d_nbits, d_max_n, d_img_out, comm=None, gathered=None, rank=0):
        """queue one step (device pointers as ints).  comm + gathered = (d_all_slots, d_all_nbits, d_all_max_n): the streams are
        all-gathered between encoder and decoder and the decoder reads this rank's rows of the gathered buffers"""
        vp = C.c_void_p
        if comm is None:
            _lib.check(self.L.spiht_pipeline_submit(self.handle, vp(d_img), vp(d_out), vp(d_nbits), vp(d_max_n), vp(d_img_out)))
        else:
            _lib.check(self.L.spiht_pipeline_submit_gather(self.handle, vp(d_img), vp(d_out), vp(d_nbits), vp(d_max_n), vp(d_img_out),
                                                           comm.handle, vp(gathered[0]), vp(gathered[1]), vp(gathered[2]), int(rank)))

    def _submit(self, elem, d_img, d_out, d_nbits, d_max_n, d_img_out, in_strides, out_strides):
        vp = C.c_void_p
        shape = (int(self.B), self.codec.c, self.codec.H, self.codec.W)
        st_in, p_in = elem.strides_arg(shape, in_strides, False)
        st_out, p_out = elem.strides_arg(shape, out_strides, True)
        elem.check_aligned(d_img)
        elem.check_aligned(d_img_out)
        _lib.check(elem.entry(self.L, "spiht_pipeline_submit_")(self.handle, vp(d_img), p_in, vp(d_out), vp(d_nbits), vp(d_max_n),
                                                                vp(d_img_out), p_out))

    def submit_u8(self, d_img, d_out, d_nbits, d_max_n, d_img_out, in_strides=None, out_strides=None):
        """queue one step of 8-bit pictures (device pointers as ints): uint8 [B, c, H, W] in and out, laid out by byte strides
        (None: dense CHW), the output cropped to H x W.  Float64, 8-bit and 16-bit steps may alternate."""
        self._submit(px.U8, d_img, d_out, d_nbits, d_max_n, d_img_out, in_strides, out_strides)

    def submit_u16(self, d_img, d_out, d_nbits, d_max_n, d_img_out, in_strides=None, out_strides=None):
        """queue one step of 16-bit pictures (device pointers as ints): uint16 [B, c, H, W] in and out, laid out by BYTE
        strides (all even; None: dense CHW), the output cropped to H x W."""
        self._submit(px.U16, d_img, d_out, d_nbits, d_max_n, d_img_out, in_strides, out_strides)

    def flush(self):
        _lib.check(self.L.spiht_pipeline_flush(self.handle))

    def synchronize(self):
        _lib.check(self.L.spiht_pipeline_synchronize(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.L.spiht_pipeline_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
