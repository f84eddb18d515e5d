"""What a pixel is, once: the element type behind the per-type calls of batch.py, spiht_wrapper.py, tiles.py, rd.py and
hoststream.py, as a `Pic` of the C side carries its element (csrc/api_internal.h).

There are seven: F64 and F32, the codec's own float pixels (dense; F32 follows PyWavelets' single-precision arithmetic); U8 and
U16 (views by byte strides, k / 255 and k / 65535 in float64); and the three float kinds of floatpx (views by byte strides, each
sample widened exactly to float64 or rounded once from it).  float32 is there twice on purpose: F32 is `pixel_dtype=float32`
and reaches the *_f32 calls, the kind float32 reaches the *_flt calls -- of_dtype gives the one, of_kind the other.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib, floatpx


@dataclass(frozen=True)
class Elem:
    name: str                # "f64", "f32", "u8", "u16", or the kind's: "float32", "float16", "bfloat16"
    storage: np.dtype        # the numpy dtype its pictures come in (bfloat16: uint16 bit patterns)
    suffix: str              # of its entry points: f64, f32, u8, u16, flt
    kind: Optional[int]      # the floatpx id of a float kind -- the argument behind the context of a *_flt call --, else None
    stream_id: Optional[int]  # the element of the spiht_hstream_* calls (F32 has none)

    @property
    def itemsize(self):
        return self.storage.itemsize

    @property
    def integer(self):
        return self.storage.kind == "u" and self.kind is None

    @property
    def peak(self):
        """the largest pixel value: of 8- and 16-bit pixels the type's, of float pixels 1.0"""
        return float(np.iinfo(self.storage).max) if self.integer else 1.0

    @property
    def view(self):
        """its calls take a view of the pictures: a strides argument behind the address"""
        return self.suffix not in ("f64", "f32")

    def entry(self, L, stem):
        """the library's entry point of that stem, a callable taking (ctx_handle, *args): (L, "spiht_decode_image_batch_") ->
        L.spiht_decode_image_batch_u16; for a kind the *_flt call with the kind behind the context"""
        fn = getattr(L, stem + self.suffix)
        if self.kind is None:
            return fn
        return lambda ctx, *args: fn(ctx, self.kind, *args)

    def check_view(self, shape, strides, output):
        """the library's rule for a view of this element (check_u8_view / check_u16_view / floatpx.check_float_view)"""
        if self.kind is not None:
            floatpx.check_float_view(self.kind, shape, strides, output)
        else:
            _check_int_view(8 * self.itemsize, shape, strides, output)

    def strides_arg(self, shape, strides, output):
        """byte strides of a view of `shape`, checked -> (the int64 array, kept by the caller until the call, its c_void_p);
        None (dense CHW): (None, None)"""
        if strides is None:
            return None, None
        st = np.ascontiguousarray([int(x) for x in strides], dtype=np.int64)
        self.check_view(shape, st, output)
        return st, C.c_void_p(st.ctypes.data)

    def check_aligned(self, ptr):
        _check_aligned(ptr, self.storage)

    def channels_last_strides(self, shape):
        """dense byte strides of the view (c, h, w) of a picture stored (h, w, c), or (B, c, h, w) of a batch (B, h, w, c)"""
        c, h, w = shape[-3:]
        es = self.itemsize
        return (es, w * c * es, c * es) if len(shape) == 3 else (h * w * c * es, es, w * c * es, c * es)


_lib.lib()  # (ENUMS is the header's, read with the library)
F64 = Elem("f64", np.dtype(np.float64), "f64", None, _lib.ENUMS["SPIHT_HS_F64"])
F32 = Elem("f32", np.dtype(np.float32), "f32", None, None)
U8 = Elem("u8", np.dtype(np.uint8), "u8", None, _lib.ENUMS["SPIHT_HS_U8"])
U16 = Elem("u16", np.dtype(np.uint16), "u16", None, _lib.ENUMS["SPIHT_HS_U16"])
_KINDS = {k: Elem(floatpx.kind_name(k), floatpx.storage_dtype(k), "flt", k, _lib.ENUMS["SPIHT_HS_" + hs])
          for k, hs in zip(floatpx.KINDS, ("FLT32", "FLT16", "BF16"))}
_BY_DTYPE = {e.storage: e for e in (F64, F32, U8, U16)}


def of_dtype(dtype):
    """np.float64, np.float32, np.uint8 or np.uint16 -> F64, F32, U8, U16; an Elem as it is"""
    if isinstance(dtype, Elem):
        return dtype
    try:
        return _BY_DTYPE[np.dtype(dtype)]
    except KeyError:
        raise ValueError("%s pictures: the pixel types are float64, float32, uint8, uint16 and the float kinds" % np.dtype(dtype).name) from None


def of_kind(dtype):
    """what floatpx.kind_arg takes -> the Elem of the float kind"""
    return _KINDS[floatpx.kind_arg(dtype)]


def of_kind_id(kind):
    """what floatpx.kind_id takes (a kind id as it is) -> the Elem of the float kind"""
    return _KINDS[floatpx.kind_id(kind)]


# ---- the rules of an integer view and of a base address, by dtype (spiht_wrapper re-exports them) ------------------------------
def _check_int_view(bits, shape, strides, output):
    """check_u8_view / check_u16_view: `bits` 8 or 16"""
    shape, strides = [int(x) for x in shape], [int(x) for x in strides]
    if len(shape) != len(strides) or len(shape) not in (3, 4):
        raise ValueError("%d strides for a %d-dimensional picture" % (len(strides), len(shape)))
    if len(shape) == 3:
        shape, strides = [1] + shape, [0] + strides
    if min(shape) < 1:
        raise ValueError("empty %d-bit picture %s" % (bits, shape))
    st = np.ascontiguousarray(strides, dtype=np.int64)
    fn = _lib.lib().spiht_check_view_u16 if bits == 16 else _lib.lib().spiht_check_view_u8
    if fn(shape[0], shape[1], shape[2], shape[3], C.c_void_p(st.ctypes.data), int(bool(output))):
        raise ValueError("the strides %s of the %d-bit %s %s are not supported (negative%s%s)"
                         % (strides, bits, "output" if output else "input", shape, ", odd" if bits == 16 else "",
                            ", or overlapping" if output else ""))


def _check_aligned(ptr, dtype):
    """a uint16 picture starts at an even address (the 16-bit loads and stores of the device)"""
    if int(ptr) % np.dtype(dtype).itemsize:
        raise ValueError("the %d-bit picture at address %#x is not aligned to its samples" % (8 * np.dtype(dtype).itemsize, int(ptr)))


def _is_dtype(a, dtype):
    """a numpy array of `dtype` in either byte order"""
    return isinstance(a, np.ndarray) and a.dtype.newbyteorder("=") == np.dtype(dtype)
