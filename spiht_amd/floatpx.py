"""Float pixels out and in: the host rules the device conversions equal (csrc/floatpx.h: flt_store_value, flt_load_value).

A decode into a float kind -- float32, float16 or bfloat16 -- returns, bit for bit,

    convert(decode_float64(...)[..., :h, :w], kind)

where convert rounds each float64 sample ONCE, to nearest, ties to even: no clip, no scale; overflow gives +-inf, subnormal
results of the target type are kept, the sign of zero is kept, NaN gives some NaN of the target type.  For float32 and
float16 that is numpy's astype, which rounds once.  numpy has no bfloat16: a bfloat16 picture is a uint16 array of bit
patterns, and the rule is written out below in integer arithmetic on the float64 bits (bfloat16_bits).  In torch:

    torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)

torch is NOT the yardstick for the narrowing direction: its CPU conversion from float64 goes through float32 and so rounds
twice.  1 + 2^-8 + 2^-40 becomes 0x3F80 there, where one rounding gives 0x3F81, and 1 + 2^-11 + 2^-40 becomes the float16
0x3C00, where numpy gives 0x3C01.  The widening direction (bfloat16_to_float64) is exact everywhere.

Float pixels IN go the other way: an encode of a picture P of a float kind returns, field by field and bit for bit, what
the float64 call returns for

    to_float64(P, kind)

the exact widening of every sample -- nothing scaled, nothing clipped, subnormals of every kind keep their value.  This is
NOT encode_image(P32): a float32 array given to encode_image keeps the reference's single-precision transform, the same
array given to encode_image_float is transformed in float64.

This module is to the kernels what overlap.py and alloc.py are: no device, no library, numpy only.
"""
import numpy as np

FLOAT32, FLOAT16, BFLOAT16 = 1, 2, 3  # the `kind` of the C ABI's *_flt calls (include/spiht_hip.h)
KINDS = (FLOAT32, FLOAT16, BFLOAT16)
_NAMES = {FLOAT32: "float32", FLOAT16: "float16", BFLOAT16: "bfloat16"}
_BY_NAME = {"float32": FLOAT32, "float16": FLOAT16, "bfloat16": BFLOAT16}


def kind_arg(dtype):
    """np.float32, np.float16 (types or dtypes), the strings "float32", "float16", "bfloat16", or str() of a torch dtype
    ("torch.bfloat16": a torch dtype itself goes through str(), torch is not imported) -> the kind id.  TypeError otherwise."""
    if isinstance(dtype, (bool, int, float, np.integer, np.floating)) or dtype is None:
        raise TypeError("not a float pixel type: %r" % (dtype,))
    if isinstance(dtype, str):
        name = dtype
    elif type(dtype).__module__.split(".")[0] == "torch":
        name = str(dtype)
    else:
        try:
            name = np.dtype(dtype).name
        except (TypeError, ValueError):
            raise TypeError("not a float pixel type: %r" % (dtype,)) from None
    if name.startswith("torch."):
        name = name[len("torch."):]
    if name not in _BY_NAME:
        raise TypeError("float pixels come as float32, float16 or bfloat16, not %r" % (dtype,))
    return _BY_NAME[name]


def kind_name(kind):
    return _NAMES[kind_id(kind)]


def kind_id(kind):
    """a kind id as it is, anything else through kind_arg"""
    return kind if isinstance(kind, int) and not isinstance(kind, bool) and kind in KINDS else kind_arg(kind)


def itemsize(kind):
    """bytes per sample: 4 or 2"""
    return 4 if kind_id(kind) == FLOAT32 else 2


def storage_dtype(kind):
    """the numpy dtype a picture of the kind comes in: float32, float16, or uint16 bit patterns for bfloat16"""
    return np.dtype({FLOAT32: np.float32, FLOAT16: np.float16, BFLOAT16: np.uint16}[kind_id(kind)])


def bfloat16_bits(a):
    """float64 array -> uint16 array of bfloat16 bit patterns, each sample rounded once to nearest, ties to even.

    A bfloat16 magnitude pattern p = (E << 7) | frac is (128 + frac) * 2^(E - 134) for E >= 1 and frac * 2^-133 for E = 0,
    so p = (max(E, 1) - 1) * 128 + sig with sig the value in units of 2^(max(E, 1) - 134): rounding the 53-bit significand
    m of the float64 (value m * 2^(e - 1075)) to that unit is a right shift by 941 - e + max(E, 1), E = e - 896, with the
    half-even rule on the bits shifted out, and a carry out of sig moves p into the next exponent by itself -- up to
    0x7F80, infinity."""
    u = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    sign = (u >> np.uint64(63)).astype(np.uint16) << np.uint16(15)
    e = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    man = u & np.uint64((1 << 52) - 1)
    m = np.where(e > 0, man | np.uint64(1 << 52), man)
    E = np.maximum(e - 896, 1)
    s = np.minimum(941 - e + E, 60).astype(np.uint64)  # (45 for a bfloat16 normal; from 54 on everything rounds to zero)
    q = m >> s
    rem = m & ((np.uint64(1) << s) - np.uint64(1))
    half = np.uint64(1) << (s - np.uint64(1))
    up = (rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))
    p = (E - 1) * 128 + q.astype(np.int64) + up
    p = np.where(E >= 255, 0x7F80, np.minimum(p, 0x7F80))
    p = np.where((e == 0x7FF) & (man != 0), 0x7FC0, p)  # NaN -> the quiet NaN of its sign
    return (p.astype(np.uint16) | sign).reshape(np.shape(a))


def bfloat16_to_float64(bits):
    """uint16 bit patterns -> float64, exact: a bfloat16 is the upper half of the float32 of the same value"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    with np.errstate(invalid="ignore"):  # (a signalling NaN pattern is a NaN like any other here)
        return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def convert(a, kind):
    """float64 array -> the array of the kind (storage_dtype), every sample rounded once"""
    kind = kind_id(kind)
    a = np.asarray(a, dtype=np.float64)
    if kind == BFLOAT16:
        return bfloat16_bits(a)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return a.astype(storage_dtype(kind))


def to_float64(a, kind):
    """array of the kind (storage_dtype: float32, float16, or uint16 bit patterns for bfloat16) -> float64, exact: the rule of
    float pixels in.  Subnormals keep their value, the sign of zero is kept, infinities stay, a NaN gives a NaN."""
    kind = kind_id(kind)
    if kind == BFLOAT16:
        return bfloat16_to_float64(a).reshape(np.shape(a))
    a = np.asarray(a)
    if a.dtype.newbyteorder("=") != storage_dtype(kind):
        raise TypeError("a %s picture comes as a %s array, not %s" % (kind_name(kind), storage_dtype(kind).name, a.dtype))
    with np.errstate(invalid="ignore"):
        return a.astype(np.float64)


def input_kind(a, dtype, name):
    """The kind of the picture `a` given to the encode call `name` with dtype=`dtype`: inferred from a float32 / float16 array
    (a dtype, if given, must say the same); uint16 bit patterns need dtype="bfloat16" or torch.bfloat16.  ValueError for an
    array that is no float picture or does not match its dtype, TypeError for a dtype that is no float kind."""
    if not isinstance(a, np.ndarray):
        raise ValueError("%s takes a float32, float16 or (bfloat16 bit patterns) uint16 array, not %s" % (name, type(a)))
    have = a.dtype.newbyteorder("=")
    if dtype is None:
        if have == np.float32:
            return FLOAT32
        if have == np.float16:
            return FLOAT16
        if have == np.uint16:
            raise TypeError("%s: a uint16 array of bit patterns needs dtype=\"bfloat16\"" % name)
        raise ValueError("%s takes a float32, float16 or (bfloat16 bit patterns) uint16 array, not %s" % (name, a.dtype))
    kind = kind_id(dtype)
    if have != storage_dtype(kind):
        raise ValueError("%s takes a %s array for dtype=%s, not %s" % (name, storage_dtype(kind).name, kind_name(kind), a.dtype))
    return kind


def check_float_view(dtype, shape, strides, output):
    """The library's rule for a float view (include/spiht_hip.h, *_flt; spiht_check_view_flt), beside check_u8_view and
    check_u16_view: BYTE strides of a (B, c, h, w) or (c, h, w) `shape` are non-negative multiples of the element size (4 or
    2), and a view that is written does not overlap itself -- sorted by stride, every dimension longer than one steps past
    the last byte the smaller ones reach.  Raises ValueError.  No device and no library needed."""
    es = itemsize(dtype)
    shape, strides = [int(x) for x in shape], [int(x) for x in strides]
    if len(shape) != len(strides) or len(shape) not in (3, 4):
        raise ValueError("%d strides for a %d-dimensional picture" % (len(strides), len(shape)))
    if len(shape) == 3:
        shape, strides = [1] + shape, [0] + strides
    if min(shape) < 1:
        raise ValueError("empty %s picture %s" % (kind_name(dtype), shape))
    what = "the strides %s of the %s %s %s" % (strides, kind_name(dtype), "output" if output else "input", shape)
    if any(st < 0 or st % es for st in strides):
        raise ValueError("%s are not supported (negative, or no multiple of %d)" % (what, es))
    if es + sum((n - 1) * st for n, st in zip(shape, strides)) >= 1 << 62:
        raise ValueError("%s span too many bytes" % what)
    if output:
        reach = 0
        for st, n in sorted(zip(strides, shape)):
            if n <= 1:
                continue
            if st < reach + es:
                raise ValueError("%s are not supported (overlapping)" % what)
            reach += (n - 1) * st
