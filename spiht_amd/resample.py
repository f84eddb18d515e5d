"""Resized crops: the host rule the resample kernel equals (csrc/resample.hip: k_tile_resample_set).

A box of any size and aspect of a decoded picture is resampled to ONE size (oh, ow), optionally mirrored left to right and
normalised per channel, and rounded ONCE to the output kind:

    resize_rule(window, (oh, ow), flip, mean, std, dtype)

with window the float64 box [c, h, w] (TiledCodec.decode_window).  The filter is the antialiased triangle ("bilinear,
antialias") of Pillow and of torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False), restated
so that every operation and its order is fixed: the weights are axis_table's, in float64; the columns are resampled first,
then the rows; every product and every sum is rounded on its own (nothing fused); `(v - mean) / std` in float64 with IEEE
division; one conversion at the end -- floatpx.convert for the float kinds, overlap.convert for 8 / 16 bits.

The kernel takes axis_table's output as it is, so its weights are these in every bit: it only multiplies and adds in the
stated order, normalises and converts.  This module is to it what overlap.py is to the blend: no device, numpy only.

Out of scope: filters other than the triangle, fractional box coordinates, vertical flips.
"""
import numpy as np

from . import floatpx, overlap

MAX_RATIO = 16   # a box side is at most this many output sides: at most MAX_TAPS taps per output sample
MAX_TAPS = 33    # 2 * MAX_RATIO + 1: the K the kernel is built for


def axis_table(n_in, n_out):
    """-> (start int32 [n_out], count int32 [n_out], weights float64 [n_out, K]), K = count.max(), rows padded with zeros:
    output i of an axis of n_in samples resampled to n_out is the sum over k < count[i] of in[start[i] + k] * weights[i, k].
    In float64: scale = n_in / n_out, support = max(scale, 1), inv = 1 / max(scale, 1), center = scale * (i + 0.5),
    start = max(0, int(center - support + 0.5)), stop = min(n_in, int(center + support + 0.5)),
    w_j = max(0, 1 - |(j - center + 0.5) * inv|), each divided by the row's sum taken in ascending j."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("axis_table(%d, %d): both sides >= 1" % (n_in, n_out))
    scale = np.float64(n_in) / np.float64(n_out)
    support = max(scale, np.float64(1.0))
    inv = np.float64(1.0) / max(scale, np.float64(1.0))
    center = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    start = np.maximum(0, (center - support + 0.5).astype(np.int64))  # (astype truncates, as int() does)
    count = np.minimum(n_in, (center + support + 0.5).astype(np.int64)) - start
    k = np.arange(int(count.max()), dtype=np.int64)
    w = np.maximum(0.0, 1.0 - np.abs(((start[:, None] + k).astype(np.float64) - center[:, None] + 0.5) * inv))
    w[k >= count[:, None]] = 0.0
    w /= np.add.accumulate(w, axis=1)[:, -1:]  # the sum in ascending j, one addition at a time; a padding zero adds nothing
    return start.astype(np.int32), count.astype(np.int32), w


def flip_table(table):
    """the table of the mirrored axis: output x is output n_out - 1 - x, the additions of every output as they were"""
    start, count, w = table
    return np.ascontiguousarray(start[::-1]), np.ascontiguousarray(count[::-1]), np.ascontiguousarray(w[::-1])


def _apply(a, table):
    """a [..., n_in] -> [..., n_out] by the table along the last axis: acc = a[start] * w[0], then acc = acc + a[start + k] *
    w[k] for k = 1 .. count - 1, every product and every sum rounded on its own"""
    start, count, w = (np.asarray(t) for t in table)
    start = start.astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = a[..., start] * w[:, 0]
        for k in range(1, w.shape[1]):
            live = k < count
            term = a[..., np.where(live, start + k, start)] * w[:, k]
            acc = np.where(live, acc + term, acc)
    return acc


def out_kind(dtype):
    """the output kind of a resample -> ("f64", None), ("int", np.dtype uint8 / uint16) or ("flt", the floatpx kind id).
    np.float64 / None, np.uint8, np.uint16; every float kind floatpx.kind_id takes; an object with .kind and .storage (px.Elem)"""
    if hasattr(dtype, "storage") and hasattr(dtype, "kind") and not isinstance(dtype, np.dtype):
        if dtype.kind is not None:
            return "flt", int(dtype.kind)
        dtype = dtype.storage
    if dtype is None:
        return "f64", None
    if not (isinstance(dtype, (str, int)) or type(dtype).__module__.split(".")[0] == "torch"):
        d = np.dtype(dtype)
        if d == np.float64:
            return "f64", None
        if d in (np.dtype(np.uint8), np.dtype(np.uint16)):
            return "int", d
    return "flt", floatpx.kind_id(dtype)


def norm_args(mean, std, c, dtype, name="resize_rule"):
    """mean / std as float64 [c] (both or neither: (None, None)); ValueError for one without the other, a wrong length, a zero
    std, and for either with an integer kind"""
    if mean is None and std is None:
        return None, None
    if mean is None or std is None:
        raise ValueError("%s: mean and std go together" % name)
    if out_kind(dtype)[0] == "int":
        raise ValueError("%s: mean / std do not go with 8- / 16-bit pixels" % name)
    mean, std = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(std, dtype=np.float64).reshape(-1)
    if len(mean) != c or len(std) != c:
        raise ValueError("%s: mean and std have one value per channel (%d)" % (name, c))
    if np.any(std == 0):
        raise ValueError("%s: std must not be zero" % name)
    return np.ascontiguousarray(mean), np.ascontiguousarray(std)


def check_box(H, W, box, size, name="resize_rule"):
    """box = (y0, x0, h, w) of an H x W picture resampled to size = (oh, ow) -> the six as ints.  ValueError for a box that is
    empty or leaves its picture, an output side below 1 and a box side above MAX_RATIO output sides."""
    y0, x0, h, w = (int(v) for v in box)
    oh, ow = (int(v) for v in size)
    if h < 1 or w < 1:
        raise ValueError("%s: the box (%d, %d, %d, %d) is empty" % (name, y0, x0, h, w))
    if y0 < 0 or x0 < 0 or y0 + h > int(H) or x0 + w > int(W):
        raise ValueError("%s: the box (%d, %d, %d, %d) leaves the %d x %d picture" % (name, y0, x0, h, w, H, W))
    if oh < 1 or ow < 1:
        raise ValueError("%s: an output of %d x %d: both sides >= 1" % (name, oh, ow))
    if h > MAX_RATIO * oh or w > MAX_RATIO * ow:
        raise ValueError("%s: a box of %d x %d to %d x %d: a box side is at most %d output sides" % (name, h, w, oh, ow, MAX_RATIO))
    return y0, x0, h, w, oh, ow


def convert(v, dtype):
    """the one conversion at the end: float64 as it is, a float kind by floatpx.convert, 8 / 16 bits by overlap.convert"""
    what, arg = out_kind(dtype)
    if what == "f64":
        return np.asarray(v, dtype=np.float64)
    return floatpx.convert(v, arg) if what == "flt" else overlap.convert(v, arg)


def resize_rule(window, size, flip=False, mean=None, std=None, dtype=np.float64):
    """window: float64 [c, h, w] -> [c, oh, ow] of the kind `dtype` (bfloat16: uint16 bit patterns): the columns by
    axis_table(w, ow) -- its rows reversed with `flip` --, then the rows by axis_table(h, oh), then (v - mean[ch]) / std[ch],
    then one conversion.  No limit on the ratio here: MAX_RATIO is the call's (check_box)."""
    window = np.asarray(window, dtype=np.float64)
    if window.ndim != 3 or min(window.shape) < 1:
        raise ValueError("resize_rule takes a window [c, h, w]")
    oh, ow = (int(v) for v in size)
    if oh < 1 or ow < 1:
        raise ValueError("resize_rule: an output of %d x %d: both sides >= 1" % (oh, ow))
    c, h, w = window.shape
    mean, std = norm_args(mean, std, c, dtype)
    cols = axis_table(w, ow)
    t = _apply(window, flip_table(cols) if flip else cols)                  # [c, h, ow]
    v = _apply(t.transpose(0, 2, 1), axis_table(h, oh)).transpose(0, 2, 1)  # [c, oh, ow]
    if mean is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            v = (v - mean[:, None, None]) / std[:, None, None]
    return np.ascontiguousarray(convert(v, dtype))
