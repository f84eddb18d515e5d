"""CPU tests of the resample rule (spiht_amd/resample.py): axis_table against a scalar loop over its definition, resize_rule
against torch's antialiased bilinear interpolation in float64, the flip, the normalisation and the conversions against scalar
loops, the refusals, and the one rounding at the end.  No device calls."""
import math

import numpy as np
import pytest

from spiht_amd import floatpx, resample

# (h, w, oh, ow): 1 x 1 boxes and outputs, upscales, ratios up to 16.7
GEOMETRIES = [(1, 1, 1, 1), (1, 9, 3, 1), (9, 1, 1, 4), (37, 53, 1, 1), (7, 5, 20, 31), (64, 48, 4, 3), (33, 97, 8, 8),
              (23, 40, 23, 41), (50, 50, 49, 51), (160, 130, 10, 9), (13, 200, 13, 12), (3, 3, 2, 2), (2, 2, 3, 3)]
TORCH_CAP = 16 * 2.0 ** -53  # five times the 3 * 2^-53 measured when the rule was written


def scalar_table(n_in, n_out):
    """axis_table's sentences, one output and one tap at a time, in Python floats (IEEE float64)"""
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = 1.0 / max(scale, 1.0)
    rows = []
    for i in range(n_out):
        center = scale * (i + 0.5)
        start = max(0, int(center - support + 0.5))
        stop = min(n_in, int(center + support + 0.5))
        w = [max(0.0, 1.0 - abs((j - center + 0.5) * inv)) for j in range(start, stop)]
        total = w[0]
        for v in w[1:]:
            total = total + v
        rows.append((start, stop - start, [v / total for v in w]))
    return rows


def scalar_resize(window, oh, ow, flip):
    """resize_rule's two passes as loops: columns, then rows, acc = a * w, then acc = acc + a * w"""
    c, h, w = window.shape
    cols, rows = scalar_table(w, ow), scalar_table(h, oh)
    if flip:
        cols = cols[::-1]
    t = np.empty((c, h, ow))
    for ch in range(c):
        for y in range(h):
            for x, (s, n, wt) in enumerate(cols):
                acc = float(window[ch, y, s]) * wt[0]
                for k in range(1, n):
                    acc = acc + float(window[ch, y, s + k]) * wt[k]
                t[ch, y, x] = acc
    out = np.empty((c, oh, ow))
    for ch in range(c):
        for y, (s, n, wt) in enumerate(rows):
            for x in range(ow):
                acc = float(t[ch, s, x]) * wt[0]
                for k in range(1, n):
                    acc = acc + float(t[ch, s + k, x]) * wt[k]
                out[ch, y, x] = acc
    return out


def test_axis_table_is_its_definition():
    worst, kmax = 0.0, 0
    for n_out in range(1, 41):
        for n_in in range(1, 41):
            if n_in > resample.MAX_RATIO * n_out:
                continue
            start, count, w = resample.axis_table(n_in, n_out)
            ref = scalar_table(n_in, n_out)
            assert start.dtype == np.int32 and count.dtype == np.int32 and w.dtype == np.float64
            assert w.shape == (n_out, int(count.max())) and w.flags.c_contiguous
            for i, (s, n, wt) in enumerate(ref):
                assert (int(start[i]), int(count[i])) == (s, n), (n_in, n_out, i)
                assert w[i, :n].tobytes() == np.asarray(wt).tobytes(), (n_in, n_out, i)
                assert not w[i, n:].any()
                worst = max(worst, abs(math.fsum(wt) - 1.0))
            assert start.min() >= 0 and (start + count).max() <= n_in and count.min() >= 1
            kmax = max(kmax, int(count.max()))
    print("largest |exact sum of a row - 1|: %.3g ulp; most taps: %d" % (worst / 2.0 ** -52, kmax))
    assert worst <= 2 * 2.0 ** -52
    assert kmax <= resample.MAX_TAPS == 2 * resample.MAX_RATIO + 1


def test_most_taps_at_the_largest_ratio():
    """K stays at MAX_TAPS for every box side of at most MAX_RATIO output sides"""
    for n_out in (1, 2, 3, 7, 14, 224):
        for n_in in (16 * n_out, 16 * n_out - 1, 15 * n_out + 1):
            assert resample.axis_table(n_in, n_out)[1].max() <= resample.MAX_TAPS


def test_equal_sizes_are_the_identity():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 40):
        start, count, w = resample.axis_table(n, n)
        assert np.array_equal(start, np.arange(n)) and count.min() >= 1 and count.max() <= 2
        assert np.array_equal(w[:, 0], np.ones(n)) and not w[:, 1:].any()
    a = rng.random((2, 9, 13))
    out = resample.resize_rule(a, (9, 13))
    assert out.tobytes() == a.tobytes(), "the rule at equal sizes is not the identity in every bit"


def test_rule_is_its_loops():
    rng = np.random.default_rng(11)
    for (h, w, oh, ow) in [(7, 5, 20, 31), (33, 47, 8, 8), (16, 40, 1, 3), (1, 1, 4, 4), (5, 32, 5, 2)]:
        a = rng.standard_normal((2, h, w)) * 3
        for flip in (False, True):
            ref = scalar_resize(a, oh, ow, flip)
            assert resample.resize_rule(a, (oh, ow), flip=flip).tobytes() == ref.tobytes(), (h, w, oh, ow, flip)


def test_rule_against_torch():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    rng = np.random.default_rng(3)
    worst = 0.0
    for (h, w, oh, ow) in GEOMETRIES:
        a = rng.random((3, h, w))
        ref = F.interpolate(torch.from_numpy(a)[None], size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0].numpy()
        d = float(np.abs(resample.resize_rule(a, (oh, ow)) - ref).max())
        print("(%d, %d, %d, %d): %.3g * 2^-53" % (h, w, oh, ow, d / 2.0 ** -53))
        worst = max(worst, d)
    print("largest difference from torch: %.3g * 2^-53" % (worst / 2.0 ** -53))
    assert worst <= TORCH_CAP


def test_flip_reverses_the_columns():
    rng = np.random.default_rng(7)
    for (h, w, oh, ow) in [(33, 97, 8, 8), (7, 5, 20, 31), (50, 50, 49, 51), (64, 48, 4, 3), (3, 1, 2, 5)]:
        a = rng.standard_normal((2, h, w))
        plain = resample.resize_rule(a, (oh, ow))
        assert resample.resize_rule(a, (oh, ow), flip=True).tobytes() == np.ascontiguousarray(plain[..., ::-1]).tobytes()
        s, n, wt = resample.axis_table(w, ow)
        fs, fn, fw = resample.flip_table((s, n, wt))
        assert np.array_equal(fs, s[::-1]) and np.array_equal(fn, n[::-1]) and np.array_equal(fw, wt[::-1])


def _scalar_convert(v, dtype):
    what, arg = resample.out_kind(dtype)
    flat = np.asarray(v, dtype=np.float64).reshape(-1)
    if what == "f64":
        return flat.reshape(v.shape)
    if what == "int":
        peak = 255.0 if arg == np.uint8 else 65535.0
        return np.asarray([int(min(max(x, 0.0), 1.0) * peak) for x in flat], dtype=arg).reshape(v.shape)
    if arg == floatpx.BFLOAT16:
        return np.asarray([int(floatpx.bfloat16_bits(np.float64(x))) for x in flat], dtype=np.uint16).reshape(v.shape)
    t = np.float32 if arg == floatpx.FLOAT32 else np.float16
    with np.errstate(over="ignore"):
        return np.asarray([t(x) for x in flat], dtype=t).reshape(v.shape)


def test_normalisation_and_conversions_are_their_loops():
    rng = np.random.default_rng(13)
    a = rng.random((3, 21, 34)) * 1.4 - 0.2  # (below 0 and above 1: the integer kinds clip)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    plain = resample.resize_rule(a, (6, 9))
    norm = np.empty_like(plain)
    for ch in range(3):
        for i in range(plain[ch].size):
            norm[ch].flat[i] = (float(plain[ch].flat[i]) - mean[ch]) / std[ch]
    assert resample.resize_rule(a, (6, 9), mean=mean, std=std).tobytes() == norm.tobytes()
    for dtype in (np.float64, np.float32, np.float16, "bfloat16", floatpx.FLOAT16, np.uint8, np.uint16):
        got = resample.resize_rule(a, (6, 9), dtype=dtype)
        ref = _scalar_convert(plain, dtype)
        assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), dtype
        if resample.out_kind(dtype)[0] != "int":
            got = resample.resize_rule(a, (6, 9), flip=True, mean=mean, std=std, dtype=dtype)
            assert got.tobytes() == _scalar_convert(np.ascontiguousarray(norm[..., ::-1]), dtype).tobytes(), dtype
    assert resample.resize_rule(a, (6, 9), dtype="bfloat16").dtype == np.uint16


def test_refusals():
    with pytest.raises(ValueError, match="at most 16"):
        resample.check_box(400, 400, (0, 0, 33, 10), (2, 10))
    with pytest.raises(ValueError, match="at most 16"):
        resample.check_box(400, 400, (0, 0, 10, 161), (10, 10))
    assert resample.check_box(400, 400, (3, 4, 32, 160), (2, 10)) == (3, 4, 32, 160, 2, 10)
    for box in [(0, 0, 0, 5), (0, 0, 5, 0), (2, 2, -1, 3)]:
        with pytest.raises(ValueError, match="empty"):
            resample.check_box(20, 30, box, (4, 4))
    for box in [(-1, 0, 5, 5), (0, -1, 5, 5), (16, 0, 5, 5), (0, 26, 5, 5), (0, 0, 21, 5)]:
        with pytest.raises(ValueError, match="leaves"):
            resample.check_box(20, 30, box, (4, 4))
    for size in [(0, 4), (4, 0), (-1, 4)]:
        with pytest.raises(ValueError, match="sides >= 1"):
            resample.check_box(20, 30, (0, 0, 5, 5), size)
    a = np.zeros((3, 8, 8))
    with pytest.raises(ValueError, match="go together"):
        resample.resize_rule(a, (4, 4), mean=[0, 0, 0])
    with pytest.raises(ValueError, match="go together"):
        resample.resize_rule(a, (4, 4), std=[1, 1, 1])
    for dtype in (np.uint8, np.uint16):
        with pytest.raises(ValueError, match="8- / 16-bit"):
            resample.resize_rule(a, (4, 4), mean=[0, 0, 0], std=[1, 1, 1], dtype=dtype)
    with pytest.raises(ValueError, match="per channel"):
        resample.resize_rule(a, (4, 4), mean=[0, 0], std=[1, 1])
    with pytest.raises(ValueError, match="zero"):
        resample.resize_rule(a, (4, 4), mean=[0, 0, 0], std=[1, 0, 1])
    with pytest.raises(ValueError):
        resample.resize_rule(a, (0, 4))
    with pytest.raises(ValueError):
        resample.axis_table(0, 4)


def test_one_rounding_not_two():
    """A picture whose resampled samples lie a hair above float16's ties: 1 + 2^-11 + 2^-40 is 0x3C01 rounded once, and 0x3C00
    through float32, which rounds it to the tie first.  At equal sizes the rule returns the picture's samples, a 2 : 1
    reduction of a constant picture returns the constant where its weights are exact; both must show the difference."""
    x = 1.0 + 2.0 ** -11 + 2.0 ** -40
    a = np.full((1, 8, 8), x)
    for size in [(8, 8), (4, 4)]:
        v = resample.resize_rule(a, size)
        once = resample.resize_rule(a, size, dtype=np.float16)
        assert once.tobytes() == v.astype(np.float16).tobytes()
        twice = v.astype(np.float32).astype(np.float16)
        n = int((once.view(np.uint16) != twice.view(np.uint16)).sum())
        print("%s: %d of %d samples differ between one rounding and two" % (size, n, once.size))
        assert n >= 1
    b = resample.resize_rule(np.full((1, 8, 8), 1.0 + 2.0 ** -8 + 2.0 ** -40), (8, 8), dtype="bfloat16")
    assert np.all(b == 0x3F81)


def test_the_librarys_table_is_axis_table_bit_for_bit():
    """spiht_resample_axis_table (host code, no device): what TileSetCodec uploads in place of B numpy tables per call"""
    import ctypes as C
    from spiht_amd import _lib
    L = _lib.lib()
    K, nb = C.c_int64(), C.c_uint64()
    cases = [(n_in, n_out) for n_out in list(range(1, 41)) + [224] for n_in in list(range(1, 41)) + [100, 333, 1000, 3583, 3584]
             if n_in <= resample.MAX_RATIO * n_out]
    for n_in, n_out in cases:
        for flip in (0, 1):
            t = resample.axis_table(n_in, n_out)
            start, count, w = resample.flip_table(t) if flip else t
            want = np.concatenate([start.view(np.uint8), count.view(np.uint8), w.reshape(-1).view(np.uint8)])
            assert L.spiht_resample_axis_table(n_in, n_out, flip, None, 0, C.byref(K), C.byref(nb)) == _lib.OK  # the question
            assert (K.value, nb.value) == (w.shape[1], want.nbytes)
            buf = np.full(want.nbytes + 8, 0xA5, np.uint8)
            assert L.spiht_resample_axis_table(n_in, n_out, flip, C.c_void_p(buf.ctypes.data), want.nbytes, C.byref(K), C.byref(nb)) == _lib.OK
            assert buf[:want.nbytes].tobytes() == want.tobytes() and (buf[want.nbytes:] == 0xA5).all(), (n_in, n_out, flip)
    buf = np.full(4096, 0xA5, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    assert L.spiht_resample_axis_table(40, 10, 0, None, 0, C.byref(K), C.byref(nb)) == _lib.OK
    assert (K.value, nb.value) == (8, 10 * 8 + 10 * 8 * 8)
    assert L.spiht_resample_axis_table(40, 10, 0, p, nb.value - 1, C.byref(K), C.byref(nb)) == _lib.ERR_ARG  # one byte short
    assert (K.value, nb.value) == (8, 10 * 8 + 10 * 8 * 8) and (buf == 0xA5).all()
    assert L.spiht_resample_axis_table(40, 10, 0, C.c_void_p(buf.ctypes.data + 4), 4000, C.byref(K), C.byref(nb)) == _lib.ERR_ARG
    for n_in, n_out in [(0, 4), (4, 0), (-1, 4)]:
        assert L.spiht_resample_axis_table(n_in, n_out, 0, p, 4096, C.byref(K), C.byref(nb)) == _lib.ERR_ARG
    assert L.spiht_resample_axis_table(4, 4, 0, p, 4096, None, C.byref(nb)) == _lib.ERR_ARG
    assert (buf == 0xA5).all()
