"""CPU tests of the float pixel rule (spiht_amd/floatpx.py): bfloat16_bits against a search for the nearest pattern on
every pattern, every midpoint and their float64 neighbours; the widening direction; convert against numpy's astype; the
type argument; the view rule.  No device calls: every comparison is equality."""
import numpy as np
import pytest

from spiht_amd import floatpx

F64_ONE_AND = lambda *exps: float(1.0 + sum(2.0 ** e for e in exps))  # noqa: E731


def _bf16_values():
    """the values of the magnitude patterns 0 .. 0x7F80, with 2^128 standing for infinity: IEEE rounds as if the exponent
    range had no end and calls what reaches 2^128 an overflow"""
    p = np.arange(0x7F81, dtype=np.uint16)
    v = floatpx.bfloat16_to_float64(p)
    v[0x7F80] = 2.0 ** 128
    assert np.all(np.diff(v) > 0)
    return v


def _nearest_pattern(x, vals):
    """the bfloat16 pattern nearest to each finite float64 x, ties to the even pattern, by search in the table of all values.
    The two distances are exact in float64: x and its two neighbours are multiples of x's ulp (of the pattern's, larger,
    quantum) and each difference is smaller than 2^53 of them."""
    ax = np.abs(x)
    hi = np.minimum(np.searchsorted(vals, ax, side="left"), 0x7F80)
    lo = np.maximum(hi - 1, 0)
    over = ax >= vals[0x7F80]
    d_lo, d_hi = ax - vals[lo], vals[hi] - ax
    pick_hi = (d_hi < d_lo) | ((d_hi == d_lo) & (hi % 2 == 0))
    p = np.where(pick_hi | (ax == vals[hi]), hi, lo)
    p = np.where(over, 0x7F80, p).astype(np.uint16)
    return p | (np.signbit(x).astype(np.uint16) << np.uint16(15))


def hard_inputs():
    """float64 samples at which a conversion to bfloat16 or float16 can go wrong: every bfloat16 value, every midpoint of
    neighbours, each of those one float64 ulp up and down, both signs; the same around float16's values; the witnesses of
    double rounding; the overflow thresholds; subnormals of all three kinds; zeros, infinities, NaN"""
    vals = _bf16_values()
    mids = (vals[:-1] + vals[1:]) / 2  # exact: neighbours differ by one quantum
    assert np.all((mids > vals[:-1]) & (mids < vals[1:]))
    h = np.arange(0x7C01, dtype=np.uint16).view(np.float16).astype(np.float64)
    h[0x7C00] = 65536.0
    hm = (h[:-1] + h[1:]) / 2
    base = np.concatenate([vals, mids, h, hm])
    pts = np.concatenate([base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf)])
    f32 = np.array([np.finfo(np.float32).max, np.finfo(np.float32).tiny, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150,
                    float(np.finfo(np.float32).max) + 2.0 ** 103, 2.0 ** 128], dtype=np.float64)
    f32 = np.concatenate([f32, np.nextafter(f32, np.inf), np.nextafter(f32, -np.inf)])
    special = np.array([0.0, F64_ONE_AND(-8, -40), F64_ONE_AND(-11, -40), F64_ONE_AND(-8), F64_ONE_AND(-7, -8),
                        0.17603515625000016, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, np.inf], dtype=np.float64)
    x = np.concatenate([pts, f32, special])
    return np.concatenate([x, -x, [np.nan, -np.nan]])


def test_bfloat16_bits_is_the_nearest_pattern():
    vals = _bf16_values()
    x = hard_inputs()
    fin = ~np.isnan(x)
    got = floatpx.bfloat16_bits(x)
    assert got.dtype == np.uint16 and got.shape == x.shape
    assert np.array_equal(got[fin], _nearest_pattern(x[fin], vals))
    nan = got[~fin]
    assert np.all((nan & 0x7F80) == 0x7F80) and np.all((nan & 0x7F) != 0)
    # the witness of double rounding, overflow at the last finite value plus half an ulp, subnormals, zeros, infinities
    one = lambda v: int(floatpx.bfloat16_bits(np.array([v]))[0])  # noqa: E731
    assert one(F64_ONE_AND(-8, -40)) == 0x3F81 and one(F64_ONE_AND(-8)) == 0x3F80 and one(F64_ONE_AND(-7, -8)) == 0x3F82
    top = float(vals[0x7F7F])
    assert one(top) == 0x7F7F and one(top + 2.0 ** 119) == 0x7F80 and one(np.nextafter(top + 2.0 ** 119, 0)) == 0x7F7F
    assert one(-top - 2.0 ** 119) == 0xFF80
    assert one(2.0 ** -133) == 0x0001 and one(2.0 ** -134) == 0x0000 and one(np.nextafter(2.0 ** -134, 1)) == 0x0001
    assert one(3 * 2.0 ** -134) == 0x0002 and one(2.0 ** -126) == 0x0080 and one(np.nextafter(2.0 ** -126, 0)) == 0x0080
    assert one(0.0) == 0 and one(-0.0) == 0x8000 and one(np.inf) == 0x7F80 and one(-np.inf) == 0xFF80
    assert one(5e-324) == 0 and one(-5e-324) == 0x8000
    assert floatpx.bfloat16_bits(np.zeros((2, 3, 4))).shape == (2, 3, 4)


def test_bfloat16_to_float64_is_the_inverse():
    p = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    v = floatpx.bfloat16_to_float64(p)
    fin = np.isfinite(v)
    assert fin.sum() == 2 * 0x7F80
    assert np.array_equal(floatpx.bfloat16_bits(v[fin]), p[fin])
    assert np.array_equal(np.isnan(v), ((p & 0x7F80) == 0x7F80) & ((p & 0x7F) != 0))
    assert v[0x3F80] == 1.0 and v[0x0001] == 2.0 ** -133 and v[0x7F7F] == (2 - 2.0 ** -7) * 2.0 ** 127
    assert np.signbit(v[0x8000]) and v[0x8000] == 0
    try:
        import torch
    except ImportError:
        return
    t = torch.from_numpy(p.view(np.int16)).view(torch.bfloat16).to(torch.float64).numpy()  # widening: exact in torch too
    assert np.array_equal(t[fin], v[fin]) and np.array_equal(np.isnan(t), np.isnan(v))


@pytest.mark.parametrize("kind, dtype", [("float32", np.float32), ("float16", np.float16)])
def test_convert_is_astype(kind, dtype):
    x = hard_inputs()
    got = floatpx.convert(x, kind)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want = x.astype(dtype)
    assert got.dtype == np.dtype(dtype)
    u = np.uint32 if dtype is np.float32 else np.uint16
    nan = np.isnan(x)
    assert np.array_equal(got.view(u)[~nan], want.view(u)[~nan]) and np.all(np.isnan(got[nan]))
    # numpy rounds once: the witness a conversion through float32 gets wrong, and float16's corners
    h = lambda v: int(floatpx.convert(np.array([v]), "float16").view(np.uint16)[0])  # noqa: E731
    assert h(F64_ONE_AND(-11, -40)) == 0x3C01 and h(F64_ONE_AND(-11)) == 0x3C00
    assert h(65504.0) == 0x7BFF and h(65520.0) == 0x7C00 and h(np.nextafter(65520.0, 0)) == 0x7BFF
    assert h(2.0 ** -24) == 0x0001 and h(2.0 ** -25) == 0x0000 and h(np.nextafter(2.0 ** -25, 1)) == 0x0001
    assert h(-0.0) == 0x8000
    f = lambda v: int(floatpx.convert(np.array([v]), "float32").view(np.uint32)[0])  # noqa: E731
    assert f(F64_ONE_AND(-24)) == 0x3F800000 and f(F64_ONE_AND(-24, -50)) == 0x3F800001 and f(2.0 ** -149) == 1
    assert f(2.0 ** -150) == 0 and f(1e39) == 0x7F800000


def test_convert_bfloat16_and_sizes():
    x = hard_inputs()
    assert np.array_equal(floatpx.convert(x, "bfloat16"), floatpx.bfloat16_bits(x))
    assert floatpx.convert(np.zeros((2, 5)), "torch.bfloat16").dtype == np.uint16
    assert [floatpx.itemsize(k) for k in ("float32", "float16", "bfloat16", np.float32, np.float16)] == [4, 2, 2, 4, 2]
    assert [floatpx.storage_dtype(k) for k in (1, 2, 3)] == [np.float32, np.float16, np.uint16]


class _FakeTorchDtype:
    """what a torch dtype looks like to kind_arg: its module and its str()"""
    def __init__(self, name):
        self.name = name

    def __str__(self):
        return "torch." + self.name


_FakeTorchDtype.__module__ = "torch"


def test_kind_arg():
    K = floatpx.kind_arg
    assert (floatpx.FLOAT32, floatpx.FLOAT16, floatpx.BFLOAT16) == (1, 2, 3)
    assert K(np.float32) == K(np.dtype(np.float32)) == K("float32") == K("torch.float32") == 1
    assert K(np.float16) == K(np.dtype("<f2")) == K("float16") == K("torch.float16") == 2
    assert K("bfloat16") == K("torch.bfloat16") == 3
    assert K(_FakeTorchDtype("bfloat16")) == 3 and K(_FakeTorchDtype("float16")) == 2
    for wrong in (np.float64, np.uint16, np.uint8, "float64", "torch.float64", "half", "", None, 2, 2.0, True, object(),
                  _FakeTorchDtype("int16")):
        with pytest.raises(TypeError):
            K(wrong)
    try:
        import torch
    except ImportError:
        return
    assert [K(t) for t in (torch.float32, torch.float16, torch.bfloat16)] == [1, 2, 3]
    with pytest.raises(TypeError):
        K(torch.float64)


def test_check_float_view():
    chk = floatpx.check_float_view
    c, h, w = 3, 5, 7
    for kind, es in (("float32", 4), ("float16", 2), ("bfloat16", 2)):
        dense = (h * w * es, w * es, es)
        hwc = (es, w * c * es, c * es)
        rgba = (es, w * 4 * es, 4 * es)
        for st in (dense, hwc, rgba):
            chk(kind, (c, h, w), st, True)
            chk(kind, (2, c, h, w), (h * w * 4 * es + 64,) + st, True)
        chk(kind, (c, h, w), (0, w * es, es), False)  # a grey picture read as three channels
        bad = [(-h * w * es, w * es, es),          # negative
               (h * w * es, w * es, es + 1),       # odd
               (h * w * es + 1, w * es, es),
               (h * w * es, w * es, es // 2)]      # samples overlap
        for st in bad:
            with pytest.raises(ValueError):
                chk(kind, (c, h, w), st, True)
        for st in ((0, w * es, es), (h * w * es, (w - 1) * es, es), (es, w * (c - 1) * es, c * es)):  # an output that overlaps
            chk(kind, (c, h, w), st, False)
            with pytest.raises(ValueError):
                chk(kind, (c, h, w), st, True)
        with pytest.raises(ValueError):
            chk(kind, (c, h, w), dense + (es,), True)
        with pytest.raises(ValueError):
            chk(kind, (c, 0, w), dense, True)
    # float32: strides that are even but no multiple of 4
    for st in ((5 * 7 * 4 + 2, 7 * 4, 4), (5 * 7 * 4, 7 * 4 + 2, 4), (5 * 7 * 4, 7 * 4, 6)):
        with pytest.raises(ValueError):
            chk("float32", (c, h, w), st, False)
        chk("float16", (c, h, w), st, False)
    with pytest.raises(TypeError):
        chk(np.float64, (c, h, w), (h * w * 8, w * 8, 8), True)


def test_check_float_view_is_the_librarys_rule():
    """the C entry point refuses and accepts what the host rule does"""
    import ctypes as C
    from spiht_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    shape = (2, 3, 5, 7)
    n_ok = 0
    for _ in range(400):
        kind = int(rng.integers(1, 4))
        es = floatpx.itemsize(kind)
        st = [int(v) for v in rng.choice([0, es, 2 * es, 3 * es, 7 * es, 21 * es, 28 * es, 35 * es, 105 * es, 140 * es, es + 2, 6, -es],
                                         size=4)]
        for output in (0, 1):
            try:
                floatpx.check_float_view(kind, shape, st, output)
                ok = True
            except ValueError:
                ok = False
            arr = np.array(st, dtype=np.int64)
            rc = L.spiht_check_view_flt(kind, *shape, C.c_void_p(arr.ctypes.data), output)
            assert (rc == 0) == ok, (kind, st, output)
            n_ok += ok
    assert n_ok > 20
    arr = np.array([420, 140, 28, 4], dtype=np.int64)
    assert L.spiht_check_view_flt(0, *shape, C.c_void_p(arr.ctypes.data), 1) != 0
    assert L.spiht_check_view_flt(4, *shape, C.c_void_p(arr.ctypes.data), 1) != 0


def test_float_names_exist():
    import spiht_amd
    from spiht_amd import _lib, spiht_wrapper, tiles
    from spiht_amd.batch import BatchCodec
    for name in ("decode_image_float", "decode_image_reduced_float", "decode_image_tiled_float", "decode_image_window_float",
                 "decode_image_layered_float", "decode_image_layered_window_float", "floatpx"):
        assert hasattr(spiht_amd, name), name
    assert spiht_wrapper.check_float_view is floatpx.check_float_view
    for name in ("decode_float", "decode_device_float", "decode_reduced_float", "decode_reduced_device_float"):
        assert callable(getattr(BatchCodec, name))
    for name in ("decode_float", "decode_window_float", "decode_layered_float", "decode_layered_window_float"):
        assert callable(getattr(tiles.TiledCodec, name))
    L = _lib.lib()
    for s in ("spiht_check_view_flt", "spiht_convert_batch_flt", "spiht_decode_image_batch_flt", "spiht_decode_image_host_flt",
              "spiht_dequant_idwt_flags_batch_flt", "spiht_dequant_idwt_reduced_batch_flt", "spiht_decode_image_reduced_batch_flt",
              "spiht_decode_image_reduced_host_flt", "spiht_tile_blend_flt", "spiht_tile_mosaic_f32"):
        assert hasattr(L, s) and s in _lib.SYMBOLS, s
    assert L.spiht_abi_version() == 2  # functions were only added
    import spiht
    assert spiht.decode_image_float is spiht_amd.decode_image_float and spiht.floatpx is floatpx
