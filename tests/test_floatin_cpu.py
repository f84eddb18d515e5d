"""Float pixels in, without a device: the host rule floatpx.to_float64 (the exact widening every encode of a float kind is
held to), the inference of the kind and the refusals of the new entry points, and the view rule of a view that is read
against the library's.  Every comparison is equality (NaN: NaN-ness)."""
import ctypes as C
import types

import numpy as np
import pytest

from floatin_cases import KINDS, bits, clear_last_bit, float_image, widen
from test_floatpx_cpu import _FakeTorchDtype


def test_to_float64_inverts_convert_on_every_16_bit_pattern():
    from spiht_amd import floatpx
    p = np.arange(65536, dtype=np.uint16)
    for kind, src in (("float16", p.view(np.float16)), ("bfloat16", p)):
        w = floatpx.to_float64(src, kind)
        assert w.dtype == np.float64 and w.shape == p.shape
        nan = np.isnan(w)
        # the NaNs of the kind are its patterns above infinity, either sign
        top, frac = (0x7C00, 0x03FF) if kind == "float16" else (0x7F80, 0x007F)
        assert np.array_equal(nan, ((p & top) == top) & ((p & frac) != 0))
        back = bits(floatpx.convert(w, kind))
        assert np.array_equal(back[~nan], p[~nan]), kind
        assert np.isnan(floatpx.to_float64(floatpx.convert(w[nan], kind), kind)).all()
        # exact: the sign of zero, the subnormals, the infinities
        assert np.array_equal(bits(w[[0, 0x8000]]), bits(np.array([0.0, -0.0])))
        sub = 2.0 ** -24 if kind == "float16" else 2.0 ** -133
        assert w[1] == sub and w[0x8001] == -sub
        inf = 0x7C00 if kind == "float16" else 0x7F80
        assert w[inf] == np.inf and w[0x8000 | inf] == -np.inf
    # float16 through numpy's own widening, bfloat16 through float32's upper half
    assert np.array_equal(bits(floatpx.to_float64(p.view(np.float16), "float16")), bits(p.view(np.float16).astype(np.float64)))
    with np.errstate(invalid="ignore"):
        up = (p.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert np.array_equal(bits(floatpx.to_float64(p, "bfloat16")), bits(up))


def test_to_float64_float32_is_astype():
    from spiht_amd import floatpx
    rng = np.random.default_rng(5)
    p = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)
    p[:12] = (0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
              0x7FC00000)
    a = p.view(np.float32)
    w = floatpx.to_float64(a, np.float32)
    with np.errstate(invalid="ignore"):
        want = a.astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(w)) and np.array_equal(bits(w)[~nan], bits(want)[~nan])
    assert w[2] == 2.0 ** -149 and w[4] == (2.0 ** 23 - 1) * 2.0 ** -149 and w[7] == (2.0 - 2.0 ** -23) * 2.0 ** 127
    assert np.array_equal(bits(w[:2]), bits(np.array([0.0, -0.0]))) and w[9] == np.inf and w[10] == -np.inf
    # the other byte order is a value like any other; a wrong array type is refused
    assert np.array_equal(bits(floatpx.to_float64(a.astype(">f4"), "float32"))[~nan], bits(want)[~nan])
    with pytest.raises(TypeError):
        floatpx.to_float64(np.zeros(4), "float32")
    with pytest.raises(TypeError):
        floatpx.to_float64(a, np.float64)


def test_generator():
    for kind in KINDS:
        P = float_image(kind, 31, 3, 57, 83)
        assert P.shape == (3, 57, 83) and not P.flags.writeable
        assert float_image(kind, 31, 3, 57, 83) is P
        v = widen(P, kind)
        assert -0.08 < v.min() < -0.05 and 1.05 < v.max() < 1.09 and (v < 0).sum() >= 150 and (v > 1).sum() >= 150
        Q = clear_last_bit(P)
        assert Q.dtype == P.dtype and ((bits(P) ^ bits(Q)) <= 1).all() and (bits(P) != bits(Q)).sum() > P.size // 3
        assert float_image(kind, 7, 3, 5, 7).shape == (3, 5, 7)


def test_kind_inference_and_refusals():
    import spiht_amd
    from spiht_amd import floatpx
    from spiht_amd.batch import BatchCodec
    f32, f16, u16 = (np.zeros((3, 32, 32), t) for t in (np.float32, np.float16, np.uint16))
    assert floatpx.input_kind(f32, None, "f") == floatpx.FLOAT32 and floatpx.input_kind(f16, None, "f") == floatpx.FLOAT16
    assert floatpx.input_kind(f32.astype(">f4"), None, "f") == floatpx.FLOAT32
    assert floatpx.input_kind(u16, "bfloat16", "f") == floatpx.BFLOAT16 and floatpx.input_kind(u16, "torch.bfloat16", "f") == floatpx.BFLOAT16
    assert floatpx.input_kind(f32, "float32", "f") == floatpx.FLOAT32 and floatpx.input_kind(f16, np.float16, "f") == floatpx.FLOAT16
    bf16, h16 = _FakeTorchDtype("bfloat16"), _FakeTorchDtype("float16")  # (what a torch dtype looks like to kind_arg)
    assert floatpx.input_kind(u16, bf16, "f") == floatpx.BFLOAT16 and floatpx.input_kind(f16, h16, "f") == floatpx.FLOAT16
    s = spiht_amd.SpihtSettings()
    calls = [lambda a, **k: spiht_amd.encode_image_float(a, s, 2, 1000, **k),
             lambda a, **k: spiht_amd.encode_image_tiled_float(a, 16, s, None, 1000, **k),
             lambda a, **k: spiht_amd.encode_image_layered_float(a, 16, s, None, 1000, 2, **k)]
    for call in calls:
        with pytest.raises(TypeError):   # bit patterns without their kind
            call(u16)
        with pytest.raises(TypeError):   # a dtype that is no float kind
            call(f32, dtype=np.float64)
        with pytest.raises(TypeError):
            call(u16, dtype=np.uint16)
        with pytest.raises(ValueError):  # an array that is no float picture, or not of its dtype
            call(f32.astype(np.float64))
        with pytest.raises(ValueError):
            call(f32.astype(np.uint8))
        with pytest.raises(ValueError):
            call(f32, dtype="bfloat16")
        with pytest.raises(ValueError):
            call(u16, dtype=np.float16)
        with pytest.raises(ValueError):
            call(f16, dtype=np.float32)
        with pytest.raises(ValueError):
            call([[1.0]])
    with pytest.raises(ValueError):      # the integer calls' words for a picture that is not [c, h, w]
        spiht_amd.encode_image_float(f32[0], s, 2, 1000)
    with pytest.raises(ValueError):      # the colour model needs three channels
        spiht_amd.encode_image_float(f32[:2], spiht_amd.SpihtSettings(color_model="IPT"), 2, 1000)
    # the float64 codec's own refusals come first: allocate="rd" without a budget, a weight map without allocate="rd"
    with pytest.raises(ValueError):
        spiht_amd.encode_image_tiled_float(f32, 16, s, None, None, allocate="rd")
    nodev = types.SimpleNamespace(handle=None)  # every refusal below happens before the context is used
    tiled = spiht_amd.TiledCodec(3, 32, 32, 16, s, None, 1000, ctx=nodev)
    for name in ("encode_float", "encode_layered_float", "tile_curves_float"):
        with pytest.raises(TypeError):
            getattr(tiled, name)(u16)
        with pytest.raises(ValueError):
            getattr(tiled, name)(f32, dtype=np.float16)
    with pytest.raises(ValueError):      # a weight map and a target quality steer allocate="rd", as for encode
        tiled.encode_float(f32, roi=np.ones((32, 32), np.uint8))
    with pytest.raises(ValueError):
        tiled.encode_float(f32, target_psnr=30.0)
    with pytest.raises(ValueError):
        tiled.encode_layered_float(f32, 2)
    with pytest.raises(ValueError):
        tiled.tile_curves_float(f32)
    with pytest.raises(ValueError):      # overlapping tiles refuse what encode refuses with them
        spiht_amd.TiledCodec(3, 32, 32, 16, s, None, 1000, ctx=nodev, allocate="rd", overlap=2).encode_float(f32, target_psnr=30.0)
    codec = BatchCodec(3, 32, 32, s, level=2, max_bits=1000, ctx=nodev)
    for bad, exc in ((dict(dtype=np.float64), TypeError), (dict(dtype=None, images=u16[None]), TypeError),
                     (dict(images=f32), ValueError), (dict(images=f32[None, :, :8]), ValueError),
                     (dict(images=f32[None], dtype=np.float16), ValueError)):
        with pytest.raises(exc):
            codec.encode_float(bad.get("images", f32[None]), **{k: v for k, v in bad.items() if k != "images"})
    # the device form: refused before any launch (null pointers) -- an unknown kind, a base off the element, strides that are
    # no multiple of the element or negative
    for kind in KINDS:
        es = floatpx.itemsize(kind)
        with pytest.raises(ValueError):
            codec.encode_device_float(es // 2, 1, 0, 0, 0, kind)
        with pytest.raises(ValueError):
            codec.encode_device_float(0, 1, 0, 0, 0, kind, strides=(3 * 1024 * es, 1024 * es, 32 * es + es // 2, es))
        with pytest.raises(ValueError):
            codec.encode_device_float(0, 1, 0, 0, 0, kind, strides=(3 * 1024 * es, 1024 * es, -32 * es, es))
    with pytest.raises(TypeError):
        codec.encode_device_float(0, 1, 0, 0, 0, np.float64)
    with pytest.raises(TypeError):
        codec.encode_device_float(0, 1, 0, 0, 0, 4)


def test_read_view_rule_equals_the_librarys():
    """check_float_view(.., output=False) against spiht_check_view_flt(kind, .., 0): the same verdict on strides that are
    dense, interleaved, broadcast (0: a view that is read may overlap itself), negative, off the element, and too long"""
    from spiht_amd import _lib, floatpx
    L = _lib.lib()
    rng = np.random.default_rng(3)
    shape = (2, 3, 5, 7)
    for kind in KINDS:
        es = floatpx.itemsize(kind)
        cases = [(105 * es, 35 * es, 7 * es, es), (105 * es, es, 21 * es, 3 * es), (0, 0, 0, 0), (0, 0, 0, es), (es, es, es, es),
                 (105 * es, 35 * es, -7 * es, es), (105 * es, 35 * es, 7 * es, es // 2), (105 * es + 1, 35 * es, 7 * es, es),
                 (1 << 61, 35 * es, 7 * es, es), (1 << 62, 0, 0, es)]
        cases += [tuple(int(v) * (es if rng.random() < 0.8 else 1) for v in rng.integers(-2, 200, 4)) for _ in range(200)]
        verdicts = set()
        for st in cases:
            arr = np.array(st, np.int64)
            lib_ok = L.spiht_check_view_flt(floatpx.kind_arg(kind), *shape, C.c_void_p(arr.ctypes.data), 0) == 0
            try:
                floatpx.check_float_view(kind, shape, st, False)
                ok = True
            except ValueError:
                ok = False
            assert ok == lib_ok, (kind, st)
            verdicts.add(ok)
        assert verdicts == {True, False}
    st = np.array((105 * 4, 35 * 4, 7 * 4, 4), np.int64)
    for kind in (0, 4, -1):
        assert L.spiht_check_view_flt(kind, *shape, C.c_void_p(st.ctypes.data), 0) == _lib.ERR_ARG
