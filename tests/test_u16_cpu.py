"""CPU tests of the 16-bit pixel path (encode_image_u16 / decode_image_u16, BatchCodec.*_u16, Pipeline.submit_u16): the
names exist, the argument checks raise before any GPU context is needed, the view rule, and the two facts about the
arithmetic the device code rests on.  No device calls."""
import numpy as np
import pytest

U16_SYMBOLS = ("spiht_check_view_u16", "spiht_encode_image_batch_u16", "spiht_decode_image_batch_u16",
               "spiht_dwt_pyramid_batch_u16", "spiht_dequant_idwt_flags_batch_u16", "spiht_idwt_level1_flags_batch_u16",
               "spiht_encode_image_host_u16", "spiht_decode_image_host_u16", "spiht_pipeline_submit_u16")


def test_u16_names_exist():
    import spiht_amd
    from spiht_amd import _lib, spiht_wrapper
    from spiht_amd.batch import BatchCodec, Pipeline
    assert callable(spiht_amd.encode_image_u16) and callable(spiht_amd.decode_image_u16)
    assert callable(spiht_wrapper.check_u16_view)
    for name in ("encode_u16", "decode_u16", "encode_device_u16", "decode_device_u16"):
        assert callable(getattr(BatchCodec, name))
    assert callable(Pipeline.submit_u16)
    L = _lib.lib()
    for s in U16_SYMBOLS:
        assert hasattr(L, s) and s in _lib.SYMBOLS, s
        assert getattr(L, s).argtypes == getattr(L, s[:-2] + "8").argtypes, s  # the 8-bit sibling's arguments
    assert L.spiht_abi_version() == 2  # functions were only added
    # the reference's surface of the alias package stays as it is
    import spiht
    assert not hasattr(spiht, "encode_image_u16") and not hasattr(spiht, "decode_image_u16")


@pytest.fixture
def no_context(monkeypatch):
    """any attempt to create a GPU context fails the test"""
    from spiht_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a context was created before the argument check")
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib.Context, "__init__", boom)


def _unaligned_u16(shape):
    """a uint16 array whose first sample lies at an odd address"""
    n = int(np.prod(shape))
    raw = np.zeros(2 * n + 8, np.uint8)
    off = 1 if raw.ctypes.data % 2 == 0 else 0
    a = np.ndarray(shape, dtype=np.uint16, buffer=raw.data, offset=off)
    assert a.ctypes.data % 2 == 1
    return a, raw


def test_encode_image_u16_argument_errors(no_context):
    import spiht_amd
    s = spiht_amd.SpihtSettings()
    for wrong in (np.float64, np.uint8, np.int16, np.float16):  # wrong dtype
        with pytest.raises(ValueError):
            spiht_amd.encode_image_u16(np.zeros((3, 8, 8), wrong), s)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u16([[1, 2], [3, 4]], s)
    with pytest.raises(ValueError):  # wrong ndim
        spiht_amd.encode_image_u16(np.zeros((8, 8), np.uint16), s)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u16(np.zeros((1, 3, 8, 8), np.uint16), s)
    with pytest.raises(ValueError):  # a colour model needs three channels
        spiht_amd.encode_image_u16(np.zeros((2, 8, 8), np.uint16), spiht_amd.SpihtSettings(color_model="IPT"))
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u16(np.zeros((8, 8, 4), np.uint16), spiht_amd.SpihtSettings(color_model="IPT"),
                                   channels_last=True)
    # odd byte strides: a uint16 view laid over bytes with a row pitch of 17
    raw = np.zeros(3 * 8 * 17 + 2, np.uint8)
    odd = np.lib.stride_tricks.as_strided(raw[:2].view(np.uint16), shape=(3, 8, 8), strides=(8 * 17, 17, 2), writeable=False)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u16(odd, s)
    # an unaligned base
    una, keep = _unaligned_u16((3, 8, 8))
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u16(una, s)


def test_decode_image_u16_colour_needs_three_channels(no_context):
    import spiht_amd
    r = spiht_amd.EncodingResult(b"\x00" * 8, 8, 8, 2, 3, None)
    with pytest.raises(ValueError):
        spiht_amd.decode_image_u16(r, spiht_amd.SpihtSettings(color_model="IPT"))


def test_batch_u16_argument_errors(no_context):
    """BatchCodec's and Pipeline's 16-bit checks need no context of their own: run on objects that never got one"""
    from spiht_amd.batch import BatchCodec, Pipeline
    bc = BatchCodec.__new__(BatchCodec)
    bc.c, bc.H, bc.W = 3, 8, 10
    with pytest.raises(ValueError):  # wrong dtype / ndim / shape
        bc.encode_u16(np.zeros((2, 3, 8, 10), np.uint8))
    with pytest.raises(ValueError):
        bc.encode_u16(np.zeros((3, 8, 10), np.uint16))
    with pytest.raises(ValueError):
        bc.encode_u16(np.zeros((2, 3, 8, 12), np.uint16))
    dense = (3 * 8 * 10 * 2, 8 * 10 * 2, 10 * 2, 2)
    with pytest.raises(ValueError):  # odd byte stride
        bc.encode_device_u16(0x1000, 2, 0, 0, 0, strides=(481, 160, 20, 2))
    with pytest.raises(ValueError):  # unaligned base
        bc.encode_device_u16(0x1001, 2, 0, 0, 0, strides=dense)
    with pytest.raises(ValueError):  # an output view that overlaps itself: channels one byte pair apart, pixels two
        bc.decode_device_u16(0, 0, 0, 2, 0x1000, strides=(480, 2, 40, 4))
    with pytest.raises(ValueError):
        bc.decode_device_u16(0, 0, 0, 2, 0x1001, strides=dense)
    pl = Pipeline.__new__(Pipeline)
    pl.codec, pl.B, pl.handle = bc, 2, None
    with pytest.raises(ValueError):
        pl.submit_u16(0x1000, 0, 0, 0, 0x2000, in_strides=(481, 160, 20, 2))
    with pytest.raises(ValueError):
        pl.submit_u16(0x1000, 0, 0, 0, 0x2000, out_strides=(480, 2, 40, 4))
    with pytest.raises(ValueError):
        pl.submit_u16(0x1000, 0, 0, 0, 0x2001)


def test_u16_view_rule(no_context):
    from spiht_amd.spiht_wrapper import check_u16_view, check_u8_view
    B, c, H, W = 2, 3, 5, 7
    shape = (B, c, H, W)
    # planar CHW, interleaved HWC (sc = 2, sw = 2c), 16-bit RGBA (sw = 8) with a padded row pitch: output and input
    for st in [(2 * c * H * W, 2 * H * W, 2 * W, 2), (2 * H * W * c, 2, 2 * W * c, 2 * c), (H * 80, 2, 80, 8),
               (H * 80 + 6, 2, 80, 8)]:
        check_u16_view(shape, st, True)
        check_u16_view(shape, st, False)
    # numpy's own strides, as they are: planar, interleaved, RGBA, and slices of them
    planar = np.zeros(shape, np.uint16)
    hwc = np.zeros((B, H, W, c), np.uint16).transpose(0, 3, 1, 2)
    rgba = np.zeros((B, H, W, 4), np.uint16)[..., :3].transpose(0, 3, 1, 2)
    wide = np.zeros((B, c, 2 * H, 2 * W + 3), np.uint16)
    for a in (planar, hwc, rgba, wide[:, :, ::2, 1:W + 1], wide[:, :, H:, ::2][..., :W], wide[1:, :, :H, :W]):
        assert a.shape[1:] == (c, H, W)
        check_u16_view(a.shape, a.strides, True)
        check_u16_view(a.shape, a.strides, False)
    assert rgba.strides[1:] == (2, W * 8, 8)
    # odd strides: never, read or written
    for st in [(2 * c * H * W + 1, 2 * H * W, 2 * W, 2), (2 * c * H * W, 2 * H * W + 1, 2 * W, 2), (2 * c * H * W, 2 * H * W, 2 * W + 1, 2),
               (2 * c * H * W, 2 * H * W, 2 * W, 1), (2 * c * H * W, 2 * H * W, 2 * W, 3)]:
        for out in (False, True):
            with pytest.raises(ValueError):
                check_u16_view(shape, st, out)
    # overlapping output views: the element's two bytes count
    for st in [(0, 2 * H * W, 2 * W, 2),                   # every picture on the same bytes
               (2 * c * H * W, 2, 2 * W, 2),               # channels over columns
               (2 * c * H * W, 2 * H * W, 2 * (W - 1), 2),   # rows over rows
               (2 * H * W * c, 2, 2 * W * c, 4)]:            # pixels of three channels two samples apart
        with pytest.raises(ValueError):
            check_u16_view(shape, st, True)
        check_u16_view(shape, st, False)  # (a view that is only read may repeat itself)
    # what the 8-bit rule lets through one byte too early: samples 1 byte apart would share a byte (and are odd)
    check_u8_view((1, 1, 1, W), (0, 0, 0, 1), True)
    with pytest.raises(ValueError):
        check_u16_view((1, 1, 1, W), (0, 0, 0, 1), True)
    # rows that start on the last sample of the row before: 2 * (W - 1) steps onto it, 2 * W steps past it
    with pytest.raises(ValueError):
        check_u16_view((1, 1, H, W), (0, 0, 2 * (W - 1), 2), True)
    check_u16_view((1, 1, H, W), (0, 0, 2 * W, 2), True)
    with pytest.raises(ValueError):
        check_u16_view(shape, (2 * c * H * W, 2 * H * W, 2 * W, -2), False)
    with pytest.raises(ValueError):
        check_u16_view(shape, (2 * c * H * W, 2 * H * W, 2 * W), True)
    # a dimension of extent one does not step anywhere
    check_u16_view((1, 3, H, W), (0, 2, W * 6, 6), True)
    # the 8-bit rule is what it was: odd strides and one-byte steps
    check_u8_view(shape, (H * W * c, 1, W * c, c), True)


def test_u16_byte_order_and_negative_strides_are_copied():
    """the picture handed to the library is native and has non-negative strides, and holds the same values"""
    import spiht_amd
    from spiht_amd.spiht_wrapper import _int_picture
    s = spiht_amd.SpihtSettings()
    rng = np.random.default_rng(5)
    a = rng.integers(0, 65536, (3, 6, 9)).astype(np.uint16)
    other = a.astype(a.dtype.newbyteorder("S"))
    assert not other.dtype.isnative and other.dtype.itemsize == 2 and np.array_equal(other, a)
    for v in (other, a[:, ::-1], a[:, :, ::-1], other[:, ::-1]):
        p = _int_picture(v, s, np.uint16, "encode_image_u16")
        assert p.dtype.isnative and p.dtype == np.uint16 and min(p.strides) > 0 and np.array_equal(p, v)
        assert p.tobytes() == np.ascontiguousarray(v).astype("=u2").tobytes()
    assert _int_picture(a, s, np.uint16, "encode_image_u16") is a  # (nothing to copy)


def test_u16_sample_value_is_the_quotient_for_every_value():
    """A proof of the algorithm of dwt_device.h's px16_value, restated here, not a run of the device code (which the GPU parity
    tests cover): q = k * (1/65535), corrected once by its residual through two fused multiply-adds, is the IEEE quotient
    k / 65535.0 (numpy's P / 65535) for all 65536 values -- and the product alone is not (88 of them differ).  fma
    emulated exactly: the exact sum, rounded once."""
    from fractions import Fraction

    def fma(a, b, c):
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    r = 1.0 / 65535.0
    ks = np.arange(65536, dtype=np.uint16)
    ref = ks / 65535
    assert ref.dtype == np.float64
    product_misses = 0
    for k in range(65536):
        x = float(k)
        q = x * r
        product_misses += q != x / 65535.0
        assert fma(fma(-q, 65535.0, x), r, q) == x / 65535.0 == ref[k], k
        assert x / 65535.0 == float(Fraction(k, 65535)), k  # (the quotient correctly rounded: what the formula is held to)
    assert product_misses == 88


def test_u16_store_returns_every_value():
    """dwt_device.h's px16_store_value, restated: (uint16)(clip(v, 0, 1) * 65535.0), truncated, gives k back for v = k / 65535.0
    for all 65536 k -- a picture that survives the codec unquantised survives the store -- and clips and drops NaN."""
    def store(v):
        c = min(max(v, 0.0), 1.0) if v == v else 0.0  # (fmax / fmin return the number of a NaN pair: fmax(NaN, 0) = 0)
        return int(c * 65535.0)
    for k in range(65536):
        assert store(k / 65535.0) == k, k
    ks = np.arange(65536, dtype=np.uint16)
    assert np.array_equal((np.clip(ks / 65535, 0, 1) * 65535.0).astype(np.uint16), ks)
    assert store(-0.14) == 0 and store(1.234) == 65535 and store(float("nan")) == 0 and store(float("inf")) == 65535
    assert store(0.5) == 32767 and store(np.nextafter(1.0, 0.0)) == 65534  # truncated, not rounded
