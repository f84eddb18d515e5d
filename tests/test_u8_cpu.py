"""CPU tests of the 8-bit pixel path (encode_image_u8 / decode_image_u8, BatchCodec.*_u8, Pipeline.submit_u8): the names
exist and the argument checks raise before any GPU context is needed.  No device calls."""
import numpy as np
import pytest


def test_u8_names_exist():
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec, Pipeline
    assert callable(spiht_amd.encode_image_u8) and callable(spiht_amd.decode_image_u8)
    for name in ("encode_u8", "decode_u8", "encode_device_u8", "decode_device_u8"):
        assert callable(getattr(BatchCodec, name))
    assert callable(Pipeline.submit_u8)
    L = _lib.lib()
    for s in ("spiht_encode_image_batch_u8", "spiht_decode_image_batch_u8", "spiht_encode_image_host_u8",
              "spiht_decode_image_host_u8", "spiht_pipeline_submit_u8"):
        assert hasattr(L, s) and s in _lib.SYMBOLS
    # the reference's surface of the alias package stays as it is
    import spiht
    assert not hasattr(spiht, "encode_image_u8")


@pytest.fixture
def no_context(monkeypatch):
    """any attempt to create a GPU context fails the test"""
    from spiht_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a context was created before the argument check")
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib.Context, "__init__", boom)


def test_encode_image_u8_argument_errors(no_context):
    import spiht_amd
    s = spiht_amd.SpihtSettings()
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u8(np.zeros((3, 8, 8), np.float64), s)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u8(np.zeros((3, 8, 8), np.uint16), s)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u8(np.zeros((8, 8), np.uint8), s)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u8(np.zeros((1, 3, 8, 8), np.uint8), s)
    with pytest.raises(ValueError):  # a colour model needs three channels
        spiht_amd.encode_image_u8(np.zeros((2, 8, 8), np.uint8), spiht_amd.SpihtSettings(color_model="IPT"))
    with pytest.raises(ValueError):
        spiht_amd.encode_image_u8(np.zeros((8, 8, 4), np.uint8), spiht_amd.SpihtSettings(color_model="IPT"),
                                  channels_last=True)


def test_decode_image_u8_colour_needs_three_channels(no_context):
    import spiht_amd
    r = spiht_amd.EncodingResult(b"\x00" * 8, 8, 8, 2, 3, None)
    with pytest.raises(ValueError):
        spiht_amd.decode_image_u8(r, spiht_amd.SpihtSettings(color_model="IPT"))


def test_u8_view_rule(no_context):
    from spiht_amd.spiht_wrapper import check_u8_view
    B, c, H, W = 2, 3, 5, 7
    shape = (B, c, H, W)
    # dense CHW, HWC, RGBA with a padded row pitch: fine for output and input
    for st in [(c * H * W, H * W, W, 1), (H * W * c, 1, W * c, c), (H * 40, 1, 40, 4), (H * 40 + 3, 1, 40, 4)]:
        check_u8_view(shape, st, True)
        check_u8_view(shape, st, False)
    # overlapping output views
    for st in [(0, H * W, W, 1),            # every picture on the same bytes
               (c * H * W, 1, W, 1),        # channels over columns
               (c * H * W, H * W, W - 1, 1),  # rows over rows
               (H * W * c, 1, W * c, 2)]:     # pixels of three channels two bytes apart
        with pytest.raises(ValueError):
            check_u8_view(shape, st, True)
        check_u8_view(shape, st, False)  # (a view that is only read may repeat itself)
    with pytest.raises(ValueError):
        check_u8_view(shape, (c * H * W, H * W, W, -1), False)
    with pytest.raises(ValueError):
        check_u8_view(shape, (c * H * W, H * W, W), True)
    # a dimension of extent one does not step anywhere
    check_u8_view((1, 3, H, W), (0, 1, W * 3, 3), True)


def test_u8_sample_value_is_the_quotient_for_every_byte():
    """A proof of the algorithm of dwt_device.h's px8_value, restated here, not a run of the device code (which the GPU parity
    tests cover): q = k * (1/255), corrected once by its residual through two fused multiply-adds, is the IEEE quotient
    k / 255.0 (numpy's P / 255) for all 256 bytes.  fma emulated exactly: the exact sum, rounded once."""
    from fractions import Fraction

    def fma(a, b, c):
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    r = 1.0 / 255.0
    for k in range(256):
        x = float(k)
        q = x * r
        assert fma(fma(-q, 255.0, x), r, q) == x / 255.0 == np.float64(np.uint8(k)) / 255, k
