"""CPU tests of the batched decode_with_metadata's boundary: argument errors raised before any context is created, the C
entry point's NULL checks, and the sub-band boxes BatchCodec hands to it.  No device needed."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture
def no_context(monkeypatch):
    """any attempt to create a context (i.e. to reach the device) fails the test"""
    from spiht_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "default_context", refuse)
    monkeypatch.setattr(_lib, "Context", refuse)


TOP = [(0, 2), (0, 2)]
OTHER = [[[(2, 4), (0, 2)], [(0, 2), (2, 4)], [(2, 4), (2, 4)]]]


def test_argument_errors_before_any_context(no_context):
    from spiht_amd.spiht import PanicException, decode_with_metadata_batch as f
    with pytest.raises(ValueError):
        f([b"ab", b"c"], [3], 1, 4, 4, 2, 2, TOP, OTHER)      # a max_n per stream
    with pytest.raises(TypeError):
        f(["ab"], [3], 1, 4, 4, 2, 2, TOP, OTHER)             # a str is not a byte string
    with pytest.raises(OverflowError):
        f([b"ab"], [256], 1, 4, 4, 2, 2, TOP, OTHER)          # n is a u8
    with pytest.raises(OverflowError):
        f([b"ab"], [3], -1, 4, 4, 2, 2, TOP, OTHER)
    with pytest.raises(TypeError):
        f([b"ab"], [3.0], 1, 4, 4, 2, 2, TOP, OTHER)
    with pytest.raises(PanicException):
        f([b"ab"], [3], 1, 4, 4, 1, 2, TOP, OTHER)            # assert!(ll_h > 1)
    with pytest.raises(PanicException):
        f([b"ab"], [3], 1, 4, 4, 2, 2, TOP[:1], OTHER)        # top_slice[1]
    with pytest.raises(PanicException):
        f([b"ab"], [3], 1, 4, 4, 2, 2, TOP, [OTHER[0][:2]])   # three filters per level
    with pytest.raises(ValueError):
        f([b"ab"], [3], 1, 4, 4, 2, 2, [(0, 2, 3), (0, 2)], OTHER)
    with pytest.raises(PanicException):
        f([b"ab"], [3], 1, 0, 4, 2, 2, TOP, OTHER)            # rec_arr[(0,0,0)]
    # what needs no device: c == 0 and an empty batch
    rec, metas = f([b"ab", b""], [3, 0], 0, 4, 4, 2, 2, TOP, OTHER)
    assert rec.shape == (2, 0, 4, 4) and [m.shape for m in metas] == [(17, 8), (1, 8)]
    rec, metas = f([], [], 1, 4, 4, 2, 2, TOP, OTHER)
    assert rec.shape == (0, 1, 4, 4) and metas == []


def test_c_entry_point_refuses_null():
    from spiht_amd import _lib
    L = _lib.lib()
    top = np.array([0, 2, 0, 2], dtype=np.int64)
    oth = np.array([2, 4, 0, 2, 0, 2, 2, 4, 2, 4, 2, 4], dtype=np.int64)
    p = C.c_void_p(16)  # never dereferenced: the checks come first
    tp, op = C.c_void_p(top.ctypes.data), C.c_void_p(oth.ctypes.data)
    assert L.spiht_decode_with_metadata_batch_i32(None, p, 4, p, p, 1, 1, 4, 4, 2, 2, tp, op, 1, None, p, 33) == _lib.ERR_ARG
    assert L.spiht_decode_with_metadata_batch_i32(None, p, 4, p, p, 0, 1, 4, 4, 2, 2, tp, op, 1, None, p, 33) == _lib.ERR_ARG


def test_metadata_boxes_are_the_wrappers_slices():
    """the boxes decode_rec_array and BatchCodec hand over are the sub-bands of get_slices_and_h_w"""
    from spiht_amd.spiht_wrapper import SpihtSettings, _geometry, _metadata_boxes, _wavelet_mode_ids, get_slices_and_h_w
    for H, W, s, level in ((72, 100, SpihtSettings(), None), (37, 53, SpihtSettings(wavelet="bior4.4"), 2),
                           (1080, 1920, SpihtSettings(), None), (64, 48, SpihtSettings(mode="periodization"), 3)):
        wid, mid = _wavelet_mode_ids(s)
        g = _geometry(H, W, wid, level, mid)
        top, other = _metadata_boxes(H, W, s, g)
        slices, enc_h, enc_w = get_slices_and_h_w(H, W, s, level)
        assert (enc_h, enc_w) == (g["enc_h"], g["enc_w"])
        assert top == [(0, slices[0][1].stop), (0, slices[0][2].stop)]
        want = [[[(sl[k][1].start or 0, sl[k][1].stop), (sl[k][2].start or 0, sl[k][2].stop)] for k in ("da", "ad", "dd")]
                for sl in slices[1:]]
        assert other == want
