"""Reduced-resolution decode, the part that needs no GPU: the contract stated through the CPU oracle reproduces PyWavelets
bit for bit (tests/golden/reduced_pywt.npz), and the arithmetic of the C ABI (spiht_reduced_shape, the error codes, the
exports) and of the Python boundary (reduced_shape, the crop window) is the oracle's geometry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["spiht_reduced_shape"] + ["spiht_%s_reduced_%s_%s" % (a, b, k)
                                         for a, b in (("dequant_idwt", "batch"), ("decode_image", "batch"), ("decode_image", "host"))
                                         for k in ("f64", "u8", "u16")]


def oracle_reduced(oracle, D, H, W, wavelet, L, mode, k):
    """The contract in the oracle's words: the top-left corner of the coefficient array is the coefficient array of the
    hs[k] x ws[k] picture at L - k levels; its inverse transform, with the DC gain 2^k taken out.  D float64 [c, enc_h, enc_w]
    (dequantised) -> R_k.  (The level goes in explicitly: None would re-derive it from the small picture.)"""
    g = oracle.geometry(H, W, wavelet, L, mode)
    hk, wk = g["hs"][k], g["ws"][k]
    gk = oracle.geometry(hk, wk, wavelet, L - k, mode)
    assert gk["hs"] == g["hs"][k:] and gk["ws"] == g["ws"][k:]
    sub = np.ascontiguousarray(D[:, :gk["enc_h"], :gk["enc_w"]])
    return oracle.waverec2_array(sub, hk, wk, wavelet, L - k, mode) * 2.0 ** -k


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def golden_cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "reduced_pywt.npz"))
    for i in range(int(z["ncases"])):
        p = "c%d_" % i
        mults = z[p + "mults"].tolist() or None
        H, W = [int(v) for v in z[p + "hw"]]
        L = int(z[p + "level"])
        yield dict(i=i, rec=z[p + "rec"], wavelet=str(z[p + "wavelet"]), mode=str(z[p + "mode"]), L=L, H=H, W=W, q=float(z[p + "q"]),
                   mults=mults, want=[z[p + "r%d" % k] for k in range(L)])


def test_oracle_form_reproduces_pywavelets(oracle):
    """every k < L of every golden case: shape and bits of waverec2(coeffs[:L - k + 1]) * 2^-k"""
    n, seen = 0, set()
    for cs in golden_cases():
        D = oracle.dequantize(cs["rec"], cs["q"], cs["mults"])
        for k in range(cs["L"]):
            got = oracle_reduced(oracle, D, cs["H"], cs["W"], cs["wavelet"], cs["L"], cs["mode"], k)
            assert same_bits(got, cs["want"][k] * 2.0 ** -k), (cs["i"], cs["wavelet"], cs["mode"], k)
            n += 1
        seen.add((cs["wavelet"], cs["mode"]))
    assert n >= 40 and ("db11", "reflect") in seen and any(m == "periodization" for _, m in seen)


def _shape(L, H, W, wid, mid, level, reduce):
    lv = C.c_int()
    v = [C.c_int64() for _ in range(8)]
    st = L.spiht_reduced_shape(H, W, wid, mid, level, reduce, C.byref(lv), *[C.byref(t) for t in v])
    return st, lv.value, [t.value for t in v]


def test_reduced_shape_is_the_oracles_geometry(oracle):
    """filter lengths 2 .. 20 and a long one, reflect and periodization, odd and even sizes, levels above dwt_max_level,
    every k: rec = the shape of the oracle's reduced inverse, pic = the band size, the window centred in it"""
    from spiht_amd import _lib
    L = _lib.lib()
    names = ["haar", "db2", "bior2.2", "db4", "bior4.4", "db6", "db7", "db8", "bior6.8", "db10", "db11"]
    n = 0
    for name in names:
        F = len(oracle.wavelet_filters(name)[0])
        wid = L.spiht_wavelet_id(name.encode())
        assert L.spiht_wavelet_taps(wid) == F
        for mode in ("reflect", "periodization"):
            mid = L.spiht_mode_id(mode.encode())
            for H, W in ((37, 64), (64, 51), (23, 23)):
                for level in (1, 3, 5):
                    g = oracle.geometry(H, W, name, level, mode)
                    Fg = 2 if mode == "periodization" else F
                    for k in range(level + 1):
                        st, lv, (rh, rw, ph, pw, oy, ox, ih, iw) = _shape(L, H, W, wid, mid, level, k)
                        assert st == _lib.OK and lv == level
                        assert (ph, pw) == (g["hs"][k], g["ws"][k])
                        if k < level:
                            assert (rh, rw) == (2 * g["hs"][k + 1] - Fg + 2, 2 * g["ws"][k + 1] - Fg + 2)
                        else:
                            assert (rh, rw) == (g["ll_h"], g["ll_w"])
                        assert (ih, iw) == (-(-H // 2 ** k), -(-W // 2 ** k))
                        assert (oy, ox) == ((0, 0) if mode == "periodization" else ((ph - ih) // 2, (pw - iw) // 2))
                        assert 0 <= oy and oy + ih <= min(ph, rh) and 0 <= ox and ox + iw <= min(pw, rw)
                        n += 1
                    if name in ("bior4.4", "db11") and (H, W) == (37, 64) and level == 3:
                        # ... and the shapes are those of the arrays the oracle returns
                        D = np.zeros((1, g["enc_h"], g["enc_w"]))
                        for k in range(level):
                            assert oracle_reduced(oracle, D, H, W, name, level, mode, k).shape[1:] == tuple(_shape(L, H, W, wid, mid, level, k)[2][:2])
    assert n > 500
    # the level the library picks when none is given
    wid = L.spiht_wavelet_id(b"bior2.2")
    g = oracle.geometry(96, 160, "bior2.2", None)
    st, lv, v = _shape(L, 96, 160, wid, 0, -1, g["level"])
    assert st == _lib.OK and lv == g["level"] and tuple(v[:2]) == (g["ll_h"], g["ll_w"])


def test_error_codes():
    """reduce outside 0 .. L, unknown wavelet / mode: SPIHT_ERR_ARG, from the call that needs no device and -- before a
    context or a pointer is looked at -- from the ones that do"""
    from spiht_amd import _lib
    L = _lib.lib()
    wid = L.spiht_wavelet_id(b"bior2.2")
    for reduce in (-1, 4, 33, 1 << 20):
        assert _shape(L, 64, 64, wid, 0, 3, reduce)[0] == _lib.ERR_ARG
    assert _shape(L, 64, 64, wid, 0, 3, 3)[0] == _lib.OK
    assert _shape(L, 64, 64, -1, 0, 3, 1)[0] == _lib.ERR_ARG and _shape(L, 64, 64, wid, 9, 3, 1)[0] == _lib.ERR_ARG
    assert _shape(L, 0, 64, wid, 0, 3, 1)[0] == _lib.ERR_ARG
    assert L.spiht_reduced_shape(64, 64, wid, 0, 3, 1, None, *[None] * 8) == _lib.OK  # (every output pointer may be NULL)
    # the calls that take a device refuse a reduce out of range before they look at the context or at a pointer
    bogus = C.c_void_p(256)
    st = np.array([64 * 64 * 3, 64 * 64, 64, 1], np.int64)
    for fn in (L.spiht_dequant_idwt_reduced_batch_u8, L.spiht_dequant_idwt_reduced_batch_u16):
        assert fn(None, bogus, 1, 3, 64, 64, wid, 0, 3, 50.0, None, bogus, C.c_void_p(st.ctypes.data), 4) == _lib.ERR_ARG
        assert fn(None, bogus, 1, 3, 64, 64, wid, 0, 3, 50.0, None, bogus, C.c_void_p(st.ctypes.data), -1) == _lib.ERR_ARG
    for fn in (L.spiht_decode_image_reduced_host_u8, L.spiht_decode_image_reduced_host_u16):
        assert fn(None, bogus, 4, 3, 3, 64, 64, wid, 0, 3, 50.0, None, bogus, None, 4) == _lib.ERR_ARG


def test_header_declares_and_library_exports_the_new_calls():
    from spiht_amd import _lib
    src = open(os.path.join(ROOT, "include", "spiht_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(spiht_[a-z0-9_]+)\s*\(", src))
    L = _lib.lib()
    assert len(NEW_SYMBOLS) == 10
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
        assert re.search(r"\bint\s+reduce\b[^;]*;", src[src.index(s + "("):src.index(s + "(") + 900]), s
    assert L.spiht_abi_version() == 2


def test_python_reduced_shape_and_crop_window():
    import spiht_amd
    from spiht_amd import spiht_wrapper as sw
    s = spiht_amd.SpihtSettings(wavelet="bior4.4")
    rs = spiht_amd.reduced_shape(61, 77, s, 3, 1)
    # bior4.4 (10 taps): bands 35 x 43, 22 x 26, 15 x 17
    assert rs == dict(level=3, rec_h=36, rec_w=44, pic_h=35, pic_w=43, off_y=2, off_x=2, in_h=31, in_w=39)
    assert spiht_amd.reduced_shape(61, 77, s, 3, 3)["rec_h"] == 15 and spiht_amd.reduced_shape(61, 77, s, 3, 0)["rec_h"] == 62
    per = spiht_amd.reduced_shape(53, 70, spiht_amd.SpihtSettings(wavelet="db2", mode="periodization"), 3, 2)
    assert (per["pic_h"], per["pic_w"], per["in_h"], per["in_w"], per["off_y"], per["off_x"]) == (14, 18, 14, 18, 0, 0)
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            spiht_amd.reduced_shape(61, 77, s, 3, bad)
    with pytest.raises(TypeError):
        spiht_amd.reduced_shape(61, 77, s, 3, 1.0)
    # the window is a view of the picture, channels first or last
    pic = np.arange(3 * 36 * 44, dtype=np.float64).reshape(3, 36, 44)
    win = sw._crop_window(pic, rs, True)
    assert win.shape == (3, 31, 39) and win.base is not None and np.shares_memory(win, pic) and win[0, 0, 0] == pic[0, 2, 2]
    assert sw._crop_window(pic, rs, False) is pic
    hwc = np.zeros((35, 43, 3), np.uint8)
    assert sw._crop_window(hwc, rs, True, channels_last=True).shape == (31, 39, 3)
    import spiht
    assert spiht.decode_image_reduced is spiht_amd.decode_image_reduced and spiht.reduced_shape is spiht_amd.reduced_shape
