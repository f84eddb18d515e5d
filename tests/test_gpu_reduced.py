"""Reduced-resolution decode on the GPU: pictures at 1/2^k size straight from a coefficient array or a stream, against the
CPU oracle's statement of the contract (tests/test_reduced_cpu.py: oracle_reduced, which reproduces PyWavelets'
waverec2(coeffs[:L - k + 1]) bit for bit).  Every comparison is equality of bits, except where a colour change is held to
the oracle's own power function.  The shapes are the kernels' seams (tests/dwt_sweep_tables.py), one pyramid level up."""
import ctypes as C
import os

import numpy as np
import pytest

import dwt_sweep_tables as T
from conftest import synth_image
from test_gpu_dwt_sweep import DTYPE, TO_INT, _Bufs, _mults_ptr, device_colour, int_layout, same_bits, untouched
from test_gpu_u8 import CONFIGS, settings, to_u8, u8_image
from test_gpu_u16 import to_u16
from test_reduced_cpu import oracle_reduced

pytestmark = pytest.mark.gpu
vp = C.c_void_p
KINDS = ["f64", "u8", "u16"]


# ---- the contract, from the oracle -------------------------------------------------------------------------------------------
def want_reduced(oracle, rec, H, W, wavelet, L, mode, k, q, mults):
    """R_k of an int32 array [c, enc_h, enc_w]; k == L: the dequantised root block"""
    D = oracle.dequantize(rec, q, mults)
    if k == L:
        g = oracle.geometry(H, W, wavelet, L, mode)
        return np.ascontiguousarray(D[:, :g["ll_h"], :g["ll_w"]]) * 2.0 ** -L
    return oracle_reduced(oracle, D, H, W, wavelet, L, mode, k)


def want_int(kind, R, hk, wk):
    """the contract's clip, scale, truncate and crop to the band size"""
    return TO_INT[kind](R, hk, wk)


def picture_for(rec_hw, F, k, integer, i):
    """(H, W) of a picture whose reduced picture at k has rec_hw samples (2 band - F + 2 of level k + 1).  Integer kinds: odd
    hs[k], ws[k] (one less than the even rec), so that the crop of the extra row and column falls on the seam; float64:
    odd and even take turns with the case number i.  Each level further down takes the odd or the even length in turn."""
    out = []
    for axis, n in enumerate(rec_hw):
        n -= 1 if integer else (i >> axis) & 1
        for j in range(k):
            n = 2 * n - F + 2 - (j & 1)
            assert n >= 1
        out.append(n)
    return tuple(out)


def array_case(oracle, wavelet, mode, H, W, level, seed, mults, c):
    """a thinned-out copy of the oracle's quantised array of a picture stretched to [-0.15, 1.15]: the clip works on both sides"""
    img = synth_image(seed, c, H, W) * 1.3 - 0.15
    arr, _ = oracle.wavedec2_array(img, wavelet, mode, level)
    return T.thin_out(oracle.quantize(arr, T.Q, mults), seed)


def shape_of(L, H, W, wid, mid, level, k):
    lv = C.c_int()
    v = [C.c_int64() for _ in range(8)]
    assert L.spiht_reduced_shape(H, W, wid, mid, level, k, C.byref(lv), *[C.byref(t) for t in v]) == 0
    return [t.value for t in v]  # rec_h, rec_w, pic_h, pic_w, off_y, off_x, in_h, in_w


def gpu_reduced(kind, rec, H, W, wavelet, mode, level, q, mults, k, layouts=("planar", "rgba")):
    """rec int32 [B, c, enc_h, enc_w] -> {layout: pictures} through spiht_dequant_idwt_reduced_batch_f64 / _u8 / _u16.  "f64":
    one dense result [B, c, rec_h, rec_w]; integer kinds (c == 3): [B, 3, pic_h, pic_w] out of a planar buffer and a padded
    RGBA one whose other bytes must keep their sentinel."""
    rec = np.ascontiguousarray(rec, np.int32)
    B, c = rec.shape[:2]
    with _Bufs() as d:
        L = d.L
        wid, mid = L.spiht_wavelet_id(wavelet.encode()), L.spiht_mode_id(mode.encode())
        rh, rw, ph, pw = shape_of(L, H, W, wid, mid, level, k)[:4]
        m, mp = _mults_ptr(mults)
        d_rec = d.put(rec)
        if kind == "f64":
            out = np.empty((B, c, rh, rw), np.float64)
            d_out = d.new(out.nbytes, 0xFF)
            d.check(L.spiht_dequant_idwt_reduced_batch_f64(d.ctx.handle, vp(d_rec), B, c, H, W, wid, mid, level, float(q), mp,
                                                           vp(d_out), k))
            d.ctx.download(out, d_out)
            return {"dense": out}
        assert c == 3
        fn = L.spiht_dequant_idwt_reduced_batch_u8 if kind == "u8" else L.spiht_dequant_idwt_reduced_batch_u16
        res = {}
        for name in layouts:
            buf, strides, view = int_layout(name, kind, B, ph, pw)
            st = None if strides is None else np.array(strides, np.int64)
            d_out = d.put(buf)
            d.check(fn(d.ctx.handle, vp(d_rec), B, c, H, W, wid, mid, level, float(q), mp, vp(d_out),
                       None if st is None else vp(st.ctypes.data), k))
            d.ctx.download(buf, d_out)
            assert untouched(name, kind, buf, pw), (name, "bytes outside the pixels were written")
            res[name] = np.ascontiguousarray(view)
        return res


def _F(oracle, wavelet):
    return len(oracle.wavelet_filters(wavelet)[0])


# ---- 1. the transform alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wavelet", T.INVERSE_MASK_WAVELETS)
def test_reduced_inverse_tiled(oracle, wavelet, kind):
    """k_idwt_level as the final level at level k + 1: L = 3, k = 1 and 2 (= L - 1: the final level is also the coarsest, its
    approximation out of the packed array) at the four seam sizes of the REDUCED picture, k = L (the root block: k_ll_to_pic)
    once; two pictures of two (integer kinds: three) channels, per-channel scales on every other case"""
    F, L = _F(oracle, wavelet), 3
    integer = kind != "f64"
    c = 3 if integer else 2
    n = 0
    for k in (1, 2, 3):
        for i, rec_hw in enumerate(T.INV_REC if k < L else T.INV_REC[2:3]):
            if k < L:
                H, W = picture_for(rec_hw, F, k, integer, i)
            else:
                H, W = picture_for(T.INV_REC[2], F, 1, integer, i)
            g = oracle.geometry(H, W, wavelet, L)
            hk, wk = g["hs"][k], g["ws"][k]
            mults = T.scales_for(i + k, c)
            rec = np.stack([array_case(oracle, wavelet, "reflect", H, W, L, 700 + i + 9 * b + 31 * k, mults, c) for b in range(2)])
            want = np.stack([want_reduced(oracle, r, H, W, wavelet, L, "reflect", k, T.Q, mults) for r in rec])
            if k < L:
                assert want.shape[2:] == rec_hw
                assert hk % 2 == 1 and wk % 2 == 1 or not integer
            else:
                assert want.shape[2:] == (g["ll_h"], g["ll_w"]) == (hk, wk)
            # (R_k has the picture's own range -- the 2^-k took the band's gain out: the clip works on both sides)
            assert want.min() < 0.0 and want.max() > 1.0, (k, H, W, float(want.min()), float(want.max()))
            if integer:
                want = np.stack([want_int(kind, w, hk, wk) for w in want])
            got = gpu_reduced(kind, rec, H, W, wavelet, "reflect", L, T.Q, mults, k)
            for name, px in got.items():
                assert same_bits(px, want), (wavelet, kind, k, H, W, name, np.argwhere(px != want)[:4].tolist())
            n += 1
    assert n == 9


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wavelet,mode", [("db11", "reflect"), ("bior4.4", "periodization"), ("db2", "periodization"),
                                          ("db11", "periodization")])
def test_reduced_inverse_two_pass(oracle, wavelet, mode, kind):
    """periodization and a filter longer than the tiled kernels take: k_idwt_axis_per at level k + 1, the conversion pass of
    the integer kinds behind it; every k <= L = 3"""
    L, c = 3, 3
    H, W = 101, 75
    g = oracle.geometry(H, W, wavelet, L, mode)
    for k in range(L + 1):
        mults = T.scales_for(k, c)
        rec = np.stack([array_case(oracle, wavelet, mode, H, W, L, 800 + k + 9 * b, mults, c) for b in range(2)])
        want = np.stack([want_reduced(oracle, r, H, W, wavelet, L, mode, k, T.Q, mults) for r in rec])
        if kind != "f64":
            want = np.stack([want_int(kind, w, g["hs"][k], g["ws"][k]) for w in want])
        for name, px in gpu_reduced(kind, rec, H, W, wavelet, mode, L, T.Q, mults, k).items():
            assert same_bits(px, want), (wavelet, mode, kind, k, name, np.argwhere(px != want)[:4].tolist())
        if k == 0 and kind == "f64":  # ... and reduce 0 is the full-size call
            full = oracle.waverec2_array(oracle.dequantize(rec[0], T.Q, mults), H, W, wavelet, L, mode)
            assert same_bits(want[0], full)


# ---- 2. the persistent kernel as the final level --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wavelet", ["bior4.4", "db2"])
def test_reduced_persistent_final_level(oracle, wavelet, kind):
    """k = 1, 1667 three-channel pictures whose REDUCED picture is 26 x 130 (2 x 2 tiles): 20 004 tiles at level 2, so
    launch_idwt_FM takes k_idwt_level_pf for the picture store of every pixel kind -- with L = 3 (the plain variant) and
    with L = 2 = k + 1 (FIRST: the coarsest level stores the picture).  8 distinct oracle-checked arrays, repeated."""
    F = _F(oracle, wavelet)
    integer = kind != "f64"
    k = 1
    H, W = picture_for(T.PF_REC, F, k, integer, 0)
    idx = np.arange(T.PF_PICTURES) % T.PF_DISTINCT
    for L, mults in ((3, None), (2, [1.0, 0.75, 2.0])):
        g = oracle.geometry(H, W, wavelet, L)
        recs = np.stack([array_case(oracle, wavelet, "reflect", H, W, L, 900 + j, mults, 3) for j in range(T.PF_DISTINCT)])
        wants = np.stack([want_reduced(oracle, r, H, W, wavelet, L, "reflect", k, T.Q, mults) for r in recs])
        assert wants.shape[2:] == T.PF_REC
        assert T.PF_PICTURES * 3 * T.tiles(T.PF_REC[0], T.INV_TH) * T.tiles(T.PF_REC[1], T.INV_TW) >= T.PF_MIN
        if integer:
            wants = np.stack([want_int(kind, w, g["hs"][k], g["ws"][k]) for w in wants])
        got = gpu_reduced(kind, recs[idx], H, W, wavelet, "reflect", L, T.Q, mults, k)
        for name, px in got.items():
            assert px.shape == (T.PF_PICTURES,) + wants.shape[1:]
            for j in range(T.PF_DISTINCT):
                part = px[j::T.PF_DISTINCT]
                assert same_bits(part, np.broadcast_to(wants[j], part.shape)), (wavelet, kind, L, name, j, np.argwhere(part != wants[j])[:4].tolist())


# ---- 3. colour -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wavelet,mode", [("bior2.2", "reflect"), ("bior4.4", "reflect"), ("db2", "periodization")])
def test_reduced_colour(oracle, wavelet, mode, kind):
    """Inside color_models.fused(ctx, "IPT"), k = 1, 2 and L = 3 (k = 2: the colour kernel is also the coarsest level; k = 3:
    the root block), reduced pictures that cross the colour kernel's tiles of 8 rows and 128 columns: the fused result
    equals the reduced decode without the colour model followed by the stand-alone colour kernel, in every bit, and that
    is the oracle's colour change of the oracle's R_k to within its power function (tests/test_gpu_image.py: 2e-14 for
    values of order one)."""
    from spiht_amd import _lib, color_models
    ctx = _lib.default_context()
    F, L = _F(oracle, wavelet), 3
    integer = kind != "f64"
    params = color_models._params("IPT", "RGB")
    for k in (1, 2, 3):
        if mode == "periodization":
            H, W = 2 ** k * 26 - 3, 2 ** k * 130 - 1
        else:
            H, W = picture_for(T.INV_REC[3] if k == 1 else T.INV_REC[2], F, min(k, 2), integer, k)
        g = oracle.geometry(H, W, wavelet, L, mode)
        hk, wk = g["hs"][k], g["ws"][k]
        mults = T.scales_for(k, 3)
        recs = []
        for b in range(2):
            rgb = synth_image(600 + k + 9 * b, 3, H, W) * 1.1 - 0.05
            arr, _ = oracle.wavedec2_array(color_models.convert(rgb, "RGB", "IPT"), wavelet, mode, L)
            recs.append(T.thin_out(oracle.quantize(arr, T.Q, mults), k + b))
        rec = np.stack(recs)
        ipt = np.stack([want_reduced(oracle, r, H, W, wavelet, L, mode, k, T.Q, mults) for r in rec])
        if k < L:
            assert ipt.shape[2] > 8 and ipt.shape[3] > 128
        plain = gpu_reduced("f64", rec, H, W, wavelet, mode, L, T.Q, mults, k)["dense"]
        assert same_bits(plain, ipt)
        want = device_colour(plain, "IPT", "RGB")
        twin = np.stack([oracle.color3(im, *params) for im in ipt])
        assert np.isfinite(want).all() and np.abs(want - twin).max() < 2e-14, float(np.abs(want - twin).max())
        if integer:
            want = np.stack([want_int(kind, w, hk, wk) for w in want])
        with color_models.fused(ctx, "IPT"):
            got = gpu_reduced(kind, rec, H, W, wavelet, mode, L, T.Q, mults, k)
        for name, px in got.items():
            assert same_bits(px, want), (wavelet, mode, kind, k, H, W, name, np.argwhere(px != want)[:4].tolist())


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def oracle_stream_reduced(oracle, enc, s, k):
    """the oracle's decode of a stream -> R_k, and the band size"""
    g = oracle.geometry(enc.h, enc.w, s.wavelet, enc.level, s.mode)
    rec = oracle.decode(enc.encoded_bytes, enc.max_n, enc.c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"])
    R = want_reduced(oracle, rec, enc.h, enc.w, s.wavelet, g["level"], s.mode, k, s.quantization_scale, s.per_channel_quant_scales)
    return R, g["hs"][k], g["ws"][k]


SMALL = [cfg for cfg in CONFIGS if cfg["H"] <= 96 and cfg["W"] <= 128]


@pytest.mark.parametrize("source", ["f64", "u8", "f32"])
@pytest.mark.parametrize("cfg", SMALL)
def test_decode_image_reduced_vs_oracle(oracle, cfg, source):
    import spiht_amd
    c, H, W = cfg["c"], cfg["H"], cfg["W"]
    s = settings(cfg)
    P = u8_image(2100 + H, c, H, W)
    if source == "u8":
        enc = spiht_amd.encode_image_u8(P, s, level=cfg["level"], max_bits=cfg["max_bits"])
    else:
        enc = spiht_amd.encode_image((P / 255).astype(np.float32 if source == "f32" else np.float64), s, level=cfg["level"],
                                     max_bits=cfg["max_bits"])
    L = oracle.geometry(H, W, s.wavelet, cfg["level"], s.mode)["level"]
    assert L >= 2
    # reduce 0: the full-size calls in every bit
    assert same_bits(spiht_amd.decode_image_reduced(enc, s, 0), spiht_amd.decode_image(enc, s))
    assert same_bits(spiht_amd.decode_image_reduced_u8(enc, s, 0), spiht_amd.decode_image_u8(enc, s))
    assert same_bits(spiht_amd.decode_image_reduced_u16(enc, s, 0, channels_last=True), spiht_amd.decode_image_u16(enc, s, channels_last=True))
    for k in range(L + 1):
        R, hk, wk = oracle_stream_reduced(oracle, enc, s, k)
        rs = spiht_amd.reduced_shape(H, W, s, cfg["level"], k)
        assert (rs["pic_h"], rs["pic_w"], rs["rec_h"], rs["rec_w"]) == (hk, wk) + R.shape[1:]
        got = spiht_amd.decode_image_reduced(enc, s, k)
        assert same_bits(got, R), (cfg, source, k, np.argwhere(got != R)[:4].tolist())
        ys, xs = slice(rs["off_y"], rs["off_y"] + rs["in_h"]), slice(rs["off_x"], rs["off_x"] + rs["in_w"])
        win = spiht_amd.decode_image_reduced(enc, s, k, crop=True)
        assert win.shape == (c, -(-H // 2 ** k), -(-W // 2 ** k)) and same_bits(win, R[:, ys, xs])
        u8 = spiht_amd.decode_image_reduced_u8(enc, s, k)
        assert u8.dtype == np.uint8 and same_bits(u8, to_u8(R, hk, wk)), (cfg, source, k)
        u16 = spiht_amd.decode_image_reduced_u16(enc, s, k)
        assert u16.dtype == np.uint16 and same_bits(u16, to_u16(R, hk, wk)), (cfg, source, k)
        hwc = spiht_amd.decode_image_reduced_u8(enc, s, k, channels_last=True)
        assert hwc.shape == (hk, wk, c) and same_bits(hwc, u8.transpose(1, 2, 0))
        assert same_bits(spiht_amd.decode_image_reduced_u8(enc, s, k, crop=True, channels_last=True), u8[:, ys, xs].transpose(1, 2, 0))
        assert same_bits(spiht_amd.decode_image_reduced_u16(enc, s, k, crop=True), u16[:, ys, xs])


# ---- 5. batch and prefixes -------------------------------------------------------------------------------------------------------
def test_batch_decode_reduced(oracle):
    """BatchCodec.decode_reduced* from host results and from the slots encode_device left on the device"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray
    c, H, W, L, B = 3, 61, 77, 3, 3
    s = spiht_amd.SpihtSettings(wavelet="bior4.4", quantization_scale=255.0, per_channel_quant_scales=[1.0, 0.2, 0.2])
    codec = BatchCodec(c, H, W, s, L, 9000)
    imgs = np.stack([synth_image(300 + b, c, H, W) for b in range(B)])
    res = codec.encode(imgs)
    for k in (1, 3):
        Rs = [oracle_stream_reduced(oracle, r, s, k) for r in res]
        hk, wk = Rs[0][1:]
        R = np.stack([x[0] for x in Rs])
        rs = codec.reduced_shape(k)
        assert same_bits(codec.decode_reduced(res, k), R)
        assert same_bits(codec.decode_reduced(res, k, crop=True),
                         R[:, :, rs["off_y"]:rs["off_y"] + rs["in_h"], rs["off_x"]:rs["off_x"] + rs["in_w"]])
        assert same_bits(codec.decode_reduced_u8(res, k), np.stack([to_u8(r, hk, wk) for r in R]))
        assert same_bits(codec.decode_reduced_u16(res, k, channels_last=True), np.stack([to_u16(r, hk, wk) for r in R]).transpose(0, 2, 3, 1))
    # device-resident: pixels -> slots -> reduced pictures, nothing but the small pictures comes back
    k = 2
    ctx = codec.ctx
    rs = codec.reduced_shape(k)
    d_img = DeviceArray(ctx, imgs.shape, np.float64)
    d_img.upload(imgs)
    d_out, d_nbits = DeviceArray(ctx, (B, codec.slot_stride), np.uint8), DeviceArray(ctx, (B,), np.uint64)
    d_nbytes, d_maxn = DeviceArray(ctx, (B,), np.uint64), DeviceArray(ctx, (B,), np.uint8)
    d_f = DeviceArray(ctx, (B, c, rs["rec_h"], rs["rec_w"]), np.float64)
    pitch = 4 * rs["pic_w"] + 8
    d_8 = DeviceArray(ctx, (B, rs["pic_h"], pitch), np.uint8)
    d_8.upload(np.full(d_8.shape, 0xA5, np.uint8))
    codec.encode_device(d_img.ptr, B, d_out.ptr, d_nbits.ptr, d_maxn.ptr)
    codec.nbits_to_nbytes(d_nbits.ptr, B, d_nbytes.ptr)
    codec.decode_reduced_device(d_out.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_f.ptr, k)
    codec.decode_reduced_device_u8(d_out.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_8.ptr, k, strides=(rs["pic_h"] * pitch, 1, pitch, 4))
    ctx.synchronize()
    R = np.stack([oracle_stream_reduced(oracle, r, s, k)[0] for r in res])
    assert same_bits(d_f.download(), R)
    rgba = d_8.download()
    px = rgba[:, :, :4 * rs["pic_w"]].reshape(B, rs["pic_h"], rs["pic_w"], 4)
    assert same_bits(px[..., :3].transpose(0, 3, 1, 2), np.stack([to_u8(r, rs["pic_h"], rs["pic_w"]) for r in R]))
    assert (px[..., 3] == 0xA5).all() and (rgba[:, :, 4 * rs["pic_w"]:] == 0xA5).all()
    with pytest.raises(ValueError):
        codec.decode_reduced_device_u8(d_out.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_8.ptr, k, strides=(0, 1, pitch, 4))
    for d in (d_img, d_out, d_nbits, d_nbytes, d_maxn, d_f, d_8):
        d.free()


@pytest.mark.parametrize("one_walk", [True, False])
def test_decode_prefixes_reduced(oracle, one_walk):
    """decode_prefixes(..., reduce=1): the reduced decode of every prefix, in the order given; reduce=0 is what it was"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    c, H, W, L = 3, 64, 96, 3
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, L)
    enc = spiht_amd.encode_image(synth_image(77, c, H, W), s, L, 16000)
    lens = [500, 40, 2000, 1200, 3]
    got = codec.decode_prefixes(enc, lens, one_walk=one_walk, reduce=1)
    for j, n in enumerate(lens):
        pre = spiht_amd.EncodingResult(enc.encoded_bytes[:n], H, W, c, enc.max_n, L)
        assert same_bits(got[j], oracle_stream_reduced(oracle, pre, s, 1)[0]), (one_walk, n)
        assert same_bits(got[j], spiht_amd.decode_image_reduced(pre, s, 1))
    full = codec.decode_prefixes(enc, lens, one_walk=one_walk)
    assert same_bits(full, codec.decode_prefixes(enc, lens, one_walk=one_walk, reduce=0))
    assert same_bits(full[2], spiht_amd.decode_image(spiht_amd.EncodingResult(enc.encoded_bytes[:2000], H, W, c, enc.max_n, L), s))


# ---- 6. the internal coefficient array stays clean ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_array_is_clean_after_a_reduced_decode(oracle, k):
    """a reduced inverse reads a corner of the context's array, the decoder wrote all over it: after the call the array is
    all zero again -- a full decode of a short stream of the same geometry on the same context equals the oracle's"""
    import spiht_amd
    c, H, W, L = 3, 72, 104, 3
    s = spiht_amd.SpihtSettings()
    rich = spiht_amd.encode_image(synth_image(11, c, H, W), s, L, None)
    poor = spiht_amd.encode_image(synth_image(12, c, H, W), s, L, 900)
    assert same_bits(spiht_amd.decode_image_reduced(rich, s, k), oracle_stream_reduced(oracle, rich, s, k)[0])
    want = oracle.decode_image(poor.encoded_bytes, poor.max_n, c, H, W, "bior2.2", L, 50.0, None)
    assert same_bits(spiht_amd.decode_image(poor, s), want)
    assert same_bits(spiht_amd.decode_image_reduced_u8(rich, s, k), to_u8(*oracle_stream_reduced(oracle, rich, s, k)))
    assert same_bits(spiht_amd.decode_image_reduced(poor, s, L - 1), oracle_stream_reduced(oracle, poor, s, L - 1)[0])


# ---- 7. arguments ---------------------------------------------------------------------------------------------------------------
def test_reduce_out_of_range_raises_and_leaves_the_context_usable(oracle):
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec
    c, H, W, L = 1, 40, 56, 3
    s = spiht_amd.SpihtSettings(wavelet="haar")
    enc = spiht_amd.encode_image(synth_image(5, c, H, W), s, L, 4000)
    for bad in (L + 1, -1):
        for fn in (spiht_amd.decode_image_reduced, spiht_amd.decode_image_reduced_u8, spiht_amd.decode_image_reduced_u16):
            with pytest.raises(ValueError):
                fn(enc, s, bad)
        with pytest.raises(ValueError):
            BatchCodec(c, H, W, s, L).decode_reduced([enc], bad)
        # ... and the C ABI itself, on a live context, before anything is queued
        ctx, lib = _lib.default_context(), _lib.lib()
        data = np.frombuffer(enc.encoded_bytes, np.uint8)
        out = np.full((c, H + 1, W + 1), 7.0)
        st = lib.spiht_decode_image_reduced_host_f64(ctx.handle, vp(data.ctypes.data), data.size, enc.max_n, c, H, W,
                                                     lib.spiht_wavelet_id(b"haar"), 0, L, 50.0, None, vp(out.ctypes.data), bad)
        assert st == _lib.ERR_ARG and (out == 7.0).all()
        assert same_bits(spiht_amd.decode_image_reduced(enc, s, 1), oracle_stream_reduced(oracle, enc, s, 1)[0])
    # a quantisation scale that q * 2^k overflows is refused; reduce 0 of it is not this call's business
    big = spiht_amd.SpihtSettings(wavelet="haar", quantization_scale=1e308)
    with pytest.raises(ValueError):
        spiht_amd.decode_image_reduced(enc, big, 2)
    assert same_bits(spiht_amd.decode_image(enc, s), oracle.decode_image(enc.encoded_bytes, enc.max_n, c, H, W, "haar", L, 50.0, None))


# ---- 8. the command-line tool ----------------------------------------------------------------------------------------------------
def test_command_line_reduce(tmp_path, capsys):
    """python -m spiht_amd.encode_decode IMAGE --reduce 1: the file holds the reduced 8-bit picture; no distance is printed"""
    import spiht_amd
    from spiht_amd import encode_decode as tool
    from spiht_amd.utils import imload, imsave
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "small.png")
    imsave(src, synth_image(21, 3, 64, 96))
    args = tool.build_parser().parse_args([src, "--bpp", "1.0", "--reduce", "1", "--out", dst])
    assert tool.build_parser().parse_args([src]).reduce == 0
    enc, small = tool.main(args)
    p = tool.plan(args, 3, 64, 96)
    want = spiht_amd.decode_image_reduced_u8(enc, p.settings, 1)
    assert small.dtype == np.uint8 and same_bits(small, want)
    rs = spiht_amd.reduced_shape(64, 96, p.settings, p.level, 1)
    assert want.shape == (3, rs["pic_h"], rs["pic_w"])
    back = np.round(imload(dst) * 255).astype(np.uint8)
    assert same_bits(back, want)
    text = capsys.readouterr().out
    assert "1/2 size" in text and "mean squared error" not in text
