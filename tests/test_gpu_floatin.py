"""Float pixels in on the GPU: encodes of float32, float16 and bfloat16 pictures, held field by field and bit for bit to

    <the float64 call of the same arguments>(floatpx.to_float64(P, kind))

-- every sample widened exactly, nothing scaled, nothing clipped -- and to the CPU oracle.  Every comparison is equality
(NaN: NaN-ness).  This is not encode_image(P32), which keeps the single-precision transform: case 2 holds the two apart."""
import ctypes as C
import functools

import numpy as np
import pytest

import call_sequence_cases as K
from floatin_cases import KINDS, bits, clear_last_bit, float_image, oracle_stream, oracle_stream_f32, widen
from test_gpu_alloc import run_sse, sse_operands
from test_gpu_batch_chunks import Scope, slot_bytes
from test_gpu_coder_edges import _unguard
from test_gpu_dwt_addressing import _levels, _reference, _same
from test_gpu_dwt_sweep import _Bufs, _geometry
from test_gpu_roi import run_sse_w
from test_gpu_u8 import CONFIGS, same_result, settings
from tile_helpers import dev

pytestmark = pytest.mark.gpu
vp = C.c_void_p
UNLIMITED = 99999999999999999
FILL = 0xA5  # the byte of everything that is no sample


def kid(kind):
    from spiht_amd import floatpx
    return floatpx.kind_arg(kind)


def esize(kind):
    from spiht_amd import floatpx
    return floatpx.itemsize(kind)


def dt_arg(kind):
    """what the Python calls take as dtype= beside an array of the kind: nothing for the numpy types, the name for bit patterns"""
    return dict(dtype="bfloat16") if kind == "bfloat16" else {}


def layouts_of(P, fill=FILL):
    """a picture [c, H, W] of a kind as {name: (buffer, view [c, H, W] inside it)}: planar, interleaved, and (three channels)
    the [..., :3] view of a four-sample buffer; whatever is no sample holds the fill byte"""
    c, H, W = P.shape
    out = {"chw": (None, P)}
    hwc = np.ascontiguousarray(P.transpose(1, 2, 0))
    out["hwc"] = (hwc, hwc.transpose(2, 0, 1))
    if c == 3:
        four = np.full((H, W, 4 * P.dtype.itemsize), fill, np.uint8).view(P.dtype)
        four[..., :3] = P.transpose(1, 2, 0)
        out["four"] = (four, four[..., :3].transpose(2, 0, 1))
    return out


# ---- 1. the widening alone ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def widening_patterns(kind):
    """the bit patterns to widen, as [3, h, w] of the storage type with odd h and w: all 65 536 of a 16-bit kind; of float32
    every pattern with a zero low half, 2^20 random ones, and subnormals, zeros, infinities and NaNs by name"""
    if kind != "float32":
        p = np.arange(65536, dtype=np.uint16)
    else:
        rng = np.random.default_rng(20)
        p = np.concatenate([np.arange(65536, dtype=np.uint32) << 16, rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
                            np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x00400000, 0x7F7FFFFF,
                                      0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32)])
    w = 211
    h = -(-p.size // (3 * w)) | 1
    body = np.zeros(3 * h * w, p.dtype)
    body[:p.size] = p
    body[p.size:] = p[:body.size - p.size]
    body = body.reshape(3, h, w)
    body.setflags(write=False)
    return body


@pytest.mark.parametrize("kind", KINDS)
def test_widening_alone(kind):
    from spiht_amd import _lib, floatpx
    from spiht_amd.batch import DeviceArray
    src = widening_patterns(kind)
    c, h, w = src.shape
    k, es = kid(kind), esize(kind)
    want = widen(src.view(floatpx.storage_dtype(kind)), kind)
    nan = np.isnan(want)
    sub = (np.abs(want) > 0) & (np.abs(want) < {"float32": 2.0 ** -126, "float16": 2.0 ** -14, "bfloat16": 2.0 ** -126}[kind])
    assert nan.sum() > 8 and sub.sum() > 8 and np.isinf(want).sum() >= 2 and (bits(want) == 1 << 63).any()
    ctx, L = _lib.default_context(), _lib.lib()
    layouts = {"dense": (h * w * es, w * es, es), "hwc": (es, w * 3 * es, 3 * es), "four": (es, w * 4 * es, 4 * es)}
    d_out = DeviceArray(ctx, (c * h * w + 2,), np.float64)
    try:
        for name, st in layouts.items():
            span = es + 2 * st[0] + (h - 1) * st[1] + (w - 1) * st[2]
            for off in (0, es):  # the base at a multiple of 16 bytes, and one element behind it
                host = np.full(off + span + 64, FILL, np.uint8)
                np.lib.stride_tricks.as_strided(host[off:off + span].view(src.dtype), (c, h, w), st)[...] = src
                d_in = dev(host)
                try:
                    assert d_in.ptr % 16 == 0
                    d_out.upload(np.full(c * h * w + 2, -7.25))
                    stv = np.array((0,) + st, dtype=np.int64)
                    _lib.check(L.spiht_widen_batch_flt(ctx.handle, k, vp(d_in.ptr + off), vp(stv.ctypes.data), 1, c, h, w,
                                                       vp(d_out.ptr + 8)))
                    ctx.synchronize()
                    got, back = d_out.download(), d_in.download()
                finally:
                    d_in.free()
                assert got[0] == -7.25 and got[-1] == -7.25, (name, off)
                got = got[1:-1].reshape(c, h, w)
                assert np.array_equal(np.isnan(got), nan), (name, off)
                assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (name, off)
                assert np.array_equal(back, host), (name, off)  # the input buffer, every byte
        # refused before any launch: a kind that is none, a base off the element, strides off the element or negative
        ok = np.array((0,) + layouts["dense"], dtype=np.int64)
        call = lambda kk, ptr, stv: L.spiht_widen_batch_flt(ctx.handle, kk, vp(ptr), vp(stv.ctypes.data), 1, c, h, w, vp(d_out.ptr))  # noqa: E731
        assert call(0, 1024, ok) == _lib.ERR_ARG and call(4, 1024, ok) == _lib.ERR_ARG
        assert call(k, 1024 + es // 2, ok) == _lib.ERR_ARG
        assert call(k, 1024, np.array((0, h * w * es + 1, w * es, es), dtype=np.int64)) == _lib.ERR_ARG
        assert call(k, 1024, np.array((0, h * w * es, -w * es, es), dtype=np.int64)) == _lib.ERR_ARG
    finally:
        d_out.free()


# ---- 2. the precision reaches the stream ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_precision_reaches_the_stream(oracle, kind):
    """Each condition is asserted on the oracle BEFORE the GPU is compared: the stream of the widened picture differs from the
    stream of the picture with its last mantissa bit cleared, and for float32 from the single-precision stream of the same
    array -- a kernel that drops a bit, or transforms in single precision, cannot pass.  (At q = 50 the three float32 streams
    are equal: asserted too, as the reason why the float32 case runs at q = 4e6.)"""
    import spiht_amd
    wv, md = "bior2.2", "reflect"
    P = np.ascontiguousarray(float_image(kind, 31, 3, 57, 83)[:, :48, :64])
    q = 4e6 if kind == "float32" else 20000.0
    co, ob, on = oracle_stream(oracle, widen(P, kind), wv, md, 2, q, UNLIMITED)
    co1, ob1, _ = oracle_stream(oracle, widen(clear_last_bit(P), kind), wv, md, 2, q, UNLIMITED)
    print("%s at q = %g: max |coefficient| %d, %d of %d quantised values differ with the last bit cleared"
          % (kind, q, np.abs(co).max(), (co != co1).sum(), co.size))
    assert ob != ob1 and (co != co1).sum() >= 100
    cases = [(P, 2, q, None, ob, on)]
    if kind == "float32":
        co32, ob32, _ = oracle_stream_f32(oracle, P, wv, md, 2, q, UNLIMITED)
        print("float32: %d of %d quantised values differ from the single-precision transform's" % ((co != co32).sum(), co.size))
        assert ob != ob32 and (co != co32).sum() >= 100
        e = [f(oracle, a, wv, md, 2, 50.0, UNLIMITED)[1] for f, a in ((oracle_stream, widen(P, kind)), (oracle_stream_f32, P),
                                                                       (oracle_stream, widen(clear_last_bit(P), kind)))]
        assert e[0] == e[1] == e[2]  # q = 50 shows nothing about the arithmetic of float32 pixels
    else:  # ... and already at the default q, level 3, 40 000 bits on the odd-sized picture
        P2 = float_image(kind, 31, 3, 57, 83)
        _, ob2, on2 = oracle_stream(oracle, widen(P2, kind), wv, md, 3, 50.0, 40000)
        assert ob2 != oracle_stream(oracle, widen(clear_last_bit(P2), kind), wv, md, 3, 50.0, 40000)[1]
        cases.append((P2, 3, 50.0, 40000, ob2, on2))
    for pic, level, qq, max_bits, want, want_n in cases:
        s = spiht_amd.SpihtSettings(wavelet=wv, mode=md, quantization_scale=qq)
        got = spiht_amd.encode_image_float(pic, s, level, max_bits, **dt_arg(kind))
        assert got.encoded_bytes == want and got.max_n == want_n
        same_result(got, spiht_amd.encode_image(widen(pic, kind), s, level=level, max_bits=max_bits))
    if kind == "float32":  # the same array through encode_image keeps the single-precision transform
        s = spiht_amd.SpihtSettings(wavelet=wv, mode=md, quantization_scale=q)
        assert spiht_amd.encode_image(P, s, level=2).encoded_bytes == ob32


# ---- 3. configurations and views -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS)
def test_configs_and_views(cfg):
    import spiht_amd
    c, H, W = cfg["c"], cfg["H"], cfg["W"]
    s = settings(cfg)
    kw = dict(level=cfg["level"], max_bits=cfg["max_bits"])
    for kind in KINDS:
        P = float_image(kind, 2000 + H, c, H, W)
        more = dict(kw, **dt_arg(kind))
        ref = spiht_amd.encode_image(widen(P, kind), s, **kw)
        for name, (buf, view) in layouts_of(P).items():
            before = None if buf is None else buf.copy()
            same_result(spiht_amd.encode_image_float(view, s, **more), ref)
            assert buf is None or np.array_equal(bits(buf), bits(before)), (kind, name)
        hwc = np.ascontiguousarray(P.transpose(1, 2, 0))
        same_result(spiht_amd.encode_image_float(hwc, s, channels_last=True, **more), ref)
        neg = np.ascontiguousarray(P[:, ::-1])[:, ::-1]
        assert neg.strides[1] < 0 and np.array_equal(bits(np.ascontiguousarray(neg)), bits(P))
        same_result(spiht_amd.encode_image_float(neg, s, **more), ref)
        other = P.astype(P.dtype.newbyteorder(">" if np.little_endian else "<"))
        assert not other.dtype.isnative
        same_result(spiht_amd.encode_image_float(other, s, **more), ref)
        if kind != "bfloat16":  # the kind named as well as inferred
            same_result(spiht_amd.encode_image_float(P, s, dtype=kind, **kw), ref)


# ---- 4. routes -------------------------------------------------------------------------------------------------------------------
ROUTES = [
    dict(color="IPT", q=1.0, mults=[50.0, 15.0, 15.0], level=3),       # colour change fused into level 1
    dict(color="IPT", mode="periodization", level=2),                    # ... in front of / behind a two-pass level
    dict(mode="smooth", level=2),
    dict(mode="antireflect", level=3),
    dict(wavelet="db11", level=2),                                       # a filter longer than the tiled kernels take
]


@pytest.mark.parametrize("cfg", ROUTES)
def test_routes_vs_float64(cfg):
    import spiht_amd
    c, H, W = 3, 57, 83
    s = settings(cfg)
    for kind in KINDS:
        P = float_image(kind, 31, c, H, W)
        ref = spiht_amd.encode_image(widen(P, kind), s, level=cfg["level"], max_bits=6000)
        same_result(spiht_amd.encode_image_float(P, s, level=cfg["level"], max_bits=6000, **dt_arg(kind)), ref)
        hwc = np.ascontiguousarray(P.transpose(1, 2, 0))
        same_result(spiht_amd.encode_image_float(hwc, s, level=cfg["level"], max_bits=6000, channels_last=True, **dt_arg(kind)), ref)


# ---- 5. the round trip in the kind ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_in_kind(oracle, kind):
    import spiht_amd
    from spiht_amd import floatpx
    c, H, W = 3, 57, 83
    P = float_image(kind, 31, c, H, W)
    s = spiht_amd.SpihtSettings()
    ob, on, _ = oracle.encode_image(widen(P, kind), "bior2.2", "reflect", 3, 50.0, None, 40000)
    o = oracle.decode_image(ob, on, c, H, W, "bior2.2", 3, 50.0, None)[:, :H, :W]
    r = spiht_amd.encode_image_float(P, s, 3, 40000, **dt_arg(kind))
    assert r.encoded_bytes == ob and r.max_n == on
    got = spiht_amd.decode_image_float(r, s, dtype=kind)
    want = floatpx.convert(o, kind)
    assert got.dtype == want.dtype == P.dtype and got.shape == P.shape and np.array_equal(bits(got), bits(want))


# ---- 6. batch and device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec_dtype", [np.float64, np.float32])
def test_batch_and_device(codec_dtype):
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray
    B, c, H, W = 5, 3, 45, 61
    s = spiht_amd.SpihtSettings(color_model="IPT") if codec_dtype == np.float64 else spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=3, max_bits=5000, pixel_dtype=codec_dtype)  # (any pixel type of the codec: the float64 arithmetic)
    ctx = codec.ctx
    for kind in KINDS:
        es = esize(kind)
        P = np.stack([float_image(kind, 100 + b, c, H, W) for b in range(B)])
        singles = [spiht_amd.encode_image_float(P[b], s, 3, 5000, **dt_arg(kind)) for b in range(B)]
        same_result(singles[1], spiht_amd.encode_image(widen(P[1], kind), s, level=3, max_bits=5000))
        res = codec.encode_float(P, **dt_arg(kind))
        assert len(res) == B
        for b in range(B):
            same_result(res[b], singles[b])
        for b, r in enumerate(codec.encode_float(np.ascontiguousarray(P.transpose(0, 2, 3, 1)), channels_last=True, **dt_arg(kind))):
            same_result(r, singles[b])
        # the device form from a padded four-channel buffer; the outputs between guard rows
        pitch = 4 * W * es + 12 * es
        host = np.full((B, H, pitch), FILL, np.uint8)
        st = (H * pitch, es, pitch, 4 * es)
        np.lib.stride_tricks.as_strided(host.reshape(-1).view(P.dtype), (B, c, H, W), st)[...] = P
        guard = lambda shape, dt: np.full(shape, 0x7F, np.uint8).view(dt)  # noqa: E731
        outs = [guard((B + 2, codec.slot_stride), np.uint8), guard((8 * (B + 2),), np.uint64), guard((B + 2,), np.uint8)]
        d_px, d = dev(host), [dev(a) for a in outs]
        try:
            ptr = [d[0].ptr + codec.slot_stride, d[1].ptr + 8, d[2].ptr + 1]
            codec.encode_device_float(d_px.ptr, B, *ptr, kind, strides=st)
            ctx.synchronize()
            out, nbits, maxn = (x.download() for x in d)
            assert np.array_equal(d_px.download(), host)
            assert (out[0] == 0x7F).all() and (out[-1] == 0x7F).all() and nbits[0] == nbits[-1] == outs[1][0] and maxn[0] == maxn[-1] == 0x7F
            for b in range(B):
                n = (int(nbits[1 + b]) + 7) // 8
                assert out[1 + b, :n].tobytes() == singles[b].encoded_bytes and int(maxn[1 + b]) == singles[b].max_n, (kind, b)
            # refused: a base off the element, a stride that is no multiple of it, an unknown kind -- the outputs keep their bytes
            for x, a in zip(d, outs):
                x.upload(a)
            with pytest.raises(ValueError):
                codec.encode_device_float(d_px.ptr + es // 2, B, *ptr, kind, strides=st)
            with pytest.raises(ValueError):
                codec.encode_device_float(d_px.ptr, B, *ptr, kind, strides=(H * pitch, es, pitch + es // 2, 4 * es))
            with pytest.raises(TypeError):
                codec.encode_device_float(d_px.ptr, B, *ptr, np.float64, strides=st)
            stv = np.array(st, np.int64)
            raw = lambda kk, p, sv: codec.L.spiht_encode_image_batch_flt(  # noqa: E731
                ctx.handle, kk, vp(p), vp(sv.ctypes.data), B, c, H, W, codec.wid, codec.mid, 3, 50.0, None, 5000, vp(ptr[0]),
                codec.slot_stride, vp(ptr[1]), vp(ptr[2]), None)
            assert raw(kid(kind), d_px.ptr + es // 2, stv) != 0 and raw(0, d_px.ptr, stv) != 0 and raw(4, d_px.ptr, stv) != 0
            assert raw(kid(kind), d_px.ptr, np.array((H * pitch, es, pitch + es // 2, 4 * es), np.int64)) != 0
            ctx.synchronize()
            for x, a in zip(d, outs):
                assert np.array_equal(x.download(), a)
        finally:
            d_px.free()
            for x in d:
                x.free()
    with pytest.raises(TypeError):
        codec.encode_float(P)  # (bfloat16 bit patterns without their kind)


# ---- 7. the forward kernel's addressing ------------------------------------------------------------------------------------------
def flt_layout(name, P):
    """two pictures [2, 3, H, W] of a kind -> (buffer, byte strides or None): planar, or four samples per pixel and 12 bytes
    behind every row; everything that is no sample holds the fill byte"""
    B, c, H, W = P.shape
    es = P.dtype.itemsize
    if name == "planar":
        return np.ascontiguousarray(P), None
    pitch = 4 * W * es + 12
    buf = np.full((B, H, pitch), FILL, np.uint8)
    st = (H * pitch, es, pitch, 4 * es)
    np.lib.stride_tricks.as_strided(buf.reshape(-1).view(P.dtype), P.shape, st)[...] = P
    return buf, st


def flt_forward(kind, buf, strides, B, c, H, W, wavelet, mode, level, q):
    """spiht_dwt_pyramid_batch_flt with the pyramid left out -> (int32 [B, c, enc_h, enc_w], max words, the input read back)"""
    with _Bufs() as d:
        L = d.L
        wid, mid = L.spiht_wavelet_id(wavelet.encode()), L.spiht_mode_id(mode.encode())
        eh, ew = _geometry(L, d.check, H, W, wid, mid, level)[2:4]
        out, ma, back = np.empty((B, c, eh, ew), np.int32), np.empty(B, np.uint32), np.empty_like(buf)
        d_in, d_out, d_ma = d.put(buf), d.new(out.nbytes, 0xFF), d.new(ma.nbytes, 0xEE)
        st = None if strides is None else np.array(strides, np.int64)
        d.check(L.spiht_dwt_pyramid_batch_flt(d.ctx.handle, kid(kind), vp(d_in), None if st is None else vp(st.ctypes.data), B, c, H, W,
                                              wid, mid, level, float(q), None, vp(d_out), None, None, vp(d_ma)))
        d.ctx.download(out, d_out)
        d.ctx.download(ma, d_ma)
        d.ctx.download(back, d_in)
        return out, ma, back


def addressing_pictures(kind, H, W):
    return np.stack([float_image(kind, 900 + H + b, 3, H, W) for b in range(2)])


@pytest.mark.parametrize("layout", ("planar", "four"))
@pytest.mark.parametrize("kind", KINDS)
def test_forward_kernel_addressing(oracle, kind, layout):
    """the grid of test_gpu_dwt_addressing.test_pixel_views on float views: one tile and a second of one column, several
    tiles, pictures shorter than the filters; zero padding reads nothing outside the view; the buffer is left alone"""
    for (H, W) in ((21, 125), (43, 123), (5, 7), (19, 251)):
        P = addressing_pictures(kind, H, W)
        buf, strides = flt_layout(layout, P)
        imgs = widen(P, kind)
        for wavelet, mode in (("bior2.2", "reflect"), ("bior2.2", "zero"), ("bior4.4", "symmetric"), ("haar", "periodic"),
                              ("bior4.4", "zero"), ("bior2.2", "constant")):
            for level in _levels(oracle, H, W, wavelet, mode):
                ref, ref_ma = _reference(oracle, kind, imgs, wavelet, mode, level, 50.0, None)
                got, ma, back = flt_forward(kind, buf, strides, 2, 3, H, W, wavelet, mode, level, 50.0)
                _same(got, ma, ref, ref_ma, (kind, layout, wavelet, mode, H, W, level))
                assert np.array_equal(bits(back), bits(buf))


@pytest.mark.parametrize("kind", KINDS)
def test_forward_kernel_wide_addressing(oracle, kind, monkeypatch):
    monkeypatch.setenv("SPIHT_DWT_ADDR64", "1")
    H, W = 21, 125
    P = addressing_pictures(kind, H, W)
    buf, strides = flt_layout("four", P)
    for wavelet, mode in (("bior2.2", "reflect"), ("bior2.2", "symmetric"), ("bior4.4", "periodic"), ("bior4.4", "zero"),
                          ("haar", "constant")):
        for level in (1, _levels(oracle, H, W, wavelet, mode)[-1]):
            ref, ref_ma = _reference(oracle, kind, widen(P, kind), wavelet, mode, level, 50.0, None)
            got, ma, back = flt_forward(kind, buf, strides, 2, 3, H, W, wavelet, mode, level, 50.0)
            _same(got, ma, ref, ref_ma, ("wide", kind, wavelet, mode, level))
            assert np.array_equal(bits(back), bits(buf))


# ---- 8. the chunk seam -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_case(kind):
    """K.SEAM2 with pictures of the kind: 127 distinct ones in turn, and the oracle on each (about 0.3 s of host time)"""
    from oracle import oracle as O
    k = K.SEAM2
    D = K.SEAM2_DISTINCT
    P = np.stack([float_image(kind, 5000 + i, k["c"], k["H"], k["W"]) for i in range(D)])
    g = O.geometry(k["H"], k["W"], k["wavelet"], k["level"], k["mode"])
    co, streams, nbits, max_n = [], [], [], []
    for i in range(D):
        a = O.quantize(O.wavedec2_array(widen(P[i], kind), k["wavelet"], k["mode"], k["level"])[0], k["q"], None)
        d, n, nb = O.encode_nbits(a, g["ll_h"], g["ll_w"], k["max_bits"])
        co.append(a), streams.append(d), nbits.append(nb), max_n.append(n)
    co = np.stack(co)
    return P, g, co, np.abs(co.astype(np.int64)).max(axis=(1, 2, 3)).astype(np.uint32), streams, np.array(nbits, np.uint64), np.array(max_n, np.uint8)


def seam_input(s, P, which):
    """the batch as a padded view (K.padded_strides: no stride is the dense one) on the device -> (array, host copy, strides)"""
    buf, view, st = K.padded_buffer(len(which), *P.shape[1:], P.dtype)
    view[...] = P[which]
    return s.dev(buf), buf, st


@pytest.mark.parametrize("kind", ["float32", "bfloat16"])  # (the element size enters the offsets)
def test_chunk_seam_dwt_pyramid(kind):
    k = K.SEAM2
    P, g, co, maxabs, _, _, _ = seam_case(kind)
    which = K.in_turn(K.SEAM2_DISTINCT)
    B, c, n = len(which), k["c"], k["c"] * g["enc_h"] * g["enc_w"]
    assert K.chunks(B, c) == [(0, 21845), (21845, 7)]
    with Scope() as s:
        wid, mid = s.L.spiht_wavelet_id(k["wavelet"].encode()), s.L.spiht_mode_id(k["mode"].encode())
        d_img, buf, st = seam_input(s, P, which)
        d_co, p_co = s.guarded((B, n), np.int32)
        d_mx, p_mx = s.guarded((B,), np.uint32)
        s.check(s.L.spiht_dwt_pyramid_batch_flt(s.ctx.handle, kid(kind), vp(d_img.ptr), vp(st.ctypes.data), B, c, k["H"], k["W"], wid, mid,
                                                k["level"], k["q"], None, vp(p_co), None, None, vp(p_mx)))
        s.ctx.synchronize()
        got = _unguard(d_co, "coefficients").reshape((B,) + co.shape[1:])
        bad = np.nonzero((got != co[which]).reshape(B, -1).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), bad[:8].tolist())
        assert np.array_equal(_unguard(d_mx, "max words"), maxabs[which])
        assert np.array_equal(bits(d_img.download()), bits(buf))


@pytest.mark.parametrize("kind", ["float32", "bfloat16"])
def test_chunk_seam_encode_image(kind):
    k = K.SEAM2
    P, g, _, _, streams, nbits, max_n = seam_case(kind)
    which = K.in_turn(K.SEAM2_DISTINCT)
    B, c = len(which), k["c"]
    slot = slot_bytes((c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"]), k["max_bits"])
    with Scope() as s:
        wid, mid = s.L.spiht_wavelet_id(k["wavelet"].encode()), s.L.spiht_mode_id(k["mode"].encode())
        d_img, buf, st = seam_input(s, P, which)
        d_out, p_out = s.guarded((B, slot), np.uint8)
        d_nb, p_nb = s.guarded((B,), np.uint64)
        d_mn, p_mn = s.guarded((B,), np.uint8)
        s.check(s.L.spiht_encode_image_batch_flt(s.ctx.handle, kid(kind), vp(d_img.ptr), vp(st.ctypes.data), B, c, k["H"], k["W"], wid, mid,
                                                 k["level"], k["q"], None, k["max_bits"], vp(p_out), slot, vp(p_nb), vp(p_mn), None))
        s.ctx.synchronize()
        assert np.array_equal(_unguard(d_nb, "nbits"), nbits[which])
        assert np.array_equal(_unguard(d_mn, "max_n"), max_n[which])
        got = _unguard(d_out, "slots")
        want = K.slots_of([streams[i] for i in which], slot)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), bad[:8].tolist())
        assert np.array_equal(bits(d_img.download()), bits(buf))


# ---- 9. tiled ------------------------------------------------------------------------------------------------------------------------
def same_allocation(a, b):
    assert repr(a) == repr(b)  # (dataclasses of floats, lists and None: NaN-free, so their text is their value)


@pytest.mark.parametrize("tile", [32, (24, 40)])
@pytest.mark.parametrize("kind", KINDS)
def test_tiled(kind, tile):
    import spiht_amd
    c, H, W = 3, 70, 90
    P = float_image(kind, 4000 + H + W + c, c, H, W)
    P64 = widen(P, kind)
    hwc = np.ascontiguousarray(P.transpose(1, 2, 0))
    s = spiht_amd.SpihtSettings()
    kw = dt_arg(kind)
    roi = np.ones((H, W), np.uint8)
    roi[20:50, 30:70] = 8
    # plain: max_bits // T bits a tile
    codec = spiht_amd.TiledCodec(c, H, W, tile, s, None, 27005)
    ref = codec.encode(P64)
    assert codec.encode_float(P, **kw).to_bytes() == ref.to_bytes()
    assert codec.encode_float(hwc, channels_last=True, **kw).to_bytes() == ref.to_bytes()
    assert spiht_amd.encode_image_tiled_float(P, tile, s, None, 27005, **kw).to_bytes() == ref.to_bytes()
    two = codec.encode_float(np.stack([P, P[:, ::-1]]), **kw)
    assert two[0].to_bytes() == ref.to_bytes() and two[1].to_bytes() == codec.encode(P64[:, ::-1]).to_bytes()
    # allocate="rd": alone, with a weight map, with a target quality
    rd = spiht_amd.TiledCodec(c, H, W, tile, s, None, 27005, allocate="rd", points=8)
    for more in (dict(), dict(roi=roi), dict(target_psnr=30.0), dict(roi=roi, target_psnr=28.0)):
        ref = rd.encode(P64, **more)
        want = rd.last_allocation
        rd.last_allocation = None
        got = rd.encode_float(P, **kw, **more)
        assert got.to_bytes() == ref.to_bytes(), more
        same_allocation(rd.last_allocation, want)
    ref = rd.tile_curves(P64, roi=roi)
    got = rd.tile_curves_float(P, roi=roi, **kw)
    assert got.lengths == ref.lengths and np.array_equal(bits(got.sse), bits(ref.sse)) and got.nbytes == ref.nbytes and got.max_n == ref.max_n
    assert spiht_amd.encode_image_tiled_float(P, tile, s, None, 27005, allocate="rd", points=8, roi=roi, **kw).to_bytes() == \
        rd.encode(P64, roi=roi).to_bytes()
    # layers
    for more in (dict(layers=[9000, 27005]), dict(layers=2, roi=roi), dict(target_psnr=[24.0, 30.0])):
        ref = rd.encode_layered(P64, **more)
        want = rd.last_allocation
        rd.last_allocation = None
        got = rd.encode_layered_float(P, **kw, **more)
        assert got.to_bytes() == ref.to_bytes(), more
        same_allocation(rd.last_allocation, want)
    assert spiht_amd.encode_image_layered_float(P, tile, s, None, 27005, [9000, 27005], points=8, **kw).to_bytes() == \
        rd.encode_layered(P64, [9000, 27005]).to_bytes()
    # overlapping tiles: plain and allocate="rd"; what they refuse, they refuse here
    for more in (dict(), dict(allocate="rd", points=8)):
        ov = spiht_amd.TiledCodec(c, H, W, tile, s, None, 27005, overlap=4, **more)
        ref = ov.encode(P64)
        want = ov.last_allocation
        got = ov.encode_float(P, **kw)
        assert got.to_bytes() == ref.to_bytes() and got.overlap == 4
        same_allocation(ov.last_allocation, want)
    with pytest.raises(ValueError):
        ov.encode_float(P, roi=roi, **kw)
    with pytest.raises(ValueError):
        ov.encode_float(P, target_psnr=30.0, **kw)
    with pytest.raises(ValueError):
        codec.encode_float(P, roi=roi, **kw)  # (a codec without allocate="rd")
    # the device form from a padded four-sample buffer
    es = P.dtype.itemsize
    pitch = 4 * W * es + 12 * es
    host = np.full((H, pitch), FILL, np.uint8)
    st = (H * pitch, es, pitch, 4 * es)
    np.lib.stride_tricks.as_strided(host.reshape(-1).view(P.dtype), (c, H, W), st[1:])[...] = P
    T = codec.T
    d_px, d_packed, d_lens, d_maxn = dev(host), dev(np.zeros(T * codec.codec.slot_stride, np.uint8)), dev(np.zeros(T, np.uint32)), dev(np.zeros(T, np.uint8))
    try:
        ref = codec.encode(P64)
        codec.encode_device_float(d_px, 1, d_packed, d_lens, d_maxn, kind, strides=st)
        codec.ctx.synchronize()
        lens = d_lens.download()
        assert [int(v) for v in lens] == ref.nbytes and [int(v) for v in d_maxn.download()] == ref.max_n
        assert d_packed.download()[:int(lens.sum())].tobytes() == ref.encoded_bytes
        assert np.array_equal(d_px.download(), host)
        with pytest.raises(ValueError):
            codec.encode_device_float(d_px.ptr + es // 2, 1, d_packed, d_lens, d_maxn, kind, strides=st)
    finally:
        for d in (d_px, d_packed, d_lens, d_maxn):
            d.free()


def run_sse_flt(kind, tiles, dec, N, H, W, maps=None, off=0):
    """spiht_sse_tiles_flt / _w_flt on tiles of the kind whose device address is `off` bytes past a multiple of 16 -> [G, NT]"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    G, NT, c, rh, rw = dec.shape
    th, tw = tiles.shape[2:]
    raw = np.full(off + tiles.nbytes, FILL, np.uint8)
    raw[off:] = np.ascontiguousarray(tiles).view(np.uint8).reshape(-1)
    d_out, d_tiles, d_dec = dev(np.full(G * NT + 2, 77.0)), dev(raw), dev(dec)
    d_w = None
    try:
        assert d_tiles.ptr % 16 == 0
        args = (ctx.handle, kid(kind), vp(d_tiles.ptr + off), vp(d_dec.ptr), G, N, c, H, W, th, tw, rh, rw, vp(d_out.ptr + 8))
        if maps is None:
            _lib.check(L.spiht_sse_tiles_flt(*args))
        else:
            d_w = dev(np.ascontiguousarray(maps))
            _lib.check(L.spiht_sse_tiles_w_flt(*args, vp(d_w.ptr), 0 if len(maps) == 1 else H * W))
        ctx.synchronize()
        got = d_out.download()
    finally:
        for d in (d_out, d_tiles, d_dec, d_w):
            if d is not None:
                d.free()
    assert got[0] == 77 and got[-1] == 77
    return got[1:-1].reshape(G, NT)


@pytest.mark.parametrize("kind", KINDS)
def test_error_sums_alone(kind):
    """the two new error-sum kernels against the float64 ones on the widened tiles: edge tiles, two row chunks and a second
    picture; an odd tile width (rows of the original that are only element-aligned) with a decode one larger; a lane's second
    column step; the tile batch at an address that is only element-aligned.  A map of ones gives the unweighted bits."""
    from spiht_amd import _lib, floatpx
    rng = np.random.default_rng(40 + kid(kind))
    es = esize(kind)
    for (N, c, H, W, th, tw, rh, rw) in [(2, 3, 70, 90, 32, 32, 32, 32), (1, 1, 70, 91, 33, 41, 34, 42), (1, 1, 20, 300, 16, 136, 16, 136)]:
        t64, dec = sse_operands(rng, np.float64, N, c, H, W, th, tw, rh, rw, 3)
        tiles = floatpx.convert(np.clip(t64, -60000.0, 60000.0), kind)  # (what lies past the valid extents stays huge, and finite)
        wide = widen(tiles, kind)
        maps = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
        want = run_sse("spiht_sse_tiles_f64", wide, dec, N, H, W, np.float64)
        want_w = run_sse_w("f64", wide, dec, N, H, W, np.float64, maps)
        assert np.isfinite(want).all() and (want > 0).all()
        for off in (0, es):
            got = run_sse_flt(kind, tiles, dec, N, H, W, None, off)
            assert np.array_equal(bits(got), bits(want)), (kind, th, tw, off)
            got = run_sse_flt(kind, tiles, dec, N, H, W, maps, off)
            assert np.array_equal(bits(got), bits(want_w)), (kind, th, tw, off)
        ones = run_sse_flt(kind, tiles, dec, N, H, W, np.ones((1, H, W), np.uint8), es)
        assert np.array_equal(bits(ones), bits(want))
    # refused before a launch: a kind that is none, tiles off their element
    L, ctx = _lib.lib(), _lib.default_context()
    call = lambda kk, p: L.spiht_sse_tiles_flt(ctx.handle, kk, vp(p), vp(1024), 1, 1, 1, 70, 90, 32, 32, 32, 32, vp(2048))  # noqa: E731
    assert call(0, 1024) == _lib.ERR_ARG and call(4, 1024) == _lib.ERR_ARG and call(kid(kind), 1024 + es // 2) == _lib.ERR_ARG
