"""Float pixels out on the GPU: decodes into float32, float16 and bfloat16 pictures, held bit for bit to

    floatpx.convert(<the float64 call of the same arguments>[..., :h, :w], kind)

-- each float64 sample rounded ONCE -- and to the CPU oracle.  Every comparison is equality (NaN: NaN-ness)."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_image
from test_floatpx_cpu import hard_inputs
from test_gpu_u8 import BIG, settings
from test_gpu_u16 import u16_image
from tile_helpers import dev

pytestmark = pytest.mark.gpu

KINDS = ("float32", "float16", "bfloat16")


def conv(a, kind):
    from spiht_amd import floatpx
    return floatpx.convert(a, kind)


def bits(a):
    """an array of a kind as unsigned integers: equality of these is equality of every bit (-0.0 is not 0.0)"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def two_step(a, kind):
    """the wrong conversion: through float32"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return conv(a.astype(np.float32).astype(np.float64), kind)


# ---- 1. the conversion alone ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conversion_inputs():
    """[1, 3, h + 1, w + 1] float64 with odd h, w: the inputs of the CPU test and, for float32, 2^18 bit patterns across its
    range and its subnormals with their midpoints and the midpoints' neighbours; row h and column w are what the crop drops"""
    rng = np.random.default_rng(18)
    p = rng.integers(0, 0x7F800000, 1 << 18, dtype=np.uint32)
    p[:4096] = rng.integers(0, 0x00800000, 4096, dtype=np.uint32)       # subnormals
    p[4096:8192] = rng.integers(0x7F000000, 0x7F800000, 4096, dtype=np.uint32)  # the last binade
    p[-4:] = (0, 1, 0x007FFFFF, 0x7F7FFFFE)
    lo, hi = p.view(np.float32).astype(np.float64), (p + 1).view(np.float32).astype(np.float64)
    hi[np.isinf(hi)] = 2.0 ** 128
    mid = (lo + hi) / 2
    f32 = np.concatenate([lo, mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf)])
    # ... and 2^18 float64 bit patterns of any fraction, from below float32's smallest subnormal to above its largest value
    e = rng.integers(1023 - 151, 1023 + 129, 1 << 18, dtype=np.uint64)
    any64 = ((e << np.uint64(52)) | rng.integers(0, 1 << 52, 1 << 18, dtype=np.uint64)).view(np.float64)
    f32 = np.concatenate([f32, any64])
    x = np.concatenate([hard_inputs(), f32, -f32])
    w = 641
    h = -(-x.size // (3 * w)) | 1
    src = np.full((1, 3, h + 1, w + 1), np.nan)
    body = np.full(3 * h * w, 1.0)
    body[:x.size] = x
    src[0, :, :h, :w] = body.reshape(3, h, w)
    src.setflags(write=False)
    return src, h, w


@pytest.mark.parametrize("kind", KINDS)
def test_conversion_alone(kind):
    from spiht_amd import _lib, floatpx
    from spiht_amd.batch import DeviceArray
    src, h, w = conversion_inputs()
    k, es = floatpx.kind_arg(kind), floatpx.itemsize(kind)
    want = conv(src[0, :, :h, :w], kind)
    nan = np.isnan(src[0, :, :h, :w])
    assert nan.sum() == 2 and (~np.isnan(src[0, :, h, :])).sum() == 0
    if kind != "float32":
        assert (bits(two_step(src[0, :, :h, :w], kind)) != bits(want)).sum() > 1000  # the inputs tell one rounding from two
    ctx, L = _lib.default_context(), _lib.lib()
    d_src = dev(src)
    layouts = {"dense": (h * w * es, w * es, es), "hwc": (es, w * 3 * es, 3 * es), "rgba": (es, w * 4 * es, 4 * es)}
    try:
        for name, st in layouts.items():
            span = es + 2 * st[0] + (h - 1) * st[1] + (w - 1) * st[2]
            for off in (0, es):  # the base at a multiple of 16 bytes, and one element behind it
                host = np.full(off + span + 64, 0xA5, np.uint8)
                d_out = DeviceArray(ctx, host.shape, np.uint8)
                try:
                    d_out.upload(host)
                    assert d_out.ptr % 16 == 0
                    stv = np.array((0,) + st, dtype=np.int64)
                    _lib.check(L.spiht_convert_batch_flt(ctx.handle, k, C.c_void_p(d_src.ptr), 1, 3, h + 1, w + 1, h, w,
                                                         C.c_void_p(d_out.ptr + off), C.c_void_p(stv.ctypes.data)))
                    ctx.synchronize()
                    got = d_out.download()
                finally:
                    d_out.free()

                def view(buf):  # the [3, h, w] view of the layout in a host copy of the buffer
                    return np.lib.stride_tricks.as_strided(buf[off:off + span].view(want.dtype), (3, h, w), st)
                assert np.all(np.isnan(bfloat_or_self(view(got)[nan], kind))), (name, off)
                expect = host.copy()
                view(expect)[...] = want
                view(got)[nan] = want[nan]
                assert np.array_equal(got, expect), (name, off)  # every sample's bits, and every byte between and around them
        # refused before any launch: a kind that is none, a base off the element, overlapping and odd strides, a crop larger
        # than the source
        ok = np.array((0,) + layouts["dense"], dtype=np.int64)
        call = lambda kk, ptr, stv, hh=h: L.spiht_convert_batch_flt(ctx.handle, kk, C.c_void_p(d_src.ptr), 1, 3, h + 1, w + 1, hh, w,  # noqa: E731
                                                                     C.c_void_p(ptr), C.c_void_p(stv.ctypes.data))
        assert call(0, 1024, ok) == _lib.ERR_ARG and call(4, 1024, ok) == _lib.ERR_ARG
        assert call(k, 1024 + es // 2, ok) == _lib.ERR_ARG
        assert call(k, 1024, np.array((0, es, w * es, es), dtype=np.int64)) == _lib.ERR_ARG
        assert call(k, 1024, np.array((0, h * w * es + 1, w * es, es), dtype=np.int64)) == _lib.ERR_ARG
        assert call(k, 1024, ok, h + 2) == _lib.ERR_ARG
    finally:
        d_src.free()


def bfloat_or_self(a, kind):
    from spiht_amd import floatpx
    return floatpx.bfloat16_to_float64(a) if kind == "bfloat16" else a


# ---- 2. one picture, the discriminating case ---------------------------------------------------------------------------------
def pattern(seed, c=3, H=57, W=83):
    return u16_image(seed, c, H, W) / 65535


@functools.lru_cache(maxsize=None)
def discriminating():
    import spiht_amd
    P = pattern(0)
    s = spiht_amd.SpihtSettings(wavelet="bior2.2", mode="reflect", quantization_scale=50.0)
    r = spiht_amd.encode_image(P, s, level=3, max_bits=40000)
    f = spiht_amd.decode_image(r, s)
    f.setflags(write=False)
    return P, s, r, f


@pytest.mark.parametrize("kind", KINDS)
def test_one_picture_single_rounding(oracle, kind):
    import spiht_amd
    P, s, r, f = discriminating()
    c, H, W = P.shape
    ob, on, _ = oracle.encode_image(P, "bior2.2", "reflect", 3, 50.0, None, 40000)
    assert r.encoded_bytes == ob and r.max_n == on
    o = oracle.decode_image(ob, on, c, H, W, "bior2.2", 3, 50.0, None)[:, :H, :W]
    # without this the test could pass on a kernel that rounds twice
    for narrow in ("float16", "bfloat16"):
        n = int((bits(two_step(o, narrow)) != bits(conv(o, narrow))).sum())
        print("%s: %d of %d samples round differently in two steps" % (narrow, n, o.size))
        assert n >= 5
    assert f.shape == (c, H + 1, W + 1)
    got = spiht_amd.decode_image_float(r, s, dtype=kind)
    assert same(got, conv(f[:, :H, :W], kind)) and same(got, conv(o, kind))
    hwc = spiht_amd.decode_image_float(r, s, dtype=kind, channels_last=True)
    assert same(hwc, np.ascontiguousarray(got.transpose(1, 2, 0)))
    if kind == "float32":
        assert same(spiht_amd.decode_image_float(r, s), got) and same(spiht_amd.decode_image_float(r, s, np.float32), got)
    if kind == "float16":
        assert same(spiht_amd.decode_image_float(r, s, np.float16), got)
    with pytest.raises(TypeError):
        spiht_amd.decode_image_float(r, s, dtype=np.float64)


# ---- 3. routes -----------------------------------------------------------------------------------------------------------
ROUTES = [
    dict(color="IPT", q=1.0, mults=[50.0, 15.0, 15.0], level=3),       # colour change fused into level 1
    dict(color="IPT", mode="periodization", level=2),                    # ... in front of / behind a two-pass level
    dict(mode="smooth", level=2),
    dict(mode="antireflect", level=3),
    dict(wavelet="db11", level=2),                                       # a filter longer than the tiled kernels take
    dict(level=3, source="u8"),                                          # a stream from 8-bit pixels
    dict(level=3, source="f32"),                                         # ... and one from float32 pixels
]


@pytest.mark.parametrize("cfg", ROUTES)
def test_routes_vs_float64(cfg):
    import spiht_amd
    c, H, W = 3, 57, 83
    U = u16_image(31, c, H, W)
    s = settings(cfg)
    if cfg.get("source") == "u8":
        r = spiht_amd.encode_image_u8((U >> 8).astype(np.uint8), s, level=cfg["level"], max_bits=6000)
    elif cfg.get("source") == "f32":
        r = spiht_amd.encode_image((U / 65535).astype(np.float32), s, level=cfg["level"], max_bits=6000)
    else:
        r = spiht_amd.encode_image(U / 65535, s, level=cfg["level"], max_bits=6000)
    f = spiht_amd.decode_image(r, s)[:, :H, :W]
    for kind in KINDS:
        got = spiht_amd.decode_image_float(r, s, dtype=kind)
        assert same(got, conv(f, kind)), kind
        assert same(spiht_amd.decode_image_float(r, s, dtype=kind, channels_last=True), np.ascontiguousarray(got.transpose(1, 2, 0)))


# ---- 4. batch equals singles -------------------------------------------------------------------------------------------------
def test_batch_equals_singles():
    import spiht_amd
    from spiht_amd import floatpx
    from spiht_amd.batch import BatchCodec, DeviceArray
    B, c, H, W = 7, 3, 45, 61
    P = np.stack([pattern(100 + b, c, H, W) for b in range(B)])
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=3, max_bits=5000)
    ctx = codec.ctx
    res = codec.encode(P)
    f = codec.decode(res)[:, :, :H, :W]
    stride, d_in = codec._streams_on_device(res)
    try:
        for kind in KINDS:
            es, dt = floatpx.itemsize(kind), floatpx.storage_dtype(kind)
            dec = codec.decode_float(res, dtype=kind)
            assert dec.shape == (B, c, H, W) and dec.dtype == dt
            for b in range(B):
                assert same(dec[b], spiht_amd.decode_image_float(res[b], s, dtype=kind)), (kind, b)
            assert same(dec, conv(f, kind))
            assert same(codec.decode_float(res, dtype=kind, channels_last=True), np.ascontiguousarray(dec.transpose(0, 2, 3, 1)))
            # the device form into a padded four-channel buffer: the fourth channel and the row padding keep their bytes
            pitch = 4 * W * es + 12 * es
            host = np.full((B, H, pitch), 0x5A, np.uint8)
            st = (H * pitch, es, pitch, 4 * es)
            d_px = DeviceArray(ctx, host.shape, np.uint8)
            try:
                d_px.upload(host)
                codec.decode_device_float(d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, B, d_px.ptr, kind, strides=st, slot_stride=stride)
                ctx.synchronize()
                got = d_px.download()
            finally:
                d_px.free()
            px = got[:, :, :4 * W * es].reshape(B, H, W, 4, es)
            chan = np.ascontiguousarray(px[:, :, :, :3]).view(bits(dec).dtype).reshape(B, H, W, 3).transpose(0, 3, 1, 2)
            assert np.array_equal(chan, bits(dec)), kind
            assert (px[:, :, :, 3] == 0x5A).all() and (got[:, :, 4 * W * es:] == 0x5A).all()
            # refused before a launch (null pointers): overlapping strides, strides off the element, a base off the element
            with pytest.raises(ValueError):
                codec.decode_device_float(0, 0, 0, B, 0, kind, strides=(H * pitch, es, pitch, 2 * es))
            with pytest.raises(ValueError):
                codec.decode_device_float(0, 0, 0, B, 0, kind, strides=(H * pitch, es, pitch + es // 2, 4 * es))
            with pytest.raises(ValueError):
                codec.decode_device_float(0, 0, 0, B, es // 2, kind, strides=st)
            assert codec.L.spiht_decode_image_batch_flt(ctx.handle, floatpx.kind_arg(kind), None, stride, None, None, B, c, H, W,
                                                        codec.wid, codec.mid, 3, 50.0, None, C.c_void_p(es // 2), None, None) != 0
        with pytest.raises(TypeError):
            codec.decode_float(res, dtype=np.float64)
    finally:
        for d in d_in:
            d.free()


# ---- 5. the persistent inverse kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,flags,kind", [(None, 1, "float16"), (None, 0, "bfloat16"), (1, 1, "float32")])  # FLAGS / plain / FIRST
def test_persistent_inverse_at_batch_size(level, flags, kind):
    """BIG: 22 080 level-1 tiles, above the 20 000 from which the launcher takes the persistent inverse kernel, odd sizes"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    B, c, H, W = BIG
    base = [pattern(600 + i, c, H, W) for i in range(4)]
    P = np.stack([np.roll(base[b % 4], 5 * (b // 4), axis=2)[:, ::-1 if (b // 4) & 1 else 1, :] for b in range(B)])
    codec = BatchCodec(c, H, W, spiht_amd.SpihtSettings(), level=level, max_bits=int(H * W * 0.5))
    ctx = codec.ctx
    res = codec.encode(P)
    old = ctx.get_option("l1_flags")
    ctx.set_option("l1_flags", flags)
    try:
        f = codec.decode(res)[:, :, :H, :W]
        got = codec.decode_float(res, dtype=kind)
        hwc = codec.decode_float(res, dtype=kind, channels_last=True)
    finally:
        ctx.set_option("l1_flags", old)
    assert got.shape == (B, c, H, W)
    for b in range(B):
        assert same(got[b], conv(f[b], kind)), b
    assert np.array_equal(bits(hwc), bits(got).transpose(0, 2, 3, 1))


# ---- 6. reduced --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", [1, 2, 3])
def test_reduced(reduce):
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    P, s, r, f = discriminating()
    c, H, W = P.shape
    rs = spiht_amd.reduced_shape(H, W, s, 3, reduce)
    full = spiht_amd.decode_image_reduced(r, s, reduce)
    codec = BatchCodec(c, H, W, s, level=3, max_bits=40000)
    res = [r, spiht_amd.encode_image(pattern(1), s, level=3, max_bits=40000), r]
    ph, pw = rs["pic_h"], rs["pic_w"]
    # the float64 pictures the float kinds are held to: cropped to the band as the integer forms are, or the centred window
    f64 = {False: full[:, :ph, :pw], True: spiht_amd.decode_image_reduced(r, s, reduce, crop=True)}
    assert f64[True].shape == (c, rs["in_h"], rs["in_w"])
    for kind in KINDS:
        for crop in (False, True):
            wc = conv(f64[crop], kind)
            g = spiht_amd.decode_image_reduced_float(r, s, reduce, dtype=kind, crop=crop)
            assert same(np.ascontiguousarray(g), wc), (kind, crop)
            g = spiht_amd.decode_image_reduced_float(r, s, reduce, dtype=kind, crop=crop, channels_last=True)
            assert same(np.ascontiguousarray(g), np.ascontiguousarray(wc.transpose(1, 2, 0))), (kind, crop)
            b = codec.decode_reduced_float(res, reduce, dtype=kind, crop=crop)
            assert same(np.ascontiguousarray(b[0]), wc) and same(np.ascontiguousarray(b[2]), wc), (kind, crop)
            wb = conv(codec.decode_reduced(res, reduce, crop=crop)[:, :, :wc.shape[1], :wc.shape[2]], kind)
            assert same(np.ascontiguousarray(b), wb), (kind, crop)
            bl = codec.decode_reduced_float(res, reduce, dtype=kind, crop=crop, channels_last=True)
            assert same(np.ascontiguousarray(bl), np.ascontiguousarray(wb.transpose(0, 2, 3, 1))), (kind, crop)


# ---- 7. tiled ----------------------------------------------------------------------------------------------------------------
WINDOWS = [(0, 0, 9, 11), (0, 79, 9, 11), (61, 0, 9, 11), (61, 79, 9, 11),   # the corners
           (33, 47, 1, 1),                                                    # one pixel
           (5, 40, 10, 12),                                                   # inside one tile
           (28, 30, 10, 8),                                                   # a four-tile corner
           (32, 0, 32, 90),                                                   # a full row of tiles
           (60, 80, 10, 10)]                                                  # the padded bottom-right edge


@functools.lru_cache(maxsize=None)
def tiled(overlap=0, tile=32):
    import spiht_amd
    c, H, W = 3, 70, 90
    P = synth_image(4000 + H + W + c, c, H, W) * 1.5 - 0.2  # (values outside [0, 1]: nothing clips them)
    s = spiht_amd.SpihtSettings()
    codec = spiht_amd.TiledCodec(c, H, W, tile, s, None, 27005, overlap=overlap)
    return P, s, codec, codec.encode(P)


@pytest.mark.parametrize("kind", KINDS)
def test_tiled_whole_windows_reduced(kind):
    import spiht_amd
    P, s, codec, res = tiled()
    dec = codec.decode(res)
    n_all = codec.last_tiles_decoded
    got = codec.decode_float(res, dtype=kind)
    assert codec.last_tiles_decoded == n_all == 9
    assert got.shape == (3, 70, 90) and same(got, conv(dec, kind))
    assert same(codec.decode_float(res, dtype=kind, channels_last=True), np.ascontiguousarray(got.transpose(1, 2, 0)))
    assert same(spiht_amd.decode_image_tiled_float(res, s, dtype=kind), got)
    for y0, x0, h, w in WINDOWS:
        want = conv(codec.decode_window(res, y0, x0, h, w), kind)
        n = codec.last_tiles_decoded
        g = codec.decode_window_float(res, y0, x0, h, w, dtype=kind)
        assert codec.last_tiles_decoded == n
        assert same(g, want) and same(g, np.ascontiguousarray(got[:, y0:y0 + h, x0:x0 + w])), (y0, x0, h, w)
        g = codec.decode_window_float(res, y0, x0, h, w, dtype=kind, channels_last=True)
        assert same(g, np.ascontiguousarray(want.transpose(1, 2, 0))), (y0, x0, h, w)
    assert same(spiht_amd.decode_image_window_float(res, s, 28, 30, 10, 8, dtype=kind), conv(dec[:, 28:38, 30:38], kind))
    # reduce = 1: the mosaic of the tiles' reduced decodes
    r1 = codec.decode(res, reduce=1)
    g1 = codec.decode_float(res, dtype=kind, reduce=1)
    assert g1.shape == (3, 35, 45) and same(g1, conv(r1, kind))
    assert same(codec.decode_float(res, dtype=kind, channels_last=True, reduce=1), np.ascontiguousarray(g1.transpose(1, 2, 0)))
    assert same(codec.decode_window_float(res, 14, 15, 6, 7, dtype=kind, reduce=1), conv(codec.decode_window(res, 14, 15, 6, 7, reduce=1), kind))
    # (24, 40) tiles once
    P2, s2, codec2, res2 = tiled(0, (24, 40))
    assert same(codec2.decode_float(res2, dtype=kind), conv(codec2.decode(res2), kind))


@pytest.mark.parametrize("kind", KINDS)
def test_tiled_layers(kind):
    import spiht_amd
    c, H, W = 3, 70, 90
    P, s, _, _ = tiled()
    codec = spiht_amd.TiledCodec(c, H, W, 32, s, None, 27005, allocate="rd")
    lay = codec.encode_layered(P, [9000, 27005])
    for upto in (1, None):
        want = conv(codec.decode_layered(lay, upto=upto), kind)
        n = codec.last_tiles_decoded
        got = codec.decode_layered_float(lay, upto=upto, dtype=kind)
        assert codec.last_tiles_decoded == n and same(got, want), upto
        assert same(codec.decode_layered_float(lay, upto=upto, dtype=kind, channels_last=True), np.ascontiguousarray(want.transpose(1, 2, 0)))
        ww = conv(codec.decode_layered_window(lay, 28, 30, 10, 8, upto=upto), kind)
        n = codec.last_tiles_decoded
        assert same(codec.decode_layered_window_float(lay, 28, 30, 10, 8, upto=upto, dtype=kind), ww)
        assert codec.last_tiles_decoded == n == 4
        assert same(spiht_amd.decode_image_layered_float(lay, s, upto=upto, dtype=kind), want)
        assert same(spiht_amd.decode_image_layered_window_float(lay, s, 28, 30, 10, 8, upto=upto, dtype=kind), ww)


@pytest.mark.parametrize("kind", KINDS)
def test_tiled_overlap(kind):
    P, s, codec, res = tiled(4)
    want = conv(codec.decode(res), kind)
    n = codec.last_tiles_decoded
    got = codec.decode_float(res, dtype=kind)
    assert codec.last_tiles_decoded == n == 9 and same(got, want)
    assert same(codec.decode_float(res, dtype=kind, channels_last=True), np.ascontiguousarray(want.transpose(1, 2, 0)))
    y0, x0, h, w = 30, 29, 12, 40  # begins inside the seam zones of rows 28 .. 35 and columns 28 .. 35
    ww = conv(codec.decode_window(res, y0, x0, h, w), kind)
    n = codec.last_tiles_decoded
    g = codec.decode_window_float(res, y0, x0, h, w, dtype=kind)
    assert codec.last_tiles_decoded == n and same(g, ww) and same(g, np.ascontiguousarray(got[:, y0:y0 + h, x0:x0 + w]))
    assert same(codec.decode_window_float(res, y0, x0, h, w, dtype=kind, channels_last=True), np.ascontiguousarray(ww.transpose(1, 2, 0)))
