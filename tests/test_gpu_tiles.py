"""Tiled pictures on the GPU: every tile stream is the single-image encode of the tile's pixels (and the oracle's), a tiled
decode is the numpy paste of the tiles' decodes, a window decodes only the tiles it meets, and the four copy kernels
(cut, paste, pack, unpack) equal their numpy statements through the C ABI."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_image
from tile_helpers import dev, padded, settings, tile_of, tile_pixels

pytestmark = pytest.mark.gpu

vp = C.c_void_p


def same_result(a, b):
    assert (a.encoded_bytes, a.h, a.w, a.c, a.max_n, a.level, a._encoding_version) == \
        (b.encoded_bytes, b.h, b.w, b.c, b.max_n, b.level, b._encoding_version)


def same_tiled(a, b):
    assert (a.h, a.w, a.c, a.th, a.tw, a.level, a.max_n, a.nbytes, a.encoded_bytes, a._encoding_version) == \
        (b.h, b.w, b.c, b.th, b.tw, b.level, b.max_n, b.nbytes, b.encoded_bytes, b._encoding_version)


def to_int(dec, dtype):
    """the contract's formula of the integer decodes: clip, scale, truncate"""
    return (np.clip(dec, 0.0, 1.0) * float(np.iinfo(dtype).max)).astype(dtype)


# the smallest shapes at which each thing can go wrong
CASES = {
    "grid3x3": dict(c=3, H=70, W=90, tile=32, max_bits=27005),                 # 26 padded rows, 6 padded columns
    "nopad": dict(c=1, H=64, W=96, tile=32, max_bits=None),
    "single": dict(c=3, H=20, W=27, tile=32, max_bits=4001),                   # one padded tile
    "oddtile": dict(c=1, H=70, W=90, tile=(33, 40), max_bits=20000),           # rec_h = 34: the crop in paste
    "bior44": dict(c=1, H=70, W=90, tile=32, max_bits=27005, wavelet="bior4.4", mode="symmetric"),
    "ipt": dict(c=3, H=70, W=90, tile=32, max_bits=27005, color="IPT"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """the picture, codec, tiled result and tiled decode of a case: computed once, shared, never changed"""
    import spiht_amd
    cfg = CASES[name]
    c, H, W = cfg["c"], cfg["H"], cfg["W"]
    P = synth_image(4000 + H + W + c, c, H, W)
    P.setflags(write=False)
    s = settings(cfg)
    codec = spiht_amd.TiledCodec(c, H, W, cfg["tile"], s, cfg.get("level"), cfg["max_bits"])
    res = codec.encode(P)
    dec = codec.decode(res)
    dec.setflags(write=False)
    return cfg, P, s, codec, res, dec


@pytest.mark.parametrize("name", list(CASES))
def test_per_tile_parity(oracle, name):
    import spiht_amd
    from spiht_amd import _lib, color_models
    cfg, P, s, codec, res, dec = case(name)
    c, H, W = P.shape
    th, tw = tile_of(cfg["tile"])
    gy, gx = spiht_amd.tile_grid(H, W, th, tw)
    T = gy * gx
    assert (res.h, res.w, res.c, res.th, res.tw, res.level) == (H, W, c, th, tw, cfg.get("level"))
    assert len(res.nbytes) == len(res.max_n) == T and sum(res.nbytes) == len(res.encoded_bytes)
    budget = None if cfg["max_bits"] is None else cfg["max_bits"] // T
    want = np.zeros((c, gy * th, gx * tw))
    for i in range(gy):
        for j in range(gx):
            px = tile_pixels(P, th, tw, i, j)
            t = res.tile(i, j)
            same_result(t, spiht_amd.encode_image(px, s, cfg.get("level"), budget))
            opx = px
            if cfg.get("color"):  # the oracle has no colour step: it codes the pixels in the device's own IPT
                d = dev(px[None])
                color_models.device_convert(_lib.default_context(), d.ptr, 1, th * tw, "RGB", cfg["color"])
                _lib.default_context().synchronize()
                opx = d.download()[0]
            ob, on, _ = oracle.encode_image(opx, s.wavelet, s.mode, cfg.get("level"), s.quantization_scale, None, budget)
            assert t.encoded_bytes == ob and t.max_n == on, (i, j)
            want[:, i * th:(i + 1) * th, j * tw:(j + 1) * tw] = spiht_amd.decode_image(t, s)[:, :th, :tw]
    assert dec.shape == (c, H, W) and dec.dtype == np.float64
    assert np.array_equal(dec, want[:, :H, :W])
    # the conveniences are the same calls
    same_tiled(spiht_amd.encode_image_tiled(P, cfg["tile"], s, cfg.get("level"), cfg["max_bits"]), res)
    assert np.array_equal(spiht_amd.decode_image_tiled(res, s), dec)
    assert np.array_equal(codec.decode(spiht_amd.TiledResult.from_bytes(res.to_bytes())), dec)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_integer_pixels(dtype):
    """3 x 37 x 53: unaligned row starts.  Encode equals the float64 form of P / peak; decode the clip-scale-truncate
    formula; CHW, HWC and RGBA views"""
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    ctx = _lib.default_context()
    peak = int(np.iinfo(dtype).max)
    es = np.dtype(dtype).itemsize
    c, H, W, tile = 3, 37, 53, 32
    P = np.round(synth_image(77, c, H, W) * peak).astype(dtype)
    s = spiht_amd.SpihtSettings()
    codec = spiht_amd.TiledCodec(c, H, W, tile, s, 2, 24000)
    T = codec.T
    u = "u8" if es == 1 else "u16"
    ref = codec.encode(P / peak)
    same_tiled(getattr(codec, "encode_" + u)(P), ref)
    same_tiled(getattr(codec, "encode_" + u)(np.ascontiguousarray(P.transpose(1, 2, 0)), channels_last=True), ref)
    same_tiled(getattr(spiht_amd, "encode_image_tiled_" + u)(P, tile, s, 2, 24000), ref)
    # an RGBA buffer on the device, cut as it lies
    rgba = np.full((H, W, 4), 77, dtype)
    rgba[..., :3] = P.transpose(1, 2, 0)
    d_rgba = dev(rgba)
    d_packed = DeviceArray(ctx, (T * codec.codec.slot_stride,), np.uint8)
    d_lens, d_maxn = DeviceArray(ctx, (T,), np.uint32), DeviceArray(ctx, (T,), np.uint8)
    codec.encode_device(d_rgba, 1, d_packed, d_lens, d_maxn, strides=(0, es, W * 4 * es, 4 * es))
    ctx.synchronize()
    assert d_lens.download().tolist() == ref.nbytes and d_maxn.download().tolist() == ref.max_n
    assert d_packed.download()[:len(ref.encoded_bytes)].tobytes() == ref.encoded_bytes
    # decode
    want = to_int(codec.decode(ref), dtype)
    got = getattr(codec, "decode_" + u)(ref)
    assert got.dtype == dtype and got.shape == (c, H, W) and np.array_equal(got, want)
    hwc = getattr(codec, "decode_" + u)(ref, channels_last=True)
    assert hwc.shape == (H, W, c) and np.array_equal(hwc, want.transpose(1, 2, 0))
    assert np.array_equal(getattr(spiht_amd, "decode_image_tiled_" + u)(ref, s), want)
    d_out = dev(np.full((H, W, 4), 77, dtype))
    codec.decode_device(d_packed, len(ref.encoded_bytes), d_lens, d_maxn, d_out, strides=(es, W * 4 * es, 4 * es))
    ctx.synchronize()
    out = d_out.download()
    assert np.array_equal(out[..., :3], want.transpose(1, 2, 0)) and (out[..., 3] == 77).all()
    # a window into an RGBA buffer keeps its alpha, too
    y0, x0, h, w = 30, 28, 7, 25
    d_win = dev(np.full((h, w, 4), 77, dtype))
    sub = spiht_amd.window_tiles(H, W, tile, tile, y0, x0, h, w)
    ts = [i * codec.gx + j for i in range(sub[0], sub[1]) for j in range(sub[2], sub[3])]
    off = np.concatenate(([0], np.cumsum(ref.nbytes)))
    run = b"".join(ref.encoded_bytes[off[t]:off[t + 1]] for t in ts)
    codec.decode_window_device(dev(np.frombuffer(run, np.uint8)), len(run), dev(np.array([ref.nbytes[t] for t in ts], np.uint32)),
                               dev(np.array([ref.max_n[t] for t in ts], np.uint8)), sub, (y0, x0, h, w), d_win,
                               strides=(es, w * 4 * es, 4 * es))
    ctx.synchronize()
    out = d_win.download()
    assert codec.last_tiles_decoded == len(ts) == 4
    assert np.array_equal(out[..., :3], want[:, y0:y0 + h, x0:x0 + w].transpose(1, 2, 0)) and (out[..., 3] == 77).all()
    assert np.array_equal(getattr(codec, "decode_window_" + u)(ref, y0, x0, h, w), want[:, y0:y0 + h, x0:x0 + w])
    assert np.array_equal(getattr(spiht_amd, "decode_image_window_" + u)(ref, s, y0, x0, h, w, channels_last=True),
                          want[:, y0:y0 + h, x0:x0 + w].transpose(1, 2, 0))


def test_float32_pixels():
    """float32 in: every tile is encode_image of the float32 tile (the single-precision transform)"""
    import spiht_amd
    c, H, W, tile = 3, 37, 53, 32
    P = synth_image(78, c, H, W).astype(np.float32)
    s = spiht_amd.SpihtSettings()
    codec = spiht_amd.TiledCodec(c, H, W, tile, s, 2, 24000, pixel_dtype=np.float32)
    res = codec.encode(P)
    same_tiled(spiht_amd.encode_image_tiled(P, tile, s, 2, 24000), res)
    for i in range(codec.gy):
        for j in range(codec.gx):
            px = tile_pixels(P, tile, tile, i, j)
            assert px.dtype == np.float32
            same_result(res.tile(i, j), spiht_amd.encode_image(px, s, 2, 24000 // codec.T))
    assert codec.decode(res).shape == (c, H, W)


WINDOWS = {
    "inside one tile": (5, 40, 10, 12),
    "a four-tile corner": (28, 30, 10, 8),
    "a full row of tiles": (32, 0, 32, 90),
    "the padded bottom-right edge": (60, 80, 10, 10),
    "the whole picture": (0, 0, 70, 90),
}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_windows(name):
    import spiht_amd
    cfg, P, s, codec, res, dec = case("grid3x3")
    y0, x0, h, w = WINDOWS[name]
    th, tw = tile_of(cfg["tile"])
    count = len(set(np.arange(y0, y0 + h) // th)) * len(set(np.arange(x0, x0 + w) // tw))
    assert count == {"inside one tile": 1, "a four-tile corner": 4, "a full row of tiles": 3,
                     "the padded bottom-right edge": 2, "the whole picture": 9}[name]
    got = codec.decode_window(res, y0, x0, h, w)
    assert got.shape == (3, h, w) and np.array_equal(got, dec[:, y0:y0 + h, x0:x0 + w])
    assert codec.last_tiles_decoded == count
    assert np.array_equal(spiht_amd.decode_image_window(res, s, y0, x0, h, w), got)
    want8 = to_int(dec, np.uint8)[:, y0:y0 + h, x0:x0 + w]
    assert np.array_equal(codec.decode_window_u8(res, y0, x0, h, w), want8)
    assert codec.last_tiles_decoded == count
    assert np.array_equal(codec.decode_window_u16(res, y0, x0, h, w, channels_last=True),
                          to_int(dec, np.uint16)[:, y0:y0 + h, x0:x0 + w].transpose(1, 2, 0))
    # an RGBA output view keeps its alpha bytes
    from spiht_amd import _lib
    sub = spiht_amd.window_tiles(70, 90, th, tw, y0, x0, h, w)
    ts = [i * codec.gx + j for i in range(sub[0], sub[1]) for j in range(sub[2], sub[3])]
    off = np.concatenate(([0], np.cumsum(res.nbytes)))
    run = b"".join(res.encoded_bytes[off[t]:off[t + 1]] for t in ts)
    d_win = dev(np.full((h, w, 4), 201, np.uint8))
    codec.decode_window_device(dev(np.frombuffer(run, np.uint8)), len(run), dev(np.array([res.nbytes[t] for t in ts], np.uint32)),
                               dev(np.array([res.max_n[t] for t in ts], np.uint8)), sub, (y0, x0, h, w), d_win,
                               strides=(1, w * 4, 4))
    _lib.default_context().synchronize()
    out = d_win.download()
    assert np.array_equal(out[..., :3], want8.transpose(1, 2, 0)) and (out[..., 3] == 201).all()
    assert codec.last_tiles_decoded == count


def test_window_that_leaves_the_picture():
    cfg, P, s, codec, res, dec = case("grid3x3")
    for bad in [(61, 0, 10, 5), (0, 81, 5, 10), (-1, 0, 5, 5), (0, 0, 0, 5), (0, 0, 71, 90)]:
        with pytest.raises(ValueError):
            codec.decode_window(res, *bad)


# ---- the kernels on their own, through the C ABI -----------------------------------------------------------------------

DTYPES = {1: np.uint8, 2: np.uint16, 4: np.float32, 8: np.float64}
SENTINEL = {1: 0xA5, 2: 0xA5A5, 4: -7.25, 8: -7.25}


def rand_array(rng, shape, es):
    if es <= 2:
        return rng.integers(0, np.iinfo(DTYPES[es]).max + 1, shape).astype(DTYPES[es])
    return rng.standard_normal(shape).astype(DTYPES[es])


def cut_fn(es):
    from spiht_amd import _lib
    return getattr(_lib.lib(), "spiht_tile_cut_" + {1: "u8", 2: "u16", 4: "f32", 8: "f64"}[es])


def paste_fn(es):
    from spiht_amd import _lib
    return getattr(_lib.lib(), "spiht_tile_paste_" + {1: "u8", 2: "u16", 4: "f32", 8: "f64"}[es])


def numpy_cut(P, th, tw):
    N, c, H, W = P.shape
    Q = padded(P, th, tw)
    gy, gx = Q.shape[2] // th, Q.shape[3] // tw
    return Q.reshape(N, c, gy, th, gx, tw).transpose(0, 2, 4, 1, 3, 5).reshape(N * gy * gx, c, th, tw)


CUT_SHAPES = [(2, 3, 37, 53, 16, 24), (1, 1, 20, 27, 32, 32), (1, 2, 70, 90, 33, 40), (1, 1, 300, 700, 256, 512)]


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_cut_kernel(es):
    """cut == np.pad(mode="edge") + the reshape, for every element size; both arrays one element off a 16-byte boundary,
    with sentinels around the output; the integer forms also through HWC and RGBA views"""
    from spiht_amd import _lib
    ctx = _lib.default_context()
    rng = np.random.default_rng(es)
    for (N, c, H, W, th, tw) in CUT_SHAPES:
        P = rand_array(rng, (N, c, H, W), es)
        want = numpy_cut(P, th, tw)
        views = [("chw", P.reshape(-1), None)]
        if es <= 2:
            hwc = np.ascontiguousarray(P.transpose(0, 2, 3, 1))
            views.append(("hwc", hwc.reshape(-1), (H * W * c * es, es, W * c * es, c * es)))
            if c == 3:
                rgba = np.zeros((N, H, W, 4), P.dtype)
                rgba[..., :3] = hwc
                views.append(("rgba", rgba.reshape(-1), (H * W * 4 * es, es, W * 4 * es, 4 * es)))
        for name, flat, strides in views:
            for shift in (0, 1):
                d_in = dev(np.concatenate([np.zeros(shift, P.dtype), flat]))
                guard = np.full(want.size + 2 * 16, SENTINEL[es], dtype=P.dtype)
                d_out = dev(guard)
                args = [ctx.handle, vp(d_in.ptr + shift * es)]
                if es <= 2:
                    st = None if strides is None else np.array(strides, np.int64)
                    args.append(None if st is None else vp(st.ctypes.data))
                _lib.check(cut_fn(es)(*args, N, c, H, W, th, tw, vp(d_out.ptr + (16 - shift) * es)))
                ctx.synchronize()
                got = d_out.download()
                body = got[16 - shift:16 - shift + want.size].reshape(want.shape)
                assert np.array_equal(body, want), (name, shift, (N, c, H, W, th, tw))
                assert (got[:16 - shift] == guard[0]).all() and (got[16 - shift + want.size:] == guard[0]).all()


def numpy_paste(out, tiles, th, tw, i0, j0, nj, y0, x0):
    """out [c, wh, ww] at (y0, x0) <- every sample from the tile that owns it; tiles [n, c, rh, rw]"""
    c, wh, ww = out.shape
    for y in range(wh):
        for x in range(ww):
            i, j = (y0 + y) // th, (x0 + x) // tw
            out[:, y, x] = tiles[(i - i0) * nj + (j - j0), :, y0 + y - i * th, x0 + x - j * tw]
    return out


PASTE_CASES = [  # (c, H, W, th, tw, rh, rw, sub-grid, window)
    (3, 70, 90, 32, 32, 32, 32, (0, 3, 0, 3), (0, 0, 70, 90)),       # the whole picture from cropped tiles
    (1, 70, 90, 33, 40, 34, 41, (0, 3, 0, 3), (0, 0, 70, 90)),       # tiles one longer: the crop
    (3, 70, 90, 32, 32, 33, 33, (0, 2, 0, 2), (28, 30, 10, 8)),      # a four-tile corner
    (2, 70, 90, 32, 32, 33, 33, (0, 3, 1, 3), (5, 40, 60, 45)),      # a sub-grid larger than the window needs
    (1, 20, 27, 32, 32, 33, 33, (0, 1, 0, 1), (3, 5, 17, 22)),       # inside a single padded tile
    (1, 300, 700, 256, 512, 257, 513, (0, 2, 0, 2), (1, 3, 299, 697)),
]


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_paste_kernel(es):
    """paste == the numpy paste into an output pre-filled with a sentinel; nothing outside the window changes"""
    from spiht_amd import _lib
    ctx = _lib.default_context()
    rng = np.random.default_rng(10 + es)
    dt = DTYPES[es]
    for (c, H, W, th, tw, rh, rw, sub, win) in PASTE_CASES:
        i0, i1, j0, j1 = sub
        y0, x0, wh, ww = win
        n = (i1 - i0) * (j1 - j0)
        tiles = rand_array(rng, (n, c, rh, rw), es)
        want = numpy_paste(np.zeros((c, wh, ww), dt), tiles, th, tw, i0, j0, j1 - j0, y0, x0) if wh * ww < 10000 else None
        if want is None:  # the large case: by slices
            want = np.zeros((c, wh, ww), dt)
            full = np.zeros((c, (i1 - i0) * th, (j1 - j0) * tw), dt)
            for k in range(n):
                i, j = divmod(k, j1 - j0)
                full[:, i * th:(i + 1) * th, j * tw:(j + 1) * tw] = tiles[k, :, :th, :tw]
            want[:] = full[:, y0 - i0 * th:y0 - i0 * th + wh, x0 - j0 * tw:x0 - j0 * tw + ww]
        d_tiles = dev(tiles)
        layouts = [("chw", (c, wh, ww), None, lambda a: a)]
        if es <= 2:
            layouts.append(("hwc", (wh, ww, c), (es, ww * c * es, c * es), lambda a: a.transpose(2, 0, 1)))
            if c == 3:
                layouts.append(("rgba", (wh, ww, 4), (es, ww * 4 * es, 4 * es), lambda a: a[..., :3].transpose(2, 0, 1)))
        for name, shape, strides, view in layouts:
            for shift in (0, 1):
                size = int(np.prod(shape))
                guard = np.full(size + 32, SENTINEL[es], dt)
                d_out = dev(guard)
                args = [ctx.handle, vp(d_tiles.ptr), c, rh, rw, H, W, th, tw, i0, i1, j0, j1, y0, x0, wh, ww,
                        vp(d_out.ptr + (16 - shift) * es)]
                if es <= 2:
                    st = None if strides is None else np.array(strides, np.int64)
                    args.append(None if st is None else vp(st.ctypes.data))
                _lib.check(paste_fn(es)(*args))
                ctx.synchronize()
                got = d_out.download()
                body = got[16 - shift:16 - shift + size].reshape(shape)
                assert np.array_equal(view(body), want), (name, shift, win)
                if name == "rgba":
                    assert (body[..., 3] == guard[0]).all()
                assert (got[:16 - shift] == guard[0]).all() and (got[16 - shift + size:] == guard[0]).all()
    # a window that leaves the picture, a sub-grid that misses a tile of the window: refused before anything is queued
    d_tiles, d_out = dev(np.zeros((4, 1, 32, 32), dt)), dev(np.zeros((1, 70, 90), dt))
    tail = [None] if es <= 2 else []
    for sub, win in [((0, 2, 0, 2), (60, 0, 11, 5)), ((0, 1, 0, 2), (28, 30, 10, 8)), ((0, 2, 1, 2), (28, 30, 10, 8)),
                     ((0, 4, 0, 1), (0, 0, 5, 5))]:
        assert paste_fn(es)(ctx.handle, vp(d_tiles.ptr), 1, 32, 32, 70, 90, 32, 32, *sub, *win, vp(d_out.ptr), *tail) == _lib.ERR_ARG
    assert paste_fn(es)(ctx.handle, vp(d_tiles.ptr), 1, 31, 32, 70, 90, 32, 32, 0, 2, 0, 2, 28, 30, 10, 8, vp(d_out.ptr), *tail) == _lib.ERR_ARG


@pytest.mark.parametrize("lengths", [[0, 1, 7, 4096, 0, 33], [5], [0], [4100, 4099, 17, 16, 15, 31, 32]])
def test_pack_unpack_kernels(lengths):
    """pack == host concatenation (+ the table), unpack its inverse into zero-padded slots; sentinels around both outputs;
    the run also one byte off its alignment"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    rng = np.random.default_rng(len(lengths))
    T, stride = len(lengths), 4100
    slots = rng.integers(1, 256, (T, stride), dtype=np.uint8)  # no zero byte: what unpack zeroes shows
    nbits = np.array([8 * n - (3 if n else 0) for n in lengths], np.uint64)  # a last byte that is not full
    concat = b"".join(slots[t, :n].tobytes() for t, n in enumerate(lengths))
    d_slots, d_nbits = dev(slots), dev(nbits)
    for shift in (0, 1):
        guard = np.full(len(concat) + 64, 0xEE, np.uint8)
        d_packed, d_lens = dev(guard), dev(np.full(T + 2, 0xFFFFFFFF, np.uint32))
        _lib.check(L.spiht_tile_pack(ctx.handle, vp(d_slots.ptr), stride, vp(d_nbits.ptr), T, vp(d_packed.ptr + 32 + shift),
                                     len(concat), vp(d_lens.ptr + 4)))
        ctx.synchronize()
        got, lens = d_packed.download(), d_lens.download()
        assert lens.tolist() == [0xFFFFFFFF] + lengths + [0xFFFFFFFF]
        assert got[32 + shift:32 + shift + len(concat)].tobytes() == concat
        assert (got[:32 + shift] == 0xEE).all() and (got[32 + shift + len(concat):] == 0xEE).all()
        # ... and back: the run read at the same (mis)alignment
        d_back = dev(np.full(T * stride + 64, 0xAA, np.uint8))
        d_nbytes = dev(np.full(T + 2, 2 ** 64 - 1, np.uint64))
        _lib.check(L.spiht_tile_unpack(ctx.handle, vp(d_packed.ptr + 32 + shift), len(concat), vp(d_lens.ptr + 4), T,
                                       vp(d_back.ptr + 32), stride, vp(d_nbytes.ptr + 8)))
        ctx.synchronize()
        back, nb = d_back.download(), d_nbytes.download()
        assert nb.tolist() == [2 ** 64 - 1] + lengths + [2 ** 64 - 1]
        body = back[32:32 + T * stride].reshape(T, stride)
        for t, n in enumerate(lengths):
            assert np.array_equal(body[t, :n], slots[t, :n]), t
            assert not body[t, n:].any(), t  # slot bytes past a stream's end are zero
        assert (back[:32] == 0xAA).all() and (back[32 + T * stride:] == 0xAA).all()
    # a capacity smaller than the run: nothing is written at or past it, the table still tells the lengths
    if len(concat) > 8:
        cap = len(concat) - 5
        d_packed = dev(np.full(len(concat) + 64, 0xEE, np.uint8))
        d_lens = dev(np.zeros(T, np.uint32))
        _lib.check(L.spiht_tile_pack(ctx.handle, vp(d_slots.ptr), stride, vp(d_nbits.ptr), T, vp(d_packed.ptr + 32), cap, vp(d_lens.ptr)))
        ctx.synchronize()
        got = d_packed.download()
        assert got[32:32 + cap].tobytes() == concat[:cap] and (got[32 + cap:] == 0xEE).all() and d_lens.download().tolist() == lengths
    assert L.spiht_tile_pack(ctx.handle, vp(d_slots.ptr), 4098, vp(d_nbits.ptr), T, vp(d_slots.ptr), 1, vp(d_nbits.ptr)) == _lib.ERR_ARG


# ---- other checks -------------------------------------------------------------------------------------------------------

def test_three_pictures_in_one_call():
    import spiht_amd
    c, H, W, tile = 3, 37, 53, 32
    Ps = np.stack([synth_image(90 + k, c, H, W) for k in range(3)])
    codec = spiht_amd.TiledCodec(c, H, W, tile, None, 2, 24000)
    many = codec.encode(Ps)
    assert isinstance(many, list) and len(many) == 3
    for k in range(3):
        same_tiled(many[k], codec.encode(Ps[k]))
    P8 = np.round(Ps * 255).astype(np.uint8)
    many8 = codec.encode_u8(P8)
    for k in range(3):
        same_tiled(many8[k], many[k])


def test_tiled_calls_leave_nothing_behind(oracle):
    """after a tiled encode and decode (colour model included) on a context, the ordinary calls on it still equal the oracle"""
    import spiht_amd
    for name in ("ipt", "grid3x3"):
        cfg, P, s, codec, res, dec = case(name)
        codec.decode_window(codec.encode(P), 28, 30, 10, 8)
        img = synth_image(1000, 3, 96, 160)
        plain = spiht_amd.SpihtSettings()
        enc = spiht_amd.encode_image(img, plain, level=3, max_bits=7680)
        ob, on, _ = oracle.encode_image(img, "bior2.2", "reflect", 3, 50.0, None, 7680)
        assert enc.encoded_bytes == ob and enc.max_n == on
        assert np.array_equal(spiht_amd.decode_image(enc, plain), oracle.decode_image(ob, on, 3, 96, 160, "bior2.2", 3, 50.0, None))


@pytest.mark.parametrize("max_bits", [None, 3])
def test_budget_edges_round_trip(max_bits):
    """max_bits=None stays None for every tile; a budget so small that max_bits // T is 0 is what encode_image does with 0"""
    import spiht_amd
    c, H, W, tile = 1, 40, 50, 32
    P = synth_image(5, c, H, W)
    s = spiht_amd.SpihtSettings()
    codec = spiht_amd.TiledCodec(c, H, W, tile, s, 2, max_bits)
    res = codec.encode(P)
    assert codec.T == 4
    for i in range(codec.gy):
        for j in range(codec.gx):
            same_result(res.tile(i, j), spiht_amd.encode_image(tile_pixels(P, tile, tile, i, j), s, 2, None if max_bits is None else 0))
    dec = codec.decode(res)
    assert dec.shape == (c, H, W) and np.isfinite(dec).all()
    assert np.array_equal(spiht_amd.decode_image_tiled(spiht_amd.TiledResult.from_bytes(res.to_bytes()), s), dec)


def test_refused_as_a_tile_sized_picture_is_refused():
    """what encode_image refuses for a th x tw picture, the constructor refuses the same way, before anything is queued"""
    import spiht_amd
    from spiht_amd import _lib
    s = spiht_amd.SpihtSettings()
    with pytest.raises(ValueError):
        spiht_amd.TiledCodec(1, 70, 90, 4, s)
    with pytest.raises(ValueError):
        spiht_amd.TiledCodec(1, 70, 90, 32, s, level=-1)
    with pytest.raises(ValueError):
        spiht_amd.TiledCodec(1, 70, 90, 32, spiht_amd.SpihtSettings(wavelet="nope"))
    with pytest.raises(_lib.PanicException):  # level 0: the root block's offspring fall outside the array
        spiht_amd.encode_image(np.zeros((1, 32, 32)), s, 0, 100)
    with pytest.raises(_lib.PanicException):
        spiht_amd.TiledCodec(1, 70, 90, 32, s, level=0)


def test_command_line_tile_and_window(tmp_path):
    """python -m spiht_amd.encode_decode IMAGE --tile N [--window Y0,X0,H,W]: the files hold the tiled decode and its window"""
    import spiht_amd
    from spiht_amd.encode_decode import build_parser, main
    from spiht_amd.utils import imload, imsave
    src = str(tmp_path / "in.png")
    imsave(src, synth_image(6, 3, 70, 90))
    P = imload(src)
    common = [src, "--bpp", "2.0", "--tile", "32", "--color_model", "RGB", "--per_channel_quant_scales", "1.,1.,1."]
    enc, dec = main(build_parser().parse_args(common + ["--out", str(tmp_path / "all.png")]))
    assert isinstance(enc, spiht_amd.TiledResult) and enc.grid() == (3, 3) and dec.shape == (3, 70, 90)
    s = spiht_amd.SpihtSettings(quantization_scale=255.0, per_channel_quant_scales=[1.0, 1.0, 1.0])
    same_tiled(enc, spiht_amd.encode_image_tiled(P, 32, s, 2, round(2.0 * 70 * 90)))
    assert np.array_equal(dec, spiht_amd.decode_image_tiled(enc, s))
    _, win = main(build_parser().parse_args(common + ["--window", "28,30,10,8", "--out", str(tmp_path / "win.png")]))
    assert np.array_equal(win, dec[:, 28:38, 30:38])
    assert imload(str(tmp_path / "win.png")).shape == (3, 10, 8)


# ---- refusals: a foreign result, a wrong output or picture array, a reduce that is no level ----------------------------------

PIN = dict(c=1, H=70, W=90, tile=32)
# one of H, W, c, th, tw changed at a time
FOREIGN = [dict(H=71), dict(W=91), dict(c=2), dict(tile=(40, 32)), dict(tile=(32, 40))]


@functools.lru_cache(maxsize=None)
def pinned(overlap, **change):
    """the codecs of PIN (or of PIN with one thing changed) with that overlap: a plain one and an allocate="rd" one, the tiled
    result of the first and the two-layer result of the second: computed once, shared, never changed"""
    import spiht_amd
    g = dict(PIN, **change)
    P = synth_image(4100 + g["H"] + g["W"] + g["c"], g["c"], g["H"], g["W"])
    plain = spiht_amd.TiledCodec(g["c"], g["H"], g["W"], g["tile"], None, None, 27005, overlap=overlap)
    rd = spiht_amd.TiledCodec(g["c"], g["H"], g["W"], g["tile"], None, None, 40000, allocate="rd", overlap=overlap)
    return plain, rd, plain.encode(P), rd.encode_layered(P, 2)


@pytest.mark.parametrize("overlap", [0, 4])
def test_foreign_result_is_refused_by_every_host_decode(overlap):
    """a result of another geometry, one whose max_n misses a tile and one whose lengths do not describe its bytes: ValueError
    from every host decode, and the codec decodes a good result afterwards as it did before"""
    import dataclasses
    plain, rd, res, lay = pinned(overlap)
    calls = [(plain, res, lambda k, r: k.decode(r)),
             (plain, res, lambda k, r: k.decode_window_u8(r, 28, 30, 10, 8)),
             (rd, lay, lambda k, r: k.decode_layered(r)),
             (rd, lay, lambda k, r: k.decode_layered_window_u16(r, 28, 30, 10, 8, upto=1))]
    for n, (codec, good, call) in enumerate(calls):
        layered = good is lay
        before = call(codec, good)
        bad = [pinned(overlap, **change)[3 if layered else 2] for change in FOREIGN]
        bad.append(dataclasses.replace(good, max_n=good.max_n[:-1]))
        if layered:  # the layered result's own tables: its pieces do not add up to its bytes
            bad.append(dataclasses.replace(good, encoded_bytes=good.encoded_bytes[:-1]))
        else:
            bad.append(dataclasses.replace(good, nbytes=[good.nbytes[0] + 1] + good.nbytes[1:]))
            bad.append(dataclasses.replace(good, nbytes=good.nbytes[:-1]))
        for r in bad:
            with pytest.raises(ValueError):
                call(codec, r)
        after = call(codec, good)
        assert after.dtype == before.dtype and after.tobytes() == before.tobytes(), n


def device_streams(res):
    """the streams, lengths and start planes of a TiledResult on the device, as decode_device takes them"""
    return (dev(np.frombuffer(res.encoded_bytes, np.uint8)), len(res.encoded_bytes), dev(np.array(res.nbytes, np.uint32)),
            dev(np.array(res.max_n, np.uint8)))


@pytest.mark.parametrize("form", ["plain", "reduced", "overlap"])
def test_decode_device_refuses_an_output_it_does_not_write(form):
    """a float32 output, a float64 output with strides: ValueError from each of the three assemblers; the output keeps the
    pattern it was filled with and last_tiles_decoded its value"""
    from spiht_amd import _lib
    ctx = _lib.default_context()
    codec, _, res, _ = pinned(4 if form == "overlap" else 0)
    reduce = 1 if form == "reduced" else 0
    rs = codec.reduced_shape(reduce)
    shape = (1, rs["Hk"], rs["Wk"])
    assert shape == ((1, 35, 45) if reduce else (1, 70, 90))
    good = codec.decode(res, reduce=reduce)
    assert good.shape == shape
    streams = device_streams(res)
    codec.last_tiles_decoded = 77
    for dtype, strides in [(np.float32, None), (np.float64, (8 * shape[1] * shape[2], 8 * shape[2], 8))]:
        pattern = np.full(shape, -7.25, dtype)
        d_out = dev(pattern)
        with pytest.raises(ValueError):
            codec.decode_device(*streams, d_out, strides=strides, reduce=reduce)
        ctx.synchronize()
        assert np.array_equal(d_out.download(), pattern)
        assert codec.last_tiles_decoded == 77
    # ... and the good call still writes all of it
    d_out = dev(np.full(shape, -7.25))
    codec.decode_device(*streams, d_out, reduce=reduce)
    ctx.synchronize()
    assert np.array_equal(d_out.download(), good) and codec.last_tiles_decoded == codec.T


def test_encode_device_refuses_no_pictures_and_foreign_arrays():
    """N = 0; a float32 picture for a float64 codec; a float64 picture with strides: ValueError"""
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    ctx = _lib.default_context()
    plain, rd, res, lay = pinned(0)
    T = plain.T
    P = synth_image(4261, 1, 70, 90)
    d_packed = DeviceArray(ctx, (T * rd.codec.slot_stride,), np.uint8)
    d_lens, d_maxn = DeviceArray(ctx, (2 * T,), np.uint32), DeviceArray(ctx, (T,), np.uint8)
    d_pic = DeviceArray(ctx, (1,), np.uint64)
    d_img = dev(P[None])
    with pytest.raises(ValueError):
        plain.encode_device(d_img, 0, d_packed, d_lens, d_maxn)
    with pytest.raises(ValueError):
        rd.encode_device(d_img, 0, d_packed, d_lens, d_maxn)
    with pytest.raises(ValueError):
        rd.encode_layered_device(d_img, 0, 2, d_packed, d_lens, d_maxn, d_pic)
    for codec in (plain, rd):
        with pytest.raises(ValueError):
            codec.encode_device(dev(P[None].astype(np.float32)), 1, d_packed, d_lens, d_maxn)
        with pytest.raises(ValueError):
            codec.encode_device(d_img, 1, d_packed, d_lens, d_maxn, strides=(8 * 70 * 90, 8 * 70 * 90, 8 * 90, 8))
    ctx.synchronize()
    # the good call, after them
    plain.encode_device(d_img, 1, d_packed, d_lens, d_maxn)
    ctx.synchronize()
    assert d_lens.download()[:T].tolist() == plain.encode(P).nbytes


# what a reduce that is no int >= 0 meets, call by call: recorded from the code as it stood before the paths were folded
REDUCE_PINS = {  # (overlap, the argument's name) -> the exception, words of its message; None: it decodes as reduce=1
    (0, "True"): (TypeError, "integer"),
    (0, "1.0"): (TypeError, "integer"),
    (0, "int64(1)"): None,
    (0, "-1"): (ValueError, "reduce = -1"),
    (4, "True"): (TypeError, "integer"),
    (4, "1.0"): (TypeError, "integer"),
    (4, "int64(1)"): (ValueError, "overlap"),
    (4, "-1"): (ValueError, "reduce = -1"),
}
REDUCE_ARGS = {"True": True, "1.0": 1.0, "int64(1)": np.int64(1), "-1": -1}


@pytest.mark.parametrize("overlap,arg", list(REDUCE_PINS))
def test_reduce_that_is_no_plain_level(overlap, arg):
    plain, rd, res, lay = pinned(overlap)
    reduce, pin = REDUCE_ARGS[arg], REDUCE_PINS[overlap, arg]
    calls = [lambda r: plain.decode(res, reduce=r), lambda r: rd.decode_layered(lay, reduce=r)]
    if pin is None:
        assert plain.reduced_shape(reduce) == plain.reduced_shape(1) and rd.reduced_shape(reduce) == rd.reduced_shape(1)
        for call in calls:
            got, want = call(reduce), call(1)
            assert got.shape == (1, 35, 45) and got.dtype == want.dtype and got.tobytes() == want.tobytes()
        return
    for call in calls + [plain.reduced_shape, rd.reduced_shape]:
        with pytest.raises(pin[0], match=pin[1]):
            call(reduce)
