"""Tiled pictures at reduced resolution on the GPU: decode(result, reduce=k) is the numpy mosaic of the tiles' reduced decodes
(which are the oracle's, i.e. PyWavelets'), windows in the reduced picture's coordinates decode only the tiles they meet,
reduce=0 is the call without the argument, it composes with quality layers, and the mosaic kernel equals its numpy statement
through the C ABI.  Every comparison is equality of bits; float64 is compared as uint64."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_image
from tile_helpers import dev, settings, tile_of
from test_reduced_cpu import oracle_reduced

pytestmark = pytest.mark.gpu

vp = C.c_void_p
KINDS = {"f64": np.float64, "u8": np.uint8, "u16": np.uint16}

# the first number is the channel count; the geometries of the last column were checked on the CPU oracle
CASES = {
    "grid3x3": dict(c=3, H=70, W=90, tile=32, max_bits=27005),                     # L = 2; thk 32 / 16 / 8; offsets 0 / 1 / 1
    "deep": dict(c=1, H=70, W=90, tile=16, level=3, max_bits=40000),               # thk down to 2, offset 2
    "rect": dict(c=1, H=70, W=90, tile=(16, 40), level=3, max_bits=20000),         # twk = 5 at k = 3
    "bior44": dict(c=1, H=70, W=90, tile=32, level=3, max_bits=27005, wavelet="bior4.4", mode="symmetric"),
    "per": dict(c=1, H=64, W=96, tile=32, level=3, max_bits=None, wavelet="db2", mode="periodization"),  # offsets 0, no rim
    "ipt": dict(c=3, H=70, W=90, tile=32, max_bits=27005, color="IPT"),
    "single": dict(c=3, H=20, W=27, tile=32, max_bits=4001),                       # one padded tile
}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def case(name):
    """the picture, settings, codec and tiled result of a case: computed once, shared, never changed"""
    import spiht_amd
    cfg = CASES[name]
    c, H, W = cfg["c"], cfg["H"], cfg["W"]
    P = synth_image(5000 + H + W + c, c, H, W)
    P.setflags(write=False)
    s = settings(cfg)
    codec = spiht_amd.TiledCodec(c, H, W, cfg["tile"], s, cfg.get("level"), cfg["max_bits"])
    res = codec.encode(P)
    return cfg, P, s, codec, res


def allowed(name):
    """every k the contract allows for the case"""
    cfg, P, s, codec, res = case(name)
    th, tw = tile_of(cfg["tile"])
    L = codec.reduced_shape(0)["level"]
    return [k for k in range(L + 1) if th % 2 ** k == 0 and tw % 2 ** k == 0]


def tile_fn(kind):
    import spiht_amd
    return {"f64": spiht_amd.decode_image_reduced, "u8": spiht_amd.decode_image_reduced_u8,
            "u16": spiht_amd.decode_image_reduced_u16}[kind]


@functools.lru_cache(maxsize=None)
def reference(name, k, kind):
    """the contract: the numpy mosaic of the tiles' own reduced decodes (crop=True), cut to Hk x Wk"""
    cfg, P, s, codec, res = case(name)
    th, tw = tile_of(cfg["tile"])
    gy, gx = res.grid()
    thk, twk = th >> k, tw >> k
    Hk, Wk = -(-cfg["H"] // 2 ** k), -(-cfg["W"] // 2 ** k)
    want = np.zeros((cfg["c"], gy * thk, gx * twk), KINDS[kind])
    for i in range(gy):
        for j in range(gx):
            t = tile_fn(kind)(res.tile(i, j), s, k, crop=True)
            assert t.shape == (cfg["c"], thk, twk)
            want[:, i * thk:(i + 1) * thk, j * twk:(j + 1) * twk] = t
    want = np.ascontiguousarray(want[:, :Hk, :Wk])
    want.setflags(write=False)
    return want


def test_the_cases_have_the_geometry_they_are_named_for():
    assert allowed("grid3x3") == [0, 1, 2] and allowed("deep") == [0, 1, 2, 3] and allowed("rect") == [0, 1, 2, 3]
    codec = case("grid3x3")[3]
    assert [(codec.reduced_shape(k)["thk"], codec.reduced_shape(k)["off_y"]) for k in range(3)] == [(32, 0), (16, 1), (8, 1)]
    rs = case("deep")[3].reduced_shape(3)
    assert (rs["thk"], rs["twk"], rs["off_y"], rs["off_x"]) == (2, 2, 2, 2)
    assert case("rect")[3].reduced_shape(3)["twk"] == 5
    rs = case("per")[3].reduced_shape(3)
    assert (rs["off_y"], rs["off_x"], rs["rec_h"], rs["pic_w"]) == (0, 0, 4, 4)
    assert max(allowed("bior44")) == 3 and len(allowed("single")) >= 2 and len(allowed("ipt")) == 3


# ---- 1. per-tile parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_per_tile_parity(name):
    import spiht_amd
    cfg, P, s, codec, res = case(name)
    c = cfg["c"]
    for k in allowed(name):
        rs = spiht_amd.tiled_reduced_shape(cfg["H"], cfg["W"], cfg["tile"], s, cfg.get("level"), k)
        Hk, Wk = rs["Hk"], rs["Wk"]
        got = codec.decode(res, reduce=k)
        assert got.dtype == np.float64 and got.shape == (c, Hk, Wk)
        assert same_bits(got, reference(name, k, "f64")), (name, k)
        assert same_bits(spiht_amd.decode_image_tiled(res, s, reduce=k), got)
        for kind in ("u8", "u16"):
            want = reference(name, k, kind)
            got = getattr(codec, "decode_" + kind)(res, reduce=k)
            assert got.dtype == KINDS[kind] and same_bits(got, want), (name, k, kind)
            hwc = getattr(codec, "decode_" + kind)(res, channels_last=True, reduce=k)
            assert hwc.shape == (Hk, Wk, c) and same_bits(hwc, want.transpose(1, 2, 0)), (name, k, kind)
            assert same_bits(getattr(spiht_amd, "decode_image_tiled_" + kind)(res, s, reduce=k), want)


# ---- 2. the chain to PyWavelets ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid3x3", "per"])
def test_tiles_are_the_oracles(oracle, name):
    """the float64 tiles the mosaic is made of are the oracle's reduced inverse of the oracle's decode of the tile's stream"""
    cfg, P, s, codec, res = case(name)
    th, tw = tile_of(cfg["tile"])
    gy, gx = res.grid()
    g = oracle.geometry(th, tw, s.wavelet, res.level, s.mode)
    L = g["level"]
    for k in allowed(name):
        rs = codec.reduced_shape(k)
        thk, twk, oy, ox = rs["thk"], rs["twk"], rs["off_y"], rs["off_x"]
        got = codec.decode(res, reduce=k)
        for i in range(gy):
            for j in range(gx):
                t = res.tile(i, j)
                rec = oracle.decode(t.encoded_bytes, t.max_n, t.c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"])
                D = oracle.dequantize(rec, s.quantization_scale, s.per_channel_quant_scales)
                if k == L:
                    R = np.ascontiguousarray(D[:, :g["ll_h"], :g["ll_w"]]) * 2.0 ** -L
                else:
                    R = oracle_reduced(oracle, D, th, tw, s.wavelet, L, s.mode, k)
                assert R.shape[1:] == (rs["rec_h"], rs["rec_w"])
                own = R[:, oy:oy + thk, ox:ox + twk]
                part = got[:, i * thk:(i + 1) * thk, j * twk:(j + 1) * twk]
                assert same_bits(part, own[:, :part.shape[1], :part.shape[2]]), (name, k, i, j)


# ---- 3. reduce = 0 -------------------------------------------------------------------------------------------------------------
def test_reduce_0_is_the_call_without_it():
    import spiht_amd
    cfg, P, s, codec, res = case("grid3x3")
    win = (28, 30, 10, 8)
    for suffix in ("", "_u8", "_u16"):
        for obj, lead in ((codec, ()), (None, (s,))):
            whole = getattr(codec, "decode" + suffix) if obj else getattr(spiht_amd, "decode_image_tiled" + suffix)
            window = getattr(codec, "decode_window" + suffix) if obj else getattr(spiht_amd, "decode_image_window" + suffix)
            assert same_bits(whole(res, *lead, reduce=0), whole(res, *lead))
            assert same_bits(window(res, *lead, *win, reduce=0), window(res, *lead, *win))
            if suffix:
                assert same_bits(whole(res, *lead, channels_last=True, reduce=0), whole(res, *lead, channels_last=True))
    for bad in (1.0, "1", None):
        with pytest.raises(TypeError):
            codec.decode(res, reduce=bad)
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            codec.decode(res, reduce=bad)
    with pytest.raises(ValueError):  # 33 is odd
        spiht_amd.TiledCodec(1, 70, 90, (33, 40), s, 3, 20000).reduced_shape(1)


# ---- 4. windows ----------------------------------------------------------------------------------------------------------------
def window_sweep(Hk, Wk, thk, twk):
    ys = [(y0, min(h, Hk - y0)) for y0 in sorted({0, 1, thk - 1, thk, Hk - 1}) if 0 <= y0 < Hk for h in (1, 2, thk + 1, Hk)]
    xs = [(x0, min(w, Wk - x0)) for x0 in sorted({0, 1, twk - 1, twk, Wk - 1}) if 0 <= x0 < Wk for w in (1, 2, twk + 1, Wk)]
    return sorted(set(ys)), sorted(set(xs))


@pytest.mark.parametrize("name,k", [(n, k) for n in ("grid3x3", "deep") for k in range(4) if (n, k) != ("grid3x3", 3)])
def test_windows(name, k):
    import spiht_amd
    cfg, P, s, codec, res = case(name)
    rs = codec.reduced_shape(k)
    Hk, Wk, thk, twk = rs["Hk"], rs["Wk"], rs["thk"], rs["twk"]
    whole = {kind: reference(name, k, kind) for kind in KINDS}
    ys, xs = window_sweep(Hk, Wk, thk, twk)
    assert len(ys) >= 12 and len(xs) >= 12
    for a, (y0, h) in enumerate(ys):
        for b, (x0, w) in enumerate(xs):
            i0, i1, j0, j1 = spiht_amd.window_tiles(Hk, Wk, thk, twk, y0, x0, h, w)
            got = codec.decode_window(res, y0, x0, h, w, reduce=k)
            assert same_bits(got, whole["f64"][:, y0:y0 + h, x0:x0 + w]), (name, k, y0, x0, h, w)
            assert codec.last_tiles_decoded == (i1 - i0) * (j1 - j0)
            if a == b % len(ys):  # the integer forms on a diagonal of the sweep
                assert same_bits(codec.decode_window_u8(res, y0, x0, h, w, reduce=k), whole["u8"][:, y0:y0 + h, x0:x0 + w])
                assert same_bits(codec.decode_window_u16(res, y0, x0, h, w, channels_last=True, reduce=k),
                                 whole["u16"][:, y0:y0 + h, x0:x0 + w].transpose(1, 2, 0))
                assert codec.last_tiles_decoded == (i1 - i0) * (j1 - j0)
    (y0, h), (x0, w) = ys[len(ys) // 2], xs[len(xs) // 2]
    assert same_bits(spiht_amd.decode_image_window(res, s, y0, x0, h, w, reduce=k), whole["f64"][:, y0:y0 + h, x0:x0 + w])
    for bad in [(Hk - 1, 0, 2, 1), (0, Wk - 1, 1, 2), (-1, 0, 1, 1), (0, 0, 0, 1), (0, 0, Hk + 1, Wk), (Hk, 0, 1, 1)]:
        with pytest.raises(ValueError):
            codec.decode_window(res, *bad, reduce=k)
    if k:  # the full picture's last sample lies outside the reduced one
        with pytest.raises(ValueError):
            codec.decode_window(res, cfg["H"] - 1, cfg["W"] - 1, 1, 1, reduce=k)


def test_window_on_the_device_into_an_rgba_view():
    """decode_window_device with reduce: the streams of the sub-grid alone, an RGBA view that keeps its alpha"""
    import spiht_amd
    from spiht_amd import _lib
    cfg, P, s, codec, res = case("grid3x3")
    k, (y0, x0, h, w) = 2, (7, 6, 3, 5)
    rs = codec.reduced_shape(k)
    sub = spiht_amd.window_tiles(rs["Hk"], rs["Wk"], rs["thk"], rs["twk"], y0, x0, h, w)
    assert sub == (0, 2, 0, 2)
    ts = [i * codec.gx + j for i in range(sub[0], sub[1]) for j in range(sub[2], sub[3])]
    off = np.concatenate(([0], np.cumsum(res.nbytes)))
    run = b"".join(res.encoded_bytes[off[t]:off[t + 1]] for t in ts)
    d_win = dev(np.full((h, w, 4), 201, np.uint8))
    codec.decode_window_device(dev(np.frombuffer(run, np.uint8)), len(run), dev(np.array([res.nbytes[t] for t in ts], np.uint32)),
                               dev(np.array([res.max_n[t] for t in ts], np.uint8)), sub, (y0, x0, h, w), d_win,
                               strides=(1, w * 4, 4), reduce=k)
    _lib.default_context().synchronize()
    out = d_win.download()
    want = reference("grid3x3", k, "u8")[:, y0:y0 + h, x0:x0 + w]
    assert np.array_equal(out[..., :3], want.transpose(1, 2, 0)) and (out[..., 3] == 201).all()
    assert codec.last_tiles_decoded == 4


# ---- 5. the kernel alone, through the C ABI, against numpy -------------------------------------------------------------------
DTYPES = {1: np.uint8, 2: np.uint16, 8: np.float64}
SUFFIX = {1: "u8", 2: "u16", 8: "f64"}
SENTINEL = {1: 0xA5, 2: 0xA5A5, 8: -7.25}
GUARD = 32
#          tw  th  oy  ox  extra rows / columns of the tile array
SHAPES = [(1, 3, 1, 2, 1, 0), (2, 2, 2, 3, 0, 2), (3, 4, 3, 0, 2, 1), (5, 5, 0, 1, 1, 3), (8, 8, 1, 3, 0, 0),
          (16, 9, 2, 2, 3, 1), (33, 8, 3, 1, 1, 2), (8, 8, 0, 0, 0, 0), (16, 9, 0, 0, 1, 1), (33, 8, 0, 0, 0, 1)]


def rand_array(rng, shape, es):
    if es <= 2:
        return rng.integers(0, np.iinfo(DTYPES[es]).max + 1, shape).astype(DTYPES[es])
    return rng.standard_normal(shape)


def numpy_mosaic(tiles, th, tw, oy, ox, i0, j0, nj, y0, x0, wh, ww):
    """[c, wh, ww] at (y0, x0): every sample from the tile that owns it, at that tile's origin; tiles [n, c, rh, rw]"""
    Y, X = y0 + np.arange(wh), x0 + np.arange(ww)
    i, j = Y // th, X // tw
    t = ((i - i0) * nj)[:, None] + (j - j0)[None, :]
    got = tiles[t, :, (oy + Y - i * th)[:, None], (ox + X - j * tw)[None, :]]  # [wh, ww, c]
    return np.ascontiguousarray(got.transpose(2, 0, 1))


def mosaic_call(es, ctx, d_tiles, c, rh, rw, oy, ox, H, W, th, tw, sub, win, out_ptr, strides):
    from spiht_amd import _lib
    fn = getattr(_lib.lib(), "spiht_tile_mosaic_" + SUFFIX[es])
    args = [ctx.handle, vp(d_tiles), c, rh, rw, oy, ox, H, W, th, tw, *sub, *win, vp(out_ptr)]
    if es <= 2:
        st = None if strides is None else np.array(strides, np.int64)
        args.append(None if st is None else vp(st.ctypes.data))
    return fn(*args)


@pytest.mark.parametrize("es", [1, 2, 8])
def test_mosaic_kernel(es):
    """tile widths 1 .. 33 (a 16-byte vector spans up to sixteen tiles), origins 0 .. 3 inside tile arrays larger than needed,
    a sub-grid smaller than the grid, x0 off alignment, the output 0 .. 15 elements into a guarded buffer, HWC and RGBA views;
    with a zero origin and sides >= 8 the output is spiht_tile_paste_*'s"""
    from spiht_amd import _lib
    ctx = _lib.default_context()
    rng = np.random.default_rng(20 + es)
    dt, c = DTYPES[es], 3
    for (tw, th, oy, ox, eh, ew) in SHAPES:
        gy, gx = 4, max(4, -(-75 // tw))
        H, W = gy * th - (th > 1), gx * tw - (tw > 2)           # the last tile row / column is short where it can be
        rh, rw = oy + th + eh, ox + tw + ew
        for sub in [(0, gy, 0, gx), (1, gy, 1, gx - 1)]:
            i0, i1, j0, j1 = sub
            n, nj = (i1 - i0) * (j1 - j0), j1 - j0
            tiles = rand_array(rng, (n, c, rh, rw), es)
            d_tiles = dev(tiles)
            Ya, Yb, Xa, Xb = i0 * th, min(i1 * th, H), j0 * tw, min(j1 * tw, W)
            wins = [(Ya, Xa, Yb - Ya, Xb - Xa), (Ya + (th > 1), Xa + 1, Yb - Ya - (th > 1), Xb - Xa - 2), (Yb - 1, Xa + 3, 1, 1),
                    (Ya, Xa + 5, 2, min(37, Xb - Xa - 5))]
            for wi, win in enumerate(wins):
                y0, x0, wh, ww = win
                want = numpy_mosaic(tiles, th, tw, oy, ox, i0, j0, nj, y0, x0, wh, ww)
                layouts = [("chw", (c, wh, ww), None, lambda a: a, range(16) if wi < 2 else (0, 7))]
                if es <= 2:
                    layouts.append(("hwc", (wh, ww, c), (es, ww * c * es, c * es), lambda a: a.transpose(2, 0, 1), (0, 1)))
                    layouts.append(("rgba", (wh, ww, 4), (es, ww * 4 * es, 4 * es), lambda a: a[..., :3].transpose(2, 0, 1), (0, 1)))
                for name, shape, strides, view, shifts in layouts:
                    size = int(np.prod(shape))
                    guard = np.full(size + 2 * GUARD, SENTINEL[es], dt)
                    for shift in shifts:
                        d_out = dev(guard)
                        lead = GUARD - 16 + shift  # 0 .. 15 elements off a 16-byte boundary of the buffer
                        _lib.check(mosaic_call(es, ctx, d_tiles.ptr, c, rh, rw, oy, ox, H, W, th, tw, sub, win,
                                               d_out.ptr + lead * es, strides))
                        ctx.synchronize()
                        got = d_out.download()
                        body = got[lead:lead + size].reshape(shape)
                        assert same_bits(view(body), want), (tw, th, sub, win, name, shift)
                        if name == "rgba":
                            assert (body[..., 3] == guard[0]).all()
                        assert (got[:lead] == guard[0]).all() and (got[lead + size:] == guard[0]).all(), (tw, win, name, shift)
                        d_out.free()
                if oy == 0 and ox == 0 and wi < 2:  # the paste, given the same tiles
                    paste = getattr(_lib.lib(), "spiht_tile_paste_" + SUFFIX[es])
                    d_out = dev(np.zeros((c, wh, ww), dt))
                    _lib.check(paste(ctx.handle, vp(d_tiles.ptr), c, rh, rw, H, W, th, tw, *sub, *win, vp(d_out.ptr),
                                     *([None] if es <= 2 else [])))
                    ctx.synchronize()
                    assert same_bits(d_out.download(), want), (tw, th, sub, win)
                    d_out.free()
            d_tiles.free()


@pytest.mark.parametrize("es", [1, 2, 8])
def test_mosaic_argument_errors(es):
    """refused with SPIHT_ERR_ARG before anything is queued: nothing is written"""
    from spiht_amd import _lib
    ctx = _lib.default_context()
    dt = DTYPES[es]
    c, th, tw, oy, ox, rh, rw, H, W = 1, 4, 5, 1, 2, 6, 8, 11, 14   # a 3 x 3 grid
    d_tiles = dev(np.zeros((9, c, rh, rw), dt))
    out = np.full((c, H, W), SENTINEL[es], dt)
    d_out = dev(out)
    good = dict(c=c, rh=rh, rw=rw, oy=oy, ox=ox, H=H, W=W, th=th, tw=tw, sub=(0, 3, 0, 3), win=(0, 0, H, W))

    def call(**kw):
        a = dict(good, **kw)
        return mosaic_call(es, ctx, d_tiles.ptr, a["c"], a["rh"], a["rw"], a["oy"], a["ox"], a["H"], a["W"], a["th"], a["tw"],
                           a["sub"], a["win"], d_out.ptr, None)

    bad = [dict(oy=-1), dict(ox=-1), dict(rh=oy + th - 1), dict(rw=ox + tw - 1), dict(th=0), dict(tw=0), dict(c=0), dict(H=0),
           dict(win=(0, 0, H + 1, W)), dict(win=(0, 0, H, W + 1)), dict(win=(-1, 0, 2, 2)), dict(win=(0, 0, 0, 1)),
           dict(sub=(0, 2, 0, 3)), dict(sub=(0, 3, 1, 3)), dict(sub=(0, 4, 0, 3)), dict(sub=(1, 1, 0, 3))]
    for kw in bad:
        assert call(**kw) == _lib.ERR_ARG, kw
    if es > 1:  # an output that is not aligned to its element
        assert mosaic_call(es, ctx, d_tiles.ptr, c, rh, rw, oy, ox, H, W, th, tw, (0, 3, 0, 3), (0, 0, H, W), d_out.ptr + 1,
                           None) == _lib.ERR_ARG
    if es <= 2:  # a view that overlaps itself
        fn = getattr(_lib.lib(), "spiht_tile_mosaic_" + SUFFIX[es])
        st = np.array([0, W * es, es], np.int64)
        assert fn(ctx.handle, vp(d_tiles.ptr), 2, rh, rw, oy, ox, H, W, th, tw, 0, 3, 0, 3, 0, 0, H, W, vp(d_out.ptr),
                  vp(st.ctypes.data)) == _lib.ERR_ARG
    ctx.synchronize()
    assert same_bits(d_out.download(), out)
    assert call() == _lib.OK
    ctx.synchronize()
    assert same_bits(d_out.download(), np.zeros((c, H, W), dt))


# ---- 6. quality layers ---------------------------------------------------------------------------------------------------------
def test_layers():
    import spiht_amd
    cfg, P, s, _, _ = case("grid3x3")
    codec = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, cfg["max_bits"], allocate="rd", points=8)
    res = codec.encode_layered(P, 3)
    assert res.layers == 3
    for q in (1, 2, 3):
        plain = res.tiled(q)
        for k in (0, 1, 2):
            want = codec.decode(plain, reduce=k)
            assert same_bits(codec.decode_layered(res, upto=q, reduce=k), want), (q, k)
            assert same_bits(codec.decode_layered_u8(res, upto=q, channels_last=True, reduce=k),
                             codec.decode_u8(plain, channels_last=True, reduce=k))
        y0, x0, h, w = 15, 14, 4, 4  # a four-tile corner of the 16 x 16 grid
        got = codec.decode_layered_window(res, y0, x0, h, w, upto=q, reduce=1)
        assert codec.last_tiles_decoded == 4
        assert same_bits(got, codec.decode(plain, reduce=1)[:, y0:y0 + h, x0:x0 + w])
        assert same_bits(spiht_amd.decode_image_layered_window_u16(res, s, y0, x0, h, w, q, reduce=1),
                         codec.decode_u16(plain, reduce=1)[:, y0:y0 + h, x0:x0 + w])
        assert same_bits(spiht_amd.decode_image_layered(res, s, q, reduce=2), codec.decode(plain, reduce=2))
    # reduce = 0 is the call without it
    assert same_bits(codec.decode_layered(res, 2, reduce=0), codec.decode_layered(res, 2))
    assert same_bits(codec.decode_layered_u16(res, reduce=0), codec.decode_layered_u16(res))
    assert same_bits(codec.decode_layered_window_u8(res, 28, 30, 10, 8, 2, reduce=0), codec.decode_layered_window_u8(res, 28, 30, 10, 8, 2))
    with pytest.raises(ValueError):
        codec.decode_layered(res, reduce=3)
    codec.close()


# ---- 7. calls in sequence ------------------------------------------------------------------------------------------------------
def test_sequence_on_one_codec():
    """reduce 2, full, reduce 1, a window, on one codec: each equals the same call on a fresh codec (and the contract's
    mosaic) -- a reduced inverse reads a corner of the context's coefficient array and has to leave all of it clean"""
    import spiht_amd
    cfg, P, s, _, res = case("grid3x3")
    calls = [lambda cd: cd.decode(res, reduce=2), lambda cd: cd.decode(res), lambda cd: cd.decode_u8(res, reduce=1),
             lambda cd: cd.decode_window(res, 3, 5, 20, 30, reduce=1), lambda cd: cd.decode_window(res, 3, 5, 20, 30)]
    one = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, cfg["max_bits"])
    got = [f(one) for f in calls]
    one.close()
    for f, g in zip(calls, got):
        fresh = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, cfg["max_bits"])
        assert same_bits(f(fresh), g)
        fresh.close()
    assert same_bits(got[0], reference("grid3x3", 2, "f64")) and same_bits(got[1], reference("grid3x3", 0, "f64"))
    assert same_bits(got[2], reference("grid3x3", 1, "u8"))
    assert same_bits(got[3], reference("grid3x3", 1, "f64")[:, 3:23, 5:35])
    assert same_bits(got[4], reference("grid3x3", 0, "f64")[:, 3:23, 5:35])


# ---- 8. the command-line tool ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [None, "3,5,20,30"])
def test_command_line(tmp_path, capsys, window):
    """--tile 32 --reduce 1 [--window ...]: the file holds the reduced 8-bit picture; no distance is printed"""
    import spiht_amd
    from spiht_amd import encode_decode as tool
    from spiht_amd.utils import imload, imsave
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "small.png")
    imsave(src, synth_image(21, 3, 70, 90))
    argv = [src, "--bpp", "1.0", "--tile", "32", "--reduce", "1", "--out", dst] + (["--window", window] if window else [])
    args = tool.build_parser().parse_args(argv)
    enc, small = tool.main(args)
    p = tool.plan(args, 3, 70, 90)
    want = spiht_amd.decode_image_tiled_u8(enc, p.settings, reduce=1)
    assert want.shape == (3, 35, 45)
    if window:
        want = want[:, 3:23, 5:35]
    assert small.dtype == np.uint8 and same_bits(small, want)
    assert same_bits(np.round(imload(dst) * 255).astype(np.uint8), want)
    text = capsys.readouterr().out
    assert "1/2 size" in text and "mean squared error" not in text
