"""Overlapping tiles on the GPU: the cut with a margin equals np.pad(mode="edge") and slicing, the blend kernel equals the rule
of spiht_amd/overlap.py bit for bit (NaN for NaN), and through the library every tile stream is encode_image of the coded tile's
pixels and every decode the rule's blend of the tiles' single-image decodes."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_image
from tile_helpers import dev, tile_of

pytestmark = pytest.mark.gpu

vp = C.c_void_p
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.float32, 8: np.float64}
SENTINEL = {1: 0xA5, 2: 0xA5A5, 4: -77.5, 8: -77.5}


def rand_array(rng, shape, es):
    if es <= 2:
        return rng.integers(0, 256 ** es, shape).astype(DTYPES[es])
    return rng.standard_normal(shape).astype(DTYPES[es])


def same_bits(got, want):
    """float64 arrays equal in every bit, a NaN for a NaN (a NaN's sign and payload are the hardware's)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


# ---- the cut -----------------------------------------------------------------------------------------------------------------
CUT_SHAPES = [(2, 3, 70, 90, 32, 32, 1), (2, 3, 70, 90, 32, 32, 5), (2, 3, 70, 90, 32, 32, 16), (2, 1, 9, 8, 8, 8, 4),
              (1, 3, 20, 20, 32, 32, 3), (2, 1, 70, 90, 32, 32, 0)]


def cut_fn(es, overlap=True):
    from spiht_amd import _lib
    return getattr(_lib.lib(), "spiht_tile_cut_%s%s" % ("overlap_" if overlap else "", {1: "u8", 2: "u16", 4: "f32", 8: "f64"}[es]))


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_cut_overlap_kernel(es):
    """cut == np.pad(mode="edge") on four sides + slicing, for every element size; both arrays also one element off a 16-byte
    boundary, sentinels around the output; the integer forms through HWC and RGBA views; m = 0 gives the bytes of the plain cut"""
    from spiht_amd import _lib, overlap
    ctx = _lib.default_context()
    rng = np.random.default_rng(40 + es)
    for (N, c, H, W, th, tw, m) in CUT_SHAPES:
        P = rand_array(rng, (N, c, H, W), es)
        want = np.concatenate([overlap.cut(P[n], th, tw, m) for n in range(N)])
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
                guard = np.full(want.size + 32, SENTINEL[es], dtype=P.dtype)
                head = [ctx.handle, vp(d_in.ptr + shift * es)]
                if es <= 2:
                    st = None if strides is None else np.array(strides, np.int64)
                    head.append(None if st is None else vp(st.ctypes.data))
                outs = []
                for plain in ([False, True] if m == 0 else [False]):
                    d_out = dev(guard)
                    tail = [N, c, H, W, th, tw] + ([] if plain else [m]) + [vp(d_out.ptr + (16 - shift) * es)]
                    _lib.check(cut_fn(es, not plain)(*head, *tail))
                    ctx.synchronize()
                    outs.append(d_out.download())
                got = outs[0]
                body = got[16 - shift:16 - shift + want.size].reshape(want.shape)
                assert np.array_equal(body.view(np.uint8), want.view(np.uint8)), (name, shift, (N, c, H, W, th, tw, m))
                assert (got[:16 - shift] == guard[0]).all() and (got[16 - shift + want.size:] == guard[0]).all()
                if m == 0:
                    assert outs[0].tobytes() == outs[1].tobytes()
    # a margin that is negative or longer than half a tile side: refused
    d_in, d_out = dev(np.zeros((1, 1, 20, 20), DTYPES[es])), dev(np.zeros((1, 1, 64, 64), DTYPES[es]))
    mid = [None] if es <= 2 else []
    for m in (-1, 17):
        assert cut_fn(es)(ctx.handle, vp(d_in.ptr), *mid, 1, 1, 20, 20, 32, 32, m, vp(d_out.ptr)) == _lib.ERR_ARG


# ---- the blend alone ---------------------------------------------------------------------------------------------------------
BLEND_GEOMS = {  # c, H, W, th, tw, m, rh, rw
    "touch": (2, 20, 27, 8, 8, 4, 16, 17),        # 2m = th: the zones touch
    "thin": (1, 70, 90, 32, 32, 1, 34, 35),       # a zone of two samples
    "inexact": (3, 40, 56, 16, 24, 3, 22, 30),    # 4m = 12: the division is not a multiplication
    "single": (1, 20, 20, 32, 32, 5, 42, 43),     # a 1 x 1 grid: the crop of the margin
    "cutzone": (1, 17, 27, 8, 8, 3, 14, 14),      # H = gy th - th + 1: the last zone is cut by the picture's end
}


def blend_windows(H, W, th, tw, m):
    """(window, sub-grid or None for the one the window needs)"""
    wins = [((0, 0, H, W), None)]
    if H > th and W > tw:
        wins += [((y, x, 1, 1), None) for y in (th - 1, th) for x in (tw - 1, tw)]    # around a four-tile corner
        wins.append(((th - 1, tw - 1, min(th + 1, H - th + 1), min(tw + 1, W - tw + 1)), None))  # from a zone into a zone
        wins.append(((1, 3, H - 2, (W - 3) if (W - 3) % 2 else W - 4), None))         # odd x0, odd width
        wins.append(((0, 0, 3, 3), (0, -(-H // th), 0, -(-W // tw))))                  # a sub-grid larger than needed
        wins.append(((th, tw + 1, 1, 2), (0, 2, 0, 2)))
    else:
        wins += [((3, 5, 9, 11), None), ((19, 19, 1, 1), None)]
    return wins


@pytest.mark.parametrize("geom", sorted(BLEND_GEOMS))
def test_blend_kernel(geom):
    """spiht_tile_blend_* == overlap.blend bit for bit on tiles with negatives, values above 1, 1e300 and NaN: float64, and
    8 / 16 bits dense, HWC and (three channels) as an RGBA view that keeps its fourth byte; sentinels around every output"""
    from spiht_amd import _lib, overlap
    L, ctx = _lib.lib(), _lib.default_context()
    c, H, W, th, tw, m, rh, rw = BLEND_GEOMS[geom]
    gy, gx = -(-H // th), -(-W // tw)
    rng = np.random.default_rng(len(geom))
    tiles = rng.standard_normal((gy * gx, c, rh, rw)) * 0.6 + 0.5
    flat = tiles.reshape(-1)
    idx = rng.choice(flat.size, 60, replace=False)
    flat[idx[:20]], flat[idx[20:40]], flat[idx[40:]] = np.nan, 1e300, -1e300
    tiles[0, 0, th + m - 1, min(tw + m, rw - 1)] = np.nan   # (in the margin, at a corner's zone)
    grid = tiles.reshape(gy, gx, c, rh, rw)
    for (y0, x0, wh, ww), sub in blend_windows(H, W, th, tw, m):
        if sub is None:
            sub = overlap.window_tiles_overlap(H, W, th, tw, m, y0, x0, wh, ww)
        i0, i1, j0, j1 = sub
        part = np.ascontiguousarray(grid[i0:i1, j0:j1]).reshape(-1, c, rh, rw)
        d_tiles = dev(part)
        for es in (8, 1, 2):
            dt = DTYPES[es]
            want = overlap.blend(part, H, W, th, tw, m, window=(y0, x0, wh, ww), sub=sub, dtype=dt)
            layouts = [("chw", (c, wh, ww), None, lambda a: a)]
            if es <= 2:
                layouts.append(("hwc", (wh, ww, c), (es, ww * c * es, c * es), lambda a: a.transpose(2, 0, 1)))
                if c == 3:
                    layouts.append(("rgba", (wh, ww, 4), (es, ww * 4 * es, 4 * es), lambda a: a[..., :3].transpose(2, 0, 1)))
            for name, shape, strides, view in layouts:
                for shift in (0, 1):
                    size = int(np.prod(shape))
                    guard = np.full(size + 32, 201 if es == 1 else SENTINEL[es], dt)
                    d_out = dev(guard)
                    args = [ctx.handle, vp(d_tiles.ptr), c, rh, rw, H, W, th, tw, m, i0, i1, j0, j1, y0, x0, wh, ww,
                            vp(d_out.ptr + (16 - shift) * es)]
                    if es <= 2:
                        st = None if strides is None else np.array(strides, np.int64)
                        args.append(None if st is None else vp(st.ctypes.data))
                    _lib.check(getattr(L, "spiht_tile_blend_" + {8: "f64", 1: "u8", 2: "u16"}[es])(*args))
                    ctx.synchronize()
                    got = d_out.download()
                    body = got[16 - shift:16 - shift + size].reshape(shape)
                    where = (geom, (y0, x0, wh, ww), sub, es, name, shift)
                    assert same_bits(view(body), want) if es == 8 else np.array_equal(view(body), want), where
                    if name == "rgba":
                        assert (body[..., 3] == guard[0]).all(), where
                    assert (got[:16 - shift] == guard[0]).all() and (got[16 - shift + size:] == guard[0]).all(), where


def test_blend_kernel_refuses_bad_arguments():
    """argument errors are returned, and nothing is written"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    d_tiles = dev(np.zeros((9, 1, 40, 40)))
    for es, fn in ((8, L.spiht_tile_blend_f64), (1, L.spiht_tile_blend_u8), (2, L.spiht_tile_blend_u16)):
        guard = np.full(70 * 90, SENTINEL[es], DTYPES[es])
        d_out = dev(guard)
        tail = [None] if es <= 2 else []
        bad = [  # c, rh, rw, H, W, th, tw, m, sub-grid, window
            (1, 40, 40, 70, 90, 32, 32, -1, (0, 3, 0, 3), (0, 0, 70, 90)),   # m < 0
            (1, 80, 80, 70, 90, 32, 32, 17, (0, 3, 0, 3), (0, 0, 70, 90)),   # 2m > a tile side
            (1, 80, 80, 70, 90, 32, 40, 17, (0, 3, 0, 3), (0, 0, 70, 90)),
            (1, 40, 40, 70, 90, 32, 32, 4, (0, 3, 0, 3), (60, 0, 11, 5)),    # a window outside the picture
            (1, 40, 40, 70, 90, 32, 32, 4, (0, 3, 0, 3), (0, 0, 0, 5)),
            (1, 40, 40, 70, 90, 32, 32, 4, (0, 1, 0, 1), (30, 30, 1, 1)),    # a sub-grid that misses a contributing tile
            (1, 40, 40, 70, 90, 32, 32, 4, (0, 2, 0, 1), (30, 30, 1, 1)),
            (1, 40, 40, 70, 90, 32, 32, 4, (1, 2, 1, 2), (35, 32, 1, 4)),
            (1, 40, 40, 70, 90, 32, 32, 4, (0, 4, 0, 3), (0, 0, 5, 5)),      # a sub-grid outside the grid
            (1, 39, 40, 70, 90, 32, 32, 4, (0, 3, 0, 3), (0, 0, 70, 90)),    # tiles shorter than the coded tile
        ]
        for (c, rh, rw, H, W, th, tw, m, sub, win) in bad:
            assert fn(ctx.handle, vp(d_tiles.ptr), c, rh, rw, H, W, th, tw, m, *sub, *win, vp(d_out.ptr), *tail) == _lib.ERR_ARG, \
                (es, m, sub, win)
        # the same window with the tiles it needs is taken
        assert fn(ctx.handle, vp(d_tiles.ptr), 1, 40, 40, 70, 90, 32, 32, 4, 0, 2, 0, 2, 30, 30, 1, 1, vp(d_out.ptr), *tail) == _lib.OK
        ctx.synchronize()
        got = d_out.download()
        assert (got[1:] == guard[0]).all() and got[0] == 0


# ---- end to end --------------------------------------------------------------------------------------------------------------
CASES = {
    "rgb": dict(c=3, H=70, W=90, tile=32, m=4, max_bits=40000),
    "grey": dict(c=1, H=40, W=56, tile=(16, 24), m=3, max_bits=12000),
    "ipt": dict(c=3, H=70, W=90, tile=32, m=4, max_bits=40000, color="IPT"),
}


def settings(cfg):
    import spiht_amd
    return spiht_amd.SpihtSettings(color_model=cfg.get("color"))


def rule_decode(result, s, window=None, dtype=np.float64):
    """the rule on the single-image decodes of every tile of a result"""
    import spiht_amd
    from spiht_amd import overlap
    gy, gx = result.grid()
    dec = np.stack([np.asarray(spiht_amd.decode_image(result.tile(i, j), s)) for i in range(gy) for j in range(gx)])
    return overlap.blend(dec, result.h, result.w, result.th, result.tw, result.overlap, window=window, dtype=dtype)


@functools.lru_cache(maxsize=None)
def case(name):
    """the picture, codec, result, its decode and the rule's decode of a case: computed once, shared, never changed"""
    import spiht_amd
    cfg = CASES[name]
    s = settings(cfg)
    P = synth_image(70 + len(name), cfg["c"], cfg["H"], cfg["W"])
    codec = spiht_amd.TiledCodec(cfg["c"], cfg["H"], cfg["W"], cfg["tile"], s, None, cfg["max_bits"], overlap=cfg["m"])
    result = codec.encode(P)
    return cfg, s, P, codec, result, codec.decode(result), rule_decode(result, s)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tile_streams_and_decode(name):
    """every tile's stream is encode_image of the edge-padded picture's slice; decode is the rule's blend of decode_image of
    every tile, bit for bit, and the 8- / 16-bit forms its conversion"""
    import spiht_amd
    from spiht_amd import overlap
    cfg, s, P, codec, result, dec, want = case(name)
    th, tw = tile_of(cfg["tile"])
    m = cfg["m"]
    gy, gx = result.grid()
    assert result.overlap == m and (result.th, result.tw) == (th, tw)
    coded = overlap.cut(P, th, tw, m)
    for i in range(gy):
        for j in range(gx):
            ref = spiht_amd.encode_image(np.ascontiguousarray(coded[i * gx + j]), s, None, cfg["max_bits"] // (gy * gx))
            got = result.tile(i, j)
            assert (got.h, got.w) == (th + 2 * m, tw + 2 * m)
            assert (got.encoded_bytes, got.h, got.w, got.c, got.max_n, got.level) == \
                (ref.encoded_bytes, ref.h, ref.w, ref.c, ref.max_n, ref.level), (i, j)
    assert dec.shape == P.shape and same_bits(dec, want)
    assert np.array_equal(codec.decode_u8(result), rule_decode(result, s, dtype=np.uint8))
    assert np.array_equal(codec.decode_u16(result, channels_last=True), rule_decode(result, s, dtype=np.uint16).transpose(1, 2, 0))
    # the container: the round trip decodes identically, through the calls that build their codec from the result
    back = spiht_amd.TiledResult.from_bytes(result.to_bytes())
    assert back == result and result.to_bytes()[:4] == b"SPOL"
    assert same_bits(spiht_amd.decode_image_tiled(back, s), dec)


def test_windows_decode_the_tiles_with_weight():
    import spiht_amd
    from spiht_amd import overlap
    cfg, s, P, codec, result, dec, want = case("rgb")
    for win in [(30, 30, 1, 1), (28, 27, 10, 9), (0, 0, 28, 28), (36, 36, 20, 20), (33, 1, 37, 89), (0, 0, 70, 90)]:
        y0, x0, h, w = win
        got = codec.decode_window(result, *win)
        assert same_bits(got, dec[:, y0:y0 + h, x0:x0 + w]), win
        i0, i1, j0, j1 = overlap.window_tiles_overlap(70, 90, 32, 32, 4, *win)
        assert codec.last_tiles_decoded == (i1 - i0) * (j1 - j0), win
    # one sample beside a four-tile corner: 2 x 2 tiles where the tiles it meets are one
    codec.decode_window(result, 30, 30, 1, 1)
    assert codec.last_tiles_decoded == 4 and spiht_amd.window_tiles(70, 90, 32, 32, 30, 30, 1, 1) == (0, 1, 0, 1)
    assert np.array_equal(codec.decode_window_u8(result, 28, 27, 10, 9, channels_last=True),
                          rule_decode(result, s, dtype=np.uint8)[:, 28:38, 27:36].transpose(1, 2, 0))
    assert np.array_equal(spiht_amd.decode_image_window_u16(result, s, 28, 27, 10, 9),
                          rule_decode(result, s, dtype=np.uint16)[:, 28:38, 27:36])
    cfg, s, P, codec, result, dec, want = case("grey")
    assert same_bits(codec.decode_window(result, 13, 21, 6, 7), dec[:, 13:19, 21:28]) and codec.last_tiles_decoded == 4
    with pytest.raises(ValueError):
        codec.decode_window(result, 30, 0, 11, 5)


def test_float32_codec():
    import spiht_amd
    from spiht_amd import overlap
    s = spiht_amd.SpihtSettings()
    P = synth_image(77, 1, 40, 56).astype(np.float32)
    result = spiht_amd.encode_image_tiled(P, (16, 24), s, None, 12000, overlap=3)
    coded = overlap.cut(P, 16, 24, 3)
    assert coded.dtype == np.float32 and result.overlap == 3
    for t in range(9):
        ref = spiht_amd.encode_image(np.ascontiguousarray(coded[t]), s, None, 12000 // 9)
        got = result.tile(t // 3, t % 3)
        assert (got.encoded_bytes, got.max_n, got.h, got.w) == (ref.encoded_bytes, ref.max_n, 22, 30), t
    assert same_bits(spiht_amd.decode_image_tiled(result, s), rule_decode(result, s))


@functools.lru_cache(maxsize=None)
def rd_case():
    import spiht_amd
    cfg, s, P, _, _, _, _ = case("rgb")
    codec = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, 40000, allocate="rd", overlap=4)
    return s, P, codec, codec.encode(P)


def test_allocate_rd_with_overlap():
    """the budget is shared by the error of the coded tiles: the lengths add up to max_bits // 8, every tile is a prefix of its
    full encode_image stream, and the decode is the rule on those prefixes"""
    import spiht_amd
    from spiht_amd import overlap
    s, P, codec, result = rd_case()
    assert result.overlap == 4 and sum(result.nbytes) == 40000 // 8 and len(set(result.nbytes)) > 1
    coded = overlap.cut(P, 32, 32, 4)
    for t in range(9):
        full = spiht_amd.encode_image(np.ascontiguousarray(coded[t]), s, None, None)
        got = result.tile(t // 3, t % 3)
        assert got.max_n == full.max_n and full.encoded_bytes[:len(got.encoded_bytes)] == got.encoded_bytes, t
    assert same_bits(codec.decode(result), rule_decode(result, s))
    assert np.array_equal(codec.decode_u8(result), rule_decode(result, s, dtype=np.uint8))


def test_layers_with_overlap():
    import spiht_amd
    s, P, codec, result = rd_case()
    layered = codec.encode_layered(P, [10000, 24000, 40000])
    assert layered.overlap == 4 and layered.layers == 3 and layered.to_bytes()[:4] == b"SPOQ"
    for q in (1, 2, 3):
        assert same_bits(codec.decode_layered(layered, upto=q), codec.decode(layered.tiled(q))), q
        assert sum(layered.tiled(q).nbytes) == [10000, 24000, 40000][q - 1] // 8
    # all layers: encode's picture
    assert layered.tiled() == result and same_bits(codec.decode_layered(layered), codec.decode(result))
    second = codec.decode(layered.tiled(2))
    assert same_bits(codec.decode_layered_window(layered, 28, 27, 10, 9, upto=2), second[:, 28:38, 27:36])
    assert codec.last_tiles_decoded == 4
    assert np.array_equal(codec.decode_layered_u8(layered, upto=2), rule_decode(layered.tiled(2), s, dtype=np.uint8))
    # a prefix of the file, cut where the first layer ends, is the picture of the first layer
    data = layered.to_bytes()
    part = spiht_amd.LayeredResult.from_bytes(data[:layered.layer_ends()[0]])
    assert part.overlap == 4
    assert same_bits(spiht_amd.decode_image_layered(part, s), codec.decode_layered(layered, upto=1))
    top = spiht_amd.encode_image_layered(P, 32, s, None, 40000, [10000, 24000, 40000], overlap=4)
    assert top == layered


def test_overlap_zero_is_the_codec_without_it():
    import spiht_amd
    cfg, s, P, _, _, _, _ = case("rgb")
    a = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, 40000)
    b = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, 40000, overlap=0)
    ra, rb = a.encode(P), b.encode(P)
    assert ra == rb and ra.to_bytes() == rb.to_bytes() and rb.to_bytes()[:4] == b"SPTL"
    assert a.decode(ra).tobytes() == b.decode(rb).tobytes()
    assert a.decode_window_u8(ra, 28, 27, 10, 9).tobytes() == b.decode_window_u8(rb, 28, 27, 10, 9).tobytes()
    assert spiht_amd.encode_image_tiled(P, 32, s, None, 40000, overlap=0) == ra


def test_out_of_scope_with_overlap():
    import spiht_amd
    s, P, codec, result = rd_case()
    roi = np.ones((70, 90), np.uint8)
    for call in (lambda: codec.encode(P, roi=roi), lambda: codec.encode(P, target_psnr=30.0),
                 lambda: codec.encode_u8((P * 255).astype(np.uint8), roi=roi),
                 lambda: codec.encode_layered(P, 2, roi=roi), lambda: codec.encode_layered(P, target_psnr=[30.0, 35.0]),
                 lambda: codec.tile_curves(P, roi=roi), lambda: codec.decode(result, reduce=1),
                 lambda: codec.decode_window_u8(result, 0, 0, 8, 8, reduce=1),
                 lambda: spiht_amd.encode_image_tiled(P, 32, s, None, 40000, "rd", roi=roi, overlap=4),
                 lambda: spiht_amd.decode_image_tiled(result, s, reduce=1)):
        with pytest.raises(ValueError, match="overlap"):
            call()
    # a result of another overlap than the codec's
    plain = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, 40000)
    with pytest.raises(ValueError, match="overlap"):
        plain.decode(result)
    with pytest.raises(ValueError, match="overlap"):
        codec.decode(plain.encode(P))
    with pytest.raises(ValueError, match="overlap"):
        plain.decode_layered(codec.encode_layered(P, 2))
    for m in (-1, 17):
        with pytest.raises(ValueError):
            spiht_amd.TiledCodec(3, 70, 90, 32, s, None, 40000, overlap=m)
    # the curves without a map are measured as for the encode
    curves = codec.tile_curves(P)
    assert np.asarray(curves.sse).shape == (9, codec.points + 1)


def test_seams_through_the_library():
    """the seam condition of the CPU test once through the library: 128 x 160 in tiles of 64 at 0.5 bpp, m = 4"""
    import spiht_amd
    from test_overlap_cpu import seam_picture, seam_step
    s = spiht_amd.SpihtSettings()
    P = seam_picture(128, 160)
    bits = int(128 * 160 * 0.5)
    step = {}
    for m in (0, 4):
        enc = spiht_amd.encode_image_tiled(P, 64, s, None, bits, overlap=m)
        step[m] = seam_step(np.asarray(spiht_amd.decode_image_tiled(enc, s)) - P, 64, 64)
    print("seam step %.4f with overlap 4, %.4f without: ratio %.3f" % (step[4], step[0], step[4] / step[0]))
    assert step[4] < 0.5 * step[0]


def test_command_line_overlap(tmp_path):
    """python -m spiht_amd.encode_decode IMAGE --tile 32 --overlap 4 [--window Y0,X0,H,W] writes the picture the API gives"""
    import spiht_amd
    from spiht_amd.encode_decode import build_parser, main
    from spiht_amd.utils import imload, imsave
    src = str(tmp_path / "in.png")
    imsave(src, synth_image(6, 3, 70, 90))
    P = imload(src)
    common = [src, "--bpp", "2.0", "--tile", "32", "--overlap", "4", "--color_model", "RGB", "--per_channel_quant_scales",
              "1.,1.,1."]
    enc, dec = main(build_parser().parse_args(common + ["--out", str(tmp_path / "all.png")]))
    s = spiht_amd.SpihtSettings(quantization_scale=255.0, per_channel_quant_scales=[1.0, 1.0, 1.0])
    want = spiht_amd.encode_image_tiled(P, 32, s, 2, round(2.0 * 70 * 90), overlap=4)
    assert isinstance(enc, spiht_amd.TiledResult) and enc == want and enc.overlap == 4 and dec.shape == (3, 70, 90)
    assert np.array_equal(dec, spiht_amd.decode_image_tiled(want, s))
    assert np.array_equal(imload(str(tmp_path / "all.png")), imload_of(dec, tmp_path))
    _, win = main(build_parser().parse_args(common + ["--window", "28,30,10,8", "--out", str(tmp_path / "win.png")]))
    assert np.array_equal(win, dec[:, 28:38, 30:38])
    assert imload(str(tmp_path / "win.png")).shape == (3, 10, 8)
    with pytest.raises(SystemExit):
        main(build_parser().parse_args(common + ["--reduce", "1"]))
    with pytest.raises(SystemExit):
        main(build_parser().parse_args([src, "--overlap", "4"]))


def imload_of(picture, tmp_path):
    """what a picture reads back as after imsave"""
    from spiht_amd.utils import imload, imsave
    path = str(tmp_path / "again.png")
    imsave(path, picture)
    return imload(path)
