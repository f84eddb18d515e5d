"""Region of interest on the GPU: the weighted per-tile error sums (spiht_sse_tiles_w_*) against Python integers and exact
rationals through the C ABI, and TiledCodec's roi= end to end -- the lengths are alloc.allocate of the WEIGHTED curves the
device measured, every cut tile is still the oracle's encode of its pixels at its own length, a map of ones changes nothing,
a map of zeros outside a box gives the tiles outside it no byte, and the weighted error falls where the map asks for it."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

from conftest import synth_image
from test_gpu_alloc import sse_operands, valid
from tile_helpers import dev, tile_pixels

pytestmark = pytest.mark.gpu

vp = C.c_void_p

# N, c, H, W, th, tw, rh, rw: edge tiles, two row chunks and a second picture; odd W (map rows start at odd addresses) and an
# odd tile with a decode buffer one larger; a lane's second column step, 128 further on
SHAPES = [(2, 3, 70, 90, 32, 32, 32, 32), (1, 1, 70, 91, 33, 40, 34, 41), (1, 1, 20, 300, 16, 136, 16, 136)]
G = 3
BEFORE, BEHIND = 13, 40  # bytes of 255 around the map: it starts at an odd address


def tile_box(H, W, th, tw, t):
    """rows and columns of tile t's valid extent in the picture"""
    gx = -(-W // tw)
    i, j = divmod(t, gx)
    vh, vw = valid(H, W, th, tw, t)
    return slice(i * th, i * th + vh), slice(j * tw, j * tw + vw)


def random_maps(rng, M, H, W, th, tw):
    """M maps, random in 0 .. 255; the first tile of the first map all zero, the last tile of the last map all 255"""
    maps = rng.integers(0, 256, (M, H, W), dtype=np.uint8)
    T = -(-H // th) * -(-W // tw)
    maps[0][tile_box(H, W, th, tw, 0)] = 0
    maps[-1][tile_box(H, W, th, tw, T - 1)] = 255
    return maps


def tile_weights(maps, N, H, W, th, tw, t):
    """the weights of tile t of a batch of N pictures over its valid extent; one map serves all pictures"""
    T = -(-H // th) * -(-W // tw)
    return maps[(t // T) % len(maps)][tile_box(H, W, th, tw, t % T)]


def run_sse_w(name, tiles, dec, N, H, W, out_dtype, maps, stride=None):
    """-> [G, NT] of spiht_sse_tiles_w_<name>, between guard words.  maps [M, H, W]: M = 1 with stride 0 is one map for all
    pictures, else one map per picture `stride` bytes apart (None: H * W); every other byte of the buffer is 255"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    g, NT, c, rh, rw = dec.shape
    th, tw = tiles.shape[2:]
    stride = H * W if stride is None else stride
    buf = np.full(BEFORE + max(stride, H * W) * len(maps) + BEHIND, 255, np.uint8)
    for k, m in enumerate(maps):
        buf[BEFORE + k * stride:BEFORE + k * stride + H * W] = m.reshape(-1)
    d_out, d_tiles, d_dec, d_w = dev(np.full(g * NT + 2, 77, out_dtype)), dev(tiles), dev(dec), dev(buf)
    _lib.check(getattr(L, "spiht_sse_tiles_w_" + name)(ctx.handle, vp(d_tiles.ptr), vp(d_dec.ptr), g, N, c, H, W, th, tw, rh, rw,
                                                       vp(d_out.ptr + 8), vp(d_w.ptr + BEFORE), stride))
    ctx.synchronize()
    got = d_out.download()
    assert got[0] == 77 and got[-1] == 77
    return got[1:-1].reshape(g, NT)


def run_sse(name, tiles, dec, N, H, W, out_dtype):
    from test_gpu_alloc import run_sse as plain
    return plain("spiht_sse_tiles_" + name, tiles, dec, N, H, W, out_dtype)


# ---- the kernels ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_integer_sums_are_exact(dtype):
    """equal to Python-integer sums of w (p - d)^2 over the valid extents, every candidate and tile; uint16 also with
    p = 65535, d = 0, w = 255 everywhere in a tile, the largest sum a tile of that size can have"""
    name = "u16" if dtype == np.uint16 else "u8"
    rng = np.random.default_rng(100 + np.dtype(dtype).itemsize)
    for (N, c, H, W, th, tw, rh, rw) in SHAPES:
        tiles, dec = sse_operands(rng, dtype, N, c, H, W, th, tw, rh, rw, G)
        maps = random_maps(rng, N, H, W, th, tw)
        NT = tiles.shape[0]
        if dtype == np.uint16:  # the tile whose weights are all 255
            vh, vw = valid(H, W, th, tw, NT - 1)
            tiles[NT - 1, :, :vh, :vw] = 65535
            dec[:, NT - 1, :, :vh, :vw] = 0
        got = run_sse_w(name, tiles, dec, N, H, W, np.uint64, maps)
        for g in range(G):
            for t in range(NT):
                vh, vw = valid(H, W, th, tw, t)
                e = tiles[t, :, :vh, :vw].astype(object) - dec[g, t, :, :vh, :vw].astype(object)
                want = int((e * e * tile_weights(maps, N, H, W, th, tw, t).astype(object)[None]).sum())
                assert int(got[g, t]) == want, (g, t)
        assert not got[:, 0].any()
        if dtype == np.uint16:
            vh, vw = valid(H, W, th, tw, NT - 1)
            assert int(got[0, NT - 1]) == 255 * 65535 ** 2 * c * vh * vw


def test_f64_sums():
    """float64: finite although whatever lies past the valid extents squares to inf; one call of G = 4 gives the bits of four
    calls of G = 1; a map of ones gives the bits of spiht_sse_tiles_f64; within (n + 3) 2^-52 S of the exact rational sum S of
    n = c vh vw terms.  The bound: a term is a subtraction, a square and a product with the weight, each rounded once, so
    (p - d)^2 w (1 + 2 d1 + d2 + d3), at most 4 u off to first order, u = 2^-53; a term passes through at most n - 1 of the
    additions, each rounded once: |S - S_exact| <= (n + 3) u S_exact, every term being >= 0 (the unweighted sum
    has (n + 2) u).  The test allows twice that."""
    rng = np.random.default_rng(80)
    for (N, c, H, W, th, tw, rh, rw) in SHAPES:
        tiles, dec = sse_operands(rng, np.float64, N, c, H, W, th, tw, rh, rw, 4)
        maps = random_maps(rng, N, H, W, th, tw)
        NT = tiles.shape[0]
        got = run_sse_w("f64", tiles, dec, N, H, W, np.float64, maps)
        assert np.isfinite(got).all()
        for g in range(4):
            one = run_sse_w("f64", tiles, dec[g:g + 1], N, H, W, np.float64, maps)
            assert np.array_equal(one[0].view(np.uint64), got[g].view(np.uint64)), g
        ones = run_sse_w("f64", tiles, dec, N, H, W, np.float64, np.ones((1, H, W), np.uint8), 0)
        assert np.array_equal(ones.view(np.uint64), run_sse("f64", tiles, dec, N, H, W, np.float64).view(np.uint64))
        for t in range(NT):  # the bound, on the first candidate
            vh, vw = valid(H, W, th, tw, t)
            wt = tile_weights(maps, N, H, W, th, tw, t)
            S = Fraction(0)
            for ch in range(c):
                for p, d, w in zip(tiles[t, ch, :vh, :vw].reshape(-1).tolist(), dec[0, t, ch, :vh, :vw].reshape(-1).tolist(),
                                   wt.reshape(-1).tolist()):
                    e = Fraction(p) - Fraction(d)
                    S += w * e * e
            assert abs(Fraction(float(got[0, t])) - S) <= (c * vh * vw + 3) * Fraction(1, 2 ** 52) * S, t
        assert not got[:, 0].any()  # the tile of zero weights: exactly 0


@pytest.mark.parametrize("name,dtype,out", [("f64", np.float64, np.float64), ("u8", np.uint8, np.uint64)])
def test_map_stride(name, dtype, out):
    """w_stride = 0 with one map is w_stride = H W with that map twice; two different maps for two pictures, H W + 7 bytes
    apart, are two calls of N = 1"""
    N, c, H, W, th, tw, rh, rw = SHAPES[0]
    rng = np.random.default_rng(81)
    tiles, dec = sse_operands(rng, dtype, N, c, H, W, th, tw, rh, rw, 2)
    maps = random_maps(rng, 2, H, W, th, tw)
    T = tiles.shape[0] // N
    shared = run_sse_w(name, tiles, dec, N, H, W, out, maps[:1], 0)
    twice = run_sse_w(name, tiles, dec, N, H, W, out, np.stack([maps[0], maps[0]]))
    assert np.array_equal(shared.view(np.uint64), twice.view(np.uint64))
    both = run_sse_w(name, tiles, dec, N, H, W, out, maps, H * W + 7)
    for n in range(2):
        alone = run_sse_w(name, tiles[n * T:(n + 1) * T], dec[:, n * T:(n + 1) * T], 1, H, W, out, maps[n:n + 1])
        assert np.array_equal(alone.view(np.uint64), both[:, n * T:(n + 1) * T].view(np.uint64)), n
    assert not np.array_equal(both[:, :T], both[:, T:])


def test_argument_errors():
    """one by one, each SPIHT_ERR_ARG, and nothing is written"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    d = dev(np.full(64, 3.0, np.float64))
    keys = ("G", "N", "c", "H", "W", "th", "tw", "rh", "rw")
    ok = dict(G=1, N=1, c=1, H=70, W=90, th=32, tw=32, rh=32, rw=32, w=d.ptr, stride=0)
    bad = [dict(w=None), dict(stride=1), dict(stride=70 * 90 - 1), dict(N=2, stride=70 * 90 - 1),
           dict(G=0), dict(N=0), dict(c=0), dict(rh=31), dict(rw=31), dict(th=4), dict(H=0)]
    for fn in (L.spiht_sse_tiles_w_f64, L.spiht_sse_tiles_w_u8, L.spiht_sse_tiles_w_u16):
        for b in bad:
            a = dict(ok)
            a.update(b)
            assert fn(ctx.handle, vp(d.ptr), vp(d.ptr), *[a[k] for k in keys], vp(d.ptr), vp(a["w"]), a["stride"]) == _lib.ERR_ARG, b
        assert fn(None, vp(d.ptr), vp(d.ptr), *[ok[k] for k in keys], vp(d.ptr), vp(d.ptr), 0) == _lib.ERR_ARG
    # the exact integer sum: c th tw <= 2^24
    for fn in (L.spiht_sse_tiles_w_u8, L.spiht_sse_tiles_w_u16):
        for c, th, tw in [(65, 512, 512), (1, 4096, 4104), (2 ** 14 + 1, 32, 32)]:
            a = dict(ok, c=c, H=th, W=tw, th=th, tw=tw, rh=th, rw=tw)
            assert fn(ctx.handle, vp(d.ptr), vp(d.ptr), *[a[k] for k in keys], vp(d.ptr), vp(d.ptr), 0) == _lib.ERR_ARG, (c, th, tw)
    ctx.synchronize()
    assert (d.download() == 3.0).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------

H, W, TILE, MAX_BITS, POINTS = 70, 90, 32, 27005, 8
BOX = (20, 30, 30, 40)  # meets the tiles 0 .. 5 of the 3 x 3 grid; the bottom row lies outside it
CASES = {"f64": dict(), "u8": dict(dtype=np.uint8), "ipt": dict(color="IPT")}


def the_map(background=1):
    import spiht_amd
    return spiht_amd.roi_map(H, W, [BOX], background=background)


def picture(cfg):
    P = synth_image(4163, 3, H, W)
    if "dtype" in cfg:
        P = np.round(P * 255).astype(cfg["dtype"])
    P.setflags(write=False)
    return P


def new_codec(cfg):
    import spiht_amd
    s = spiht_amd.SpihtSettings(color_model=cfg.get("color"))
    return s, spiht_amd.TiledCodec(3, H, W, TILE, s, None, MAX_BITS, allocate="rd", points=POINTS)


@functools.lru_cache(maxsize=None)
def case(name):
    """the picture, map, settings, codec, result, cut and weighted curves of a case: computed once, shared, never changed"""
    cfg = CASES[name]
    P, m = picture(cfg), the_map()
    s, codec = new_codec(cfg)
    res = codec.encode_u8(P, roi=m) if "dtype" in cfg else codec.encode(P, roi=m)
    cut = codec.last_allocation
    curves = codec.tile_curves(P, cfg.get("dtype"), roi=m)
    return cfg, P, m, s, codec, res, cut, curves


def weighted_error(m, P, dec):
    e = P.astype(np.float64) - dec.astype(np.float64)
    return float((m[None].astype(np.float64) * (e * e)).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end(oracle, name):
    import spiht_amd
    from spiht_amd import _lib, alloc, color_models
    cfg, P, m, s, codec, res, cut, curves = case(name)
    integer = "dtype" in cfg
    th = tw = TILE
    T, budget = codec.T, MAX_BITS // 8
    # the lengths are the rule's, fed by the weighted curves the device measured; last_allocation reports that table's lambda*
    assert curves.sse.shape == (T, POINTS + 1) and curves.sse.dtype == (np.uint64 if integer else np.float64)
    want, lam = alloc.allocate(curves.lengths, curves.sse, budget)
    assert res.nbytes == want and cut == spiht_amd.TileAllocation(lam, want)
    ends = sum(r[alloc.lower_hull(r, d)[-1]] for r, d in zip(curves.lengths, curves.sse))
    assert sum(res.nbytes) == min(budget, ends) == len(res.encoded_bytes)
    assert res.max_n == curves.max_n
    # the map moved the cut: the unweighted call gives other lengths
    plain = codec.encode_u8(P) if integer else codec.encode(P)
    assert plain.nbytes != res.nbytes
    # every tile is the oracle's encode of its pixels at its own length; the decode is the paste of the tiles' decodes
    tiles_px = [tile_pixels(P, th, tw, *divmod(t, codec.gx)) for t in range(T)]
    pasted = np.zeros((3, codec.gy * th, codec.gx * tw))
    for t in range(T):
        i, j = divmod(t, codec.gx)
        e = res.tile(i, j)
        px = tiles_px[t] / 255.0 if integer else tiles_px[t]
        if cfg.get("color"):  # the oracle has no colour step: it codes the pixels in the device's own IPT
            d = dev(px[None])
            color_models.device_convert(_lib.default_context(), d.ptr, 1, th * tw, "RGB", cfg["color"])
            _lib.default_context().synchronize()
            px = d.download()[0]
        if len(e.encoded_bytes):
            ob, on, _ = oracle.encode_image(px, s.wavelet, s.mode, None, s.quantization_scale, None, 8 * len(e.encoded_bytes))
            assert e.encoded_bytes == ob and e.max_n == on, t
        pasted[:, i * th:(i + 1) * th, j * tw:(j + 1) * tw] = spiht_amd.decode_image(e, s)[:, :th, :tw]
    dec = codec.decode(res)
    assert np.array_equal(dec, pasted[:, :H, :W])
    assert np.array_equal(codec.decode_window(res, 28, 30, 10, 8), dec[:, 28:38, 30:38])
    assert np.array_equal(spiht_amd.decode_image_tiled(spiht_amd.TiledResult.from_bytes(res.to_bytes()), s), dec)
    # sse[t][k] is the weighted error of decode_image of the first lengths[t][k] bytes of the tile's full stream
    full = codec.codec.encode_u8(np.stack(tiles_px)) if integer else codec.codec.encode(np.stack(tiles_px))
    for t in range(T):
        assert len(full[t].encoded_bytes) == curves.nbytes[t] and full[t].max_n == curves.max_n[t]
        vh, vw = valid(H, W, th, tw, t)
        wt = m[tile_box(H, W, th, tw, t)]
        for k, length in enumerate(curves.lengths[t]):
            pre = spiht_amd.EncodingResult(full[t].encoded_bytes[:length], th, tw, 3, full[t].max_n, None)
            if integer:
                e = tiles_px[t][:, :vh, :vw].astype(np.int64) - spiht_amd.decode_image_u8(pre, s)[:, :vh, :vw].astype(np.int64)
                assert int(curves.sse[t, k]) == int((e * e * wt[None].astype(np.int64)).sum()), (t, k)
            else:
                S = weighted_error(wt, tiles_px[t][:, :vh, :vw], spiht_amd.decode_image(pre, s)[:, :vh, :vw])
                assert abs(curves.sse[t, k] - S) <= (3 * vh * vw + 3) * 2.0 ** -52 * S, (t, k)
    # the numbers do not depend on the grouping: one candidate at a time
    codec.max_bytes = 1
    try:
        again = codec.tile_curves(P, cfg.get("dtype"), roi=m)
    finally:
        codec.max_bytes = 2 ** 31
    assert np.array_equal(again.sse.view(np.uint64), curves.sse.view(np.uint64)) and codec.last_allocation == cut
    # the convenience is the same call
    if integer:
        conv = spiht_amd.encode_image_tiled_u8(P, TILE, s, None, MAX_BITS, allocate="rd", points=POINTS, roi=m)
    else:
        conv = spiht_amd.encode_image_tiled(P, TILE, s, None, MAX_BITS, allocate="rd", points=POINTS, roi=m)
    assert conv == res


def test_a_map_of_ones_changes_nothing():
    cfg, P, m, s, codec, res, cut, curves = case("f64")
    ones = np.ones((H, W), np.uint8)
    plain = codec.encode(P)
    plain_cut = codec.last_allocation
    assert codec.encode(P, roi=ones) == plain and codec.last_allocation == plain_cut
    assert codec.encode(P, roi=ones.astype(bool)) == plain
    a, b = codec.tile_curves(P, roi=ones), codec.tile_curves(P)
    assert np.array_equal(a.sse.view(np.uint64), b.sse.view(np.uint64))
    assert codec.encode_layered(P, 4, roi=ones) == codec.encode_layered(P, 4)
    Pu = picture(CASES["u8"])
    assert codec.encode_u8(Pu, roi=ones) == codec.encode_u8(Pu)


def test_zero_outside_the_box():
    """every tile that does not meet the box has 0 bytes at every layer, the picture still decodes, and the tiles that meet the
    box share the whole budget"""
    import spiht_amd
    from spiht_amd import alloc
    cfg, P, m, s, codec, res, cut, curves = case("f64")
    zero = the_map(background=0)
    inside = [t for t in range(codec.T) if zero[tile_box(H, W, TILE, TILE, t)].any()]
    assert inside == [0, 1, 2, 3, 4, 5]
    r = codec.encode(P, roi=zero)
    assert all((r.nbytes[t] > 0) == (t in inside) for t in range(codec.T))
    assert sum(r.nbytes) == MAX_BITS // 8
    dec = codec.decode(r)
    assert dec.shape == (3, H, W) and np.isfinite(dec).all()
    assert np.array_equal(dec[:, 64:, :32], spiht_amd.decode_image(r.tile(2, 0), s)[:, :H - 64, :32])  # as an empty stream does
    lay = codec.encode_layered(P, 4, roi=zero)
    assert lay.tiled() == r
    assert all(lay.cum[q][t] == 0 for q in range(4) for t in range(codec.T) if t not in inside)
    assert sum(lay.cum[0]) == alloc.layer_budgets(MAX_BITS, 4)[0] // 8  # layer 0 is spent inside the box, to the byte


def test_it_helps_where_asked():
    """the weighted error sum of w (P - decode)^2 at the same 3375 bytes: on the CPU, the oracle feeding alloc.allocate,
    3000.58 for the plain allocate="rd" cut and 1366.24 with roi_map(70, 90, [(20, 30, 30, 40)]) (966.03 against 2950.20 with
    background 0): no margin is needed"""
    cfg, P, m, s, codec, res, cut, curves = case("f64")
    plain = codec.encode(P)
    assert sum(plain.nbytes) == sum(res.nbytes) == MAX_BITS // 8
    a, b = weighted_error(m, P, codec.decode(plain)), weighted_error(m, P, codec.decode(res))
    print("weighted error: plain rd %.4f, roi %.4f" % (a, b))
    assert b < a


def test_layers():
    """the cumulative table is alloc.allocate_layers of the weighted curves; the decode of q layers is the decode of the cut
    alloc.allocate makes at layer q's budget, and all layers are encode's picture with the same map"""
    import spiht_amd
    from spiht_amd import alloc
    cfg, P, m, s, codec, res, cut, curves = case("f64")
    lay = codec.encode_layered(P, 4, roi=m)
    cuts = codec.last_allocation
    budgets = [b // 8 for b in alloc.layer_budgets(MAX_BITS, 4)]
    cum, lams = alloc.allocate_layers(curves.lengths, curves.sse, budgets)
    assert lay.cum == cum and [a.lam for a in cuts] == lams and [a.nbytes for a in cuts] == cum
    assert lay.tiled() == res
    off = np.concatenate(([0], np.cumsum(res.nbytes)))
    for q in range(1, 5):
        at_q = spiht_amd.TiledResult(H, W, 3, TILE, TILE, None, res.max_n, cum[q - 1],
                                     b"".join(res.encoded_bytes[off[t]:off[t] + cum[q - 1][t]] for t in range(codec.T)))
        assert lay.tiled(q) == at_q
        assert np.array_equal(codec.decode_layered(lay, upto=q), codec.decode(at_q)), q
    back = spiht_amd.LayeredResult.from_bytes(lay.to_bytes())
    assert back == lay and np.array_equal(codec.decode_layered(back), codec.decode(res))
    assert spiht_amd.encode_image_layered(P, TILE, s, None, MAX_BITS, 4, points=POINTS, roi=m) == lay
    Pu = picture(CASES["u8"])
    assert codec.encode_layered_u8(Pu, 4, roi=m).tiled() == codec.encode_u8(Pu, roi=m)


def test_two_pictures_two_maps_one_call():
    cfg, P, m, s, codec, res, cut, curves = case("f64")
    Q = synth_image(91, 3, H, W)
    m2 = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
    many = codec.encode(np.stack([P, Q]), roi=np.stack([m, m2]))
    cuts = codec.last_allocation
    assert many[0] == res and cuts[0] == cut
    assert many[1] == codec.encode(Q, roi=m2) and cuts[1] == codec.last_allocation
    shared = codec.encode(np.stack([P, Q]), roi=m)  # one map for both
    assert shared[0] == res and shared[1] == codec.encode(Q, roi=m) and shared[1] != many[1]
    lay = codec.encode_layered(np.stack([P, Q]), 4, roi=np.stack([m, m2]))
    assert lay[0].tiled() == res and lay[1].tiled() == many[1]


def test_device_form():
    """encode_device with a device map gives the host form's bytes; the map lies at an odd address between other bytes"""
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    cfg, P, m, s, codec, res, cut, curves = case("f64")
    ctx = _lib.default_context()
    Q = synth_image(91, 3, H, W)
    m2 = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
    want = codec.encode(np.stack([P, Q]), roi=np.stack([m, m2]))
    stride = H * W + 3
    buf = np.full(BEFORE + 2 * stride + BEHIND, 255, np.uint8)
    buf[BEFORE:BEFORE + H * W] = m.reshape(-1)
    buf[BEFORE + stride:BEFORE + stride + H * W] = m2.reshape(-1)
    d_img, d_roi = dev(np.stack([P, Q])), dev(buf)
    NT = 2 * codec.T
    d_packed = DeviceArray(ctx, (NT * codec.codec.slot_stride,), np.uint8)
    d_lens, d_maxn = DeviceArray(ctx, (NT,), np.uint32), DeviceArray(ctx, (NT,), np.uint8)
    codec.encode_device(d_img, 2, d_packed, d_lens, d_maxn, d_roi=d_roi.ptr + BEFORE, roi_stride=stride)
    ctx.synchronize()
    lens, packed = d_lens.download(), d_packed.download()
    assert lens.tolist() == want[0].nbytes + want[1].nbytes
    assert d_maxn.download().tolist() == want[0].max_n + want[1].max_n
    assert packed[:int(lens.sum())].tobytes() == want[0].encoded_bytes + want[1].encoded_bytes
    with pytest.raises(ValueError):
        codec.encode_device(d_img, 2, d_packed, d_lens, d_maxn, d_roi=d_roi.ptr, roi_stride=H * W - 1)


def test_refusals():
    """a map on a codec without allocate="rd", a map of the wrong kind, integer tiles too large for the exact weighted sum"""
    import spiht_amd
    P, m = picture(CASES["f64"]), the_map()
    s = spiht_amd.SpihtSettings()
    equal = spiht_amd.TiledCodec(3, H, W, TILE, s, None, MAX_BITS)
    with pytest.raises(ValueError):
        equal.encode(P, roi=m)
    with pytest.raises(ValueError):
        equal.encode_u8(picture(CASES["u8"]), roi=m)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_tiled(P, TILE, s, None, MAX_BITS, roi=m)
    assert equal.encode(P, roi=None) == equal.encode(P)
    cfg, P, m, s, codec, res, cut, curves = case("f64")
    with pytest.raises(TypeError):
        codec.encode(P, roi=m.astype(np.float64))
    with pytest.raises(ValueError):
        codec.encode(P, roi=m[:, :-1])
    with pytest.raises(ValueError):
        codec.encode(P, roi=np.stack([m, m]))
    big = spiht_amd.TiledCodec(3, 4096, 4096, 4096, s, None, 10 ** 6, allocate="rd")  # 3 * 2^24 samples a tile
    with pytest.raises(ValueError):  # refused before anything is uploaded
        big.encode_u8(np.zeros((3, 4096, 4096), np.uint8), roi=np.ones((4096, 4096), np.uint8))
    big.close()


def test_command_line_roi(tmp_path):
    import spiht_amd
    from spiht_amd.encode_decode import build_parser, main
    from spiht_amd.utils import imload, imsave
    src = str(tmp_path / "in.png")
    imsave(src, synth_image(6, 3, H, W))
    P = imload(src)
    out = str(tmp_path / "out.png")
    common = [src, "--bpp", "2.0", "--tile", "32", "--color_model", "RGB", "--per_channel_quant_scales", "1.,1.,1.", "--out", out]
    rd = ["--allocate", "rd", "--points", "8"]
    s = spiht_amd.SpihtSettings(quantization_scale=255.0, per_channel_quant_scales=[1.0, 1.0, 1.0])
    bits = round(2.0 * H * W)
    enc, dec = main(build_parser().parse_args(common + rd + ["--roi", "20,30,30,40"]))
    assert enc == spiht_amd.encode_image_tiled(P, 32, s, 2, bits, allocate="rd", points=8, roi=the_map())
    assert enc != spiht_amd.encode_image_tiled(P, 32, s, 2, bits, allocate="rd", points=8)
    assert np.array_equal(dec, spiht_amd.decode_image_tiled(enc, s))
    imsave(str(tmp_path / "want.png"), dec)
    assert np.array_equal(imload(out), imload(str(tmp_path / "want.png")))
    # weight and background, twice: the larger weight where the boxes overlap
    enc, _ = main(build_parser().parse_args(common + rd + ["--roi", "20,30,30,40:200:0", "--roi", "0,0,30,40:9"]))
    m = spiht_amd.roi_map(H, W, [(20, 30, 30, 40, 200), (0, 0, 30, 40, 9)], background=0)
    assert m[25, 35] == 200 and m[0, 0] == 9 and m[69, 89] == 0
    assert enc == spiht_amd.encode_image_tiled(P, 32, s, 2, bits, allocate="rd", points=8, roi=m)
    lay, dec = main(build_parser().parse_args(common + rd + ["--layers", "3", "--roi", "20,30,30,40"]))
    assert lay == spiht_amd.encode_image_layered(P, 32, s, 2, bits, 3, points=8, roi=the_map())
    assert np.array_equal(dec, spiht_amd.decode_image_layered(lay, s))
    for bad in (common + ["--roi", "20,30,30,40"], common + ["--layers", "3", "--roi", "20,30,30,40"], [src, "--roi", "20,30,30,40"],
                common + rd + ["--roi", "20,30,30"], common + rd + ["--roi", "20,30,30,40:300"]):
        with pytest.raises(SystemExit):
            main(build_parser().parse_args(bad))
