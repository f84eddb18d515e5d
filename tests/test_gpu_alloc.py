"""Rate allocation across tiles on the GPU: the three kernels against their numpy / Python statements through the C ABI, and
TiledCodec(allocate="rd") end to end -- the lengths are alloc.allocate of the measured curves, every cut tile is still the
oracle's encode of the tile's pixels at its own length, and the allocated picture is better than the equal split."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

from alloc_cases import PINNED
from conftest import synth_image
from tile_helpers import dev, padded, tile_pixels

pytestmark = pytest.mark.gpu

vp = C.c_void_p


# ---- prefix slots ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k0,G", [(0, 9), (3, 2), (8, 1)])
def test_prefix_slots(k0, G):
    """slot (k - k0) NT + t = the first ceil(n_t k / K) bytes of slot t and zeros behind, between guard bytes; lengths 0, 1,
    n < K and a full slot; both slot bases 4 bytes off a 16-byte boundary; the source slots have no zero byte at all"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    K, stride, out_stride = 8, 4100, 4104
    n = [0, 1, 3, 4100, 700, 4099]
    NT = len(n)
    rng = np.random.default_rng(k0)
    slots = rng.integers(1, 256, (NT, stride), dtype=np.uint8)
    nbits = np.array([8 * v - (3 if v else 0) for v in n], np.uint64)
    max_n = np.array([3, 0, 9, 30, 1, 7], np.uint8)
    d_slots = dev(np.concatenate([np.full(4, 0x77, np.uint8), slots.reshape(-1)]))
    guard = np.full(36 + G * NT * out_stride + 64, 0xEE, np.uint8)
    d_out, d_nbytes, d_maxn = dev(guard), dev(np.full(G * NT + 2, 2 ** 64 - 1, np.uint64)), dev(np.full(G * NT + 2, 0xCC, np.uint8))
    d_nbits, d_max_n = dev(nbits), dev(max_n)
    _lib.check(L.spiht_tile_prefix_slots(ctx.handle, vp(d_slots.ptr + 4), stride, vp(d_nbits.ptr), NT, K, k0, G, vp(d_out.ptr + 36),
                                         out_stride, vp(d_nbytes.ptr + 8), vp(d_max_n.ptr), vp(d_maxn.ptr + 1)))
    ctx.synchronize()
    got, nb, mn = d_out.download(), d_nbytes.download(), d_maxn.download()
    want_len = [-(-v * k // K) for k in range(k0, k0 + G) for v in n]
    assert nb.tolist() == [2 ** 64 - 1] + want_len + [2 ** 64 - 1]
    assert mn.tolist() == [0xCC] + max_n.tolist() * G + [0xCC]
    body = got[36:36 + G * NT * out_stride].reshape(G * NT, out_stride)
    for s, length in enumerate(want_len):
        assert np.array_equal(body[s, :length], slots[s % NT, :length]), s
        assert not body[s, length:].any(), s
    assert (got[:36] == 0xEE).all() and (got[36 + G * NT * out_stride:] == 0xEE).all()
    # argument errors, before anything is queued
    bad = [dict(K=0), dict(K=256), dict(k0=-1), dict(G=0), dict(k0=8, G=2), dict(out_stride=4102), dict(out=d_out.ptr + 1)]
    for b in bad:
        a = dict(K=K, k0=0, G=1, out_stride=out_stride, out=d_out.ptr)
        a.update(b)
        assert L.spiht_tile_prefix_slots(ctx.handle, vp(d_slots.ptr + 4), stride, vp(d_nbytes.ptr), NT, a["K"], a["k0"], a["G"],
                                         vp(a["out"]), a["out_stride"], vp(d_nbytes.ptr), None, None) == _lib.ERR_ARG, b


# ---- per-tile error sums ----------------------------------------------------------------------------------------------------

def valid(H, W, th, tw, t):
    gx = -(-W // tw)
    i, j = divmod(t % (-(-H // th) * gx), gx)
    return min(th, H - i * th), min(tw, W - j * tw)


def sse_operands(rng, dtype, N, c, H, W, th, tw, rh, rw, G):
    """tiles [NT, c, th, tw] and decodes [G, NT, c, rh, rw]; whatever lies past a tile's valid extent -- the replicated padding
    of edge tiles, the extra row and column of an odd tile's float64 decode -- is garbage in both"""
    NT = N * -(-H // th) * -(-W // tw)
    if np.dtype(dtype).kind == "u":
        peak = np.iinfo(dtype).max
        tiles = rng.integers(0, peak + 1, (NT, c, th, tw)).astype(dtype)
        dec = rng.integers(0, peak + 1, (G, NT, c, rh, rw)).astype(dtype)
        junk = lambda shape: rng.integers(0, peak + 1, shape).astype(dtype)  # noqa: E731
    else:
        tiles = rng.random((NT, c, th, tw))
        dec = tiles[None, :, :, :1, :1] + 0.1 * rng.standard_normal((G, NT, c, rh, rw))
        junk = lambda shape: np.full(shape, 1e200) * rng.choice([-1.0, 1.0], shape)  # noqa: E731  (squares to inf)
    for t in range(NT):
        vh, vw = valid(H, W, th, tw, t)
        tiles[t, :, vh:, :] = junk(tiles[t, :, vh:, :].shape)
        tiles[t, :, :, vw:] = junk(tiles[t, :, :, vw:].shape)
        dec[:, t, :, vh:, :] = junk(dec[:, t, :, vh:, :].shape)
        dec[:, t, :, :, vw:] = junk(dec[:, t, :, :, vw:].shape)
    return tiles, dec


def run_sse(name, tiles, dec, N, H, W, out_dtype):
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    G, NT, c, rh, rw = dec.shape
    th, tw = tiles.shape[2:]
    d_out, d_tiles, d_dec = dev(np.full(G * NT + 2, 77, out_dtype)), dev(tiles), dev(dec)
    _lib.check(getattr(L, name)(ctx.handle, vp(d_tiles.ptr), vp(d_dec.ptr), G, N, c, H, W, th, tw, rh, rw, vp(d_out.ptr + 8)))
    ctx.synchronize()
    got = d_out.download()
    assert got[0] == 77 and got[-1] == 77
    return got[1:-1].reshape(G, NT)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_sse_tiles_integer_exact(dtype):
    """2 x 3 x 70 x 90 in tiles of 32 (padded edge tiles, more than one row chunk, a second picture) and 1 x 70 x 90 in tiles
    of (33, 40): exact against int64 sums over the valid extents"""
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    for (N, c, H, W, th, tw) in [(2, 3, 70, 90, 32, 32), (1, 1, 70, 90, 33, 40)]:
        tiles, dec = sse_operands(rng, dtype, N, c, H, W, th, tw, th, tw, 3)
        got = run_sse("spiht_sse_tiles_u16" if dtype == np.uint16 else "spiht_sse_tiles_u8", tiles, dec, N, H, W, np.uint64)
        for g in range(3):
            for t in range(tiles.shape[0]):
                vh, vw = valid(H, W, th, tw, t)
                e = tiles[t, :, :vh, :vw].astype(np.int64) - dec[g, t, :, :vh, :vw].astype(np.int64)
                assert int(got[g, t]) == int((e * e).sum()), (g, t)


def test_sse_tiles_f64_bound_and_grouping():
    """float64: within (n + 3) 2^-52 S of the exact rational sum S, n = c vh vw terms (n - 1 additions, and a
    subtraction and a product per term, each rounded once); the garbage past the valid extent would make the sum inf; one call
    of G = 4 gives the bits of four calls of G = 1"""
    rng = np.random.default_rng(8)
    for (N, c, H, W, th, tw, rh, rw) in [(1, 2, 70, 90, 33, 40, 34, 41), (2, 1, 70, 90, 32, 32, 32, 32)]:
        tiles, dec = sse_operands(rng, np.float64, N, c, H, W, th, tw, rh, rw, 4)
        got = run_sse("spiht_sse_tiles_f64", tiles, dec, N, H, W, np.float64)
        assert np.isfinite(got).all()
        for g in range(4):
            one = run_sse("spiht_sse_tiles_f64", tiles, dec[g:g + 1], N, H, W, np.float64)
            assert np.array_equal(one[0].view(np.uint64), got[g].view(np.uint64)), g
        for t in range(tiles.shape[0]):  # the bound, on the first candidate
            vh, vw = valid(H, W, th, tw, t)
            S = Fraction(0)
            for p, d in zip(tiles[t, :, :vh, :vw].reshape(-1).tolist(), dec[0, t, :, :vh, :vw].reshape(-1).tolist()):
                e = Fraction(p) - Fraction(d)
                S += e * e
            assert abs(Fraction(float(got[0, t])) - S) <= (c * vh * vw + 3) * Fraction(1, 2 ** 52) * S, t


def test_sse_tiles_argument_errors():
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    d = dev(np.zeros(64, np.float64))
    ok = dict(G=1, N=1, c=1, H=70, W=90, th=32, tw=32, rh=32, rw=32)
    for b in [dict(G=0), dict(N=0), dict(c=0), dict(rh=31), dict(rw=31), dict(th=4), dict(H=0)]:
        a = dict(ok)
        a.update(b)
        assert L.spiht_sse_tiles_f64(ctx.handle, vp(d.ptr), vp(d.ptr), *[a[k] for k in ("G", "N", "c", "H", "W", "th", "tw", "rh", "rw")],
                                     vp(d.ptr)) == _lib.ERR_ARG, b


# ---- the allocation kernel ---------------------------------------------------------------------------------------------------

def run_allocate(nbytes, K, D, budget, kind):
    """nbytes [N][T], D [N][T][K + 1] -> (bytes [N][T], lambda [N]) of spiht_tile_allocate, between guard words"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    nbytes = np.asarray(nbytes, np.uint64)
    N, T = nbytes.shape
    nbits = np.where(nbytes > 0, 8 * nbytes - 5, 0).astype(np.uint64)  # a last byte that is not full
    table = np.ascontiguousarray(np.asarray(D, np.uint64 if kind else np.float64).reshape(N * T, K + 1).T)
    d_out, d_lam, d_nbits, d_table = dev(np.full(N * T + 2, 99, np.uint64)), dev(np.full(N + 2, -1.0)), dev(nbits.reshape(-1)), dev(table)
    _lib.check(L.spiht_tile_allocate(ctx.handle, vp(d_nbits.ptr), vp(d_table.ptr), kind, K, N, T, int(budget),
                                     vp(d_out.ptr + 8), vp(d_lam.ptr + 8)))
    ctx.synchronize()
    out, lam = d_out.download(), d_lam.download()
    assert out[0] == 99 and out[-1] == 99 and lam[0] == -1.0 and lam[-1] == -1.0
    assert not (out[1:-1] % 8).any()
    return (out[1:-1] // 8).reshape(N, T).tolist(), lam[1:-1].tolist()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", list(PINNED))
def test_allocate_pinned(name, kind):
    case = PINNED[name]
    out, lam = run_allocate([case["nbytes"]], case["K"], [case["D"]], case["budget"], kind)
    assert out == [case["want"]] and lam == [case["lam"]]


def random_table(rng, N, T, K, nmax, integer):
    """curves that fall, with noise large enough that some points rise again and many lie above their hull"""
    nbytes = rng.integers(0, nmax, (N, T))
    nbytes[rng.random((N, T)) < 0.05] = 0
    drop = rng.random((N, T, K + 1)) ** 3 * rng.integers(1, 1000, (N, T, 1))
    D = np.cumsum(drop[:, :, ::-1], axis=2)[:, :, ::-1] + rng.random((N, T, K + 1)) * 30
    if integer:
        D = (D * 2 ** 40).astype(np.uint64) + np.uint64(2 ** 60 + 1)  # every sum above 2^53: the one rounding counts
    for n in range(N):  # D is a function of R: equal lengths share one distortion
        for t in range(T):
            R = [-(-int(nbytes[n, t]) * k // K) for k in range(K + 1)]
            for k in range(1, K + 1):
                if R[k] == R[k - 1]:
                    D[n, t, k] = D[n, t, k - 1]
    return nbytes, D


@pytest.mark.parametrize("N,T,K,kind", [(1, 1500, 4, 0), (2, 300, 16, 0), (2, 37, 255, 1), (1, 257, 7, 1)])
def test_allocate_random_tables(N, T, K, kind):
    """exact in every length and in lambda* against alloc.allocate: more tiles than a workgroup has lanes, two pictures in a
    call, K at its limit, uint64 sums above 2^53; budgets from nothing to more than the hulls hold"""
    from spiht_amd import alloc
    rng = np.random.default_rng(T)
    nbytes, D = random_table(rng, N, T, K, 3000, kind == 1)
    total = int(nbytes.sum(axis=1).min())
    for budget in (0, 1, total // 7, total // 2, total - 1, 2 * total):
        out, lam = run_allocate(nbytes, K, D, budget, kind)
        for n in range(N):
            R = [alloc.tile_lengths(int(v), K) for v in nbytes[n]]
            want, wlam = alloc.allocate(R, D[n], budget)
            assert lam[n] == wlam, (budget, n)
            assert out[n] == want, (budget, n)


def test_allocate_argument_errors():
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    d = dev(np.zeros(64, np.uint64))
    for kind, K, N, T in [(2, 4, 1, 4), (0, 0, 1, 4), (0, 256, 1, 4), (0, 4, -1, 4), (0, 4, 1, 0)]:
        assert L.spiht_tile_allocate(ctx.handle, vp(d.ptr), vp(d.ptr), kind, K, N, T, 10, vp(d.ptr), None) == _lib.ERR_ARG


# ---- end to end -----------------------------------------------------------------------------------------------------------------

CASES = {
    "grid3x3": dict(c=3, H=70, W=90, tile=32, max_bits=27005),
    "grey": dict(c=1, H=70, W=90, tile=32, max_bits=27005),
    "oddtile": dict(c=1, H=70, W=90, tile=(33, 40), max_bits=20000),
    "ipt": dict(c=3, H=70, W=90, tile=32, max_bits=27005, color="IPT"),
    "u8": dict(c=3, H=70, W=90, tile=32, max_bits=27005, dtype=np.uint8),
}
POINTS = 8


def picture(cfg):
    P = synth_image(4000 + cfg["H"] + cfg["W"] + cfg["c"], cfg["c"], cfg["H"], cfg["W"])
    if "dtype" in cfg:
        P = np.round(P * 255).astype(cfg["dtype"])
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def case(name):
    """the picture, settings, codec, result and curves of a case: computed once, shared, never changed"""
    import spiht_amd
    cfg = CASES[name]
    P = picture(cfg)
    s = spiht_amd.SpihtSettings(color_model=cfg.get("color"))
    codec = spiht_amd.TiledCodec(cfg["c"], cfg["H"], cfg["W"], cfg["tile"], s, None, cfg["max_bits"], allocate="rd", points=POINTS)
    if "dtype" in cfg:
        res = codec.encode_u8(np.ascontiguousarray(P.transpose(1, 2, 0)), channels_last=True)
    else:
        res = codec.encode(P)
    cut = codec.last_allocation
    curves = codec.tile_curves(P, cfg.get("dtype"))
    return cfg, P, s, codec, res, cut, curves


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end(oracle, name):
    import spiht_amd
    from spiht_amd import _lib, alloc, color_models
    cfg, P, s, codec, res, cut, curves = case(name)
    c, H, W = P.shape
    th, tw = codec.th, codec.tw
    T, budget = codec.T, cfg["max_bits"] // 8
    # the lengths are the rule's, fed by the curves the device measured
    assert len(curves.lengths) == T and curves.sse.shape == (T, POINTS + 1)
    assert curves.sse.dtype == (np.uint64 if "dtype" in cfg else np.float64)
    assert all(r == alloc.tile_lengths(n, POINTS) for r, n in zip(curves.lengths, curves.nbytes))
    ceiling = alloc.ceiling_bits(cfg["max_bits"], T, 4.0)
    assert ceiling % 8 == 0 and max(curves.nbytes) <= ceiling // 8
    want, lam = alloc.allocate(curves.lengths, curves.sse, budget)
    assert res.nbytes == want and cut.nbytes == want and cut.lam == lam
    ends = sum(r[alloc.lower_hull(r, d)[-1]] for r, d in zip(curves.lengths, curves.sse))
    assert sum(res.nbytes) == min(budget, ends) == len(res.encoded_bytes)
    assert res.max_n == curves.max_n
    # every tile is the oracle's encode of its pixels at its own length; the decode is the paste of the tiles' decodes
    pasted = np.zeros((c, codec.gy * th, codec.gx * tw))
    for i in range(codec.gy):
        for j in range(codec.gx):
            t = res.tile(i, j)
            px = tile_pixels(P, th, tw, i, j)
            px = px / 255.0 if "dtype" in cfg else px
            if cfg.get("color"):  # the oracle has no colour step: it codes the pixels in the device's own IPT
                d = dev(px[None])
                color_models.device_convert(_lib.default_context(), d.ptr, 1, th * tw, "RGB", cfg["color"])
                _lib.default_context().synchronize()
                px = d.download()[0]
            if len(t.encoded_bytes):
                ob, on, _ = oracle.encode_image(px, s.wavelet, s.mode, None, s.quantization_scale, None, 8 * len(t.encoded_bytes))
                assert t.encoded_bytes == ob and t.max_n == on, (i, j)
            pasted[:, i * th:(i + 1) * th, j * tw:(j + 1) * tw] = spiht_amd.decode_image(t, s)[:, :th, :tw]
    dec = codec.decode(res)
    assert np.array_equal(dec, pasted[:, :H, :W])
    assert np.array_equal(codec.decode_window(res, 28, 30, 10, 8), dec[:, 28:38, 30:38])
    assert np.array_equal(spiht_amd.decode_image_tiled(spiht_amd.TiledResult.from_bytes(res.to_bytes()), s), dec)
    # the numbers do not depend on the grouping: one candidate at a time
    codec.max_bytes = 1
    try:
        again = codec.tile_curves(P, cfg.get("dtype"))
    finally:
        codec.max_bytes = 2 ** 31
    assert np.array_equal(again.sse.view(np.uint64), curves.sse.view(np.uint64)) and codec.last_allocation == cut
    # the convenience is the same call
    if "dtype" in cfg:
        conv = spiht_amd.encode_image_tiled_u8(P, cfg["tile"], s, None, cfg["max_bits"], allocate="rd", points=POINTS)
    else:
        conv = spiht_amd.encode_image_tiled(P, cfg["tile"], s, None, cfg["max_bits"], allocate="rd", points=POINTS)
    assert conv == res


def test_curves_are_the_errors_of_the_prefixes():
    """sse[t][k] is the squared error, over the tile's valid region, of decode_image of the first lengths[t][k] bytes"""
    import spiht_amd
    cfg, P, s, codec, res, cut, curves = case("oddtile")
    th, tw = codec.th, codec.tw
    full = codec.codec.encode(np.stack([tile_pixels(P, th, tw, i, j) for i in range(codec.gy) for j in range(codec.gx)]))
    for t in range(codec.T):
        assert len(full[t].encoded_bytes) == curves.nbytes[t] and full[t].max_n == curves.max_n[t]
        vh, vw = valid(cfg["H"], cfg["W"], th, tw, t)
        px = tile_pixels(P, th, tw, *divmod(t, codec.gx))[:, :vh, :vw]
        for k, length in enumerate(curves.lengths[t]):
            pre = spiht_amd.EncodingResult(full[t].encoded_bytes[:length], th, tw, 1, full[t].max_n, None)
            S = float(((px - spiht_amd.decode_image(pre, s)[:, :vh, :vw]) ** 2).sum())
            assert abs(curves.sse[t, k] - S) <= 2 * (vh * vw + 3) * 2.0 ** -52 * S, (t, k)


def test_two_pictures_in_one_call():
    import spiht_amd
    cfg, P, s, codec, res, cut, curves = case("grid3x3")
    Q = synth_image(91, 3, 70, 90)
    many = codec.encode(np.stack([P, Q]))
    cuts = codec.last_allocation
    assert many[0] == res and cuts[0] == cut
    assert many[1] == codec.encode(Q) and cuts[1] == codec.last_allocation
    assert many[1].nbytes != res.nbytes


def sse_of(codec, res, P):
    return float(((codec.decode(res) - P) ** 2).sum())


@pytest.mark.parametrize("which", ["left half constant", "plain"])
def test_allocated_beats_the_equal_split(which):
    """at max_bits 27005 with points 8 (the oracle, fed to the host rule, gave 4.2 dB and 0.6 dB): no margin is needed"""
    import spiht_amd
    if which == "plain":
        P = synth_image(4161, 3, 70, 90)
    else:
        P = synth_image(4161, 1, 70, 90)
        P[:, :, :45] = P[0, 0, 0]
    s = spiht_amd.SpihtSettings()
    rd = spiht_amd.TiledCodec(P.shape[0], 70, 90, 32, s, None, 27005, allocate="rd", points=8)
    eq = spiht_amd.TiledCodec(P.shape[0], 70, 90, 32, s, None, 27005)
    a, b = rd.encode(P), eq.encode(P)
    assert sum(a.nbytes) == 27005 // 8 and sum(b.nbytes) <= 27005 // 8
    sa, sb = sse_of(rd, a, P), sse_of(eq, b, P)
    print("%s: equal split %.2f dB, allocated %.2f dB" % (which, 10 * np.log10(P.size / sb), 10 * np.log10(P.size / sa)))
    assert sa < sb


def test_without_allocate_nothing_changes():
    """allocate=None: points and spread mean nothing, every tile is encode_image of its pixels at max_bits // T"""
    import spiht_amd
    P = synth_image(4163, 3, 70, 90)
    s = spiht_amd.SpihtSettings()
    plain = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, 27005).encode(P)
    codec = spiht_amd.TiledCodec(3, 70, 90, 32, s, None, 27005, allocate=None, points=5, spread=2.0)
    res = codec.encode(P)
    assert res == plain and codec.last_allocation is None
    assert spiht_amd.encode_image_tiled(P, 32, s, None, 27005) == plain
    for i in range(3):
        for j in range(3):
            e = spiht_amd.encode_image(tile_pixels(P, 32, 32, i, j), s, None, 27005 // 9)
            assert res.tile(i, j).encoded_bytes == e.encoded_bytes and res.tile(i, j).max_n == e.max_n
    with pytest.raises(ValueError):
        codec.tile_curves(P)


def test_command_line_allocate(tmp_path):
    import spiht_amd
    from spiht_amd.encode_decode import build_parser, main
    from spiht_amd.utils import imload, imsave
    src = str(tmp_path / "in.png")
    imsave(src, synth_image(6, 3, 70, 90))
    P = imload(src)
    common = [src, "--bpp", "2.0", "--tile", "32", "--color_model", "RGB", "--per_channel_quant_scales", "1.,1.,1.",
              "--out", str(tmp_path / "out.png")]
    enc, dec = main(build_parser().parse_args(common + ["--allocate", "rd", "--points", "8"]))
    s = spiht_amd.SpihtSettings(quantization_scale=255.0, per_channel_quant_scales=[1.0, 1.0, 1.0])
    assert enc == spiht_amd.encode_image_tiled(P, 32, s, 2, round(2.0 * 70 * 90), allocate="rd", points=8)
    assert sum(enc.nbytes) <= round(2.0 * 70 * 90) // 8 and np.array_equal(dec, spiht_amd.decode_image_tiled(enc, s))
    with pytest.raises(SystemExit):
        main(build_parser().parse_args([src, "--allocate", "rd"]))
