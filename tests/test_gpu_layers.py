"""Quality layers of a tiled picture on the GPU: the two copies (spiht_layer_pack, spiht_layer_unpack) against numpy through
the C ABI, and TiledCodec.encode_layered / decode_layered end to end -- every layer's lengths are alloc.allocate of the
measured curves at that layer's budget, all layers together are the TiledResult of encode, every tile of every layer is
still the oracle's encode of the tile's pixels at its own length, and every prefix of the file decodes to the picture of the
clipped lengths."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_image
from tile_helpers import dev, padded

pytestmark = pytest.mark.gpu

vp = C.c_void_p
GUARD = 0xEE


# ---- the two copies against numpy ------------------------------------------------------------------------------------------

def bits_of(nbytes):
    """bit counts whose last byte is not full: ceil(bits / 8) = nbytes"""
    nbytes = np.asarray(nbytes, np.uint64)
    return np.where(nbytes > 0, 8 * nbytes - 3, 0).astype(np.uint64)


def want_pack(slots, bits, N, T, stride):
    """slots [N * T, stride], bits [Q][N * T] -> (cum [N][Q][T], the runs of the N pictures): the kernel's own definition"""
    Q = bits.shape[0]
    B = np.maximum.accumulate(np.minimum((bits + np.uint64(7)) // np.uint64(8), np.uint64(stride)).astype(np.int64), axis=0)
    cum = B.reshape(Q, N, T).transpose(1, 0, 2)
    runs = []
    for n in range(N):
        parts = [slots[n * T + t, (cum[n, q - 1, t] if q else 0):cum[n, q, t]] for q in range(Q) for t in range(T)]
        runs.append(np.concatenate(parts + [np.zeros(0, np.uint8)]))
    return cum, runs


def run_pack(slots, bits, N, T, stride, shift=0, cap=None):
    """-> (cum, pic_bytes, the bytes at the run pointer up to cap); everything around the three outputs must keep its guard"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    Q, NT = bits.shape[0], N * T
    cap = NT * stride if cap is None else cap
    d_slots, d_bits = dev(slots), dev(bits)
    d_packed = dev(np.full(16 + shift + cap + 64, GUARD, np.uint8))
    d_cum, d_pic = dev(np.full(N * Q * T + 2, 0xABABABAB, np.uint32)), dev(np.full(N + 2, 2 ** 64 - 1, np.uint64))
    _lib.check(L.spiht_layer_pack(ctx.handle, vp(d_slots.ptr), stride, vp(d_bits.ptr), Q, N, T, vp(d_packed.ptr + 16 + shift), cap,
                                  vp(d_cum.ptr + 4), vp(d_pic.ptr + 8)))
    ctx.synchronize()
    packed, cum, pic = d_packed.download(), d_cum.download(), d_pic.download()
    assert (packed[:16 + shift] == GUARD).all() and (packed[16 + shift + cap:] == GUARD).all()
    assert cum[0] == cum[-1] == 0xABABABAB and pic[0] == pic[-1] == 2 ** 64 - 1
    return cum[1:-1].reshape(N, Q, T).astype(np.int64), pic[1:-1].astype(np.int64), packed[16 + shift:16 + shift + cap]


def check_pack(slots, bits, N, T, stride, shift=0, cap=None):
    cum, pic, packed = run_pack(slots, bits, N, T, stride, shift, cap)
    wcum, runs = want_pack(slots, bits, N, T, stride)
    run = np.concatenate(runs)
    assert np.array_equal(cum, wcum)
    assert pic.tolist() == [len(r) for r in runs]
    k = min(len(run), len(packed))
    assert np.array_equal(packed[:k], run[:k])
    assert (packed[k:] == GUARD).all()  # nothing behind the run either
    return wcum, runs


def want_unpack(run, layers_bytes, cum, upto, sel, stride):
    """the slots of spiht_layer_unpack: bytes of the run at or past layers_bytes read as zero; a tile is cut at stride"""
    Q, T = cum.shape
    lens = np.diff(cum, axis=0, prepend=0)
    off = (np.cumsum(lens.reshape(-1)) - lens.reshape(-1)).reshape(Q, T)
    src = np.zeros(int(lens.sum()), np.uint8)
    k = min(layers_bytes, len(run), len(src))
    src[:k] = run[:k]
    out = np.zeros((len(sel), stride), np.uint8)
    for s, t in enumerate(sel):
        t = min(max(t, 0), T - 1)
        tile = np.concatenate([src[off[q, t]:off[q, t] + lens[q, t]] for q in range(upto)])[:stride]
        out[s, :len(tile)] = tile
    return out, [min(int(cum[upto - 1, min(max(t, 0), T - 1)]), stride) for t in sel]


def check_unpack(run, cum, upto, sel, stride, layers_bytes=None, shift=0):
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    Q, T = cum.shape
    layers_bytes = len(run) if layers_bytes is None else layers_bytes
    S = T if sel is None else len(sel)
    d_run = dev(np.concatenate([np.full(shift, 0x55, np.uint8), run, np.full(64, 0x55, np.uint8)]))
    d_cum = dev(cum.astype(np.uint32))
    d_sel = None if sel is None else dev(np.asarray(sel, np.int32))
    d_slots, d_nb = dev(np.full(20 + S * stride + 64, GUARD, np.uint8)), dev(np.full(S + 2, 2 ** 64 - 1, np.uint64))
    _lib.check(L.spiht_layer_unpack(ctx.handle, vp(d_run.ptr + shift), layers_bytes, vp(d_cum.ptr), Q, T, upto,
                                    None if sel is None else vp(d_sel.ptr), S, vp(d_slots.ptr + 20), stride, vp(d_nb.ptr + 8)))
    ctx.synchronize()
    got, nb = d_slots.download(), d_nb.download()
    assert (got[:20] == GUARD).all() and (got[20 + S * stride:] == GUARD).all()
    assert nb[0] == nb[-1] == 2 ** 64 - 1
    want, wnb = want_unpack(run, layers_bytes, cum, upto, list(range(T)) if sel is None else sel, stride)
    assert nb[1:-1].tolist() == wnb
    body = got[20:20 + S * stride].reshape(S, stride)
    for s in range(S):
        assert np.array_equal(body[s], want[s]), s
        assert not body[s, wnb[s]:].any(), s  # the tail is zero


# piece lengths [q][t]: 0, 1, 15, 16, 17, 4099, 4100, 16383, 16384, 16385 and 20000 bytes -- a 16-KiB chunk seam inside a
# piece, piece seams inside chunks; the tiles are 36400, 20516, 20485 and 36400 bytes in slots of 40000
LENGTHS = np.array([[1, 16, 4099, 0], [15, 17, 16385, 16383], [16384, 4100, 0, 20000], [20000, 16383, 1, 17]])


def nonzero_slots(seed, NT, stride):
    return np.random.default_rng(seed).integers(1, 256, (NT, stride), dtype=np.uint8)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_pack_and_unpack_piece_lengths(shift):
    """the run pointer 0 .. 3 bytes off a 16-byte boundary; then the run back into slots: all layers and upto < Q, all tiles
    and a selection with repeats, out of order and out of range, a slot shorter than a tile, a run shorter than its table"""
    stride, T, Q = 40000, 4, 4
    slots = nonzero_slots(shift, T, stride)
    bits = bits_of(np.cumsum(LENGTHS, axis=0))
    cum, runs = check_pack(slots, bits, 1, T, stride, shift)
    assert np.array_equal(cum[0], np.cumsum(LENGTHS, axis=0))
    run, cum = runs[0], cum[0]
    check_unpack(run, cum, Q, None, stride, shift=shift)
    check_unpack(run, cum, 2, None, stride)
    check_unpack(run, cum, 3, [3, 0, 3, 1, 1], stride, shift=shift)
    if shift == 0:
        check_unpack(run, cum, Q, [2, -5, 99, 0], stride)  # the kernel clamps: tiles 2, 0, 3, 0
        check_unpack(run, cum, Q, None, 20000)             # tiles 0 and 3 are cut at the slot's end
        check_unpack(run, cum, 1, [1], 4)
        for short in (0, 1, int(LENGTHS[0].sum()), int(LENGTHS[:2].sum()) + 7, len(run) - 20001, len(run) - 1):
            check_unpack(run, cum, Q, [3, 0, 1, 2], stride, layers_bytes=short)  # the bytes behind are there, and not read


def test_pack_capacity_smaller_than_the_run():
    stride, T = 40000, 4
    slots = nonzero_slots(9, T, stride)
    bits = bits_of(np.cumsum(LENGTHS, axis=0))
    total = int(LENGTHS.sum())
    for cap in (0, 1, int(LENGTHS[0].sum()), int(LENGTHS[:2].sum()) + 5000, total - 1, total, total + 3):
        check_pack(slots, bits, 1, T, stride, cap % 4, cap)


@pytest.mark.parametrize("name,N,T,Q,stride", [("Q=1", 1, 3, 1, 4100), ("T=1", 1, 1, 3, 4100), ("Q=255", 1, 3, 255, 1024),
                                               ("N=2", 2, 3, 4, 4100), ("many", 3, 300, 5, 64)])
def test_pack_and_unpack_shapes(name, N, T, Q, stride):
    """Q = 1, T = 1, Q at its limit, two pictures in a call, more pieces than the scan's workgroup takes in a round; random
    nested tables with empty pieces, empty tiles and tiles that fill their slot"""
    rng = np.random.default_rng(Q * T)
    NT = N * T
    lens = rng.integers(0, 2 * stride // Q + 2, (Q, NT))
    lens[rng.random((Q, NT)) < 0.3] = 0
    lens[:, 0] = 0
    nbytes = np.minimum(np.cumsum(lens, axis=0), stride)
    slots = nonzero_slots(NT, NT, stride)
    cum, runs = check_pack(slots, bits_of(nbytes), N, T, stride, 1)
    assert np.array_equal(cum, nbytes.reshape(Q, N, T).transpose(1, 0, 2))
    for n in range(N):
        for upto in sorted({1, (Q + 1) // 2, Q}):
            check_unpack(runs[n], cum[n], upto, None, stride)
    check_unpack(runs[-1], cum[-1], Q, [T - 1, 0, 0], stride, shift=3)


def test_pack_table_that_does_not_nest():
    """rows that fall, and a length past the slot: B(q, t) is the running maximum of min(ceil(bits / 8), slot_stride); the
    unpack takes a falling table the same way"""
    stride, N, T = 4100, 2, 3
    nbytes = np.array([[10, 0, 4100, 7, 300, 0], [4, 50, 9000, 7, 200, 0], [11, 20, 1, 4000, 301, 0], [2 ** 40, 0, 0, 0, 0, 1]])
    slots = nonzero_slots(4, N * T, stride)
    cum, runs = check_pack(slots, bits_of(nbytes), N, T, stride)
    assert cum[0].tolist() == [[10, 0, 4100], [10, 50, 4100], [11, 50, 4100], [4100, 50, 4100]]
    assert cum[1].tolist() == [[7, 300, 0], [7, 300, 0], [4000, 301, 0], [4000, 301, 1]]
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    falling = np.array([[7, 300, 0], [3, 100, 0], [4000, 301, 0], [0, 0, 1]], np.uint32)  # the running maximum is cum[1]
    d_run, d_cum = dev(np.concatenate([runs[1], np.zeros(8, np.uint8)])), dev(falling)
    d_slots, d_nb = dev(np.full(T * stride, GUARD, np.uint8)), dev(np.zeros(T, np.uint64))
    _lib.check(L.spiht_layer_unpack(ctx.handle, vp(d_run.ptr), len(runs[1]), vp(d_cum.ptr), 4, T, 4, None, T, vp(d_slots.ptr), stride,
                                    vp(d_nb.ptr)))
    ctx.synchronize()
    want, wnb = want_unpack(runs[1], len(runs[1]), cum[1], 4, [0, 1, 2], stride)
    assert d_nb.download().tolist() == wnb == [4000, 301, 1]
    assert np.array_equal(d_slots.download().reshape(T, stride), want)
    assert np.array_equal(want[0, :4000], slots[3, :4000])


def test_argument_errors_write_nothing():
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    d = {k: dev(np.full(4096, GUARD, np.uint8)) for k in ("slots", "bits", "packed", "cum", "pic", "sel")}
    ok = dict(slots=d["slots"].ptr, stride=64, bits=d["bits"].ptr, Q=2, N=1, T=3, packed=d["packed"].ptr, cap=4096, cum=d["cum"].ptr,
              pic=d["pic"].ptr)
    bad = [dict(Q=0), dict(Q=256), dict(T=0), dict(N=-1), dict(stride=0), dict(stride=66), dict(slots=None), dict(bits=None),
           dict(packed=None), dict(cum=None), dict(pic=None), dict(bits=d["bits"].ptr + 4), dict(cum=d["cum"].ptr + 2),
           dict(pic=d["pic"].ptr + 4)]
    large = [dict(stride=2 ** 29 + 4), dict(N=2 ** 20, Q=255, T=2 ** 10), dict(N=1, Q=1, T=2 ** 31)]
    for b, err in [(b, _lib.ERR_ARG) for b in bad] + [(b, _lib.ERR_TOO_LARGE) for b in large]:
        a = dict(ok)
        a.update(b)
        assert L.spiht_layer_pack(ctx.handle, vp(a["slots"]), a["stride"], vp(a["bits"]), a["Q"], a["N"], a["T"], vp(a["packed"]),
                                  a["cap"], vp(a["cum"]), vp(a["pic"])) == err, b
    assert L.spiht_layer_pack(None, vp(ok["slots"]), 64, vp(ok["bits"]), 2, 1, 3, vp(ok["packed"]), 4096, vp(ok["cum"]),
                              vp(ok["pic"])) == _lib.ERR_ARG
    ok = dict(layers=d["packed"].ptr, nbytes=100, cum=d["cum"].ptr, Q=2, T=3, upto=2, sel=d["sel"].ptr, S=3, slots=d["slots"].ptr, stride=64,
              out=d["pic"].ptr)
    bad = [dict(Q=0), dict(Q=256), dict(T=0), dict(upto=0), dict(upto=3), dict(S=-1), dict(sel=None, S=4), dict(stride=0), dict(stride=66),
           dict(layers=None), dict(cum=None), dict(slots=None), dict(out=None), dict(cum=d["cum"].ptr + 2), dict(sel=d["sel"].ptr + 2),
           dict(out=d["pic"].ptr + 4)]
    large = [dict(stride=2 ** 29 + 4), dict(Q=255, upto=1, T=2 ** 24)]
    for b, err in [(b, _lib.ERR_ARG) for b in bad] + [(b, _lib.ERR_TOO_LARGE) for b in large]:
        a = dict(ok)
        a.update(b)
        assert L.spiht_layer_unpack(ctx.handle, vp(a["layers"]), a["nbytes"], vp(a["cum"]), a["Q"], a["T"], a["upto"], vp(a["sel"]), a["S"],
                                    vp(a["slots"]), a["stride"], vp(a["out"])) == err, b
    ctx.synchronize()
    for k, buf in d.items():
        assert (buf.download() == GUARD).all(), k


# ---- end to end ---------------------------------------------------------------------------------------------------------------

CASES = {
    "grid3x3": dict(c=3, H=70, W=90, tile=32, max_bits=27005),
    "grey": dict(c=1, H=70, W=90, tile=32, max_bits=27005),
    "oddtile": dict(c=1, H=70, W=90, tile=(33, 40), max_bits=20000),
    "ipt": dict(c=3, H=70, W=90, tile=32, max_bits=27005, color="IPT"),
    "u8": dict(c=3, H=70, W=90, tile=32, max_bits=27005, dtype=np.uint8),
}
POINTS = 8


def layers_of(cfg):
    return [3000, 9000, cfg["max_bits"]]


def picture(cfg):
    P = synth_image(4000 + cfg["H"] + cfg["W"] + cfg["c"], cfg["c"], cfg["H"], cfg["W"])
    if "dtype" in cfg:
        P = np.round(P * 255).astype(cfg["dtype"])
    P.setflags(write=False)
    return P


def hwc(P):
    return np.ascontiguousarray(P.transpose(1, 2, 0))


@functools.lru_cache(maxsize=None)
def case(name):
    """the picture, settings, codec, layered result, its allocations, the plain result and the curves of a case: computed
    once, shared, never changed"""
    import spiht_amd
    cfg = CASES[name]
    P = picture(cfg)
    s = spiht_amd.SpihtSettings(color_model=cfg.get("color"))
    codec = spiht_amd.TiledCodec(cfg["c"], cfg["H"], cfg["W"], cfg["tile"], s, None, cfg["max_bits"], allocate="rd", points=POINTS)
    if "dtype" in cfg:
        res = codec.encode_layered_u8(hwc(P), layers_of(cfg), channels_last=True)
        cuts = codec.last_allocation
        plain = codec.encode_u8(hwc(P), channels_last=True)
    else:
        res = codec.encode_layered(P, layers_of(cfg))
        cuts = codec.last_allocation
        plain = codec.encode(P)
    curves = codec.tile_curves(P, cfg.get("dtype"))
    return cfg, P, s, codec, res, cuts, plain, curves


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end(name):
    import spiht_amd
    from spiht_amd import alloc
    cfg, P, s, codec, res, cuts, plain, curves = case(name)
    budgets = layers_of(cfg)
    Q, T = 3, codec.T
    # every layer's lengths are the rule's at that layer's budget, fed by the curves the device measured
    assert isinstance(res, spiht_amd.LayeredResult) and res.layers == Q and len(cuts) == Q
    for q, b in enumerate(budgets):
        want, lam = alloc.allocate(curves.lengths, curves.sse, b // 8)
        assert res.cum[q] == want, q
        assert cuts[q] == spiht_amd.TileAllocation(lam, want), q
    assert (res.cum, [a.lam for a in cuts]) == alloc.allocate_layers(curves.lengths, curves.sse, [b // 8 for b in budgets])
    assert len(res.encoded_bytes) == sum(res.cum[-1]) and res.max_n == curves.max_n
    # all layers together are the picture of encode, bit for bit
    assert res.tiled() == plain
    # the layered decode of u layers is the decode of the TiledResult of u layers
    for u in (1, 2, 3):
        t = res.tiled(u)
        assert t.nbytes == res.cum[u - 1]
        if "dtype" in cfg:
            assert np.array_equal(codec.decode_layered_u8(res, u, channels_last=True), codec.decode_u8(t, channels_last=True)), u
            assert np.array_equal(codec.decode_layered_window_u8(res, 28, 30, 10, 8, u), codec.decode_window_u8(t, 28, 30, 10, 8)), u
        full = codec.decode(t)
        assert np.array_equal(codec.decode_layered(res, u), full), u
        assert codec.last_tiles_decoded == T
        assert np.array_equal(codec.decode_layered_window(res, 28, 30, 10, 8, u), full[:, 28:38, 30:38]), u  # crosses a tile seam
        i0, i1, j0, j1 = spiht_amd.window_tiles(cfg["H"], cfg["W"], codec.th, codec.tw, 28, 30, 10, 8)
        assert codec.last_tiles_decoded == (i1 - i0) * (j1 - j0) >= 2
    assert np.array_equal(codec.decode_layered(res), codec.decode(plain))
    # the container and the conveniences
    back = spiht_amd.LayeredResult.from_bytes(res.to_bytes())
    assert back == res and np.array_equal(codec.decode_layered(back, 2), codec.decode(res.tiled(2)))
    if "dtype" in cfg:
        conv = spiht_amd.encode_image_layered_u8(P, cfg["tile"], s, None, cfg["max_bits"], budgets, points=POINTS)
        assert np.array_equal(spiht_amd.decode_image_layered_u8(res, s, 2), codec.decode_u8(res.tiled(2)))
        assert np.array_equal(spiht_amd.decode_image_layered_window_u8(res, s, 28, 30, 10, 8, 1), codec.decode_window_u8(res.tiled(1), 28, 30, 10, 8))
    else:
        conv = spiht_amd.encode_image_layered(P, cfg["tile"], s, None, cfg["max_bits"], budgets, points=POINTS)
    assert conv == res
    assert np.array_equal(spiht_amd.decode_image_layered(res, s, 2), codec.decode(res.tiled(2)))
    assert np.array_equal(spiht_amd.decode_image_layered_window(res, s, 28, 30, 10, 8), codec.decode(plain)[:, 28:38, 30:38])
    for bad in (0, 4):
        with pytest.raises(ValueError):
            codec.decode_layered(res, bad)


def test_every_tile_of_every_layer_is_the_oracles_encode(oracle):
    """a tile through layer q is encode_image of the tile's pixels at max_bits = 8 * its length"""
    cfg, P, s, codec, res, cuts, plain, curves = case("grey")
    th, tw = codec.th, codec.tw
    seen = 0
    for u in (1, 2, 3):
        t = res.tiled(u)
        for i in range(codec.gy):
            for j in range(codec.gx):
                e = t.tile(i, j)
                if len(e.encoded_bytes):
                    px = np.ascontiguousarray(padded(P, th, tw)[:, i * th:(i + 1) * th, j * tw:(j + 1) * tw])
                    ob, on, _ = oracle.encode_image(px, s.wavelet, s.mode, None, s.quantization_scale, None, 8 * len(e.encoded_bytes))
                    assert e.encoded_bytes == ob and e.max_n == on, (u, i, j)
                    seen += 1
    assert seen > 2 * codec.T


def test_int_form_of_layers():
    from spiht_amd import alloc
    cfg, P, s, codec, res, cuts, plain, curves = case("grid3x3")
    four = codec.encode_layered(P, 4)
    budgets = alloc.layer_budgets(cfg["max_bits"], 4)
    assert budgets == [3375, 6751, 13502, 27005] and four.layers == 4
    assert four.cum == alloc.allocate_layers(curves.lengths, curves.sse, [b // 8 for b in budgets])[0]
    assert four.tiled() == plain
    assert [a.nbytes for a in codec.last_allocation] == four.cum
    one = codec.encode_layered(P, 1)
    assert one.cum == [plain.nbytes] and one.encoded_bytes == plain.encoded_bytes  # one layer: the runs are the same bytes
    with pytest.raises(ValueError):
        codec.encode_layered(P, [3000, 9000])
    with pytest.raises(TypeError):
        codec.encode_layered(P, 2.0)


def clipped(cum, a):
    """the rule of LayeredResult.from_bytes, piece by piece in file order"""
    cum = np.asarray(cum, dtype=np.int64)
    out, o = np.zeros_like(cum), 0
    for q in range(cum.shape[0]):
        for t in range(cum.shape[1]):
            length = int(cum[q, t] - (cum[q - 1, t] if q else 0))
            out[q, t] = (out[q - 1, t] if q else 0) + min(max(a - o, 0), length)
            o += length
    return out.tolist()


@pytest.mark.parametrize("name", ["grid3x3", "u8"])
def test_prefixes_of_the_file_decode(name):
    """the file cut at every layer's end, a byte either side, at the tables' end and inside a piece: with all Q layers asked
    for, the decode is the picture codec.decode gives for the tiles' streams cut at the clipped lengths"""
    import spiht_amd
    cfg, P, s, codec, res, cuts, plain, curves = case(name)
    blob = res.to_bytes()
    Q, T = 3, codec.T
    head = 28 + 4 * Q * T + T
    ends = res.layer_ends()
    assert ends[-1] == len(blob) and ends == [head + sum(row) for row in res.cum]
    first = next(t for t in range(T) if res.cum[0][t] >= 2)  # the middle of a piece of layer 0
    cuts_at = {head, head + sum(res.cum[0][:first]) + res.cum[0][first] // 2}
    for e in ends:
        cuts_at |= {e - 1, e, e + 1}
    off = np.concatenate(([0], np.cumsum(plain.nbytes)))
    for n in sorted(k for k in cuts_at if head <= k <= len(blob)):
        p = spiht_amd.LayeredResult.from_bytes(blob[:n])
        want = clipped(res.cum, n - head)
        assert p.layers == Q and p.cum == want, n
        cut = spiht_amd.TiledResult(res.h, res.w, res.c, res.th, res.tw, res.level, res.max_n, want[-1],
                                    b"".join(plain.encoded_bytes[off[t]:off[t] + want[-1][t]] for t in range(T)))
        if "dtype" in cfg:
            assert np.array_equal(codec.decode_layered_u8(p), codec.decode_u8(cut)), n
        else:
            assert np.array_equal(codec.decode_layered(p), codec.decode(cut)), n
    with pytest.raises(ValueError):
        spiht_amd.LayeredResult.from_bytes(blob[:head - 1])


# ---- more cases -----------------------------------------------------------------------------------------------------------------

def test_two_pictures_in_one_call():
    cfg, P, s, codec, res, cuts, plain, curves = case("grid3x3")
    Q2 = synth_image(91, 3, 70, 90)
    many = codec.encode_layered(np.stack([P, Q2]), layers_of(cfg))
    both = codec.last_allocation
    assert many[0] == res and both[0] == cuts
    assert many[1] == codec.encode_layered(Q2, layers_of(cfg)) and both[1] == codec.last_allocation
    assert many[1].cum != res.cum and many[1].tiled() == codec.encode(Q2)


def test_device_form_selects_tiles_of_the_whole_run():
    """decode_layers_device with d_sel: the whole picture's run and table stay on the device, a window names its tiles"""
    from spiht_amd import _lib, window_tiles
    from spiht_amd.batch import DeviceArray
    cfg, P, s, codec, res, cuts, plain, curves = case("grid3x3")
    window = (28, 30, 10, 8)
    i0, i1, j0, j1 = sub = window_tiles(cfg["H"], cfg["W"], codec.th, codec.tw, *window)
    ts = [i * codec.gx + j for i in range(i0, i1) for j in range(j0, j1)]
    d_run = dev(np.frombuffer(res.encoded_bytes + b"\x00" * 4, np.uint8))
    d_cum, d_sel = dev(np.asarray(res.cum, np.uint32)), dev(np.asarray(ts, np.int32))
    d_maxn = dev(np.asarray([res.max_n[t] for t in ts], np.uint8))
    d_out = DeviceArray(_lib.default_context(), (cfg["c"], window[2], window[3]), np.float64)
    for upto in (1, 3):
        stride = (max(res.cum[upto - 1]) + 3) & ~3
        codec.decode_layers_device(d_run, len(res.encoded_bytes), d_cum, d_maxn, 3, upto, sub, window, d_out, None, stride, d_sel)
        codec.ctx.synchronize()
        assert np.array_equal(d_out.download(), codec.decode_layered_window(res, *window, upto)), upto


def test_a_codec_without_allocate_is_refused():
    import spiht_amd
    P = synth_image(4163, 3, 70, 90)
    codec = spiht_amd.TiledCodec(3, 70, 90, 32, spiht_amd.SpihtSettings(), None, 27005)
    with pytest.raises(ValueError):
        codec.encode_layered(P, 2)
    with pytest.raises(ValueError):
        codec.encode_layered_u8(np.zeros((3, 70, 90), np.uint8), 2)
    d = dev(P)
    with pytest.raises(ValueError):
        codec.encode_layered_device(d, 1, 2, d, d, d, d)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_layered(P, 32, spiht_amd.SpihtSettings(), None, None, 2)  # a budget is required


def test_layered_calls_leave_nothing_behind(oracle):
    """after a layered encode and decode (colour model included) on a context, the ordinary calls on it still equal the
    oracle: the context's coefficient array is left zero"""
    import spiht_amd
    for name in ("ipt", "grid3x3"):
        cfg, P, s, codec, res, cuts, plain, curves = case(name)
        codec.decode_layered_window(codec.encode_layered(P, layers_of(cfg)), 28, 30, 10, 8, 2)
        img = synth_image(1000, 3, 96, 160)
        std = spiht_amd.SpihtSettings()
        enc = spiht_amd.encode_image(img, std, level=3, max_bits=7680)
        ob, on, _ = oracle.encode_image(img, "bior2.2", "reflect", 3, 50.0, None, 7680)
        assert enc.encoded_bytes == ob and enc.max_n == on
        assert np.array_equal(spiht_amd.decode_image(enc, std), oracle.decode_image(ob, on, 3, 96, 160, "bior2.2", 3, 50.0, None))


def test_command_line_layers(tmp_path, capsys):
    import spiht_amd
    from spiht_amd.encode_decode import build_parser, main
    from spiht_amd.utils import imload, imsave
    src = str(tmp_path / "in.png")
    imsave(src, synth_image(6, 3, 70, 90))
    P = imload(src)
    common = [src, "--bpp", "2.0", "--tile", "32", "--color_model", "RGB", "--per_channel_quant_scales", "1.,1.,1.",
              "--out", str(tmp_path / "out.png")]
    s = spiht_amd.SpihtSettings(quantization_scale=255.0, per_channel_quant_scales=[1.0, 1.0, 1.0])
    enc, dec = main(build_parser().parse_args(common + ["--allocate", "rd", "--points", "8", "--layers", "3"]))
    assert enc == spiht_amd.encode_image_layered(P, 32, s, 2, round(2.0 * 70 * 90), 3, points=8)
    assert enc.layers == 3 and np.array_equal(dec, spiht_amd.decode_image_layered(enc, s))
    out = capsys.readouterr().out
    for q, end in enumerate(enc.layer_ends()):
        assert any(line.split()[:2] == [str(q), str(end)] for line in out.splitlines()), (q, out)
    enc2, _ = main(build_parser().parse_args(common + ["--allocate", "rd", "--points", "8", "--layers", "3150,6300,12600"]))
    assert enc2.layers == 3 and enc2.tiled() == enc.tiled()
    with pytest.raises(SystemExit):
        main(build_parser().parse_args(common + ["--layers", "3"]))
    with pytest.raises(SystemExit):
        main(build_parser().parse_args([src, "--layers", "3"]))
