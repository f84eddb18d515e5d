"""GPU tests of the picture sets (spiht_amd/tileset.py, csrc/tileset.hip): TileSetCodec against the per-picture path -- a
TiledCodec of each size, which test_gpu_tiles.py holds to the oracle -- in every field and byte; the two C calls alone against
cut_rule / paste_rule; two calls queued without a synchronise between them; and the status codes of spoiled tables."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_image
from tile_helpers import dev, tile_of, tile_pixels

pytestmark = pytest.mark.gpu

vp = C.c_void_p
LEVEL, TILE_BITS = 2, 3001  # (a budget that is no multiple of 8)
#         A: 2 x 2, padded  B: one tile  C: smaller than a tile  D: 3 x 1, one valid row  E: 1 x 4, one valid column
SIZES = [(20, 27), (16, 16), (5, 7), (33, 16), (16, 49)]
CONFIGS = {"rgb16": (3, 16), "grey16x24": (1, (16, 24))}
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def same_tiled(a, b):
    assert (a.h, a.w, a.c, a.th, a.tw, a.level, a.max_n, a.nbytes, a.encoded_bytes, a._encoding_version) == \
        (b.h, b.w, b.c, b.th, b.tw, b.level, b.max_n, b.nbytes, b.encoded_bytes, b._encoding_version)


def tiles_of(H, W, tile):
    th, tw = tile_of(tile)
    return -(-H // th) * -(-W // tw)


@functools.lru_cache(maxsize=None)
def case(name):
    """the set, its codec, and the yardstick: a TiledCodec per picture with its float64 result and decode"""
    import spiht_amd
    c, tile = CONFIGS[name]
    pics = [synth_image(7000 + 10 * k + c, c, H, W) for k, (H, W) in enumerate(SIZES)]
    for P in pics:
        P.setflags(write=False)
    codec = spiht_amd.TileSetCodec(c, tile, None, LEVEL, TILE_BITS)
    per = [spiht_amd.TiledCodec(c, H, W, tile, None, LEVEL, TILE_BITS * tiles_of(H, W, tile)) for H, W in SIZES]
    res = [k.encode(P) for k, P in zip(per, pics)]
    dec = [k.decode(r) for k, r in zip(per, res)]
    return c, tile_of(tile), pics, codec, per, res, dec


def test_the_set_is_thirteen_tiles_and_picture_a_is_the_oracle_s(oracle):
    import spiht_amd
    c, (th, tw), pics, codec, per, res, dec = case("rgb16")
    assert sum(len(r.nbytes) for r in res) == 13
    got = codec.encode(pics)
    A, s = got[0], spiht_amd.SpihtSettings()
    assert (A.h, A.w, A.c, A.th, A.tw, A.level) == (20, 27, 3, 16, 16, LEVEL) and len(A.nbytes) == 4
    for i in range(2):
        for j in range(2):
            t = A.tile(i, j)
            ob, on, _ = oracle.encode_image(tile_pixels(pics[0], th, tw, i, j), s.wavelet, s.mode, LEVEL, s.quantization_scale, None,
                                            TILE_BITS)
            assert t.encoded_bytes == ob and t.max_n == on, (i, j)


ENCODES = ["f64", "u8", "u8_hwc", "u16", "float32", "float16", "bfloat16"]


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("form", ENCODES)
def test_encode_equals_the_per_picture_codecs(name, form):
    from spiht_amd import floatpx
    c, tile, pics, codec, per, res, dec = case(name)
    if form == "f64":
        args, kw, fn = pics, {}, "encode"
    elif form in ("u8", "u8_hwc", "u16"):
        dt = np.uint16 if form == "u16" else np.uint8
        args = [np.round(P * np.iinfo(dt).max).astype(dt) for P in pics]
        kw, fn = {}, "encode_" + form[:3].rstrip("_")
        if form == "u8_hwc":
            args, kw = [np.ascontiguousarray(P.transpose(1, 2, 0)) for P in args], dict(channels_last=True)
    else:
        args, kw, fn = [floatpx.convert(P, form) for P in pics], dict(dtype=form), "encode_float"
    want = [getattr(k, fn)(P, **kw) for k, P in zip(per, args)]
    if form in ("f64", "u8", "u8_hwc"):  # (the same picture in every pixel form that holds it exactly)
        for w, r in zip(want, res):
            same_tiled(w, r)
    got = getattr(codec, fn)(args, **kw)
    assert len(got) == len(SIZES)
    for g, w in zip(got, want):
        same_tiled(g, w)
    # the order of the set and its size change nothing of a picture
    for g, w in zip(getattr(codec, fn)(args[::-1], **kw), want[::-1]):
        same_tiled(g, w)
    for P, w in zip(args, want):
        g, = getattr(codec, fn)([P], **kw)
        same_tiled(g, w)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_decode_equals_the_per_picture_codecs(name):
    from spiht_amd import TiledResult
    c, tile, pics, codec, per, res, dec = case(name)
    total = sum(len(r.nbytes) for r in res)
    got = codec.decode(res)
    assert codec.last_tiles_decoded == total and len(got) == len(res)
    for g, d, (H, W) in zip(got, dec, SIZES):
        assert g.shape == (c, H, W) and g.dtype == np.float64 and np.array_equal(g, d)
    got = codec.decode_u8(res, channels_last=True)
    for g, k, r, (H, W) in zip(got, per, res, SIZES):
        assert g.shape == (H, W, c) and g.dtype == np.uint8 and np.array_equal(g, k.decode_u8(r, channels_last=True))
    got = codec.decode_float(res, np.float16)
    for g, k, r in zip(got, per, res):
        w = k.decode_float(r, np.float16)
        assert g.dtype == np.float16 and np.array_equal(g.view(np.uint16), w.view(np.uint16))
    assert codec.last_tiles_decoded == total
    # results that went through the container, in another order
    back = [TiledResult.from_bytes(r.to_bytes()) for r in res[::-1]]
    for g, d in zip(codec.decode(back), dec[::-1]):
        assert np.array_equal(g, d)


CROPS = [(0, (0, 0)), (0, (9, 14)), (3, (22, 3)), (4, (5, 36))]  # A twice; four tiles to A's last sample; the single valid row, column


@pytest.mark.parametrize("name", list(CONFIGS))
def test_windows_and_crops_equal_decode_window(name):
    from spiht_amd import window_tiles
    c, (th, tw), pics, codec, per, res, dec = case(name)
    for size, crops in (((11, 13), CROPS), ((4, 5), CROPS + [(2, (1, 2))])):
        h, w = size
        rs, origins = [res[p] for p, _ in crops], [o for _, o in crops]
        count = 0
        for p, (y0, x0) in crops:
            i0, i1, j0, j1 = window_tiles(*SIZES[p], th, tw, y0, x0, h, w)
            count += (i1 - i0) * (j1 - j0)
        if name == "rgb16" and size == (11, 13):
            assert count == 1 + 4 + 2 + 2
        got = codec.decode_crops(rs, origins, size)
        assert got.shape == (len(crops), c, h, w) and got.dtype == np.float64 and codec.last_tiles_decoded == count
        got8 = codec.decode_crops_u8(rs, origins, size)  # (rows of 13 bytes: every row starts unaligned for the 16-byte stores)
        assert got8.shape == (len(crops), c, h, w) and got8.dtype == np.uint8 and codec.last_tiles_decoded == count
        got8l = codec.decode_crops_u8(rs, origins, size, channels_last=True)
        assert got8l.shape == (len(crops), h, w, c)
        got16 = codec.decode_crops_float(rs, origins, size, np.float16)
        wins = codec.decode_windows(rs, [(y0, x0, h, w) for y0, x0 in origins])
        for b, (p, (y0, x0)) in enumerate(crops):
            assert np.array_equal(got[b], per[p].decode_window(res[p], y0, x0, h, w)), (size, b)
            assert np.array_equal(got[b], dec[p][:, y0:y0 + h, x0:x0 + w])
            assert np.array_equal(wins[b], got[b])
            want8 = per[p].decode_window_u8(res[p], y0, x0, h, w)
            assert np.array_equal(got8[b], want8) and np.array_equal(got8l[b], want8.transpose(1, 2, 0))
            assert np.array_equal(got16[b].view(np.uint16), per[p].decode_window_float(res[p], y0, x0, h, w, np.float16).view(np.uint16))
    with pytest.raises(ValueError):
        codec.decode_crops([res[0], res[2]], [(0, 0), (0, 0)], (11, 13))
    # windows of different sizes, None among them
    windows = [(3, 5, 17, 20), None, (4, 0, 1, 7), (32, 0, 1, 16), None]
    got = codec.decode_windows_u16(res, windows, channels_last=True)
    count = 0
    for g, k, r, win, (H, W) in zip(got, per, res, windows, SIZES):
        y0, x0, h, w = (0, 0, H, W) if win is None else win
        i0, i1, j0, j1 = window_tiles(H, W, th, tw, y0, x0, h, w)
        count += (i1 - i0) * (j1 - j0)
        assert np.array_equal(g, k.decode_window_u16(r, y0, x0, h, w, channels_last=True))
    assert codec.last_tiles_decoded == count


def gathered(results, windows, th, tw):
    """what decode_windows_device takes of host results: the run, the lengths and the start planes of the gathered tiles, and
    the items"""
    from spiht_amd import set_tables
    t = set_tables([(r.h, r.w) for r in results], th, tw, list(enumerate(windows)))
    run, lens, maxn = [], [], []
    for b, r in enumerate(results):
        off = np.concatenate(([0], np.cumsum(r.nbytes)))
        for k in t["gather"][int(t["s0"][b]):int(t["s0"][b + 1])]:
            run.append(r.encoded_bytes[int(off[k]):int(off[k + 1])])
            lens.append(r.nbytes[k])
            maxn.append(r.max_n[k])
    run = np.frombuffer(b"".join(run), np.uint8)
    return run, np.asarray(lens, np.uint32), np.asarray(maxn, np.uint8), list(zip(t["subs"], t["windows"]))


def test_a_channels_last_crop_batch_inside_a_larger_buffer():
    """uint8 crops written as the [..., :3] samples of the inner h x w of a [B, h + 2, w + 3, 4] buffer: no other byte changes"""
    from spiht_amd import _lib
    c, (th, tw), pics, codec, per, res, dec = case("rgb16")
    h, w = 11, 13
    rs = [res[p] for p, _ in CROPS]
    run, lens, maxn, items = gathered(rs, [(y0, x0, h, w) for _, (y0, x0) in CROPS], th, tw)
    want = np.full((len(CROPS), h + 2, w + 3, 4), 0xA5, np.uint8)
    for b, (p, (y0, x0)) in enumerate(CROPS):
        want[b, 1:1 + h, 2:2 + w, :3] = per[p].decode_window_u8(res[p], y0, x0, h, w, channels_last=True)
    d_buf = dev(np.full(want.shape, 0xA5, np.uint8))
    row, pic = (w + 3) * 4, (h + 2) * (w + 3) * 4
    outs = [(d_buf.ptr + b * pic + row + 8, r.h, r.w, (1, row, 4)) for b, r in enumerate(rs)]
    d_run, d_lens, d_maxn = dev(run), dev(lens), dev(maxn)
    n = codec.decode_windows_device(d_run, len(run), d_lens, d_maxn, items, outs, np.uint8)
    _lib.default_context().synchronize()
    assert n == len(lens) == codec.last_tiles_decoded
    assert np.array_equal(d_buf.download(), want)


# ---- the two C calls alone ---------------------------------------------------------------------------------------------------
def rand_array(rng, shape, es):
    return rng.integers(1, 250, shape).astype(DTYPES[es]) * DTYPES[es](0x0101010101010101 & (2 ** (8 * es) - 1))


def cut_set(es, c, th, tw, rows, d_tiles):
    """rows: (address, (sc, sh, sw), H, W) -> the status of spiht_tile_cut_set"""
    from spiht_amd import _lib
    tab = (_lib.TileSetPic * len(rows))()
    for r, (addr, st, H, W) in zip(tab, rows):
        r.d_img, (r.sc, r.sh, r.sw), r.H, r.W = addr, st, H, W
    return _lib.lib().spiht_tile_cut_set(_lib.default_context().handle, es, len(rows), c, th, tw, C.byref(tab), vp(d_tiles))


def paste_set(es, c, rh, rw, th, tw, rows, d_tiles, S):
    """rows: (address, (sc, sh, sw), H, W, sub, window) -> the status of spiht_tile_paste_set"""
    from spiht_amd import _lib
    tab = (_lib.TileSetItem * len(rows))()
    for r, (addr, st, H, W, sub, win) in zip(tab, rows):
        r.d_out, (r.sc, r.sh, r.sw), r.H, r.W = addr, st, H, W
        (r.i0, r.i1, r.j0, r.j1), (r.y0, r.x0, r.wh, r.ww) = sub, win
    return _lib.lib().spiht_tile_paste_set(_lib.default_context().handle, es, len(rows), c, rh, rw, th, tw, C.byref(tab),
                                           vp(d_tiles), S)


def cut_problem(es, c=3, seed=0):
    """the set as arrays of es-byte elements in ONE host buffer: picture A as the [..., :3] view of a four-sample buffer, the
    others dense CHW one behind the other (so at unaligned addresses) -> (pictures, the buffer, rows relative to its start)"""
    rng = np.random.default_rng(100 + es + seed)
    pics = [rand_array(rng, (c, H, W), es) for H, W in SIZES]
    parts, rows, off = [], [], 0
    for k, (P, (H, W)) in enumerate(zip(pics, SIZES)):
        if k == 0:
            a = np.zeros((H, W, 4), P.dtype)
            a[..., :c] = P.transpose(1, 2, 0)
            st = (es, W * 4 * es, 4 * es)
        else:
            a, st = P, (H * W * es, W * es, es)
        rows.append((off, st, H, W))
        parts.append(a.reshape(-1).view(np.uint8))
        off += a.nbytes
    return pics, np.concatenate(parts), rows


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_cut_set_alone(es):
    from spiht_amd import _lib, cut_rule
    ctx = _lib.default_context()
    for c, th, tw in ((3, 16, 16), (1, 16, 24), (2, 8, 40)):
        pics, buf, rows = cut_problem(es, c)
        want = cut_rule(pics, th, tw)
        d_in = dev(buf)
        guard = np.full(want.nbytes + 64 + 32, 0xEE, np.uint8)
        d_tiles = dev(guard)
        assert cut_set(es, c, th, tw, [(d_in.ptr + o, st, H, W) for o, st, H, W in rows], d_tiles.ptr + 32) == _lib.OK
        ctx.synchronize()
        got = d_tiles.download()
        assert (got[:32] == 0xEE).all() and (got[32 + want.nbytes:] == 0xEE).all()
        assert np.array_equal(got[32:32 + want.nbytes].view(want.dtype).reshape(want.shape), want), (c, th, tw)


def paste_problem(es, c, th, tw, rh, rw, seed=0):
    """windows of the set's pictures, one per kind, into ONE buffer pre-filled with 0xA5: dense CHW windows with 5 + es guard
    bytes between them, the second one as the [..., :c] samples of a four-sample buffer -> (tiles, rows relative to the
    buffer's start, S, the buffer as it must be afterwards)"""
    from spiht_amd import paste_rule, set_tables
    rng = np.random.default_rng(200 + es + seed)
    items = [(0, (9, 14, 11, 13)), (0, None), (2, (1, 2, 4, 5)), (3, (22, 3, 11, 13)), (4, (5, 36, 11, 13)), (1, None), (4, (0, 47, 16, 2))]
    t = set_tables(SIZES, th, tw, items)
    S = int(t["s0"][-1])
    tiles = rand_array(rng, (S, c, rh, rw), es)
    wins = paste_rule(tiles, list(zip(t["subs"], t["windows"])), th, tw)
    rows, parts, off = [], [], es
    parts.append(np.full(es, 0xA5, np.uint8))
    for b, ((p, _), sub, win, wdw) in enumerate(zip(items, t["subs"], t["windows"], wins)):
        _, _, h, w = win
        if b == 1:
            a = np.full((h, w, 4), 0xA5A5A5A5A5A5A5A5 & (2 ** (8 * es) - 1), tiles.dtype)
            a[..., :c] = wdw.transpose(1, 2, 0)
            st = (es, w * 4 * es, 4 * es)
        else:
            a, st = wdw, (h * w * es, w * es, es)
        rows.append((off, st, SIZES[p][0], SIZES[p][1], sub, win))
        parts += [np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.full(5 * es, 0xA5, np.uint8)]
        off += a.nbytes + 5 * es
    return tiles, rows, S, np.concatenate(parts)


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_paste_set_alone(es):
    from spiht_amd import _lib
    ctx = _lib.default_context()
    for c, th, tw, rh, rw in ((3, 16, 16, 17, 19), (1, 16, 24, 16, 24)):
        tiles, rows, S, want = paste_problem(es, c, th, tw, rh, rw)
        d_tiles, d_out = dev(tiles), dev(np.full(want.shape, 0xA5, np.uint8))
        assert paste_set(es, c, rh, rw, th, tw, [(d_out.ptr + r[0],) + tuple(r[1:]) for r in rows], d_tiles.ptr, S) == _lib.OK
        ctx.synchronize()
        assert np.array_equal(d_out.download(), want), (c, th, tw)


# ---- two calls queued without a synchronise between them ----------------------------------------------------------------------
SIZES2 = [(24, 40), (9, 9), (40, 17)]


def test_two_encodes_queued_back_to_back_each_see_their_own_tables():
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    c, (th, tw), pics, codec, per, res, dec = case("rgb16")
    ctx = _lib.default_context()
    set1 = [np.round(P * 255).astype(np.uint8) for P in pics]
    set2 = [np.round(synth_image(7100 + k, c, H, W) * 255).astype(np.uint8) for k, (H, W) in enumerate(SIZES2)]
    want = [codec.encode_u8(set1), codec.encode_u8(set2)]  # (each alone; the scratch has its largest size from here on)
    jobs = []
    for pset in (set1, set2):
        NT = sum(tiles_of(P.shape[1], P.shape[2], (th, tw)) for P in pset)
        d_pics = [dev(P) for P in pset]
        out = (DeviceArray(ctx, (NT * codec.codec.slot_stride,), np.uint8), DeviceArray(ctx, (NT,), np.uint32), DeviceArray(ctx, (NT,), np.uint8))
        jobs.append((d_pics, [(d.ptr, P.shape[1], P.shape[2], None) for d, P in zip(d_pics, pset)], out, NT))
    ctx.synchronize()
    for _, rows, out, NT in jobs:  # queued back to back
        assert codec.encode_device(rows, *out, np.uint8) == NT
    ctx.synchronize()
    for (_, _, (d_packed, d_lens, d_maxn), NT), results in zip(jobs, want):
        lens, maxn, run = d_lens.download(), d_maxn.download(), d_packed.download()
        assert [int(v) for v in lens] == [n for r in results for n in r.nbytes]
        assert [int(v) for v in maxn] == [n for r in results for n in r.max_n]
        assert run[:int(lens.sum())].tobytes() == b"".join(r.encoded_bytes for r in results)


def test_two_decodes_queued_back_to_back_each_see_their_own_tables():
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    c, (th, tw), pics, codec, per, res, dec = case("rgb16")
    ctx = _lib.default_context()
    res2 = codec.encode_u8([np.round(synth_image(7100 + k, c, H, W) * 255).astype(np.uint8) for k, (H, W) in enumerate(SIZES2)])
    calls = [(res, [None, None, (1, 2, 4, 5), (22, 3, 11, 13), (5, 36, 11, 13)]), (res2, [(3, 7, 20, 30), None, (39, 0, 1, 17)])]
    want = [codec.decode_windows_u8(rs, wins) for rs, wins in calls]  # (each alone)
    jobs = []
    for (rs, wins), ws in zip(calls, want):
        run, lens, maxn, items = gathered(rs, wins, th, tw)
        outs = [DeviceArray(ctx, w.shape, np.uint8) for w in ws]
        jobs.append((dev(run), len(run), dev(lens), dev(maxn), items, outs, [(o.ptr, r.h, r.w, None) for o, r in zip(outs, rs)]))
    ctx.synchronize()
    for d_run, nb, d_lens, d_maxn, items, outs, rows in jobs:  # queued back to back
        codec.decode_windows_device(d_run, nb, d_lens, d_maxn, items, rows, np.uint8)
    ctx.synchronize()
    for job, ws in zip(jobs, want):
        for o, w in zip(job[5], ws):
            assert np.array_equal(o.download(), w)


# ---- status codes ------------------------------------------------------------------------------------------------------------
def test_spoiled_tables_are_refused_before_anything_is_queued():
    from spiht_amd import _lib, cut_rule
    ctx = _lib.default_context()
    es, c, th, tw = 2, 3, 16, 16
    # the cut
    pics, buf, rows = cut_problem(es, c, seed=5)
    want = cut_rule(pics, th, tw)
    d_in = dev(buf)
    rows = [(d_in.ptr + o, st, H, W) for o, st, H, W in rows]
    d_tiles = dev(np.full(want.nbytes, 0xA5, np.uint8))

    def cut_ok():
        assert cut_set(es, c, th, tw, rows, d_tiles.ptr) == _lib.OK
        ctx.synchronize()
        assert np.array_equal(d_tiles.download().view(want.dtype).reshape(want.shape), want)
        d_tiles.upload(np.full(want.nbytes, 0xA5, np.uint8))

    def spoil(rows, k, **kw):
        names = ("addr", "st", "H", "W", "sub", "win")
        r = dict(zip(names, rows[k]))
        r.update(kw)
        return rows[:k] + [tuple(r[n] for n in names[:len(rows[k])])] + rows[k + 1:]

    cut_ok()
    a, st, H, W = rows[3]
    spoils = [(es, c, th, tw, spoil(rows, 3, H=0), _lib.ERR_ARG), (es, c, 7, tw, rows, _lib.ERR_ARG), (es, c, th, 7, rows, _lib.ERR_ARG),
              (es, c, th, tw, spoil(rows, 3, st=(st[0], st[1] + 1, st[2])), _lib.ERR_ARG),
              (es, c, th, tw, spoil(rows, 4, addr=rows[4][0] + 1), _lib.ERR_ARG),
              (es, c, th, tw, spoil(rows, 2, st=(st[0], -2, st[2])), _lib.ERR_ARG),
              (es, c, th, tw, spoil(rows, 1, addr=None), _lib.ERR_ARG), (3, c, th, tw, rows, _lib.ERR_ARG),
              (es, c, th, tw, [], _lib.ERR_ARG), (es, 65536, th, tw, rows, _lib.ERR_TOO_LARGE),
              (es, c, th, tw, spoil(rows, 4, H=1 << 30), _lib.ERR_TOO_LARGE)]
    for e, cc, a_th, a_tw, rr, status in spoils:
        assert cut_set(e, cc, a_th, a_tw, rr, d_tiles.ptr) == status
        ctx.synchronize()
        assert (d_tiles.download() == 0xA5).all()  # nothing was queued
        cut_ok()                                   # ... and the context is usable
    # the paste
    rh, rw = 17, 19
    tiles, prow, S, pwant = paste_problem(es, c, th, tw, rh, rw, seed=5)
    d_src, d_out = dev(tiles), dev(np.full(pwant.shape, 0xA5, np.uint8))
    prow = [(d_out.ptr + r[0],) + tuple(r[1:]) for r in prow]

    def paste_ok():
        assert paste_set(es, c, rh, rw, th, tw, prow, d_src.ptr, S) == _lib.OK
        ctx.synchronize()
        assert np.array_equal(d_out.download(), pwant)
        d_out.upload(np.full(pwant.shape, 0xA5, np.uint8))

    paste_ok()
    a, st, H, W, sub, win = prow[3]  # D: (22, 3, 11, 13) of 33 x 16, rows 1 .. 2 of a 3 x 1 grid
    assert (H, W, sub, win) == (33, 16, (1, 3, 0, 1), (22, 3, 11, 13))
    spoils = [dict(rows=spoil(prow, 3, win=(23, 3, 11, 13))),          # a window one sample past the picture
              dict(rows=spoil(prow, 3, win=(22, 4, 11, 13))),
              dict(rows=spoil(prow, 3, sub=(2, 3, 0, 1)), S=S - 1),    # a sub-grid missing a tile its window meets
              dict(rows=spoil(prow, 3, st=(st[0], st[1] + 1, st[2]))),  # an odd stride for es = 2
              dict(S=S + 1), dict(S=S - 1),                            # S not the sum of the sub-grids
              dict(rows=spoil(prow, 3, H=0)), dict(th=7), dict(tw=7),
              dict(rows=spoil(prow, 0, st=(0, prow[0][1][1], prow[0][1][2]))),  # a view that is written over itself
              dict(rh=th - 1), dict(rows=spoil(prow, 5, addr=None)), dict(rows=[]),
              dict(c=65536, status=_lib.ERR_TOO_LARGE)]
    for sp in spoils:
        status = sp.pop("status", _lib.ERR_ARG)
        kw = dict(es=es, c=c, rh=rh, rw=rw, th=th, tw=tw, rows=prow, d_tiles=d_src.ptr, S=S)
        kw.update(sp)
        assert paste_set(**kw) == status, sp
        ctx.synchronize()
        assert (d_out.download() == 0xA5).all()
        paste_ok()
