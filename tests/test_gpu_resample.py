"""GPU tests of the resized crops (spiht_amd/resample.py, csrc/resample.hip): spiht_tile_resample_set alone on tile batches made
here, against resize_rule of paste_rule's window, bit for bit in every kind and layout with sentinels around and between the
samples; its argument errors; and TileSetCodec.decode_resized_crops* against resize_rule of TiledCodec.decode_window."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_image
from tile_helpers import dev

pytestmark = pytest.mark.gpu

vp = C.c_void_p
KINDS = ["f64", "u8", "u16", "float32", "float16", "bfloat16"]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def elem(kind):
    from spiht_amd import px
    return {"f64": px.F64, "u8": px.U8, "u16": px.U16}.get(kind) or px.of_kind_id(kind)


# ---- the kernel alone -----------------------------------------------------------------------------------------------------
# (c, th, tw, rh, rw): decoded tiles are larger than the tile on both axes
CONFIGS = {"8x8": (3, 8, 8, 11, 10), "16x24": (2, 16, 24, 17, 29)}


def launches(th, tw):
    """(size, [(picture, box, flip)]) per launch; picture 0 is a 3 x 4 grid with a ragged last row, picture 1 one wide strip"""
    sizes = [(3 * th - 2, 4 * tw), (16, 203)]
    H, W = sizes[0]
    return sizes, [
        ((1, 1), [(0, (5, 6, 1, 1), False), (0, (1, 1, 5, 6), True), (0, (th - 3, tw - 2, 9, 7), False)]),
        ((11, 13), [(0, (th - 5, tw - 6, 11, 13), False), (0, (0, 0, 11, 13), True), (0, (H - 11, W - 13, 11, 13), True)]),
        # upscaled: a seam across the rows only, across the columns only, one tile, one row, one column, one sample
        ((20, 31), [(0, (th - 2, 1, 5, 7), False), (0, (1, tw - 3, 5, 7), True), (0, (0, 0, 5, 7), False),
                    (0, (4, 2, 1, 2 * tw + 1), True), (0, (2, 4, 2 * th + 1, 1), False), (0, (H - 1, W - 1, 1, 1), True)]),
        ((1, 2), [(0, (3, 1, 16, 9), True), (0, (0, W - 32, 16, 32), False)]),           # a ratio of exactly 16, on each axis
        ((3, 6), [(0, (0, 0, H, W), False), (0, (0, 0, H, W), True), (1, (0, 3, 16, 96), True)]),  # the whole 3 x 4 grid
        ((13, 13), [(1, (2, 3, 13, 200), False), (1, (0, 0, 13, 200), True)]),
    ]


def tables_of(boxes, size, flips):
    """the tables of a call as spiht_tile_resample_set takes them, every item with its own: (int64 [B, 4], the blob)"""
    from spiht_amd import resample
    oh, ow = size
    parts, tabs, off = [], [], 0
    for (_, _, h, w), flip in zip(boxes, flips):
        row = []
        for n_in, n_out, f in ((w, ow, flip), (h, oh, False)):
            t = resample.axis_table(n_in, n_out)
            start, count, wt = resample.flip_table(t) if f else t
            row += [off, wt.shape[1]]
            parts += [start.view(np.uint8), count.view(np.uint8), wt.reshape(-1).view(np.uint8)]
            off += 8 * n_out + wt.nbytes
        tabs.append(row)
    return np.asarray(tabs, np.int64), np.concatenate(parts)


def resample_set(kind, c, rh, rw, th, tw, size, rows, tabs, tables, d_tiles, S, mean=None, std=None, B=None):
    """rows: (address, (sc, sh, sw), H, W, sub, box) -> the status of spiht_tile_resample_set"""
    from spiht_amd import _lib
    tab = (_lib.TileSetItem * max(len(rows), 1))()
    for r, (addr, st, H, W, sub, box) in zip(tab, rows):
        r.d_out, (r.sc, r.sh, r.sw), r.H, r.W = addr, st, H, W
        (r.i0, r.i1, r.j0, r.j1), (r.y0, r.x0, r.wh, r.ww) = sub, box
    m = None if mean is None else np.asarray(mean, np.float64)
    s = None if std is None else np.asarray(std, np.float64)
    tabs, tables = np.ascontiguousarray(tabs), np.ascontiguousarray(tables)
    return _lib.lib().spiht_tile_resample_set(
        _lib.default_context().handle, elem(kind).stream_id, len(rows) if B is None else B, c, rh, rw, th, tw, size[0], size[1],
        C.byref(tab), vp(tabs.ctypes.data), vp(tables.ctypes.data), tables.nbytes, None if m is None else vp(m.ctypes.data),
        None if s is None else vp(s.ctypes.data), vp(d_tiles), S)


@functools.lru_cache(maxsize=None)
def problem(name, k):
    """launch k of a configuration: the tile batch with values below 0, above 1 and +-1e300, the items' sub-grids and boxes,
    and the float64 windows the boxes are (paste_rule)"""
    from spiht_amd import paste_rule, set_tables
    c, th, tw, rh, rw = CONFIGS[name]
    sizes, ls = launches(th, tw)
    size, items = ls[k]
    t = set_tables(sizes, th, tw, [(p, box) for p, box, _ in items])
    S = int(t["s0"][-1])
    rng = np.random.default_rng(300 + 10 * k + c)
    tiles = rng.standard_normal((S, c, rh, rw)) * 2 + 0.5
    spots = rng.random(tiles.shape)
    tiles[spots < 0.01] = 1e300
    tiles[spots > 0.99] = -1e300
    tiles.setflags(write=False)
    wins = paste_rule(tiles, list(zip(t["subs"], t["windows"])), th, tw)
    return tiles, S, size, [sizes[p] for p, _, _ in items], t["subs"], t["windows"], [f for _, _, f in items], wins


def out_buffer(want, layout, lead):
    """want [B, c, oh, ow] in a byte buffer pre-filled with 0xA5: "dense" CHW rows `lead` bytes in, or "hwc", the first c
    samples of four -> (the buffer as it must be afterwards, (sb, sc, sh, sw))"""
    B, c, oh, ow = want.shape
    es = want.dtype.itemsize
    if layout == "dense":
        buf = np.full(lead + want.nbytes + 24, 0xA5, np.uint8)
        buf[lead:lead + want.nbytes] = want.reshape(-1).view(np.uint8)
        return buf, (c * oh * ow * es, oh * ow * es, ow * es, es)
    a = np.full((B, oh, ow, 4 * es), 0xA5, np.uint8)
    a[..., :c * es] = np.ascontiguousarray(want.transpose(0, 2, 3, 1)).view(np.uint8).reshape(B, oh, ow, c * es)
    buf = np.full(lead + a.nbytes + 24, 0xA5, np.uint8)
    buf[lead:lead + a.nbytes] = a.reshape(-1)
    return buf, (oh * ow * 4 * es, es, ow * 4 * es, 4 * es)


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("kind", KINDS)
def test_resample_set_alone(name, kind):
    from spiht_amd import _lib, resample
    ctx = _lib.default_context()
    c, th, tw, rh, rw = CONFIGS[name]
    dt = elem(kind)
    es = dt.itemsize
    for k in range(len(launches(th, tw)[1])):
        tiles, S, size, pics, subs, boxes, flips, wins = problem(name, k)
        d_tiles = dev(tiles)
        tabs, tables = tables_of(boxes, size, flips)
        norms = [(None, None)] if dt.integer else [(None, None), (MEAN[:c], STD[:c])]
        for li, (layout, lead) in enumerate((("dense", 16), ("dense", 16 + es), ("hwc", 16 + es))):
            mean, std = norms[li % len(norms)]
            want = np.stack([resample.resize_rule(w, size, flip=f, mean=mean, std=std, dtype=dt) for w, f in zip(wins, flips)])
            buf, (sb, sc, sh, sw) = out_buffer(want, layout, lead)
            d_out = dev(np.full(buf.shape, 0xA5, np.uint8))
            rows = [(d_out.ptr + lead + b * sb, (sc, sh, sw), H, W, sub, box) for b, ((H, W), sub, box) in enumerate(zip(pics, subs, boxes))]
            assert resample_set(kind, c, rh, rw, th, tw, size, rows, tabs, tables, d_tiles.ptr, S, mean, std) == _lib.OK
            ctx.synchronize()
            got = d_out.download()
            assert np.array_equal(got, buf), (name, kind, k, layout, lead, int((got != buf).sum()))


def test_shared_tables_and_a_wider_sub_grid():
    """items that share one table blob entry, and a sub-grid larger than the tiles the box meets"""
    from spiht_amd import _lib, paste_rule, resample
    ctx = _lib.default_context()
    c, th, tw, rh, rw = CONFIGS["8x8"]
    H, W = 22, 32
    rng = np.random.default_rng(77)
    subs, boxes = [(0, 3, 0, 4), (1, 3, 1, 4)], [(9, 10, 7, 12), (12, 17, 7, 12)]
    S = 12 + 6
    tiles = rng.standard_normal((S, c, rh, rw))
    wins = paste_rule(tiles, list(zip(subs, boxes)), th, tw)
    size = (4, 5)
    tabs, tables = tables_of(boxes[:1], size, [False])
    tabs = np.repeat(tabs, 2, axis=0)
    want = np.stack([resample.resize_rule(w, size) for w in wins])
    d_tiles, d_out = dev(tiles), dev(np.zeros(want.shape))
    rows = [(d_out.ptr + b * want[0].nbytes, (size[0] * size[1] * 8, size[1] * 8, 8), H, W, sub, box)
            for b, (sub, box) in enumerate(zip(subs, boxes))]
    assert resample_set("f64", c, rh, rw, th, tw, size, rows, tabs, tables, d_tiles.ptr, S) == _lib.OK
    ctx.synchronize()
    assert d_out.download().tobytes() == want.tobytes()


def test_argument_errors_write_nothing():
    from spiht_amd import _lib, resample
    ctx = _lib.default_context()
    name, kind = "8x8", "u16"
    c, th, tw, rh, rw = CONFIGS[name]
    tiles, S, size, pics, subs, boxes, flips, wins = problem(name, 2)
    want = np.stack([resample.resize_rule(w, size, flip=f, dtype=np.uint16) for w, f in zip(wins, flips)])
    d_tiles, d_out = dev(tiles), dev(np.full(want.nbytes, 0xA5, np.uint8))
    tabs, tables = tables_of(boxes, size, flips)
    st = (size[0] * size[1] * 2, size[1] * 2, 2)
    rows = [(d_out.ptr + b * want[0].nbytes, st, H, W, sub, box) for b, ((H, W), sub, box) in enumerate(zip(pics, subs, boxes))]

    def ok():
        assert resample_set(kind, c, rh, rw, th, tw, size, rows, tabs, tables, d_tiles.ptr, S) == _lib.OK
        ctx.synchronize()
        assert d_out.download().tobytes() == want.tobytes()
        d_out.upload(np.full(want.nbytes, 0xA5, np.uint8))

    def spoil(k, **kw):
        names = ("addr", "st", "H", "W", "sub", "box")
        r = dict(zip(names, rows[k]))
        r.update(kw)
        return rows[:k] + [tuple(r[n] for n in names)] + rows[k + 1:]

    def table_with(item, axis, field, i, value):
        """the blob with one start (field 0) or count (field 1) of an item's column (axis 0) or row (axis 1) table changed"""
        t = tables.copy()
        n = size[1] if axis == 0 else size[0]
        v = t[int(tabs[item, 2 * axis]):][:8 * n].view(np.int32)
        v[field * n + i] = value
        return t

    def tabs_with(item, col, value):
        t = tabs.copy()
        t[item, col] = value
        return t

    ok()
    i0, i1, j0, j1 = subs[1]
    y0, x0, h, w = boxes[1]
    base = dict(c=c, rh=rh, rw=rw, th=th, tw=tw, size=size, rows=rows, tabs=tabs, tables=tables, S=S, mean=None, std=None, B=None, kind=kind)
    spoils = [dict(rows=spoil(1, sub=(i0, i1, j0, j1 - 1))),        # the sub-grid does not hold the box's tiles
              dict(rows=spoil(0, sub=(subs[0][0] + 1, subs[0][1], subs[0][2], subs[0][3]))),
              dict(rh=th - 1), dict(rw=tw - 1),
              dict(tabs=tabs_with(0, 1, 34)), dict(tabs=tabs_with(0, 3, 0)),   # K the kernel is not built for, K below 1
              dict(tabs=tabs_with(2, 0, int(tabs[2, 0]) + 4)),              # a table at no multiple of 8
              dict(tabs=tabs_with(2, 2, tables.nbytes - 8)),                # a table that leaves the blob
              dict(tables=table_with(1, 0, 0, 3, w)),                       # a run of taps that leaves the box, columns
              dict(tables=table_with(1, 1, 0, 10, h - 1)),                  # ... rows (output 10 has two taps)
              dict(tables=table_with(0, 0, 0, 0, -1)), dict(tables=table_with(0, 0, 1, 0, 0)),
              dict(tables=table_with(0, 1, 1, 0, 3)),                       # a count above K
              dict(B=0), dict(c=0), dict(size=(0, size[1])), dict(size=(size[0], 0)),
              dict(rows=spoil(3, addr=rows[3][0] + 1)),                     # misaligned for uint16
              dict(rows=spoil(3, st=(st[0], st[1], 1))), dict(rows=spoil(2, addr=None)),
              dict(rows=spoil(4, box=(2, 4, 2 * th + 1, 0))), dict(rows=spoil(5, box=(pics[5][0] - 1, pics[5][1] - 1, 2, 1))),
              dict(mean=MEAN), dict(std=STD), dict(mean=MEAN, std=STD),     # one without the other; either with 16 bits
              dict(S=S + 1), dict(S=S - 1), dict(kind=None)]
    for s in spoils:
        a = dict(base, **s)
        if a["kind"] is None:
            status = _lib.lib().spiht_tile_resample_set(ctx.handle, 6, len(rows), c, rh, rw, th, tw, size[0], size[1], None, None, None, 0,
                                                        None, None, vp(d_tiles.ptr), S)
        else:
            status = resample_set(a["kind"], a["c"], a["rh"], a["rw"], a["th"], a["tw"], a["size"], a["rows"], a["tabs"], a["tables"],
                                  d_tiles.ptr, a["S"], a["mean"], a["std"], a["B"])
        assert status == _lib.ERR_ARG, sorted(s)
        ctx.synchronize()
        assert (d_out.download() == 0xA5).all(), sorted(s)  # nothing was queued
    assert resample_set("float32", c, rh, rw, th, tw, size, rows, tabs, tables, d_tiles.ptr, S, MEAN, [0.2, 0.0, 0.2]) == _lib.ERR_ARG
    assert resample_set(kind, 65536, rh, rw, th, tw, size, rows, tabs, tables, d_tiles.ptr, S) == _lib.ERR_TOO_LARGE
    ctx.synchronize()
    assert (d_out.download() == 0xA5).all()
    ok()  # ... and the context is usable


def test_a_row_table_that_spans_more_than_a_workgroup_holds_is_refused():
    """150 box rows to 10: every 8 outputs span at most 145 rows by the rule; a table whose first 8 outputs reach from row 0 to
    row 149 is the caller's own and is refused"""
    from spiht_amd import _lib, paste_rule, resample
    ctx = _lib.default_context()
    c, th, tw, rh, rw = 1, 8, 8, 8, 8
    H, W, size, box, sub = 150, 8, (10, 4), (0, 0, 150, 8), (0, 19, 0, 1)
    tiles = np.random.default_rng(9).random((19, c, rh, rw))
    want = resample.resize_rule(paste_rule(tiles, [(sub, box)], th, tw)[0], size)
    d_tiles, d_out = dev(tiles), dev(np.zeros(want.shape))
    rows = [(d_out.ptr, (want.nbytes, size[1] * 8, 8), H, W, sub, box)]
    tabs, tables = tables_of([box], size, [False])
    assert resample_set("f64", c, rh, rw, th, tw, size, rows, tabs, tables, d_tiles.ptr, 19) == _lib.OK
    ctx.synchronize()
    assert d_out.download().tobytes() == want.tobytes()
    d_out.upload(np.zeros(want.shape))
    bad = tables.copy()
    v = bad[int(tabs[0, 2]):][:80].view(np.int32)
    v[7] = 150 - v[10 + 7]  # output 7 reads the box's last rows
    assert resample_set("f64", c, rh, rw, th, tw, size, rows, tabs, bad, d_tiles.ptr, 19) == _lib.ERR_ARG
    ctx.synchronize()
    assert not d_out.download().any()


# ---- end to end ------------------------------------------------------------------------------------------------------------
LEVEL, TILE_BITS = 2, 3001
SIZES = [(33, 47), (70, 90), (16, 16)]
# (picture, box, flip): picture 1 twice; a box of one sample; whole pictures; a ratio of exactly 16 down the rows of picture 1
ITEMS = [(0, (2, 3, 30, 40), False), (1, (5, 7, 60, 80), True), (2, (0, 0, 16, 16), False), (1, (33, 10, 20, 31), False),
         (0, (16, 16, 1, 1), True), (0, (0, 0, 33, 47), True), (1, (6, 0, 64, 90), False)]
SIZE = (4, 10)


@functools.lru_cache(maxsize=None)
def case(name):
    """the set codec, a TiledCodec per picture, the results and the float64 windows of ITEMS"""
    import spiht_amd
    kw = {"rgb": {}, "ipt": dict(settings=spiht_amd.SpihtSettings(color_model="IPT")), "f32": dict(pixel_dtype=np.float32)}[name]
    s, pd = kw.get("settings"), kw.get("pixel_dtype", np.float64)
    pics = [synth_image(8000 + 10 * k, 3, H, W) for k, (H, W) in enumerate(SIZES)]
    codec = spiht_amd.TileSetCodec(3, 16, s, LEVEL, TILE_BITS, pixel_dtype=pd)
    per = [spiht_amd.TiledCodec(3, H, W, 16, s, LEVEL, TILE_BITS * (-(-H // 16)) * (-(-W // 16)), pixel_dtype=pd) for H, W in SIZES]
    res = codec.encode([P.astype(codec.pixel_dtype) for P in pics])
    wins = [per[p].decode_window(res[p], *box) for p, box, _ in ITEMS]
    return codec, per, res, wins


def want_of(wins, kind, mean=None, std=None, size=SIZE):
    from spiht_amd import resample
    return np.stack([resample.resize_rule(w, size, flip=f, mean=mean, std=std, dtype=elem(kind)) for w, (_, _, f) in zip(wins, ITEMS)])


@pytest.mark.parametrize("name", ["rgb", "ipt", "f32"])
def test_resized_crops_equal_the_rule_of_decode_window(name):
    import spiht_amd
    codec, per, res, wins = case(name)
    rs, boxes, flips = [res[p] for p, _, _ in ITEMS], [b for _, b, _ in ITEMS], [f for _, _, f in ITEMS]
    got = codec.decode_resized_crops(rs, boxes, SIZE, flips)
    assert got.dtype == np.float64 and got.shape == (len(ITEMS), 3) + SIZE
    assert got.tobytes() == want_of(wins, "f64").tobytes()
    assert codec.last_tiles_decoded == sum((i1 - i0) * (j1 - j0) for i0, i1, j0, j1 in
                                           (spiht_amd.window_tiles(SIZES[p][0], SIZES[p][1], 16, 16, *b) for p, b, _ in ITEMS))
    assert codec.decode_resized_crops(rs, boxes, SIZE, flips, MEAN, STD).tobytes() == want_of(wins, "f64", MEAN, STD).tobytes()
    assert codec.decode_resized_crops(rs, boxes, SIZE).tobytes() == \
        np.stack([spiht_amd.resample.resize_rule(w, SIZE) for w in wins]).tobytes()
    for kind, call in (("u8", codec.decode_resized_crops_u8), ("u16", codec.decode_resized_crops_u16)):
        want = want_of(wins, kind)
        g = call(rs, boxes, SIZE, flips)
        assert g.dtype == want.dtype and g.tobytes() == want.tobytes(), kind
        g = call(rs, boxes, SIZE, flips, channels_last=True)
        assert g.shape == (len(ITEMS),) + SIZE + (3,) and np.array_equal(g, want.transpose(0, 2, 3, 1)), kind
    for kind in ("float32", "float16", "bfloat16"):
        want = want_of(wins, kind, MEAN, STD)
        g = codec.decode_resized_crops_float(rs, boxes, SIZE, flips, MEAN, STD, dtype=kind)
        assert g.dtype == want.dtype and g.tobytes() == want.tobytes(), kind
        g = codec.decode_resized_crops_float(rs, boxes, SIZE, flips, dtype=kind, channels_last=True)
        assert g.tobytes() == np.ascontiguousarray(want_of(wins, kind).transpose(0, 2, 3, 1)).tobytes(), kind
    # an upscale of every box
    up = (40, 97)
    assert codec.decode_resized_crops_float(rs[:5], boxes[:5], up, flips[:5], dtype=np.float16).tobytes() == \
        want_of(wins[:5], "float16", size=up).tobytes()


def gathered(results, boxes):
    """what decode_resized_device takes of host results: the run, the lengths and the start planes of the gathered tiles, and
    the items"""
    from spiht_amd import set_tables
    t = set_tables([(r.h, r.w) for r in results], 16, 16, list(enumerate(boxes)))
    run, lens, maxn = [], [], []
    for b, r in enumerate(results):
        off = np.concatenate(([0], np.cumsum(r.nbytes)))
        for k in t["gather"][int(t["s0"][b]):int(t["s0"][b + 1])]:
            run.append(r.encoded_bytes[int(off[k]):int(off[k + 1])])
            lens.append(r.nbytes[k])
            maxn.append(r.max_n[k])
    run = np.frombuffer(b"".join(run), np.uint8)
    items = [(sub, box, (r.h, r.w)) for sub, box, r in zip(t["subs"], boxes, results)]
    return run, np.asarray(lens, np.uint32), np.asarray(maxn, np.uint8), items


def test_the_device_form_into_a_strided_view_writes_nothing_else():
    """bfloat16 rows written as the [..., :3] samples of the inner oh x ow of a [B, oh + 2, ow + 3, 4] buffer"""
    from spiht_amd import _lib, tiles
    codec, per, res, wins = case("rgb")
    rs, boxes, flips = [res[p] for p, _, _ in ITEMS], [b for _, b, _ in ITEMS], [f for _, _, f in ITEMS]
    oh, ow = SIZE
    want = np.full((len(ITEMS), oh + 2, ow + 3, 4), 0xA5A5, np.uint16)
    want[:, 1:1 + oh, 2:2 + ow, :3] = want_of(wins, "bfloat16", MEAN, STD).transpose(0, 2, 3, 1)
    d_buf = dev(np.full(want.shape, 0xA5A5, np.uint16))
    row, pic = (ow + 3) * 8, (oh + 2) * (ow + 3) * 8
    run, lens, maxn, items = gathered(rs, boxes)
    d_run, d_lens, d_maxn = dev(run), dev(lens), dev(maxn)
    n = codec.decode_resized_device(d_run, len(run), d_lens, d_maxn, items, d_buf.ptr + row + 16, SIZE, tiles.float_elem("bfloat16"),
                                    (pic, 2, row, 8), flips, MEAN, STD)
    _lib.default_context().synchronize()
    assert n == len(lens) == codec.last_tiles_decoded
    assert np.array_equal(d_buf.download(), want)


def test_two_calls_queued_back_to_back_each_see_their_own_tables():
    from spiht_amd import _lib, resample
    from spiht_amd.batch import DeviceArray
    codec, per, res, wins = case("rgb")
    ctx = _lib.default_context()
    calls = [([res[p] for p, _, _ in ITEMS], [b for _, b, _ in ITEMS], [f for _, _, f in ITEMS], SIZE),
             ([res[1], res[0]], [(0, 0, 70, 90), (3, 4, 9, 11)], [True, False], (9, 11))]
    want = [codec.decode_resized_crops_float(rs, boxes, size, flips, MEAN, STD, dtype=np.float16) for rs, boxes, flips, size in calls]
    assert want[1][1].tobytes() == resample.resize_rule(per[0].decode_window(res[0], 3, 4, 9, 11), (9, 11), False, MEAN, STD, np.float16).tobytes()
    jobs = []
    for (rs, boxes, flips, size), w in zip(calls, want):
        run, lens, maxn, items = gathered(rs, boxes)
        jobs.append((dev(run), len(run), dev(lens), dev(maxn), items, DeviceArray(ctx, w.shape, np.float16), size, flips))
    ctx.synchronize()
    for d_run, nb, d_lens, d_maxn, items, d_out, size, flips in jobs:  # queued back to back
        codec.decode_resized_device(d_run, nb, d_lens, d_maxn, items, d_out, size, elem("float16"), None, flips, MEAN, STD)
    ctx.synchronize()
    for job, w in zip(jobs, want):
        assert job[5].download().tobytes() == w.tobytes()


def test_refusals():
    import spiht_amd
    codec, per, res, wins = case("rgb")
    r = res[1]  # 70 x 90
    for box, size, match in [((0, 0, 65, 10), (4, 10), "at most 16"), ((0, 0, 10, 81), (10, 5), "at most 16"),
                             ((0, 0, 0, 5), (4, 4), "empty"), ((60, 0, 11, 5), (4, 4), "leaves"), ((0, -1, 5, 5), (4, 4), "leaves"),
                             ((0, 0, 5, 5), (0, 4), "sides >= 1")]:
        with pytest.raises(ValueError, match=match):
            codec.decode_resized_crops([r], [box], size)
    ok = ([r], [(0, 0, 20, 20)], (5, 5))
    with pytest.raises(ValueError, match="go together"):
        codec.decode_resized_crops(*ok, mean=MEAN)
    with pytest.raises(ValueError, match="go together"):
        codec.decode_resized_crops_float(*ok, std=STD)
    with pytest.raises(ValueError, match="8- / 16-bit"):
        codec.decode_resized_device(0, 0, 0, 0, [(None, (0, 0, 20, 20), (70, 90))], 0, (5, 5), np.uint8, mean=MEAN, std=STD)
    with pytest.raises(ValueError, match="flips"):
        codec.decode_resized_crops(*ok, flips=[True, False])
    with pytest.raises(ValueError, match="boxes"):
        codec.decode_resized_crops([r, r], [(0, 0, 20, 20)], (5, 5))
    with pytest.raises(ValueError, match="reduce > 0 is not supported for a picture set"):
        codec.decode_resized_crops(*ok, reduce=1)
    lapped = spiht_amd.TiledCodec(3, 70, 90, 16, None, LEVEL, TILE_BITS * 30, overlap=2).encode(synth_image(8010, 3, 70, 90))
    with pytest.raises(ValueError, match="overlap > 0 is not supported for a picture set"):
        codec.decode_resized_crops_u8([lapped], ok[1], ok[2])
    assert codec.decode_resized_crops(*ok).shape == (1, 3, 5, 5)  # ... and the codec is usable
