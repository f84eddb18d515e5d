"""CPU tests of the picture sets (spiht_amd/tileset.py): the rules in numpy -- cut_rule, paste_rule, set_tables -- against brute
force, and the refusals of TileSetCodec, each raised before a context is created or used.  No device."""
import ctypes as C

import numpy as np
import pytest

from tile_helpers import tile_pixels

# the set of the GPU tests: 2 x 2 with padding on both axes, one tile, smaller than a tile, 3 x 1, 1 x 4
SIZES = [(20, 27), (16, 16), (5, 7), (33, 16), (16, 49)]


def picture(seed, c, H, W):
    return np.random.default_rng(seed).integers(0, 256, (c, H, W)).astype(np.uint8)


def random_sets(n=200, seed=20261):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        P = int(rng.integers(1, 7))
        th, tw = int(rng.integers(8, 25)), int(rng.integers(8, 25))
        yield [(int(rng.integers(1, 71)), int(rng.integers(1, 71))) for _ in range(P)], th, tw, rng


def brute_windows(H, W):
    """every kind of window of an H x W picture: all of it, each corner sample, a band across, an inner box"""
    out = [(0, 0, H, W), (0, 0, 1, 1), (H - 1, W - 1, 1, 1), (0, W - 1, H, 1), (H - 1, 0, 1, W), (H // 2, 0, H - H // 2, W)]
    if H > 2 and W > 2:
        out.append((1, 1, H - 2, W - 2))
    return out


@pytest.mark.parametrize("tile", [(16, 16), (16, 24), (8, 11)])
def test_cut_rule_is_tile_pixels_and_paste_rule_gives_the_windows_back(tile):
    from spiht_amd import cut_rule, paste_rule, set_tables, window_tiles
    th, tw = tile
    for c in (1, 3):
        pics = [picture(10 * c + p, c, H, W) for p, (H, W) in enumerate(SIZES)]
        tiles = cut_rule(pics, th, tw)
        t = set_tables(SIZES, th, tw)
        assert tiles.shape == (int(t["tile0"][-1]), c, th, tw) and tiles.dtype == np.uint8
        for p, P in enumerate(pics):
            gy, gx = t["grids"][p]
            for i in range(gy):
                for j in range(gx):
                    assert np.array_equal(tiles[int(t["tile0"][p]) + i * gx + j], tile_pixels(P, th, tw, i, j))
        # every window of a brute-force list, from only the tiles it meets; decoded tiles may be larger than the tile
        items = [(p, w) for p, (H, W) in enumerate(SIZES) for w in brute_windows(H, W)]
        t = set_tables(SIZES, th, tw, items)
        rows = np.concatenate([int(t["tile0"][p]) + t["gather"][int(t["s0"][b]):int(t["s0"][b + 1])] for b, (p, _) in enumerate(items)])
        big = np.full((len(rows), c, th + 1, tw + 2), 0xEE, np.uint8)
        big[:, :, :th, :tw] = tiles[rows]
        got = paste_rule(big, list(zip(t["subs"], t["windows"])), th, tw)
        assert len(got) == len(items)
        for (p, _), (y0, x0, h, w), g in zip(items, t["windows"], got):
            assert np.array_equal(g, pics[p][:, y0:y0 + h, x0:x0 + w])
        with pytest.raises(ValueError):
            paste_rule(big[:-1], list(zip(t["subs"], t["windows"])), th, tw)
        sub, win = t["subs"][0], t["windows"][0]
        with pytest.raises(ValueError):  # a sub-grid missing a tile its window meets
            paste_rule(big, [((sub[0], sub[1] - 1 if sub[1] - sub[0] > 1 else sub[1], sub[2] + 1, sub[3]), win)], th, tw)
        assert window_tiles(20, 27, 16, 16, 9, 14, 11, 13) == (0, 2, 0, 2)


def check_tables(sizes, th, tw, items):
    from spiht_amd import set_tables, window_tiles
    t = set_tables(sizes, th, tw, items)
    counts = [-(-H // th) * -(-W // tw) for H, W in sizes]
    assert t["grids"] == [(-(-H // th), -(-W // tw)) for H, W in sizes]
    assert list(t["tile0"]) == [sum(counts[:p]) for p in range(len(sizes) + 1)]
    assert t["pic_of_tile"].dtype == np.uint32 and len(t["pic_of_tile"]) == sum(counts)
    for row, p in enumerate(t["pic_of_tile"]):
        assert t["tile0"][p] <= row < t["tile0"][p + 1]
    s0, gather, owner = 0, [], []
    for b, (p, win) in enumerate(items):
        H, W = sizes[p]
        y0, x0, h, w = (0, 0, H, W) if win is None else win
        assert t["windows"][b] == (y0, x0, h, w)
        sub = window_tiles(H, W, th, tw, y0, x0, h, w)
        assert t["subs"][b] == sub
        # brute force: the tiles that hold a sample of the window, row-major
        meets = [i * t["grids"][p][1] + j for i in range(t["grids"][p][0]) for j in range(t["grids"][p][1])
                 if i * th < y0 + h and (i + 1) * th > y0 and j * tw < x0 + w and (j + 1) * tw > x0]
        assert meets == sorted(meets)
        assert t["s0"][b] == s0
        gather += meets
        owner += [b] * len(meets)
        s0 += len(meets)
    assert t["s0"][-1] == s0 and list(t["gather"]) == gather and list(t["item_of_tile"]) == owner
    assert t["item_of_tile"].dtype == np.uint32


def test_set_tables_against_brute_force():
    from spiht_amd import set_tables
    for tile in ((16, 16), (16, 24)):
        items = [(p, w) for p, (H, W) in enumerate(SIZES) for w in brute_windows(H, W) + [None]]
        items += [(0, (9, 14, 11, 13)), (0, (0, 0, 11, 13)), (3, (22, 3, 11, 13)), (4, (5, 36, 11, 13))]
        check_tables(SIZES, *tile, items)
    assert int(set_tables(SIZES, 16, 16)["tile0"][-1]) == 13
    for sizes, th, tw, rng in random_sets():
        items = []
        for _ in range(int(rng.integers(1, 9))):
            p = int(rng.integers(0, len(sizes)))
            H, W = sizes[p]
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            items.append((p, (y0, x0, int(rng.integers(1, H - y0 + 1)), int(rng.integers(1, W - x0 + 1)))))
        items.append((0, None))
        check_tables(sizes, th, tw, items)
    for bad in (dict(sizes=[], th=16, tw=16), dict(sizes=[(0, 4)], th=16, tw=16), dict(sizes=[(4, 4)], th=7, tw=16),
                dict(sizes=[(4, 4)], th=16, tw=16, items=[]), dict(sizes=[(4, 4)], th=16, tw=16, items=[(0, (0, 0, 5, 4))])):
        with pytest.raises(ValueError):
            set_tables(**bad)


# ---- the refusals ----------------------------------------------------------------------------------------------------------
class StubContext:
    """a context whose handle is never given to the library: whatever a call would do with it fails the test"""
    device = 0
    handle = C.c_void_p(0x10)

    def __getattr__(self, name):
        raise AssertionError("a refused call reached the context (%s)" % name)


@pytest.fixture
def no_context(monkeypatch):
    """any attempt to create a GPU context fails the test"""
    from spiht_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a context was created by a call on a stub context")
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib.Context, "__init__", boom)


def result_of(H, W, c=3, th=16, tw=16, level=2, overlap=0):
    from spiht_amd import TiledResult
    T = -(-H // th) * -(-W // tw)
    return TiledResult(H, W, c, th, tw, level, [3] * T, [2] * T, b"\0\0" * T, overlap=overlap)


def test_refusals_come_before_a_context(no_context):
    import spiht_amd
    from spiht_amd import TileSetCodec
    codec = TileSetCodec(3, 16, None, 2, 3001, StubContext())
    good = result_of(20, 27)
    decodes = [codec.decode, codec.decode_u8, codec.decode_u16, codec.decode_float]
    # a window outside the picture
    for win in ((0, 0, 21, 27), (10, 15, 11, 13), (-1, 0, 4, 4), (0, 0, 0, 4)):
        for fn in (codec.decode_windows, codec.decode_windows_u8, codec.decode_windows_u16, codec.decode_windows_float):
            with pytest.raises(ValueError, match="window"):
                fn([good, good], [None, win])
    for fn in (codec.decode_crops, codec.decode_crops_u8, codec.decode_crops_u16, codec.decode_crops_float):
        with pytest.raises(ValueError, match="window"):
            fn([good, result_of(5, 7)], [(0, 0), (0, 0)], (11, 13))
        with pytest.raises(ValueError):
            fn([good], [(0, 0), (1, 1)], (4, 4))
    # results that are not the codec's
    other = {"tile sides": result_of(20, 27, tw=24), "c": result_of(20, 27, c=1), "level": result_of(20, 27, level=1)}
    for what, r in other.items():
        for fn in decodes:
            with pytest.raises(ValueError, match="the codec's"):
                fn([good, r])
    spol = result_of(20, 27, overlap=2)
    assert spol.to_bytes()[:4] == b"SPOL" and spiht_amd.TiledResult.from_bytes(spol.to_bytes()).overlap == 2
    for fn in decodes:
        with pytest.raises(ValueError, match="overlap"):
            fn([spol])
    short = result_of(20, 27)
    short.nbytes = short.nbytes[:-1]
    with pytest.raises(ValueError, match="tables"):
        codec.decode([short])
    # an empty list
    for fn in decodes + [codec.encode, codec.encode_u8, codec.encode_u16, codec.encode_float]:
        with pytest.raises(ValueError, match="empty"):
            fn([])
    for fn in (codec.decode_windows, codec.decode_windows_u8):
        with pytest.raises(ValueError, match="empty"):
            fn([], [])
    with pytest.raises(ValueError, match="empty"):
        codec.decode_crops([], [], (4, 4))
    # every out-of-scope keyword, named
    with pytest.raises(ValueError, match="allocate"):
        TileSetCodec(3, 16, None, 2, 3001, StubContext(), allocate="rd")
    with pytest.raises(ValueError, match="overlap"):
        TileSetCodec(3, 16, None, 2, 3001, StubContext(), overlap=4)
    P8 = picture(1, 3, 20, 27)
    for fn, P in ((codec.encode, P8 / 255.0), (codec.encode_u8, P8), (codec.encode_u16, P8.astype(np.uint16)),
                  (codec.encode_float, P8.astype(np.float32))):
        for key, value in (("roi", np.ones((20, 27), np.uint8)), ("target_psnr", 40.0), ("layers", 2)):
            with pytest.raises(ValueError, match=key):
                fn([P], **{key: value})
    for fn in decodes:
        with pytest.raises(ValueError, match="reduce"):
            fn([good], reduce=1)
    with pytest.raises(ValueError, match="reduce"):
        codec.decode_windows([good], [None], reduce=1)
    with pytest.raises(ValueError, match="reduce"):
        codec.decode_crops([good], [(0, 0)], (4, 4), reduce=1)
    # what the grid refuses, and pictures that are not the codec's
    with pytest.raises(ValueError):
        TileSetCodec(3, 7, None, 2, 3001, StubContext())
    with pytest.raises(ValueError, match="channels"):
        codec.encode_u8([picture(2, 1, 20, 27)])
    with pytest.raises(ValueError, match="uint8"):
        codec.encode_u8([P8.astype(np.uint16)])
    with pytest.raises(ValueError, match="channels_last"):
        codec.decode_crops([good], [(0, 0)], (4, 4), channels_last=True)
