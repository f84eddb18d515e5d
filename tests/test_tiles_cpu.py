"""Tiled pictures without a GPU: the grid and window arithmetic, and the container of a TiledResult."""
import struct

import numpy as np
import pytest


def test_tile_grid_arithmetic():
    from spiht_amd.tiles import tile_grid
    assert tile_grid(70, 90, 32, 32) == (3, 3)
    assert tile_grid(64, 96, 32, 32) == (2, 3)          # an exact multiple: no padded tile
    assert tile_grid(20, 27, 32, 32) == (1, 1)          # a picture smaller than one tile
    assert tile_grid(70, 90, 33, 40) == (3, 3)
    assert tile_grid(33, 41, 33, 40) == (1, 2)
    assert tile_grid(1, 1, 8, 8) == (1, 1)
    assert tile_grid(4096, 4096, 512, 512) == (8, 8)
    assert tile_grid(1080, 1920, 128, 128) == (9, 15)
    for bad in [(70, 90, 7, 32), (70, 90, 32, 7), (0, 90, 32, 32), (70, 0, 32, 32), (70, 90, 0, 0), (-1, 5, 8, 8)]:
        with pytest.raises(ValueError):
            tile_grid(*bad)
    with pytest.raises(OverflowError):
        tile_grid(1 << 30, 90, 32, 32)


def test_tile_grid_through_the_c_abi():
    """spiht_tile_grid on its own: statuses, and output pointers that may be NULL"""
    import ctypes as C
    from spiht_amd import _lib
    L = _lib.lib()
    gy, gx = C.c_int64(-1), C.c_int64(-1)
    assert L.spiht_tile_grid(70, 90, 32, 40, C.byref(gy), C.byref(gx)) == _lib.OK and (gy.value, gx.value) == (3, 3)
    assert L.spiht_tile_grid(70, 90, 32, 40, None, None) == _lib.OK
    assert L.spiht_tile_grid(70, 90, 32, 7, C.byref(gy), C.byref(gx)) == _lib.ERR_ARG
    assert (gy.value, gx.value) == (3, 3)  # untouched by a refused call


def test_window_to_sub_grid():
    from spiht_amd.tiles import window_tiles
    H, W, th, tw = 70, 90, 32, 32
    assert window_tiles(H, W, th, tw, 5, 40, 10, 12) == (0, 1, 1, 2)      # inside one tile
    assert window_tiles(H, W, th, tw, 0, 0, 32, 32) == (0, 1, 0, 1)       # exactly one tile: ends at the seam
    assert window_tiles(H, W, th, tw, 0, 0, 33, 32) == (0, 2, 0, 1)       # one row past the seam
    assert window_tiles(H, W, th, tw, 31, 31, 1, 1) == (0, 1, 0, 1)       # the last sample before a seam
    assert window_tiles(H, W, th, tw, 32, 32, 1, 1) == (1, 2, 1, 2)       # the first sample behind it
    assert window_tiles(H, W, th, tw, 31, 31, 2, 2) == (0, 2, 0, 2)       # across a four-tile corner
    assert window_tiles(H, W, th, tw, 32, 0, 32, 90) == (1, 2, 0, 3)      # a full row of tiles
    assert window_tiles(H, W, th, tw, 69, 89, 1, 1) == (2, 3, 2, 3)       # the last row and column (a padded tile)
    assert window_tiles(H, W, th, tw, 60, 80, 10, 10) == (1, 3, 2, 3)
    assert window_tiles(H, W, th, tw, 0, 0, 70, 90) == (0, 3, 0, 3)       # the whole picture
    assert window_tiles(70, 90, 33, 40, 33, 40, 33, 40) == (1, 2, 1, 2)   # an odd tile
    assert window_tiles(20, 27, 32, 32, 19, 26, 1, 1) == (0, 1, 0, 1)     # a single padded tile
    for bad in [(-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 5, 0), (61, 0, 10, 5), (0, 81, 5, 10), (70, 0, 1, 1),
                (0, 0, 71, 90)]:
        with pytest.raises(ValueError):
            window_tiles(H, W, th, tw, *bad)
    # the count of tiles a window meets, against a count done sample by sample
    rng = np.random.default_rng(1)
    for _ in range(200):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w = int(rng.integers(1, H - y0 + 1)), int(rng.integers(1, W - x0 + 1))
        i0, i1, j0, j1 = window_tiles(H, W, th, tw, y0, x0, h, w)
        ys, xs = np.arange(y0, y0 + h) // th, np.arange(x0, x0 + w) // tw
        assert (i0, i1 - 1, j0, j1 - 1) == (ys.min(), ys.max(), xs.min(), xs.max())
        assert (i1 - i0) * (j1 - j0) == len(set(ys)) * len(set(xs))


def _result(level=2, seed=0):
    from spiht_amd.tiles import TiledResult
    rng = np.random.default_rng(seed)
    nbytes = [0, 1, 7, 300, 0, 33, 2, 5, 11]
    data = rng.integers(0, 256, sum(nbytes), dtype=np.uint8).tobytes()
    return TiledResult(70, 90, 3, 32, 32, level, [int(v) for v in rng.integers(0, 31, 9)], nbytes, data)


@pytest.mark.parametrize("level", [2, None, 0])
def test_tiled_result_bytes_round_trip(level):
    from spiht_amd.tiles import TiledResult
    r = _result(level)
    b = r.to_bytes()
    assert b[:4] == b"SPTL" and b[4] == 1 and b[5] == (255 if level is None else level)
    assert struct.unpack_from("<HIIII", b, 6) == (3, 70, 90, 32, 32)
    assert np.frombuffer(b, "<u4", 9, 24).tolist() == r.nbytes and list(b[24 + 36:24 + 45]) == r.max_n
    assert b[24 + 45:] == r.encoded_bytes and len(b) == 24 + 45 + len(r.encoded_bytes)
    back = TiledResult.from_bytes(b)
    assert back == r and back.level == level
    assert TiledResult.from_bytes(bytearray(b)) == r
    # the tiles are slices of the run, in row-major order
    off = np.concatenate(([0], np.cumsum(r.nbytes)))
    for i in range(3):
        for j in range(3):
            t = r.tile(i, j)
            k = 3 * i + j
            assert (t.encoded_bytes, t.h, t.w, t.c, t.max_n, t.level) == (r.encoded_bytes[off[k]:off[k + 1]], 32, 32, 3, r.max_n[k], level)
    with pytest.raises(IndexError):
        r.tile(3, 0)


def test_tiled_result_single_tile_and_empty_streams():
    from spiht_amd.tiles import TiledResult
    r = TiledResult(20, 27, 1, 32, 32, None, [0], [0], b"")
    assert TiledResult.from_bytes(r.to_bytes()) == r and r.tile(0, 0).encoded_bytes == b""


def test_malformed_containers():
    from spiht_amd.tiles import TiledResult
    good = _result().to_bytes()
    TiledResult.from_bytes(good)
    bad = {
        "magic": b"SPTX" + good[4:],
        "version": good[:4] + b"\x02" + good[5:],
        "short header": good[:20],
        "short table": good[:24 + 40],
        "one byte missing": good[:-1],
        "one byte more": good + b"\x00",
        "a length changed": good[:24] + struct.pack("<I", 1) + good[28:],
        "a tile side below 8": good[:16] + struct.pack("<I", 4) + good[20:],
    }
    for name, b in bad.items():
        with pytest.raises(ValueError):
            TiledResult.from_bytes(b)
    r = _result()
    r.nbytes[0] += 1
    with pytest.raises(ValueError):
        r.to_bytes()


def test_names_are_exported():
    import spiht
    import spiht_amd
    for name in ["TiledCodec", "TiledResult", "tile_grid", "window_tiles", "encode_image_tiled", "encode_image_tiled_u8",
                 "encode_image_tiled_u16", "decode_image_tiled", "decode_image_tiled_u8", "decode_image_tiled_u16",
                 "decode_image_window", "decode_image_window_u8", "decode_image_window_u16"]:
        assert getattr(spiht, name) is getattr(spiht_amd, name)
    assert spiht.tiles is spiht_amd.tiles
    from spiht_amd.encode_decode import build_parser
    a = build_parser().parse_args(["x.png", "--tile", "64", "--window", "1,2,3,4"])
    assert a.tile == 64 and a.window == "1,2,3,4"
    assert build_parser().parse_args(["x.png"]).tile is None
