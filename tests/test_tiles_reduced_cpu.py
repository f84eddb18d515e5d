"""Tiled pictures at reduced resolution, without a GPU: spiht_tile_reduced_grid / tiled_reduced_shape against the closed
forms and against reduced_shape of one tile, their refusals, the exported names and the command line's parser."""
import ctypes as C

import pytest

WAVELETS = ["haar", "bior2.2", "bior4.4", "bior6.8"]
MODES = ["reflect", "periodization"]
TILES = [32, 16, (16, 40), (33, 40)]
PICTURES = [(70, 90), (64, 96), (20, 27), (1, 1)]
NAMES = ("thk", "twk", "Hk", "Wk", "gy", "gx", "rec_h", "rec_w", "pic_h", "pic_w", "off_y", "off_x")


def tile_of(tile):
    return tuple(tile) if isinstance(tile, tuple) else (tile, tile)


def grid_call(H, W, th, tw, wid, mid, level, reduce):
    from spiht_amd import _lib
    lv = C.c_int(-7)
    v = [C.c_int64(-7) for _ in NAMES]
    st = _lib.lib().spiht_tile_reduced_grid(H, W, th, tw, wid, mid, level, reduce, C.byref(lv), *[C.byref(t) for t in v])
    return st, lv.value, dict(zip(NAMES, [t.value for t in v]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_reduced_grid_closed_forms(wavelet, mode):
    """every tile, picture, level and k: the closed forms of the contract, and reduced_shape of a th x tw picture"""
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.spiht_wrapper import _wavelet_mode_ids
    s = spiht_amd.SpihtSettings(wavelet=wavelet, mode=mode)
    wid, mid = _wavelet_mode_ids(s)
    n = 0
    for tile in TILES:
        th, tw = tile_of(tile)
        for level in (None, 1, 2, 3):
            L = spiht_amd.reduced_shape(th, tw, s, level, 0)["level"]
            assert level is None or L == level
            for k in range(L + 1):
                allowed = th % 2 ** k == 0 and tw % 2 ** k == 0
                for (H, W) in PICTURES:
                    st, lv, g = grid_call(H, W, th, tw, wid, mid, -1 if level is None else level, k)
                    if not allowed:
                        assert st == _lib.ERR_ARG
                        with pytest.raises(ValueError):
                            spiht_amd.tiled_reduced_shape(H, W, tile, s, level, k)
                        continue
                    assert st == _lib.OK and lv == L
                    rs = spiht_amd.reduced_shape(th, tw, s, level, k)
                    want = dict(thk=th >> k, twk=tw >> k, Hk=-(-H // 2 ** k), Wk=-(-W // 2 ** k), gy=-(-H // th), gx=-(-W // tw),
                                rec_h=rs["rec_h"], rec_w=rs["rec_w"], pic_h=rs["pic_h"], pic_w=rs["pic_w"], off_y=rs["off_y"],
                                off_x=rs["off_x"])
                    assert g == want, (tile, level, k, H, W)
                    assert spiht_amd.tiled_reduced_shape(H, W, tile, s, level, k) == dict(level=L, **want)
                    # the crop=True window of the reduced tile is the reduced tile itself, inside both of its pictures
                    assert (rs["in_h"], rs["in_w"]) == (g["thk"], g["twk"])
                    assert g["off_y"] + g["thk"] <= min(g["rec_h"], g["pic_h"]) and g["off_x"] + g["twk"] <= min(g["rec_w"], g["pic_w"])
                    # the reduced grid is the full one; an edge tile owns ceil((H - i th) / 2^k) rows
                    assert -(-g["Hk"] // g["thk"]) == g["gy"] and -(-g["Wk"] // g["twk"]) == g["gx"]
                    i, j = g["gy"] - 1, g["gx"] - 1
                    assert g["Hk"] - i * g["thk"] == -(-(H - i * th) // 2 ** k) and g["Wk"] - j * g["twk"] == -(-(W - j * tw) // 2 ** k)
                    if mode == "periodization":
                        assert (g["off_y"], g["off_x"]) == (0, 0)
                    n += 1
    assert n >= 100


def test_refusals():
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.spiht_wrapper import _wavelet_mode_ids
    s = spiht_amd.SpihtSettings()
    wid, mid = _wavelet_mode_ids(s)
    assert grid_call(70, 90, 32, 32, wid, mid, 3, 3)[0] == _lib.OK
    for args in [(70, 90, 32, 32, wid, mid, 3, 4),      # k > L
                 (70, 90, 32, 32, wid, mid, 3, -1),     # k < 0
                 (70, 90, 32, 32, wid, mid, 3, 1 << 20),
                 (70, 90, 33, 40, wid, mid, 3, 1),      # 33 is odd
                 (70, 90, 16, 40, wid, mid, 4, 4),      # 40 = 8 * 5
                 (70, 90, 32, 7, wid, mid, 1, 0),       # what spiht_tile_grid refuses
                 (0, 90, 32, 32, wid, mid, 3, 1),
                 (70, 90, 32, 32, -1, mid, 3, 1),
                 (70, 90, 32, 32, wid, 9, 3, 1)]:
        st, lv, g = grid_call(*args)
        assert st == _lib.ERR_ARG, args
    assert grid_call(70, 90, 16, 40, wid, mid, 4, 3)[0] == _lib.OK  # twk = 5
    for tile, level, k in [(32, 3, 4), (32, 3, -1), ((33, 40), 3, 1), ((33, 40), None, 1), ((16, 40), 4, 4)]:
        with pytest.raises(ValueError):
            spiht_amd.tiled_reduced_shape(70, 90, tile, s, level, k)
    for k in (1.0, "1", None, True):
        with pytest.raises(TypeError):
            spiht_amd.tiled_reduced_shape(70, 90, 32, s, 3, k)
    assert spiht_amd.tiled_reduced_shape(70, 90, (33, 40), s, 3, 0)["thk"] == 33


def test_null_output_pointers():
    from spiht_amd import _lib
    L = _lib.lib()
    wid = L.spiht_wavelet_id(b"bior6.8")
    assert L.spiht_tile_reduced_grid(4096, 4096, 512, 512, wid, 0, -1, 3, None, *[None] * 12) == _lib.OK
    assert L.spiht_tile_reduced_grid(4096, 4096, 512, 512, wid, 0, -1, 99, None, *[None] * 12) == _lib.ERR_ARG
    hk = C.c_int64()
    args = [None] * 12
    args[2] = C.byref(hk)
    assert L.spiht_tile_reduced_grid(4095, 4096, 512, 512, wid, 0, -1, 3, None, *args) == _lib.OK and hk.value == 512


def test_window_tiles_of_a_reduced_grid():
    """the sub-grid arithmetic takes reduced tiles of any side >= 1"""
    from spiht_amd import window_tiles
    assert window_tiles(9, 12, 2, 2, 1, 2, 3, 3) == (0, 2, 1, 3)
    assert window_tiles(9, 12, 2, 5, 8, 11, 1, 1) == (4, 5, 2, 3)
    assert window_tiles(3, 3, 1, 1, 1, 1, 2, 2) == (1, 3, 1, 3)
    for bad in [(9, 12, 0, 2, 0, 0, 1, 1), (9, 12, 2, 2, 8, 0, 2, 1), (9, 12, 2, 2, 0, 0, 0, 1)]:
        with pytest.raises(ValueError):
            window_tiles(*bad)


def test_names_are_exported_and_the_parser_takes_the_flags():
    import inspect

    import spiht
    import spiht_amd
    from spiht_amd import _lib
    assert spiht.tiled_reduced_shape is spiht_amd.tiled_reduced_shape is spiht_amd.tiles.tiled_reduced_shape
    for s in ["spiht_tile_reduced_grid", "spiht_tile_mosaic_u8", "spiht_tile_mosaic_u16", "spiht_tile_mosaic_f64"]:
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)
    # every decode form takes reduce, 0 by default
    names = ["decode_image_tiled", "decode_image_window", "decode_image_layered", "decode_image_layered_window"]
    for name in names:
        for suffix in ("", "_u8", "_u16"):
            assert inspect.signature(getattr(spiht_amd, name + suffix)).parameters["reduce"].default == 0
    for name in ["decode", "decode_window", "decode_layered", "decode_layered_window"]:
        for suffix in ("", "_u8", "_u16"):
            assert inspect.signature(getattr(spiht_amd.TiledCodec, name + suffix)).parameters["reduce"].default == 0
    for name in ["decode_window_device", "decode_device", "decode_layers_device"]:
        assert inspect.signature(getattr(spiht_amd.TiledCodec, name)).parameters["reduce"].default == 0
    from spiht_amd.encode_decode import build_parser
    a = build_parser().parse_args(["x.png", "--tile", "32", "--reduce", "1", "--window", "1,2,3,4"])
    assert (a.tile, a.reduce, a.window) == (32, 1, "1,2,3,4")
