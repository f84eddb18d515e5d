"""Overlapping tiles without a GPU: the rule of spiht_amd/overlap.py (the axis plan, the blend, the tiles a window needs)
against brute-force loops, the SPOL / SPOQ containers, and -- with the oracle's per-tile encode and decode -- that the
cross-fade does what it is for: the step of the decoding error across a seam falls below half of what hard seams leave."""
import numpy as np
import pytest

from spiht_amd import overlap
from spiht_amd.tiles import LayeredResult, TiledResult, window_tiles


def brute_axis(n, t, m):
    """per position: the list of (tile, sample index, weight) with non-zero weight, straight from the rule's sentences"""
    g = -(-n // t)
    out = []
    for P in range(n):
        hit = [k for k in range(1, g) if k * t - m <= P < k * t + m]
        assert len(hit) <= 1  # the zones are disjoint
        if hit:
            k = hit[0]
            u = P - (k * t - m)
            a = 2 * u + 1
            out.append([(k - 1, P - (k - 1) * t + m, 4 * m - a), (k, P - k * t + m, a)])
        else:
            out.append([(P // t, P - (P // t) * t + m, 4 * m)])
    return out


def plan_rows(p):
    rows = []
    for P in range(len(p.zone)):
        if p.zone[P]:
            rows.append([(int(p.k0[P]), int(p.i0[P]), int(p.b[P])), (int(p.k1[P]), int(p.i1[P]), int(p.a[P]))])
        else:
            assert (p.k1[P], p.i1[P], p.a[P]) == (p.k0[P], p.i0[P], 0)
            rows.append([(int(p.k0[P]), int(p.i0[P]), int(p.b[P]))])
    return rows


@pytest.mark.parametrize("t", [8, 9, 32])
def test_axis_plan_against_brute_force(t):
    for n in range(1, 81):
        for m in range(1, t // 2 + 1):
            p = overlap.axis_plan(n, t, m)
            assert plan_rows(p) == brute_axis(n, t, m), (n, t, m)
            # a zone's weights add up to 4m, every sample index lies in the coded tile
            assert ((p.a + p.b) == 4 * m).all() and (p.i0 >= 0).all() and (p.i0 < t + 2 * m).all() and (p.i1 < t + 2 * m).all()
            assert (p.a[p.zone] >= 1).all() and (p.b[p.zone] >= 1).all()


def test_axis_plan_symmetry_touching_zones_and_cut_zone():
    # a(u) = b(2m - 1 - u) across a whole zone
    p = overlap.axis_plan(64, 32, 5)
    z = np.arange(32 - 5, 32 + 5)
    assert p.zone[z].all() and not p.zone[26] and not p.zone[37]
    assert np.array_equal(p.a[z], p.b[z][::-1]) and list(p.a[z]) == list(range(1, 20, 2))
    # 2m = t: the zones touch, every position between the first and the last seam's reach lies in exactly one
    p = overlap.axis_plan(40, 8, 4)
    assert not p.zone[:4].any() and p.zone[4:36].all() and not p.zone[36:].any()
    assert list(p.k1[4:36]) == [1] * 8 + [2] * 8 + [3] * 8 + [4] * 8
    # a last tile of one row: its zone is cut by the picture's end, and simply shorter
    p = overlap.axis_plan(17, 8, 3)
    assert list(np.flatnonzero(p.zone)) == [5, 6, 7, 8, 9, 10, 13, 14, 15, 16]
    assert (p.k0[16], p.i0[16], p.b[16], p.k1[16], p.i1[16], p.a[16]) == (1, 11, 5, 2, 3, 7)
    for bad in [(10, 8, 5), (10, 8, -1), (0, 8, 1)]:
        with pytest.raises(ValueError):
            overlap.axis_plan(*bad)
    assert overlap.overlap_arg(4, 8, 9) == 4
    with pytest.raises(ValueError):
        overlap.overlap_arg(5, 8, 16)
    with pytest.raises(TypeError):
        overlap.overlap_arg(1.0, 8, 8)


def brute_blend(tiles, H, W, th, tw, m):
    """the whole picture by scalar loops over the rule: columns first, then rows, each operation rounded once"""
    gx = -(-W // tw)
    ax_, ay_ = brute_axis(W, tw, m), brute_axis(H, th, m)
    c = tiles.shape[1]
    out = np.empty((c, H, W))
    fm = np.float64(4 * m)

    def hval(i, ch, row, X):
        e = ax_[X]
        if len(e) == 1:
            return tiles[i * gx + e[0][0], ch, row, e[0][1]]
        (kl, il, b), (kr, ir, a) = e
        return (np.float64(b) * tiles[i * gx + kl, ch, row, il] + np.float64(a) * tiles[i * gx + kr, ch, row, ir]) / fm

    for ch in range(c):
        for Y in range(H):
            e = ay_[Y]
            for X in range(W):
                if len(e) == 1:
                    out[ch, Y, X] = hval(e[0][0], ch, e[0][1], X)
                else:
                    (kt, it, b), (kb, ib, a) = e
                    out[ch, Y, X] = (np.float64(b) * hval(kt, ch, it, X) + np.float64(a) * hval(kb, ch, ib, X)) / fm
    return out


def test_blend_against_loops_ones_windows_and_integer_forms():
    rng = np.random.default_rng(5)
    H, W, t, m = 20, 27, 8, 3
    gy, gx = 3, 4
    tiles = rng.standard_normal((gy * gx, 2, t + 2 * m + 1, t + 2 * m)) * 0.4 + 0.5  # (one row longer than needed)
    full = overlap.blend(tiles, H, W, t, t, m)
    assert full.dtype == np.float64 and np.array_equal(full, brute_blend(tiles, H, W, t, t, m))
    # weights that add up to 4m, divided by 4m: tiles of ones give exactly 1.0
    assert (overlap.blend(np.ones_like(tiles), H, W, t, t, m) == 1.0).all()
    assert (overlap.blend(np.ones((6, 1, 14, 22)), 14, 40, 8, 16, 3) == 1.0).all()  # (4m = 12: an inexact reciprocal)
    # a window is the crop of the whole picture, from the sub-grid window_tiles_overlap names: every window
    grid = tiles.reshape((gy, gx) + tiles.shape[1:])
    for y0 in range(H):
        for x0 in range(W):
            for (h, w) in {(1, 1), (H - y0, W - x0), (min(5, H - y0), min(9, W - x0))}:
                i0, i1, j0, j1 = sub = overlap.window_tiles_overlap(H, W, t, t, m, y0, x0, h, w)
                part = np.ascontiguousarray(grid[i0:i1, j0:j1]).reshape((-1,) + tiles.shape[1:])
                got = overlap.blend(part, H, W, t, t, m, window=(y0, x0, h, w), sub=sub)
                assert np.array_equal(got, full[:, y0:y0 + h, x0:x0 + w]), (y0, x0, h, w)
    assert np.array_equal(overlap.blend(tiles, H, W, t, t, m, window=(7, 6, 3, 5)), full[:, 7:10, 6:11])
    with pytest.raises(ValueError):  # a sub-grid that misses a tile with weight in the window
        overlap.blend(tiles[:4], H, W, t, t, m, window=(5, 0, 1, 1), sub=(0, 1, 0, 4))
    # the 8- / 16-bit forms: the documented conversion of the float64 result, NaN -> 0
    tiles[3, 0, 5, 5], tiles[0, 1, 4, 4], tiles[1, 1, 9, 9] = np.nan, 1e300, -7.0
    full = overlap.blend(tiles, H, W, t, t, m)
    assert np.isnan(full).any() and (full > 1).any() and (full < 0).any()
    for dtype, peak in ((np.uint8, 255.0), (np.uint16, 65535.0)):
        want = np.trunc(np.where(np.isnan(full), 0.0, np.clip(full, 0.0, 1.0)) * peak).astype(dtype)
        got = overlap.blend(tiles, H, W, t, t, m, dtype=dtype)
        assert got.dtype == dtype and np.array_equal(got, want)
    # m = 0: every sample from the tile that owns it
    plain = rng.random((12, 1, 8, 8))
    want = plain.reshape(3, 4, 8, 8).transpose(0, 2, 1, 3).reshape(1, 24, 32)[:, :H, :W]
    assert np.array_equal(overlap.blend(plain, H, W, 8, 8, 0), want)


def test_cut_is_edge_padding_on_four_sides():
    P = np.arange(2 * 9 * 13, dtype=np.float64).reshape(2, 9, 13)
    tiles = overlap.cut(P, 8, 8, 3)
    assert tiles.shape == (4, 2, 14, 14)
    for t, (i, j) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        for y in (0, 2, 3, 10, 13):
            for x in (0, 3, 7, 13):
                assert (tiles[t, :, y, x] == P[:, min(max(i * 8 - 3 + y, 0), 8), min(max(j * 8 - 3 + x, 0), 12)]).all()


def test_window_tiles_overlap_against_brute_force():
    for (H, W, th, tw, m) in [(20, 27, 8, 8, 3), (20, 27, 8, 8, 4), (17, 40, 8, 16, 1), (9, 8, 8, 8, 4), (30, 30, 32, 32, 16)]:
        by, bx = brute_axis(H, th, m), brute_axis(W, tw, m)
        rng = np.random.default_rng(H + m)
        windows = [(y, x, 1, 1) for y in range(H) for x in range(W)] + [(0, 0, H, W)]
        for _ in range(200):
            y0, x0 = int(rng.integers(H)), int(rng.integers(W))
            windows.append((y0, x0, int(rng.integers(1, H - y0 + 1)), int(rng.integers(1, W - x0 + 1))))
        for (y0, x0, h, w) in windows:
            ti = {k for Y in range(y0, y0 + h) for (k, _, wt) in by[Y] if wt}
            tj = {k for X in range(x0, x0 + w) for (k, _, wt) in bx[X] if wt}
            want = (min(ti), max(ti) + 1, min(tj), max(tj) + 1)
            assert ti == set(range(want[0], want[1])) and tj == set(range(want[2], want[3]))
            assert overlap.window_tiles_overlap(H, W, th, tw, m, y0, x0, h, w) == want, (H, W, th, tw, m, y0, x0, h, w)
            assert overlap.window_tiles_overlap(H, W, th, tw, 0, y0, x0, h, w) == window_tiles(H, W, th, tw, y0, x0, h, w)
    # one sample left of a four-tile corner needs 2 x 2 tiles where the tiles it meets are one
    assert window_tiles(70, 90, 32, 32, 30, 30, 1, 1) == (0, 1, 0, 1)
    assert overlap.window_tiles_overlap(70, 90, 32, 32, 4, 30, 30, 1, 1) == (0, 2, 0, 2)
    for bad in [(70, 90, 32, 32, 17, 0, 0, 1, 1), (70, 90, 32, 32, 4, 0, 0, 71, 1), (70, 90, 32, 32, 4, 0, 0, 0, 1)]:
        with pytest.raises(ValueError):
            overlap.window_tiles_overlap(*bad)


def test_containers_with_overlap():
    rng = np.random.default_rng(9)
    T = 6  # 20 x 27 in tiles of 8 x 16: 3 x 2
    nbytes = [5, 0, 17, 3, 9, 1]
    run = rng.integers(0, 256, sum(nbytes), dtype=np.uint8).tobytes()
    plain = TiledResult(20, 27, 2, 8, 16, 1, [3, 0, 4, 2, 1, 5], nbytes, run)
    assert plain.overlap == 0 and plain.to_bytes()[:4] == b"SPTL"
    # overlap = 0 writes the bytes of a result built without the field
    assert TiledResult(20, 27, 2, 8, 16, 1, [3, 0, 4, 2, 1, 5], nbytes, run, plain._encoding_version, 0).to_bytes() == plain.to_bytes()
    r = TiledResult(20, 27, 2, 8, 16, 1, [3, 0, 4, 2, 1, 5], nbytes, run, overlap=3)
    data = r.to_bytes()
    assert data[:4] == b"SPOL" and data[4] == 1 and len(data) == len(plain.to_bytes()) + 4
    assert data[24:28] == (3).to_bytes(4, "little") and data[28:] == plain.to_bytes()[24:]
    back = TiledResult.from_bytes(data)
    assert back == r and back.overlap == 3
    e = back.tile(1, 0)
    assert (e.h, e.w, e.c, e.max_n, e.encoded_bytes) == (14, 22, 2, 4, run[5:22])
    assert TiledResult.from_bytes(plain.to_bytes()) == plain
    for bad in [b"SPOX" + data[4:], data[:4] + b"\x02" + data[5:], data[:26], data[:30], data + b"\x00",
                data[:24] + (5).to_bytes(4, "little") + data[28:], data[:24] + (0).to_bytes(4, "little") + data[28:]]:
        with pytest.raises(ValueError):
            TiledResult.from_bytes(bad)
    # layered
    cum = [[2, 0, 5, 1, 4, 0], [5, 0, 17, 3, 9, 1]]
    pieces = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in [2, 0, 5, 1, 4, 0, 3, 0, 12, 2, 5, 1]]
    lplain = LayeredResult(20, 27, 2, 8, 16, None, [3, 0, 4, 2, 1, 5], cum, b"".join(pieces))
    assert lplain.to_bytes()[:4] == b"SPTQ"
    assert LayeredResult(20, 27, 2, 8, 16, None, [3, 0, 4, 2, 1, 5], cum, b"".join(pieces), lplain._encoding_version, 0).to_bytes() \
        == lplain.to_bytes()
    lr = LayeredResult(20, 27, 2, 8, 16, None, [3, 0, 4, 2, 1, 5], cum, b"".join(pieces), overlap=4)
    ldata = lr.to_bytes()
    assert ldata[:4] == b"SPOQ" and ldata[28:32] == (4).to_bytes(4, "little") and ldata[32:] == lplain.to_bytes()[28:]
    assert LayeredResult.from_bytes(ldata) == lr
    assert lr.layer_ends() == [v + 4 for v in lplain.layer_ends()] and lr.layer_ends()[-1] == len(ldata)
    assert lr.tiled().overlap == 4 and lr.tiled(1).overlap == 4 and lr.tiled(1).nbytes == cum[0]
    # every prefix that holds the tables decodes to the clipped tables, as for SPTQ
    head = 32 + 4 * 2 * T + T
    for cutlen in [head, head + 1, lr.layer_ends()[0], lr.layer_ends()[0] + 7, len(ldata) - 1]:
        part = LayeredResult.from_bytes(ldata[:cutlen])
        ref = LayeredResult.from_bytes(lplain.to_bytes()[:cutlen - 4])
        assert part.overlap == 4 and part.cum == ref.cum and part.encoded_bytes == ref.encoded_bytes == ldata[head:cutlen]
    assert LayeredResult.from_bytes(ldata[:lr.layer_ends()[0]]).tiled() == lr.tiled(1)
    for bad in [b"SPOL" + ldata[4:], ldata[:head - 1], ldata[:30], ldata[:28] + (5).to_bytes(4, "little") + ldata[32:],
                ldata[:4] + b"\x02" + ldata[5:], ldata + b"\x00"]:
        with pytest.raises(ValueError):
            LayeredResult.from_bytes(bad)


# ---- the seams, with the oracle's coder --------------------------------------------------------------------------------------
def seam_picture(H, W):
    y, x = np.arange(H)[:, None] / H, np.arange(W)[None, :] / W
    p = 0.5 + 0.25 * np.sin(10.7 * x + 2 * y) * np.cos(5 * y) + 0.1 * np.sin(40 * x * y) \
        + 0.15 * ((x - 0.4) ** 2 + (y - 0.6) ** 2 < 0.05)
    return np.clip(p, 0.0, 1.0)[None]


def seam_step(err, th, tw):
    """the mean absolute jump of err [c, H, W] across the tile boundaries"""
    H, W = err.shape[-2:]
    jumps = [np.abs(err[:, s, :] - err[:, s - 1, :]).ravel() for s in range(th, H, th)]
    jumps += [np.abs(err[:, :, s] - err[:, :, s - 1]).ravel() for s in range(tw, W, tw)]
    return float(np.concatenate(jumps).mean())


def oracle_tiled_decode(P, t, m, total_bits):
    """every coded tile through the oracle's encode_image / decode_image at an equal share of the bits, then the rule's blend"""
    from oracle import oracle as O
    tiles = overlap.cut(P, t, t, m)
    share = total_bits // len(tiles)
    dec = []
    for tile in tiles:
        data, max_n, _ = O.encode_image(np.ascontiguousarray(tile), max_bits=share)
        dec.append(O.decode_image(data, max_n, 1, t + 2 * m, t + 2 * m))
    return overlap.blend(np.stack(dec), P.shape[1], P.shape[2], t, t, m)


@pytest.mark.parametrize("H,W,t,bpp", [(128, 160, 64, 0.5), (70, 90, 32, 1.0)])
def test_cross_fade_halves_the_seam_step(H, W, t, bpp):
    """the seam step of decoded - original with overlap m is below half of the step of hard seams at the same total bits
    (measured with this oracle when the feature was proposed: ratios of 0.10 - 0.22 and 0.18 - 0.29 for these cases)"""
    P = seam_picture(H, W)
    bits = int(H * W * bpp)
    hard = seam_step(oracle_tiled_decode(P, t, 0, bits) - P, t, t)
    for m in (2, 4, 8):
        soft = seam_step(oracle_tiled_decode(P, t, m, bits) - P, t, t)
        print("%d x %d, tiles of %d, %.2f bpp, m = %d: seam step %.4f, without overlap %.4f, ratio %.3f"
              % (H, W, t, bpp, m, soft, hard, soft / hard))
        assert soft < 0.5 * hard, (m, soft, hard)
