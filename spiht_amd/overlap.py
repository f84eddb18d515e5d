"""Overlapping tiles, cross-faded at the seams: the rule (host, numpy) of csrc/overlap.hip, as alloc.py is alloc.hip's.

A tiled picture has tiles of th x tw on the grid gy x gx = tile_grid(H, W, th, tw).  With overlap = m (1 <= m, 2 m <=
min(th, tw)) every tile is coded with a margin of m pixels of its neighbours: coded tile (i, j) is [c, th + 2m, tw + 2m], its
sample (y, x) the picture's sample at row clamp(i th - m + y, 0, H - 1), column clamp(j tw - m + x, 0, W - 1) -- np.pad(mode=
"edge") on all four sides (cut).  The decoder cross-fades the decoded tiles over the 2m-wide strip around each seam (blend).

Along one axis (length n, core t, seams at s = k t for 1 <= k < g): position P lies in the zone of seam s when s - m <= P <
s + m; the zones are disjoint because 2m <= t.  In a zone, u = P - (s - m), tile k has the integer weight a = 2u + 1 and tile
k - 1 the weight b = 4m - a; outside every zone the one tile P // t has the whole weight.  Tile k's sample index for position P
is P - k t + m.  The picture's own borders are not blended, and a zone the picture's end cuts short is simply shorter.

The blend is float64 on the float64 decodes of the tiles, every multiplication, addition and division rounded once (no fused
multiply-add), a and b converted to double exactly: horizontally r = (bx L + ax R) / (4m) in a column zone, else the one
tile's sample; then vertically out = (by r_top + ay r_bottom) / (4m) in a row zone, else r.  8- and 16-bit output: out goes
through the conversion the decoder applies to a float64 sample (convert).
"""
from collections import namedtuple

import numpy as np

AxisPlan = namedtuple("AxisPlan", "zone k0 k1 i0 i1 b a")
AxisPlan.__doc__ = """per position P of one axis, int64 arrays: zone -- P lies in a seam's zone; k0, i0 -- the (first) tile and
its sample index; k1, i1 -- the second tile (the seam's own, k0 + 1) and its sample index, equal to k0, i0 outside the zones;
b, a -- the integer weights of the two, (4m, 0) outside the zones"""


def overlap_arg(m, th, tw):
    """the overlap as an int; ValueError unless 0 <= m and 2 m <= min(th, tw); TypeError for a non-integer"""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
        raise TypeError("overlap must be an integer, not %s" % type(m).__name__)
    m = int(m)
    if m < 0 or 2 * m > min(int(th), int(tw)):
        raise ValueError("overlap = %d of tiles of %d x %d: 0 <= overlap and 2 * overlap <= the shorter tile side" % (m, th, tw))
    return m


def axis_tiles(P, n, t, m):
    """the tiles (k_lo, k_hi) with non-zero weight at position P of an axis of length n in cores of t: both weights of a zone
    are positive (1 <= a <= 4m - 1), so a zone has its two tiles and any other position its one"""
    g = -(-n // t)
    k = (P + m) // t
    if m > 0 and 1 <= k < g and P + m - k * t < 2 * m:
        return k - 1, k
    return P // t, P // t


def axis_plan(n, t, m):
    """AxisPlan of the positions 0 .. n - 1 of an axis in cores of t with overlap m"""
    n, t, m = int(n), int(t), int(m)
    if n < 1 or t < 1 or m < 0 or 2 * m > t:
        raise ValueError("axis_plan(%d, %d, %d)" % (n, t, m))
    g = -(-n // t)
    P = np.arange(n, dtype=np.int64)
    k = (P + m) // t
    u = P + m - k * t
    zone = (k >= 1) & (k < g) & (u < 2 * m)
    k0 = np.where(zone, k - 1, P // t)
    k1 = np.where(zone, k, k0)
    a = np.where(zone, 2 * u + 1, 0)
    return AxisPlan(zone, k0, k1, P - k0 * t + m, P - k1 * t + m, 4 * m - a, a)


def window_tiles_overlap(H, W, th, tw, m, y0, x0, h, w):
    """The sub-grid (i0, i1, j0, j1) of the tiles with non-zero weight somewhere in the window [y0, y0 + h) x [x0, x0 + w):
    window_tiles, widened by the neighbour wherever the window's first or last row / column lies in a seam's zone.  m = 0
    gives window_tiles.  A window that is empty or leaves the picture: ValueError."""
    H, W, th, tw, m = int(H), int(W), int(th), int(tw), int(m)
    y0, x0, h, w = int(y0), int(x0), int(h), int(w)
    if H < 1 or W < 1 or th < 1 or tw < 1 or m < 0 or 2 * m > min(th, tw):
        raise ValueError("a %d x %d picture in tiles of %d x %d with overlap %d" % (H, W, th, tw, m))
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError("the window (%d, %d, %d, %d) is empty or leaves the %d x %d picture" % (y0, x0, h, w, H, W))
    return (axis_tiles(y0, H, th, m)[0], axis_tiles(y0 + h - 1, H, th, m)[1] + 1,
            axis_tiles(x0, W, tw, m)[0], axis_tiles(x0 + w - 1, W, tw, m)[1] + 1)


def cut(picture, th, tw, m):
    """picture [c, H, W] -> the coded tiles [gy * gx, c, th + 2m, tw + 2m], row-major: np.pad(mode="edge") and slicing"""
    picture = np.asarray(picture)
    c, H, W = picture.shape
    gy, gx = -(-H // th), -(-W // tw)
    padded = np.pad(picture, ((0, 0), (m, gy * th - H + m), (m, gx * tw - W + m)), mode="edge")
    return np.stack([padded[:, i * th:(i + 1) * th + 2 * m, j * tw:(j + 1) * tw + 2 * m] for i in range(gy) for j in range(gx)])


def convert(out, dtype):
    """the decoder's conversion of a float64 sample to 8 / 16 bits: clip to [0, 1], times 255 / 65535, truncate, NaN -> 0
    (fmax / fmin return the number of a pair with a NaN)"""
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return np.asarray(out, dtype=np.float64)
    peak = {1: 255.0, 2: 65535.0}[dtype.itemsize]
    return (np.fmin(np.fmax(out, 0.0), 1.0) * peak).astype(np.uint32).astype(dtype)


def blend(tiles, H, W, th, tw, m, window=None, sub=None, dtype=np.float64):
    """tiles: float64 [n, c, rh, rw] (rh >= th + 2m, rw >= tw + 2m), the decodes of the tiles of the sub-grid sub = (i0, i1, j0,
    j1) in row-major order (None: the whole grid) -> the window (y0, x0, h, w) of the picture (None: all of it), [c, h, w] of
    dtype float64, uint8 or uint16.  ValueError if the sub-grid misses a tile with weight in the window.  m = 0: every sample
    from the tile that owns it."""
    tiles = np.asarray(tiles, dtype=np.float64)
    H, W, th, tw, m = int(H), int(W), int(th), int(tw), int(m)
    gy, gx = -(-H // th), -(-W // tw)
    i0, i1, j0, j1 = (0, gy, 0, gx) if sub is None else [int(v) for v in sub]
    y0, x0, h, w = (0, 0, H, W) if window is None else [int(v) for v in window]
    need = window_tiles_overlap(H, W, th, tw, m, y0, x0, h, w)
    if not (0 <= i0 <= need[0] and need[1] <= i1 <= gy and 0 <= j0 <= need[2] and need[3] <= j1 <= gx):
        raise ValueError("the sub-grid %s does not hold the tiles %s of the window" % ((i0, i1, j0, j1), need))
    ni, nj = i1 - i0, j1 - j0
    if tiles.ndim != 4 or tiles.shape[0] != ni * nj or tiles.shape[2] < th + 2 * m or tiles.shape[3] < tw + 2 * m:
        raise ValueError("tiles of shape %s for a sub-grid of %d x %d tiles of %d x %d" % (tiles.shape, ni, nj, th + 2 * m, tw + 2 * m))
    c = tiles.shape[1]
    grid = tiles.reshape((ni, nj) + tiles.shape[1:])
    px, py = axis_plan(W, tw, m), axis_plan(H, th, m)
    xs, ys = slice(x0, x0 + w), slice(y0, y0 + h)
    fm = np.float64(4 * m)
    with np.errstate(all="ignore"):
        # horizontally, per tile row of the sub-grid: r[i] is [c, rh, w]
        bx, ax = px.b[xs].astype(np.float64), px.a[xs].astype(np.float64)
        r = []
        for si in range(ni):
            L = np.moveaxis(grid[si][px.k0[xs] - j0, :, :, px.i0[xs]], 0, -1)
            R = np.moveaxis(grid[si][px.k1[xs] - j0, :, :, px.i1[xs]], 0, -1)
            r.append(np.where(px.zone[xs], (bx * L + ax * R) / fm, L) if m else L)
        r = np.stack(r)  # [ni, c, rh, w]
        # then vertically
        top = np.moveaxis(r[py.k0[ys] - i0, :, py.i0[ys], :], 0, 1)  # [c, h, w]
        if m:
            bot = np.moveaxis(r[py.k1[ys] - i0, :, py.i1[ys], :], 0, 1)
            by, ay = py.b[ys].astype(np.float64)[None, :, None], py.a[ys].astype(np.float64)[None, :, None]
            out = np.where(py.zone[ys][None, :, None], (by * top + ay * bot) / fm, top)
        else:
            out = top
        assert out.shape == (c, h, w)
        return np.ascontiguousarray(convert(out, dtype))
