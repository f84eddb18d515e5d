"""Tiled pictures: one picture as a grid of equal tiles, one SPIHT stream per tile.

A single decode is one workgroup walking one stream; the batched calls code one image per workgroup.  A tiled picture is a
batch of tiles: the picture is cut into gy x gx tiles of th x tw on the device (edge tiles padded by replication, numpy's
np.pad(mode="edge")), the tiles are coded by a BatchCodec(c, th, tw) in one batched call, and the T streams are packed into
one run of bytes with a table of lengths.  Every tile stream is exactly what encode_image gives for that tile's pixels
(TiledResult.tile(i, j) is an ordinary EncodingResult that the reference decodes).  Decoding is the way back -- unpack,
one batched decode, paste -- and a window of the picture needs only the tiles it meets.

The four copies (cut, paste, pack, unpack) are HIP kernels of the library (csrc/tiles.hip, include/spiht_hip.h:
spiht_tile_*); nothing here touches a sample on the host.

allocate="rd" shares the bit budget between the tiles by their rate-distortion curves instead of equally: every tile is coded
past its share, K prefixes of every tile are decoded and measured on the device, and every tile is cut where one more byte
buys the same drop in distortion (alloc.py is the rule, csrc/alloc.hip the kernels).  The container and every decoder are
unchanged: a tile's stream is still encode_image of the tile's pixels, at max_bits = 8 * its length.

Quality layers (encode_layered, LayeredResult): the allocation is run at Q growing budgets on the one table of distortions;
the cuts nest (alloc.allocate_layers), and the container stores for every tile the bytes between consecutive cuts, layer by
layer.  The file through layer q is the whole picture at budget q, and any prefix of the file that holds the tables decodes.
The coder is untouched: two more copies (csrc/layers.hip, spiht_layer_*) put the slots into that order and gather a tile's
pieces back into a decoder slot.

Region of interest (the encode calls' roi=, the device forms' d_roi=): a uint8 weight per pixel position, and allocate="rd"
cuts the tiles by the squared error weighted with it (alloc.roi_arg is the rule, csrc/roi.hip the weighted error sums), so
the bytes -- with layers, the first layers -- go where the caller says the picture matters.  Streams, containers and decoders
are untouched.

Target quality (the encode calls' target_psnr=, the device forms' d_target=): a PSNR in place of a size.  On the same table
allocate="rd" measures, every tile is cut at the hull vertex of the steepest common slope at which the picture's squared error
is at or below the target (alloc.allocate_target is the rule, k_tile_allocate_target the kernel); max_bits stays the cap, and
a target it cannot pay for gives the cut at max_bits.  Layers can be given as PSNRs.  Streams, containers and decoders are
untouched.

Reduced resolution (every decode call's reduce=k; tiled_reduced_shape): the tiles are decoded at 1/2^k size by the batched
reduced decode and assembled into the picture at 1/2^k size by one more copy (k_tile_mosaic, spiht_tile_mosaic_*), which takes
every sample from the centred window of its tile's reduced decode.  It composes with windows (given in the reduced picture's
coordinates) and with quality layers.

Overlapping tiles (the constructor's and the encode calls' overlap=m; overlap.py is the rule, csrc/overlap.hip the kernels): every
tile is coded with a margin of m samples of its neighbours (spiht_tile_cut_overlap_*), and every decode call decodes the tiles in
float64 and cross-fades them over the 2m samples around each seam (spiht_tile_blend_*), so the seams of independent tiles do
not show.  The tile codec is one of slightly larger tiles; the coder, pack / unpack and the layer copies are untouched, results
carry the overlap (containers SPOL / SPOQ), and overlap=0 is the path without it in every byte.
"""
import ctypes as C
import struct
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib, alloc, floatpx, px
from . import overlap as _overlap
from .batch import BatchCodec, DeviceArray
from .spiht_wrapper import ENCODER_DECODER_VERSION, EncodingResult, SpihtSettings, _check_version, _wavelet_mode_ids

MAGIC = b"SPTL"
CONTAINER_VERSION = 1
_HEADER = struct.Struct("<4sBBHIIII")
LAYERED_MAGIC = b"SPTQ"
LAYERED_VERSION = 1
_LAYERED_HEADER = struct.Struct("<4sBBHIIIIHH")
# overlapping tiles (overlap > 0): magics of their own, the same header followed by a u32 overlap, then the same tables and bytes
OVERLAP_MAGIC = b"SPOL"
OVERLAP_LAYERED_MAGIC = b"SPOQ"
OVERLAP_VERSION = 1
_OVERLAP_FIELD = struct.Struct("<I")


def _tile_arg(tile):
    if isinstance(tile, (tuple, list)):
        if len(tile) != 2:
            raise ValueError("tile is an int or (th, tw)")
        return int(tile[0]), int(tile[1])
    return int(tile), int(tile)


def tile_grid(H, W, th, tw):
    """(gy, gx) = (ceil(H / th), ceil(W / tw)): the tiles of an H x W picture, row-major (spiht_tile_grid; no device).
    ValueError for an empty picture or a tile side below 8."""
    gy, gx = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().spiht_tile_grid(int(H), int(W), int(th), int(tw), C.byref(gy), C.byref(gx)))
    return int(gy.value), int(gx.value)


def window_tiles(H, W, th, tw, y0, x0, h, w):
    """The sub-grid (i0, i1, j0, j1) of the tiles that meet the window [y0, y0 + h) x [x0, x0 + w): rows i0 <= i < i1,
    columns j0 <= j < j1.  A window that is empty or leaves the H x W picture: ValueError.  Pure arithmetic; the tile may be
    a reduced one of any side >= 1 (tiled_reduced_shape: Hk, Wk, thk, twk)."""
    H, W, th, tw = int(H), int(W), int(th), int(tw)
    y0, x0, h, w = int(y0), int(x0), int(h), int(w)
    if H < 1 or W < 1 or th < 1 or tw < 1:
        raise ValueError("a %d x %d picture in tiles of %d x %d" % (H, W, th, tw))
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError("the window (%d, %d, %d, %d) is empty or leaves the %d x %d picture" % (y0, x0, h, w, H, W))
    return y0 // th, (y0 + h - 1) // th + 1, x0 // tw, (x0 + w - 1) // tw + 1


def _reduce_arg(reduce):
    """reduce as an int; TypeError for what is no integer (a bool is none)"""
    if isinstance(reduce, bool) or not isinstance(reduce, (int, np.integer)):
        raise TypeError("reduce must be an integer, not %s" % type(reduce).__name__)
    return int(reduce)


_REDUCED_NAMES = ("thk", "twk", "Hk", "Wk", "gy", "gx", "rec_h", "rec_w", "pic_h", "pic_w", "off_y", "off_x")


def tiled_reduced_shape(H, W, tile, settings, level, reduce):
    """Sizes of a tiled picture decoded at 1/2^reduce size (spiht_tile_reduced_grid; no device).  H, W: the picture; tile: an
    int or (th, tw); level: the tile codec's (None: the default of a th x tw picture).  Returns a dict: level -- the levels L
    of a tile's stream; thk, twk = th >> reduce, tw >> reduce -- the reduced tile; Hk, Wk = ceil(H / 2^reduce),
    ceil(W / 2^reduce) -- the reduced picture; gy, gx -- the grid; rec_h, rec_w / pic_h, pic_w -- the float64 / 8- and 16-bit
    reduced decode of one tile (reduced_shape of a th x tw picture); off_y, off_x -- where the tile's own thk x twk samples lie
    in either.  ValueError unless 0 <= reduce <= L and 2^reduce divides th and tw; TypeError for a reduce that is no integer."""
    th, tw = _tile_arg(tile)
    wid, mid = _wavelet_mode_ids(settings if settings is not None else SpihtSettings())
    if level is not None and level < 0:
        raise ValueError("Level value of %d is too low . Minimum level is 0." % level)
    reduce = _reduce_arg(reduce)
    if not 0 <= reduce < 64:
        raise ValueError("reduce = %d" % reduce)
    tile_grid(H, W, th, tw)  # (its own refusals, in its own words)
    lv = C.c_int()
    v = [C.c_int64() for _ in _REDUCED_NAMES]
    try:
        _lib.check(_lib.lib().spiht_tile_reduced_grid(int(H), int(W), th, tw, wid, mid, -1 if level is None else int(level),
                                                      int(reduce), C.byref(lv), *[C.byref(t) for t in v]))
    except ValueError:
        raise ValueError("reduce = %d of a %d x %d picture in tiles of %d x %d: 0 <= reduce <= the tile's levels, and 2^reduce "
                         "divides both tile sides" % (reduce, H, W, th, tw)) from None
    return dict(level=lv.value, **{k: t.value for k, t in zip(_REDUCED_NAMES, v)})


class _Container:
    """What TiledResult and LayeredResult share: the grid, and the header of their containers -- the magic of the form, u8 version,
    u8 level (255 = None), u16 c, u32 H, W, th, tw, then the form's own fields; with overlap = m > 0 the other magic, version
    OVERLAP_VERSION and a u32 m behind the same fields."""

    def grid(self):
        return tile_grid(self.h, self.w, self.th, self.tw)

    def _head(self, header, magic, overlap_magic, version, *more):
        """the writer's side"""
        if self.level is not None and not 0 <= int(self.level) < 255:
            raise ValueError("level %r does not fit the container" % (self.level,))
        fields = (255 if self.level is None else int(self.level), self.c, self.h, self.w, self.th, self.tw) + more
        m = int(self.overlap)
        if m == 0:
            return header.pack(magic, version, *fields)
        if m < 0 or m >= 2 ** 32:
            raise ValueError("overlap %d does not fit the container" % m)
        return header.pack(overlap_magic, OVERLAP_VERSION, *fields) + _OVERLAP_FIELD.pack(m)


def _parse_head(data, header, magic, overlap_magic, known, what):
    """the reader's side: the magic tells the form, whose version is checked -> (level, c, h, w, th, tw and the form's own
    fields, overlap, bytes in front of the tables)"""
    if len(data) < header.size:
        raise ValueError("a %s container has a %d-byte header; got %d bytes" % (what, header.size, len(data)))
    found, version, level, *fields = header.unpack_from(data, 0)
    if found not in (magic, overlap_magic):
        raise ValueError("not a %s container: magic %r" % (what if what == "tiled" else what + " tiled", found))
    fields = [None if level == 255 else level] + fields
    if found == magic:
        if version != known:
            raise ValueError("%s container version %d, this reader knows %d" % (what, version, known))
        return fields, 0, header.size
    if version != OVERLAP_VERSION:
        raise ValueError("%s container with overlap, version %d, this reader knows %d" % (what, version, OVERLAP_VERSION))
    if len(data) < header.size + _OVERLAP_FIELD.size:
        raise ValueError("a %s container with overlap has a %d-byte header; got %d bytes"
                         % (what, header.size + _OVERLAP_FIELD.size, len(data)))
    m, = _OVERLAP_FIELD.unpack_from(data, header.size)
    th, tw = fields[4], fields[5]
    if m < 1 or 2 * m > min(th, tw):
        raise ValueError("overlap = %d of tiles of %d x %d: 1 <= overlap and 2 * overlap <= the shorter tile side" % (m, th, tw))
    return fields, m, header.size + _OVERLAP_FIELD.size


@dataclass
class TiledResult(_Container):
    """The streams of one tiled picture.  h, w, c: the PICTURE; th, tw: the tile; max_n, nbytes: one entry per tile,
    row-major; encoded_bytes: the tiles' streams one behind the other.  overlap = m > 0: every tile was coded with a margin of
    m samples of its neighbours (overlap.py), so a tile's stream is that of a (th + 2m) x (tw + 2m) picture."""
    h: int
    w: int
    c: int
    th: int
    tw: int
    level: Optional[int]
    max_n: List[int]
    nbytes: List[int]
    encoded_bytes: bytes
    _encoding_version: str = ENCODER_DECODER_VERSION
    overlap: int = 0

    def _offsets(self):
        return np.concatenate(([0], np.cumsum(np.asarray(self.nbytes, dtype=np.int64))))

    def tile(self, i, j):
        """Tile (i, j) as an ordinary EncodingResult with h = th + 2 overlap, w = tw + 2 overlap: what encode_image gives for
        the (coded) tile's pixels, and a stream the reference itself decodes."""
        gy, gx = self.grid()
        if not (0 <= i < gy and 0 <= j < gx):
            raise IndexError("tile (%d, %d) of a %d x %d grid" % (i, j, gy, gx))
        t = i * gx + j
        off = self._offsets()
        return EncodingResult(self.encoded_bytes[int(off[t]):int(off[t + 1])], self.th + 2 * self.overlap,
                              self.tw + 2 * self.overlap, self.c, int(self.max_n[t]), self.level, self._encoding_version)

    def to_bytes(self):
        """The container, little-endian: b"SPTL", u8 version = 1, u8 level (255 = None), u16 c, u32 H, W, th, tw, then
        T x u32 nbytes, T x u8 max_n, then the packed streams.  overlap > 0: b"SPOL", version 1, and a u32 overlap behind the
        header; overlap = 0 writes the bytes it always wrote."""
        T = len(self.nbytes)
        if len(self.max_n) != T or sum(self.nbytes) != len(self.encoded_bytes):
            raise ValueError("the tables do not describe %d tiles of %d bytes" % (T, len(self.encoded_bytes)))
        return (self._head(_HEADER, MAGIC, OVERLAP_MAGIC, CONTAINER_VERSION) + np.asarray(self.nbytes, dtype="<u4").tobytes()
                + np.asarray(self.max_n, dtype=np.uint8).tobytes() + bytes(self.encoded_bytes))

    @staticmethod
    def from_bytes(data):
        """Inverse of to_bytes; the magic tells which of the two forms.  ValueError on a wrong magic or version, a short table,
        a length sum that is not the remaining byte count, or an overlap that is 0 or more than half a tile side."""
        data = bytes(data)
        (level, c, h, w, th, tw), m, head = _parse_head(data, _HEADER, MAGIC, OVERLAP_MAGIC, CONTAINER_VERSION, "tiled")
        gy, gx = tile_grid(h, w, th, tw)
        T = gy * gx
        if len(data) < head + 5 * T:
            raise ValueError("the tables of %d tiles need %d bytes; %d are left" % (T, 5 * T, len(data) - head))
        nbytes = np.frombuffer(data, dtype="<u4", count=T, offset=head).astype(np.int64)
        max_n = np.frombuffer(data, dtype=np.uint8, count=T, offset=head + 4 * T)
        rest = len(data) - head - 5 * T
        if int(nbytes.sum()) != rest:
            raise ValueError("the table's lengths add up to %d bytes; %d follow it" % (int(nbytes.sum()), rest))
        return TiledResult(h, w, c, th, tw, level, [int(v) for v in max_n], [int(v) for v in nbytes],
                           data[head + 5 * T:], overlap=m)


@dataclass
class LayeredResult(_Container):
    """The streams of one tiled picture in Q quality layers.  h, w, c, th, tw, level, max_n: as TiledResult; cum [Q][T]:
    cum[q][t] the bytes of tile t through layer q, non-decreasing in q; encoded_bytes: the layers one behind the other,
    layer q being, for t = 0 .. T - 1, the bytes [cum[q - 1][t], cum[q][t]) of tile t's stream (cum[-1] = 0)."""
    h: int
    w: int
    c: int
    th: int
    tw: int
    level: Optional[int]
    max_n: List[int]
    cum: List[List[int]]
    encoded_bytes: bytes
    _encoding_version: str = ENCODER_DECODER_VERSION
    overlap: int = 0

    @property
    def layers(self):
        return len(self.cum)

    def _table(self):
        """(cum [Q][T], piece lengths [Q][T], piece offsets in encoded_bytes [Q][T]) as int64; ValueError if the tables do not
        describe encoded_bytes"""
        T = len(self.max_n)
        cum = np.asarray(self.cum, dtype=np.int64)
        if cum.ndim != 2 or not 1 <= cum.shape[0] <= alloc.MAX_LAYERS or cum.shape[1] != T or T < 1:
            raise ValueError("cum is [Q][T] with 1 <= Q <= %d; got shape %s for %d tiles" % (alloc.MAX_LAYERS, cum.shape, T))
        lens = np.diff(cum, axis=0, prepend=0)
        if (lens < 0).any() or (cum >= 2 ** 32).any():
            raise ValueError("cum must not fall from a layer to the next and must fit 32 bits")
        if int(lens.sum()) != len(self.encoded_bytes):
            raise ValueError("the table's pieces add up to %d bytes; the layers hold %d" % (int(lens.sum()), len(self.encoded_bytes)))
        off = (np.cumsum(lens.reshape(-1)) - lens.reshape(-1)).reshape(lens.shape)
        return cum, lens, off

    def layer_ends(self):
        """the Q lengths of to_bytes() at which each layer is complete: where a server cuts the file"""
        cum, lens, _ = self._table()
        head = _LAYERED_HEADER.size + (_OVERLAP_FIELD.size if self.overlap else 0) + 4 * cum.size + cum.shape[1]
        return [head + int(v) for v in np.cumsum(lens.sum(axis=1))]

    def tiled(self, upto=None):
        """the TiledResult of the first `upto` layers (None: all; 1 <= upto <= Q): tile t is its pieces one behind the other,
        nbytes = cum[upto - 1].  Host-side numpy, for every decoder of a TiledResult and the reference's per-tile decode; the
        device path is TiledCodec.decode_layered."""
        cum, lens, off = self._table()
        upto = _upto_arg(upto, cum.shape[0])
        data = np.frombuffer(self.encoded_bytes, dtype=np.uint8)
        parts = [data[int(off[q, t]):int(off[q, t] + lens[q, t])] for t in range(cum.shape[1]) for q in range(upto)]
        run = np.concatenate(parts) if parts else data[:0]
        return TiledResult(self.h, self.w, self.c, self.th, self.tw, self.level, [int(v) for v in self.max_n],
                           [int(v) for v in cum[upto - 1]], run.tobytes(), self._encoding_version, self.overlap)

    def to_bytes(self):
        """The container, little-endian: b"SPTQ", u8 version = 1, u8 level (255 = None), u16 c, u32 H, W, th, tw, u16 Q, u16 0
        (28 bytes), then Q x T u32 cum (row q tile-major), T x u8 max_n, then the layers.  Every prefix at least
        28 + 4 Q T + T bytes long is a picture (from_bytes).  overlap > 0: b"SPOQ", version 1, and a u32 overlap behind the
        header (32 bytes in front of the tables); the prefix rule is the same."""
        cum, _, _ = self._table()
        return (self._head(_LAYERED_HEADER, LAYERED_MAGIC, OVERLAP_LAYERED_MAGIC, LAYERED_VERSION, cum.shape[0], 0)
                + cum.astype("<u4").tobytes() + np.asarray(self.max_n, dtype=np.uint8).tobytes() + bytes(self.encoded_bytes))

    @staticmethod
    def from_bytes(data):
        """Inverse of to_bytes, of the file or of a PREFIX of it that holds header and tables.  With a < total stream bytes
        behind the tables the table is clipped: the piece (q, t) at stream offset o of length l keeps clamp(a - o, 0, l)
        bytes and cum'[q][t] = cum'[q - 1][t] + kept; Q stays (absent layers are empty).  The result is an ordinary
        LayeredResult.  ValueError: wrong magic or version, fewer bytes than header and tables, a table that falls from a
        layer to the next, more bytes than the table accounts for."""
        data = bytes(data)
        (level, c, h, w, th, tw, Q, _), m, tables = _parse_head(data, _LAYERED_HEADER, LAYERED_MAGIC, OVERLAP_LAYERED_MAGIC,
                                                                 LAYERED_VERSION, "layered")
        if not 1 <= Q <= alloc.MAX_LAYERS:
            raise ValueError("a layered container has 1 .. %d layers, not %d" % (alloc.MAX_LAYERS, Q))
        gy, gx = tile_grid(h, w, th, tw)
        T = gy * gx
        head = tables + 4 * Q * T + T
        if len(data) < head:
            raise ValueError("header and tables of %d layers of %d tiles are %d bytes; got %d" % (Q, T, head, len(data)))
        cum = np.frombuffer(data, dtype="<u4", count=Q * T, offset=tables).astype(np.int64).reshape(Q, T)
        max_n = np.frombuffer(data, dtype=np.uint8, count=T, offset=tables + 4 * Q * T)
        lens = np.diff(cum, axis=0, prepend=0)
        if (lens < 0).any():
            raise ValueError("the table falls from a layer to the next")
        a, total = len(data) - head, int(lens.sum())
        if a > total:
            raise ValueError("the table's pieces add up to %d bytes; %d follow it" % (total, a))
        if a < total:
            flat = lens.reshape(-1)
            off = np.cumsum(flat) - flat
            cum = np.cumsum(np.clip(a - off, 0, flat).reshape(Q, T), axis=0)
        return LayeredResult(h, w, c, th, tw, level, [int(v) for v in max_n],
                             [[int(v) for v in row] for row in cum], data[head:], overlap=m)


def _upto_arg(upto, Q):
    if upto is None:
        return Q
    if isinstance(upto, bool) or not isinstance(upto, (int, np.integer)):
        raise TypeError("upto must be an integer or None, not %s" % type(upto).__name__)
    if not 1 <= upto <= Q:
        raise ValueError("upto = %d: 1 .. %d layers" % (upto, Q))
    return int(upto)


@dataclass
class TileCurves:
    """What allocate="rd" measured of one picture, one row per tile: lengths [T][K + 1] -- the candidate byte lengths
    alloc.tile_lengths(nbytes[t], K); sse [T][K + 1] -- the squared error of the tile's valid region at each, summed over the
    channels: float64, or uint64 (exact) for 8- / 16-bit pixels; nbytes [T] -- the full streams; max_n [T] -- start planes."""
    lengths: List[List[int]]
    sse: np.ndarray
    nbytes: List[int]
    max_n: List[int]


@dataclass
class TileAllocation:
    """the cut of one picture: lam -- lambda*, the drop in squared error per byte every tile was cut at (inf: the budget lies
    below every tile's first hull edge); nbytes -- the bytes per tile.  Of a call with target_psnr: met -- the target was
    reached within max_bits; dist -- the (weighted) squared error of the picture at the cut, the table's sum in the order of
    alloc.total_distortion, and psnr -- its PSNR in dB; both None where the budget bound, since a tile cut inside a hull edge
    was never measured there.  All three are None for a call without a target."""
    lam: float
    nbytes: List[int]
    dist: Optional[float] = None
    psnr: Optional[float] = None
    met: Optional[bool] = None


def _alloc_args(allocate, points, spread, max_bits, pixel_dtype):
    """the host checks of the three keywords, before a context is asked for"""
    alloc.allocate_arg(allocate)
    points, spread = alloc.points_arg(points), alloc.spread_arg(spread)
    if allocate is not None:
        if max_bits is None:
            raise ValueError('allocate="rd" shares a budget: max_bits is required')
        if np.dtype(pixel_dtype) in (np.float32, np.float16):
            raise ValueError('allocate="rd" takes the pictures of a float64 codec')
    return points, spread


def _ptr(x):
    """the device address of a DeviceArray, or the integer itself"""
    return int(x.ptr) if hasattr(x, "ptr") else int(x)


# the element type of a tile call is a px.Elem: of_dtype of a DeviceArray's dtype, float_elem(dtype) for the float kinds.
# float pixels out and in: a tile batch of a kind is copied as elements of its size -- both 16-bit kinds by the uint16 copies,
# float32 by the strided 4-byte ones; the blend rounds to the kind at its store, the error sums widen the original's samples
_FLOAT_COPY = {("spiht_tile_paste_", 2): "spiht_tile_paste_u16", ("spiht_tile_paste_", 4): "spiht_tile_paste_f32s",
               ("spiht_tile_mosaic_", 2): "spiht_tile_mosaic_u16", ("spiht_tile_mosaic_", 4): "spiht_tile_mosaic_f32",
               ("spiht_tile_cut_", 2): "spiht_tile_cut_u16", ("spiht_tile_cut_", 4): "spiht_tile_cut_f32s",
               ("spiht_tile_cut_overlap_", 2): "spiht_tile_cut_overlap_u16",
               ("spiht_tile_cut_overlap_", 4): "spiht_tile_cut_overlap_f32s"}
_FLOAT_KIND_CALL = ("spiht_tile_blend_", "spiht_sse_tiles_", "spiht_sse_tiles_w_")  # entry points that take the kind


def _entry(L, stem, dt):
    """the library's entry point of a tile stem for an element type (px.Elem.entry: (L, "spiht_tile_paste_", px.U16) ->
    L.spiht_tile_paste_u16), with the one rule that is the tiles' own: a tile batch of a float kind is copied by its element
    size; only the blend into the kind and the error sums of tiles of the kind are *_flt calls"""
    if dt.kind is not None and stem not in _FLOAT_KIND_CALL:
        return getattr(L, _FLOAT_COPY[stem, dt.itemsize])
    return dt.entry(L, stem)


class TiledCodec:
    """encode / decode pictures [c, H, W] as tiles of `tile` = th x tw (an int or (th, tw), sides >= 8).

    settings / level / max_bits have the meaning of encode_image for EVERY TILE: level=None is the default level of a th x tw
    picture, each tile's bit budget is max_bits // T (None stays None), and whatever encode_image refuses for a th x tw
    picture is refused here, in the constructor.  The colour model change is per pixel and happens inside the tile codec.
    pixel_dtype float32: the encoder runs PyWavelets' single-precision arithmetic, as encode_image does for float32 pixels.

    allocate="rd" (max_bits required; not for a float32 codec): the tiles share max_bits by their rate-distortion curves.
    Every tile is coded with the ceiling alloc.ceiling_bits(max_bits, T, spread), measured at `points` prefixes and cut at
    equal slope (alloc.allocate); the lengths add up to max_bits // 8 whenever the tiles' hulls can take that much.
    max_bytes (an attribute) bounds the device memory of the prefixes decoded at a time; results do not depend on it.

    overlap = m > 0 (2 m <= min(th, tw); overlap.py is the rule, csrc/overlap.hip the kernels): every tile is coded with a margin
    of m samples of its neighbours -- coded tile (i, j) is the picture's rows i th - m .. (i + 1) th + m and columns j tw - m ..
    (j + 1) tw + m, clamped to the picture (np.pad(mode="edge") on all four sides) -- and every decode call cross-fades the
    decoded tiles over the 2m samples around each seam.  The tile codec is one of (th + 2m) x (tw + 2m) pictures, whose level
    and refusals hold; a tile's stream is still encode_image of the (coded) tile's pixels, and the budgets are unchanged
    (max_bits // T per tile, or the ceiling of allocate="rd").  Every decode call decodes the tiles in float64 and blends once;
    8- and 16-bit output is the decoder's conversion of the blended float64 sample.  A window needs the tiles with weight in
    it (overlap.window_tiles_overlap): one more row or column of them where it begins or ends inside a seam's zone.
    allocate="rd" and the layers measure the error of the CODED tiles -- margins and padding included, every tile's whole
    extent -- not of the blended picture.  Out of scope with overlap > 0, each a ValueError: roi / d_roi, target_psnr /
    d_target, reduce > 0 and tile_curves(roi=...).  overlap = 0 is the codec without it in every byte."""

    overlap = 0

    def __init__(self, c, H, W, tile, settings=None, level=None, max_bits=None, ctx=None, pixel_dtype=np.float64, allocate=None,
                 points=alloc.POINTS, spread=alloc.SPREAD, overlap=0):
        self.settings = settings if settings is not None else SpihtSettings()
        if self.settings.color_model not in (None, "RGB"):
            pixel_dtype = np.float64  # as encode_image: colour pictures are coded in float64
        self.points, self.spread = _alloc_args(allocate, points, spread, max_bits, pixel_dtype)
        self.allocate = allocate
        self.c, self.H, self.W = int(c), int(H), int(W)
        self.th, self.tw = _tile_arg(tile)
        self.gy, self.gx = tile_grid(self.H, self.W, self.th, self.tw)
        self.T = self.gy * self.gx
        self.overlap = _overlap.overlap_arg(overlap, self.th, self.tw)
        self.cth, self.ctw = self.th + 2 * self.overlap, self.tw + 2 * self.overlap  # the coded tile
        self.level = level
        self.max_bits = max_bits
        if allocate is not None:
            tile_bits = alloc.ceiling_bits(max_bits, self.T, self.spread)
        else:
            tile_bits = None if max_bits is None else int(max_bits) // self.T
        self.codec = BatchCodec(self.c, self.cth, self.ctw, self.settings, level, tile_bits, ctx, pixel_dtype)
        self.ctx, self.L = self.codec.ctx, self.codec.L
        self.pixel_dtype = self.codec.pixel_dtype
        self.last_tiles_decoded = 0  # tiles the last decode call ran
        self.last_allocation = None  # allocate="rd": the TileAllocation of the last host encode (a list for several pictures)
        self.max_bytes = 2 ** 31     # allocate="rd": device bytes of the prefixes decoded at a time
        self._bufs = {}
        self._reduced = {}           # reduce -> tiled_reduced_shape

    # ---- device scratch, grow-only per name ------------------------------------------------------
    def _buf(self, name, nbytes):
        b = self._bufs.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self._bufs[name] = DeviceArray(self.ctx, (int(nbytes) + int(nbytes) // 4 + 16,), np.uint8)
        return b

    def close(self):
        for b in self._bufs.values():
            b.free()
        self._bufs = {}

    def _download(self, ptr, shape, dtype):
        """a host array of that shape, filled from the device address: one download (none of an empty array)"""
        out = np.empty(shape, dtype=dtype)
        if out.size:
            self.ctx.download(out, ptr)
        return out

    def _download_cuts(self, s, Q, N, target):
        """what _allocate_device left of the last device encode: [lambda* [Q][N]]; of a cut at a target also the errors reached
        and whether each was met.  s: as _allocate_device's"""
        names = ("lambda", np.float64), ("tdist", np.float64), ("tmet", np.uint32)
        return [self._download(self._bufs[k + s].ptr, (Q, N), t) for k, t in names[:3 if target else 1]]

    # ---- overlapping tiles: what is out of scope with them ------------------------------------------
    def _overlap_refuses(self, name, roi=None, target=None, reduce=0):
        """ValueError for what a codec of overlapping tiles does not do, before anything is uploaded or queued"""
        if not self.overlap:
            return
        if roi is not None:
            raise ValueError("%s: a weight map is not supported with overlap > 0: the map is indexed in picture coordinates, and a "
                             "coded tile's margin lies in its neighbours" % name)
        if target is not None:
            raise ValueError("%s: a target quality is not supported with overlap > 0: overlapping tiles count pixels twice, so the "
                             "sum of the tiles' errors is not the picture's" % name)
        if reduce > 0:
            raise ValueError("%s: reduce = %d is not supported with overlap > 0: a reduced decode has no cross-fade" % (name, reduce))

    # ---- device-resident forms ---------------------------------------------------------------------
    # ---- region of interest ----------------------------------------------------------------------
    def _roi_check(self, dtype, name):
        """what a call with a weight map needs of the codec, before anything is uploaded or queued"""
        if self.allocate is None:
            raise ValueError('%s: a weight map steers allocate="rd"; the codec was not built with it' % name)
        if px.of_dtype(dtype).integer and self.c * self.th * self.tw > alloc.ROI_MAX_TILE_SAMPLES:
            raise ValueError("%s: the exact weighted sum of integer pixels takes tiles of c * th * tw <= 2^24 samples, not %d"
                             % (name, self.c * self.th * self.tw))

    def _roi_device(self, d_roi, roi_stride, dtype, name):
        """the device map of a device form -> None, or (address, bytes from one picture's map to the next)"""
        if d_roi is None:
            return None
        self._roi_check(dtype, name)
        roi_stride = int(roi_stride)
        if roi_stride != 0 and roi_stride < self.H * self.W:
            raise ValueError("%s: roi_stride = %d: 0 (one map for all pictures) or at least H * W = %d"
                             % (name, roi_stride, self.H * self.W))
        return _ptr(d_roi), roi_stride

    def _roi_upload(self, roi, N):
        """the host map of a host form -> (d_roi, roi_stride) for the device form: one upload"""
        if roi is None:
            return None, 0
        roi = alloc.roi_arg(roi, N, self.H, self.W)
        d_roi = self._buf("roi", roi.nbytes)
        self.ctx.upload(d_roi.ptr, roi)
        return d_roi, 0 if roi.ndim == 2 else self.H * self.W

    # ---- target quality ----------------------------------------------------------------------------
    def _target_check(self, name):
        if self.allocate is None:
            raise ValueError('%s: a target quality is reached by allocate="rd"; the codec was not built with it' % name)

    def _weight_sums(self, roi, N):
        """the sum of the weights of each of the N pictures as Python ints: H * W without a map"""
        if roi is None:
            return [self.H * self.W] * N
        roi = alloc.roi_arg(roi, N, self.H, self.W)
        if roi.ndim == 2:
            return [int(roi.sum(dtype=np.int64))] * N
        return [int(roi[n].sum(dtype=np.int64)) for n in range(N)]

    def _targets_upload(self, rows, sums, dtype):
        """rows: Q lists of N target PSNRs; sums: the N weight sums -> the device double [Q][N] of squared errors, in the buffer
        "targets": one upload"""
        peak = px.of_dtype(dtype).peak
        table = np.array([[alloc.target_sqerr(db, peak, self.c, s) for db, s in zip(row, sums)] for row in rows], dtype=np.float64)
        d_target = self._buf("targets", table.nbytes)
        self.ctx.upload(d_target.ptr, table)
        return d_target

    def _allocation(self, lam, nbytes, target=None):
        """the TileAllocation of a cut; target: (dist, met, the picture's weight sum, pixel dtype) of a cut at a target, dist NaN
        where the budget bound"""
        if target is None:
            return TileAllocation(float(lam), nbytes)
        from .rd import psnr_of
        dist, met, weight_sum, dtype = target
        if np.isnan(dist):
            return TileAllocation(float(lam), nbytes, None, None, bool(met))
        return TileAllocation(float(lam), nbytes, float(dist), psnr_of(float(dist) / (self.c * weight_sum), px.of_dtype(dtype).peak),
                              bool(met))

    def encode_device(self, d_img, N, d_packed, d_lens, d_max_n, strides=None, d_roi=None, roi_stride=0, d_target=None):
        """d_img: DeviceArray of N pictures [N, c, H, W] -- float64 (float32 for a float32 codec), or uint8 / uint16 laid out by
        `strides` (bytes (sb, sc, sh, sw); None: dense CHW).  -> d_packed: the N * T streams one behind the other (uint8, at
        least N * T * codec.slot_stride bytes always suffice; nothing is written past the array), d_lens: uint32 [N * T] their
        lengths, d_max_n: uint8 [N * T].  Picture n's tiles are rows [n * T, (n + 1) * T).  One cut, one batched encode, one
        pack, queued on the codec's context.  allocate="rd": between the encode and the pack, per group of candidate lengths,
        the prefix slots, one batched decode of them and the per-tile error sums; then one spiht_tile_allocate, whose lengths
        the pack takes.  No host wait anywhere.
        d_roi (allocate="rd" codecs; otherwise ValueError): a device weight map, uint8 [H, W] for all pictures (roi_stride 0)
        or [N, H, W] with roi_stride >= H * W bytes from one picture's map to the next, at any address.  The error sums are
        then the weighted ones (spiht_sse_tiles_w_*; alloc.roi_arg has the rule); nothing else in the path changes.
        d_target (allocate="rd" codecs; otherwise ValueError): a device double [N], per picture the squared error of the whole
        picture to reach (alloc.target_sqerr; with a weight map, the weighted error -- a caller with a device map computes its
        own).  spiht_tile_allocate_target then takes the place of spiht_tile_allocate: one launch for one launch, max_bits the
        cap (alloc.allocate_target); lambda, the error reached and whether the target was met stay in the buffers "lambda",
        "tdist" (double [N], NaN where the budget bound) and "tmet" (uint32 [N])."""
        N, vp = int(N), C.c_void_p
        self._overlap_refuses("encode_device", d_roi, d_target)
        if d_target is not None:
            self._target_check("encode_device")
        roi = self._roi_device(d_roi, roi_stride, d_img.dtype, "encode_device")
        dt, d_tiles, d_slots, d_nbits = self._encode_slots(d_img, N, d_max_n, strides, "encode_device")
        NT, stride = N * self.T, self.codec.slot_stride
        if self.allocate is not None:
            d_nbits = self._allocate_device(dt, N, d_tiles, d_slots, d_nbits, d_max_n, roi, [int(self.max_bits)], d_target)
        _lib.check(self.L.spiht_tile_pack(self.ctx.handle, vp(d_slots.ptr), stride, vp(d_nbits.ptr), NT, vp(d_packed.ptr),
                                          d_packed.nbytes, vp(d_lens.ptr)))

    def _encode_slots(self, d_img, N, d_max_n, strides, name):
        """the cut and the batched encode of the N * T tiles -> (element type, the buffers of the tiles, the stream slots and
        the streams' lengths in bits)"""
        N = int(N)
        dt = px.of_dtype(d_img.dtype)  # (float pixels in: a view of the kind, cut as elements of its size)
        NT, vp = N * self.T, C.c_void_p
        if N < 1:
            raise ValueError("%s: no pictures" % name)
        d_tiles = self._buf("tiles", NT * self.c * self.cth * self.ctw * dt.itemsize)
        geom = (N, self.c, self.H, self.W, self.th, self.tw)
        # overlap > 0: the cut with a margin (spiht_tile_cut_overlap_*: the tile's arguments, then m)
        stem = "spiht_tile_cut_"
        if self.overlap:
            geom, stem = geom + (self.overlap,), "spiht_tile_cut_overlap_"
        view = ()  # the integer forms and the float kinds take a view of the pictures: the strides, behind the address
        if dt.view:
            st, st_p = dt.strides_arg((N, self.c, self.H, self.W), strides, False)
            dt.check_aligned(d_img.ptr)
            view = (st_p,)
        elif dt.storage != self.pixel_dtype or strides is not None:
            raise ValueError("%s: %s pictures, the codec's are dense %s" % (name, dt.storage.name, self.pixel_dtype.name))
        _lib.check(_entry(self.L, stem, dt)(self.ctx.handle, vp(d_img.ptr), *view, *geom, vp(d_tiles.ptr)))
        d_slots = self._buf("slots", NT * self.codec.slot_stride)
        d_nbits = self._buf("nbits", NT * 8)
        self.codec._encode_device(dt, d_tiles.ptr, NT, d_slots.ptr, d_nbits.ptr, d_max_n.ptr)
        return dt, d_tiles, d_slots, d_nbits

    def _allocate_device(self, dt, N, d_tiles, d_slots, d_nbits, d_max_n, roi, budgets, d_target=None, s=""):
        """the NT full streams in d_slots -> the buffer of the cut lengths in bits (uint64 [Q][NT]), one row per budget (in bits)
        of `budgets`, each row one spiht_tile_allocate on the one table of distortions; the table stays in the buffer "D"
        ([K + 1][NT]) and the rows' lambda* in "lambda" ([Q][N]) for the host forms.  d_target (double [Q][N]): row q is the cut at
        the target squared errors of its row q under the cap budgets[q], whose further outputs stay in "tdist" and "tmet"
        ([Q][N] each).  s = "s" gives the four buffers the layered form's names: "cuts", "lambdas", "tdists" and "tmets"."""
        NT, Q, vp = N * self.T, len(budgets), C.c_void_p
        d_D = self._measure_device(dt, N, d_tiles, d_slots, d_nbits, d_max_n, roi)
        d_cut = self._buf("cut" + s, Q * NT * 8)
        d_lam = self._buf("lambda" + s, Q * N * 8)
        if d_target is not None:
            d_dist, d_met = self._buf("tdist" + s, Q * N * 8), self._buf("tmet" + s, Q * N * 4)
        args = (self.ctx.handle, vp(d_nbits.ptr), vp(d_D.ptr), 1 if dt.integer else 0, self.points, N, self.T)
        for q, bits in enumerate(budgets):
            cut, lam = vp(d_cut.ptr + 8 * q * NT), vp(d_lam.ptr + 8 * q * N)
            if d_target is None:
                _lib.check(self.L.spiht_tile_allocate(*args, bits // 8, cut, lam))
            else:
                _lib.check(self.L.spiht_tile_allocate_target(*args, bits // 8, vp(_ptr(d_target) + 8 * q * N), cut, lam,
                                                             vp(d_dist.ptr + 8 * q * N), vp(d_met.ptr + 4 * q * N)))
        return d_cut

    def _measure_device(self, dt, N, d_tiles, d_slots, d_nbits, d_max_n, roi=None):
        """the NT full streams in d_slots -> the buffer "D": float64 / uint64 [K + 1][NT], the error of every tile at its K + 1
        candidate lengths; roi = (address, stride) of a device weight map: the weighted error.  overlap > 0: the error of the
        CODED tiles, margins and padding included -- the sums are taken with the geometry of a picture of gy x gx whole coded
        tiles, in which every tile's valid extent is the whole tile -- not the error of the blended picture.  Tiles of a float
        kind (float pixels in) are measured against float64 decodes, their samples widened in the sums (spiht_sse_tiles_flt)"""
        NT, K, vp, c = N * self.T, self.points, C.c_void_p, self.c
        stride = self.codec.slot_stride
        tile_dt = dt
        if dt.kind is not None:
            dt = px.F64  # (the decodes' element)
        integer = dt.integer
        rh, rw = (self.cth, self.ctw) if integer else (self.codec.geom["rec_h"], self.codec.geom["rec_w"])
        H, W = (self.gy * self.cth, self.gx * self.ctw) if self.overlap else (self.H, self.W)
        G = max(1, min(K + 1, int(self.max_bytes) // (NT * (stride + c * rh * rw * dt.itemsize + 9))))
        d_pre = self._buf("pre", G * NT * stride)
        d_prebytes = self._buf("prebytes", G * NT * 8)
        d_premaxn = self._buf("premaxn", G * NT)
        d_dec = self._buf("dec", G * NT * c * rh * rw * dt.itemsize)
        d_D = self._buf("D", (K + 1) * NT * 8)
        if roi is None:
            sse, w_args = _entry(self.L, "spiht_sse_tiles_", tile_dt), ()
        else:
            sse, w_args = _entry(self.L, "spiht_sse_tiles_w_", tile_dt), (vp(roi[0]), roi[1])
        for k0 in range(0, K + 1, G):
            g = min(G, K + 1 - k0)
            _lib.check(self.L.spiht_tile_prefix_slots(self.ctx.handle, vp(d_slots.ptr), stride, vp(d_nbits.ptr), NT, K, k0, g,
                                                      vp(d_pre.ptr), stride, vp(d_prebytes.ptr), vp(d_max_n.ptr), vp(d_premaxn.ptr)))
            self.codec._decode_device(dt, d_pre.ptr, d_prebytes.ptr, d_premaxn.ptr, g * NT, d_dec.ptr, slot_stride=stride)
            _lib.check(sse(self.ctx.handle, vp(d_tiles.ptr), vp(d_dec.ptr), g, N, c, H, W, self.cth, self.ctw, rh, rw,
                           vp(d_D.ptr + 8 * k0 * NT), *w_args))
        return d_D

    def encode_layered_device(self, d_img, N, layers, d_packed, d_cum, d_max_n, d_pic_bytes, strides=None, d_roi=None,
                              roi_stride=0, target_psnr=None, d_target=None):
        """encode_device in Q quality layers (allocate="rd" codecs; layers: alloc.layer_budgets(max_bits, layers)).  d_img, N,
        d_max_n, strides: as encode_device.  -> d_packed: picture n's layers behind picture n - 1's, inside a picture layer by
        layer and tile by tile (N * T * codec.slot_stride bytes always suffice; nothing is written past the array); d_cum: uint32
        [N][Q][T], the bytes of every tile through every layer; d_pic_bytes: uint64 [N], the pictures' lengths in d_packed.
        What encode_device queues up to the table of distortions, then Q spiht_tile_allocate on that one table -- the cuts
        stay in the buffers "cuts" (bits, uint64 [Q][N * T]) and "lambdas" ([Q][N]) -- then one spiht_layer_pack.  No host
        wait anywhere.  The last layer's cut is encode_device's.  Returns Q.
        d_roi, roi_stride: a device weight map, as encode_device; the first layers then hold the bytes of the tiles it favours.
        target_psnr: the layers as Q strictly increasing PSNRs in dB in place of budgets (layers is then None or Q): layer q is
        the cut of spiht_tile_allocate_target at target q under the cap max_bits // 8 (alloc.allocate_target_layers: the rows
        nest), and a layer whose target the cap cannot pay for repeats the cut at the cap.  The squared errors are
        alloc.target_sqerr of the unweighted picture, uploaded once; or d_target, a device double [Q][N] of them, which a call
        with d_roi must give (the weights' sums are the caller's).  "tdists" (double [Q][N]) and "tmets" (uint32 [Q][N]) keep
        the errors reached and whether each target was met."""
        if self.allocate is None:
            raise ValueError('encode_layered: the codec was not built with allocate="rd"')
        self._overlap_refuses("encode_layered_device", d_roi, target_psnr if target_psnr is not None else d_target)
        N, vp = int(N), C.c_void_p
        if target_psnr is None:
            if d_target is not None:
                raise ValueError("encode_layered_device: d_target goes with target_psnr, the layers' PSNRs")
            budgets = alloc.layer_budgets(self.max_bits, layers)
            Q = len(budgets)
        else:
            dbs = alloc.layer_targets_arg(target_psnr, layers)
            Q = len(dbs)
            budgets = [int(self.max_bits)] * Q  # every layer's cap
            if d_target is None and d_roi is not None:
                raise ValueError("encode_layered_device: with a device weight map, give the weighted squared errors as d_target")
        roi = self._roi_device(d_roi, roi_stride, d_img.dtype, "encode_layered_device")
        if target_psnr is not None and d_target is None:
            if N < 1:
                raise ValueError("encode_layered_device: no pictures")
            d_target = self._targets_upload([[db] * N for db in dbs], self._weight_sums(None, N), d_img.dtype)
        dt, d_tiles, d_slots, d_nbits = self._encode_slots(d_img, N, d_max_n, strides, "encode_layered_device")
        d_cuts = self._allocate_device(dt, N, d_tiles, d_slots, d_nbits, d_max_n, roi, budgets, d_target, "s")
        _lib.check(self.L.spiht_layer_pack(self.ctx.handle, vp(d_slots.ptr), self.codec.slot_stride, vp(d_cuts.ptr), Q, N, self.T,
                                           vp(_ptr(d_packed)), int(d_packed.nbytes), vp(_ptr(d_cum)), vp(_ptr(d_pic_bytes))))
        return Q

    def reduced_shape(self, reduce):
        """tiled_reduced_shape of the codec's pictures: TypeError / ValueError for a reduce the codec does not decode at"""
        reduce = _reduce_arg(reduce)  # (a reduce of another type is refused here, before it becomes a key)
        self._overlap_refuses("decode", reduce=reduce)
        if self.overlap and reduce == 0:
            # (full size: the picture and the grid; the levels are the coded tile's, which tiled_reduced_shape does not know)
            return dict(level=self.level, thk=self.th, twk=self.tw, Hk=self.H, Wk=self.W, gy=self.gy, gx=self.gx)
        rs = self._reduced.get(reduce)
        if rs is None:
            rs = self._reduced[reduce] = tiled_reduced_shape(self.H, self.W, (self.th, self.tw), self.settings, self.level, reduce)
        return rs

    def _window_arg(self, window, rs):
        """None: the whole (reduced) picture"""
        return (0, 0, rs["Hk"], rs["Wk"]) if window is None else tuple(int(v) for v in window)

    def _window_tiles(self, rs, y0, x0, h, w):
        """the sub-grid a window needs: the tiles it meets, or with overlap > 0 those with weight in it"""
        if self.overlap:
            return _overlap.window_tiles_overlap(self.H, self.W, self.th, self.tw, self.overlap, y0, x0, h, w)
        return window_tiles(rs["Hk"], rs["Wk"], rs["thk"], rs["twk"], y0, x0, h, w)

    def _sub_window(self, sub, window, rs):
        i0, i1, j0, j1 = [int(v) for v in sub]
        y0, x0, h, w = [int(v) for v in window]
        need = self._window_tiles(rs, y0, x0, h, w)
        if not (0 <= i0 <= need[0] and need[1] <= i1 <= self.gy and 0 <= j0 <= need[2] and need[3] <= j1 <= self.gx):
            raise ValueError("the sub-grid %s does not hold the tiles %s of the window %s" % ((i0, i1, j0, j1), need, (y0, x0, h, w)))
        return (i0, i1, j0, j1), (y0, x0, h, w)

    def decode_window_device(self, d_packed, packed_bytes, d_lens, d_max_n, sub, window, d_out, strides=None, slot_stride=None,
                             reduce=0):
        """d_packed / d_lens / d_max_n: the streams, lengths (uint32) and start planes (uint8) of the tiles of the sub-grid
        sub = (i0, i1, j0, j1) in row-major order -- only those are unpacked and decoded.  window = (y0, x0, h, w) inside the
        picture and inside the sub-grid.  -> d_out: DeviceArray [c, h, w], float64, or uint8 / uint16 laid out by `strides`
        (bytes (sc, sh, sw); None: dense CHW; what lies between the view's samples is not written); float pixels out: an
        object with .ptr and .dtype = float_elem(dtype), laid out by `strides` the same way.  slot_stride: bytes per
        stream slot the streams are unpacked into, a multiple of 4 no stream is longer than (None: the codec's bound).
        One unpack, one batched decode, one paste, queued on the codec's context.
        Streams of an allocate="rd" encoder: a tile may be longer than the bound of an equal-split codec, and
        spiht_tile_unpack takes a length as at most slot_stride -- the tile would be cut short.  Pass slot_stride >= the longest
        length of d_lens (the host forms size the slots by the longest stream already).
        reduce = k > 0 (0 <= k <= the tile's levels, 2^k dividing th and tw; reduced_shape(k) gives the sizes): the picture at
        1/2^k size, [c, Hk, Wk].  The window is in ITS coordinates and the tiles are those it meets in the thk x twk grid;
        sample (Y, X) is the reduced decode of its tile (decode_image_reduced*(result.tile(i, j), settings, k, crop=True)).
        The same unpack, one batched reduced decode, one mosaic (spiht_tile_mosaic_*); reduce = 0 is the paste above."""
        rs = self.reduced_shape(reduce)
        (i0, i1, j0, j1), (y0, x0, h, w) = self._sub_window(sub, self._window_arg(window, rs), rs)
        n, vp = (i1 - i0) * (j1 - j0), C.c_void_p
        stride = self.codec.slot_stride if slot_stride is None else int(slot_stride)
        d_slots = self._buf("slots", n * stride)
        d_nbytes = self._buf("nbytes", n * 8)
        _lib.check(self.L.spiht_tile_unpack(self.ctx.handle, vp(_ptr(d_packed)), int(packed_bytes), vp(_ptr(d_lens)), n,
                                            vp(d_slots.ptr), stride, vp(d_nbytes.ptr)))
        self._decode_slots(d_slots, d_nbytes, _ptr(d_max_n), stride, (i0, i1, j0, j1), (y0, x0, h, w), d_out, strides, rs, reduce)

    def _decode_slots(self, d_slots, d_nbytes, max_n, stride, sub, window, d_out, strides, rs, reduce):
        """the zero-padded slots of the sub-grid's tiles -> the window: one batched decode, one paste (reduce > 0: one batched
        reduced decode, one mosaic; overlap > 0, every element type: one batched float64 decode of the coded tiles, one blend,
        which converts the blended sample for 8- and 16-bit output and rounds it for a float kind).  A float kind goes
        the integer kinds' way: the tiles' *_float decode into a dense tile batch of the kind, cropped as theirs, then a copy"""
        (i0, i1, j0, j1), (y0, x0, h, w) = sub, window
        n, vp, k = (i1 - i0) * (j1 - j0), C.c_void_p, int(reduce)
        dt = px.of_dtype(d_out.dtype)
        integer = dt.view  # (a view of the output, tiles cropped to the picture's samples)
        # the plan: the element type of the batched decode's tiles, rh x rw of one decoded tile, the call that assembles them
        # and the geometry it takes in front of the sub-grid and the window
        rec = self.codec.geom["rec_h"], self.codec.geom["rec_w"]
        tile_dt = dt
        if k:
            rh, rw = (rs["pic_h"], rs["pic_w"]) if integer else (rs["rec_h"], rs["rec_w"])
            stem, geom = "spiht_tile_mosaic_", (rs["off_y"], rs["off_x"], rs["Hk"], rs["Wk"], rs["thk"], rs["twk"])
        elif self.overlap:
            tile_dt, (rh, rw) = px.F64, rec
            stem, geom = "spiht_tile_blend_", (self.H, self.W, self.th, self.tw, self.overlap)
        else:
            rh, rw = (self.th, self.tw) if integer else rec
            stem, geom = "spiht_tile_paste_", (self.H, self.W, self.th, self.tw)
        view = ()  # the integer forms write a view of the output: the strides, behind the address
        if integer:
            st, st_p = dt.strides_arg((self.c, h, w), strides, True)
            dt.check_aligned(d_out.ptr)
            view = (st_p,)
        elif dt is not px.F64 or strides is not None:
            raise ValueError("decode: the float form gives dense float64 pictures")
        d_dec = self._buf("dec", n * self.c * rh * rw * tile_dt.itemsize)
        self.codec._decode_device(tile_dt, d_slots.ptr, d_nbytes.ptr, max_n, n, d_dec.ptr, slot_stride=stride, reduce=k or None)
        _lib.check(_entry(self.L, stem, dt)(self.ctx.handle, vp(d_dec.ptr), self.c, rh, rw, *geom, i0, i1, j0, j1, y0, x0, h, w,
                                            vp(d_out.ptr), *view))
        self.last_tiles_decoded = n

    def decode_device(self, d_packed, packed_bytes, d_lens, d_max_n, d_out, strides=None, slot_stride=None, reduce=0):
        """decode_window_device of the whole picture: all T tiles -> d_out [c, H, W] (reduce = k: [c, Hk, Wk])"""
        self.decode_window_device(d_packed, packed_bytes, d_lens, d_max_n, (0, self.gy, 0, self.gx), None, d_out, strides,
                                  slot_stride, reduce)

    def decode_layers_device(self, d_layers, layers_bytes, d_cum, d_max_n, Q, upto, sub, window, d_out, strides=None,
                             slot_stride=None, d_sel=None, reduce=0):
        """decode_window_device of a layered run.  d_layers / layers_bytes: the layers, or a prefix of them, that the table
        d_cum (uint32 [Q][n]) describes: those of the n tiles of the sub-grid in row-major order.  With d_sel (int32 [n]) the
        run and the table ([Q][T]) are the whole picture's and d_sel names the sub-grid's tiles in it.  d_max_n: uint8 [n], the
        start planes of the sub-grid's tiles.  The layers 0 .. upto - 1 are decoded.  sub, window, d_out, strides: as
        decode_window_device; slot_stride: a multiple of 4 no tile is longer than through layer upto - 1 (None: the codec's
        bound; the host forms size the slots by the longest gathered tile).
        One layer-unpack, one batched decode, one paste, queued on the codec's context.  reduce: as decode_window_device (the
        window in the reduced picture's coordinates; None: all of it)."""
        rs = self.reduced_shape(reduce)
        sub, window = self._sub_window(sub, self._window_arg(window, rs), rs)
        n, vp = (sub[1] - sub[0]) * (sub[3] - sub[2]), C.c_void_p
        stride = self.codec.slot_stride if slot_stride is None else int(slot_stride)
        d_slots = self._buf("slots", n * stride)
        d_nbytes = self._buf("nbytes", n * 8)
        _lib.check(self.L.spiht_layer_unpack(self.ctx.handle, vp(_ptr(d_layers)), int(layers_bytes), vp(_ptr(d_cum)), int(Q),
                                             n if d_sel is None else self.T, int(upto), None if d_sel is None else vp(_ptr(d_sel)), n,
                                             vp(d_slots.ptr), stride, vp(d_nbytes.ptr)))
        self._decode_slots(d_slots, d_nbytes, _ptr(d_max_n), stride, sub, window, d_out, strides, rs, reduce)

    # ---- host forms ----------------------------------------------------------------------------------
    def _encode_host(self, images, dtype, channels_last, name, roi=None, target_psnr=None, layered=False, layers=None):
        """the frame of every host encode: the checks, the uploads (pictures, targets, weight map), the device form, one
        synchronise, the downloads, and the results with last_allocation.  layered: encode_layered_device and LayeredResult
        in place of encode_device and TiledResult; the table of lengths is then cum [N][Q][T], otherwise lens [N][1][T]"""
        if layered and self.allocate is None:
            raise ValueError('%s: the codec was not built with allocate="rd"' % name)
        self._overlap_refuses(name, roi, target_psnr)
        if roi is not None:
            self._roi_check(dtype, name)
        Q = 1
        if not layered:
            if target_psnr is not None:
                self._target_check(name)
        elif target_psnr is None:
            Q = len(alloc.layer_budgets(self.max_bits, layers))
        else:
            dbs = alloc.layer_targets_arg(target_psnr, layers)
            Q = len(dbs)
        single, N, d_img, strides = self._upload_pictures(images, dtype, channels_last, name)
        T, NT = self.T, N * self.T
        d_packed = self._buf("packed", NT * self.codec.slot_stride)
        d_table = self._buf("cum", N * Q * T * 4) if layered else self._buf("lens", NT * 4)
        d_maxn = self._buf("maxn", NT)
        if layered:
            d_pic = self._buf("picbytes", N * 8)
        d_target = None
        if target_psnr is not None:
            sums = self._weight_sums(roi, N)
            rows = [[db] * N for db in dbs] if layered else [alloc.target_psnr_arg(target_psnr, N)]
            d_target = self._targets_upload(rows, sums, dtype)
        if layered:
            self.encode_layered_device(d_img, N, layers, d_packed, d_table, d_maxn, d_pic, strides, *self._roi_upload(roi, N),
                                       target_psnr, d_target)
        else:
            self.encode_device(d_img, N, d_packed, d_table, d_maxn, strides, *self._roi_upload(roi, N), d_target)
        self.ctx.synchronize()
        table = self._download(d_table.ptr, (N, Q, T), np.uint32)  # the tables: one download each
        maxn = self._download(d_maxn.ptr, NT, np.uint8)
        if layered:
            pic = self._download(d_pic.ptr, N, np.uint64).astype(np.int64)
            cuts = self._download_cuts("s", Q, N, d_target is not None)
        else:
            pic = table.sum(axis=(1, 2), dtype=np.int64)
        off = np.concatenate(([0], np.cumsum(pic)))
        run = self._download(d_packed.ptr, int(off[-1]), np.uint8)  # the streams (layers) of all pictures: one download
        if not layered and self.allocate is not None:  # (the plain form fetches its cut behind the streams)
            cuts = self._download_cuts("", Q, N, d_target is not None)
        out, allocations = [], []
        for n in range(N):
            rows = [[int(v) for v in row] for row in table[n]]
            head = (self.H, self.W, self.c, self.th, self.tw, self.level, [int(v) for v in maxn[n * T:(n + 1) * T]])
            data = run[int(off[n]):int(off[n + 1])].tobytes()
            out.append(LayeredResult(*head, rows, data, overlap=self.overlap) if layered else
                       TiledResult(*head, list(rows[0]), data, overlap=self.overlap))
            if self.allocate is not None:
                target = [None] * Q if d_target is None else [(cuts[1][q, n], cuts[2][q, n], sums[n], dtype) for q in range(Q)]
                allocations.append([self._allocation(cuts[0][q, n], rows[q], target[q]) for q in range(Q)])
        if self.allocate is not None:
            if not layered:
                allocations = [a[0] for a in allocations]
            self.last_allocation = allocations[0] if single else allocations
        return out[0] if single else out

    def encode(self, image_or_images, roi=None, target_psnr=None):
        """one float picture [c, H, W] -> TiledResult; N pictures [N, c, H, W] -> a list of them -- from one cut, one batched
        encode of the N * T tiles and one pack; the packed bytes and the table come back in one download each.
        roi (allocate="rd" codecs; otherwise ValueError): a weight map, bool or uint8 [H, W] for all pictures or [N, H, W]
        (alloc.roi_arg, alloc.roi_map), uploaded once: the tiles share the budget by the squared error weighted per pixel, so
        the bytes go where the map is large and a tile of zero weights gets none.  The streams, the container and every
        decoder are as without it; last_allocation and tile_curves report the weighted table's numbers.
        target_psnr (allocate="rd" codecs; otherwise ValueError): a PSNR in dB, or one per picture, in place of a size.  Every
        tile is cut at the hull vertex of the steepest common slope at which the picture's squared error -- with roi, the
        weighted one -- is at or below alloc.target_sqerr(target_psnr, peak, c, H * W or the weights' sum), peak 1.0 / 255 /
        65535 (alloc.allocate_target).  max_bits stays the ceiling the tiles are coded with and the cap: a target it cannot
        pay for gives the cut of the call without a target, and one that no cut reaches gives every tile's whole hull if that
        fits.  last_allocation.met tells (with dist and psnr, the error reached)."""
        return self._encode_host(image_or_images, self.pixel_dtype, False, "encode", roi, target_psnr)

    def encode_u8(self, image_or_images, channels_last=False, roi=None, target_psnr=None):
        """uint8 pictures [c, H, W] / [N, c, H, W] (or [H, W, c] / [N, H, W, c] with channels_last) -> what encode gives for
        pictures / 255.0"""
        return self._encode_host(image_or_images, np.uint8, channels_last, "encode_u8", roi, target_psnr)

    def encode_u16(self, image_or_images, channels_last=False, roi=None, target_psnr=None):
        """uint16 pictures -> what encode gives for pictures / 65535.0"""
        return self._encode_host(image_or_images, np.uint16, channels_last, "encode_u16", roi, target_psnr)

    # ---- float pixels in (floatpx): what the float64 call gives for floatpx.to_float64 of the pictures, every sample widened
    # exactly on the device -- the float64 arithmetic of a float64 codec, NOT the single-precision transform of a float32 codec.
    # dtype: None (inferred from a float32 / float16 array) or what floatpx.kind_arg takes ("bfloat16" for uint16 bit patterns).
    def encode_float(self, image_or_images, dtype=None, channels_last=False, roi=None, target_psnr=None):
        """pictures of a float kind [c, H, W] / [N, c, H, W] (or [H, W, c] / [N, H, W, c] with channels_last) -> what encode gives
        for floatpx.to_float64(pictures, kind): allocate="rd", roi and target_psnr as there, with the same ValueErrors"""
        kind = floatpx.input_kind(np.asarray(image_or_images), dtype, "encode_float")
        return self._encode_host(image_or_images, px.of_kind_id(kind), channels_last, "encode_float", roi, target_psnr)

    def encode_layered_float(self, image_or_images, layers=None, dtype=None, channels_last=False, roi=None, target_psnr=None):
        """encode_layered of pictures of a float kind, as encode_float"""
        kind = floatpx.input_kind(np.asarray(image_or_images), dtype, "encode_layered_float")
        return self._encode_host(image_or_images, px.of_kind_id(kind), channels_last, "encode_layered_float", roi, target_psnr, True,
                                 layers)

    def encode_device_float(self, d_img, N, d_packed, d_lens, d_max_n, dtype, strides=None, d_roi=None, roi_stride=0,
                            d_target=None):
        """encode_device of N pictures of the kind `dtype` on the device (a DeviceArray or an address), laid out by `strides`
        (BYTES (sb, sc, sh, sw), non-negative multiples of the element size, as the base; None: dense CHW)"""
        self.encode_device(_View(_ptr(d_img), px.of_kind_id(dtype)), N, d_packed, d_lens, d_max_n, strides, d_roi, roi_stride, d_target)

    def tile_curves_float(self, image, dtype=None, roi=None):
        """tile_curves of one picture of a float kind: the curves of tile_curves(floatpx.to_float64(image, kind))"""
        image = np.asarray(image)
        return self.tile_curves(image, px.of_kind_id(floatpx.input_kind(image, dtype, "tile_curves_float")), roi)

    def _upload_pictures(self, images, dtype, channels_last, name):
        """the host checks of _encode_host and the upload -> (single, N, the device view, strides)"""
        images = np.asarray(images)
        single = images.ndim == 3
        if single:
            images = images[None]
        if images.ndim != 4:
            raise ValueError("%s takes a picture [c, H, W] or pictures [N, c, H, W]" % name)
        dtype = px.of_dtype(dtype)
        strides = None
        if dtype.view and not px._is_dtype(images, dtype.storage):  # (a float kind goes in as its storage type: bit patterns)
            raise ValueError("%s takes a %s array, not %s" % (name, dtype.storage.name, images.dtype))
        images = np.ascontiguousarray(images, dtype=dtype.storage)
        shape = images.shape
        if dtype.view and channels_last:
            N, H, W, c = shape
            shape = (N, c, H, W)
            strides = dtype.channels_last_strides(shape)
        if tuple(shape[1:]) != (self.c, self.H, self.W):
            raise ValueError("%s: pictures of shape %s, the codec's are %s" % (name, tuple(shape[1:]), (self.c, self.H, self.W)))
        d_img = self._buf("img", images.nbytes)
        self.ctx.upload(d_img.ptr, images)
        return single, shape[0], _View(d_img.ptr, dtype), strides

    def encode_layered(self, image_or_images, layers=None, roi=None, target_psnr=None):
        """encode in quality layers (a codec built with allocate="rd"; otherwise ValueError).  layers: an int Q or the layers'
        bit budgets, the last one max_bits (alloc.layer_budgets).  -> LayeredResult, or a list for [N, c, H, W];
        result.tiled() is what encode gives.  last_allocation: a list of Q TileAllocation, one per layer (a list of such lists
        for several pictures).  roi: a weight map, as encode -- the first layers then hold the bytes of the tiles it favours,
        so a truncated file shows the region of interest first.
        target_psnr: the layers as strictly increasing PSNRs in dB, e.g. [30, 35, 40], in place of budgets (layers is then None
        or their number).  Layer q ends where encode(..., target_psnr=target_psnr[q]) cuts: result.tiled(q + 1) is that
        TiledResult.  max_bits stays the cap; a layer whose target it cannot pay for ends at the cut of max_bits, and the layers
        behind it are empty.  The container is the same SPTQ."""
        return self._encode_host(image_or_images, self.pixel_dtype, False, "encode_layered", roi, target_psnr, True, layers)

    def encode_layered_u8(self, image_or_images, layers=None, channels_last=False, roi=None, target_psnr=None):
        """encode_layered of uint8 pictures, as encode_u8"""
        return self._encode_host(image_or_images, np.uint8, channels_last, "encode_layered_u8", roi, target_psnr, True, layers)

    def encode_layered_u16(self, image_or_images, layers=None, channels_last=False, roi=None, target_psnr=None):
        """encode_layered of uint16 pictures, as encode_u16"""
        return self._encode_host(image_or_images, np.uint16, channels_last, "encode_layered_u16", roi, target_psnr, True, layers)

    def tile_curves(self, image, dtype=None, roi=None):
        """The curves allocate="rd" cuts by, of one picture [c, H, W] (dtype None: the codec's float pixels; np.uint8 /
        np.uint16: integer pixels) -> TileCurves.  alloc.allocate(curves.lengths, curves.sse, max_bits // 8) gives the lengths
        of encode / encode_u8 / encode_u16 of that picture; last_allocation is set as by them.  roi: the weight map of that
        encode call -- sse is then the weighted error."""
        if self.allocate is None:
            raise ValueError('tile_curves: the codec was not built with allocate="rd"')
        image = np.asarray(image)
        if image.ndim != 3:
            raise ValueError("tile_curves takes one picture [c, H, W]")
        dtype = px.of_dtype(self.pixel_dtype if dtype is None else dtype)
        self._encode_host(image, dtype, False, "tile_curves", roi)
        T, K = self.T, self.points
        D = self._download(self._bufs["D"].ptr, (K + 1, T), np.uint64 if dtype.integer else np.float64)
        nbits = self._download(self._bufs["nbits"].ptr, T, np.uint64)
        maxn = self._download(self._bufs["maxn"].ptr, T, np.uint8)
        nbytes = [(int(v) + 7) // 8 for v in nbits]
        return TileCurves([alloc.tile_lengths(n, K) for n in nbytes], np.ascontiguousarray(D.T), nbytes, [int(v) for v in maxn])

    def _check_result(self, r, layered):
        """ValueError for a result that is not one of this codec's pictures; a TiledResult's tables are checked here, a
        LayeredResult's by its own _table()"""
        _check_version(r)
        if (r.h, r.w, r.c, r.th, r.tw) != (self.H, self.W, self.c, self.th, self.tw) or (layered and len(r.max_n) != self.T):
            raise ValueError("a result of geometry %s, the codec's is %s" % ((r.h, r.w, r.c, r.th, r.tw),
                                                                            (self.H, self.W, self.c, self.th, self.tw)))
        if r.overlap != self.overlap:
            raise ValueError("a result of overlap %d, the codec's is %d" % (r.overlap, self.overlap))
        if not layered and (len(r.nbytes) != self.T or len(r.max_n) != self.T or sum(r.nbytes) != len(r.encoded_bytes)):
            raise ValueError("the tables of the result do not describe %d tiles of %d bytes" % (self.T, len(r.encoded_bytes)))

    def _decode_host(self, result, window, dtype, channels_last, reduce=0, layered=False, upto=None):
        """the frame of every host decode, of a TiledResult or (layered) of the first upto layers of a LayeredResult: the checks,
        the window and its sub-grid, one upload of a blob -- a u32 table [rows][n] of the sub-grid's n tiles whose last row is
        their lengths, their start planes padded to a multiple of 4, their bytes -- the device form, one synchronise and one
        download.  The kinds differ in the table (lens [1][n] / cum [upto][n]), in the byte ranges gathered and in the device form"""
        self._check_result(result, layered)
        if layered:
            cum, lens, off = result._table()
            upto = _upto_arg(upto, cum.shape[0])
        rs = self.reduced_shape(reduce)
        y0, x0, h, w = self._window_arg(window, rs)
        i0, i1, j0, j1 = sub = self._window_tiles(rs, y0, x0, h, w)
        dtype = px.of_dtype(dtype)
        ts = [i * self.gx + j for i in range(i0, i1) for j in range(j0, j1)]
        n = len(ts)
        # a row of the sub-grid, tiles a .. b - 1, is contiguous in the run (per layer, in the file)
        rows = [(i * self.gx + j0, i * self.gx + j1) for i in range(i0, i1)]
        if layered:
            table = np.ascontiguousarray(cum[:upto, ts], dtype=np.uint32)
            ranges = [(int(off[q, a]), int(off[q, b - 1] + lens[q, b - 1])) for q in range(upto) for a, b in rows]
        else:
            table = np.asarray([[result.nbytes[t] for t in ts]], dtype=np.uint32)
            off = result._offsets()
            ranges = [(int(off[a]), int(off[b])) for a, b in rows]
        total = table[-1]  # the tiles' lengths
        nb = int(total.sum(dtype=np.int64))
        planes = 4 * table.size
        head = planes + ((n + 3) & ~3)
        blob = np.zeros(head + max(nb, 1), dtype=np.uint8)
        blob[:planes] = table.reshape(-1).view(np.uint8)
        blob[planes:planes + n] = np.asarray([result.max_n[t] for t in ts], dtype=np.uint8)
        data = np.frombuffer(result.encoded_bytes, dtype=np.uint8)
        p = head
        for a, b in ranges:
            blob[p:p + b - a] = data[a:b]
            p += b - a
        d_in = self._buf("in", blob.nbytes)
        self.ctx.upload(d_in.ptr, blob)  # the table, the start planes and the streams of the sub-grid's tiles: one upload
        strides = dtype.channels_last_strides((self.c, h, w)) if channels_last else None
        d_out = self._buf("out", self.c * h * w * dtype.itemsize)
        stride = max(4, (int(total.max()) + 3) & ~3)
        streams = (d_in.ptr + head, nb, d_in.ptr, d_in.ptr + planes)
        where = (sub, (y0, x0, h, w), _View(d_out.ptr, dtype), strides, stride)
        if layered:
            self.decode_layers_device(*streams, upto, upto, *where, None, reduce)
        else:
            self.decode_window_device(*streams, *where, reduce)
        self.ctx.synchronize()
        out = _lib.result_array((h, w, self.c) if channels_last else (self.c, h, w), dtype.storage)
        self.ctx.download(out, d_out.ptr)
        return out

    def decode_layered(self, result, upto=None, reduce=0):
        """LayeredResult -> float64 [c, H, W] from its first `upto` layers (None: all): what decode gives for
        result.tiled(upto), with the tiles' pieces gathered on the device -- one upload, one layer-unpack, one batched decode,
        one paste.  A prefix of a file (LayeredResult.from_bytes) decodes like any other result.  reduce: as decode."""
        return self._decode_host(result, None, np.float64, False, reduce, True, upto)

    def decode_layered_u8(self, result, upto=None, channels_last=False, reduce=0):
        return self._decode_host(result, None, np.uint8, channels_last, reduce, True, upto)

    def decode_layered_u16(self, result, upto=None, channels_last=False, reduce=0):
        return self._decode_host(result, None, np.uint16, channels_last, reduce, True, upto)

    def decode_layered_window(self, result, y0, x0, h, w, upto=None, reduce=0):
        """-> float64 [c, h, w] = decode_layered(result, upto)[:, y0:y0 + h, x0:x0 + w]; only the pieces of the tiles that meet
        the window, of the layers below upto, are uploaded (last_tiles_decoded tells how many tiles).  reduce: as decode_window."""
        return self._decode_host(result, (y0, x0, h, w), np.float64, False, reduce, True, upto)

    def decode_layered_window_u8(self, result, y0, x0, h, w, upto=None, channels_last=False, reduce=0):
        return self._decode_host(result, (y0, x0, h, w), np.uint8, channels_last, reduce, True, upto)

    def decode_layered_window_u16(self, result, y0, x0, h, w, upto=None, channels_last=False, reduce=0):
        return self._decode_host(result, (y0, x0, h, w), np.uint16, channels_last, reduce, True, upto)

    def decode(self, result, reduce=0):
        """TiledResult -> float64 [c, H, W]: one upload, one unpack, one batched decode of all T tiles, one paste.  Unlike
        decode_image, whose float64 picture is one longer on an odd axis (pywt.waverec2's size), the result is CROPPED to the
        picture's H x W: a tile's extra row and column belong to no picture sample.
        reduce = k > 0: the picture at 1/2^k size, float64 [c, Hk, Wk] = [c, ceil(H / 2^k), ceil(W / 2^k)] (reduced_shape(k);
        0 <= k <= the tile's levels and 2^k dividing both tile sides, else ValueError): sample (Y, X) is sample
        (Y - i thk, X - j twk) of decode_image_reduced(result.tile(i, j), settings, k, crop=True), (i, j) = (Y // thk, X // twk).
        One batched reduced decode of the tiles and one mosaic: only the small picture is assembled and comes back."""
        return self._decode_host(result, None, np.float64, False, reduce)

    def decode_u8(self, result, channels_last=False, reduce=0):
        """-> uint8 [c, H, W] (or [H, W, c]): the rule of decode_image_u8 per tile (reduce = k: of decode_image_reduced_u8)"""
        return self._decode_host(result, None, np.uint8, channels_last, reduce)

    def decode_u16(self, result, channels_last=False, reduce=0):
        """-> uint16 [c, H, W] (or [H, W, c])"""
        return self._decode_host(result, None, np.uint16, channels_last, reduce)

    def decode_window(self, result, y0, x0, h, w, reduce=0):
        """-> float64 [c, h, w] = decode(result)[:, y0:y0 + h, x0:x0 + w]; only the tiles that meet the window are uploaded,
        unpacked and decoded (last_tiles_decoded tells how many).  A window that leaves the picture: ValueError.
        reduce = k > 0: the window is given in the REDUCED picture's coordinates, inside Hk x Wk, and the result is
        decode(result, reduce=k)[:, y0:y0 + h, x0:x0 + w]; the tiles decoded are those it meets in the thk x twk grid."""
        return self._decode_host(result, (y0, x0, h, w), np.float64, False, reduce)

    def decode_window_u8(self, result, y0, x0, h, w, channels_last=False, reduce=0):
        """decode_window into uint8 [c, h, w] (or [h, w, c])"""
        return self._decode_host(result, (y0, x0, h, w), np.uint8, channels_last, reduce)

    def decode_window_u16(self, result, y0, x0, h, w, channels_last=False, reduce=0):
        """decode_window into uint16 [c, h, w] (or [h, w, c])"""
        return self._decode_host(result, (y0, x0, h, w), np.uint16, channels_last, reduce)

    # ---- float pixels out (floatpx): floatpx.convert(<the float64 call>, dtype) in every bit, each sample rounded once, with
    # the conversion on the device -- in the tiles' decode, or with overlap > 0 at the blend's store.  dtype: np.float32,
    # np.float16, "bfloat16" or a torch dtype; bfloat16 comes as uint16 bit patterns.
    def decode_float(self, result, dtype=np.float32, channels_last=False, reduce=0):
        """-> [c, H, W] (or [H, W, c]) of the kind: floatpx.convert(decode(result, reduce), dtype)"""
        return self._decode_host(result, None, px.of_kind_id(dtype), channels_last, reduce)

    def decode_window_float(self, result, y0, x0, h, w, dtype=np.float32, channels_last=False, reduce=0):
        """-> [c, h, w] (or [h, w, c]) of the kind: floatpx.convert(decode_window(result, y0, x0, h, w, reduce), dtype)"""
        return self._decode_host(result, (y0, x0, h, w), px.of_kind_id(dtype), channels_last, reduce)

    def decode_layered_float(self, result, upto=None, dtype=np.float32, channels_last=False, reduce=0):
        """floatpx.convert(decode_layered(result, upto, reduce), dtype)"""
        return self._decode_host(result, None, px.of_kind_id(dtype), channels_last, reduce, True, upto)

    def decode_layered_window_float(self, result, y0, x0, h, w, upto=None, dtype=np.float32, channels_last=False, reduce=0):
        """floatpx.convert(decode_layered_window(result, y0, x0, h, w, upto, reduce), dtype)"""
        return self._decode_host(result, (y0, x0, h, w), px.of_kind_id(dtype), channels_last, reduce, True, upto)


class _View:
    """a device address with an element type (what the device forms need of a DeviceArray), owning nothing"""

    def __init__(self, ptr, dtype):
        self.ptr, self.dtype = int(ptr), px.of_dtype(dtype)


# ---- top-level conveniences, after the single-image calls -------------------------------------------------------------
_codecs = {}


def _codec_for(c, H, W, tile, settings, level, max_bits, pixel_dtype=np.float64, allocate=None, points=alloc.POINTS,
               spread=alloc.SPREAD, overlap=0):
    """a TiledCodec per geometry and settings, kept (a few of them) so that repeated calls reuse its device buffers"""
    th, tw = _tile_arg(tile)
    if getattr(settings, "color_model", None) not in (None, "RGB"):
        pixel_dtype = np.float64  # as TiledCodec: colour pictures are coded in float64
    points, spread = _alloc_args(allocate, points, spread, max_bits, pixel_dtype)
    overlap = _overlap.overlap_arg(overlap, th, tw)
    key = (c, H, W, th, tw, repr(settings), level, max_bits, np.dtype(pixel_dtype).name, allocate, points, spread,
           id(_lib.default_context()), overlap)
    codec = _codecs.get(key)
    if codec is None:
        while len(_codecs) >= 4:
            _codecs.pop(next(iter(_codecs))).close()
        codec = _codecs[key] = TiledCodec(c, H, W, (th, tw), settings, level, max_bits, None, pixel_dtype, allocate, points, spread,
                                          overlap)
    return codec


def _picture_shape(image, channels_last):
    """(c, h, w) of the one picture a module-level encode call takes"""
    if not isinstance(image, np.ndarray) or image.ndim != 3:
        raise ValueError('image ndim must be 3: c,h,w')
    return (image.shape[2], image.shape[0], image.shape[1]) if channels_last else image.shape


def _encode_tiled(image, tile, spiht_settings, level, max_bits, dtype, channels_last, name, allocate=None, points=alloc.POINTS,
                  spread=alloc.SPREAD, roi=None, target_psnr=None, overlap=0):
    c, h, w = _picture_shape(image, channels_last)
    if dtype is None:
        dtype = np.float32 if image.dtype in (np.float32, np.float16) else np.float64
    own = not px.of_dtype(dtype).view  # the codec's own float pixels (integer pixels and the float kinds: a float64 codec)
    codec = _codec_for(c, h, w, tile, spiht_settings, level, max_bits, dtype if own else np.float64, allocate, points, spread,
                       overlap)
    return codec._encode_host(image, codec.pixel_dtype if own else dtype, channels_last, name, roi, target_psnr)


def encode_image_tiled(image, tile, spiht_settings=SpihtSettings(), level=None, max_bits=None, allocate=None, points=alloc.POINTS,
                       spread=alloc.SPREAD, roi=None, target_psnr=None, overlap=0):
    """encode_image of a picture (c, h, w) as tiles of `tile` (an int or (th, tw)) -> TiledResult.  level and max_bits are
    per tile as in TiledCodec: every tile gets max_bits // T bits; float32 pixels run the single-precision transform.
    allocate="rd" (with points, spread): the tiles share max_bits by their rate-distortion curves, as in TiledCodec.
    roi (with allocate="rd"): a weight map [h, w], bool or uint8 (roi_map), that steers the shares, as in TiledCodec.encode.
    target_psnr (with allocate="rd"): a PSNR in dB to reach with the fewest bytes the measured curves allow, max_bits the cap, as
    in TiledCodec.encode.
    overlap = m > 0: every tile is coded with a margin of m samples of its neighbours and the decode calls cross-fade the seams,
    as in TiledCodec (the result carries the overlap; roi and target_psnr are then refused)."""
    return _encode_tiled(image, tile, spiht_settings, level, max_bits, None, False, "encode_image_tiled", allocate, points, spread,
                         roi, target_psnr, overlap)


def encode_image_tiled_u8(image, tile, spiht_settings=SpihtSettings(), level=None, max_bits=None, channels_last=False,
                          allocate=None, points=alloc.POINTS, spread=alloc.SPREAD, roi=None, target_psnr=None, overlap=0):
    """uint8 pixels: the TiledResult of encode_image_tiled(image / 255.0, ...); allocate="rd" measures 8-bit decodes"""
    return _encode_tiled(image, tile, spiht_settings, level, max_bits, np.uint8, channels_last, "encode_image_tiled_u8", allocate,
                         points, spread, roi, target_psnr, overlap)


def encode_image_tiled_u16(image, tile, spiht_settings=SpihtSettings(), level=None, max_bits=None, channels_last=False,
                           allocate=None, points=alloc.POINTS, spread=alloc.SPREAD, roi=None, target_psnr=None, overlap=0):
    """uint16 pixels: the TiledResult of encode_image_tiled(image / 65535.0, ...); allocate="rd" measures 16-bit decodes"""
    return _encode_tiled(image, tile, spiht_settings, level, max_bits, np.uint16, channels_last, "encode_image_tiled_u16", allocate,
                         points, spread, roi, target_psnr, overlap)


def encode_image_tiled_float(image, tile, spiht_settings=SpihtSettings(), level=None, max_bits=None, dtype=None, channels_last=False,
                             allocate=None, points=alloc.POINTS, spread=alloc.SPREAD, roi=None, target_psnr=None, overlap=0):
    """float pixels in (float32, float16, or uint16 bit patterns with dtype="bfloat16"): the TiledResult of
    encode_image_tiled(floatpx.to_float64(image, kind), ...), every sample widened exactly on the device -- the float64
    transform, not the single-precision one encode_image_tiled runs for a float32 array"""
    kind = floatpx.input_kind(image, dtype, "encode_image_tiled_float")
    return _encode_tiled(image, tile, spiht_settings, level, max_bits, px.of_kind_id(kind), channels_last, "encode_image_tiled_float",
                         allocate, points, spread, roi, target_psnr, overlap)


def _decode_tiled(result, spiht_settings, window, dtype, channels_last, reduce=0, layered=False, upto=None):
    codec = _codec_for(result.c, result.h, result.w, (result.th, result.tw), spiht_settings, result.level, None,
                       overlap=result.overlap)
    return codec._decode_host(result, window, dtype, channels_last, reduce, layered, upto)


def decode_image_tiled(result, spiht_settings, reduce=0):
    """TiledResult -> float64 (c, h, w), cropped to the picture's size (see TiledCodec.decode); reduce = k: the picture at
    1/2^k size, (c, ceil(h / 2^k), ceil(w / 2^k)) (tiled_reduced_shape)"""
    return _decode_tiled(result, spiht_settings, None, np.float64, False, reduce)


def decode_image_tiled_u8(result, spiht_settings, channels_last=False, reduce=0):
    return _decode_tiled(result, spiht_settings, None, np.uint8, channels_last, reduce)


def decode_image_tiled_u16(result, spiht_settings, channels_last=False, reduce=0):
    return _decode_tiled(result, spiht_settings, None, np.uint16, channels_last, reduce)


def decode_image_window(result, spiht_settings, y0, x0, h, w, reduce=0):
    """the window [y0, y0 + h) x [x0, x0 + w) of the picture -> float64 (c, h, w), decoding only the tiles it meets; reduce = k:
    the window of the picture at 1/2^k size, in that picture's coordinates"""
    return _decode_tiled(result, spiht_settings, (y0, x0, h, w), np.float64, False, reduce)


def decode_image_window_u8(result, spiht_settings, y0, x0, h, w, channels_last=False, reduce=0):
    return _decode_tiled(result, spiht_settings, (y0, x0, h, w), np.uint8, channels_last, reduce)


def decode_image_window_u16(result, spiht_settings, y0, x0, h, w, channels_last=False, reduce=0):
    return _decode_tiled(result, spiht_settings, (y0, x0, h, w), np.uint16, channels_last, reduce)


def decode_image_tiled_float(result, spiht_settings, dtype=np.float32, channels_last=False, reduce=0):
    """TiledResult -> the picture in a float kind (np.float32, np.float16, "bfloat16", a torch dtype; bfloat16 as uint16 bit
    patterns): floatpx.convert(decode_image_tiled(result, spiht_settings, reduce), dtype) in every bit, converted on the device"""
    return _decode_tiled(result, spiht_settings, None, px.of_kind_id(dtype), channels_last, reduce)


def decode_image_window_float(result, spiht_settings, y0, x0, h, w, dtype=np.float32, channels_last=False, reduce=0):
    """floatpx.convert(decode_image_window(result, spiht_settings, y0, x0, h, w, reduce), dtype)"""
    return _decode_tiled(result, spiht_settings, (y0, x0, h, w), px.of_kind_id(dtype), channels_last, reduce)


def decode_image_layered_float(result, spiht_settings, upto=None, dtype=np.float32, channels_last=False, reduce=0):
    """floatpx.convert(decode_image_layered(result, spiht_settings, upto, reduce), dtype)"""
    return _decode_tiled(result, spiht_settings, None, px.of_kind_id(dtype), channels_last, reduce, True, upto)


def decode_image_layered_window_float(result, spiht_settings, y0, x0, h, w, upto=None, dtype=np.float32, channels_last=False,
                                      reduce=0):
    """floatpx.convert(decode_image_layered_window(result, spiht_settings, y0, x0, h, w, upto, reduce), dtype)"""
    return _decode_tiled(result, spiht_settings, (y0, x0, h, w), px.of_kind_id(dtype), channels_last, reduce, True, upto)


def float_elem(dtype):
    """the element type the device forms (decode_window_device, decode_device, decode_layers_device) take as d_out.dtype for
    float pixels out"""
    return px.of_kind_id(dtype)


def _encode_layered(image, tile, spiht_settings, level, max_bits, layers, dtype, channels_last, name, points, spread, roi=None,
                    target_psnr=None, overlap=0):
    if layers is None and target_psnr is None:
        layers = 1
    c, h, w = _picture_shape(image, channels_last)
    codec = _codec_for(c, h, w, tile, spiht_settings, level, max_bits, np.float64, "rd", points, spread, overlap)
    return codec._encode_host(image, codec.pixel_dtype if dtype is None else dtype, channels_last, name, roi, target_psnr, True,
                              layers)


def encode_image_layered(image, tile, spiht_settings=SpihtSettings(), level=None, max_bits=None, layers=None, points=alloc.POINTS,
                         spread=alloc.SPREAD, roi=None, target_psnr=None, overlap=0):
    """encode_image_tiled(..., allocate="rd") of a float64 picture (c, h, w) in quality layers -> LayeredResult.  layers: an
    int Q or the layers' bit budgets, the last one max_bits (alloc.layer_budgets); result.tiled() is the TiledResult of
    encode_image_tiled, and any prefix of result.to_bytes() that holds the tables is a picture.  roi: a weight map, as
    encode_image_tiled -- the first layers then hold the region of interest.  layers=None is one layer, or with target_psnr
    as many as it holds: the layers as strictly increasing PSNRs in dB in place of budgets, max_bits the cap, as in
    TiledCodec.encode_layered.  overlap: overlapping tiles, as encode_image_tiled (layers as budgets only)."""
    return _encode_layered(image, tile, spiht_settings, level, max_bits, layers, None, False, "encode_image_layered", points, spread,
                           roi, target_psnr, overlap)


def encode_image_layered_u8(image, tile, spiht_settings=SpihtSettings(), level=None, max_bits=None, layers=None, points=alloc.POINTS,
                            spread=alloc.SPREAD, channels_last=False, roi=None, target_psnr=None, overlap=0):
    return _encode_layered(image, tile, spiht_settings, level, max_bits, layers, np.uint8, channels_last, "encode_image_layered_u8",
                           points, spread, roi, target_psnr, overlap)


def encode_image_layered_u16(image, tile, spiht_settings=SpihtSettings(), level=None, max_bits=None, layers=None, points=alloc.POINTS,
                             spread=alloc.SPREAD, channels_last=False, roi=None, target_psnr=None, overlap=0):
    return _encode_layered(image, tile, spiht_settings, level, max_bits, layers, np.uint16, channels_last, "encode_image_layered_u16",
                           points, spread, roi, target_psnr, overlap)


def encode_image_layered_float(image, tile, spiht_settings=SpihtSettings(), level=None, max_bits=None, layers=None, dtype=None,
                               points=alloc.POINTS, spread=alloc.SPREAD, channels_last=False, roi=None, target_psnr=None, overlap=0):
    """float pixels in: the LayeredResult of encode_image_layered(floatpx.to_float64(image, kind), ...)"""
    kind = floatpx.input_kind(image, dtype, "encode_image_layered_float")
    return _encode_layered(image, tile, spiht_settings, level, max_bits, layers, px.of_kind_id(kind), channels_last,
                           "encode_image_layered_float", points, spread, roi, target_psnr, overlap)


def decode_image_layered(result, spiht_settings, upto=None, reduce=0):
    """LayeredResult -> float64 (c, h, w) from its first `upto` layers (None: all), cropped as decode_image_tiled; reduce: as
    decode_image_tiled"""
    return _decode_tiled(result, spiht_settings, None, np.float64, False, reduce, True, upto)


def decode_image_layered_u8(result, spiht_settings, upto=None, channels_last=False, reduce=0):
    return _decode_tiled(result, spiht_settings, None, np.uint8, channels_last, reduce, True, upto)


def decode_image_layered_u16(result, spiht_settings, upto=None, channels_last=False, reduce=0):
    return _decode_tiled(result, spiht_settings, None, np.uint16, channels_last, reduce, True, upto)


def decode_image_layered_window(result, spiht_settings, y0, x0, h, w, upto=None, reduce=0):
    """the window of the picture from its first `upto` layers, decoding only the tiles it meets; reduce: as decode_image_window"""
    return _decode_tiled(result, spiht_settings, (y0, x0, h, w), np.float64, False, reduce, True, upto)


def decode_image_layered_window_u8(result, spiht_settings, y0, x0, h, w, upto=None, channels_last=False, reduce=0):
    return _decode_tiled(result, spiht_settings, (y0, x0, h, w), np.uint8, channels_last, reduce, True, upto)


def decode_image_layered_window_u16(result, spiht_settings, y0, x0, h, w, upto=None, channels_last=False, reduce=0):
    return _decode_tiled(result, spiht_settings, (y0, x0, h, w), np.uint16, channels_last, reduce, True, upto)
