"""Picture sets: pictures of DIFFERENT sizes coded as one batch of tiles, and windows of many pictures decoded in one batch.

Everything else that is batched here is bound to one picture size.  A tile is a picture of its own and all tiles of a codec
have one shape, so the tiles of pictures of any sizes can share one batch of the coder: TileSetCodec cuts a list of pictures
into ONE dense tile batch (csrc/tileset.hip: k_tile_cut_set), codes it by one BatchCodec(c, th, tw) call and packs the streams;
the way back is one unpack, one batched decode and one paste into all the windows at once (k_tile_paste_set) -- whole pictures,
a window per picture, or the training read "a crop of one size from each of B pictures as one array [B, c, h, w]".

The budget is PER TILE (tile_bits), so a set is coded at one rate per pixel, up to the padding of edge tiles.  Every result
is defined by calls that exist: picture p's TiledResult is, field by field and byte by byte, that of
TiledCodec(c, H_p, W_p, tile, settings, level, max_bits=None if tile_bits is None else tile_bits * T_p).encode*(picture_p),
and every decode is that codec's decode* / decode_window*.  The coder, the transforms, pack / unpack, TiledResult and its SPTL
container are untouched.

The rules in numpy, as overlap.py and alloc.py hold theirs: cut_rule (the dense tile batch of a set), paste_rule (the windows
of a tile batch) and set_tables (where every picture's tiles lie in the batch, which tiles every window needs and in which
order their streams are gathered).

Resized crops (decode_resized_crops*, decode_resized_device) are the read of a training loop: a box of ANY size from each of B
pictures, resampled to one size, mirrored and normalised, as one array [B, c, oh, ow].  The tiles a box meets are decoded to
float64 as above and one kernel (csrc/resample.hip: k_tile_resample_set) reads that tile batch through the boxes; the rule in
numpy is resample.py: resize_rule.

Out of scope, each refused with a ValueError that names it: allocate="rd", roi, target_psnr, layers, overlap > 0 and
reduce > 0 -- the allocation takes one tile count per picture, the blend and the mosaic are kernels of their own.
"""
import ctypes as C

import numpy as np

from . import _lib, floatpx, px, resample
from .batch import BatchCodec
from .spiht_wrapper import SpihtSettings, _check_version
from .tiles import TiledCodec, TiledResult, _ptr, _tile_arg, window_tiles

_ALIGN = 16  # pictures and windows of a host call lie at multiples of it in their one buffer: the copies' 16-byte loads and stores


# ---- the rules, in numpy ---------------------------------------------------------------------------------------------------
def _grid(H, W, th, tw):
    """(gy, gx) of an H x W picture in tiles of th x tw, by spiht_tile_grid's rule; ValueError for what it refuses"""
    H, W, th, tw = int(H), int(W), int(th), int(tw)
    if H < 1 or W < 1 or th < 8 or tw < 8:
        raise ValueError("a %d x %d picture in tiles of %d x %d: sides >= 1, tile sides >= 8" % (H, W, th, tw))
    return -(-H // th), -(-W // tw)


def cut_rule(pictures, th, tw):
    """pictures: arrays [c, H_p, W_p] of one c and dtype -> the dense tile batch [NT, c, th, tw]: picture p extended by edge
    replication to whole tiles (np.pad(mode="edge")), its tiles in row-major order behind those of picture p - 1"""
    out = []
    for P in pictures:
        P = np.asarray(P)
        c, H, W = P.shape
        gy, gx = _grid(H, W, th, tw)
        Q = np.pad(P, [(0, 0), (0, gy * th - H), (0, gx * tw - W)], mode="edge")
        out.append(Q.reshape(c, gy, th, gx, tw).transpose(1, 3, 0, 2, 4).reshape(gy * gx, c, th, tw))
    return np.concatenate(out)


def paste_rule(tiles, items, th, tw):
    """tiles: [S, c, rh, rw], rh >= th, rw >= tw; items: one ((i0, i1, j0, j1), (y0, x0, h, w)) per window, item b owning the
    tiles [s0_b, s0_b + (i1 - i0) * (j1 - j0)) of the batch, its sub-grid in row-major order -> the list of windows [c, h, w]:
    sample (Y, X) of the picture is sample (Y - i th, X - j tw) of tile (i, j) = (Y // th, X // tw)"""
    tiles, items = np.asarray(tiles), list(items)
    S = sum((i1 - i0) * (j1 - j0) for (i0, i1, j0, j1), _ in items)
    if S != len(tiles):
        raise ValueError("the items own %d tiles, the batch holds %d" % (S, len(tiles)))
    out, s0 = [], 0
    for (i0, i1, j0, j1), (y0, x0, h, w) in items:
        Y, X = np.arange(y0, y0 + h)[:, None], np.arange(x0, x0 + w)[None, :]
        i, j = Y // th, X // tw
        if i.min() < i0 or i.max() >= i1 or j.min() < j0 or j.max() >= j1:
            raise ValueError("the sub-grid %s does not hold the tiles of the window %s" % ((i0, i1, j0, j1), (y0, x0, h, w)))
        s = s0 + (i - i0) * (j1 - j0) + (j - j0)
        out.append(np.ascontiguousarray(tiles[s, :, Y - i * th, X - j * tw].transpose(2, 0, 1)))
        s0 += (i1 - i0) * (j1 - j0)
    return out


def set_tables(sizes, th, tw, items=None):
    """The tables of a set.  sizes: (H, W) per picture -> a dict with
      grids        (gy, gx) per picture
      tile0        int64 [P + 1]: picture p's tiles are rows [tile0[p], tile0[p + 1]) of the cut's batch (the running sum of T_p)
      pic_of_tile  uint32 [NT]: the picture of every row
    and, with items = one (p, window) per window -- p the picture's index, window (y0, x0, h, w) or None for all of it --,
      windows      the windows, None resolved
      subs         (i0, i1, j0, j1) per item: the tiles its window meets (window_tiles)
      s0           int64 [B + 1]: item b's tiles are rows [s0[b], s0[b + 1]) of the paste's batch
      item_of_tile uint32 [S]: the item of every row
      gather       int64 [S]: the tile of its picture every row is, i * gx + j -- the order the streams are gathered in:
                   item by item, each sub-grid in row-major order
    ValueError for an empty set, a picture or tile side spiht_tile_grid refuses, and a window that is empty or leaves its
    picture.  Pure arithmetic: no device."""
    th, tw = int(th), int(tw)
    sizes = [(int(H), int(W)) for H, W in sizes]
    if not sizes:
        raise ValueError("an empty set of pictures")
    grids = [_grid(H, W, th, tw) for H, W in sizes]
    counts = np.asarray([gy * gx for gy, gx in grids], dtype=np.int64)
    t = dict(grids=grids, tile0=np.concatenate(([0], np.cumsum(counts))),
             pic_of_tile=np.repeat(np.arange(len(sizes), dtype=np.uint32), counts))
    if items is None:
        return t
    items = list(items)
    if not items:
        raise ValueError("an empty list of windows")
    windows, subs, gather = [], [], []
    for p, window in items:
        H, W = sizes[p]
        y0, x0, h, w = (0, 0, H, W) if window is None else (int(v) for v in window)
        i0, i1, j0, j1 = window_tiles(H, W, th, tw, y0, x0, h, w)
        windows.append((y0, x0, h, w))
        subs.append((i0, i1, j0, j1))
        gather.append((np.arange(i0, i1)[:, None] * grids[p][1] + np.arange(j0, j1)[None, :]).reshape(-1))
    counts = np.asarray([len(g) for g in gather], dtype=np.int64)
    t.update(windows=windows, subs=subs, s0=np.concatenate(([0], np.cumsum(counts))),
             item_of_tile=np.repeat(np.arange(len(items), dtype=np.uint32), counts), gather=np.concatenate(gather).astype(np.int64))
    return t


# ---- the codec ---------------------------------------------------------------------------------------------------------------
_OUT_OF_SCOPE = {
    "allocate": 'allocate="rd" is not supported for a picture set: the allocation takes one tile count per picture',
    "roi": "roi (a weight map) is not supported for a picture set: it steers allocate=\"rd\"",
    "target_psnr": "target_psnr is not supported for a picture set: it is reached by allocate=\"rd\"",
    "layers": "layers are not supported for a picture set: they are cuts of allocate=\"rd\"",
    "overlap": "overlap > 0 is not supported for a picture set: the blend is a kernel of its own",
    "reduce": "reduce > 0 is not supported for a picture set: the mosaic is a kernel of its own",
}


def _refuse(name, **kw):
    """ValueError for an out-of-scope keyword that is set (None and 0: not set), naming it"""
    for k, v in kw.items():
        if v is not None and not (k in ("overlap", "reduce") and not isinstance(v, bool) and v == 0):
            raise ValueError("%s: %s" % (name, _OUT_OF_SCOPE[k]))


def _align(n):
    return (int(n) + _ALIGN - 1) // _ALIGN * _ALIGN


class TileSetCodec:
    """encode / decode LISTS of pictures [c, H_p, W_p] of any sizes as tiles of `tile` = th x tw (an int or (th, tw), sides >= 8).

    settings / level / tile_bits have the meaning of encode_image for EVERY TILE: the codec holds one
    BatchCodec(c, th, tw, settings, level, tile_bits, ctx, pixel_dtype), and whatever encode_image refuses for a th x tw picture
    is refused here, in the constructor.  tile_bits is the bit budget of a tile (None: none), so picture p's result is that of
    TiledCodec(c, H_p, W_p, tile, settings, level, max_bits=tile_bits * T_p) in every field and byte, and every decode call
    gives what that codec's gives.  pixel_dtype float32: the single-precision transform, as in TiledCodec.

    Out of scope, each a ValueError that names it: allocate="rd", roi, target_psnr, layers, overlap > 0, reduce > 0."""

    def __init__(self, c, tile, settings=None, level=None, tile_bits=None, ctx=None, pixel_dtype=np.float64, allocate=None,
                 overlap=0):
        _refuse("TileSetCodec", allocate=allocate, overlap=overlap)
        self.settings = settings if settings is not None else SpihtSettings()
        if self.settings.color_model not in (None, "RGB"):
            pixel_dtype = np.float64  # as encode_image: colour pictures are coded in float64
        self.c = int(c)
        self.th, self.tw = _tile_arg(tile)
        _grid(1, 1, self.th, self.tw)  # (the tile sides, in the grid's own words)
        self.level = level
        self.tile_bits = tile_bits
        self.codec = BatchCodec(self.c, self.th, self.tw, self.settings, level, tile_bits, ctx, pixel_dtype)
        self.ctx, self.L = self.codec.ctx, self.codec.L
        self.pixel_dtype = self.codec.pixel_dtype
        self.last_tiles_decoded = 0  # tiles the last decode call ran
        self._bufs = {}

    # the device scratch, grow-only per name, and the download: TiledCodec's
    _buf = TiledCodec._buf
    close = TiledCodec.close
    _download = TiledCodec._download

    # ---- device-resident forms ---------------------------------------------------------------------
    def _elem(self, dtype):
        return px.of_dtype(self.pixel_dtype if dtype is None else dtype)

    @staticmethod
    def _strides(dt, c, h, w, strides):
        """the three byte strides (sc, sh, sw) of a view [c, h, w]; None: dense CHW"""
        es = dt.itemsize
        if strides is None:
            return h * w * es, w * es, es
        if len(strides) != 3:
            raise ValueError("a picture's strides are (sc, sh, sw) in bytes")
        return tuple(int(v) for v in strides)

    def encode_device(self, pics, d_packed, d_lens, d_max_n, dtype=None):
        """pics: one (address, H, W, strides | None) per picture: a device address (or an object with .ptr) of a picture
        [c, H, W] of the element `dtype` -- None: the codec's float pixels; np.uint8 / np.uint16 or a float kind's px.Elem
        (tiles.float_elem) laid out by `strides`, BYTES (sc, sh, sw); None: dense CHW.  -> d_packed: the NT streams one behind
        the other (a DeviceArray of uint8; NT * codec.slot_stride bytes always suffice, nothing is written past it), d_lens:
        uint32 [NT] their lengths, d_max_n: uint8 [NT].  Picture p's tiles are rows [tile0_p, tile0_p + T_p), row-major
        (set_tables).  One cut of all pictures (spiht_tile_cut_set), one batched encode of the NT tiles, one pack, queued on the
        codec's context with no host wait; the picture table may be dropped when the call returns, and calls queued back to back
        each see their own."""
        dt = self._elem(dtype)
        pics = list(pics)
        if not pics:
            raise ValueError("encode_device: no pictures")
        rows, NT, vp = (_lib.TileSetPic * len(pics))(), 0, C.c_void_p
        for r, (addr, H, W, strides) in zip(rows, pics):
            H, W = int(H), int(W)
            gy, gx = _grid(H, W, self.th, self.tw)
            NT += gy * gx
            if not dt.view and (dt.storage != self.pixel_dtype or strides is not None):
                raise ValueError("encode_device: %s pictures, the codec's are dense %s" % (dt.storage.name, self.pixel_dtype.name))
            dt.check_aligned(_ptr(addr))
            r.d_img, r.H, r.W = _ptr(addr), H, W
            r.sc, r.sh, r.sw = self._strides(dt, self.c, H, W, strides)
        d_tiles = self._buf("tiles", NT * self.c * self.th * self.tw * dt.itemsize)
        _lib.check(self.L.spiht_tile_cut_set(self.ctx.handle, dt.itemsize, len(pics), self.c, self.th, self.tw, C.byref(rows),
                                             vp(d_tiles.ptr)))
        d_slots = self._buf("slots", NT * self.codec.slot_stride)
        d_nbits = self._buf("nbits", NT * 8)
        self.codec._encode_device(dt, d_tiles.ptr, NT, d_slots.ptr, d_nbits.ptr, _ptr(d_max_n))
        _lib.check(self.L.spiht_tile_pack(self.ctx.handle, vp(d_slots.ptr), self.codec.slot_stride, vp(d_nbits.ptr), NT,
                                          vp(_ptr(d_packed)), int(d_packed.nbytes), vp(_ptr(d_lens))))
        return NT

    def decode_windows_device(self, d_packed, packed_bytes, d_lens, d_max_n, items, outs, dtype=None, slot_stride=None):
        """d_packed / d_lens / d_max_n: the streams, lengths (uint32) and start planes (uint8) of the S tiles the items need, item
        by item, each item's sub-grid in row-major order (set_tables: gather).  items: one (sub, window) per window --
        sub = (i0, i1, j0, j1), or None for the tiles the window meets; window = (y0, x0, h, w) inside the picture, or None for
        all of it.  outs: one (address, H, W, strides | None) per item: where the window [c, h, w] is written, the size of the
        PICTURE it lies in, and the window's BYTE strides (sc, sh, sw) (None: dense CHW; what lies between a view's samples is
        not written).  dtype: the windows' element -- None / np.float64: float64; np.uint8 / np.uint16; a float kind's px.Elem.
        slot_stride: as TiledCodec.decode_window_device.  One unpack, one batched decode of the S tiles, one paste into all
        windows (spiht_tile_paste_set), queued on the codec's context with no host wait.  Returns S."""
        dt = px.of_dtype(np.float64 if dtype is None else dtype)
        if not dt.view and dt is not px.F64:
            raise ValueError("decode: the float form gives float64 pictures")
        items, outs = list(items), list(outs)
        if not items or len(items) != len(outs):
            raise ValueError("decode_windows_device: %d items and %d outputs" % (len(items), len(outs)))
        rows, S, vp = (_lib.TileSetItem * len(items))(), 0, C.c_void_p
        for r, (sub, window), (addr, H, W, strides) in zip(rows, items, outs):
            H, W = int(H), int(W)
            gy, gx = _grid(H, W, self.th, self.tw)
            y0, x0, h, w = (0, 0, H, W) if window is None else (int(v) for v in window)
            need = window_tiles(H, W, self.th, self.tw, y0, x0, h, w)
            i0, i1, j0, j1 = need if sub is None else (int(v) for v in sub)
            if not (0 <= i0 <= need[0] and need[1] <= i1 <= gy and 0 <= j0 <= need[2] and need[3] <= j1 <= gx):
                raise ValueError("the sub-grid %s does not hold the tiles %s of the window %s" % ((i0, i1, j0, j1), need, (y0, x0, h, w)))
            dt.check_aligned(_ptr(addr))
            r.d_out, r.H, r.W = _ptr(addr), H, W
            r.sc, r.sh, r.sw = self._strides(dt, self.c, h, w, strides)
            r.i0, r.i1, r.j0, r.j1, r.y0, r.x0, r.wh, r.ww = i0, i1, j0, j1, y0, x0, h, w
            S += (i1 - i0) * (j1 - j0)
        stride = self.codec.slot_stride if slot_stride is None else int(slot_stride)
        d_slots = self._buf("slots", S * stride)
        d_nbytes = self._buf("nbytes", S * 8)
        _lib.check(self.L.spiht_tile_unpack(self.ctx.handle, vp(_ptr(d_packed)), int(packed_bytes), vp(_ptr(d_lens)), S,
                                            vp(d_slots.ptr), stride, vp(d_nbytes.ptr)))
        # the decoded tiles: float64 ones are the inverse transform's rec_h x rec_w, the others are cropped to the tile
        rh, rw = (self.th, self.tw) if dt.view else (self.codec.geom["rec_h"], self.codec.geom["rec_w"])
        d_dec = self._buf("dec", S * self.c * rh * rw * dt.itemsize)
        self.codec._decode_device(dt, d_slots.ptr, d_nbytes.ptr, _ptr(d_max_n), S, d_dec.ptr, slot_stride=stride)
        _lib.check(self.L.spiht_tile_paste_set(self.ctx.handle, dt.itemsize, len(items), self.c, rh, rw, self.th, self.tw,
                                               C.byref(rows), vp(d_dec.ptr), S))
        self.last_tiles_decoded = S
        return S

    # ---- host forms ----------------------------------------------------------------------------------
    def _encode_host(self, pictures, dtype, channels_last, name, **refused):
        """the frame of every host encode: the checks, ONE upload of all pictures back to back, the device form, one
        synchronise, one download each of the lengths, the start planes and the run"""
        _refuse(name, **refused)
        if isinstance(pictures, np.ndarray) and pictures.ndim == 3:
            raise ValueError("%s takes a list of pictures" % name)
        pictures = list(pictures)
        if not pictures:
            raise ValueError("%s: an empty list of pictures" % name)
        dt = px.of_dtype(dtype)
        if channels_last and not dt.view:
            raise ValueError("%s: channels_last goes with the elements that have views" % name)
        arrs, pics, off = [], [], 0
        for P in pictures:
            P = np.asarray(P)
            if P.ndim != 3:
                raise ValueError("%s takes pictures [c, H, W]" % name)
            if dt.view and not px._is_dtype(P, dt.storage):  # (a float kind goes in as its storage type: bit patterns)
                raise ValueError("%s takes %s arrays, not %s" % (name, dt.storage.name, P.dtype))
            P = np.ascontiguousarray(P, dtype=dt.storage)
            (H, W, c), strides = (P.shape, dt.channels_last_strides((P.shape[2],) + P.shape[:2])) if channels_last else \
                ((P.shape[1], P.shape[2], P.shape[0]), None)
            if c != self.c:
                raise ValueError("%s: a picture of %d channels, the codec's have %d" % (name, c, self.c))
            _grid(H, W, self.th, self.tw)
            arrs.append((off, P))
            pics.append((off, H, W, strides))
            off = _align(off + P.nbytes)
        blob = np.zeros(off, dtype=np.uint8)
        for o, P in arrs:
            blob[o:o + P.nbytes] = P.reshape(-1).view(np.uint8)
        t = set_tables([(H, W) for _, H, W, _ in pics], self.th, self.tw)
        NT = int(t["tile0"][-1])
        d_img = self._buf("img", blob.nbytes)
        self.ctx.upload(d_img.ptr, blob)  # all pictures: one upload
        d_packed = self._buf("packed", NT * self.codec.slot_stride)
        d_lens = self._buf("lens", NT * 4)
        d_maxn = self._buf("maxn", NT)
        self.encode_device([(d_img.ptr + o, H, W, st) for o, H, W, st in pics], d_packed, d_lens, d_maxn, dt)
        self.ctx.synchronize()
        lens = self._download(d_lens.ptr, NT, np.uint32)
        maxn = self._download(d_maxn.ptr, NT, np.uint8)
        ends = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))
        run = self._download(d_packed.ptr, int(ends[-1]), np.uint8)  # the streams of all pictures: one download
        out = []
        for p, (_, H, W, _) in enumerate(pics):
            a, b = int(t["tile0"][p]), int(t["tile0"][p + 1])
            out.append(TiledResult(H, W, self.c, self.th, self.tw, self.level, [int(v) for v in maxn[a:b]],
                                   [int(v) for v in lens[a:b]], run[int(ends[a]):int(ends[b])].tobytes()))
        return out

    def encode(self, pictures, roi=None, target_psnr=None, layers=None):
        """a list of float pictures [c, H_p, W_p] -> the list of their TiledResult: one upload of all pictures back to back, one
        cut, one batched encode of the NT tiles, one pack, and one download each of the lengths, the start planes and the run"""
        return self._encode_host(pictures, self.pixel_dtype, False, "encode", roi=roi, target_psnr=target_psnr, layers=layers)

    def encode_u8(self, pictures, channels_last=False, roi=None, target_psnr=None, layers=None):
        """uint8 pictures [c, H_p, W_p] (or [H_p, W_p, c] with channels_last) -> what encode gives for pictures / 255.0"""
        return self._encode_host(pictures, np.uint8, channels_last, "encode_u8", roi=roi, target_psnr=target_psnr, layers=layers)

    def encode_u16(self, pictures, channels_last=False, roi=None, target_psnr=None, layers=None):
        """uint16 pictures -> what encode gives for pictures / 65535.0"""
        return self._encode_host(pictures, np.uint16, channels_last, "encode_u16", roi=roi, target_psnr=target_psnr, layers=layers)

    def encode_float(self, pictures, dtype=None, channels_last=False, roi=None, target_psnr=None, layers=None):
        """pictures of a float kind (float32, float16, or uint16 bit patterns with dtype="bfloat16"; None: inferred from the first
        picture) -> what encode gives for floatpx.to_float64(pictures, kind), every sample widened exactly on the device"""
        _refuse("encode_float", roi=roi, target_psnr=target_psnr, layers=layers)
        pictures = list(pictures)
        if not pictures:
            raise ValueError("encode_float: an empty list of pictures")
        kind = floatpx.input_kind(np.asarray(pictures[0]), dtype, "encode_float")
        return self._encode_host(pictures, px.of_kind_id(kind), channels_last, "encode_float")

    def _check_result(self, r):
        """ValueError for a result that is not one of this codec's: TiledCodec._check_result's rules, the picture's size free"""
        _check_version(r)
        if getattr(r, "overlap", 0):
            raise ValueError("a result of overlapping tiles (overlap %d, container SPOL): %s" % (r.overlap, _OUT_OF_SCOPE["overlap"]))
        if (r.c, r.th, r.tw, r.level) != (self.c, self.th, self.tw, self.level):
            raise ValueError("a result of c = %d, tiles of %d x %d and level %r; the codec's are %d, %d x %d and %r"
                             % (r.c, r.th, r.tw, r.level, self.c, self.th, self.tw, self.level))
        gy, gx = _grid(r.h, r.w, self.th, self.tw)
        if len(r.nbytes) != gy * gx or len(r.max_n) != gy * gx or sum(r.nbytes) != len(r.encoded_bytes):
            raise ValueError("the tables of the result do not describe %d tiles of %d bytes" % (gy * gx, len(r.encoded_bytes)))

    def _upload_streams(self, results, t):
        """ONE upload of a blob -- the lengths of the S gathered tiles of set_tables' t, their start planes padded to a multiple
        of 4, their bytes -- -> (the device buffer, the offset of the bytes in it, their count, the slot stride that holds the
        longest stream)"""
        S = int(t["s0"][-1])
        lens = np.empty(S, dtype=np.uint32)
        maxn = np.empty(S, dtype=np.uint8)
        parts = []
        for b, r in enumerate(results):
            a, e = int(t["s0"][b]), int(t["s0"][b + 1])
            ts = t["gather"][a:e]
            lens[a:e] = np.asarray(r.nbytes, dtype=np.int64)[ts]
            maxn[a:e] = np.asarray(r.max_n, dtype=np.int64)[ts]
            off = r._offsets()
            data = np.frombuffer(r.encoded_bytes, dtype=np.uint8)
            i0, i1, j0, j1 = t["subs"][b]
            gx = t["grids"][b][1]
            # a row of the sub-grid is contiguous in the run
            parts += [data[int(off[i * gx + j0]):int(off[i * gx + j1])] for i in range(i0, i1)]
        nb = int(lens.sum(dtype=np.int64))
        head = 4 * S + ((S + 3) & ~3)
        blob = np.zeros(head + max(nb, 1), dtype=np.uint8)
        blob[:4 * S] = lens.view(np.uint8)
        blob[4 * S:5 * S] = maxn
        if nb:
            blob[head:head + nb] = np.concatenate(parts)
        d_in = self._buf("in", blob.nbytes)
        self.ctx.upload(d_in.ptr, blob)  # the lengths, the start planes and the streams of the gathered tiles: one upload
        return d_in, head, nb, max(4, (int(lens.max()) + 3) & ~3)

    def _decode_host(self, results, windows, dtype, channels_last, name, crop=None, reduce=0):
        """the frame of every host decode: the checks, the windows and their sub-grids, ONE upload of a blob -- the lengths of
        the S gathered tiles, their start planes padded to a multiple of 4, their bytes --, the device form, one synchronise and
        ONE download of all windows.  crop = (h, w): the windows are crops of that size and the output is one array"""
        _refuse(name, reduce=reduce)
        results = list(results)
        if not results:
            raise ValueError("%s: an empty list of results" % name)
        dt = px.of_dtype(dtype)
        if channels_last and not dt.view:
            raise ValueError("%s: channels_last goes with the elements that have views" % name)
        for r in results:
            self._check_result(r)
        windows = [None] * len(results) if windows is None else list(windows)
        if len(windows) != len(results):
            raise ValueError("%s: %d windows for %d results" % (name, len(windows), len(results)))
        # (a window outside its picture: window_tiles' ValueError, before anything is uploaded)
        t = set_tables([(r.h, r.w) for r in results], self.th, self.tw, list(enumerate(windows)))
        S, B = int(t["s0"][-1]), len(results)
        d_in, head, nb, stride = self._upload_streams(results, t)
        # the windows in one device buffer: crops as one dense array, other windows one behind the other
        es, c = dt.itemsize, self.c
        offs, o = [], 0
        for (_, _, h, w) in t["windows"]:
            offs.append(o)
            o = o + c * h * w * es if crop else _align(o + c * h * w * es)
        d_out = self._buf("out", max(o, 1))
        outs = [(d_out.ptr + oo, r.h, r.w, dt.channels_last_strides((c, h, w)) if channels_last else None)
                for oo, r, (_, _, h, w) in zip(offs, results, t["windows"])]
        self.decode_windows_device(d_in.ptr + head, nb, d_in.ptr, d_in.ptr + 4 * S, list(zip(t["subs"], t["windows"])), outs, dt,
                                   stride)
        self.ctx.synchronize()
        if crop:
            h, w = crop
            out = _lib.result_array((B, h, w, c) if channels_last else (B, c, h, w), dt.storage)
            self.ctx.download(out, d_out.ptr)
            return out
        flat = _lib.result_array((o,), np.uint8)
        self.ctx.download(flat, d_out.ptr)  # all windows: one download
        return [flat[oo:oo + c * h * w * es].view(dt.storage).reshape((h, w, c) if channels_last else (c, h, w))
                for oo, (_, _, h, w) in zip(offs, t["windows"])]

    def decode(self, results, reduce=0):
        """a list of TiledResult -> the list of float64 pictures [c, H_p, W_p], each TiledCodec.decode of its result: one upload
        of the gathered streams, one unpack, one batched decode of all tiles, one paste, one download"""
        return self._decode_host(results, None, np.float64, False, "decode", reduce=reduce)

    def decode_u8(self, results, channels_last=False, reduce=0):
        """-> uint8 pictures [c, H_p, W_p] (or [H_p, W_p, c])"""
        return self._decode_host(results, None, np.uint8, channels_last, "decode_u8", reduce=reduce)

    def decode_u16(self, results, channels_last=False, reduce=0):
        """-> uint16 pictures [c, H_p, W_p] (or [H_p, W_p, c])"""
        return self._decode_host(results, None, np.uint16, channels_last, "decode_u16", reduce=reduce)

    def decode_float(self, results, dtype=np.float32, channels_last=False, reduce=0):
        """-> pictures of the float kind: floatpx.convert(decode(results)[p], dtype), converted on the device"""
        return self._decode_host(results, None, px.of_kind_id(dtype), channels_last, "decode_float", reduce=reduce)

    def decode_windows(self, results, windows, reduce=0):
        """windows: one (y0, x0, h, w) or None (the whole picture) per result -> the list of float64 windows [c, h, w], each
        TiledCodec.decode_window of its result.  Only the tiles each window meets are gathered, uploaded and decoded
        (window_tiles); last_tiles_decoded tells how many.  A window that leaves its picture: ValueError, before anything is
        uploaded."""
        return self._decode_host(results, windows, np.float64, False, "decode_windows", reduce=reduce)

    def decode_windows_u8(self, results, windows, channels_last=False, reduce=0):
        return self._decode_host(results, windows, np.uint8, channels_last, "decode_windows_u8", reduce=reduce)

    def decode_windows_u16(self, results, windows, channels_last=False, reduce=0):
        return self._decode_host(results, windows, np.uint16, channels_last, "decode_windows_u16", reduce=reduce)

    def decode_windows_float(self, results, windows, dtype=np.float32, channels_last=False, reduce=0):
        return self._decode_host(results, windows, px.of_kind_id(dtype), channels_last, "decode_windows_float", reduce=reduce)

    def _crops(self, results, origins, size, dtype, channels_last, name, reduce):
        results, origins = list(results), list(origins)
        if len(origins) != len(results):
            raise ValueError("%s: %d origins for %d results" % (name, len(origins), len(results)))
        h, w = (int(v) for v in size)
        return self._decode_host(results, [(int(y0), int(x0), h, w) for y0, x0 in origins], dtype, channels_last, name, (h, w),
                                 reduce)

    def decode_crops(self, results, origins, size, channels_last=False, reduce=0):
        """origins[b] = (y0, x0), size = (h, w): the crop [y0, y0 + h) x [x0, x0 + w) of every result -> ONE float64 array
        [B, c, h, w], written by the one paste: row b is TiledCodec.decode_window(results[b], y0, x0, h, w).  A result may
        appear several times; its tiles are then gathered and decoded once per appearance.  A crop that leaves its picture:
        ValueError, before anything is uploaded.  channels_last goes with the elements that have views (the forms below:
        [B, h, w, c])."""
        return self._crops(results, origins, size, np.float64, channels_last, "decode_crops", reduce)

    def decode_crops_u8(self, results, origins, size, channels_last=False, reduce=0):
        return self._crops(results, origins, size, np.uint8, channels_last, "decode_crops_u8", reduce)

    def decode_crops_u16(self, results, origins, size, channels_last=False, reduce=0):
        return self._crops(results, origins, size, np.uint16, channels_last, "decode_crops_u16", reduce)

    def decode_crops_float(self, results, origins, size, dtype=np.float32, channels_last=False, reduce=0):
        """-> one array [B, c, h, w] (or [B, h, w, c]) of the float kind; bfloat16 as uint16 bit patterns"""
        return self._crops(results, origins, size, px.of_kind_id(dtype), channels_last, "decode_crops_float", reduce)

    def _axis_tables(self, keys):
        """keys: one (n_in, n_out, flip) per table -> (int64 [T, 2]: every table's byte offset and K, the blob): the tables of
        resample.axis_table -- flip_table'd where flip -- as spiht_tile_resample_set takes them, every distinct key once, written
        by the library's host code (spiht_resample_axis_table: the rule in C, bit for bit) in place of T numpy calls"""
        where, off, K, nb = {}, 0, C.c_int64(), C.c_uint64()
        distinct = list(dict.fromkeys(keys))
        # (the taps of an output span 2 * support samples: at most ceil(2 * support) + 1 of them)
        cap = sum(8 * n_out * (2 + int(np.ceil(2.0 * max(n_in / n_out, 1.0)))) for n_in, n_out, _ in distinct)
        blob = np.empty(cap, dtype=np.uint8)
        for key in distinct:
            n_in, n_out, flip = key
            _lib.check(self.L.spiht_resample_axis_table(n_in, n_out, int(flip), C.c_void_p(blob.ctypes.data + off), cap - off,
                                                        C.byref(K), C.byref(nb)))
            where[key] = (off, K.value)
            off += nb.value
        return np.asarray([where[k] for k in keys], dtype=np.int64), blob[:off]

    # ---- resized crops: a box of any size of every picture, resampled to one size (resample.py) ------------------------
    # Row b of every call below is, bit for bit,
    #     resample.resize_rule(TiledCodec.decode_window(results[b], y0, x0, h, w), (oh, ow), flip=flips[b], mean=mean, std=std,
    #                          dtype=kind)
    # -- the crop first, then the resize: samples outside the box never contribute.  The tiles are decoded to float64 whatever the
    # output's kind and each output sample is rounded once, at the kernel's store (csrc/resample.hip).
    def decode_resized_device(self, d_packed, packed_bytes, d_lens, d_max_n, items, d_out, size, dtype=None, out_strides=None,
                              flips=None, mean=None, std=None, slot_stride=None):
        """d_packed / d_lens / d_max_n / slot_stride: as decode_windows_device.  items: one (sub, box, (H, W)) per output row --
        box = (y0, x0, h, w) inside its H x W picture, sub = (i0, i1, j0, j1) or None for the tiles the box meets.  d_out: a
        device address (or an object with .ptr) of the output [B, c, oh, ow], size = (oh, ow), laid out by the BYTE strides
        out_strides = (sb, sc, sh, sw) (None: dense; what lies between a view's samples is not written).  dtype: the output's
        element -- None / np.float64, np.uint8 / np.uint16, or a float kind's px.Elem (tiles.float_elem).  flips: B booleans or
        None; mean / std: one value per channel, both or neither, not with 8 / 16 bits.  One unpack, one batched float64 decode
        of the S tiles, one resample of all boxes (spiht_tile_resample_set), queued on the codec's context with no host wait;
        the tables may be dropped when the call returns.  Returns S."""
        dt = px.of_dtype(np.float64 if dtype is None else dtype)
        if not dt.view and dt is not px.F64:
            raise ValueError("decode_resized_device: the float form gives float64 pictures")
        items = list(items)
        B, c, vp = len(items), self.c, C.c_void_p
        if not items:
            raise ValueError("decode_resized_device: no items")
        flips = [False] * B if flips is None else [bool(f) for f in flips]
        if len(flips) != B:
            raise ValueError("decode_resized_device: %d flips for %d items" % (len(flips), B))
        mean, std = resample.norm_args(mean, std, c, dt, "decode_resized_device")
        oh, ow = (int(v) for v in size)
        es = dt.itemsize
        sb, sc, sh, sw = (c * oh * ow * es, oh * ow * es, ow * es, es) if out_strides is None else (int(v) for v in out_strides)
        dt.check_aligned(_ptr(d_out))
        if out_strides is not None and dt.view:  # (a float64 view: the library's check)
            dt.check_view((B, c, oh, ow), (sb, sc, sh, sw), True)
        rows, keys, S = (_lib.TileSetItem * B)(), [], 0
        for b, (r, (sub, box, (H, W)), flip) in enumerate(zip(rows, items, flips)):
            H, W = int(H), int(W)
            gy, gx = _grid(H, W, self.th, self.tw)
            y0, x0, h, w, _, _ = resample.check_box(H, W, box, (oh, ow), "decode_resized_device")
            need = window_tiles(H, W, self.th, self.tw, y0, x0, h, w)
            i0, i1, j0, j1 = need if sub is None else (int(v) for v in sub)
            if not (0 <= i0 <= need[0] and need[1] <= i1 <= gy and 0 <= j0 <= need[2] and need[3] <= j1 <= gx):
                raise ValueError("the sub-grid %s does not hold the tiles %s of the box %s" % ((i0, i1, j0, j1), need, (y0, x0, h, w)))
            r.d_out, r.H, r.W = _ptr(d_out) + b * sb, H, W
            r.sc, r.sh, r.sw = sc, sh, sw
            r.i0, r.i1, r.j0, r.j1, r.y0, r.x0, r.wh, r.ww = i0, i1, j0, j1, y0, x0, h, w
            S += (i1 - i0) * (j1 - j0)
            keys += [(w, ow, flip), (h, oh, False)]
        tabs, tables = self._axis_tables(keys)
        tabs = tabs.reshape(B, 4)
        stride = self.codec.slot_stride if slot_stride is None else int(slot_stride)
        d_slots = self._buf("slots", S * stride)
        d_nbytes = self._buf("nbytes", S * 8)
        _lib.check(self.L.spiht_tile_unpack(self.ctx.handle, vp(_ptr(d_packed)), int(packed_bytes), vp(_ptr(d_lens)), S,
                                            vp(d_slots.ptr), stride, vp(d_nbytes.ptr)))
        rh, rw = self.codec.geom["rec_h"], self.codec.geom["rec_w"]  # the tiles are decoded to float64 whatever the output
        d_dec = self._buf("dec", S * c * rh * rw * 8)
        self.codec._decode_device(px.F64, d_slots.ptr, d_nbytes.ptr, _ptr(d_max_n), S, d_dec.ptr, slot_stride=stride)
        _lib.check(self.L.spiht_tile_resample_set(
            self.ctx.handle, dt.stream_id, B, c, rh, rw, self.th, self.tw, oh, ow, C.byref(rows), vp(tabs.ctypes.data),
            vp(tables.ctypes.data), tables.nbytes, None if mean is None else vp(mean.ctypes.data),
            None if std is None else vp(std.ctypes.data), vp(d_dec.ptr), S))
        self.last_tiles_decoded = S
        return S

    def _resized(self, results, boxes, size, flips, mean, std, dtype, channels_last, name, reduce=0):
        """the frame of the host forms: the checks, ONE upload of the gathered streams (_upload_streams), the device form, one
        synchronise and ONE download of the [B, ...] array"""
        _refuse(name, reduce=reduce)
        results, boxes = list(results), list(boxes)
        if not results:
            raise ValueError("%s: an empty list of results" % name)
        if len(boxes) != len(results):
            raise ValueError("%s: %d boxes for %d results" % (name, len(boxes), len(results)))
        dt = px.of_dtype(dtype)
        if channels_last and not dt.view:
            raise ValueError("%s: channels_last goes with the elements that have views" % name)
        for r in results:
            self._check_result(r)
        flips = None if flips is None else list(flips)
        if flips is not None and len(flips) != len(results):
            raise ValueError("%s: %d flips for %d results" % (name, len(flips), len(results)))
        resample.norm_args(mean, std, self.c, dt, name)
        oh, ow = (int(v) for v in size)
        boxes = [resample.check_box(r.h, r.w, box, (oh, ow), name)[:4] for r, box in zip(results, boxes)]
        t = set_tables([(r.h, r.w) for r in results], self.th, self.tw, list(enumerate(boxes)))
        S, B, c = int(t["s0"][-1]), len(results), self.c
        d_in, head, nb, stride = self._upload_streams(results, t)
        d_out = self._buf("out", B * c * oh * ow * dt.itemsize)
        self.decode_resized_device(d_in.ptr + head, nb, d_in.ptr, d_in.ptr + 4 * S,
                                   [(sub, box, (r.h, r.w)) for sub, box, r in zip(t["subs"], boxes, results)], d_out.ptr, (oh, ow),
                                   dt, dt.channels_last_strides((B, c, oh, ow)) if channels_last else None, flips, mean, std,
                                   stride)
        self.ctx.synchronize()
        out = _lib.result_array((B, oh, ow, c) if channels_last else (B, c, oh, ow), dt.storage)
        self.ctx.download(out, d_out.ptr)
        return out

    def decode_resized_crops(self, results, boxes, size, flips=None, mean=None, std=None, reduce=0):
        """boxes[b] = (y0, x0, h, w) inside picture b, size = (oh, ow) -> ONE float64 array [B, c, oh, ow]: row b is
        resample.resize_rule(TiledCodec.decode_window(results[b], y0, x0, h, w), size, flips[b], mean, std).  Only the tiles each
        box meets are gathered, uploaded and decoded (last_tiles_decoded tells how many); a result may appear several times.  A
        box that is empty, leaves its picture or has a side above resample.MAX_RATIO output sides: ValueError, before anything
        is uploaded."""
        return self._resized(results, boxes, size, flips, mean, std, np.float64, False, "decode_resized_crops", reduce)

    def decode_resized_crops_u8(self, results, boxes, size, flips=None, channels_last=False, reduce=0):
        """-> uint8 [B, c, oh, ow] (or [B, oh, ow, c]): the resampled sample clipped to [0, 1], times 255, truncated"""
        return self._resized(results, boxes, size, flips, None, None, np.uint8, channels_last, "decode_resized_crops_u8", reduce)

    def decode_resized_crops_u16(self, results, boxes, size, flips=None, channels_last=False, reduce=0):
        return self._resized(results, boxes, size, flips, None, None, np.uint16, channels_last, "decode_resized_crops_u16", reduce)

    def decode_resized_crops_float(self, results, boxes, size, flips=None, mean=None, std=None, dtype=np.float32,
                                   channels_last=False, reduce=0):
        """-> one array [B, c, oh, ow] (or [B, oh, ow, c]) of the float kind, every sample rounded once from the float64
        resample; bfloat16 as uint16 bit patterns"""
        return self._resized(results, boxes, size, flips, mean, std, px.of_kind_id(dtype), channels_last,
                             "decode_resized_crops_float", reduce)
