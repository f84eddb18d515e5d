"""The row words of the inverse transform's level 1 (common.h: L1Flags.rows): bit r of a tile's row word says that band row r
of the region the tile stages -- its 12 band rows and the F/2 - 1 halo rows behind them, every staged column, any of the three
level-1 detail bands -- holds a decoded cell.  The list decoder sets them (spiht_decode_lists_rows_batch_i32); the inverse
level-1 kernels neither read nor filter a detail row whose bit is clear (spiht_idwt_level1_rows_batch_*).  Checked here: the
decoder's words against numpy; the inverse alone on hand-made arrays whose masks are exactly the rows that hold a cell, through
the workgroup-per-tile and the persistent kernel; planes whose zeros do not dequantise to +0.0; the round trip against the
oracle; the pipelined schedule.  Every comparison of pictures is equality of bits.

The shape: 60 x 300 pictures, whose level 1 is 3 x 3 tiles of 24 x 128 outputs with partial last ones -- the smallest at which a
tile has neighbours on both sides; two channels, two pictures; halos of 0, 2, 4, 8 and 9 band positions."""
import ctypes as C

import numpy as np
import pytest

import dwt_sweep_tables as T
from conftest import synth_image
from test_gpu_dwt_sweep import _Bufs, _geometry, _mults_ptr, same_bits

pytestmark = pytest.mark.gpu
vp = C.c_void_p

WAVELETS = ["haar", "bior2.2", "bior4.4", "bior6.8", "db10"]  # F = 2, 6, 10, 18, 20
H0, W0, C0, B0 = 60, 300, 2, 2
TR, TC = T.INV_TH // 2, T.INV_TW // 2  # band rows / columns of a tile: 12, 64
DTYPE = {"f64": np.float64, "u8": np.uint8, "u16": np.uint16}
SENTINEL = {"u8": 0xA5, "u16": 0xA55A}
KINDS = [("f64", False), ("u8", False), ("u8", True), ("u16", False), ("u16", True)]  # (pixel kind, padded and strided view)


def _F(oracle, wavelet):
    return len(oracle.wavelet_filters(wavelet)[0])


def numpy_masks(rec, H, W, F):
    """packed arrays [.., enc_h, enc_w] -> (words, row words) [.., gy, gx] as common.h defines them, from the cells that are
    not zero"""
    bands = T.level1_detail_bands(rec, H, W, F)
    occ = (bands[0] != 0) | (bands[1] != 0) | (bands[2] != 0)
    hs, ws = occ.shape[-2:]
    gy, gx = T.tiles(2 * hs - F + 2, T.INV_TH), T.tiles(2 * ws - F + 2, T.INV_TW)
    rows = np.zeros(occ.shape[:-2] + (gy, gx), np.uint32)
    for ty in range(gy):
        for tx in range(gx):
            r, c = T.staged(ty, tx, F)
            in_row = occ[..., r, c].any(axis=-1)  # [.., staged rows inside the band]
            for i in range(in_row.shape[-1]):
                rows[..., ty, tx] |= in_row[..., i].astype(np.uint32) << np.uint32(i)
    return (rows != 0).astype(np.uint32), rows


def int_buffer(kind, B, c, H, W, strided):
    """-> (host buffer filled with the sentinel, byte strides or None for dense CHW, view [B, c, H, W] of the pixels in it);
    strided: c + 1 samples per pixel and 12 bytes behind every row"""
    dt = np.dtype(DTYPE[kind])
    es = dt.itemsize
    if not strided:
        buf = np.full((B, c, H, W), SENTINEL[kind], dt)
        return buf, None, buf
    pitch = (c + 1) * W * es + 12
    buf = np.full((B, H, pitch // es), SENTINEL[kind], dt)
    view = buf[:, :, :(c + 1) * W].reshape(B, H, W, c + 1)[..., :c].transpose(0, 3, 1, 2)
    return buf, (H * pitch, es, pitch, (c + 1) * es), view


class Level1:
    """level 1 of the inverse transform of one device-resident (rec, approximation) pair, called in its several forms"""

    def __init__(self, d, rec, approx, H, W, wavelet, level, q, mults):
        self.d, self.L = d, d.L
        self.B, self.c = rec.shape[:2]
        self.H, self.W, self.level, self.q = H, W, level, float(q)
        self.wid, self.mid = d.L.spiht_wavelet_id(wavelet.encode()), d.L.spiht_mode_id(b"reflect")
        self.g = _geometry(d.L, d.check, H, W, self.wid, self.mid, level)
        assert rec.shape[2:] == (self.g[2], self.g[3])
        self.m, self.mp = _mults_ptr(mults)
        self.d_rec, self.d_ap = d.put(rec), d.put(approx)

    def tail(self):
        return (self.B, self.c, self.H, self.W, self.wid, self.mid, self.level, self.q, self.mp)

    def run(self, kind, strided, words=None, rows=None, entry="rows"):
        """entry "rows": spiht_idwt_level1_rows_batch_*; "flags": the _flags_ calls (rows unused); "plain": float64 without words"""
        d, L = self.d, self.L
        p_w = None if words is None else vp(d.put(np.ascontiguousarray(words, np.uint32)))
        p_r = None if rows is None else vp(d.put(np.ascontiguousarray(rows, np.uint32)))
        head = (d.ctx.handle, vp(self.d_rec), vp(self.d_ap))
        if kind == "f64":
            out = np.empty((self.B, self.c, self.g[4], self.g[5]), np.float64)
            d_out = d.new(out.nbytes, 0xFF)
            if entry == "plain":
                d.check(L.spiht_idwt_level1_batch_f64(*head, *self.tail(), vp(d_out)))
            elif entry == "flags":
                d.check(L.spiht_idwt_level1_flags_batch_f64(*head, p_w, *self.tail(), vp(d_out)))
            else:
                d.check(L.spiht_idwt_level1_rows_batch_f64(*head, p_w, p_r, *self.tail(), vp(d_out)))
            d.ctx.download(out, d_out)
            return out
        buf, strides, view = int_buffer(kind, self.B, self.c, self.H, self.W, strided)
        st = None if strides is None else np.array(strides, np.int64)
        p_st = None if st is None else vp(st.ctypes.data)
        d_out = d.put(buf)
        if entry == "rows":
            fn = L.spiht_idwt_level1_rows_batch_u8 if kind == "u8" else L.spiht_idwt_level1_rows_batch_u16
            d.check(fn(*head, p_w, p_r, *self.tail(), vp(d_out), p_st))
        else:
            fn = L.spiht_idwt_level1_flags_batch_u8 if kind == "u8" else L.spiht_idwt_level1_flags_batch_u16
            d.check(fn(*head, p_w, *self.tail(), vp(d_out), p_st))
        d.ctx.download(buf, d_out)
        if strided:  # the spare sample of every pixel and the bytes behind every row are what they were
            B, H, W, c = self.B, self.H, self.W, self.c
            assert (buf[:, :, :(c + 1) * W].reshape(B, H, W, c + 1)[..., c] == SENTINEL[kind]).all()
            assert (buf[:, :, (c + 1) * W:] == SENTINEL[kind]).all()
        return np.ascontiguousarray(view)


def coarse_approx(rec, H, W, wavelet, level, q, mults):
    """the approximation level 1 starts from, [B * c, a_h, a_w], by spiht_idwt_coarse_batch_f64"""
    B, c = rec.shape[:2]
    with _Bufs() as d:
        L = d.L
        wid, mid = L.spiht_wavelet_id(wavelet.encode()), L.spiht_mode_id(b"reflect")
        a_h, a_w = C.c_int64(), C.c_int64()
        d.check(L.spiht_idwt_approx_shape(H, W, wid, level, C.byref(a_h), C.byref(a_w)))
        ap = np.empty((B * c, a_h.value, a_w.value), np.float64)
        d_rec, d_ap = d.put(rec), d.new(ap.nbytes, 0xFF)
        m, mp = _mults_ptr(mults)
        d.check(L.spiht_idwt_coarse_batch_f64(d.ctx.handle, vp(d_rec), B, c, H, W, wid, mid, level, float(q), mp, vp(d_ap)))
        d.ctx.download(ap, d_ap)
    return ap


VALUES = [1, -1, 2 ** 30, -(2 ** 30)]


def handmade(oracle, wavelet, level, band_sel, mults):
    """-> (rec int32 [2, 2, enc_h, enc_w], approximation float64 [4, a_h, a_w]).  The approximation comes from a real coarse run
    of a thinned-out quantised array, with -0.0 and denormals put into it; the level-1 detail bands are zero except single cells
    of value +-1, +-2^30 in band `band_sel` (None: the bands in turn): tile-local rows 0, hf1 - 1, hf1, 11 of the first two tile
    rows -- those of the second are the halo rows 12 .. 12 + hf1 - 1 of the first --, the band's last row, the same set in
    columns (0, hf1 - 1, 63 and the halo columns 64 .. 64 + hf1 - 1, the last column): the four corners are among them.  The
    cells go to the four planes in turn, so that most rows of most tiles stay empty.  Plane 0 also gets two cells of different
    bands in one row."""
    F = _F(oracle, wavelet)
    hf1 = F // 2 - 1
    rec = np.stack([T.inverse_case(oracle, wavelet, H0, W0, level, 300 + b, mults, c=C0)[0] for b in range(B0)])
    approx = coarse_approx(rec, H0, W0, wavelet, level, T.Q, mults)
    approx[:, 0, 0] = -0.0
    approx[:, 1, 2] = 5e-324
    approx[:, 2, 1] = -1.1e-308
    approx[:, -1, -1] = -0.0
    approx[1::2, 7, 70:80] = -0.0
    bands = T.level1_detail_bands(rec, H0, W0, F)
    for b in bands:
        b[...] = 0
    hs, ws = bands[0].shape[-2:]
    rset = sorted({r for r in (0, hf1 - 1, hf1, TR - 1, TR, TR + hf1 - 1, TR + hf1, 2 * TR - 1, hs - 1) if 0 <= r < hs})
    cset = sorted({c for c in (0, hf1 - 1, TC - 1, TC, TC + hf1 - 1, ws - 1) if 0 <= c < ws})
    i = 0
    for r in rset:
        for c in cset:
            band = bands[band_sel if band_sel is not None else i % 3]
            band[(i % 4) // C0, (i % 4) % C0, r, c] = VALUES[(i + i // 4) % 4]
            i += 1
    k = 0 if band_sel is None else band_sel
    bands[(k + 1) % 3][0, 0, 5, 10] = 1
    bands[(k + 2) % 3][0, 0, 5, 100] = -1
    return rec, approx


def mask_variants(rows, F, seed):
    """the exact row words; the same with random further bits; every bit of every word -> [(name, words, rows)]"""
    rng = np.random.default_rng(seed)
    extra = rows | (rng.integers(0, 1 << (TR + F // 2 - 1), rows.shape, dtype=np.uint32) & rng.integers(0, 2, rows.shape, dtype=np.uint32) * np.uint32(0xFFFFFFFF))
    ones = np.full(rows.shape, 0xFFFFFFFF, np.uint32)
    return [("exact", (rows != 0).astype(np.uint32), rows), ("extra", (extra != 0).astype(np.uint32), extra),
            ("ones", np.ones(rows.shape, np.uint32), ones)]


# ---- 1. + 4. the decoder's row words against numpy; the round trip ------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 3])
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_decoder_row_words_and_round_trip(oracle, wavelet, level):
    """Streams of the encoder at 0.1 / 0.5 / 2 bpp and three byte strings no encoder made: every staged row, halo included, of
    every tile that holds a non-zero detail cell has its bit; no bit in a tile whose word is 0 and none at or above 12 + hf1;
    the words are those of spiht_decode_lists_flags_batch_i32.  The encoder's streams go on through coarse levels and
    spiht_idwt_level1_rows_batch_f64: the oracle's picture, also by the _flags_ route and by the image-level decode call."""
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec
    from spiht_amd.spiht_wrapper import SpihtSettings
    F = _F(oracle, wavelet)
    hf1 = F // 2 - 1
    s = SpihtSettings(wavelet=wavelet)
    q = float(s.quantization_scale)
    imgs = np.stack([synth_image(820 + b, C0, H0, W0) for b in range(B0)])
    junk_rng = np.random.default_rng(23)
    for bpp in (0.1, 0.5, 2.0, "junk0", "junk1", "junk2"):
        junk = isinstance(bpp, str)
        mb = int(H0 * W0 * (2.0 if junk else bpp))
        cd = BatchCodec(C0, H0, W0, s, level, mb, ctx=_lib.default_context())
        g = cd.geom
        assert g["level"] == level
        if junk:
            stride = 4096
            data = junk_rng.integers(0, 256, (B0, stride), dtype=np.uint8)
            nbytes, maxn = np.array([stride - 3 * int(bpp[-1]), stride // 2], np.uint64), np.array([9 + int(bpp[-1]), 6], np.uint8)
        else:
            res = cd.encode(imgs)
            stride = max(4, (max(len(r.encoded_bytes) for r in res) + 3) & ~3)
            data = np.zeros((B0, stride), np.uint8)
            for b, r in enumerate(res):
                data[b, :len(r.encoded_bytes)] = np.frombuffer(r.encoded_bytes, np.uint8)
            nbytes, maxn = np.array([len(r.encoded_bytes) for r in res], np.uint64), np.array([r.max_n for r in res], np.uint8)
        with _Bufs() as d:
            L = d.L
            nw = C.c_uint64()
            d.check(L.spiht_l1_flags_words(C0, H0, W0, cd.wid, cd.mid, cd._lv, C.byref(nw)))
            n_words = B0 * nw.value
            assert n_words == B0 * C0 * 9
            d_data, d_nb, d_mn = d.put(data), d.put(nbytes), d.put(maxn)
            rec = np.empty((B0, C0, g["enc_h"], g["enc_w"]), np.int32)
            head = (d.ctx.handle, vp(d_data), stride, vp(d_nb), vp(d_mn), B0, C0, H0, W0, cd.wid, cd.mid, cd._lv)
            # the words alone, then words and rows as one buffer (one fill), then as two
            d_rec = d.new(rec.nbytes, 0)
            d_fl = d.new(4 * n_words, 0xEE)
            d.check(L.spiht_decode_lists_flags_batch_i32(*head, vp(d_rec), vp(d_fl)))
            words_f = np.empty((B0, C0, 3, 3), np.uint32)
            d.ctx.download(words_f, d_fl)
            got = []
            for one in (True, False):
                d_rec2 = d.new(rec.nbytes, 0)
                d_w = d.new(8 * n_words, 0xEE)
                d_r = d_w + 4 * n_words if one else d.new(4 * n_words, 0xEE)
                d.check(L.spiht_decode_lists_rows_batch_i32(*head, vp(d_rec2), vp(d_w), vp(d_r)))
                words, rows = np.empty((B0, C0, 3, 3), np.uint32), np.empty((B0, C0, 3, 3), np.uint32)
                d.ctx.download(words, d_w)
                d.ctx.download(rows, d_r)
                d.ctx.download(rec, d_rec2)
                got.append((words.copy(), rows.copy(), rec.copy()))
            assert all(np.array_equal(a, b) for a, b in zip(got[0], got[1]))
            words, rows, rec = got[0]
            assert np.array_equal(words, words_f) and set(np.unique(words)) <= {0, 1}
            want_words, want_rows = numpy_masks(rec, H0, W0, F)
            assert not (want_rows & ~rows).any(), (wavelet, level, bpp, np.argwhere(want_rows & ~rows)[:4].tolist())
            assert not rows[words == 0].any() and not (rows >> np.uint32(TR + hf1)).any()
            assert not (want_words & ~words).any()
            assert np.array_equal(rows != 0, words != 0)  # (every cell that sets a word sets a bit of the same tile)
            # the inverse: coarse levels, then level 1 by row words, by words, without
            ap = coarse_approx(rec, H0, W0, wavelet, level, q, None)
            l1 = Level1(d, rec, ap, H0, W0, wavelet, level, q, None)
            by_rows = l1.run("f64", False, words, rows)
            assert same_bits(by_rows, l1.run("f64", False, entry="plain")), (wavelet, level, bpp)
            assert same_bits(by_rows, l1.run("f64", False, words, entry="flags"))
            assert same_bits(by_rows, l1.run("f64", False, words, None))  # (no row words: the _flags_ call)
            for kind, strided in KINDS[1:]:
                assert same_bits(l1.run(kind, strided, words, rows), l1.run(kind, strided, entry="flags")), (kind, strided, bpp)
        if not junk:
            dec = cd.decode(res)  # the image-level call: decoder, words and row words, inverse, inside the library
            for b in range(B0):
                ref = oracle.decode_image(res[b].encoded_bytes, res[b].max_n, C0, H0, W0, wavelet, level, q, None)
                assert same_bits(by_rows[b], ref), (wavelet, level, bpp, b)
                assert same_bits(np.asarray(dec[b]), ref)


def test_one_level_has_no_words(oracle):
    """a transform of one level has no words (spiht_l1_flags_words == 0): both pointers are ignored and left alone"""
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec
    from spiht_amd.spiht_wrapper import SpihtSettings
    s = SpihtSettings(wavelet="bior2.2")
    cd = BatchCodec(C0, H0, W0, s, 1, int(H0 * W0 * 1.0), ctx=_lib.default_context())
    g = cd.geom
    imgs = np.stack([synth_image(840 + b, C0, H0, W0) for b in range(B0)])
    res = cd.encode(imgs)
    stride = (max(len(r.encoded_bytes) for r in res) + 3) & ~3
    data = np.zeros((B0, stride), np.uint8)
    for b, r in enumerate(res):
        data[b, :len(r.encoded_bytes)] = np.frombuffer(r.encoded_bytes, np.uint8)
    with _Bufs() as d:
        L = d.L
        nw = C.c_uint64(7)
        d.check(L.spiht_l1_flags_words(C0, H0, W0, cd.wid, cd.mid, cd._lv, C.byref(nw)))
        assert nw.value == 0
        d_data = d.put(data)
        d_nb, d_mn = d.put(np.array([len(r.encoded_bytes) for r in res], np.uint64)), d.put(np.array([r.max_n for r in res], np.uint8))
        rec = np.empty((B0, C0, g["enc_h"], g["enc_w"]), np.int32)
        d_rec = d.new(rec.nbytes, 0)
        guard = np.full(64, 0xEEEEEEEE, np.uint32)
        d_w, d_r = d.put(guard), d.put(guard)
        d.check(L.spiht_decode_lists_rows_batch_i32(d.ctx.handle, vp(d_data), stride, vp(d_nb), vp(d_mn), B0, C0, H0, W0, cd.wid, cd.mid,
                                                    cd._lv, vp(d_rec), vp(d_w), vp(d_r)))
        d.ctx.download(rec, d_rec)
        out = [np.empty((B0, C0, g["rec_h"], g["rec_w"]), np.float64) for _ in range(2)]
        for o, (w, r) in zip(out, ((vp(d_w), vp(d_r)), (None, None))):
            d_out = d.new(o.nbytes, 0xFF)
            d.check(L.spiht_idwt_level1_rows_batch_f64(d.ctx.handle, vp(d_rec), None, w, r, B0, C0, H0, W0, cd.wid, cd.mid, cd._lv,
                                                       float(s.quantization_scale), None, vp(d_out)))
            d.ctx.download(o, d_out)
        for p in (d_w, d_r):
            back = np.empty_like(guard)
            d.ctx.download(back, p)
            assert np.array_equal(back, guard)
    assert same_bits(out[0], out[1])
    for b in range(B0):
        ref = oracle.decode_image(res[b].encoded_bytes, res[b].max_n, C0, H0, W0, "bior2.2", 1, float(s.quantization_scale), None)
        assert same_bits(out[0][b], ref)


# ---- 2. the inverse alone: hand-made arrays, minimal masks --------------------------------------------------------------------
@pytest.mark.parametrize("band", [0, 1, 2])
@pytest.mark.parametrize("level", [2, 3])
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_inverse_with_minimal_masks(oracle, wavelet, level, band):
    """the workgroup-per-tile kernel (two pictures): every mask variant, every pixel kind and layout, against the call without
    words on the same arrays"""
    F = _F(oracle, wavelet)
    mults = None if level == 2 else [2.0, 0.75]
    rec, approx = handmade(oracle, wavelet, level, band, mults)
    _, rows = numpy_masks(rec, H0, W0, F)
    assert (rows != 0).any() and (rows == 0).any()
    with _Bufs() as d:
        l1 = Level1(d, rec, approx, H0, W0, wavelet, level, T.Q, mults)
        for kind, strided in KINDS:
            want = l1.run(kind, strided, entry="plain" if kind == "f64" else "flags")
            for name, w, r in mask_variants(rows, F, 5 + band):
                got = l1.run(kind, strided, w, r)
                assert same_bits(got, want), (wavelet, level, band, kind, strided, name, np.argwhere(got != want)[:4].tolist())


PF_B = -(-T.PF_MIN // (C0 * 9))  # pictures from which launch_idwt_FM takes the persistent kernel at 9 tiles per plane


@pytest.mark.parametrize("level", [2, 3])
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_inverse_with_minimal_masks_persistent(oracle, wavelet, level):
    """the persistent kernel: the two hand-made pictures repeated to 20 000 tiles and more; picture b is that of array b % 2 by
    the call without words"""
    F = _F(oracle, wavelet)
    assert PF_B * C0 * 9 >= T.PF_MIN
    mults = None if level == 3 else [0.5, 3.0]
    rec, approx = handmade(oracle, wavelet, level, None, mults)
    _, rows = numpy_masks(rec, H0, W0, F)
    idx = np.arange(PF_B) % B0
    with _Bufs() as d:
        small = Level1(d, rec, approx, H0, W0, wavelet, level, T.Q, mults)
        want = {"f64": small.run("f64", False, entry="plain"), "u8": small.run("u8", False, entry="flags"),
                "u16": small.run("u16", True, entry="flags")}
    variants = mask_variants(rows, F, 11)
    with _Bufs() as d:
        big = Level1(d, rec[idx], approx.reshape((B0, C0) + approx.shape[1:])[idx].reshape((-1,) + approx.shape[1:]), H0, W0, wavelet,
                     level, T.Q, mults)
        for kind, strided, names in (("f64", False, ("exact", "extra")), ("u8", False, ("exact",)), ("u16", True, ("extra",))):
            for name, w, r in variants:
                if name not in names:
                    continue
                got = big.run(kind, strided, w[idx], r[idx])
                for k in range(B0):
                    part = got[k::B0]
                    assert same_bits(part, np.broadcast_to(want[kind][k], part.shape)), (wavelet, level, kind, name, k)


# ---- 3. zeros that do not dequantise to +0.0 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", [False, True])
def test_negative_channel_scale_takes_the_full_path(oracle, persistent):
    """a negative scale on one channel: 0 / m / q is -0.0 there and the kernels take no row's fast path; equal to the call without
    words, in the workgroup-per-tile kernel and in the persistent one"""
    wavelet, level, mults = "bior2.2", 2, [-1.5, 2.0]
    F = _F(oracle, wavelet)
    rec, approx = handmade(oracle, wavelet, level, None, mults)
    _, rows = numpy_masks(rec, H0, W0, F)
    with _Bufs() as d:
        small = Level1(d, rec, approx, H0, W0, wavelet, level, T.Q, mults)
        want = small.run("f64", False, entry="plain")
        if not persistent:
            for name, w, r in mask_variants(rows, F, 3):
                assert same_bits(small.run("f64", False, w, r), want), name
                assert same_bits(small.run("u8", True, w, r), small.run("u8", True, entry="flags")), name
            return
    idx = np.arange(PF_B) % B0
    with _Bufs() as d:
        big = Level1(d, rec[idx], approx.reshape((B0, C0) + approx.shape[1:])[idx].reshape((-1,) + approx.shape[1:]), H0, W0, wavelet,
                     level, T.Q, mults)
        got = big.run("f64", False, (rows != 0).astype(np.uint32)[idx], rows[idx])
        for k in range(B0):
            part = got[k::B0]
            assert same_bits(part, np.broadcast_to(want[k], part.shape)), k


# ---- 5. the pipelined schedule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "u8"])
def test_pipeline_steps(kind):
    """three steps of a two-picture pipeline at the small shape: streams and pictures are those of the serial calls"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray, Pipeline
    steps, level, mb = 3, 3, int(H0 * W0 * 0.5)
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(C0, H0, W0, s, level=level, max_bits=mb)
    g, ctx = codec.geom, codec.ctx
    pl = Pipeline(codec, B0)
    f64 = kind == "f64"
    if f64:
        imgs = [np.stack([synth_image(860 + 10 * st + b, C0, H0, W0) for b in range(B0)]) for st in range(steps)]
    else:
        imgs = [np.stack([np.round(synth_image(860 + 10 * st + b, C0, H0, W0).clip(0, 1) * 255).astype(np.uint8) for b in range(B0)])
                for st in range(steps)]
    dt = np.float64 if f64 else np.uint8
    d_in = [DeviceArray(ctx, (B0, C0, H0, W0), dt) for _ in range(steps)]
    d_pic = [DeviceArray(ctx, (B0, C0, g["rec_h"], g["rec_w"]) if f64 else (B0, C0, H0, W0), dt) for _ in range(steps)]
    d_out = [DeviceArray(ctx, (B0, pl.slot_stride), np.uint8) for _ in range(steps)]
    d_nbits = [DeviceArray(ctx, (B0,), np.uint64) for _ in range(steps)]
    d_maxn = [DeviceArray(ctx, (B0,), np.uint8) for _ in range(steps)]
    for st in range(steps):
        d_in[st].upload(imgs[st])
    ctx.synchronize()
    for st in range(steps):
        if f64:
            pl.submit(d_in[st].ptr, d_out[st].ptr, d_nbits[st].ptr, d_maxn[st].ptr, d_pic[st].ptr)
        else:
            pl.submit_u8(d_in[st].ptr, d_out[st].ptr, d_nbits[st].ptr, d_maxn[st].ptr, d_pic[st].ptr)
    pl.flush()
    pl.synchronize()
    for st in range(steps):
        res = codec.encode(imgs[st]) if f64 else codec.encode_u8(imgs[st])
        nb, out, mn = d_nbits[st].download(), d_out[st].download(), d_maxn[st].download()
        for b in range(B0):
            assert (int(nb[b]) + 7) // 8 == len(res[b].encoded_bytes) and int(mn[b]) == res[b].max_n
            assert out[b, :len(res[b].encoded_bytes)].tobytes() == res[b].encoded_bytes
        want = np.stack([np.asarray(p) for p in codec.decode(res)]) if f64 else codec.decode_u8(res)
        assert same_bits(d_pic[st].download(), np.ascontiguousarray(want)), (kind, st)
    pl.close()
    for a in d_in + d_pic + d_out + d_nbits + d_maxn:
        a.free()
