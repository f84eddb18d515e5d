"""Every tiled transform kernel of spiht_amd/csrc/dwt_fwd.hip and dwt_inv.hip against the plain loops of oracle/dwt_oracle.c, over the product the
launchers dispatch on: filter length x zero-tap mask x pixel kind x kernel family x extension mode, at picture sizes that
put the tile seams of each kernel where they can go wrong (tests/dwt_sweep_tables.py; tests/test_dwt_sweep_tables.py holds
that grid to its purpose without a GPU).  Through the C ABI; every comparison is equality of bits.  The max|coefficient| word
(maxabs_of) is compared in every forward case, but these pictures keep their largest coefficient in the root block:
tests/test_gpu_maxabs.py moves it through the bands, overhang cells, tiles and threads."""
import ctypes as C

import numpy as np
import pytest

import dwt_sweep_tables as T
from test_gpu_u8 import to_u8, u8_image
from test_gpu_u16 import to_u16, u16_image

pytestmark = pytest.mark.gpu
vp = C.c_void_p

FULL = {"u8": 255.0, "u16": 65535.0}
DTYPE = {"f64": np.float64, "u8": np.uint8, "u16": np.uint16}
SENTINEL = {"u8": 0xA5, "u16": 0xA55A}
INT_IMAGE = {"u8": u8_image, "u16": u16_image}
TO_INT = {"u8": to_u8, "u16": to_u16}


class _Bufs:
    """device buffers of one call, freed on the way out"""

    def __init__(self):
        from spiht_amd import _lib
        self.ctx, self.L, self.check, self.ptrs = _lib.default_context(), _lib.lib(), _lib.check, []

    def new(self, nbytes, fill=None):
        p = self.ctx.alloc(max(int(nbytes), 4))
        self.ptrs.append(p)
        if fill is not None:
            self.ctx.memset(p, fill, int(nbytes))
        return p

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.new(arr.nbytes)
        self.ctx.upload(p, arr)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.free(p)
        return False


def _geometry(L, check, H, W, wid, mid, level):
    v = [C.c_int64() for _ in range(6)]
    lv = C.c_int()
    check(L.spiht_geometry_mode(H, W, wid, mid, level, C.byref(lv), *[C.byref(t) for t in v]))
    assert lv.value == level
    return [t.value for t in v]  # ll_h, ll_w, enc_h, enc_w, rec_h, rec_w


def _mults_ptr(mults):
    m = None if mults is None else np.ascontiguousarray(mults, np.float64)
    return m, (None if m is None else vp(m.ctypes.data))


def int_layout(name, kind, B, H, W, pixels=None):
    """A host buffer for B three-channel pictures of an integer kind in one of two layouts, filled with the sentinel (and with
    `pixels` [B, 3, H, W] where given) -> (buffer, byte strides (sb, sc, sh, sw) or None for dense CHW, view [B, 3, H, W]
    of the pixels inside the buffer).  "rgba": four samples per pixel and a few bytes behind every row."""
    dt = np.dtype(DTYPE[kind])
    es = dt.itemsize
    if name == "planar":
        buf = np.full((B, 3, H, W), SENTINEL[kind], dt)
        view, strides = buf, None
    else:
        pitch = 4 * W * es + 12
        buf = np.full((B, H, pitch // es), SENTINEL[kind], dt)
        view = buf[:, :, :4 * W].reshape(B, H, W, 4)[..., :3].transpose(0, 3, 1, 2)
        strides = (H * pitch, es, pitch, 4 * es)
    if pixels is not None:
        view[...] = pixels
    return buf, strides, view


def untouched(name, kind, buf, W):
    """alpha samples and row padding of an "rgba" buffer still hold the sentinel"""
    if name == "planar":
        return True
    B, H = buf.shape[:2]
    return bool((buf[:, :, :4 * W].reshape(B, H, W, 4)[..., 3] == SENTINEL[kind]).all() and (buf[:, :, 4 * W:] == SENTINEL[kind]).all())


def gpu_forward(kind, buf, strides, B, c, H, W, wavelet, mode, level, q, mults, entry="pyramid"):
    """-> (int32 [B, c, enc_h, enc_w], max|coefficient| uint32 [B] or None).  kind "f64" / "f32": buf is the dense picture
    batch; "u8" / "u16": a buffer and the byte strides of the view in it.  entry "quant": spiht_dwt_quant_batch_*;
    "pyramid": spiht_dwt_pyramid_batch_* with the pyramid left out, which also gives the max|coefficient| words."""
    with _Bufs() as d:
        L = d.L
        wid, mid = L.spiht_wavelet_id(wavelet.encode()), L.spiht_mode_id(mode.encode())
        eh, ew = _geometry(L, d.check, H, W, wid, mid, level)[2:4]
        out, ma = np.empty((B, c, eh, ew), np.int32), np.empty(B, np.uint32)
        m, mp = _mults_ptr(mults)
        d_in = d.put(buf)
        d_out = d.new(out.nbytes, 0xFF)  # the padding cells are proven written
        d_ma = d.new(ma.nbytes, 0xEE)
        if entry == "quant":
            fn = L.spiht_dwt_quant_batch_f32 if kind == "f32" else L.spiht_dwt_quant_batch_f64
            d.check(fn(d.ctx.handle, vp(d_in), B, c, H, W, wid, mid, level, float(q), mp, vp(d_out)))
        elif kind == "f64":
            d.check(L.spiht_dwt_pyramid_batch_f64(d.ctx.handle, vp(d_in), B, c, H, W, wid, mid, level, float(q), mp, vp(d_out),
                                                  None, None, vp(d_ma)))
        else:
            fn = L.spiht_dwt_pyramid_batch_u8 if kind == "u8" else L.spiht_dwt_pyramid_batch_u16
            st = None if strides is None else np.array(strides, np.int64)
            d.check(fn(d.ctx.handle, vp(d_in), None if st is None else vp(st.ctypes.data), B, c, H, W, wid, mid, level, float(q), mp,
                       vp(d_out), None, None, vp(d_ma)))
        d.ctx.download(out, d_out)
        if entry == "quant":
            return out, None
        d.ctx.download(ma, d_ma)
        return out, ma


def gpu_inverse(kind, rec, flags, H, W, wavelet, mode, level, q, mults, layouts=("planar", "rgba")):
    """rec int32 [B, c, enc_h, enc_w] (and the L1Flags words of its level 1, or None) -> {layout: pictures}.  "f64":
    spiht_dequant_idwt_batch_f64 (spiht_dequant_idwt_flags_batch_f64 with words), one dense result [B, c, rec_h, rec_w];
    "u8" / "u16": spiht_dequant_idwt_flags_batch_u8 / _u16 into every layout asked for, [B, 3, H, W] each, the bytes of the
    buffer outside the pixels checked to be what they were."""
    rec = np.ascontiguousarray(rec, np.int32)
    B, c = rec.shape[:2]
    with _Bufs() as d:
        L = d.L
        wid, mid = L.spiht_wavelet_id(wavelet.encode()), L.spiht_mode_id(mode.encode())
        g = _geometry(L, d.check, H, W, wid, mid, level)
        assert rec.shape[2:] == (g[2], g[3])
        m, mp = _mults_ptr(mults)
        d_rec = d.put(rec)
        d_fl = None if flags is None else d.put(np.ascontiguousarray(flags, np.uint32))
        if kind == "f64":
            out = np.empty((B, c, g[4], g[5]), np.float64)
            d_out = d.new(out.nbytes, 0xFF)
            if d_fl is None:
                d.check(L.spiht_dequant_idwt_batch_f64(d.ctx.handle, vp(d_rec), B, c, H, W, wid, mid, level, float(q), mp, vp(d_out)))
            else:
                d.check(L.spiht_dequant_idwt_flags_batch_f64(d.ctx.handle, vp(d_rec), vp(d_fl), B, c, H, W, wid, mid, level, float(q),
                                                             mp, vp(d_out)))
            d.ctx.download(out, d_out)
            return {"dense": out}
        assert c == 3
        fn = L.spiht_dequant_idwt_flags_batch_u8 if kind == "u8" else L.spiht_dequant_idwt_flags_batch_u16
        res = {}
        for name in layouts:
            buf, strides, view = int_layout(name, kind, B, H, W)
            st = None if strides is None else np.array(strides, np.int64)
            d_out = d.put(buf)
            d.check(fn(d.ctx.handle, vp(d_rec), None if d_fl is None else vp(d_fl), B, c, H, W, wid, mid, level, float(q), mp,
                       vp(d_out), None if st is None else vp(st.ctypes.data)))
            d.ctx.download(buf, d_out)
            assert untouched(name, kind, buf, W), (name, "bytes outside the pixels were written")
            res[name] = np.ascontiguousarray(view)
        return res


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return a.dtype == b.dtype and np.array_equal(a, b)


def maxabs_of(ref):
    return np.abs(ref.astype(np.int64)).reshape(ref.shape[0], -1).max(axis=1).astype(np.uint32)


def device_colour(imgs, src, dest):
    """the stand-alone colour kernel (the same function as the fused kernels' and the same bits) on float64 pictures
    [B, 3, h, w], downloaded"""
    from spiht_amd import color_models
    imgs = np.ascontiguousarray(imgs, np.float64)
    with _Bufs() as d:
        p = d.put(imgs)
        color_models.device_convert(d.ctx, p, imgs.shape[0], imgs.shape[2] * imgs.shape[3], src, dest)
        out = np.empty_like(imgs)
        d.ctx.download(out, p)
    return out


def _F(oracle, wavelet):
    return T.instantiation(oracle, wavelet)[0]


# ---- 1. forward, float64: k_dwt_level + k_dwt_edge -------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", T.WAVELETS)
def test_forward_float64(oracle, wavelet):
    """all modes x the four seam sizes (pictures shorter than the filter among them), two levels (the ll_out path and the
    last one), per-channel scales on every other size: the int32 array of spiht_dwt_quant_batch_f64 and of
    spiht_dwt_pyramid_batch_f64, and the latter's max|coefficient| word per image"""
    F = _F(oracle, wavelet)
    n = 0
    for i, (H, W) in enumerate(T.forward_sizes(F)):
        imgs, mults = T.sweep_images(1000 + i, 2, 2, H, W), T.scales_for(i, 2)
        for mode in T.MODES:
            ref = np.stack([oracle.quantize(oracle.wavedec2_array(im, wavelet, mode, 2)[0], T.Q, mults) for im in imgs])
            got, _ = gpu_forward("f64", imgs, None, 2, 2, H, W, wavelet, mode, 2, T.Q, mults, entry="quant")
            assert same_bits(got, ref), (wavelet, mode, H, W, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
            got, ma = gpu_forward("f64", imgs, None, 2, 2, H, W, wavelet, mode, 2, T.Q, mults)
            assert same_bits(got, ref), (wavelet, mode, H, W, "pyramid entry")
            assert np.array_equal(ma, maxabs_of(ref)), (wavelet, mode, H, W, ma, maxabs_of(ref))
            n += 1
    assert n == 20


# ---- 2. forward, float32: k_dwt_level_f32 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", T.WAVELETS)
def test_forward_float32(oracle, wavelet):
    """the same grid on the single-precision kernel's tile (16 rows), every level's input at least as long as the filter
    (tests/dwt_sweep_tables.py: f32_level), against the oracle's single-precision transform and quantiser"""
    F = _F(oracle, wavelet)
    n = 0
    for i, (H, W) in enumerate(T.forward_sizes(F, T.FWD32_TH)):
        level = T.f32_level(F, H, W)
        if level is None:
            continue
        imgs, mults = T.sweep_images(1000 + i, 2, 2, H, W).astype(np.float32), T.scales_for(i, 2)
        for mode in T.MODES:
            ref = np.stack([oracle.quantize_f32(oracle.wavedec2_array_f32(im, wavelet, mode, level)[0], T.Q, mults) for im in imgs])
            got, _ = gpu_forward("f32", imgs, None, 2, 2, H, W, wavelet, mode, level, T.Q, mults, entry="quant")
            assert same_bits(got, ref), (wavelet, mode, H, W, level, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
            n += 1
    assert n >= 5


# ---- 3. forward, 8- and 16-bit pixels: k_dwt_level<.., PX> + k_dwt_edge<F, PX> --------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "u16"])
@pytest.mark.parametrize("wavelet", T.WAVELETS)
def test_forward_integer_pixels(oracle, wavelet, kind):
    """all modes x {exactly one tile, one past two tiles with odd sizes}, planar and padded RGBA views: the array and the
    max|coefficient| words of spiht_dwt_pyramid_batch_u8 / _u16 against the oracle on P / 255.0 (P / 65535.0)"""
    F = _F(oracle, wavelet)
    for i, (H, W) in enumerate(T.forward_sizes_reduced(F)):
        P = np.stack([INT_IMAGE[kind](3000 + i + 5 * b, 3, H, W) for b in range(2)])
        mults = T.scales_for(i, 3)
        views = [int_layout(name, kind, 2, H, W, P)[:2] for name in ("planar", "rgba")]
        for mode in T.MODES:
            ref = np.stack([oracle.quantize(oracle.wavedec2_array(p / FULL[kind], wavelet, mode, 2)[0], T.Q, mults) for p in P])
            for buf, strides in views:
                got, ma = gpu_forward(kind, buf, strides, 2, 3, H, W, wavelet, mode, 2, T.Q, mults)
                assert same_bits(got, ref), (wavelet, kind, mode, H, W, strides, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
                assert np.array_equal(ma, maxabs_of(ref)), (wavelet, kind, mode, H, W, strides)


# ---- 4. forward, colour change on the loads: k_dwt1_color ------------------------------------------------------------------
def _int_patches(P, full):
    P = P.copy()
    H, W = P.shape[-2:]
    P[..., :max(1, H // 3), :max(1, W // 4)] = 0
    P[..., H - max(1, H // 4):, W - max(1, W // 3):] = int(full)
    return P


@pytest.mark.parametrize("kind", ["f64", "u8", "u16"])
@pytest.mark.parametrize("wavelet", T.WAVELETS)
def test_forward_colour_fused(oracle, wavelet, kind):
    """Inside color_models.fused(ctx, "IPT"): all modes x the two reduced sizes, and one picture that crosses the kernel's
    strips in both directions under one mode (which one rotates through the wavelet list).  The reference pixels are the
    stand-alone colour kernel's, downloaded -- the same function and the same bits -- and go through the oracle's plain
    transform.  Patches of exact 0 and exact 1 in every picture."""
    from spiht_amd import _lib, color_models
    F = _F(oracle, wavelet)
    ctx = _lib.default_context()
    big_mode = T.MODES[T.WAVELETS.index(wavelet) % len(T.MODES)]
    cases = [(i, H, W, 2, T.MODES) for i, (H, W) in enumerate(T.forward_sizes_reduced(F))] + [(2, *T.COLOUR_BIG, 1, [big_mode])]
    for i, H, W, B, modes in cases:
        mults = T.scales_for(i, 3)
        if kind == "f64":
            pix = T.with_patches(T.sweep_images(2000 + i, B, 3, H, W))
            views = [(pix, None)]
            rgb = pix
        else:
            P = _int_patches(np.stack([INT_IMAGE[kind](4000 + i + 5 * b, 3, H, W) for b in range(B)]), FULL[kind])
            views = [int_layout(name, kind, B, H, W, P)[:2] for name in ("planar", "rgba")]
            rgb = P / FULL[kind]
        assert (rgb == 0.0).any() and (rgb == 1.0).any()
        ipt = device_colour(rgb, "RGB", "IPT")
        for mode in modes:
            ref = np.stack([oracle.quantize(oracle.wavedec2_array(im, wavelet, mode, 2)[0], T.Q, mults) for im in ipt])
            for buf, strides in views:
                with color_models.fused(ctx, "IPT"):
                    got, ma = gpu_forward(kind, buf, strides, B, 3, H, W, wavelet, mode, 2, T.Q, mults)
                assert same_bits(got, ref), (wavelet, kind, mode, H, W, strides, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
                assert np.array_equal(ma, maxabs_of(ref)), (wavelet, kind, mode, H, W, strides)


# ---- 5. inverse: k_idwt_level ------------------------------------------------------------------------------------------------
def _int_want(kind, want, H, W):
    return np.stack([TO_INT[kind](w, H, W) for w in want])


@pytest.mark.parametrize("kind", ["f64", "u8", "u16"])
@pytest.mark.parametrize("wavelet", T.WAVELETS)
def test_inverse(oracle, wavelet, kind):
    """the four seam sizes at two levels (the 26 x 130 one also at one level: the approximation out of the packed array), from
    a thinned-out copy of the oracle's quantised array of a picture that overshoots [0, 1]: the oracle's picture back, for
    the integer kinds through the contract's clip, scale, truncate and crop, in a planar and a padded RGBA buffer whose other
    bytes keep their sentinel.  The extension mode does not enter the inverse of the index-map modes: two of them, same bits.
    Then the largest size once more with L1Flags words of which about half are zero."""
    integer = kind != "f64"
    c = 3 if integer else 2
    sizes = T.inverse_sizes(integer)
    for i, (H, W), level in [(i, s, 2) for i, s in enumerate(sizes)] + [(2, sizes[2], 1)]:
        mults = T.scales_for(i + level, c)
        pairs = [T.inverse_case(oracle, wavelet, H, W, level, 500 + i + 9 * b, mults, c) for b in range(2)]
        rec, want = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        assert want.shape[2:] == T.INV_REC[i] and want[:, :, :H, :W].min() < 0.0 and want[:, :, :H, :W].max() > 1.0
        if integer:
            want = _int_want(kind, want, H, W)
        first = None
        for mode in ("reflect", "periodic"):
            got = gpu_inverse(kind, rec, None, H, W, wavelet, mode, level, T.Q, mults)
            for name, px in got.items():
                assert same_bits(px, want), (wavelet, kind, mode, H, W, level, name, np.argwhere(px != want)[:4].tolist())
            first = first or got
            assert all(same_bits(got[k], first[k]) for k in got)
    # the occupancy words in front of the workgroup-per-tile kernel (a batch this small never takes the persistent one): the
    # 3 x 3-tile size, the detail bands of about half the tiles zeroed, with the words and without them
    F = _F(oracle, wavelet)
    H, W = sizes[3]
    mults = T.scales_for(0, c)
    rec = np.stack([T.empty_some_tiles(T.inverse_case(oracle, wavelet, H, W, 2, 520 + 9 * b, mults, c)[0], H, W, F, 60 + b) for b in range(2)])
    words = T.occupancy_words(rec, H, W, F)
    assert words.shape == (2, c, 3, 3) and 0.2 <= float((words == 0).mean()) <= 0.8
    want = np.stack([oracle.waverec2_array(oracle.dequantize(r, T.Q, mults), H, W, wavelet, 2) for r in rec])
    if integer:
        want = _int_want(kind, want, H, W)
    for flags in (words, None):
        for name, px in gpu_inverse(kind, rec, flags, H, W, wavelet, "reflect", 2, T.Q, mults).items():
            assert same_bits(px, want), (wavelet, kind, H, W, name, flags is None, np.argwhere(px != want)[:4].tolist())


# ---- 6. inverse, colour change on the stores: k_idwt1_color ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "u8", "u16"])
@pytest.mark.parametrize("wavelet", T.WAVELETS)
def test_inverse_colour_fused(oracle, wavelet, kind):
    """Inside color_models.fused(ctx, "IPT"): the oracle's inverse of an array coded in IPT, uploaded, through the stand-alone
    colour kernel IPT -> RGB and back down, then the pixel kind's store formula -- against the fused kernel's picture."""
    from conftest import synth_image
    from spiht_amd import _lib, color_models
    ctx = _lib.default_context()
    integer = kind != "f64"
    for i, (H, W) in enumerate(T.inverse_sizes(integer)):
        mults = T.scales_for(i, 3)
        recs, ipts = [], []
        for b in range(2):
            rgb = synth_image(600 + i + 9 * b, 3, H, W) * 1.1 - 0.05
            arr, _ = oracle.wavedec2_array(color_models.convert(rgb, "RGB", "IPT"), wavelet, "reflect", 2)
            recs.append(T.thin_out(oracle.quantize(arr, T.Q, mults), i + b))
            ipts.append(oracle.waverec2_array(oracle.dequantize(recs[-1], T.Q, mults), H, W, wavelet, 2))
        rec = np.stack(recs)
        want = device_colour(np.stack(ipts), "IPT", "RGB")
        assert want.shape[2:] == T.INV_REC[i] and want.min() < 0.0 and want.max() > 1.0 and np.isfinite(want).all()
        if integer:
            want = _int_want(kind, want, H, W)
        with color_models.fused(ctx, "IPT"):
            got = gpu_inverse(kind, rec, None, H, W, wavelet, "reflect", 2, T.Q, mults)
        for name, px in got.items():
            assert same_bits(px, want), (wavelet, kind, H, W, name, np.argwhere(px != want)[:4].tolist())


# ---- 7. the persistent inverse: k_idwt_level_pf, FIRST / plain / FLAGS -----------------------------------------------------
def test_persistent_batch_geometry():
    """1667 three-channel pictures of 2 x 2 tiles: 20 004 tiles in one launch, at or above the 20 000 from which
    launch_idwt_FM takes k_idwt_level_pf, with plane offsets that fit 32 bits (or it would fall back to k_idwt_level)"""
    assert T.pf_tile_count() >= T.PF_MIN
    assert (T.PF_REC[0] + T.INV_TH) * T.PF_REC[1] * 8 < 2 ** 31 and T.PF_PICTURES * 3 <= 65535


@pytest.mark.parametrize("kind", ["f64", "u8", "u16"])
@pytest.mark.parametrize("wavelet", T.INVERSE_MASK_WAVELETS)
def test_persistent_inverse(oracle, wavelet, kind):
    """Every mask instantiation of the persistent kernel in its three variants -- one level (FIRST), two levels without words
    (plain), two levels with the L1Flags words (FLAGS; the words are made here from the array, the detail bands of about
    half the tiles zeroed first) -- on a batch of 8 distinct oracle-checked arrays repeated: picture b must be the oracle's
    picture of array b % 8."""
    F = _F(oracle, wavelet)
    integer = kind != "f64"
    idx = np.arange(T.PF_PICTURES) % T.PF_DISTINCT
    for variant, level, empty, mults in (("FIRST", 1, False, [1.0, 0.75, 2.0]), ("plain", 2, False, None), ("FLAGS", 2, True, [2.0, 1.0, 0.75])):
        recs, wants, H, W = T.pf_cases(oracle, wavelet, level, integer, empty, mults)
        flags = None
        if variant == "FLAGS":
            words = T.occupancy_words(recs, H, W, F)
            assert words.shape == (T.PF_DISTINCT, 3, 2, 2) and 0.2 <= float((words == 0).mean()) <= 0.8
            flags = words[idx]
        if integer:
            wants = _int_want(kind, wants, H, W)
        got = gpu_inverse(kind, recs[idx], flags, H, W, wavelet, "reflect", level, T.Q, mults)
        for name, px in got.items():
            assert px.shape == (T.PF_PICTURES,) + wants.shape[1:]
            for k in range(T.PF_DISTINCT):
                part = px[k::T.PF_DISTINCT]
                ok = same_bits(part, np.broadcast_to(wants[k], part.shape))
                assert ok, (wavelet, kind, variant, name, k, np.argwhere(part != wants[k])[:4].tolist())
