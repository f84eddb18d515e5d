"""The addressing of the tiled forward transform kernel (spiht_amd/csrc/dwt_fwd.hip: k_dwt_level): one plane descriptor and 32-bit
offsets per tile, store offsets advanced by launch-time constants, tile -> (column, row, plane) and plane -> (image, channel)
by multipliers, extension indices without a division.  The smallest shapes at which each of these can go wrong, every
quantised array and every max|coefficient| word (the start plane max_n is its bit length) equal to the oracle's, bit for bit.
The 64-bit addressing that pictures of 2^30 bytes and more take is run on the same small shapes (SPIHT_DWT_ADDR64)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from conftest import synth_image
from test_gpu_dwt_sweep import INT_IMAGE, FULL, gpu_forward, int_layout, untouched

pytestmark = pytest.mark.gpu
vp = C.c_void_p

WAVELETS = ("haar", "bior2.2", "bior4.4")
MODES = ("reflect", "symmetric", "periodic", "zero", "constant")
# 64 / 65 output columns (one tile; a second tile of one column), several tiles; 12 / 13 output rows, several tiles;
# and pictures shorter than or as long as the filters
WIDTHS = (123, 125, 251, 3, 5, 7)
HEIGHTS = (19, 21, 43, 3, 5, 7)

_ref_cache = {}


def _levels(oracle, H, W, wavelet, mode):
    """one level, and the maximum: what level=None gives, two at least (small pictures go above PyWavelets' maximum), as far as
    the root block stays larger than one row and one column (the entry point refuses the others, as the reference does)"""
    top = max(2, oracle.geometry(H, W, wavelet, None, mode)["level"])
    while top > 1 and min(oracle.geometry(H, W, wavelet, top, mode)[k] for k in ("ll_h", "ll_w")) <= 1:
        top -= 1
    return (1, top) if top > 1 else (1,)


def _reference(oracle, tag, imgs, wavelet, mode, level, q, mults):
    """the oracle's quantised arrays [B, c, enc_h, enc_w] and max|coefficient| per image, computed once per case"""
    key = (tag, hashlib.sha1(imgs.tobytes()).hexdigest(), imgs.shape, wavelet, mode, level, q, None if mults is None else tuple(mults))
    if key not in _ref_cache:
        ref = np.stack([oracle.quantize(oracle.wavedec2_array(im, wavelet, mode, level)[0], q, mults) for im in imgs])
        ref.setflags(write=False)
        _ref_cache[key] = (ref, np.abs(ref.astype(np.int64)).max(axis=(1, 2, 3)).astype(np.uint32))
    return _ref_cache[key]


def _same(got, ma, ref, ref_ma, what):
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())
    assert np.array_equal(ma, ref_ma), (what, ma.tolist(), ref_ma.tolist())


def _pictures(seed, B, c, H, W):
    return np.stack([synth_image(seed + b, c, H, W) for b in range(B)])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_sizes_modes_wavelets(oracle, wavelet, mode):
    """every width x height of the grid, at one level and at the maximum level, two images of three channels with channel
    scales (12 and 24 tiles per level-1 launch at the one-tile sizes: no multiple of 8)"""
    mults = [1.0, 0.5, 2.0]
    for H in HEIGHTS:
        for W in WIDTHS:
            imgs = _pictures(100 + H + 7 * W, 2, 3, H, W)
            for level in _levels(oracle, H, W, wavelet, mode):
                ref, ref_ma = _reference(oracle, "f64", imgs, wavelet, mode, level, 50.0, mults)
                got, ma = gpu_forward("f64", imgs, None, 2, 3, H, W, wavelet, mode, level, 50.0, mults)
                _same(got, ma, ref, ref_ma, (wavelet, mode, H, W, level))


@pytest.mark.parametrize("c", (1, 3, 4))
@pytest.mark.parametrize("B", (1, 2, 5))
def test_planes_to_image_and_channel(oracle, B, c):
    """plane -> (image, channel): the channel picks the scale, the image the max|coefficient| word.  125 x 21 is 2 x 2 tiles
    a plane at level 1: 4 tiles in all (fewer than the 8 XCDs) with one plane, 12, 20, 24, ... 80 with more"""
    H, W = 21, 125
    mults = [1.0, 0.25, 3.0, 0.5][:c]
    imgs = _pictures(300 + 10 * B + c, B, c, H, W)
    imgs *= (1.0 + np.arange(B))[:, None, None, None]  # every image its own maximum
    for wavelet, mode, level in (("bior2.2", "reflect", 1), ("bior2.2", "reflect", 3), ("bior4.4", "periodic", 2), ("haar", "zero", 2)):
        ref, ref_ma = _reference(oracle, "f64", imgs, wavelet, mode, level, 50.0, mults)
        assert len(set(ref_ma.tolist())) == B
        got, ma = gpu_forward("f64", imgs, None, B, c, H, W, wavelet, mode, level, 50.0, mults)
        _same(got, ma, ref, ref_ma, (B, c, wavelet, mode, level))


def _int_pictures(kind, seed, H, W):
    """two three-channel pictures of an integer kind (the other tests' generators; plain noise over the whole range where a
    picture is too small for them)"""
    if 3 * H * W >= 256:
        return np.stack([INT_IMAGE[kind](seed + b, 3, H, W) for b in range(2)])
    return np.random.default_rng(seed).integers(0, int(FULL[kind]) + 1, (2, 3, H, W)).astype(np.uint8 if kind == "u8" else np.uint16)


@pytest.mark.parametrize("layout", ("planar", "rgba"))
@pytest.mark.parametrize("kind", ("u8", "u16"))
def test_pixel_views(oracle, kind, layout):
    """8- and 16-bit views, dense and with four samples per pixel and padded rows (channel stride one element, row stride
    not the dense one), every mode -- zero padding reads nothing outside the view's pixels, and the buffer is left alone"""
    for (H, W) in ((21, 125), (43, 123), (5, 7), (19, 251)):
        P = _int_pictures(kind, 900 + H, H, W)
        buf, strides, _ = int_layout(layout, kind, 2, H, W, P)
        imgs = P / FULL[kind]
        for wavelet, mode in (("bior2.2", "reflect"), ("bior2.2", "zero"), ("bior4.4", "symmetric"), ("haar", "periodic"),
                              ("bior4.4", "zero"), ("bior2.2", "constant")):
            for level in _levels(oracle, H, W, wavelet, mode):
                ref, ref_ma = _reference(oracle, kind, imgs, wavelet, mode, level, 50.0, None)
                got, ma = gpu_forward(kind, buf, strides, 2, 3, H, W, wavelet, mode, level, 50.0, None)
                _same(got, ma, ref, ref_ma, (kind, layout, wavelet, mode, H, W, level))
        assert untouched(layout, kind, buf, W)


def _forward_at(ctx, L, d_in, imgs, wavelet, mode, level, q):
    """spiht_dwt_pyramid_batch_f64 of the float64 pictures already at device address d_in -> (arrays, max words)"""
    from spiht_amd import _lib
    B, c, H, W = imgs.shape
    wid, mid = L.spiht_wavelet_id(wavelet.encode()), L.spiht_mode_id(mode.encode())
    v, lv = [C.c_int64() for _ in range(6)], C.c_int()
    _lib.check(L.spiht_geometry_mode(H, W, wid, mid, level, C.byref(lv), *[C.byref(t) for t in v]))
    out, ma = np.empty((B, c, v[2].value, v[3].value), np.int32), np.empty(B, np.uint32)
    d_out, d_ma = ctx.alloc(out.nbytes), ctx.alloc(max(ma.nbytes, 4))
    try:
        ctx.memset(d_out, 0xFF, out.nbytes)
        ctx.memset(d_ma, 0xEE, ma.nbytes)
        _lib.check(L.spiht_dwt_pyramid_batch_f64(ctx.handle, vp(d_in), B, c, H, W, wid, mid, level, float(q), None, vp(d_out),
                                                 None, None, vp(d_ma)))
        ctx.download(out, d_out)
        ctx.download(ma, d_ma)
    finally:
        ctx.free(d_out)
        ctx.free(d_ma)
    return out, ma


def test_picture_eight_bytes_off_a_sixteen_byte_boundary(oracle):
    """a float64 picture whose device address is 8 modulo 16: the 8-byte loads through the descriptor need no more"""
    from spiht_amd import _lib
    ctx, L = _lib.default_context(), _lib.lib()
    imgs = _pictures(500, 2, 3, 43, 125)
    base = ctx.alloc(imgs.nbytes + 32)
    try:
        d_in = base + (8 - base % 16) % 16
        assert d_in % 16 == 8
        ctx.upload(d_in, imgs)
        for wavelet, mode, level in (("bior2.2", "reflect", 1), ("bior4.4", "zero", 2), ("haar", "symmetric", 3)):
            ref, ref_ma = _reference(oracle, "f64", imgs, wavelet, mode, level, 50.0, None)
            got, ma = _forward_at(ctx, L, d_in, imgs, wavelet, mode, level, 50.0)
            _same(got, ma, ref, ref_ma, (wavelet, mode, level))
    finally:
        ctx.free(base)


def test_small_magnitudes_after_large_on_one_context(oracle):
    """the cached look at the max|coefficient| word (block_raise_max) sees nothing from before the word was zeroed: a batch of
    large magnitudes, then one of small magnitudes, same context, same buffers, several times over"""
    from spiht_amd import _lib
    ctx, L = _lib.default_context(), _lib.lib()
    big = _pictures(600, 3, 1, 43, 251) * 4000.0
    small = _pictures(610, 3, 1, 43, 251) * 0.02
    refs = {name: _reference(oracle, name, imgs, "bior2.2", "reflect", 2, 50.0, None) for name, imgs in (("big", big), ("small", small))}
    assert refs["big"][1].min() > 256 * refs["small"][1].max()
    d_in = ctx.alloc(big.nbytes)
    try:
        for _ in range(3):
            for name, imgs in (("big", big), ("small", small)):
                ctx.upload(d_in, imgs)
                got, ma = _forward_at(ctx, L, d_in, imgs, "bior2.2", "reflect", 2, 50.0)
                _same(got, ma, refs[name][0], refs[name][1], name)
    finally:
        ctx.free(d_in)


@pytest.mark.parametrize("wavelet", WAVELETS)
def test_wide_addressing_gives_the_same_bits(oracle, wavelet, monkeypatch):
    """the 64-bit addressing the launcher chooses for planes of 2^30 bytes and more (tests/test_dwt_addressing_cpu.py holds the
    choice itself), forced onto small pictures: float64 and both integer kinds, every mode"""
    monkeypatch.setenv("SPIHT_DWT_ADDR64", "1")
    for mode in MODES:
        for (H, W) in ((21, 125), (43, 123), (5, 7)):
            imgs = _pictures(100 + H + 7 * W, 2, 3, H, W)
            level = _levels(oracle, H, W, wavelet, mode)[-1]
            ref, ref_ma = _reference(oracle, "f64", imgs, wavelet, mode, level, 50.0, [1.0, 0.5, 2.0])
            got, ma = gpu_forward("f64", imgs, None, 2, 3, H, W, wavelet, mode, level, 50.0, [1.0, 0.5, 2.0])
            _same(got, ma, ref, ref_ma, ("wide", wavelet, mode, H, W, level))
        for kind in ("u8", "u16"):
            H, W = 21, 125
            P = _int_pictures(kind, 900 + H, H, W)
            buf, strides, _ = int_layout("rgba", kind, 2, H, W, P)
            ref, ref_ma = _reference(oracle, kind, P / FULL[kind], wavelet, mode, 1, 50.0, None)
            got, ma = gpu_forward(kind, buf, strides, 2, 3, H, W, wavelet, mode, 1, 50.0, None)
            _same(got, ma, ref, ref_ma, ("wide", kind, wavelet, mode))
