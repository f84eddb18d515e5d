"""The max|coefficient| word of every forward route -- the start plane max_n is its bit length, so one wrong word changes every
byte of a stream -- on pictures that put the largest quantised coefficient where natural pictures never do
(tests/maxabs_cases.py; tests/test_maxabs_cases.py holds those pictures to their purpose on the oracle): in each detail band
and overhang class of level 1, in the level-2 bands, on every thread of a tile, in the cells a wavefront shares with the
neighbouring image.  Every comparison is an equality with the oracle: the word, the int32 array, and where a stream is made,
max_n and its bytes.

A. classes, float64 (k_dwt_level + k_dwt_edge, both addressing forms)      D. the step word -> max_n -> stream (single precision too)
B. every thread of a tile                                                    E. the two-pass levels (k_dwt_pack_ext, wave_raise_max)
C. 8- / 16-bit, float-kind and colour-fused pixels                           F. k_absmax
(k_quant_plain's word has no way out: every entry point that returns it refuses a picture without a transform level.)"""
import ctypes as C

import numpy as np
import pytest

import dwt_sweep_tables as T
import maxabs_cases as M
from test_gpu_dwt_sweep import device_colour, gpu_forward, int_layout, maxabs_of, untouched

pytestmark = pytest.mark.gpu
vp = C.c_void_p


def _oracle():
    from oracle import oracle as O
    return O


def same(got, ma, ref, what):
    """array and word of every image of a batch"""
    for b in range(len(ref)):
        bad = np.argwhere(got[b] != ref[b])
        assert len(bad) == 0, (what, b, len(bad), bad[:4].tolist())
    want = maxabs_of(ref)
    assert np.array_equal(ma, want), (what, ma.tolist(), want.tolist())


def cases(kind, wavelet, mode):
    """the batches of (kind, wavelet, mode) with the oracle's arrays, made once per test (addressing forms and layouts share them)"""
    O = _oracle()
    out = []
    for pics, classes, mults in M.batches(O, kind, wavelet, mode):
        ref = None if kind in M.COLOUR_KINDS else M.batch_reference(O, kind, wavelet, mode, pics, mults)
        out.append((pics, classes, mults, ref))
    return out


def wavelets_of(kind):
    """the wavelets that reach a class of the kind (from the list of what is not reached: no oracle at collection time)"""
    level, modes, classes = M.GRID[kind]
    return [w for w in T.WAVELETS if any(M.key(w, m, c) not in M.UNREACHED[kind] for m in modes for c in classes)]


# ---- A. classes, float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", T.WAVELETS)
def test_classes_float64(oracle, wavelet, monkeypatch):
    """every reached class of levels 1 and 2, one past two tiles (odd x odd), reflect and zero padding, batches of three whose
    neighbours hold different classes at magnitudes a factor 4 apart, channel scales on every other batch -- through both
    addressing forms (the 64-bit one forced as tests/test_gpu_dwt_addressing.py forces it)"""
    H, W = M.size_of(oracle, wavelet)
    todo = [(mode, case) for mode in M.FLOAT_MODES for case in cases("f64", wavelet, mode)]
    assert len(todo) >= 8
    for wide in (False, True):
        with monkeypatch.context() as mp:
            if wide:
                mp.setenv("SPIHT_DWT_ADDR64", "1")
            for mode, (pics, classes, mults, ref) in todo:
                got, ma = gpu_forward("f64", pics, None, 3, 2, H, W, wavelet, mode, 2, M.Q, mults)
                same(got, ma, ref, (wavelet, mode, "wide" if wide else "narrow", [M.cname(c) for c in classes], mults))


# ---- B. every thread ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet,mode", M.THREAD_WAVELETS)
def test_every_thread(oracle, wavelet, mode):
    """level 1 of a 2 x 2-tile picture, the one largest coefficient on each (row, column) of a tile in turn -- every lane of the
    three wavefronts at each of a thread's four rows -- and on the edges of all four tiles; 64 pictures a call, each its own word"""
    F = T.instantiation(oracle, wavelet)[0]
    H, W = M.thread_size(F)
    n = 0
    for tg, pics, refs in M.thread_cases(oracle, wavelet, mode):
        got, ma = gpu_forward("f64", pics, None, len(pics), 1, H, W, wavelet, mode, 1, M.Q, None)
        same(got, ma, refs, (wavelet, mode, tg[0], tg[-1]))
        n += len(tg)
    assert n >= T.FWD_TH * T.FWD_TW


# ---- C. pixel kinds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,wavelet", [(k, w) for k in M.INT_KINDS for w in wavelets_of(k)])
def test_classes_integer_pixels(oracle, wavelet, kind):
    """k_dwt_level<.., PX> + k_dwt_edge<F, PX>: planar and the padded RGBA view, whose other bytes keep their sentinel"""
    H, W = M.size_of(oracle, wavelet)
    for pics, classes, mults, ref in cases(kind, wavelet, "reflect"):
        for name in ("planar", "rgba"):
            buf, strides, _ = int_layout(name, kind, 3, H, W, pics)
            got, ma = gpu_forward(kind, buf, strides, 3, 3, H, W, wavelet, "reflect", 1, M.Q, mults)
            same(got, ma, ref, (wavelet, kind, name, [M.cname(c) for c in classes]))
            assert untouched(name, kind, buf, W)


@pytest.mark.parametrize("kind", M.FLT_KINDS)
@pytest.mark.parametrize("wavelet", T.WAVELETS)
def test_classes_float_pixels(oracle, wavelet, kind):
    """PX_FLT: float32, float16 and bfloat16 pixels in, widened exactly; planar and four samples a pixel"""
    from test_gpu_floatin import flt_forward, flt_layout
    H, W = M.size_of(oracle, wavelet)
    for mode in M.FLOAT_MODES:
        for pics, classes, mults, ref in cases(kind, wavelet, mode):
            assert mults is None
            for name in ("planar", "four"):
                buf, strides = flt_layout(name, pics)
                got, ma, _ = flt_forward(kind, buf, strides, 3, 2, H, W, wavelet, mode, 2, M.Q)
                same(got, ma, ref, (wavelet, kind, mode, name, [M.cname(c) for c in classes]))


@pytest.mark.parametrize("kind,wavelet", [(k, w) for k in M.COLOUR_KINDS for w in wavelets_of(k)])
def test_classes_colour_fused(oracle, wavelet, kind):
    """k_dwt1_color inside color_models.fused(ctx, "IPT"), float64 and 8-bit pixels.  As in test_gpu_dwt_sweep: the reference
    pixels are the stand-alone colour kernel's (the same function, the same bits) through the oracle's plain transform."""
    from spiht_amd import _lib, color_models
    ctx = _lib.default_context()
    H, W = M.size_of(oracle, wavelet)
    for pics, classes, mults, _ in cases(kind, wavelet, "reflect"):
        ipt = device_colour(pics / 255.0 if kind == "ipt-u8" else pics, "RGB", "IPT")
        ref = np.stack([oracle.quantize(oracle.wavedec2_array(im, wavelet, "reflect", 1)[0], M.Q, mults) for im in ipt])
        views = [(pics, None)] if kind == "ipt-f64" else [int_layout(name, "u8", 3, H, W, pics)[:2] for name in ("planar", "rgba")]
        for buf, strides in views:
            with color_models.fused(ctx, "IPT"):
                got, ma = gpu_forward("f64" if kind == "ipt-f64" else "u8", buf, strides, 3, 3, H, W, wavelet, "reflect", 1, M.Q, mults)
            same(got, ma, ref, (wavelet, kind, strides, [M.cname(c) for c in classes]))


# ---- D. word -> max_n -> stream -------------------------------------------------------------------------------------------------
STEP_BITS = 6000


def _settings(wavelet, q):
    import spiht_amd
    return spiht_amd.SpihtSettings(wavelet=wavelet, mode="reflect", quantization_scale=q)


@pytest.mark.parametrize("wavelet", M.STEP_WAVELETS)
def test_step_single_precision(oracle, wavelet):
    """k_dwt_level_f32 returns no word of its own: float32 pictures through encode_image and BatchCodec(pixel_dtype=float32),
    the class's maximum at 2^10 or just above and everything else below -- the start plane is the class's, and every byte
    behind it"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    H, W = M.size_of(oracle, wavelet)
    n = 0
    for cls in M.LEVEL1:
        case = M.step_case(oracle, "f32t", wavelet, "reflect", 2, cls)
        if case is None:
            continue
        stored, q, inside, outside = case
        assert stored.dtype == np.float32
        want, want_n, _ = oracle.encode_image(stored, wavelet, "reflect", 2, q, None, STEP_BITS)
        assert want_n == oracle.start_plane(inside) and (outside == 0 or oracle.start_plane(outside) < want_n)
        got = spiht_amd.encode_image(stored, _settings(wavelet, q), level=2, max_bits=STEP_BITS)
        assert (got.max_n, got.encoded_bytes) == (want_n, want), (wavelet, M.cname(cls), got.max_n, want_n)
        if n % 4 == 0:
            codec = BatchCodec(1, H, W, _settings(wavelet, q), level=2, max_bits=STEP_BITS, pixel_dtype=np.float32)
            res = codec.encode(np.stack([stored, -stored]))
            want_neg, neg_n, _ = oracle.encode_image(-stored, wavelet, "reflect", 2, q, None, STEP_BITS)
            assert [(r.max_n, r.encoded_bytes) for r in res] == [(want_n, want), (neg_n, want_neg)], (wavelet, M.cname(cls))
        n += 1
    assert n >= 10


@pytest.mark.parametrize("wavelet", M.STEP_WAVELETS)
def test_step_float64_and_8bit(oracle, wavelet):
    """the same step once per kind through the double-precision kernels: the chain word -> max_n -> stream"""
    import spiht_amd
    done = set()
    for kind, level in (("f64", 2), ("u8", 1)):
        for cls in reversed(M.LEVEL1):  # (the overhang classes first)
            case = M.step_case(oracle, kind, wavelet, "reflect", level, cls)
            if case is None:
                continue
            stored, q, inside, outside = case
            if kind == "f64":
                want, want_n, _ = oracle.encode_image(stored, wavelet, "reflect", level, q, None, STEP_BITS)
                got = spiht_amd.encode_image(stored, _settings(wavelet, q), level=level, max_bits=STEP_BITS)
            else:
                want, want_n, _ = oracle.encode_image(stored / 255.0, wavelet, "reflect", level, q, None, STEP_BITS)
                got = spiht_amd.encode_image_u8(stored, _settings(wavelet, q), level=level, max_bits=STEP_BITS)
            assert want_n == oracle.start_plane(inside)
            assert (got.max_n, got.encoded_bytes) == (want_n, want), (wavelet, kind, M.cname(cls), got.max_n, want_n)
            done.add(kind)
            break
    assert done == {"f64", "u8"}


# ---- E. the two-pass levels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet,mode", M.PACK_ROUTES)
def test_two_pass_routes(oracle, wavelet, mode):
    """k_dwt_pack_ext over a filter longer than the tiled kernels take, a computed extension, and periodization: three pictures
    whose plane sizes are no multiple of 64, so that wavefronts straddle two images; the one largest coefficient in the first
    cell of an image (its thread 0) or the last (its last thread), of the level-1 'dd' band or of the root block, alternating
    between the images at magnitudes a factor 4 apart (maxabs_cases.PACK_UNREACHED names the corners no picture reaches)"""
    H, W = M.pack_size(mode)
    n = 0
    for pics, targets in M.pack_batches(oracle, wavelet, mode):
        ref = np.stack([M.quantised(oracle, p, "f64", wavelet, mode, 2) for p in pics])
        got, ma = gpu_forward("f64", pics, None, 3, 2, H, W, wavelet, mode, 2, M.Q, None)
        same(got, ma, ref, (wavelet, mode, targets))
        n += 1
    assert n >= 2


# ---- F. k_absmax -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", M.ABSMAX_GEOMS)
def test_absmax(oracle, geom):
    """int32 arrays of |x| <= 3 with one cell of 2^k + 1 (either sign) per image, at both ends, every residue mod 4 and either
    side of multiples of 256 and 1024, both load paths (n = 0 and != 0 mod 4), three images a call: the word out of
    spiht_pyramid_batch_i32, and max_n and the stream out of spiht_amd.encode"""
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    L, ctx = _lib.lib(), _lib.default_context()
    c, h, w, lh, lw = geom
    n = c * h * w
    d_x, d_ma = DeviceArray(ctx, (3, n), np.int32), DeviceArray(ctx, (3,), np.uint32)
    d_dm, d_lm = DeviceArray(ctx, (3, n), np.uint8), DeviceArray(ctx, (3, n), np.uint8)
    try:
        for j, (x, ks) in enumerate(M.absmax_arrays(geom)):
            d_x.upload(x.reshape(3, n))
            ctx.memset(d_ma.ptr, 0xEE, d_ma.nbytes)
            _lib.check(L.spiht_pyramid_batch_i32(ctx.handle, vp(d_x.ptr), 3, c, h, w, lh, lw, vp(d_dm.ptr), vp(d_lm.ptr), vp(d_ma.ptr)))
            ctx.synchronize()
            assert d_ma.download().tolist() == [2 ** k + 1 for k in ks], (geom, j, ks)
            b = j % 3
            want, want_n = oracle.encode(x[b], lh, lw, 900)
            got, got_n = spiht_amd.encode(x[b], lh, lw, 900)
            assert want_n == ks[b] and (got_n, bytes(got)) == (want_n, want), (geom, j, b, got_n, want_n)
    finally:
        for d in (d_x, d_ma, d_dm, d_lm):
            d.free()
