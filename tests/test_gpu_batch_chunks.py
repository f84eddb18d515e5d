"""Both sides of the 65535-plane seam: batch_chunks (api_internal.h) cuts every batched call into launches of at most 65535 planes,
and before this module no test passed more, so no launch had b0 != 0, none had exactly 65535 planes in grid.y.  Here every
chunked entry point runs once through the seam -- 21852 distinct pictures of 3 planes: 65535 planes in the first launch, 21
in the second -- and the raw coder calls also with one plane per picture, where the chunk is 65535 pictures.  Every image of
every batch is compared with the CPU oracle (cases and references: tests/call_sequence_cases.py, held to their purpose by
tests/test_call_sequence_cases.py; the oracle's pass over the 21852 pictures is host time, 1.4 to 5.6 s by the host, spent
once inside whichever test asks first -- the GPU side of an item is some hundredths of a second); every output lies between guard regions that must survive; slot tails past a stream
must be zero.  Each case runs on a context of its own.

At that geometry (3 x 8 x 8, haar, one level) every per-picture size is 192 and the interleaved views are dense, so the first
half of the module cannot tell one offset from another.  The second half (test_seam2_*, test_two_pass_*) runs the same batch
of 21852 pictures -- 127 distinct ones in turn; the oracle's pass over them is 0.5 s of host time, once -- at K.SEAM2, 3 x 17
x 25 under bior2.2 at two levels, where the picture (1275 elements), the float64 reconstruction (1404), the coefficient
array (2835), the approximation plane of the two-part inverse (576) and the reduced pictures (576 / 240 dense, 495 as a view)
all differ, and at K.SEAM_PER for the two-pass kernels and the conversion passes; integer and float-kind pixels lie in views
whose every stride differs from the dense one (K.padded_strides), and the bytes between their samples must keep the guard
byte.  Every chunked image entry point runs there with b0 != 0; each test's docstring names the offsets it pins.  A batch
with a colour model is not among them: it is not bit-exact against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import call_sequence_cases as K
from test_gpu_coder_edges import GUARD, _slots, _unguard

pytestmark = pytest.mark.gpu
vp = C.c_void_p


class Scope:
    """a context of its own and the device arrays of one case, released together"""

    def __init__(self):
        from spiht_amd import _lib
        self.ctx = _lib.Context(0)
        self.L = _lib.lib()
        self.check = _lib.check
        self.arrays = []
        if os.environ.get("SPIHT_DECODER_WAVES"):  # runs of the whole suite on the 8-wavefront decoder
            self.ctx.set_decoder_waves(int(os.environ["SPIHT_DECODER_WAVES"]))

    def empty(self, shape, dtype):
        from spiht_amd.batch import DeviceArray
        d = DeviceArray(self.ctx, shape, dtype)
        self.arrays.append(d)
        return d

    def dev(self, arr, dtype=None):
        arr = np.ascontiguousarray(arr, dtype)
        d = self.empty(arr.shape, arr.dtype)
        d.upload(arr)
        return d

    def zeros(self, shape, dtype):
        d = self.empty(shape, dtype)
        d.zero()
        return d

    def guarded(self, shape, dtype):
        """a device array of shape[0] + 2 rows filled with the guard byte -> (array, pointer to row 1)"""
        d = self.empty((shape[0] + 2,) + tuple(shape[1:]), dtype)
        self.ctx.memset(d.ptr, GUARD, d.nbytes)
        return d, d.ptr + d.nbytes // (shape[0] + 2)

    def close(self):
        for d in self.arrays:
            d.free()
        self.arrays = []
        self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def ids(k):
    from spiht_amd import _lib
    L = _lib.lib()
    return L.spiht_wavelet_id(k["wavelet"].encode()), L.spiht_mode_id(k["mode"].encode()), -1 if k["level"] is None else k["level"]


def slot_bytes(geom, max_bits):
    from spiht_amd import _lib
    b = C.c_uint64()
    _lib.check(_lib.lib().spiht_encode_bound(*geom, 0x3FFFFFFF, max_bits or 0, C.byref(b)))
    return max(4, int(b.value))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_batch(got, want, what, where=None):
    """every image of the batch; the message names how many differ, the first ones, and which launch they were in"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = bits(got) != bits(want)
    if where is not None:
        ne &= where
    if ne.any():
        bad = np.nonzero(ne.reshape(len(got), -1).any(axis=1))[0]
        raise AssertionError("%s: %d of %d images differ, first %s" % (what, len(bad), len(got), bad[:8].tolist()))


def strided_hwc(P, dtype):
    """[B, c, H, W] uint8 pictures -> (host buffer [B, H, W, c] of dtype holding the same samples k / 255 = 257 k / 65535,
    byte strides (sb, sc, sh, sw))"""
    B, c, H, W = P.shape
    es = np.dtype(dtype).itemsize
    buf = np.ascontiguousarray(P.transpose(0, 2, 3, 1)).astype(dtype) * (257 if es == 2 else 1)
    return buf.astype(dtype), np.array([H * W * c * es, es, W * c * es, c * es], np.int64)


def to_int(pics, dtype):
    top = 255.0 if np.dtype(dtype) == np.uint8 else 65535.0
    return (np.clip(pics, 0.0, 1.0) * top).astype(dtype)


def encoded_same(s, d_out, d_nb, d_mn, R, slot, what):
    same_batch(_unguard(d_nb, what + " nbits"), R["nbits"], what + " nbits")
    same_batch(_unguard(d_mn, what + " max_n"), R["max_n"], what + " max_n")
    same_batch(_unguard(d_out, what + " slots"), K.slots_of(R["streams"], slot), what + " streams and the zeros behind them")


def streams_on_device(s, streams, max_n, slot):
    data, nbytes = _slots(streams, slot)  # (the bytes of a slot past its stream hold 0xFF)
    return s.dev(data), s.dev(nbytes), s.dev(np.asarray(max_n, np.uint8))


# ------------------------------------------------------------------------------------------------ the forward half

@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_dwt_quant_through_the_seam(oracle, kind):
    """spiht_dwt_quant_batch_f64 / _f32: Pic::at for dense float pictures, d_coeffs + b0 c enc_h enc_w"""
    k, P = K.CHUNK, K.chunk_pictures()
    want = K.chunk_reference(oracle)["coeffs"] if kind == "f64" else K.chunk_coeffs_f32(oracle)
    B, c = P.shape[:2]
    assert K.chunks(B, c) == [(0, 21845), (21845, 7)]
    wid, mid, lv = ids(k)
    with Scope() as s:
        d_img = s.dev(P / 255, np.float64 if kind == "f64" else np.float32)
        d_co, p_co = s.guarded((B, c * 64), np.int32)
        fn = s.L.spiht_dwt_quant_batch_f64 if kind == "f64" else s.L.spiht_dwt_quant_batch_f32
        s.check(fn(s.ctx.handle, vp(d_img.ptr), B, c, k["H"], k["W"], wid, mid, lv, k["q"], None, vp(p_co)))
        s.ctx.synchronize()
        same_batch(_unguard(d_co, "coefficients").reshape(want.shape), want, "coefficients (%s)" % kind)


@pytest.mark.parametrize("kind", ["f64", "u8", "u16"])
def test_dwt_pyramid_through_the_seam(oracle, kind):
    """spiht_dwt_pyramid_batch_f64 / _u8 / _u16 (the integer forms on an interleaved HWC view: Pic::at by px.sb):
    coefficients, D / L codes at every node that is looked up, and the max|coefficient| word of every image"""
    k, P, R = K.CHUNK, K.chunk_pictures(), K.chunk_reference(oracle)
    B, c = P.shape[:2]
    wid, mid, lv = ids(k)
    with Scope() as s:
        d_co, p_co = s.guarded((B, c * 64), np.int32)
        d_dm, p_dm = s.guarded((B, c * 64), np.uint8)
        d_lm, p_lm = s.guarded((B, c * 64), np.uint8)
        d_mx, p_mx = s.guarded((B,), np.uint32)
        tail = (B, c, k["H"], k["W"], wid, mid, lv, k["q"], None, vp(p_co), vp(p_dm), vp(p_lm), vp(p_mx))
        if kind == "f64":
            d_img = s.dev(P / 255, np.float64)
            s.check(s.L.spiht_dwt_pyramid_batch_f64(s.ctx.handle, vp(d_img.ptr), *tail))
        else:
            buf, st = strided_hwc(P, np.uint8 if kind == "u8" else np.uint16)
            d_img = s.dev(buf)
            fn = s.L.spiht_dwt_pyramid_batch_u8 if kind == "u8" else s.L.spiht_dwt_pyramid_batch_u16
            s.check(fn(s.ctx.handle, vp(d_img.ptr), vp(st.ctypes.data), *tail))
        s.ctx.synchronize()
        shape = R["coeffs"].shape
        same_batch(_unguard(d_co, "coefficients").reshape(shape), R["coeffs"], "coefficients (%s)" % kind)
        same_batch(_unguard(d_mx, "max words"), R["maxabs"], "max|coefficient| words (%s)" % kind)
        same_batch(_unguard(d_dm, "D codes").reshape(shape), R["dcode"], "D codes (%s)" % kind, R["d_where"][None])
        same_batch(_unguard(d_lm, "L codes").reshape(shape), R["lcode"], "L codes (%s)" % kind, R["l_where"][None])


@pytest.mark.parametrize("kind", ["f64", "u8"])
def test_encode_image_through_the_seam(oracle, kind):
    """spiht_encode_image_batch_f64 (with the caller's coefficient arrays: d_coeffs + b0 n) and _u8 (with the context's own):
    d_out + b0 slot_stride, d_nbits + b0, d_max_n + b0"""
    k, P, R = K.CHUNK, K.chunk_pictures(), K.chunk_reference(oracle)
    B, c = P.shape[:2]
    wid, mid, lv = ids(k)
    slot = slot_bytes((c, 8, 8, 4, 4), k["max_bits"])
    with Scope() as s:
        d_out, p_out = s.guarded((B, slot), np.uint8)
        d_nb, p_nb = s.guarded((B,), np.uint64)
        d_mn, p_mn = s.guarded((B,), np.uint8)
        if kind == "f64":
            d_img = s.dev(P / 255, np.float64)
            d_co, p_co = s.guarded((B, c * 64), np.int32)
            s.check(s.L.spiht_encode_image_batch_f64(s.ctx.handle, vp(d_img.ptr), B, c, k["H"], k["W"], wid, mid, lv, k["q"], None,
                                                     k["max_bits"], vp(p_out), slot, vp(p_nb), vp(p_mn), vp(p_co)))
        else:
            buf, st = strided_hwc(P, np.uint8)
            d_img = s.dev(buf)
            s.check(s.L.spiht_encode_image_batch_u8(s.ctx.handle, vp(d_img.ptr), vp(st.ctypes.data), B, c, k["H"], k["W"], wid, mid,
                                                    lv, k["q"], None, k["max_bits"], vp(p_out), slot, vp(p_nb), vp(p_mn), None))
        s.ctx.synchronize()
        encoded_same(s, d_out, d_nb, d_mn, R, slot, "encode_image (%s)" % kind)
        if kind == "f64":
            same_batch(_unguard(d_co, "coefficients").reshape(R["coeffs"].shape), R["coeffs"], "the caller's coefficient arrays")


# ------------------------------------------------------------------------------------------------ the inverse half

@pytest.mark.parametrize("kind", ["f64-internal", "f64-rec", "u8-internal", "u8-rec", "reduced-internal", "reduced-rec"])
def test_decode_image_through_the_seam(oracle, kind):
    """spiht_decode_image_batch_f64 / _u8 and the float64 decode at reduce = 1 (ImgCall::at on the reduced geometry), each
    with the context's internal array (zeroed again between the two launches: the first reuses its slots) and with a
    caller's d_rec (d_rec + b0 n)"""
    k, R = K.CHUNK, K.chunk_reference(oracle)
    B, c = R["coeffs"].shape[:2]
    wid, mid, lv = ids(k)
    form, own_rec = kind.split("-")
    slot = 52
    with Scope() as s:
        d_data, d_ny, d_mn = streams_on_device(s, R["streams"], R["max_n"], slot)
        p_rec = None
        if own_rec == "rec":
            d_rec, p_rec = s.guarded((B, c * 64), np.int32)
        head = (s.ctx.handle, vp(d_data.ptr), slot, vp(d_ny.ptr), vp(d_mn.ptr), B, c, k["H"], k["W"], wid, mid, lv, k["q"], None)
        if form == "f64":
            d_img, p_img = s.guarded((B, c * 64), np.float64)
            s.check(s.L.spiht_decode_image_batch_f64(*head, vp(p_img), vp(p_rec)))
            want = R["pics"]
        elif form == "reduced":
            d_img, p_img = s.guarded((B, c * 16), np.float64)
            s.check(s.L.spiht_decode_image_reduced_batch_f64(*head, vp(p_img), vp(p_rec), 1))
            want = R["half"]
        else:
            d_img, p_img = s.guarded((B, 8, 8, c), np.uint8)
            st = np.array([64 * c, 1, 8 * c, c], np.int64)
            s.check(s.L.spiht_decode_image_batch_u8(*head, vp(p_img), vp(st.ctypes.data), vp(p_rec)))
            want = to_int(R["pics"], np.uint8)
        s.ctx.synchronize()
        got = _unguard(d_img, "pictures")
        got = got.transpose(0, 3, 1, 2) if form == "u8" else got.reshape(want.shape)
        same_batch(np.ascontiguousarray(got), want, "pictures (%s)" % kind)
        if p_rec:
            same_batch(_unguard(d_rec, "d_rec").reshape(R["rec"].shape), R["rec"], "the caller's decoded arrays (%s)" % kind)


def test_idwt_flags_through_the_seam(oracle):
    """spiht_dequant_idwt_flags_batch_f64 at a two-level geometry, where spiht_l1_flags_words is not zero: d_flags + b0 c gy gx.
    About half the words are zero; 127 coefficient arrays in turn (the image at the seam is not the first of them, and a
    launch that read the words of picture 0 for picture 21845 would skip detail bands that hold coefficients)."""
    k, R = K.FLAGS, K.flags_reference(oracle)
    B, c = K.CHUNK_B, k["c"]
    wid, mid, lv = ids(k)
    words = C.c_uint64()
    from spiht_amd import _lib
    _lib.check(_lib.lib().spiht_l1_flags_words(c, k["H"], k["W"], wid, mid, lv, C.byref(words)))
    assert words.value == R["words"][0].size == 3
    which = np.arange(B) % K.FLAGS_DISTINCT
    with Scope() as s:
        d_rec = s.dev(R["rec"][which])
        d_fl = s.dev(R["words"][which])
        shape = R["pics"].shape[1:]
        d_img, p_img = s.guarded((B, int(np.prod(shape))), np.float64)
        s.check(s.L.spiht_dequant_idwt_flags_batch_f64(s.ctx.handle, vp(d_rec.ptr), vp(d_fl.ptr), B, c, k["H"], k["W"], wid, mid, lv,
                                                       k["q"], None, vp(p_img)))
        s.ctx.synchronize()
        same_batch(_unguard(d_img, "pictures").reshape((B,) + shape), R["pics"][which], "pictures")


# ------------------------------------------------------------------------------------------------ the raw coder calls

def raw_coder_case(s, call, xs, dcode, lcode, streams, nbits, max_n, rec, geom, max_bits, what):
    """one of spiht_encode_batch_i32 / spiht_encode_lists_batch_i32 / spiht_decode_batch_i32 on the batch xs [B, c, h, w]"""
    c, h, w, lh, lw = geom
    B, n = len(xs), c * h * w
    slot = slot_bytes(geom, max_bits)
    R = dict(streams=streams, nbits=nbits, max_n=max_n)
    if call == "decode_batch":
        d_data, d_ny, d_mn = streams_on_device(s, streams, max_n, slot)
        d_rec, p_rec = s.guarded((B, n), np.int32)
        s.check(s.L.spiht_decode_batch_i32(s.ctx.handle, vp(d_data.ptr), slot, vp(d_ny.ptr), vp(d_mn.ptr), B, c, h, w, lh, lw, vp(p_rec)))
        s.ctx.synchronize()
        same_batch(_unguard(d_rec, what).reshape(rec.shape), rec, what)
        return
    d_x = s.dev(xs, np.int32)
    d_out, p_out = s.guarded((B, slot), np.uint8)
    d_nb, p_nb = s.guarded((B,), np.uint64)
    d_mn, p_mn = s.guarded((B,), np.uint8)
    if call == "encode_batch":
        s.check(s.L.spiht_encode_batch_i32(s.ctx.handle, vp(d_x.ptr), B, c, h, w, lh, lw, max_bits, vp(p_out), slot, vp(p_nb), vp(p_mn)))
    else:  # the codes and maxima the oracle gives (only the nodes that are looked up carry a code: the rest is never read)
        d_dm, d_lm = s.dev(dcode), s.dev(lcode)
        d_mx = s.dev(np.abs(xs.astype(np.int64)).reshape(B, -1).max(axis=1).astype(np.uint32))
        s.check(s.L.spiht_encode_lists_batch_i32(s.ctx.handle, vp(d_x.ptr), vp(d_dm.ptr), vp(d_lm.ptr), vp(d_mx.ptr), B, c, h, w, lh, lw,
                                                 max_bits, vp(p_out), slot, vp(p_nb), vp(p_mn)))
    s.ctx.synchronize()
    encoded_same(s, d_out, d_nb, d_mn, R, slot, what)


@pytest.mark.parametrize("call", ["encode_batch", "encode_lists", "decode_batch"])
def test_raw_coder_through_the_seam(oracle, call):
    """spiht_encode_batch_i32 and spiht_encode_lists_batch_i32 (its alloc_lists per chunk) on the 21852 coefficient arrays,
    and spiht_decode_batch_i32 -- which is not chunked: it walks the batch by slots -- on their streams"""
    R = K.chunk_reference(oracle)
    with Scope() as s:
        raw_coder_case(s, call, R["coeffs"], R["dcode"], R["lcode"], R["streams"], R["nbits"], R["max_n"], R["rec"], (3, 8, 8, 4, 4),
                       K.CHUNK["max_bits"], call)


@pytest.mark.parametrize("call", ["encode_batch", "encode_lists", "decode_batch"])
def test_one_plane_per_picture(oracle, call):
    """c = 1: the chunk is 65535 pictures exactly (a launch of 65535 in grid.y), 5 pictures behind it.  61 arrays in turn --
    a prime that does not divide 65535, so the picture at the seam is not the first of them"""
    k, R = K.ONE_PLANE, K.one_plane_reference(oracle)
    B = K.ONE_PLANE_B
    assert K.chunks(B, 1) == [(0, 65535), (65535, 5)]
    which = np.arange(B) % K.ONE_PLANE_DISTINCT
    codes = [oracle.set_codes(x, k["ll_h"], k["ll_w"]) for x in R["xs"]]
    dcode, lcode = np.stack([cd[0] for cd in codes]), np.stack([cd[1] for cd in codes])
    with Scope() as s:
        raw_coder_case(s, call, R["xs"][which], dcode[which], lcode[which], [R["streams"][i] for i in which], R["nbits"][which],
                       R["max_n"][which], R["rec"][which], (k["c"], k["h"], k["w"], k["ll_h"], k["ll_w"]), k["max_bits"], call)


def test_limits_are_refused(oracle):
    """spiht_pyramid_batch_i32 and spiht_color3_batch_f64 are not chunked: more than 65535 planes / pictures is
    SPIHT_ERR_ARG before anything is queued, exactly 65535 is taken, and the context works afterwards"""
    R = K.one_plane_reference(oracle)
    k = K.ONE_PLANE
    geom = (k["c"], k["h"], k["w"], k["ll_h"], k["ll_w"])
    which = np.arange(K.SEAM + 1) % K.ONE_PLANE_DISTINCT
    with Scope() as s:
        xs = R["xs"][which]
        d_x = s.dev(xs)
        d_dm, p_dm = s.guarded((K.SEAM + 1, 64), np.uint8)
        d_lm, p_lm = s.guarded((K.SEAM + 1, 64), np.uint8)
        d_mx, p_mx = s.guarded((K.SEAM + 1,), np.uint32)
        args = (1, 8, 8, 4, 4, vp(p_dm), vp(p_lm), vp(p_mx))
        with pytest.raises(ValueError):
            s.check(s.L.spiht_pyramid_batch_i32(s.ctx.handle, vp(d_x.ptr), K.SEAM + 1, *args))
        with pytest.raises(ValueError):
            s.check(s.L.spiht_pyramid_batch_i32(s.ctx.handle, vp(d_x.ptr), 21846, 3, 8, 8, 4, 4, vp(p_dm), vp(p_lm), vp(p_mx)))
        s.ctx.synchronize()
        for d in (d_dm, d_lm, d_mx):  # nothing was queued
            assert (d.download() == np.frombuffer(bytes([GUARD]) * d.dtype.itemsize, d.dtype)[0]).all()
        s.check(s.L.spiht_pyramid_batch_i32(s.ctx.handle, vp(d_x.ptr), K.SEAM, *args))
        s.ctx.synchronize()
        mx = d_mx.download()
        assert np.array_equal(mx[1:K.SEAM + 1], np.abs(xs[:K.SEAM].astype(np.int64)).reshape(K.SEAM, -1).max(axis=1))
        assert mx[K.SEAM + 1] == mx[0]  # (the row past the call's last image is still guard bytes)
        has = oracle.set_codes(R["xs"][0], 4, 4)[2]
        dm = d_dm.download()[1:K.SEAM + 1].reshape(K.SEAM, 1, 8, 8)
        want = np.stack([oracle.set_codes(x, 4, 4)[0] for x in R["xs"]])[which[:K.SEAM]]
        same_batch(dm, want, "D codes of 65535 planes", has[None])
        # the colour change: 65536 pictures of one pixel (RGB -> IPT; the bound is the one of
        # test_device_colour_conversion_and_config3_batch: the device's power function is within 4 units in the last place)
        from spiht_amd import color_models
        A, M, p = color_models._params("RGB", "IPT")
        A, M = np.ascontiguousarray(A), np.ascontiguousarray(M)
        d_px = s.dev(np.random.default_rng(3).random((K.SEAM + 1, 3, 1)))
        d_to = s.zeros((K.SEAM + 1, 3, 1), np.float64)
        with pytest.raises(ValueError):
            s.check(s.L.spiht_color3_batch_f64(s.ctx.handle, vp(d_px.ptr), vp(d_to.ptr), K.SEAM + 1, 1, vp(A.ctypes.data), vp(M.ctypes.data), p))
        s.ctx.synchronize()
        assert not d_to.download().any()
        s.check(s.L.spiht_color3_batch_f64(s.ctx.handle, vp(d_px.ptr), vp(d_to.ptr), K.SEAM, 1, vp(A.ctypes.data), vp(M.ctypes.data), p))
        s.ctx.synchronize()
        got, src = d_to.download(), d_px.download()
        assert not got[K.SEAM].any()
        want = oracle.color3(src[:K.SEAM].transpose(1, 0, 2).copy(), A, M, p).transpose(1, 0, 2)
        assert np.abs(got[:K.SEAM] - want).max() < 2e-14, float(np.abs(got[:K.SEAM] - want).max())
        # the context works afterwards
        raw_coder_case(s, "encode_batch", R["xs"], None, None, R["streams"], R["nbits"], R["max_n"], R["rec"], geom, k["max_bits"], "afterwards")


# ------------------------------------------------------------ the seam where no two sizes agree (K.SEAM2, K.SEAM_PER)
# At K.CHUNK every per-picture size is 3 * 64 and strided_hwc() is dense; below, every array of a call has a size of its own
# (tests/test_call_sequence_cases.py asserts it) and every integer or float-kind view is K.padded_strides': RGBA-like
# pixels, padded rows, spare rows behind each picture, the guard byte in all of it before the call and after.

PX = {"u8": (1, 0), "u16": (2, 0), "f32": (4, 1), "f16": (2, 2), "bf16": (2, 3)}  # kind: (element size, float kind or 0)


def px_want(pics, kind, h, w):
    """what a view of the kind holds of float64 pictures [.., rec_h, rec_w]: cropped to h x w, then the integer rule
    (to_int) or spiht_amd.floatpx.convert; float kinds as the unsigned integers of their bits"""
    from spiht_amd import floatpx
    p = np.ascontiguousarray(pics[..., :h, :w])
    if not PX[kind][1]:
        return to_int(p, np.uint8 if kind == "u8" else np.uint16)
    return np.ascontiguousarray(floatpx.convert(p, PX[kind][1])).view(np.dtype("u%d" % PX[kind][0]))


def padded_out(s, B, c, h, w, kind):
    """a device buffer of B padded pictures between two guard rows, all of it guard bytes -> (array, pointer, strides)"""
    es = PX[kind][0]
    st = K.padded_strides(c, h, w, es)
    d, p = s.guarded((B, int(st[0]) // es), np.dtype("u%d" % es))
    return d, p, st


def padded_got(d, c, h, w, what):
    """the samples [B, c, h, w] of a padded_out buffer (float kinds as their bits); guard rows and padding untouched"""
    buf = _unguard(d, what)
    assert K.padding_untouched(buf, c, h, w), "%s: bytes between the samples were written" % what
    return np.ascontiguousarray(K.samples_of(buf, c, h, w))


def padded_in(s, P, dtype):
    """uint8 pictures [B, c, H, W] as a padded view of dtype on the device (k / 255 = 257 k / 65535) -> (array, strides)"""
    buf, view, st = K.padded_buffer(*P.shape, dtype)
    view[...] = P.astype(dtype) * (257 if np.dtype(dtype).itemsize == 2 else 1)
    return s.dev(buf), st


def px_call(s, name, kind, *args):
    """name_u8 / name_u16 / name_flt (the kind behind the context)"""
    if PX[kind][1]:
        s.check(getattr(s.L, name + "_flt")(s.ctx.handle, PX[kind][1], *args))
    else:
        s.check(getattr(s.L, name + "_" + kind)(s.ctx.handle, *args))


def seam_case(oracle, k=None):
    """(case, reference over the distinct pictures, which of them stands where, B, ids, (c, enc_h, enc_w, ll_h, ll_w))"""
    k = k or K.SEAM2
    R = K.seam2_reference(oracle) if k is K.SEAM2 else K.seam_per_reference(oracle)
    which = K.in_turn(K.SEAM2_DISTINCT if k is K.SEAM2 else K.SEAM_PER_DISTINCT)
    g = R["geom"]
    assert K.chunks(len(which), k["c"]) == [(0, 21845), (21845, 7)]
    return k, R, which, len(which), ids(k), (k["c"], g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"])


def encoded_reference(R, which, f32=False):
    t = "_f32" if f32 else ""
    return dict(streams=[R["streams" + t][i] for i in which], nbits=R["nbits" + t][which], max_n=R["max_n" + t][which])


def coeffs_same(d_co, want, which, what):
    same_batch(_unguard(d_co, what).reshape((len(which),) + want.shape[1:]), want[which], what)


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_seam2_dwt_quant(oracle, kind):
    """spiht_dwt_quant_batch_f64 / _f32 on dense pictures: Pic::at steps by b0 c H W (1275 elements a picture), the
    coefficient arrays by b0 c enc_h enc_w (2835)"""
    k, R, which, B, (wid, mid, lv), geom = seam_case(oracle)
    c, n = k["c"], int(np.prod(geom[:3]))
    with Scope() as s:
        d_img = s.dev(K.seam_pictures(k, K.SEAM2_DISTINCT)[which] / 255, np.float64 if kind == "f64" else np.float32)
        d_co, p_co = s.guarded((B, n), np.int32)
        fn = s.L.spiht_dwt_quant_batch_f64 if kind == "f64" else s.L.spiht_dwt_quant_batch_f32
        s.check(fn(s.ctx.handle, vp(d_img.ptr), B, c, k["H"], k["W"], wid, mid, lv, k["q"], None, vp(p_co)))
        s.ctx.synchronize()
        coeffs_same(d_co, R["coeffs" if kind == "f64" else "coeffs_f32"], which, "coefficients (%s)" % kind)


def test_seam2_dwt_pyramid_u16(oracle):
    """spiht_dwt_pyramid_batch_u16 on a padded view: Pic::at steps by b0 px.sb (no dense size), d_coeffs / d_dmsb / d_lmsb by
    b0 g.n, d_maxabs by b0"""
    k, R, which, B, (wid, mid, lv), geom = seam_case(oracle)
    c, n = k["c"], int(np.prod(geom[:3]))
    with Scope() as s:
        d_img, st = padded_in(s, K.seam_pictures(k, K.SEAM2_DISTINCT)[which], np.uint16)
        d_co, p_co = s.guarded((B, n), np.int32)
        d_dm, p_dm = s.guarded((B, n), np.uint8)
        d_lm, p_lm = s.guarded((B, n), np.uint8)
        d_mx, p_mx = s.guarded((B,), np.uint32)
        s.check(s.L.spiht_dwt_pyramid_batch_u16(s.ctx.handle, vp(d_img.ptr), vp(st.ctypes.data), B, c, k["H"], k["W"], wid, mid, lv,
                                                k["q"], None, vp(p_co), vp(p_dm), vp(p_lm), vp(p_mx)))
        s.ctx.synchronize()
        shape = (B,) + R["coeffs"].shape[1:]
        coeffs_same(d_co, R["coeffs"], which, "coefficients")
        same_batch(_unguard(d_mx, "max words"), R["maxabs"][which], "max|coefficient| words")
        same_batch(_unguard(d_dm, "D codes").reshape(shape), R["dcode"][which], "D codes", R["d_where"][None])
        same_batch(_unguard(d_lm, "L codes").reshape(shape), R["lcode"][which], "L codes", R["l_where"][None])


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_seam2_encode_image(oracle, kind):
    """spiht_encode_image_batch_f32 on dense float32 pictures (b0 c H W 4 bytes) with the caller's coefficient arrays
    (d_coeffs + b0 g.n), against the single-precision transform; spiht_encode_image_batch_u16 on a padded view (b0 px.sb) with
    the context's own array.  Both: d_out + b0 slot_stride, d_nbits + b0, d_max_n + b0, and zeros behind every stream"""
    k, R, which, B, (wid, mid, lv), geom = seam_case(oracle)
    c, n = k["c"], int(np.prod(geom[:3]))
    slot = slot_bytes(geom, k["max_bits"])
    P = K.seam_pictures(k, K.SEAM2_DISTINCT)[which]
    with Scope() as s:
        d_out, p_out = s.guarded((B, slot), np.uint8)
        d_nb, p_nb = s.guarded((B,), np.uint64)
        d_mn, p_mn = s.guarded((B,), np.uint8)
        tail = (B, c, k["H"], k["W"], wid, mid, lv, k["q"], None, k["max_bits"], vp(p_out), slot, vp(p_nb), vp(p_mn))
        if kind == "f32":
            d_img = s.dev(P / 255, np.float32)
            d_co, p_co = s.guarded((B, n), np.int32)
            s.check(s.L.spiht_encode_image_batch_f32(s.ctx.handle, vp(d_img.ptr), *tail, vp(p_co)))
        else:
            d_img, st = padded_in(s, P, np.uint16)
            s.check(s.L.spiht_encode_image_batch_u16(s.ctx.handle, vp(d_img.ptr), vp(st.ctypes.data), *tail, None))
        s.ctx.synchronize()
        encoded_same(s, d_out, d_nb, d_mn, encoded_reference(R, which, kind == "f32"), slot, "encode_image (%s)" % kind)
        if kind == "f32":
            coeffs_same(d_co, R["coeffs_f32"], which, "the caller's coefficient arrays")


@pytest.mark.parametrize("kind", ["f64", "u8", "u16", "f32", "f16", "bf16"])
def test_seam2_dequant_idwt(oracle, kind):
    """spiht_dequant_idwt_batch_f64 without occupancy words (d_rec + b0 c enc_h enc_w; dense output by pig = ig: b0 c rec_H
    rec_W, 1404 where the input pictures have 1275), and spiht_dequant_idwt_flags_batch_u8 / _u16 / _flt (all three kinds)
    into padded views (b0 px.sb) with about half the words zero (d_flags + b0 c gy gx)"""
    k, R, which, B, (wid, mid, lv), geom = seam_case(oracle)
    c, H, W = k["c"], k["H"], k["W"]
    with Scope() as s:
        head = (B, c, H, W, wid, mid, lv, k["q"], None)
        if kind == "f64":
            d_rec = s.dev(R["rec"][which])
            d_img, p_img = s.guarded((B, int(np.prod(R["pics"].shape[1:]))), np.float64)
            s.check(s.L.spiht_dequant_idwt_batch_f64(s.ctx.handle, vp(d_rec.ptr), *head, vp(p_img)))
            s.ctx.synchronize()
            same_batch(_unguard(d_img, "pictures").reshape((B,) + R["pics"].shape[1:]), R["pics"][which], "pictures")
            return
        d_rec, d_fl = s.dev(R["rec_fl"][which]), s.dev(R["words"][which])
        d_img, p_img, st = padded_out(s, B, c, H, W, kind)
        px_call(s, "spiht_dequant_idwt_flags_batch", kind, vp(d_rec.ptr), vp(d_fl.ptr), *head, vp(p_img), vp(st.ctypes.data))
        s.ctx.synchronize()
        same_batch(padded_got(d_img, c, H, W, "pictures"), px_want(R["pics_fl"], kind, H, W)[which], "pictures (%s)" % kind)


@pytest.mark.parametrize("call", ["level1_f64", "flags_f64", "flags_u8", "flags_u16"])
def test_seam2_two_part_inverse(oracle, call):
    """spiht_idwt_coarse_batch_f64 into a guarded d_approx (d_approx + b0 c a_plane, a_plane = 12 x 16 and not hs[1] x ws[1]),
    then spiht_idwt_level1_batch_f64 / spiht_idwt_level1_flags_batch_f64 / _u8 / _u16 reading it (the same offset, d_rec + b0
    c enc_h enc_w, d_flags + b0 c gy gx, the pictures by Pic::at).  d_approx itself is asserted for every image: it is twice
    the oracle's reduced picture at k = 1 (the reduced reconstruction before scaling and cropping), exactly."""
    k, R, which, B, (wid, mid, lv), geom = seam_case(oracle)
    c, H, W = k["c"], k["H"], k["W"]
    flagged = call != "level1_f64"
    with Scope() as s:
        d_rec = s.dev(R["rec_fl" if flagged else "rec"][which])
        d_ap, p_ap = s.guarded((B, int(np.prod(R["approx"].shape[1:]))), np.float64)
        head = (B, c, H, W, wid, mid, lv, k["q"], None)
        s.check(s.L.spiht_idwt_coarse_batch_f64(s.ctx.handle, vp(d_rec.ptr), *head, vp(p_ap)))
        want = R["pics_fl" if flagged else "pics"]
        if call.endswith("f64"):
            d_img, p_img = s.guarded((B, int(np.prod(want.shape[1:]))), np.float64)
            if flagged:
                d_fl = s.dev(R["words"][which])
                s.check(s.L.spiht_idwt_level1_flags_batch_f64(s.ctx.handle, vp(d_rec.ptr), vp(p_ap), vp(d_fl.ptr), *head, vp(p_img)))
            else:
                s.check(s.L.spiht_idwt_level1_batch_f64(s.ctx.handle, vp(d_rec.ptr), vp(p_ap), *head, vp(p_img)))
            s.ctx.synchronize()
            same_batch(_unguard(d_img, "pictures").reshape((B,) + want.shape[1:]), want[which], "pictures (%s)" % call)
        else:
            kind = call.split("_")[1]
            d_fl = s.dev(R["words"][which])
            d_img, p_img, st = padded_out(s, B, c, H, W, kind)
            px_call(s, "spiht_idwt_level1_flags_batch", kind, vp(d_rec.ptr), vp(p_ap), vp(d_fl.ptr), *head, vp(p_img), vp(st.ctypes.data))
            s.ctx.synchronize()
            same_batch(padded_got(d_img, c, H, W, "pictures"), px_want(want, kind, H, W)[which], "pictures (%s)" % call)
        same_batch(_unguard(d_ap, "d_approx").reshape((B,) + R["approx"].shape[1:]), R["approx"][which], "d_approx (%s)" % call)


@pytest.mark.parametrize("reduce", [1, 2])
@pytest.mark.parametrize("kind", ["f64", "u8", "u16", "f32", "f16", "bf16"])
def test_seam2_dequant_idwt_reduced(oracle, kind, reduce):
    """spiht_dequant_idwt_reduced_batch_f64 / _u8 / _u16 / _flt at reduce = 1 (a synthesis level runs) and reduce = 2 = L
    (k_ll_to_pic): d_rec + b0 c enc_h enc_w by the FULL geometry, the pictures by the reduced one -- ImgCall::at takes pig, not
    ig: dense b0 c 12 16 / b0 c 8 10 where ig would give b0 c 18 26; views b0 px.sb of the 11 x 15 / 8 x 10 pictures"""
    k, R, which, B, (wid, mid, lv), geom = seam_case(oracle)
    c = k["c"]
    want = R["red"][reduce]
    h, w = R["geom"]["hs"][reduce], R["geom"]["ws"][reduce]
    with Scope() as s:
        d_rec = s.dev(R["rec"][which])
        head = (vp(d_rec.ptr), B, c, k["H"], k["W"], wid, mid, lv, k["q"], None)
        if kind == "f64":
            d_img, p_img = s.guarded((B, int(np.prod(want.shape[1:]))), np.float64)
            s.check(s.L.spiht_dequant_idwt_reduced_batch_f64(s.ctx.handle, *head, vp(p_img), reduce))
            s.ctx.synchronize()
            same_batch(_unguard(d_img, "pictures").reshape((B,) + want.shape[1:]), want[which], "pictures")
            return
        d_img, p_img, st = padded_out(s, B, c, h, w, kind)
        px_call(s, "spiht_dequant_idwt_reduced_batch", kind, *head, vp(p_img), vp(st.ctypes.data), reduce)
        s.ctx.synchronize()
        same_batch(padded_got(d_img, c, h, w, "pictures"), px_want(want, kind, h, w)[which], "pictures (%s, reduce %d)" % (kind, reduce))


def fused_decode_case(oracle, k, name, kind, own_rec, want, h, w, *extra):
    """one fused decode into a padded view of the kind, with the context's internal array or a caller's d_rec"""
    k, R, which, B, (wid, mid, lv), geom = seam_case(oracle, k)
    c, n = k["c"], int(np.prod(geom[:3]))
    slot = slot_bytes(geom, k["max_bits"])
    with Scope() as s:
        d_data, d_ny, d_mn = streams_on_device(s, [R["streams"][i] for i in which], R["max_n"][which], slot)
        p_rec = None
        if own_rec == "rec":
            d_rec, p_rec = s.guarded((B, n), np.int32)
        d_img, p_img, st = padded_out(s, B, c, h, w, kind)
        px_call(s, name, kind, vp(d_data.ptr), slot, vp(d_ny.ptr), vp(d_mn.ptr), B, c, k["H"], k["W"], wid, mid, lv, k["q"], None,
                vp(p_img), vp(st.ctypes.data), vp(p_rec), *extra)
        s.ctx.synchronize()
        same_batch(padded_got(d_img, c, h, w, "pictures"), px_want(want, kind, h, w)[which], "pictures (%s, %s)" % (kind, own_rec))
        if p_rec:
            coeffs_same(d_rec, R["rec"], which, "the caller's decoded arrays (%s)" % kind)


@pytest.mark.parametrize("own_rec", ["internal", "rec"])
@pytest.mark.parametrize("kind", ["u8", "u16", "f16"])
def test_seam2_decode_image_reduced(oracle, kind, own_rec):
    """spiht_decode_image_reduced_batch_u8 / _u16 / _flt at reduce = 1: streams by b0 slot_stride, d_nbytes / d_max_n by b0,
    d_rec + b0 g.n (or the internal array, zeroed again between the launches), the 11 x 15 pictures by b0 px.sb"""
    R = K.seam2_reference(oracle)
    fused_decode_case(oracle, K.SEAM2, "spiht_decode_image_reduced_batch", kind, own_rec, R["red"][1], R["geom"]["hs"][1],
                      R["geom"]["ws"][1], 1)


@pytest.mark.parametrize("own_rec", ["internal", "rec"])
@pytest.mark.parametrize("kind", ["u16", "f16"])
def test_seam2_decode_image(oracle, kind, own_rec):
    """spiht_decode_image_batch_u16 / _flt (float16; the other two kinds run through the seam in test_seam2_dequant_idwt):
    streams by b0 slot_stride, d_nbytes / d_max_n by b0, d_rec + b0 g.n, the decoder's own occupancy words per chunk, the
    pictures by b0 px.sb"""
    fused_decode_case(oracle, K.SEAM2, "spiht_decode_image_batch", kind, own_rec, K.seam2_reference(oracle)["pics"], K.SEAM2["H"],
                      K.SEAM2["W"])


@pytest.mark.parametrize("call", ["dwt_quant_f64", "encode_u8", "decode_u8", "decode_f32"])
def test_two_pass_levels_through_the_seam(oracle, call):
    """K.SEAM_PER (periodization): the two-pass kernels, whose temporaries are carved per chunk from `planes`.
    spiht_dwt_quant_batch_f64 (k_dwt_axis_ext, k_dwt_pack_ext: pictures by b0 c 9 13, arrays by b0 c 10 14);
    spiht_encode_image_batch_u8 on a padded view (k_px_to_f64 in front of them, into ctx->pix per chunk);
    spiht_decode_image_batch_u8 / _flt (k_idwt_axis_per, then the k_f64_to_px pass from ctx->pix into the padded view)"""
    k = K.SEAM_PER
    k, R, which, B, (wid, mid, lv), geom = seam_case(oracle, k)
    c, n = k["c"], int(np.prod(geom[:3]))
    if call.startswith("decode"):
        fused_decode_case(oracle, k, "spiht_decode_image_batch", call.split("_")[1], "internal", R["pics"], k["H"], k["W"])
        return
    P = K.seam_pictures(k, K.SEAM_PER_DISTINCT)[which]
    with Scope() as s:
        if call == "dwt_quant_f64":
            d_img = s.dev(P / 255, np.float64)
            d_co, p_co = s.guarded((B, n), np.int32)
            s.check(s.L.spiht_dwt_quant_batch_f64(s.ctx.handle, vp(d_img.ptr), B, c, k["H"], k["W"], wid, mid, lv, k["q"], None, vp(p_co)))
            s.ctx.synchronize()
            coeffs_same(d_co, R["coeffs"], which, "coefficients")
            return
        slot = slot_bytes(geom, k["max_bits"])
        d_img, st = padded_in(s, P, np.uint8)
        d_out, p_out = s.guarded((B, slot), np.uint8)
        d_nb, p_nb = s.guarded((B,), np.uint64)
        d_mn, p_mn = s.guarded((B,), np.uint8)
        s.check(s.L.spiht_encode_image_batch_u8(s.ctx.handle, vp(d_img.ptr), vp(st.ctypes.data), B, c, k["H"], k["W"], wid, mid, lv,
                                                k["q"], None, k["max_bits"], vp(p_out), slot, vp(p_nb), vp(p_mn), None))
        s.ctx.synchronize()
        encoded_same(s, d_out, d_nb, d_mn, encoded_reference(R, which), slot, "encode_image (u8, two-pass)")


def test_a_picture_of_too_many_planes_is_refused(oracle):
    """c = 65536: batch_chunks never cuts inside a picture, and the launchers carry a launch's planes in grid.y / grid.z.  One
    call of each family -- forward, fused encode, inverse, fused decode (and spiht_encode_batch_i32) -- is SPIHT_ERR_TOO_LARGE
    before anything is queued: the guard-filled outputs are untouched after a synchronize, and the context works afterwards"""
    c, H, W = K.SEAM + 1, 2, 2
    R1 = K.one_plane_reference(oracle)
    k1 = K.ONE_PLANE
    with Scope() as s:
        wid, mid = s.L.spiht_wavelet_id(b"haar"), s.L.spiht_mode_id(b"reflect")
        d_img = s.dev(np.full((1, c, H, W), 0.5))
        d_x = s.dev(np.ones((1, c, H, W), np.int32))
        outs = dict(co=s.guarded((1, c * H * W), np.int32), out=s.guarded((1, 64), np.uint8), nb=s.guarded((1,), np.uint64),
                    mn=s.guarded((1,), np.uint8), img=s.guarded((1, c * H * W), np.float64), rec=s.guarded((1, c * H * W), np.int32))
        p = {name: vp(v[1]) for name, v in outs.items()}
        d_data, d_ny, d_n = s.zeros((1, 64), np.uint8), s.dev(np.array([8], np.uint64)), s.dev(np.array([3], np.uint8))
        geo = (1, c, H, W, wid, mid, 1, 50.0, None)
        calls = [
            lambda: s.L.spiht_dwt_quant_batch_f64(s.ctx.handle, vp(d_img.ptr), *geo, p["co"]),
            lambda: s.L.spiht_encode_image_batch_f64(s.ctx.handle, vp(d_img.ptr), *geo, 400, p["out"], 64, p["nb"], p["mn"], p["co"]),
            lambda: s.L.spiht_dequant_idwt_batch_f64(s.ctx.handle, vp(d_x.ptr), *geo, p["img"]),
            lambda: s.L.spiht_decode_image_batch_f64(s.ctx.handle, vp(d_data.ptr), 64, vp(d_ny.ptr), vp(d_n.ptr), *geo, p["img"], p["rec"]),
            lambda: s.L.spiht_encode_batch_i32(s.ctx.handle, vp(d_x.ptr), 1, c, 4, 4, 2, 2, 400, p["out"], 64, p["nb"], p["mn"]),
        ]
        for call in calls:
            with pytest.raises(OverflowError):  # (_lib.check: SPIHT_ERR_TOO_LARGE)
                s.check(call())
        s.ctx.synchronize()
        for name, (d, _) in outs.items():  # nothing was queued
            assert (d.download().view(np.uint8) == GUARD).all(), name
        # 65535 planes are no error of this kind (the geometry's own status: a 1 x 1 root block), and the context works afterwards
        from spiht_amd import _lib
        with pytest.raises(_lib.PanicException):  # SPIHT_ERR_LL
            s.check(s.L.spiht_encode_image_batch_f64(s.ctx.handle, vp(d_img.ptr), 1, K.SEAM, H, W, wid, mid, 1, 50.0, None, 400, p["out"],
                                                     64, p["nb"], p["mn"], None))
        geom = (k1["c"], k1["h"], k1["w"], k1["ll_h"], k1["ll_w"])
        raw_coder_case(s, "encode_batch", R1["xs"], None, None, R1["streams"], R1["nbits"], R1["max_n"], R1["rec"], geom, k1["max_bits"],
                       "afterwards")


# ------------------------------------------------------------------------------------------------ the Python level

def test_batch_codec_through_the_second_seam(oracle):
    """BatchCodec on K.SEAM2: encode_u16 -> every EncodingResult; decode_float(float16) and decode_reduced(.., 1, crop=True)
    of them -> every picture, against the references of the tests above"""
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec
    k, R, which, B, _, geom = seam_case(oracle)
    g = R["geom"]
    P = K.seam_pictures(k, K.SEAM2_DISTINCT)[which]
    ctx = _lib.Context(0)
    try:
        s = spiht_amd.SpihtSettings(wavelet=k["wavelet"], quantization_scale=k["q"], mode=k["mode"])
        codec = BatchCodec(k["c"], k["H"], k["W"], s, k["level"], k["max_bits"], ctx=ctx)
        res = codec.encode_u16(P.astype(np.uint16) * 257)
        assert len(res) == B
        bad = [b for b, r in enumerate(res) if r.encoded_bytes != R["streams"][which[b]] or r.max_n != int(R["max_n"][which[b]])
               or (r.h, r.w, r.c, r.level) != (k["H"], k["W"], k["c"], k["level"])]
        assert not bad, "%d EncodingResults differ, first %s" % (len(bad), bad[:8])
        got = np.ascontiguousarray(codec.decode_float(res, dtype=np.float16))
        assert got.dtype == np.float16
        same_batch(got.view(np.uint16), px_want(R["pics"], "f16", k["H"], k["W"])[which], "decode_float(float16)")
        ih, iw = (k["H"] + 1) // 2, (k["W"] + 1) // 2  # the centred window of ceil(H / 2) x ceil(W / 2) in the 11 x 15 picture
        oy, ox = (g["hs"][1] - ih) // 2, (g["ws"][1] - iw) // 2
        want = np.ascontiguousarray(R["red"][1][:, :, oy:oy + ih, ox:ox + iw])
        same_batch(np.ascontiguousarray(codec.decode_reduced(res, 1, crop=True)), want[which], "decode_reduced(1, crop=True)")
    finally:
        ctx.close()


def test_batch_codec_through_the_seam(oracle):
    """BatchCodec.encode / .decode of the 21852 pictures: every EncodingResult and every picture"""
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec
    k, P, R = K.CHUNK, K.chunk_pictures(), K.chunk_reference(oracle)
    ctx = _lib.Context(0)
    try:
        s = spiht_amd.SpihtSettings(wavelet=k["wavelet"], quantization_scale=k["q"], mode=k["mode"])
        codec = BatchCodec(k["c"], k["H"], k["W"], s, k["level"], k["max_bits"], ctx=ctx)
        res = codec.encode(P / 255)
        assert len(res) == len(P)
        bad = [b for b, r in enumerate(res) if r.encoded_bytes != R["streams"][b] or r.max_n != int(R["max_n"][b])
               or (r.h, r.w, r.c, r.level) != (k["H"], k["W"], k["c"], k["level"])]
        assert not bad, "%d EncodingResults differ, first %s" % (len(bad), bad[:8])
        same_batch(codec.decode(res), R["pics"], "decoded pictures")
    finally:
        ctx.close()
