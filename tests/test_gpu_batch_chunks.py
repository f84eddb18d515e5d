"""Both sides of the 65535-plane seam: batch_chunks (api.cpp) cuts every batched call into launches of at most 65535 planes,
and before this module no test passed more, so no launch had b0 != 0, none had exactly 65535 planes in grid.y.  Here every
chunked entry point runs once through the seam -- 21852 distinct pictures of 3 planes: 65535 planes in the first launch, 21
in the second -- and the raw coder calls also with one plane per picture, where the chunk is 65535 pictures.  Every image of
every batch is compared with the CPU oracle (cases and references: tests/call_sequence_cases.py, held to their purpose by
tests/test_call_sequence_cases.py; the oracle's pass over the 21852 pictures is host time, 1.4 to 5.6 s by the host, spent
once inside whichever test asks first -- the GPU side of an item is some hundredths of a second); every output lies between guard regions that must survive; slot tails past a stream
must be zero.  Each case runs on a context of its own."""
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


# ------------------------------------------------------------------------------------------------ the Python level

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
