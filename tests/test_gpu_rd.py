"""Rate-distortion reductions, curve and cut on the GPU (include/spiht_hip.h: spiht_sqerr_i32, spiht_sse_f64 / _u8 / _u16;
spiht_amd/rd.py).  The integer sums are held to Python integers exactly; the float64 sum to the exact rational sum of its
float64 inputs within a bound derived from the number of roundings; the curve and the cuts to the CPU oracle's decode of
every prefix."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import synth_image

pytestmark = pytest.mark.gpu
vp = C.c_void_p
ERR_ARG = 6
GUARD = 0xA5A5A5A5A5A5A5A5


class Dev:
    """device buffers of one test on the default context, freed at the end"""

    def __enter__(self):
        from spiht_amd import _lib
        self.lib, self.ctx, self.L, self.held = _lib, _lib.default_context(), _lib.lib(), []
        return self

    def __exit__(self, *exc):
        self.ctx.synchronize()
        for p in self.held:
            self.ctx.free(p)

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.alloc(max(arr.nbytes, 4))
        self.held.append(p)
        self.ctx.upload(p, arr)
        return p

    def rows(self, fn, n_words, dtype=np.uint64):
        """run fn(pointer to n_words 8-byte results) between two guard words on either side -> the results"""
        buf = np.full(n_words + 4, GUARD, np.uint64)
        p = self.put(buf)
        status = fn(p + 16)
        self.ctx.synchronize()
        self.ctx.download(buf, p)
        assert status == 0, status
        assert (buf[:2] == GUARD).all() and (buf[-2:] == GUARD).all(), "written outside the result rows"
        return buf[2:-2].view(dtype)


def py_sqerr(X, Y):
    d = X.astype(np.int64).ravel() - Y.astype(np.int64).ravel()
    return sum(int(v) * int(v) for v in d)


def gpu_sqerr(X, Y):
    K, (c, h, w) = Y.shape[0], X.shape
    with Dev() as d:
        dx, dy = d.put(X.astype(np.int32)), d.put(Y.astype(np.int32))
        out = d.rows(lambda p: d.L.spiht_sqerr_i32(d.ctx.handle, vp(dx), vp(dy), K, c, h, w, vp(p)), 2 * K)
    return [int(out[2 * k]) | (int(out[2 * k + 1]) << 64) for k in range(K)]


# ---- 1. spiht_sqerr_i32 ---------------------------------------------------------------------------------------------------------
def test_sqerr_carries_into_the_high_word():
    X = np.full((1, 64, 64), 2 ** 30 - 1, np.int32)
    Y = np.full((1, 1, 64, 64), -(2 ** 31 - 1), np.int32)
    want = 4096 * (2 ** 30 - 1 + 2 ** 31 - 1) ** 2
    assert want >> 64 and want >> 75 == 1
    assert gpu_sqerr(X, Y) == [want]


def test_sqerr_single_largest_term():
    rng = np.random.default_rng(1)
    X = rng.integers(-2 ** 31, 2 ** 31, (3, 8, 8)).astype(np.int32)
    X[1, 3, 5] = -2 ** 31
    Y = np.stack([X, X])
    Y[1, 1, 3, 5] = 2 ** 31 - 1
    assert gpu_sqerr(X, Y) == [0, (2 ** 32 - 1) ** 2]


@pytest.mark.parametrize("K,shape", [(5, (3, 37, 53)), (2, (1, 130, 257))])
def test_sqerr_random_against_python_integers(K, shape):
    """odd sizes and a ragged last workgroup; 130 x 257: five workgroups per plane, planes that start off a 16-byte boundary"""
    rng = np.random.default_rng(K)
    X = rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32)
    Y = rng.integers(-2 ** 31, 2 ** 31, (K,) + shape).astype(np.int32)
    Y[0] = X
    want = [py_sqerr(X, Y[k]) for k in range(K)]
    assert want[0] == 0 and want[1] >> 64
    assert gpu_sqerr(X, Y) == want


def test_sqerr_argument_errors():
    with Dev() as d:
        p = d.put(np.zeros(64, np.int32))
        h = d.ctx.handle
        assert d.L.spiht_sqerr_i32(h, vp(p), vp(p), 0, 1, 4, 4, vp(p)) == ERR_ARG
        assert d.L.spiht_sqerr_i32(h, vp(p), vp(p), 65536, 1, 4, 4, vp(p)) == ERR_ARG
        for args in ((None, vp(p), 1, 1, 4, 4, vp(p)), (vp(p), None, 1, 1, 4, 4, vp(p)), (vp(p), vp(p), 1, 1, 4, 4, None)):
            assert d.L.spiht_sqerr_i32(h, *args) == ERR_ARG
        assert d.L.spiht_sqerr_i32(None, vp(p), vp(p), 1, 1, 4, 4, vp(p)) == ERR_ARG
        assert d.L.spiht_sqerr_i32(h, vp(p), vp(p), 1, 1, 0, 4, vp(p)) == ERR_ARG
        assert d.L.spiht_sqerr_i32(h, vp(p), vp(p), 1, 1, 2 ** 14, 2 ** 14, vp(p)) == d.lib.ERR_TOO_LARGE


# ---- 2. spiht_sse_u8 / _u16 -----------------------------------------------------------------------------------------------------
def _views(dtype, c, H, W, rng):
    """name -> (buffer, byte strides or None, the (c, H, W) view): what lies outside a view is random, never zero"""
    es = np.dtype(dtype).itemsize
    hi = np.iinfo(dtype).max + 1
    planar = rng.integers(0, hi, (c, H, W)).astype(dtype)
    hwc = rng.integers(0, hi, (H, W, c)).astype(dtype)
    rgba = rng.integers(1, hi, (H, W + 3, 4)).astype(dtype)
    return {"planar": (planar, None, planar),
            "planar_strides": (planar, (H * W * es, W * es, es), planar),
            "interleaved": (hwc, (es, W * c * es, c * es), hwc.transpose(2, 0, 1)),
            "rgba_padded": (rgba, (es, (W + 3) * 4 * es, 4 * es), rgba[:, :W, :3].transpose(2, 0, 1))}


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_sse_int_views_exact(dtype):
    c, H, W, K = 3, 37, 53, 4
    rng = np.random.default_rng(7)
    es = np.dtype(dtype).itemsize
    D = rng.integers(0, np.iinfo(dtype).max + 1, (K, c, H, W)).astype(dtype)
    D[1] = 0
    # the decoded pictures three samples into a buffer: off the 16-byte boundary the vector loads start at
    dbuf = np.concatenate([np.full(3, np.iinfo(dtype).max, dtype), D.ravel(), np.full(3, np.iinfo(dtype).max, dtype)])
    with Dev() as d:
        fn = d.L.spiht_sse_u16 if es == 2 else d.L.spiht_sse_u8
        dd = d.put(dbuf) + 3 * es
        for name, (buf, strides, view) in _views(dtype, c, H, W, rng).items():
            if name.startswith("planar"):
                view[0] = np.iinfo(dtype).max  # against D[1] = 0: the largest term everywhere in a plane
            st = None if strides is None else np.array(strides, np.int64)
            dp = d.put(buf)
            got = d.rows(lambda p: fn(d.ctx.handle, vp(dp), None if st is None else vp(st.ctypes.data), vp(dd), K, c, H, W,
                                      vp(p)), K * c).reshape(K, c)
            diff = view[None].astype(np.int64) - D.astype(np.int64)
            assert np.array_equal(got, (diff * diff).sum(axis=(2, 3)).astype(np.uint64)), name
        dp = d.put(np.zeros((c, H, W), dtype))
        out = d.put(np.zeros(K * c, np.uint64))
        if es == 2:  # an odd byte stride of 16-bit samples
            bad = np.array([H * W * es, W * es, es + 1], np.int64)
            assert fn(d.ctx.handle, vp(dp), vp(bad.ctypes.data), vp(dd), K, c, H, W, vp(out)) == ERR_ARG
        neg = np.array([H * W * es, -W * es, es], np.int64)
        assert fn(d.ctx.handle, vp(dp), vp(neg.ctypes.data), vp(dd), K, c, H, W, vp(out)) == ERR_ARG
        assert fn(d.ctx.handle, vp(dp), None, vp(dd), 0, c, H, W, vp(out)) == ERR_ARG
        assert fn(d.ctx.handle, None, None, vp(dd), K, c, H, W, vp(out)) == ERR_ARG


# ---- 3. spiht_sse_f64 -----------------------------------------------------------------------------------------------------------
def exact_sse(P, D):
    """sum (P - D)^2 of two float64 arrays of one shape as a Fraction: the inputs as integers over a common power of two"""
    def ints(a, emin):
        m, e = np.frexp(a.ravel())
        mi = np.ldexp(m, 53).astype(np.int64)
        return [int(v) << max(int(s), 0) for v, s in zip(mi, e - 53 - emin)]
    both = np.concatenate([P.ravel(), D.ravel()])
    nz = both[both != 0]
    emin = int(np.frexp(nz)[1].min()) - 53 if nz.size else 0
    total = sum((p - q) ** 2 for p, q in zip(ints(P, emin), ints(D, emin)))
    return Fraction(total) * Fraction(2) ** (2 * emin)


def within_bound(S, exact, n):
    """every term carries two roundings and the sum of n non-negative terms n - 1 more, in any order: to first order
    |S - exact| <= (n + 2) 2^-53 exact; a factor of two on top for the second-order terms"""
    return abs(Fraction(float(S)) - exact) <= Fraction(n + 3, 2 ** 52) * exact


def test_exact_sse_helper():
    P, D = np.array([0.1, 0.5, 0.0, 3.0]), np.array([0.3, 0.25, 1e-30, 3.0])
    want = sum((Fraction(float(p)) - Fraction(float(q))) ** 2 for p, q in zip(P, D))
    assert exact_sse(P, D) == want


def test_sse_f64_crop_bound_and_determinism():
    c, H, W, K, rh, rw = 3, 37, 53, 4, 38, 55
    rng = np.random.default_rng(11)
    P = synth_image(3001, c, H, W)
    D = np.full((K, c, rh, rw), 1e300)
    D[:, :, :H, :W] = P[None] + rng.standard_normal((K, c, H, W)) * np.array([1e-1, 1e-3, 1e-6, 0.0])[:, None, None, None]
    with Dev() as d:
        dp, dd = d.put(P), d.put(D)
        h = d.ctx.handle
        call = lambda ptr, k: d.rows(lambda p: d.L.spiht_sse_f64(h, vp(dp), vp(ptr), k, c, H, W, rh, rw, vp(p)), k * c, np.float64)
        S = call(dd, K).reshape(K, c)
        again = call(dd, K).reshape(K, c)
        ones = np.stack([call(dd + k * c * rh * rw * 8, 1) for k in range(K)])
        out = d.put(np.zeros(K * c))
        assert d.L.spiht_sse_f64(h, vp(dp), vp(dd), K, c, H, W, H - 1, rw, vp(out)) == ERR_ARG
        assert d.L.spiht_sse_f64(h, vp(dp), vp(dd), K, c, H, W, rh, W - 1, vp(out)) == ERR_ARG
        assert d.L.spiht_sse_f64(h, vp(dp), vp(dd), 0, c, H, W, rh, rw, vp(out)) == ERR_ARG
        # K * c beyond a grid's extent: refused before anything is queued
        assert d.L.spiht_sse_f64(h, vp(dp), vp(dd), 65535, 65535, 1, 1, 1, 1, vp(out)) == d.lib.ERR_TOO_LARGE
    assert np.isfinite(S).all(), "the rim shows up: the crop is wrong"
    assert S.tobytes() == again.tobytes(), "two calls, different bits"
    assert S.tobytes() == ones.tobytes(), "K = 4 in one call and four calls of K = 1 differ"
    assert (S[3] == 0).all()
    for k in range(K):
        for ch in range(c):
            assert within_bound(S[k, ch], exact_sse(P[ch], D[k, ch, :H, :W]), H * W), (k, ch)


# ---- 4. rd_curve ----------------------------------------------------------------------------------------------------------------
MAX_BITS = 2400  # streams of 300 bytes


def _settings(case):
    import spiht_amd
    if case == "b":
        return spiht_amd.SpihtSettings(wavelet="bior4.4", mode="symmetric"), 3
    if case == "c":
        return spiht_amd.SpihtSettings(quantization_scale=1, color_model="IPT", per_channel_quant_scales=[100, 20, 20]), None
    return spiht_amd.SpihtSettings(), None


def _lengths(n, seed):
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2] + [int(v) for v in rng.integers(3, n - 1, 5)] + [n - 1, n, n + 5]
    lens.append(lens[4])  # one twice
    return [lens[i] for i in rng.permutation(len(lens))]


def _prefix(r, k):
    import spiht_amd
    return spiht_amd.EncodingResult(r.encoded_bytes[:k], r.h, r.w, r.c, r.max_n, r.level)


def _oracle_coef_sqerr(oracle, X, r, s, lens):
    g = oracle.geometry(r.h, r.w, s.wavelet, r.level, s.mode)
    return [py_sqerr(X, oracle.decode(r.encoded_bytes[:k], r.max_n, r.c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"]))
            for k in lens]


def _same_curve(a, b):
    assert (a.byte_lengths, a.bits, a.coef_sqerr, a.bpp) == (b.byte_lengths, b.bits, b.coef_sqerr, b.bpp)
    assert np.asarray(a.sse).tobytes() == np.asarray(b.sse).tobytes()
    assert np.asarray(a.mse).tobytes() == np.asarray(b.mse).tobytes()
    assert np.asarray(a.psnr).tobytes() == np.asarray(b.psnr).tobytes()


def _non_increasing_in_length(lens, values):
    order = sorted(range(len(lens)), key=lambda i: lens[i])
    return all(values[a] >= values[b] for a, b in zip(order, order[1:]))


@pytest.mark.parametrize("case,shape,seed", [("a", (3, 37, 53), 4101), ("b", (1, 64, 64), 4102), ("c", (3, 40, 56), 4103)])
def test_rd_curve_float64(oracle, case, shape, seed):
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray
    s, level = _settings(case)
    c, H, W = shape
    img = synth_image(seed, c, H, W)
    r = spiht_amd.encode_image(img, s, level, MAX_BITS)
    n = len(r.encoded_bytes)
    assert n == MAX_BITS // 8
    codec = BatchCodec(c, H, W, s, level, MAX_BITS)
    full_before = spiht_amd.decode_image(r, s)
    lens = _lengths(n, seed)
    curve = codec.rd_curve(img, r, lens)
    assert curve.byte_lengths == lens and curve.bits == [8 * min(k, n) for k in lens]
    assert curve.bpp == [b / (H * W) for b in curve.bits]
    # the coefficient error, exactly
    if case == "c":  # the colour arithmetic is the library's own: X as the encoder hands it out
        d_img, d_x = DeviceArray(codec.ctx, img.shape, np.float64), DeviceArray(codec.ctx, (c, codec.geom["enc_h"], codec.geom["enc_w"]), np.int32)
        d_o, d_nb, d_mn = (DeviceArray(codec.ctx, (1, codec.slot_stride), np.uint8), DeviceArray(codec.ctx, (1,), np.uint64),
                           DeviceArray(codec.ctx, (1,), np.uint8))
        d_img.upload(img)
        codec.encode_device(d_img.ptr, 1, d_o.ptr, d_nb.ptr, d_mn.ptr, d_coeffs=d_x.ptr)
        codec.ctx.synchronize()
        X = d_x.download()
        for a in (d_img, d_x, d_o, d_nb, d_mn):
            a.free()
    else:
        arr, _ = oracle.wavedec2_array(img, s.wavelet, s.mode, level)
        X = oracle.quantize(arr, s.quantization_scale, s.per_channel_quant_scales)
    assert curve.coef_sqerr == _oracle_coef_sqerr(oracle, X, r, s, lens)
    assert all(type(e) is int for e in curve.coef_sqerr)
    assert _non_increasing_in_length(lens, curve.coef_sqerr)
    # the pixel error: the exact sum over decode_prefixes' pictures (held to the oracle in every bit elsewhere), within the bound
    pics = codec.decode_prefixes(r, lens)
    sse = np.asarray(curve.sse)
    assert sse.shape == (len(lens), c) and sse.dtype == np.float64
    for k in range(len(lens)):
        for ch in range(c):
            assert within_bound(sse[k, ch], exact_sse(img[ch], pics[k, ch, :H, :W]), H * W), (k, ch)
        total = float(sse[k, 0])
        for ch in range(1, c):
            total += float(sse[k, ch])
        assert curve.mse[k] == total / (c * H * W)
        assert curve.psnr[k] == (math.inf if curve.mse[k] == 0 else 10 * math.log10(1.0 / curve.mse[k]))
    assert curve.psnr[lens.index(n)] > curve.psnr[lens.index(0)]
    # one budget per group: the same bits in every field
    _same_curve(codec.rd_curve(img, r, lens, max_bytes=1), curve)
    # the context is as it was: an ordinary decode gives the oracle's picture
    after = spiht_amd.decode_image(r, s)
    assert after.tobytes() == full_before.tobytes()
    if case != "c":
        ref = oracle.decode_image(r.encoded_bytes, r.max_n, c, H, W, s.wavelet, level, s.quantization_scale,
                                  s.per_channel_quant_scales, mode=s.mode)
        assert np.array_equal(after, ref)


def test_rd_curve_encodes_first_and_default_grid(oracle):
    """result=None: the picture is encoded with the codec's settings; the default grid of lengths"""
    import spiht_amd
    from spiht_amd import rd
    img = synth_image(4101, 3, 37, 53)
    s = spiht_amd.SpihtSettings()
    data, max_n, g = oracle.encode_image(img, s.wavelet, s.mode, None, s.quantization_scale, None, MAX_BITS)
    n = len(data)
    curve = spiht_amd.rd_curve(img, s, points=7, max_bits=MAX_BITS)
    assert curve.byte_lengths == rd.default_lengths(n, 7) and curve.byte_lengths[-1] == n
    arr, _ = oracle.wavedec2_array(img, s.wavelet, s.mode, None)
    X = oracle.quantize(arr, s.quantization_scale)
    r = spiht_amd.EncodingResult(data, 37, 53, 3, max_n, None)
    assert curve.coef_sqerr == _oracle_coef_sqerr(oracle, X, r, s, curve.byte_lengths)
    _same_curve(spiht_amd.rd_curve(img, s, result=r, points=7, max_bits=MAX_BITS), curve)


@pytest.mark.parametrize("bits", [8, 16])
def test_rd_curve_integer_pixels(oracle, bits):
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    dtype, peak = (np.uint8, 255) if bits == 8 else (np.uint16, 65535)
    enc, dec = ((spiht_amd.encode_image_u8, spiht_amd.decode_image_u8) if bits == 8 else
                (spiht_amd.encode_image_u16, spiht_amd.decode_image_u16))
    c, H, W = 3, 37, 53
    img = np.round(synth_image(4104, c, H, W) * peak).astype(dtype)
    s = spiht_amd.SpihtSettings()
    r = enc(img, s, None, MAX_BITS)
    n = len(r.encoded_bytes)
    codec = BatchCodec(c, H, W, s, None, MAX_BITS)
    lens = _lengths(n, bits)
    curve = getattr(codec, "rd_curve_u%d" % bits)(img, r, lens)
    arr, _ = oracle.wavedec2_array(img / float(peak), s.wavelet, s.mode, None)
    X = oracle.quantize(arr, s.quantization_scale)
    assert curve.coef_sqerr == _oracle_coef_sqerr(oracle, X, r, s, lens)
    assert _non_increasing_in_length(lens, curve.coef_sqerr)
    want = []
    for k in lens:
        diff = img.astype(np.int64) - dec(_prefix(r, k), s).astype(np.int64)
        want.append([int(v) for v in (diff * diff).sum(axis=(1, 2))])
    assert curve.sse == want and all(type(v) is int for row in curve.sse for v in row)
    assert curve.mse == [sum(row) / (c * H * W) for row in want]
    assert curve.psnr == [math.inf if m == 0 else 10 * math.log10(float(peak) * float(peak) / m) for m in curve.mse]
    _same_curve(getattr(codec, "rd_curve_u%d" % bits)(img, r, lens, max_bytes=1), curve)
    ref = oracle.decode_image(r.encoded_bytes, r.max_n, c, H, W, s.wavelet, None, s.quantization_scale, None)
    assert np.array_equal(spiht_amd.decode_image(r, s), ref)


# ---- 5. cut_to_sqerr ------------------------------------------------------------------------------------------------------------
def test_cut_to_sqerr_against_every_prefix(oracle):
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    c, H, W = 3, 37, 53
    img = synth_image(4101, c, H, W)
    s = spiht_amd.SpihtSettings()
    r = spiht_amd.encode_image(img, s, None, 3200)
    n = len(r.encoded_bytes)
    assert n <= 400
    arr, _ = oracle.wavedec2_array(img, s.wavelet, s.mode, None)
    X = oracle.quantize(arr, s.quantization_scale)
    E = _oracle_coef_sqerr(oracle, X, r, s, range(n + 1))
    codec = BatchCodec(c, H, W, s, None)
    for j in range(1, 6):
        target = E[n * j // 6]
        cut, value, met = codec.cut_to_sqerr(img, r, target)
        L = len(cut.encoded_bytes)
        assert met and cut.encoded_bytes == r.encoded_bytes[:L] and value == E[L] <= target
        assert L == min(k for k in range(n + 1) if E[k] <= target), (j, target, L)
    # target 0 on the unlimited stream: the whole stream comes back
    full = spiht_amd.encode_image(img, s)
    nf = len(full.encoded_bytes)
    e_full = _oracle_coef_sqerr(oracle, X, full, s, [nf, nf - 1])
    cut, value, met = codec.cut_to_sqerr(img, full, 0)
    assert cut.encoded_bytes == full.encoded_bytes and value == e_full[0] and met == (e_full[0] == 0)
    assert e_full[1] > 0


# ---- 6. cut_to_psnr -------------------------------------------------------------------------------------------------------------
def test_cut_to_psnr_u8_contract(oracle):
    import spiht_amd
    c, H, W = 3, 37, 53
    img = np.round(synth_image(4104, c, H, W) * 255).astype(np.uint8)
    s = spiht_amd.SpihtSettings()
    r = spiht_amd.encode_image_u8(img, s, None, 8 * 1500)

    def psnr(k):
        diff = img.astype(np.int64) - spiht_amd.decode_image_u8(_prefix(r, k), s).astype(np.int64)
        total = int((diff * diff).sum())
        return math.inf if total == 0 else 10 * math.log10(255.0 * 255.0 / (total / (c * H * W)))
    whole = psnr(len(r.encoded_bytes))
    for target in (psnr(40) + 0.5, (psnr(0) + whole) / 2, whole):
        cut, value, met = spiht_amd.cut_to_psnr_u8(img, r, target, s, points=5)
        L = len(cut.encoded_bytes)
        assert met and cut.encoded_bytes == r.encoded_bytes[:L]
        assert value == psnr(L) >= target and (L == 0 or psnr(L - 1) < target), (target, L)
        assert spiht_amd.decode_image_u8(cut, s).shape == (c, H, W)
    cut, value, met = spiht_amd.cut_to_psnr_u8(img, r, whole + 0.01, s)
    assert not met and cut == r and value == whole
    cut, value, met = spiht_amd.cut_to_psnr_u8(img, r, -math.inf, s)
    assert met and cut.encoded_bytes == b""


def test_cut_to_psnr_float64_contract(oracle):
    import spiht_amd
    c, H, W = 3, 37, 53
    img = synth_image(4101, c, H, W)
    s = spiht_amd.SpihtSettings()
    r = spiht_amd.encode_image(img, s, None, 8 * 1500)
    eps = 1e-9

    def psnr(k):
        pic = spiht_amd.decode_image(_prefix(r, k), s)[:, :H, :W]
        total = sum(exact_sse(img[ch], pic[ch]) for ch in range(c))
        return 10 * math.log10(1.0 / float(total / (c * H * W)))
    whole = psnr(len(r.encoded_bytes))
    for target in (psnr(40) + 0.5, (psnr(0) + whole) / 2):
        cut, value, met = spiht_amd.cut_to_psnr(img, r, target, s)
        L = len(cut.encoded_bytes)
        assert met and cut.encoded_bytes == r.encoded_bytes[:L] and abs(value - psnr(L)) < eps
        assert psnr(L) >= target - eps and (L == 0 or psnr(L - 1) < target + eps), (target, L)
        # the cut decodes with the plain call, to the oracle's picture of that prefix
        ref = oracle.decode_image(cut.encoded_bytes, cut.max_n, c, H, W, s.wavelet, None, s.quantization_scale, None)
        assert np.array_equal(spiht_amd.decode_image(cut, s), ref)
    cut, value, met = spiht_amd.cut_to_psnr(img, r, whole + 1.0, s)
    assert not met and cut == r and abs(value - whole) < eps


# ---- 7. the command line --------------------------------------------------------------------------------------------------------
def test_cli_rd_curve_and_psnr(tmp_path, capsys):
    pytest.importorskip("PIL")
    from spiht_amd import utils
    from spiht_amd.encode_decode import build_parser, main
    img = np.round(synth_image(77, 3, 48, 64) * 255) / 255
    utils.imsave(tmp_path / "in.png", img)
    common = [str(tmp_path / "in.png"), "--bpp", "2.0", "--color_model", "RGB", "--per_channel_quant_scales", "1., 1., 1.",
              "--out", str(tmp_path / "out.png")]
    enc, _ = main(build_parser().parse_args(common + ["--rd-curve", "5"]))
    text = capsys.readouterr().out
    rows = [ln.split() for ln in text.splitlines() if len(ln.split()) == 3 and ln.split()[0].isdigit()]
    assert len(rows) == 5 and int(rows[-1][0]) == len(enc.encoded_bytes) == 2 * 48 * 64 // 8
    cut, dec = main(build_parser().parse_args(common + ["--psnr", "15", "--save", str(tmp_path / "cut.spiht")]))
    text = capsys.readouterr().out
    assert "cut to 15.00 dB" in text and ("%d bytes" % len(cut.encoded_bytes)) in text
    assert 0 < len(cut.encoded_bytes) < len(enc.encoded_bytes) and cut.encoded_bytes == enc.encoded_bytes[:len(cut.encoded_bytes)]
    assert utils.load_encoding(tmp_path / "cut.spiht") == cut
    mse = float(((utils.imload(tmp_path / "in.png") - dec) ** 2).mean())
    assert 10 * math.log10(1.0 / mse) >= 15 - 1e-6
    # a loaded stream brings its own level: the curve is taken with it, not with the command line's default (2 here)
    saved, _ = main(build_parser().parse_args(common + ["--level", "1", "--save", str(tmp_path / "l1.spiht")]))
    capsys.readouterr()
    loaded, _ = main(build_parser().parse_args(common + ["--load", str(tmp_path / "l1.spiht"), "--rd-curve", "3"]))
    assert loaded == saved and saved.level == 1 and "rate-distortion curve, 3 prefixes" in capsys.readouterr().out
