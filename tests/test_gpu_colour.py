"""The colour kernel -- k_color3 (csrc/dwt_plain.hip) over color3_px and csrc/spow.h, the reference of every other colour test --
held to the host build of the same header in every bit: the power function alone (identity matrices), the whole pixel with the
real matrices, the kernel's own addressing, and the routes that carry the colour model change, at inputs outside [0, 1].  Every
comparison is equality of bits (a NaN for a NaN); the only bounds are the ulp bounds of tests/test_colour_cases.py, which hold the
host build to 60-digit arithmetic.  Cases: tests/colour_cases.py."""
import ctypes as C

import numpy as np
import pytest

import colour_cases as K

pytestmark = pytest.mark.gpu
vp = C.c_void_p
SENTINEL = 0x7F
GUARD = 64   # bytes in front of and behind an out-of-place result


def color3_call(ctx, d_in, d_out, B, npix, A, M, p):
    from spiht_amd import _lib
    A, M = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(M, np.float64)
    return _lib.lib().spiht_color3_batch_f64(ctx.handle, vp(d_in), vp(d_out), int(B), int(npix), vp(A.ctypes.data), vp(M.ctypes.data),
                                             float(p))


def device_color3(u, A, M, p):
    """u [B, 3, n] through k_color3, in place"""
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    ctx = _lib.default_context()
    u = np.ascontiguousarray(u, np.float64)
    d = DeviceArray(ctx, u.shape, np.float64)
    try:
        d.upload(u)
        _lib.check(color3_call(ctx, d.ptr, d.ptr, u.shape[0], u.shape[2], A, M, p))
        ctx.synchronize()
        return d.download()
    finally:
        d.free()


@pytest.mark.parametrize("p", K.DEVICE_EXPONENTS, ids=lambda p: "%.4g" % p)
def test_power_function_alone(p):
    """A = M = identity: the kernel computes spow_signed(u_r, p) per channel -- (u0 * 1 + u1 * 0) + u2 * 0 is u0 apart from the sign
    of a zero, which the rule carries the same way.  power_inputs() and its negation over the three channels; inputs whose
    result is not finite fill all three channels of their pixel (0 * inf in the matrix step would make NaNs of their neighbours),
    as do NaN and the infinities."""
    spow = K.host_spow()
    x = K.power_inputs()
    x = np.concatenate([x, -x, [0.0, -0.0]])
    finite = np.isfinite(spow(x, p))
    fin = x[finite]
    fin = np.concatenate([fin, fin[:(-len(fin)) % 3]]).reshape(3, -1)
    rest = np.concatenate([x[~finite], [np.nan, np.inf, -np.inf]])
    u = np.concatenate([fin, np.tile(rest, (3, 1))], axis=1)[None]
    assert np.isfinite(fin).all() and len(rest) >= 3 and u.shape[2] > 4096
    want = K.color3_rule(u, K.IDENTITY, K.IDENTITY, p, spow)
    n = fin.shape[1]
    assert np.array_equal(np.abs(want[0, :, :n]), np.abs(spow(fin, p)))   # the identity matrices do leave the power function alone
    got = device_color3(u, K.IDENTITY, K.IDENTITY, p)
    K.assert_same_bits(got, want, "spow(x, %.17g) on the device against the host build of csrc/spow.h" % p)


@pytest.mark.parametrize("pair", ["iec", "lindbloom"])
def test_whole_pixel(pair):
    """pixel_inputs() through RGB -> IPT and the triples of the way back through IPT -> RGB, with the matrices of
    color_models._params for both selectable RGB / XYZ pairs: color3_rule with the host build of the power function, in every bit"""
    from spiht_amd import color_models
    spow = K.host_spow()
    prev = color_models.set_rgb_xyz(pair)
    try:
        for src, dst, sets in (("RGB", "IPT", K.pixel_inputs()), ("IPT", "RGB", K.back_inputs(spow))):
            A, M, p = color_models._params(src, dst)
            u = np.concatenate(list(sets.values()), axis=1)[None]
            assert np.isfinite(u).all() and u.shape[2] > 8000
            got = device_color3(u, A, M, p)
            want = K.color3_rule(u, A, M, p, spow)
            at = np.cumsum([0] + [v.shape[1] for v in sets.values()])
            for k, name in enumerate(sets):
                K.assert_same_bits(got[..., at[k]:at[k + 1]], want[..., at[k]:at[k + 1]], "%s -> %s (%s), set %s" % (src, dst, pair, name))
    finally:
        color_models.set_rgb_xyz(prev)


def addressing_pixels(B, npix):
    px = K.pixel_inputs()
    pool = np.concatenate([px[k] for k in ("uniform", "negative", "above_one", "zero_one", "tiny")], axis=1)
    idx = (np.arange(B * npix) * 7 + 3) % pool.shape[1]
    return np.ascontiguousarray(pool[:, idx].reshape(3, B, npix).transpose(1, 0, 2))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("npix", K.NPIX)
def test_addressing(npix, B):
    """spiht_launch_color3's grid, ceil(npix / 1024) blocks of 256 threads by B: out of place into a block [B, 3, npix] between
    64 guard bytes -- the block is the rule, the guards keep the sentinel, the source is unchanged -- and in place the same bits"""
    from spiht_amd import _lib, color_models
    from spiht_amd.batch import DeviceArray
    ctx = _lib.default_context()
    A, M, p = color_models._params("RGB", "IPT")
    u = addressing_pixels(B, npix)
    want = K.color3_rule(u, A, M, p, K.host_spow())
    d_in, d_out = DeviceArray(ctx, u.shape, np.float64), DeviceArray(ctx, (u.nbytes + 2 * GUARD,), np.uint8)
    try:
        d_in.upload(u)
        ctx.memset(d_out.ptr, SENTINEL, d_out.nbytes)
        _lib.check(color3_call(ctx, d_in.ptr, d_out.ptr + GUARD, B, npix, A, M, p))
        ctx.synchronize()
        raw = d_out.download()
        assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), "a guard byte was written"
        K.assert_same_bits(raw[GUARD:-GUARD].view(np.float64).reshape(u.shape), want, "out of place, npix %d, B %d" % (npix, B))
        assert np.array_equal(K.bits(d_in.download()), K.bits(u)), "the source was written"
        _lib.check(color3_call(ctx, d_in.ptr, d_in.ptr, B, npix, A, M, p))
        ctx.synchronize()
        K.assert_same_bits(d_in.download(), want, "in place, npix %d, B %d" % (npix, B))
    finally:
        d_in.free()
        d_out.free()


def test_refusals():
    """npix = 0, B = 65536 and null pointers are SPIHT_ERR_ARG, and nothing is written"""
    from spiht_amd import _lib, color_models
    from spiht_amd.batch import DeviceArray
    ctx = _lib.default_context()
    A, M, p = color_models._params("RGB", "IPT")
    u = addressing_pixels(1, 256)
    d_in, d_out = DeviceArray(ctx, u.shape, np.float64), DeviceArray(ctx, u.shape, np.float64)
    try:
        d_in.upload(u)
        ctx.memset(d_out.ptr, SENTINEL, d_out.nbytes)
        good = (ctx, d_in.ptr, d_out.ptr, 1, 256, A, M, p)
        for at, bad in ((4, 0), (4, -1), (3, 65536), (3, -1), (1, None), (2, None)):
            args = list(good)
            args[at] = bad
            with pytest.raises(ValueError):
                _lib.check(color3_call(*args))
        L = _lib.lib()
        for a, m in ((None, M), (A, None)):
            with pytest.raises(ValueError):
                _lib.check(L.spiht_color3_batch_f64(ctx.handle, vp(d_in.ptr), vp(d_out.ptr), 1, 256, vp(a.ctypes.data) if a is not None else None,
                                                    vp(m.ctypes.data) if m is not None else None, p))
        with pytest.raises(ValueError):
            _lib.check(L.spiht_color3_batch_f64(None, vp(d_in.ptr), vp(d_out.ptr), 1, 256, vp(A.ctypes.data), vp(M.ctypes.data), p))
        ctx.synchronize()
        assert (d_out.download().view(np.uint8) == SENTINEL).all() and np.array_equal(K.bits(d_in.download()), K.bits(u))
        _lib.check(color3_call(ctx, d_in.ptr, d_out.ptr, 0, 256, A, M, p))   # no picture: nothing to do, no error
        ctx.synchronize()
        assert (d_out.download().view(np.uint8) == SENTINEL).all()
    finally:
        d_in.free()
        d_out.free()


# ---- the routes that carry the colour model change, at inputs outside [0, 1] -----------------------------------------------------

def convert_on_device(ctx, a, src, dst):
    """[B, 3, h, w] through color_models.device_convert (k_color3 as a pass of its own, in place)"""
    from spiht_amd import color_models
    from spiht_amd.batch import DeviceArray
    d = DeviceArray(ctx, a.shape, np.float64)
    try:
        d.upload(a)
        color_models.device_convert(ctx, d.ptr, a.shape[0], a.shape[2] * a.shape[3], src, dst)
        ctx.synchronize()
        return d.download()
    finally:
        d.free()


@pytest.mark.parametrize("mode,level", [("reflect", 1), ("reflect", 2), ("periodization", 2)])
@pytest.mark.parametrize("which", [0, 1], ids=["33x47", "67x131"])
def test_routes_fused_equals_separate_pass(which, mode, level):
    """The form of test_gpu_image.py::test_fused_colour_equals_separate_colour_pass -- streams, start planes and decoded pictures
    of the call with a colour model against the colour change as a pass of its own around the plain call, bit for bit -- on
    route_pictures(): negative values, values above 1, magnitudes of 1e-300 and zero patches go in, and the decoded IPT pictures of
    these budgets hand the way back LMS values of either sign.  bior2.2 / reflect at one and two levels: the colour change inside
    the tiled level 1, both ways.  periodization: api_dwt.cpp's `color && twopass` branch, the pass of its own (out of place into
    ctx->img) in front of the two-pass level, and in place behind the two-pass inverse level 1."""
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec
    pic = K.route_pictures()[which]
    imgs = np.stack([pic, pic[::-1, ::-1, :].copy()])
    H, W = pic.shape[1:]
    spow = K.host_spow()
    ctx = _lib.default_context()
    for mb in (H * W // 2, 6 * H * W):
        kw = dict(wavelet="bior2.2", mode=mode, quantization_scale=50.0)
        fused = BatchCodec(3, H, W, spiht_amd.SpihtSettings(color_model="IPT", **kw), level, mb, ctx=ctx)
        plain = BatchCodec(3, H, W, spiht_amd.SpihtSettings(**kw), level, mb, ctx=ctx)
        ipt = convert_on_device(ctx, imgs, "RGB", "IPT")
        from spiht_amd import color_models
        K.assert_same_bits(ipt, K.color3_rule(imgs.reshape(2, 3, -1), *color_models._params("RGB", "IPT"), spow).reshape(imgs.shape),
                           "the pass of its own")
        res_f, res_p = fused.encode(imgs), plain.encode(ipt)
        for b in range(2):
            assert res_f[b].max_n == res_p[b].max_n and res_f[b].encoded_bytes == res_p[b].encoded_bytes, (mode, level, mb, b)
        dec_p = plain.decode(res_p)
        back = convert_on_device(ctx, dec_p, "IPT", "RGB")
        K.assert_same_bits(fused.decode(res_f), back, "decoded pictures, %s level %d, %d bits" % (mode, level, mb))
        lms = np.einsum("rk,bkn->brn", color_models._params("IPT", "RGB")[0], dec_p.reshape(2, 3, -1))
        assert (lms < 0).any() and (lms > 0).any()


def test_route_no_transform_level():
    """The `ig.L == 0` branch of both directions in api_dwt.cpp: k_color3 out of place into ctx->a0 in front of the plain quantiser,
    and in place behind the plain dequantiser.  (The image calls refuse level 0 -- the root block's offspring fall outside the
    array -- so: spiht_dwt_quant_batch_f64 / spiht_dequant_idwt_batch_f64 inside color_models.fused.)  A (9, 13) picture; the
    call with the colour model equals the call without it on the rule's pixels, and the rule on the plain call's pixels."""
    import spiht_amd
    from spiht_amd import _lib, color_models
    from spiht_amd.batch import DeviceArray
    from spiht_amd.spiht_wrapper import _geometry, _wavelet_mode_ids
    ctx, L, spow = _lib.default_context(), _lib.lib(), K.host_spow()
    wid, mid = _wavelet_mode_ids(spiht_amd.SpihtSettings())
    B, H, W, q = 2, 9, 13, 1000.0
    g = _geometry(H, W, wid, 0, mid)
    assert (g["level"], g["enc_h"], g["enc_w"]) == (0, H, W)
    big = K.route_pictures()[0]
    imgs = np.stack([big[:, :H, :W], big[:, 20:20 + H, 30:30 + W]])
    assert (imgs < 0).any() and (imgs > 1).any() and (imgs == 0).any()
    ipt = K.color3_rule(imgs.reshape(B, 3, -1), *color_models._params("RGB", "IPT"), spow).reshape(imgs.shape)
    d_img, d_co = DeviceArray(ctx, imgs.shape, np.float64), DeviceArray(ctx, imgs.shape, np.int32)
    try:
        coeffs = {}
        for name, src, model in (("fused", imgs, "IPT"), ("plain", ipt, None)):
            d_img.upload(src)
            ctx.memset(d_co.ptr, SENTINEL, d_co.nbytes)
            with color_models.fused(ctx, model):
                _lib.check(L.spiht_dwt_quant_batch_f64(ctx.handle, vp(d_img.ptr), B, 3, H, W, wid, mid, 0, q, None, vp(d_co.ptr)))
            ctx.synchronize()
            coeffs[name] = d_co.download()
            assert np.array_equal(K.bits(d_img.download()), K.bits(src)), "the pictures were written"
        assert np.array_equal(coeffs["fused"], coeffs["plain"])
        assert len(np.unique(coeffs["fused"])) > 100
        # the way back from coefficients of a coarser quantiser's size: LMS values of either sign
        co = (coeffs["fused"] // 64) * 64
        d_co.upload(co)
        pics = {}
        for name, model in (("fused", "IPT"), ("plain", None)):
            ctx.memset(d_img.ptr, SENTINEL, d_img.nbytes)
            with color_models.fused(ctx, model):
                _lib.check(L.spiht_dequant_idwt_batch_f64(ctx.handle, vp(d_co.ptr), B, 3, H, W, wid, mid, 0, q, None, vp(d_img.ptr)))
            ctx.synchronize()
            pics[name] = d_img.download()
        assert np.array_equal(pics["plain"], co / q)
        A, M, p = color_models._params("IPT", "RGB")
        lms = np.einsum("rk,bkn->brn", A, pics["plain"].reshape(B, 3, -1))
        assert (lms < 0).sum() > 10 and (lms > 0).sum() > 10
        K.assert_same_bits(pics["fused"], K.color3_rule(pics["plain"].reshape(B, 3, -1), A, M, p, spow).reshape(imgs.shape), "level 0, the way back")
    finally:
        d_img.free()
        d_co.free()


@pytest.mark.parametrize("kind", ["float32", "float16"])
def test_route_float_pixels_in(kind):
    """encode_image_float with color_model="IPT" on route_pictures() as float32, and as float16 with float16 subnormals among the
    samples: nothing clipped, subnormals kept -- the float64 call on floatpx.to_float64 of the same picture, field by field"""
    import spiht_amd
    from spiht_amd import floatpx
    from test_gpu_u8 import same_result
    s = spiht_amd.SpihtSettings(color_model="IPT")
    for pic in K.route_pictures():
        P = pic.astype(np.float32) if kind == "float32" else pic.astype(np.float16)
        if kind == "float16":   # the 1e-300 magnitudes round to zero in float16: subnormal bit patterns of either sign in their place
            tiny = (pic != 0) & (np.abs(pic) < 1e-299)
            pat = (np.arange(int(tiny.sum())) * 37 % 1023 + 1).astype(np.uint16) | (np.arange(int(tiny.sum())) % 2 << 15).astype(np.uint16)
            P[tiny] = pat.view(np.float16)
            assert ((P != 0) & (np.abs(P.astype(np.float64)) < 2.0 ** -14)).sum() >= tiny.sum() > 100
        wide = floatpx.to_float64(P, kind)
        assert (wide < 0).any() and (wide > 1).any() and np.array_equal(wide, P.astype(np.float64))
        for level, mb in ((2, pic[0].size // 2), (None, 6 * pic[0].size)):
            same_result(spiht_amd.encode_image_float(P, s, level, mb), spiht_amd.encode_image(wide, s, level, mb))
