"""The 8-bit pixel path on the GPU: uint8 pictures in and out, converted inside level 1 of the transforms (or by a pass of
their own on the routes whose level 1 has no 8-bit form), held bit for bit to the float64 path and to the CPU oracle:
  encode_image_u8(P)  == encode_image(P / 255.0)                                   (every field)
  decode_image_u8(r)  == (np.clip(decode_image(r), 0, 1) * 255.0).astype(np.uint8)[:, :h, :w]"""
import numpy as np
import pytest

from conftest import synth_image

pytestmark = pytest.mark.gpu


def u8_image(seed, c, H, W):
    return np.round(synth_image(seed, c, H, W) * 255).astype(np.uint8)


def to_u8(dec, h, w):
    """the contract's formula: clip, scale, truncate, crop"""
    return (np.clip(dec, 0.0, 1.0) * 255.0).astype(np.uint8)[:, :h, :w]


def settings(cfg):
    import spiht_amd
    return spiht_amd.SpihtSettings(wavelet=cfg.get("wavelet", "bior2.2"), quantization_scale=cfg.get("q", 50.0),
                                   mode=cfg.get("mode", "reflect"), color_model=cfg.get("color"),
                                   per_channel_quant_scales=cfg.get("mults"))


def same_result(a, b):
    assert (a.encoded_bytes, a.h, a.w, a.c, a.max_n, a.level, a._encoding_version) == \
        (b.encoded_bytes, b.h, b.w, b.c, b.max_n, b.level, b._encoding_version)


# the configurations of tests/test_gpu_image.py::test_encode_image_decode_image_vs_oracle
CONFIGS = [
    dict(c=1, H=32, W=32, level=2, max_bits=None),
    dict(c=3, H=48, W=64, level=None, max_bits=3000),
    dict(c=3, H=37, W=53, level=2, max_bits=12345),
    dict(c=3, H=64, W=96, level=3, max_bits=4000, q=1.0, mults=[100.0, 20.0, 20.0]),
    dict(c=1, H=96, W=128, level=None, max_bits=9999, wavelet="bior4.4", mode="symmetric"),
    dict(c=2, H=45, W=70, level=2, max_bits=None, wavelet="bior4.4", mode="symmetric", q=255.0, mults=[1.0, 0.2]),
    dict(c=1, H=160, W=144, level=None, max_bits=20001, wavelet="bior6.8"),
    dict(c=1, H=40, W=56, level=3, max_bits=777, wavelet="haar"),
]


@pytest.mark.parametrize("cfg", CONFIGS)
def test_encode_decode_u8_vs_float64_and_oracle(oracle, cfg):
    import spiht_amd
    c, H, W = cfg["c"], cfg["H"], cfg["W"]
    P = u8_image(2000 + H, c, H, W)
    s = settings(cfg)
    ref = spiht_amd.encode_image(P / 255, s, level=cfg["level"], max_bits=cfg["max_bits"])
    ob, on, _ = oracle.encode_image(P / 255, s.wavelet, s.mode, cfg["level"], s.quantization_scale,
                                    s.per_channel_quant_scales, cfg["max_bits"])
    assert ref.encoded_bytes == ob and ref.max_n == on
    views = {"chw": P, "hwc": np.ascontiguousarray(P.transpose(1, 2, 0)).transpose(2, 0, 1)}
    if c == 3:
        rgba = np.full((H, W, 4), 77, np.uint8)
        rgba[..., :3] = P.transpose(1, 2, 0)
        views["rgba"] = rgba[..., :3].transpose(2, 0, 1)
    for name, v in views.items():
        enc = spiht_amd.encode_image_u8(v, s, level=cfg["level"], max_bits=cfg["max_bits"])
        same_result(enc, ref)
    enc = spiht_amd.encode_image_u8(P.transpose(1, 2, 0), s, level=cfg["level"], max_bits=cfg["max_bits"], channels_last=True)
    same_result(enc, ref)
    # decode
    dec = spiht_amd.decode_image_u8(ref, s)
    assert dec.dtype == np.uint8 and dec.shape == (c, H, W)
    assert np.array_equal(dec, to_u8(spiht_amd.decode_image(ref, s), H, W))
    odec = oracle.decode_image(ob, on, c, H, W, s.wavelet, cfg["level"], s.quantization_scale, s.per_channel_quant_scales)
    assert np.array_equal(dec, to_u8(odec, H, W))
    hwc = spiht_amd.decode_image_u8(ref, s, channels_last=True)
    assert hwc.shape == (H, W, c) and np.array_equal(hwc, dec.transpose(1, 2, 0))


def test_decode_u8_saturated_odd_sizes(oracle):
    """blocks of 0 and 255 at a high quantisation scale: decoded values overshoot [0, 1] on both sides (the clip), odd
    sizes (the crop of the extra row and column)"""
    import spiht_amd
    c, H, W = 3, 41, 67
    P = np.zeros((c, H, W), np.uint8)
    P[:, ::2, :] = 255
    P[1, :, 10:30] = 255
    P[2, 20:, :] = 0
    s = spiht_amd.SpihtSettings(quantization_scale=1000.0)
    enc = spiht_amd.encode_image_u8(P, s, level=3)
    same_result(enc, spiht_amd.encode_image(P / 255, s, level=3))
    f = spiht_amd.decode_image(enc, s)
    assert f.shape == (c, H + 1, W + 1) and f.min() < 0.0 and f.max() > 1.0
    dec = spiht_amd.decode_image_u8(enc, s)
    assert dec.shape == (c, H, W) and np.array_equal(dec, to_u8(f, H, W))
    odec = oracle.decode_image(enc.encoded_bytes, enc.max_n, c, H, W, "bior2.2", 3, 1000.0, None)
    assert np.array_equal(dec, to_u8(odec, H, W))


@pytest.mark.parametrize("cfg", [
    dict(color="IPT", q=1.0, mults=[50.0, 15.0, 15.0], level=3),       # colour change fused into level 1
    dict(color="IPT", mode="periodization", level=2),                    # ... in front of / behind a two-pass level
    dict(mode="smooth", level=2),
    dict(mode="antireflect", level=3),
    dict(wavelet="db11", level=2),                                       # a filter longer than the tiled kernels take
])
def test_u8_routes_vs_float64(cfg):
    import spiht_amd
    c, H, W = 3, 57, 83
    P = u8_image(31, c, H, W)
    s = settings(cfg)
    enc = spiht_amd.encode_image_u8(P, s, level=cfg["level"], max_bits=6000)
    ref = spiht_amd.encode_image(P / 255, s, level=cfg["level"], max_bits=6000)
    same_result(enc, ref)
    hwc = np.ascontiguousarray(P.transpose(1, 2, 0))
    same_result(spiht_amd.encode_image_u8(hwc, s, level=cfg["level"], max_bits=6000, channels_last=True), ref)
    dec = spiht_amd.decode_image_u8(enc, s)
    assert np.array_equal(dec, to_u8(spiht_amd.decode_image(ref, s), H, W))
    assert np.array_equal(spiht_amd.decode_image_u8(enc, s, channels_last=True), dec.transpose(1, 2, 0))


@pytest.mark.parametrize("color", [None, "IPT"])
def test_u8_level0_fails_as_float64(color):
    """level 0: the root block is the whole array and its offspring fall outside it -- the float64 path refuses such a
    geometry (the reference panics), and so does the 8-bit one, with the same exception"""
    import spiht_amd
    from spiht_amd import _lib
    P = u8_image(32, 3, 48, 64)
    s = settings(dict(color=color))
    with pytest.raises(_lib.PanicException):
        spiht_amd.encode_image(P / 255, s, level=0, max_bits=6000)
    with pytest.raises(_lib.PanicException):
        spiht_amd.encode_image_u8(P, s, level=0, max_bits=6000)


def test_encode_image_keeps_treating_uint8_as_values():
    """encode_image(uint8) still transforms the values 0..255 (PyWavelets' dtype rule): the new path is opt-in"""
    import spiht_amd
    P = u8_image(5, 3, 40, 48)
    s = spiht_amd.SpihtSettings()
    a = spiht_amd.encode_image(P, s, level=2, max_bits=4000)
    same_result(a, spiht_amd.encode_image(P.astype(np.float64), s, level=2, max_bits=4000))
    assert a.encoded_bytes != spiht_amd.encode_image_u8(P, s, level=2, max_bits=4000).encoded_bytes


def test_batch_u8_equals_single_calls():
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    B, c, H, W = 7, 3, 45, 61
    P = np.stack([u8_image(100 + b, c, H, W) for b in range(B)])
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=3, max_bits=5000)
    res = codec.encode_u8(P)
    singles = [spiht_amd.encode_image_u8(P[b], s, level=3, max_bits=5000) for b in range(B)]
    for r, q in zip(res, singles):
        same_result(r, q)
    for r, q in zip(codec.encode_u8(P.transpose(0, 2, 3, 1), channels_last=True), singles):
        same_result(r, q)
    dec = codec.decode_u8(res)
    assert dec.shape == (B, c, H, W)
    for b in range(B):
        assert np.array_equal(dec[b], spiht_amd.decode_image_u8(singles[b], s))
    assert np.array_equal(codec.decode_u8(res, channels_last=True), dec.transpose(0, 2, 3, 1))
    # pixel_dtype float32 does not change what 8-bit pixels go through
    c32 = BatchCodec(c, H, W, s, level=3, max_bits=5000, pixel_dtype=np.float32)
    for r, q in zip(c32.encode_u8(P), singles):
        same_result(r, q)


def test_decode_device_u8_into_rgba_keeps_alpha_and_padding():
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray
    B, c, H, W = 3, 3, 37, 50
    pitch = 4 * W + 12
    P = np.stack([u8_image(200 + b, c, H, W) for b in range(B)])
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=2, max_bits=4000)
    ctx = codec.ctx
    res = codec.encode_u8(P)
    want = codec.decode_u8(res)
    data = np.zeros((B, codec.slot_stride), np.uint8)
    for b, r in enumerate(res):
        data[b, :len(r.encoded_bytes)] = np.frombuffer(r.encoded_bytes, np.uint8)
    d_data = DeviceArray(ctx, data.shape, np.uint8)
    d_nbytes = DeviceArray(ctx, (B,), np.uint64)
    d_maxn = DeviceArray(ctx, (B,), np.uint8)
    d_out = DeviceArray(ctx, (B, H, pitch), np.uint8)
    try:
        d_data.upload(data)
        d_nbytes.upload(np.array([len(r.encoded_bytes) for r in res], np.uint64))
        d_maxn.upload(np.array([r.max_n for r in res], np.uint8))
        d_out.upload(np.full((B, H, pitch), 0xA5, np.uint8))
        codec.decode_device_u8(d_data.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_out.ptr, strides=(H * pitch, 1, pitch, 4))
        ctx.synchronize()
        out = d_out.download()
    finally:
        for d in (d_data, d_nbytes, d_maxn, d_out):
            d.free()
    px = out[:, :, :4 * W].reshape(B, H, W, 4)
    assert np.array_equal(px[..., :3].transpose(0, 3, 1, 2), want)
    assert (px[..., 3] == 0xA5).all() and (out[:, :, 4 * W:] == 0xA5).all()
    with pytest.raises(ValueError):  # overlapping output strides: refused before a launch
        codec.decode_device_u8(0, 0, 0, B, 0, strides=(H * pitch, 1, pitch, 2))


def test_u8_batch_stride_beyond_2gib():
    """two pictures 2^31 + 64 bytes apart in one device buffer: every plane offset needs 64 bits"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray
    B, c, H, W = 2, 3, 40, 52
    sb = 2 ** 31 + 64
    P = np.stack([u8_image(300 + b, c, H, W) for b in range(B)])
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=2, max_bits=3000)
    ctx = codec.ctx
    singles = [spiht_amd.encode_image_u8(P[b], s, level=2, max_bits=3000) for b in range(B)]
    buf = DeviceArray(ctx, (sb + c * H * W,), np.uint8)
    d_out = DeviceArray(ctx, (B, codec.slot_stride), np.uint8)
    d_nbits = DeviceArray(ctx, (B,), np.uint64)
    d_maxn = DeviceArray(ctx, (B,), np.uint8)
    d_nbytes = DeviceArray(ctx, (B,), np.uint64)
    try:
        for b in range(B):
            buf.upload(P[b], offset_bytes=b * sb)
        st = (sb, H * W, W, 1)
        codec.encode_device_u8(buf.ptr, B, d_out.ptr, d_nbits.ptr, d_maxn.ptr, strides=st)
        codec.nbits_to_nbytes(d_nbits.ptr, B, d_nbytes.ptr)
        ctx.synchronize()
        out, nbits, maxn = d_out.download(), d_nbits.download(), d_maxn.download()
        for b in range(B):
            assert out[b, :(int(nbits[b]) + 7) // 8].tobytes() == singles[b].encoded_bytes and int(maxn[b]) == singles[b].max_n
        ctx.memset(buf.ptr, 0, c * H * W)
        ctx.memset(buf.ptr + sb, 0, c * H * W)
        codec.decode_device_u8(d_out.ptr, d_nbytes.ptr, d_maxn.ptr, B, buf.ptr, strides=st)
        ctx.synchronize()
        for b in range(B):
            got = np.empty((c, H, W), np.uint8)
            ctx.download(got, buf.ptr + b * sb)
            assert np.array_equal(got, spiht_amd.decode_image_u8(singles[b], s))
    finally:
        for d in (buf, d_out, d_nbits, d_maxn, d_nbytes):
            d.free()


def test_pipeline_u8_steps(oracle):
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray, Pipeline
    B, c, H, W, steps, level, mb = 4, 3, 64, 80, 5, 3, 6000
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=level, max_bits=mb)
    ctx = codec.ctx
    pl = Pipeline(codec, B)
    imgs = [np.stack([u8_image(400 + 10 * st + b, c, H, W) for b in range(B)]) for st in range(steps)]
    hwc = (H * W * c, 1, W * c, c)
    d_in = [DeviceArray(ctx, (B, H, W, c), np.uint8) for _ in range(steps)]
    d_rec = [DeviceArray(ctx, (B, H, W, c), np.uint8) for _ in range(steps)]
    d_out = [DeviceArray(ctx, (B, pl.slot_stride), np.uint8) for _ in range(steps)]
    d_nbits = [DeviceArray(ctx, (B,), np.uint64) for _ in range(steps)]
    d_maxn = [DeviceArray(ctx, (B,), np.uint8) for _ in range(steps)]
    for st in range(steps):
        d_in[st].upload(imgs[st].transpose(0, 2, 3, 1))
    ctx.synchronize()
    for st in range(steps):
        pl.submit_u8(d_in[st].ptr, d_out[st].ptr, d_nbits[st].ptr, d_maxn[st].ptr, d_rec[st].ptr, in_strides=hwc, out_strides=hwc)
    pl.flush()
    pl.synchronize()
    for st in range(steps):
        res = codec.encode_u8(imgs[st])
        nb, out, mn = d_nbits[st].download(), d_out[st].download(), d_maxn[st].download()
        for b in range(B):
            assert (int(nb[b]) + 7) // 8 == len(res[b].encoded_bytes) and int(mn[b]) == res[b].max_n
            assert out[b, :len(res[b].encoded_bytes)].tobytes() == res[b].encoded_bytes
            ob, on, _ = oracle.encode_image(imgs[st][b] / 255, "bior2.2", "reflect", level, 50.0, None, mb)
            assert res[b].encoded_bytes == ob and res[b].max_n == on
        assert np.array_equal(d_rec[st].download().transpose(0, 3, 1, 2), codec.decode_u8(res))
    pl.close()
    for d in d_in + d_rec + d_out + d_nbits + d_maxn:
        d.free()


def test_pipeline_float64_and_u8_steps_alternate():
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray, Pipeline
    B, c, H, W, level, mb = 3, 3, 48, 72, 3, 5000
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=level, max_bits=mb)
    g = codec.geom
    ctx = codec.ctx
    pl = Pipeline(codec, B)
    P = [np.stack([u8_image(500 + 10 * st + b, c, H, W) for b in range(B)]) for st in range(3)]
    kinds = ["f64", "u8", "f64"]
    d_in, d_rec = [], []
    for st, k in enumerate(kinds):
        if k == "f64":
            d_in.append(DeviceArray(ctx, (B, c, H, W), np.float64))
            d_in[-1].upload(P[st] / 255)
            d_rec.append(DeviceArray(ctx, (B, c, g["rec_h"], g["rec_w"]), np.float64))
        else:
            d_in.append(DeviceArray(ctx, (B, c, H, W), np.uint8))
            d_in[-1].upload(P[st])
            d_rec.append(DeviceArray(ctx, (B, c, H, W), np.uint8))
    d_out = [DeviceArray(ctx, (B, pl.slot_stride), np.uint8) for _ in kinds]
    d_nbits = [DeviceArray(ctx, (B,), np.uint64) for _ in kinds]
    d_maxn = [DeviceArray(ctx, (B,), np.uint8) for _ in kinds]
    ctx.synchronize()
    for st, k in enumerate(kinds):
        f = pl.submit if k == "f64" else pl.submit_u8
        f(d_in[st].ptr, d_out[st].ptr, d_nbits[st].ptr, d_maxn[st].ptr, d_rec[st].ptr)
    pl.synchronize()
    for st, k in enumerate(kinds):
        res = codec.encode(P[st] / 255)
        out = d_out[st].download()
        for b in range(B):
            assert out[b, :len(res[b].encoded_bytes)].tobytes() == res[b].encoded_bytes
        if k == "f64":
            assert np.array_equal(d_rec[st].download(), codec.decode(res))
        else:
            assert np.array_equal(d_rec[st].download(), codec.decode_u8(res))
    pl.close()
    for d in d_in + d_rec + d_out + d_nbits + d_maxn:
        d.free()


def test_u8_full_size_1080p():
    import spiht_amd
    c, H, W = 3, 1080, 1920
    P = u8_image(9, c, H, W)
    s = spiht_amd.SpihtSettings()
    mb = int(H * W * 0.5)
    enc = spiht_amd.encode_image_u8(P, s, max_bits=mb)
    ref = spiht_amd.encode_image(P / 255, s, max_bits=mb)
    same_result(enc, ref)
    dec = spiht_amd.decode_image_u8(enc, s)
    assert np.array_equal(dec, to_u8(spiht_amd.decode_image(ref, s), H, W))


def _batch_u8_images(B, c, H, W, seed):
    """B distinct pictures from 8 generated ones (shifted / mirrored variants: the generator is slow at this size)"""
    base = [u8_image(seed + i, c, H, W) for i in range(min(B, 8))]
    out = np.empty((B, c, H, W), np.uint8)
    for b in range(B):
        v = np.roll(base[b % len(base)], 5 * (b // len(base)), axis=2)
        out[b] = v[:, ::-1, :] if (b // len(base)) & 1 else v
    return out


# 40 RGB pictures of 541 x 961: level 1 of the inverse has 8 x 23 tiles of 128 x 24 per plane, 22 080 in all -- above the
# 20 000 from which the launcher takes the persistent inverse kernel (dwt_inv.hip: k_idwt_level_pf) -- and odd sizes, so that
# its crop of the extra row and column is exercised
BIG = (40, 3, 541, 961)


def test_big_batch_geometry_takes_the_persistent_inverse():
    B, c, H, W = BIG
    gx, gy = -(-(W + 1) // 128), -(-(H + 1) // 24)
    assert gx * gy * B * c >= 20000


@pytest.mark.parametrize("level,flags", [(None, 1), (None, 0), (1, 1)])  # FLAGS / plain / FIRST variants
def test_u8_persistent_inverse_at_batch_size(level, flags):
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray
    B, c, H, W = BIG
    P = _batch_u8_images(B, c, H, W, 600)
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=level, max_bits=int(H * W * 0.5))
    ctx = codec.ctx
    res = codec.encode_u8(P)
    for r, q in zip(res, codec.encode(P / 255)):
        same_result(r, q)
    old = ctx.get_option("l1_flags")
    ctx.set_option("l1_flags", flags)
    try:
        f = codec.decode(res)
        u = codec.decode_u8(res)
        u_hwc = codec.decode_u8(res, channels_last=True)
    finally:
        ctx.set_option("l1_flags", old)
    assert f.shape == (B, c, H + 1, W + 1) and u.shape == (B, c, H, W)
    for b in range(B):
        assert np.array_equal(u[b], to_u8(f[b], H, W)), b
    assert np.array_equal(u_hwc, u.transpose(0, 2, 3, 1))
    if level is not None or not flags:
        return
    # into a padded RGBA device buffer: alpha and row padding keep their bytes
    pitch = 4 * W + 20
    data = np.zeros((B, codec.slot_stride), np.uint8)
    for b, r in enumerate(res):
        data[b, :len(r.encoded_bytes)] = np.frombuffer(r.encoded_bytes, np.uint8)
    d_data = DeviceArray(ctx, data.shape, np.uint8)
    d_nbytes = DeviceArray(ctx, (B,), np.uint64)
    d_maxn = DeviceArray(ctx, (B,), np.uint8)
    d_out = DeviceArray(ctx, (B, H, pitch), np.uint8)
    try:
        d_data.upload(data)
        d_nbytes.upload(np.array([len(r.encoded_bytes) for r in res], np.uint64))
        d_maxn.upload(np.array([r.max_n for r in res], np.uint8))
        d_out.upload(np.full((B, H, pitch), 0x5A, np.uint8))
        codec.decode_device_u8(d_data.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_out.ptr, strides=(H * pitch, 1, pitch, 4))
        ctx.synchronize()
        out = d_out.download()
    finally:
        for d in (d_data, d_nbytes, d_maxn, d_out):
            d.free()
    px = out[:, :, :4 * W].reshape(B, H, W, 4)
    assert np.array_equal(px[..., :3].transpose(0, 3, 1, 2), u)
    assert (px[..., 3] == 0x5A).all() and (out[:, :, 4 * W:] == 0x5A).all()


def test_pipeline_u8_at_batch_size():
    """the pipelined schedule at a size whose inverse level 1 is the persistent kernel's FLAGS variant"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray, Pipeline
    B, c, H, W = BIG
    steps = 2
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=None, max_bits=int(H * W * 0.5))
    ctx = codec.ctx
    pl = Pipeline(codec, B)
    imgs = [_batch_u8_images(B, c, H, W, 700 + 10 * st) for st in range(steps)]
    hwc = (H * W * c, 1, W * c, c)
    d_in = [DeviceArray(ctx, (B, H, W, c), np.uint8) for _ in range(steps)]
    d_rec = [DeviceArray(ctx, (B, H, W, c), np.uint8) for _ in range(steps)]
    d_out = [DeviceArray(ctx, (B, pl.slot_stride), np.uint8) for _ in range(steps)]
    d_nbits = [DeviceArray(ctx, (B,), np.uint64) for _ in range(steps)]
    d_maxn = [DeviceArray(ctx, (B,), np.uint8) for _ in range(steps)]
    try:
        for st in range(steps):
            d_in[st].upload(imgs[st].transpose(0, 2, 3, 1))
        ctx.synchronize()
        for st in range(steps):
            pl.submit_u8(d_in[st].ptr, d_out[st].ptr, d_nbits[st].ptr, d_maxn[st].ptr, d_rec[st].ptr, in_strides=hwc,
                         out_strides=hwc)
        pl.synchronize()
        for st in range(steps):
            res = codec.encode(imgs[st] / 255)
            out = d_out[st].download()
            for b in range(B):
                assert out[b, :len(res[b].encoded_bytes)].tobytes() == res[b].encoded_bytes, (st, b)
            f = codec.decode(res)
            got = d_rec[st].download().transpose(0, 3, 1, 2)
            for b in range(B):
                assert np.array_equal(got[b], to_u8(f[b], H, W)), (st, b)
    finally:
        pl.close()
        for d in d_in + d_rec + d_out + d_nbits + d_maxn:
            d.free()
