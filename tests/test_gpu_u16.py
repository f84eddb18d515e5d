"""The 16-bit pixel path on the GPU: uint16 pictures in and out, converted inside level 1 of the transforms (or by a pass of
their own on the routes whose level 1 has no integer form), held bit for bit to the float64 path and to the CPU oracle:
  encode_image_u16(P)  == encode_image(P / 65535.0)                                   (every field)
  decode_image_u16(r)  == (np.clip(decode_image(r), 0, 1) * 65535.0).astype(np.uint16)[:, :h, :w]
No tolerance anywhere: every comparison is equality.  The pictures use all 16 bits (u16_image): conftest.synth_image lies
on the 8-bit grid, and a 16-bit path that dropped the low byte would pass on it."""
import numpy as np
import pytest

from test_gpu_u8 import CONFIGS, BIG, settings, same_result, to_u8

pytestmark = pytest.mark.gpu


def u16_image(seed, c, H, W):
    """A smooth pattern plus noise, rounded to uint16, whose low bytes are noise of their own: every run of 256 samples
    holds all 256 low-byte values (asserted here), so nothing about a picture survives an 8-bit detour."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    planes = []
    for k in range(c):
        fy, fx, ph = rng.uniform(1.0, 4.0), rng.uniform(1.0, 4.0), rng.uniform(0.0, 6.28)
        smooth = 0.5 + 0.3 * np.sin(fy * y / H * 3.1 + ph) * np.cos(fx * x / W * 2.7 + 0.4 * k) + 0.12 * ((x + 2 * y) % 37 > 18)
        planes.append(smooth + rng.normal(0.0, 0.01, (H, W)))
    v = np.round(np.clip(np.stack(planes), 0.0, 1.0) * 65535).astype(np.uint16).reshape(-1)
    low = np.concatenate([rng.permutation(256) for _ in range(-(-v.size // 256))])[:v.size].astype(np.uint16)
    v = ((v & 0xFF00) | low).reshape(c, H, W)
    assert v.size >= 256 and len(np.unique(v & 0xFF)) == 256 and len(np.unique(v >> 8)) > 32
    return v


def to_u16(dec, h, w):
    """the contract's formula: clip, scale, truncate, crop"""
    return (np.clip(dec, 0.0, 1.0) * 65535.0).astype(np.uint16)[:, :h, :w]


def views_of(P):
    """the picture as planar, interleaved and (three channels) 16-bit RGBA views, all (c, H, W)"""
    c, H, W = P.shape
    v = {"chw": P, "hwc": np.ascontiguousarray(P.transpose(1, 2, 0)).transpose(2, 0, 1)}
    if c == 3:
        rgba = np.full((H, W, 4), 0x7777, np.uint16)
        rgba[..., :3] = P.transpose(1, 2, 0)
        v["rgba"] = rgba[..., :3].transpose(2, 0, 1)
        assert v["rgba"].strides == (2, 8 * W, 8)
    return v


@pytest.mark.parametrize("cfg", CONFIGS)
def test_encode_decode_u16_vs_float64_and_oracle(oracle, cfg):
    import spiht_amd
    c, H, W = cfg["c"], cfg["H"], cfg["W"]
    P = u16_image(2000 + H, c, H, W)
    s = settings(cfg)
    ref = spiht_amd.encode_image(P / 65535, s, level=cfg["level"], max_bits=cfg["max_bits"])
    ob, on, _ = oracle.encode_image(P / 65535, s.wavelet, s.mode, cfg["level"], s.quantization_scale,
                                    s.per_channel_quant_scales, cfg["max_bits"])
    assert ref.encoded_bytes == ob and ref.max_n == on
    for name, v in views_of(P).items():
        enc = spiht_amd.encode_image_u16(v, s, level=cfg["level"], max_bits=cfg["max_bits"])
        same_result(enc, ref)
    enc = spiht_amd.encode_image_u16(P.transpose(1, 2, 0), s, level=cfg["level"], max_bits=cfg["max_bits"], channels_last=True)
    same_result(enc, ref)
    # the other byte order and a negative stride are copied first: same result
    same_result(spiht_amd.encode_image_u16(P.astype(">u2" if P.dtype.isnative and np.little_endian else "<u2"), s,
                                           level=cfg["level"], max_bits=cfg["max_bits"]), ref)
    neg = np.ascontiguousarray(P[:, ::-1])[:, ::-1]
    assert neg.strides[1] < 0 and np.array_equal(neg, P)
    same_result(spiht_amd.encode_image_u16(neg, s, level=cfg["level"], max_bits=cfg["max_bits"]), ref)
    # decode
    dec = spiht_amd.decode_image_u16(ref, s)
    assert dec.dtype == np.uint16 and dec.shape == (c, H, W)
    assert np.array_equal(dec, to_u16(spiht_amd.decode_image(ref, s), H, W))
    odec = oracle.decode_image(ob, on, c, H, W, s.wavelet, cfg["level"], s.quantization_scale, s.per_channel_quant_scales)
    assert np.array_equal(dec, to_u16(odec, H, W))
    hwc = spiht_amd.decode_image_u16(ref, s, channels_last=True)
    assert hwc.shape == (H, W, c) and np.array_equal(hwc, dec.transpose(1, 2, 0))


def test_u16_low_byte_is_carried(oracle):
    """The low byte reaches the stream and comes back: at q = 20000 without a bit limit the oracle's own round trip of the
    16-bit picture stays under a quarter of one 8-bit step on average (the condition on the input: no 8-bit path can reach
    that), its stream differs from that of the picture rounded to 8 bits, and the GPU equals the oracle bit for bit."""
    import spiht_amd
    c, H, W, level, q = 3, 48, 64, 2, 20000.0
    P = u16_image(77, c, H, W)
    s = spiht_amd.SpihtSettings(wavelet="bior2.2", mode="reflect", quantization_scale=q)
    ob, on, _ = oracle.encode_image(P / 65535, "bior2.2", "reflect", level, q, None, None)
    P8 = np.round(P / 257.0).astype(np.uint8)
    ob8, on8, _ = oracle.encode_image(P8 / 255, "bior2.2", "reflect", level, q, None, None)
    assert ob != ob8
    odec = to_u16(oracle.decode_image(ob, on, c, H, W, "bior2.2", level, q, None), H, W)
    err = np.abs(odec.astype(np.int64) - P.astype(np.int64))
    print("oracle round trip at q = %g: mean |error| %.2f sixteen-bit steps, max %d" % (q, err.mean(), err.max()))
    assert err.mean() < 64.0
    enc = spiht_amd.encode_image_u16(P, s, level=level)
    assert enc.encoded_bytes == ob and enc.max_n == on
    same_result(enc, spiht_amd.encode_image(P / 65535, s, level=level))
    dec = spiht_amd.decode_image_u16(enc, s)
    assert np.array_equal(dec, odec)
    assert np.array_equal(spiht_amd.decode_image_u16(enc, s, channels_last=True), odec.transpose(1, 2, 0))


def test_decode_u16_saturated_odd_sizes(oracle):
    """blocks of 0 and 65535 at a high quantisation scale: decoded values overshoot [0, 1] on both sides (the clip), odd
    sizes (the crop of the extra row and column)"""
    import spiht_amd
    c, H, W = 3, 41, 67
    P = np.zeros((c, H, W), np.uint16)
    P[:, ::2, :] = 65535
    P[1, :, 10:30] = 65535
    P[2, 20:, :] = 0
    s = spiht_amd.SpihtSettings(quantization_scale=1000.0)
    enc = spiht_amd.encode_image_u16(P, s, level=3)
    same_result(enc, spiht_amd.encode_image(P / 65535, s, level=3))
    f = spiht_amd.decode_image(enc, s)
    assert f.shape == (c, H + 1, W + 1) and f.min() < 0.0 and f.max() > 1.0
    dec = spiht_amd.decode_image_u16(enc, s)
    assert dec.shape == (c, H, W) and np.array_equal(dec, to_u16(f, H, W))
    assert dec.min() == 0 and dec.max() == 65535
    odec = oracle.decode_image(enc.encoded_bytes, enc.max_n, c, H, W, "bior2.2", 3, 1000.0, None)
    assert odec.shape == (c, H + 1, W + 1)
    assert np.array_equal(dec, to_u16(odec, H, W))


@pytest.mark.parametrize("cfg", [
    dict(color="IPT", q=1.0, mults=[50.0, 15.0, 15.0], level=3),       # colour change fused into level 1
    dict(color="IPT", mode="periodization", level=2),                    # ... in front of / behind a two-pass level
    dict(mode="smooth", level=2),
    dict(mode="antireflect", level=3),
    dict(wavelet="db11", level=2),                                       # a filter longer than the tiled kernels take
])
def test_u16_routes_vs_float64(cfg):
    import spiht_amd
    c, H, W = 3, 57, 83
    P = u16_image(31, c, H, W)
    s = settings(cfg)
    ref = spiht_amd.encode_image(P / 65535, s, level=cfg["level"], max_bits=6000)
    for name, v in views_of(P).items():
        same_result(spiht_amd.encode_image_u16(v, s, level=cfg["level"], max_bits=6000), ref)
    hwc = np.ascontiguousarray(P.transpose(1, 2, 0))
    same_result(spiht_amd.encode_image_u16(hwc, s, level=cfg["level"], max_bits=6000, channels_last=True), ref)
    dec = spiht_amd.decode_image_u16(ref, s)
    assert np.array_equal(dec, to_u16(spiht_amd.decode_image(ref, s), H, W))
    assert np.array_equal(spiht_amd.decode_image_u16(ref, s, channels_last=True), dec.transpose(1, 2, 0))


def test_one_stream_decodes_into_every_format(oracle):
    """a stream does not record the pixel format it came from: one encoded from float64 decodes into float64, uint16 and
    uint8 by the contract's formulas on the one float64 result"""
    import spiht_amd
    c, H, W = 3, 45, 59
    img = u16_image(8, c, H, W) / 65535
    s = spiht_amd.SpihtSettings(quantization_scale=300.0)
    enc = spiht_amd.encode_image(img, s, level=3, max_bits=20000)
    f = spiht_amd.decode_image(enc, s)
    assert np.array_equal(f, oracle.decode_image(enc.encoded_bytes, enc.max_n, c, H, W, "bior2.2", 3, 300.0, None))
    u16 = spiht_amd.decode_image_u16(enc, s)
    u8 = spiht_amd.decode_image_u8(enc, s)
    assert np.array_equal(u16, to_u16(f, H, W)) and np.array_equal(u8, to_u8(f, H, W))
    # and a stream from 8-bit pixels decodes into 16-bit ones
    P8 = np.round(img * 255).astype(np.uint8)
    e8 = spiht_amd.encode_image_u8(P8, s, level=3, max_bits=20000)
    assert np.array_equal(spiht_amd.decode_image_u16(e8, s), to_u16(spiht_amd.decode_image(e8, s), H, W))


def test_batch_u16_equals_single_calls():
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    B, c, H, W = 7, 3, 45, 61
    P = np.stack([u16_image(100 + b, c, H, W) for b in range(B)])
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=3, max_bits=5000)
    res = codec.encode_u16(P)
    singles = [spiht_amd.encode_image_u16(P[b], s, level=3, max_bits=5000) for b in range(B)]
    for r, q in zip(res, singles):
        same_result(r, q)
    for r, q in zip(codec.encode_u16(P.transpose(0, 2, 3, 1), channels_last=True), singles):
        same_result(r, q)
    dec = codec.decode_u16(res)
    assert dec.shape == (B, c, H, W) and dec.dtype == np.uint16
    for b in range(B):
        assert np.array_equal(dec[b], spiht_amd.decode_image_u16(singles[b], s))
    assert np.array_equal(codec.decode_u16(res, channels_last=True), dec.transpose(0, 2, 3, 1))


def _batch_u16_images(B, c, H, W, seed):
    """B distinct pictures from 4 generated ones (shifted / mirrored variants)"""
    base = [u16_image(seed + i, c, H, W) for i in range(min(B, 4))]
    out = np.empty((B, c, H, W), np.uint16)
    for b in range(B):
        v = np.roll(base[b % len(base)], 5 * (b // len(base)), axis=2)
        out[b] = v[:, ::-1, :] if (b // len(base)) & 1 else v
    return out


@pytest.mark.parametrize("level,flags", [(None, 1), (None, 0), (1, 1)])  # FLAGS / plain / FIRST variants
def test_u16_persistent_inverse_at_batch_size(level, flags):
    """BIG: 22 080 level-1 tiles, above the 20 000 from which the launcher takes the persistent inverse kernel, odd sizes"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray
    B, c, H, W = BIG
    P = _batch_u16_images(B, c, H, W, 600)
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=level, max_bits=int(H * W * 0.5))
    ctx = codec.ctx
    res = codec.encode_u16(P)
    for r, q in zip(res, codec.encode(P / 65535)):
        same_result(r, q)
    old = ctx.get_option("l1_flags")
    ctx.set_option("l1_flags", flags)
    try:
        f = codec.decode(res)
        u = codec.decode_u16(res)
        u_hwc = codec.decode_u16(res, channels_last=True)
    finally:
        ctx.set_option("l1_flags", old)
    assert f.shape == (B, c, H + 1, W + 1) and u.shape == (B, c, H, W) and u.dtype == np.uint16
    for b in range(B):
        assert np.array_equal(u[b], to_u16(f[b], H, W)), b
    assert np.array_equal(u_hwc, u.transpose(0, 2, 3, 1))
    # the device forms on strided views: from a padded 16-bit RGBA buffer, and back into one -- alpha and row padding keep
    # their bytes
    pitch = 8 * W + 20  # bytes
    host = np.full((B, H, pitch // 2), 0x5A5A, np.uint16)
    host[:, :, :4 * W].reshape(B, H, W, 4)[..., :3] = P.transpose(0, 2, 3, 1)
    st = (H * pitch, 2, pitch, 8)
    d_px = DeviceArray(ctx, host.shape, np.uint16)
    d_out = DeviceArray(ctx, (B, codec.slot_stride), np.uint8)
    d_nbits = DeviceArray(ctx, (B,), np.uint64)
    d_nbytes = DeviceArray(ctx, (B,), np.uint64)
    d_maxn = DeviceArray(ctx, (B,), np.uint8)
    ctx.set_option("l1_flags", flags)
    try:
        d_px.upload(host)
        codec.encode_device_u16(d_px.ptr, B, d_out.ptr, d_nbits.ptr, d_maxn.ptr, strides=st)
        codec.nbits_to_nbytes(d_nbits.ptr, B, d_nbytes.ptr)
        ctx.synchronize()
        out, nbits, maxn = d_out.download(), d_nbits.download(), d_maxn.download()
        for b in range(B):
            assert out[b, :(int(nbits[b]) + 7) // 8].tobytes() == res[b].encoded_bytes and int(maxn[b]) == res[b].max_n, b
        d_px.upload(np.full(host.shape, 0x5A5A, np.uint16))
        codec.decode_device_u16(d_out.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_px.ptr, strides=st)
        ctx.synchronize()
        got = d_px.download()
    finally:
        ctx.set_option("l1_flags", old)
        for d in (d_px, d_out, d_nbits, d_nbytes, d_maxn):
            d.free()
    px = got[:, :, :4 * W].reshape(B, H, W, 4)
    assert np.array_equal(px[..., :3].transpose(0, 3, 1, 2), u)
    assert (px[..., 3] == 0x5A5A).all() and (got[:, :, 4 * W:] == 0x5A5A).all()
    with pytest.raises(ValueError):  # overlapping output strides: refused before a launch
        codec.decode_device_u16(0, 0, 0, B, 0, strides=(H * pitch, 2, pitch, 4))


def test_pipeline_u16_steps(oracle):
    """Pipeline.submit_u16 against the unpipelined calls: several steps and the flush, interleaved views, and float64,
    8-bit and 16-bit steps alternating on one pipeline"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray, Pipeline
    B, c, H, W, steps, level, mb = 4, 3, 64, 80, 5, 3, 6000
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=level, max_bits=mb)
    g = codec.geom
    ctx = codec.ctx
    pl = Pipeline(codec, B)
    imgs = [np.stack([u16_image(400 + 10 * st + b, c, H, W) for b in range(B)]) for st in range(steps)]
    kinds = ["u16", "u16", "f64", "u8", "u16"]
    hwc = (2 * H * W * c, 2, 2 * W * c, 2 * c)
    d_in, d_rec = [], []
    for st, k in enumerate(kinds):
        if k == "u16":
            d_in.append(DeviceArray(ctx, (B, H, W, c), np.uint16))
            d_in[-1].upload(imgs[st].transpose(0, 2, 3, 1))
            d_rec.append(DeviceArray(ctx, (B, H, W, c), np.uint16))
        elif k == "u8":
            d_in.append(DeviceArray(ctx, (B, c, H, W), np.uint8))
            d_in[-1].upload((imgs[st] >> 8).astype(np.uint8))
            d_rec.append(DeviceArray(ctx, (B, c, H, W), np.uint8))
        else:
            d_in.append(DeviceArray(ctx, (B, c, H, W), np.float64))
            d_in[-1].upload(imgs[st] / 65535)
            d_rec.append(DeviceArray(ctx, (B, c, g["rec_h"], g["rec_w"]), np.float64))
    d_out = [DeviceArray(ctx, (B, pl.slot_stride), np.uint8) for _ in range(steps)]
    d_nbits = [DeviceArray(ctx, (B,), np.uint64) for _ in range(steps)]
    d_maxn = [DeviceArray(ctx, (B,), np.uint8) for _ in range(steps)]
    try:
        ctx.synchronize()
        for st, k in enumerate(kinds):
            if k == "u16":
                pl.submit_u16(d_in[st].ptr, d_out[st].ptr, d_nbits[st].ptr, d_maxn[st].ptr, d_rec[st].ptr, in_strides=hwc,
                              out_strides=hwc)
            else:
                (pl.submit if k == "f64" else pl.submit_u8)(d_in[st].ptr, d_out[st].ptr, d_nbits[st].ptr, d_maxn[st].ptr, d_rec[st].ptr)
        pl.flush()
        pl.synchronize()
        for st, k in enumerate(kinds):
            res = codec.encode_u8((imgs[st] >> 8).astype(np.uint8)) if k == "u8" else codec.encode_u16(imgs[st])
            nb, out, mn = d_nbits[st].download(), d_out[st].download(), d_maxn[st].download()
            for b in range(B):
                assert (int(nb[b]) + 7) // 8 == len(res[b].encoded_bytes) and int(mn[b]) == res[b].max_n
                assert out[b, :len(res[b].encoded_bytes)].tobytes() == res[b].encoded_bytes
                if k != "u8":
                    ob, on, _ = oracle.encode_image(imgs[st][b] / 65535, "bior2.2", "reflect", level, 50.0, None, mb)
                    assert res[b].encoded_bytes == ob and res[b].max_n == on
            if k == "u16":
                assert np.array_equal(d_rec[st].download().transpose(0, 3, 1, 2), codec.decode_u16(res))
            elif k == "u8":
                assert np.array_equal(d_rec[st].download(), codec.decode_u8(res))
            else:
                assert np.array_equal(d_rec[st].download(), codec.decode(res))
        with pytest.raises(ValueError):  # a bad view leaves the pipeline as it was
            pl.submit_u16(d_in[0].ptr, d_out[0].ptr, d_nbits[0].ptr, d_maxn[0].ptr, d_rec[0].ptr, out_strides=(2 * H * W * c, 2, 2 * W * c, 4))
        pl.submit_u16(d_in[0].ptr, d_out[0].ptr, d_nbits[0].ptr, d_maxn[0].ptr, d_rec[0].ptr, in_strides=hwc, out_strides=hwc)
        pl.synchronize()
        assert np.array_equal(d_rec[0].download().transpose(0, 3, 1, 2), codec.decode_u16(codec.encode_u16(imgs[0])))
    finally:
        pl.close()
        for d in d_in + d_rec + d_out + d_nbits + d_maxn:
            d.free()


def test_pipeline_u16_at_batch_size():
    """the pipelined schedule at a size whose inverse level 1 is the persistent kernel's FLAGS variant"""
    import spiht_amd
    from spiht_amd.batch import BatchCodec, DeviceArray, Pipeline
    B, c, H, W = BIG
    steps = 2
    s = spiht_amd.SpihtSettings()
    codec = BatchCodec(c, H, W, s, level=None, max_bits=int(H * W * 0.5))
    ctx = codec.ctx
    pl = Pipeline(codec, B)
    imgs = [_batch_u16_images(B, c, H, W, 700 + 10 * st) for st in range(steps)]
    hwc = (2 * H * W * c, 2, 2 * W * c, 2 * c)
    d_in = [DeviceArray(ctx, (B, H, W, c), np.uint16) for _ in range(steps)]
    d_rec = [DeviceArray(ctx, (B, H, W, c), np.uint16) for _ in range(steps)]
    d_out = [DeviceArray(ctx, (B, pl.slot_stride), np.uint8) for _ in range(steps)]
    d_nbits = [DeviceArray(ctx, (B,), np.uint64) for _ in range(steps)]
    d_maxn = [DeviceArray(ctx, (B,), np.uint8) for _ in range(steps)]
    try:
        for st in range(steps):
            d_in[st].upload(imgs[st].transpose(0, 2, 3, 1))
        ctx.synchronize()
        for st in range(steps):
            pl.submit_u16(d_in[st].ptr, d_out[st].ptr, d_nbits[st].ptr, d_maxn[st].ptr, d_rec[st].ptr, in_strides=hwc,
                          out_strides=hwc)
        pl.synchronize()
        for st in range(steps):
            res = codec.encode(imgs[st] / 65535)
            out = d_out[st].download()
            for b in range(B):
                assert out[b, :len(res[b].encoded_bytes)].tobytes() == res[b].encoded_bytes, (st, b)
            f = codec.decode(res)
            got = d_rec[st].download().transpose(0, 3, 1, 2)
            for b in range(B):
                assert np.array_equal(got[b], to_u16(f[b], H, W)), (st, b)
    finally:
        pl.close()
        for d in d_in + d_rec + d_out + d_nbits + d_maxn:
            d.free()
