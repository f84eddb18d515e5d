"""GPU tests of the batched decode_with_metadata (spiht_decode_with_metadata_batch_i32, spiht.decode_with_metadata_batch,
BatchCodec.decode_with_metadata / decode_with_metadata_device): every image's decoded array and every metadata row
against the CPU oracle's restatement, exactly."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth_coeffs, synth_image
from test_gpu_metadata import SHAPES, nominal_slices, tree_generations

pytestmark = pytest.mark.gpu
UNLIMITED = 99999999999999999


def _check_batch(O, streams, ns, shape, lh, lw, top, other):
    import spiht_amd
    c, h, w = shape
    rec, metas = spiht_amd.spiht.decode_with_metadata_batch(streams, ns, c, h, w, lh, lw, top, other)
    assert rec.dtype == np.int32 and rec.shape == (len(streams), c, h, w)
    assert len(metas) == len(streams)
    for b, (d, n) in enumerate(zip(streams, ns)):
        m = metas[b]
        assert m.dtype == np.int32 and m.shape == (8 * len(d) + 1, 8) and m.flags.c_contiguous
        r_ref, m_ref = O.decode_with_metadata(d, n, c, h, w, lh, lw, top, other)
        if not np.array_equal(m, m_ref):
            bad = np.argwhere((m != m_ref).any(axis=1))[:, 0]
            q = int(bad[0])
            raise AssertionError("image %d (%d bytes, n=%d): metadata differs in %d rows of %d, first row %d: got %s want %s"
                                 % (b, len(d), n, len(bad), len(m), q, m[q].tolist(), m_ref[q].tolist()))
        assert np.array_equal(rec[b], r_ref), "image %d: decoded array differs" % b
    return rec, metas


def _mixed_streams(shape, seed):
    import spiht_amd
    c, h, w, lh, lw = shape
    x = synth_coeffs(h * 1000 + w, c, h, w, lh, lw, scale=60.0)
    d, n = spiht_amd.encode(x, lh, lw, UNLIMITED)
    rng = np.random.default_rng(seed)
    streams = [d, d[:0], d[:1], d[:7], d[:len(d) // 2], d[:max(len(d) - 1, 0)], d + b"\xa5" * 9]
    ns = [n] * len(streams)
    for nb, rn in ((5, 0), (40, 3), (200, 9), (13, 17)):
        streams.append(rng.integers(0, 256, nb, dtype=np.uint8).tobytes())
        ns.append(rn)
    return streams, ns


@pytest.mark.parametrize("shape", SHAPES)
def test_batch_matches_oracle(oracle, shape):
    c, h, w, lh, lw = shape
    top, other = nominal_slices(lh, lw, tree_generations(h, w, lh, lw))
    streams, ns = _mixed_streams(shape, 11)
    _check_batch(oracle, streams, ns, (c, h, w), lh, lw, top, other)


def _dev(ctx, arr):
    from spiht_amd.batch import DeviceArray
    d = DeviceArray(ctx, arr.shape, arr.dtype)
    d.upload(arr)
    return d


def _slots(streams, stride):
    data = np.zeros((len(streams), stride), dtype=np.uint8)
    for b, d in enumerate(streams):
        data[b, :len(d)] = np.frombuffer(d, np.uint8)
    return data


def _slice_args(top, other):
    topv = np.array([top[0][0], top[0][1], top[1][0], top[1][1]], dtype=np.int64)
    oth = np.array([[[f[0][0], f[0][1], f[1][0], f[1][1]] for f in lv] for lv in other], dtype=np.int64).reshape(-1)
    return topv, np.ascontiguousarray(oth)


def _call(ctx, d_data, stride, d_nb, d_mn, B, shape, lh, lw, topv, oth, level, d_out, d_meta, meta_rows):
    from spiht_amd import _lib
    c, h, w = shape
    return _lib.lib().spiht_decode_with_metadata_batch_i32(
        ctx.handle, C.c_void_p(d_data), stride, C.c_void_p(d_nb), C.c_void_p(d_mn), B, c, h, w, lh, lw,
        C.c_void_p(topv.ctypes.data), C.c_void_p(oth.ctypes.data), level, C.c_void_p(d_out) if d_out else None,
        C.c_void_p(d_meta), meta_rows)


def test_device_form_tail_rows_and_meta_rows(oracle):
    """meta_rows larger than needed: every row past an image's 8 * nbytes + 1 is written as zero; too few rows: refused"""
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    c, h, w, lh, lw = 3, 33, 29, 6, 5
    top, other = nominal_slices(lh, lw, tree_generations(h, w, lh, lw))
    topv, oth = _slice_args(top, other)
    streams, ns = _mixed_streams((c, h, w, lh, lw), 3)
    B = len(streams)
    stride = (max(len(d) for d in streams) + 3) & ~3
    meta_rows = 8 * stride + 1 + 37
    ctx = _lib.default_context()
    d_data = _dev(ctx, _slots(streams, stride))
    d_nb = _dev(ctx, np.array([len(d) for d in streams], dtype=np.uint64))
    d_mn = _dev(ctx, np.array(ns, dtype=np.uint8))
    d_meta = DeviceArray(ctx, (B, meta_rows, 8), np.int32)
    d_out = DeviceArray(ctx, (B, c, h, w), np.int32)
    try:
        ctx.memset(d_meta.ptr, 0x7F, d_meta.nbytes)  # what was there before is overwritten, tail rows included
        _lib.check(_call(ctx, d_data.ptr, stride, d_nb.ptr, d_mn.ptr, B, (c, h, w), lh, lw, topv, oth, len(other),
                         d_out.ptr, d_meta.ptr, meta_rows))
        ctx.synchronize()
        meta, rec = d_meta.download(), d_out.download()
        for b, (d, n) in enumerate(zip(streams, ns)):
            r_ref, m_ref = oracle.decode_with_metadata(d, n, c, h, w, lh, lw, top, other)
            rows = 8 * len(d) + 1
            assert np.array_equal(meta[b, :rows], m_ref), b
            assert not meta[b, rows:].any(), b
            assert np.array_equal(rec[b], r_ref), b
        # without d_out the same tables
        ctx.memset(d_meta.ptr, 0x7F, d_meta.nbytes)
        _lib.check(_call(ctx, d_data.ptr, stride, d_nb.ptr, d_mn.ptr, B, (c, h, w), lh, lw, topv, oth, len(other),
                         None, d_meta.ptr, meta_rows))
        ctx.synchronize()
        assert np.array_equal(d_meta.download(), meta)
        st = _call(ctx, d_data.ptr, stride, d_nb.ptr, d_mn.ptr, B, (c, h, w), lh, lw, topv, oth, len(other), d_out.ptr,
                   d_meta.ptr, 8 * stride)
        assert st == _lib.ERR_ARG
        st = _call(ctx, d_data.ptr, stride + 2, d_nb.ptr, d_mn.ptr, B, (c, h, w), lh, lw, topv, oth, len(other), d_out.ptr,
                   d_meta.ptr, meta_rows + 100)
        assert st == _lib.ERR_ARG  # slot_stride % 4
        assert _call(ctx, d_data.ptr, stride, d_nb.ptr, d_mn.ptr, 0, (c, h, w), lh, lw, topv, oth, len(other), d_out.ptr,
                     d_meta.ptr, meta_rows) == _lib.OK
        ctx.synchronize()
    finally:
        for d in (d_data, d_nb, d_mn, d_meta, d_out):
            d.free()


def test_slot_reuse(oracle):
    """more images than the decoder has slots (num_cu * 8): slots serve several images in one launch"""
    import spiht_amd
    from spiht_amd import _lib
    c, h, w, lh, lw = 1, 16, 16, 2, 2
    B = max(2100, _lib.default_context().get_option("num_cu") * 8 + 52)
    top, other = nominal_slices(lh, lw, tree_generations(h, w, lh, lw))
    base = []
    for s in range(30):
        x = synth_coeffs(500 + s, c, h, w, lh, lw, scale=float(4 + 7 * s))
        base.append(spiht_amd.encode(x, lh, lw, UNLIMITED))
    streams, ns = [], []
    for b in range(B):
        d, n = base[b % 30]
        streams.append(d[:max(0, len(d) - (b // 30) % 9)])
        ns.append(n)
    _check_batch(oracle, streams, ns, (c, h, w), lh, lw, top, other)


def test_chunk_boundaries(oracle):
    """meta_chunk 1 and 3 over ten images: the tables of the automatic setting, and the oracle's"""
    import spiht_amd
    from spiht_amd import _lib
    c, h, w, lh, lw = 3, 24, 40, 3, 5
    top, other = nominal_slices(lh, lw, tree_generations(h, w, lh, lw))
    streams, ns = _mixed_streams((c, h, w, lh, lw), 5)
    streams, ns = streams[:10], ns[:10]
    ctx = _lib.default_context()
    assert ctx.get_option("meta_chunk") == 0
    rec0, m0 = _check_batch(oracle, streams, ns, (c, h, w), lh, lw, top, other)
    try:
        for k in (1, 3):
            ctx.set_option("meta_chunk", k)
            assert ctx.get_option("meta_chunk") == k
            rec, m = spiht_amd.spiht.decode_with_metadata_batch(streams, ns, c, h, w, lh, lw, top, other)
            assert np.array_equal(rec, rec0), k
            assert all(np.array_equal(a, b) for a, b in zip(m, m0)), k
    finally:
        ctx.set_option("meta_chunk", 0)


@pytest.mark.parametrize("case", ["default", "bior4.4-level2", "odd-size", "IPT-scales"])
def test_batch_codec_decode_with_metadata(case):
    from spiht_amd import EncodingResult, SpihtSettings, decode_image, encode_image
    from spiht_amd.batch import BatchCodec
    c, H, W, level, max_bits = 3, 64, 96, None, 9000
    settings = SpihtSettings()
    if case == "bior4.4-level2":
        settings, level = SpihtSettings(wavelet="bior4.4", quantization_scale=20.0), 2
    elif case == "odd-size":
        H, W = 37, 53
    elif case == "IPT-scales":
        settings = SpihtSettings(color_model="IPT", per_channel_quant_scales=[100.0, 20.0, 20.0])
    imgs = np.stack([synth_image(40 + b, c, H, W) for b in range(4)])
    codec = BatchCodec(c, H, W, settings, level=level, max_bits=max_bits)
    results = [encode_image(im, settings, level=level, max_bits=max_bits) for im in imgs]
    r = results[1]
    results.append(EncodingResult(r.encoded_bytes[:len(r.encoded_bytes) // 3], r.h, r.w, r.c, r.max_n, r.level))
    images, metas = codec.decode_with_metadata(results)
    assert np.array_equal(images, codec.decode(results))
    for b, r in enumerate(results):
        im_ref, m_ref = decode_image(r, settings, return_metadata=True)
        assert metas[b].shape == (8 * len(r.encoded_bytes) + 1, 8) and metas[b].flags.c_contiguous
        assert np.array_equal(metas[b], m_ref), b
        assert np.allclose(images[b], im_ref), b


def test_device_pipeline_without_host_round_trip(oracle):
    """encode_device -> nbits_to_nbytes -> decode_with_metadata_device: the codec's own slots, nothing through the host"""
    from spiht_amd import SpihtSettings
    from spiht_amd.batch import BatchCodec, DeviceArray
    from spiht_amd.spiht_wrapper import _metadata_boxes
    c, H, W, B = 3, 48, 80, 6
    settings = SpihtSettings(wavelet="bior4.4")
    codec = BatchCodec(c, H, W, settings, level=3, max_bits=6000)
    g = codec.geom
    ctx = codec.ctx
    imgs = np.stack([synth_image(70 + b, c, H, W) for b in range(B)])
    ss = codec.slot_stride
    meta_rows = 8 * ss + 1
    d_img = _dev(ctx, imgs)
    bufs = [DeviceArray(ctx, (B, ss), np.uint8), DeviceArray(ctx, (B,), np.uint64), DeviceArray(ctx, (B,), np.uint64),
            DeviceArray(ctx, (B,), np.uint8), DeviceArray(ctx, (B, meta_rows, 8), np.int32),
            DeviceArray(ctx, (B, c, g["rec_h"], g["rec_w"]), np.float64), DeviceArray(ctx, (B, c, g["enc_h"], g["enc_w"]), np.int32)]
    d_out, d_nbits, d_nbytes, d_maxn, d_meta, d_pix, d_rec = bufs
    try:
        codec.encode_device(d_img.ptr, B, d_out.ptr, d_nbits.ptr, d_maxn.ptr)
        codec.nbits_to_nbytes(d_nbits.ptr, B, d_nbytes.ptr)
        codec.decode_with_metadata_device(d_out.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_meta.ptr, meta_rows, d_img_out=d_pix.ptr,
                                          d_rec=d_rec.ptr)
        ctx.synchronize()
        slots, nbytes, maxn = d_out.download(), d_nbytes.download(), d_maxn.download()
        meta, pix, rec = d_meta.download(), d_pix.download(), d_rec.download()
        # the scratch form (no d_rec) gives the same pictures
        d_pix.zero()
        codec.decode_with_metadata_device(d_out.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_meta.ptr, meta_rows, d_img_out=d_pix.ptr)
        ctx.synchronize()
        assert np.array_equal(d_pix.download(), pix)
        codec.decode_device(d_out.ptr, d_nbytes.ptr, d_maxn.ptr, B, d_pix.ptr)
        ctx.synchronize()
        assert np.array_equal(d_pix.download(), pix)
    finally:
        for d in bufs + [d_img]:
            d.free()
    top, other = _metadata_boxes(H, W, settings, g)
    for b in range(B):
        d = slots[b, :int(nbytes[b])].tobytes()
        r_ref, m_ref = oracle.decode_with_metadata(d, int(maxn[b]), c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"], top, other)
        rows = 8 * len(d) + 1
        assert np.array_equal(meta[b, :rows], m_ref), b
        assert not meta[b, rows:].any(), b
        assert np.array_equal(rec[b], r_ref), b


def test_errors():
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    c, h, w, lh, lw = 1, 32, 32, 2, 2
    x = synth_coeffs(3, c, h, w, lh, lw, scale=40.0)
    d, n = spiht_amd.encode(x, lh, lw, UNLIMITED)
    top, other = nominal_slices(lh, lw, 3)  # the tree has 4 generations
    with pytest.raises(spiht_amd.spiht.PanicException):
        spiht_amd.spiht.decode_with_metadata_batch([d, d], [n, n], c, h, w, lh, lw, top, other)
    # max_n = 31 on the device: reported by synchronize; the next good call on the context succeeds
    top, other = nominal_slices(lh, lw, 4)
    topv, oth = _slice_args(top, other)
    stride = (len(d) + 3) & ~3
    ctx = _lib.default_context()
    d_data = _dev(ctx, _slots([d, d], stride))
    d_nb = _dev(ctx, np.array([len(d), len(d)], dtype=np.uint64))
    d_mn = _dev(ctx, np.array([n, 31], dtype=np.uint8))
    d_meta = DeviceArray(ctx, (2, 8 * stride + 1, 8), np.int32)
    try:
        _lib.check(_call(ctx, d_data.ptr, stride, d_nb.ptr, d_mn.ptr, 2, (c, h, w), lh, lw, topv, oth, 4, None, d_meta.ptr,
                         8 * stride + 1))
        with pytest.raises(spiht_amd.spiht.SpihtHipError):  # the device error word, as every batched decode reports it
            ctx.synchronize()
    finally:
        for a in (d_data, d_nb, d_mn, d_meta):
            a.free()
    rec, metas = spiht_amd.spiht.decode_with_metadata_batch([d, d[:5]], [n, n], c, h, w, lh, lw, top, other)
    r1, m1 = spiht_amd.spiht.decode_with_metadata(d, n, c, h, w, lh, lw, top, other)
    assert np.array_equal(rec[0], r1) and np.array_equal(metas[0], m1) and np.array_equal(rec[0], x)
