"""GPU tests of the host-fed streams (spiht_amd/hoststream.py over include/spiht_hip.h: spiht_hstream_*): every result of a
stream equals the single-picture call's, field by field and bit for bit; the ring's rules hold on the device as they do in the
model.  Shapes are the smallest that still reuse slots (7 steps on 2 or 3 slots), end on a short batch (n = 1) and have an odd
geometry.  No test asserts a time."""
import functools

import numpy as np
import pytest

from conftest import synth_image

pytestmark = pytest.mark.gpu

B, C3, STEPS = 3, 3, 7
NPIC = B * (STEPS - 1) + 1   # 19 pictures: six full steps and one of a single picture

# (H, W, level, wavelet, mode)
GEOMS = {
    "16x24": (16, 24, 2, "bior2.2", "reflect"),
    "33x41": (33, 41, None, "bior2.2", "reflect"),
    "33x41-per": (33, 41, None, "bior4.4", "periodization"),
}
MID_BYTE = 1237   # a budget that ends inside a byte


def _settings(geom, **kw):
    import spiht_amd
    _, _, _, wavelet, mode = GEOMS[geom]
    return spiht_amd.SpihtSettings(wavelet=wavelet, mode=mode, **kw)


@functools.lru_cache(maxsize=None)
def _pictures(geom, dtype):
    """the 19 pictures of a geometry in one pixel type (made once, never written)"""
    from spiht_amd import floatpx
    H, W = GEOMS[geom][:2]
    f = [synth_image(7000 + 31 * k + H, C3, H, W) for k in range(NPIC)]
    if dtype == "float64":
        out = f
    elif dtype == "uint8":
        out = [np.round(p * 255).astype(np.uint8) for p in f]
    elif dtype == "uint16":
        rng = np.random.default_rng(5)
        out = [np.clip(np.round(p * 65535) + rng.integers(-40, 40, p.shape), 0, 65535).astype(np.uint16) for p in f]
    elif dtype == "bfloat16":
        out = [floatpx.bfloat16_bits(p) for p in f]
    else:
        out = [p.astype(dtype) for p in f]
    for p in out:
        p.setflags(write=False)
    return tuple(out)


def _single_encode(p, dtype, s, level, max_bits):
    import spiht_amd
    if dtype == "float64":
        return spiht_amd.encode_image(p, s, level, max_bits)
    if dtype == "uint8":
        return spiht_amd.encode_image_u8(p, s, level, max_bits)
    if dtype == "uint16":
        return spiht_amd.encode_image_u16(p, s, level, max_bits)
    return spiht_amd.encode_image_float(p, s, level, max_bits, dtype="bfloat16" if dtype == "bfloat16" else None)


@functools.lru_cache(maxsize=None)
def _single_encodes(geom, dtype, max_bits):
    """the single-picture encodes the streams are held to (made once per case, shared)"""
    level = GEOMS[geom][2]
    return tuple(_single_encode(p, dtype, _settings(geom), level, max_bits) for p in _pictures(geom, dtype))


def _batches(pics):
    return [np.stack(pics[i:i + B]) for i in range(0, len(pics), B)]


def _same(a, b):
    assert (a.encoded_bytes, a.max_n, a.h, a.w, a.c, a.level, a._encoding_version) == \
        (b.encoded_bytes, b.max_n, b.h, b.w, b.c, b.level, b._encoding_version)


ENCODE_CASES = [(d, g, depth, mb)
                for d in ("float64", "uint8", "uint16", "float32", "float16", "bfloat16")
                for (g, depth, mb) in (("16x24", 2, None), ("33x41", 3, MID_BYTE))] + \
               [("float64", "33x41-per", 3, MID_BYTE), ("uint8", "33x41-per", 2, None), ("float64", "33x41", 2, None),
                ("uint8", "16x24", 3, MID_BYTE)]


@pytest.mark.parametrize("dtype,geom,depth,max_bits", ENCODE_CASES)
def test_stream_encoder_equals_single_picture_calls(dtype, geom, depth, max_bits):
    import spiht_amd
    H, W, level = GEOMS[geom][:3]
    pics = _pictures(geom, dtype)
    want = _single_encodes(geom, dtype, max_bits)
    with spiht_amd.StreamEncoder(C3, H, W, _settings(geom), level, max_bits, dtype=dtype, batch=B, depth=depth) as enc:
        got = list(enc.run(_batches(pics)))
    assert [len(g) for g in got] == [B] * (STEPS - 1) + [1]
    for r, w in zip([r for g in got for r in g], want):
        _same(r, w)
    if max_bits is not None:
        assert max(len(r.encoded_bytes) for g in got for r in g) == (max_bits + 7) // 8   # the budget does cut, inside a byte
    # ... and through the convenience, one result per picture
    fn = {"float64": spiht_amd.encode_images, "uint8": spiht_amd.encode_images_u8, "uint16": spiht_amd.encode_images_u16}.get(dtype)
    kw = {} if fn else dict(dtype=dtype)
    out = list((fn or spiht_amd.encode_images_float)(iter(pics[:5]), _settings(geom), level, max_bits, batch=2, depth=depth, **kw))
    assert len(out) == 5
    for r, w in zip(out, want):
        _same(r, w)


@pytest.mark.parametrize("dtype", ["float64", "uint8"])
def test_one_step_against_the_oracle(oracle, dtype):
    import spiht_amd
    geom = "33x41"
    H, W, level, wavelet, mode = GEOMS[geom]
    pics = _pictures(geom, dtype)[:B]
    with spiht_amd.StreamEncoder(C3, H, W, _settings(geom), level, MID_BYTE, dtype=dtype, batch=B, depth=2) as enc:
        enc.input()[:B] = np.stack(pics)
        enc.submit(B)
        got = enc.next()
    for p, r in zip(pics, got):
        ref_bytes, ref_n, _ = oracle.encode_image(p / 255.0 if dtype == "uint8" else p, wavelet, mode, level, 50.0, None, MID_BYTE)
        assert (r.encoded_bytes, r.max_n) == (ref_bytes, ref_n)


def test_colour_model_and_channel_scales():
    import spiht_amd
    H, W, level = GEOMS["33x41"][:3]
    s = _settings("33x41", color_model="IPT", quantization_scale=80.0, per_channel_quant_scales=[1.0, 0.5, 0.25])
    pics = _pictures("33x41", "float64")[:2 * B + 1]
    want = [spiht_amd.encode_image(p, s, level, 4001) for p in pics]
    plain = spiht_amd.encode_image(pics[0], _settings("33x41"), level, 4001)
    assert plain.encoded_bytes != want[0].encoded_bytes   # the settings matter
    got = list(spiht_amd.encode_images(pics, s, level, 4001, batch=B, depth=2))
    for r, w in zip(got, want):
        _same(r, w)
    dec = list(spiht_amd.decode_images(got, s, batch=B, depth=2))
    for d, w in zip(dec, want):
        assert np.array_equal(d, spiht_amd.decode_image(w, s))
    # the context is as it was: no colour model left on it
    _same(spiht_amd.encode_image(pics[0], _settings("33x41"), level, 4001), plain)


def _single_decode(r, s, dtype):
    import spiht_amd
    if dtype == "float64":
        return spiht_amd.decode_image(r, s)
    if dtype == "uint8":
        return spiht_amd.decode_image_u8(r, s)
    if dtype == "uint16":
        return spiht_amd.decode_image_u16(r, s)
    return spiht_amd.decode_image_float(r, s, dtype)


@pytest.mark.parametrize("dtype,geom,depth", [("float64", "33x41", 3), ("uint8", "33x41", 2), ("uint16", "16x24", 3), ("float16", "33x41", 2),
                                              ("float64", "16x24", 2), ("uint8", "33x41-per", 3), ("float64", "33x41-per", 2)])
def test_stream_decoder_equals_single_picture_calls(dtype, geom, depth):
    import spiht_amd
    H, W, level = GEOMS[geom][:3]
    s = _settings(geom)
    # streams of several lengths: the budgeted ones and, every third, the whole stream
    res = [a if k % 3 else b for k, (a, b) in enumerate(zip(_single_encodes(geom, "float64", MID_BYTE), _single_encodes(geom, "float64", None)))]
    want = [_single_decode(r, s, dtype) for r in res]
    lists = [list(res[i:i + B]) for i in range(0, len(res), B)]
    with spiht_amd.StreamDecoder(C3, H, W, s, level, dtype=dtype, batch=B, depth=depth) as dec:
        got = list(dec.run(lists))
    assert [len(g) for g in got] == [B] * (STEPS - 1) + [1]
    flat = np.concatenate(got)
    assert flat.dtype == want[0].dtype and flat.shape[1:] == want[0].shape
    for d, w in zip(flat, want):
        assert np.array_equal(d.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))   # every bit
    fn = {"float64": spiht_amd.decode_images, "uint8": spiht_amd.decode_images_u8, "uint16": spiht_amd.decode_images_u16}.get(dtype)
    kw = {} if fn else dict(dtype=dtype)
    out = list((fn or spiht_amd.decode_images_float)(iter(res[:5]), s, batch=2, depth=depth, max_bytes=max(len(r.encoded_bytes) for r in res), **kw))
    assert len(out) == 5 and all(np.array_equal(o, w) for o, w in zip(out, want))


@pytest.mark.parametrize("dtype", ["float64", "uint8"])
def test_decoder_device_destination(dtype):
    import spiht_amd
    from spiht_amd.batch import DeviceArray
    geom = "33x41"
    H, W, level = GEOMS[geom][:3]
    s = _settings(geom)
    res = list(_single_encodes(geom, "float64", MID_BYTE)[:2 * B])
    want = np.stack([_single_decode(r, s, dtype) for r in res])
    with spiht_amd.StreamDecoder(C3, H, W, s, level, dtype=dtype, batch=B, depth=2) as dec:
        d_out = [DeviceArray(dec.ctx, want[:B].shape, want.dtype) for _ in range(2)]
        try:
            for k in range(2):
                dec.put(res[k * B:(k + 1) * B], device_out=d_out[k].ptr)
            assert dec.next() is None and dec.next() is None   # nothing comes to the host; the pictures are complete
            got = np.concatenate([d.download() for d in d_out])   # one download each
        finally:
            for d in d_out:
                d.free()
    assert np.array_equal(got, want)


def test_full_ring_is_busy_and_changes_nothing():
    import spiht_amd
    from spiht_amd import hoststream as hs
    geom, dtype = "16x24", "uint8"
    H, W, level = GEOMS[geom][:3]
    pics, want = _pictures(geom, dtype), _single_encodes(geom, dtype, None)
    with spiht_amd.StreamEncoder(C3, H, W, _settings(geom), level, None, dtype=dtype, batch=B, depth=2) as enc:
        with pytest.raises(hs.StreamIdle):
            enc.next(30.0)   # nothing submitted: at once, with its own status, whatever the time allowed
        for k in range(2):
            enc.input()[:B] = np.stack(pics[k * B:(k + 1) * B])
            enc.submit(B)
        with pytest.raises(hs.StreamBusy):
            enc.input()
        with pytest.raises(hs.StreamBusy):
            enc.submit(B)
        assert enc.pending() == 2 and enc._be.pending() == 2
        try:
            first = enc.next(0)   # one look: done already, or a timeout that leaves the stream as it was
        except hs.StreamTimeout:
            assert enc.pending() == 2 and enc._be.pending() == 2
            first = enc.next()
        staging = enc.input()   # after one next the same calls pass
        staging[:B] = np.stack(pics[2 * B:3 * B])
        assert enc.input().ctypes.data == staging.ctypes.data   # asked again before the submit: the same buffer
        enc.submit(B)
        got = first + enc.next() + enc.next()
        with pytest.raises(hs.StreamIdle):
            enc.next(0)
        with pytest.raises(ValueError):   # a submit without an input, on a ring with room
            enc.submit(B)
    for r, w in zip(got, want):
        _same(r, w)


def test_results_stay_until_their_slot_is_reissued():
    import spiht_amd
    geom, dtype = "16x24", "uint8"
    H, W, level = GEOMS[geom][:3]
    pics, want = _pictures(geom, dtype), _single_encodes(geom, dtype, None)
    step = lambda k: np.stack(pics[k * B:(k + 1) * B])
    packed = lambda k: b"".join(w.encoded_bytes for w in want[k * B:(k + 1) * B])
    with spiht_amd.StreamEncoder(C3, H, W, _settings(geom), level, None, dtype=dtype, batch=B, depth=3) as enc:
        for k in range(2):
            enc.input()[:B] = step(k)
            enc.submit(B)
        data, lens, max_n = enc.next(raw=True)   # step 0, on slot 0: views of the page-locked output
        sentinel = (data.tobytes(), lens.tobytes(), max_n.tobytes())
        assert sentinel[0] == packed(0) and lens.tolist() == [len(w.encoded_bytes) for w in want[:B]]
        enc.input()[:B] = step(2)   # slot 2
        enc.submit(B)
        assert enc.next(raw=True)[0].tobytes() == packed(1)   # step 1 is through, step 2 at least queued
        assert (data.tobytes(), lens.tobytes(), max_n.tobytes()) == sentinel   # unchanged after the following submit
        enc.input()[:B] = step(3)   # slot 0 again: re-issued
        enc.submit(B)
        assert enc.next(raw=True)[0].tobytes() == packed(2)
        d3 = enc.next(raw=True)[0]   # step 3 has come out through slot 0's staging
        assert d3.tobytes() == packed(3) and d3.ctypes.data == data.ctypes.data
        assert (data.tobytes(), lens.tobytes(), max_n.tobytes()) != sentinel   # ... and only now have the bytes changed


def test_destroy_with_steps_queued_then_the_context_works(oracle):
    import spiht_amd
    geom = "33x41"
    H, W, level, wavelet, mode = GEOMS[geom]
    pics = _pictures(geom, "float64")
    enc = spiht_amd.StreamEncoder(C3, H, W, _settings(geom), level, MID_BYTE, dtype="float64", batch=B, depth=3)
    for k in range(2):
        enc.input()[:B] = np.stack(pics[k * B:(k + 1) * B])
        enc.submit(B)
    enc.input()   # ... and a slot handed out and never submitted on top
    enc.close()   # two steps queued, none taken
    dec = spiht_amd.StreamDecoder(C3, H, W, _settings(geom), level, dtype="uint8", batch=B, depth=2)
    dec.put(list(_single_encodes(geom, "float64", MID_BYTE)[:B]))
    dec.close()
    # an ordinary round trip on the same context, against the oracle
    r = spiht_amd.encode_image(pics[4], _settings(geom), level, MID_BYTE)
    ref_bytes, ref_n, _ = oracle.encode_image(pics[4], wavelet, mode, level, 50.0, None, MID_BYTE)
    assert (r.encoded_bytes, r.max_n) == (ref_bytes, ref_n)
    ref = oracle.decode_image(ref_bytes, ref_n, C3, H, W, wavelet, level, 50.0, None)
    assert np.array_equal(spiht_amd.decode_image(r, _settings(geom)), ref)


def test_encoder_feeds_decoder_on_one_context():
    import spiht_amd
    from spiht_amd import _lib
    geom = "33x41"
    H, W, level = GEOMS[geom][:3]
    s = _settings(geom)
    pics = _pictures(geom, "float64")
    want = [spiht_amd.decode_image(w, s) for w in _single_encodes(geom, "float64", MID_BYTE)]
    ctx = _lib.default_context()
    got = []
    with spiht_amd.StreamEncoder(C3, H, W, s, level, MID_BYTE, dtype="float64", batch=B, depth=2, ctx=ctx) as enc, \
            spiht_amd.StreamDecoder(C3, H, W, s, level, dtype="float64", batch=B, depth=2, ctx=ctx, max_bytes=(MID_BYTE + 7) // 8) as dec:
        for batch in _batches(pics):   # alternating: a step in, and as soon as the encoder is full its oldest result on to the decoder
            if enc.pending() == 2:
                if dec.pending() == 2:
                    got.extend(dec.next())
                dec.put(enc.next())
            enc.input()[:len(batch)] = batch
            enc.submit(len(batch))
        while enc.pending():
            if dec.pending() == 2:
                got.extend(dec.next())
            dec.put(enc.next())
        while dec.pending():
            got.extend(dec.next())
    assert len(got) == NPIC
    for d, w in zip(got, want):
        assert np.array_equal(d, w)


@pytest.mark.parametrize("dtype,geom,depth", [("uint8", "33x41", 2), ("uint16", "16x24", 3), ("float16", "33x41-per", 2)])
def test_strided_staging_channels_last(dtype, geom, depth):
    """the view of the staged pictures by strides (spiht_hstream_create's `strides`): pictures [n, H, W, c] in, out, and at a
    device destination, against the single-picture calls with channels_last"""
    import spiht_amd
    from spiht_amd.batch import DeviceArray
    H, W, level = GEOMS[geom][:3]
    s = _settings(geom)
    hwc = [np.ascontiguousarray(p.transpose(1, 2, 0)) for p in _pictures(geom, dtype)]
    want = _single_encodes(geom, dtype, MID_BYTE)   # (the CHW encodes: the same pictures, the same streams)
    with spiht_amd.StreamEncoder(C3, H, W, s, level, MID_BYTE, dtype=dtype, batch=B, depth=depth, channels_last=True) as enc:
        assert enc.input().shape == (B, H, W, C3)
        got = [r for g in enc.run(_batches(hwc)) for r in g]
    assert len(got) == NPIC
    for r, w in zip(got, want):
        _same(r, w)
    single = {"uint8": spiht_amd.decode_image_u8, "uint16": spiht_amd.decode_image_u16}.get(dtype)
    dec_want = [single(w, s, channels_last=True) if single else spiht_amd.decode_image_float(w, s, dtype, channels_last=True)
                for w in want]
    lists = [list(want[i:i + B]) for i in range(0, NPIC, B)]
    with spiht_amd.StreamDecoder(C3, H, W, s, level, dtype=dtype, batch=B, depth=depth, channels_last=True) as dec:
        pics = np.concatenate(list(dec.run(lists)))
        assert pics.shape == (NPIC, H, W, C3) and pics.dtype == dec_want[0].dtype
        for d, w in zip(pics, dec_want):
            assert np.array_equal(d.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
        # ... and into a device destination laid out the same way, two pictures of a step of three
        d_out = DeviceArray(dec.ctx, (B, H, W, C3), dec_want[0].dtype)
        try:
            d_out.upload(np.full((B, H, W, C3), 7, dec_want[0].dtype).view(dec_want[0].dtype))
            dec.put(list(want[:2]), device_out=d_out.ptr)
            assert dec.next() is None
            on_dev = d_out.download()
        finally:
            d_out.free()
    for d, w in zip(on_dev[:2], dec_want[:2]):
        assert np.array_equal(d.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
    assert np.array_equal(on_dev[2].view(np.uint8), np.full((H, W, C3), 7, dec_want[0].dtype).view(np.uint8))   # not written

