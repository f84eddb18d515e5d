"""GPU tests of the host-fed streams (spiht_amd/hoststream.py over include/spiht_hip.h: spiht_hstream_*): every result of a
stream equals the single-picture call's, field by field and bit for bit; the ring's rules hold on the device as they do in the
model.  Shapes are the smallest that still reuse slots (7 steps on 2 or 3 slots), end on a short batch (n = 1) and have an odd
geometry.  No test asserts a time.

What a stream answers to ONE bad argument at _create or _submit is a table (hs_rules) against tests/golden/hstream_status.json:

    python tests/test_gpu_hoststream.py record FILE     writes the JSON from the library that is loaded (GPU; SPIHT_HIP_LIB)
"""
import ctypes as C
import functools
import json
import os
import sys

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


# ---- what a stream answers to one bad argument ------------------------------------------------------------------------------
# A row is (call, element, direction, spoil) -> status.  Every row starts from a spiht_hstream_create that passes -- B = 2, depth 2,
# c = 3, 16 x 16, level 2, bior2.2, reflect -- and spoils what its name says; the _submit rows spoil that call's own arguments on
# a stream that has handed out a slot.  Nothing spoiled lets work be queued: every row is refused before the first copy.  The
# expected statuses (tests/golden/hstream_status.json) were recorded by running this table on the GPU against the library of the
# commit before the stream kept its element as a PicElem; rows that library did not refuse are not in the table (HS_NOT_REFUSED).
HS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hstream_status.json")
HS_ELEMS = {"f64": (0, 8), "u8": (1, 1), "u16": (2, 2), "flt32": (3, 4), "flt16": (4, 2), "bf16": (5, 2)}   # SPIHT_HS_*: id, bytes
HS_DIRS = {"enc": 0, "dec": 1}
HS_B, HS_DEPTH, HS_C, HS_H, HS_W, HS_LEVEL = 2, 2, 3, 16, 16, 2
HS_CREATE = ["elem", "f64_strides", "neg_stride", "odd_stride", "overlap", "c0", "B65536", "wavelet", "mode", "depth_lo", "depth_hi"]
HS_SUBMIT = ["n0", "n_over", "dst_on_encoder", "dst_misaligned"]
HS_NOT_REFUSED = set()


def hs_spoils(call, elem, d):
    es, out = HS_ELEMS[elem][1], []
    for s in (HS_CREATE if call == "create" else HS_SUBMIT):
        if s == "f64_strides" and elem != "f64":
            continue  # (dense strides are a valid view of every other element)
        if s in ("neg_stride", "odd_stride", "overlap") and elem == "f64":
            continue  # (float64 takes no strides at all: f64_strides)
        if s == "odd_stride" and es == 1:
            continue
        if s == "overlap" and d != "dec":
            continue  # (an encoder only reads its view)
        if s == "dst_on_encoder" and d != "enc":
            continue
        if s == "dst_misaligned" and (d != "dec" or es == 1):
            continue  # (a byte is always aligned)
        out.append(s)
    return out


def hs_row_id(row):
    return "%s[%s,%s] %s" % row


def hs_rules():
    rows = [(call, e, d, s) for call in ("create", "submit") for e in HS_ELEMS for d in HS_DIRS for s in hs_spoils(call, e, d)]
    return [r for r in rows if hs_row_id(r) not in HS_NOT_REFUSED]


class HsBench:
    def __init__(self, ctx):
        from spiht_amd import _lib
        self.ctx, self.L = ctx, _lib.lib()
        self.wv, self.md = self.L.spiht_wavelet_id(b"bior2.2"), self.L.spiht_mode_id(b"reflect")
        self.dst = ctx.alloc(1 << 16)   # a device destination: four times the largest step (float64 [2, 3, 18, 18])

    def close(self):
        self.ctx.free(self.dst)

    def create(self, elem, d, spoil=None, dense_strides=False):
        eid, es = HS_ELEMS[elem]
        a = dict(elem=eid, B=HS_B, depth=HS_DEPTH, c=HS_C, wavelet=self.wv, mode=self.md)
        st = None
        if dense_strides or spoil in ("f64_strides", "neg_stride", "odd_stride", "overlap"):
            st = (C.c_int64 * 4)(HS_C * HS_H * HS_W * es, HS_H * HS_W * es, HS_W * es, es)
        if spoil == "neg_stride":
            st[3] = -es
        elif spoil == "odd_stride":
            st[2] += 1
        elif spoil == "overlap":
            st[2] = es   # rows on top of one another
        elif spoil and spoil != "f64_strides":
            key, bad = {"elem": ("elem", 6), "c0": ("c", 0), "B65536": ("B", 65536), "wavelet": ("wavelet", 1000), "mode": ("mode", 9),
                        "depth_lo": ("depth", 1), "depth_hi": ("depth", 5)}[spoil]
            a[key] = bad
        h = C.c_void_p()
        status = self.L.spiht_hstream_create(self.ctx.handle, HS_DIRS[d], a["elem"], a["B"], a["depth"], a["c"], HS_H, HS_W, a["wavelet"],
                                             a["mode"], HS_LEVEL, 50.0, None, 16384, C.addressof(st) if st else None, C.byref(h))
        return int(status), h

    def create_row(self, elem, d, spoil):
        status, h = self.create(elem, d, spoil)
        if h.value:   # (not refused: the stream exists)
            self.L.spiht_hstream_destroy(h)
        return status

    def submit_rows(self, elem, d, spoils, base):
        """the statuses of the spoiled submits of one stream; into base: the valid calls around them, and what is queued after"""
        L, key = self.L, "[%s,%s]" % (elem, d)
        base["create" + key], h = self.create(elem, d)
        if base["create" + key] != 0:
            return {}
        if d == "dec":   # (no lengths of a stream that were never written, should a row not be refused)
            ln, mx = C.c_void_p(), C.c_void_p()
            base["input" + key] = int(L.spiht_hstream_decode_input(h, None, C.byref(ln), C.byref(mx)))
            C.memset(ln, 0, HS_B * 4)
            C.memset(mx, 0, HS_B)
        else:
            p = C.c_void_p()
            base["input" + key] = int(L.spiht_hstream_input(h, C.byref(p)))
        args = {"n0": (0, None), "n_over": (HS_B + 1, None), "dst_on_encoder": (HS_B, self.dst), "dst_misaligned": (HS_B, self.dst + 1)}
        out = {s: int(L.spiht_hstream_submit(h, *args[s])) for s in spoils}
        pending = C.c_int(-1)
        L.spiht_hstream_pending(h, C.byref(pending))
        base["pending" + key] = pending.value   # nothing was queued
        base["destroy" + key] = int(L.spiht_hstream_destroy(h))
        return out


def hs_run_table(ctx):
    b = HsBench(ctx)
    try:
        base, got = {}, {}
        for e in HS_ELEMS:
            for d in HS_DIRS:
                if e != "f64":   # the valid view the stride rows are spoiled from
                    st, h = b.create(e, d, dense_strides=True)
                    base["create[%s,%s] dense_strides" % (e, d)] = st
                    if h.value:
                        b.L.spiht_hstream_destroy(h)
                sub = b.submit_rows(e, d, [r[3] for r in hs_rules() if r[:3] == ("submit", e, d)], base)
                got.update({hs_row_id(("submit", e, d, s)): v for s, v in sub.items()})
        for r in hs_rules():
            if r[0] == "create":
                got[hs_row_id(r)] = b.create_row(*r[1:])
    finally:
        b.close()
    return base, got


def test_status_of_every_refused_create_and_submit():
    from spiht_amd import _lib
    with open(HS_GOLDEN) as fh:  # {"call[element,direction]": {"spoil": status}}, one line per call and stream
        want = {"%s %s" % (k, sp): v for k, m in json.load(fh).items() for sp, v in m.items()}
    base, got = hs_run_table(_lib.default_context())
    assert {k: v for k, v in base.items() if v != 0} == {}, "a valid call was refused, or a refused submit queued a step"
    assert sorted(got) == sorted(want), "the table and the recorded rows differ"
    assert all(v != 0 for v in want.values())
    assert 4 * len(HS_NOT_REFUSED) <= len(HS_NOT_REFUSED) + len(want)   # at most a quarter of the rows is left out
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    for k, (g, w) in sorted(diff.items()):
        print("%s: returned %d, recorded %d" % (k, g, w))
    assert not diff


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    from spiht_amd import _lib as _l
    base_, got_ = hs_run_table(_l.default_context())
    print("library:", _l.LIB_PATH)
    print("valid calls refused / steps queued:", {k: v for k, v in base_.items() if v})
    print("not refused:", sorted(k for k, v in got_.items() if v == 0))
    rows_ = {}
    for k_, v_ in sorted(got_.items()):
        if v_ != 0:
            rows_.setdefault(k_.split(" ")[0], {})[k_.split(" ")[1]] = v_
    with open(sys.argv[2], "w") as fh:
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(s_), json.dumps(m_, separators=(",", ":"))) for s_, m_ in rows_.items()) + "\n}\n")

