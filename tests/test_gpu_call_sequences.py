"""What a call leaves behind on its context: the internal decoder array that is kept all-zero between fused decodes, the
cached channel scales and long filters, the record of the last list decode, the persistent inverse's tile counters, the
colour model, the decoder width and the options, the latched error word, and every scratch buffer that grows by being
freed and allocated again.  A stale value in any of them gives wrong pixels or a wrong stream and no error.  Each case
disturbs one named piece of state, compares the disturbing call's own results with the CPU oracle wherever the oracle
defines them, and then runs the probe -- one small fused round trip with known answers -- which must still be the
oracle's, bit for bit.  Cases: tests/call_sequence_cases.py (held to their purpose by tests/test_call_sequence_cases.py).
Unless it says otherwise a case runs on a context of its own."""
import ctypes as C

import numpy as np
import pytest

import call_sequence_cases as K
import dwt_sweep_tables as T
from test_gpu_batch_chunks import Scope, ids, same_batch
from test_gpu_coder_edges import _slots
from test_gpu_reduced import want_reduced

pytestmark = pytest.mark.gpu
vp = C.c_void_p


def codec_for(k, ctx, mults=None, c=None, dtype=np.float64):
    import spiht_amd
    from spiht_amd.batch import BatchCodec
    s = spiht_amd.SpihtSettings(wavelet=k["wavelet"], quantization_scale=k["q"], mode=k["mode"], per_channel_quant_scales=mults)
    return BatchCodec(k["c"] if c is None else c, k["H"], k["W"], s, k["level"], k["max_bits"], ctx=ctx, pixel_dtype=dtype)


def results_of(k, streams, ns):
    import spiht_amd
    return [spiht_amd.EncodingResult(d, k["H"], k["W"], k["c"], int(n), k["level"]) for d, n in zip(streams, ns)]


def streams_same(res, streams, ns, what):
    bad = [b for b, r in enumerate(res) if r.encoded_bytes != streams[b] or r.max_n != int(ns[b])]
    assert not bad, "%s: %d of %d streams differ, first %s" % (what, len(bad), len(res), bad[:8])


def roundtrip(O, ctx, k, imgs, what, ref=None):
    """encode_image_batch and decode_image_batch (internal array) of imgs under case k, both against the oracle"""
    streams, ns, pics, _ = ref or K.image_reference(O, k, imgs)
    codec = codec_for(k, ctx)
    res = codec.encode(imgs)
    streams_same(res, streams, ns, what)
    same_batch(codec.decode(res), pics, what + ": pictures")
    return res


def probe(O, ctx, after):
    ref = K.probe_reference(O)
    roundtrip(O, ctx, K.PROBE, ref[0], "the probe after " + after, ref[1:])


def empty_probe(O, ctx, k, after):
    """B empty streams of case k's geometry through the fused decode: the pictures are what the oracle makes of nothing, so
    every band cell of the internal array that the last call left dirty shows"""
    res = results_of(k, [b""] * k["B"], [0] * k["B"])
    same_batch(codec_for(k, ctx).decode(res), K.decoded_pictures(O, k, [b""] * k["B"], [0] * k["B"]), "empty streams after " + after)


# ------------------------------------------------------------------------------------------------ the internal decoder array

def test_probe_on_a_fresh_context(oracle):
    with Scope() as s:
        probe(oracle, s.ctx, "nothing")
        probe(oracle, s.ctx, "itself")


def test_array_after_a_dense_decode_of_larger_pictures(oracle):
    """the buffer grows (its capacity changes: zero-filled anew) and nearly every cell is written; the probe before it, so
    that the growth happens to an array in use"""
    with Scope() as s:
        probe(oracle, s.ctx, "nothing")
        roundtrip(oracle, s.ctx, K.DENSE, K.pictures(K.DENSE, 4200), "dense")
        probe(oracle, s.ctx, "a dense decode")
        empty_probe(oracle, s.ctx, K.DENSE, "a dense decode")


def test_array_after_arbitrary_bytes(oracle):
    """byte strings no encoder made through the fused decode on an odd LL block: duplicated cells, and cells no encoder would
    write, padding cells included -- all of them in the decoder's lists, so all of them cleared"""
    k = K.ODD_LL
    streams, ns = K.arbitrary_streams(k["B"])
    with Scope() as s:
        codec = codec_for(k, s.ctx)
        same_batch(codec.decode(results_of(k, streams, ns)), K.decoded_pictures(oracle, k, streams, ns), "arbitrary bytes")
        empty_probe(oracle, s.ctx, k, "arbitrary bytes")
        probe(oracle, s.ctx, "arbitrary bytes")


def test_array_after_slot_reuse(oracle):
    """more tiny pictures than the decoder has slots: the lists of the earlier images of a slot are gone, the array cannot be
    cleared through them and is marked dirty"""
    k = K.TINY
    imgs = K.tiny_pictures()
    base = K.image_reference(oracle, k, imgs[:k["distinct"]])
    which = np.arange(k["B"]) % k["distinct"]
    ref = ([base[0][i] for i in which], [base[1][i] for i in which], base[2][which], None)
    with Scope() as s:
        assert k["B"] > 8 * s.ctx.get_option("num_cu")
        probe(oracle, s.ctx, "nothing")
        roundtrip(oracle, s.ctx, k, imgs, "tiny pictures", ref)
        probe(oracle, s.ctx, "slot reuse")
        empty_probe(oracle, s.ctx, k, "slot reuse")


def test_array_after_reduced_decodes(oracle):
    """reduce = 1, 2 and L: the decoder writes all over the array, the inverse reads a corner of it"""
    k = K.PROBE
    imgs, streams, ns, pics, recs = K.probe_reference(oracle)
    L = oracle.geometry(k["H"], k["W"], k["wavelet"], k["level"], k["mode"])["level"]
    assert L >= 3
    with Scope() as s:
        codec = codec_for(k, s.ctx)
        res = results_of(k, streams, ns)
        for r in (1, 2, L):
            want = np.stack([want_reduced(oracle, rec, k["H"], k["W"], k["wavelet"], L, k["mode"], r, k["q"], None) for rec in recs])
            same_batch(codec.decode_reduced(res, r), want, "reduce = %d" % r)
            probe(oracle, s.ctx, "a decode at reduce = %d" % r)


def test_small_large_small_on_a_fresh_context(oracle):
    """every scratch buffer grows by being freed and allocated again, with work of the smaller size just queued"""
    with Scope() as s:
        small, dense = K.pictures(K.SMALL, 4300), K.pictures(K.DENSE, 4200)
        roundtrip(oracle, s.ctx, K.SMALL, small, "small")
        roundtrip(oracle, s.ctx, K.DENSE, dense, "large")
        roundtrip(oracle, s.ctx, K.SMALL, small, "small again")
        probe(oracle, s.ctx, "small, large, small")


# ------------------------------------------------------------------------------------------------ the latched error

def bad_batches(O):
    """[(what, streams, nbytes, max_n, slot, bad image)]: the probe's streams twice over, one image with max_n = 31; the same
    with one image whose nbytes exceeds the slot"""
    _, streams, ns, pics, _ = K.probe_reference(O)
    streams, ns = streams * 2, list(ns) * 2
    data, nbytes = _slots(streams)
    slot = data.shape[1]
    n31 = np.array(ns, np.uint8)
    n31[1] = 31
    long = nbytes.copy()
    long[2] = slot + 8
    return [("max_n = 31", data, nbytes, n31, slot, 1), ("nbytes > slot_stride", data, long, np.array(ns, np.uint8), slot, 2)]


def queue_bad_batch(ctx, case, arrays):
    """the fused decode of a bad batch, queued on ctx and not waited for -> the device array of the pictures"""
    from spiht_amd.batch import DeviceArray
    what, data, nbytes, ns, slot, bad = case
    k = K.PROBE
    codec = codec_for(k, ctx)
    ds = [DeviceArray(ctx, a.shape, a.dtype) for a in (data, nbytes, ns)]
    for d, a in zip(ds, (data, nbytes, ns)):
        d.upload(a)
    d_img = DeviceArray(ctx, (len(ns), k["c"], codec.geom["rec_h"], codec.geom["rec_w"]), np.float64)
    arrays += ds + [d_img]
    codec.decode_device(ds[0].ptr, ds[1].ptr, ds[2].ptr, len(ns), d_img.ptr, slot_stride=slot)
    return d_img


def others_are_the_oracles(O, d_img, case):
    pics = K.probe_reference(O)[3]
    got = d_img.download()
    keep = [b for b in range(len(got)) if b != case[5]]
    same_batch(got[keep], np.concatenate([pics, pics])[keep], "the other images of the batch with " + case[0])


def test_latched_error_is_reported_by_synchronize(oracle):
    """synchronize() raises, a second one is clean, the images that tripped no guard are the oracle's, and the probe is
    right: the bad image's cells are in its list and were cleared with the rest"""
    from spiht_amd import _lib
    for case in bad_batches(oracle):
        with Scope() as s:
            d_img = queue_bad_batch(s.ctx, case, s.arrays)
            with pytest.raises(_lib.SpihtHipError):
                s.ctx.synchronize()
            s.ctx.synchronize()
            others_are_the_oracles(oracle, d_img, case)
            probe(oracle, s.ctx, "a latched error (%s)" % case[0])


@pytest.mark.parametrize("single", ["decode", "encode"])
def test_latched_error_is_not_cleared_by_a_single_call(oracle, single):
    """The bad batch with NO synchronize, followed directly by a single call on the same context (the default one: that is
    where spiht.decode / spiht.encode run).  The error is reported exactly once, by that first call that waits for the
    stream; the same call made again works, and a synchronize() after it is clean.  (Before the single calls looked at the
    error word they zeroed it unseen, by the code of stage_stream and spiht_encode_i32 as it was: nothing was raised.)"""
    import spiht_amd
    from spiht_amd import _lib
    ctx = _lib.default_context()
    k = K.UNSCATTER
    geom = (k["c"], k["h"], k["w"], k["ll_h"], k["ll_w"])
    x = K.synth_coeffs(77, *geom)
    d_ref, n_ref = oracle.encode(x, k["ll_h"], k["ll_w"], k["max_bits"])
    r_ref = oracle.decode(d_ref, n_ref, *geom)

    def call():
        if single == "decode":
            assert np.array_equal(spiht_amd.decode(d_ref, n_ref, *geom), r_ref)
        else:
            assert spiht_amd.encode(x, k["ll_h"], k["ll_w"], k["max_bits"]) == (d_ref, n_ref)

    arrays = []
    try:
        ctx.synchronize()
        for case in bad_batches(oracle):
            d_img = queue_bad_batch(ctx, case, arrays)
            with pytest.raises(_lib.SpihtHipError):
                call()
            call()
            ctx.synchronize()  # reported once: nothing is left
            others_are_the_oracles(oracle, d_img, case)
            probe(oracle, ctx, "a latched error reported by a single %s (%s)" % (single, case[0]))
    finally:
        try:
            ctx.synchronize()  # (a failure above must not leave its error to the next test of this context)
        except Exception:
            pass
        for d in arrays:
            d.free()


# ------------------------------------------------------------------------------------------------ cached scales and filters

def test_channel_scales_back_to_back(oracle):
    """upload_mults keeps the last scales: s1, other scales of the same length, s1 again, none, another channel count --
    queued back to back without a synchronize; every stream and picture must be the oracle's"""
    k = K.SCALED
    with Scope() as s:
        runs = []
        for i, (c, mults) in enumerate(K.SCALES):
            kc = dict(k, c=c)
            imgs = K.pictures(kc, 4400 + i)
            codec = codec_for(kc, s.ctx, mults)
            B = k["B"]
            d_img = s.dev(imgs)
            d_out, d_nb, d_mn, d_ny = (s.empty((B, codec.slot_stride), np.uint8), s.empty((B,), np.uint64), s.empty((B,), np.uint8),
                                       s.empty((B,), np.uint64))
            d_pic = s.empty((B, c, codec.geom["rec_h"], codec.geom["rec_w"]), np.float64)
            codec.encode_device(d_img.ptr, B, d_out.ptr, d_nb.ptr, d_mn.ptr)
            codec.nbits_to_nbytes(d_nb.ptr, B, d_ny.ptr)
            codec.decode_device(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_pic.ptr)
            runs.append((kc, mults, imgs, d_out, d_nb, d_mn, d_pic))
        s.ctx.synchronize()
        for i, (kc, mults, imgs, d_out, d_nb, d_mn, d_pic) in enumerate(runs):
            streams, ns, pics, _ = K.image_reference(oracle, kc, imgs, mults)
            out, nb, mn = d_out.download(), d_nb.download(), d_mn.download()
            for b in range(len(imgs)):
                assert (out[b, :(int(nb[b]) + 7) // 8].tobytes(), int(mn[b])) == (streams[b], ns[b]), (i, mults, b)
            same_batch(d_pic.download(), pics, "pictures of run %d, scales %s" % (i, mults))


def test_long_filters_interleaved(oracle):
    """upload_filters keeps the last wavelet's filters on the device for the two-pass levels: db11 and sym11 (22 taps both:
    the device copy keeps its size, only its contents change) and coif4 in single precision (whose float filters are
    separate data), forward and inverse interleaved on one context"""
    k = K.LONG
    B, c, H, W = k["B"], k["c"], k["H"], k["W"]
    imgs = K.pictures(k, 4500)
    with Scope() as s:
        d_img, d_img32 = s.dev(imgs), s.dev(imgs, np.float32)
        want, got = [], []
        order = [("fwd", "db11"), ("inv", "sym11"), ("fwd", "sym11"), ("inv", "db11"), ("f32", "coif4"), ("inv", "db11"), ("fwd", "db11"),
                 ("f32", "coif4"), ("inv", "coif4"), ("f32", "sym11"), ("fwd", "coif4"), ("inv", "sym11")]
        for i, (op, wavelet) in enumerate(order):
            kw = dict(k, wavelet=wavelet)
            wid, mid, lv = ids(kw)
            if op == "inv":
                cases = [T.inverse_case(oracle, wavelet, H, W, lv, 4600 + 10 * i + b, None, c=c) for b in range(B)]
                rec = np.stack([cs[0] for cs in cases])
                want.append(np.stack([cs[1] for cs in cases]))
                d_rec = s.dev(rec)
                d_o = s.empty(want[-1].shape, np.float64)
                s.check(s.L.spiht_dequant_idwt_batch_f64(s.ctx.handle, vp(d_rec.ptr), B, c, H, W, wid, mid, lv, k["q"], None, vp(d_o.ptr)))
            else:
                if op == "fwd":
                    want.append(np.stack([oracle.quantize(oracle.wavedec2_array(im, wavelet, k["mode"], lv)[0], k["q"], None) for im in imgs]))
                else:
                    want.append(np.stack([oracle.quantize_f32(oracle.wavedec2_array_f32(im.astype(np.float32), wavelet, k["mode"], lv)[0],
                                                              k["q"], None) for im in imgs]))
                d_o = s.empty(want[-1].shape, np.int32)
                fn, src = (s.L.spiht_dwt_quant_batch_f64, d_img) if op == "fwd" else (s.L.spiht_dwt_quant_batch_f32, d_img32)
                s.check(fn(s.ctx.handle, vp(src.ptr), B, c, H, W, wid, mid, lv, k["q"], None, vp(d_o.ptr)))
            got.append(d_o)
        s.ctx.synchronize()
        for i, (op, wavelet) in enumerate(order):
            same_batch(got[i].download(), want[i], "step %d: %s %s" % (i, op, wavelet))


# ------------------------------------------------------------------------------------------------ settings of the context

def test_colour_model_after_an_exception_in_the_block(oracle):
    """an exception inside color_models.fused(ctx, "IPT") -- a bad argument to a call of the block -- leaves the context
    without a colour model and unlocked: the probe, in RGB, is the oracle's"""
    from spiht_amd import color_models
    with Scope() as s:
        with pytest.raises(ValueError):
            with color_models.fused(s.ctx, "IPT"):
                s.check(s.L.spiht_dwt_quant_batch_f64(s.ctx.handle, None, 1, 3, 8, 8, 0, 0, 1, 50.0, None, None))
        on = C.c_int(-1)
        s.check(s.L.spiht_ctx_get_color3(s.ctx.handle, C.byref(on), None, None, None, None, None, None))
        assert on.value == 0
        probe(oracle, s.ctx, "an exception in a colour block")


def test_decoder_width_and_flags_alternating(oracle):
    """8 / 12 wavefronts and occupancy words off / on, alternating on one geometry and one context: the same bits, the
    oracle's"""
    k = K.WIDTHS
    imgs = K.pictures(k, 4700)
    ref = K.image_reference(oracle, k, imgs)
    with Scope() as s:
        for waves, flags in K.WIDTH_SETTINGS:
            s.ctx.set_decoder_waves(waves)
            s.ctx.set_option("l1_flags", flags)
            roundtrip(oracle, s.ctx, k, imgs, "%d wavefronts, l1_flags %d" % (waves, flags), ref)
        probe(oracle, s.ctx, "the alternation")


def test_tile_counters_of_the_persistent_inverse(oracle):
    """The persistent inverse draws its tiles from counters that are never reset (the launcher tracks where they stand).  The
    persistent case of the sweep four times on one context with 4, 3, 1 and 4 workgroups per CU -- the number of workgroups
    that draw from the counters changes -- and a workgroup-per-tile launch of another geometry between each pair."""
    F = len(oracle.wavelet_filters(K.PF_WAVELET)[0])
    recs, wants, H, W = T.pf_cases(oracle, K.PF_WAVELET, 2, False, True)
    words = T.occupancy_words(recs, H, W, F)
    idx = np.arange(T.PF_PICTURES) % T.PF_DISTINCT
    assert T.pf_tile_count() >= T.PF_MIN
    wid, mid, _ = ids(dict(wavelet=K.PF_WAVELET, mode="reflect", level=2))
    kf, Rf = K.FLAGS, K.flags_reference(oracle)
    fwid, fmid, flv = ids(kf)
    nb = 5
    with Scope() as s:
        d_rec, d_fl = s.dev(recs[idx]), s.dev(words[idx])
        d_small = s.dev(Rf["rec"][:nb])
        outs, smalls = [], []
        for groups in K.PF_GROUPS:
            s.ctx.set_option("idwt_groups", groups)
            d_o = s.empty((T.PF_PICTURES,) + wants.shape[1:], np.float64)
            s.check(s.L.spiht_dequant_idwt_flags_batch_f64(s.ctx.handle, vp(d_rec.ptr), vp(d_fl.ptr), T.PF_PICTURES, 3, H, W, wid, mid, 2,
                                                           T.Q, None, vp(d_o.ptr)))
            outs.append(d_o)
            d_s = s.empty(Rf["pics"][:nb].shape, np.float64)
            s.check(s.L.spiht_dequant_idwt_batch_f64(s.ctx.handle, vp(d_small.ptr), nb, kf["c"], kf["H"], kf["W"], fwid, fmid, flv, kf["q"],
                                                     None, vp(d_s.ptr)))
            smalls.append(d_s)
        s.ctx.synchronize()
        for i, groups in enumerate(K.PF_GROUPS):
            same_batch(outs[i].download(), wants[idx], "run %d, %d workgroups per CU" % (i, groups))
            same_batch(smalls[i].download(), Rf["pics"][:nb], "the small launch after run %d" % i)


# ------------------------------------------------------------------------------------------------ the record of the last list decode

@pytest.mark.parametrize("fallback", ["other_array", "other_batch_size"])
def test_unscatter_falls_back_to_the_fill(oracle, fallback):
    """spiht_unscatter_lists_batch_i32 clears through the lists of the context's LAST list decode; when that was a decode into
    another array, or of another batch size, the lists do not describe this array and the call has to zero-fill it.  The
    array is all zero afterwards, and the next decode into it is exact."""
    k = K.UNSCATTER
    B, c, h, w, lh, lw, mb = (k[x] for x in ("B", "c", "h", "w", "ll_h", "ll_w", "max_bits"))
    xs = [K.synth_coeffs(900 + b, c, h, w, lh, lw) for b in range(2 * B)]
    enc = [oracle.encode(x, lh, lw, mb) for x in xs]
    rec = np.stack([oracle.decode(d, n, c, h, w, lh, lw) for d, n in enc]).reshape(2 * B, -1)
    data, nbytes = _slots([d for d, _ in enc])
    slot = data.shape[1]
    n = c * h * w
    with Scope() as s:
        d_data, d_ny, d_mn = s.dev(data), s.dev(nbytes), s.dev(np.array([m for _, m in enc], np.uint8))
        d_a, d_b = s.zeros((B, n), np.int32), s.zeros((B, n), np.int32)

        def decode(d_to, first, count):
            s.check(s.L.spiht_decode_lists_batch_i32(s.ctx.handle, vp(d_data.ptr + first * slot), slot, vp(d_ny.ptr + 8 * first),
                                                     vp(d_mn.ptr + first), count, c, h, w, lh, lw, vp(d_to.ptr)))

        def unscatter(d_to, count):
            s.check(s.L.spiht_unscatter_lists_batch_i32(s.ctx.handle, vp(d_to.ptr), count, c, h, w))

        if fallback == "other_array":
            decode(d_a, 0, B)
            decode(d_b, B, B)
            s.ctx.synchronize()
            assert np.array_equal(d_a.download(), rec[:B]) and np.array_equal(d_b.download(), rec[B:])
            unscatter(d_a, B)  # the lists are those of d_b's decode
            unscatter(d_b, B)  # ... and this one goes through them
        else:
            decode(d_a, 0, B - 1)  # (the last image of the array stays zero)
            s.ctx.synchronize()
            assert np.array_equal(d_a.download()[:B - 1], rec[:B - 1]) and not d_a.download()[B - 1].any()
            unscatter(d_a, B)
        s.ctx.synchronize()
        assert not d_a.download().any() and not d_b.download().any()
        decode(d_a, B, B)
        s.ctx.synchronize()
        assert np.array_equal(d_a.download(), rec[B:])
