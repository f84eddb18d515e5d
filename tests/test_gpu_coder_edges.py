"""The SPIHT list coder at the edges a random draw does not land on (cases: tests/coder_edge_cases.py, held to their purpose
by tests/test_coder_edge_cases.py): maxima on every step of the start-plane rule, magnitudes up to 2^30 - 1 and the
refusals beyond, lists driven to their capacities, and batches larger than the slot count in which every image differs.
Every comparison is equality of bytes or of integer arrays with the CPU oracle; every image of every batch is compared and
every batched output lies between two guard regions that must come back untouched."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import coder_edge_cases as E
from conftest import synth_coeffs, synth_image
from test_gpu_metadata import nominal_slices, tree_generations

pytestmark = pytest.mark.gpu
UNLIMITED = E.UNLIMITED
GUARD = 0x7F
vp = C.c_void_p
_REF = {}  # oracle results, shared between the cases of a test (narrow / wide coder, 12 / 8 wavefronts)

# coder: (wide_groups, wide_solo) -- wide_solo 0: the group of workgroups takes over in the first plane (the empty one of a
# band maximum), 40: a few planes later
CODERS = {"narrow": None, "wide2": (2, 0), "wide5": (5, 40)}


def _ref(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _ref_encode(O, x, lh, lw, mb):
    return _ref(("enc", x.shape, x.tobytes(), lh, lw, mb), lambda: O.encode_nbits(x, lh, lw, mb))


def _ref_decode(O, d, n, geom):
    r = _ref(("dec", bytes(d), int(n), geom), lambda: O.decode(d, n, *geom))
    r.flags.writeable = False
    return r


@contextlib.contextmanager
def _coder(name):
    from spiht_amd import _lib
    ctx = _lib.default_context()
    try:
        if CODERS[name] is not None:
            ctx.set_option("wide_encode", 2)
            ctx.set_option("wide_groups", CODERS[name][0])
            ctx.set_option("wide_solo", CODERS[name][1])
        yield ctx
    finally:
        ctx.set_option("wide_encode", 1)
        ctx.set_option("wide_groups", 0)
        ctx.set_option("wide_solo", 24576)


@contextlib.contextmanager
def _waves(w):
    from spiht_amd import _lib
    ctx = _lib.default_context()
    try:
        ctx.set_decoder_waves(w)
        yield ctx
    finally:
        ctx.set_decoder_waves(12)


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.asarray(got) != np.asarray(want))
        raise AssertionError("%s: %d cells differ, first %s: got %d want %d"
                             % (what, len(bad), bad[0], np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])]))


def _check_encode(O, x, lh, lw, mb, what):
    import spiht_amd
    d_ref, n_ref, nb_ref = _ref_encode(O, x, lh, lw, mb)
    d, n = spiht_amd.encode(x, lh, lw, mb)
    assert n == n_ref, "%s: max_n %d, oracle %d" % (what, n, n_ref)
    assert len(d) == len(d_ref) == (nb_ref + 7) // 8, "%s: %d bytes, oracle %d" % (what, len(d), len(d_ref))
    if d != d_ref:
        a, b = np.frombuffer(d, np.uint8), np.frombuffer(d_ref, np.uint8)
        raise AssertionError("%s: stream differs at byte %d of %d" % (what, int(np.nonzero(a != b)[0][0]), len(d)))
    return d, n


def _check_decode(O, d, n, geom, what):
    import spiht_amd
    r = spiht_amd.decode(d, n, *geom)
    assert r.dtype == np.int32 and r.shape == geom[:3]
    _same(r, _ref_decode(O, d, n, geom), what)
    return r


def _roundtrip(O, x, geom, mb, what, coded=None):
    """stream, max_n and decoded array against the oracle; coded: the budget is unlimited -- the array comes back"""
    d, n = _check_encode(O, x, geom[3], geom[4], mb, what)
    r = _check_decode(O, d, n, geom, what)
    if coded is not None:
        _same(r[coded], x[coded], what + " (not lossless)")
        assert not r[~coded].any()
    return d, n


def _dev(ctx, arr):
    from spiht_amd.batch import DeviceArray
    d = DeviceArray(ctx, arr.shape, arr.dtype)
    d.upload(arr)
    return d


def _guarded(ctx, shape, dtype):
    """a device array of shape[0] + 2 rows filled with the guard byte: the call gets the rows 1 .. shape[0]"""
    from spiht_amd.batch import DeviceArray
    d = DeviceArray(ctx, (shape[0] + 2,) + tuple(shape[1:]), dtype)
    ctx.memset(d.ptr, GUARD, d.nbytes)
    return d, d.ptr + d.nbytes // (shape[0] + 2)


def _unguard(d, what):
    a = d.download()
    g = np.frombuffer(bytes([GUARD]) * a.dtype.itemsize, a.dtype)[0]
    assert (a[0] == g).all() and (a[-1] == g).all(), "%s: a guard region was written" % what
    return a[1:-1]


def _bound(geom, max_abs=0x3FFFFFFF):
    from spiht_amd import _lib
    b = C.c_uint64()
    _lib.check(_lib.lib().spiht_encode_bound(*geom, max_abs, 0, C.byref(b)))
    return int(b.value) + 4


def _encode_batch(ctx, xs, geom, mb, slot):
    """spiht_encode_batch_i32 with every output between guards -> (slots uint8 [B, slot], nbits [B], max_n [B]) and the
    device arrays (out, nbits, max_n: pointers to row 1), still allocated"""
    from spiht_amd import _lib
    c, h, w, lh, lw = geom
    B = len(xs)
    d_x = _dev(ctx, np.ascontiguousarray(xs, np.int32))
    d_out, p_out = _guarded(ctx, (B, slot), np.uint8)
    d_nb, p_nb = _guarded(ctx, (B,), np.uint64)
    d_mn, p_mn = _guarded(ctx, (B,), np.uint8)
    _lib.check(_lib.lib().spiht_encode_batch_i32(ctx.handle, vp(d_x.ptr), B, c, h, w, lh, lw, mb, vp(p_out), slot, vp(p_nb), vp(p_mn)))
    ctx.synchronize()
    res = (_unguard(d_out, "encoder slots"), _unguard(d_nb, "d_nbits"), _unguard(d_mn, "d_max_n"))
    return res, (d_x, d_out, d_nb, d_mn), (p_out, p_nb, p_mn)


def _check_encoded_batch(O, xs, geom, mb, slot, res, what):
    out, nbits, maxn = res
    c, h, w, lh, lw = geom
    for b in range(len(xs)):
        d_ref, n_ref, nb_ref = _ref_encode(O, xs[b], lh, lw, min(mb, 8 * slot))
        assert (int(nbits[b]), int(maxn[b])) == (nb_ref, n_ref), "%s image %d: %d bits max_n %d, oracle %d / %d" % (
            what, b, nbits[b], maxn[b], nb_ref, n_ref)
        assert out[b, :len(d_ref)].tobytes() == d_ref, "%s image %d: stream differs" % (what, b)
        assert not out[b, len(d_ref):].any(), "%s image %d: bytes past the stream are not zero" % (what, b)


def _decode_batch_ptrs(ctx, p_data, slot, p_nbytes, p_maxn, B, geom, what):
    from spiht_amd import _lib
    c, h, w, lh, lw = geom
    d_rec, p_rec = _guarded(ctx, (B, c * h * w), np.int32)
    _lib.check(_lib.lib().spiht_decode_batch_i32(ctx.handle, vp(p_data), slot, vp(p_nbytes), vp(p_maxn), B, c, h, w, lh, lw, vp(p_rec)))
    ctx.synchronize()
    rec = _unguard(d_rec, what).reshape(B, c, h, w)
    d_rec.free()
    return rec


def _decode_batch(ctx, data, nbytes, ns, geom, what):
    """spiht_decode_batch_i32 of host slots -> int32 [B, c, h, w]; the output lies between two guard images"""
    B, slot = data.shape
    assert slot % 4 == 0
    ds = [_dev(ctx, np.ascontiguousarray(data, np.uint8)), _dev(ctx, np.asarray(nbytes, np.uint64)), _dev(ctx, np.asarray(ns, np.uint8))]
    try:
        return _decode_batch_ptrs(ctx, ds[0].ptr, slot, ds[1].ptr, ds[2].ptr, B, geom, what)
    finally:
        for d in ds:
            d.free()


def _check_decoded_batch(O, rec, data, nbytes, ns, geom, what):
    for b in range(len(rec)):  # every image
        d = data[b, :int(nbytes[b])].tobytes()
        _same(rec[b], _ref_decode(O, d, int(ns[b]), geom), "%s image %d (%d bytes, n=%d)" % (what, b, len(d), ns[b]))


def _slots(streams, slot=None):
    """host slots whose tails past each stream hold 0xFF"""
    slot = slot or max(4, (max(len(d) for d in streams) + 3) & ~3)
    data = np.full((len(streams), slot), 0xFF, np.uint8)
    for b, d in enumerate(streams):
        data[b, :len(d)] = np.frombuffer(d, np.uint8)
    return data, np.array([len(d) for d in streams], np.uint64)


# ------------------------------------------------------------------------------------------------ 1

@pytest.mark.parametrize("part", ["narrow", "wide2", "wide5", "batch", "image"])
def test_start_plane_at_every_threshold(oracle, part):
    """`(max as f32).log2() as u8` through the device's threshold table (encode_common.h: start_plane(), api_ctx.cpp:
    log2_thresh): every maximum around a power of two and around the step of the band below 2^21 .. 2^30, in the root block,
    in a leaf, in the last cell and on a duplicated node, both signs, alone and among small values.  A band maximum starts a
    plane above its top bit: that first plane holds no significant coefficient, and budgets cut inside and just behind it.
    A wrong table entry would show as max_n off by one for the maxima of one band (735 of them below 2^30), and every byte
    of the stream after it."""
    O = oracle
    if part in CODERS:
        with _coder(part):
            for geom in E.SMALL_GEOMS:
                c, h, w, lh, lw = geom
                roots, coded = c * lh * lw, E.coded_cells(O, geom)
                for (m, name, sign, fill), x in E.placed_cases(O, geom, E.plane_maxima(O)):
                    what = "%s %s max %d at %s sign %d fill %d" % (part, geom, m, name, sign, fill)
                    d, n = _roundtrip(O, x, geom, UNLIMITED, what, coded)
                    assert n == O.start_plane(m)
                    if E.in_band(O, m):
                        assert n == m.bit_length()
                        for mb in (1, 2, roots, roots + 1, roots + 7):
                            _roundtrip(O, x, geom, mb, what + " budget %d" % mb)
    elif part == "batch":
        _start_plane_batch(O)
    else:
        _start_plane_image(O)


def _start_plane_batch(O):
    """one spiht_encode_batch_i32 call, a different maximum in every image, an all-zero image between a band maximum and
    the value below it: max_n, bit count and bytes per image; the maxima of spiht_pyramid_batch_i32 (k_absmax) per image"""
    from spiht_amd import _lib
    geom = E.ODD_GEOM
    c, h, w, lh, lw = geom
    pl = E.placements(O, geom)
    vals = E.plane_maxima(O)
    xs, want_max = [], []
    for t, m in enumerate(vals):
        xs.append(E.placed(geom, pl[t % len(pl)][1], m, 1 if t % 3 else -1, t % 4 != 0))
        want_max.append(m)
        if m + 1 == E.band(O, 24)[0]:
            xs.append(np.zeros((c, h, w), np.int32))
            want_max.append(0)
    xs = np.stack(xs)
    B = len(xs)
    assert B == len(vals) + 1 and any(E.in_band(O, a) != E.in_band(O, b) for a, b in zip(want_max, want_max[1:]))
    ctx = _lib.default_context()
    slot = _bound(geom)
    res, devs, (p_out, p_nb, p_mn) = _encode_batch(ctx, xs, geom, UNLIMITED, slot)
    _check_encoded_batch(O, xs, geom, UNLIMITED, slot, res, "batch of maxima")
    assert [int(v) for v in res[2]] == [O.start_plane(m) for m in want_max]
    d_dm, d_lm = _dev(ctx, np.zeros((B, c * h * w), np.uint8)), _dev(ctx, np.zeros((B, c * h * w), np.uint8))
    d_mx, p_mx = _guarded(ctx, (B,), np.uint32)
    _lib.check(_lib.lib().spiht_pyramid_batch_i32(ctx.handle, vp(devs[0].ptr), B, c, h, w, lh, lw, vp(d_dm.ptr), vp(d_lm.ptr), vp(p_mx)))
    ctx.synchronize()
    assert [int(v) for v in _unguard(d_mx, "d_mx")] == want_max
    # ... and back through the batched decoder, from where the streams lie
    d_ny = _dev(ctx, np.zeros(B, np.uint64))
    _lib.check(_lib.lib().spiht_nbits_to_nbytes(ctx.handle, vp(p_nb), B, vp(d_ny.ptr)))
    rec = _decode_batch_ptrs(ctx, p_out, slot, d_ny.ptr, p_mn, B, geom, "decode of the batch of maxima")
    coded = E.coded_cells(O, geom)
    for b in range(B):
        _same(rec[b][coded], xs[b][coded], "image %d" % b)
        assert not rec[b][~coded].any()
    for d in devs + (d_dm, d_lm, d_mx, d_ny):
        d.free()


def _start_plane_image(O):
    """the maximum reduced inside the transform kernels (the image path never runs k_absmax): a picture whose largest
    quantised coefficient is the first value of the band below 2^24, and of the band below 2^27"""
    import spiht_amd
    img = synth_image(77, 1, 32, 40)
    arr, g = O.wavedec2_array(img, "haar", "reflect", 2)
    for k in (24, 27):
        first = E.band(O, k)[0]
        q = (first + 0.5) / float(np.abs(arr).max())
        coeffs = O.quantize(arr, q)
        assert int(np.abs(coeffs.astype(np.int64)).max()) == first and O.start_plane(first) == k == first.bit_length()
        s = spiht_amd.SpihtSettings(wavelet="haar", quantization_scale=q, mode="reflect")
        ref_bytes, ref_n, _ = O.encode_image(img, "haar", "reflect", 2, q, None, None)
        assert ref_n == k
        enc = spiht_amd.encode_image(img, s, level=2)
        assert enc.max_n == ref_n and enc.encoded_bytes == ref_bytes, "k=%d: max_n %d, oracle %d" % (k, enc.max_n, ref_n)
        dec = spiht_amd.decode_image(enc, s)
        ref = O.decode_image(ref_bytes, ref_n, 1, 32, 40, "haar", 2, q, None)
        assert dec.shape == ref.shape and np.array_equal(dec, ref), k


# ------------------------------------------------------------------------------------------------ 2

def _limit_maxima(O):
    return [1 << 29, (1 << 29) + 1, E.band(O, 30)[0] - 1, (1 << 30) - 1]


def _limit_arrays(O, geom):
    """[(what, array)]: every placement of each maximum, and a dense array of values up to it (every plane busy)"""
    out = []
    for m in _limit_maxima(O):
        for key, x in E.placed_cases(O, geom, [m]):
            out.append(("max %d at %s sign %d fill %d" % key, x))
        x = np.random.default_rng(m % 1000).integers(-m, m + 1, geom[:3]).astype(np.int32)
        x[0, 0, 1] = -m
        out.append(("dense up to %d" % m, x))
    return out


@pytest.mark.parametrize("part", ["narrow", "wide2", "wide5", "batch", "decode12", "decode8", "refusals"])
def test_magnitudes_up_to_the_limit(oracle, part):
    """Magnitudes in [2^29, 2^30) are accepted: 2^30 - 1 lies in the band below 2^30 and starts at plane 30, where a
    decoded value reaches 2^31 - 1.  Encoder (one workgroup, several, batched) and decoder (decode, decode_budgets,
    decode_with_metadata, both widths) at n = 30 and 29; everything from 2^30 on, INT32_MIN included, is refused with the
    error of SPIHT_ERR_MAGNITUDE, by the single call and by synchronize() after the batched one; n above 30 is refused by
    decode() and reported by synchronize() after the batched decoder.  Every refusal leaves the context usable.  A wrong plane 30 would show as an overflowed sign or a lost top bit in the decoded array."""
    O = oracle
    geoms = E.SMALL_GEOMS + [E.MID_GEOM]
    assert _limit_maxima(O)[2] == (1 << 30) - 1 - len(E.band(O, 30)) and O.start_plane((1 << 30) - 1) == 30
    if part in CODERS:
        with _coder(part):
            for geom in geoms:
                coded = E.coded_cells(O, geom)
                for what, x in _limit_arrays(O, geom):
                    what = "%s %s %s" % (part, geom, what)
                    _roundtrip(O, x, geom, UNLIMITED, what, coded)
                    if what.find("dense") >= 0:
                        total = _ref_encode(O, x, geom[3], geom[4], UNLIMITED)[2]
                        for mb in (97, total // 2, total - 1):
                            _roundtrip(O, x, geom, mb, what + " budget %d" % mb)
    elif part == "batch":
        from spiht_amd import _lib
        ctx = _lib.default_context()
        for geom in geoms:
            xs = np.stack([x for _, x in _limit_arrays(O, geom)])
            B, slot = len(xs), _bound(geom)
            assert B > 1
            res, devs, (p_out, p_nb, p_mn) = _encode_batch(ctx, xs, geom, UNLIMITED, slot)
            _check_encoded_batch(O, xs, geom, UNLIMITED, slot, res, "batch %s" % (geom,))
            d_ny = _dev(ctx, np.zeros(B, np.uint64))
            _lib.check(_lib.lib().spiht_nbits_to_nbytes(ctx.handle, vp(p_nb), B, vp(d_ny.ptr)))
            rec = _decode_batch_ptrs(ctx, p_out, slot, d_ny.ptr, p_mn, B, geom, "decode of the batch")
            coded = E.coded_cells(O, geom)
            for b in range(B):
                _same(rec[b][coded], xs[b][coded], "%s image %d" % (geom, b))
                assert not rec[b][~coded].any()
            for d in devs + (d_ny,):
                d.free()
    elif part.startswith("decode"):
        with _waves(int(part[6:])):
            _decode_at_the_limit(O, geoms)
    else:
        _refusals(O)


def _hostile_streams():
    rng = np.random.default_rng(29)
    out = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (1, 3, 17, 200, 1500)]
    out += [(rng.integers(0, 256, ln, dtype=np.uint8) | rng.integers(0, 256, ln, dtype=np.uint8)).astype(np.uint8).tobytes()
            for ln in (40, 600)]
    return out + [b"\xff" * 4000, b"\x00" * 300]


def _check_three_decoders(O, d, n, geom, what):
    """decode, decode_budgets and decode_with_metadata (its value column holds the coefficient before each bit)"""
    import spiht_amd
    from spiht_amd.spiht import decode_budgets, decode_with_metadata
    c, h, w, lh, lw = geom
    what = "%s n=%d %d bytes" % (what, n, len(d))
    r = _check_decode(O, d, n, geom, what)
    nb = 8 * len(d)
    bud = sorted({0, 1, 2, 9, nb // 3, nb // 2 + 1, nb - 1, nb, nb + 40})
    bits = O.bytes_to_bits(d)
    refs = _ref(("bud", d, n, geom), lambda: [O.decode_bits(bits[:b], n, c, h, w, lh, lw) for b in bud])
    got = decode_budgets(d, n, c, h, w, lh, lw, bud)
    for k, b in enumerate(bud):
        _same(got[k], refs[k], "%s budget %d bits" % (what, b))
    _same(got[-1], r, what + " last budget")
    top, other = nominal_slices(lh, lw, tree_generations(h, w, lh, lw))
    r_ref, m_ref = _ref(("meta", d, n, geom), lambda: O.decode_with_metadata(d, n, c, h, w, lh, lw, top, other))
    rec, meta = decode_with_metadata(d, n, c, h, w, lh, lw, top, other)
    _same(rec, r_ref, what + " metadata rec")
    if not np.array_equal(meta, m_ref):
        q = int(np.argwhere((meta != m_ref).any(axis=1))[0, 0])
        raise AssertionError("%s: metadata row %d: got %s want %s" % (what, q, meta[q].tolist(), m_ref[q].tolist()))


def _decode_at_the_limit(O, geoms):
    top_value = 0
    for geom in geoms:
        for d in _hostile_streams():
            for n in (30, 29, 1, 0):
                _check_three_decoders(O, d, n, geom, "hostile %s" % (geom,))
                top_value = max(top_value, int(np.abs(_ref_decode(O, d, n, geom).astype(np.int64)).max()))
    assert top_value == (1 << 31) - 1  # (the cases reach the largest value a stream can decode to)
    for p, v in E.periodic_patterns():
        d = E.periodic_stream(p, v, 40)
        for n in (30, 29, 1, 0):
            _check_three_decoders(O, d, n, E.ODD_GEOM, "period %d pattern %d" % (p, v))


def _refusals(O):
    import spiht_amd
    from spiht_amd import _lib
    ctx, L = _lib.default_context(), _lib.lib()
    geom = E.ODD_GEOM
    c, h, w, lh, lw = geom
    good = synth_coeffs(3, c, h, w, lh, lw, scale=900.0)

    def still_works():
        ctx.synchronize()  # a second synchronize() is clean
        _roundtrip(O, good, geom, UNLIMITED, "after a refusal", E.coded_cells(O, geom))
        _roundtrip(O, good, geom, 777, "after a refusal")

    for v in (1 << 30, (1 << 31) - 1, -(1 << 31), -(1 << 30)):
        for alone in (True, False):
            x = np.zeros((c, h, w), np.int32) if alone else good.copy()
            x[c - 1, h // 2, w // 3] = v
            with pytest.raises(ValueError):
                spiht_amd.encode(x, lh, lw, UNLIMITED)
            still_works()
            xs = np.stack([good, x, good])
            d_x = _dev(ctx, xs)
            d_out, d_nb, d_mn = _dev(ctx, np.zeros((3, 400), np.uint8)), _dev(ctx, np.zeros(3, np.uint64)), _dev(ctx, np.zeros(3, np.uint8))
            _lib.check(L.spiht_encode_batch_i32(ctx.handle, vp(d_x.ptr), 3, c, h, w, lh, lw, 3000, vp(d_out.ptr), 400, vp(d_nb.ptr), vp(d_mn.ptr)))
            with pytest.raises(ValueError):
                ctx.synchronize()
            still_works()
            for d in (d_x, d_out, d_nb, d_mn):
                d.free()
    stream, n_good = O.encode(good, lh, lw, 3000)
    for n in (31, 255):
        with pytest.raises(ValueError):
            spiht_amd.decode(stream, n, c, h, w, lh, lw)
        still_works()
        data, nbytes = _slots([stream, stream, b"", stream])
        for bad_at in (0, 2, 3):
            ns = np.full(4, n_good, np.uint8)
            ns[bad_at] = n
            with pytest.raises(_lib.SpihtHipError):  # the device error word, as every batched decode reports it
                _decode_batch(ctx, data, nbytes, ns, geom, "n = %d" % n)
            still_works()


# ------------------------------------------------------------------------------------------------ 3

CAP_PARTS = ["enc-%d-%s" % (g, cd) for g in (0, 1) for cd in ("narrow", "wide5")] + ["dec-0", "dec-1", "dec-odd", "neighbours"]


@pytest.mark.parametrize("part", CAP_PARTS)
def test_lists_at_their_capacity(oracle, part):
    """list_caps() (api_coder.cpp) sizes LIP, LSP and LIS from the stream length -- roots + mb + 16384, mb/2 + 1 + 16384,
    roots + 4 mb + 16384 -- or from the tree's node count, whichever is smaller.  Arrays that are significant everywhere,
    only in the finest level, or in one far cell, at budgets on either side of the points where the two terms meet; streams
    of ones (the LSP bound mb/2 + 1 is tight), of zeros and of every short period through the decoder.  A cap too small
    shows as SPIHT_ERR_INTERNAL (an exception here) or as a neighbouring slot's image corrupted."""
    O = oracle
    kind = part.split("-")
    if kind[0] == "enc":
        geom = E.CAP_GEOMS[int(kind[1])]
        bind, free = E.cap_budgets(O, geom)
        with _coder(kind[2]) as ctx:
            if kind[2] != "narrow":
                ctx.set_option("wide_solo", 300)
            for M in (1, 1 << 12, E.band(O, E.CAP_MAGNITUDE_PLANES)[0]):
                for name, x in E.extremal_arrays(geom, M).items():
                    for mb in bind + free:
                        _roundtrip(O, x, geom, mb, "%s %s %s of %d, budget %d" % (kind[2], geom, name, M, mb))
    elif kind[0] == "dec":
        import spiht_amd
        geom = E.ODD_GEOM if kind[1] == "odd" else E.CAP_GEOMS[int(kind[1])]
        for ln in (1, 8, 64, 512, 4096, 20000):
            streams = E.extremal_streams(ln)
            data, nbytes = _slots(streams)
            for n in (30, 5):
                refs = [O.decode(d, n, *geom) for d in streams]  # (once for both widths, and not kept)
                for waves in (12, 8):
                    what = "%s, %d wavefronts, %d bytes, n=%d" % (geom, waves, ln, n)
                    with _waves(waves) as ctx:
                        rec = _decode_batch(ctx, data, nbytes, np.full(len(streams), n, np.uint8), geom, what)
                        for b in range(len(streams)):  # every stream
                            _same(rec[b], refs[b], "%s, stream %d" % (what, b))
                        for b in (0, 1):  # all ones, all zeros: through the single call too
                            _same(spiht_amd.decode(streams[b], n, *geom), refs[b], what + " single")
    else:
        from spiht_amd import _lib
        ctx = _lib.default_context()
        geom = E.CAP_GEOMS[1]
        c, h, w, lh, lw = geom
        slot = 20000
        streams, ns = [], []
        for b in range(16):
            if b % 2:
                streams.append(b"\xff" * (slot - (b // 2) % 3))
                ns.append(30)
            else:
                d, n = O.encode(synth_coeffs(600 + b, c, h, w, lh, lw, scale=float(40 * 4 ** (b // 2))), lh, lw, 8 * slot - 5 * b)
                streams.append(d)
                ns.append(n)
        data, nbytes = _slots(streams, slot)
        rec = _decode_batch(ctx, data, nbytes, ns, geom, "neighbouring slots")
        _check_decoded_batch(O, rec, data, nbytes, ns, geom, "neighbouring slots")


# ------------------------------------------------------------------------------------------------ 4

@pytest.mark.parametrize("part", ["decode12", "decode8", "window12", "window8", "encode"])
def test_mixed_batches_with_slot_reuse(oracle, part):
    """k_decode and k_encode walk images b, b + gridDim.x, ... in one workgroup: batches larger than the slot count
    (8 * num_cu decoder slots, num_cu encoder slots) in which every image differs in length, start plane and content, a
    list-heavy hostile stream shares its workgroup with an empty one, and the bytes of a slot past its stream are not zero.
    State carried from one image to the next, or a reader that looks past nbytes, shows as a wrong image; a write outside
    the call's own arrays shows in the guard regions."""
    from spiht_amd import _lib
    O = oracle
    ctx = _lib.default_context()
    num_cu = ctx.get_option("num_cu")
    if part.startswith("decode") or part.startswith("window"):
        if part.startswith("decode"):
            geom, slot, nslots, B = E.ODD_GEOM, 96, 8 * num_cu, 8 * num_cu + 300
            assert B > 8 * num_cu
        else:
            geom, slot, nslots, B = E.WINDOW_GEOM, 6000, 8 * num_cu, 64
        data, nbytes, ns, kinds = _ref(("mixed", geom, B), lambda: E.mixed_batch(O, B, geom, slot, nslots, 4 if slot == 96 else 5))
        with _waves(int(part[6:])):
            rec = _decode_batch(ctx, data, nbytes, ns, geom, part)
        _check_decoded_batch(O, rec, data, nbytes, ns, geom, part)
    else:
        geom, mb = E.MID_GEOM, 3001
        c, h, w, lh, lw = geom
        B = num_cu + 50
        assert B > num_cu
        xs = E.encoder_batch(O, B, geom, 9)
        slot = ((mb + 7) // 8 + 3) & ~3
        res, devs, (p_out, p_nb, p_mn) = _encode_batch(ctx, xs, geom, mb, slot)
        _check_encoded_batch(O, xs, geom, mb, slot, res, "mixed encoder batch")
        # that output, as it lies in device memory, through the batched decoder
        d_ny = _dev(ctx, np.zeros(B, np.uint64))
        _lib.check(_lib.lib().spiht_nbits_to_nbytes(ctx.handle, vp(p_nb), B, vp(d_ny.ptr)))
        rec = _decode_batch_ptrs(ctx, p_out, slot, d_ny.ptr, p_mn, B, geom, "decode of the mixed encoder batch")
        out, nbits, maxn = res
        _check_decoded_batch(O, rec, out, (nbits.astype(np.uint64) + 7) // 8, maxn, geom, "decode of the mixed encoder batch")
        for d in devs + (d_ny,):
            d.free()
