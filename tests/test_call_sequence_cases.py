"""tests/call_sequence_cases.py held to its purpose where no GPU is: the batches really straddle the 65535-plane seam with
the pictures they claim, the disturbances of tests/test_gpu_call_sequences.py really have the property each is named for,
and the schedules of tests/test_gpu_ordering.py really differ between producer and consumer."""
import numpy as np

import call_sequence_cases as K
import dwt_sweep_tables as T


def _prime(n):
    return n > 1 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def test_the_batches_straddle_the_seam():
    assert K.SEAM == 65535 == 3 * 5 * 17 * 257
    assert K.CHUNK_B == 21852 and K.chunks(K.CHUNK_B, 3) == [(0, 21845), (21845, 7)]
    assert 3 * 21845 == K.SEAM and 3 * 7 == 21              # 65535 planes in the first launch exactly, 21 in the second
    assert K.chunks(K.ONE_PLANE_B, 1) == [(0, 65535), (65535, 5)]
    # (the largest batch of the transform sweep stays below: there batch_chunks does not split)
    assert T.PF_PICTURES * 3 <= K.SEAM < K.CHUNK_B * 3
    for distinct in (K.ONE_PLANE_DISTINCT, K.FLAGS_DISTINCT):
        assert _prime(distinct) and K.SEAM % distinct != 0
    # the picture at the seam is not the first of the arrays that take turns, and the pictures behind the seam are others than
    # those at the start of the batch
    assert K.SEAM % K.ONE_PLANE_DISTINCT != 0 and (K.SEAM // 3) % K.FLAGS_DISTINCT != 0


def test_every_picture_of_the_seam_batch_is_distinct():
    P = K.chunk_pictures()
    assert P.shape == (K.CHUNK_B, 3, 8, 8) and P.dtype == np.uint8
    assert len(np.unique(P.reshape(len(P), -1), axis=0)) == len(P)
    assert 30e6 < (P / 255).nbytes < 36e6  # about 34 MB as float64


def test_the_oracle_takes_the_seam_geometry(oracle):
    k = K.CHUNK
    g = oracle.geometry(k["H"], k["W"], k["wavelet"], k["level"], k["mode"])
    assert (g["level"], g["ll_h"], g["ll_w"], g["enc_h"], g["enc_w"]) == (1, 4, 4, 8, 8)
    P = K.chunk_pictures()[:64]
    seen = set()
    for p in P:
        d, n, gg = oracle.encode_image(p / 255, k["wavelet"], k["mode"], k["level"], k["q"], None, k["max_bits"])
        assert 0 < len(d) <= (k["max_bits"] + 7) // 8
        seen.add(d)
        rec = oracle.decode_image(d, n, 3, 8, 8, k["wavelet"], k["level"], k["q"], None)
        assert rec.shape == (3, 8, 8) and np.isfinite(rec).all()
    assert len(seen) == len(P)  # distinct pictures give distinct streams: a picture taken for another one shows
    # the single-precision transform differs from the double one somewhere (it is a reference of its own)
    a32 = oracle.quantize_f32(oracle.wavedec2_array_f32((P[0] / 255).astype(np.float32), "haar", "reflect", 1)[0], k["q"], None)
    assert a32.shape == (3, 8, 8)


def test_the_raw_coder_arrays(oracle):
    R = K.one_plane_reference(oracle)
    assert len(R["streams"]) == K.ONE_PLANE_DISTINCT == 61 and len(set(R["streams"])) > 50
    assert len(set(R["max_n"].tolist())) >= 3 and all(0 < len(d) <= 50 for d in R["streams"])


def test_the_occupancy_words_of_the_seam_case(oracle):
    k, R = K.FLAGS, K.flags_reference(oracle)
    g = oracle.geometry(k["H"], k["W"], k["wavelet"], k["level"], k["mode"])
    assert g["level"] == 2  # two levels: the occupancy words exist
    assert R["words"].shape == (K.FLAGS_DISTINCT, 3, 1, 1) and R["rec"].shape[1:] == (3, g["enc_h"], g["enc_w"])
    zero = float((R["words"] == 0).mean())
    assert 0.3 <= zero <= 0.7, zero
    # what a launch that took the words of picture b for picture 21845 + b would do wrong: somewhere among the pictures behind
    # the seam a plane with coefficients in its detail bands gets a zero word
    b0 = K.SEAM // 3
    behind = (np.arange(b0, K.CHUNK_B)) % K.FLAGS_DISTINCT
    front = np.arange(K.CHUNK_B - b0) % K.FLAGS_DISTINCT
    assert ((R["words"][behind] != 0) & (R["words"][front] == 0)).any()
    assert len(np.unique(R["rec"].reshape(K.FLAGS_DISTINCT, -1), axis=0)) == K.FLAGS_DISTINCT


def _library_sizes(k):
    """what the library says of case k: (rec_h, rec_w), (enc_h, enc_w), the approximation plane, {r: (dense reduced picture,
    the picture of an integer or float-kind view)} for r = 1 .. L, and the occupancy words per picture"""
    import ctypes as C
    from spiht_amd import _lib
    L = _lib.lib()
    wid, mid, lv = L.spiht_wavelet_id(k["wavelet"].encode()), L.spiht_mode_id(k["mode"].encode()), k["level"]
    i64 = [C.c_int64() for _ in range(8)]
    used = C.c_int()
    assert L.spiht_geometry_mode(k["H"], k["W"], wid, mid, lv, C.byref(used), *[C.byref(v) for v in i64[:6]]) == 0
    enc, rec = (i64[2].value, i64[3].value), (i64[4].value, i64[5].value)
    ah, aw = C.c_int64(), C.c_int64()
    assert L.spiht_idwt_approx_shape(k["H"], k["W"], wid, lv, C.byref(ah), C.byref(aw)) == 0
    red = {}
    for r in range(1, used.value + 1):
        assert L.spiht_reduced_shape(k["H"], k["W"], wid, mid, lv, r, C.byref(used), *[C.byref(v) for v in i64]) == 0
        red[r] = ((i64[0].value, i64[1].value), (i64[2].value, i64[3].value))
    words = C.c_uint64()
    assert L.spiht_l1_flags_words(k["c"], k["H"], k["W"], wid, mid, lv, C.byref(words)) == 0
    return rec, enc, (ah.value, aw.value), red, int(words.value)


def test_no_two_sizes_of_the_second_seam_case_agree(oracle):
    """SEAM2 exists so that a launch which stepped one of its arrays by another array's size lands on another picture.  The
    per-picture element counts -- each is the multiplier of b0 somewhere in api_image.cpp or api_coder.cpp -- are pairwise different, with one
    exception that no geometry can avoid: the approximation plane of the two-part inverse IS the float64 picture at
    reduce = 1 (2 hs[2] - F + 2 by 2 ws[2] - F + 2, both), so c a_plane and that dense size are one number, and are
    asserted to be.  The integer / float-kind picture at reduce = 1 (hs[1] x ws[1]) stands in the list as well."""
    k = K.SEAM2
    S = K.seam2_sizes(oracle)
    g = oracle.geometry(k["H"], k["W"], k["wavelet"], k["level"], k["mode"])
    assert (g["level"], g["hs"], g["ws"]) == (2, [17, 11, 8], [25, 15, 10])
    rec, enc, approx, red, words = _library_sizes(k)
    c = k["c"]
    # the oracle's geometry and the library's say the same
    assert enc == (g["enc_h"], g["enc_w"]) == (27, 35) and rec == (18, 26) and approx == (12, 16)
    assert red[1] == ((12, 16), (11, 15)) and red[2] == ((8, 10), (8, 10)) and (g["ll_h"], g["ll_w"]) == (8, 10)
    assert S == dict(picture=c * 17 * 25, rec=c * rec[0] * rec[1], array=c * enc[0] * enc[1], approx=c * approx[0] * approx[1],
                     reduced1=c * red[1][0][0] * red[1][0][1], reduced2=c * red[2][0][0] * red[2][0][1],
                     reduced1_int=c * red[1][1][0] * red[1][1][1])
    assert S["approx"] == S["reduced1"]  # (one quantity by definition: see above)
    different = [S[n] for n in ("picture", "rec", "array", "approx", "reduced2", "reduced1_int")]
    assert len(set(different)) == len(different), S
    assert len({S[n] for n in ("picture", "rec", "array", "reduced1", "reduced2", "reduced1_int")}) == 6, S
    assert words > 0 and words == c  # one inverse tile per plane
    # the batch, and the pictures that take turns in it
    for distinct in (K.SEAM2_DISTINCT, K.SEAM_PER_DISTINCT):
        assert _prime(distinct) and distinct >= 100 and (K.SEAM // 3) % distinct != 0 and 21845 % distinct != 0
    assert K.chunks(K.CHUNK_B, c) == [(0, 21845), (21845, 7)]
    which = K.in_turn(K.SEAM2_DISTINCT)
    assert len(which) == K.CHUNK_B and which[21845] == 1 and which[0] == 0


def test_the_second_seam_reference(oracle):
    k, R = K.SEAM2, K.seam2_reference(oracle)
    D, c = K.SEAM2_DISTINCT, k["c"]
    P = K.seam_pictures(k, D)
    assert P.shape == (D, c, 17, 25) and len(np.unique(P.reshape(D, -1), axis=0)) == D
    assert R["coeffs"].shape == R["rec"].shape == R["coeffs_f32"].shape == (D, c, 27, 35)
    assert R["pics"].shape == R["pics_fl"].shape == (D, c, 18, 26)
    assert R["red"][1].shape == R["approx"].shape == (D, c, 12, 16) and R["red"][2].shape == (D, c, 8, 10)
    assert all(not v.flags.writeable for v in list(R.values()) + list(R["red"].values()) if isinstance(v, np.ndarray))
    # the budget cuts every stream short of lossless; distinct pictures give distinct streams
    assert (R["nbits"] == k["max_bits"]).all() and (R["rec"] != R["coeffs"]).any(axis=(1, 2, 3)).all()
    assert len(set(R["streams"])) == D and len(set(R["streams_f32"])) == D and (R["nbits_f32"] == k["max_bits"]).all()
    # the single-precision transform is a reference of its own
    assert (R["coeffs_f32"] != R["coeffs"]).any()
    # about half the occupancy words are zero, and the pictures behind the seam need words the pictures at the front lack
    assert R["words"].shape == (D, c, 1, 1)
    zero = float((R["words"] == 0).mean())
    assert 0.3 <= zero <= 0.7, zero
    b0 = K.SEAM // 3
    behind, front = K.in_turn(D)[b0:], K.in_turn(D)[:K.CHUNK_B - b0]
    assert ((R["words"][behind] != 0) & (R["words"][front] == 0)).any()
    assert (R["pics_fl"] != R["pics"]).any()  # (emptying the tiles changed pictures: the decoded arrays had level-1 details)
    # the reduced pictures are not crops or copies of one another
    assert np.array_equal(R["approx"], R["red"][1] * 2) and R["red"][1].std() > 0 and R["red"][2].std() > 0


def test_the_two_pass_seam_reference(oracle):
    k, R = K.SEAM_PER, K.seam_per_reference(oracle)
    g = R["geom"]
    taps = len(oracle.wavelet_filters(k["wavelet"])[0])
    assert k["mode"] == "periodization" and 2 < taps <= 20  # the two-pass route of a filter the tiled kernels would take
    assert (g["level"], g["hs"], g["ws"], g["enc_h"], g["enc_w"]) == (1, [9, 5], [13, 7], 10, 14)
    rec, enc, approx, red, words = _library_sizes(k)
    assert rec == (10, 14) and enc == (10, 14) and words == 0
    assert k["H"] * k["W"] != rec[0] * rec[1]  # (the pixels and the array step by different sizes)
    assert R["pics"].shape == (K.SEAM_PER_DISTINCT, 3, 10, 14) and "red" not in R
    assert len(set(R["streams"])) == K.SEAM_PER_DISTINCT and (R["nbits"] == k["max_bits"]).all()


def test_the_padded_views_differ_from_the_dense_ones_and_are_taken():
    """every stride of K.padded_strides differs from dense HWC (what strided_hwc makes) and from dense CHW, and the library
    takes the view as an output of every kind, for the full and for the reduced pictures"""
    import ctypes as C
    from spiht_amd import _lib, floatpx
    L = _lib.lib()
    B, c = K.CHUNK_B, 3
    for H, W in ((17, 25), (11, 15), (8, 10), (9, 13)):
        for es in (1, 2, 4):
            st = K.padded_strides(c, H, W, es)
            sb, sc, sh, sw = (int(v) for v in st)
            assert sc == es and sw not in (c * es, es) and sh not in (W * c * es, W * es, W * sw) and sb not in (H * W * c * es, H * sh)
            assert sw > c * es and sh > W * sw and sb > H * sh and all(v % es == 0 for v in (sb, sh, sw))
            p = C.c_void_p(st.ctypes.data)
            if es == 1:
                assert L.spiht_check_view_u8(B, c, H, W, p, 1) == 0 and L.spiht_check_view_u8(B, c, H, W, p, 0) == 0
            if es == 2:
                assert L.spiht_check_view_u16(B, c, H, W, p, 1) == 0 and L.spiht_check_view_u16(B, c, H, W, p, 0) == 0
            for kind in floatpx.KINDS:
                if floatpx.itemsize(kind) == es:
                    assert L.spiht_check_view_flt(kind, B, c, H, W, p, 1) == 0
    # the buffer helpers: samples go where the strides say, and a byte written into the padding shows
    buf, view, st = K.padded_buffer(5, 3, 4, 6, np.uint16)
    assert buf.shape == (5, int(st[0]) // 2) and (buf.view(np.uint8) == K.PAD_BYTE).all() and K.padding_untouched(buf, 3, 4, 6)
    view[...] = np.arange(5 * 3 * 4 * 6, dtype=np.uint16).reshape(5, 3, 4, 6)
    flat = buf.reshape(-1)
    for b, ch, y, x in ((0, 0, 0, 0), (4, 2, 3, 5), (1, 1, 2, 3)):
        assert flat[(b * st[0] + ch * st[1] + y * st[2] + x * st[3]) // 2] == view[b, ch, y, x] == ((b * 3 + ch) * 4 + y) * 6 + x
    assert K.padding_untouched(buf, 3, 4, 6)
    for off in (3, int(st[3]) // 2 * 6, int(st[2]) // 2 * 4, buf.shape[1] - 1):  # alpha, row padding, spare row, last sample
        bad = buf.copy()
        bad[2, off] ^= 1
        assert not K.padding_untouched(bad, 3, 4, 6), off


def test_the_probe_and_the_dense_decode(oracle):
    imgs, streams, ns, pics, recs = K.probe_reference(oracle)
    assert imgs.shape == (2, 3, 70, 90) and pics.shape[:2] == (2, 3) and streams[0] != streams[1]
    assert all(len(d) == (K.PROBE["max_bits"] + 7) // 8 for d in streams)  # 0.5 bits per pixel, reached
    g = oracle.geometry(70, 90, "bior2.2", None)
    assert g["level"] >= 3  # (reduce = 1, 2 and L are three different decodes)
    # the dense decode writes more cells than the probe's whole array has, into a larger array
    dense = K.image_reference(oracle, K.DENSE, K.pictures(K.DENSE, 4200))
    assert int((dense[3] != 0).sum()) > recs.size and dense[3][0].size > recs[0].size
    small = K.image_reference(oracle, K.SMALL, K.pictures(K.SMALL, 4300))
    assert small[3][0].size < recs[0].size < dense[3][0].size


def test_the_odd_ll_case_has_duplicated_and_padding_cells(oracle):
    k = K.ODD_LL
    g = oracle.geometry(k["H"], k["W"], k["wavelet"], k["level"], k["mode"])
    assert g["ll_h"] % 2 == 1 and g["ll_w"] % 2 == 1
    geom = (k["c"], g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"])
    assert K.duplicated_cells(oracle, geom) > 0
    pad = K.padding_cells(oracle, k)
    assert pad.shape == (g["enc_h"], g["enc_w"]) and 0 < pad.sum() < pad.size // 4
    streams, ns = K.arbitrary_streams(k["B"])
    assert len(streams) == k["B"] and len({len(d) for d in streams}) >= 8
    reached = [int((oracle.decode(d, n, *geom)[:, pad] != 0).sum()) for d, n in zip(streams, ns)]
    assert sum(1 for v in reached if v > 0) >= 3, reached  # the byte strings write padding cells, which no encoder's stream does
    probe = K.probe_reference(oracle)
    assert not any(rec[:, K.padding_cells(oracle, K.PROBE)].any() for rec in probe[4])


def test_the_tiny_batch_exceeds_every_slot_count():
    k = K.TINY
    assert k["B"] > K.MAX_DECODER_SLOTS == 8 * 256
    P = K.tiny_pictures()
    assert P.shape == (k["B"], 1, 8, 8) and _prime(k["distinct"])
    assert len(np.unique(P.reshape(len(P), -1), axis=0)) == k["distinct"]
    assert K.MAX_DECODER_SLOTS % k["distinct"] != 0  # the image that takes a slot over is another one than the slot's first


def test_the_state_cases():
    assert K.PF_GROUPS == [4, 3, 1, 4] and T.pf_tile_count() >= T.PF_MIN
    (c1, s1), (c2, s2), (c3, s3), (c4, s4), (c5, s5) = K.SCALES
    assert s1 == s3 and s1 != s2 and len(s1) == len(s2) and c1 == c2 == c3 == c4 and s4 is None and c5 != c1 and len(s5) == c5
    assert K.LONG_FILTERS == ["db11", "sym11", "coif4"]
    assert {w for w, _ in K.WIDTH_SETTINGS} == {8, 12} and {f for _, f in K.WIDTH_SETTINGS} == {0, 1}
    assert all(a != b for a, b in zip(K.WIDTH_SETTINGS, K.WIDTH_SETTINGS[1:]))


def test_the_long_filters(oracle):
    taps = {w: len(oracle.wavelet_filters(w)[0]) for w in K.LONG_FILTERS}
    assert taps["db11"] == taps["sym11"] == 22 and taps["coif4"] > 20  # longer than the tiled kernels take (20)
    assert not np.array_equal(oracle.wavelet_filters("db11")[0], oracle.wavelet_filters("sym11")[0])
    k = K.LONG
    for w, F in taps.items():  # every level's input is at least as long as the filter (the single-precision rule)
        assert min(T.band_len(k["H"], F), T.band_len(k["W"], F)) >= F and k["level"] == 2


def test_the_schedules_of_the_ordering_cases():
    assert K.ROUNDS == 2 and 0 < K.GATE_US <= 10000
    assert (K.LIST["B"], K.LIST["c"], K.LIST["H"], K.LIST["W"]) == (40, 3, 541, 961)  # test_pipeline_u8_at_batch_size
    for B in (K.LIST["B"], K.REST["B"]):
        a, b = K.round_order(B, 0), K.round_order(B, 1)
        assert sorted(a) == sorted(b) == list(range(B)) and (a != b).sum() >= B - 1
    assert K.LIST["B"] % K.LIST["distinct"] == 0 and K.LIST["distinct"] % 2 == 0  # (reversing the batch moves every picture)
    # in every place of the batch the consumer's picture is another one than the producers' -- by content: the list pictures
    # take turns -- and the producers' second round has another picture there than their first
    for k in (K.LIST, K.REST):
        B, distinct = k["B"], k.get("distinct", k["B"])
        seen = []
        for r in range(K.ROUNDS):
            po, mine = K.orders(B, r)
            assert sorted(mine) == list(range(B)) and ((po % distinct) != (mine % distinct)).all()
            seen += [po % distinct, mine % distinct]
        assert (seen[0] != seen[2]).all()  # (each round has arrays of its own; the producers' pictures change place)
