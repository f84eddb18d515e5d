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
