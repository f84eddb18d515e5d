"""The grid of tests/test_gpu_dwt_sweep.py held to its purpose, without a GPU: conditions on the tables and on the inputs
(tests/dwt_sweep_tables.py), none of them a measurement of the code under test."""
import numpy as np

import dwt_sweep_tables as T


def test_wavelet_list_reaches_every_mask_instantiation(oracle):
    """The launchers' mask rule recomputed from the oracle's filters: per filter length the all-taps instantiation, and the
    specialised one of lengths 6, 10 and 18 (for two taps the specialised masks ARE all taps: one instantiation, reached
    through the first branch), forward and inverse; and among the all-taps banks one with and one without a leading tap
    that is zero in both analysis filters (the extent k_dwt_edge recomputes depends on it)."""
    want = {(F, "all") for F in T.FILTER_LENGTHS if F != 2} | {(F, "special") for F in T.FWD_SPECIALISED}
    assert len(want) == 13 and len(T.FWD_SPECIALISED) + len(T.FILTER_LENGTHS) == 14  # 14 branches, 13 distinct kernels
    for inverse in (False, True):
        got = {T.instantiation(oracle, w, inverse)[:2] for w in T.WAVELETS}
        assert got == want, (inverse, sorted(want - got), sorted(got - want))
    assert {T.instantiation(oracle, w, True)[:2] for w in T.INVERSE_MASK_WAVELETS} == want
    assert len(T.INVERSE_MASK_WAVELETS) == len(want)
    zs = {T.instantiation(oracle, w)[2] for w in T.WAVELETS if T.instantiation(oracle, w)[1] == "all"}
    assert zs == {0, 1}
    # every generic bank with z = 1 of the lengths that have one
    assert {w for w in T.WAVELETS if T.instantiation(oracle, w)[1:] == ("all", 1)} == {"bior2.4", "rbio5.5", "bior2.6", "bior2.8"}


def test_size_lists_sit_on_the_tile_seams():
    for F in T.FILTER_LENGTHS:
        for th in (T.FWD_TH, T.FWD32_TH):
            sizes = T.forward_sizes(F, th)
            assert [T.band_len(h, F) for h, _ in sizes] == [th - 1, th, th + 1, 2 * th + 1]
            assert [T.band_len(w, F) for _, w in sizes] == [T.FWD_TW - 1, T.FWD_TW, T.FWD_TW + 1, 2 * T.FWD_TW + 1]
            assert [(T.tiles(T.band_len(h, F), th), T.tiles(T.band_len(w, F), T.FWD_TW)) for h, w in sizes] == [(1, 1), (1, 1), (2, 2), (3, 3)]
            assert all(h >= 1 and w >= 1 for h, w in sizes)
            assert {h & 1 for h, _ in sizes} == {0, 1} and {w & 1 for _, w in sizes} == {0, 1}
        red = T.forward_sizes_reduced(F)
        assert [(T.band_len(h, F), T.band_len(w, F)) for h, w in red] == [(T.FWD_TH, T.FWD_TW), (2 * T.FWD_TH + 1, 2 * T.FWD_TW + 1)]
        assert red[1][0] & 1 and red[1][1] & 1
        # the single-precision grid: some case of every length runs, and the largest size runs both levels
        lv = [T.f32_level(F, h, w) for h, w in T.forward_sizes(F, T.FWD32_TH)]
        assert lv[3] == 2 and all(v in (None, 1, 2) for v in lv)
        for (h, w), v in zip(T.forward_sizes(F, T.FWD32_TH), lv):
            if v:
                assert min(h, w) >= F and (v == 1 or min(T.band_len(h, F), T.band_len(w, F)) >= F)
        # the colour picture: more than one strip of k_dwt1_color in both directions
        H, W = T.COLOUR_BIG
        assert T.tiles(T.band_len(H, F), T.C1_ROWS) == 2 and T.tiles(T.band_len(W, F), T.c1_sw(F)) >= 3
        # inverse: the level-1 bands of every picture give back the listed sizes
        for integer in (False, True):
            for (h, w), (rh, rw) in zip(T.inverse_sizes(integer), T.INV_REC):
                assert (2 * T.band_len(h, F) - F + 2, 2 * T.band_len(w, F) - F + 2) == (rh, rw)
                assert not integer or (h & 1 and w & 1 and (h + 1, w + 1) == (rh, rw))
    assert [(T.tiles(h, T.INV_TH), T.tiles(w, T.INV_TW)) for h, w in T.INV_REC] == [(1, 1), (1, 1), (2, 2), (3, 3)]
    assert [T.tiles(h, T.INVC_TH) for h, _ in T.INV_REC] == [3, 3, 4, 7]
    # the persistent inverse: enough tiles in one launch, and nothing to spare (the geometry, not the count, carries the test)
    assert (T.tiles(T.PF_REC[0], T.INV_TH), T.tiles(T.PF_REC[1], T.INV_TW)) == (2, 2)
    assert T.pf_tile_count() >= T.PF_MIN
    # ... and its 32-bit plane offsets hold (launch_idwt_FM: off32), or the launcher falls back to k_idwt_level
    assert (T.PF_REC[0] + T.INV_TH) * T.PF_REC[1] * 8 < 2 ** 31
    assert T.PF_PICTURES * 3 <= 65535  # one launch: batch_chunks of api_internal.h does not split the batch


def _dense(arr, H, W, F):
    """the least share of non-zero cells among the three level-1 detail bands"""
    return min(float((b != 0).mean()) for b in T.level1_detail_bands(arr, H, W, F))


def _interior(arr, H, W, F):
    """(non-zero cells, cells) of the three level-1 detail bands over the cells whose filter windows lie inside the picture
    along both axes: outputs F/2 - 1 .. N/2 - 1 of an axis of N samples"""
    if min(H, W) < F:
        return 0, 0
    inner = [b[..., F // 2 - 1:H // 2, F // 2 - 1:W // 2] for b in T.level1_detail_bands(arr, H, W, F)]
    return sum(int((b != 0).sum()) for b in inner), sum(b.size for b in inner)


def test_inputs_are_dense_in_the_detail_bands(oracle):
    """A wrong sample of a level-1 detail band shows only where the quantised coefficient is not zero anyway.  Of the oracle's
    arrays of the float pictures of the forward sweep (both tile heights, all modes, q = 1000) at least 90 % of the level-1
    detail cells are non-zero
      - in every band of every picture under reflect and periodic, pictures shorter than the filter included;
      - under symmetric, zero and constant among the cells whose windows lie inside the picture, per wavelet, mode and tile
        height.  The border cells of those three modes cannot be held to a share: a half-sample mirror image, a constant
        and zeros continue the picture so that the high-pass sums next to the border are zero or next to it whatever the
        picture holds (the last row of a haar level of an odd-sized picture is exactly zero under symmetric; under
        constant 13 % of the cells of a 3 x 108 picture's bior3.9 bands are non-zero, under zero 21 %) -- a wrong index
        there makes them non-zero, which shows.
    The same for a representative 8-bit and 16-bit picture."""
    from test_gpu_u8 import u8_image
    from test_gpu_u16 import u16_image
    worst, inner = {}, {}
    for wv in T.WAVELETS:
        F = T.instantiation(oracle, wv)[0]
        for th in (T.FWD_TH, T.FWD32_TH):
            for i, (H, W) in enumerate(T.forward_sizes(F, th)):
                imgs = T.sweep_images(1000 + i, 2, 2, H, W)
                for mode in T.MODES:
                    for b in range(2):
                        arr, _ = oracle.wavedec2_array(imgs[b], wv, mode, 2)
                        qa = oracle.quantize(arr, T.Q, T.scales_for(i, 2))
                        worst[mode] = min(worst.get(mode, (1.0, None)), (_dense(qa, H, W, F), (wv, H, W, b)))
                        nz, n = _interior(qa, H, W, F)
                        k = (wv, mode, th)
                        inner[k] = (inner.get(k, (0, 0))[0] + nz, inner.get(k, (0, 0))[1] + n)
    for mode in T.MODES:
        print("least dense level-1 detail band, %-9s: %.3f at %s" % (mode, *worst[mode]))
    share = {k: nz / n for k, (nz, n) in inner.items()}
    assert len(share) == len(T.WAVELETS) * len(T.MODES) * 2 and min(n for _, n in inner.values()) >= 1000
    k = min(share, key=share.get)
    print("least dense interior: %.3f at %s" % (share[k], k))
    assert share[k] >= 0.9, (k, share[k])
    for mode in ("reflect", "periodic"):
        assert worst[mode][0] >= 0.9, (mode, worst[mode])
    for wv in ("bior2.2", "db10"):
        F = T.instantiation(oracle, wv)[0]
        H, W = T.forward_sizes_reduced(F)[1]
        for P, full in ((u8_image(3000, 3, H, W), 255.0), (u16_image(3000, 3, H, W), 65535.0)):
            arr, _ = oracle.wavedec2_array(P / full, wv, "reflect", 2)
            assert _dense(oracle.quantize(arr, T.Q, None), H, W, F) >= 0.9


def test_inverse_inputs_overshoot_and_flags_are_mixed(oracle):
    """the inverse sweep's pictures leave [0, 1] on both sides (the clip of the integer kinds has work to do), and in the
    FLAGS cases of the persistent inverse between 20 % and 80 % of the occupancy words are zero"""
    for wv in ("haar", "bior4.4", "db10"):
        for H, W in T.inverse_sizes(True):
            _, want = T.inverse_case(oracle, wv, H, W, 2, 77, None, c=3)
            assert want[:, :H, :W].min() < 0.0 and want[:, :H, :W].max() > 1.0
    for wv in T.INVERSE_MASK_WAVELETS:
        F = T.instantiation(oracle, wv)[0]
        for integer in (False, True):
            recs, _, H, W = T.pf_cases(oracle, wv, 2, integer, True)
            words = T.occupancy_words(recs, H, W, F)
            assert words.shape == (T.PF_DISTINCT, 3, 2, 2)
            zero = float((words == 0).mean())
            assert 0.2 <= zero <= 0.8, (wv, integer, zero)
            full, _, _, _ = T.pf_cases(oracle, wv, 2, integer, False)
            assert (T.occupancy_words(full, H, W, F) != 0).all()
