"""CPU tests of the rate-distortion module (spiht_amd/rd.py): the search, the default grid of lengths, the grouping
arithmetic, the curve's formulas and the argument checks.  No device: the search runs against made-up curves."""
import math

import numpy as np
import pytest

from spiht_amd import rd
from spiht_amd.rd import default_lengths, group_size, search_cut, search_rounds_bound


class Curve:
    """a made-up curve: value(length), with the calls and everything asked for counted"""

    def __init__(self, value):
        self.value, self.calls, self.asked = value, 0, []

    def __call__(self, lengths):
        self.calls += 1
        self.asked.append(list(lengths))
        return [self.value(k) for k in lengths]


def _contract(curve, n, target, length, met):
    """what cut_to_psnr promises of the length it returns"""
    if not met:
        assert length == n and curve.value(n) < target
        return
    assert curve.value(length) >= target
    assert length == 0 or curve.value(length - 1) < target


@pytest.mark.parametrize("points", [1, 2, 32])
@pytest.mark.parametrize("n", [1, 7, 1000, 130000])
def test_search_monotone_curve_and_number_of_calls(n, points):
    """a monotone curve: the smallest passing length, whatever the target; and the number of curve calls.  The whole stream
    is looked at first (one call: without it `met` is not known, and with n = 1, points = 1 no search can tell both
    psnr(1) and psnr(0) in ceil(log 2 / log 2) = 1 call); the rounds after it number at most
    ceil(log(n + 1) / log(points + 1))."""
    bound = math.ceil(math.log(n + 1) / math.log(points + 1) - 1e-12)
    assert search_rounds_bound(n, points) == bound
    for first_pass in sorted({0, 1, n // 3, n // 2, n - 1, n}):
        curve = Curve(lambda k: 20.0 + (10.0 if k >= first_pass else 0.0) + k * 1e-9)
        length, value, met = search_cut(n, points, curve, lambda v: v >= 30.0)
        assert (length, met) == (first_pass, True) and value == curve.value(first_pass)
        assert curve.asked[0] == [n] and curve.calls - 1 <= bound, (curve.calls, bound)
        assert all(1 <= len(a) <= points for a in curve.asked)
        assert all(a == sorted(set(a)) and 0 <= a[0] and a[-1] <= n for a in curve.asked)


@pytest.mark.parametrize("points", [1, 2, 32])
def test_search_curve_with_a_dip(points):
    """one dip below the target after the curve first passed it: a crossing comes back, not necessarily the first"""
    n, target = 1000, 30.0

    def value(k):
        if k < 200:
            return 10.0 + k * 0.05
        return 25.0 if 400 <= k < 450 else 31.0 + k * 0.001
    curve = Curve(value)
    length, v, met = search_cut(n, points, curve, lambda x: x >= target)
    _contract(curve, n, target, length, met)
    assert met and length in (200, 450) and v == value(length)
    assert curve.calls - 1 <= search_rounds_bound(n, points)


def test_search_edges():
    # a target above what the whole stream reaches: the whole stream, not met, one call
    curve = Curve(lambda k: 0.01 * k)
    assert search_cut(500, 32, curve, lambda v: v >= 99.0) == (500, 5.0, False) and curve.calls == 1
    # target -inf: every length passes, the empty prefix comes back
    curve = Curve(lambda k: 0.01 * k)
    assert search_cut(500, 32, curve, lambda v: v >= -math.inf) == (0, 0.0, True)
    _contract(curve, 500, -math.inf, 0, True)
    # an empty stream: one call, length 0 either way
    for target, met in ((-1.0, True), (1.0, False)):
        curve = Curve(lambda k: 0.0)
        assert search_cut(0, 4, curve, lambda v: v >= target) == (0, 0.0, met) and curve.calls == 1
    # a non-increasing curve and "at most": the search of cut_to_sqerr, smallest length with E <= bound
    err = Curve(lambda k: max(0, 10 ** 30 - k * 10 ** 27))
    assert search_cut(2000, 5, err, lambda v: v <= 5 * 10 ** 29) == (500, 5 * 10 ** 29, True)
    with pytest.raises(ValueError):
        search_cut(10, 0, err, lambda v: True)


def test_default_lengths():
    for n in (1, 2, 5, 31, 32, 33, 400, 129600):
        for points in (1, 2, 7, 32):
            g = default_lengths(n, points)
            assert g[-1] == n and g[0] >= 1 and all(a < b for a, b in zip(g, g[1:])), (n, points)
            assert len(g) == min(n, points), (n, points, g)
            # evenly spaced: no step more than one above another
            steps = [b - a for a, b in zip([0] + g, g)]
            assert max(steps) - min(steps) <= 1
    assert default_lengths(0, 32) == [0]
    with pytest.raises(ValueError):
        default_lengths(10, 0)


def test_group_size():
    per = 3 * (1111 * 1949 * 4 + 1080 * 1920 * 8)
    assert group_size(3, 1111, 1949, 1080, 1920, 2 ** 31) == 2 ** 31 // per >= 1
    assert group_size(3, 1111, 1949, 1080, 1920, per) == 1 and group_size(3, 1111, 1949, 1080, 1920, 2 * per - 1) == 1
    assert group_size(3, 1111, 1949, 1080, 1920, 2 * per) == 2
    # at least one, however small the bound
    assert group_size(3, 1111, 1949, 1080, 1920, 0) == 1 and group_size(1, 4096, 4096, 4096, 4096, 1000) == 1


def test_curve_formulas():
    c, h, w = 3, 5, 7
    lens, n = [9, 0, 4, 4], 6
    # float pixels
    sse = [[0.5, 0.25, 0.125], [3.0, 2.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    cv = rd.curve_from_sums(lens, n, [0, 2 ** 90, 7, 7], sse, c, h, w, 1.0)
    assert cv.byte_lengths == lens and cv.bits == [48, 0, 32, 32] and cv.bpp == [48 / 35, 0.0, 32 / 35, 32 / 35]
    assert cv.coef_sqerr == [0, 2 ** 90, 7, 7] and all(type(e) is int for e in cv.coef_sqerr)
    assert cv.mse == [0.875 / 105, 6.0 / 105, 0.0, 0.0]
    assert cv.psnr[0] == 10 * math.log10(1.0 / (0.875 / 105)) and cv.psnr[2:] == [math.inf, math.inf]
    # integer pixels: Python ints, peak 255 / 65535
    cv = rd.curve_from_sums([1], 1, [1], [[10, 20, 33]], c, h, w, 255)
    assert cv.mse == [63 / 105] and cv.psnr == [10 * math.log10(255.0 * 255.0 / (63 / 105))]
    big = 65535 ** 2 * 2 ** 29
    cv = rd.curve_from_sums([1], 1, [1], [[big, big, big]], 3, 2 ** 15, 2 ** 14, 65535)
    assert cv.mse == [float(65535 ** 2)] and cv.psnr == [0.0]
    assert rd.PEAK[None] == 1.0 and rd.PEAK[np.dtype(np.uint8)] == 255 and rd.PEAK[np.dtype(np.uint16)] == 65535


def test_argument_errors_before_any_device_work():
    """lengths, points and targets are checked on the host: these raise with or without a GPU"""
    import spiht_amd
    img = np.zeros((1, 16, 16))
    res = spiht_amd.EncodingResult(b"\x00" * 8, 16, 16, 1, 3, None)
    for fn, im in ((spiht_amd.rd_curve, img), (spiht_amd.rd_curve_u8, img.astype(np.uint8)),
                   (spiht_amd.rd_curve_u16, img.astype(np.uint16))):
        with pytest.raises(ValueError):
            fn(im, result=res, byte_lengths=[3, -1])
        with pytest.raises(ValueError):
            fn(im, result=res, points=0)
        with pytest.raises(TypeError):
            fn(im, result=res, byte_lengths=[1.5])
    for fn in (spiht_amd.cut_to_psnr, spiht_amd.cut_to_psnr_u8, spiht_amd.cut_to_psnr_u16):
        with pytest.raises(ValueError):
            fn(img, res, float("nan"))
        with pytest.raises(ValueError):
            fn(img, res, 30.0, points=0)
    import spiht
    assert spiht.rd_curve is spiht_amd.rd_curve and spiht.cut_to_psnr is spiht_amd.cut_to_psnr and spiht.RDCurve is rd.RDCurve
