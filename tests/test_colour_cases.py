"""The host half of the colour anchor (no GPU): tests/colour_cases.py's sets hold to their purpose, the host build of csrc/spow.h
stays within stated units in the last place of 60-digit arithmetic on them, its special cases are exact, and color3_rule -- the
restatement tests/test_gpu_colour.py holds the device kernel to, bit for bit -- is the published transform."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

import colour_cases as K

TWO = Decimal(2)


def exact_pow(x, p):
    """x^p for the float64 numbers x > 0 and p, to 60 digits (as tests/test_oracle.py::test_colour_power_function_accuracy)"""
    getcontext().prec = 60
    fp, fx = Fraction(p), Fraction(x)
    return (Decimal(fp.numerator) / Decimal(fp.denominator) * (Decimal(fx.numerator) / Decimal(fx.denominator)).ln()).exp()


_EXACT = {}


def exact_results(p):
    """power_inputs() -> their exact results, computed once per exponent"""
    if p not in _EXACT:
        _EXACT[p] = [exact_pow(float(x), p) for x in K.power_inputs()]
    return _EXACT[p]


def test_cases_hold_to_their_purpose():
    """every table interval at both of its ends; subnormal inputs; for p = 1 / 0.43 at least 20 inputs whose exact result is
    subnormal and one whose exact result is below 2^-1075, where the function must return 0"""
    sets = K.fixed_power_inputs()
    t = sets["table"]
    mant = K.bits(t) & np.uint64(0xFFFFFFFFFFFFF)
    idx = K.table_interval(t)
    for i in range(64):
        assert ((idx == i) & (mant == np.uint64(i << 46))).sum() == len(K.TABLE_EXPONENTS)
        assert ((idx == i) & (mant == np.uint64(((i + 1) << 46) - 1))).sum() == len(K.TABLE_EXPONENTS)
    x = K.power_inputs()
    assert (x > 0).all() and np.isfinite(x).all() and len(np.unique(x)) >= len(x) - 8
    assert 4000 <= sum(len(v) for v in sets.values()) <= 4100 and len(x) >= 6000
    assert ((x < 2.0 ** -1022)).sum() >= 5
    ref = exact_results(1 / 0.43)
    sub = [r for r in ref if TWO ** -1075 <= r < TWO ** -1022]
    gone = [k for k, r in enumerate(ref) if r < TWO ** -1075]
    assert len(sub) >= 20 and gone
    assert (K.host_spow()(x[gone], 1 / 0.43) == 0.0).all()
    px = K.pixel_inputs()
    assert all(v.shape[0] == 3 and v.dtype == np.float64 for v in px.values())
    assert all(((px[k] >= 0) & (px[k] <= 1)).all() for k in K.UNIT_SETS)
    assert (px["negative"] < 0).any() and (px["above_one"] > 1).all() and (px["above_one"] <= 4).all()
    assert (np.abs(px["subnormal"]) < 2.0 ** -1022).all() and (px["subnormal"] != 0).all()
    assert (np.abs(px["tiny"]) < 1e-299).all() and (np.abs(px["tiny"]) >= 1e-300).all()
    corners = {tuple(c) for c in px["zero_one"].T[:8]}
    assert len(corners) == 8
    # the way back: the scaled triples do hand the power function negative LMS values
    from spiht_amd import color_models
    back = K.back_inputs(K.host_spow())
    A = color_models._params("IPT", "RGB")[0]
    assert all(np.isfinite(v).all() and v.shape[0] == 3 for v in back.values())
    assert ((A @ back["coarse"]) < 0).sum() >= 100 and ((A @ back["negative_wide"]) < 0).sum() >= 1000
    pics = K.route_pictures()
    assert [p.shape for p in pics] == [(3, 33, 47), (3, 67, 131)]
    for p in pics:
        assert (p < 0).any() and (p > 1).any() and (p == 0).any() and ((p != 0) & (np.abs(p) < 1e-299)).any()


@pytest.mark.parametrize("p,bound", [(0.43, 1.5), (1 / 0.43, 3.5)], ids=["fwd", "back"])
def test_power_function_against_60_digits(p, bound):
    """csrc/spow.h, host build, on power_inputs() against 60-digit arithmetic.  Normal results: under 1.5 ulp for p = 0.43 and under
    3.5 ulp for p = 1 / 0.43 (the bounds of tests/test_oracle.py, kept); subnormal results: at most 1 ulp of the subnormal spacing
    (the final sum and the ldexp are two roundings of at most half an ulp each); an exact result past the largest number is inf.
    Measured on this set (7012 inputs: 4012 fixed, 3000 seeded random), the worst of each class printed by the test:
    p = 0.43: fixed inputs 1.134 ulp at 0x1.b1b1b1b1b1b1bp-1 (= 216 / 255), random ones 1.140 at 0x1.d5d31bc720ec6p-1; no
    subnormal result.  p = 1 / 0.43: fixed inputs 2.860 ulp at 0x1.fffffffffffe7p-1 (1 - 25 ulp), random ones 3.184 at
    0x1.ffa9b25580895p-1 (just under 1, where the older test measured its 3.5 too); subnormal results 0.495 ulp of their spacing at
    0x1.c800000000001p-452.  No class of the new inputs goes over the bounds the older test's random inputs were measured under,
    so none is held to the 4 ulp csrc/spow.h documents instead."""
    spow = K.host_spow()
    x = K.power_inputs()
    got = spow(x, p)
    ref = exact_results(p)
    big = Decimal(K.DBL_MAX) + TWO ** 970           # halfway to 2^1024: from here on the correctly rounded result is inf
    sets = dict(K.fixed_power_inputs(), random=K.random_power_inputs())
    name = np.repeat(list(sets), [len(v) for v in sets.values()])
    worst, worst_sub = {k: (0.0, "-") for k in sets}, (0.0, "-")
    for xi, g, r, k in zip(x, got, ref, name):
        xi, g = float(xi), float(g)
        if r >= big or math.isinf(g):
            assert math.isinf(g) and r > Decimal(K.DBL_MAX) * (1 - TWO ** -50), (xi.hex(), g)
            continue
        if r < TWO ** -1022:
            worst_sub = max(worst_sub, (float(abs(Decimal(g) - r) / TWO ** -1074), xi.hex()))
        else:
            worst[k] = max(worst[k], (float(abs(Decimal(g) - r) / Decimal(math.ulp(float(r)))), xi.hex()))
    print("spow, p = %.17g, %d inputs, worst ulp: %s; on subnormal results %.3f at %s"
          % (p, len(x), ", ".join("%s %.3f at %s" % ((k,) + v) for k, v in worst.items()), *worst_sub))
    worst = max(worst.values())
    assert worst[0] < bound, worst
    assert worst_sub[0] <= 1.0, worst_sub


def test_power_function_exact_cases():
    """spow(+-0) = +0; odd symmetry on the whole set; NaN stays NaN, infinities pass through; 1^p = 1; (-8)^(1/3) = -2"""
    spow = K.host_spow()
    x = K.power_inputs()
    for p in K.DEVICE_EXPONENTS:
        z = spow(np.array([0.0, -0.0]), p)
        assert (K.bits(z) == 0).all(), p
        assert (K.bits(spow(-x, p)) == K.bits(-spow(x, p))).all(), p
        s = spow(np.array([np.nan, np.inf, -np.inf, 1.0, -1.0]), p)
        assert np.isnan(s[0]) and s[1] == np.inf and s[2] == -np.inf and s[3] == 1.0 and s[4] == -1.0, p
    assert spow(np.array([-8.0]), 1 / 3.0)[0] == -2.0
    assert spow(np.array([K.DBL_MAX]), 2.3)[0] == np.inf
    assert (spow(np.array([5e-324, -5e-324]), 1 / 0.43) == 0.0).all()


def test_colour_rule_is_the_published_transform():
    """color3_rule with the real matrices and the host build of the power function against color_models.convert (numpy's pow)
    within 1e-12 on the [0, 1] part of pixel_inputs(), both ways and for both selectable RGB / XYZ pairs; the round trip
    RGB -> IPT -> RGB with the derived pair returns the input to rounding.  (Parity with colour-science itself stays unpinned: the
    package is not available; convert() is the published Ebner-Fairchild transform.)"""
    from spiht_amd import color_models
    spow = K.host_spow()
    px = K.pixel_inputs()
    unit = np.concatenate([px[k] for k in K.UNIT_SETS], axis=1)
    prev = color_models.set_rgb_xyz("iec")
    try:
        for pair in ("iec", "lindbloom"):
            color_models.set_rgb_xyz(pair)
            ipt = K.color3_rule(unit, *color_models._params("RGB", "IPT"), spow)
            host = color_models.convert(unit[:, None, :], "RGB", "IPT")[:, 0, :]
            assert np.abs(ipt - host).max() < 1e-12, pair
            rgb = K.color3_rule(ipt, *color_models._params("IPT", "RGB"), spow)
            assert np.abs(rgb - color_models.convert(ipt[:, None, :], "IPT", "RGB")[:, 0, :]).max() < 1e-12, pair
            if pair == "lindbloom":   # (the standard's printed inverse matrix is not the numerical inverse: 4th decimal)
                assert np.abs(rgb - unit).max() < 1e-13, float(np.abs(rgb - unit).max())
    finally:
        color_models.set_rgb_xyz(prev)
