"""The cut at a target quality across tiles, host side (no device): the rule of spiht_amd/alloc.py -- total_distortion,
allocate_target, allocate_target_layers, target_sqerr -- against literal restatements, cases worked out by hand and brute
force, and the checks of the new keyword that need no device."""
import itertools
import math

import numpy as np
import pytest

from alloc_cases import lengths
from target_cases import PINNED, all_slopes, dist_at, hulls_of, random_table, same_float


# ---- total_distortion ------------------------------------------------------------------------------------------------------

def literal_sum(values):
    """the order of alloc.total_distortion, in plain Python floats: 256 serial accumulators, the butterfly of each run of 64,
    the four results in order"""
    acc = [0.0] * 256
    for i, v in enumerate(values):
        acc[i % 256] = acc[i % 256] + float(v)
    for off in (32, 16, 8, 4, 2, 1):
        acc = [acc[i] + acc[i ^ off] for i in range(256)]
    assert all(acc[i] == acc[i & ~63] for i in range(256))
    return ((acc[0] + acc[64]) + acc[128]) + acc[192]


@pytest.mark.parametrize("T", [1, 63, 64, 255, 256, 257, 1500])
def test_total_distortion_is_the_literal_order(T):
    from spiht_amd import alloc
    rng = np.random.default_rng(T)
    v = rng.random(T) * 10.0 ** rng.integers(-8, 9, T)  # magnitudes far apart: another order gives other bits
    got = alloc.total_distortion(v)
    assert got == literal_sum(v.tolist()) and isinstance(got, float)
    assert alloc.total_distortion(v.tolist()) == got
    # integer values are converted with one rounding each
    big = [2 ** 60 + 1 + int(x) for x in rng.integers(0, 2 ** 40, T)]
    assert alloc.total_distortion(big) == literal_sum([float(x) for x in big])
    assert alloc.total_distortion(np.asarray(big, np.uint64)) == literal_sum([float(x) for x in big])


def test_total_distortion_edges_and_monotone():
    from spiht_amd import alloc
    assert alloc.total_distortion([]) == 0.0 and alloc.total_distortion([0.0] * 300) == 0.0
    assert alloc.total_distortion([1.5]) == 1.5 and alloc.total_distortion([1, 2, 3, 4]) == 10.0
    rng = np.random.default_rng(7)
    for T in (1, 5, 64, 257, 700):
        v = rng.random(T) * 10.0 ** rng.integers(-8, 9, T)
        base = alloc.total_distortion(v)
        for _ in range(40):  # raising one term never lowers the sum, lowering one never raises it
            i = int(rng.integers(0, T))
            up, down = v.copy(), v.copy()
            up[i] = math.nextafter(v[i], math.inf) if rng.random() < 0.5 else v[i] * (1 + rng.random())
            down[i] = math.nextafter(v[i], 0.0) if rng.random() < 0.5 else v[i] * rng.random()
            assert alloc.total_distortion(up) >= base >= alloc.total_distortion(down), (T, i)


# ---- allocate_target ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PINNED))
def test_pinned(name):
    from spiht_amd import alloc
    case = PINNED[name]
    for dt in (None, np.uint64, np.float64):
        D = case["D"] if dt is None else np.asarray(case["D"], dtype=dt)
        out, lam, dist, met = alloc.allocate_target(lengths(case), D, case["target"], case["budget"])
        assert out == case["want"] and lam == case["lam"] and same_float(dist, case["dist"]) and met is case["met"], \
            (out, lam, dist, met)
        assert sum(out) <= case["budget"]
        if case["dist"] is None:  # the budget binds: allocate, in every entry
            assert (out, lam) == alloc.allocate(lengths(case), D, case["budget"])


def linear_rule(R, D, target, budget):
    """allocate_target as the issue states it, by a scan over every candidate slope from the largest down"""
    from spiht_amd import alloc
    hulls = hulls_of(R, D)
    cand = all_slopes(hulls)
    ok = [s for s in cand if dist_at(hulls, s) <= target]
    mu = max(ok) if ok else min(cand)
    out = [0] * len(R)
    for s, _, end, t in alloc.hull_edges(R, D):
        if s >= mu:
            out[t] = max(out[t], end)
    if sum(out) <= budget:
        return out, mu, dist_at(hulls, mu), bool(ok)
    return alloc.allocate(R, D, budget) + (math.nan, False)


def targets_of(rng, hulls, n):
    """n falling targets around the vertex sums: one of them, just below one, between two, below the last"""
    slopes = all_slopes(hulls)
    picks = [dist_at(hulls, slopes[int(i)]) for i in rng.integers(0, len(slopes), n)]
    last = dist_at(hulls, slopes[-1])
    out = []
    for j, v in enumerate(picks):
        how = (j + int(rng.integers(0, 4))) % 4
        out.append(v if how == 0 else math.nextafter(v, 0.0) if how == 1 else v * 0.999 if how == 2 else last * 0.5)
    return sorted(out, reverse=True)


def test_random_tables():
    """320 tables, T <= 300, K <= 16, five falling targets each: within the budget; met implies dist <= target; the rows of
    allocate_target_layers nest and lam does not rise; the bisection is the literal scan; all three branches occur"""
    from spiht_amd import alloc
    rng = np.random.default_rng(20261)
    seen = {"vertices": 0, "budget": 0, "unreachable": 0}
    for i in range(320):
        small = i % 4 != 0
        T = int(rng.integers(1, 12 if small else 301))
        K = int(rng.integers(1, 17))
        nbytes, D = random_table(rng, T, K, 200 if small else 3000, integer=bool(i % 3 == 0))
        R = [alloc.tile_lengths(int(v), K) for v in nbytes]
        hulls = hulls_of(R, D)
        ends = sum(r[alloc.lower_hull(r, d)[-1]] for r, d in zip(R, D))
        budget = int(rng.integers(0, ends + 2)) if i % 2 else ends + 5
        targets = targets_of(rng, hulls, 5)
        cum, lams, dists, mets = alloc.allocate_target_layers(R, D, targets, budget)
        for q, target in enumerate(targets):
            one = alloc.allocate_target(R, D, target, budget)
            assert (cum[q], lams[q], mets[q]) == (one[0], one[1], one[3])
            assert same_float(dists[q], None if math.isnan(one[2]) else one[2])
            assert sum(cum[q]) <= budget, (i, q)
            if mets[q]:
                assert dists[q] <= target, (i, q)
                seen["vertices"] += 1
            elif math.isnan(dists[q]):
                assert (cum[q], lams[q]) == alloc.allocate(R, D, budget), (i, q)
                seen["budget"] += 1
            else:
                assert dists[q] > target and cum[q] == [r[alloc.lower_hull(r, d)[-1]] for r, d in zip(R, D)], (i, q)
                seen["unreachable"] += 1
            if q:
                assert all(a <= b for a, b in zip(cum[q - 1], cum[q])) and lams[q] <= lams[q - 1], (i, q)
            if small:
                want = linear_rule(R, D, target, budget)
                assert (cum[q], lams[q], mets[q]) == (want[0], want[1], want[3])
                assert same_float(dists[q], None if math.isnan(want[2]) else want[2])
    assert all(v >= 50 for v in seen.values()), seen


def test_brute_force():
    """T <= 3, K <= 4, integer D: a met result reaches the target, and no combination of grid points (hull vertices among them)
    of at most its bytes has a lower error -- it is a point of the picture's own lower hull, as allocate's cut is.

    The rule is the steepest EQUAL-SLOPE cut that reaches the target, not the cheapest combination of hull vertices that does:
    with the tiles R = [0, 10], D = [100, 0] (slope 10) and R = [0, 1], D = [9, 0] (slope 9) and the target 100, the second
    tile's one byte alone reaches it (error 100), but its slope is not the steepest, and the rule gives the first tile 10
    bytes (error 9).  Such a combination lies above the picture's hull between two equal-slope cuts; a cut by it would not
    nest with the cuts at other targets, which the layers need."""
    from spiht_amd import alloc
    assert alloc.allocate_target([[0, 10], [0, 1]], [[100, 0], [9, 0]], 100.0, 50) == ([10, 0], 10.0, 9.0, True)
    rng = np.random.default_rng(20262)
    met_cases = 0
    for _ in range(1500):
        T, K = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        R, D = [], []
        for t in range(T):
            r = alloc.tile_lengths(int(rng.integers(0, 7)), K)
            of = {v: int(rng.integers(0, 50)) for v in set(r)}
            R.append(r)
            D.append([of[v] for v in r])
        total0 = sum(d[0] for d in D)
        target = float(rng.integers(0, total0 + 2)) - (0.5 if rng.random() < 0.3 else 0.0)
        out, lam, dist, met = alloc.allocate_target(R, D, target, 10 ** 6)
        assert dist == sum(dict(zip(R[t], D[t]))[out[t]] for t in range(T))
        if not met:
            assert dist > target
            continue
        met_cases += 1
        assert dist <= target
        for ks in itertools.product(range(K + 1), repeat=T):
            if sum(R[t][k] for t, k in enumerate(ks)) <= sum(out):
                assert sum(D[t][k] for t, k in enumerate(ks)) >= dist, (R, D, target, ks)
        # and of the equal-slope cuts it is the cheapest that reaches the target: the next steeper one does not
        if lam != math.inf:
            steeper = [s for s in all_slopes(hulls_of(R, D)) if s > lam]
            assert dist_at(hulls_of(R, D), min(steeper)) > target
    assert met_cases > 500


# ---- target_sqerr, PSNR ------------------------------------------------------------------------------------------------------------

def test_target_sqerr():
    from spiht_amd import alloc, rd
    assert alloc.target_sqerr(30, 1.0, 3, 70 * 90) == float(3 * 6300) * 1.0 / 10.0 ** 3.0
    assert alloc.target_sqerr(30.5, 255, 1, 6300) == 6300.0 * (255.0 * 255.0) / 10.0 ** (30.5 / 10.0)
    assert alloc.target_sqerr(np.float32(20), 65535, 2, 10) == 20.0 * (65535.0 * 65535.0) / 100.0
    # a map of ones is no map
    ones = np.ones((70, 90), np.uint8)
    for db in (0, 17.3, 42):
        assert alloc.target_sqerr(db, 255, 3, int(ones.sum(dtype=np.int64))) == alloc.target_sqerr(db, 255, 3, 70 * 90)
    # a PSNR and back: the squared error at a target is that target's PSNR to rounding
    t = alloc.target_sqerr(33.0, 255, 3, 6300)
    assert abs(rd.psnr_of(t / (3 * 6300), 255) - 33.0) < 1e-9
    for bad in ("30", None, [30], True):
        with pytest.raises(TypeError):
            alloc.target_sqerr(bad, 1.0, 1, 10)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError):
            alloc.target_sqerr(bad, 1.0, 1, 10)
    with pytest.raises(ValueError):
        alloc.target_sqerr(30, 1.0, 1, 0)


def test_keyword_arguments():
    from spiht_amd import alloc
    assert alloc.target_psnr_arg(30, 3) == [30.0] * 3 and alloc.target_psnr_arg([30, 35.5], 2) == [30.0, 35.5]
    assert alloc.target_psnr_arg(np.array([1.0, 2.0]), 2) == [1.0, 2.0] and alloc.target_psnr_arg(np.float64(3), 1) == [3.0]
    with pytest.raises(ValueError):
        alloc.target_psnr_arg([30, 35], 3)
    with pytest.raises(ValueError):
        alloc.target_psnr_arg(math.nan, 1)
    for bad in ("30", None, [None], [True]):
        with pytest.raises(TypeError):
            alloc.target_psnr_arg(bad, 1)
    assert alloc.layer_targets_arg([30, 35, 40]) == [30.0, 35.0, 40.0] and alloc.layer_targets_arg((30,), 1) == [30.0]
    for bad in ([30, 30], [35, 30], [], [30, math.inf], list(range(256))):
        with pytest.raises(ValueError):
            alloc.layer_targets_arg(bad)
    with pytest.raises(ValueError):
        alloc.layer_targets_arg([30, 35], 3)
    for bad in (30, "30,35", [[30, 35]]):
        with pytest.raises(TypeError):
            alloc.layer_targets_arg(bad)
    with pytest.raises(ValueError):
        alloc.allocate_target_layers([[0, 1]], [[2, 1]], [1.0, 2.0], 5)
    with pytest.raises(ValueError):
        alloc.allocate_target([[0, 1]], [[2, 1]], 1.0, -1)


def test_the_package_exports_the_rule():
    import spiht
    import spiht_amd
    from spiht_amd import _lib, alloc
    assert spiht_amd.target_sqerr is alloc.target_sqerr and spiht.target_sqerr is alloc.target_sqerr
    assert "spiht_tile_allocate_target" in _lib.SYMBOLS
    a = spiht_amd.TileAllocation(1.0, [1, 2])
    assert (a.dist, a.psnr, a.met) == (None, None, None)


def test_target_psnr_needs_allocate_rd():
    """the checks of the keyword come before anything is uploaded or queued: run on a codec object that never got a context"""
    import inspect
    import spiht_amd
    tc = spiht_amd.TiledCodec.__new__(spiht_amd.TiledCodec)
    tc.allocate, tc.c, tc.H, tc.W, tc.th, tc.tw, tc.max_bits, tc.pixel_dtype = None, 1, 70, 90, 32, 32, 27005, np.dtype(np.float64)
    P = np.zeros((1, 70, 90))
    for call in (lambda: tc.encode(P, target_psnr=30), lambda: tc.encode_u8(P.astype(np.uint8), target_psnr=30),
                 lambda: tc.encode_u16(P.astype(np.uint16), target_psnr=[30]),
                 lambda: tc.encode_device(None, 1, None, None, None, d_target=0x1000),
                 lambda: tc.encode_layered(P, target_psnr=[30, 35])):
        with pytest.raises(ValueError):
            call()
    tc.allocate = "rd"
    for bad, exc in (([35, 30], ValueError), ([30, 30], ValueError), (30, TypeError), ("30,35", TypeError)):
        with pytest.raises(exc):
            tc.encode_layered(P, target_psnr=bad)
    with pytest.raises(ValueError):
        tc.encode_layered(P, 3, target_psnr=[30, 35])
    # every new keyword defaults to today's behaviour
    for name in ["encode", "encode_layered", "encode_image_tiled", "encode_image_layered"]:
        for suffix in ("", "_u8", "_u16"):
            owner = spiht_amd if name.startswith("encode_image") else spiht_amd.TiledCodec
            assert inspect.signature(getattr(owner, name + suffix)).parameters["target_psnr"].default is None
    assert inspect.signature(spiht_amd.TiledCodec.encode_device).parameters["d_target"].default is None
    assert inspect.signature(spiht_amd.TiledCodec.encode_layered_device).parameters["d_target"].default is None


def test_command_line_arguments():
    from spiht_amd.encode_decode import build_parser
    a = build_parser().parse_args(["x.png", "--tile", "32", "--allocate", "rd", "--psnr", "31.5", "--layer-psnr", "30,35,40"])
    assert (a.tile, a.allocate, a.psnr, a.layer_psnr) == (32, "rd", 31.5, "30,35,40")
    assert build_parser().parse_args(["x.png"]).layer_psnr is None
