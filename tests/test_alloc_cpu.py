"""The rate allocation across tiles, host side (no device): the rule of spiht_amd/alloc.py against brute force and against
cases worked out by hand, the ceiling, the container with uneven lengths, and the checks of the three keywords."""
import itertools
import math

import numpy as np
import pytest

from alloc_cases import PINNED, lengths


def test_brute_force_3000_random_cases():
    """T <= 3, K <= 4, integer D that is a function of R.  The lengths add up to min(budget, the hulls' ends), and the
    allocation over the edges of slope >= lambda* is not beaten by any combination of grid points of at most its total rate."""
    from spiht_amd import alloc
    rng = np.random.default_rng(20260)
    for _ in range(3000):
        T, K = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        R, D = [], []
        for t in range(T):
            r = alloc.tile_lengths(int(rng.integers(0, 7)), K)
            of = {v: int(rng.integers(0, 50)) for v in set(r)}
            R.append(r)
            D.append([of[v] for v in r])
        budget = int(rng.integers(0, sum(r[-1] for r in R) + 3))
        out, lam = alloc.allocate(R, D, budget)
        hulls = [alloc.lower_hull(R[t], D[t]) for t in range(T)]
        assert sum(out) == min(budget, sum(R[t][hulls[t][-1]] for t in range(T))), (R, D, budget)
        # the vertices reached over edges of slope >= lambda*
        base = [0] * T
        for s, _, end, t in alloc.hull_edges(R, D):
            if s >= lam:
                base[t] = max(base[t], end)
        assert sum(base) <= budget and all(b <= o for b, o in zip(base, out))
        of = [dict(zip(R[t], D[t])) for t in range(T)]
        rate, dist = sum(base), sum(of[t][base[t]] for t in range(T))
        for ks in itertools.product(range(K + 1), repeat=T):
            if sum(R[t][k] for t, k in enumerate(ks)) <= rate:
                assert sum(D[t][k] for t, k in enumerate(ks)) >= dist, (R, D, budget, ks)


@pytest.mark.parametrize("name", list(PINNED))
def test_pinned(name):
    from spiht_amd import alloc
    case = PINNED[name]
    out, lam = alloc.allocate(lengths(case), case["D"], case["budget"])
    assert out == case["want"] and lam == case["lam"]
    # the same from a uint64 table (exact sums of integer pixels) and a float64 one
    for dt in (np.uint64, np.float64):
        assert alloc.allocate(lengths(case), np.asarray(case["D"], dtype=dt), case["budget"]) == (out, lam)


def test_hull_of_a_curve_that_is_not_monotone():
    from spiht_amd import alloc
    assert alloc.tile_lengths(8, 4) == [0, 2, 4, 6, 8] and alloc.tile_lengths(2, 4) == [0, 1, 1, 2, 2]
    assert alloc.tile_lengths(0, 3) == [0, 0, 0, 0] and alloc.tile_lengths(333, 16)[-1] == 333
    assert alloc.lower_hull([0, 2, 4, 6, 8], [100, 120, 30, 50, 10]) == [0, 2, 4]
    assert alloc.lower_hull([0, 1, 1, 2, 2], [50, 20, 20, 5, 5]) == [0, 1, 3]
    assert alloc.lower_hull([0, 0, 0], [7, 7, 7]) == [0]
    # a point above the chord is popped: slopes 10, then 50 -> the chord's 30
    assert alloc.lower_hull([0, 1, 2], [100, 90, 40]) == [0, 2]
    # a sum above 2^53 is rounded once
    big = 2 ** 60 + 1
    assert alloc.slope([0, 4], [big, 0], 0, 1) == float(big) / 4.0


def test_ceiling():
    from spiht_amd import alloc
    for max_bits, T, spread in [(27005, 12, 4.0), (12000, 6, 4.0), (27005, 9, 1.0), (27005, 2, 8.0), (100, 7, 1.5), (7, 3, 4.0)]:
        ceil = alloc.ceiling_bits(max_bits, T, spread)
        assert ceil % 8 == 0 and ceil <= max_bits and ceil <= spread * (max_bits // T)
        assert ceil + 8 > min(max_bits, math.floor(spread * (max_bits // T)))
    assert alloc.ceiling_bits(27005, 12, 4.0) == 9000 and alloc.ceiling_bits(27005, 2, 8.0) == 27000


def test_container_with_uneven_lengths():
    import spiht_amd
    rng = np.random.default_rng(3)
    nbytes = [0, 1, 700, 3, 0, 41]
    r = spiht_amd.TiledResult(40, 90, 3, 32, 32, 2, [5, 0, 7, 6, 0, 9], nbytes, rng.bytes(sum(nbytes)))  # 2 x 3 tiles
    back = spiht_amd.TiledResult.from_bytes(r.to_bytes())
    assert back == r
    off = np.concatenate(([0], np.cumsum(nbytes)))
    for t in range(6):
        assert back.tile(t // 3, t % 3).encoded_bytes == r.encoded_bytes[off[t]:off[t + 1]]


def test_keyword_checks_come_before_a_context():
    """every refusal here is a ValueError / TypeError of the host checks -- also on a machine with no device, where asking for
    a context would raise something else"""
    import spiht_amd
    P = np.zeros((1, 70, 90))
    s = spiht_amd.SpihtSettings()
    for kw, exc in [(dict(allocate="equal"), ValueError), (dict(allocate=True), ValueError),
                    (dict(allocate="rd", max_bits=None), ValueError),
                    (dict(allocate="rd", points=0), ValueError), (dict(allocate="rd", points=256), ValueError),
                    (dict(allocate="rd", points=8.0), TypeError), (dict(allocate="rd", points=True), TypeError),
                    (dict(points=0), ValueError),
                    (dict(allocate="rd", spread=0.5), ValueError), (dict(allocate="rd", spread=float("nan")), ValueError),
                    (dict(allocate="rd", spread=float("inf")), ValueError), (dict(allocate="rd", spread="4"), TypeError),
                    (dict(allocate="rd", pixel_dtype=np.float32), ValueError)]:
        args = dict(max_bits=27005)
        args.update(kw)
        with pytest.raises(exc):
            spiht_amd.TiledCodec(1, 70, 90, 32, s, 2, **args)
        if "pixel_dtype" not in kw:
            with pytest.raises(exc):
                spiht_amd.encode_image_tiled(P, 32, s, 2, **args)
            with pytest.raises(exc):
                spiht_amd.encode_image_tiled_u8(P.astype(np.uint8), 32, s, 2, **args)
    with pytest.raises(ValueError):
        spiht_amd.encode_image_tiled(P.astype(np.float32), 32, s, 2, 27005, allocate="rd")
