"""Pinned cases of the rate allocation across tiles, worked out by hand; shared by the CPU test of the rule
(spiht_amd/alloc.py) and the GPU test of the kernel (spiht_tile_allocate).

A case: nbytes -- the tiles' full stream lengths; K -- points; D -- [T][K + 1] distortions at alloc.tile_lengths(nbytes[t], K);
budget -- bytes; want -- the bytes per tile; lam -- lambda*.
"""
import math

# two edges per tile of 10 bytes at K = 2: lengths 0, 5, 10; slopes (100 - 40) / 5 = 12 and (40 - 10) / 5 = 6
_A = [100, 40, 10]
# slopes 10 and 4
_B = [100, 50, 30]

# four tiles at K = 4:
#   0: 8 bytes, lengths 0 2 4 6 8, D not monotone: 120 and 50 are skipped; edges 17.5 (to 4) and 5 (to 8)
#   1: 2 bytes, lengths 0 1 1 2 2 (duplicates, n < K); edges 30 (to 1) and 15 (to 2)
#   2: an empty stream; no edge
#   3: 4 bytes, lengths 0 1 2 3 4; edges 32, 16, 8, 4
# cost by slope, descending: 32 -> 1, 30 -> 2, 17.5 -> 6, 16 -> 7, 15 -> 8, 8 -> 9, 5 -> 13, 4 -> 14
_MIXED = dict(nbytes=[8, 2, 0, 4], K=4, D=[[100, 120, 30, 50, 10], [50, 20, 20, 5, 5], [7, 7, 7, 7, 7], [64, 32, 16, 8, 4]])

PINNED = {
    "below the first edge": dict(nbytes=[10, 10], K=2, D=[_A, _B], budget=3, want=[3, 0], lam=math.inf),
    "above every hull": dict(nbytes=[10, 10], K=2, D=[_A, _B], budget=100, want=[10, 10], lam=4.0),
    "equal slopes, first edges": dict(nbytes=[10, 10, 10], K=2, D=[_A, _A, _A], budget=12, want=[5, 5, 2], lam=math.inf),
    "equal slopes, second edges": dict(nbytes=[10, 10, 10], K=2, D=[_A, _A, _A], budget=22, want=[10, 7, 5], lam=12.0),
    "equal slopes, exact fit": dict(nbytes=[10, 10, 10], K=2, D=[_A, _A, _A], budget=15, want=[5, 5, 5], lam=12.0),
    "mixed, budget 11": dict(budget=11, want=[6, 2, 0, 3], lam=8.0, **_MIXED),
    "mixed, budget 5": dict(budget=5, want=[3, 1, 0, 1], lam=30.0, **_MIXED),
    "mixed, budget 0": dict(budget=0, want=[0, 0, 0, 0], lam=math.inf, **_MIXED),
    "mixed, budget 14": dict(budget=14, want=[8, 2, 0, 4], lam=4.0, **_MIXED),
    "mixed, budget 1000": dict(budget=1000, want=[8, 2, 0, 4], lam=4.0, **_MIXED),
    "one tile": dict(nbytes=[10], K=2, D=[_A], budget=7, want=[7], lam=12.0),
    "one empty tile": dict(nbytes=[0], K=3, D=[[9, 9, 9, 9]], budget=7, want=[0], lam=math.inf),
    # slopes that are not exact in binary: (10 - 3) / 3 against 7 / 3 of another tile -- equal after one rounding each
    "thirds": dict(nbytes=[3, 6], K=1, D=[[10, 3], [20, 6]], budget=4, want=[3, 1], lam=math.inf),
}


def lengths(case):
    from spiht_amd import alloc
    return [alloc.tile_lengths(n, case["K"]) for n in case["nbytes"]]
