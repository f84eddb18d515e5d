"""Pinned cases of the cut at a target squared error, worked out by hand; shared by the CPU test of the rule
(spiht_amd/alloc.py: allocate_target) and the GPU test of the kernel (spiht_tile_allocate_target).

A case: nbytes, K, D -- as in alloc_cases; target -- the squared error to reach; budget -- the cap in bytes; want -- the bytes
per tile; lam, dist (None: NaN, the budget bound), met -- the rule's other results.  Every sum here is a small integer, exact in
any order.
"""
import math

from alloc_cases import _A, _B, _MIXED

# _A: lengths 0, 5, 10, D 100 40 10, slopes 12 and 6;  _B: D 100 50 30, slopes 10 and 4.  Tiles [_A, _B], slopes descending:
#   slope   inf   12   10    6    4
#   dist    200  140   90   60   40
#   cost      0    5   10   15   20
_AB = dict(nbytes=[10, 10], K=2, D=[_A, _B])
# [_A, _A, _B]: slope 12 in two tiles.  dist(inf) = 300, dist(12) = 40 + 40 + 100 = 180 at cost 10
_AAB = dict(nbytes=[10, 10, 10], K=2, D=[_A, _A, _B])
# _MIXED (alloc_cases): vertices' D  t0: 100 30 10 (slopes 17.5, 5), t1: 50 20 5 (30, 15), t2: 7, t3: 64 32 16 8 4 (32 16 8 4)
#   slope   inf   32   30  17.5   16   15    8    5    4
#   dist    221  189  159    89   73   58   50   30   26
#   cost      0    1    2     6    7    8    9   13   14
BELOW_90 = math.nextafter(90.0, 0.0)

PINNED = {
    "reached exactly at a vertex": dict(target=90.0, budget=100, want=[5, 5], lam=10.0, dist=90.0, met=True, **_AB),
    "one ulp below a vertex: the next slope": dict(target=BELOW_90, budget=100, want=[10, 5], lam=6.0, dist=60.0, met=True, **_AB),
    "equal slopes in two tiles, both taken": dict(target=200.0, budget=100, want=[5, 5, 0], lam=12.0, dist=180.0, met=True, **_AAB),
    "equal slopes, the budget binds": dict(target=200.0, budget=7, want=[5, 2, 0], lam=math.inf, dist=None, met=False, **_AAB),
    "a tile of zero D gets no bytes": dict(nbytes=[10, 10, 10], K=2, D=[_A, [0, 0, 0], _B], target=40.0, budget=100,
                                           want=[10, 0, 10], lam=4.0, dist=40.0, met=True),
    "target inf": dict(target=math.inf, budget=100, want=[0, 0], lam=math.inf, dist=200.0, met=True, **_AB),
    "target inf, budget 0": dict(target=math.inf, budget=0, want=[0, 0], lam=math.inf, dist=200.0, met=True, **_AB),
    "target 0, unreachable within the budget": dict(target=0.0, budget=100, want=[10, 10], lam=4.0, dist=40.0, met=False, **_AB),
    "target 0, reached": dict(nbytes=[10], K=2, D=[[100, 40, 0]], target=0.0, budget=10, want=[10], lam=8.0, dist=0.0, met=True),
    "target NaN": dict(target=math.nan, budget=100, want=[10, 10], lam=4.0, dist=40.0, met=False, **_AB),
    "target negative": dict(target=-1.0, budget=20, want=[10, 10], lam=4.0, dist=40.0, met=False, **_AB),
    "target NaN, the budget binds": dict(target=math.nan, budget=12, want=[7, 5], lam=10.0, dist=None, met=False, **_AB),
    "the budget binds": dict(target=60.0, budget=12, want=[7, 5], lam=10.0, dist=None, met=False, **_AB),
    "the budget fits exactly": dict(target=60.0, budget=15, want=[10, 5], lam=6.0, dist=60.0, met=True, **_AB),
    "mixed, target 73": dict(target=73.0, budget=1000, want=[4, 1, 0, 2], lam=16.0, dist=73.0, met=True, **_MIXED),
    "mixed, target 72.5": dict(target=72.5, budget=1000, want=[4, 2, 0, 2], lam=15.0, dist=58.0, met=True, **_MIXED),
    "mixed, target 58 at budget 7": dict(target=58.0, budget=7, want=[4, 1, 0, 2], lam=16.0, dist=None, met=False, **_MIXED),
    "mixed, unreachable": dict(target=25.0, budget=14, want=[8, 2, 0, 4], lam=4.0, dist=26.0, met=False, **_MIXED),
    "one empty tile": dict(nbytes=[0], K=3, D=[[9, 9, 9, 9]], target=5.0, budget=7, want=[0], lam=math.inf, dist=9.0, met=False),
    "one empty tile, met": dict(nbytes=[0], K=3, D=[[9, 9, 9, 9]], target=9.0, budget=7, want=[0], lam=math.inf, dist=9.0, met=True),
}


def same_float(a, b):
    """equal as the rule's dist: None stands for NaN"""
    if b is None:
        return isinstance(a, float) and math.isnan(a)
    return a == b


def random_table(rng, T, K, nmax=3000, integer=False):
    """one picture's curves, falling with noise (some points rise again, many lie above their hull): nbytes [T], D [T][K + 1]"""
    import numpy as np
    nbytes = rng.integers(0, nmax, T)
    nbytes[rng.random(T) < 0.05] = 0
    drop = rng.random((T, K + 1)) ** 3 * rng.integers(1, 1000, (T, 1))
    D = np.cumsum(drop[:, ::-1], axis=1)[:, ::-1] + rng.random((T, K + 1)) * 30
    if integer:
        D = (D * 2 ** 40).astype(np.uint64) + np.uint64(2 ** 60 + 1)  # every value above 2^53: the one rounding counts
    for t in range(T):  # D is a function of R: equal lengths share one distortion
        R = [-(-int(nbytes[t]) * k // K) for k in range(K + 1)]
        for k in range(1, K + 1):
            if R[k] == R[k - 1]:
                D[t, k] = D[t, k - 1]
    return nbytes, D


def hulls_of(R, D):
    """per tile (the hull edges' slopes, the hull vertices' distortions as float64), restated from lower_hull and slope"""
    from spiht_amd import alloc
    out = []
    for t in range(len(R)):
        Dt = alloc._f64(D[t])
        h = alloc.lower_hull(R[t], Dt)
        out.append(([alloc.slope(R[t], Dt, a, b) for a, b in zip(h, h[1:])], [Dt[k] for k in h]))
    return out


def dist_at(hulls, s):
    """the rule's dist(s), restated: every tile at its last hull vertex over edges of slope >= s"""
    from spiht_amd import alloc
    return alloc.total_distortion([vD[sum(1 for x in sl if x >= s)] for sl, vD in hulls])


def all_slopes(hulls):
    """inf and every edge slope, descending"""
    return [math.inf] + sorted({x for sl, _ in hulls for x in sl}, reverse=True)
