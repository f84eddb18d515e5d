"""Region of interest, host side (no device): the two helpers that make and check a weight map, and what weighting a tile's row
of the table of distortions does to the unchanged rule of spiht_amd/alloc.py."""
import numpy as np
import pytest

from alloc_cases import PINNED, lengths


# ---- roi_arg ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.bool_, np.uint8])
def test_roi_arg_accepts_both_shapes(dtype):
    from spiht_amd import alloc
    rng = np.random.default_rng(1)
    for shape in [(7, 9), (3, 7, 9)]:
        m = rng.integers(0, 2 if dtype == np.bool_ else 256, shape).astype(dtype)
        out = alloc.roi_arg(m, 3, 7, 9)
        assert out.dtype == np.uint8 and out.shape == shape and out.flags.c_contiguous
        assert np.array_equal(out, m.astype(np.uint8))
    # a view that is not contiguous comes back contiguous; one picture takes [1, H, W] too
    big = rng.integers(0, 256, (7, 18)).astype(np.uint8)
    out = alloc.roi_arg(big[:, ::2], 1, 7, 9)
    assert out.flags.c_contiguous and np.array_equal(out, big[:, ::2])
    assert alloc.roi_arg(big[None, :, ::2], 1, 7, 9).shape == (1, 7, 9)


def test_roi_arg_rejects():
    from spiht_amd import alloc
    for dtype in (np.float64, np.float32, np.int64, np.int8, np.uint16):
        with pytest.raises(TypeError):
            alloc.roi_arg(np.ones((7, 9), dtype), 3, 7, 9)
    for shape in [(9, 7), (7, 8), (2, 7, 9), (4, 7, 9), (3, 1, 7, 9), (63,), ()]:
        with pytest.raises(ValueError):
            alloc.roi_arg(np.ones(shape, np.uint8), 3, 7, 9)


# ---- roi_map ------------------------------------------------------------------------------------------------------------------

def test_roi_map():
    from spiht_amd import alloc
    import spiht
    import spiht_amd
    assert spiht_amd.roi_map is alloc.roi_map and spiht.roi_map is alloc.roi_map
    m = alloc.roi_map(10, 12, [(2, 3, 4, 5)])
    want = np.ones((10, 12), np.uint8)
    want[2:6, 3:8] = 255
    assert m.dtype == np.uint8 and np.array_equal(m, want)
    # no box: the background; weight and background as given, 0 included
    assert np.array_equal(alloc.roi_map(3, 4, [], background=7), np.full((3, 4), 7, np.uint8))
    m = alloc.roi_map(10, 12, [(0, 0, 2, 2)], weight=9, background=0)
    assert m[:2, :2].tolist() == [[9, 9], [9, 9]] and int(m.sum()) == 36
    # clipping: a box that leaves the picture on every side, one that lies outside it, an empty one
    m = alloc.roi_map(10, 12, [(-3, -2, 5, 4), (8, 10, 50, 50), (20, 20, 3, 3), (-9, 0, 4, 4), (4, 4, 0, 3)], weight=3, background=1)
    want = np.ones((10, 12), np.uint8)
    want[:2, :2] = 3
    want[8:, 10:] = 3
    assert np.array_equal(m, want)
    # overlap: the larger weight holds, in either order of the boxes
    for boxes in ([(0, 0, 6, 6, 10), (3, 3, 6, 6, 200)], [(3, 3, 6, 6, 200), (0, 0, 6, 6, 10)]):
        m = alloc.roi_map(10, 12, boxes, background=1)
        want = np.ones((10, 12), np.uint8)
        want[:6, :6] = 10
        want[3:9, 3:9] = 200
        assert np.array_equal(m, want)
    # a box's own weight holds inside it, below the background too
    assert alloc.roi_map(4, 4, [(0, 0, 2, 2, 0)], background=5)[0, 0] == 0
    for bad in (dict(weight=256), dict(weight=-1), dict(background=256), dict(background=-1), dict(weight=1.5), dict(weight=True)):
        with pytest.raises(ValueError):
            alloc.roi_map(10, 12, [(0, 0, 2, 2)], **bad)
    with pytest.raises(ValueError):
        alloc.roi_map(10, 12, [(0, 0, 2, 2, 300)])
    with pytest.raises(ValueError):
        alloc.roi_map(10, 12, [(0, 0, 2)])


# ---- the rule on weighted tables ------------------------------------------------------------------------------------------------

def random_tables(count, seed):
    """integer tables on the shapes (nbytes, K) of the pinned cases: D a function of R, small enough that every weighted
    entry and every difference of two is exact in float64 and two different slopes never round to one"""
    from spiht_amd import alloc
    rng = np.random.default_rng(seed)
    shapes = [(c["nbytes"], c["K"]) for c in PINNED.values()]
    for _ in range(count):
        nbytes, K = shapes[int(rng.integers(len(shapes)))]
        R = [alloc.tile_lengths(n, K) for n in nbytes]
        D = []
        for r in R:
            of, level = {}, int(rng.integers(50, 1000))
            for v in sorted(set(r)):  # falls on the whole, not monotone
                of[v] = max(0, level + int(rng.integers(-20, 21)))
                level = level * int(rng.integers(20, 100)) // 100
            D.append([of[v] for v in r])
        yield R, D


def test_zero_weight_gets_no_bytes():
    """a tile whose row is scaled by 0 has D = 0 at every k: its hull is the vertex 0 and it gets no byte at any budget"""
    from spiht_amd import alloc
    assert alloc.lower_hull([0, 2, 4], [0, 0, 0]) == [0]
    for R, D in random_tables(60, 5):
        for t in range(len(R)):
            Dz = [row if u != t else [0] * len(row) for u, row in enumerate(D)]
            for budget in range(sum(r[-1] for r in R) + 1):
                out, _ = alloc.allocate(R, Dz, budget)
                assert out[t] == 0, (R, D, t, budget)
            for dt in (np.uint64, np.float64):
                assert alloc.allocate(R, np.asarray(Dz, dtype=dt), 5)[0][t] == 0


def test_weight_255_moves_bytes_one_way():
    """scaling one tile's row by 255 never lowers that tile's bytes and never raises another's: every budget from 0 to the
    sum of the streams, 240 random tables and the pinned ones.  (The allocation hands out min(delta R, rest) along the edges in
    the order (slope falling, tile rising); a scaled tile's edges only move forward in it.)"""
    from spiht_amd import alloc
    tables = list(random_tables(240, 6)) + [(lengths(c), c["D"]) for c in PINNED.values()]
    moved = 0
    for R, D in tables:
        for t in range(len(R)):
            Dw = [row if u != t else [255 * v for v in row] for u, row in enumerate(D)]
            for budget in range(sum(r[-1] for r in R) + 1):
                a, _ = alloc.allocate(R, D, budget)
                b, _ = alloc.allocate(R, Dw, budget)
                assert b[t] >= a[t], (R, D, t, budget)
                assert all(b[u] <= a[u] for u in range(len(R)) if u != t), (R, D, t, budget)
                moved += a != b
    assert moved > 1000  # the walk is not vacuous


def test_layers_of_a_weighted_table_nest():
    """allocate_layers on a table whose rows carry different weights (0 among them): the rows still nest, lambda* does not
    rise, and the last row is allocate's"""
    from spiht_amd import alloc
    rng = np.random.default_rng(7)
    for R, D in random_tables(200, 8):
        w = [int(v) for v in rng.choice([0, 1, 2, 17, 255], len(R))]
        Dw = [[w[t] * v for v in row] for t, row in enumerate(D)]
        total = sum(r[-1] for r in R)
        budgets = sorted(int(v) for v in rng.integers(0, total + 3, 4))
        cum, lams = alloc.allocate_layers(R, Dw, budgets)
        for q in range(1, 4):
            assert all(a <= b for a, b in zip(cum[q - 1], cum[q])) and lams[q - 1] >= lams[q], (R, Dw, budgets)
        assert (cum[-1], lams[-1]) == alloc.allocate(R, Dw, budgets[-1])
        assert all(cum[-1][t] == 0 for t in range(len(R)) if w[t] == 0)
