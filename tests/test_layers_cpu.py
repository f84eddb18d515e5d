"""Quality layers of a tiled picture without a device: the allocations at growing budgets nest (the property the layer-major
container stands on), the budgets of the layers, and the container -- round trip, every prefix, every refusal."""
import math
import struct

import numpy as np
import pytest

from alloc_cases import _MIXED, PINNED, lengths


# ---- the rule ----------------------------------------------------------------------------------------------------------------

def random_curves(rng):
    """T <= 6 tiles at K <= 6 points: integer distortions with many tied slopes, or float curves that are not monotone"""
    from spiht_amd import alloc
    T, K = int(rng.integers(1, 7)), int(rng.integers(1, 7))
    nbytes = [int(v) for v in rng.integers(0, 31, T)]
    R = [alloc.tile_lengths(n, K) for n in nbytes]
    if rng.random() < 0.5:
        D = [[int(v) for v in np.cumsum(rng.integers(0, 4, K + 1))[::-1] * 6] for _ in range(T)]  # small multiples: ties
        if rng.random() < 0.5:
            D = [[v + int(rng.integers(0, 2)) * 6 for v in row] for row in D]  # some points rise again
    else:
        D = [[float(v) for v in np.cumsum(rng.random(K + 1) ** 2)[::-1] * 50 + rng.random(K + 1) * 8] for _ in range(T)]
    for t in range(T):  # D is a function of R: equal lengths share one distortion
        for k in range(1, K + 1):
            if R[t][k] == R[t][k - 1]:
                D[t][k] = D[t][k - 1]
    return R, D


def test_allocations_nest():
    """2000 random tables, every budget from 0 to the hull ends + 2: no tile's length falls as the budget grows, lambda* does
    not rise, and the sum is min(budget, the hull ends) -- so at most the budget"""
    from spiht_amd import alloc
    rng = np.random.default_rng(2024)
    pairs = 0
    for _ in range(2000):
        R, D = random_curves(rng)
        ends = sum(r[alloc.lower_hull(r, d)[-1]] for r, d in zip(R, D))
        prev, prev_lam = [0] * len(R), math.inf
        for budget in range(ends + 3):
            out, lam = alloc.allocate(R, D, budget)
            assert all(a <= b for a, b in zip(prev, out)), (R, D, budget)
            assert lam <= prev_lam, (R, D, budget)
            assert sum(out) == min(budget, ends) <= budget, (R, D, budget)
            prev, prev_lam = out, lam
            pairs += 1
    assert pairs > 80000


def test_allocate_layers_pinned_rows():
    from spiht_amd import alloc
    budgets = [0, 5, 11, 14, 1000]
    cum, lams = alloc.allocate_layers(lengths(_MIXED), _MIXED["D"], budgets)
    for q, b in enumerate(budgets):
        pin = PINNED["mixed, budget %d" % b]
        assert cum[q] == pin["want"] and lams[q] == pin["lam"], b
    assert all(a <= b for lo, hi in zip(cum, cum[1:]) for a, b in zip(lo, hi))
    assert cum[-1] == alloc.allocate(lengths(_MIXED), _MIXED["D"], 1000)[0]
    seven = alloc.allocate(lengths(_MIXED), _MIXED["D"], 7)
    assert alloc.allocate_layers(lengths(_MIXED), _MIXED["D"], [7, 7]) == ([seven[0]] * 2, [seven[1]] * 2)  # an empty layer
    with pytest.raises(ValueError):
        alloc.allocate_layers(lengths(_MIXED), _MIXED["D"], [5, 4])
    with pytest.raises(ValueError):
        alloc.allocate_layers(lengths(_MIXED), _MIXED["D"], [-1, 4])


def test_layer_budgets():
    from spiht_amd import alloc
    assert alloc.layer_budgets(27005, 1) == [27005]
    assert alloc.layer_budgets(27005, 4) == [3375, 6751, 13502, 27005]
    assert alloc.layer_budgets(27005, np.int64(2)) == [13502, 27005]
    assert alloc.layer_budgets(255, 8) == [1, 3, 7, 15, 31, 63, 127, 255]
    assert alloc.layer_budgets(0, 1) == [0] and alloc.layer_budgets(0, [0]) == [0]
    assert alloc.layer_budgets(27005, [3000, 9000, 27005]) == [3000, 9000, 27005]
    assert alloc.layer_budgets(27005, (0, np.int32(8), 27005)) == [0, 8, 27005]
    assert alloc.layer_budgets(2 ** 300, 255)[0] == 2 ** 46 and len(alloc.layer_budgets(2 ** 300, 255)) == 255
    assert alloc.layer_budgets(300, list(range(46, 301))) == list(range(46, 301))  # 255 layers
    assert alloc.layer_budgets(255, 9) == [0, 1, 3, 7, 15, 31, 63, 127, 255]
    for bad in [0, 256, -1, [],  # the number of layers
                10, 255,  # 27005 >> 15 == 27005 >> 16 == 0: the halves stop increasing
                [3000, 3000, 27005], [9000, 3000, 27005], [-1, 27005],  # not strictly increasing, negative
                [3000, 9000], [27005, 27006]]:  # the last entry is not max_bits
        with pytest.raises(ValueError):
            alloc.layer_budgets(27005, 17 if bad == 10 else bad)
    with pytest.raises(ValueError):
        alloc.layer_budgets(300, list(range(45, 301)))  # 256 layers
    with pytest.raises(ValueError):
        alloc.layer_budgets(255, 10)
    with pytest.raises(ValueError):
        alloc.layer_budgets(-8, 1)
    for bad in [2.0, "3", b"3", None, True, [3000.0, 27005], [True, 27005], ["a"]]:
        with pytest.raises(TypeError):
            alloc.layer_budgets(27005, bad)
    with pytest.raises(TypeError):
        alloc.layer_budgets(27005.0, 1)


# ---- the container -------------------------------------------------------------------------------------------------------------

HEAD = 28


def make(rng, H, W, th, tw, cum, c=3, level=2):
    """a LayeredResult of random bytes under a hand-made nested table, and its tiles' streams"""
    from spiht_amd import LayeredResult
    cum = np.asarray(cum, dtype=np.int64)
    Q, T = cum.shape
    tiles = [rng.integers(0, 256, int(cum[-1, t]), dtype=np.uint8) for t in range(T)]
    lo = np.vstack([np.zeros((1, T), np.int64), cum[:-1]])
    body = np.concatenate([tiles[t][lo[q, t]:cum[q, t]] for q in range(Q) for t in range(T)] + [np.zeros(0, np.uint8)])
    max_n = [int(v) for v in rng.integers(0, 31, T)]
    return LayeredResult(H, W, c, th, tw, level, max_n, cum.tolist(), body.tobytes()), tiles


CONTAINERS = {
    # 2 x 3 tiles, 4 layers: tile 2 is empty, layer 2 is empty, tile 4 starts late, tile 0 ends early
    "grid": dict(H=40, W=70, th=32, tw=32, cum=[[3, 0, 0, 5, 0, 1], [9, 4, 0, 5, 0, 2], [9, 4, 0, 5, 0, 2], [9, 11, 0, 40, 7, 3]]),
    "Q=1": dict(H=40, W=70, th=32, tw=32, cum=[[3, 1, 0, 5, 2, 6]]),
    "T=1": dict(H=20, W=30, th=32, tw=32, cum=[[0], [4], [4], [9]]),
    "Q=1,T=1": dict(H=20, W=30, th=32, tw=32, cum=[[6]]),
    "nothing": dict(H=20, W=30, th=32, tw=32, cum=[[0], [0]]),
}


def clipped(cum, a):
    """the rule of from_bytes, piece by piece in file order"""
    cum = np.asarray(cum, dtype=np.int64)
    Q, T = cum.shape
    out, o = np.zeros_like(cum), 0
    for q in range(Q):
        for t in range(T):
            length = int(cum[q, t] - (cum[q - 1, t] if q else 0))
            out[q, t] = (out[q - 1, t] if q else 0) + min(max(a - o, 0), length)
            o += length
    return out.tolist()


@pytest.mark.parametrize("name", list(CONTAINERS))
def test_container_round_trip_and_every_prefix(name):
    from spiht_amd import LayeredResult, TiledResult
    cfg = CONTAINERS[name]
    r, tiles = make(np.random.default_rng(len(name)), **cfg)
    cum = np.asarray(cfg["cum"])
    Q, T = cum.shape
    blob = r.to_bytes()
    head = HEAD + 4 * Q * T + T
    assert r.layers == Q and r.grid() == (-(-cfg["H"] // 32), -(-cfg["W"] // 32))
    assert len(blob) == head + int(cum[-1].sum())
    assert struct.unpack_from("<4sBBHIIIIHH", blob) == (b"SPTQ", 1, 2, 3, cfg["H"], cfg["W"], 32, 32, Q, 0)
    assert np.array_equal(np.frombuffer(blob, "<u4", Q * T, HEAD).reshape(Q, T), cum)
    assert list(blob[HEAD + 4 * Q * T:head]) == r.max_n
    assert r.layer_ends() == [head + int(cum[q].sum()) for q in range(Q)]
    assert LayeredResult.from_bytes(blob) == r
    assert LayeredResult.from_bytes(bytearray(blob)) == r
    for u in list(range(1, Q + 1)) + [None]:
        t = r.tiled(u)
        row = cum[(Q if u is None else u) - 1]
        assert isinstance(t, TiledResult) and t.nbytes == row.tolist() and t.max_n == r.max_n
        assert t.encoded_bytes == b"".join(tiles[k][:row[k]].tobytes() for k in range(T))
        assert (t.h, t.w, t.c, t.th, t.tw, t.level) == (r.h, r.w, r.c, r.th, r.tw, r.level)
        TiledResult.from_bytes(t.to_bytes())
    for bad in (0, Q + 1, -1):
        with pytest.raises(ValueError):
            r.tiled(bad)
    with pytest.raises(TypeError):
        r.tiled(1.0)
    # every prefix from the tables on is a picture: the table clipped by the rule, every tile a prefix of the full tile
    for n in range(head, len(blob) + 1):
        p = LayeredResult.from_bytes(blob[:n])
        assert p.cum == clipped(cum, n - head) and p.layers == Q and p.max_n == r.max_n, n
        assert p.encoded_bytes == blob[head:n]
        assert p.to_bytes() == blob[:HEAD] + np.asarray(p.cum, "<u4").tobytes() + blob[HEAD + 4 * Q * T:n]
        assert LayeredResult.from_bytes(p.to_bytes()) == p
        full, part = r.tiled(), p.tiled()
        assert sum(part.nbytes) == n - head
        for i in range(full.grid()[0]):
            for j in range(full.grid()[1]):
                a, b = full.tile(i, j).encoded_bytes, part.tile(i, j).encoded_bytes
                assert a[:len(b)] == b, (n, i, j)
    for n in range(head):
        with pytest.raises(ValueError):
            LayeredResult.from_bytes(blob[:n])


def test_container_chosen_prefixes_of_a_larger_file():
    """8 x 8 tiles in 5 layers of up to 3000 bytes a piece, cut at a dozen places: the ends of layers, inside pieces, the
    tables alone"""
    from spiht_amd import LayeredResult
    rng = np.random.default_rng(77)
    T, Q = 64, 5
    lens = rng.integers(0, 3000, (Q, T))
    lens[rng.random((Q, T)) < 0.2] = 0
    lens[2] = 0
    cum = np.cumsum(lens, axis=0)
    r, tiles = make(rng, 256, 250, 32, 32, cum, c=1, level=None)
    blob = r.to_bytes()
    head = HEAD + 4 * Q * T + T
    ends = r.layer_ends()
    assert ends[-1] == len(blob) and ends[1] == ends[2]
    cuts = [head, head + 1, ends[0] - 1, ends[0], ends[0] + 1, ends[1], ends[3] - 1, ends[3] + 1, (ends[0] + ends[1]) // 2,
            head + int(lens[0, :5].sum()) + int(lens[0, 5]) // 2, len(blob) - 1, len(blob)]
    full = r.tiled()
    off = np.concatenate(([0], np.cumsum(full.nbytes)))
    for n in cuts:
        p = LayeredResult.from_bytes(blob[:n])
        assert p.level is None and p.cum == clipped(cum, n - head), n
        part = p.tiled()
        poff = np.concatenate(([0], np.cumsum(part.nbytes)))
        for t in range(T):
            assert part.encoded_bytes[poff[t]:poff[t + 1]] == full.encoded_bytes[off[t]:off[t] + part.nbytes[t]], (n, t)
    for q in range(Q):  # cut at a layer's end, the layers through it are whole and the others empty
        p = LayeredResult.from_bytes(blob[:ends[q]])
        assert p.cum == [cum[min(k, q)].tolist() for k in range(Q)]
        assert p.tiled() == r.tiled(q + 1)


def test_container_refusals():
    from spiht_amd import LayeredResult, TiledResult
    r, _ = make(np.random.default_rng(5), **CONTAINERS["grid"])
    blob = r.to_bytes()
    Q, T = 4, 6
    head = HEAD + 4 * Q * T + T
    bad = {
        "magic": b"SPTL" + blob[4:],
        "version": blob[:4] + b"\x02" + blob[5:],
        "no layers": blob[:24] + struct.pack("<HH", 0, 0) + blob[28:],
        "short header": blob[:27],
        "short tables": blob[:head - 1],
        "trailing bytes": blob + b"\x00",
        "falling table": blob[:HEAD + 4 * T] + struct.pack("<I", 2) + blob[HEAD + 4 * T + 4:],  # cum[1][0] = 2 < cum[0][0] = 3
    }
    for what, data in bad.items():
        with pytest.raises(ValueError):
            LayeredResult.from_bytes(data)
    with pytest.raises(ValueError):
        TiledResult.from_bytes(blob)  # the two containers do not read one another
    with pytest.raises(ValueError):
        LayeredResult.from_bytes(r.tiled().to_bytes())
    # to_bytes refuses tables that do not describe the bytes
    for field, value in [("cum", [[3, 0, 0, 5, 0, 1]] * 3 + [[9, 11, 0, 40, 7, 4]]), ("cum", [[9, 11, 0, 40, 7, 3], [3, 0, 0, 5, 0, 1]]),
                         ("max_n", r.max_n[:-1]), ("encoded_bytes", r.encoded_bytes[:-1]), ("level", 255), ("cum", [])]:
        broken = LayeredResult(**{**{k: getattr(r, k) for k in ("h", "w", "c", "th", "tw", "level", "max_n", "cum", "encoded_bytes")},
                                  field: value})
        with pytest.raises(ValueError):
            broken.to_bytes()
    none = LayeredResult(r.h, r.w, r.c, r.th, r.tw, None, r.max_n, r.cum, r.encoded_bytes)
    assert LayeredResult.from_bytes(none.to_bytes()).level is None
