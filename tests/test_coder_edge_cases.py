"""The cases of tests/test_gpu_coder_edges.py held to their purpose, without a GPU: conditions on the generator
(tests/coder_edge_cases.py) that hold with the oracle alone, none of them a measurement of the code under test."""
import ctypes as C

import numpy as np

import coder_edge_cases as E


def test_bands_of_the_start_plane_rule(oracle):
    """`(max as f32).log2() as u8`: below 2^21 no maximum starts above its top bit; from k = 21 to 30 some do, the band
    below 2^k.  The generator's "first in the band" is the step itself."""
    for k in range(1, 21):
        assert E.band(oracle, k) == [], k
    firsts = E.band_firsts(oracle)
    assert sorted(firsts) == list(range(21, 31))
    for k in range(21, 31):
        b = E.band(oracle, k)
        assert len(b) >= 1 and b[-1] == (1 << k) - 1 and b == list(range(b[0], 1 << k)), k
        assert oracle.start_plane(b[0]) == k and oracle.start_plane(b[0] - 1) == k - 1, k
        assert all(E.in_band(oracle, m) for m in (b[0], b[-1])) and not E.in_band(oracle, b[0] - 1)
        assert not E.in_band(oracle, 1 << k) or k == 30
    vals = E.plane_maxima(oracle)
    assert vals == sorted(set(vals)) and vals[0] == 1 and vals[-1] == (1 << 30) - 1
    for k in range(1, 31):
        want = {(1 << k) - 1} | ({1 << k, (1 << k) + 1} if k < 30 else set())
        if k >= 21:
            want |= {firsts[k] - 1, firsts[k]}
        assert want <= set(vals), k
    assert all(0 < m < (1 << 30) for m in vals)
    # both sides of every step are there: a value of plane k - 1 right below a value of plane k
    planes = {m: oracle.start_plane(m) for m in vals}
    for k in range(1, 31):
        assert any(planes[m] == k and planes.get(m - 1) == k - 1 for m in vals), k


def test_placements_reach_what_they_name(oracle):
    for geom in E.SMALL_GEOMS + [E.MID_GEOM]:
        c, h, w, lh, lw = geom
        cover = E.parents_of_cells(oracle, h, w, lh, lw)
        pl = dict(E.placements(oracle, geom))
        k, i, j = pl["root"]
        assert i < lh and j < lw and cover[i, j] == 0
        k, i, j = pl["leaf"]
        assert E.is_leaf(h, w)[i, j] and cover[i, j] >= 1 and (i >= lh or j >= lw)
        assert pl["last"] == (c - 1, h - 1, w - 1)
        if geom == E.ODD_GEOM:
            k, i, j = pl["dup"]
            assert cover[i, j] >= 2
    cases = list(E.placed_cases(oracle, E.ODD_GEOM, [5, (1 << 24) - 1]))
    assert len(cases) == 2 * 4 * 2 * 2
    for (m, name, sign, fill), x in cases:
        assert x.dtype == np.int32 and int(np.abs(x.astype(np.int64)).max()) == m
        assert int(x[dict(E.placements(oracle, E.ODD_GEOM))[name]]) == sign * m
        assert bool(np.count_nonzero(x) > 1) == (fill and m > 4)
    assert {s for (_, _, s, _), _ in cases} == {1, -1}


def test_capacity_budgets_bind(oracle):
    """list_caps() takes min(node instances, roots + mb + 16384): the budgets meant to bind are below the point where the
    two meet, the others are not.  The node count is not c*h*w on these geometries (ll 5x5 and 6x9: an odd side leaves some
    cells outside every tree and reaches others twice -- 21849 instances of 25600 cells, 39942 of 39456), so a budget binds
    only when roots + mb + 16384 is below BOTH; the budgets on either side of c*h*w - roots - 16384 are in the list as well."""
    for geom, more_nodes_than_cells in zip(E.CAP_GEOMS, (False, True)):
        c, h, w, lh, lw = geom
        cells, roots = c * h * w, c * lh * lw
        nodes = c * E.node_instances(oracle, h, w, lh, lw)
        assert (nodes > cells) == more_nodes_than_cells and nodes != cells
        bind, free = E.cap_budgets(oracle, geom)
        assert {1, 64, 4000} <= set(bind) and E.UNLIMITED in free
        assert max(bind) + 1 == min(free)  # either side of the point where the two terms meet
        assert {E.cap_pivot(geom) - 1, E.cap_pivot(geom)} <= set(bind + free)
        for mb in bind:
            assert nodes > roots + mb + E.CHUNK_SLACK, (geom, mb)
        for mb in (1, 64, 4000):
            assert cells > roots + mb + E.CHUNK_SLACK, (geom, mb)
        for mb in free:
            assert nodes <= roots + mb + E.CHUNK_SLACK, (geom, mb)
        assert cells > roots + (E.cap_pivot(geom) - 1) + E.CHUNK_SLACK and cells <= roots + E.cap_pivot(geom) + E.CHUNK_SLACK
        assert cells <= roots + E.UNLIMITED + E.CHUNK_SLACK
        # the LSP's cap mb/2 + 1 + 16384 against the node count, either side
        lo, hi = [mb for mb in bind + free if 0 <= nodes - (mb // 2 + 1 + E.CHUNK_SLACK) <= 1], \
            [mb for mb in bind + free if mb != E.UNLIMITED and mb // 2 + 1 + E.CHUNK_SLACK > nodes]
        assert lo and hi, (geom, lo, hi)
        first = E.band(oracle, E.CAP_MAGNITUDE_PLANES)[0]
        for M in (1, 1 << 12, first):
            arrs = E.extremal_arrays(geom, M)
            assert sorted(arrs) == ["corner", "finest", "full"]
            assert (np.abs(arrs["full"]) == M).all() and (arrs["full"] > 0).any() and (arrs["full"] < 0).any()
            leaf = E.is_leaf(h, w)
            assert (np.abs(arrs["finest"][:, leaf]) == M).all() and not arrs["finest"][:, ~leaf].any()
            assert np.count_nonzero(arrs["corner"]) == 1 and abs(int(arrs["corner"][c - 1, h - 1, w - 1])) == M


def test_worst_case_stream_within_the_bound(oracle):
    """every cell +-(2^k - 1), k = 30 included: the oracle's unlimited stream is no longer than spiht_encode_bound says
    (a host function of the library: no device needed)"""
    from spiht_amd import _lib
    L = _lib.lib()
    for geom in E.SMALL_GEOMS + [E.MID_GEOM]:
        c, h, w, lh, lw = geom
        for k in (1, 2, 12, 21, 24, 29, 30):
            M = (1 << k) - 1
            x = E.extremal_arrays(geom, M, seed=k)["full"]
            d, n, nbits = oracle.encode_nbits(x, lh, lw, E.UNLIMITED)
            bound = C.c_uint64()
            assert L.spiht_encode_bound(c, h, w, lh, lw, M, 0, C.byref(bound)) == _lib.OK
            assert len(d) <= bound.value, (geom, k, len(d), bound.value)
            # ... and it is the whole array: without loss wherever the reference codes a cell at all
            r, m = oracle.decode(d, n, c, h, w, lh, lw), E.coded_cells(oracle, geom)
            assert np.array_equal(r[m], x[m]) and not r[~m].any(), (geom, k)
    assert E.coded_cells(oracle, E.SMALL_GEOMS[0]).all() and not E.coded_cells(oracle, E.ODD_GEOM).all()


def test_extremal_streams():
    pats = E.periodic_patterns()
    assert len(pats) == 2 + 2 + 6 + 12 + 30 + 54 + 126 + 240  # sequences of least period 1 .. 8
    for ln in (1, 8, 64, 512):
        s = E.extremal_streams(ln)
        assert len(set(s)) == len(s) and all(len(d) == ln for d in s)
        assert b"\xff" * ln in s and b"\x00" * ln in s
    assert len(E.extremal_streams(1)) == 256 and len(E.extremal_streams(840)) == len(pats)
    for p, v in pats[::17]:
        bits = np.unpackbits(np.frombuffer(E.periodic_stream(p, v, 53), np.uint8), bitorder="little")
        assert all(int(bits[t]) == (v >> (t % p)) & 1 for t in range(len(bits)))


def _mixed_batch_conditions(oracle, B, shape, slot, nslots, seed):
    c, h, w, lh, lw = shape
    data, nbytes, ns, kinds = E.mixed_batch(oracle, B, shape, slot, nslots, seed)
    assert data.shape == (B, slot) and data.dtype == np.uint8 and len(nbytes) == len(ns) == len(kinds) == B
    streams = [data[b, :int(nbytes[b])].tobytes() for b in range(B)]
    for b in range(B):
        assert 0 <= int(nbytes[b]) <= slot and 0 <= int(ns[b]) <= 30
        assert int(nbytes[b]) == slot or data[b, int(nbytes[b]):].all(), "slot tail of image %d holds a zero" % b
        if b:
            assert (streams[b], int(ns[b])) != (streams[b - 1], int(ns[b - 1])), b
    lens = {int(v) for v in nbytes}
    assert {0, 1, slot} <= lens and any(v % 4 for v in lens if v > 4)
    assert {0, 29, 30} <= {int(v) for v in ns}
    assert {k for _, k in kinds} == {"enc", "prefix", "random", "dense", "ones", "periodic"}
    for b in range(max(0, B - nslots)):
        roles = (kinds[b][0], kinds[b + nslots][0])
        assert roles in (("heavy", "light"), ("light", "heavy")), b
        lo, hi = sorted((int(nbytes[b]), int(nbytes[b + nslots])))
        assert lo <= 1 and hi >= slot // 2
    for b in range(B):  # every stream is one the oracle decodes
        r = oracle.decode(streams[b], int(ns[b]), c, h, w, lh, lw)
        assert r.shape == (c, h, w)
    return data, nbytes, ns, kinds


def test_mixed_batches(oracle):
    for num_cu in (256, 304, 8):
        nslots = 8 * num_cu
        _mixed_batch_conditions(oracle, nslots + 300, E.ODD_GEOM, 96, nslots, 4)
    data, nbytes, ns, kinds = _mixed_batch_conditions(oracle, 64, E.WINDOW_GEOM, 6000, 64, 5)
    assert int(nbytes.max()) == 6000
    assert len({(data[b, :int(nbytes[b])].tobytes(), int(ns[b])) for b in range(64)}) == 64  # every image differs


def test_encoder_batch_images_differ(oracle):
    xs = E.encoder_batch(oracle, 306, E.MID_GEOM, 9)
    assert xs.dtype == np.int32 and xs.shape == (306,) + E.MID_GEOM[:3]
    mx = np.abs(xs.astype(np.int64)).reshape(306, -1).max(axis=1)
    assert (mx < (1 << 30)).all() and not xs[0].any() and not xs[305].any()
    assert any(E.in_band(oracle, int(m)) for m in mx) and (mx >= (1 << 20)).any()
    for b in range(1, 306):
        assert not np.array_equal(xs[b], xs[b - 1]), b
    assert all(not xs[b, :, 13:, :].any() for b in range(4, 306, 5))
