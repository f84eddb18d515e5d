"""tests/maxabs_cases.py held to its purpose on the oracle alone: which (wavelet, class, kind) the constructions reach -- the
table is printed -- with floors under it, the list of what is not reached exact in both directions, and every derived set
(batches, thread sweep, step cases, corner cells, k_absmax arrays) checked for the property the GPU tests rely on.  The first
test records why all this exists: in the forward sweep's own pictures the largest coefficient lies in the root block, every
time, so nothing a level-1 launch adds to the max|coefficient| word decides a comparison there."""
import numpy as np
import pytest

import dwt_sweep_tables as T
import maxabs_cases as M


def test_sweep_pictures_keep_their_maximum_in_the_root_block(oracle):
    """21 wavelets x 4 sizes x 5 modes x 2 pictures x 2 channels of test_gpu_dwt_sweep.test_forward_float64"""
    n = inside = 0
    for wavelet in T.WAVELETS:
        F = T.instantiation(oracle, wavelet)[0]
        for i, (H, W) in enumerate(T.forward_sizes(F)):
            imgs, mults = T.sweep_images(1000 + i, 2, 2, H, W), T.scales_for(i, 2)
            for mode in T.MODES:
                root = M.root_mask(oracle.geometry(H, W, wavelet, 2, mode))
                for im in imgs:
                    qa = oracle.quantize(oracle.wavedec2_array(im, wavelet, mode, 2)[0], T.Q, mults)
                    for ch in qa:
                        hold, _ = M.holders(ch[None])
                        n += 1
                        inside += not (hold[0] & ~root).any()
    print("maximum inside the root block: %d of %d (picture, channel) cases" % (inside, n))
    assert n == 1680 and inside == n


@pytest.fixture(scope="module")
def table(oracle):
    """kind -> {(wavelet, mode, class): reached}; printed once"""
    out = {}
    for kind in M.GRID:
        level, modes, classes = M.GRID[kind]
        got = {(w, m, c): M.place(oracle, w, m, l, H, W, c, kind) is not None for (w, m, l, H, W, c) in M.grid(oracle, kind)}
        out[kind] = got
        for mode in modes:
            print("\n%s, %s, level %d (x reached, . not)\n%-10s %s" % (kind, mode, level, "", " ".join("%-7s" % M.cname(c) for c in classes)))
            for w in T.WAVELETS:
                print("%-10s %s" % (w, " ".join("%-7s" % ("x" if got[(w, mode, c)] else ".") for c in classes)))
    return out


def test_unreached_list_is_exact(table):
    """nothing is left out silently: a case is in UNREACHED exactly when place() gives None, and names nothing outside the grid"""
    for kind, got in table.items():
        miss = {M.key(w, m, c) for (w, m, c), ok in got.items() if not ok}
        assert miss == set(M.UNREACHED[kind]), (kind, sorted(miss ^ set(M.UNREACHED[kind])))


def test_placed_pictures_hold_their_class(oracle):
    """place() again from the stored picture: every cell that holds the maximum is inside the class, and the picture is of its
    kind (integer range, no non-finite pixel, every magnitude far below 2^30)"""
    for kind in M.GRID:
        for (w, m, l, H, W, c) in M.reached(oracle, kind)[::7]:
            p = M.place(oracle, w, m, l, H, W, c, kind)
            qa = M.quantised(oracle, p, kind, w, m, l)
            assert M.in_class(oracle, w, m, l, H, W, c, qa), (kind, w, m, c)
            assert np.abs(qa.astype(np.int64)).max() < 2 ** 20
            assert np.isfinite(M.oracle_input(oracle, p, kind)).all()


def _wavelets_reaching(got, mode, cls):
    return [w for w in T.WAVELETS if got[(w, mode, cls)]]


def test_floors_float(oracle, table):
    for kind in ("f64",) + M.FLT_KINDS:
        got = table[kind]
        for mode in M.FLOAT_MODES:
            for cls in M.INTERIOR1:  # every wavelet reaches the three interior level-1 classes
                assert _wavelets_reaching(got, mode, cls) == T.WAVELETS, (kind, mode, cls)
            for cls in M.LEVEL1:
                assert len(_wavelets_reaching(got, mode, cls)) >= 10, (kind, mode, cls)
            for cls in M.INTERIOR2:
                assert len(_wavelets_reaching(got, mode, cls)) >= 10, (kind, mode, cls)
            # every filter length from 4 to 20: an overhang-row class and an overhang-column class
            for F in T.FILTER_LENGTHS[1:]:
                ws = [w for w in T.WAVELETS if T.instantiation(oracle, w)[0] == F]
                assert any(got[(w, mode, c)] for w in ws for c in M.LEVEL1 if c[2]), (kind, mode, F, "row")
                assert any(got[(w, mode, c)] for w in ws for c in M.LEVEL1 if c[3]), (kind, mode, F, "column")


def test_floors_integer_and_colour(table):
    for kind in M.INT_KINDS + M.COLOUR_KINDS:
        got = table[kind]
        for cls in M.LEVEL1:
            assert len(_wavelets_reaching(got, "reflect", cls)) >= 1, (kind, cls)
        assert len([w for w in T.WAVELETS if any(got[(w, "reflect", c)] for c in M.LEVEL1)]) >= 12, kind


def test_batches_keep_their_classes(oracle):
    """part A / C as built -- scaled, two channels, channel scales on every other batch: each image's maximum is still in its
    class alone, neighbouring images hold different classes, and the three words of a batch differ"""
    for kind in ("f64", "bfloat16", "u8", "ipt-f64"):
        level = M.GRID[kind][0]
        for wavelet in ("bior2.2", "db4", "bior6.8", "db10"):
            H, W = M.size_of(oracle, wavelet)
            for mode in M.GRID[kind][1]:
                for pics, classes, mults in M.batches(oracle, kind, wavelet, mode):
                    ref = M.batch_reference(oracle, kind, wavelet, mode, pics, mults)
                    words = [int(np.abs(r.astype(np.int64)).max()) for r in ref]
                    assert max(words) < 2 ** 30
                    if kind in ("f64", "bfloat16"):
                        assert len(set(words)) == 3, (kind, wavelet, mode, words)
                    for b, cls in enumerate(classes):
                        assert M.in_class(oracle, wavelet, mode, level, H, W, cls, ref[b]), (kind, wavelet, mode, cls, mults)
                    assert len(classes) < 2 or classes[0] != classes[1]


@pytest.mark.parametrize("wavelet,mode", M.THREAD_WAVELETS)
def test_thread_sweep(oracle, wavelet, mode):
    """part B's set: one cell holds the maximum, the target; every (row, column) of a tile -- every lane of every wavefront at
    every one of a thread's rows -- is a target in some tile; all four tiles have targets on their edges; what is
    left out lies within F / 2 - 1 cells of the band's border"""
    F = T.instantiation(oracle, wavelet)[0]
    assert F == {"haar": 2, "bior2.2": 6, "db5": 10, "db9": 18}[wavelet]
    seen = set()
    for tg, pics, refs in M.thread_cases(oracle, wavelet, mode):
        g = oracle.geometry(pics.shape[2], pics.shape[3], wavelet, 1, mode)
        r0, c0, _, _ = M.band_origin(g, 1, "dd")
        for (r, c), qa in zip(tg, refs):
            hold, top = M.holders(qa)
            assert hold.sum() == 1 and hold[0, r0 + r, c0 + c] and 0 < top < 2 ** 20
        seen.update(tg)
    th, tw, edge = T.FWD_TH, T.FWD_TW, F // 2 - 1
    assert {(r % th, c % tw) for (r, c) in seen} == {(r, c) for r in range(th) for c in range(tw)}
    for ty in (0, 1):
        for tx in (0, 1):
            # (at least the tile's row that faces the inside of the picture, less the border's cells)
            assert sum(1 for (r, c) in seen if r // th == ty and c // tw == tx) >= tw - 2 * edge
    missing = [t for t in M.thread_targets() if t not in seen and (t[0] >= th or t[1] >= tw)]
    print("%s: %d targets, %d left out" % (wavelet, len(seen), len(missing)))
    for (r, c) in missing:
        assert min(r, 2 * th - 1 - r) < edge or min(c, 2 * tw - 1 - c) < edge, (r, c)


def test_step_cases(oracle):
    """part D: the class's maximum reaches 2^k and nothing outside it does, in the arithmetic of the kind"""
    n = {"f32t": 0, "f64": 0, "u8": 0}
    for wavelet in M.STEP_WAVELETS:
        for kind in n:
            level = 1 if kind == "u8" else 2
            for cls in M.LEVEL1:
                case = M.step_case(oracle, kind, wavelet, "reflect", level, cls)
                if case is None:
                    continue
                stored, q, inside, outside = case
                assert inside >= 2 ** M.STEP_K > outside
                assert outside == 0 or oracle.start_plane(outside) < oracle.start_plane(inside) == M.STEP_K
                print("%s %s %s: q = %.6g, maximum %d, second %d" % (wavelet, kind, M.cname(cls), q, inside, outside))
                n[kind] += 1
    assert n["f32t"] >= 30 and n["f64"] >= 30 and n["u8"] >= 12, n


def test_corner_cells(oracle):
    """part E: one cell holds the maximum, the first or the last of its band; PACK_UNREACHED is exact; every route has a
    'first' or a 'last' cell in each of its two launches or says which is missing; no plane size is a multiple of 64"""
    for wavelet, mode in M.PACK_ROUTES:
        H, W = M.pack_size(mode)
        g = oracle.geometry(H, W, wavelet, 2, mode)
        for l in (1, 2):
            assert (g["hs"][l] * g["ws"][l]) % 64 != 0 and (2 * g["hs"][l] * g["ws"][l]) % 64 != 0
        for band, which in M.PACK_TARGETS:
            pic = M.corner_picture(oracle, wavelet, mode, band, which)
            assert (pic is None) == ("%s/%s/%s/%s" % (wavelet, mode, band, which) in M.PACK_UNREACHED), (wavelet, mode, band, which)
        for pics, targets in M.pack_batches(oracle, wavelet, mode):
            words = []
            for p, (band, which) in zip(pics, targets):
                qa = M.quantised(oracle, p, "f64", wavelet, mode, 2)
                hold, top = M.holders(qa)
                cell = M.corner_cell(g, band, which)
                assert hold.sum() == 1 and hold[0 if which == "first" else 1, cell[0], cell[1]], (wavelet, mode, band, which)
                words.append(top)
            assert len(set(words)) == 3 and max(words) < 2 ** 30
    reached = {(w, m, b) for (w, m) in M.PACK_ROUTES for (b, wh) in M.PACK_TARGETS if M.corner_picture(oracle, w, m, b, wh) is not None}
    assert {("db20", "reflect", "dd"), ("db20", "reflect", "aa"), ("db4", "smooth", "aa"), ("haar", "smooth", "dd"),
            ("bior4.4", "periodization", "dd"), ("bior4.4", "periodization", "aa")} <= reached


def test_absmax_arrays():
    """part F: both load paths, and the one large cell at every residue mod 4, at both ends, and beside multiples of 256 and 1024"""
    ns = [g[0] * g[1] * g[2] for g in M.ABSMAX_GEOMS]
    assert ns[0] % 4 == 0 and ns[1] % 4 and ns[2] % 4
    for geom, n in zip(M.ABSMAX_GEOMS, ns):
        pos, signs = set(), set()
        for x, ks in M.absmax_arrays(geom):
            flat = np.abs(x.reshape(3, -1).astype(np.int64))
            for b in range(3):
                at = np.nonzero(flat[b] > 3)[0]
                assert len(at) == 1 and flat[b, at[0]] == 2 ** ks[b] + 1 < 2 ** 30
                pos.add(int(at[0]))
            assert len(set(ks)) == 3
            signs.update(np.sign(x[np.abs(x) > 3]).tolist())
        assert signs == {-1, 1}
        assert {0, n - 1, 255, 256, 257, 1023, 1024, 1025} <= pos and {p % 4 for p in pos} == {0, 1, 2, 3}
