"""A target quality across tiles on the GPU: spiht_tile_allocate_target against the rule (alloc.allocate_target) bit for bit
through the C ABI, and TiledCodec(allocate="rd") with target_psnr= end to end -- the cut is the rule's on the measured curves,
every cut tile is still the oracle's encode of the tile's pixels at its own length, and the decoded picture's error is at or
below the target whenever the call says it was met."""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import synth_image
from target_cases import PINNED, all_slopes, dist_at, hulls_of, random_table, same_float
from tile_helpers import dev, tile_pixels

pytestmark = pytest.mark.gpu

vp = C.c_void_p
NAN_GUARD = 0x7FF8000000000123  # a NaN that is not the kernel's: an output not written shows


def run_target(nbytes, K, D, budget, kind, targets, optional=True):
    """nbytes [N][T], D [N][T][K + 1], targets [N] -> (bytes [N][T], lambda [N], dist [N], met [N]) of
    spiht_tile_allocate_target, between guard words; optional=False: the three optional outputs are NULL"""
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    nbytes = np.asarray(nbytes, np.uint64)
    N, T = nbytes.shape
    nbits = np.where(nbytes > 0, 8 * nbytes - 5, 0).astype(np.uint64)  # a last byte that is not full
    table = np.ascontiguousarray(np.asarray(D, np.uint64 if kind else np.float64).reshape(N * T, K + 1).T)
    d_out, d_lam = dev(np.full(N * T + 2, 99, np.uint64)), dev(np.full(N + 2, -1.0))
    d_dist, d_met = dev(np.full(N + 2, NAN_GUARD, np.uint64)), dev(np.full(N + 2, 77, np.uint32))
    d_nbits, d_table, d_target = dev(nbits.reshape(-1)), dev(table), dev(np.asarray(targets, np.float64))
    opt = (vp(d_lam.ptr + 8), vp(d_dist.ptr + 8), vp(d_met.ptr + 4)) if optional else (None, None, None)
    _lib.check(L.spiht_tile_allocate_target(ctx.handle, vp(d_nbits.ptr), vp(d_table.ptr), kind, K, N, T, int(budget),
                                            vp(d_target.ptr), vp(d_out.ptr + 8), *opt))
    ctx.synchronize()
    out, lam, dist, met = d_out.download(), d_lam.download(), d_dist.download(), d_met.download()
    assert out[0] == 99 and out[-1] == 99 and lam[0] == -1.0 and lam[-1] == -1.0
    assert dist[0] == NAN_GUARD and dist[-1] == NAN_GUARD and met[0] == 77 and met[-1] == 77
    assert not (out[1:-1] % 8).any()
    if not optional:
        assert (lam == -1.0).all() and (dist == NAN_GUARD).all() and (met == 77).all()
    return (out[1:-1] // 8).reshape(N, T).tolist(), lam[1:-1].tolist(), dist[1:-1].view(np.float64).tolist(), met[1:-1].tolist()


def same_bits(a, b):
    """two floats equal in every bit; any NaN equals the rule's NaN"""
    if math.isnan(b):
        return math.isnan(a)
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", list(PINNED))
def test_kernel_pinned(name, kind):
    case = PINNED[name]
    out, lam, dist, met = run_target([case["nbytes"]], case["K"], [case["D"]], case["budget"], kind, [case["target"]])
    assert out == [case["want"]] and lam == [case["lam"]] and same_float(dist[0], case["dist"]) and met == [int(case["met"])]


@pytest.mark.parametrize("N,T,K,kind", [(1, 1, 4, 0), (1, 256, 7, 1), (1, 257, 7, 0), (2, 300, 16, 0), (2, 37, 255, 1), (1, 1500, 4, 0)])
def test_kernel_is_the_rule_bit_for_bit(N, T, K, kind):
    """lengths, lam, the bits of dist and met against alloc.allocate_target: the seam of thread ownership at 256 / 257 tiles, more
    than one round per thread, two pictures with their own targets in a call, K at its limit, uint64 sums above 2^53.  Targets
    from the rule's own vertex sums -- the value, its predecessor double -- and inf, 0, NaN; budgets that bind and that do not."""
    from spiht_amd import alloc
    rng = np.random.default_rng(1000 * T + K)
    tables = [random_table(rng, T, K, 3000, kind == 1) for _ in range(N)]
    nbytes, D = np.stack([t[0] for t in tables]), np.stack([t[1] for t in tables])
    R = [[alloc.tile_lengths(int(v), K) for v in nbytes[n]] for n in range(N)]
    per_picture, ends = [], []
    for n in range(N):
        hulls = hulls_of(R[n], D[n])
        slopes = all_slopes(hulls)
        sums = [dist_at(hulls, slopes[i]) for i in sorted({len(slopes) // 3, 2 * len(slopes) // 3, len(slopes) - 1})]
        per_picture.append([v for s in sums for v in (s, math.nextafter(s, 0.0))] + [math.inf, 0.0, math.nan])
        ends.append(sum(r[alloc.lower_hull(r, d)[-1]] for r, d in zip(R[n], D[n])))
    rounds = max(len(p) for p in per_picture)
    branches = set()
    for budget in (min(ends) // 3, max(ends) + 1):
        for j in range(rounds):
            targets = [per_picture[n][(j + 2 * n) % len(per_picture[n])] for n in range(N)]  # (the pictures' targets differ)
            out, lam, dist, met = run_target(nbytes, K, D, budget, kind, targets)
            for n in range(N):
                want, wlam, wdist, wmet = alloc.allocate_target(R[n], D[n], targets[n], budget)
                assert out[n] == want, (budget, j, n)
                assert same_bits(lam[n], wlam) and same_bits(dist[n], wdist) and met[n] == int(wmet), \
                    (budget, j, n, lam[n], wlam, dist[n], wdist)
                branches.add("met" if wmet else "budget" if math.isnan(wdist) else "unreachable")
    assert branches == {"met", "budget", "unreachable"}
    # the optional outputs may be NULL: the same lengths
    targets = [per_picture[n][0] for n in range(N)]
    assert run_target(nbytes, K, D, max(ends) + 1, kind, targets, optional=False)[0] == \
        [alloc.allocate_target(R[n], D[n], targets[n], max(ends) + 1)[0] for n in range(N)]


def test_kernel_argument_errors():
    from spiht_amd import _lib
    L, ctx = _lib.lib(), _lib.default_context()
    d = dev(np.zeros(64, np.uint64))
    p = vp(d.ptr)
    for kind, K, N, T in [(2, 4, 1, 4), (0, 0, 1, 4), (0, 256, 1, 4), (0, 4, -1, 4), (0, 4, 1, 0)]:
        assert L.spiht_tile_allocate_target(ctx.handle, p, p, kind, K, N, T, 10, p, p, None, None, None) == _lib.ERR_ARG
    assert L.spiht_tile_allocate_target(ctx.handle, p, p, 0, 4, 1, 4, 10, None, p, p, p, p) == _lib.ERR_ARG  # no targets
    assert L.spiht_tile_allocate_target(ctx.handle, p, p, 0, 4, 1, 4, 10, vp(d.ptr + 4), p, p, p, p) == _lib.ERR_ARG
    assert L.spiht_tile_allocate_target(ctx.handle, p, p, 0, 4, 1, 4, 10, p, p, p, vp(d.ptr + 4), p) == _lib.ERR_ARG
    assert L.spiht_tile_allocate_target(ctx.handle, p, p, 0, 4, 1, 4, 10, p, p, p, p, vp(d.ptr + 2)) == _lib.ERR_ARG
    assert L.spiht_tile_allocate_target(ctx.handle, p, p, 0, 4, 2 ** 31, 4, 10, p, p, p, p, p) == _lib.ERR_TOO_LARGE
    assert L.spiht_tile_allocate_target(ctx.handle, p, p, 0, 4, 0, 4, 10, p, p, p, p, p) == _lib.OK  # no pictures: nothing queued
    ctx.synchronize()
    assert not d.download().any()


# ---- end to end -----------------------------------------------------------------------------------------------------------------

MAX_BITS, TILE, POINTS = 27005, 32, 8
PEAK = {None: 1.0, np.uint8: 255.0, np.uint16: 65535.0}


def picture(which, dtype):
    """the allocation tests' pictures: synth_image(4161, 3, 70, 90), and synth_image(4161, 1, 70, 90) with a constant left half"""
    if which == "plain":
        P = synth_image(4161, 3, 70, 90)
    else:
        P = synth_image(4161, 1, 70, 90)
        P[:, :, :45] = P[0, 0, 0]
    if dtype is not None:
        P = np.round(P * PEAK[dtype]).astype(dtype)
    P.setflags(write=False)
    return P


def db_of(sqerr, peak, c, weight_sum):
    return 10.0 * math.log10(c * weight_sum * peak * peak / sqerr)


def choose_targets(curves, budget, peak, c, weight_sum):
    """by the rule on the CPU: PSNRs of which one is met on hull vertices with some bytes, one is capped by the budget and one is
    beyond every hull vertex -> {"vertices": dB, "budget": dB, "unreachable": dB}"""
    from spiht_amd import alloc
    hulls = hulls_of(curves.lengths, curves.sse)
    found = {}
    for s in all_slopes(hulls):
        v = dist_at(hulls, s)
        if not v > 0:
            break
        db = db_of(v, peak, c, weight_sum) - 0.01  # (a target a little above the vertex sum: the rounding of dB and back)
        out, lam, dist, met = alloc.allocate_target(curves.lengths, curves.sse, alloc.target_sqerr(db, peak, c, weight_sum), budget)
        if met and sum(out):
            found["vertices"] = db  # (the last one that fits: the most bytes)
        elif math.isnan(dist):
            found.setdefault("budget", db)
    found["unreachable"] = db_of(dist_at(hulls, all_slopes(hulls)[-1]), peak, c, weight_sum) + 3.0
    assert set(found) == {"vertices", "budget", "unreachable"}, found
    return found


@functools.lru_cache(maxsize=None)
def case(which, dtype, with_roi=False):
    """the picture, codec, curves and chosen targets of a case: computed once, shared, never changed"""
    import spiht_amd
    from spiht_amd import alloc
    P = picture(which, dtype)
    s = spiht_amd.SpihtSettings()
    codec = spiht_amd.TiledCodec(P.shape[0], 70, 90, TILE, s, None, MAX_BITS, allocate="rd", points=POINTS)
    roi = alloc.roi_map(70, 90, [(20, 30, 30, 40)]) if with_roi else None
    curves = codec.tile_curves(P, dtype, roi=roi)
    ws = 70 * 90 if roi is None else int(roi.sum(dtype=np.int64))
    dbs = choose_targets(curves, MAX_BITS // 8, PEAK[dtype], P.shape[0], ws)
    return P, s, codec, curves, roi, ws, dbs


def encode(codec, P, dtype, **kw):
    return codec.encode(P, **kw) if dtype is None else codec.encode_u8(P, **kw) if dtype == np.uint8 else codec.encode_u16(P, **kw)


def decode(codec, res, dtype):
    return codec.decode(res) if dtype is None else codec.decode_u8(res) if dtype == np.uint8 else codec.decode_u16(res)


def weighted_error(P, dec, roi, dtype):
    """(the exact squared error of the decoded picture, weighted by the map, as a Fraction; numpy's float64 sum of it)"""
    w = np.ones(P.shape[1:], np.int64) if roi is None else roi.astype(np.int64)
    if dtype is not None:
        e = P.astype(np.int64) - dec.astype(np.int64)
        S = int((e * e * w[None]).sum())
        return Fraction(S), float(S)
    S = Fraction(0)
    for p, d, wt in zip(P.reshape(-1).tolist(), dec.reshape(-1).tolist(), np.broadcast_to(w, P.shape).reshape(-1).tolist()):
        e = Fraction(p) - Fraction(d)
        S += wt * e * e
    return S, float((w[None] * ((P - dec) * (P - dec))).sum())


def check_result(oracle, which, dtype, with_roi, branch):
    import spiht_amd
    from spiht_amd import alloc, rd
    P, s, codec, curves, roi, ws, dbs = case(which, dtype, with_roi)
    c, peak, budget, db = P.shape[0], PEAK[dtype], MAX_BITS // 8, dbs[branch]
    res = encode(codec, P, dtype, roi=roi, target_psnr=db)
    cut = codec.last_allocation
    # the cut is the rule's, on the table the device measured
    target = alloc.target_sqerr(db, peak, c, ws)
    want, lam, dist, met = alloc.allocate_target(curves.lengths, curves.sse, target, budget)
    assert {"vertices": met, "budget": math.isnan(dist), "unreachable": not met}[branch]
    assert res.nbytes == want and cut.nbytes == want and cut.lam == lam and cut.met is met
    assert sum(res.nbytes) <= budget and sum(res.nbytes) == len(res.encoded_bytes) and res.max_n == curves.max_n
    if math.isnan(dist):
        assert cut.dist is None and cut.psnr is None
        plain = encode(codec, P, dtype, roi=roi)  # the cut of the call without a target
        assert res == plain and codec.last_allocation.nbytes == want and codec.last_allocation.met is None
    else:
        assert cut.dist == dist and cut.psnr == rd.psnr_of(dist / (c * ws), peak)
        assert (cut.dist <= target) is met and (not met or cut.psnr >= db - 1e-9)
    # every tile is the oracle's encode of its pixels at its own length
    for i in range(codec.gy):
        for j in range(codec.gx):
            t = res.tile(i, j)
            if len(t.encoded_bytes):
                px = tile_pixels(P, TILE, TILE, i, j)
                px = px if dtype is None else px / peak
                ob, on, _ = oracle.encode_image(px, s.wavelet, s.mode, None, s.quantization_scale, None, 8 * len(t.encoded_bytes))
                assert t.encoded_bytes == ob and t.max_n == on, (i, j)
    # the decoded picture's own error: what the call reports, and at or below the target when met
    if not math.isnan(dist):
        S, S_numpy = weighted_error(P, decode(codec, res, dtype), roi, dtype)
        print("%s %s %s: target %.2f dB, %d bytes, dist %r, numpy %r" % (which, dtype, branch, db, sum(want), dist, S_numpy))
        if dtype is not None:
            assert Fraction(dist) == S and (S <= Fraction(target)) is met  # exact: every sum is an integer below 2^53
        else:
            n = P.size
            bound = (n + 3) * Fraction(1, 2 ** 52) * S
            assert abs(Fraction(dist) - S) <= bound and abs(Fraction(S_numpy) - S) <= bound
            assert not met or S <= Fraction(target) + bound
    return res, cut


@pytest.mark.parametrize("branch", ["vertices", "budget", "unreachable"])
@pytest.mark.parametrize("dtype", [None, np.uint8, np.uint16])
@pytest.mark.parametrize("which", ["plain", "left half constant"])
def test_end_to_end(oracle, which, dtype, branch):
    check_result(oracle, which, dtype, False, branch)


@pytest.mark.parametrize("dtype", [None, np.uint8])
def test_with_roi(oracle, dtype):
    """a weighted target: the rule on the weighted table, the target from the weights' sum; a map of ones is no map"""
    P, s, codec, curves, roi, ws, dbs = case("plain", dtype, True)
    res, cut = check_result(oracle, "plain", dtype, True, "vertices")
    check_result(oracle, "plain", dtype, True, "budget")
    _, _, _, _, _, _, plain_dbs = case("plain", dtype, False)
    db = plain_dbs["vertices"]
    a = encode(codec, P, dtype, target_psnr=db)
    cut_a = codec.last_allocation
    b = encode(codec, P, dtype, roi=np.ones((70, 90), np.uint8), target_psnr=db)
    assert a == b and codec.last_allocation == cut_a and cut_a.met
    assert encode(codec, P, dtype, roi=roi, target_psnr=db).nbytes != a.nbytes
    with pytest.raises(ValueError):
        encode(codec, P, dtype, roi=np.zeros((70, 90), np.uint8), target_psnr=db)


def test_unreachable_within_the_budget(oracle):
    """spread = 1: every tile is coded with its share alone, so all hulls together fit the budget, and a target beyond them
    gives every tile's whole hull, the error reached and met = False"""
    import spiht_amd
    from spiht_amd import alloc
    P = picture("plain", None)
    s = spiht_amd.SpihtSettings()
    codec = spiht_amd.TiledCodec(3, 70, 90, TILE, s, None, MAX_BITS, allocate="rd", points=POINTS, spread=1.0)
    curves = codec.tile_curves(P)
    res = codec.encode(P, target_psnr=80.0)
    cut = codec.last_allocation
    want, lam, dist, met = alloc.allocate_target(curves.lengths, curves.sse, alloc.target_sqerr(80.0, 1.0, 3, 6300), MAX_BITS // 8)
    assert not met and not math.isnan(dist) and want == [r[alloc.lower_hull(r, d)[-1]] for r, d in zip(curves.lengths, curves.sse)]
    assert res.nbytes == want and (cut.lam, cut.dist, cut.met) == (lam, dist, False) and cut.psnr < 80.0
    S, _ = weighted_error(P, codec.decode(res), None, None)
    assert abs(Fraction(dist) - S) <= (P.size + 3) * Fraction(1, 2 ** 52) * S


def test_two_pictures_with_their_own_targets():
    P, s, codec, curves, roi, ws, dbs = case("plain", None)
    Q = synth_image(91, 3, 70, 90)
    many = codec.encode(np.stack([P, Q]), target_psnr=[dbs["vertices"], dbs["vertices"] - 4.0])
    cuts = codec.last_allocation
    assert many[0] == codec.encode(P, target_psnr=dbs["vertices"]) and cuts[0] == codec.last_allocation
    assert many[1] == codec.encode(Q, target_psnr=dbs["vertices"] - 4.0) and cuts[1] == codec.last_allocation
    assert cuts[0].met and many[1].nbytes != many[0].nbytes
    both = codec.encode(np.stack([P, Q]), target_psnr=dbs["vertices"])  # one number is every picture's
    assert both[0] == many[0] and both[1] == codec.encode(Q, target_psnr=dbs["vertices"])
    with pytest.raises(ValueError):
        codec.encode(np.stack([P, Q]), target_psnr=[30.0])


def test_device_form_and_the_module_function():
    """encode_device with d_target is what the host form queues; the convenience is the same call"""
    import spiht_amd
    from spiht_amd import _lib, alloc
    P, s, codec, curves, roi, ws, dbs = case("plain", None)
    res = codec.encode(P, target_psnr=dbs["vertices"])
    NT, ctx = codec.T, _lib.default_context()
    d_img, d_target = dev(P[None]), dev(np.array([alloc.target_sqerr(dbs["vertices"], 1.0, 3, 70 * 90)]))
    d_packed = dev(np.zeros(NT * codec.codec.slot_stride, np.uint8))
    d_lens, d_maxn = dev(np.zeros(NT, np.uint32)), dev(np.zeros(NT, np.uint8))
    codec.encode_device(d_img, 1, d_packed, d_lens, d_maxn, d_target=d_target)
    ctx.synchronize()
    lens = d_lens.download()
    assert lens.tolist() == res.nbytes and d_packed.download()[:int(lens.sum())].tobytes() == res.encoded_bytes
    assert spiht_amd.encode_image_tiled(P, TILE, s, None, MAX_BITS, allocate="rd", points=POINTS, target_psnr=dbs["vertices"]) == res
    plain = spiht_amd.TiledCodec(3, 70, 90, TILE, s, None, MAX_BITS)
    with pytest.raises(ValueError):
        plain.encode(P, target_psnr=30.0)
    with pytest.raises(ValueError):
        plain.encode_device(d_img, 1, d_packed, d_lens, d_maxn, d_target=d_target)


@pytest.mark.parametrize("dtype", [None, np.uint8])
def test_layers_by_psnr(dtype):
    """target_psnr=[a, b, c]: cum nests, the picture through layer q is the one-rate encode at target q, the last target is
    beyond the cap and repeats the cut at the cap, and every layer decodes through the unchanged decode_layered"""
    import spiht_amd
    P, s, codec, curves, roi, ws, dbs = case("plain", dtype)
    targets = [dbs["vertices"] - 6.0, dbs["vertices"], dbs["budget"]]
    layered = codec.encode_layered if dtype is None else codec.encode_layered_u8
    res = layered(P, target_psnr=targets)
    cuts = codec.last_allocation
    assert res.layers == 3 and layered(P, 3, target_psnr=targets) == res
    assert all(a <= b for q in range(2) for a, b in zip(res.cum[q], res.cum[q + 1]))
    assert [c.met for c in cuts] == [True, True, False] and cuts[2].dist is None
    assert cuts[0].lam >= cuts[1].lam >= cuts[2].lam and sum(res.cum[0]) < sum(res.cum[1]) < sum(res.cum[2]) <= MAX_BITS // 8
    for q, db in enumerate(targets):
        one = encode(codec, P, dtype, target_psnr=db)
        assert res.tiled(upto=q + 1) == one and cuts[q] == codec.last_allocation, q
        got = codec.decode_layered(res, q + 1) if dtype is None else codec.decode_layered_u8(res, q + 1)
        assert np.array_equal(got, decode(codec, one, dtype)), q
    assert res.tiled() == encode(codec, P, dtype)  # the cap's cut: the picture of the call without a target
    back = spiht_amd.LayeredResult.from_bytes(res.to_bytes())
    assert back == res
    if dtype is None:
        assert spiht_amd.encode_image_layered(P, TILE, s, None, MAX_BITS, points=POINTS, target_psnr=targets) == res
    else:
        assert spiht_amd.encode_image_layered_u8(P, TILE, s, None, MAX_BITS, points=POINTS, target_psnr=targets) == res
    with pytest.raises(ValueError):
        layered(P, 2, target_psnr=targets)


def test_command_line(tmp_path, capsys):
    import spiht_amd
    from spiht_amd.encode_decode import build_parser, main
    from spiht_amd.utils import imload, imsave
    src = str(tmp_path / "in.png")
    imsave(src, synth_image(6, 3, 70, 90))
    P = imload(src)
    common = [src, "--bpp", "2.0", "--tile", "32", "--color_model", "RGB", "--per_channel_quant_scales", "1.,1.,1.",
              "--out", str(tmp_path / "out.png"), "--allocate", "rd", "--points", "8"]
    s = spiht_amd.SpihtSettings(quantization_scale=255.0, per_channel_quant_scales=[1.0, 1.0, 1.0])
    bits = round(2.0 * 70 * 90)
    enc, dec = main(build_parser().parse_args(common + ["--psnr", "30"]))
    assert enc == spiht_amd.encode_image_tiled(P, 32, s, 2, bits, allocate="rd", points=8, target_psnr=30.0)
    assert np.array_equal(dec, spiht_amd.decode_image_tiled(enc, s)) and sum(enc.nbytes) <= bits // 8
    out = capsys.readouterr().out
    line = [x for x in out.splitlines() if x.startswith("cut to 30.00 dB")]
    assert len(line) == 1 and "%d bytes" % len(enc.encoded_bytes) in line[0] and ("target met" in line[0] or "not reached" in line[0])
    if "target met" in line[0]:
        assert 10 * math.log10(1.0 / float(((P - dec) ** 2).mean())) >= 30.0 - 1e-6
    # with a region of interest: the weighted target
    roi = spiht_amd.roi_map(70, 90, [[20, 30, 30, 40, 255]])
    enc_w, _ = main(build_parser().parse_args(common + ["--psnr", "30", "--roi", "20,30,30,40"]))
    assert enc_w == spiht_amd.encode_image_tiled(P, 32, s, 2, bits, allocate="rd", points=8, roi=roi, target_psnr=30.0)
    # layers by PSNR
    capsys.readouterr()
    lay, dec = main(build_parser().parse_args(common + ["--layer-psnr", "24,30,90"]))
    assert lay == spiht_amd.encode_image_layered(P, 32, s, 2, bits, points=8, target_psnr=[24.0, 30.0, 90.0])
    assert lay.layers == 3 and lay.tiled(2) == enc and np.array_equal(dec, spiht_amd.decode_image_layered(lay, s))
    out = capsys.readouterr().out
    assert sum(1 for x in out.splitlines() if x.strip().startswith("layer") and " dB: " in x) == 3
    for bad in (["--psnr", "30", "--layer-psnr", "24,30"], ["--layer-psnr", "30,24"], ["--layer-psnr", "x"]):
        with pytest.raises(SystemExit):
            main(build_parser().parse_args(common + bad))
    with pytest.raises(SystemExit):  # a target needs the curves
        main(build_parser().parse_args(common[:-4] + ["--psnr", "30"]))
    with pytest.raises(SystemExit):
        main(build_parser().parse_args([src, "--layer-psnr", "24,30"]))
