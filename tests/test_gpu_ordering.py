"""The ordering primitives of the C ABI (spiht_event_create / _record, spiht_ctx_wait_event, spiht_ctx_wait_on,
spiht_ctx_wait_resident), tested directly, in the schedule in which a fill queued in front of the encoder was once seen to
land on words the kernel had already written: two producer contexts P0 and P1, a consumer context L that waits for an
event of each and then, with nothing in between, makes the call under test -- a call that starts with a fill its own
kernels depend on.  No host wait stands between the producers' calls and the consumer's.  Each producer's queue starts
behind the library's own bounded gate (spiht_ctx_wait_resident on a word of the test's that stays 0: it ends by itself
after 3 ms), so the consumer's wait is a real one without a timer in the test.  P0 transforms a batch into caller-owned
coefficient / pyramid / maximum arrays, P1 decodes another into a caller-owned array; the consumer reads, or overwrites,
what they made, so a wait that did not hold shows as wrong data.  Every schedule runs twice in a row without a synchronize
between the rounds (the defect was in the second step), every image is compared with the CPU oracle and with the same
calls made on one idle context.

What a pass means: the runtime's reason for that late fill was never established, so a pass here is evidence that the
remaining fill-then-kernel pairs are in order on the machine the suite ran on, not a proof that they always are.  Nothing
is run in a loop until it differs.  Cases: tests/call_sequence_cases.py."""
import ctypes as C

import numpy as np
import pytest

import call_sequence_cases as K
import dwt_sweep_tables as T
from test_gpu_batch_chunks import Scope, ids, same_batch, slot_bytes
from test_gpu_coder_edges import _slots
from test_gpu_metadata import nominal_slices, tree_generations

pytestmark = pytest.mark.gpu
vp = C.c_void_p


# ------------------------------------------------------------------------------------------------ the worlds: data + oracle

class World:
    """one geometry: the pictures of a batch and, per distinct picture, the oracle's coefficient array, stream and decoded array"""

    def __init__(self, O, k, pictures, ref):
        self.k, self.P = k, pictures
        self.B, self.c = k["B"], k["c"]
        g = ref["geom"]
        self.geom = (k["c"], g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"])
        self.n = k["c"] * g["enc_h"] * g["enc_w"]
        self.which = np.arange(self.B) % len(ref["streams"])  # picture b is distinct picture which[b]
        self.ref = ref
        self.slot = slot_bytes(self.geom, k["max_bits"])
        self.wid, self.mid, self.lv = ids(k)
        self.F = len(O.wavelet_filters(k["wavelet"])[0])

    def streams(self, order):
        return [self.ref["streams"][self.which[b]] for b in order]

    def max_n(self, order):
        return np.array([self.ref["max_n"][self.which[b]] for b in order], np.uint8)

    def nbits(self, order):
        return np.array([self.ref["nbits"][self.which[b]] for b in order], np.uint64)

    def same_rows(self, got, name, order, what):
        """got [B, n] against the oracle's arrays ref[name] of the pictures in `order`, image by image"""
        assert got.shape == (len(order), self.n) and got.dtype == np.int32, (what, got.shape, got.dtype)
        bad = [b for b, pic in enumerate(order) if not np.array_equal(got[b], self.ref[name][self.which[pic]].reshape(-1))]
        assert not bad, "%s: %d of %d images differ, first %s" % (what, len(bad), len(order), bad[:8])

    def max_words(self, order):
        mx = [int(np.abs(x.astype(np.int64)).max()) for x in self.ref["coeffs"]]
        return np.array([mx[self.which[b]] for b in order], np.uint32)


def list_world(O):
    return K.cached("list_world", lambda: World(O, K.LIST, K.list_pictures(), K.list_reference(O)))


def rest_world(O):
    def make():
        k = K.REST
        P = K.pictures(k, 4800)
        streams, ns, nbits, recs, coeffs = [], [], [], [], []
        for img in P:
            arr, g = O.wavedec2_array(img, k["wavelet"], k["mode"], k["level"])
            co = O.quantize(arr, k["q"], None)
            d, n, nb = O.encode_nbits(co, g["ll_h"], g["ll_w"], k["max_bits"])
            streams.append(d)
            ns.append(n)
            nbits.append(nb)
            coeffs.append(co)
            recs.append(O.decode(d, n, k["c"], g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"]))
        return World(O, k, P, dict(streams=streams, max_n=ns, nbits=nbits, rec=recs, coeffs=coeffs, geom=g))
    return K.cached("rest_world", make)


orders = K.orders


# ------------------------------------------------------------------------------------------------ producers and the schedule

class Run:
    """the arrays of one run of a schedule (allocated through one Scope; device memory belongs to no context) and the calls
    of the two producers"""

    def __init__(self, O, w, s):
        self.O, self.w, self.s = O, w, s
        B, n = w.B, w.n
        self.word = s.zeros((1,), np.uint32)  # the gate's: it stays 0
        self.img, self.co, self.dm, self.lm, self.mx, self.R, self.p1 = [], [], [], [], [], [], []
        for r in range(K.ROUNDS):
            po, _ = orders(B, r)
            self.img.append(s.dev(w.P[po]))
            self.co.append(s.empty((B, n), np.int32))
            self.dm.append(s.empty((B, n), np.uint8))
            self.lm.append(s.empty((B, n), np.uint8))
            self.mx.append(s.empty((B,), np.uint32))
            for d in (self.co[-1], self.dm[-1], self.lm[-1], self.mx[-1]):
                s.ctx.memset(d.ptr, 0x7F, d.nbytes)
            self.R.append(s.empty((B, n), np.int32))
            s.ctx.memset(self.R[-1].ptr, 0x7F, self.R[-1].nbytes)
            self.p1.append(self.streams(po))
        s.ctx.synchronize()

    def streams(self, order):
        data, nbytes = _slots(self.w.streams(order), self.w.slot)
        return self.s.dev(data), self.s.dev(nbytes), self.s.dev(self.w.max_n(order))

    def gate(self, p):
        p.check(p.L.spiht_ctx_wait_resident(p.ctx.handle, vp(self.word.ptr), 1, K.GATE_US))

    def produce0(self, p, r):
        w, k = self.w, self.w.k
        p.check(p.L.spiht_dwt_pyramid_batch_f64(p.ctx.handle, vp(self.img[r].ptr), w.B, w.c, k["H"], k["W"], w.wid, w.mid, w.lv, k["q"], None,
                                                vp(self.co[r].ptr), vp(self.dm[r].ptr), vp(self.lm[r].ptr), vp(self.mx[r].ptr)))

    def produce1(self, p, r):
        w = self.w
        d, ny, mn = self.p1[r]
        p.check(p.L.spiht_decode_batch_i32(p.ctx.handle, vp(d.ptr), w.slot, vp(ny.ptr), vp(mn.ptr), w.B, *w.geom, vp(self.R[r].ptr)))


def schedule(run, case, p0, p1, l, wait="events"):
    """ROUNDS rounds, nothing waited for on the host until the end.  p0 is p1 is l: the idle form, one context, no events."""
    events = []
    for r in range(K.ROUNDS):
        case.before(run, l, r)
        if p0 is l:
            run.produce0(l, r)
            run.produce1(l, r)
        else:
            for p, produce in ((p0, run.produce0), (p1, run.produce1)):
                run.gate(p)
                produce(p, r)
                if wait == "events":
                    events.append(p.ctx.record())
                    l.ctx.wait_event(events[-1])
                else:
                    l.ctx.wait_on(p.ctx)
        case.consume(run, l, r)
    for s in (l, p0, p1):
        s.ctx.synchronize()


def run_case(O, w, case, wait="events"):
    with Scope() as si:
        case.configure(si)
        run = Run(O, w, si)
        case.setup(run)
        schedule(run, case, si, si, si)
        idle = case.collect(run)
    with Scope() as l, Scope() as p0, Scope() as p1:
        case.configure(l)
        run = Run(O, w, l)
        case.setup(run)
        schedule(run, case, p0, p1, l, wait)
        got = case.collect(run)
        for r in range(K.ROUNDS):  # what the producers left, where the consumer did not overwrite it
            producers_products(O, w, run, r, *case.producers_keep)
    for r in range(K.ROUNDS):
        case.against_the_oracle(O, w, got[r], r)
        for name in got[r]:
            same_batch(got[r][name], idle[r][name], "round %d, %s against the idle context" % (r, name))


class Case:
    producers_keep = (True, True)  # (P0's arrays, P1's) still hold the producers' results after the consumer's call

    def configure(self, l):
        pass

    def setup(self, run):
        pass

    def before(self, run, l, r):
        pass


def producers_products(O, w, run, r, co=True, R=True):
    po, _ = orders(w.B, r)
    if co:
        w.same_rows(run.co[r].download(), "coeffs", po, "round %d: P0's coefficient arrays" % r)
        same_batch(run.mx[r].download(), w.max_words(po), "round %d: P0's max words" % r)
    if R:
        w.same_rows(run.R[r].download(), "rec", po, "round %d: P1's decoded arrays" % r)


# ------------------------------------------------------------------------------------------------ the consumer calls

class EncodeLists(Case):
    """spiht_encode_lists_batch_i32 on P0's arrays.  wide_encode 0: k_encode clears its own slot; 2: the several-CUs encoder,
    whose slots and control words are zero-filled in front of it"""

    def __init__(self, wide):
        self.wide = wide

    def configure(self, l):
        l.ctx.set_option("wide_encode", self.wide)

    def setup(self, run):
        w, s = run.w, run.s
        self.out = [s.empty((w.B, w.slot), np.uint8) for _ in range(K.ROUNDS)]
        self.nb = [s.empty((w.B,), np.uint64) for _ in range(K.ROUNDS)]
        self.mn = [s.empty((w.B,), np.uint8) for _ in range(K.ROUNDS)]
        for d in self.out + self.nb + self.mn:
            s.ctx.memset(d.ptr, 0x7F, d.nbytes)
        s.ctx.synchronize()

    def consume(self, run, l, r):
        w = run.w
        l.check(l.L.spiht_encode_lists_batch_i32(l.ctx.handle, vp(run.co[r].ptr), vp(run.dm[r].ptr), vp(run.lm[r].ptr), vp(run.mx[r].ptr),
                                                 w.B, *w.geom, w.k["max_bits"], vp(self.out[r].ptr), w.slot, vp(self.nb[r].ptr),
                                                 vp(self.mn[r].ptr)))

    def collect(self, run):
        return [dict(slots=self.out[r].download(), nbits=self.nb[r].download(), max_n=self.mn[r].download()) for r in range(K.ROUNDS)]

    def against_the_oracle(self, O, w, got, r):
        po, _ = orders(w.B, r)
        streams = w.streams(po)
        same_batch(got["max_n"], w.max_n(po), "round %d: max_n" % r)
        same_batch(got["nbits"], w.nbits(po), "round %d: nbits" % r)
        same_batch(got["slots"], K.slots_of(streams, w.slot), "round %d: streams and the zeros behind them" % r)


class DecodeInto(Case):
    """a decode call of the consumer's own streams into the array P1 has just written (decode_batch, metadata, unscatter) or
    into an array kept zero (lists_flags)"""

    def __init__(self, call):
        self.call = call
        self.producers_keep = (True, call == "lists_flags")

    def setup(self, run):
        w, s = run.w, run.s
        self.mine = [run.streams(orders(w.B, r)[1]) for r in range(K.ROUNDS)]
        if self.call == "lists_flags":
            words = C.c_uint64()
            s.check(s.L.spiht_l1_flags_words(w.c, w.k["H"], w.k["W"], w.wid, w.mid, w.lv, C.byref(words)))
            assert words.value > 0
            self.words = int(words.value)
            self.Z = [s.zeros((w.B, w.n), np.int32) for _ in range(K.ROUNDS)]
            self.fl = [s.empty((w.B, self.words), np.uint32) for _ in range(K.ROUNDS)]
            for d in self.fl:
                s.ctx.memset(d.ptr, 0x7F, d.nbytes)
        if self.call == "metadata":
            c, h, ww, lh, lw = w.geom
            self.top, self.other = nominal_slices(lh, lw, tree_generations(h, ww, lh, lw))
            self.flat = run.O.flatten_slices(self.top, self.other)
            self.rows = 8 * w.slot + 1
            self.meta = [s.empty((w.B, self.rows, 8), np.int32) for _ in range(K.ROUNDS)]
            for d in self.meta:
                s.ctx.memset(d.ptr, 0x7F, d.nbytes)
        s.ctx.synchronize()

    def consume(self, run, l, r):
        w = run.w
        d, ny, mn = self.mine[r]
        head = (l.ctx.handle, vp(d.ptr), w.slot, vp(ny.ptr), vp(mn.ptr), w.B)
        if self.call == "decode_batch":
            l.check(l.L.spiht_decode_batch_i32(*head, *w.geom, vp(run.R[r].ptr)))
        elif self.call == "lists_flags":
            l.check(l.L.spiht_decode_lists_flags_batch_i32(*head, w.c, w.k["H"], w.k["W"], w.wid, w.mid, w.lv, vp(self.Z[r].ptr),
                                                           vp(self.fl[r].ptr)))
        elif self.call == "metadata":
            topv, oth, level = self.flat
            l.check(l.L.spiht_decode_with_metadata_batch_i32(*head, *w.geom, vp(topv.ctypes.data), vp(oth.ctypes.data), level,
                                                             vp(run.R[r].ptr), vp(self.meta[r].ptr), self.rows))
        else:  # the fill fall-back (the context's last list decode, if any, was into another array), then a decode into it
            l.check(l.L.spiht_unscatter_lists_batch_i32(l.ctx.handle, vp(run.R[r].ptr), w.B, *w.geom[:3]))
            l.check(l.L.spiht_decode_lists_batch_i32(*head, *w.geom, vp(run.R[r].ptr)))

    def collect(self, run):
        got = []
        for r in range(K.ROUNDS):
            if self.call == "lists_flags":
                got.append(dict(rec=self.Z[r].download(), words=self.fl[r].download()))
            else:
                got.append(dict(rec=run.R[r].download()))
            if self.call == "metadata":
                got[-1]["meta"] = self.meta[r].download()
        return got

    def against_the_oracle(self, O, w, got, r):
        mine = orders(w.B, r)[1]
        w.same_rows(got["rec"], "rec", mine, "round %d: decoded arrays (%s)" % (r, self.call))
        if self.call == "lists_flags":
            k = w.k
            rec = got["rec"].reshape(w.B, w.c, w.geom[1], w.geom[2])
            occ = T.occupancy_words(rec, k["H"], k["W"], w.F).reshape(w.B, -1)
            assert occ.shape == got["words"].shape
            assert not (occ[got["words"] == 0]).any(), "round %d: a zero word over a tile that holds coefficients" % r
            assert (got["words"] == 0).any() and (got["words"] != 0).any()
        if self.call == "metadata":
            for b, pic in enumerate(mine):
                d, n = w.ref["streams"][w.which[pic]], w.ref["max_n"][w.which[pic]]
                _, m = O.decode_with_metadata(d, n, *w.geom, self.top, self.other)
                assert np.array_equal(got["meta"][b, :len(m)], m), "round %d image %d: metadata rows" % (r, b)
                assert not got["meta"][b, len(m):].any(), "round %d image %d: rows past the stream" % (r, b)


class Budgets(Case):
    """spiht_decode_budgets_dev_i32 of one stream to B budgets into the array P1 has just written (zero-filled by the call).
    The call waits for its context's stream when it stages the stream, so its fill of the K arrays is queued with the wait
    already over: a late fill after a wait cannot be reached through this call, in this schedule or any other.  What the
    case shows is that the wait holds (the arrays are P1's before, the call's after) and that the call is right there."""

    producers_keep = (True, False)

    @staticmethod
    def budgets(w, r):
        pic = orders(w.B, r)[1][0]
        d = np.frombuffer(w.ref["streams"][w.which[pic]], np.uint8)
        return d, int(w.ref["max_n"][w.which[pic]]), np.ascontiguousarray([1 + (8 * len(d) * (j + 1)) // w.B - (j % 2) for j in range(w.B)],
                                                                            np.uint64)

    def consume(self, run, l, r):
        w = run.w
        d, n, bud = self.budgets(w, r)
        l.check(l.L.spiht_decode_budgets_dev_i32(l.ctx.handle, vp(d.ctypes.data), len(d), n, *w.geom, vp(bud.ctypes.data), w.B,
                                                 vp(run.R[r].ptr)))

    def collect(self, run):
        return [dict(rec=run.R[r].download()) for r in range(K.ROUNDS)]

    def against_the_oracle(self, O, w, got, r):
        d, n, bud = self.budgets(w, r)
        bits = O.bytes_to_bits(d.tobytes())
        want = np.stack([O.decode_bits(bits[:int(b)], n, *w.geom) for b in bud]).reshape(w.B, -1)
        same_batch(got["rec"], want, "round %d: the arrays of the budgets" % r)


class Pyramid(Case):
    """spiht_dwt_pyramid_batch_f64 of the consumer's own pictures into the arrays P0 has just written: the max words are
    zero-filled in front of kernels that raise them with atomicMax"""

    producers_keep = (False, True)

    def setup(self, run):
        w = run.w
        self.mine = [run.s.dev(w.P[orders(w.B, r)[1]]) for r in range(K.ROUNDS)]
        run.s.ctx.synchronize()

    def consume(self, run, l, r):
        w, k = run.w, run.w.k
        l.check(l.L.spiht_dwt_pyramid_batch_f64(l.ctx.handle, vp(self.mine[r].ptr), w.B, w.c, k["H"], k["W"], w.wid, w.mid, w.lv, k["q"], None,
                                                vp(run.co[r].ptr), vp(run.dm[r].ptr), vp(run.lm[r].ptr), vp(run.mx[r].ptr)))

    def collect(self, run):
        return [dict(coeffs=run.co[r].download(), max_words=run.mx[r].download(), dcode=run.dm[r].download(), lcode=run.lm[r].download())
                for r in range(K.ROUNDS)]

    def against_the_oracle(self, O, w, got, r):
        mine = orders(w.B, r)[1]
        co = [w.ref["coeffs"][w.which[b]] for b in mine]
        w.same_rows(got["coeffs"], "coeffs", mine, "round %d: coefficient arrays" % r)
        same_batch(got["max_words"], w.max_words(mine), "round %d: max words" % r)
        c, h, ww, lh, lw = w.geom
        I, J = np.arange(h)[:, None], np.arange(ww)[None, :]
        b_entry = ((4 * I + 3 < h) & (4 * J + 3 < ww))[None]
        for b in range(w.B):
            d_ref, l_ref, has = O.set_codes(co[b], lh, lw)
            assert np.array_equal(got["dcode"][b].reshape(c, h, ww)[has], d_ref[has]), (r, b)
            assert np.array_equal(got["lcode"][b].reshape(c, h, ww)[has & b_entry], l_ref[has & b_entry]), (r, b)


class FusedAfterSlotReuse(Case):
    """spiht_decode_image_batch_f64 with the internal array, right after a call that reused its decoder slots has left that
    array marked dirty: the call starts with the fill of the whole array"""

    def setup(self, run):
        w, s, O = run.w, run.s, run.O
        k = K.TINY
        base = K.image_reference(O, k, K.tiny_pictures()[:k["distinct"]])
        which = np.arange(k["B"]) % k["distinct"]
        data, nbytes = _slots([base[0][i] for i in which])
        self.tiny = (s.dev(data), s.dev(nbytes), s.dev(np.array([base[1][i] for i in which], np.uint8)), data.shape[1])
        self.tiny_out = s.empty((k["B"], k["c"], k["H"], k["W"]), np.float64)
        self.tiny_want = base[2][which]
        self.mine = [run.streams(orders(w.B, r)[1]) for r in range(K.ROUNDS)]
        g = O.geometry(w.k["H"], w.k["W"], w.k["wavelet"], w.k["level"], w.k["mode"])
        self.pics = [s.empty((w.B, w.c, 2 * g["hs"][1] - w.F + 2, 2 * g["ws"][1] - w.F + 2), np.float64) for _ in range(K.ROUNDS)]
        for d in self.pics:
            s.ctx.memset(d.ptr, 0x7F, d.nbytes)
        s.ctx.synchronize()

    def before(self, run, l, r):
        k = K.TINY
        wid, mid, lv = ids(k)
        d, ny, mn, slot = self.tiny
        assert k["B"] > 8 * l.ctx.get_option("num_cu")
        l.check(l.L.spiht_decode_image_batch_f64(l.ctx.handle, vp(d.ptr), slot, vp(ny.ptr), vp(mn.ptr), k["B"], k["c"], k["H"], k["W"], wid,
                                                 mid, lv, k["q"], None, vp(self.tiny_out.ptr), None))

    def consume(self, run, l, r):
        w, k = run.w, run.w.k
        d, ny, mn = self.mine[r]
        l.check(l.L.spiht_decode_image_batch_f64(l.ctx.handle, vp(d.ptr), w.slot, vp(ny.ptr), vp(mn.ptr), w.B, w.c, k["H"], k["W"], w.wid,
                                                 w.mid, w.lv, k["q"], None, vp(self.pics[r].ptr), None))

    def collect(self, run):
        same_batch(self.tiny_out.download(), self.tiny_want, "the tiny pictures of the slot-reuse call")
        return [dict(pictures=self.pics[r].download()) for r in range(K.ROUNDS)]

    def against_the_oracle(self, O, w, got, r):
        k = w.k
        mine = orders(w.B, r)[1]
        want = np.stack([O.waverec2_array(O.dequantize(w.ref["rec"][w.which[b]], k["q"], None), k["H"], k["W"], k["wavelet"], k["level"],
                                          k["mode"]) for b in mine])
        same_batch(got["pictures"], want, "round %d: pictures" % r)


# ------------------------------------------------------------------------------------------------ the tests

def test_the_gate_ends_by_itself():
    """spiht_ctx_wait_resident on a word that never reaches its target: the call returns, the gate gives up after its
    bound, and synchronize() succeeds; on a word that is there already, and without a word, nothing waits; a bound above
    10 ms is refused"""
    with Scope() as s:
        word = s.zeros((2,), np.uint32)
        s.ctx.upload(word.ptr + 4, np.array([7], np.uint32))
        s.check(s.L.spiht_ctx_wait_resident(s.ctx.handle, vp(word.ptr), 1, K.GATE_US))
        s.ctx.synchronize()
        s.check(s.L.spiht_ctx_wait_resident(s.ctx.handle, vp(word.ptr + 4), 7, 10000))
        s.check(s.L.spiht_ctx_wait_resident(s.ctx.handle, None, 1, 10000))
        s.ctx.synchronize()
        with pytest.raises(ValueError):
            s.check(s.L.spiht_ctx_wait_resident(s.ctx.handle, vp(word.ptr), 1, 10001))
        assert word.download().tolist() == [0, 7]


@pytest.mark.parametrize("wide", [0, 2])
def test_encode_lists_first_after_the_waits(oracle, wide):
    run_case(oracle, list_world(oracle), EncodeLists(wide))


def test_decode_lists_flags_first_after_the_waits(oracle):
    run_case(oracle, list_world(oracle), DecodeInto("lists_flags"))


@pytest.mark.parametrize("call", ["decode_batch", "metadata", "unscatter"])
def test_decode_first_after_the_waits(oracle, call):
    run_case(oracle, rest_world(oracle), DecodeInto(call))


def test_unscatter_fill_first_after_the_waits_at_batch_size(oracle):
    """the fill fall-back of spiht_unscatter_lists_batch_i32 and the list decode behind it, at the size at which the pipelined
    schedule queues that fill as the first operation after spiht_ctx_wait_event"""
    run_case(oracle, list_world(oracle), DecodeInto("unscatter"))


def test_decode_budgets_first_after_the_waits(oracle):
    run_case(oracle, rest_world(oracle), Budgets())


def test_dwt_pyramid_first_after_the_waits(oracle):
    run_case(oracle, rest_world(oracle), Pyramid())


def test_fused_decode_first_after_the_waits(oracle):
    run_case(oracle, rest_world(oracle), FusedAfterSlotReuse())


def test_wait_on_orders_the_same_pair(oracle):
    """spiht_ctx_wait_on in place of the two events"""
    run_case(oracle, rest_world(oracle), DecodeInto("decode_batch"), wait="wait_on")
