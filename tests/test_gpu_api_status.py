"""What every pixel-typed entry point answers to ONE bad argument (or two: the order of the checks), row by row.

A row is (entry point, element, spoiled arguments) -> status.  Every row starts from a call that passes -- B = 2, c = 3, 16 x 16
pictures, level 2, bior2.2, reflect; tiles of 8 x 8 on a 16 x 24 picture, overlap margin 2; device buffers behind every pointer
that hold the operands of these shapes many times over -- and spoils what its name says.  Only arguments the host code refuses
before it queues anything are spoiled (rules(): which spoil applies to which family), so nothing here ever runs a kernel on a
bad pointer.  The expected statuses (tests/golden/api_status.json) were recorded by running this table on the GPU at the commit
before the one api.cpp of then was split by topic (today: csrc/api_*.cpp); rows that returned SPIHT_OK there are not in the table (NOT_REFUSED).

    python tests/test_gpu_api_status.py record FILE     writes the JSON from the library that is built (GPU)
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_status.json")
ES = {"f64": 8, "f32": 4, "f32s": 4, "u8": 1, "u16": 2, "flt1": 4, "flt2": 2}  # (flt1: the float32 kind, flt2: float16)
VIEW = ("u8", "u16", "f32s", "flt1", "flt2")  # elements that come as a view by byte strides
BUF = 1 << 20  # bytes of every device buffer: the largest operand of these shapes (float64 [2, 3, 16, 24]) is 18 KB

IMG = "B c H W wavelet mode level q mults"
ONE = "c H W wavelet mode level q mults"
WIN = "i0 i1 j0 j1 y0 x0 wh ww"
S_IMG = ["null_pic", "misalign", "neg_stride", "odd_stride", "overlap", "c0", "c65536", "H_big", "wavelet", "mode", "level0",
         "kind"]
S_TILE = ["null_pic", "misalign", "neg_stride", "odd_stride", "overlap", "c0", "c65536"]
S_WIN = S_TILE + ["window", "subgrid"]


def fam(sig, pic, symbols, spoils, sdims=None, writes=False, dense_aligned=False):
    return dict(sig=sig.split(), pic=pic, symbols=symbols, spoils=spoils, sdims=sdims, writes=writes, dense_aligned=dense_aligned)


def _sym(stem, elems):
    return {e: "spiht_%s_%s" % (stem, "flt" if e.startswith("flt") else e) for e in elems.split()}


# [kind]: only the *_flt calls have it; [strides]: only the views.  sdims: the extents the strides describe.
FAMILIES = {
    "enc_batch": fam("ctx [kind] img [strides] " + IMG + " max_bits slots slot_stride nbits maxn coef", "img",
                     _sym("encode_image_batch", "f64 f32 u8 u16 flt1 flt2"), S_IMG, "B c H W"),
    "dec_batch": fam("ctx [kind] slots slot_stride nbytes maxn " + IMG + " pix_out [strides] coef", "pix_out",
                     _sym("decode_image_batch", "f64 u8 u16 flt1 flt2"), S_IMG, "B c H W", writes=True),
    "enc_host": fam("ctx [kind] himg [strides] " + ONE + " max_bits hout out_cap p_nbits p_maxn", "himg",
                    _sym("encode_image_host", "f64 f32 u8 u16 flt1 flt2"), S_IMG, "c H W"),
    # (level 0: the host decode stages its stream before the batch call refuses the geometry -- not a row)
    "dec_host": fam("ctx [kind] hdata nbytes0 n0 " + ONE + " himg_out [strides]", "himg_out",
                    _sym("decode_image_host", "f64 u8 u16 flt1 flt2"), [s for s in S_IMG if s != "level0"], "c H W", writes=True),
    "dequant_host": fam("ctx hrec " + ONE + " himg_out", "himg_out", _sym("dequant_idwt_host", "f64"), S_IMG),
    "dwt_quant": fam("ctx img " + IMG + " coef", "img", _sym("dwt_quant_batch", "f64 f32"), S_IMG),
    "dequant": fam("ctx coef " + IMG + " pix_out", "pix_out", _sym("dequant_idwt_batch", "f64"), S_IMG),
    "dequant_flags": fam("ctx [kind] coef flags " + IMG + " pix_out [strides]", "pix_out",
                         _sym("dequant_idwt_flags_batch", "f64 u8 u16 flt1 flt2"), S_IMG, "B c H W", writes=True),
    "idwt_coarse": fam("ctx coef " + IMG + " approx", "approx", _sym("idwt_coarse_batch", "f64"), S_IMG),
    "idwt_level1": fam("ctx coef approx " + IMG + " pix_out", "pix_out", _sym("idwt_level1_batch", "f64"), S_IMG),
    "idwt_level1_flags": fam("ctx coef approx flags " + IMG + " pix_out [strides]", "pix_out",
                             _sym("idwt_level1_flags_batch", "f64 u8 u16"), S_IMG, "B c H W", writes=True),
    "dwt_pyramid": fam("ctx [kind] img [strides] " + IMG + " coef dmsb lmsb maxabs", "img",
                       _sym("dwt_pyramid_batch", "f64 u8 u16 flt1 flt2"), S_IMG, "B c H W"),
    "dequant_reduced": fam("ctx [kind] coef " + IMG + " pix_out [strides] reduce", "pix_out",
                           _sym("dequant_idwt_reduced_batch", "f64 u8 u16 flt1 flt2"), S_IMG + ["reduce"], "B c RH RW", writes=True),
    "dec_reduced": fam("ctx [kind] slots slot_stride nbytes maxn " + IMG + " pix_out [strides] coef reduce", "pix_out",
                       _sym("decode_image_reduced_batch", "f64 u8 u16 flt1 flt2"), S_IMG + ["reduce"], "B c RH RW", writes=True),
    "dec_reduced_host": fam("ctx [kind] hdata nbytes0 n0 " + ONE + " himg_out [strides] reduce", "himg_out",
                            _sym("decode_image_reduced_host", "f64 u8 u16 flt1 flt2"),
                            [s for s in S_IMG if s != "level0"] + ["reduce"], "c RH RW", writes=True),
    "convert": fam("ctx kind f64in B c H2 W2 H W pix_out strides", "pix_out", {"flt1": "spiht_convert_batch_flt", "flt2": "spiht_convert_batch_flt"},
                   ["null_pic", "misalign", "neg_stride", "odd_stride", "overlap", "c0", "H_big", "kind"], "B c H W", writes=True),
    "widen": fam("ctx kind img strides B c H W f64out", "img", {"flt1": "spiht_widen_batch_flt", "flt2": "spiht_widen_batch_flt"},
                 ["null_pic", "misalign", "neg_stride", "odd_stride", "c0", "H_big", "kind"], "B c H W"),
    "check_view": fam("[kind] B c H W strides output", None, _sym("check_view", "u8 u16 flt1 flt2"),
                      ["neg_stride", "odd_stride", "overlap", "c0", "c65536", "H_big", "kind"], "B c H W", writes=True),
    # the sums and the tiles take pictures of up to 2^30 rows: H = 2^24 + 1 is no error there, so it is no row
    "sse_f64": fam("ctx pic dec K c H W H2 W2 out", "pic", _sym("sse", "f64"), S_TILE),
    "sse": fam("ctx pic strides dec K c H W out", "pic", _sym("sse", "u8 u16"), S_TILE, "c H W"),
    "tile_cut": fam("ctx timg [strides] N c PH PW th tw tiles", "timg", _sym("tile_cut", "u8 u16 f32s f32 f64"), S_TILE, "N c PH PW",
                    dense_aligned=True),
    "tile_cut_overlap": fam("ctx timg [strides] N c PH PW th tw m tiles", "timg", _sym("tile_cut_overlap", "u8 u16 f32s f32 f64"),
                            S_TILE + ["m_big"], "N c PH PW", dense_aligned=True),
    "tile_paste": fam("ctx tiles c th tw PH PW th tw " + WIN + " tout [strides]", "tout", _sym("tile_paste", "u8 u16 f32s f32 f64"),
                      S_WIN, "c wh ww", writes=True, dense_aligned=True),
    "tile_mosaic": fam("ctx tiles c th tw oy ox PH PW th tw " + WIN + " tout [strides]", "tout",
                       dict(_sym("tile_mosaic", "u8 u16 f64"), f32s="spiht_tile_mosaic_f32"), S_WIN, "c wh ww", writes=True,
                       dense_aligned=True),
    "tile_blend": fam("ctx [kind] tiles c thm twm PH PW th tw m " + WIN + " tout [strides]", "tout",
                      _sym("tile_blend", "u8 u16 flt1 flt2 f64"), S_WIN + ["m_big", "kind"], "c wh ww", writes=True, dense_aligned=True),
    "sse_tiles": fam("ctx [kind] tiles dec G N c PH PW th tw th tw out", "tiles", _sym("sse_tiles", "f64 u8 u16 flt1 flt2"),
                     ["null_pic", "misalign", "c0", "c65536", "kind"], dense_aligned=True),
    "sse_tiles_w": fam("ctx [kind] tiles dec G N c PH PW th tw th tw out w w_stride", "tiles", _sym("sse_tiles_w", "f64 u8 u16 flt1 flt2"),
                       ["null_pic", "misalign", "c0", "c65536", "kind"], dense_aligned=True),
}

# rows of rules() that the library at the recording commit did NOT refuse (they returned SPIHT_OK): not part of the table
NOT_REFUSED = set()


def spoils_of(f, elem):
    es, view, out = ES[elem], elem in VIEW, []
    for s in f["spoils"]:
        if s == "misalign" and (es == 1 or not (view or f["dense_aligned"])):
            continue  # (a byte is always aligned; the dense image calls do not look at the base)
        if s in ("neg_stride", "odd_stride", "overlap") and not view:
            continue
        if s == "odd_stride" and es == 1:
            continue
        if s == "overlap" and not f["writes"]:
            continue
        if s == "level0" and elem == "f64":
            continue  # (float64 pictures have a level 0)
        if s == "kind" and not elem.startswith("flt"):
            continue
        out.append(s)
    return out


def rules():
    """the table: (family, element, (spoil, ...)), every single spoil of an entry point and the pairs of neighbours in its list"""
    rows = []
    for name, f in FAMILIES.items():
        for elem in f["symbols"]:
            sp = spoils_of(f, elem)
            rows += [(name, elem, (s,)) for s in sp]
            pairs = [(sp[i], sp[(i + 1) % len(sp)]) for i in range(len(sp)) if len(sp) > 2]
            rows += [(name, elem, p) for p in pairs if p != ("c0", "c65536")]  # (both are values of c)
    return [r for r in rows if row_id(r) not in NOT_REFUSED]


def row_id(row):
    name, elem, sp = row
    return "%s[%s] %s" % (FAMILIES[name]["symbols"][elem], elem, "+".join(sp))


class Bench:
    """the operands of the valid calls: one zero-filled device buffer per pointer argument, host arrays for the host calls"""
    DEV = "img pix_out coef slots nbits nbytes maxn dmsb lmsb maxabs flags approx dec tiles timg tout out w f64in f64out pic".split()
    HOST = "himg hout hdata hrec himg_out".split()

    def __init__(self, ctx):
        from spiht_amd import _lib
        self.ctx, self.L = ctx, _lib.lib()
        self.dev = {n: ctx.alloc(BUF) for n in self.DEV}
        for p in self.dev.values():
            ctx.memset(p, 0, BUF)
        self.host = {n: np.zeros(1 << 16, np.uint8) for n in self.HOST}
        wv, md = self.L.spiht_wavelet_id(b"bior2.2"), self.L.spiht_mode_id(b"reflect")
        ph, pw = C.c_int64(), C.c_int64()
        z = C.POINTER(C.c_int64)()
        assert self.L.spiht_reduced_shape(16, 16, wv, md, 2, 1, None, z, z, C.byref(ph), C.byref(pw), z, z, z, z) == 0
        self.vals = dict(B=2, c=3, H=16, W=16, H2=16, W2=16, wavelet=wv, mode=md, level=2, q=50.0, mults=None, max_bits=16384,
                         slot_stride=4096, out_cap=4096, nbytes0=0, n0=0, reduce=1, RH=ph.value, RW=pw.value, K=2, G=1, N=2, PH=16,
                         PW=24, th=8, tw=8, m=2, thm=12, twm=12, oy=0, ox=0, i0=0, i1=2, j0=0, j1=3, y0=0, x0=0, wh=16, ww=24,
                         w_stride=16 * 24, output=1)
        self.keep = []

    def close(self):
        for p in self.dev.values():
            self.ctx.free(p)

    def call(self, name, elem, spoils=()):
        f, es = FAMILIES[name], ES[elem]
        a = dict(self.vals, ctx=self.ctx.handle, kind={"flt1": 1, "flt2": 2}.get(elem, 0))
        a.update({n: p for n, p in self.dev.items()})
        a.update({n: h.ctypes.data for n, h in self.host.items()})
        nb, mn = C.c_uint64(), C.c_uint8()
        a.update(p_nbits=C.byref(nb), p_maxn=C.byref(mn))
        if f["sdims"]:  # dense, in bytes
            ext = [a[d] for d in f["sdims"].split()]
            st = [es * int(np.prod(ext[i + 1:])) for i in range(len(ext))]
            a["strides"] = (C.c_int64 * len(st))(*st)
        n = len(a.get("strides", ()))
        for s in spoils:
            if s == "null_pic":
                a[f["pic"]] = None
            elif s == "misalign":
                a[f["pic"]] = a[f["pic"]] and a[f["pic"]] + 1
            elif s == "neg_stride":
                a["strides"][n - 1] = -es
            elif s == "odd_stride":
                a["strides"][n - 2] += 1
            elif s == "overlap":
                a["strides"][n - 2] = es  # rows on top of one another
            else:
                key, bad = {"c0": ("c", 0), "c65536": ("c", 65536), "H_big": ("H", (1 << 24) + 1), "wavelet": ("wavelet", 1000),
                            "mode": ("mode", 9), "level0": ("level", 0), "reduce": ("reduce", 3), "window": ("y0", 1),
                            "subgrid": ("i1", 1), "m_big": ("m", 5), "kind": ("kind", 7)}[s]
                a[key] = bad
        args = []
        for t in f["sig"]:
            if t == "[kind]":
                if elem.startswith("flt"):
                    args.append(a["kind"])
            elif t == "[strides]":
                if elem in VIEW:
                    args.append(C.addressof(a["strides"]))
            elif t == "strides":
                args.append(C.addressof(a["strides"]))
            else:
                args.append(a[t])
        return int(getattr(self.L, f["symbols"][elem])(*args))


def run_table(ctx):
    b = Bench(ctx)
    try:
        base = {}
        for name, f in FAMILIES.items():  # the valid calls the rows are spoiled from: every one passes
            for elem in f["symbols"]:
                base["%s[%s]" % (f["symbols"][elem], elem)] = b.call(name, elem)
        from spiht_amd import _lib
        base["spiht_ctx_synchronize"] = int(_lib.lib().spiht_ctx_synchronize(ctx.handle))
        got = {row_id(r): b.call(*r) for r in rules()}
    finally:
        b.close()
    return base, got


def test_status_of_every_spoiled_argument(oracle):
    import spiht_amd
    from spiht_amd import _lib
    from conftest import synth_image
    with open(GOLDEN) as fh:  # {"entry point[element]": {"spoil+spoil": status}}, one line per entry point
        want = {"%s %s" % (sym, sp): v for sym, m in json.load(fh).items() for sp, v in m.items()}
    ctx = _lib.default_context()
    base, got = run_table(ctx)
    assert [k for k, v in base.items() if v != 0] == [], "a valid call was refused: %r" % {k: v for k, v in base.items() if v}
    assert sorted(got) == sorted(want), "the table and the recorded rows differ"
    assert all(v != 0 for v in want.values())
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    for k, (g, w) in sorted(diff.items()):
        print("%s: returned %d, recorded %d" % (k, g, w))
    assert not diff
    # ... and the context works as before: one round trip against the oracle (as smoke() does)
    img = synth_image(1000, 3, 16, 16)
    s = spiht_amd.SpihtSettings()
    enc = spiht_amd.encode_image(img, s, level=2, max_bits=16 * 16 * 4)
    ref_bytes, ref_n, _ = oracle.encode_image(img, "bior2.2", "reflect", 2, 50.0, None, 16 * 16 * 4)
    assert enc.encoded_bytes == ref_bytes and enc.max_n == ref_n
    dec = spiht_amd.decode_image(enc, s)
    ref = oracle.decode_image(ref_bytes, ref_n, 3, 16, 16, "bior2.2", 2, 50.0, None)
    assert dec.shape == ref.shape and np.array_equal(dec, ref)


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from spiht_amd import _lib as _l
    base_, got_ = run_table(_l.default_context())
    print("valid calls refused:", {k: v for k, v in base_.items() if v})
    print("not refused:", sorted(k for k, v in got_.items() if v == 0))
    rows_ = {}
    for k_, v_ in sorted(got_.items()):
        if v_ != 0:
            rows_.setdefault(k_.split(" ")[0], {})[k_.split(" ")[1]] = v_
    with open(sys.argv[2], "w") as fh:
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(s_), json.dumps(m_, separators=(",", ":"))) for s_, m_ in rows_.items()) + "\n}\n")
