"""The C calls behind the pixel-typed device methods, case by case, without a device.

A case runs one method of BatchCodec, Pipeline or TiledCodec on a codec whose context is a stub and whose library is a
Recorder: every entry point the method reaches is logged with its arguments and answers SPIHT_OK.  What a constructor or an
argument check needs of the library -- the geometry, the stream bound, the reduced shapes, the view rules: none of them needs a
device -- is forwarded to the library itself.  tests/golden/pixel_calls.json holds the logs of all cases, recorded at the commit
before the Python layer got one pixel element type (spiht_amd/px.py); test_pixel_calls_cpu.py holds every later tree to them.

An argument is logged as what the C side sees of it: a c_void_p as its integer, a host pointer (HOST says at which positions
they are) as the int64 strides or the channel scales it points to, a byref as the tag "byref", a float by repr.  Device
pointers are constants of the case; the stub context hands out 0x40000000, 0x41000000, ... in the order it is asked.

The host forms of TiledCodec, tile_curves and the rate-distortion calls of rd.py read tables back from the device and are left
to the GPU tests.

    python tests/pixel_call_cases.py record FILE     writes the JSON from the tree as it stands (no GPU)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pixel_calls.json")

FORWARDED = ("spiht_encode_bound", "spiht_geometry_mode", "spiht_reduced_shape", "spiht_check_view_u8", "spiht_check_view_u16",
             "spiht_check_view_flt", "spiht_tile_grid", "spiht_tile_reduced_grid", "spiht_wavelet_id", "spiht_mode_id",
             "spiht_wavelet_taps")
FAKE_LIMIT = 1 << 40  # every device pointer of a case lies below it; a host address does not

# ---- where the host pointers are: entry point -> {position (negative: from the end): ("i64", n) strides | ("f64", n) scales}
S4, S3, M = ("i64", 4), ("i64", 3), ("f64", 3)
HOST = {"spiht_encode_image_batch_f64": {10: M}, "spiht_encode_image_batch_f32": {10: M},
        "spiht_decode_image_batch_f64": {13: M}, "spiht_decode_image_reduced_batch_f64": {13: M}}
for _sfx, _k in (("u8", 0), ("u16", 0), ("flt", 1)):  # (a *_flt call has the kind behind the context)
    HOST["spiht_encode_image_batch_" + _sfx] = {2 + _k: S4, 11 + _k: M}
    HOST["spiht_decode_image_batch_" + _sfx] = HOST["spiht_decode_image_reduced_batch_" + _sfx] = {13 + _k: M, 15 + _k: S4}
for _sfx in ("u8", "u16"):
    HOST["spiht_pipeline_submit_" + _sfx] = {2: S4, 7: S4}
for _sfx in ("u8", "u16", "f32s"):
    HOST["spiht_tile_cut_" + _sfx] = HOST["spiht_tile_cut_overlap_" + _sfx] = {2: S4}
for _name in ("paste_u8", "paste_u16", "paste_f32s", "mosaic_u8", "mosaic_u16", "mosaic_f32", "blend_u8", "blend_u16", "blend_flt"):
    HOST["spiht_tile_" + _name] = {-1: S3}


def _norm(name, args):
    host = {(i if i >= 0 else len(args) + i): v for i, v in HOST.get(name, {}).items()}
    out = []
    for i, a in enumerate(args):
        if i in host and a is not None:
            ctype, n = host[i]
            values = ({"i64": C.c_int64, "f64": C.c_double}[ctype] * n).from_address(a.value)
            out.append([ctype] + [int(v) if ctype == "i64" else repr(float(v)) for v in values])
        elif a is None:
            out.append(None)
        elif isinstance(a, C.c_void_p):
            if a.value is not None and a.value >= FAKE_LIMIT:
                raise AssertionError("%s: a host pointer at position %d, which HOST does not list" % (name, i))
            out.append(a.value)
        elif type(a).__name__ == "CArgObject":
            out.append("byref")
        elif isinstance(a, (float, np.floating)):
            out.append(repr(float(a)))
        elif isinstance(a, (int, np.integer)) and not isinstance(a, bool):
            out.append(int(a))
        else:
            raise AssertionError("%s: argument %d is a %s" % (name, i, type(a).__name__))
    return out


class Recorder:
    """stands in for a codec's L"""

    def __init__(self, real):
        self._real, self.log = real, []

    def __getattr__(self, name):
        if not name.startswith("spiht_"):
            raise AttributeError(name)
        if name in FORWARDED:
            return getattr(self._real, name)

        def call(*args):
            self.log.append([name, _norm(name, args)])
            return 0
        return call


class StubContext:
    """what the methods need of a _lib.Context, with no device behind it"""
    device = 0

    def __init__(self):
        self.handle = C.c_void_p(0x10)
        self._next = 0x40000000

    def alloc(self, nbytes):
        p, self._next = self._next, self._next + 0x1000000
        return p

    def free(self, ptr):
        pass

    def memset(self, ptr, value, nbytes):
        pass

    def upload(self, ptr, arr):
        pass

    def synchronize(self):
        pass


class Dev:
    """a device buffer as the tile calls take one: an address, an element type, a size"""

    def __init__(self, ptr, dtype=np.uint8, nbytes=1 << 20):
        self.ptr, self.dtype, self.nbytes = ptr, dtype, nbytes


# the device pointers of the cases
IMG, OUT, NBITS, MAXN, COEF, DATA, NBYTES, PIX, REC = (0x10000000 + 0x1000000 * i for i in range(9))
PACKED, LENS, CUM, PICB, ROI, TARGET, SEL = (0x20000000 + 0x1000000 * i for i in range(7))
B, CH = 2, 3
# the codecs of the batch cases: (3, 8, 10) with level=1, and -- the library refuses an 8 x 10 picture at its default level, whose
# root block is larger than its sub-bands -- the default level on (3, 16, 20)
CODECS = {"L1": (8, 10, 1), "LNone": (16, 20, None)}
ES = {"f64": 8, "f32": 4, "u8": 1, "u16": 2, "float32": 4, "float16": 2, "bfloat16": 2}
KINDS = ("float32", "float16", "bfloat16")


def cl4(b_unused, c, h, w, es):
    """byte strides (sb, sc, sh, sw) of [B, c, h, w] pictures stored channels-last"""
    return (h * w * c * es, es, w * c * es, c * es)


def cl3(c, h, w, es):
    return (es, w * c * es, c * es)


def _batch_codec(which="L1", pixel_dtype=np.float64, scales=None):
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec
    s = spiht_amd.SpihtSettings(per_channel_quant_scales=scales)
    H, W, level = CODECS[which]
    codec = BatchCodec(CH, H, W, s, level, 4000, ctx=StubContext(), pixel_dtype=pixel_dtype)
    codec.L = Recorder(_lib.lib())
    return codec


def _encode(codec, elem, strides, coef):
    enc = (IMG, B, OUT, NBITS, MAXN)
    if elem in ("f64", "f32"):
        codec.encode_device(*enc, d_coeffs=coef)
    elif elem in KINDS:
        codec.encode_device_float(*enc, elem, strides, coef)
    else:
        getattr(codec, "encode_device_" + elem)(*enc, strides)


def _decode(codec, elem, reduce, strides, rec, slot):
    dec = (DATA, NBYTES, MAXN, B, PIX)
    red = () if reduce is None else (reduce,)
    stem = "decode_device" if reduce is None else "decode_reduced_device"
    if elem == "f64":
        getattr(codec, stem)(*dec, *red, d_rec=rec, slot_stride=slot)
    elif elem in KINDS:
        getattr(codec, stem + "_float")(*dec, *red, elem, strides, rec, slot)
    else:
        getattr(codec, stem + "_" + elem)(*dec, *red, strides, rec, slot)


def batch_cases():
    """name -> a function that runs the case and returns the log"""
    cases = {}

    def add(name, make, run):
        def case():
            codec = make()
            run(codec)
            return codec.L.log
        assert name not in cases
        cases[name] = case

    for lv in CODECS:
        def f64(lv=lv):
            return _batch_codec(lv)

        def f32(lv=lv):
            return _batch_codec(lv, np.float32)
        for elem in ("f64", "f32", "u8", "u16") + KINDS:
            view = elem not in ("f64", "f32")
            for st in ((None, "cl") if view else (None,)):
                for coef in ((None, COEF) if elem not in ("u8", "u16") else (None,)):
                    add("%s/encode/%s/st=%s/coef=%s" % (lv, elem, st, bool(coef)), f32 if elem == "f32" else f64,
                        lambda c, e=elem, st=st, k=coef: _encode(c, e, cl4(B, CH, c.H, c.W, ES[e]) if st else None, k))
        for elem in ("f64", "u8", "u16") + KINDS:
            for reduce in (None, 0, 1):
                for st in ((None, "cl") if elem != "f64" else (None,)):
                    for rec in (None, REC):
                        for slot in (None, 64):
                            def run(c, e=elem, r=reduce, st=st, rec=rec, slot=slot):
                                rs = c.reduced_shape(r or 0)
                                h, w = (c.H, c.W) if r is None else (rs["pic_h"], rs["pic_w"])
                                _decode(c, e, r, cl4(B, CH, h, w, ES[e]) if st else None, rec, slot)
                            add("%s/decode/%s/reduce=%s/st=%s/rec=%s/slot=%s" % (lv, elem, reduce, st, bool(rec), slot), f64, run)

    def scaled():
        return _batch_codec("L1", scales=[1.0, 0.5, 0.25])
    add("scales/encode/u8", scaled, lambda c: _encode(c, "u8", cl4(B, CH, c.H, c.W, 1), None))
    add("scales/encode/f64", scaled, lambda c: _encode(c, "f64", None, COEF))
    add("scales/decode/float16", scaled, lambda c: _decode(c, "float16", None, cl4(B, CH, c.H, c.W, 2), None, None))
    add("scales/decode/f64/reduce=1", scaled, lambda c: _decode(c, "f64", 1, None, REC, 64))

    from spiht_amd.batch import Pipeline
    for sfx in ("u8", "u16"):
        for st_in in (None, "cl"):
            for st_out in (None, "cl"):
                def run(c, sfx=sfx, st_in=st_in, st_out=st_out):
                    pl = Pipeline.__new__(Pipeline)
                    pl.codec, pl.B, pl.handle, pl.L = c, B, C.c_void_p(0x20), c.L
                    cl = cl4(B, CH, c.H, c.W, ES[sfx])
                    getattr(pl, "submit_" + sfx)(IMG, OUT, NBITS, MAXN, PIX, cl if st_in else None, cl if st_out else None)
                    pl.handle = None  # (nothing to destroy)
                add("pipeline/submit_%s/in=%s/out=%s" % (sfx, st_in, st_out), _batch_codec, run)
    return cases


# ---- TiledCodec(3, 16, 20, 8), level=1 (an 8 x 8 tile has no default level either): the device forms ---------------------------------------------------------------------------
TH, TW_, TILE = 16, 20, 8


def _tiled_codec(overlap=0, allocate=None):
    from spiht_amd import _lib
    from spiht_amd.tiles import TiledCodec
    tc = TiledCodec(CH, TH, TW_, TILE, None, 1, 24000, ctx=StubContext(), allocate=allocate, overlap=overlap)
    tc.L = tc.codec.L = Recorder(_lib.lib())
    return tc


def _tile_dtype(elem):
    from spiht_amd import tiles
    return tiles.float_elem(elem) if elem in KINDS else np.dtype({"f64": np.float64, "u8": np.uint8, "u16": np.uint16}[elem])


def tiled_cases():
    cases = {}
    N = 2

    def add(name, make, run):
        def case():
            tc = make()
            run(tc)
            return tc.L.log
        assert name not in cases
        cases[name] = case

    out = (Dev(PACKED), Dev(LENS), Dev(MAXN))
    for overlap in (0, 2):
        for allocate in (None, "rd"):
            def make(overlap=overlap, allocate=allocate):
                return _tiled_codec(overlap, allocate)
            tag = "ov%d/%s" % (overlap, allocate)
            for elem in ("f64", "u8", "u16", "float32", "float16", "bfloat16"):
                for st in ((None, "cl") if elem != "f64" else (None,)):
                    strides = cl4(N, CH, TH, TW_, ES[elem]) if st else None

                    def run(tc, elem=elem, strides=strides):
                        if elem in KINDS:
                            tc.encode_device_float(IMG, N, *out, elem, strides)
                        else:
                            tc.encode_device(Dev(IMG, _tile_dtype(elem)), N, *out, strides)
                    add("tiled/%s/encode/%s/st=%s" % (tag, elem, st), make, run)
            if allocate == "rd":
                for elem in ("f64", "u16", "float16"):
                    add("tiled/%s/encode_layered/%s" % (tag, elem), make,
                        lambda tc, elem=elem: tc.encode_layered_device(Dev(IMG, _tile_dtype(elem)), N, 2, Dev(PACKED), Dev(CUM),
                                                                       Dev(MAXN), Dev(PICB)))
            if allocate == "rd" and not overlap:
                for elem in ("f64", "u8", "float32"):
                    add("tiled/%s/encode/%s/roi" % (tag, elem), make,
                        lambda tc, elem=elem: tc.encode_device(Dev(IMG, _tile_dtype(elem)), N, *out, None, ROI, TH * TW_))
                    add("tiled/%s/encode/%s/target" % (tag, elem), make,
                        lambda tc, elem=elem: tc.encode_device(Dev(IMG, _tile_dtype(elem)), N, *out, None, None, 0, TARGET))
                add("tiled/%s/encode_layered/u8/target_psnr" % tag, make,
                    lambda tc: tc.encode_layered_device(Dev(IMG, _tile_dtype("u8")), N, None, Dev(PACKED), Dev(CUM), Dev(MAXN),
                                                        Dev(PICB), target_psnr=[30.0, 35.0]))
        # the decodes do not depend on how the encoder shared its bits
        def make(overlap=overlap):
            return _tiled_codec(overlap)
        for elem in ("f64", "u8", "u16", "float32", "float16", "bfloat16"):
            for reduce in ((0, 1) if not overlap else (0,)):
                for st in ((None, "cl") if elem != "f64" else (None,)):
                    def whole(tc, elem=elem, reduce=reduce, st=st):
                        rs = tc.reduced_shape(reduce)
                        strides = cl3(CH, rs["Hk"], rs["Wk"], ES[elem]) if st else None
                        tc.decode_device(PACKED, 5000, LENS, MAXN, Dev(PIX, _tile_dtype(elem)), strides, None, reduce)

                    def window(tc, elem=elem, reduce=reduce, st=st):
                        y0, x0, h, w = (3, 5, 4, 3) if reduce else (5, 9, 9, 7)
                        strides = cl3(CH, h, w, ES[elem]) if st else None
                        sub = tc._window_tiles(tc.reduced_shape(reduce), y0, x0, h, w)
                        tc.decode_window_device(PACKED, 5000, LENS, MAXN, sub, (y0, x0, h, w), Dev(PIX, _tile_dtype(elem)),
                                                strides, 128, reduce)

                    def layers(tc, elem=elem, reduce=reduce, st=st):
                        rs = tc.reduced_shape(reduce)
                        strides = cl3(CH, rs["Hk"], rs["Wk"], ES[elem]) if st else None
                        tc.decode_layers_device(PACKED, 5000, CUM, MAXN, 2, 1, (0, tc.gy, 0, tc.gx), None,
                                                Dev(PIX, _tile_dtype(elem)), strides, None, SEL if st else None, reduce)
                    name = "tiled/ov%d/%%s/%s/reduce=%d/st=%s" % (overlap, elem, reduce, st)
                    add(name % "decode", make, whole)
                    add(name % "decode_window", make, window)
                    add(name % "decode_layers", make, layers)
    return cases


def all_cases():
    cases = batch_cases()
    cases.update(tiled_cases())
    return cases


def run_all():
    return {name: case() for name, case in all_cases().items()}


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "record":
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[2], "w") as f:
        json.dump(run_all(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
