#!/usr/bin/env python3
"""Float pixels out against float64, 8-bit and 16-bit pixels (profiles/floatpx_timing.txt), everything in one run, the kinds in
rotation within every part:
  level 1   B (256) distinct 1080p RGB pictures at 0.5 bpp, streams resident in HBM: BatchCodec.decode_device* of each kind, the
            library's stage timer of level 1 of the inverse transform (idwt_level1: the conversion happens inside it) and of the
            other levels, and the whole decode by the host clock
  single    one 1080p picture: host array to host array (decode_image*) and with stream and picture in HBM (decode_device*, B = 1)
  tiled     one 4096x4096 RGB picture at 0.5 bpp in tiles of 256: TiledCodec.decode* host to host and decode_window_device in HBM
All host-clock times are around calls that end in a synchronise of the context; medians of R timed rounds after warm-up rounds.
A build without the float names (the commit before them) is measured with the same tool: the float rows are then left out, and
its float64, uint8 and uint16 rows are what the new build's are held against.
Usage: python tools/floatpx_timing.py [B] [rounds] [output file] [label] [parts]
parts: "all" (default) or "level1", the first part alone (what a second run of the parent is for: the spread)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import BatchCodec, DeviceArray  # noqa: E402
from spiht_amd.tiles import TiledCodec  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else None
LABEL = sys.argv[4] if len(sys.argv) > 4 else "this build"
PARTS = sys.argv[5] if len(sys.argv) > 5 else "all"
WARM = 2
c, H, W = 3, 1080, 1920
MB = int(H * W * 0.5)
HAS_FLT = hasattr(spiht_amd, "decode_image_float")
FLT = ("float32", "float16", "bfloat16") if HAS_FLT else ()
KINDS = ("float64", "uint8", "uint16") + FLT
ES = {"float64": 8, "uint8": 1, "uint16": 2, "float32": 4, "float16": 2, "bfloat16": 2}
ctx = _lib.default_context(0)
s = spiht_amd.SpihtSettings()


def synth_u16(seed, h, w):
    """a smooth pattern with edges plus noise, rounded to uint16 (tools/u16_timing.py)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((c, h, w), np.uint16)
    for k in range(c):
        fy, fx, ph = rng.uniform(2.0, 9.0), rng.uniform(2.0, 9.0), rng.uniform(0.0, 6.28)
        v = 0.5 + 0.3 * np.sin(fy * y / h + ph) * np.cos(fx * x / w + 0.4 * k) + 0.12 * ((x + 2 * y + 31 * k) % 97 > 48)
        out[k] = np.round(np.clip(v + rng.normal(0.0, 0.004, (h, w)), 0.0, 1.0) * 65535)
    return out


def note(text):
    print(text, file=sys.stderr, flush=True)


def rotated(names, r):
    names = list(names)
    return names[r % len(names):] + names[:r % len(names)]


def timed(fns, rounds=R):
    """{name: callable} -> {name: [ms per timed round]}, in rotation, a synchronise before and after each call"""
    t = {n: [] for n in fns}
    for r in range(WARM + rounds):
        for n in rotated(fns, r):
            ctx.synchronize()
            t0 = time.perf_counter()
            fns[n]()
            ctx.synchronize()
            if r >= WARM:
                t[n].append((time.perf_counter() - t0) * 1e3)
    return t


def row(name, xs):
    return "  %-9s median %8.3f   min %8.3f  max %8.3f   spread %4.1f %%" % (name, np.median(xs), min(xs), max(xs),
                                                                             100.0 * (max(xs) - min(xs)) / np.median(xs))


def decode_dev(codec, kind, streams, n, d_out, stride=None):
    if kind == "float64":
        codec.decode_device(*streams, n, d_out.ptr, slot_stride=stride)
    elif kind in FLT:
        codec.decode_device_float(*streams, n, d_out.ptr, kind, slot_stride=stride)
    else:
        getattr(codec, "decode_device_u8" if kind == "uint8" else "decode_device_u16")(*streams, n, d_out.ptr, slot_stride=stride)


lines = ["%s: float pixels out beside float64, uint8 and uint16; %dx%d RGB, bior2.2 reflect, level None, %d bits (0.5 bpp); median of %d "
         "rounds after %d warm-up rounds, the kinds in rotation" % (LABEL, H, W, MB, R, WARM), ""]

# ---- level 1 of B pictures ----------------------------------------------------------------------------------------------
base = [synth_u16(1000 + i, H, W) for i in range(8)]
codec = BatchCodec(c, H, W, s, None, MB, ctx=ctx)
g = codec.geom
d_px = DeviceArray(ctx, (B, c, H, W), np.uint16)
for b in range(B):  # B distinct pictures: 8 generated ones, shifted and mirrored
    v = np.roll(base[b % 8], 7 * (b // 8), axis=2)
    d_px.upload(v[:, ::-1, :] if (b // 8) & 1 else v, offset_bytes=b * c * H * W * 2)
d_out = DeviceArray(ctx, (B, codec.slot_stride), np.uint8)
d_nb, d_ny, d_mn = DeviceArray(ctx, (B,), np.uint64), DeviceArray(ctx, (B,), np.uint64), DeviceArray(ctx, (B,), np.uint8)
codec.encode_device_u16(d_px.ptr, B, d_out.ptr, d_nb.ptr, d_mn.ptr)
codec.nbits_to_nbytes(d_nb.ptr, B, d_ny.ptr)
ctx.synchronize()
d_px.free()
note("%d pictures encoded" % B)
streams = (d_out.ptr, d_ny.ptr, d_mn.ptr)
d_rec = DeviceArray(ctx, (B, c, g["rec_h"], g["rec_w"]), np.float64)  # (every kind decodes into the one buffer)
st = {k: [] for k in KINDS}
for r in range(WARM + R):
    for kind in rotated(KINDS, r):
        ctx.reset_timing()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        decode_dev(codec, kind, streams, B, d_rec)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        ctx.set_timing(False)
        t = ctx.timing()
        if r >= WARM:
            st[kind].append((t["idwt_level1"][0], t["idwt_rest"][0], ms))
    note("level 1: round %d" % r)
if HAS_FLT:  # the decodes give the pictures of the contract (first picture)
    from spiht_amd import floatpx
    decode_dev(codec, "float64", streams, 1, d_rec)
    ctx.synchronize()
    f = np.empty((c, g["rec_h"], g["rec_w"]), np.float64)
    ctx.download(f, d_rec.ptr)
    for kind in FLT:
        decode_dev(codec, kind, streams, 1, d_rec)
        ctx.synchronize()
        u = np.empty((c, H, W), floatpx.storage_dtype(kind))
        ctx.download(u, d_rec.ptr)
        assert u.tobytes() == floatpx.convert(f[:, :H, :W], kind).tobytes(), kind
lines.append("inverse transform of %d pictures, streams and pictures in HBM (stage timers; whole decode by the host clock; ms):" % B)
lines.append("  %-9s %12s %10s %12s   bytes stored / picture" % ("pixels", "idwt_level1", "idwt_rest", "whole decode"))
for kind in KINDS:
    a = np.array(st[kind])
    lines.append("  %-9s %12.3f %10.3f %12.2f   %5.1f MB" % ((kind,) + tuple(np.median(a, axis=0)) + (
        c * (g["rec_h"] * g["rec_w"] if kind == "float64" else H * W) * ES[kind] / 1e6,)))
    lines.append("            idwt_level1 runs: %s   spread %.1f %%" % (" ".join("%.3f" % x for x in a[:, 0]),
                                                                        100.0 * (a[:, 0].max() - a[:, 0].min()) / np.median(a[:, 0])))
lines.append("")


def finish():
    print("\n".join(lines))
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if PARTS == "level1":
    finish()
    sys.exit(0)

# ---- one picture ----------------------------------------------------------------------------------------------------------
img = base[0] / 65535
enc = spiht_amd.encode_image(img, s, max_bits=MB)
host = {"float64": lambda: spiht_amd.decode_image(enc, s), "uint8": lambda: spiht_amd.decode_image_u8(enc, s),
        "uint16": lambda: spiht_amd.decode_image_u16(enc, s)}
for kind in FLT:
    host[kind] = lambda kind=kind: spiht_amd.decode_image_float(enc, s, dtype=kind)
one = {kind: (lambda kind=kind: decode_dev(codec, kind, streams, 1, d_rec)) for kind in KINDS}
th, td = timed(host, 2 * R), timed(one, 2 * R)
note("one picture: done")
lines.append("one picture, host array to host array (decode_image*; ms):")
lines += [row(k, th[k]) for k in KINDS]
lines.append("one picture, stream and picture in HBM (decode_device*, B = 1; ms):")
lines += [row(k, td[k]) for k in KINDS]
lines.append("")
for d in (d_out, d_nb, d_ny, d_mn, d_rec):
    d.free()

# ---- 4096 x 4096 in tiles of 256 --------------------------------------------------------------------------------------------
TH, TS = 4096, 256
TMB = int(TH * TH * 0.5)
P = synth_u16(7, TH, TH) / 65535
tc = TiledCodec(c, TH, TH, TS, s, None, TMB, ctx=ctx)
res = tc.encode(P)
note("tiled picture encoded")
TK = tuple(k for k in KINDS if k != "uint16")
hostt = {"float64": lambda: tc.decode(res), "uint8": lambda: tc.decode_u8(res)}
for kind in FLT:
    hostt[kind] = lambda kind=kind: tc.decode_float(res, dtype=kind)
run = np.frombuffer(res.encoded_bytes, np.uint8)
d_run, d_lens, d_maxn = DeviceArray(ctx, run.shape, np.uint8), DeviceArray(ctx, (tc.T,), np.uint32), DeviceArray(ctx, (tc.T,), np.uint8)
d_run.upload(run)
d_lens.upload(np.asarray(res.nbytes, np.uint32))
d_maxn.upload(np.asarray(res.max_n, np.uint8))
stride = max(4, (max(res.nbytes) + 3) & ~3)
d_pic = DeviceArray(ctx, (c, TH, TH), np.float64)


class View:
    def __init__(self, kind):
        from spiht_amd import tiles
        self.ptr = d_pic.ptr
        self.dtype = tiles.float_elem(kind) if kind in FLT else np.dtype(kind)


dev = {kind: (lambda v=View(kind): tc.decode_window_device(d_run, run.size, d_lens, d_maxn, (0, tc.gy, 0, tc.gx), None, v,
                                                            slot_stride=stride)) for kind in TK}
tht, tdt = timed(hostt), timed(dev)
lines.append("%dx%d RGB in tiles of %d (%d tiles), %d bits: TiledCodec.decode* host to host (ms):" % (TH, TH, TS, tc.T, TMB))
lines += [row(k, tht[k]) for k in TK]
lines.append("... streams and picture in HBM (decode_window_device of the whole picture; ms):")
lines += [row(k, tdt[k]) for k in TK]
finish()
