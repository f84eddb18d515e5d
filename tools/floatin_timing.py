#!/usr/bin/env python3
"""Float pixels in against float64 and 16-bit pixels (profiles/floatin_timing.txt), everything in one run, the kinds in rotation
within every part:
  level 1   B (256) 1080p RGB pictures in HBM (8 distinct ones in turn): spiht_dwt_pyramid_batch_* of each kind with the pyramid
            left out -- the forward transform alone -- by the library's stage timer of level 1 (dwt_level1: the conversion happens
            inside it) and of the other levels, and the whole call by the host clock
  single    one 1080p picture at 0.5 bpp: host array to host array (encode_image*) and with the pixels in HBM (encode_device*, B = 1)
  tiled     one 4096x4096 RGB picture at 1 bpp in tiles of 256: TiledCodec.encode* host to host, plain and allocate="rd"
  sums      the per-tile error sums of that picture's tiles alone: spiht_sse_tiles_flt / _w_flt beside _f64 / _w_f64
All host-clock times are around calls that end in a synchronise of the context; medians of R timed rounds after warm-up rounds.
A build without the float names (the commit before them) is measured with the same tool: the float rows are then left out, and
its float64 and uint16 rows are what the new build's are held against.
Usage: python tools/floatin_timing.py [B] [rounds] [output file] [label] [parts]
parts: "all" (default) or "level1", the first part alone (what a second run of the parent is for: the spread)"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib, floatpx  # noqa: E402
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
HAS_FLT = hasattr(spiht_amd, "encode_image_float")
FLT = ("float32", "float16", "bfloat16") if HAS_FLT else ()
KINDS = ("float64", "uint16") + FLT
ES = {"float64": 8, "uint16": 2, "float32": 4, "float16": 2, "bfloat16": 2}
STORE = {"float64": np.float64, "uint16": np.uint16, "float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}
ctx = _lib.default_context(0)
L = _lib.lib()
s = spiht_amd.SpihtSettings()
vp = C.c_void_p


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


def of_kind(u16, kind):
    """a uint16 picture as a picture of the kind: itself, k / 65535 in float64, or that rounded to a float kind"""
    if kind == "uint16":
        return u16
    v = u16 / 65535
    return v if kind == "float64" else floatpx.convert(v, kind)


def dt_arg(kind):
    return dict(dtype="bfloat16") if kind == "bfloat16" else {}


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


lines = ["%s: float pixels in beside float64 and uint16; %dx%d RGB, bior2.2 reflect, level None; median of %d rounds after %d "
         "warm-up rounds, the kinds in rotation" % (LABEL, H, W, R, WARM), ""]

# ---- forward level 1 of B pictures ----------------------------------------------------------------------------------------
base = [synth_u16(1000 + i, H, W) for i in range(8)]
codec = BatchCodec(c, H, W, s, None, MB, ctx=ctx)
g = codec.geom
d_px = {}
for kind in KINDS:
    d = d_px[kind] = DeviceArray(ctx, (B, c, H, W), STORE[kind])
    pic = c * H * W * ES[kind]
    for b in range(min(B, 8)):
        d.upload(np.ascontiguousarray(of_kind(base[b], kind)), offset_bytes=b * pic)
    for b in range(8, B):  # (the transform's time does not depend on the samples: the 8 pictures in turn, copied on the device)
        _lib.check(L.spiht_dev_copy(ctx.handle, vp(d.ptr + b * pic), vp(d.ptr + (b % 8) * pic), pic))
    ctx.synchronize()
    note("%s: %d pictures in HBM" % (kind, B))
d_co = DeviceArray(ctx, (B, c, g["enc_h"], g["enc_w"]), np.int32)
d_mx = DeviceArray(ctx, (B,), np.uint32)


def forward(kind, n):
    tail = (n, c, H, W, codec.wid, codec.mid, -1, 50.0, None, vp(d_co.ptr), None, None, vp(d_mx.ptr))
    if kind == "float64":
        _lib.check(L.spiht_dwt_pyramid_batch_f64(ctx.handle, vp(d_px[kind].ptr), *tail))
    elif kind == "uint16":
        _lib.check(L.spiht_dwt_pyramid_batch_u16(ctx.handle, vp(d_px[kind].ptr), None, *tail))
    else:
        _lib.check(L.spiht_dwt_pyramid_batch_flt(ctx.handle, floatpx.kind_arg(kind), vp(d_px[kind].ptr), None, *tail))


st = {k: [] for k in KINDS}
for r in range(WARM + R):
    for kind in rotated(KINDS, r):
        ctx.reset_timing()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        forward(kind, B)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        ctx.set_timing(False)
        t = ctx.timing()
        if r >= WARM:
            st[kind].append((t["dwt_level1"][0], t["dwt_rest"][0], ms))
    note("level 1: round %d" % r)
if HAS_FLT:  # the transforms give the arrays of the contract (first picture)
    for kind in FLT:
        d64 = DeviceArray(ctx, (1, c, H, W), np.float64)
        d64.upload(floatpx.to_float64(of_kind(base[0], kind), kind)[None])
        _lib.check(L.spiht_dwt_pyramid_batch_f64(ctx.handle, vp(d64.ptr), 1, c, H, W, codec.wid, codec.mid, -1, 50.0, None, vp(d_co.ptr),
                                                 None, None, vp(d_mx.ptr)))
        ctx.synchronize()
        want = np.empty((c, g["enc_h"], g["enc_w"]), np.int32)
        ctx.download(want, d_co.ptr)
        d64.free()
        forward(kind, 1)
        ctx.synchronize()
        got = np.empty_like(want)
        ctx.download(got, d_co.ptr)
        assert np.array_equal(got, want), kind
lines.append("forward transform of %d pictures in HBM (stage timers; the whole call by the host clock; ms):" % B)
lines.append("  %-9s %12s %10s %12s   bytes read / picture" % ("pixels", "dwt_level1", "dwt_rest", "whole call"))
for kind in KINDS:
    a = np.array(st[kind])
    lines.append("  %-9s %12.3f %10.3f %12.2f   %5.1f MB" % ((kind,) + tuple(np.median(a, axis=0)) + (c * H * W * ES[kind] / 1e6,)))
    lines.append("            dwt_level1 runs: %s   spread %.1f %%" % (" ".join("%.3f" % x for x in a[:, 0]),
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
pics = {kind: np.ascontiguousarray(of_kind(base[0], kind)) for kind in KINDS}
host = {"float64": lambda: spiht_amd.encode_image(pics["float64"], s, max_bits=MB),
        "uint16": lambda: spiht_amd.encode_image_u16(pics["uint16"], s, max_bits=MB)}
for kind in FLT:
    host[kind] = lambda kind=kind: spiht_amd.encode_image_float(pics[kind], s, max_bits=MB, **dt_arg(kind))
d_out = DeviceArray(ctx, (1, codec.slot_stride), np.uint8)
d_nb, d_mn = DeviceArray(ctx, (1,), np.uint64), DeviceArray(ctx, (1,), np.uint8)


def encode_dev(kind):
    a = (d_px[kind].ptr, 1, d_out.ptr, d_nb.ptr, d_mn.ptr)
    if kind == "float64":
        codec.encode_device(*a)
    elif kind == "uint16":
        codec.encode_device_u16(*a)
    else:
        codec.encode_device_float(*a, kind)


one = {kind: (lambda kind=kind: encode_dev(kind)) for kind in KINDS}
th, td = timed(host, 2 * R), timed(one, 2 * R)
note("one picture: done")
lines.append("one picture at %d bits (0.5 bpp), host array to host array (encode_image*; ms):" % MB)
lines += [row(k, th[k]) for k in KINDS]
lines.append("one picture, pixels and stream in HBM (encode_device*, B = 1; ms):")
lines += [row(k, td[k]) for k in KINDS]
lines.append("")
for d in list(d_px.values()) + [d_co, d_mx, d_out, d_nb, d_mn]:
    d.free()

# ---- 4096 x 4096 in tiles of 256 --------------------------------------------------------------------------------------------
TH, TS = 4096, 256
TMB = TH * TH
u = synth_u16(7, TH, TH)
tp = {kind: np.ascontiguousarray(of_kind(u, kind)) for kind in KINDS}
for label, more in (("plain", dict()), ('allocate="rd"', dict(allocate="rd"))):
    tc = TiledCodec(c, TH, TH, TS, s, None, TMB, ctx=ctx, **more)
    fns = {"float64": lambda: tc.encode(tp["float64"]), "uint16": lambda: tc.encode_u16(tp["uint16"])}
    for kind in FLT:
        fns[kind] = lambda kind=kind: tc.encode_float(tp[kind], **dt_arg(kind))
    tt = timed(fns)
    note("tiled %s: done" % label)
    lines.append("%dx%d RGB in tiles of %d (%d tiles), %d bits (1 bpp), %s: TiledCodec.encode* host to host (ms):" % (TH, TH, TS, tc.T, TMB, label))
    lines += [row(k, tt[k]) for k in KINDS]
    if more:  # the error sums alone, on the tiles and the decodes the last call left in the codec's buffers
        K1, NT = tc.points + 1, tc.T
        rh, rw = tc.codec.geom["rec_h"], tc.codec.geom["rec_w"]
        G = max(1, min(K1, int(tc.max_bytes) // (NT * (tc.codec.slot_stride + c * rh * rw * 8 + 9))))  # (TiledCodec's group)
        geom = (G, 1, c, TH, TH, TS, TS, rh, rw)
        d_w = DeviceArray(ctx, (TH, TH), np.uint8)
        d_w.upload(np.random.default_rng(3).integers(0, 256, (TH, TH), dtype=np.uint8))
        d_D = DeviceArray(ctx, (G * NT,), np.float64)
        sums = {}
        last = FLT[-1] if FLT else "float64"  # (the tiles in the buffer are the last call's: its kind, or float64)
        tc.encode_float(tp[last], **dt_arg(last)) if FLT else tc.encode(tp["float64"])
        tiles, dec = tc._bufs["tiles"].ptr, tc._bufs["dec"].ptr
        if FLT:
            k = floatpx.kind_arg(last)
            sums["%s" % last] = lambda: _lib.check(L.spiht_sse_tiles_flt(ctx.handle, k, vp(tiles), vp(dec), *geom, vp(d_D.ptr)))
            sums["%s w" % last] = lambda: _lib.check(L.spiht_sse_tiles_w_flt(ctx.handle, k, vp(tiles), vp(dec), *geom, vp(d_D.ptr), vp(d_w.ptr), 0))
        # (the float64 kernels on the same addresses: they read 8 bytes a sample of whatever lies there -- the time of the sums
        # does not depend on the values)
        d_t64 = DeviceArray(ctx, (NT, c, TS, TS), np.float64)
        d_t64.zero()
        sums["float64"] = lambda: _lib.check(L.spiht_sse_tiles_f64(ctx.handle, vp(d_t64.ptr), vp(dec), *geom, vp(d_D.ptr)))
        sums["float64 w"] = lambda: _lib.check(L.spiht_sse_tiles_w_f64(ctx.handle, vp(d_t64.ptr), vp(dec), *geom, vp(d_D.ptr), vp(d_w.ptr), 0))
        ts = timed(sums, 2 * R)
        lines.append("the error sums alone, %d candidates x %d tiles of %d x %d x %d against float64 decodes (ms):" % (G, NT, c, TS, TS))
        lines += [row(k, ts[k]) for k in sums]
        for d in (d_w, d_D, d_t64):
            d.free()
    tc.close()
finish()
