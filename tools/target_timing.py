#!/usr/bin/env python3
"""What a target quality costs the rate allocation across tiles (profiles/target_timing.txt), everything in one run:
  pictures  the two of tools/tiled_timing.py: one 4096x4096 RGB picture, bior6.8, 1 bpp, and one 1920x1080 RGB picture,
            bior2.2, 0.5 bpp; tiles of 512, 256 and 128 at the default level of a tile; allocate="rd", points 16, spread 4
  encode    TiledCodec.encode_device, pixels and streams resident in HBM: without a target (spiht_tile_allocate), with a target
            the budget pays for (d_target: the table's total at candidate 2 of 16, about half the budget's bytes; the cut
            lies on hull vertices) and with one it cannot pay for (0: the target search, then the budget search, one launch)
  kernels   spiht_tile_allocate and spiht_tile_allocate_target alone on the table and the stream lengths that an encode of
            the picture leaves in the codec's buffers, CALLS calls queued back to back; per call
All times: the host clock (time.perf_counter) around calls that end in a synchronise of the context; medians of R timed
rounds after warm-up rounds, the forms in rotation.
Usage: python tools/target_timing.py [rounds] [output file] [label]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import DeviceArray  # noqa: E402
from spiht_amd.tiles import TiledCodec  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else None
LABEL = sys.argv[3] if len(sys.argv) > 3 else "this build"
WARM = 2
CALLS = 20
TILES = (512, 256, 128)
POINTS = 16
ctx = _lib.default_context(0)
L, vp = _lib.lib(), C.c_void_p


def synth(seed, c, H, W):
    """the picture of tools/tiled_timing.py: a smooth pattern with edges plus noise, rounded to 8 bits, float64 in [0, 1]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((c, H, W))
    for k in range(c):
        fy, fx, ph = rng.uniform(2.0, 9.0), rng.uniform(2.0, 9.0), rng.uniform(0.0, 6.28)
        v = 0.5 + 0.3 * np.sin(fy * y / H + ph) * np.cos(fx * x / W + 0.4 * k) + 0.12 * ((x + 2 * y + 31 * k) % 97 > 48)
        out[k] = np.round(np.clip(v + rng.normal(0.0, 0.004, (H, W)), 0.0, 1.0) * 255) / 255
    return out


def timed(fns):
    """fns: {name: callable} -> {name: [ms] * R}, the forms in rotation"""
    names = list(fns)
    t = {n: [] for n in names}
    for r in range(WARM + R):
        for n in names[r % len(names):] + names[:r % len(names)]:
            ctx.synchronize()
            t0 = time.perf_counter()
            fns[n]()
            ctx.synchronize()
            if r >= WARM:
                t[n].append((time.perf_counter() - t0) * 1e3)
    return t


lines = []


def say(*new):
    """a line of the report, shown as soon as it is known"""
    lines.extend(new)
    print("\n".join(new), flush=True)


def spread(v):
    return "%8.3f ms (min %.3f, max %.3f)" % (np.median(v), min(v), max(v))


say(*["%s: tiled encode with allocate=\"rd\" to a bit budget and to a target squared error under that budget, and the two"
      % LABEL, "allocation kernels alone; host clock around synchronised calls, median of %d after %d warm-up rounds, the forms in"
      % (R, WARM), "rotation; the kernels alone: %d calls queued back to back, time per call" % CALLS, ""])
for (title, c, H, W, s, bpp) in [
        ("4096x4096 RGB, bior6.8, 1 bpp", 3, 4096, 4096, spiht_amd.SpihtSettings(wavelet="bior6.8"), 1.0),
        ("1920x1080 RGB, bior2.2, 0.5 bpp", 3, 1080, 1920, spiht_amd.SpihtSettings(), 0.5)]:
    MB = int(H * W * bpp)
    P = synth(7, c, H, W)
    pictures = {np.dtype(np.float64): P[None], np.dtype(np.uint8): np.round(P[None] * 255).astype(np.uint8)}
    d_imgs = {}
    for dt, px in pictures.items():
        d_imgs[dt] = DeviceArray(ctx, px.shape, dt)
        d_imgs[dt].upload(px)
    say("== %s: %d bits = %d bytes in all ==" % (title, MB, MB // 8))
    for t in TILES:
        k = TiledCodec(c, H, W, t, s, None, MB, ctx=ctx, allocate="rd", points=POINTS)
        T = k.T
        d_packed = DeviceArray(ctx, (T * k.codec.slot_stride,), np.uint8)
        d_lens, d_maxn = DeviceArray(ctx, (T,), np.uint32), DeviceArray(ctx, (T,), np.uint8)
        d_target = DeviceArray(ctx, (2,), np.float64)
        say("tile %d (T = %d)" % (t, T))
        for dt, d_img in d_imgs.items():
            integer = dt.kind == "u"
            k.encode_device(d_img, 1, d_packed, d_lens, d_maxn)  # leaves the table "D" [K + 1][T] and "nbits" [T]
            ctx.synchronize()
            D = np.empty((POINTS + 1, T), np.uint64 if integer else np.float64)
            ctx.download(D, k._bufs["D"].ptr)
            d_target.upload(np.array([float(D[2].astype(np.float64).sum()), 0.0]))
            lens, met, dist = np.empty(T, np.uint32), np.empty(1, np.uint32), np.empty(1, np.float64)
            notes = []
            for name, off in (("paid", 0), ("unpayable", 8)):
                k.encode_device(d_img, 1, d_packed, d_lens, d_maxn, d_target=d_target.ptr + off)
                ctx.synchronize()
                for arr, ptr in ((lens, d_lens.ptr), (met, k._bufs["tmet"].ptr), (dist, k._bufs["tdist"].ptr)):
                    ctx.download(arr, ptr)
                notes.append("%s: met %d, %d bytes" % (name, met[0], int(lens.sum(dtype=np.int64))))
            tm = timed({"budget": lambda: k.encode_device(d_img, 1, d_packed, d_lens, d_maxn),
                        "paid": lambda: k.encode_device(d_img, 1, d_packed, d_lens, d_maxn, d_target=d_target.ptr),
                        "unpayable": lambda: k.encode_device(d_img, 1, d_packed, d_lens, d_maxn, d_target=d_target.ptr + 8)})
            a = np.median(tm["budget"])
            say("  %-7s encode_device   (%s)" % (dt.name, "; ".join(notes)))
            for name, text in (("budget", "to the budget"), ("paid", "to a target it pays for"),
                               ("unpayable", "to a target it cannot pay")):
                say("    %-28s %s   x%5.3f" % (text, spread(tm[name]), np.median(tm[name]) / a))
            # the kernels alone, on the table and the lengths of that encode
            args = (ctx.handle, vp(k._bufs["nbits"].ptr), vp(k._bufs["D"].ptr), 1 if integer else 0, POINTS, 1, T, MB // 8)
            cut, lam = vp(k._bufs["cut"].ptr), vp(k._bufs["lambda"].ptr)
            more = (vp(k._bufs["tdist"].ptr), vp(k._bufs["tmet"].ptr))

            def many(fn, *a):
                for _ in range(CALLS):
                    _lib.check(fn(*a))
            tk = timed({"budget": lambda: many(L.spiht_tile_allocate, *args, cut, lam),
                        "paid": lambda: many(L.spiht_tile_allocate_target, *args, vp(d_target.ptr), cut, lam, *more),
                        "unpayable": lambda: many(L.spiht_tile_allocate_target, *args, vp(d_target.ptr + 8), cut, lam, *more)})
            say("    kernels alone, per call: k_tile_allocate %.4f ms   k_tile_allocate_target %.4f ms (paid)  %.4f ms "
                "(unpayable: both searches)" % tuple(np.median(tk[n]) / CALLS for n in ("budget", "paid", "unpayable")))
        k.close()
        for d in (d_packed, d_lens, d_maxn, d_target):
            d.free()
    for d in d_imgs.values():
        d.free()
    say("")
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
