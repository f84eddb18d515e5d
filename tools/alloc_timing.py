#!/usr/bin/env python3
"""Rate allocation across tiles against the equal split (profiles/alloc_timing.txt), everything in one run:
  pictures  the two of tools/tiled_timing.py: one 4096x4096 RGB picture, bior6.8, 1 bpp, and one 1920x1080 RGB picture,
            bior2.2, 0.5 bpp; tiles of 512, 256 and 128 at the default level of a tile
  encode    TiledCodec.encode_device, pixels and streams resident in HBM, with allocate=None and with allocate="rd" at
            points 8 / 16 / 32 (spread 4) and spread 2 / 4 / 8 (points 16)
  psnr      of the decode of each against the picture, with the bytes each one spent of the same budget
All times: the host clock (time.perf_counter) around calls that end in a synchronise of the context; medians of R timed
rounds after warm-up rounds, the forms in rotation.
Usage: python tools/alloc_timing.py [rounds] [output file] [label]"""
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
TILES = (512, 256, 128)
FORMS = [("equal split", None, 16, 4.0), ("rd, points 16, spread 4", "rd", 16, 4.0), ("rd, points  8, spread 4", "rd", 8, 4.0),
         ("rd, points 32, spread 4", "rd", 32, 4.0), ("rd, points 16, spread 2", "rd", 16, 2.0), ("rd, points 16, spread 8", "rd", 16, 8.0)]
ctx = _lib.default_context(0)


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


def psnr(a, b):
    return 10.0 * np.log10(1.0 / float(((a - b) ** 2).mean()))


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


say(*["%s: tiled encode with the budget shared by rate-distortion curves against the equal split; host clock around"
         % LABEL, "synchronised calls, median of %d after %d warm-up rounds, the forms in rotation" % (R, WARM), ""])
for (title, c, H, W, s, bpp) in [
        ("4096x4096 RGB, bior6.8, 1 bpp", 3, 4096, 4096, spiht_amd.SpihtSettings(wavelet="bior6.8"), 1.0),
        ("1920x1080 RGB, bior2.2, 0.5 bpp", 3, 1080, 1920, spiht_amd.SpihtSettings(), 0.5)]:
    MB = int(H * W * bpp)
    P = synth(7, c, H, W)
    d_img = DeviceArray(ctx, (1, c, H, W), np.float64)
    d_img.upload(P[None])
    say("== %s: %d bits = %d bytes in all ==" % (title, MB, MB // 8))
    for t in TILES:
        codecs = {name: TiledCodec(c, H, W, t, s, None, MB, ctx=ctx, allocate=a, points=p, spread=sp) for name, a, p, sp in FORMS}
        T = codecs["equal split"].T
        stride = max(k.codec.slot_stride for k in codecs.values())
        d_packed = DeviceArray(ctx, (T * stride,), np.uint8)
        d_lens, d_maxn = DeviceArray(ctx, (T,), np.uint32), DeviceArray(ctx, (T,), np.uint8)
        tm = timed({name: (lambda k=k: k.encode_device(d_img, 1, d_packed, d_lens, d_maxn)) for name, k in codecs.items()})
        say("tile %d (T = %d): encode_device (ms), then PSNR of the decode (dB) and the bytes spent" % (t, T))
        base = np.median(tm["equal split"])
        for name, k in codecs.items():
            res = k.encode(P)
            lam = "" if k.allocate is None else ", lambda* %.3g" % k.last_allocation.lam
            say("  %-26s %8.2f  (min %.2f, max %.2f)  x%5.2f   %6.2f dB  %8d bytes%s"
                         % (name, np.median(tm[name]), min(tm[name]), max(tm[name]), np.median(tm[name]) / base,
                            psnr(P, k.decode(res)), len(res.encoded_bytes), lam))
            k.close()
        for d in (d_packed, d_lens, d_maxn):
            d.free()
    d_img.free()
    say("")
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
