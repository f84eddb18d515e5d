#!/usr/bin/env python3
"""What a weight map costs the rate allocation across tiles (profiles/roi_timing.txt), everything in one run:
  pictures  the two of tools/tiled_timing.py: one 4096x4096 RGB picture, bior6.8, 1 bpp, and one 1920x1080 RGB picture,
            bior2.2, 0.5 bpp; tiles of 512, 256 and 128 at the default level of a tile; allocate="rd", points 16, spread 4
  encode    TiledCodec.encode_device, pixels, map and streams resident in HBM, without a map and with one (weight 255 in
            the centred box of half the picture's sides, 1 outside)
  kernels   spiht_sse_tiles_w_f64 / _u8 / _u16 alone beside spiht_sse_tiles_f64 / _u8 / _u16 on the same operands -- the
            cut tiles and the last group of decodes that an encode of the picture leaves in the codec's buffers -- CALLS
            calls queued back to back; per call: the time, and over it the bytes of the picture's tiles, of their G decodes
            and of the map, each counted once (the tiles are read by every candidate, the map by every candidate and channel)
All times: the host clock (time.perf_counter) around calls that end in a synchronise of the context; medians of R timed
rounds after warm-up rounds, the forms in rotation.
Usage: python tools/roi_timing.py [rounds] [output file] [label]"""
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


def kernels_alone(k, dt, d_roi, c, H, W):
    """the weighted and the unweighted error sums on the tiles and the last group of decodes the codec's buffers hold"""
    dt = np.dtype(dt)
    kind = {1: "u8", 2: "u16", 8: "f64"}[dt.itemsize]
    rh, rw = (k.th, k.tw) if dt.kind == "u" else (k.codec.geom["rec_h"], k.codec.geom["rec_w"])
    # the group of _measure_device: "dec" holds that many decodes of every tile (of the last groups measured)
    G = max(1, min(POINTS + 1, int(k.max_bytes) // (k.T * (k.codec.slot_stride + c * rh * rw * dt.itemsize + 9))))
    args = (ctx.handle, vp(k._bufs["tiles"].ptr), vp(k._bufs["dec"].ptr), G, 1, c, H, W, k.th, k.tw, rh, rw, vp(k._bufs["D"].ptr))
    plain, weighted = getattr(L, "spiht_sse_tiles_" + kind), getattr(L, "spiht_sse_tiles_w_" + kind)

    def many(fn, *more):
        for _ in range(CALLS):
            _lib.check(fn(*args, *more))
    tm = timed({"plain": lambda: many(plain), "weighted": lambda: many(weighted, vp(d_roi.ptr), 0)})
    a, b = np.median(tm["plain"]) / CALLS, np.median(tm["weighted"]) / CALLS
    operands, side = (G + 1) * c * H * W * dt.itemsize, H * W  # the G decodes and the tiles, which all G candidates share
    say("    sse %-3s G = %2d: plain %7.3f ms (%6.0f GB/s)   weighted %7.3f ms (%6.0f GB/s with the map's %.1f MB)   x%5.3f"
        % (kind, G, a, operands / a / 1e6, b, (operands + side) / b / 1e6, side / 1e6, b / a))


say(*["%s: tiled encode with allocate=\"rd\", with and without a weight map, and the weighted error sums beside the unweighted"
      % LABEL, "ones; host clock around synchronised calls, median of %d after %d warm-up rounds, the forms in rotation; the kernels"
      % (R, WARM), "alone: %d calls queued back to back, time per call" % CALLS, ""])
for (title, c, H, W, s, bpp) in [
        ("4096x4096 RGB, bior6.8, 1 bpp", 3, 4096, 4096, spiht_amd.SpihtSettings(wavelet="bior6.8"), 1.0),
        ("1920x1080 RGB, bior2.2, 0.5 bpp", 3, 1080, 1920, spiht_amd.SpihtSettings(), 0.5)]:
    MB = int(H * W * bpp)
    P = synth(7, c, H, W)
    roi = spiht_amd.roi_map(H, W, [(H // 4, W // 4, H // 2, W // 2)])
    pictures = {np.dtype(np.float64): P[None], np.dtype(np.uint8): np.round(P[None] * 255).astype(np.uint8),
                np.dtype(np.uint16): np.round(P[None] * 65535).astype(np.uint16)}
    d_imgs = {}
    for dt, px in pictures.items():
        d_imgs[dt] = DeviceArray(ctx, px.shape, dt)
        d_imgs[dt].upload(px)
    d_roi = DeviceArray(ctx, roi.shape, np.uint8)
    d_roi.upload(roi)
    say("== %s: %d bits = %d bytes in all ==" % (title, MB, MB // 8))
    for t in TILES:
        k = TiledCodec(c, H, W, t, s, None, MB, ctx=ctx, allocate="rd", points=POINTS)
        T = k.T
        d_packed = DeviceArray(ctx, (T * k.codec.slot_stride,), np.uint8)
        d_lens, d_maxn = DeviceArray(ctx, (T,), np.uint32), DeviceArray(ctx, (T,), np.uint8)
        say("tile %d (T = %d)" % (t, T))
        for dt, d_img in d_imgs.items():
            tm = timed({"no map": lambda: k.encode_device(d_img, 1, d_packed, d_lens, d_maxn),
                        "map": lambda: k.encode_device(d_img, 1, d_packed, d_lens, d_maxn, d_roi=d_roi, roi_stride=0)})
            a, b = np.median(tm["no map"]), np.median(tm["map"])
            say("  %-7s encode_device: no map %8.2f ms (min %.2f, max %.2f)   map %8.2f ms (min %.2f, max %.2f)   x%5.3f"
                % (dt.name, a, min(tm["no map"]), max(tm["no map"]), b, min(tm["map"]), max(tm["map"]), b / a))
            kernels_alone(k, dt, d_roi, c, H, W)
        k.close()
        for d in (d_packed, d_lens, d_maxn):
            d.free()
    for d in list(d_imgs.values()) + [d_roi]:
        d.free()
    say("")
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
