#!/usr/bin/env python3
"""Tiled pictures at reduced resolution (profiles/tiled_reduced_timing.txt), everything in one run:
  pictures  those of tools/tiled_timing.py: one 4096x4096 RGB picture, bior6.8, 1 bpp, and one 1920x1080 RGB picture, bior2.2,
            0.5 bpp, in tiles of 512, 256 and 128 at the default level of a tile
  forms     for reduce = 0 .. 3, float64 and uint8: the whole picture and a window of 1/16 of the area (Hk/4 x Wk/4 of the
            reduced picture), each with streams and picture resident in HBM (decode_window_device) and from a host result to a
            host array (decode* / decode_window*); beside them the untiled decode_image_reduced of the same picture
  kernel    spiht_tile_mosaic_* alone at reduce 0 and 3 (the deepest the tile has, if that is less) beside spiht_tile_paste_*
            (where it can run: sides >= 8, no origin) and a device-to-device copy of the bytes the mosaic writes
All times: the host clock (time.perf_counter) around calls that end in a synchronise of the context; medians of R timed
rounds after warm-up rounds, the forms in rotation.
Usage: python tools/tiled_reduced_timing.py [rounds] [output file] [label]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import DeviceArray  # noqa: E402
from spiht_amd.tiles import TiledCodec, window_tiles  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else None
LABEL = sys.argv[3] if len(sys.argv) > 3 else "this build"
WARM = 2
TILES = (512, 256, 128)
KS = (0, 1, 2, 3)
ctx = _lib.default_context(0)
L = _lib.lib()
vp = C.c_void_p


def synth(seed, c, H, W):
    """the pattern of tools/tiled_timing.py: smooth with edges plus noise, rounded to 8 bits, float64 in [0, 1]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((c, H, W))
    for k in range(c):
        fy, fx, ph = rng.uniform(2.0, 9.0), rng.uniform(2.0, 9.0), rng.uniform(0.0, 6.28)
        v = 0.5 + 0.3 * np.sin(fy * y / H + ph) * np.cos(fx * x / W + 0.4 * k) + 0.12 * ((x + 2 * y + 31 * k) % 97 > 48)
        out[k] = np.round(np.clip(v + rng.normal(0.0, 0.004, (H, W)), 0.0, 1.0) * 255) / 255
    return out


def timed(fns):
    """fns: {name: callable} -> {name: median ms}, the forms in rotation, a synchronise before and after each"""
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
    return {n: float(np.median(v)) for n, v in t.items()}


def launches(fn, n=20):
    """ms per call of n calls queued back to back"""
    fn()
    ctx.synchronize()
    best = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        ctx.synchronize()
        best.append((time.perf_counter() - t0) * 1e3 / n)
    return float(np.median(best))


def sub_streams(res, gx, sub):
    """the streams, lengths and start planes of the sub-grid's tiles, on the device"""
    ts = [i * gx + j for i in range(sub[0], sub[1]) for j in range(sub[2], sub[3])]
    off = res._offsets()
    run = np.frombuffer(b"".join(res.encoded_bytes[int(off[t]):int(off[t + 1])] for t in ts) or b"\0", np.uint8)
    out = []
    for arr in (run, np.array([res.nbytes[t] for t in ts], np.uint32), np.array([res.max_n[t] for t in ts], np.uint8)):
        d = DeviceArray(ctx, arr.shape, arr.dtype)
        d.upload(np.ascontiguousarray(arr))
        out.append(d)
    return out + [sum(res.nbytes[t] for t in ts), max(4, (max(res.nbytes[t] for t in ts) + 3) & ~3)]


lines = ["%s: tiled pictures at reduced resolution; host clock around synchronised calls, median of %d after %d warm-up rounds"
         % (LABEL, R, WARM), ""]

for (title, c, H, W, s, level, bpp) in [
        ("4096x4096 RGB, bior6.8, 1 bpp", 3, 4096, 4096, spiht_amd.SpihtSettings(wavelet="bior6.8"), 9, 1.0),
        ("1920x1080 RGB, bior2.2, 0.5 bpp", 3, 1080, 1920, spiht_amd.SpihtSettings(), 7, 0.5)]:
    MB = int(H * W * bpp)
    P = synth(7, c, H, W)
    lines += ["== %s: %d bits ==" % (title, MB)]
    enc0 = spiht_amd.encode_image(P, s, level, MB)
    tm = timed({k: (lambda k=k: spiht_amd.decode_image_reduced(enc0, s, k)) for k in KS})
    lines.append("untiled decode_image_reduced, host result to host array (ms): " + ", ".join("k = %d: %.2f" % (k, tm[k]) for k in KS))
    for t in TILES:
        codec = TiledCodec(c, H, W, t, s, None, MB, ctx=ctx)
        res = codec.encode(P)
        ks = [k for k in KS if k <= codec.reduced_shape(0)["level"]]  # (a 128-tile under bior6.8 has two levels)
        lines.append("tile %d (T = %d, level %d): ms, float64 / uint8" % (t, codec.T, codec.reduced_shape(0)["level"]))
        lines.append("  %-3s %-11s %-9s %17s %17s %17s %17s" % ("k", "picture", "tile", "whole, HBM", "whole, host", "window, HBM", "window, host"))
        fns, keep, note = {}, [], {}
        for k in ks:
            rs = codec.reduced_shape(k)
            Hk, Wk = rs["Hk"], rs["Wk"]
            win = (Hk // 2 - 5, Wk // 2 - 5, Hk // 4, Wk // 4)
            sub = window_tiles(Hk, Wk, rs["thk"], rs["twk"], *win)
            whole = sub_streams(res, codec.gx, (0, codec.gy, 0, codec.gx))
            part = sub_streams(res, codec.gx, sub)
            note[k] = (rs, (sub[1] - sub[0]) * (sub[3] - sub[2]))
            keep += whole[:3] + part[:3]
            for dt, u in ((np.float64, ""), (np.uint8, "_u8")):
                d_out = DeviceArray(ctx, (c, Hk, Wk), dt)
                keep.append(d_out)
                fns[(k, u, "wd")] = (lambda k=k, w=whole, o=d_out: codec.decode_window_device(
                    w[0], w[3], w[1], w[2], (0, codec.gy, 0, codec.gx), None, o, slot_stride=w[4], reduce=k))
                fns[(k, u, "wh")] = (lambda k=k, u=u: getattr(codec, "decode" + u)(res, reduce=k))
                fns[(k, u, "pd")] = (lambda k=k, p=part, o=d_out, sub=sub, win=win: codec.decode_window_device(
                    p[0], p[3], p[1], p[2], sub, win, o, slot_stride=p[4], reduce=k))
                fns[(k, u, "ph")] = (lambda k=k, u=u, win=win: getattr(codec, "decode_window" + u)(res, *win, reduce=k))
            # the window is the slice of the whole picture: checked here on one form, all of them in the tests
            assert np.array_equal(codec.decode_window_u8(res, *win, reduce=k),
                                  codec.decode_u8(res, reduce=k)[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
        tm = timed(fns)
        for k in ks:
            rs, n = note[k]
            lines.append("  %-3d %-11s %-9s " % (k, "%dx%d" % (rs["Hk"], rs["Wk"]), "%dx%d" % (rs["thk"], rs["twk"]))
                         + " ".join("%8.2f/%8.2f" % (tm[(k, "", f)], tm[(k, "_u8", f)]) for f in ("wd", "wh", "pd", "ph"))
                         + "   (the window: %d tiles)" % n)
        for d in keep:
            d.free()
        # ---- the kernel alone: reduce 0 and 3
        if H == 4096 and t in (512, 128):
            lines.append("  the mosaic alone, tile %d (ms per call of 20 queued back to back; GB/s = bytes read + written / time):" % t)
            for k in (0, ks[-1]):
                rs = codec.reduced_shape(k)
                Hk, Wk, thk, twk, oy, ox = rs["Hk"], rs["Wk"], rs["thk"], rs["twk"], rs["off_y"], rs["off_x"]
                for name, es, rh, rw, mosaic, paste in (("float64", 8, rs["rec_h"], rs["rec_w"], L.spiht_tile_mosaic_f64, L.spiht_tile_paste_f64),
                                                        ("uint8", 1, rs["pic_h"], rs["pic_w"], L.spiht_tile_mosaic_u8, L.spiht_tile_paste_u8)):
                    nbytes = c * Hk * Wk * es
                    d_tiles = DeviceArray(ctx, (codec.T * c * rh * rw * es,), np.uint8)
                    d_win, d_copy = DeviceArray(ctx, (nbytes,), np.uint8), DeviceArray(ctx, (nbytes,), np.uint8)
                    st = (None,) if es == 1 else ()
                    grid = (Hk, Wk, thk, twk, 0, codec.gy, 0, codec.gx, 0, 0, Hk, Wk)
                    ms = launches(lambda: _lib.check(mosaic(ctx.handle, vp(d_tiles.ptr), c, rh, rw, oy, ox, *grid, vp(d_win.ptr), *st)))
                    lines.append("    %-52s %8.4f ms  %8.1f GB/s" % ("mosaic %s, k = %d (tile %dx%d of %dx%d at %d, %d)"
                                                                    % (name, k, thk, twk, rh, rw, oy, ox), ms, 2 * nbytes / ms / 1e6))
                    if thk >= 8:
                        ms = launches(lambda: _lib.check(paste(ctx.handle, vp(d_tiles.ptr), c, rh, rw, *grid, vp(d_win.ptr), *st)))
                        lines.append("    %-52s %8.4f ms  %8.1f GB/s" % ("paste  %s of the same tiles (no origin)" % name, ms, 2 * nbytes / ms / 1e6))
                    ms = launches(lambda: _lib.check(L.spiht_dev_copy(ctx.handle, vp(d_copy.ptr), vp(d_win.ptr), nbytes)))
                    lines.append("    %-52s %8.4f ms  %8.1f GB/s" % ("device-to-device copy of %d bytes" % nbytes, ms, 2 * nbytes / ms / 1e6))
                    for d in (d_tiles, d_win, d_copy):
                        d.free()
        codec.close()
    lines.append("")

print("\n".join(lines))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
