#!/usr/bin/env python3
"""Overlapping tiles (profiles/overlap_timing.txt), everything in one run, every overlap beside overlap = 0 of the same codec:
  pictures  one 4096x4096 RGB picture, bior6.8, 1 bpp, in tiles of 512 and 256 with m = 8 and 16; one 1920x1080 RGB picture,
            bior2.2, 0.5 bpp, in tiles of 128 with m = 4 and 8; the default level of a (coded) tile
  forms     encode and decode of the whole picture with picture and streams resident in HBM (encode_device,
            decode_window_device) and host to host (encode, decode); a window of 1/16 of the picture both ways; the PSNR and
            the seam step (the mean absolute jump of decoded - original across the tile boundaries) of each
  kernel    spiht_tile_blend_f64 alone beside spiht_tile_paste_f64 of the same tiles and a device-to-device copy of the bytes
            the blend writes
  expected  the coder's work grows with the tile area, (1 + 2m/th)(1 + 2m/tw), printed beside the measured ratios; the blend
            reads up to four float64 tiles per output sample in the zones and one elsewhere
All times: the host clock (time.perf_counter) around calls that end in a synchronise of the context; medians of R timed
rounds after warm-up rounds, the forms in rotation.
Usage: python tools/overlap_timing.py [rounds] [output file] [label]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import DeviceArray  # noqa: E402
from spiht_amd.overlap import window_tiles_overlap  # noqa: E402
from spiht_amd.tiles import TiledCodec  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else None
LABEL = sys.argv[3] if len(sys.argv) > 3 else "this build"
WARM = 2
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


def device(arr):
    d = DeviceArray(ctx, arr.shape, arr.dtype)
    d.upload(np.ascontiguousarray(arr))
    return d


def sub_streams(res, gx, sub):
    """the streams, lengths and start planes of the sub-grid's tiles, on the device"""
    ts = [i * gx + j for i in range(sub[0], sub[1]) for j in range(sub[2], sub[3])]
    off = res._offsets()
    run = np.frombuffer(b"".join(res.encoded_bytes[int(off[t]):int(off[t + 1])] for t in ts) or b"\0", np.uint8)
    out = [device(run), device(np.array([res.nbytes[t] for t in ts], np.uint32)), device(np.array([res.max_n[t] for t in ts], np.uint8))]
    return out + [sum(res.nbytes[t] for t in ts), max(4, (max(res.nbytes[t] for t in ts) + 3) & ~3)]


def seam_step(err, th, tw):
    H, W = err.shape[-2:]
    jumps = [np.abs(err[:, s, :] - err[:, s - 1, :]).ravel() for s in range(th, H, th)]
    jumps += [np.abs(err[:, :, s] - err[:, :, s - 1]).ravel() for s in range(tw, W, tw)]
    return float(np.concatenate(jumps).mean())


def step_elsewhere(err):
    return float(np.concatenate([np.abs(np.diff(err, axis=1)).ravel(), np.abs(np.diff(err, axis=2)).ravel()]).mean())


FORMS = ("enc HBM", "enc host", "dec HBM", "dec host", "win HBM", "win host")
lines = ["%s: overlapping tiles beside overlap = 0; host clock around synchronised calls, median of %d after %d warm-up rounds"
         % (LABEL, R, WARM), ""]

for (title, c, H, W, s, bpp, configs) in [
        ("4096x4096 RGB, bior6.8, 1 bpp", 3, 4096, 4096, spiht_amd.SpihtSettings(wavelet="bior6.8"), 1.0, ((512, (8, 16)), (256, (8, 16)))),
        ("1920x1080 RGB, bior2.2, 0.5 bpp", 3, 1080, 1920, spiht_amd.SpihtSettings(), 0.5, ((128, (4, 8)),))]:
    MB = int(H * W * bpp)
    P = synth(7, c, H, W)
    d_img = device(P)
    win = (H // 2 - 5, W // 2 - 5, H // 4, W // 4)
    lines += ["== %s: %d bits; the window: %d x %d at (%d, %d) ==" % (title, MB, win[2], win[3], win[0], win[1])]
    for t, ms_ in configs:
        lines.append("tile %d: ms" % t)
        lines.append("  %-4s %-9s " % ("m", "area") + " ".join("%9s" % f for f in FORMS) + "   PSNR dB  seam step  elsewhere  window tiles")
        fns, keep, note, codecs = {}, [], {}, {}
        for m in (0,) + tuple(ms_):
            codec = codecs[m] = TiledCodec(c, H, W, t, s, None, MB, ctx=ctx, overlap=m)
            res = codec.encode(P)
            NT = codec.T
            d_packed = DeviceArray(ctx, (NT * codec.codec.slot_stride,), np.uint8)
            d_lens, d_maxn = DeviceArray(ctx, (NT,), np.uint32), DeviceArray(ctx, (NT,), np.uint8)
            d_out, d_win = DeviceArray(ctx, (c, H, W), np.float64), DeviceArray(ctx, (c, win[2], win[3]), np.float64)
            sub = window_tiles_overlap(H, W, t, t, m, *win)
            whole, part = sub_streams(res, codec.gx, (0, codec.gy, 0, codec.gx)), sub_streams(res, codec.gx, sub)
            keep += [d_packed, d_lens, d_maxn, d_out, d_win] + whole[:3] + part[:3]
            fns[(m, "enc HBM")] = lambda cd=codec, a=d_packed, b=d_lens, e=d_maxn: cd.encode_device(d_img, 1, a, b, e)
            fns[(m, "enc host")] = lambda cd=codec: cd.encode(P)
            fns[(m, "dec HBM")] = lambda cd=codec, w=whole, o=d_out: cd.decode_window_device(
                w[0], w[3], w[1], w[2], (0, cd.gy, 0, cd.gx), None, o, slot_stride=w[4])
            fns[(m, "dec host")] = lambda cd=codec, r=res: cd.decode(r)
            fns[(m, "win HBM")] = lambda cd=codec, p=part, o=d_win, sub=sub: cd.decode_window_device(
                p[0], p[3], p[1], p[2], sub, win, o, slot_stride=p[4])
            fns[(m, "win host")] = lambda cd=codec, r=res: cd.decode_window(r, *win)
            dec = codec.decode(res)
            assert np.array_equal(codec.decode_window(res, *win), dec[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
            err = np.asarray(dec) - P
            note[m] = (10 * np.log10(1.0 / float((err ** 2).mean())), seam_step(err, t, t), step_elsewhere(err),
                       (sub[1] - sub[0]) * (sub[3] - sub[2]))
        tm = timed(fns)
        for m in (0,) + tuple(ms_):
            area = (1 + 2 * m / t) ** 2
            lines.append("  %-4d x%-8.3f " % (m, area) + " ".join("%9.2f" % tm[(m, f)] for f in FORMS)
                         + "   %7.3f  %9.5f  %9.5f  %6d" % note[m])
            if m:
                lines.append("  %-4s %-9s " % ("", "ratio") + " ".join("%9.3f" % (tm[(m, f)] / tm[(0, f)]) for f in FORMS))
        for d in keep:
            d.free()
        # ---- the blend alone, beside the paste of the same tiles and a copy of the bytes it writes
        lines.append("  the blend alone (ms per call of 20 queued back to back; GB/s = bytes written + as many read / time):")
        nbytes = c * H * W * 8
        d_win, d_copy = DeviceArray(ctx, (nbytes,), np.uint8), DeviceArray(ctx, (nbytes,), np.uint8)
        for m in ms_:
            codec = codecs[m]
            rh, rw = codec.codec.geom["rec_h"], codec.codec.geom["rec_w"]
            d_tiles = DeviceArray(ctx, (codec.T * c * rh * rw * 8,), np.uint8)
            ctx.memset(d_tiles.ptr, 0, d_tiles.nbytes)
            grid = (0, codec.gy, 0, codec.gx, 0, 0, H, W)
            for name, fn in (("blend float64, m = %d (tiles of %dx%d)" % (m, rh, rw),
                              lambda: _lib.check(L.spiht_tile_blend_f64(ctx.handle, vp(d_tiles.ptr), c, rh, rw, H, W, t, t, m, *grid, vp(d_win.ptr)))),
                             ("paste float64 of the same tiles (their corner)",
                              lambda: _lib.check(L.spiht_tile_paste_f64(ctx.handle, vp(d_tiles.ptr), c, rh, rw, H, W, t, t, *grid, vp(d_win.ptr))))):
                v = launches(fn)
                lines.append("    %-52s %8.4f ms  %8.1f GB/s" % (name, v, 2 * nbytes / v / 1e6))
            d_tiles.free()
        v = launches(lambda: _lib.check(L.spiht_dev_copy(ctx.handle, vp(d_copy.ptr), vp(d_win.ptr), nbytes)))
        lines.append("    %-52s %8.4f ms  %8.1f GB/s" % ("device-to-device copy of %d bytes" % nbytes, v, 2 * nbytes / v / 1e6))
        d_win.free()
        d_copy.free()
        for codec in codecs.values():
            codec.close()
        print("%s, tile %d: done" % (title, t), file=sys.stderr, flush=True)
    d_img.free()
    lines.append("")

print("\n".join(lines))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
