#!/usr/bin/env python3
"""Tiled pictures against the untiled calls (profiles/tiled_timing.txt), everything in one run:
  pictures  one 4096x4096 RGB picture, bior6.8, 1 bpp (cfg5 of tools/other_configs.py; untiled at level 9) and one
            1920x1080 RGB picture, bior2.2, 0.5 bpp (cfg2; untiled at level 7); tiles of 512, 256 and 128 at the default level
            of a tile, every tile with max_bits // T bits
  host      encode / decode from a host array to a host array: encode_image / decode_image against TiledCodec.encode / .decode
  device    the same with pixels, streams and pictures resident in HBM: BatchCodec.*_device (B = 1) against
            TiledCodec.*_device
  window    a 1/16-area window (H/4 x W/4) from a host result to a host array
  psnr      of each decode against the picture, at the same total bit budget
  kernels   cut, paste, pack, unpack on their own: bytes read + written over time, beside a device-to-device copy of the
            picture (spiht_dev_copy) and, when its output is given, the figures of tools/ubench/bw.hip from the same run
All times: the host clock (time.perf_counter) around calls that end in a synchronise of the context; medians of R timed
rounds after warm-up rounds, the forms in rotation.
Usage: python tools/tiled_timing.py [rounds] [output file] [output of tools/ubench/bw.hip] [label]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import BatchCodec, DeviceArray  # noqa: E402
from spiht_amd.tiles import TiledCodec  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else None
BW = sys.argv[3] if len(sys.argv) > 3 else None
LABEL = sys.argv[4] if len(sys.argv) > 4 else "this build"
WARM = 2
TILES = (512, 256, 128)
ctx = _lib.default_context(0)
L = _lib.lib()
vp = C.c_void_p


def synth(seed, c, H, W):
    """a smooth pattern with edges plus noise, rounded to 8 bits, as float64 in [0, 1]"""
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
    """fns: {name: callable ending in a synchronise or returning host data} -> {name: [ms] * R}, the forms in rotation"""
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


def row(name, xs):
    return "  %-34s %9.2f   (min %.2f, max %.2f)" % (name, np.median(xs), min(xs), max(xs))


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


lines = ["%s: tiled pictures against the untiled calls; host clock around synchronised calls, median of %d after %d warm-up rounds"
         % (LABEL, R, WARM), ""]
ratios = {}

for (title, c, H, W, s, level, bpp) in [
        ("4096x4096 RGB, bior6.8, 1 bpp (untiled: level 9)", 3, 4096, 4096, spiht_amd.SpihtSettings(wavelet="bior6.8"), 9, 1.0),
        ("1920x1080 RGB, bior2.2, 0.5 bpp (untiled: level 7)", 3, 1080, 1920, spiht_amd.SpihtSettings(), 7, 0.5)]:
    MB = int(H * W * bpp)
    P = synth(7, c, H, W)
    lines += ["== %s: %d bits ==" % (title, MB)]
    # ---- host array to host array
    enc0 = spiht_amd.encode_image(P, s, level, MB)
    dec0 = spiht_amd.decode_image(enc0, s)[:, :H, :W]
    codecs = {t: TiledCodec(c, H, W, t, s, None, MB, ctx=ctx) for t in TILES}
    res = {t: codecs[t].encode(P) for t in TILES}
    dec = {t: codecs[t].decode(res[t]) for t in TILES}
    for t in TILES:  # a tiled decode is the paste of the tiles' own decodes: one tile checked here, all of them in the tests
        i, j = codecs[t].gy - 1, codecs[t].gx - 1
        tile = spiht_amd.decode_image(res[t].tile(i, j), s)[:, :t, :t]
        assert np.array_equal(tile[:, :H - i * t, :W - j * t], dec[t][:, i * t:, j * t:])
    fns = {"untiled encode_image": lambda: spiht_amd.encode_image(P, s, level, MB),
           "untiled decode_image": lambda: spiht_amd.decode_image(enc0, s)}
    for t in TILES:
        fns["tile %3d encode (T = %d)" % (t, codecs[t].T)] = (lambda t=t: codecs[t].encode(P))
        fns["tile %3d decode" % t] = (lambda t=t: codecs[t].decode(res[t]))
    y0, x0, wh, ww = H // 2 - 5, W // 2 - 5, H // 4, W // 4
    for t in TILES:
        fns["tile %3d window %dx%d" % (t, wh, ww)] = (lambda t=t: codecs[t].decode_window(res[t], y0, x0, wh, ww))
    tm = timed(fns)
    lines.append("host array to host array (ms):")
    lines += [row(n, tm[n]) for n in fns]
    for t in TILES:
        codecs[t].decode_window(res[t], y0, x0, wh, ww)
        lines.append("  tile %3d: the window decodes %d of %d tiles; decode x%.2f, window x%.2f of the untiled decode; encode x%.2f of the untiled encode"
                     % (t, codecs[t].last_tiles_decoded, codecs[t].T,
                        np.median(tm["untiled decode_image"]) / np.median(tm["tile %3d decode" % t]),
                        np.median(tm["untiled decode_image"]) / np.median(tm["tile %3d window %dx%d" % (t, wh, ww)]),
                        np.median(tm["tile %3d encode (T = %d)" % (t, codecs[t].T)]) / np.median(tm["untiled encode_image"])))
    # ---- device-resident
    bc = BatchCodec(c, H, W, s, level, MB, ctx=ctx)
    d_img = DeviceArray(ctx, (1, c, H, W), np.float64)
    d_img.upload(P[None])
    d_pic = DeviceArray(ctx, (1, c, bc.geom["rec_h"], bc.geom["rec_w"]), np.float64)
    d_str = DeviceArray(ctx, (1, bc.slot_stride), np.uint8)
    d_nb, d_ny, d_mn = DeviceArray(ctx, (1,), np.uint64), DeviceArray(ctx, (1,), np.uint64), DeviceArray(ctx, (1,), np.uint8)

    def enc_dev():
        bc.encode_device(d_img.ptr, 1, d_str.ptr, d_nb.ptr, d_mn.ptr)
        bc.nbits_to_nbytes(d_nb.ptr, 1, d_ny.ptr)

    enc_dev()
    ctx.synchronize()
    fns = {"untiled encode_device": enc_dev,
           "untiled decode_device": lambda: bc.decode_device(d_str.ptr, d_ny.ptr, d_mn.ptr, 1, d_pic.ptr)}
    dv = {}
    for t in TILES:
        k = codecs[t]
        d_packed = DeviceArray(ctx, (k.T * k.codec.slot_stride,), np.uint8)
        d_lens, d_maxn = DeviceArray(ctx, (k.T,), np.uint32), DeviceArray(ctx, (k.T,), np.uint8)
        d_out = DeviceArray(ctx, (c, H, W), np.float64)
        k.encode_device(d_img, 1, d_packed, d_lens, d_maxn)
        ctx.synchronize()
        total = int(d_lens.download().sum(dtype=np.int64))
        assert d_packed.download()[:total].tobytes() == res[t].encoded_bytes
        dv[t] = (d_packed, d_lens, d_maxn, d_out, total)
        fns["tile %3d encode_device" % t] = (lambda t=t: codecs[t].encode_device(d_img, 1, dv[t][0], dv[t][1], dv[t][2]))
        fns["tile %3d decode_device" % t] = (lambda t=t: codecs[t].decode_device(dv[t][0], dv[t][4], dv[t][1], dv[t][2], dv[t][3]))
    tm = timed(fns)
    lines.append("device-resident, pixels / streams / pictures in HBM (ms):")
    lines += [row(n, tm[n]) for n in fns]
    for t in TILES:
        ratios[(title, t)] = np.median(tm["untiled decode_device"]) / np.median(tm["tile %3d decode_device" % t])
        lines.append("  tile %3d: decode x%.2f of the untiled decode, encode x%.2f of the untiled encode"
                     % (t, ratios[(title, t)], np.median(tm["tile %3d encode_device" % t]) / np.median(tm["untiled encode_device"])))
        assert np.array_equal(dv[t][3].download(), dec[t])
    # ---- quality at the same total bits
    lines.append("PSNR against the picture at %d bits in all (dB): untiled %.2f (%d bytes)%s" % (
        MB, psnr(P, dec0), len(enc0.encoded_bytes),
        "".join(", tile %d %.2f (%d bytes)" % (t, psnr(P, dec[t]), len(res[t].encoded_bytes)) for t in TILES)))
    # ---- the four kernels on their own (float64 and 8-bit pictures, tile 512 and 128)
    if H == 4096:
        lines.append("kernels on their own, %dx%d RGB (ms per call of 20 queued back to back; GB/s = bytes read + written / time):" % (H, W))
        d_copy = DeviceArray(ctx, (c, H, W), np.float64)
        ms = launches(lambda: _lib.check(L.spiht_dev_copy(ctx.handle, vp(d_copy.ptr), vp(d_img.ptr), d_img.nbytes)))
        lines.append("  %-44s %8.3f ms  %8.1f GB/s" % ("device-to-device copy of the float64 picture", ms, 2 * d_img.nbytes / ms / 1e6))
        d_img8 = DeviceArray(ctx, (1, c, H, W), np.uint8)
        d_img8.upload(np.round(P[None] * 255).astype(np.uint8))
        for t in (512, 128):
            k = codecs[t]
            for name, es, src, cut, paste in (("float64", 8, d_img, L.spiht_tile_cut_f64, L.spiht_tile_paste_f64),
                                              ("uint8", 1, d_img8, L.spiht_tile_cut_u8, L.spiht_tile_paste_u8)):
                tiles_bytes = k.T * c * t * t * es
                d_tiles = DeviceArray(ctx, (tiles_bytes,), np.uint8)
                d_win = DeviceArray(ctx, (c * H * W * es,), np.uint8)
                st = (None,) if es == 1 else ()
                ms = launches(lambda: _lib.check(cut(ctx.handle, vp(src.ptr), *st, 1, c, H, W, t, t, vp(d_tiles.ptr))))
                lines.append("  %-44s %8.3f ms  %8.1f GB/s" % ("cut   %s, tile %d" % (name, t), ms, (c * H * W * es + tiles_bytes) / ms / 1e6))
                ms = launches(lambda: _lib.check(paste(ctx.handle, vp(d_tiles.ptr), c, t, t, H, W, t, t, 0, k.gy, 0, k.gx, 0, 0, H, W,
                                                       vp(d_win.ptr), *st)))
                lines.append("  %-44s %8.3f ms  %8.1f GB/s" % ("paste %s, tile %d" % (name, t), ms, 2 * c * H * W * es / ms / 1e6))
                d_tiles.free()
                d_win.free()
            # pack / unpack of this tiling's real streams
            d_packed, d_lens, d_maxn, _, total = dv[t]
            stride = k.codec.slot_stride
            d_slots, d_nbits, d_nbytes = DeviceArray(ctx, (k.T, stride), np.uint8), DeviceArray(ctx, (k.T,), np.uint64), DeviceArray(ctx, (k.T,), np.uint64)
            d_nbits.upload(8 * d_lens.download().astype(np.uint64))
            ms = launches(lambda: _lib.check(L.spiht_tile_unpack(ctx.handle, vp(d_packed.ptr), total, vp(d_lens.ptr), k.T, vp(d_slots.ptr),
                                                                 stride, vp(d_nbytes.ptr))))
            lines.append("  %-44s %8.3f ms  %8.1f GB/s" % ("unpack the %d streams of tile %d (%d bytes)" % (k.T, t, total), ms,
                                                          (total + k.T * stride) / ms / 1e6))
            ms = launches(lambda: _lib.check(L.spiht_tile_pack(ctx.handle, vp(d_slots.ptr), stride, vp(d_nbits.ptr), k.T, vp(d_packed.ptr),
                                                               d_packed.nbytes, vp(d_lens.ptr))))
            lines.append("  %-44s %8.3f ms  %8.1f GB/s" % ("pack   them", ms, 2 * total / ms / 1e6))
        # ... and of streams long enough to measure a rate: 1024 full slots of 256 KiB
        T2, stride = 1024, 256 * 1024
        d_slots, d_nbits = DeviceArray(ctx, (T2, stride), np.uint8), DeviceArray(ctx, (T2,), np.uint64)
        d_nbits.upload(np.full(T2, 8 * stride - 3, np.uint64))
        d_packed, d_lens, d_nbytes = DeviceArray(ctx, (T2 * stride,), np.uint8), DeviceArray(ctx, (T2,), np.uint32), DeviceArray(ctx, (T2,), np.uint64)
        ms = launches(lambda: _lib.check(L.spiht_tile_pack(ctx.handle, vp(d_slots.ptr), stride, vp(d_nbits.ptr), T2, vp(d_packed.ptr + 1),
                                                           d_packed.nbytes - 1, vp(d_lens.ptr))))
        lines.append("  %-44s %8.3f ms  %8.1f GB/s" % ("pack   1024 streams of 256 KiB, run 1 byte off", ms, 2 * T2 * stride / ms / 1e6))
        ms = launches(lambda: _lib.check(L.spiht_tile_unpack(ctx.handle, vp(d_packed.ptr + 1), T2 * stride - 1, vp(d_lens.ptr), T2,
                                                             vp(d_slots.ptr), stride, vp(d_nbytes.ptr))))
        lines.append("  %-44s %8.3f ms  %8.1f GB/s" % ("unpack them", ms, 2 * T2 * stride / ms / 1e6))
        for d in (d_slots, d_nbits, d_packed, d_lens, d_nbytes, d_copy, d_img8):
            d.free()
    for t in TILES:
        for d in dv[t][:4]:
            d.free()
        codecs[t].close()
    for d in (d_img, d_pic, d_str, d_nb, d_ny, d_mn):
        d.free()
    lines.append("")

if BW and os.path.exists(BW):
    lines.append("tools/ubench/bw.hip in the same run (read float64, write float64 + 3 x int32, by access width):")
    lines += ["  " + ln.rstrip() for ln in open(BW) if ln.strip()]
print("\n".join(lines))
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
