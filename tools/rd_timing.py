#!/usr/bin/env python3
"""Rate-distortion curve and cut against doing it by hand (profiles/rd_timing.txt): one 1080p RGB float64 picture coded at
1 bpp, 32 prefix lengths.
  rd_curve     BatchCodec.rd_curve(image, result, points=32) by the host clock, and its stages one by one with a wait after
               each (upload of the picture, forward transform for X, per group of lengths: the one-walk decode, the
               coefficient error, the batched inverse transform, the pixel error; download of the rows)
  cut_to_psnr  BatchCodec.cut_to_psnr(image, result, 35 dB), and at 33 dB (a target the 1 bpp stream reaches, so that the rounds run)
  by hand      what the feature replaces: decode_prefixes of the same lengths, the K float64 pictures brought to the host,
               the error computed in numpy
Usage: python tools/rd_timing.py [rounds] [output file] [label]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib, rd  # noqa: E402
from spiht_amd.batch import BatchCodec, DeviceArray  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 3
LABEL = sys.argv[3] if len(sys.argv) > 3 else "this build"
c, H, W = 3, 1080, 1920
MB = H * W  # 1 bpp
POINTS, TARGETS = 32, (35.0, 33.0)
ctx = _lib.default_context(0)
L = _lib.lib()
vp = C.c_void_p
s = spiht_amd.SpihtSettings()


def synth(seed):
    """a smooth pattern with edges plus noise, on the 8-bit grid"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((c, H, W))
    for k in range(c):
        fy, fx, ph = rng.uniform(2.0, 9.0), rng.uniform(2.0, 9.0), rng.uniform(0.0, 6.28)
        v = 0.5 + 0.3 * np.sin(fy * y / H + ph) * np.cos(fx * x / W + 0.4 * k) + 0.12 * ((x + 2 * y + 31 * k) % 97 > 48)
        out[k] = np.round(np.clip(v + rng.normal(0.0, 0.004, (H, W)), 0.0, 1.0) * 255) / 255
    return out


def ms(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


img = synth(1000)
codec = BatchCodec(c, H, W, s, None, MB, ctx=ctx)
g = codec.geom
enc = codec.encode(img[None])[0]
n = len(enc.encoded_bytes)
lens = rd.default_lengths(n, POINTS)
Kg = min(len(lens), rd.group_size(c, g["enc_h"], g["enc_w"], g["rec_h"], g["rec_w"], 2 ** 31))
q = float(s.quantization_scale)


def staged():
    """the path of rd_curve with a wait after every stage -> {stage: ms}"""
    t = {}
    held = []

    def dev(shape, dt):
        held.append(DeviceArray(ctx, shape, dt))
        return held[-1]

    def add(name, fn):
        t[name] = t.get(name, 0.0) + ms(fn)[1]

    d_pic, d_x, d_ma = dev(img.shape, np.float64), dev((c, g["enc_h"], g["enc_w"]), np.int32), dev((1,), np.uint32)
    d_rec, d_dec = dev((Kg, c, g["enc_h"], g["enc_w"]), np.int32), dev((Kg, c, g["rec_h"], g["rec_w"]), np.float64)
    d_e, d_s = dev((len(lens), 2), np.uint64), dev((len(lens), c), np.float64)
    add("upload", lambda: d_pic.upload(img))
    add("forward", lambda: _lib.check(L.spiht_dwt_pyramid_batch_f64(
        ctx.handle, vp(d_pic.ptr), 1, c, H, W, codec.wid, codec.mid, codec._lv, q, codec._mults_p, vp(d_x.ptr), None, None,
        vp(d_ma.ptr))))
    data = np.frombuffer(enc.encoded_bytes, np.uint8)
    for k0 in range(0, len(lens), Kg):
        kg = min(Kg, len(lens) - k0)
        bud = np.ascontiguousarray([8 * k for k in lens[k0:k0 + kg]], dtype=np.uint64)
        add("walk", lambda: _lib.check(L.spiht_decode_budgets_dev_i32(
            ctx.handle, vp(data.ctypes.data), data.size, int(enc.max_n), c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"],
            vp(bud.ctypes.data), kg, vp(d_rec.ptr))))
        add("sqerr", lambda: _lib.check(L.spiht_sqerr_i32(ctx.handle, vp(d_x.ptr), vp(d_rec.ptr), kg, c, g["enc_h"], g["enc_w"],
                                                          vp(d_e.ptr + 16 * k0))))
        add("inverse", lambda: _lib.check(L.spiht_dequant_idwt_batch_f64(
            ctx.handle, vp(d_rec.ptr), kg, c, H, W, codec.wid, codec.mid, codec._lv, q, codec._mults_p, vp(d_dec.ptr))))
        add("sse", lambda: _lib.check(L.spiht_sse_f64(ctx.handle, vp(d_pic.ptr), vp(d_dec.ptr), kg, c, H, W, g["rec_h"],
                                                      g["rec_w"], vp(d_s.ptr + 8 * c * k0))))
    add("download", lambda: (d_e.download(), d_s.download()))
    for d in held:
        d.free()
    return t


def by_hand():
    pics = codec.decode_prefixes(enc, lens)
    return [float(((img - p[:, :H, :W]) ** 2).mean()) for p in pics]


curve = codec.rd_curve(img, enc, points=POINTS)  # (warm-up: buffers of the context grow once)
staged()
mse_hand = by_hand()
assert np.allclose(curve.mse, mse_hand, rtol=1e-9, atol=0)

t_curve, t_cut, t_hand, stages, cuts = [], {t: [] for t in TARGETS}, [], [], {}
for r in range(R):
    t_curve.append(ms(lambda: codec.rd_curve(img, enc, points=POINTS))[1])
    stages.append(staged())
    for target in TARGETS:
        cuts[target], t = ms(lambda: codec.cut_to_psnr(img, enc, target, POINTS))
        t_cut[target].append(t)
    t_hand.append(ms(by_hand)[1])

STAGES = ("upload", "forward", "walk", "sqerr", "inverse", "sse", "download")
groups = -(-len(lens) // Kg)
read_gb = {"sqerr": len(lens) * c * g["enc_h"] * g["enc_w"] * 4 / 1e9, "sse": len(lens) * c * H * W * 8 / 1e9}
lines = ["%s: rate-distortion curve of one %dx%d RGB float64 picture, bior2.2 reflect, level None (%d), %d bits (1 bpp), stream of "
         "%d bytes" % (LABEL, H, W, g["level"], MB, n),
         "%d prefix lengths in %d group(s) of at most %d (max_bytes 2^31); median of %d runs, ms, by the host clock"
         % (len(lens), groups, Kg, R), ""]
lines.append("rd_curve, one call                       %9.2f   (runs: %s)" % (np.median(t_curve), " ".join("%.2f" % x for x in t_curve)))
lines.append("  its stages, a wait after each:")
for name in STAGES:
    v = float(np.median([st[name] for st in stages]))
    extra = "   %.2f GB of decoded data read: %.0f GB/s" % (read_gb[name], read_gb[name] / (v / 1e3)) if name in read_gb else ""
    lines.append("    %-10s %9.3f%s" % (name, v, extra))
for target in TARGETS:
    cut, db, met = cuts[target]
    lines.append("cut_to_psnr(%.0f dB), %d-point rounds         %9.2f   -> %d bytes, %.3f dB, met %s   (runs: %s)"
                 % (target, POINTS, np.median(t_cut[target]), len(cut.encoded_bytes), db, met,
                    " ".join("%.2f" % x for x in t_cut[target])))
lines.append("by hand: decode_prefixes + numpy error    %9.2f   (%.1f MB of pictures over the link; runs: %s)"
             % (np.median(t_hand), len(lens) * c * g["rec_h"] * g["rec_w"] * 8 / 1e6, " ".join("%.2f" % x for x in t_hand)))
lines.append("")
lines.append("curve: bytes, bpp, PSNR dB")
for i in range(0, len(lens), 4):
    lines.append("  " + "   ".join("%7d %.3f %6.2f" % (curve.byte_lengths[j], curve.bpp[j], curve.psnr[j])
                                   for j in range(i, min(i + 4, len(lens)))))
print("\n".join(lines))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write("\n".join(lines) + "\n")
