#!/usr/bin/env python3
"""Reduced-resolution decode against the full-size decode (profiles/reduced_timing.txt): 256 distinct 1080p RGB streams at
0.5 bpp, reduce = 0, 1, 2, 3, float64 and 8-bit pictures, the forms alternating within one run.
  batch     BatchCodec.decode_reduced_device / _u8 of the 256 streams (device-resident): the whole call by the host clock
            (queue + synchronize) and by stage (the library's stage timers: the list decoder, level 1 of the inverse
            transform, the other levels, the clearing of the coefficient array), and the bytes of the pictures written
  single    one stream from a host array to a host array: decode_image_reduced / decode_image_reduced_u8
Usage: python tools/reduced_timing.py [B] [rounds] [output file] [label]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import BatchCodec, DeviceArray  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LABEL = sys.argv[4] if len(sys.argv) > 4 else "this build"
c, H, W = 3, 1080, 1920
MB = int(H * W * 0.5)
KS = (0, 1, 2, 3)
KINDS = ("f64", "u8")
ctx = _lib.default_context(0)
s = spiht_amd.SpihtSettings()


def synth_u8(seed):
    """a smooth pattern with edges plus noise, rounded to uint8"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((c, H, W), np.uint8)
    for k in range(c):
        fy, fx, ph = rng.uniform(2.0, 9.0), rng.uniform(2.0, 9.0), rng.uniform(0.0, 6.28)
        v = 0.5 + 0.3 * np.sin(fy * y / H + ph) * np.cos(fx * x / W + 0.4 * k) + 0.12 * ((x + 2 * y + 31 * k) % 97 > 48)
        out[k] = np.round(np.clip(v + rng.normal(0.0, 0.004, (H, W)), 0.0, 1.0) * 255)
    return out


# B distinct pictures: 8 generated ones, each shifted and mirrored into variants
base = [synth_u8(1000 + i) for i in range(8)]
P = np.empty((B, c, H, W), np.uint8)
for b in range(B):
    v = np.roll(base[b % 8], 7 * (b // 8), axis=2)
    P[b] = v[:, ::-1, :] if (b // 8) & 1 else v

codec = BatchCodec(c, H, W, s, None, MB, ctx=ctx)
g = codec.geom
shapes = {k: codec.reduced_shape(k) for k in KS}
d_img = DeviceArray(ctx, (B, c, H, W), np.uint8)
d_img.upload(P)
d_out = DeviceArray(ctx, (B, codec.slot_stride), np.uint8)
d_nb, d_ny, d_mn = DeviceArray(ctx, (B,), np.uint64), DeviceArray(ctx, (B,), np.uint64), DeviceArray(ctx, (B,), np.uint8)
codec.encode_device_u8(d_img.ptr, B, d_out.ptr, d_nb.ptr, d_mn.ptr)
codec.nbits_to_nbytes(d_nb.ptr, B, d_ny.ptr)
ctx.synchronize()
d_img.free()
# one picture buffer per kind, of the full size (every reduced picture fits)
d_pic = {"f64": DeviceArray(ctx, (B, c, g["rec_h"], g["rec_w"]), np.float64), "u8": DeviceArray(ctx, (B, c, H, W), np.uint8)}


def pic_bytes(kind, k):
    rs = shapes[k]
    return B * c * (rs["rec_h"] * rs["rec_w"] * 8 if kind == "f64" else rs["pic_h"] * rs["pic_w"])


def decode(kind, k):
    if kind == "f64":
        codec.decode_reduced_device(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_pic[kind].ptr, k)
    else:
        codec.decode_reduced_device_u8(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_pic[kind].ptr, k)


def spread(xs):
    return "spread %.1f %%" % (100.0 * (max(xs) - min(xs)) / np.median(xs))


lines = ["%s: reduced-resolution decode, %d distinct %dx%d RGB streams, bior2.2 reflect, level None (%d), %d bits (0.5 bpp)"
         % (LABEL, B, H, W, g["level"], MB), ""]
cases = [(kind, k) for kind in KINDS for k in KS]
for kind, k in cases:
    decode(kind, k)
ctx.synchronize()
# reduce 0 is the full-size call (first two pictures)
full = np.empty((2, c, g["rec_h"], g["rec_w"]), np.float64)
codec.decode_device(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_pic["f64"].ptr)
ctx.synchronize()
ctx.download(full, d_pic["f64"].ptr)
decode("f64", 0)
ctx.synchronize()
again = np.empty_like(full)
ctx.download(again, d_pic["f64"].ptr)
assert np.array_equal(full.view(np.uint64), again.view(np.uint64))

STAGES = ("decode_lists", "idwt_level1", "idwt_rest", "memset")
wall = {cs: [] for cs in cases}
st = {cs: [] for cs in cases}
for r in range(R):
    rot = cases[r % len(cases):] + cases[:r % len(cases)]
    for cs in rot:
        ctx.synchronize()
        t0 = time.perf_counter()
        decode(*cs)
        ctx.synchronize()
        wall[cs].append((time.perf_counter() - t0) * 1e3)
    for cs in rot:  # (the stage timers put events between the kernels: a run of their own)
        ctx.reset_timing()
        ctx.set_timing(True)
        decode(*cs)
        ctx.synchronize()
        ctx.set_timing(False)
        t = ctx.timing()
        st[cs].append(tuple(t[name][0] for name in STAGES))
lines.append("batched decode of the %d streams, device-resident (median of %d, the forms in rotation; ms; MB written = the pictures):"
             % (B, R))
lines.append("  %-6s %6s %9s %9s | %12s %11s %9s %7s" % (("pixels", "reduce", "call", "MB") + STAGES))
for cs in cases:
    a = np.median(np.array(st[cs]), axis=0)
    lines.append("  %-6s %6d %9.2f %9.1f | %12.3f %11.3f %9.3f %7.3f" % (cs + (np.median(wall[cs]), pic_bytes(*cs) / 1e6) + tuple(a)))
    lines.append("         call runs: %s   %s" % (" ".join("%.2f" % x for x in wall[cs]), spread(wall[cs])))
lines.append("")

# ---- single call, host array to host array ----
enc = spiht_amd.encode_image_u8(P[0], s, max_bits=MB)
FN = {"f64": spiht_amd.decode_image_reduced, "u8": spiht_amd.decode_image_reduced_u8}
sc = {cs: [] for cs in cases}
for r in range(4 + 2 * R):
    rot = cases[r % len(cases):] + cases[:r % len(cases)]
    for kind, k in rot:
        t0 = time.perf_counter()
        FN[kind](enc, s, k)
        if r >= 2:
            sc[(kind, k)].append((time.perf_counter() - t0) * 1e3)
lines.append("single call, one %dx%d RGB stream, host array to host array (median of %d; ms; min-max; KB returned):"
             % (H, W, len(sc[cases[0]])))
for kind, k in cases:
    x = sc[(kind, k)]
    lines.append("  %-6s reduce %d  %7.2f (%.2f-%.2f)  %9.1f KB" % (kind, k, np.median(x), min(x), max(x), pic_bytes(kind, k) / B / 1e3))
print("\n".join(lines))
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        f.write("\n".join(lines) + "\n")
