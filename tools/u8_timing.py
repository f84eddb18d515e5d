#!/usr/bin/env python3
"""8-bit pixels against float64 pixels (profiles/u8_timing.txt): 256 distinct 1080p RGB pictures at 0.5 bpp, the two forms
alternating within one run.
  stages    BatchCodec round trip (encode_device + decode_device, and the *_u8 forms): the library's stage timers of level 1 of
            the forward and the inverse transform (dwt_level1, idwt_level1: the 8-bit conversion happens inside them)
  pipeline  Pipeline.submit / submit_u8: the pipelined step, steady state (steps of one kind back to back)
  single    one picture from host array to host array: encode_image(P / 255) / decode_image against encode_image_u8(P) /
            decode_image_u8
Usage: python tools/u8_timing.py [B] [rounds] [output file]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_u8  # noqa: E402
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import BatchCodec, DeviceArray, Pipeline  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
R = int(sys.argv[2]) if len(sys.argv) > 2 else 3
c, H, W = 3, 1080, 1920
MB = int(H * W * 0.5)
ctx = _lib.default_context(0)
s = spiht_amd.SpihtSettings()

# 256 distinct pictures: 8 generated ones, each shifted and mirrored into 32 variants (the generator takes a second each)
base = [synth_u8(1000 + i, c, H, W) for i in range(8)]
P = np.empty((B, c, H, W), np.uint8)
for b in range(B):
    v = np.roll(base[b % 8], 7 * (b // 8), axis=2)
    P[b] = v[:, ::-1, :] if (b // 8) & 1 else v
assert len({P[b, 0, 500, :64].tobytes() + bytes([b % 8]) for b in range(B)}) == B

codec = BatchCodec(c, H, W, s, None, MB, ctx=ctx)
g = codec.geom
d_f = DeviceArray(ctx, (B, c, H, W), np.float64)
d_u = DeviceArray(ctx, (B, c, H, W), np.uint8)
d_rf = DeviceArray(ctx, (B, c, g["rec_h"], g["rec_w"]), np.float64)
d_ru = DeviceArray(ctx, (B, c, H, W), np.uint8)
d_out = DeviceArray(ctx, (B, codec.slot_stride), np.uint8)
d_nb = DeviceArray(ctx, (B,), np.uint64)
d_mn = DeviceArray(ctx, (B,), np.uint8)
d_ny = DeviceArray(ctx, (B,), np.uint64)
for b in range(B):
    d_f.upload(P[b] / 255, offset_bytes=b * c * H * W * 8)
d_u.upload(P)
ctx.synchronize()
lines = ["8-bit pixels against float64 pixels: %d distinct %dx%d RGB pictures, bior2.2 reflect, level None, %d bits (0.5 bpp)"
         % (B, H, W, MB), ""]


def rt(kind):
    if kind == "f64":
        codec.encode_device(d_f.ptr, B, d_out.ptr, d_nb.ptr, d_mn.ptr)
        codec.nbits_to_nbytes(d_nb.ptr, B, d_ny.ptr)
        codec.decode_device(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_rf.ptr)
    else:
        codec.encode_device_u8(d_u.ptr, B, d_out.ptr, d_nb.ptr, d_mn.ptr)
        codec.nbits_to_nbytes(d_nb.ptr, B, d_ny.ptr)
        codec.decode_device_u8(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_ru.ptr)


# ---- stages ----
st = {"f64": [], "u8": []}
for kind in ("f64", "u8"):
    rt(kind)
ctx.synchronize()
for r in range(R):
    for kind in (("f64", "u8") if r % 2 == 0 else ("u8", "f64")):
        ctx.reset_timing()
        ctx.set_timing(True)
        rt(kind)
        ctx.synchronize()
        ctx.set_timing(False)
        t = ctx.timing()
        st[kind].append((t["dwt_level1"][0], t["idwt_level1"][0], t["dwt_rest"][0], t["idwt_rest"][0]))
# the two decodes give the same pictures (the u8 one by the contract's formula, cropped)
ref = (np.clip(d_rf.download()[:2], 0.0, 1.0) * 255.0).astype(np.uint8)[:, :, :H, :W]
assert np.array_equal(d_ru.download()[:2], ref)
lines.append("stage timers, BatchCodec round trip of the %d pictures (median of %d, alternating; ms):" % (B, R))
lines.append("  %-6s %10s %10s %10s %10s" % ("pixels", "dwt_level1", "idwt_level1", "dwt_rest", "idwt_rest"))
for kind in ("f64", "u8"):
    a = np.median(np.array(st[kind]), axis=0)
    lines.append("  %-6s %10.3f %10.3f %10.3f %10.3f" % ((kind,) + tuple(a)))
    lines.append("         runs: " + "  ".join("%.3f/%.3f" % (x[0], x[1]) for x in st[kind]))
lines.append("")

# ---- pipelined step ----
pl = Pipeline(codec, B)
NS = 4


def steps(kind):
    for _ in range(NS):
        if kind == "f64":
            pl.submit(d_f.ptr, d_out.ptr, d_nb.ptr, d_mn.ptr, d_rf.ptr)
        else:
            pl.submit_u8(d_u.ptr, d_out.ptr, d_nb.ptr, d_mn.ptr, d_ru.ptr)
    pl.synchronize()


ps = {"f64": [], "u8": []}
steps("f64")
steps("u8")
for r in range(R):
    for kind in (("f64", "u8") if r % 2 == 0 else ("u8", "f64")):
        t0 = time.perf_counter()
        steps(kind)
        ps[kind].append((time.perf_counter() - t0) * 1e3 / NS)
pl.close()
lines.append("pipelined step (Pipeline, %d images per step, %d steps back to back incl. the flush; ms per step):" % (B, NS))
for kind in ("f64", "u8"):
    lines.append("  %-6s median %8.2f   runs: %s" % (kind, np.median(ps[kind]), " ".join("%.2f" % x for x in ps[kind])))
lines.append("")

# ---- single call, host array to host array ----
img8 = P[0]
imgf = img8 / 255
enc = spiht_amd.encode_image(imgf, s, max_bits=MB)
sc = {k: [] for k in ("enc_f64", "enc_u8", "dec_f64", "dec_u8")}
for r in range(5 + 2 * R):
    for k in (("enc_f64", "enc_u8", "dec_f64", "dec_u8") if r % 2 == 0 else ("enc_u8", "enc_f64", "dec_u8", "dec_f64")):
        t0 = time.perf_counter()
        if k == "enc_f64":
            spiht_amd.encode_image(imgf, s, max_bits=MB)
        elif k == "enc_u8":
            spiht_amd.encode_image_u8(img8, s, max_bits=MB)
        elif k == "dec_f64":
            spiht_amd.decode_image(enc, s)
        else:
            spiht_amd.decode_image_u8(enc, s)
        if r >= 2:
            sc[k].append((time.perf_counter() - t0) * 1e3)
lines.append("single call, one %dx%d RGB picture, host array to host array (median of %d; ms):" % (H, W, len(sc["enc_f64"])))
lines.append("  encode  float64 %.2f   uint8 %.2f" % (np.median(sc["enc_f64"]), np.median(sc["enc_u8"])))
lines.append("  decode  float64 %.2f   uint8 %.2f" % (np.median(sc["dec_f64"]), np.median(sc["dec_u8"])))
print("\n".join(lines))
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        f.write("\n".join(lines) + "\n")
