#!/usr/bin/env python3
"""16-bit pixels against float64 and 8-bit pixels (profiles/u16_timing.txt): 256 distinct 1080p RGB pictures at 0.5 bpp, the
forms alternating within one run.
  stages    BatchCodec round trip (encode_device + decode_device, and the *_u8 / *_u16 forms): the library's stage timers of
            level 1 of the forward and the inverse transform (dwt_level1, idwt_level1: the integer conversions happen inside
            them) and of the other levels
  pipeline  Pipeline.submit / submit_u8 / submit_u16: the pipelined step, steady state (steps of one kind back to back)
  single    one picture from host array to host array: encode_image(P / 65535) / decode_image against the *_u8 and *_u16 calls
A build without the 16-bit names (the commit before them) is measured with the same tool: the uint16 rows are then left out,
and the float64 and uint8 rows are what the new build's are held against.
Usage: python tools/u16_timing.py [B] [rounds] [output file] [label]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import BatchCodec, DeviceArray, Pipeline  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LABEL = sys.argv[4] if len(sys.argv) > 4 else "this build"
c, H, W = 3, 1080, 1920
MB = int(H * W * 0.5)
HAS16 = hasattr(spiht_amd, "encode_image_u16")
KINDS = ("f64", "u8", "u16") if HAS16 else ("f64", "u8")
ctx = _lib.default_context(0)
s = spiht_amd.SpihtSettings()


def synth_u16(seed):
    """a smooth pattern with edges plus noise, rounded to uint16: the low bytes vary (all 256 values present)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((c, H, W), np.uint16)
    for k in range(c):
        fy, fx, ph = rng.uniform(2.0, 9.0), rng.uniform(2.0, 9.0), rng.uniform(0.0, 6.28)
        v = 0.5 + 0.3 * np.sin(fy * y / H + ph) * np.cos(fx * x / W + 0.4 * k) + 0.12 * ((x + 2 * y + 31 * k) % 97 > 48)
        out[k] = np.round(np.clip(v + rng.normal(0.0, 0.004, (H, W)), 0.0, 1.0) * 65535)
    assert len(np.unique(out & 0xFF)) == 256
    return out


# 256 distinct pictures: 8 generated ones, each shifted and mirrored into 32 variants
base = [synth_u16(1000 + i) for i in range(8)]
P = np.empty((B, c, H, W), np.uint16)
for b in range(B):
    v = np.roll(base[b % 8], 7 * (b // 8), axis=2)
    P[b] = v[:, ::-1, :] if (b // 8) & 1 else v
assert len({P[b, 0, 500, :64].tobytes() + bytes([b % 8]) for b in range(B)}) == B
P8 = (P >> 8).astype(np.uint8)  # the 8-bit pictures: the high bytes

codec = BatchCodec(c, H, W, s, None, MB, ctx=ctx)
g = codec.geom
DT = {"f64": np.float64, "u8": np.uint8, "u16": np.uint16}
d_in = {k: DeviceArray(ctx, (B, c, H, W), DT[k]) for k in KINDS}
d_rec = {k: DeviceArray(ctx, (B, c, g["rec_h"], g["rec_w"]) if k == "f64" else (B, c, H, W), DT[k]) for k in KINDS}
d_out = DeviceArray(ctx, (B, codec.slot_stride), np.uint8)
d_nb = DeviceArray(ctx, (B,), np.uint64)
d_mn = DeviceArray(ctx, (B,), np.uint8)
d_ny = DeviceArray(ctx, (B,), np.uint64)
for b in range(B):
    d_in["f64"].upload(P[b] / 65535, offset_bytes=b * c * H * W * 8)
d_in["u8"].upload(P8)
if HAS16:
    d_in["u16"].upload(P)
ctx.synchronize()
lines = ["%s: float64, 8-bit and 16-bit pixels, %d distinct %dx%d RGB pictures, bior2.2 reflect, level None, %d bits (0.5 bpp)"
         % (LABEL, B, H, W, MB), ""]
ENC = {"f64": "encode_device", "u8": "encode_device_u8", "u16": "encode_device_u16"}
DEC = {"f64": "decode_device", "u8": "decode_device_u8", "u16": "decode_device_u16"}
SUB = {"f64": "submit", "u8": "submit_u8", "u16": "submit_u16"}


def order(r):
    """the kinds, rotated from round to round"""
    return KINDS[r % len(KINDS):] + KINDS[:r % len(KINDS)]


def spread(xs):
    return "spread %.1f %%" % (100.0 * (max(xs) - min(xs)) / np.median(xs))


def rt(kind):
    getattr(codec, ENC[kind])(d_in[kind].ptr, B, d_out.ptr, d_nb.ptr, d_mn.ptr)
    codec.nbits_to_nbytes(d_nb.ptr, B, d_ny.ptr)
    getattr(codec, DEC[kind])(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_rec[kind].ptr)


# ---- stages ----
st = {k: [] for k in KINDS}
for kind in KINDS:
    rt(kind)
ctx.synchronize()
for r in range(R):
    for kind in order(r):
        ctx.reset_timing()
        ctx.set_timing(True)
        rt(kind)
        ctx.synchronize()
        ctx.set_timing(False)
        t = ctx.timing()
        st[kind].append((t["dwt_level1"][0], t["idwt_level1"][0], t["dwt_rest"][0], t["idwt_rest"][0]))
    if r == 0 and HAS16:  # the decodes give the pictures of the contract's formula (first two pictures)
        rt("f64")
        ctx.synchronize()
        f = np.empty((2, c, g["rec_h"], g["rec_w"]), np.float64)
        ctx.download(f, d_rec["f64"].ptr)
        rt("u16")
        ctx.synchronize()
        u = np.empty((2, c, H, W), np.uint16)
        ctx.download(u, d_rec["u16"].ptr)
        assert np.array_equal(u, (np.clip(f, 0.0, 1.0) * 65535.0).astype(np.uint16)[:, :, :H, :W])
lines.append("stage timers, BatchCodec round trip of the %d pictures (median of %d, the kinds in rotation; ms):" % (B, R))
lines.append("  %-6s %10s %11s %10s %10s" % ("pixels", "dwt_level1", "idwt_level1", "dwt_rest", "idwt_rest"))
for kind in KINDS:
    a = np.array(st[kind])
    lines.append("  %-6s %10.3f %11.3f %10.3f %10.3f" % ((kind,) + tuple(np.median(a, axis=0))))
    lines.append("         runs (dwt_level1/idwt_level1): " + "  ".join("%.3f/%.3f" % (x[0], x[1]) for x in st[kind]))
    lines.append("         %s / %s" % (spread(a[:, 0]), spread(a[:, 1])))
lines.append("")

# ---- pipelined step ----
pl = Pipeline(codec, B)
NS = 4


def steps(kind):
    for _ in range(NS):
        getattr(pl, SUB[kind])(d_in[kind].ptr, d_out.ptr, d_nb.ptr, d_mn.ptr, d_rec[kind].ptr)
    pl.synchronize()


ps = {k: [] for k in KINDS}
for kind in KINDS:
    steps(kind)
for r in range(R):
    for kind in order(r):
        t0 = time.perf_counter()
        steps(kind)
        ps[kind].append((time.perf_counter() - t0) * 1e3 / NS)
pl.close()
lines.append("pipelined step (Pipeline, %d images per step, %d steps back to back incl. the flush; ms per step):" % (B, NS))
for kind in KINDS:
    lines.append("  %-6s median %8.2f   runs: %s   %s" % (kind, np.median(ps[kind]), " ".join("%.2f" % x for x in ps[kind]),
                                                         spread(ps[kind])))
lines.append("")

# ---- single call, host array to host array ----
img = {"f64": P[0] / 65535, "u8": P8[0], "u16": P[0]}
enc = spiht_amd.encode_image(img["f64"], s, max_bits=MB)
EF = {"f64": "encode_image", "u8": "encode_image_u8", "u16": "encode_image_u16"}
DF = {"f64": "decode_image", "u8": "decode_image_u8", "u16": "decode_image_u16"}
sc = {(d, k): [] for d in ("enc", "dec") for k in KINDS}
for r in range(4 + 2 * R):
    for d in ("enc", "dec"):
        for k in order(r):
            t0 = time.perf_counter()
            if d == "enc":
                getattr(spiht_amd, EF[k])(img[k], s, max_bits=MB)
            else:
                getattr(spiht_amd, DF[k])(enc, s)
            if r >= 2:
                sc[(d, k)].append((time.perf_counter() - t0) * 1e3)
lines.append("single call, one %dx%d RGB picture, host array to host array (median of %d; ms; min-max):" % (H, W, len(sc[("enc", "f64")])))
for d, name in (("enc", "encode"), ("dec", "decode")):
    lines.append("  %s  " % name + "   ".join("%s %.2f (%.2f-%.2f)" % (k, np.median(sc[(d, k)]), min(sc[(d, k)]), max(sc[(d, k)]))
                                               for k in KINDS))
print("\n".join(lines))
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        f.write("\n".join(lines) + "\n")
