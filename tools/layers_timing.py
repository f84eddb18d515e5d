#!/usr/bin/env python3
"""Quality layers of a tiled picture against the one-rate tiled calls (profiles/layers_timing.txt), everything in one run:
  pictures  the two of tools/tiled_timing.py: one 4096x4096 RGB picture, bior6.8, 1 bpp, and one 1920x1080 RGB picture,
            bior2.2, 0.5 bpp; tiles of 512, 256 and 128 at the default level of a tile; allocate="rd", points 16, spread 4
  encode    TiledCodec.encode_layered_device with Q = 1, 4 and 8 layers beside encode_device of the same codec, pixels and
            streams resident in HBM
  decode    TiledCodec.decode_layers_device of all Q layers beside decode_device of result.tiled(), streams and picture
            resident in HBM
  copies    spiht_layer_pack / spiht_layer_unpack on their own, on the slots and runs of those encodes, against a
            device-to-device copy (spiht_dev_copy) of as many bytes as the run holds
  psnr      of the decode after every layer, with the file length at which the layer is complete
All times: the host clock (time.perf_counter) around calls that end in a synchronise of the context; medians of R timed
rounds after warm-up rounds, the forms in rotation.
Usage: python tools/layers_timing.py [rounds] [output file] [label]"""
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
TILES = (512, 256, 128)
LAYERS = (1, 4, 8)
ctx = _lib.default_context(0)
L = _lib.lib()
vp = C.c_void_p


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


lines = []


def say(*new):
    """a line of the report, shown as soon as it is known"""
    lines.extend(new)
    print("\n".join(new), flush=True)


def row(name, ms, base):
    say("  %-34s %8.2f  (min %.2f, max %.2f)  x%5.2f" % (name, np.median(ms), min(ms), max(ms), np.median(ms) / base))


say(*["%s: quality layers of a tiled picture against the one-rate tiled calls of the same allocate=\"rd\" codec; host clock" % LABEL,
      "around synchronised calls, median of %d after %d warm-up rounds, the forms in rotation" % (R, WARM), ""])
for (title, c, H, W, s, bpp) in [
        ("4096x4096 RGB, bior6.8, 1 bpp", 3, 4096, 4096, spiht_amd.SpihtSettings(wavelet="bior6.8"), 1.0),
        ("1920x1080 RGB, bior2.2, 0.5 bpp", 3, 1080, 1920, spiht_amd.SpihtSettings(), 0.5)]:
    MB = int(H * W * bpp)
    P = synth(7, c, H, W)
    d_img = DeviceArray(ctx, (1, c, H, W), np.float64)
    d_img.upload(P[None])
    d_out = DeviceArray(ctx, (c, H, W), np.float64)
    say("== %s: %d bits = %d bytes in all ==" % (title, MB, MB // 8))
    for t in TILES:
        k = TiledCodec(c, H, W, t, s, None, MB, ctx=ctx, allocate="rd")
        T, stride = k.T, k.codec.slot_stride
        d_packed = DeviceArray(ctx, (T * stride,), np.uint8)
        d_lens, d_maxn = DeviceArray(ctx, (T,), np.uint32), DeviceArray(ctx, (T,), np.uint8)
        d_cum, d_pic = DeviceArray(ctx, (max(LAYERS) * T,), np.uint32), DeviceArray(ctx, (1,), np.uint64)
        enc = {"encode_device": lambda: k.encode_device(d_img, 1, d_packed, d_lens, d_maxn)}
        for Q in LAYERS:
            enc["encode_layered_device, Q = %d" % Q] = lambda Q=Q: k.encode_layered_device(d_img, 1, Q, d_packed, d_cum, d_maxn, d_pic)
        tm = timed(enc)
        say("tile %d (T = %d, slots of %d bytes): encode (ms)" % (t, T, stride))
        for name in enc:
            row(name, tm[name], np.median(tm["encode_device"]))
        # the decodes, each on the streams of its own encode; every form gets slots of the longest tile
        res = {Q: k.encode_layered(P, Q) for Q in LAYERS}
        plain = res[LAYERS[0]].tiled()
        longest = max(4, (max(plain.nbytes) + 3) & ~3)
        total = len(plain.encoded_bytes)
        d_run = {Q: DeviceArray(ctx, (total + 16,), np.uint8) for Q in LAYERS}
        d_tab = {Q: DeviceArray(ctx, (Q * T,), np.uint32) for Q in LAYERS}
        for Q in LAYERS:
            d_run[Q].upload(np.concatenate([np.frombuffer(res[Q].encoded_bytes, np.uint8), np.zeros(16, np.uint8)]))
            d_tab[Q].upload(np.asarray(res[Q].cum, np.uint32).reshape(-1))
        d_plain = DeviceArray(ctx, (total + 16,), np.uint8)
        d_plain.upload(np.concatenate([np.frombuffer(plain.encoded_bytes, np.uint8), np.zeros(16, np.uint8)]))
        d_lens.upload(np.asarray(plain.nbytes, np.uint32))
        d_maxn.upload(np.asarray(plain.max_n, np.uint8))
        whole, pic = (0, k.gy, 0, k.gx), (0, 0, H, W)
        dec = {"decode_device of tiled()": lambda: k.decode_device(d_plain, total, d_lens, d_maxn, d_out, None, longest)}
        for Q in LAYERS:
            dec["decode_layers_device, Q = %d" % Q] = lambda Q=Q: k.decode_layers_device(d_run[Q], total, d_tab[Q], d_maxn, Q, Q, whole,
                                                                                        pic, d_out, None, longest)
        tm = timed(dec)
        say("tile %d: decode of all layers, %d bytes (ms)" % (t, total))
        for name in dec:
            row(name, tm[name], np.median(tm["decode_device of tiled()"]))
        # the two copies on their own, on the slots the last encode left and the run of Q layers
        d_copy = DeviceArray(ctx, (total + 16,), np.uint8)
        ms = launches(lambda: _lib.check(L.spiht_dev_copy(ctx.handle, vp(d_copy.ptr), vp(d_plain.ptr), total)))
        say("tile %d: the copies on their own (ms per call of 20 queued back to back; GB/s = 2 x %d bytes / time)" % (t, total),
            "  %-34s %8.3f ms  %8.1f GB/s" % ("device-to-device copy", ms, 2 * total / ms / 1e6))
        d_slots, d_nbytes = DeviceArray(ctx, (T * longest,), np.uint8), DeviceArray(ctx, (T,), np.uint64)
        for Q in LAYERS:
            k.encode_layered_device(d_img, 1, Q, d_packed, d_cum, d_maxn, d_pic)  # leaves the slots and the Q cuts in the codec
            ms = launches(lambda: _lib.check(L.spiht_layer_pack(ctx.handle, vp(k._bufs["slots"].ptr), stride, vp(k._bufs["cuts"].ptr), Q, 1,
                                                                T, vp(d_packed.ptr), d_packed.nbytes, vp(d_cum.ptr), vp(d_pic.ptr))))
            say("  %-34s %8.3f ms  %8.1f GB/s" % ("spiht_layer_pack, Q = %d" % Q, ms, 2 * total / ms / 1e6))
            ms = launches(lambda: _lib.check(L.spiht_layer_unpack(ctx.handle, vp(d_run[Q].ptr), total, vp(d_tab[Q].ptr), Q, T, Q, None, T,
                                                                  vp(d_slots.ptr), longest, vp(d_nbytes.ptr))))
            say("  %-34s %8.3f ms  %8.1f GB/s  (slots of %d bytes: %d written)" % ("spiht_layer_unpack, Q = %d" % Q, ms,
                                                                                   (total + T * longest) / ms / 1e6, longest, T * longest))
        # what the layers hold
        for Q in LAYERS[1:]:
            ends = res[Q].layer_ends()
            say("tile %d, Q = %d: file bytes and PSNR (dB) after each layer: " % (t, Q)
                + ", ".join("%d %.2f" % (ends[q], psnr(P, k.decode_layered(res[Q], q + 1))) for q in range(Q)))
        for d in [d_packed, d_lens, d_maxn, d_cum, d_pic, d_plain, d_copy, d_slots, d_nbytes] + list(d_run.values()) + list(d_tab.values()):
            d.free()
        k.close()
    d_img.free()
    d_out.free()
    say("")
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
