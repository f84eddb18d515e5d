#!/usr/bin/env python3
"""Host-fed streams against the batched host calls (profiles/hostfed_timing.txt): 1080p RGB pictures at 0.5 bpp that start and
end in host arrays, uint8 (32 per step) and float64 (8 per step), a ring of 2 and of 3 slots.  Per case, STEPS steps after WARM
warm-up steps, each figure taken ROUNDS times in rotation within one process:
  stream    StreamEncoder / StreamDecoder: images/s from the first timed submit to the last result taken.  "copied": every
            batch is copied from a pageable array into the staging first and the results leave as EncodingResults (what
            encoder.run does); "in place": the staging is taken as filled (a decoder library that writes straight into it)
            and the results are read where they lie.  The decoder likewise: "views", the pictures read where they lie in the
            staging (next(copy=False): valid until their slot is handed out again); "copied", every step's pictures copied
            into an array the caller owns, as (a) returns them (next(), what decoder.run and decode_images* do).  "per
            picture": encode_images* / decode_images* fed one picture or stream at a time (uint8 and float64 forms)
  (a)       the loop a caller had before: BatchCodec.encode_u8 / decode_u8 (float64: encode / decode) over the same host batches
  (b)       the coding alone, on device-resident data (encode_device* / decode_device*, one wait per step)
  (c)       the page-locked copy alone, both ways, GB/s
and which of link and GPU bounds the steady step: the stream's step beside upload, coding and download taken alone.
Usage: python tools/hostfed_timing.py [output file] [steps] [rounds]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_u8  # noqa: E402
import spiht_amd  # noqa: E402
from spiht_amd import _lib  # noqa: E402
from spiht_amd.batch import BatchCodec, DeviceArray  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 16
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
WARM = 2
c, H, W = 3, 1080, 1920
MB = int(H * W * 0.5)
NBATCH = 3   # distinct host batches, taken in turn
ctx = _lib.default_context(0)
s = spiht_amd.SpihtSettings()
base = [synth_u8(1000 + i, c, H, W) for i in range(8)]
lines = ["host-fed streams against the batched host calls: %dx%d RGB, bior2.2 reflect, level None, %d bits (0.5 bpp);"
         % (H, W, MB), "%d steps after %d warm-up steps, %d rounds in rotation; images/s: median (min .. max)" % (STEPS, WARM, ROUNDS), ""]


def host_batches(dtype, B):
    out = []
    for k in range(NBATCH):
        P = np.empty((B, c, H, W), np.uint8)
        for b in range(B):
            v = np.roll(base[(b + k) % 8], 7 * (b // 8) + 13 * k, axis=2)
            P[b] = v[:, ::-1, :] if (b // 8) & 1 else v
        out.append(P if dtype == np.uint8 else P / 255.0)
    return out


def spread(v):
    return "%9.1f (%8.1f .. %8.1f)" % (np.median(v), min(v), max(v))


def case(dtype, B, depth):
    name = np.dtype(dtype).name
    batches = host_batches(dtype, B)
    codec = BatchCodec(c, H, W, s, None, MB, ctx=ctx)
    enc_a = codec.encode_u8 if dtype == np.uint8 else codec.encode
    dec_a = codec.decode_u8 if dtype == np.uint8 else codec.decode
    results = [enc_a(p) for p in batches]
    max_bytes = max(len(r.encoded_bytes) for rs in results for r in rs)
    n_img = STEPS * B
    fig = {k: [] for k in ("enc_copied", "enc_inplace", "enc_each", "dec", "dec_copied", "dec_each", "a_enc", "a_dec", "b_enc", "b_dec", "h2d", "d2h")}
    # one stream alive at a time: the page-locked pool hands out 4 GiB, a float64 stream of depth 3 holds 1.2 of them
    live = {}

    def stream(kind):
        if kind not in live:
            for v in live.values():
                v.close()
            live.clear()
            if kind == "enc":
                live[kind] = spiht_amd.StreamEncoder(c, H, W, s, None, MB, dtype=dtype, batch=B, depth=depth, ctx=ctx)
            elif kind == "dec":
                live[kind] = spiht_amd.StreamDecoder(c, H, W, s, None, dtype=dtype, batch=B, depth=depth, ctx=ctx, max_bytes=max_bytes)
        return live.get(kind)

    # the streams give what (a) gives
    got = list(stream("enc").run(batches[:1]))[0]
    assert [(r.encoded_bytes, r.max_n) for r in got] == [(r.encoded_bytes, r.max_n) for r in results[0]]
    assert np.array_equal(list(stream("dec").run([results[0]]))[0], dec_a(results[0]))

    def stream_enc(copied):
        enc = stream("enc")
        t0 = None
        for k in range(WARM + STEPS):
            if k == WARM:
                while enc.pending():
                    enc.next()
                t0 = time.perf_counter()
            if enc.pending() == depth:
                enc.next(raw=not copied)
            buf = enc.input()
            if copied:
                buf[:] = batches[k % NBATCH]
            enc.submit(B)
        while enc.pending():
            enc.next(raw=not copied)
        return n_img / (time.perf_counter() - t0)

    flat_pics = [p for k in range(WARM + STEPS) for p in batches[k % NBATCH]]
    flat_res = [r for k in range(WARM + STEPS) for r in results[k % NBATCH]]
    enc_each_fn = spiht_amd.encode_images_u8 if dtype == np.uint8 else spiht_amd.encode_images
    dec_each_fn = spiht_amd.decode_images_u8 if dtype == np.uint8 else spiht_amd.decode_images

    def each(gen):   # the conveniences: one item in, one out; timed from the result that ends the warm-up steps
        stream("none")   # (they make a stream of their own)
        t0 = None
        for i, _ in enumerate(gen):
            if i == WARM * B - 1:
                t0 = time.perf_counter()
        return n_img / (time.perf_counter() - t0)

    def stream_dec(copy=False):
        dec = stream("dec")
        t0 = None
        for k in range(WARM + STEPS):
            if k == WARM:
                while dec.pending():
                    dec.next(copy=copy)
                t0 = time.perf_counter()
            if dec.pending() == depth:
                dec.next(copy=copy)
            dec.put(results[k % NBATCH])
        while dec.pending():
            dec.next(copy=copy)
        return n_img / (time.perf_counter() - t0)

    def loop_a(fn, items):
        for k in range(WARM):
            fn(items[k % NBATCH])
        t0 = time.perf_counter()
        for k in range(STEPS):
            fn(items[k % NBATCH])
        return n_img / (time.perf_counter() - t0)

    g = codec.geom
    d_img = DeviceArray(ctx, (B, c, H, W), dtype)
    d_rec = DeviceArray(ctx, (B, c, H, W) if dtype == np.uint8 else (B, c, g["rec_h"], g["rec_w"]), dtype)
    d_out = DeviceArray(ctx, (B, codec.slot_stride), np.uint8)
    d_nb, d_ny, d_mn = DeviceArray(ctx, (B,), np.uint64), DeviceArray(ctx, (B,), np.uint64), DeviceArray(ctx, (B,), np.uint8)
    d_img.upload(batches[0])

    def dev_enc():
        if dtype == np.uint8:
            codec.encode_device_u8(d_img.ptr, B, d_out.ptr, d_nb.ptr, d_mn.ptr)
        else:
            codec.encode_device(d_img.ptr, B, d_out.ptr, d_nb.ptr, d_mn.ptr)
        ctx.synchronize()

    def dev_dec():
        if dtype == np.uint8:
            codec.decode_device_u8(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_rec.ptr)
        else:
            codec.decode_device(d_out.ptr, d_ny.ptr, d_mn.ptr, B, d_rec.ptr)
        ctx.synchronize()

    def loop_b(fn):
        for _ in range(WARM):
            fn()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        return n_img / (time.perf_counter() - t0)

    pinned = _lib.result_array(batches[0].shape, dtype)
    pinned[:] = batches[0]
    pin_rec = _lib.result_array(d_rec.shape, dtype)

    def copy_rate(fn, nbytes):
        fn()
        t0 = time.perf_counter()
        for _ in range(4):
            fn()
        return 4 * nbytes / (time.perf_counter() - t0) / 1e9

    dev_enc()
    codec.nbits_to_nbytes(d_nb.ptr, B, d_ny.ptr)
    ctx.synchronize()
    runs = {
        "enc_copied": lambda: stream_enc(True), "enc_inplace": lambda: stream_enc(False), "dec": stream_dec, "dec_copied": lambda: stream_dec(True),
        "enc_each": lambda: each(enc_each_fn(flat_pics, s, None, MB, batch=B, depth=depth, ctx=ctx)),
        "dec_each": lambda: each(dec_each_fn(flat_res, s, batch=B, depth=depth, ctx=ctx, max_bytes=max_bytes)),
        "a_enc": lambda: loop_a(enc_a, batches), "a_dec": lambda: loop_a(dec_a, results),
        "b_enc": lambda: loop_b(dev_enc), "b_dec": lambda: loop_b(dev_dec),
        "h2d": lambda: copy_rate(lambda: ctx.upload(d_img.ptr, pinned), pinned.nbytes),
        "d2h": lambda: copy_rate(lambda: ctx.download(pin_rec, d_rec.ptr), pin_rec.nbytes),
    }
    order = list(runs)
    for r in range(ROUNDS):
        for k in order[r % len(order):] + order[:r % len(order)]:
            fig[k].append(runs[k]())
    stream("none")
    for d in (d_img, d_rec, d_out, d_nb, d_ny, d_mn):
        d.free()

    med = {k: float(np.median(v)) for k, v in fig.items() if v}
    pic_in, pic_out = batches[0].nbytes / 1e9, pin_rec.nbytes / 1e9
    stream_bytes = sum(len(r.encoded_bytes) for r in results[0]) / 1e9
    out = ["%s pictures, %d per step, depth %d  (a step: %.1f MB of pictures, %.2f MB of streams)" % (name, B, depth, pic_in * 1e3, stream_bytes * 1e3)]
    out.append("  encode  stream, copied   %s   over (a): %.2f  (%.2f .. %.2f)" % (
        spread(fig["enc_copied"]), med["enc_copied"] / med["a_enc"], min(fig["enc_copied"]) / max(fig["a_enc"]), max(fig["enc_copied"]) / min(fig["a_enc"])))
    out.append("          stream, in place %s   over (a): %.2f" % (spread(fig["enc_inplace"]), med["enc_inplace"] / med["a_enc"]))
    out.append("          per picture      %s   over (a): %.2f" % (spread(fig["enc_each"]), med["enc_each"] / med["a_enc"]))
    out.append("          (a) batched host %s" % spread(fig["a_enc"]))
    out.append("          (b) coding alone %s" % spread(fig["b_enc"]))
    out.append("  decode  stream, views    %s   over (a): %.2f  (%.2f .. %.2f)" % (
        spread(fig["dec"]), med["dec"] / med["a_dec"], min(fig["dec"]) / max(fig["a_dec"]), max(fig["dec"]) / min(fig["a_dec"])))
    out.append("          stream, copied   %s   over (a): %.2f  (%.2f .. %.2f)" % (
        spread(fig["dec_copied"]), med["dec_copied"] / med["a_dec"], min(fig["dec_copied"]) / max(fig["a_dec"]), max(fig["dec_copied"]) / min(fig["a_dec"])))
    out.append("          per stream       %s   over (a): %.2f" % (spread(fig["dec_each"]), med["dec_each"] / med["a_dec"]))
    out.append("          (a) batched host %s" % spread(fig["a_dec"]))
    out.append("          (b) coding alone %s" % spread(fig["b_dec"]))
    out.append("  (c) page-locked copy alone: host to device %.1f GB/s, device to host %.1f GB/s" % (med["h2d"], med["d2h"]))
    # the steady step beside its parts taken alone (ms per step of B pictures)
    for what, key, up, code, down in (("encode", "enc_inplace", pic_in / med["h2d"], B / med["b_enc"], stream_bytes / med["d2h"]),
                                      ("decode", "dec", stream_bytes / med["h2d"], B / med["b_dec"], pic_out / med["d2h"])):
        step = B / med[key] * 1e3
        parts = {"upload": up * 1e3, "coding": code * 1e3, "download": down * 1e3}
        top = max(parts, key=parts.get)
        near = "the maximum" if abs(step - parts[top]) < abs(step - sum(parts.values())) else "the SUM"
        out.append("  %s step %.2f ms; alone: upload %.2f, coding %.2f, download %.2f ms -> max %.2f (%s: %s-bound), sum %.2f: nearer %s"
                   % (what, step, parts["upload"], parts["coding"], parts["download"], parts[top], top,
                      "GPU" if top == "coding" else "link", sum(parts.values()), near))
    out.append("")
    return out


for dtype, B in ((np.uint8, 32), (np.float64, 8)):
    for depth in (2, 3):
        lines += case(dtype, B, depth)
        print("\n".join(lines[-16:]), flush=True)
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
