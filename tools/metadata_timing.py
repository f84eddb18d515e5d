#!/usr/bin/env python3
"""decode_with_metadata of many pictures (profiles/metadata_timing.txt): B single calls (spiht.decode_with_metadata in a
loop: the stream from the host, the table and the array back to the host) against one batched call on device-resident
streams (BatchCodec.decode_with_metadata_device on the encoder's own slots, nbits_to_nbytes and max_n; tables and arrays
stay on the device).  Sizes:
  1080p   64 distinct RGB 1080x1920 pictures at 0.5 bpp
  256     1024 distinct RGB 256x256 pictures at 1 bpp
Host timers around work that ends in a device synchronize, after one warm-up of each form; median of R runs, the forms
alternating within a run.
Usage: python tools/metadata_timing.py [--sizes 1080p,256] [--runs R] [--out FILE]
       python tools/metadata_timing.py --profile SIZE    set-up, then two batched calls (under rocprofv3 --kernel-trace --stats)
       python tools/metadata_timing.py --split RESULTS.db [--calls 2]  the kernel time of such a run per batched call:
                                                         traced decode, fills, keys, rows, sort, fold"""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"1080p": (3, 1080, 1920, 0.5, 64), "256": (3, 256, 256, 1.0, 1024)}


def setup(name):
    """B distinct pictures encoded on the device -> (codec, B, device buffers, host streams)"""
    from bench import synth_u8
    import spiht_amd
    from spiht_amd import _lib
    from spiht_amd.batch import BatchCodec, DeviceArray
    c, H, W, bpp, B = SIZES[name]
    ctx = _lib.default_context(0)
    codec = BatchCodec(c, H, W, spiht_amd.SpihtSettings(), None, int(H * W * bpp), ctx=ctx)
    g, ss = codec.geom, codec.slot_stride
    base = [synth_u8(1000 + i, c, H, W) for i in range(8)]
    d_img = DeviceArray(ctx, (B, c, H, W), np.float64)
    for b in range(B):  # 8 generated pictures, each shifted and mirrored into B / 8 variants
        v = np.roll(base[b % 8], 7 * (b // 8), axis=2)
        d_img.upload((v[:, ::-1, :] if (b // 8) & 1 else v) / 255.0, offset_bytes=b * c * H * W * 8)
    d = dict(out=DeviceArray(ctx, (B, ss), np.uint8), nbits=DeviceArray(ctx, (B,), np.uint64),
             nbytes=DeviceArray(ctx, (B,), np.uint64), maxn=DeviceArray(ctx, (B,), np.uint8))
    codec.encode_device(d_img.ptr, B, d["out"].ptr, d["nbits"].ptr, d["maxn"].ptr)
    codec.nbits_to_nbytes(d["nbits"].ptr, B, d["nbytes"].ptr)
    ctx.synchronize()
    d_img.free()
    d["meta_rows"] = 8 * ss + 1
    d["meta"] = DeviceArray(ctx, (B, d["meta_rows"], 8), np.int32)
    d["rec"] = DeviceArray(ctx, (B, c, g["enc_h"], g["enc_w"]), np.int32)
    slots, nbytes, maxn = d["out"].download(), d["nbytes"].download(), d["maxn"].download()
    streams = [(slots[b, :int(nbytes[b])].tobytes(), int(maxn[b])) for b in range(B)]
    return codec, B, d, streams


def batched(codec, B, d):
    codec.decode_with_metadata_device(d["out"].ptr, d["nbytes"].ptr, d["maxn"].ptr, B, d["meta"].ptr, d["meta_rows"],
                                      d_rec=d["rec"].ptr)
    codec.ctx.synchronize()


def measure(name, runs):
    import spiht_amd
    from spiht_amd.spiht_wrapper import _metadata_boxes
    codec, B, d, streams = setup(name)
    c, H, W, bpp, _ = SIZES[name]
    g, ctx = codec.geom, codec.ctx
    top, other = _metadata_boxes(H, W, codec.settings, g)
    args = (c, g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"], top, other)

    def single():
        for data, n in streams:
            spiht_amd.spiht.decode_with_metadata(data, n, *args)

    forms = [("single calls", single), ("one batched call", lambda: batched(codec, B, d))]
    for _, f in forms:  # warm-up
        f()
    # the batched tables against the single call, first and last picture
    for b in (0, B - 1):
        rows = 8 * len(streams[b][0]) + 1
        m = np.empty((rows, 8), np.int32)
        ctx.download(m, d["meta"].ptr + b * d["meta_rows"] * 32)
        r1, m1 = spiht_amd.spiht.decode_with_metadata(streams[b][0], streams[b][1], *args)
        assert np.array_equal(m, m1), "picture %d: the batched table differs from the single call's" % b
    t = {k: [] for k, _ in forms}
    for _ in range(runs):
        for k, f in forms:
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    nb = np.array([len(s[0]) for s in streams])
    lines = ["%s: %d RGB %dx%d pictures at %g bpp (bior2.2, reflect, level None): streams %d .. %d bytes, slot %d bytes, "
             "%d rows per table (%.1f MB)" % (name, B, H, W, bpp, nb.min(), nb.max(), codec.slot_stride, d["meta_rows"],
                                              d["meta_rows"] * 32 / 1e6),
             "  per picture on the device: trace + sort buffers %.1f MB (21 bytes a row), table %.1f MB"
             % (21 * d["meta_rows"] / 1e6, 32 * d["meta_rows"] / 1e6)]
    base = np.median(t[forms[0][0]])
    for k, _ in forms:
        med = float(np.median(t[k]))
        lines.append("  %-40s %9.2f ms  (%7.3f ms a picture, %5.1fx)   runs: %s"
                     % (k, med, med / B, base / med, " ".join("%.2f" % x for x in t[k])))
    return lines


def split(path, calls):
    """kernel time per batched call from the database of a rocprofv3 --kernel-trace run of --profile (its default rocpd
    output): the kernels that start after the set-up's last one (k_nbits_to_nbytes), by group"""
    import sqlite3
    groups = [("traced decode (k_decode<true>)", ("k_decode",)), ("fills (act, decoded arrays)", ("fill", "memset")),
              ("keys (k_meta_keys_batch)", ("k_meta_keys_batch",)), ("rows (k_meta_rows_batch)", ("k_meta_rows_batch",)),
              ("sort (rocPRIM)", ("rocprim",)), ("fold (k_meta_fold_batch)", ("k_meta_fold_batch",))]
    con = sqlite3.connect(path)
    rows = con.execute("select name, start, end, duration from kernels order by start").fetchall()
    t0 = max(r[2] for r in rows if "k_nbits_to_nbytes" in r[0])
    tot = {k: 0.0 for k, _ in groups}
    other = 0.0
    for name, start, _, ns in rows:
        if start < t0:
            continue
        for k, keys in groups:
            if any(x in name for x in keys):
                tot[k] += ns
                break
        else:
            other += ns
    s = sum(tot.values()) + other
    lines = ["  kernel time per batched call (rocprofv3 --kernel-trace, %d calls):" % calls]
    for k, _ in groups + [("other", ())]:
        v = tot.get(k, other)
        lines.append("    %-34s %9.3f ms  %5.1f %%" % (k, v / calls / 1e6, 100 * v / s if s else 0))
    lines.append("    %-34s %9.3f ms" % ("sum", s / calls / 1e6))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,256")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    ap.add_argument("--split", default=None)
    ap.add_argument("--calls", type=int, default=2)
    a = ap.parse_args()
    if a.split is not None:
        lines = split(a.split, a.calls)
    elif a.profile:
        codec, B, d, _ = setup(a.profile)
        for _ in range(2):
            batched(codec, B, d)
        lines = ["profiled: %s, 2 batched calls" % a.profile]
    else:
        lines = []
        for name in a.sizes.split(","):
            lines += measure(name, a.runs) + [""]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
