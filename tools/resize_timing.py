#!/usr/bin/env python3
"""Resized crops (profiles/resize_timing.txt), everything in one run:
  workload  256 uint8-coded RGB pictures, sides drawn from 256 .. 1024 by a fixed seed, tiles of 128, 0.5 bit per pixel per
            tile, bior2.2, the default level of a tile; one random box per picture of 8 .. 100 % of its area and aspect
            3/4 .. 4/3, resampled to 224 x 224 float16, half of them mirrored, normalised per channel
  calls     decode_resized_crops_float of the set -- ONE array [256, 3, 224, 224] -- beside decode_windows_float of the same
            boxes, which gives 256 float16 windows of 256 sizes still to be resized
  kernel    spiht_tile_resample_set alone on the decoded float64 tiles of those boxes, beside spiht_tile_paste_set of the same
            tiles into float64 windows of the boxes and a device-to-device copy of the bytes the boxes hold
The new call's rows are compared with resize_rule of TiledCodec.decode_window for the first pictures before anything is timed.
All times: the host clock (time.perf_counter) around calls that end in a synchronise of the context; medians of R timed rounds
after a warm-up round, the forms in rotation.
Usage: python tools/resize_timing.py [rounds] [output file] [label] [pictures]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spiht_amd import _lib, px, resample  # noqa: E402
from spiht_amd.batch import DeviceArray  # noqa: E402
from spiht_amd.tiles import TiledCodec  # noqa: E402
from spiht_amd.tileset import TileSetCodec, set_tables  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else None
LABEL = sys.argv[3] if len(sys.argv) > 3 else "this build"
NPIC = int(sys.argv[4]) if len(sys.argv) > 4 else 256
WARM = 1
C3, TILE, SIZE = 3, 128, (224, 224)
TILE_BITS = TILE * TILE // 2
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ctx = _lib.default_context(0)
L = _lib.lib()
vp = C.c_void_p


def synth_u8(rng, c, H, W):
    """smooth with edges plus noise, 8 bits"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((c, H, W), np.uint8)
    for k in range(c):
        fy, fx, ph = rng.uniform(2.0, 9.0), rng.uniform(2.0, 9.0), rng.uniform(0.0, 6.28)
        v = 0.5 + 0.3 * np.sin(fy * y / H + ph) * np.cos(fx * x / W + 0.4 * k) + 0.12 * ((x + 2 * y + 31 * k) % 97 > 48)
        out[k] = np.round(np.clip(v + rng.normal(0.0, 0.004, (H, W)), 0.0, 1.0) * 255)
    return out


def timed(fns):
    """fns: {name: callable} -> {name: (median, min, max) ms}, the forms in rotation, a synchronise before and after each"""
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
    return {n: (float(np.median(v)), float(min(v)), float(max(v))) for n, v in t.items()}


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


def random_box(rng, H, W):
    """8 .. 100 % of the area at an aspect of 3/4 .. 4/3, cut to the picture"""
    area = rng.uniform(0.08, 1.0) * H * W
    aspect = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
    w, h = min(W, max(1, int(round(np.sqrt(area * aspect))))), min(H, max(1, int(round(np.sqrt(area / aspect)))))
    return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w


rng = np.random.default_rng(2026)
sizes = [(int(rng.integers(256, 1025)), int(rng.integers(256, 1025))) for _ in range(NPIC)]
pics = [synth_u8(rng, C3, H, W) for H, W in sizes]
boxes = [random_box(rng, H, W) for H, W in sizes]
flips = [bool(b & 1) for b in range(NPIC)]
tab = set_tables(sizes, TILE, TILE, list(enumerate(boxes)))
S = int(tab["s0"][-1])
box_samples = sum(C3 * h * w for _, _, h, w in boxes)
print("%d pictures; the boxes hold %d samples and meet %d tiles" % (NPIC, box_samples, S), file=sys.stderr, flush=True)

codec = TileSetCodec(C3, TILE, None, None, TILE_BITS, ctx)
res = codec.encode_u8(pics)

# ---- the new call's rows are the rule's
got = codec.decode_resized_crops_float(res, boxes, SIZE, flips, MEAN, STD, np.float16)
for b in range(min(NPIC, 4)):
    H, W = sizes[b]
    k = TiledCodec(C3, H, W, TILE, None, None, TILE_BITS * (-(-H // TILE) * -(-W // TILE)), ctx)
    want = resample.resize_rule(k.decode_window(res[b], *boxes[b]), SIZE, flips[b], MEAN, STD, np.float16)
    assert got[b].tobytes() == want.tobytes(), b
    k.close()
print("results equal", file=sys.stderr, flush=True)

tm = timed({
    "decode_resized_crops_float, one [B, 3, 224, 224]": lambda: codec.decode_resized_crops_float(res, boxes, SIZE, flips, MEAN, STD, np.float16),
    "decode_windows_float, B windows of B sizes": lambda: codec.decode_windows_float(res, boxes, np.float16),
})
out_bytes = NPIC * C3 * SIZE[0] * SIZE[1] * 2
lines = ["%s: resized crops beside the windows they are made from; host clock around synchronised calls, median (min .. max) of %d "
         "after %d warm-up round(s)" % (LABEL, R, WARM),
         "%d uint8-coded RGB pictures, sides 256 .. 1024 (seed 2026), tiles of %d, %d bits per tile; boxes of 8 .. 100 %% of the area, "
         "aspect 3/4 .. 4/3: %d samples in %d tiles -> %d x %d float16, flipped and normalised" % (NPIC, TILE, TILE_BITS, box_samples, S,
                                                                                                SIZE[0], SIZE[1]),
         "bytes downloaded: %d (resized) against %d (float16 windows)" % (out_bytes, 2 * box_samples), ""]
for n, v in tm.items():
    lines.append("  %-52s %10.2f ms  (%.2f .. %.2f)" % ((n,) + v))
print("timed the calls", file=sys.stderr, flush=True)

# ---- the kernel alone, beside the paste of the same tiles and a device-to-device copy of the boxes' bytes
rh, rw = codec.codec.geom["rec_h"], codec.codec.geom["rec_w"]
d_tiles = DeviceArray(ctx, (S, C3, rh, rw), np.float64)
ctx.memset(d_tiles.ptr, 0x3C, d_tiles.nbytes)
d_out = DeviceArray(ctx, (NPIC, C3) + SIZE, np.float16)
d_wins = DeviceArray(ctx, (box_samples,), np.float64)
d_copy = DeviceArray(ctx, (box_samples,), np.float64)
rs_rows, ps_rows = (_lib.TileSetItem * NPIC)(), (_lib.TileSetItem * NPIC)()
tabs, parts, off, woff = np.empty((NPIC, 4), np.int64), [], 0, 0
for b, (r, p, (H, W), sub, (y0, x0, h, w)) in enumerate(zip(rs_rows, ps_rows, sizes, tab["subs"], boxes)):
    for q in (r, p):
        q.H, q.W, (q.i0, q.i1, q.j0, q.j1), (q.y0, q.x0, q.wh, q.ww) = H, W, sub, (y0, x0, h, w)
    r.d_out, r.sc, r.sh, r.sw = d_out.ptr + b * C3 * SIZE[0] * SIZE[1] * 2, SIZE[0] * SIZE[1] * 2, SIZE[1] * 2, 2
    p.d_out, p.sc, p.sh, p.sw = d_wins.ptr + woff, h * w * 8, w * 8, 8
    woff += C3 * h * w * 8
    for k, (n_in, n_out, f) in enumerate(((w, SIZE[1], flips[b]), (h, SIZE[0], False))):
        t = resample.axis_table(n_in, n_out)
        start, count, wt = resample.flip_table(t) if f else t
        tabs[b, 2 * k:2 * k + 2] = off, wt.shape[1]
        parts += [start.view(np.uint8), count.view(np.uint8), wt.reshape(-1).view(np.uint8)]
        off += 8 * n_out + wt.nbytes
tables = np.concatenate(parts)
mean, std = np.asarray(MEAN), np.asarray(STD)
kernels = [
    ("spiht_tile_resample_set -> [%d, 3, %d, %d] float16" % ((NPIC,) + SIZE),
     lambda: _lib.check(L.spiht_tile_resample_set(ctx.handle, px.of_kind_id(np.float16).stream_id, NPIC, C3, rh, rw, TILE, TILE, SIZE[0],
                                                  SIZE[1], C.byref(rs_rows), vp(tabs.ctypes.data), vp(tables.ctypes.data), tables.nbytes,
                                                  vp(mean.ctypes.data), vp(std.ctypes.data), vp(d_tiles.ptr), S)),
     8 * box_samples + out_bytes),
    ("spiht_tile_paste_set of the same boxes, float64",
     lambda: _lib.check(L.spiht_tile_paste_set(ctx.handle, 8, NPIC, C3, rh, rw, TILE, TILE, C.byref(ps_rows), vp(d_tiles.ptr), S)),
     16 * box_samples),
    ("device-to-device copy of %d bytes" % (8 * box_samples),
     lambda: _lib.check(L.spiht_dev_copy(ctx.handle, vp(d_copy.ptr), vp(d_wins.ptr), 8 * box_samples)), 16 * box_samples),
]
lines += ["", "the kernel alone (ms per call of 20 queued back to back, the set calls with their table copies; GB/s = bytes of the "
          "boxes read + bytes written / time):"]
for name, fn, moved in kernels:
    v = launches(fn)
    lines.append("  %-52s %8.4f ms  %8.1f GB/s" % (name, v, moved / v / 1e6))

print("\n".join(lines))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
