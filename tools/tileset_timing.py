#!/usr/bin/env python3
"""Picture sets (profiles/tileset_timing.txt), everything in one run, the set call beside the loop over per-size codecs:
  workload  256 uint8 RGB pictures, sides drawn from 256 .. 1024 by a fixed seed, tiles of 128, 0.5 bit per pixel per tile,
            bior2.2, the default level of a tile
  encode    TileSetCodec.encode_u8 of the set beside the loop over cached per-size TiledCodec.encode_u8 calls of the same
            pictures, host array to host array; encode_device of the set beside the loop over TiledCodec.encode_device with the
            pixels resident in HBM (one synchronise behind the whole set either way)
  crops     decode_crops_float(results, origins, (224, 224), float16) of 256 random crops beside the loop over
            TiledCodec.decode_window_float and a stack on the host
  kernels   spiht_tile_cut_set / spiht_tile_paste_set of the whole set alone beside spiht_tile_cut_u8 / spiht_tile_paste_u8 of
            ONE picture of the same bytes and a device-to-device copy of those bytes
The results of the two ways are compared before anything is timed.  All times: the host clock (time.perf_counter) around calls
that end in a synchronise of the context; medians of R timed rounds after warm-up rounds, the forms in rotation.
Usage: python tools/tileset_timing.py [rounds] [output file] [label] [pictures]"""
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
from spiht_amd.tileset import TileSetCodec, set_tables  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else None
LABEL = sys.argv[3] if len(sys.argv) > 3 else "this build"
NPIC = int(sys.argv[4]) if len(sys.argv) > 4 else 256
WARM = 1
C3, TILE, CROP = 3, 128, (224, 224)
TILE_BITS = TILE * TILE // 2
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


def device(arr):
    d = DeviceArray(ctx, arr.shape, arr.dtype)
    d.upload(np.ascontiguousarray(arr))
    return d


rng = np.random.default_rng(2026)
sizes = [(int(rng.integers(256, 1025)), int(rng.integers(256, 1025))) for _ in range(NPIC)]
pics = [synth_u8(rng, C3, H, W) for H, W in sizes]
origins = [(int(rng.integers(0, H - CROP[0] + 1)), int(rng.integers(0, W - CROP[1] + 1))) for H, W in sizes]
tab = set_tables(sizes, TILE, TILE, [(p, (y0, x0) + CROP) for p, (y0, x0) in enumerate(origins)])
NT, S = int(tab["tile0"][-1]), int(tab["s0"][-1])
nbytes = sum(P.nbytes for P in pics)
print("%d pictures, %d bytes, %d tiles; the crops meet %d tiles" % (NPIC, nbytes, NT, S), file=sys.stderr, flush=True)

codec = TileSetCodec(C3, TILE, None, None, TILE_BITS, ctx)
per = {}
for H, W in sizes:
    if (H, W) not in per:
        per[(H, W)] = TiledCodec(C3, H, W, TILE, None, None, TILE_BITS * (-(-H // TILE) * -(-W // TILE)), ctx)
loop = [per[s] for s in sizes]

# ---- the two ways give the same bytes
res = codec.encode_u8(pics)
for k, P, r in zip(loop, pics, res):
    w = k.encode_u8(P)
    assert (w.nbytes, w.max_n, w.encoded_bytes) == (r.nbytes, r.max_n, r.encoded_bytes)
crops = codec.decode_crops_float(res, origins, CROP, np.float16)
for b, (k, r, (y0, x0)) in enumerate(zip(loop, res, origins)):
    assert np.array_equal(crops[b].view(np.uint16), k.decode_window_float(r, y0, x0, *CROP, np.float16).view(np.uint16))
print("results equal", file=sys.stderr, flush=True)

# ---- the pixels resident in HBM
d_pics = [device(P[None]) for P in pics]
slot = codec.codec.slot_stride
d_packed, d_lens, d_maxn = DeviceArray(ctx, (NT * slot,), np.uint8), DeviceArray(ctx, (NT,), np.uint32), DeviceArray(ctx, (NT,), np.uint8)
rows = [(d.ptr, H, W, None) for d, (H, W) in zip(d_pics, sizes)]


class Slice:
    """a part of a DeviceArray: the loop's calls write picture p's rows of the same three arrays"""

    def __init__(self, base, offset, nbytes):
        self.ptr, self.nbytes = base.ptr + offset, nbytes


def loop_encode_device():
    for p, (k, d) in enumerate(zip(loop, d_pics)):
        t0 = int(tab["tile0"][p])
        k.encode_device(d, 1, Slice(d_packed, t0 * slot, k.T * slot), Slice(d_lens, 4 * t0, 4 * k.T), Slice(d_maxn, t0, k.T))


def loop_crops():
    return np.stack([k.decode_window_float(r, y0, x0, *CROP, np.float16) for k, r, (y0, x0) in zip(loop, res, origins)])


tm = timed({
    "encode, host to host: the set call": lambda: codec.encode_u8(pics),
    "encode, host to host: the loop": lambda: [k.encode_u8(P) for k, P in zip(loop, pics)],
    "encode, pixels in HBM: the set call": lambda: codec.encode_device(rows, d_packed, d_lens, d_maxn, np.uint8),
    "encode, pixels in HBM: the loop": loop_encode_device,
    "crops 224x224 float16: the set call": lambda: codec.decode_crops_float(res, origins, CROP, np.float16),
    "crops 224x224 float16: the loop + stack": loop_crops,
})
lines = ["%s: picture sets beside the loop over per-size codecs; host clock around synchronised calls, median (min .. max) of %d after %d "
         "warm-up round(s)" % (LABEL, R, WARM),
         "%d uint8 RGB pictures, sides 256 .. 1024 (seed 2026): %d bytes, %d tiles of %d, %d bits per tile; %d distinct sizes; the %d "
         "crops of %dx%d meet %d tiles" % (NPIC, nbytes, NT, TILE, TILE_BITS, len(per), NPIC, CROP[0], CROP[1], S), ""]
names = list(tm)
for a, b in zip(names[0::2], names[1::2]):
    for n in (a, b):
        lines.append("  %-42s %10.2f ms  (%.2f .. %.2f)" % ((n,) + tm[n]))
    lines.append("  %-42s %10.2f x" % ("loop / set", tm[b][0] / tm[a][0]))
print("timed the forms", file=sys.stderr, flush=True)

# ---- the two kernels alone, beside the one-picture copies of the same bytes and a device-to-device copy
side = int(np.sqrt(nbytes / C3))
Hb, Wb = side, nbytes // (C3 * side)
big = DeviceArray(ctx, (C3, Hb, Wb), np.uint8)
ctx.memset(big.ptr, 7, big.nbytes)
gy, gx = spiht_amd.tile_grid(Hb, Wb, TILE, TILE)
d_tiles = DeviceArray(ctx, (max(NT, gy * gx) * C3 * TILE * TILE,), np.uint8)
d_copy = DeviceArray(ctx, (nbytes,), np.uint8)
cut_rows = (_lib.TileSetPic * NPIC)()
for r, d, (H, W) in zip(cut_rows, d_pics, sizes):
    r.d_img, r.sc, r.sh, r.sw, r.H, r.W = d.ptr, H * W, W, 1, H, W
d_wins = [DeviceArray(ctx, (C3, H, W), np.uint8) for H, W in sizes]
paste_rows = (_lib.TileSetItem * NPIC)()
for r, d, (H, W) in zip(paste_rows, d_wins, sizes):
    r.d_out, r.sc, r.sh, r.sw, r.H, r.W = d.ptr, H * W, W, 1, H, W
    r.i0, r.i1, r.j0, r.j1 = 0, -(-H // TILE), 0, -(-W // TILE)
    r.y0, r.x0, r.wh, r.ww = 0, 0, H, W
kernels = [
    ("spiht_tile_cut_set, %d pictures" % NPIC,
     lambda: _lib.check(L.spiht_tile_cut_set(ctx.handle, 1, NPIC, C3, TILE, TILE, C.byref(cut_rows), vp(d_tiles.ptr)))),
    ("spiht_tile_cut_u8, one %d x %d picture" % (Hb, Wb),
     lambda: _lib.check(L.spiht_tile_cut_u8(ctx.handle, vp(big.ptr), None, 1, C3, Hb, Wb, TILE, TILE, vp(d_tiles.ptr)))),
    ("spiht_tile_paste_set, %d whole pictures" % NPIC,
     lambda: _lib.check(L.spiht_tile_paste_set(ctx.handle, 1, NPIC, C3, TILE, TILE, TILE, TILE, C.byref(paste_rows), vp(d_tiles.ptr), NT))),
    ("spiht_tile_paste_u8, one %d x %d picture" % (Hb, Wb),
     lambda: _lib.check(L.spiht_tile_paste_u8(ctx.handle, vp(d_tiles.ptr), C3, TILE, TILE, Hb, Wb, TILE, TILE, 0, gy, 0, gx, 0, 0, Hb,
                                              Wb, vp(big.ptr), None))),
    ("device-to-device copy of %d bytes" % nbytes,
     lambda: _lib.check(L.spiht_dev_copy(ctx.handle, vp(d_copy.ptr), vp(big.ptr), min(nbytes, big.nbytes)))),
]
lines += ["", "the kernels alone (ms per call of 20 queued back to back, the set calls with their table copies; GB/s = picture bytes "
          "written + as many read / time):"]
for name, fn in kernels:
    v = launches(fn)
    lines.append("  %-50s %8.4f ms  %8.1f GB/s" % (name, v, 2 * nbytes / v / 1e6))

print("\n".join(lines))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
