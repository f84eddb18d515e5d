"""Cases of the colour tests (no GPU; nothing in here is a test): the host build of the colour kernels' power function, the
colour model change of one pixel restated in numpy, and the inputs at which either can go wrong.

The device kernel (csrc/dwt_device.h: color3_px, over csrc/spow.h) is a fixed sequence of correctly rounded IEEE operations --
add, multiply, fma, rint, ldexp, integer work -- so the device must give, bit for bit, what the same header gives on the host
(tests/native/spow_probe.c, built without multiply-add contraction) inside the same three matrix sums (color3_rule: elementwise
numpy, which does not contract).  tests/test_gpu_colour.py holds the device to that; tests/test_colour_cases.py holds the host
build to 60-digit arithmetic and these sets to their purpose."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# spiht_launch_color3: ceil(npix / 1024) blocks of 256 threads -- one thread, both sides of one block, both sides of four
# trips of the grid-stride loop, a ragged last block
NPIX = (1, 255, 256, 257, 1023, 1024, 1025, 4097)
EXPONENTS = (0.43, 1 / 0.43)                       # the two directions of the IPT transform
DEVICE_EXPONENTS = (0.43, 1 / 0.43, 1 / 3.0, 1.0, 2.3)
TABLE_EXPONENTS = (-1022, -600, -452, -20, -8, -3, -1, 0, 1, 2, 7, 300, 1023)
DBL_MAX = float(np.finfo(np.float64).max)
IDENTITY = np.eye(3)

_probe = None


def host_spow():
    """csrc/spow.h compiled for the CPU with the gcc line of test_oracle._spow_probe -> vectorised spow(x, p) (float64 in and out,
    any shape)"""
    global _probe
    if _probe is None:
        tmp = tempfile.mkdtemp(prefix="spow_probe_")
        atexit.register(shutil.rmtree, tmp, True)
        so = os.path.join(tmp, "spow_probe.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-std=c11", "-ffp-contract=off", "-shared", "-o", so,
                               os.path.join(HERE, "native", "spow_probe.c"), "-lm"])
        L = C.CDLL(so)
        L.probe_spow_n.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_long]
        L.probe_spow_n.restype = None
        _probe = L

    def spow(x, p):
        x = np.ascontiguousarray(x, np.float64)
        out = np.empty_like(x)
        _probe.probe_spow_n(x.ctypes.data, float(p), out.ctypes.data, x.size)
        return out
    return spow


def color3_rule(u, A, M, p, spow):
    """color3_px in numpy for u [..., 3, n]: the three sums in the kernel's order, each product and each sum rounded on its own"""
    u = np.asarray(u, np.float64)
    A, M = np.asarray(A, np.float64).reshape(3, 3), np.asarray(M, np.float64).reshape(3, 3)
    u0, u1, u2 = u[..., 0, :], u[..., 1, :], u[..., 2, :]
    with np.errstate(all="ignore"):
        v = [spow((u0 * A[r, 0] + u1 * A[r, 1]) + u2 * A[r, 2], p) for r in range(3)]
        w = [(v[0] * M[r, 0] + v[1] * M[r, 1]) + v[2] * M[r, 2] for r in range(3)]
    return np.stack(w, axis=-2)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(got, want):
    """every bit equal, a NaN standing for any NaN -> bool array"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def assert_same_bits(got, want, what):
    ok = same_bits(got, want)
    if not ok.all():
        k = np.argwhere(~ok)[0]
        g, w = float(np.asarray(got)[tuple(k)]), float(np.asarray(want)[tuple(k)])
        raise AssertionError("%s: %d of %d values differ, first at %s: got %s (%r), want %s (%r)"
                             % (what, int((~ok).sum()), ok.size, tuple(int(v) for v in k), g.hex(), g, w.hex(), w))


def table_interval(x):
    """i = mantissa >> 46 of spow_pos (for a subnormal: of x * 2^54, as the header scales it)"""
    x = np.abs(np.asarray(x, np.float64))
    with np.errstate(over="ignore"):
        x = np.where(x < 2.0 ** -1022, x * 2.0 ** 54, x)
    return ((bits(x) & np.uint64(0xFFFFFFFFFFFFF)) >> np.uint64(46)).astype(np.int64)


def _from_fields(e, mant):
    return np.array([((e + 1023) << 52) | m for m in mant], np.uint64).view(np.float64)


def fixed_power_inputs():
    """name -> positive float64 values: the fixed part of power_inputs()"""
    ends = []
    for i in range(64):
        ends += [i << 46, (i << 46) + 1, (i << 46) + (1 << 45), ((i + 1) << 46) - 1]
    sets = {"table": np.concatenate([_from_fields(e, ends) for e in TABLE_EXPONENTS])}
    k = np.arange(1, 40, dtype=np.float64)
    sets["near_one"] = np.concatenate([1.0 + k * 2.0 ** -52, 1.0 - k * 2.0 ** -53])
    sets["extremes"] = np.array([5e-324, 1e-323, 1.5 * 2.0 ** -1060, 2.0 ** -1023, 2.0 ** -1022 - 5e-324, DBL_MAX])
    # with p = 1 / 0.43 these give results in and just under the subnormal range
    sets["tiny_result"] = np.array([f * 2.0 ** -e for e in range(436, 466) for f in (1.0, 1.3, 1.9)])
    sets["grid8"] = np.arange(1, 256) / 255                     # what the 8- and 16-bit pixel kinds produce
    sets["grid16"] = np.arange(1, 65536, 257) / 65535
    return sets


def random_power_inputs():
    """seeded values in the ranges tests/test_oracle.py::test_colour_power_function_accuracy draws from"""
    rng, n = np.random.default_rng(11), 600
    return np.concatenate([rng.uniform(1e-6, 1e-3, n), rng.uniform(1e-3, 1.0, n), rng.uniform(1, 4, n),
                           2.0 ** rng.integers(-200, 200, n) * rng.uniform(1, 2, n), 1 + rng.uniform(-1e-3, 1e-3, n)])


def power_inputs():
    """the positive float64 values where x^p can go wrong: both ends, the next value and the middle of each of the 64 table
    intervals at thirteen exponents, the neighbours of 1, the smallest and the largest numbers, inputs whose result is subnormal,
    the integer pixel grids, and seeded random values"""
    return np.concatenate(list(fixed_power_inputs().values()) + [random_power_inputs()])


def pixel_inputs():
    """name -> RGB-side pixels [3, n] for the real matrices"""
    rng, n = np.random.default_rng(12), 3000
    g8, g16 = np.arange(256) / 255, np.arange(0, 65536, 257) / 65535
    g16 = np.concatenate([g16, rng.integers(0, 65536, 256) / 65535])
    sets = {"uniform": rng.random((3, n))}
    sets["grid8"] = np.stack([g8, g8[rng.permutation(256)], g8[rng.permutation(256)]])
    sets["grid8_grey"] = np.stack([g8, g8, g8])
    sets["grid16"] = np.stack([g16, g16[rng.permutation(512)], g16[rng.permutation(512)]])
    sets["grid_mixed"] = np.stack([g8[rng.integers(0, 256, 512)], g16, rng.random(512)])
    corners = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], np.float64).T  # exact 0 and 1, every combination
    part = rng.random((3, 64))                                                                  # ... and beside other values
    for k in range(64):
        for ch in range(3):
            if (k >> (2 * ch)) & 3 < 2:
                part[ch, k] = (k >> (2 * ch)) & 1
    sets["zero_one"] = np.concatenate([corners, part], axis=1)
    sets["negative"] = -rng.uniform(0, 0.5, (3, n // 2))
    sets["negative"][rng.integers(0, 3, n // 4), np.arange(n // 4)] = rng.random(n // 4)          # one channel back inside
    sets["above_one"] = 4.0 - rng.uniform(0, 3, (3, n // 2))
    sets["tiny"] = rng.uniform(1, 9.99, (3, 600)) * 1e-300 * rng.choice([1.0, -1.0], (3, 600))
    sub = (rng.integers(1, 1 << 52, (3, 600)).astype(np.uint64) >> rng.integers(0, 52, (3, 600)).astype(np.uint64)) | np.uint64(1)
    sets["subnormal"] = sub.view(np.float64) * rng.choice([1.0, -1.0], (3, 600))
    sets["subnormal"][:, :4] = np.array([[5e-324, -5e-324, 2.0 ** -1023, 2.0 ** -1022 - 5e-324]] * 3)
    return {k: np.ascontiguousarray(v, np.float64) for k, v in sets.items()}


UNIT_SETS = ("uniform", "grid8", "grid8_grey", "grid16", "grid_mixed", "zero_one")  # the part of pixel_inputs() inside [0, 1]


def back_inputs(spow):
    """name -> IPT-side pixels [3, n] for the way back: pixel_inputs() through color3_rule with the matrices now selected, and
    the same with P and T scaled by 1.5 -- colours outside the gamut.  (Measured: that scale alone turns no LMS value of an
    in-gamut pixel negative; the negative LMS values a low-rate decode hands the inverse colour change come from the triples of
    the negative, tiny and subnormal pixels, some thousands, and from "coarse": the triples of dark pixels, uniform in [0, 0.05),
    with an error of a coarse quantiser's size, +-0.2, on every channel.)"""
    from spiht_amd import color_models
    A, M, p = color_models._params("RGB", "IPT")
    out = {}
    for name, rgb in pixel_inputs().items():
        ipt = color3_rule(rgb, A, M, p, spow)
        out[name] = ipt
        out[name + "_wide"] = ipt * np.array([[1.0], [1.5], [1.5]])
    dark = color3_rule(pixel_inputs()["uniform"] * 0.05, A, M, p, spow)
    out["coarse"] = dark + np.random.default_rng(14).uniform(-0.2, 0.2, dark.shape)
    return out


def route_pictures():
    """two 3-channel pictures, (33, 47) and (67, 131), of values the routes never saw: in [0, 1], negative, above 1, of magnitude
    1e-300, and patches of zero"""
    rng, pics = np.random.default_rng(13), []
    for h, w in ((33, 47), (67, 131)):
        p = rng.random((3, h, w))
        kind = rng.integers(0, 8, (h, w))
        p[:, kind == 0] = -rng.uniform(0, 0.5, (3, int((kind == 0).sum())))
        p[:, kind == 1] = 4.0 - rng.uniform(0, 3, (3, int((kind == 1).sum())))
        p[:, kind == 2] = rng.uniform(1, 9.99, (3, int((kind == 2).sum()))) * 1e-300 * rng.choice([1.0, -1.0], (3, int((kind == 2).sum())))
        p[1, kind == 3] = -rng.uniform(0, 0.5, int((kind == 3).sum()))
        p[:, 3:9, 5:12] = 0.0
        p[0, h - 6:, :7] = 0.0
        p[2, :4, w - 9:] = 1.0
        pics.append(p)
    return pics
