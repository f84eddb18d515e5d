"""Golden vectors of the reduced-resolution decode (run in the build container, never on the GPU box).

PyWavelets 1.1.1 alone (python3.9); the reference is not imported.  For about twenty small cases: an int32 coefficient
array as a decoder leaves it (the quantised transform of a seeded picture, thinned out), and for every k < L what
PyWavelets gives back from the dequantised array when the k finest levels are left out,

    pywt.waverec2(coeffs[:L - k + 1], wavelet, mode)        (raw: the 2^-k of the contract is not applied here)

-> reduced_pywt.npz.  The cases cover the tiled filter lengths, periodization, a filter longer than 20 taps (db11), the other
extension modes, odd and even sizes, levels above pywt.dwt_max_level, per-channel scales, and one array that comes from
float32 pixels (PyWavelets' single-precision transform and the wrapper's single-precision quantisation).

usage:
  PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 -W ignore tests/golden/make_reduced_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))


def synth_image(seed, c, H, W):
    """tests/conftest.py: synth_image"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((c, H, W))
    b = np.cumsum(np.cumsum(g, axis=1), axis=2)
    mn = b.min(axis=(1, 2), keepdims=True)
    mx = b.max(axis=(1, 2), keepdims=True)
    b = (b - mn) / (mx - mn)
    b = b + 0.02 * rng.standard_normal((c, H, W))
    return np.round(np.clip(b, 0, 1) * 255).astype(np.uint8) / 255


def thin_out(qa, seed):
    """a decoder's partial picture of the int32 array: about half the coefficients lose their two low bits"""
    rng = np.random.default_rng(seed)
    return (qa - (qa % 4) * (rng.random(qa.shape) < 0.5)).astype(np.int32)


# (wavelet, mode, level, c, H, W, q, per-channel scales, float32 pixels)
CASES = [
    ("bior4.4", "reflect", 3, 2, 61, 77, 50.0, None, False),
    ("bior2.2", "symmetric", 4, 1, 64, 96, 255.0, None, False),
    ("db2", "periodization", 3, 2, 53, 70, 50.0, [1.0, 0.2], False),
    ("haar", "reflect", 3, 1, 40, 41, 10.0, None, False),
    ("sym5", "zero", 2, 1, 57, 66, 50.0, None, False),
    ("bior4.4", "periodization", 2, 1, 35, 48, 255.0, None, False),
    ("db4", "smooth", 3, 1, 71, 64, 50.0, None, False),
    ("db11", "reflect", 2, 1, 44, 51, 50.0, None, False),          # longer than the tiled kernels take
    ("db11", "periodization", 2, 1, 37, 40, 50.0, None, False),
    ("bior6.8", "reflect", 2, 1, 45, 38, 100.0, None, False),
    ("bior2.2", "reflect", 5, 1, 33, 47, 50.0, None, False),      # levels above dwt_max_level
    ("db3", "constant", 3, 2, 29, 54, 50.0, [2.0, 0.75], False),
    ("db10", "periodic", 2, 1, 50, 43, 50.0, None, False),
    ("bior2.2", "reflect", 3, 3, 48, 36, 1.0, [100.0, 20.0, 20.0], False),
    ("coif1", "antisymmetric", 2, 1, 39, 58, 50.0, None, False),
    ("db6", "antireflect", 2, 1, 52, 31, 50.0, None, False),
    ("bior2.2", "reflect", 3, 2, 47, 62, 50.0, None, True),        # an array that float32 pixels made
    ("haar", "periodization", 4, 1, 37, 59, 50.0, None, False),
    ("db8", "symmetric", 1, 1, 30, 45, 50.0, None, False),
    ("bior4.4", "symmetric", 2, 2, 45, 70, 255.0, [1.0, 0.2], False),
]


def main():
    import pywt
    out = {"pywt_version": np.array(pywt.__version__), "ncases": np.array(len(CASES))}
    for i, (wv, mode, L, c, H, W, q, mults, f32) in enumerate(CASES):
        img = synth_image(4100 + i, c, H, W) * 1.3 - 0.15
        if f32:
            img = img.astype(np.float32)
        arr, slices = pywt.coeffs_to_array(pywt.wavedec2(img, wavelet=wv, level=L, mode=mode), axes=(-2, -1))
        m = None if mults is None else np.array(mults)[:, None, None]
        if f32:
            assert arr.dtype == np.float32 and m is None
            quant = (arr * np.float32(q)).astype(np.int32)
        else:
            quant = ((arr if m is None else m * arr) * q).astype(np.int32)
        rec = thin_out(quant, i)
        D = rec.astype(np.float64)
        if m is not None:
            D = D / m
        D = D / q
        coeffs = pywt.array_to_coeffs(D, slices, output_format="wavedec2")
        p = "c%d_" % i
        out[p + "rec"] = rec
        out[p + "wavelet"], out[p + "mode"] = np.array(wv), np.array(mode)
        out[p + "level"], out[p + "hw"], out[p + "q"] = np.array(L), np.array([H, W]), np.array(q)
        out[p + "mults"] = np.array([] if mults is None else mults, dtype=np.float64)
        for k in range(L):
            r = pywt.waverec2(coeffs[:L - k + 1], wavelet=wv, mode=mode, axes=(-2, -1))
            assert r.dtype == np.float64
            out[p + "r%d" % k] = r
    path = os.path.join(HERE, "reduced_pywt.npz")
    np.savez_compressed(path, **out)
    print("wrote reduced_pywt.npz:", len(CASES), "cases;", os.path.getsize(path), "bytes; pywt", pywt.__version__)


if __name__ == "__main__":
    main()
