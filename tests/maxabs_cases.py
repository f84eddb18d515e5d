"""Pictures whose largest quantised coefficient lies where the suite's natural pictures never put it: in a chosen detail band,
level and tile, on a chosen thread, or in the outputs of the bottom / right overhang -- so that the max|coefficient| word
(dwt_device.h: block_raise_max, wave_raise_max) is decided by the launch, wavefront and lane that holds that cell.  The
oracle decides whether a construction holds; tests/test_maxabs_cases.py holds the set to its floors without a GPU and
tests/test_gpu_maxabs.py runs it.  Nothing here is a test.

A class of a packed cell: (level, band, overhang row, overhang column).  Level 1 is the finest.  The band is named as the
kernels name it, rows first: "ad" top right, "da" bottom left, "dd" bottom right, "aa" the root block (last level only).
Output o of a level hangs over when 2 o + 1 >= the length of the level's input: the outputs k_dwt_edge computes again."""
import functools

import numpy as np

import dwt_sweep_tables as T

Q = T.Q
DETAIL = ("ad", "da", "dd")
LEVEL1 = [(1, b, r, c) for b in DETAIL for r in (False, True) for c in (False, True)]
INTERIOR1 = [(1, b, False, False) for b in DETAIL]
INTERIOR2 = [(2, b, False, False) for b in DETAIL]
CLASSES = LEVEL1 + INTERIOR2
FLOAT_MODES = ("reflect", "zero")
FULL = {"u8": 255, "u16": 65535}
# kind -> what the oracle transforms.  "f64": the picture; "float32" / "float16" / "bfloat16": the picture rounded to the kind
# and widened (PX_FLT pixels in); "u8" / "u16": P / 255, P / 65535; "ipt-f64" / "ipt-u8": the colour-fused level 1
FLT_KINDS = ("float32", "float16", "bfloat16")
INT_KINDS = ("u8", "u16")
COLOUR_KINDS = ("ipt-f64", "ipt-u8")


def cname(cls):
    l, band, r, c = cls
    return "%d%s%s%s" % (l, band, "+r" if r else "", "+c" if c else "")


def size_of(oracle, wavelet):
    """one past two forward tiles, odd x odd"""
    return T.forward_sizes(T.instantiation(oracle, wavelet)[0])[3]


def band_origin(g, l, band):
    """(row, column) of the band's first cell in the packed array, and its size"""
    h, w = g["hs"][l], g["ws"][l]
    r0 = g["ll_h"] + sum(g["hs"][l + 1:]) if band[0] == "d" else 0
    c0 = g["ll_w"] + sum(g["ws"][l + 1:]) if band[1] == "d" else 0
    return r0, c0, h, w


def overhang_from(n_out, n_in):
    """first output o with 2 o + 1 >= n_in (n_out where none hangs over)"""
    return min(n_out, n_in // 2)


def class_mask(g, cls):
    """bool [enc_h, enc_w]: the cells of the class"""
    l, band, ovr, ovc = cls
    r0, c0, h, w = band_origin(g, l, band)
    fr, fc = overhang_from(h, g["hs"][l - 1]), overhang_from(w, g["ws"][l - 1])
    m = np.zeros((g["enc_h"], g["enc_w"]), bool)
    rows = slice(r0 + fr, r0 + h) if ovr else slice(r0, r0 + fr)
    cols = slice(c0 + fc, c0 + w) if ovc else slice(c0, c0 + fc)
    m[rows, cols] = True
    return m


def root_mask(g):
    m = np.zeros((g["enc_h"], g["enc_w"]), bool)
    m[:g["ll_h"], :g["ll_w"]] = True
    return m


# ---- what the oracle makes of a picture of a kind ---------------------------------------------------------------------------
def to_kind(pic, kind):
    """float64 picture -> the stored picture of the kind (float kinds: rounded to the kind; "f64": itself)"""
    if kind in FLT_KINDS:
        from spiht_amd import floatpx
        return floatpx.convert(pic, kind)
    return pic


def oracle_input(oracle, stored, kind):
    """the float64 picture the transform sees"""
    if kind in FLT_KINDS:
        from floatin_cases import widen
        return widen(stored, kind)
    if kind in INT_KINDS:
        return stored / float(FULL[kind])
    if kind in COLOUR_KINDS:
        rgb = stored / 255.0 if kind == "ipt-u8" else stored
        return ipt_forward(oracle, rgb)
    return stored


def ipt_params(src, dest):
    from spiht_amd import color_models
    return color_models._params(src, dest)


def ipt_forward(oracle, rgb):
    A, M, p = ipt_params("RGB", "IPT")
    return oracle.color3(rgb, A, M, p)


def ipt_inverse(oracle, ipt):
    A, M, p = ipt_params("IPT", "RGB")
    return oracle.color3(ipt, A, M, p)


def quantised(oracle, stored, kind, wavelet, mode, level, mults=None, q=Q):
    return oracle.quantize(oracle.wavedec2_array(oracle_input(oracle, stored, kind), wavelet, mode, level)[0], q, mults)


def holders(qa):
    """bool [c, enc_h, enc_w]: the cells that hold max|.|, and the maximum"""
    a = np.abs(qa.astype(np.int64))
    return a == a.max(), int(a.max())


def second(qa, mask):
    """the largest magnitude outside the mask (mask [enc_h, enc_w] or [c, enc_h, enc_w])"""
    a = np.abs(qa.astype(np.int64))
    out = a[~np.broadcast_to(mask, a.shape)]
    return int(out.max()) if out.size else 0


# ---- constructions ------------------------------------------------------------------------------------------------------------
def tent(n, centre, radius):
    return np.maximum(0.0, 1.0 - np.abs(np.arange(n) - centre) / float(radius))


def pattern(H, W, band, cr, cc, radius):
    """alternating signs along every axis the band takes the detail of, under a tent that peaks on row cr and column cc"""
    i, j = np.arange(H)[:, None], np.arange(W)[None, :]
    s = np.ones((H, W))
    if band[0] == "d":
        s = s * (1 - 2 * (i & 1))
    if band[1] == "d":
        s = s * (1 - 2 * (j & 1))
    return s * tent(H, cr, radius)[:, None] * tent(W, cc, radius)[None, :]


def synthesis(oracle, wavelet, mode, level, H, W, cell):
    """the synthesis function of a packed cell, cropped to the picture and scaled to max|.| = 1"""
    g = oracle.geometry(H, W, wavelet, level, mode)
    unit = np.zeros((1, g["enc_h"], g["enc_w"]))
    unit[0, cell[0], cell[1]] = 1.0
    pic = oracle.waverec2_array(unit, H, W, wavelet, level, mode)[0, :H, :W]
    top = np.abs(pic).max()
    return pic / top if top > 0 else None


def candidates(oracle, wavelet, mode, level, H, W, cls):
    """float pictures [H, W] in [-1, 1] to try for a class, in a fixed order"""
    l, band, ovr, ovc = cls
    g = oracle.geometry(H, W, wavelet, level, mode)
    m = class_mask(g, cls)
    rows, cols = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    if len(rows) == 0 or len(cols) == 0:
        return
    for fr, fc in ((0.5, 0.5), (0.3, 0.7), (1.0, 1.0), (0.0, 0.0)):
        cell = (int(rows[int(fr * (len(rows) - 1))]), int(cols[int(fc * (len(cols) - 1))]))
        pic = synthesis(oracle, wavelet, mode, level, H, W, cell)
        if pic is not None:
            yield pic
    if l != 1:
        return
    for radius in range(3, 15):
        for dr in ((1, 2) if ovr else (0, 1)):
            for dc in ((1, 2) if ovc else (0, 1)):
                yield pattern(H, W, band, H - dr if ovr else H // 2 + dr, W - dc if ovc else W // 2 + dc, radius)


def stored_forms(oracle, pic, kind):
    """the stored pictures [c, H, W] a pattern in [-1, 1] gives for a kind"""
    if kind == "f64" or kind in FLT_KINDS:
        yield to_kind(pic[None], kind)
    elif kind in INT_KINDS:
        full = FULL[kind]
        dt = np.uint8 if kind == "u8" else np.uint16
        black = np.zeros((3,) + pic.shape, dt)
        black[1] = np.round(full * np.clip(pic, 0.0, 1.0))
        yield black
        grey = np.zeros((3,) + pic.shape, dt)
        grey[1] = (full + 1) // 2 + np.round((full // 2) * pic).astype(np.int64)
        yield grey
    elif kind == "ipt-f64":
        # the wanted picture in the transformed domain (signed, no background: the signed power takes it), taken back to RGB
        for ch, amp in ((0, 0.5), (1, 0.25)):
            ipt = np.zeros((3,) + pic.shape)
            ipt[ch] = amp * pic
            yield ipt_inverse(oracle, ipt)
    else:
        # ... as a grey picture, I = the pattern on black or around mid-grey, rounded to 8 bits on the way back
        for I in (np.clip(pic, 0.0, 1.0), 0.5 + 0.5 * pic):
            ipt = np.zeros((3,) + pic.shape)
            ipt[0] = I
            yield np.round(np.clip(ipt_inverse(oracle, ipt), 0.0, 1.0) * 255.0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _place(oracle, wavelet, mode, level, H, W, cls, kind):
    g = oracle.geometry(H, W, wavelet, level, mode)
    m = class_mask(g, cls)
    for pic in candidates(oracle, wavelet, mode, level, H, W, cls):
        for stored in stored_forms(oracle, pic, kind):
            # (an integer picture's pattern is in channel 1 alone, and black channels transform to zeros)
            seen = stored[1:2] if kind in INT_KINDS else stored
            hold, top = holders(quantised(oracle, seen, kind, wavelet, mode, level))
            if top > 0 and not (hold & ~m).any():
                stored.setflags(write=False)
                return stored
    return None


def place(oracle, wavelet, mode, level, H, W, cls, kind="f64"):
    """A picture [c, H, W] of the kind whose quantised array (q = 1000, no channel scales) holds its maximum only in cells of
    the class, or None where none of the constructions does.  Read-only, computed once."""
    return _place(oracle, wavelet, mode, level, H, W, tuple(cls), kind)


# ---- the grid: kind -> (level, modes, classes); what is not reached is named --------------------------------------------------
GRID = {k: (2, FLOAT_MODES, CLASSES) for k in ("f64",) + FLT_KINDS}
GRID.update({k: (1, ("reflect",), LEVEL1) for k in INT_KINDS + COLOUR_KINDS})


def grid(oracle, kind):
    """every (wavelet, mode, level, H, W, class) of a kind's grid"""
    level, modes, classes = GRID[kind]
    for wavelet in T.WAVELETS:
        H, W = size_of(oracle, wavelet)
        for mode in modes:
            for cls in classes:
                yield wavelet, mode, level, H, W, cls


def key(wavelet, mode, cls):
    return "%s/%s/%s" % (wavelet, mode, cname(cls))


def reached(oracle, kind, wavelet=None):
    """the grid without what UNREACHED names: what the GPU tests iterate over"""
    return [c for c in grid(oracle, kind) if key(c[0], c[1], c[5]) not in UNREACHED[kind] and wavelet in (None, c[0])]


# Not reached by any construction of place(), on the oracle (tests/test_maxabs_cases.py holds this list to the oracle in both
# directions): wavelet/mode/class.
UNREACHED = {
    "f64": frozenset("""
        haar/zero/1ad+r haar/zero/1ad+r+c haar/zero/1da+c haar/zero/1da+r+c haar/zero/1dd+c haar/zero/1dd+r
        haar/zero/1dd+r+c bior6.8/reflect/2da bior6.8/reflect/2dd bior2.8/reflect/2ad bior2.8/reflect/2da
        bior2.8/reflect/2dd db10/zero/2ad
    """.split()),
    "float32": frozenset("""
        haar/zero/1ad+r haar/zero/1ad+r+c haar/zero/1da+c haar/zero/1da+r+c haar/zero/1dd+c haar/zero/1dd+r
        haar/zero/1dd+r+c bior6.8/reflect/2da bior6.8/reflect/2dd bior2.8/reflect/2ad bior2.8/reflect/2da
        bior2.8/reflect/2dd db10/zero/2ad
    """.split()),
    "float16": frozenset("""
        haar/zero/1ad+r haar/zero/1ad+r+c haar/zero/1da+c haar/zero/1da+r+c haar/zero/1dd+c haar/zero/1dd+r
        haar/zero/1dd+r+c bior6.8/reflect/2da bior6.8/reflect/2dd bior2.8/reflect/2ad bior2.8/reflect/2da
        bior2.8/reflect/2dd db10/zero/2ad
    """.split()),
    "bfloat16": frozenset("""
        haar/zero/1ad+r haar/zero/1ad+r+c haar/zero/1da+c haar/zero/1da+r+c haar/zero/1dd+c haar/zero/1dd+r
        haar/zero/1dd+r+c bior6.8/reflect/2da bior6.8/reflect/2dd bior2.8/reflect/2ad bior2.8/reflect/2da
        bior2.8/reflect/2dd db10/zero/2ad
    """.split()),
    "u8": frozenset("""
        haar/reflect/1ad haar/reflect/1ad+c haar/reflect/1ad+r haar/reflect/1ad+r+c haar/reflect/1da haar/reflect/1da+c
        haar/reflect/1da+r haar/reflect/1da+r+c haar/reflect/1dd haar/reflect/1dd+c haar/reflect/1dd+r haar/reflect/1dd+r+c
        bior2.2/reflect/1ad bior2.2/reflect/1ad+c bior2.2/reflect/1ad+r bior2.2/reflect/1ad+r+c bior2.2/reflect/1da
        bior2.2/reflect/1da+c bior2.2/reflect/1da+r bior2.2/reflect/1da+r+c bior2.2/reflect/1dd+r+c bior3.3/reflect/1ad
        bior3.3/reflect/1ad+c bior3.3/reflect/1ad+r bior3.3/reflect/1ad+r+c bior3.3/reflect/1da bior3.3/reflect/1da+c
        bior3.3/reflect/1da+r bior3.3/reflect/1da+r+c bior3.3/reflect/1dd bior3.3/reflect/1dd+c bior3.3/reflect/1dd+r
        bior3.3/reflect/1dd+r+c db5/reflect/1ad+c db5/reflect/1da+r bior2.4/reflect/1ad bior2.4/reflect/1ad+c
        bior2.4/reflect/1ad+r bior2.4/reflect/1ad+r+c bior2.4/reflect/1da bior2.4/reflect/1da+c bior2.4/reflect/1da+r
        bior2.4/reflect/1da+r+c db6/reflect/1ad+c db6/reflect/1da+r bior2.6/reflect/1ad bior2.6/reflect/1ad+c
        bior2.6/reflect/1ad+r bior2.6/reflect/1ad+r+c bior2.6/reflect/1da bior2.6/reflect/1da+c bior2.6/reflect/1da+r
        bior2.6/reflect/1da+r+c bior3.7/reflect/1ad bior3.7/reflect/1ad+c bior3.7/reflect/1ad+r+c bior3.7/reflect/1da
        bior3.7/reflect/1da+c bior3.7/reflect/1da+r bior3.7/reflect/1da+r+c bior3.7/reflect/1dd bior3.7/reflect/1dd+c
        bior3.7/reflect/1dd+r bior3.7/reflect/1dd+r+c bior6.8/reflect/1ad+c bior2.8/reflect/1ad bior2.8/reflect/1ad+c
        bior2.8/reflect/1ad+r bior2.8/reflect/1ad+r+c bior2.8/reflect/1da bior2.8/reflect/1da+c bior2.8/reflect/1da+r
        bior2.8/reflect/1da+r+c bior3.9/reflect/1ad bior3.9/reflect/1ad+c bior3.9/reflect/1ad+r bior3.9/reflect/1ad+r+c
        bior3.9/reflect/1da bior3.9/reflect/1da+c bior3.9/reflect/1da+r bior3.9/reflect/1da+r+c bior3.9/reflect/1dd
        bior3.9/reflect/1dd+c bior3.9/reflect/1dd+r bior3.9/reflect/1dd+r+c
    """.split()),
    "u16": frozenset("""
        haar/reflect/1ad haar/reflect/1ad+c haar/reflect/1ad+r haar/reflect/1ad+r+c haar/reflect/1da haar/reflect/1da+c
        haar/reflect/1da+r haar/reflect/1da+r+c haar/reflect/1dd haar/reflect/1dd+c haar/reflect/1dd+r haar/reflect/1dd+r+c
        bior2.2/reflect/1ad bior2.2/reflect/1ad+c bior2.2/reflect/1ad+r bior2.2/reflect/1ad+r+c bior2.2/reflect/1da
        bior2.2/reflect/1da+c bior2.2/reflect/1da+r bior2.2/reflect/1da+r+c bior2.2/reflect/1dd+r+c bior3.3/reflect/1ad
        bior3.3/reflect/1ad+c bior3.3/reflect/1ad+r bior3.3/reflect/1ad+r+c bior3.3/reflect/1da bior3.3/reflect/1da+c
        bior3.3/reflect/1da+r bior3.3/reflect/1da+r+c bior3.3/reflect/1dd bior3.3/reflect/1dd+c bior3.3/reflect/1dd+r
        bior3.3/reflect/1dd+r+c db5/reflect/1ad+c db5/reflect/1da+r bior2.4/reflect/1ad bior2.4/reflect/1ad+c
        bior2.4/reflect/1ad+r bior2.4/reflect/1ad+r+c bior2.4/reflect/1da bior2.4/reflect/1da+c bior2.4/reflect/1da+r
        bior2.4/reflect/1da+r+c db6/reflect/1ad+c db6/reflect/1da+r bior2.6/reflect/1ad bior2.6/reflect/1ad+c
        bior2.6/reflect/1ad+r bior2.6/reflect/1ad+r+c bior2.6/reflect/1da bior2.6/reflect/1da+c bior2.6/reflect/1da+r
        bior2.6/reflect/1da+r+c bior3.7/reflect/1ad bior3.7/reflect/1ad+c bior3.7/reflect/1ad+r+c bior3.7/reflect/1da
        bior3.7/reflect/1da+c bior3.7/reflect/1da+r bior3.7/reflect/1da+r+c bior3.7/reflect/1dd bior3.7/reflect/1dd+c
        bior3.7/reflect/1dd+r bior3.7/reflect/1dd+r+c bior6.8/reflect/1ad+c bior2.8/reflect/1ad bior2.8/reflect/1ad+c
        bior2.8/reflect/1ad+r bior2.8/reflect/1ad+r+c bior2.8/reflect/1da bior2.8/reflect/1da+c bior2.8/reflect/1da+r
        bior2.8/reflect/1da+r+c bior3.9/reflect/1ad bior3.9/reflect/1ad+c bior3.9/reflect/1ad+r+c bior3.9/reflect/1da
        bior3.9/reflect/1da+c bior3.9/reflect/1da+r bior3.9/reflect/1da+r+c bior3.9/reflect/1dd bior3.9/reflect/1dd+c
        bior3.9/reflect/1dd+r bior3.9/reflect/1dd+r+c
    """.split()),
    "ipt-f64": frozenset("""
    """.split()),
    "ipt-u8": frozenset("""
        haar/reflect/1ad haar/reflect/1ad+c haar/reflect/1ad+r haar/reflect/1ad+r+c haar/reflect/1da haar/reflect/1da+c
        haar/reflect/1da+r haar/reflect/1da+r+c haar/reflect/1dd haar/reflect/1dd+c haar/reflect/1dd+r haar/reflect/1dd+r+c
        bior2.2/reflect/1ad bior2.2/reflect/1ad+c bior2.2/reflect/1ad+r bior2.2/reflect/1ad+r+c bior2.2/reflect/1da
        bior2.2/reflect/1da+c bior2.2/reflect/1da+r bior2.2/reflect/1da+r+c bior2.2/reflect/1dd+r+c bior3.3/reflect/1ad
        bior3.3/reflect/1ad+c bior3.3/reflect/1ad+r bior3.3/reflect/1ad+r+c bior3.3/reflect/1da bior3.3/reflect/1da+c
        bior3.3/reflect/1da+r bior3.3/reflect/1da+r+c bior3.3/reflect/1dd bior3.3/reflect/1dd+c bior3.3/reflect/1dd+r
        bior3.3/reflect/1dd+r+c db5/reflect/1ad+c db5/reflect/1da+r bior2.4/reflect/1ad bior2.4/reflect/1ad+c
        bior2.4/reflect/1ad+r bior2.4/reflect/1ad+r+c bior2.4/reflect/1da bior2.4/reflect/1da+c bior2.4/reflect/1da+r
        bior2.4/reflect/1da+r+c db6/reflect/1ad+c db6/reflect/1da+r bior2.6/reflect/1ad bior2.6/reflect/1ad+c
        bior2.6/reflect/1ad+r bior2.6/reflect/1ad+r+c bior2.6/reflect/1da bior2.6/reflect/1da+c bior2.6/reflect/1da+r
        bior2.6/reflect/1da+r+c bior3.7/reflect/1ad bior3.7/reflect/1ad+c bior3.7/reflect/1ad+r+c bior3.7/reflect/1da
        bior3.7/reflect/1da+c bior3.7/reflect/1da+r bior3.7/reflect/1da+r+c bior3.7/reflect/1dd bior3.7/reflect/1dd+c
        bior3.7/reflect/1dd+r bior3.7/reflect/1dd+r+c bior6.8/reflect/1ad+c bior2.8/reflect/1ad bior2.8/reflect/1ad+c
        bior2.8/reflect/1ad+r bior2.8/reflect/1ad+r+c bior2.8/reflect/1da bior2.8/reflect/1da+c bior2.8/reflect/1da+r
        bior2.8/reflect/1da+r+c bior3.9/reflect/1ad bior3.9/reflect/1ad+c bior3.9/reflect/1ad+r bior3.9/reflect/1ad+r+c
        bior3.9/reflect/1da bior3.9/reflect/1da+c bior3.9/reflect/1da+r bior3.9/reflect/1da+r+c bior3.9/reflect/1dd
        bior3.9/reflect/1dd+c bior3.9/reflect/1dd+r bior3.9/reflect/1dd+r+c
    """.split()),
}


# ---- A / C: batches of three in which neighbouring images hold different classes and magnitudes --------------------------------
MAGNITUDES = (1.0, 4.0, 16.0)  # powers of two: exact in every float kind


def batches(oracle, kind, wavelet, mode):
    """[(pictures [3, c, H, W] of the kind, classes of the three, per-channel scales or None)] over the reached classes of
    (kind, wavelet, mode), three in turn (the last batch filled up from the front).  Float kinds: two channels, the class's
    picture times the magnitude and, an eighth as large, the next class's; three magnitudes a factor 4 apart that rotate
    through the batches.  Integer and colour kinds: the three-channel pictures as place() gives them."""
    todo = [c for c in reached(oracle, kind, wavelet) if c[1] == mode]
    out = []
    for j in range(0, len(todo), 3):
        three = [todo[(j + i) % len(todo)] for i in range(3)]
        pics, classes = [], []
        for i, (w, m, l, H, W, cls) in enumerate(three):
            p = place(oracle, w, m, l, H, W, cls, kind)
            if kind == "f64" or kind in FLT_KINDS:
                nxt = todo[(j + i + 1) % len(todo)]
                other = place(oracle, w, m, l, H, W, nxt[5], kind)
                mag = MAGNITUDES[(i + j // 3) % 3]
                wide = np.concatenate([oracle_input(oracle, p, kind) * mag, oracle_input(oracle, other, kind) * (mag / 8.0)])
                p = to_kind(wide, kind)
            pics.append(p)
            classes.append(cls)
        # (the float kinds' entry point is called without channel scales)
        out.append((np.stack(pics), classes, None if kind in FLT_KINDS else T.scales_for(j // 3, pics[0].shape[0])))
    return out


def batch_reference(oracle, kind, wavelet, mode, pics, mults):
    level = GRID[kind][0]
    return np.stack([quantised(oracle, p, kind, wavelet, mode, level, mults) for p in pics])


def in_class(oracle, wavelet, mode, level, H, W, cls, qa):
    """the maximum of one image's array [c, enc_h, enc_w] lies in cells of the class only"""
    hold, top = holders(qa)
    return top > 0 and not (hold & ~class_mask(oracle.geometry(H, W, wavelet, level, mode), cls)).any()


# ---- B: every thread of a tile ------------------------------------------------------------------------------------------------
THREAD_WAVELETS = (("haar", "reflect"), ("bior2.2", "zero"), ("db5", "reflect"), ("db9", "zero"))  # F = 2, 6, 10, 18


def thread_size(F):
    """2 x 2 forward tiles exactly"""
    return 2 * (2 * T.FWD_TH) - F + 2, 2 * (2 * T.FWD_TW) - F + 2


def thread_targets():
    """dd cells (row, column) of the 24 x 128 band: all of tile (0, 0) -- every lane of the three wavefronts at every one of a
    thread's four rows -- then the first and last row and column of each of the four tiles"""
    th, tw = T.FWD_TH, T.FWD_TW
    out = [(r, c) for r in range(th) for c in range(tw)]
    for ty in (0, 1):
        for tx in (0, 1):
            for r in range(th):
                for c in range(tw):
                    if r in (0, th - 1) or c in (0, tw - 1):
                        out.append((ty * th + r, tx * tw + c))
    return list(dict.fromkeys(out))


def thread_cases(oracle, wavelet, mode, chunk=64):
    """-> yields (targets [(r, c)], pictures [n, 1, H, W], reference [n, 1, enc_h, enc_w]) in chunks, every picture with its
    maximum in one cell only: the target.  The synthesis function of a cell next to the picture's border does not peak there
    (the band holds F / 2 - 1 more cells than half the picture); such a target of tile (0, 0) is taken at the same place of
    the tile below, to the right, or both, and one that fails there too is left out."""
    F = T.instantiation(oracle, wavelet)[0]
    H, W = thread_size(F)
    g = oracle.geometry(H, W, wavelet, 1, mode)
    r0, c0, h, w = band_origin(g, 1, "dd")
    assert (h, w) == (2 * T.FWD_TH, 2 * T.FWD_TW)

    def one(r, c):
        pic = synthesis(oracle, wavelet, mode, 1, H, W, (r0 + r, c0 + c))
        if pic is None:
            return None
        qa = quantised(oracle, pic[None], "f64", wavelet, mode, 1)
        hold, _ = holders(qa)
        return (pic[None], qa) if hold.sum() == 1 and hold[0, r0 + r, c0 + c] else None

    done, tg, pics, refs = set(), [], [], []
    for (r, c) in thread_targets():
        for (rr, cc) in ((r, c), (r + T.FWD_TH, c), (r, c + T.FWD_TW), (r + T.FWD_TH, c + T.FWD_TW)):
            if (rr, cc) in done or rr >= h or cc >= w:
                continue
            got = one(rr, cc)
            if got is not None:
                done.add((rr, cc))
                tg.append((rr, cc)), pics.append(got[0]), refs.append(got[1])
                break
            if r >= T.FWD_TH or c >= T.FWD_TW:
                break  # (only tile (0, 0) has a stand-in)
        if len(tg) == chunk:
            yield tg, np.stack(pics), np.stack(refs)
            tg, pics, refs = [], [], []
    if tg:
        yield tg, np.stack(pics), np.stack(refs)


# ---- D: the step from the word to the start plane -------------------------------------------------------------------------------
STEP_WAVELETS = ("bior2.2", "db4", "bior4.4")
STEP_K = 10


def quantised_f32(oracle, stored, wavelet, mode, level, q):
    """the single-precision transform and quantiser (what float32 pixels take through encode_image)"""
    return oracle.quantize_f32(oracle.wavedec2_array_f32(stored, wavelet, mode, level)[0], q, None)


@functools.lru_cache(maxsize=None)
def step_case(oracle, kind, wavelet, mode, level, cls, k=STEP_K):
    """-> (stored picture, q, maximum, second) with maximum >= 2^k > second: the class alone decides the start plane -- or
    None.  kind "f32t": float32 pixels in the single-precision transform; "f64", "u8": as in place().  The picture is place()'s,
    the quantiser's scale is searched just above 2^k / max|coefficient of the class|."""
    H, W = size_of(oracle, wavelet)
    stored = place(oracle, wavelet, mode, level, H, W, cls, "float32" if kind == "f32t" else kind)
    if stored is None:
        return None
    g = oracle.geometry(H, W, wavelet, level, mode)
    m = class_mask(g, cls)
    if kind == "f32t":
        arr = oracle.wavedec2_array_f32(stored, wavelet, mode, level)[0].astype(np.float64)
        quant = lambda q: quantised_f32(oracle, stored, wavelet, mode, level, q)  # noqa: E731
    else:
        arr = oracle.wavedec2_array(oracle_input(oracle, stored, kind), wavelet, mode, level)[0]
        quant = lambda q: quantised(oracle, stored, kind, wavelet, mode, level, None, q)  # noqa: E731
    top = np.abs(arr[:, m]).max()
    if top == 0:
        return None
    for j in range(64):
        q = float(np.float32(2.0 ** k / top * (1.0 + j / 1024.0)))  # (a float32 value: the same scale in both precisions)
        qa = quant(q)
        a = np.abs(qa.astype(np.int64))
        inside, outside = int(a[:, m].max()), second(qa, m)
        if inside >= 2 ** k > outside:
            return stored, q, inside, outside
    return None


# ---- E: the two-pass levels (k_dwt_pack_ext), wavefronts that straddle two images ---------------------------------------------
# (route, what it is there for); two levels, two channels, 67 x 101 pictures (66 x 102 under periodization: no padding
# column, so the last cell of a band is reached): no plane size of either level is a multiple of 64
PACK_ROUTES = (("db20", "reflect"), ("db4", "smooth"), ("haar", "smooth"), ("bior4.4", "periodization"))
PACK_TARGETS = (("dd", "first"), ("dd", "last"), ("aa", "first"), ("aa", "last"))
# the corner cells no construction reaches (a long filter's outermost taps are ~1e-7: the cell cannot dominate its neighbours)
PACK_UNREACHED = frozenset("""
    db20/reflect/dd/last db20/reflect/aa/first db4/smooth/dd/first db4/smooth/dd/last haar/smooth/dd/last
""".split())


def pack_size(mode):
    return (66, 102) if mode == "periodization" else (67, 101)


def corner_cell(g, band, which):
    r0, c0, h, w = (0, 0, g["ll_h"], g["ll_w"]) if band == "aa" else band_origin(g, 1, band)
    return (r0, c0) if which == "first" else (r0 + h - 1, c0 + w - 1)


def least_squares_picture(oracle, wavelet, mode, level, H, W, cell, which, patch=8):
    """the picture on a patch x patch corner whose transform is nearest the unit at the cell (scaled to max|.| = 1)"""
    g = oracle.geometry(H, W, wavelet, level, mode)
    rows = range(patch) if which == "first" else range(H - patch, H)
    cols = range(patch) if which == "first" else range(W - patch, W)
    px = [(i, j) for i in rows for j in cols]
    units = np.zeros((len(px), H, W))
    for n, (i, j) in enumerate(px):
        units[n, i, j] = 1.0
    A = oracle.wavedec2_array(units, wavelet, mode, level)[0].reshape(len(px), -1).T
    e = np.zeros(A.shape[0])
    e[cell[0] * g["enc_w"] + cell[1]] = 1.0
    x = np.linalg.lstsq(A, e, rcond=None)[0]
    pic = np.zeros((H, W))
    for n, (i, j) in enumerate(px):
        pic[i, j] = x[n]
    top = np.abs(pic).max()
    return pic / top if top > 0 and np.isfinite(top) else None


@functools.lru_cache(maxsize=None)
def corner_picture(oracle, wavelet, mode, band, which):
    """a picture [H, W] whose quantised array (two levels, q = 1000) has its maximum in one cell only: the first or the last
    cell of the level-1 'dd' band or of the root block -- or None"""
    H, W = pack_size(mode)
    g = oracle.geometry(H, W, wavelet, 2, mode)
    cell = corner_cell(g, band, which)

    def tries():
        yield synthesis(oracle, wavelet, mode, 2, H, W, cell)
        for radius in range(2, 7):
            for d in (0, 1, 2):
                yield pattern(H, W, band, d if which == "first" else H - 1 - d, d if which == "first" else W - 1 - d, radius)
        yield least_squares_picture(oracle, wavelet, mode, 2, H, W, cell, which)

    for pic in tries():
        if pic is None:
            continue
        hold, _ = holders(quantised(oracle, pic[None], "f64", wavelet, mode, 2))
        if hold.sum() == 1 and hold[0, cell[0], cell[1]]:
            pic.setflags(write=False)
            return pic
    return None


def pack_batches(oracle, wavelet, mode):
    """[(pictures [3, 2, H, W], targets of the three)]: the reached targets alternate between the images -- a 'first' cell in
    channel 0 (thread 0 of the image), a 'last' cell in channel 1 (the image's last thread) -- at magnitudes a factor 4 apart;
    the other channel holds an interior picture an eighth as large"""
    H, W = pack_size(mode)
    todo = [(b, wh) for (b, wh) in PACK_TARGETS if "%s/%s/%s/%s" % (wavelet, mode, b, wh) not in PACK_UNREACHED]
    g = oracle.geometry(H, W, wavelet, 2, mode)
    mid = synthesis(oracle, wavelet, mode, 2, H, W, (g["enc_h"] - g["hs"][1] // 2, g["enc_w"] - g["ws"][1] // 2))
    out = []
    for j in range(len(todo)):
        pics, targets = [], []
        for i in range(3):
            band, which = todo[(j + i) % len(todo)]
            mag = MAGNITUDES[(i + j) % 3]
            p = np.zeros((2, H, W))
            ch = 0 if which == "first" else 1
            p[ch] = corner_picture(oracle, wavelet, mode, band, which) * mag
            p[1 - ch] = mid * (mag / 8.0)
            pics.append(p)
            targets.append((band, which))
        out.append((np.stack(pics), targets))
    return out


# ---- F: k_absmax ------------------------------------------------------------------------------------------------------------------
ABSMAX_GEOMS = ((1, 33, 64, 5, 8), (1, 33, 65, 5, 9), (3, 17, 25, 3, 4))  # (c, h, w, ll_h, ll_w): n = 2112 (0 mod 4), 2145, 1275


def absmax_positions(n):
    """index 0, n - 1, every residue mod 4, either side of a multiple of 256 and of 1024"""
    want = [0, 1, 2, 3, n - 1, n - 2, n - 3, n - 4, 255, 256, 257, 1023, 1024, 1025, 4 * 255, 4 * 256, 4 * 256 + 3]
    return [p for p in dict.fromkeys(want) if 0 <= p < n]


def absmax_arrays(geom, seed=7):
    """[(x int32 [3, c, h, w], k)]: |x| <= 3 and one cell per image of magnitude 2^k + 1, negative on every other image, the
    position moving through absmax_positions and k through 2 .. 29, three different positions and magnitudes per batch"""
    c, h, w = geom[:3]
    n = c * h * w
    pos = absmax_positions(n)
    rng = np.random.default_rng(seed + n)
    out = []
    for j in range(len(pos)):
        x = rng.integers(-3, 4, (3, n)).astype(np.int32)
        ks = []
        for b in range(3):
            k = 2 + (5 * j + 9 * b) % 28
            x[b, pos[(j + 5 * b) % len(pos)]] = (2 ** k + 1) * (-1 if (j + b) & 1 else 1)
            ks.append(k)
        out.append((x.reshape(3, c, h, w), ks))
    return out
