"""The grid of tests/test_gpu_dwt_sweep.py: wavelets, extension modes, picture sizes placed on the seams of the transform
kernels' tiles, and the input data -- everything that needs no GPU, so that tests/test_dwt_sweep_tables.py can hold the
grid to its purpose (every template instantiation reached, every size on the seam it names, inputs dense enough to
tell a wrong sample) where no GPU is.  Nothing here is a test."""
import numpy as np

from conftest import synth_image

# One name per (filter length, zero-tap mask instantiation, leading joint zero taps) of spiht_launch_dwt_level /
# spiht_launch_idwt_level (dwt_fwd.hip: launch_dwt_F, launch_dwt_FM's z; dwt_inv.hip: launch_idwt_F); test_dwt_sweep_tables.py recomputes
# the grouping from the filters.
WAVELETS = ["haar", "db2", "bior2.2", "db3", "rbio1.3", "db4", "bior3.3", "bior4.4", "db5", "bior2.4", "db6", "rbio5.5", "db7",
            "bior2.6", "db8", "bior3.7", "bior6.8", "db9", "bior2.8", "db10", "bior3.9"]
# one name per instantiation of the inverse kernels (the leading zero taps do not enter them)
INVERSE_MASK_WAVELETS = ["haar", "db2", "bior2.2", "db3", "db4", "bior4.4", "db5", "db6", "db7", "db8", "bior6.8", "db9", "db10"]
MODES = ["reflect", "symmetric", "periodic", "zero", "constant"]  # the index maps: the modes the tiled kernels take

# the switch of spiht_launch_dwt_level / spiht_launch_idwt_level (dwt_fwd.hip, dwt_inv.hip): F -> (mask of the low-pass, of the high-pass
# filter) of the bank that length is specialised for; any other bank of that length takes the all-taps instantiation
FWD_SPECIALISED = {2: (0x3, 0x3), 6: (0x3E, 0x0E), 10: (0x3FE, 0x0FE), 18: (0x3FFFE, 0x3FF8)}
INV_SPECIALISED = {2: (0x3, 0x3), 6: (0x0E, 0x3E), 10: (0x0FE, 0x3FE), 18: (0x3FF8, 0x3FFFE)}
FILTER_LENGTHS = [2, 4, 6, 8, 10, 12, 14, 16, 18, 20]

# tile constants of the kernels, mirrored
FWD_TH, FWD_TW = 12, 64    # dwt_device.h  DW_TH, DW_TW: output rows / columns per tile of k_dwt_level
FWD32_TH = 16              # dwt_device.h  DW32_TH: output rows per tile of k_dwt_level_f32
C1_ROWS = 136              # dwt_fwd.hip  C1_ROWS: output rows a workgroup of k_dwt1_color marches down
INV_TH, INV_TW = 24, 128   # common.h  IW_TH, IW_TW: output rows / columns per tile of k_idwt_level(_pf)
INVC_TH = 8                # dwt_inv.hip  IWC_TH: output rows per tile of k_idwt1_color
PF_MIN = 20000             # dwt_inv.hip  launch_idwt_FM's pf_min: tiles of a level from which launch_idwt_FM takes k_idwt_level_pf


def c1_sw(F):
    """dwt_fwd.hip  k_dwt1_color's SW: output columns per strip of k_dwt1_color"""
    return (256 - (F - 2)) // 2


def tap_mask(f):
    return sum(1 << j for j in range(len(f)) if f[j] != 0.0)


def instantiation(oracle, name, inverse=False):
    """(F, 'special' | 'all', z) as launch_dwt_F / launch_idwt_F pick it for the wavelet's filters; z: leading taps that are
    zero in both analysis filters (launch_dwt_FM: it moves the extent k_dwt_edge recomputes)"""
    dec_lo, dec_hi, rec_lo, rec_hi = oracle.wavelet_filters(name)
    F = len(dec_lo)
    lo, hi = (rec_lo, rec_hi) if inverse else (dec_lo, dec_hi)
    special = (INV_SPECIALISED if inverse else FWD_SPECIALISED).get(F) == (tap_mask(lo), tap_mask(hi))
    z = 0
    while z < F and dec_lo[z] == 0.0 and dec_hi[z] == 0.0:
        z += 1
    return F, "special" if special else "all", z


def band_len(n, F):
    return (n + F - 1) // 2


def tiles(n, t):
    return -(-n // t)


# ---- forward sizes: level-1 output counts T - 1, T, T + 1, 2 T + 1 per axis, rows and columns paired up -----------------
# (an input of 2 K - F + 1 or 2 K - F + 2 samples gives K outputs: the odd and the even one take turns)
_FWD_PARITY = [(1, 0), (0, 1), (0, 0), (1, 1)]  # 1: the odd input length


def forward_sizes(F, th=FWD_TH):
    """[(H, W)] x 4: under one tile, exactly one tile, one past a tile, one past two tiles (that one odd x odd).  With a
    long filter the first ones are shorter than the filter (3 x 107 under db10): legal for float64 and the integer kinds."""
    out = []
    for (kh, kw), (ph, pw) in zip(zip((th - 1, th, th + 1, 2 * th + 1), (FWD_TW - 1, FWD_TW, FWD_TW + 1, 2 * FWD_TW + 1)), _FWD_PARITY):
        out.append((2 * kh - F + 2 - ph, 2 * kw - F + 2 - pw))
    return out


def forward_sizes_reduced(F):
    """the integer and colour-fused families: exactly one tile, and one past two tiles with odd sizes"""
    s = forward_sizes(F)
    return [s[1], s[3]]


def f32_level(F, H, W):
    """The single-precision kernel takes no level input shorter than the filter (dwt_fwd.hip, above k_dwt_level_f32): two levels
    where both levels' inputs are long enough, one where only the picture is, None (left out) otherwise."""
    if min(H, W) < F:
        return None
    return 2 if min(band_len(H, F), band_len(W, F)) >= F else 1


COLOUR_BIG = (281, 523)  # crosses a strip of k_dwt1_color in both directions for every filter length


# ---- inverse sizes: rec = 2 band - F + 2 output samples per axis ----------------------------------------------------------
INV_REC = [(22, 126), (24, 128), (26, 130), (50, 258)]  # under a tile, a tile, one sample pair past it, past two tiles


def inverse_sizes(integer):
    """[(H, W)]: pictures whose level-1 bands give back INV_REC (a picture of rec or rec - 1 samples has the same bands).
    Integer kinds: odd H and W, so that the crop of the extra row and column falls on the seam."""
    if integer:
        return [(h - 1, w - 1) for h, w in INV_REC]
    return [(h - (i & 1), w - ((i >> 1) & 1)) for i, (h, w) in enumerate(INV_REC)]


# ---- the persistent inverse ------------------------------------------------------------------------------------------------
PF_REC = (26, 130)     # 2 x 2 tiles, three of them slivers
PF_PICTURES = 1667     # x 3 channels x 4 tiles = 20 004 tiles
PF_DISTINCT = 8


def pf_tile_count():
    return PF_PICTURES * 3 * tiles(PF_REC[0], INV_TH) * tiles(PF_REC[1], INV_TW)


# ---- data --------------------------------------------------------------------------------------------------------------------
Q = 1000.0  # the last bits of the coefficients decide the quantised value


def sweep_images(seed, B, c, H, W):
    return np.stack([synth_image(seed + 7 * b, c, H, W) for b in range(B)])


def scales_for(i, c):
    """per-channel scales on every other case"""
    return None if i % 2 == 0 else [2.0, 0.75, 1.5][:c]


def with_patches(img):
    """patches of exact 0 and exact 1 (float pictures; the integer kinds scale them to 0 and 255 / 65535)"""
    img = img.copy()
    H, W = img.shape[-2:]
    img[..., : max(1, H // 3), : max(1, W // 4)] = 0.0
    img[..., H - max(1, H // 4):, W - max(1, W // 3):] = 1.0
    return img


def thin_out(qa, seed):
    """tests/golden/make_golden.py: a decoder's partial picture of the int32 array"""
    from golden.make_golden import thin_out as t
    return t(qa, seed)


def inverse_case(oracle, wavelet, H, W, level, seed, mults, c=2):
    """-> (rec int32 [c, enc_h, enc_w], want float64 [c, rec_h, rec_w]): a thinned-out copy of the oracle's quantised array
    of a picture stretched to [-0.15, 1.15] (the reconstruction overshoots [0, 1] on both sides), and the oracle's picture
    back from it"""
    img = synth_image(seed, c, H, W) * 1.3 - 0.15
    arr, _ = oracle.wavedec2_array(img, wavelet, "reflect", level)
    rec = thin_out(oracle.quantize(arr, Q, mults), seed)
    want = oracle.waverec2_array(oracle.dequantize(rec, Q, mults), H, W, wavelet, level)
    return rec, want


def level1_detail_bands(arr, H, W, F):
    """the three level-1 detail bands of a packed array [.., enc_h, enc_w] (views)"""
    hs, ws = band_len(H, F), band_len(W, F)
    oh, ow = arr.shape[-2] - hs, arr.shape[-1] - ws
    return arr[..., :hs, ow:ow + ws], arr[..., oh:oh + hs, :ws], arr[..., oh:oh + hs, ow:ow + ws]


def staged(ty, tx, F):
    """band rows and columns tile (ty, tx) of the inverse level stages: its own INV_TH/2 x INV_TW/2 band positions and the
    halo of F/2 - 1 behind them (dwt_inv.hip: KH, KW)"""
    hf1 = F // 2 - 1
    return slice(INV_TH // 2 * ty, INV_TH // 2 * ty + INV_TH // 2 + hf1), slice(INV_TW // 2 * tx, INV_TW // 2 * tx + INV_TW // 2 + hf1)


def occupancy_words(rec, H, W, F):
    """L1Flags words [.., gy, gx] of a packed array (common.h: L1Flags): non-zero iff a detail band holds a non-zero cell in
    the region the tile stages"""
    bands = level1_detail_bands(rec, H, W, F)
    occ = (bands[0] != 0) | (bands[1] != 0) | (bands[2] != 0)
    hs, ws = occ.shape[-2:]
    gy, gx = tiles(2 * hs - F + 2, INV_TH), tiles(2 * ws - F + 2, INV_TW)
    words = np.zeros(occ.shape[:-2] + (gy, gx), np.uint32)
    for ty in range(gy):
        for tx in range(gx):
            r, c = staged(ty, tx, F)
            words[..., ty, tx] = occ[..., r, c].any(axis=(-2, -1))
    return words


def empty_some_tiles(rec, H, W, F, seed):
    """zero, in place, the level-1 detail cells that about half the (channel, tile) pairs of the inverse level stage, so that
    their L1Flags words are zero; rec int32 [c, enc_h, enc_w]"""
    rng = np.random.default_rng(seed)
    hs, ws = band_len(H, F), band_len(W, F)
    gy, gx = tiles(2 * hs - F + 2, INV_TH), tiles(2 * ws - F + 2, INV_TW)
    for ch in range(rec.shape[0]):
        for ty in range(gy):
            for tx in range(gx):
                if rng.random() < 0.5:
                    r, c = staged(ty, tx, F)
                    for band in level1_detail_bands(rec[ch], H, W, F):
                        band[r, c] = 0
    return rec


def pf_cases(oracle, wavelet, level, integer, empty_tiles, mults=None):
    """PF_DISTINCT pictures of the persistent-inverse batch -> (recs [8, 3, enc_h, enc_w], wants [8, 3, rec_h, rec_w], H, W).
    empty_tiles: the detail bands of about half the tiles are zeroed first, so that their L1Flags words are zero.  mults: the
    call's per-channel scales (one set for the whole batch)."""
    F = len(oracle.wavelet_filters(wavelet)[0])
    H, W = (PF_REC[0] - 1, PF_REC[1] - 1) if integer else PF_REC
    recs, wants = [], []
    for k in range(PF_DISTINCT):
        rec, _ = inverse_case(oracle, wavelet, H, W, level, 900 + k, mults, c=3)
        if empty_tiles:
            empty_some_tiles(rec, H, W, F, 40 + k)
        recs.append(rec)
        wants.append(oracle.waverec2_array(oracle.dequantize(rec, Q, mults), H, W, wavelet, level))
    return np.stack(recs), np.stack(wants), H, W
