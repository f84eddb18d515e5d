"""The cases of tests/test_gpu_batch_chunks.py, tests/test_gpu_call_sequences.py and tests/test_gpu_ordering.py: what a call
inherits -- from the chunk before it, from the call before it, from another context.  Geometries, batch sizes, input data
and the oracle's answers, everything that needs no GPU, so that tests/test_call_sequence_cases.py can hold the tables to
their purpose where no GPU is.  Nothing here is a test."""
import numpy as np

import dwt_sweep_tables as T
from conftest import synth_coeffs, synth_image

SEAM = 65535  # api_internal.h: batch_chunks -- planes per launch (grid.y, and the decoder's slot limit)
UNLIMITED = 99999999999999999
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def chunks(B, c):
    """[(b0, nb)] as batch_chunks cuts a batch of B pictures of c planes"""
    step = max(1, SEAM // c)
    return [(b0, min(step, B - b0)) for b0 in range(0, B, step)]


# =================================================================================================== A. the chunk seam
# c * 21845 = 65535 planes exactly in the first launch, 7 pictures (21 planes) in the second
CHUNK = dict(c=3, H=8, W=8, wavelet="haar", mode="reflect", level=1, q=50.0, max_bits=400)
CHUNK_B = SEAM // 3 + 7
# the raw coder calls with one plane per picture: a chunk of exactly 65535 pictures and 5 behind it; 61 arrays in turn
ONE_PLANE = dict(c=1, h=8, w=8, ll_h=4, ll_w=4, max_bits=400)
ONE_PLANE_B = SEAM + 5
ONE_PLANE_DISTINCT = 61
# occupancy words (two levels at least): one inverse tile per plane, 3 words per picture; 127 arrays in turn
FLAGS = dict(c=3, H=16, W=24, wavelet="bior2.2", mode="reflect", level=2, q=T.Q)
FLAGS_DISTINCT = 127


def chunk_pictures():
    """uint8 [CHUNK_B, 3, 8, 8], every picture different from every other; the float pictures are these / 255"""
    def make():
        p = np.random.default_rng(20261018).integers(0, 256, (CHUNK_B, CHUNK["c"], CHUNK["H"], CHUNK["W"]), dtype=np.uint8)
        p.flags.writeable = False
        return p
    return cached("chunk_pictures", make)


def chunk_reference(O):
    """the oracle on every picture of chunk_pictures() / 255 -> dict of arrays over the whole batch: coeffs int32 [B,3,8,8],
    dcode / lcode uint8 and the masks d_where / l_where of the nodes whose code is looked up, maxabs uint32 [B], streams
    (list of bytes), nbits uint64 [B], max_n uint8 [B], rec int32 [B,3,8,8] (the decoded arrays), pics float64 [B,3,8,8],
    half float64 [B,3,4,4] (the decode at reduce = 1 = L)"""
    def make():
        k = CHUNK
        P = chunk_pictures()
        B, c = P.shape[:2]
        g = O.geometry(k["H"], k["W"], k["wavelet"], k["level"], k["mode"])
        assert (g["ll_h"], g["ll_w"], g["enc_h"], g["enc_w"], g["level"]) == (4, 4, 8, 8, 1)
        co = np.empty((B, c, 8, 8), np.int32)
        rec = np.empty((B, c, 8, 8), np.int32)
        dc, lc = np.empty((B, c, 8, 8), np.uint8), np.empty((B, c, 8, 8), np.uint8)
        pics = np.empty((B, c, 8, 8), np.float64)
        half = np.empty((B, c, 4, 4), np.float64)
        streams, nbits, max_n = [], np.empty(B, np.uint64), np.empty(B, np.uint8)
        has = None
        for b in range(B):
            arr, _ = O.wavedec2_array(P[b] / 255, k["wavelet"], k["mode"], k["level"])
            co[b] = O.quantize(arr, k["q"], None)
            dc[b], lc[b], has = O.set_codes(co[b], 4, 4)
            d, n, nb = O.encode_nbits(co[b], 4, 4, k["max_bits"])
            streams.append(d)
            nbits[b], max_n[b] = nb, n
            rec[b] = O.decode(d, n, c, 8, 8, 4, 4)
            D = O.dequantize(rec[b], k["q"], None)
            pics[b] = O.waverec2_array(D, k["H"], k["W"], k["wavelet"], k["level"], k["mode"])
            half[b] = D[:, :4, :4] * 0.5
        I, J = np.arange(8)[:, None], np.arange(8)[None, :]
        b_entry = ((4 * I + 3 < 8) & (4 * J + 3 < 8))[None]
        out = dict(coeffs=co, dcode=dc, lcode=lc, d_where=has, l_where=has & b_entry, streams=streams, nbits=nbits, max_n=max_n,
                   rec=rec, pics=pics, half=half, maxabs=np.abs(co.astype(np.int64)).max(axis=(1, 2, 3)).astype(np.uint32))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        return out
    return cached("chunk_reference", make)


def chunk_coeffs_f32(O):
    """the single-precision transform of the same pictures (float32 of P / 255) -> int32 [B,3,8,8]"""
    def make():
        k = CHUNK
        P = chunk_pictures()
        co = np.empty(P.shape, np.int32)
        for b in range(len(P)):
            arr, _ = O.wavedec2_array_f32((P[b] / 255).astype(np.float32), k["wavelet"], k["mode"], k["level"])
            co[b] = O.quantize_f32(arr, k["q"], None)
        co.flags.writeable = False
        return co
    return cached("chunk_coeffs_f32", make)


def slots_of(streams, slot):
    """uint8 [B, slot]: the streams, zeros behind each (what an encoder call leaves in its slots)"""
    out = np.zeros((len(streams), slot), np.uint8)
    for b, d in enumerate(streams):
        out[b, :len(d)] = np.frombuffer(d, np.uint8)
    return out


def one_plane_reference(O):
    """61 arrays of one 8 x 8 plane: xs int32 [61,1,8,8], their streams, nbits, max_n, decoded arrays and D / L codes"""
    def make():
        k = ONE_PLANE
        geom = (k["c"], k["h"], k["w"], k["ll_h"], k["ll_w"])
        xs = np.stack([synth_coeffs(3000 + i, *geom, scale=float(30 * (1 + i % 7))) for i in range(ONE_PLANE_DISTINCT)])
        streams, nbits, max_n, rec = [], [], [], []
        for x in xs:
            d, n, nb = O.encode_nbits(x, k["ll_h"], k["ll_w"], k["max_bits"])
            streams.append(d)
            nbits.append(nb)
            max_n.append(n)
            rec.append(O.decode(d, n, *geom))
        return dict(xs=xs, streams=streams, nbits=np.array(nbits, np.uint64), max_n=np.array(max_n, np.uint8), rec=np.stack(rec))
    return cached("one_plane_reference", make)


def flags_reference(O):
    """127 coefficient arrays of the FLAGS geometry with the level-1 detail bands of about half the (plane, tile) pairs
    emptied, their occupancy words as dwt_sweep_tables.occupancy_words makes them, and the oracle's pictures"""
    def make():
        k = FLAGS
        F = len(O.wavelet_filters(k["wavelet"])[0])
        recs, wants = [], []
        for i in range(FLAGS_DISTINCT):
            rec, _ = T.inverse_case(O, k["wavelet"], k["H"], k["W"], k["level"], 5000 + i, None, c=k["c"])
            T.empty_some_tiles(rec, k["H"], k["W"], F, 70 + i)
            recs.append(rec)
            wants.append(O.waverec2_array(O.dequantize(rec, k["q"], None), k["H"], k["W"], k["wavelet"], k["level"]))
        recs = np.stack(recs)
        return dict(rec=recs, words=T.occupancy_words(recs, k["H"], k["W"], F), pics=np.stack(wants))
    return cached("flags_reference", make)


# ---- the seam once more, at a geometry whose sizes all differ ------------------------------------------------------
# At CHUNK every per-picture size is 3 * 64 (H W = rec_H rec_W = enc_h enc_w, the reduced picture is the root block), and at
# FLAGS rec_H = H: a launch that stepped its pictures by the wrong one of them would land on the right picture all the same.
# SEAM2: hs = [17, 11, 8], ws = [25, 15, 10]; the array is 27 x 35, the float64 picture 18 x 26, the approximation plane of
# the two-part inverse 12 x 16 (which is also the float64 picture at reduce = 1: the same number by definition), the root
# block 8 x 10 (the float64 picture at reduce = 2 = L), the reduced integer pictures 11 x 15 and 8 x 10.  The budget cuts
# every stream short.  127 pictures in turn: 21845 % 127 = 1.
SEAM2 = dict(c=3, H=17, W=25, wavelet="bior2.2", mode="reflect", level=2, q=50.0, max_bits=4000)
SEAM2_DISTINCT = 127
# the two-pass route (k_dwt_axis_ext / k_dwt_pack_ext, k_idwt_axis_per, and the conversion passes k_px_to_f64 / k_f64_to_px
# around them for integer and float-kind pixels): periodization, hs = [9, 5], ws = [13, 7], array and float64 picture 10 x 14
SEAM_PER = dict(c=3, H=9, W=13, wavelet="db2", mode="periodization", level=1, q=50.0, max_bits=900)
SEAM_PER_DISTINCT = 127


def seam_pictures(k, distinct):
    """uint8 [distinct, c, H, W]: the pictures that take turns through the batch of case k (picture b is b % distinct)"""
    def make():
        p = np.random.default_rng(20261020 + k["H"]).integers(0, 256, (distinct, k["c"], k["H"], k["W"]), dtype=np.uint8)
        p.flags.writeable = False
        return p
    return cached(("seam_pictures", k["H"], k["W"], distinct), make)


def in_turn(distinct, B=None):
    """which of the distinct pictures stands at each place of the batch"""
    return np.arange(CHUNK_B if B is None else B) % distinct


def seam2_sizes(O):
    """the per-picture element counts the offsets of a chunk are multiples of (api_image.cpp, api_coder.cpp; each times b0), from the oracle's
    geometry -> dict"""
    k = SEAM2
    g = O.geometry(k["H"], k["W"], k["wavelet"], k["level"], k["mode"])
    F = len(O.wavelet_filters(k["wavelet"])[0])
    c, L = k["c"], g["level"]
    rec = lambda n: 2 * n - F + 2  # noqa: E731  (what one inverse level returns for a band of n)
    return dict(picture=c * k["H"] * k["W"], rec=c * rec(g["hs"][1]) * rec(g["ws"][1]), array=c * g["enc_h"] * g["enc_w"],
                approx=c * rec(g["hs"][2]) * rec(g["ws"][2]), reduced1=c * rec(g["hs"][2]) * rec(g["ws"][2]),
                reduced2=c * g["hs"][L] * g["ws"][L], reduced1_int=c * g["hs"][1] * g["ws"][1])


def _reduced(O, D, k, g, r):
    """R_r of a dequantised array [c, enc_h, enc_w] (tests/test_gpu_reduced.py: want_reduced; tests/test_reduced_cpu.py:
    oracle_reduced): the corner of the array is the array of the hs[r] x ws[r] picture at L - r levels; its inverse transform
    times 2^-r; at r = L the root block times 2^-L"""
    L = g["level"]
    if r == L:
        return np.ascontiguousarray(D[:, :g["ll_h"], :g["ll_w"]]) * 2.0 ** -L
    gk = O.geometry(g["hs"][r], g["ws"][r], k["wavelet"], L - r, k["mode"])
    sub = np.ascontiguousarray(D[:, :gk["enc_h"], :gk["enc_w"]])
    return O.waverec2_array(sub, g["hs"][r], g["ws"][r], k["wavelet"], L - r, k["mode"]) * 2.0 ** -r


def _frozen(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


def seam_reference(O, k, distinct):
    """the oracle on the distinct pictures of case k (/ 255) -> dict of arrays over them, read-only (picture b of the batch is
    b % distinct): coeffs int32 [D, c, enc_h, enc_w] with dcode / lcode, the masks d_where / l_where and maxabs as
    chunk_reference has them; coeffs_f32 (the single-precision transform of float32(P / 255)); streams, nbits, max_n of
    coeffs, and streams_f32, nbits_f32, max_n_f32 of coeffs_f32; rec (the decoded arrays); pics float64 [D, c, rec_h, rec_w];
    geom (the oracle's geometry).  With two levels or more also: red[r] for r = 1 .. L (the reduced pictures, float64,
    uncropped); approx = 2 red[1], what the coarse half of the two-part inverse leaves; rec_fl, a copy of rec with the level-1
    detail bands of about half the (plane, tile) pairs emptied, its occupancy words (dwt_sweep_tables.occupancy_words) and
    its pictures pics_fl.  Host time, once per process: 0.5 s for SEAM2's 127 pictures, under 0.1 s for SEAM_PER's."""
    def make():
        P = seam_pictures(k, distinct)
        c, H, W, wv, md, lv, q = k["c"], k["H"], k["W"], k["wavelet"], k["mode"], k["level"], k["q"]
        g = O.geometry(H, W, wv, lv, md)
        F = len(O.wavelet_filters(wv)[0])
        eh, ew, lh, lw = g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"]
        out = dict(coeffs=[], coeffs_f32=[], dcode=[], lcode=[], streams=[], nbits=[], max_n=[], streams_f32=[], nbits_f32=[],
                   max_n_f32=[], rec=[], pics=[])
        two = g["level"] >= 2
        if two:
            out.update(rec_fl=[], pics_fl=[])
            red = {r: [] for r in range(1, g["level"] + 1)}
        has = None
        for i in range(distinct):
            co = O.quantize(O.wavedec2_array(P[i] / 255, wv, md, lv)[0], q, None)
            co32 = O.quantize_f32(O.wavedec2_array_f32((P[i] / 255).astype(np.float32), wv, md, lv)[0], q, None)
            dc, lc, has = O.set_codes(co, lh, lw)
            d, n, nb = O.encode_nbits(co, lh, lw, k["max_bits"])
            d32, n32, nb32 = O.encode_nbits(co32, lh, lw, k["max_bits"])
            rec = O.decode(d, n, c, eh, ew, lh, lw)
            D = O.dequantize(rec, q, None)
            for name, v in (("coeffs", co), ("coeffs_f32", co32), ("dcode", dc), ("lcode", lc), ("streams", d), ("nbits", nb),
                            ("max_n", n), ("streams_f32", d32), ("nbits_f32", nb32), ("max_n_f32", n32), ("rec", rec),
                            ("pics", O.waverec2_array(D, H, W, wv, lv, md))):
                out[name].append(v)
            if two:
                for r in red:
                    red[r].append(_reduced(O, D, k, g, r))
                fl = T.empty_some_tiles(rec.copy(), H, W, F, 70 + i)
                out["rec_fl"].append(fl)
                out["pics_fl"].append(O.waverec2_array(O.dequantize(fl, q, None), H, W, wv, lv, md))
        for name, dt in (("nbits", np.uint64), ("max_n", np.uint8), ("nbits_f32", np.uint64), ("max_n_f32", np.uint8)):
            out[name] = np.array(out[name], dt)
        for name in out:
            if isinstance(out[name], list) and not name.startswith("streams"):
                out[name] = np.stack(out[name])
        I, J = np.arange(eh)[:, None], np.arange(ew)[None, :]
        out.update(d_where=has, l_where=has & ((4 * I + 3 < eh) & (4 * J + 3 < ew))[None], geom=g,
                   maxabs=np.abs(out["coeffs"].astype(np.int64)).max(axis=(1, 2, 3)).astype(np.uint32))
        if two:
            out["red"] = {r: np.stack(v) for r, v in red.items()}
            for v in out["red"].values():
                v.flags.writeable = False
            out["approx"] = out["red"][1] * 2.0  # (exact: the reduced picture is the approximation times 2^-1)
            out["words"] = T.occupancy_words(out["rec_fl"], H, W, F)
        return _frozen(out)
    return cached(("seam_reference", k["H"], k["W"], k["mode"], distinct), make)


def seam2_reference(O):
    return seam_reference(O, SEAM2, SEAM2_DISTINCT)


def seam_per_reference(O):
    return seam_reference(O, SEAM_PER, SEAM_PER_DISTINCT)


# ---- padded views: every stride differs from the dense one ---------------------------------------------------------
PAD_BYTE = 0x7F  # (the guard byte of tests/test_gpu_coder_edges.py)


def padded_strides(c, H, W, es):
    """byte strides (sb, sc, sh, sw) of a channels-last view with one spare sample behind the c of every pixel (RGBA-like),
    three spare samples behind every row and two spare rows behind every picture: none of sb, sh, sw is the dense HWC one"""
    sw = (c + 1) * es
    sh = W * sw + 3 * es
    return np.array([(H + 2) * sh, es, sh, sw], np.int64)


def padded_buffer(B, c, H, W, dtype):
    """-> (host buffer [B, sb / es] of dtype, every byte the guard byte; its view [B, c, H, W] of the samples; the strides).
    For a float kind take the unsigned integer of its size (the guard pattern is a NaN in float16)."""
    dtype = np.dtype(dtype)
    st = padded_strides(c, H, W, dtype.itemsize)
    buf = np.full((B, int(st[0])), PAD_BYTE, np.uint8).view(dtype)
    return buf, samples_of(buf, c, H, W), st


def samples_of(buf, c, H, W):
    """the [B, c, H, W] view of the samples in a buffer [B, sb / es] laid out by padded_strides"""
    st = padded_strides(c, H, W, buf.dtype.itemsize)
    assert buf.ndim == 2 and buf.flags.c_contiguous and buf.shape[1] * buf.dtype.itemsize == st[0]
    return np.lib.stride_tricks.as_strided(buf, (len(buf), c, H, W), tuple(int(v) for v in st))


def padding_untouched(buf, c, H, W):
    """every byte of the buffer that is no sample still holds the guard byte"""
    b = np.array(buf.view(np.dtype("u%d" % buf.dtype.itemsize)), copy=True)
    samples_of(b, c, H, W)[...] = int.from_bytes(bytes([PAD_BYTE]) * b.dtype.itemsize, "little")
    return bool((b.view(np.uint8) == PAD_BYTE).all())


# =================================================================================== B. what a call leaves behind
# the probe: one small fused round trip whose answers the oracle gives
PROBE = dict(B=2, c=3, H=70, W=90, wavelet="bior2.2", mode="reflect", level=None, q=50.0, max_bits=int(70 * 90 * 0.5))
# larger pictures at a rate that fills the array: the internal array grows, and more cells are written than the probe's has
DENSE = dict(B=3, c=3, H=150, W=200, wavelet="bior2.2", mode="reflect", level=None, q=400.0, max_bits=None)
# an odd LL block in both directions: duplicated tree nodes, and padding cells inside the array
ODD_LL = dict(B=9, c=3, H=70, W=90, wavelet="bior2.2", mode="reflect", level=3, q=50.0, max_bits=None)
# more pictures than the list decoder has slots at most (8 per CU, 256 CUs): slots are reused inside the launch
MAX_DECODER_SLOTS = 2048
TINY = dict(B=MAX_DECODER_SLOTS + 37, c=1, H=8, W=8, wavelet="haar", mode="reflect", level=1, q=50.0, max_bits=300, distinct=13)
# small, large, small
SMALL = dict(B=2, c=1, H=33, W=47, wavelet="haar", mode="reflect", level=2, q=50.0, max_bits=2000)
# long filters: two of 22 taps (the device copy keeps its size, only its contents change), and one in single precision
LONG_FILTERS = ["db11", "sym11", "coif4"]
LONG = dict(B=2, c=2, H=61, W=83, mode="reflect", level=2, q=T.Q)
# decoder width and occupancy words, alternating on one geometry of several level-1 tiles: (wavefronts, l1_flags)
WIDTHS = dict(B=3, c=3, H=129, W=257, wavelet="bior2.2", mode="reflect", level=3, q=50.0, max_bits=int(129 * 257 * 0.5))
WIDTH_SETTINGS = [(8, 0), (12, 1), (8, 1), (12, 0), (8, 0), (12, 1)]
# the persistent inverse's tile counters: workgroups per CU of the four runs, a small launch of another geometry between them
PF_GROUPS = [4, 3, 1, 4]
PF_WAVELET = "bior2.2"
# spiht_unscatter_lists_batch_i32
UNSCATTER = dict(B=3, c=2, h=40, w=56, ll_h=5, ll_w=7, max_bits=6000)
# channel scales back to back: (c, scales)
SCALES = [(3, [2.0, 0.75, 1.5]), (3, [1.0, 0.2, 0.3]), (3, [2.0, 0.75, 1.5]), (3, None), (2, [0.5, 4.0])]
SCALED = dict(B=2, H=40, W=56, wavelet="bior2.2", mode="reflect", level=2, q=50.0, max_bits=6000)


def pictures(k, seed):
    return np.stack([synth_image(seed + 7 * b, k["c"], k["H"], k["W"]) for b in range(k["B"])])


def image_reference(O, k, imgs, mults=None):
    """the oracle's round trip of the pictures imgs [B, c, H, W] under case k -> (streams, max_n, pictures float64
    [B, c, rec_h, rec_w], decoded arrays int32 [B, c, enc_h, enc_w])"""
    streams, ns, pics, recs = [], [], [], []
    for img in imgs:
        d, n, g = O.encode_image(img, k["wavelet"], k["mode"], k["level"], k["q"], mults, k["max_bits"])
        rec = O.decode(d, n, img.shape[0], g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"])
        streams.append(d)
        ns.append(n)
        recs.append(rec)
        pics.append(O.waverec2_array(O.dequantize(rec, k["q"], mults), k["H"], k["W"], k["wavelet"], k["level"], k["mode"]))
    return streams, ns, np.stack(pics), np.stack(recs)


def probe_reference(O):
    return cached("probe", lambda: (pictures(PROBE, 4100),) + image_reference(O, PROBE, pictures(PROBE, 4100)))


def decoded_pictures(O, k, streams, ns, mults=None):
    """the oracle's decode_image of arbitrary (stream, n) pairs under case k -> float64 [B, c, rec_h, rec_w]"""
    return np.stack([O.decode_image(d, n, k["c"], k["H"], k["W"], k["wavelet"], k["level"], k["q"], mults, mode=k["mode"])
                     for d, n in zip(streams, ns)])


def arbitrary_streams(B):
    """byte strings no encoder made, as test_decode_arbitrary_bytes has them: uniform bytes of several lengths, and
    strings dense in ones (many significance hits: duplicated cells get written by all their list entries) -> (streams, ns)"""
    rng = np.random.default_rng(5)
    streams, ns = [], []
    for i in range(B):
        ln = [1, 3, 17, 200, 1500, 40, 600, 900, 2500][i % 9]
        a = rng.integers(0, 256, ln, dtype=np.uint8)
        if i % 9 >= 5:
            a = a | rng.integers(0, 256, ln, dtype=np.uint8)
        streams.append(a.astype(np.uint8).tobytes())
        ns.append([9, 3, 0, 6][i % 4])
    return streams, ns


def duplicated_cells(O, geom):
    """cells of a [h, w] plane that are offspring of more than one node (encoder_decoder.rs:43-75 on an odd LL block)"""
    c, h, w, lh, lw = geom
    seen = np.zeros((h, w), np.int32)
    for i in range(h):
        for j in range(w):
            off = O.get_offspring(i, j, h, w, lh, lw)
            for (y, x) in off or []:
                seen[y, x] += 1
    return int((seen > 1).sum())


def padding_cells(O, k):
    """bool [enc_h, enc_w]: the cells of the packed array that belong to no band (coeffs_to_array leaves them zero): zero in
    the transforms of two different noise pictures"""
    rng = np.random.default_rng(8)
    pad = None
    for _ in range(2):
        arr, _g = O.wavedec2_array(rng.random((1, k["H"], k["W"])) + 0.5, k["wavelet"], k["mode"], k["level"])
        pad = (arr[0] == 0.0) if pad is None else pad & (arr[0] == 0.0)
    return pad


def tiny_pictures():
    k = TINY
    base = np.random.default_rng(99).integers(0, 256, (k["distinct"], k["c"], k["H"], k["W"]), dtype=np.uint8) / 255
    return base[np.arange(k["B"]) % k["distinct"]]


# =========================================================================== C. the first call after a wait on other contexts
# the list-coder cases: batch size and geometry of test_pipeline_u8_at_batch_size
LIST = dict(B=40, c=3, H=541, W=961, wavelet="bior2.2", mode="reflect", level=None, q=50.0, max_bits=int(541 * 961 * 0.5), distinct=10)
# everything else
REST = dict(B=6, c=2, H=40, W=56, wavelet="bior2.2", mode="reflect", level=2, q=50.0, max_bits=5000)
GATE_US = 3000  # each producer's queue starts behind the library's bounded gate on a word that stays 0
ROUNDS = 2      # the defect of the encoder's fill showed in the second step


def list_pictures():
    """40 pictures: 10 generated ones in turn (the oracle takes a third of a second for each at this size)"""
    def make():
        k = LIST
        base = [synth_image(700 + i, k["c"], k["H"], k["W"]) for i in range(k["distinct"])]
        return np.stack([base[b % len(base)] for b in range(k["B"])])
    return cached("list_pictures", make)


def list_reference(O):
    """the oracle on the 10 distinct pictures -> lists of 10 (picture b of the batch is b % 10): coefficient arrays, streams,
    bit counts, max_n and decoded arrays; and the geometry"""
    def make():
        k = LIST
        P = list_pictures()
        streams, ns, nbits, recs, coeffs = [], [], [], [], []
        for i in range(k["distinct"]):
            arr, g = O.wavedec2_array(P[i], k["wavelet"], k["mode"], k["level"])
            co = O.quantize(arr, k["q"], None)
            d, n, nb = O.encode_nbits(co, g["ll_h"], g["ll_w"], k["max_bits"])
            streams.append(d)
            ns.append(n)
            nbits.append(nb)
            coeffs.append(co)
            recs.append(O.decode(d, n, k["c"], g["enc_h"], g["enc_w"], g["ll_h"], g["ll_w"]))
        return dict(streams=streams, max_n=ns, nbits=nbits, rec=recs, coeffs=coeffs, geom=g)
    return cached("list_reference", make)


def round_order(B, r):
    """which picture stands where in round r: the second round has the batch back to front"""
    return np.arange(B) if r % 2 == 0 else np.arange(B)[::-1]


def orders(B, r):
    """(the producers' order of the pictures in round r, the consumer's own: another picture in every place)"""
    po = round_order(B, r)
    return po, np.roll(po, 1 + r)
