"""The cases of tests/test_gpu_batch_chunks.py, tests/test_gpu_call_sequences.py and tests/test_gpu_ordering.py: what a call
inherits -- from the chunk before it, from the call before it, from another context.  Geometries, batch sizes, input data
and the oracle's answers, everything that needs no GPU, so that tests/test_call_sequence_cases.py can hold the tables to
their purpose where no GPU is.  Nothing here is a test."""
import numpy as np

import dwt_sweep_tables as T
from conftest import synth_coeffs, synth_image

SEAM = 65535  # api.cpp: batch_chunks -- planes per launch (grid.y, and the decoder's slot limit)
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
