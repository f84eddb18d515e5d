"""The cases of tests/test_gpu_coder_edges.py: coefficient maxima on the steps of the start-plane rule, placements of the
maximum in the tree, arrays and byte strings that drive the coder's lists to their capacities, and batches in which no two
neighbouring images are alike -- everything that needs no GPU, so that tests/test_coder_edge_cases.py can hold the cases to
their purpose (every band non-empty, every capacity budget binding, no slot tail zero) where no GPU is.  The oracle is
passed in (the `oracle` fixture).  Nothing here is a test."""
import numpy as np

from conftest import synth_coeffs

UNLIMITED = 99999999999999999
CHUNK_SLACK = 16384           # api_coder.cpp: list_caps(), chunk_slack
SMALL_GEOMS = [(1, 8, 8, 2, 2), (3, 13, 17, 3, 5)]   # c, h, w, ll_h, ll_w; the second has duplicated tree nodes
ODD_GEOM = (3, 13, 17, 3, 5)
MID_GEOM = (2, 26, 38, 13, 19)
CAP_GEOMS = [(1, 160, 160, 5, 5), (3, 96, 137, 6, 9)]
WINDOW_GEOM = (1, 128, 128, 4, 4)
CAP_MAGNITUDE_PLANES = 24     # the band value of the capacity arrays: band(24)[0]

_band_cache = {}
# the n of the images of a batch, in turn: neighbours differ, the ends of the range come first
N_ORDER = [5, 30, 0, 29, 1] + [v for v in range(2, 29) if v != 5]


def band(oracle, k):
    """the maxima m < 2^k that the reference's `(m as f32).log2() as u8` starts at plane k, ascending: found by walking down
    from 2^k - 1 with the oracle"""
    if k not in _band_cache:
        out, m = [], (1 << k) - 1
        while m >= 1 and oracle.start_plane(m) == k:
            out.append(m)
            m -= 1
        _band_cache[k] = out[::-1]
    return list(_band_cache[k])


def in_band(oracle, m):
    """the first plane of an array with this maximum holds no significant coefficient"""
    return m > 0 and oracle.start_plane(m) > m.bit_length() - 1


def plane_maxima(oracle):
    """every maximum at which the start plane steps: around each power of two, and for the k with a band the value below
    the band, the first in it (the value just above the step of the library's threshold table) and 2^k - 1"""
    out = []
    for k in range(1, 31):
        bk = band(oracle, k)
        if bk:
            out += [bk[0] - 1, bk[0]]
        out.append((1 << k) - 1)
        if k < 30:
            out += [1 << k, (1 << k) + 1]
    return sorted(set(out))


def band_firsts(oracle):
    return {k: band(oracle, k)[0] for k in range(1, 31) if band(oracle, k)}


# ---------------------------------------------------------------- the tree

def parents_of_cells(oracle, h, w, lh, lw):
    """int [h, w]: how many nodes list the cell among their offspring (0: the root block, or a cell no tree reaches; 2 and
    more: a duplicated node, odd ll_h / ll_w)"""
    cnt = np.zeros((h, w), np.int64)
    for i in range(h):
        for j in range(w):
            off = oracle.get_offspring(i, j, h, w, lh, lw)
            for (r, s) in off or ():
                cnt[r, s] += 1
    return cnt


def node_instances(oracle, h, w, lh, lw):
    """tree-node instances of one channel, duplicates counted as the coder's lists hold them (api_coder.cpp: instance_counts)"""
    frontier = {(i, j): 1 for i in range(lh) for j in range(lw)}
    total = 0
    while frontier:
        total += sum(frontier.values())
        nxt = {}
        for (i, j), m in frontier.items():
            for cell in oracle.get_offspring(i, j, h, w, lh, lw) or ():
                nxt[cell] = nxt.get(cell, 0) + m
        frontier = nxt
    return total


def coded_cells(oracle, geom):
    """bool [c, h, w]: the cells an unlimited budget codes without loss.  With an odd ll_h or ll_w, or an odd h or w, the
    reference's index rules leave some cells outside every tree (and some sub-trees without a type-B entry): those decode
    as zero whatever they hold.  Taken from the oracle: the round trip of an array of ones."""
    c, h, w, lh, lw = geom
    d, n = oracle.encode(np.ones((c, h, w), np.int32), lh, lw, UNLIMITED)
    return oracle.decode(d, n, c, h, w, lh, lw) != 0


def is_leaf(h, w):
    """bool [h, w]: cells without offspring (encoder_decoder.rs: has offspring iff 2i+1 < h and 2j+1 < w)"""
    i, j = np.arange(h)[:, None], np.arange(w)[None, :]
    return ~((2 * i + 1 < h) & (2 * j + 1 < w))


def placements(oracle, geom):
    """[(name, (k, i, j))]: where the maximum goes"""
    c, h, w, lh, lw = geom
    out = [("root", (0, lh - 1, lw - 1)), ("leaf", (0, h - 2, w // 2 + 1)), ("last", (c - 1, h - 1, w - 1))]
    if lh % 2 or lw % 2:
        dup = np.argwhere(parents_of_cells(oracle, h, w, lh, lw) >= 2)
        i, j = (int(v) for v in dup[len(dup) // 2])
        out.append(("dup", (c // 2, i, j)))
    return out


def placed(geom, pos, m, sign, fill):
    """an array whose largest magnitude is m, at pos, with the given sign; fill: the other cells small (below 2^2, both
    signs, some zero) or zero"""
    c, h, w, lh, lw = geom
    if fill and m > 4:
        x = np.random.default_rng(m % 9973 + 17 * pos[1] + pos[2]).integers(-3, 4, (c, h, w)).astype(np.int32)
    else:
        x = np.zeros((c, h, w), np.int32)
    x[pos] = sign * m
    return x


def placed_cases(oracle, geom, values):
    """every value at every placement, both signs, the rest small and the rest zero"""
    for m in values:
        for name, pos in placements(oracle, geom):
            for sign in (1, -1):
                for fill in (False, True):
                    yield (m, name, sign, fill), placed(geom, pos, m, sign, fill)


# ---------------------------------------------------------------- capacities

def extremal_arrays(geom, M, seed=0):
    """{name: array}: every cell +-M; only the finest-level cells (those without offspring) non-zero; one non-zero cell in
    the far corner"""
    c, h, w, lh, lw = geom
    sgn = np.where(np.random.default_rng(seed).integers(0, 2, (c, h, w)) == 1, 1, -1).astype(np.int32)
    full = (sgn * np.int32(M)).astype(np.int32)
    finest = np.where(is_leaf(h, w)[None], full, 0).astype(np.int32)
    corner = np.zeros((c, h, w), np.int32)
    corner[c - 1, h - 1, w - 1] = -M
    return {"full": full, "finest": finest, "corner": corner}


def cap_pivot(geom):
    """the budget at which roots + mb + 16384 reaches c*h*w"""
    c, h, w, lh, lw = geom
    return c * h * w - c * lh * lw - CHUNK_SLACK


def cap_budgets(oracle, geom):
    """(budgets at which the LIP's budget-limited cap roots + mb + 16384 is the smaller term of list_caps(), budgets at
    which the node count is).  The node count is that of the tree's node instances: with an odd ll_h or ll_w some cells are
    reached twice and others by no tree at all, so it is not c*h*w -- the budgets on either side of both meeting points are
    here, and of the point where the LSP's cap mb/2 + 1 + 16384 meets the node count."""
    c, h, w, lh, lw = geom
    nodes = c * node_instances(oracle, h, w, lh, lw)
    roots = c * lh * lw
    meet = nodes - roots - CHUNK_SLACK
    lsp_meet = 2 * (nodes - 1 - CHUNK_SLACK)
    every = sorted({1, 64, 4000, cap_pivot(geom) - 1, cap_pivot(geom), meet - 1, meet, lsp_meet - 1, lsp_meet + 2, UNLIMITED})
    return [mb for mb in every if mb < meet], [mb for mb in every if mb >= meet]


def periodic_patterns():
    """every bit pattern of period 2 .. 8 as (period, value), bit t of the stream = bit (t mod period) of value; patterns
    that repeat a shorter one of the list are left out (the same byte strings)"""
    seen, out = set(), []
    for p in range(2, 9):
        for v in range(1 << p):
            bits = tuple((v >> (t % p)) & 1 for t in range(840))  # 840 = lcm(2..8): one canonical stretch
            if bits not in seen:
                seen.add(bits)
                out.append((p, v))
    return out


def periodic_stream(p, v, nbytes):
    bits = np.array([(v >> (t % p)) & 1 for t in range(p * 8)], np.uint8)  # p bytes: a whole number of periods
    return np.resize(np.packbits(bits, bitorder="little"), nbytes).tobytes()


def extremal_streams(nbytes):
    """distinct byte strings of this length: all ones, all zeros, every periodic pattern"""
    out = [b"\xff" * nbytes, b"\x00" * nbytes] + [periodic_stream(p, v, nbytes) for p, v in periodic_patterns()]
    return list(dict.fromkeys(out))


# ---------------------------------------------------------------- batches

def _encoder_streams(oracle, shape, nbytes, seed):
    c, h, w, lh, lw = shape
    out = []
    for s, scale in enumerate((30.0, 400.0, 6000.0, 2.0 ** 27)):
        x = synth_coeffs(seed + s, c, h, w, lh, lw, scale=scale)
        if s == 3:
            x = np.clip(x, -(1 << 30) + 1, (1 << 30) - 1).astype(np.int32)
            x[0, 0, 0] = (1 << 30) - 1 - s
        out.append(oracle.encode(x, lh, lw, 8 * nbytes))
    return out


def mixed_batch(oracle, B, shape, slot, nslots, seed):
    """-> (data uint8 [B, slot], nbytes uint64 [B], n uint8 [B], kinds [B]).  No two neighbouring images are alike; the
    lengths include 0, 1, values not divisible by 4 and exactly `slot`; n runs from 0 to 30; the content is an oracle encoder
    stream, a prefix of one, random bytes, dense ones, all ones or a periodic pattern.  Images b and b + nslots (one
    workgroup's consecutive images when slots are reused) are a list-heavy stream followed by an empty or one-byte one, or the
    reverse.  Every slot's tail past nbytes holds 0xFF or random non-zero bytes."""
    rng = np.random.default_rng(seed)
    enc = _encoder_streams(oracle, shape, slot, seed)
    pats = periodic_patterns()
    data = np.zeros((B, slot), np.uint8)
    nbytes, ns, kinds = np.zeros(B, np.uint64), np.zeros(B, np.uint8), []
    odd_lengths = [0, 1, 2, 3, 5, 7, slot - 1, slot - 2, slot - 3, slot, slot // 2 + 1, slot // 3]
    for b in range(B):
        if nslots < B and (b < B - nslots or b >= nslots):       # shares a workgroup with b - nslots or b + nslots
            role = "heavy" if ((b % nslots) + (b // nslots)) % 2 == 0 else "light"
        else:
            role = "free"
        if role == "light":
            ln = b // 2 % 2
        elif role == "heavy":
            ln = slot - [0, 1, 2, 3, 0, slot // 5, slot // 4][b % 7]
        else:
            ln = odd_lengths[b % 16] if b % 16 < len(odd_lengths) else int(rng.integers(0, slot + 1))
        ln = max(0, min(slot, ln))
        n = N_ORDER[b % 31]
        kind = ("enc", "ones", "random", "dense", "periodic", "prefix")[b % 6 if role != "heavy" else (b // 2) % 5]
        if kind in ("enc", "prefix"):
            d, n_enc = enc[(b // 6 + b // 48) % len(enc)]
            if kind == "prefix":
                d = d[:max(1, len(d) - 1 - b % 11)]
            d = (d + rng.integers(0, 256, slot, dtype=np.uint8).tobytes())[:ln] if role == "heavy" else d[:ln]
            ln = len(d)
            n = n_enc if ln >= 8 else n  # (a few bytes of it: any n)
        elif kind == "ones":
            d = b"\xff" * ln
        elif kind == "random":
            d = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        elif kind == "dense":
            d = (rng.integers(0, 256, ln, dtype=np.uint8) | rng.integers(0, 256, ln, dtype=np.uint8)).astype(np.uint8).tobytes()
        else:
            p, v = pats[(b * 37 + seed) % len(pats)]
            d = periodic_stream(p, v, ln)
        data[b, :ln] = np.frombuffer(d, np.uint8)
        data[b, ln:] = 0xFF if b % 2 == 0 else rng.integers(1, 256, slot - ln, dtype=np.uint8)
        nbytes[b], ns[b] = ln, n
        kinds.append((role, kind))
    return data, nbytes, ns, kinds


def encoder_batch(oracle, B, shape, seed):
    """int32 [B, c, h, w]: images that differ one by one -- all zero, a single huge cell, a band maximum, dense Laplace, an
    empty half"""
    c, h, w, lh, lw = shape
    rng = np.random.default_rng(seed)
    firsts = sorted(band_firsts(oracle).items())
    xs = np.zeros((B, c, h, w), np.int32)
    for b in range(B):
        kind = b % 5
        if kind == 1:
            xs[b].reshape(-1)[int(rng.integers(0, c * h * w))] = int(rng.integers(1 << 20, 1 << 30)) * (1 if b % 2 else -1)
        elif kind == 2:
            k, m = firsts[(b // 5) % len(firsts)]
            xs[b] = rng.integers(-9, 10, (c, h, w))
            xs[b].reshape(-1)[int(rng.integers(0, c * h * w))] = m + (b // 5) % 2 * (((1 << k) - 1) - m)
        elif kind == 3:
            xs[b] = np.trunc(rng.laplace(0, 1, (c, h, w)) * float(10 ** rng.uniform(0.5, 4.0)))
        elif kind == 4:
            xs[b] = np.trunc(rng.laplace(0, 1, (c, h, w)) * 200)
            xs[b, :, h // 2:, :] = 0
    return xs
