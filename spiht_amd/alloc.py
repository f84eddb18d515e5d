"""Rate allocation across the tiles of a picture: the rule, in Python and numpy, with no device.

Every tile of a tiled picture is an embedded stream, so any byte prefix of it is a stream.  A tile coded past its share of
the budget and measured at K prefixes has a rate-distortion curve; cutting every tile where one more byte buys the same
drop in distortion (equal slope on the lower convex hull of the curves) spends a fixed total where it helps most.  This
module is the statement the kernel spiht_tile_allocate (csrc/alloc.hip) is held to, bit for bit: every slope is one rounded
float64 subtraction and one rounded float64 division, and nothing else here rounds.
"""
import math

import numpy as np

SPREAD = 4.0
POINTS = 16
MAX_POINTS = 255


def points_arg(points):
    if isinstance(points, bool) or not isinstance(points, (int, np.integer)):
        raise TypeError("points must be an integer, not %s" % type(points).__name__)
    if not 1 <= points <= MAX_POINTS:
        raise ValueError("points = %d: 1 .. %d lengths per tile" % (points, MAX_POINTS))
    return int(points)


def spread_arg(spread):
    if isinstance(spread, bool) or not isinstance(spread, (int, float, np.integer, np.floating)):
        raise TypeError("spread must be a number, not %s" % type(spread).__name__)
    spread = float(spread)
    if not spread >= 1.0 or math.isinf(spread):
        raise ValueError("spread = %r: a finite factor >= 1" % spread)
    return spread


def allocate_arg(allocate):
    if allocate not in (None, "rd"):
        raise ValueError('allocate is None or "rd", not %r' % (allocate,))
    return allocate


def ceiling_bits(max_bits, T, spread=SPREAD):
    """the bit budget every tile is coded with before the cut: min(max_bits, floor(spread * (max_bits // T))), rounded down
    to whole bytes -- so a full stream either ends by itself or has exactly that many bits, and every prefix of L >= 1 bytes
    is encode_image(tile, max_bits=8 L)"""
    max_bits, T = int(max_bits), int(T)
    if max_bits < 0 or T < 1:
        raise ValueError("ceiling_bits: max_bits >= 0 and T >= 1")
    return min(max_bits, math.floor(spread_arg(spread) * (max_bits // T))) // 8 * 8


def tile_lengths(n, K):
    """the K + 1 candidate byte lengths of a stream of n bytes: R[k] = ceil(n k / K); R[0] = 0, R[K] = n"""
    n, K = int(n), points_arg(K)
    return [-(-n * k // K) for k in range(K + 1)]


def _f64(D):
    """float64 with one rounding: exact integer sums (Python ints, uint64) round once, floats are taken as they are"""
    return [float(int(v)) if isinstance(v, (int, np.integer)) else float(v) for v in D]


def slope(R, D, a, b):
    """(D[a] - D[b]) / float64(R[b] - R[a]): distortion dropped per byte from a to b; one rounded subtraction, one rounded
    division"""
    return float((np.float64(D[a]) - np.float64(D[b])) / np.float64(int(R[b]) - int(R[a])))


def lower_hull(R, D):
    """indices of the lower convex hull of the points (R[k], D[k]), k = 0 .. K, from k = 0; R non-decreasing.  A point no
    longer than the top, or not strictly better, is skipped (curves need not be monotone); the edges' slopes are strictly
    decreasing."""
    D = _f64(D)
    s = [0]
    for k in range(1, len(R)):
        if R[k] == R[s[-1]] or not D[k] < D[s[-1]]:
            continue
        while len(s) >= 2 and slope(R, D, s[-2], s[-1]) <= slope(R, D, s[-1], k):
            s.pop()
        s.append(k)
    return s


def hull_edges(R, D):
    """the hull edges of all tiles, tile by tile: (slope, delta R, R of the end vertex, tile)"""
    edges = []
    for t in range(len(R)):
        Dt = _f64(D[t])
        h = lower_hull(R[t], Dt)
        for a, b in zip(h, h[1:]):
            edges.append((slope(R[t], Dt, a, b), int(R[t][b]) - int(R[t][a]), int(R[t][b]), t))
    return edges


def allocate(R, D, budget_bytes):
    """R, D: [T][K + 1] candidate lengths and their distortions; budget_bytes: the bytes of all tiles together.
    -> (bytes per tile, lambda*).  lambda* is the smallest edge slope whose edges and all steeper ones fit the budget (inf if
    none does): every tile goes to the last vertex it reaches over edges of slope >= lambda*.  What is left of the budget goes
    to the edges of the next slope below, min(delta R, rest) each in tile order -- a partial edge is a valid prefix.  The sum
    is min(budget_bytes, the tiles' last hull vertices together)."""
    budget = int(budget_bytes)
    if budget < 0:
        raise ValueError("budget_bytes = %d is negative" % budget)
    edges = hull_edges(R, D)
    lam, cost = math.inf, 0
    by_slope = {}
    for s, dr, _, _ in edges:
        by_slope[s] = by_slope.get(s, 0) + dr
    for s in sorted(by_slope, reverse=True):  # cost(s) grows as s falls: the last slope that still fits
        cost += by_slope[s]
        if cost > budget:
            break
        lam = s
    out = [0] * len(R)
    for s, _, end, t in edges:
        if s >= lam:
            out[t] = max(out[t], end)
    rest = budget - sum(out)
    below = [e[0] for e in edges if e[0] < lam]
    if below:
        nxt = max(below)
        for s, dr, _, t in edges:  # at most one edge of a slope per tile, the tiles ascending
            if s == nxt and rest > 0:
                give = min(dr, rest)
                out[t] += give
                rest -= give
    return out, lam


ROI_MAX_TILE_SAMPLES = 2 ** 24


def roi_arg(roi, N, H, W):
    """a weight map of a call on N pictures of H x W -> contiguous uint8 [H, W] (one map for all pictures) or [N, H, W].
    roi: a bool or uint8 array of either shape (True is weight 1).  Another dtype: TypeError; another shape: ValueError.

    The map steers allocate="rd": the table the tiles are cut by holds, for tile (i, j) of th x tw with valid extent vh x vw and
    candidate k, D_w[t][k] = sum over the channels and y < vh, x < vw of w[i th + y, j tw + x] * (p - d)^2 -- the same weight for
    every channel.  Integer pictures: exact in uint64, for c th tw <= ROI_MAX_TILE_SAMPLES (255 * 65535^2 * 2^24 < 2^64).
    float64: every term float64(w) * ((p - d) * (p - d)), three roundings, added in the order of the unweighted sum, so a map
    of ones gives the unweighted table in every bit.  tile_lengths, lower_hull, allocate and allocate_layers are unchanged: a
    tile whose weights are all zero has D = 0 at every k, its hull is the single vertex 0, and it gets no bytes."""
    roi = np.asarray(roi)
    if roi.dtype != np.bool_ and roi.dtype != np.uint8:
        raise TypeError("roi must be a bool or uint8 array, not %s" % roi.dtype)
    if roi.shape != (int(H), int(W)) and roi.shape != (int(N), int(H), int(W)):
        raise ValueError("roi of shape %s: the weights of %d picture(s) are [%d, %d] or [%d, %d, %d]"
                         % (roi.shape, N, H, W, N, H, W))
    return np.ascontiguousarray(roi).view(np.uint8)


def roi_map(H, W, boxes, weight=255, background=1):
    """uint8 [H, W]: `background` everywhere, `weight` inside every box (y0, x0, h, w) of `boxes`; a box (y0, x0, h, w, weight)
    carries its own weight.  Boxes are clipped to the picture; where boxes overlap, the larger weight holds.  Weights are
    integers in 0 .. 255, else ValueError."""
    def weight_arg(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 255:
            raise ValueError("%s = %r: an integer in 0 .. 255" % (name, v))
        return int(v)
    weight, background = weight_arg("weight", weight), weight_arg("background", background)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("a %d x %d picture" % (H, W))
    inside = np.full((H, W), -1, dtype=np.int16)  # the largest weight of the boxes that hold the pixel; -1: none does
    for box in boxes:
        if len(box) not in (4, 5):
            raise ValueError("a box is (y0, x0, h, w) or (y0, x0, h, w, weight), not %r" % (tuple(box),))
        y0, x0, h, w = [int(v) for v in box[:4]]
        wt = weight_arg("a box's weight", box[4]) if len(box) == 5 else weight
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
        if ya < yb and xa < xb:
            inside[ya:yb, xa:xb] = np.maximum(inside[ya:yb, xa:xb], wt)
    return np.where(inside >= 0, inside, background).astype(np.uint8)


MAX_LAYERS = 255


def layer_budgets(max_bits, layers):
    """the bit budgets of the Q quality layers of a tiled picture, 1 <= Q <= MAX_LAYERS, the last one max_bits.
    layers: an int Q -- [max_bits >> (Q - 1 - q) for q in range(Q)], every layer twice the one before (ValueError if these
    do not strictly increase: max_bits is too small for Q halvings); or a sequence of strictly increasing non-negative ints
    whose last entry is max_bits.  The byte budget of a layer is bits // 8, as for allocate="rd"; two layers of the same
    byte budget are ordinary (the later one is empty)."""
    if isinstance(max_bits, bool) or not isinstance(max_bits, (int, np.integer)):
        raise TypeError("max_bits must be an integer, not %s" % type(max_bits).__name__)
    max_bits = int(max_bits)
    if max_bits < 0:
        raise ValueError("max_bits = %d is negative" % max_bits)
    if isinstance(layers, bool) or isinstance(layers, (str, bytes)):
        raise TypeError("layers must be an integer or a sequence of integers, not %s" % type(layers).__name__)
    if isinstance(layers, (int, np.integer)):
        Q = int(layers)
        if not 1 <= Q <= MAX_LAYERS:
            raise ValueError("layers = %d: 1 .. %d layers" % (Q, MAX_LAYERS))
        out = [max_bits >> (Q - 1 - q) for q in range(Q)]
        if any(b <= a for a, b in zip(out, out[1:])):
            raise ValueError("layers = %d: halving max_bits = %d that often does not give increasing budgets" % (Q, max_bits))
        return out
    try:
        seq = list(layers)
    except TypeError:
        raise TypeError("layers must be an integer or a sequence of integers, not %s" % type(layers).__name__)
    for b in seq:
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)):
            raise TypeError("a layer's budget must be an integer, not %s" % type(b).__name__)
    out = [int(b) for b in seq]
    if not 1 <= len(out) <= MAX_LAYERS:
        raise ValueError("%d layers: 1 .. %d" % (len(out), MAX_LAYERS))
    if out[0] < 0 or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("the layers' budgets must be non-negative and strictly increasing: %r" % (out,))
    if out[-1] != max_bits:
        raise ValueError("the last layer's budget is %d, max_bits is %d" % (out[-1], max_bits))
    return out


def allocate_layers(R, D, budgets_bytes):
    """R, D: [T][K + 1] as for allocate; budgets_bytes: Q non-decreasing byte budgets.  -> (cum, lams): cum[q], lams[q] =
    allocate(R, D, budgets_bytes[q]).

    The rows NEST: cum[q][t] <= cum[q + 1][t] for every tile, and lams[q] >= lams[q + 1] -- so a tile's stream cut at cum[q][t]
    is a prefix of its stream cut at cum[q + 1][t], and the bytes between them are what layer q + 1 adds.  Why: the cost of
    the edges of slope >= s grows as s falls, so for budgets b1 <= b2, lambda*(b2) <= lambda*(b1).  A tile's hull edges have
    strictly decreasing slopes, so the edges it takes at b1 (those of slope >= lambda*(b1)) are the first of those it takes at
    b2.  If lambda*(b2) < lambda*(b1), the slope the rest of b1 went to is >= lambda*(b2): those edges, partial at b1, are
    whole at b2.  If the two are equal, the same next slope takes min(delta R, rest) in tile order, and what a tile gets does
    not fall as the rest grows.  The last row is what allocate="rd" gives for the whole budget."""
    budgets = [int(b) for b in budgets_bytes]
    if any(b < a for a, b in zip(budgets, budgets[1:])):
        raise ValueError("budgets_bytes must not fall: %r" % (budgets,))
    cum, lams = [], []
    for b in budgets:
        out, lam = allocate(R, D, b)
        cum.append(out)
        lams.append(lam)
    return cum, lams


# ---- a target quality in place of a size -------------------------------------------------------------------------------------

SUM_LANES = 256


def total_distortion(values):
    """the float64 sum of T non-negative float64 values in an order fixed by T alone -- the order of a 256-thread workgroup
    (k_tile_allocate_target, csrc/alloc.hip, adds in it):
      1. accumulator i of 256 starts at +0.0 and adds values[i], values[i + 256], ... in ascending order;
      2. within each run of 64 accumulators, six rounds x[i] <- x[i] + x[i ^ off], off = 32, 16, 8, 4, 2, 1 (addition
         commutes, so after them all 64 hold the same bits);
      3. the four results are added in order, ((r0 + r1) + r2) + r3.
    Every addition is rounded to nearest once.  A rounded addition does not fall when an operand grows, and the order does not
    depend on the values, so the sum is MONOTONE in every term: raising one value never lowers it.  allocate_target relies on
    that -- the total over the vertices reached does not rise as the slope falls."""
    v = np.asarray(_f64(values), dtype=np.float64)
    rounds = -(-len(v) // SUM_LANES)
    acc = np.zeros(SUM_LANES)
    if rounds:  # (a missing value adds nothing; + 0.0 leaves a non-negative accumulator as it is)
        for row in np.concatenate([v, np.zeros(rounds * SUM_LANES - len(v))]).reshape(rounds, SUM_LANES):
            acc = acc + row
    lane = np.arange(SUM_LANES)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ off]
    return float(((acc[0] + acc[64]) + acc[128]) + acc[192])


def target_sqerr(db, peak, c, weight_sum):
    """the squared error of a c-channel picture at a PSNR of db: float(c * weight_sum) * (peak * peak) / 10 ** (db / 10).
    weight_sum: H * W without a weight map, the Python-int sum of the uint8 map with one -- a map of ones gives the unweighted
    target in every bit.  The PSNR of a (weighted) squared error is rd.psnr_of(dist / (c * weight_sum), peak).  db: a finite
    number, else TypeError / ValueError; weight_sum = 0 (a map of zeros): ValueError."""
    if isinstance(db, bool) or not isinstance(db, (int, float, np.integer, np.floating)):
        raise TypeError("a target PSNR must be a number, not %s" % type(db).__name__)
    db = float(db)
    if not math.isfinite(db):
        raise ValueError("a target PSNR of %r dB" % db)
    c, weight_sum, peak = int(c), int(weight_sum), float(peak)
    if c < 1 or weight_sum < 0:
        raise ValueError("target_sqerr: c >= 1 and weight_sum >= 0")
    if weight_sum == 0:
        raise ValueError("the weights add up to zero: no PSNR is defined")
    return float(c * weight_sum) * (peak * peak) / 10.0 ** (db / 10.0)


def allocate_target(R, D, target_sqerr, budget_bytes):
    """R, D: as for allocate; target_sqerr: the squared error of the whole picture to reach; budget_bytes: the cap.
    -> (bytes per tile, lam, dist, met).

    For a slope s, vertex_t(s) is tile t's last hull vertex over edges of slope >= s, dist(s) = total_distortion of the D_t
    there (integer D converted with one rounding, _f64) and cost(s) the bytes of those edges.  mu is the largest value of
    {inf} and the edge slopes with dist(mu) <= target_sqerr; if there is none -- the target is unreachable -- mu is the
    smallest edge slope (inf without edges).  dist does not rise as s falls (total_distortion is monotone), so the values with
    dist <= target are the slopes from some slope down, and mu is found by bisection of the descending list.
      cost(mu) <= budget_bytes: every tile goes to vertex_t(mu) -- edges of equal slope are all taken and none partially, since
        the error inside an edge was never measured.  lam = mu, dist = dist(mu), met = the target was reachable.
      otherwise: exactly allocate(R, D, budget_bytes); lam is its lambda*, dist = nan (a partial edge's error is unmeasured),
        met = False.
    A target that is NaN or negative is never met (the comparison is false); +inf is met with zero bytes."""
    budget, target = int(budget_bytes), float(target_sqerr)
    if budget < 0:
        raise ValueError("budget_bytes = %d is negative" % budget)
    hulls = []  # per tile: its edges' slopes (strictly decreasing), its vertices' lengths and distortions
    for t in range(len(R)):
        Dt = _f64(D[t])
        h = lower_hull(R[t], Dt)
        hulls.append(([slope(R[t], Dt, a, b) for a, b in zip(h, h[1:])], [int(R[t][k]) for k in h], [Dt[k] for k in h]))

    def at(s):
        ends = [sum(1 for x in sl if x >= s) for sl, _, _ in hulls]
        return [vR[e] for e, (_, vR, _) in zip(ends, hulls)], total_distortion([vD[e] for e, (_, _, vD) in zip(ends, hulls)])

    cand = sorted({math.inf}.union(*[set(sl) for sl, _, _ in hulls]), reverse=True)
    lo, hi = 0, len(cand)  # the first candidate, descending, with dist <= target; len(cand): none
    while lo < hi:
        m = (lo + hi) // 2
        if at(cand[m])[1] <= target:
            hi = m
        else:
            lo = m + 1
    mu = cand[min(lo, len(cand) - 1)]  # unreachable: the smallest slope (cand is [inf] without edges)
    out, dist = at(mu)
    if sum(out) <= budget:
        return out, mu, dist, dist <= target
    out, lam = allocate(R, D, budget)
    return out, lam, math.nan, False


def allocate_target_layers(R, D, targets, budget_bytes):
    """targets: Q non-increasing squared errors.  -> (cum, lams, dists, mets): row q is allocate_target(R, D, targets[q],
    budget_bytes).

    The rows NEST, cum[q][t] <= cum[q + 1][t], and lams does not rise.  Why: dist(s) does not rise as s falls, so mu_q falls
    as the target falls, and a tile's hull slopes strictly decrease: the vertex it reaches only advances.  cost(s) grows as s
    falls, so once cost(mu_q) exceeds the budget it does so for every later row, and those rows are all allocate(R, D, budget).
    lambda*(budget) is the smallest slope whose cost fits, so lambda* <= mu_q for every row that fit: the budget row takes
    every edge those rows took, whole, and dominates them all.  An unreachable target gives mu = the smallest slope, below
    every other row's."""
    targets = [float(v) for v in targets]
    if any(b > a for a, b in zip(targets, targets[1:])):
        raise ValueError("the targets must not rise: %r" % (targets,))
    rows = [allocate_target(R, D, v, budget_bytes) for v in targets]
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]


def target_psnr_arg(target_psnr, N):
    """the target_psnr= of a one-rate encode of N pictures -> N floats: a number for all pictures or one number per picture"""
    if isinstance(target_psnr, (str, bytes)):
        raise TypeError("target_psnr must be a number or a sequence of numbers, not %s" % type(target_psnr).__name__)
    if isinstance(target_psnr, (list, tuple, np.ndarray)) and np.ndim(target_psnr) > 0:
        seq = list(target_psnr)
        if len(seq) != N:
            raise ValueError("target_psnr holds %d values for %d picture(s)" % (len(seq), N))
    else:
        seq = [target_psnr] * N
    for db in seq:
        target_sqerr(db, 1.0, 1, 1)  # (its refusals)
    return [float(db) for db in seq]


def layer_targets_arg(target_psnr, layers=None):
    """the target_psnr= of a layered encode -> Q floats: a sequence of 1 .. MAX_LAYERS strictly increasing finite dB values;
    layers is then None or Q"""
    if isinstance(target_psnr, (str, bytes)) or np.ndim(target_psnr) != 1:
        raise TypeError("the layers' target_psnr must be a sequence of numbers")
    seq = list(target_psnr)
    for db in seq:
        target_sqerr(db, 1.0, 1, 1)
    out = [float(db) for db in seq]
    if not 1 <= len(out) <= MAX_LAYERS:
        raise ValueError("%d layers: 1 .. %d" % (len(out), MAX_LAYERS))
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("the layers' target PSNRs must strictly increase: %r" % (out,))
    if layers is not None and (isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or int(layers) != len(out)):
        raise ValueError("layers = %r with %d target PSNRs: None or their number" % (layers, len(out)))
    return out
