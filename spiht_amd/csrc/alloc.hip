// Rate allocation across the tiles of a picture (gfx950): every tile is coded past its share, K prefixes of every tile are
// decoded and measured, and every tile is cut where one more byte buys the same drop in distortion.
//   k_tile_prefix_slots  NT stream slots -> G * NT slots holding the prefixes of candidates k0 .. k0 + G - 1, zero behind
//   k_sse_tiles_f64      per-tile error sum over the tile's valid extent, float64, in a fixed order of additions
//   k_sse_tiles_flt      k_sse_tiles_f64 with original tiles of a float kind, widened on the load (float pixels in)
//   k_sse_tiles_px       the same for 8- / 16-bit samples, exact in 64 bits
//   k_tile_allocate      lower convex hulls, the common slope by bisection, the fill in tile order: one workgroup per picture
//   k_tile_allocate_target  the same hulls, the steepest common slope at which the picture's error is at or below a target
// The rule is spiht_amd/alloc.py; the allocation equals it bit for bit.  Compiled with -ffp-contract=off: a term is
// (p - d) * (p - d) rounded, then added; a slope is one rounded subtraction and one rounded division.  No atomics.
#include "sse_tiles.h"
#include "copy_bytes.h"

// ---- prefix slots ----------------------------------------------------------------------------------------------------------

// grid (G * NT, chunks of a slot).  Slot g * NT + t: the first R_t[k0 + g] = ceil(n_t (k0 + g) / K) bytes of slot t, n_t =
// ceil(nbits[t] / 8), then zeros up to out_stride.
__global__ __launch_bounds__(TL_THREADS) void k_tile_prefix_slots(const uint8_t *__restrict__ slots, uint64_t slot_stride,
                                                                  const uint64_t *__restrict__ nbits, uint32_t NT, uint32_t K,
                                                                  uint32_t k0, uint8_t *__restrict__ out, uint64_t out_stride,
                                                                  uint64_t *__restrict__ nbytes, const uint8_t *__restrict__ max_n,
                                                                  uint8_t *__restrict__ max_n_out) {
    const uint32_t s = blockIdx.x, g = s / NT, t = s - g * NT;
    const uint64_t n = min((nbits[t] + 7) >> 3, slot_stride);
    const uint64_t len = min((n * (k0 + g) + K - 1) / K, out_stride);
    const uint8_t *src = slots + (size_t)t * slot_stride;
    copy_bytes(out + (size_t)s * out_stride, src, out_stride, len, src, src + slot_stride, blockIdx.y);
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        nbytes[s] = len;
        if (max_n_out) max_n_out[s] = max_n[t];
    }
}

// ---- per-tile error sums -----------------------------------------------------------------------------------------------------

// grid (G * NT, chunks, c), one body (sse_tiles.h, where the partition and the order of additions are stated).  _flt: the
// ORIGINAL tiles are bit patterns of a float kind, each widened exactly on the load, so the sums are k_sse_tiles_f64's bits on
// the widened tiles.  _px: a term is at most 65535^2 < 2^32; any order is exact.
__global__ __launch_bounds__(AL_THREADS) void k_sse_tiles_f64(const TileSseArgs a) {
    sse_tiles_body<SSE_F64, double, false>(a, nullptr, 0);
}
template <typename T>
__global__ __launch_bounds__(AL_THREADS) void k_sse_tiles_flt(const TileSseArgs a, int kind) {
    sse_tiles_body<SSE_FLT, T, false>(a, nullptr, kind);
}
template <typename T>
__global__ __launch_bounds__(AL_THREADS) void k_sse_tiles_px(const TileSseArgs a) { sse_tiles_body<SSE_PX, T, false>(a, nullptr, 0); }

// part [G * NT, c, chunks] -> out [G * NT]: one thread per sum; the channels in order, of each the chunks that hold valid rows
// in order (the others were not written)
template <typename S>
__global__ __launch_bounds__(64) void k_sum_tiles(const TileSseArgs a, uint32_t n) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    int vh, vw;
    valid_extent(a, s % a.NT, vh, vw);
    const uint32_t used = (uint32_t)(vh + AL_TILE_ROWS - 1) / AL_TILE_ROWS;
    const S *p = (const S *)a.part + (size_t)s * a.c * a.chunks;
    S acc = p[0];
    for (uint32_t ch = 0; ch < (uint32_t)a.c; ch++)
        for (uint32_t k = ch ? 0 : 1; k < used; k++) acc += p[(size_t)ch * a.chunks + k];
    ((S *)a.out)[s] = acc;
}

// ---- the allocation ------------------------------------------------------------------------------------------------------------

enum { RED_SUM, RED_MIN, RED_MAX };
template <int OP> __device__ __forceinline__ uint64_t red_op(uint64_t x, uint64_t y) {
    return OP == RED_SUM ? x + y : OP == RED_MIN ? min(x, y) : max(x, y);
}
// every thread gets the workgroup's result; sh: AL_THREADS / 64 words no reduction still in flight uses
template <int OP> __device__ __forceinline__ uint64_t block_reduce(uint64_t v, uint64_t *sh) {
    for (int off = 32; off; off >>= 1) v = red_op<OP>(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = sh[0];
    for (int i = 1; i < AL_THREADS / 64; i++) r = red_op<OP>(r, sh[i]);
    return r;
}

// the hull of one tile in device memory, entry j of tile t at [j * NT + t]
struct Hulls {
    double *vD;     // [K + 1] the vertices' distortions
    double *eS;     // [K] the slope of the edge from vertex j to vertex j + 1: positive and strictly decreasing in j
    uint32_t *vR;   // [K + 1] the vertices' byte lengths
    uint32_t *cnt;  // vertices
    uint64_t NT;
};
// the number of edges of tile t whose slope is at least the double of bit pattern x (positive doubles order as their bits)
__device__ __forceinline__ uint32_t edges_from(const Hulls &h, uint64_t t, uint32_t cnt, uint64_t x) {
    uint32_t lo = 0, hi = cnt - 1;
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if ((uint64_t)__double_as_longlong(h.eS[m * h.NT + t]) >= x) lo = m + 1;
        else hi = m;
    }
    return lo;
}

#define AL_INF_BITS 0x7FF0000000000000ull

// Both allocation kernels: one workgroup per picture; thread i owns the tiles i, i + 256, ... of it in every phase, so a hull is
// read by the thread that wrote it.  kind: D is float64 (0) or uint64 (1: converted with one rounding).

// the hulls (alloc.py: lower_hull), one lane per tile
__device__ __forceinline__ void build_hulls(const uint64_t *__restrict__ nbits, const void *__restrict__ D, int kind, uint32_t K,
                                            uint32_t T, const Hulls &h) {
    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * T, NT = h.NT;
    for (uint32_t tl = tid; tl < T; tl += AL_THREADS) {
        const uint64_t t = t0 + tl;
        const uint64_t n = min((nbits[t] + 7) >> 3, (uint64_t)0x1FFFFFFF);
        uint32_t cnt = 1, topR = 0;
        double topD = kind ? (double)((const uint64_t *)D)[t] : ((const double *)D)[t];
        h.vR[t] = 0;
        h.vD[t] = topD;
        for (uint32_t k = 1; k <= K; k++) {
            const uint32_t Rk = (uint32_t)((n * k + K - 1) / K);
            const double Dk = kind ? (double)((const uint64_t *)D)[k * NT + t] : ((const double *)D)[k * NT + t];
            if (Rk == topR || !(Dk < topD)) continue;
            double sl = (topD - Dk) / (double)(Rk - topR);
            while (cnt >= 2 && h.eS[(cnt - 2) * NT + t] <= sl) {
                cnt--;
                topR = h.vR[(cnt - 1) * NT + t];
                topD = h.vD[(cnt - 1) * NT + t];
                sl = (topD - Dk) / (double)(Rk - topR);
            }
            h.eS[(cnt - 1) * NT + t] = sl;
            h.vR[cnt * NT + t] = Rk;
            h.vD[cnt * NT + t] = Dk;
            cnt++;
            topR = Rk;
            topD = Dk;
        }
        h.cnt[t] = cnt;
    }
}

// the cut at a budget (alloc.py: allocate) from the hulls this workgroup built: the common slope by bisection, then the fill in
// tile order.  sh: no reduction of the caller is still in flight.
__device__ __forceinline__ void budget_cut(uint32_t T, uint64_t budget, const Hulls &h, uint64_t (*sh)[AL_THREADS / 64],
                                           uint64_t *__restrict__ nbits_out, double *__restrict__ lambda) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * T, NT = h.NT;
    // x0: the smallest bit pattern x with cost(x) <= budget, cost(x) = the bytes of all edges of slope >= x; cost(inf) = 0
    uint64_t lo = 0, hi = AL_INF_BITS, cost0 = 0;
    int par = 0;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        uint64_t mine = 0;
        for (uint32_t tl = tid; tl < T; tl += AL_THREADS) {
            const uint64_t t = t0 + tl;
            mine += h.vR[edges_from(h, t, h.cnt[t], mid) * NT + t];
        }
        const uint64_t cost = block_reduce<RED_SUM>(mine, sh[par]);
        par ^= 1;
        if (cost <= budget) hi = mid;
        else lo = mid + 1;
    }
    const uint64_t x0 = lo;
    // lambda*: the smallest slope >= x0; the next slope below it (as bits + 1; 0: there is none); what the edges from x0 cost
    uint64_t lmin = AL_INF_BITS, lnext = 0;
    for (uint32_t tl = tid; tl < T; tl += AL_THREADS) {
        const uint64_t t = t0 + tl;
        const uint32_t cnt = h.cnt[t], e = edges_from(h, t, cnt, x0);
        cost0 += h.vR[e * NT + t];
        if (e >= 1) lmin = min(lmin, (uint64_t)__double_as_longlong(h.eS[(e - 1) * NT + t]));
        if (e + 1 < cnt) lnext = max(lnext, (uint64_t)__double_as_longlong(h.eS[e * NT + t]) + 1);
    }
    __syncthreads();  // the last round's words have been read
    cost0 = block_reduce<RED_SUM>(cost0, sh[0]);
    lmin = block_reduce<RED_MIN>(lmin, sh[1]);
    __syncthreads();
    lnext = block_reduce<RED_MAX>(lnext, sh[0]);
    __syncthreads();
    if (tid == 0 && lambda) lambda[blockIdx.x] = __longlong_as_double((long long)lmin);

    // what is left goes to the edges of the next slope, min(delta R, rest) each in tile order: an exclusive scan, 256 tiles a round
    const uint64_t rest = budget - cost0;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < T; base += AL_THREADS) {
        const uint32_t tl = base + tid;
        const uint64_t t = t0 + tl;
        uint64_t want = 0, reached = 0;
        if (tl < T) {
            const uint32_t cnt = h.cnt[t], e = edges_from(h, t, cnt, x0);
            reached = h.vR[e * NT + t];
            if (e + 1 < cnt && (uint64_t)__double_as_longlong(h.eS[e * NT + t]) + 1 == lnext) want = h.vR[(e + 1) * NT + t] - reached;
        }
        uint64_t x = want;
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = __shfl_up(x, o);
            if ((int)lane >= o) x += y;
        }
        if (lane == 63) sh[0][wv] = x;
        __syncthreads();
        uint64_t pre = 0, total = 0;
        for (uint32_t k = 0; k < AL_THREADS / 64; k++) {
            if (k < wv) pre += sh[0][k];
            total += sh[0][k];
        }
        if (tl < T) {
            const uint64_t before = carry + pre + x - want;
            nbits_out[t] = 8 * (reached + min(want, rest > before ? rest - before : (uint64_t)0));
        }
        carry += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(AL_THREADS) void k_tile_allocate(const uint64_t *__restrict__ nbits, const void *__restrict__ D, int kind,
                                                              uint32_t K, uint32_t T, uint64_t budget, Hulls h,
                                                              uint64_t *__restrict__ nbits_out, double *__restrict__ lambda) {
    __shared__ uint64_t sh[2][AL_THREADS / 64];
    build_hulls(nbits, D, kind, K, T, h);
    budget_cut(T, budget, h, sh, nbits_out, lambda);
}

// the workgroup's float64 sum in the order of alloc.py: total_distortion.  v: the thread's own terms, added in ascending order
// from +0.0; then the butterfly of each wavefront (every lane ends with the same bits) and the four wavefronts in order.
__device__ __forceinline__ double block_sum_f64(double v, uint64_t *sh) {
    for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (uint64_t)__double_as_longlong(v);
    __syncthreads();
    double r = __longlong_as_double((long long)sh[0]);
    for (int i = 1; i < AL_THREADS / 64; i++) r = r + __longlong_as_double((long long)sh[i]);
    return r;
}

// The cut at a target squared error (alloc.py: allocate_target).  dist(x) = the total distortion of the vertices the tiles reach
// over edges of slope >= the double of bit pattern x; it does not fall as x grows.  mu, the largest slope (or inf) with
// dist(mu) <= target, the smallest slope if there is none: every tile goes to its vertex at mu if that fits the budget;
// otherwise the workgroup goes on into the cut at the budget.  One launch either way.
__global__ __launch_bounds__(AL_THREADS) void k_tile_allocate_target(const uint64_t *__restrict__ nbits, const void *__restrict__ D,
                                                                     int kind, uint32_t K, uint32_t T, uint64_t budget,
                                                                     const double *__restrict__ targets, Hulls h,
                                                                     uint64_t *__restrict__ nbits_out, double *__restrict__ lambda,
                                                                     double *__restrict__ dist_out, uint32_t *__restrict__ met_out) {
    __shared__ uint64_t sh[2][AL_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * T, NT = h.NT;
    build_hulls(nbits, D, kind, K, T, h);
    const double target = targets[blockIdx.x];

    // x1: the largest bit pattern x with dist(x) <= target; 0 if there is none (a NaN or negative target compares false)
    uint64_t lo = 0, hi = AL_INF_BITS;
    int par = 0;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        double mine = 0.0;
        for (uint32_t tl = tid; tl < T; tl += AL_THREADS) {
            const uint64_t t = t0 + tl;
            mine = mine + h.vD[edges_from(h, t, h.cnt[t], mid) * NT + t];
        }
        const double d = block_sum_f64(mine, sh[par]);
        par ^= 1;
        if (d <= target) lo = mid;
        else hi = mid - 1;
    }
    // mu: the smallest slope >= x1 -- x1 itself where the target is reachable (dist steps only at slopes), inf above every
    // slope, the smallest slope of all where it is not
    uint64_t mu = AL_INF_BITS;
    for (uint32_t tl = tid; tl < T; tl += AL_THREADS) {
        const uint64_t t = t0 + tl;
        const uint32_t e = edges_from(h, t, h.cnt[t], lo);
        if (e >= 1) mu = min(mu, (uint64_t)__double_as_longlong(h.eS[(e - 1) * NT + t]));
    }
    __syncthreads();  // the last round's words have been read
    mu = block_reduce<RED_MIN>(mu, sh[0]);
    double mine = 0.0;
    uint64_t cost = 0;
    for (uint32_t tl = tid; tl < T; tl += AL_THREADS) {
        const uint64_t t = t0 + tl;
        const uint32_t e = edges_from(h, t, h.cnt[t], mu);
        mine = mine + h.vD[e * NT + t];
        cost += h.vR[e * NT + t];
    }
    cost = block_reduce<RED_SUM>(cost, sh[1]);
    __syncthreads();
    const double dist = block_sum_f64(mine, sh[0]);
    __syncthreads();
    if (cost <= budget) {  // (the same for every thread)
        for (uint32_t tl = tid; tl < T; tl += AL_THREADS) {
            const uint64_t t = t0 + tl;
            nbits_out[t] = 8 * (uint64_t)h.vR[edges_from(h, t, h.cnt[t], mu) * NT + t];
        }
        if (tid == 0) {
            if (lambda) lambda[blockIdx.x] = __longlong_as_double((long long)mu);
            if (dist_out) dist_out[blockIdx.x] = dist;
            if (met_out) met_out[blockIdx.x] = dist <= target ? 1u : 0u;
        }
        return;
    }
    // the budget binds: the cut at the budget, whose partial edges have no measured error
    if (tid == 0) {
        if (dist_out) dist_out[blockIdx.x] = __longlong_as_double(0x7FF8000000000000ll);
        if (met_out) met_out[blockIdx.x] = 0u;
    }
    budget_cut(T, budget, h, sh, nbits_out, lambda);
}

// ---- host launchers ------------------------------------------------------------------------------------------------------------

extern "C" int spiht_launch_tile_prefix_slots(const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_nbits, int64_t NT, int K,
                                              int k0, int G, uint8_t *d_out, uint64_t out_stride, uint64_t *d_nbytes,
                                              const uint8_t *d_max_n, uint8_t *d_max_n_out, hipStream_t st) {
    hipLaunchKernelGGL(k_tile_prefix_slots, dim3((uint32_t)(G * NT), slot_chunks(out_stride)), dim3(TL_THREADS), 0, st, d_slots, slot_stride, d_nbits,
                       (uint32_t)NT, (uint32_t)K, (uint32_t)k0, d_out, out_stride, d_nbytes, d_max_n, d_max_n_out);
    return (int)hipGetLastError();
}
// es: 8 float64, 1 / 2 integer samples
extern "C" int spiht_launch_sse_tiles(const TileSseArgs *a, int es, int64_t G, hipStream_t st) {
    const uint32_t n = (uint32_t)(G * a->NT);
    const dim3 grid(n, a->chunks, a->c);
    if (es == 8) {
        hipLaunchKernelGGL(k_sse_tiles_f64, grid, dim3(AL_THREADS), 0, st, *a);
        hipLaunchKernelGGL(k_sum_tiles<double>, dim3((n + 63) / 64), dim3(64), 0, st, *a, n);
    } else {
        if (es == 2) hipLaunchKernelGGL(k_sse_tiles_px<uint16_t>, grid, dim3(AL_THREADS), 0, st, *a);
        else hipLaunchKernelGGL(k_sse_tiles_px<uint8_t>, grid, dim3(AL_THREADS), 0, st, *a);
        hipLaunchKernelGGL(k_sum_tiles<uint64_t>, dim3((n + 63) / 64), dim3(64), 0, st, *a, n);
    }
    return (int)hipGetLastError();
}
// float pixels in: originals of a float kind against float64 decodes, float64 sums
extern "C" int spiht_launch_sse_tiles_flt(const TileSseArgs *a, int kind, int64_t G, hipStream_t st) {
    const uint32_t n = (uint32_t)(G * a->NT);
    const dim3 grid(n, a->chunks, a->c);
    if (flt_itemsize(kind) == 4) hipLaunchKernelGGL(k_sse_tiles_flt<uint32_t>, grid, dim3(AL_THREADS), 0, st, *a, kind);
    else hipLaunchKernelGGL(k_sse_tiles_flt<uint16_t>, grid, dim3(AL_THREADS), 0, st, *a, kind);
    hipLaunchKernelGGL(k_sum_tiles<double>, dim3((n + 63) / 64), dim3(64), 0, st, *a, n);
    return (int)hipGetLastError();
}
// the second launch alone, for the weighted forms (roi.hip), whose partials it adds: n sums, float64 (es 8) or uint64
extern "C" int spiht_launch_sum_tiles(const TileSseArgs *a, int es, uint32_t n, hipStream_t st) {
    if (es == 8) hipLaunchKernelGGL(k_sum_tiles<double>, dim3((n + 63) / 64), dim3(64), 0, st, *a, n);
    else hipLaunchKernelGGL(k_sum_tiles<uint64_t>, dim3((n + 63) / 64), dim3(64), 0, st, *a, n);
    return (int)hipGetLastError();
}
// d_target NULL: the cut at the budget; else [N] squared errors: the cut at a target (d_dist, d_met: its further outputs)
extern "C" int spiht_launch_tile_allocate(const uint64_t *d_nbits, const void *d_D, int kind, int K, int64_t N, int64_t T,
                                          uint64_t budget, const double *d_target, void *scratch, uint64_t *d_nbits_out,
                                          double *d_lambda, double *d_dist, uint32_t *d_met, hipStream_t st) {
    const uint64_t NT = (uint64_t)N * T;
    Hulls h;
    h.NT = NT;
    h.vD = (double *)scratch;
    h.eS = h.vD + (size_t)(K + 1) * NT;
    h.vR = (uint32_t *)(h.eS + (size_t)K * NT);
    h.cnt = h.vR + (size_t)(K + 1) * NT;
    if (d_target)
        hipLaunchKernelGGL(k_tile_allocate_target, dim3((uint32_t)N), dim3(AL_THREADS), 0, st, d_nbits, d_D, kind, (uint32_t)K,
                           (uint32_t)T, budget, d_target, h, d_nbits_out, d_lambda, d_dist, d_met);
    else
        hipLaunchKernelGGL(k_tile_allocate, dim3((uint32_t)N), dim3(AL_THREADS), 0, st, d_nbits, d_D, kind, (uint32_t)K, (uint32_t)T,
                           budget, h, d_nbits_out, d_lambda);
    return (int)hipGetLastError();
}
