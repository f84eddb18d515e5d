// Region of interest (gfx950): the per-tile error sums of alloc.hip with every term weighted by a per-pixel map, so that the
// allocation of equal slope spends the budget where the caller says it matters.
//   k_sse_tiles_w_f64    sum of double(w) * ((p - d) * (p - d)) over the tile's valid extent, in the order of k_sse_tiles_f64
//   k_sse_tiles_w_flt    k_sse_tiles_w_f64 with original tiles of a float kind, widened on the load (float pixels in)
//   k_sse_tiles_w_px     sum of w * (p - d)^2 for 8- / 16-bit samples, exact in 64 bits
// The map is uint8 [N or 1][H][W] in PICTURE coordinates, one weight for all channels and candidates; a sample of tile (i, j)
// at (y, x) inside the valid extent reads byte (i th + y) W + j tw + x, so no byte outside the map is read.  It is read byte
// by byte: a row of the map starts at any address (W may be odd), and it is 1/8 .. 1/16 of the bytes a lane reads anyway.
// The partials go to the context's buffer and are added by alloc.hip's second launch.  Compiled with -ffp-contract=off: the
// subtraction, the square and the product with the weight are each rounded once.  No atomics.
#include "alloc.h"
#include "floatpx.h"

// the map's first byte for tile t: picture t / T (or the one map), row i th, column j tw
__device__ __forceinline__ const uint8_t *map_of(const TileSseWArgs &q, uint32_t t) {
    const uint32_t n = t / q.a.T, tl = t - n * q.a.T;
    const uint32_t i = tl / (uint32_t)q.a.gx, j = tl - i * (uint32_t)q.a.gx;
    return q.w + (size_t)n * q.w_stride + (size_t)i * q.a.th * q.a.W + (size_t)j * q.a.tw;
}

// grid (G * NT, chunks, c): the partition and the order of additions of k_sse_tiles_f64.  A map of ones gives its bits.
__global__ __launch_bounds__(AL_THREADS) void k_sse_tiles_w_f64(const TileSseWArgs q) {
    const TileSseArgs &a = q.a;
    const uint32_t s = blockIdx.x, chunk = blockIdx.y, ch = blockIdx.z, tid = threadIdx.x;
    const uint32_t t = s % a.NT;
    int vh, vw;
    valid_extent(a, t, vh, vw);
    if ((int)chunk * AL_TILE_ROWS >= vh) return;
    const int wv = tid >> 6, lane = tid & 63;
    const double *p = (const double *)a.tiles + ((size_t)t * a.c + ch) * (size_t)a.th * a.tw;
    const double *d = (const double *)a.dec + ((size_t)s * a.c + ch) * (size_t)a.rh * a.rw;
    const uint8_t *w = map_of(q, t);
    double acc = 0.0;
    for (int r = wv; r < AL_TILE_ROWS; r += AL_THREADS / 64) {
        const int y = (int)chunk * AL_TILE_ROWS + r;
        if (y >= vh) break;
        const double *pr = p + (size_t)y * a.tw, *dr = d + (size_t)y * a.rw;
        const uint8_t *wr = w + (size_t)y * a.W;
#pragma unroll 4
        for (int x = 2 * lane; x < vw; x += 128) {
            if (x + 1 < vw) {
                const F64x2 pv = *reinterpret_cast<const F64x2 *>(pr + x), dv = *reinterpret_cast<const F64x2 *>(dr + x);
                const double w0 = (double)wr[x], w1 = (double)wr[x + 1];
                const double t0 = pv.a - dv.a, t1 = pv.b - dv.b;
                acc += w0 * (t0 * t0);
                acc += w1 * (t1 * t1);
            } else {
                const double t0 = pr[x] - dr[x];
                acc += (double)wr[x] * (t0 * t0);
            }
        }
    }
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off);
    __shared__ double sh[AL_THREADS / 64];
    if (lane == 0) sh[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < AL_THREADS / 64; i++) acc += sh[i];
        ((double *)a.part)[((size_t)s * a.c + ch) * a.chunks + chunk] = acc;
    }
}

// Float pixels in: the weighted form of alloc.hip's k_sse_tiles_flt -- original tiles of float32 (T = uint32_t) or float16 /
// bfloat16 (T = uint16_t) bit patterns of kind `kind`, widened exactly on the load; the partition and the order of additions
// of k_sse_tiles_w_f64, so its bits on the widened tiles.  A map of ones gives the bits of k_sse_tiles_flt.
template <typename T>
__global__ __launch_bounds__(AL_THREADS) void k_sse_tiles_w_flt(const TileSseWArgs q, int kind) {
    const TileSseArgs &a = q.a;
    const uint32_t s = blockIdx.x, chunk = blockIdx.y, ch = blockIdx.z, tid = threadIdx.x;
    const uint32_t t = s % a.NT;
    int vh, vw;
    valid_extent(a, t, vh, vw);
    if ((int)chunk * AL_TILE_ROWS >= vh) return;
    const int wv = tid >> 6, lane = tid & 63;
    const T *p = (const T *)a.tiles + ((size_t)t * a.c + ch) * (size_t)a.th * a.tw;
    const double *d = (const double *)a.dec + ((size_t)s * a.c + ch) * (size_t)a.rh * a.rw;
    const uint8_t *w = map_of(q, t);
    double acc = 0.0;
    for (int r = wv; r < AL_TILE_ROWS; r += AL_THREADS / 64) {
        const int y = (int)chunk * AL_TILE_ROWS + r;
        if (y >= vh) break;
        const T *pr = p + (size_t)y * a.tw;
        const double *dr = d + (size_t)y * a.rw;
        const uint8_t *wr = w + (size_t)y * a.W;
#pragma unroll 4
        for (int x = 2 * lane; x < vw; x += 128) {
            if (x + 1 < vw) {
                const uint32_t r0 = pr[x], r1 = pr[x + 1];
                const F64x2 dv = *reinterpret_cast<const F64x2 *>(dr + x);
                const double w0 = (double)wr[x], w1 = (double)wr[x + 1];
                const double t0 = flt_load_value(r0, kind) - dv.a, t1 = flt_load_value(r1, kind) - dv.b;
                acc += w0 * (t0 * t0);
                acc += w1 * (t1 * t1);
            } else {
                const double t0 = flt_load_value(pr[x], kind) - dr[x];
                acc += (double)wr[x] * (t0 * t0);
            }
        }
    }
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off);
    __shared__ double sh[AL_THREADS / 64];
    if (lane == 0) sh[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < AL_THREADS / 64; i++) acc += sh[i];
        ((double *)a.part)[((size_t)s * a.c + ch) * a.chunks + chunk] = acc;
    }
}

// the partition of k_sse_tiles_px.  A term is at most 255 * 65535^2 < 2^40, a tile has at most 2^24 of them: exact in any order.
template <typename T>
__global__ __launch_bounds__(AL_THREADS) void k_sse_tiles_w_px(const TileSseWArgs q) {
    const TileSseArgs &a = q.a;
    const uint32_t s = blockIdx.x, chunk = blockIdx.y, ch = blockIdx.z, tid = threadIdx.x;
    const uint32_t t = s % a.NT;
    int vh, vw;
    valid_extent(a, t, vh, vw);
    if ((int)chunk * AL_TILE_ROWS >= vh) return;
    const int wv = tid >> 6, lane = tid & 63;
    const T *p = (const T *)a.tiles + ((size_t)t * a.c + ch) * (size_t)a.th * a.tw;
    const T *d = (const T *)a.dec + ((size_t)s * a.c + ch) * (size_t)a.rh * a.rw;
    const uint8_t *w = map_of(q, t);
    uint64_t acc = 0;
    for (int r = wv; r < AL_TILE_ROWS; r += AL_THREADS / 64) {
        const int y = (int)chunk * AL_TILE_ROWS + r;
        if (y >= vh) break;
        const T *pr = p + (size_t)y * a.tw, *dr = d + (size_t)y * a.rw;
        const uint8_t *wr = w + (size_t)y * a.W;
#pragma unroll 4
        for (int x = lane; x < vw; x += 64) {
            const int32_t e = (int32_t)pr[x] - (int32_t)dr[x];
            const uint32_t u = (uint32_t)(e < 0 ? -e : e);
            acc += (uint64_t)(u * u) * wr[x];
        }
    }
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off);
    __shared__ uint64_t sh[AL_THREADS / 64];
    if (lane == 0) sh[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < AL_THREADS / 64; i++) acc += sh[i];
        ((uint64_t *)a.part)[((size_t)s * a.c + ch) * a.chunks + chunk] = acc;
    }
}

extern "C" int spiht_launch_sum_tiles(const TileSseArgs *a, int es, uint32_t n, hipStream_t st);

// es: 8 float64, 1 / 2 integer samples
extern "C" int spiht_launch_sse_tiles_w(const TileSseWArgs *q, int es, int64_t G, hipStream_t st) {
    const uint32_t n = (uint32_t)(G * q->a.NT);
    const dim3 grid(n, q->a.chunks, q->a.c);
    if (es == 8) hipLaunchKernelGGL(k_sse_tiles_w_f64, grid, dim3(AL_THREADS), 0, st, *q);
    else if (es == 2) hipLaunchKernelGGL(k_sse_tiles_w_px<uint16_t>, grid, dim3(AL_THREADS), 0, st, *q);
    else hipLaunchKernelGGL(k_sse_tiles_w_px<uint8_t>, grid, dim3(AL_THREADS), 0, st, *q);
    return spiht_launch_sum_tiles(&q->a, es, n, st);
}
// float pixels in: originals of a float kind against float64 decodes, float64 sums
extern "C" int spiht_launch_sse_tiles_w_flt(const TileSseWArgs *q, int kind, int64_t G, hipStream_t st) {
    const uint32_t n = (uint32_t)(G * q->a.NT);
    const dim3 grid(n, q->a.chunks, q->a.c);
    if (flt_itemsize(kind) == 4) hipLaunchKernelGGL(k_sse_tiles_w_flt<uint32_t>, grid, dim3(AL_THREADS), 0, st, *q, kind);
    else hipLaunchKernelGGL(k_sse_tiles_w_flt<uint16_t>, grid, dim3(AL_THREADS), 0, st, *q, kind);
    return spiht_launch_sum_tiles(&q->a, 8, n, st);
}
