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
#include "sse_tiles.h"

// grid (G * NT, chunks, c): alloc.hip's kernels with q.w, one body (sse_tiles.h).  A map of ones gives their bits.
__global__ __launch_bounds__(AL_THREADS) void k_sse_tiles_w_f64(const TileSseWArgs q) {
    sse_tiles_body<SSE_F64, double, true>(q.a, &q, 0);
}
template <typename T>
__global__ __launch_bounds__(AL_THREADS) void k_sse_tiles_w_flt(const TileSseWArgs q, int kind) {
    sse_tiles_body<SSE_FLT, T, true>(q.a, &q, kind);
}

// The partition of k_sse_tiles_px.  A term is at most 255 * 65535^2 < 2^40, a tile has at most 2^24 of them: exact in any order.
// Written out, not a call of the body: on the body the 8-bit sum of one measured shape lay above the spread of this text's own
// runs (profiles/tile_kernels_fold.txt).
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
