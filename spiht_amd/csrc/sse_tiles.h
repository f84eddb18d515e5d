// Error sums over rows of samples (device code): the one body of the per-tile kernels of alloc.hip and roi.hip, and what
// rd.hip's sums over a whole picture share with them.
//
// THE ORDER OF ADDITIONS of every float64 sum, which is documented, bit-exact behaviour (spiht_amd/alloc.py, rd.py).  The
// partition is a function of the extent (vh, vw) alone, never of where the samples lie or how many sums a launch takes: a
// workgroup of 256 takes a chunk of 16 rows, wavefront wv the rows wv, wv + 4, ... of them in ascending order, lane l of a row
// the columns 2 l, 2 l + 1, then 128 further on.  A lane adds its terms in that order to +0.0; the wavefront adds the lanes
// by the __shfl_down tree (offsets 32, 16, ..., 1); thread 0 adds the wavefronts 1, 2, 3 to its own in that order.  A term is
// (p - d) * (p - d), rounded, or double(w) * that, rounded again (the units are built with -ffp-contract=off).  The integer
// sums are exact in 64 bits in any order; they take the same rows, lane l the columns l, l + 64, ...
#pragma once
#include "alloc.h"
#include "floatpx.h"

#include <type_traits>

// two float64 at an address that is only 8-byte aligned: which samples a lane adds must not depend on where the samples lie
struct __attribute__((aligned(8))) F64x2 {
    double a, b;
};

template <typename S>
__device__ __forceinline__ S wave_sum(S v) {
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    return v;
}
// The workgroup's sum of one value per thread, in the order above; thread 0 alone gets it.  tid = threadIdx.x, wv = tid >> 6,
// lane = tid & 63 are the caller's, which has them for its own loop: one value each in the kernel, read once.
template <typename S, int THREADS>
__device__ __forceinline__ S block_sum_ordered(S v, uint32_t tid, int wv, int lane) {
    __shared__ S sh[THREADS / 64];
    v = wave_sum(v);
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    if (tid == 0)
        for (int i = 1; i < THREADS / 64; i++) v += sh[i];
    return v;
}

// the sample kind: the originals p are float64, bit patterns of a float kind widened exactly on the load (floatpx.h; T =
// uint32_t for float32, uint16_t for float16 / bfloat16, `kind` uniform over the launch), or 8- / 16-bit integers (T).  The
// decodes d are float64 for the first two and T for the third; the sum is float64 and uint64_t.
enum { SSE_F64, SSE_FLT, SSE_PX };
template <int KIND, typename T> using SseDec = std::conditional_t<KIND == SSE_PX, T, double>;
template <int KIND> using SseSum = std::conditional_t<KIND == SSE_PX, uint64_t, double>;

// One lane's sum over the rows [16 chunk, 16 chunk + 16) below vh and the columns below vw of p against d (rows of ps and ds
// elements); WEIGHTED: every term times the byte of w (rows of ws bytes) at its position.  A row of p of a float kind is only
// element-aligned (ps may be odd): its pair is two loads of one element; float64 rows keep the paired load.  (The weighted
// integer sum is roi.hip's own text.)
template <int KIND, typename T, bool WEIGHTED>
__device__ __forceinline__ SseSum<KIND> sse_lane_sum(const T *p, size_t ps, const SseDec<KIND, T> *d, size_t ds, const uint8_t *w,
                                                     size_t ws, int chunk, int vh, int vw, int kind, int wv, int lane) {
    static_assert(!(KIND == SSE_PX && WEIGHTED), "k_sse_tiles_w_px is written out in roi.hip");
    SseSum<KIND> acc = 0;
    for (int r = wv; r < AL_TILE_ROWS; r += AL_THREADS / 64) {
        const int y = chunk * AL_TILE_ROWS + r;
        if (y >= vh) break;
        const T *pr = p + (size_t)y * ps;
        const SseDec<KIND, T> *dr = d + (size_t)y * ds;
        const uint8_t *wr = WEIGHTED ? w + (size_t)y * ws : nullptr;
        if constexpr (KIND == SSE_PX) {
#pragma unroll 4
            for (int x = lane; x < vw; x += 64) {
                const int32_t e = (int32_t)pr[x] - (int32_t)dr[x];
                const uint32_t u = (uint32_t)(e < 0 ? -e : e);
                acc += (uint64_t)(u * u);
            }
        } else {
            // what a sample of p is loaded as (float64; the bits of a float kind), and its value
            typedef std::conditional_t<KIND == SSE_FLT, uint32_t, double> Raw;
            auto value = [&](Raw v) -> double {
                if constexpr (KIND == SSE_FLT) return flt_load_value(v, kind);
                else return v;
            };
            auto term = [&](double t, double wt) -> double {
                if constexpr (WEIGHTED) return wt * (t * t);
                else return t * t;
            };
#pragma unroll 4
            for (int x = 2 * lane; x < vw; x += 128) {
                if (x + 1 < vw) {
                    Raw r0, r1;
                    if constexpr (KIND == SSE_F64) {
                        const F64x2 pv = *reinterpret_cast<const F64x2 *>(pr + x);
                        r0 = pv.a, r1 = pv.b;
                    } else {
                        r0 = pr[x], r1 = pr[x + 1];
                    }
                    const F64x2 dv = *reinterpret_cast<const F64x2 *>(dr + x);
                    const double w0 = WEIGHTED ? (double)wr[x] : 1.0, w1 = WEIGHTED ? (double)wr[x + 1] : 1.0;
                    const double t0 = value(r0) - dv.a, t1 = value(r1) - dv.b;
                    acc += term(t0, w0);
                    acc += term(t1, w1);
                } else {
                    const double t0 = value(pr[x]) - dr[x];
                    acc += term(t0, WEIGHTED ? (double)wr[x] : 1.0);
                }
            }
        }
    }
    return acc;
}

// the map's first byte for tile t: picture t / T (or the one map), row i th, column j tw
__device__ __forceinline__ const uint8_t *map_of(const TileSseWArgs &q, uint32_t t) {
    const uint32_t n = t / q.a.T, tl = t - n * q.a.T;
    const uint32_t i = tl / (uint32_t)q.a.gx, j = tl - i * (uint32_t)q.a.gx;
    return q.w + (size_t)n * q.w_stride + (size_t)i * q.a.th * q.a.W + (size_t)j * q.a.tw;
}

// The body of k_sse_tiles_* (q NULL) and k_sse_tiles_w_f64 / _w_flt (a = q->a): grid (G * NT, chunks, c), AL_THREADS threads; the
// workgroup's sum over its chunk of the valid extent of tile s % NT, candidate s / NT, to part [G * NT, c, chunks].  A chunk
// without valid rows writes nothing.
template <int KIND, typename T, bool WEIGHTED>
__device__ __forceinline__ void sse_tiles_body(const TileSseArgs &a, const TileSseWArgs *q, int kind) {
    typedef SseSum<KIND> S;
    const uint32_t s = blockIdx.x, chunk = blockIdx.y, ch = blockIdx.z, tid = threadIdx.x;
    const int wv = tid >> 6, lane = tid & 63;
    const uint32_t t = s % a.NT;
    int vh, vw;
    valid_extent(a, t, vh, vw);
    if ((int)chunk * AL_TILE_ROWS >= vh) return;
    const T *p = (const T *)a.tiles + ((size_t)t * a.c + ch) * (size_t)a.th * a.tw;
    const SseDec<KIND, T> *d = (const SseDec<KIND, T> *)a.dec + ((size_t)s * a.c + ch) * (size_t)a.rh * a.rw;
    const uint8_t *w = nullptr;
    if constexpr (WEIGHTED) w = map_of(*q, t);
    const S mine = sse_lane_sum<KIND, T, WEIGHTED>(p, a.tw, d, a.rw, w, a.W, chunk, vh, vw, kind, wv, lane);
    const S acc = block_sum_ordered<S, AL_THREADS>(mine, tid, wv, lane);
    if (tid == 0) ((S *)a.part)[((size_t)s * a.c + ch) * a.chunks + chunk] = acc;
}
