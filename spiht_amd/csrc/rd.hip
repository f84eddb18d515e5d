// Distortion of K decoded versions of one picture against the original, reduced in HBM to K small rows (gfx950):
//   k_sqerr_i32   coefficient domain: E[k] = sum (X - Y[k])^2 over int32 arrays, exact in 128 bits
//   k_sse_f64     pixel domain, float64: S[k, ch] = sum over the H x W window of (P - D[k])^2, in a fixed order of additions
//   k_sse_px      pixel domain, 8- / 16-bit: the same sum, exact in 64 bits
// All three stream their input once: grid (tiles, c, K), 256 threads, per-lane partial -> wavefront (__shfl_down) ->
// workgroup (four words of LDS) -> one partial per workgroup in device memory; a second small launch adds the partials.
// No atomics: the integer sums do not need them and the float64 sum must not depend on arrival order.
// Compiled with -ffp-contract=off: a float64 term is (P - D) * (P - D) rounded, then added -- never a fused multiply-add.
#include "rd.h"
#include "sse_tiles.h"

struct U128 {
    uint64_t lo, hi;
};
__device__ __forceinline__ void add128(U128 &a, uint64_t lo, uint64_t hi) {
    a.lo += lo;
    a.hi += hi + (a.lo < lo ? 1 : 0);
}
// (x - y)^2 of two int32: |x - y| < 2^32, so the square fits 64 bits unsigned (not signed)
__device__ __forceinline__ void sq_i32(U128 &a, int32_t x, int32_t y) {
    const int64_t d = (int64_t)x - (int64_t)y;
    const uint64_t u = (uint64_t)(d < 0 ? -d : d);
    add128(a, u * u, 0);
}

// a 16-byte load from an address that is only 4-byte aligned (X, when the planes of X and Y are not congruent modulo 16)
struct __attribute__((packed, aligned(4))) I32x4u {
    int32_t v[4];
};

// X [c, hw], Y [K, c, hw] -> part [K, c, tiles][2].  A workgroup takes RD_TILE_I32 consecutive cells of one plane: the cells
// before the first 16-byte boundary of Y one per lane, then 16-byte loads (aligned in Y, the operand that comes from HBM;
// X is read K times and stays in the caches), then the cells after the last whole vector one per lane.
__global__ __launch_bounds__(RD_THREADS) void k_sqerr_i32(const int32_t *__restrict__ X, const int32_t *__restrict__ Y,
                                                          uint32_t hw, uint32_t c, uint32_t tiles, uint64_t *__restrict__ part) {
    const uint32_t tile = blockIdx.x, ch = blockIdx.y, k = blockIdx.z, tid = threadIdx.x;
    const int32_t *x = X + (size_t)ch * hw;
    const int32_t *y = Y + ((size_t)k * c + ch) * hw;
    const uint32_t s = tile * RD_TILE_I32, e = min(s + (uint32_t)RD_TILE_I32, hw);
    const uint32_t hd = min(e - s, (uint32_t)((16 - ((uintptr_t)(y + s) & 15)) & 15) / 4);
    const uint32_t v0 = s + hd, nvec = (e - v0) / 4, t0 = v0 + 4 * nvec;
    U128 a = {0, 0};
    if (tid < hd) sq_i32(a, x[s + tid], y[s + tid]);
    if (tid < e - t0) sq_i32(a, x[t0 + tid], y[t0 + tid]);
    constexpr int VPT = RD_TILE_I32 / 4 / RD_THREADS;
    int4 yv[VPT];
    I32x4u xv[VPT];
#pragma unroll
    for (int j = 0; j < VPT; j++) {
        const uint32_t v = tid + j * RD_THREADS;
        yv[j] = make_int4(0, 0, 0, 0);
        xv[j] = I32x4u{{0, 0, 0, 0}};
        if (v < nvec) {
            yv[j] = *reinterpret_cast<const int4 *>(y + v0 + 4 * v);
            xv[j] = *reinterpret_cast<const I32x4u *>(x + v0 + 4 * v);
        }
    }
#pragma unroll
    for (int j = 0; j < VPT; j++) {
        sq_i32(a, xv[j].v[0], yv[j].x);
        sq_i32(a, xv[j].v[1], yv[j].y);
        sq_i32(a, xv[j].v[2], yv[j].z);
        sq_i32(a, xv[j].v[3], yv[j].w);
    }
    for (int off = 32; off; off >>= 1) {
        const uint64_t lo = __shfl_down(a.lo, off), hi = __shfl_down(a.hi, off);
        add128(a, lo, hi);
    }
    __shared__ uint64_t sh[RD_THREADS / 64][2];
    if ((tid & 63) == 0) {
        sh[tid >> 6][0] = a.lo;
        sh[tid >> 6][1] = a.hi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < RD_THREADS / 64; wv++) add128(a, sh[wv][0], sh[wv][1]);
        uint64_t *o = part + 2 * (((size_t)k * c + ch) * tiles + tile);
        o[0] = a.lo;
        o[1] = a.hi;
    }
}
// part [K, per][2] -> out [K][2]: one wavefront per k
__global__ __launch_bounds__(64) void k_sum_u128(const uint64_t *__restrict__ part, uint32_t per, uint64_t *__restrict__ out) {
    const uint64_t *p = part + 2 * (size_t)blockIdx.x * per;
    U128 a = {0, 0};
    for (uint32_t i = threadIdx.x; i < per; i += 64) add128(a, p[2 * i], p[2 * i + 1]);
    for (int off = 32; off; off >>= 1) {
        const uint64_t lo = __shfl_down(a.lo, off), hi = __shfl_down(a.hi, off);
        add128(a, lo, hi);
    }
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = a.lo;
        out[2 * blockIdx.x + 1] = a.hi;
    }
}
// part [n, per] -> out [n]: one wavefront per sum (integers: any order)
__global__ __launch_bounds__(64) void k_sum_u64(const uint64_t *__restrict__ part, uint32_t per, uint64_t *__restrict__ out) {
    const uint64_t *p = part + (size_t)blockIdx.x * per;
    uint64_t a = 0;
    for (uint32_t i = threadIdx.x; i < per; i += 64) a += p[i];
    a = wave_sum(a);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// P [c, H, W], D [K, c, rec_h, rec_w] (the window is D[..., :H, :W]) -> part [K, c, tiles].  The partition is a function of
// (H, W) alone and the order of additions is the per-tile sums' (sse_tiles.h: a workgroup takes RD_TILE_ROWS rows), so
// S[k, ch] is the same bits whatever K is and wherever picture k lies.
static_assert(RD_TILE_ROWS == AL_TILE_ROWS && RD_THREADS == AL_THREADS, "sse_lane_sum cuts the rows by alloc.h's constants");
__global__ __launch_bounds__(RD_THREADS) void k_sse_f64(const double *__restrict__ P, const double *__restrict__ D, int32_t H,
                                                        int32_t W, int32_t rec_h, int32_t rec_w, uint32_t c, uint32_t tiles,
                                                        double *__restrict__ part) {
    const uint32_t tile = blockIdx.x, ch = blockIdx.y, k = blockIdx.z, tid = threadIdx.x;
    const int wv = tid >> 6, lane = tid & 63;
    const double *p = P + (size_t)ch * H * W;
    const double *d = D + ((size_t)k * c + ch) * rec_h * rec_w;
    const double mine = sse_lane_sum<SSE_F64, double, false>(p, W, d, rec_w, nullptr, 0, tile, H, W, 0, wv, lane);
    const double acc = block_sum_ordered<double, RD_THREADS>(mine, tid, wv, lane);
    if (tid == 0) part[((size_t)k * c + ch) * tiles + tile] = acc;
}
// part [n, tiles] -> out [n]: one thread per sum, the partials in index order
__global__ __launch_bounds__(64) void k_sum_f64(const double *__restrict__ part, uint32_t n, uint32_t tiles, double *__restrict__ out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double *p = part + (size_t)i * tiles;
    double a = p[0];
    for (uint32_t t = 1; t < tiles; t++) a += p[t];
    out[i] = a;
}

// P: the original through its view (byte strides, as every *_u8 / *_u16 call reads it), D [K, c, H, W] dense -> part
// [K, c, tiles].  A workgroup takes RD_TILE_PX consecutive samples of one decoded plane, cut as in k_sqerr_i32: up to the
// first 16-byte boundary of D one per lane, 16-byte loads of D, the rest one per lane.  A term is at most 65535^2 < 2^32.
template <typename T>
__device__ __forceinline__ uint64_t sq_px(const uint8_t *pb, const PxView &px, uint32_t y, uint32_t x, uint32_t dv) {
    const int32_t t = (int32_t)*reinterpret_cast<const T *>(pb + (int64_t)y * px.sh + (int64_t)x * px.sw) - (int32_t)dv;
    const uint32_t u = (uint32_t)(t < 0 ? -t : t);
    return (uint64_t)(u * u);
}
template <typename T>
__global__ __launch_bounds__(RD_THREADS) void k_sse_px(const PxView px, const T *__restrict__ D, uint32_t tiles,
                                                       uint64_t *__restrict__ part) {
    const uint32_t tile = blockIdx.x, ch = blockIdx.y, k = blockIdx.z, tid = threadIdx.x;
    const uint32_t W = (uint32_t)px.w, hw = (uint32_t)px.h * W, c = (uint32_t)px.c;
    const uint8_t *pb = px.in + (int64_t)ch * px.sc;
    const T *d = D + ((size_t)k * c + ch) * hw;
    constexpr uint32_t EPV = 16 / sizeof(T), BITS = 8 * sizeof(T), MASK = (1u << BITS) - 1, PER_WORD = 4 / sizeof(T);
    const uint32_t s = tile * RD_TILE_PX, e = min(s + (uint32_t)RD_TILE_PX, hw);
    const uint32_t hd = min(e - s, (uint32_t)((16 - ((uintptr_t)(d + s) & 15)) & 15) / (uint32_t)sizeof(T));
    const uint32_t v0 = s + hd, nvec = (e - v0) / EPV, t0 = v0 + EPV * nvec;
    uint64_t a = 0;
    if (tid < hd) {
        const uint32_t i = s + tid;
        a += sq_px<T>(pb, px, i / W, i % W, d[i]);
    }
    if (tid < e - t0) {
        const uint32_t i = t0 + tid;
        a += sq_px<T>(pb, px, i / W, i % W, d[i]);
    }
    constexpr int VPT = RD_TILE_PX / EPV / RD_THREADS;
    uint4 q[VPT];
#pragma unroll
    for (int j = 0; j < VPT; j++) {
        const uint32_t v = tid + j * RD_THREADS;
        q[j] = make_uint4(0, 0, 0, 0);
        if (v < nvec) q[j] = *reinterpret_cast<const uint4 *>(d + v0 + EPV * v);
    }
#pragma unroll
    for (int j = 0; j < VPT; j++) {
        const uint32_t v = tid + j * RD_THREADS;
        if (v >= nvec) break;
        const uint32_t i0 = v0 + EPV * v;
        uint32_t y = i0 / W, x = i0 - y * W;
        const uint32_t wd[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (uint32_t i = 0; i < EPV; i++) {
            a += sq_px<T>(pb, px, y, x, (wd[i / PER_WORD] >> (BITS * (i % PER_WORD))) & MASK);
            if (++x == W) {
                x = 0;
                y++;
            }
        }
    }
    a = block_sum_ordered<uint64_t, RD_THREADS>(a, tid, tid >> 6, tid & 63);
    if (tid == 0) part[((size_t)k * c + ch) * tiles + tile] = a;
}

// ---- host launchers: `part` holds K * c * tiles partials (rd.h: rd_tiles) of 16, 8 and 8 bytes -------------------------

extern "C" int spiht_launch_sqerr_i32(const int32_t *d_x, const int32_t *d_y, int K, int c, uint32_t hw, uint64_t *part,
                                      uint64_t *d_out, hipStream_t st) {
    const uint32_t tiles = rd_tiles(hw, RD_TILE_I32);
    hipLaunchKernelGGL(k_sqerr_i32, dim3(tiles, c, K), dim3(RD_THREADS), 0, st, d_x, d_y, hw, (uint32_t)c, tiles, part);
    hipLaunchKernelGGL(k_sum_u128, dim3(K), dim3(64), 0, st, part, (uint32_t)c * tiles, d_out);
    return (int)hipGetLastError();
}
extern "C" int spiht_launch_sse_f64(const double *d_pic, const double *d_dec, int K, int c, int H, int W, int rec_h, int rec_w,
                                    double *part, double *d_out, hipStream_t st) {
    const uint32_t tiles = rd_tiles(H, RD_TILE_ROWS), n = (uint32_t)K * c;
    hipLaunchKernelGGL(k_sse_f64, dim3(tiles, c, K), dim3(RD_THREADS), 0, st, d_pic, d_dec, H, W, rec_h, rec_w, (uint32_t)c,
                       tiles, part);
    hipLaunchKernelGGL(k_sum_f64, dim3((n + 63) / 64), dim3(64), 0, st, part, n, tiles, d_out);
    return (int)hipGetLastError();
}
extern "C" int spiht_launch_sse_px(const PxView *px, const void *d_dec, int K, uint64_t *part, uint64_t *d_out, hipStream_t st) {
    const uint32_t tiles = rd_tiles((uint64_t)px->h * px->w, RD_TILE_PX);
    const dim3 grid(tiles, px->c, K);
    if (px->es == 2)
        hipLaunchKernelGGL(k_sse_px<uint16_t>, grid, dim3(RD_THREADS), 0, st, *px, (const uint16_t *)d_dec, tiles, part);
    else
        hipLaunchKernelGGL(k_sse_px<uint8_t>, grid, dim3(RD_THREADS), 0, st, *px, (const uint8_t *)d_dec, tiles, part);
    hipLaunchKernelGGL(k_sum_u64, dim3((uint32_t)K * px->c), dim3(64), 0, st, part, tiles, d_out);
    return (int)hipGetLastError();
}
