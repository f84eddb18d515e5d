// Rate allocation across tiles (alloc.hip, roi.hip): how the launchers cut the work, shared with api.cpp, which checks the
// arguments and sizes the context's buffers from it.  The device code of the error sums is sse_tiles.h.
#pragma once
#include "common.h"

#define AL_THREADS 256
#define AL_TILE_ROWS 16  // k_sse_tiles_*: tile rows per workgroup, 4 per wavefront

// the per-tile error sums: original tiles [NT, c, th, tw] against decodes [G, NT, c, rh, rw], each over the tile's valid extent
struct TileSseArgs {
    const void *tiles, *dec;
    void *part;  // [G * NT, c, chunks] per-workgroup partial sums (8 bytes each)
    void *out;   // [G * NT]
    int32_t c, H, W, th, tw, rh, rw, gx;
    uint32_t T, NT, chunks;
};

// the weighted forms (roi.hip): the same sums, every term times the weight of its pixel position
struct TileSseWArgs {
    TileSseArgs a;
    const uint8_t *w;   // [N or 1][H][W], in picture coordinates
    uint64_t w_stride;  // bytes from one picture's map to the next; 0: one map for all pictures
};

static inline uint32_t al_chunks(int64_t th) { return (uint32_t)((th + AL_TILE_ROWS - 1) / AL_TILE_ROWS); }

// the valid extent of tile t of a picture batch: rows and columns that are picture samples, not replicated padding
__device__ __forceinline__ void valid_extent(const TileSseArgs &a, uint32_t t, int &vh, int &vw) {
    const uint32_t tl = t % a.T;
    const int i = (int)(tl / (uint32_t)a.gx), j = (int)(tl - (uint32_t)i * (uint32_t)a.gx);
    vh = min(a.th, a.H - i * a.th);
    vw = min(a.tw, a.W - j * a.tw);
}

// spiht_tile_allocate's scratch, per tile: K + 1 hull vertices (float64 distortion, uint32 length), K edge slopes, a count
static inline size_t al_scratch_bytes(uint64_t NT, uint64_t K) { return (size_t)(NT * ((K + 1) * 12 + K * 8 + 4)); }

// the launchers of alloc.hip and roi.hip (called from api.cpp)
extern "C" {
int spiht_launch_tile_prefix_slots(const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_nbits, int64_t NT, int K, int k0,
                                   int G, uint8_t *d_out, uint64_t out_stride, uint64_t *d_nbytes, const uint8_t *d_max_n,
                                   uint8_t *d_max_n_out, hipStream_t st);
int spiht_launch_sse_tiles(const TileSseArgs *a, int es, int64_t G, hipStream_t st);
int spiht_launch_sse_tiles_w(const TileSseWArgs *q, int es, int64_t G, hipStream_t st);
int spiht_launch_sse_tiles_flt(const TileSseArgs *a, int kind, int64_t G, hipStream_t st);
int spiht_launch_sse_tiles_w_flt(const TileSseWArgs *q, int kind, int64_t G, hipStream_t st);
int spiht_launch_tile_allocate(const uint64_t *d_nbits, const void *d_D, int kind, int K, int64_t N, int64_t T, uint64_t budget,
                               const double *d_target, void *scratch, uint64_t *d_nbits_out, double *d_lambda, double *d_dist,
                               uint32_t *d_met, hipStream_t st);
}
