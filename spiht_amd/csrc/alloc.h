// Rate allocation across tiles (alloc.hip): how the launchers cut the work, shared with api.cpp, which checks the arguments
// and sizes the context's buffers from it.
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

static inline uint32_t al_chunks(int64_t th) { return (uint32_t)((th + AL_TILE_ROWS - 1) / AL_TILE_ROWS); }

// spiht_tile_allocate's scratch, per tile: K + 1 hull vertices (float64 distortion, uint32 length), K edge slopes, a count
static inline size_t al_scratch_bytes(uint64_t NT, uint64_t K) { return (size_t)(NT * ((K + 1) * 12 + K * 8 + 4)); }
