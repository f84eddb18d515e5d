// Tiled pictures (tiles.hip, overlap.hip): the arguments of the copy kernels and of the blend, shared with api.cpp, which checks
// them, and what the launchers of the kernels' files share (their device code: tiles_device.h).
#pragma once
#include "common.h"

#include <algorithm>
#include <type_traits>

#define TL_THREADS 256
#define TL_CHUNK 16384        // pack / unpack: bytes of one stream a workgroup moves (four 16-byte stores per lane)
#define TL_BLOCK_BYTES 16384  // cut / paste: about as many bytes of tile rows per workgroup
#define TL_MOSAIC_WGS 1024    // mosaic: workgroups a launch aims for before a workgroup takes TL_BLOCK_BYTES

// cut: a picture batch [N, c, H, W] by byte strides -> the dense tile batch [N * gy * gx, c, th, tw], edge-replicated
struct TileCutArgs {
    const uint8_t *in;
    int64_t sb, sc, sh, sw;  // bytes
    uint8_t *out;
    int32_t c, H, W, th, tw, gy, gx;
    int32_t rows;            // tile rows per workgroup (a multiple of the workgroup's y extent)
};

// paste: the dense tile batch [ni * nj, c, rh, rw] of the sub-grid [i0, i0 + ni) x [j0, j0 + nj) -> the window
// [c, wh, ww] at (y0, x0) of the picture, by byte strides
struct TilePasteArgs {
    const uint8_t *tiles;
    uint8_t *out;
    int64_t sc, sh, sw;      // bytes
    int32_t c, rh, rw, th, tw, i0, j0, nj, y0, x0, wh, ww;
    int32_t rows;            // picture rows of a tile per workgroup
};

// mosaic: paste with a source origin and tiles of any side >= 1 (reduced tiles: a rim of extension samples around th x tw).
// Tile (i, j) gives its samples [oy, oy + th) x [ox, ox + tw) of [rh, rw]; the picture, the tile and the window are the
// ones being assembled.  Workgroups own rows of the window, not tiles.
struct TileMosaicArgs {
    const uint8_t *tiles;
    uint8_t *out;
    int64_t sc, sh, sw;      // bytes
    int32_t c, rh, rw, oy, ox, th, tw, i0, j0, nj, y0, x0, wh, ww;
    int32_t rows;            // window rows per workgroup (a multiple of the workgroup's y extent)
};

// overlapping tiles (overlap.hip).  cut: TileCutArgs with a margin of m picture samples around every tile, clamped on all
// four sides -> the dense tile batch [N * gy * gx, c, th + 2m, tw + 2m]
struct TileCutOverlapArgs {
    TileCutArgs cut;         // rows: rows of the CODED tile per workgroup
    int32_t m;
};

// blend: the dense float64 tile batch [ni * nj, c, rh, rw] of the sub-grid, every tile with its margin of m (its core at
// (m, m)) -> the window [c, wh, ww] at (y0, x0) of the picture, cross-faded over the 2m samples around each seam; float64, or
// 8- / 16-bit samples by byte strides.  Workgroups own rows of the window.
struct TileBlendArgs {
    const double *tiles;
    uint8_t *out;
    int64_t sc, sh, sw;      // bytes
    int32_t c, rh, rw, th, tw, m, gy, gx, i0, j0, nj, y0, x0, wh, ww;
    int32_t rows;            // window rows per workgroup (a multiple of the workgroup's y extent)
};

// the unsigned integer of ES bytes: what a copy moves of an element
template <int ES> struct ElemOf;
template <> struct ElemOf<1> { typedef uint8_t type; };
template <> struct ElemOf<2> { typedef uint16_t type; };
template <> struct ElemOf<4> { typedef uint32_t type; };
template <> struct ElemOf<8> { typedef uint64_t type; };

// The workgroup's shape for rows of `units` pieces (16-byte vectors, or elements of a strided row) of row_bytes bytes, `rows`
// of them: bx lanes along the row (a power of two), 256 / bx rows at a time, about TL_BLOCK_BYTES per workgroup.
static inline void row_blocks(int64_t units, int64_t row_bytes, int64_t rows, dim3 *block, int *rows_per_wg, uint32_t *gz) {
    int bx = 1;
    while (bx < units && bx < TL_THREADS) bx *= 2;
    const int by = TL_THREADS / bx;
    int64_t per = (int64_t)by * std::max<int64_t>(1, TL_BLOCK_BYTES / std::max<int64_t>(1, row_bytes * by));
    if ((rows + per - 1) / per > 65535) per = ((rows + 65534) / 65535 + by - 1) / by * by;
    *block = dim3(bx, by);
    *rows_per_wg = (int)per;
    *gz = (uint32_t)std::max<int64_t>(1, (rows + per - 1) / per);
}

// ... for workgroups that own rows of a window [c, rows, n] of es-byte elements (mosaic, blend); dense: the elements of a row
// are contiguous.  A small (reduced) window: fewer rows per workgroup, down to one pass of the block, until there are
// workgroups for every CU a few times over.
static inline void window_blocks(bool dense, int64_t n, int es, int64_t rows, int c, dim3 *block, int *rows_per_wg, uint32_t *gz) {
    row_blocks(dense ? (n * es + 15) / 16 + 1 : n, n * es, rows, block, rows_per_wg, gz);
    const int by = (int)block->y;
    while ((int64_t)*gz * c < TL_MOSAIC_WGS && *rows_per_wg > by) {
        *rows_per_wg = std::max<int>(by, *rows_per_wg / 2 / by * by);
        *gz = (uint32_t)((rows + *rows_per_wg - 1) / *rows_per_wg);
    }
}

// pack / unpack and their kin: the grid's chunks of a slot (a chunk may start up to 15 bytes into it)
static inline uint32_t slot_chunks(uint64_t slot_stride) { return (uint32_t)((slot_stride + 15 + TL_CHUNK - 1) / TL_CHUNK); }

// The element-size dispatch of every copy launcher: f(std::integral_constant<int, ES>()) for es = 1, 2, 4; anything else is 8.
template <typename F>
static inline int dispatch_es(int es, F f) {
    switch (es) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
    }
}

// the launchers of tiles.hip, layers.hip and overlap.hip (called from api.cpp)
extern "C" {
int spiht_launch_tile_cut(const TileCutArgs *a, int es, int64_t NT, hipStream_t st);
int spiht_launch_tile_paste(const TilePasteArgs *a, int es, int64_t ntiles, hipStream_t st);
int spiht_launch_tile_mosaic(const TileMosaicArgs *a, int es, hipStream_t st);
int spiht_launch_tile_cut_overlap(const TileCutOverlapArgs *a, int es, int64_t NT, hipStream_t st);
int spiht_launch_tile_blend(const TileBlendArgs *a, int es, hipStream_t st);
int spiht_launch_tile_blend_flt(const TileBlendArgs *a, int kind, hipStream_t st);
int spiht_launch_tile_pack(const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_nbytes, int64_t T, uint64_t *d_off,
                           uint8_t *d_packed, uint64_t cap, uint32_t *d_lens, hipStream_t st);
int spiht_launch_tile_unpack(const uint8_t *d_packed, uint64_t packed_bytes, const uint32_t *d_lens, int64_t T, uint64_t *d_off,
                             uint8_t *d_slots, uint64_t slot_stride, uint64_t *d_nbytes, hipStream_t st);
int spiht_launch_layer_pack(const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_cum_bits, int64_t Q, int64_t N, int64_t T,
                            uint64_t *d_off, uint8_t *d_packed, uint64_t cap, uint32_t *d_cum, uint64_t *d_pic_bytes, hipStream_t st);
int spiht_launch_layer_unpack(const uint8_t *d_layers, uint64_t layers_bytes, const uint32_t *d_cum, int64_t T, int64_t upto,
                              const int32_t *d_sel, int64_t S, uint64_t *d_off, uint32_t *d_M, uint8_t *d_slots, uint64_t slot_stride,
                              uint64_t *d_nbytes, hipStream_t st);
}
