// Tiled pictures (tiles.hip): the arguments of the four copy kernels, shared with api.cpp, which checks them.
#pragma once
#include "common.h"

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
