// Picture sets (tileset.hip): pictures of different sizes as ONE dense tile batch, and one dense batch of decoded tiles into many
// windows of many pictures.  The batched forms of k_tile_cut / k_tile_paste (tiles.hip): what those take as launch arguments
// -- one picture, one window -- a workgroup here reads from two device tables, a row per picture (item) and the picture (item)
// of every tile.  api_tiles.cpp builds the tables from the caller's host rows, checks them and copies them to the device.
#pragma once
#include "tiles.h"

// one picture of a cut: its view by byte strides, its size, its grid's width and its first row in the tile batch
struct TileSetPic {
    const uint8_t *in;
    int64_t sc, sh, sw;      // bytes
    int32_t H, W, gx;
    uint32_t tile0;
};
// one item of a paste: the window (y0, x0, wh, ww) of its picture, written at `out` by byte strides from the tiles
// [s0, s0 + ni * nj) of the batch, the sub-grid [i0, i0 + ni) x [j0, j0 + nj) in row-major order
struct TileSetItem {
    uint8_t *out;
    int64_t sc, sh, sw;      // bytes
    int32_t i0, j0, nj;
    uint32_t s0;
    int32_t y0, x0, wh, ww;
};

struct TileSetCutArgs {
    const TileSetPic *pics;        // device, [P]
    const uint32_t *pic_of_tile;   // device, [NT]
    uint8_t *out;                  // the dense tile batch [NT, c, th, tw]
    int32_t c, th, tw;
    int32_t rows;                  // tile rows per workgroup (a multiple of the workgroup's y extent)
};
struct TileSetPasteArgs {
    const TileSetItem *items;      // device, [B]
    const uint32_t *item_of_tile;  // device, [S]
    const uint8_t *tiles;          // the dense tile batch [S, c, rh, rw]
    int32_t c, rh, rw, th, tw;
    int32_t rows;                  // picture rows of a tile per workgroup
};

// one set of tables on its way to the device: page-locked host memory that a call fills and the copy reads, and the event behind
// that copy.  A call takes a stage whose copy is done (or makes one): two calls queued back to back never share one.
struct TableStage {
    void *host = nullptr;
    size_t cap = 0;
    hipEvent_t copied = nullptr;
};
#define TS_MAX_STAGES 8  // stages a context keeps; with all of them in flight a call waits for the oldest copy

extern "C" {
int spiht_launch_tile_cut_set(const TileSetCutArgs *a, int es, int64_t NT, hipStream_t st);
// n: the longest row piece a tile gives any item, rows: the most rows; strided: an item's samples are not contiguous
int spiht_launch_tile_paste_set(const TileSetPasteArgs *a, int es, int64_t S, int64_t n, int64_t rows, int strided, hipStream_t st);
}
