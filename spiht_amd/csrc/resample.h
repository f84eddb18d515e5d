// Resized crops (resample.hip): one dense batch of decoded float64 tiles -> B boxes of B pictures, each resampled to ONE size
// [c, oh, ow] by the antialiased triangle filter, mirrored, normalised and rounded once to the output kind.  The rule is
// spiht_amd/resample.py; the weights are the host's (axis_table), the kernel multiplies and adds in the rule's order.
// api_tiles.cpp checks the caller's rows and tables and copies them to the device (tileset.h: TableStage).
#pragma once
#include "tiles.h"

#define RS_MAX_TAPS 33   // taps per output sample the kernel is built for: a box side of at most 16 output sides
#define RS_ROWS 8        // output rows of a workgroup
#define RS_COLS 32       // output columns of a workgroup
// source rows a workgroup filters into LDS: the taps of RS_ROWS consecutive output rows span at most
// scale * (RS_ROWS - 1) + 2 * support + 1 source rows, scale = support <= 16; api_tiles.cpp refuses a row table that spans more
#define RS_SPAN (16 * (RS_ROWS - 1) + RS_MAX_TAPS)

// one table of an axis with n outputs and K taps, at a multiple of 8 bytes in the table blob:
//   int32 start[n], int32 count[n], float64 weights[n][K]     (start: from the box's first sample)
static inline size_t rs_table_bytes(int64_t n, int64_t K) { return (size_t)n * 8 + (size_t)n * (size_t)K * 8; }

// one item: the box (y0, x0, h, w) of its picture, made from the tiles [s0, s0 + ni * nj) of the batch -- the sub-grid
// [i0, i0 + ni) x [j0, j0 + nj) in row-major order --, written at `out` as [c, oh, ow] by byte strides
struct ResampleItem {
    uint8_t *out;
    int64_t sc, sh, sw;      // bytes
    int32_t i0, j0, nj;
    uint32_t s0;
    int32_t y0, x0, h, w;
    uint32_t ctab, rtab;     // bytes from the blob's start to the column table and to the row table
    int32_t ck, rk;          // their K
};

struct ResampleArgs {
    const ResampleItem *items;   // device, [B]
    const uint8_t *tables;       // device: the blob the items' offsets count from
    const double *mean, *std;    // device, [c] each, or both NULL
    const double *tiles;         // the dense tile batch [S, c, rh, rw]
    int32_t c, rh, rw, th, tw, oh, ow;
    int32_t ncol;                // column chunks of a row chunk: blockIdx.x = row chunk * ncol + column chunk
};

extern "C" {
// es / kind: bytes per output sample and its float kind (floatpx.h; 0: float64 for es = 8, the 8- / 16-bit conversion for 1 / 2)
int spiht_launch_tile_resample_set(const ResampleArgs *a, int es, int kind, int64_t B, hipStream_t st);
}
