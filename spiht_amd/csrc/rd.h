// Rate-distortion reductions (rd.hip): how the launchers cut the work into workgroups, shared with api.cpp, which sizes the
// context's buffer of per-workgroup partial sums from it.
#pragma once
#include "common.h"

#define RD_THREADS 256
#define RD_TILE_I32 8192    // k_sqerr_i32: coefficients per workgroup (32 KiB of each operand: 8 16-byte loads per lane)
#define RD_TILE_ROWS 16     // k_sse_f64: picture rows per workgroup, 4 per wavefront
#define RD_TILE_PX 16384    // k_sse_px: samples per workgroup (4 / 8 16-byte loads per lane of 8- / 16-bit samples)

static inline uint32_t rd_tiles(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// the launchers of rd.hip (called from api.cpp)
extern "C" {
int spiht_launch_sqerr_i32(const int32_t *d_x, const int32_t *d_y, int K, int c, uint32_t hw, uint64_t *part, uint64_t *d_out,
                           hipStream_t st);
int spiht_launch_sse_f64(const double *d_pic, const double *d_dec, int K, int c, int H, int W, int rec_h, int rec_w, double *part,
                         double *d_out, hipStream_t st);
int spiht_launch_sse_px(const PxView *px, const void *d_dec, int K, uint64_t *part, uint64_t *d_out, hipStream_t st);
}
