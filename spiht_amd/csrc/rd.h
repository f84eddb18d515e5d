// Rate-distortion reductions (rd.hip): how the launchers cut the work into workgroups, shared with api.cpp, which sizes the
// context's buffer of per-workgroup partial sums from it.
#pragma once
#include "common.h"

#define RD_THREADS 256
#define RD_TILE_I32 8192    // k_sqerr_i32: coefficients per workgroup (32 KiB of each operand: 8 16-byte loads per lane)
#define RD_TILE_ROWS 16     // k_sse_f64: picture rows per workgroup, 4 per wavefront
#define RD_TILE_PX 16384    // k_sse_px: samples per workgroup (4 / 8 16-byte loads per lane of 8- / 16-bit samples)

static inline uint32_t rd_tiles(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }
