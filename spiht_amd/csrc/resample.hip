// Resized crops (gfx950): boxes of any size of B pictures, read straight out of the dense batch of their decoded float64 tiles
// and resampled to ONE size [c, oh, ow] by the antialiased triangle filter.  The rule is spiht_amd/resample.py.
//   k_tile_resample_set  dense float64 tile batch [S, c, rh, rw] -> B outputs [c, oh, ow] by byte strides; item b is the box
//                        (y0, x0, h, w) of its picture, made from the tiles [s0_b, s0_b + ni_b * nj_b) of the batch.  Columns
//                        first, then rows: acc = s[start] * w[0], then acc = acc + s[start + k] * w[k], every product and every
//                        sum rounded on its own (this file is built with -ffp-contract=off); then (v - mean) / std, IEEE's
//                        division; then ONE conversion at the store: float64, a float kind (floatpx.h) or 8 / 16 bits.
// The weights are the host's, read from the item's two tables: the kernel computes none, so they are the rule's in every bit.
// A workgroup is an item (z), a channel (y) and RS_ROWS x RS_COLS output samples (x).  It has no intermediate picture: it
// filters the source rows its output rows' taps span -- at most RS_SPAN -- along the columns into LDS, gathering each run of
// taps straight from the tiles (one division for the run's first tile, then a step from tile to tile), and combines them down
// the rows.  Source rows that two row chunks share are filtered by both.  The item's row and its tables are found by blockIdx
// alone, so those reads are scalar loads.
// LDS: a row is RS_COLS float64 = 256 bytes, all 64 banks once: the column pass stores and the row pass loads 32 consecutive
// float64 per lane group, without a conflict; the column weights lie tap-major for the same reason.
#include "resample.h"
#include "tiles_device.h"
#include "floatpx.h"

template <int ES, int FK>
__global__ __launch_bounds__(RS_ROWS *RS_COLS) void k_tile_resample_set(const ResampleArgs a) {
    typedef typename ElemOf<ES>::type T;
    __shared__ double s_rows[RS_SPAN][RS_COLS];     // the source rows of the chunk, filtered along the columns
    __shared__ double s_cw[RS_MAX_TAPS][RS_COLS];   // the column weights of the chunk's columns, tap-major
    __shared__ double s_rw[RS_ROWS][RS_MAX_TAPS];   // the row weights of the chunk's rows
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const uint32_t ch = blockIdx.y;
    const ResampleItem d = a.items[blockIdx.z];  // (uniform: scalar loads)
    const int rchunk = (int)(blockIdx.x / (uint32_t)a.ncol), cchunk = (int)(blockIdx.x - (uint32_t)rchunk * (uint32_t)a.ncol);
    const int r0 = rchunk * RS_ROWS, nr = min(RS_ROWS, a.oh - r0);
    const int c0 = cchunk * RS_COLS, nc = min(RS_COLS, a.ow - c0);
    const int32_t *cstart = reinterpret_cast<const int32_t *>(a.tables + d.ctab), *ccount = cstart + a.ow;
    const double *cwt = reinterpret_cast<const double *>(ccount + a.ow);
    const int32_t *rstart = reinterpret_cast<const int32_t *>(a.tables + d.rtab), *rcount = rstart + a.oh;
    const double *rwt = reinterpret_cast<const double *>(rcount + a.oh);

    // the source rows the chunk's taps span, [lo, hi) of the box (uniform)
    int lo = rstart[r0], hi = lo + rcount[r0];
    for (int r = 1; r < nr; r++) {
        const int s = rstart[r0 + r];
        lo = min(lo, s);
        hi = max(hi, s + rcount[r0 + r]);
    }

    // the weights into LDS: this lane's column, this lane's row
    const int x = c0 + tx;
    const bool live = tx < nc;
    int xs = 0, xn = 0;
    if (live) {
        xs = cstart[x];
        xn = ccount[x];
        for (int k = ty; k < xn; k += RS_ROWS) s_cw[k][tx] = cwt[(size_t)x * d.ck + k];
    }
    if (ty < nr) {
        const int rn = rcount[r0 + ty];
        for (int k = tx; k < rn; k += RS_COLS) s_rw[ty][k] = rwt[(size_t)(r0 + ty) * d.rk + k];
    }
    __syncthreads();

    // columns: source row sr of the box at this lane's output column.  The run of taps starts in tile column j at sample u0
    const size_t plane = (size_t)a.rh * a.rw;
    const int64_t tstep = (int64_t)((size_t)a.c * plane);  // doubles from a tile to its right neighbour
    const int X = d.x0 + xs, j = X / a.tw, u0 = X - j * a.tw;
    if (live) {
        for (int sr = lo + ty; sr < hi; sr += RS_ROWS) {
            const int Y = d.y0 + sr, i = Y / a.th, v = Y - i * a.th;
            const double *p = a.tiles + ((size_t)d.s0 + (size_t)(i - d.i0) * d.nj + (size_t)(j - d.j0)) * (size_t)tstep +
                              (size_t)ch * plane + (size_t)v * a.rw + u0;
            int u = u0;
            double acc = *p * s_cw[0][tx];
            for (int k = 1; k < xn; k++) {
                ++u;
                ++p;
                if (u == a.tw) {  // the seam: first sample of the same row of the tile to the right
                    u = 0;
                    p += tstep - a.tw;
                }
                acc = acc + *p * s_cw[k][tx];
            }
            s_rows[sr - lo][tx] = acc;
        }
    }
    __syncthreads();

    // rows, the normalisation and the one store
    if (live && ty < nr) {
        const int r = r0 + ty, rs = rstart[r] - lo, rn = rcount[r];
        double acc = s_rows[rs][tx] * s_rw[ty][0];
        for (int k = 1; k < rn; k++) acc = acc + s_rows[rs + k][tx] * s_rw[ty][k];
        if (a.mean) acc = (acc - a.mean[ch]) / a.std[ch];
        *reinterpret_cast<T *>(d.out + (int64_t)ch * d.sc + (int64_t)r * d.sh + (int64_t)x * d.sw) = px_store_value<ES, FK>(acc);
    }
}

// ---- host launcher -------------------------------------------------------------------------------------------------------
template <int ES, int FK>
static int launch_resample(ResampleArgs a, int64_t B, hipStream_t st) {
    const uint32_t nrow = (uint32_t)((a.oh + RS_ROWS - 1) / RS_ROWS);
    a.ncol = (a.ow + RS_COLS - 1) / RS_COLS;
    hipLaunchKernelGGL((k_tile_resample_set<ES, FK>), dim3(nrow * (uint32_t)a.ncol, a.c, (uint32_t)B), dim3(RS_COLS, RS_ROWS), 0, st,
                       a);
    return (int)hipGetLastError();
}
extern "C" int spiht_launch_tile_resample_set(const ResampleArgs *a, int es, int kind, int64_t B, hipStream_t st) {
    switch (kind) {
    case SPIHT_FLT_F32: return launch_resample<4, SPIHT_FLT_F32>(*a, B, st);
    case SPIHT_FLT_F16: return launch_resample<2, SPIHT_FLT_F16>(*a, B, st);
    case SPIHT_FLT_BF16: return launch_resample<2, SPIHT_FLT_BF16>(*a, B, st);
    default: break;
    }
    switch (es) {
    case 1: return launch_resample<1, 0>(*a, B, st);
    case 2: return launch_resample<2, 0>(*a, B, st);
    case 8: return launch_resample<8, 0>(*a, B, st);
    default: return -1;
    }
}
