// Overlapping tiles (gfx950): every tile coded with a margin of m samples of its neighbours, the decoded tiles cross-faded
// over the 2m samples around each seam.  The rule is spiht_amd/overlap.py.
//   k_tile_cut_overlap  picture batch [N, c, H, W] -> dense tile batch [N * T, c, th + 2m, tw + 2m]; coded tile (i, j)'s sample
//                       (y, x) is the picture's at row clamp(i th - m + y, 0, H - 1), column clamp(j tw - m + x, 0, W - 1):
//                       k_tile_cut with an origin and a clamp on all four sides (m = 0 gives its bytes)
//   k_tile_blend        dense float64 tile batch of a sub-grid -> a window of the picture.  Where k_tile_paste copies, this does
//                       arithmetic: in the zone of a seam, (b * one tile + a * the other) / 4m, columns first, then rows, every
//                       operation rounded once (this file is built with -ffp-contract=off) and the division IEEE's;
//                       elsewhere the one tile's sample.  Output float64, or 8 / 16 bits by the decoder's conversion.
// Workgroups own rows of the window, as k_tile_mosaic's do: whether a row lies in a zone, its two tile rows and their weights
// are the same for all lanes of the row; only the column zone is per lane.  Both kernels store their rows by store_row
// (tiles_device.h).
#include "tiles_device.h"
#include "floatpx.h"

// ---- cut ---------------------------------------------------------------------------------------------------------------------
// One row of a coded tile: n elements of ES bytes to the dense dst, element k from picture column clamp(X0 + k, 0, W - 1) of the
// row at src (stride ss).  The lanes lane, lane + nlanes, ... of the caller share the row.  A 16-byte vector is one 16-byte load
// where its columns are contiguous in the source, unclamped and aligned.
template <int ES>
__device__ __forceinline__ void cut_row(uint8_t *dst, const uint8_t *src, int64_t ss, int n, int X0, int W, int lane, int nlanes) {
    typedef typename ElemOf<ES>::type T;
    auto elem = [&](int k) { return *reinterpret_cast<const T *>(src + (int64_t)min(max(X0 + k, 0), W - 1) * ss); };
    store_row<ES, int>(dst, ES, n, lane, nlanes, elem, [&](int k0) {
        const int X = X0 + k0;
        const uint8_t *s = src + (int64_t)X * ss;  // (formed, not read, where X is clamped)
        if (ss == ES && X >= 0 && X + 16 / ES <= W && ((uintptr_t)s & 15) == 0) return *reinterpret_cast<const Vec16 *>(s);
        return gather_vec<ES>(k0, elem);
    });
}

// grid (N * T, c, row chunks); block (bx, by): bx lanes along a row, by rows at a time
template <int ES>
__global__ __launch_bounds__(TL_THREADS) void k_tile_cut_overlap(const TileCutOverlapArgs q) {
    const TileCutArgs &a = q.cut;
    const uint32_t nt = blockIdx.x, ch = blockIdx.y, T = (uint32_t)a.gy * (uint32_t)a.gx;
    const uint32_t n = nt / T, t = nt - n * T;
    const int i = (int)(t / (uint32_t)a.gx), j = (int)(t - (uint32_t)i * (uint32_t)a.gx);
    const int ch_h = a.th + 2 * q.m, ch_w = a.tw + 2 * q.m;  // the coded tile
    const uint8_t *src0 = a.in + (int64_t)n * a.sb + (int64_t)ch * a.sc;
    uint8_t *dst0 = a.out + ((size_t)nt * a.c + ch) * (size_t)ch_h * ch_w * ES;
    const int ya = (int)blockIdx.z * a.rows, yb = min(ya + a.rows, ch_h);
    for (int y = ya + (int)threadIdx.y; y < yb; y += (int)blockDim.y) {
        const int Y = min(max(i * a.th - q.m + y, 0), a.H - 1);
        cut_row<ES>(dst0 + (size_t)y * ch_w * ES, src0 + (int64_t)Y * a.sh, a.sw, ch_w, j * a.tw - q.m, a.W, (int)threadIdx.x,
                    (int)blockDim.x);
    }
}

// ---- blend -------------------------------------------------------------------------------------------------------------------
// what a sample of the window is stored as: px_store_value (tiles_device.h)
// grid (row chunks of the window, c); block (bx, by): bx lanes along a window row, by rows at a time
template <int ES, int FK = 0>
__global__ __launch_bounds__(TL_THREADS) void k_tile_blend(const TileBlendArgs a) {
    typedef typename ElemOf<ES>::type T;
    const uint32_t ch = blockIdx.y;
    const int m = a.m, lane = (int)threadIdx.x, nlanes = (int)blockDim.x;
    const size_t plane = (size_t)a.rh * a.rw;
    const int64_t tstep = (int64_t)((size_t)a.c * plane);  // doubles from a tile to its right neighbour
    const double fm = (double)(4 * m);
    const uint32_t tw = (uint32_t)a.tw;
    const int64_t ya = (int64_t)blockIdx.x * a.rows;
    const int yb = (int)min(ya + a.rows, (int64_t)a.wh);
    for (int y = (int)ya + (int)threadIdx.y; y < yb; y += (int)blockDim.y) {
        // the row: one tile row, or the two around a seam with their weights
        const int Y = a.y0 + y, ky = (Y + m) / a.th, uy = Y + m - ky * a.th;
        const bool zy = ky >= 1 && ky < a.gy && uy < 2 * m;
        const int it = zy ? ky - 1 : (uy >= m ? ky : ky - 1);  // outside a zone: Y / th
        const double ay = (double)(2 * uy + 1), by = (double)(4 * m - (2 * uy + 1));
        // the row's sample of tile column j0, first sample of the coded tile
        const double *top = a.tiles + ((size_t)(it - a.i0) * a.nj * a.c + ch) * plane + (size_t)(Y - it * a.th + m) * a.rw;
        const double *bot = zy ? a.tiles + ((size_t)(ky - a.i0) * a.nj * a.c + ch) * plane + (size_t)uy * a.rw : top;
        auto hval = [&](const double *row, int X) -> double {  // the columns' blend of one tile row at picture column X
            const uint32_t kx = (uint32_t)(X + m) / tw, ux = (uint32_t)(X + m) - kx * tw;
            if (kx >= 1 && (int)kx < a.gx && (int)ux < 2 * m) {
                const double L = row[(int64_t)((int)kx - 1 - a.j0) * tstep + (ux + tw)];
                const double R = row[(int64_t)((int)kx - a.j0) * tstep + ux];
                const double ax = (double)(2 * ux + 1), bx = (double)(4 * m - (int)(2 * ux + 1));
                return (bx * L + ax * R) / fm;
            }
            const int j = (int)ux >= m ? (int)kx : (int)kx - 1;  // X / tw
            return row[(int64_t)(j - a.j0) * tstep + (X - j * a.tw + m)];
        };
        auto val = [&](int X) -> T {
            double r = hval(top, X);
            if (zy) r = (by * r + ay * hval(bot, X)) / fm;
            return px_store_value<ES, FK>(r);
        };
        auto elem = [&](int k) { return val(a.x0 + k); };
        store_row<ES, int64_t>(a.out + (int64_t)ch * a.sc + (int64_t)y * a.sh, a.sw, a.ww, lane, nlanes, elem,
                      [&](int k0) { return gather_vec<ES>(k0, elem); });
    }
}

// ---- host launchers ----------------------------------------------------------------------------------------------------------
extern "C" int spiht_launch_tile_cut_overlap(const TileCutOverlapArgs *p, int es, int64_t NT, hipStream_t st) {
    return dispatch_es(es, [&](auto e) {
        constexpr int ES = decltype(e)::value;
        TileCutOverlapArgs a = *p;
        dim3 block;
        uint32_t gz;
        const int64_t cw = (int64_t)a.cut.tw + 2 * a.m, chh = (int64_t)a.cut.th + 2 * a.m;
        row_blocks((cw * ES + 15) / 16 + 1, cw * ES, chh, &block, &a.cut.rows, &gz);
        hipLaunchKernelGGL(k_tile_cut_overlap<ES>, dim3((uint32_t)NT, a.cut.c, gz), block, 0, st, a);
        return (int)hipGetLastError();
    });
}

template <int ES, int FK = 0>
static int launch_blend(TileBlendArgs a, hipStream_t st) {
    dim3 block;
    uint32_t gz;
    window_blocks(a.sw == ES, a.ww, ES, a.wh, a.c, &block, &a.rows, &gz);  // a workgroup's rows are the window's
    hipLaunchKernelGGL((k_tile_blend<ES, FK>), dim3(gz, a.c), block, 0, st, a);
    return (int)hipGetLastError();
}
// es: bytes per sample of the OUTPUT: 8 float64, 1 / 2 the 8- / 16-bit conversion
extern "C" int spiht_launch_tile_blend(const TileBlendArgs *a, int es, hipStream_t st) {
    // (4-byte samples are a float kind: spiht_launch_tile_blend_flt)
    return dispatch_es(es, [&](auto e) { return launch_blend<decltype(e)::value == 4 ? 8 : decltype(e)::value>(*a, st); });
}
// ... into a float kind (floatpx.h)
extern "C" int spiht_launch_tile_blend_flt(const TileBlendArgs *a, int kind, hipStream_t st) {
    switch (kind) {
    case SPIHT_FLT_F32: return launch_blend<4, SPIHT_FLT_F32>(*a, st);
    case SPIHT_FLT_F16: return launch_blend<2, SPIHT_FLT_F16>(*a, st);
    case SPIHT_FLT_BF16: return launch_blend<2, SPIHT_FLT_BF16>(*a, st);
    default: return -1;
    }
}
