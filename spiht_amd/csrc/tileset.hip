// Picture sets (gfx950): the cut and the paste of tiles.hip for many pictures of different sizes in one launch.
//   k_tile_cut_set    P pictures, each a view of its own -> ONE dense tile batch [NT, c, th, tw], NT the sum of the pictures'
//                     tile counts; picture p's tiles at rows [tile0_p, tile0_p + T_p), edge-replicated as k_tile_cut's
//   k_tile_paste_set  one dense batch [S, c, rh, rw] of decoded tiles -> B windows of B pictures, item b made from the tiles
//                     [s0_b, s0_b + ni_b * nj_b) of the batch; every sample from the one tile that owns it
// A workgroup is one tile (x), one channel (y) and a chunk of the tile's rows (z), as in tiles.hip.  What k_tile_cut and
// k_tile_paste find in their launch arguments it reads from two device tables: the picture (item) of its tile, then that
// picture's (item's) row.  Both addresses depend on blockIdx alone, so both reads are scalar loads -- one dependent pair in
// front of the rows -- and nothing but the tiles (the windows) is written.  A table of the tile's picture costs 4 bytes a tile
// and one load; the search over tile0 it replaces would be log2(P) dependent loads in every workgroup.
// The rows are copied by tiles.hip's copy_row (tiles_device.h).
#include "tileset.h"
#include "tiles_device.h"

// grid (NT, c, row chunks); block (bx, by): bx lanes along a row, by rows at a time
template <int ES>
__global__ __launch_bounds__(TL_THREADS) void k_tile_cut_set(const TileSetCutArgs a) {
    const uint32_t nt = blockIdx.x, ch = blockIdx.y;
    const TileSetPic d = a.pics[a.pic_of_tile[nt]];  // (uniform: scalar loads)
    const uint32_t t = nt - d.tile0;
    const int i = (int)(t / (uint32_t)d.gx), j = (int)(t - (uint32_t)i * (uint32_t)d.gx);
    const int X0 = j * a.tw, nvalid = min(a.tw, d.W - X0);
    const uint8_t *src0 = d.in + (int64_t)ch * d.sc + (int64_t)X0 * d.sw;
    uint8_t *dst0 = a.out + ((size_t)nt * a.c + ch) * (size_t)a.th * a.tw * ES;
    const int ya = (int)blockIdx.z * a.rows, yb = min(ya + a.rows, a.th);
    for (int y = ya + (int)threadIdx.y; y < yb; y += (int)blockDim.y) {
        const int Y = min(i * a.th + y, d.H - 1);
        copy_row<ES>(dst0 + (size_t)y * a.tw * ES, ES, src0 + (int64_t)Y * d.sh, d.sw, a.tw, nvalid, (int)threadIdx.x, (int)blockDim.x);
    }
}

// grid (S, c, row chunks); a tile that does not meet its item's window has nothing to do
template <int ES>
__global__ __launch_bounds__(TL_THREADS) void k_tile_paste_set(const TileSetPasteArgs a) {
    const uint32_t s = blockIdx.x, ch = blockIdx.y;
    const TileSetItem d = a.items[a.item_of_tile[s]];  // (uniform: scalar loads)
    const uint32_t ls = s - d.s0;
    const int si = (int)(ls / (uint32_t)d.nj), sj = (int)(ls - (uint32_t)si * (uint32_t)d.nj);
    const int i = d.i0 + si, j = d.j0 + sj;
    const int Ya = max(i * a.th, d.y0), Yb = min((i + 1) * a.th, d.y0 + d.wh);
    const int Xa = max(j * a.tw, d.x0), Xb = min((j + 1) * a.tw, d.x0 + d.ww);
    if (Xb <= Xa || Yb <= Ya) return;
    const int n = Xb - Xa;
    const uint8_t *src0 = a.tiles + ((size_t)s * a.c + ch) * (size_t)a.rh * a.rw * ES + (size_t)(Xa - j * a.tw) * ES;
    uint8_t *dst0 = d.out + (int64_t)ch * d.sc + (int64_t)(Xa - d.x0) * d.sw;
    const int ya = Ya + (int)blockIdx.z * a.rows, yb = min(ya + a.rows, Yb);
    for (int Y = ya + (int)threadIdx.y; Y < yb; Y += (int)blockDim.y)
        copy_row<ES>(dst0 + (int64_t)(Y - d.y0) * d.sh, d.sw, src0 + (size_t)(Y - i * a.th) * a.rw * ES, ES, n, n, (int)threadIdx.x,
                     (int)blockDim.x);
}

// ---- host launchers ------------------------------------------------------------------------------------------------------

extern "C" int spiht_launch_tile_cut_set(const TileSetCutArgs *p, int es, int64_t NT, hipStream_t st) {
    return dispatch_es(es, [&](auto e) {
        constexpr int ES = decltype(e)::value;
        TileSetCutArgs a = *p;
        dim3 block;
        uint32_t gz;
        row_blocks(((int64_t)a.tw * ES + 15) / 16 + 1, (int64_t)a.tw * ES, a.th, &block, &a.rows, &gz);
        hipLaunchKernelGGL(k_tile_cut_set<ES>, dim3((uint32_t)NT, a.c, gz), block, 0, st, a);
        return (int)hipGetLastError();
    });
}

extern "C" int spiht_launch_tile_paste_set(const TileSetPasteArgs *p, int es, int64_t S, int64_t n, int64_t rows, int strided,
                                           hipStream_t st) {
    return dispatch_es(es, [&](auto e) {
        constexpr int ES = decltype(e)::value;
        TileSetPasteArgs a = *p;
        dim3 block;
        uint32_t gz;
        row_blocks(strided ? n : (n * ES + 15) / 16 + 1, n * ES, rows, &block, &a.rows, &gz);
        hipLaunchKernelGGL(k_tile_paste_set<ES>, dim3((uint32_t)S, a.c, gz), block, 0, st, a);
        return (int)hipGetLastError();
    });
}
