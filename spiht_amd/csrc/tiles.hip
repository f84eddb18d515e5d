// Tiled pictures (gfx950): one picture as a batch of equal tiles, each coded as a picture of its own by the batched calls.
//   k_tile_cut     picture batch [N, c, H, W] -> dense tile batch [N * T, c, th, tw]; samples past the picture's bottom /
//                  right edge repeat the last row / column (numpy's np.pad(mode="edge"))
//   k_tile_paste   dense tile batch of a sub-grid -> a window of the picture; every sample from the one tile that owns it
//   k_tile_mosaic  the paste of reduced tiles: a source origin inside the tile, tile sides down to 1, workgroups that own rows
//                  of the window and gather across the tiles
//   k_tile_scan    stream lengths -> their exclusive prefix sums (one workgroup)
//   k_tile_pack    T stream slots -> one contiguous run of bytes
//   k_tile_unpack  the run -> T zero-padded slots
// All of them are copies with index arithmetic.  A lane stores 16 bytes at a 16-byte-aligned address of the destination
// wherever the destination is contiguous; what lies in front of the first and behind the last such address of a row (a
// stream) goes element by element (byte by byte).  The source side: cut / paste load 16 bytes where the source address is
// aligned as well and element by element where it is not; pack / unpack, whose two sides are never aligned to one another,
// load the aligned 32-bit words around the bytes and shift them into place.
#include "tiles_device.h"
#include "copy_bytes.h"

// grid (N * T, c, row chunks); block (bx, by): bx lanes along a row, by rows at a time
template <int ES>
__global__ __launch_bounds__(TL_THREADS) void k_tile_cut(const TileCutArgs a) {
    const uint32_t nt = blockIdx.x, ch = blockIdx.y, T = (uint32_t)a.gy * (uint32_t)a.gx;
    const uint32_t n = nt / T, t = nt - n * T;
    const int i = (int)(t / (uint32_t)a.gx), j = (int)(t - (uint32_t)i * (uint32_t)a.gx);
    const int X0 = j * a.tw, nvalid = min(a.tw, a.W - X0);
    const uint8_t *src0 = a.in + (int64_t)n * a.sb + (int64_t)ch * a.sc + (int64_t)X0 * a.sw;
    uint8_t *dst0 = a.out + ((size_t)nt * a.c + ch) * (size_t)a.th * a.tw * ES;
    const int ya = (int)blockIdx.z * a.rows, yb = min(ya + a.rows, a.th);
    for (int y = ya + (int)threadIdx.y; y < yb; y += (int)blockDim.y) {
        const int Y = min(i * a.th + y, a.H - 1);
        copy_row<ES>(dst0 + (size_t)y * a.tw * ES, ES, src0 + (int64_t)Y * a.sh, a.sw, a.tw, nvalid, (int)threadIdx.x, (int)blockDim.x);
    }
}

// grid (tiles of the sub-grid, c, row chunks); a tile that does not meet the window has nothing to do
template <int ES>
__global__ __launch_bounds__(TL_THREADS) void k_tile_paste(const TilePasteArgs a) {
    const uint32_t s = blockIdx.x, ch = blockIdx.y;
    const int si = (int)(s / (uint32_t)a.nj), sj = (int)(s - (uint32_t)si * (uint32_t)a.nj);
    const int i = a.i0 + si, j = a.j0 + sj;
    const int Ya = max(i * a.th, a.y0), Yb = min((i + 1) * a.th, a.y0 + a.wh);
    const int Xa = max(j * a.tw, a.x0), Xb = min((j + 1) * a.tw, a.x0 + a.ww);
    if (Xb <= Xa || Yb <= Ya) return;
    const int n = Xb - Xa;
    const uint8_t *src0 = a.tiles + ((size_t)s * a.c + ch) * (size_t)a.rh * a.rw * ES + (size_t)(Xa - j * a.tw) * ES;
    uint8_t *dst0 = a.out + (int64_t)ch * a.sc + (int64_t)(Xa - a.x0) * a.sw;
    const int ya = Ya + (int)blockIdx.z * a.rows, yb = min(ya + a.rows, Yb);
    for (int Y = ya + (int)threadIdx.y; Y < yb; Y += (int)blockDim.y)
        copy_row<ES>(dst0 + (int64_t)(Y - a.y0) * a.sh, a.sw, src0 + (size_t)(Y - i * a.th) * a.rw * ES, ES, n, n, (int)threadIdx.x,
                     (int)blockDim.x);
}

// One row of the mosaic: n elements of ES bytes, element k being picture column x0 + k, taken from the tile that owns it.
// row: the address of the row's sample of picture column j0 * tw (the first sample the row's first tile of the sub-grid
// gives); tile j's samples lie (j - j0) * tstep bytes further on.  A 16-byte vector of the destination may span several
// tiles (8-bit tiles of 2 columns: eight); a vector that lies in one tile and has an aligned source is one 16-byte load,
// any other is gathered element by element, stepping to the next tile at each seam.  The lanes lane, lane + nlanes, ... of
// the caller share the row: consecutive lanes store consecutive vectors.
template <int ES>
__device__ __forceinline__ void mosaic_row(uint8_t *dst, int64_t ds, const uint8_t *row, int64_t tstep, uint32_t tw, int j0, int x0,
                                           int n, int lane, int nlanes) {
    typedef typename ElemOf<ES>::type T;
    constexpr int EPV = 16 / ES;
    auto elem = [&](int k) {
        const uint32_t X = (uint32_t)(x0 + k), j = X / tw, tx = X - j * tw;  // picture column X >= 0
        return *reinterpret_cast<const T *>(row + (int64_t)((int)j - j0) * tstep + (size_t)tx * ES);
    };
    store_row<ES, int64_t>(dst, ds, n, lane, nlanes, elem, [&](int k0) {
        const uint32_t X = (uint32_t)(x0 + k0), j = X / tw;
        uint32_t tx = X - j * tw;
        const uint8_t *s = row + (int64_t)((int)j - j0) * tstep + (size_t)tx * ES;
        if (tx + EPV <= tw && ((uintptr_t)s & 15) == 0) return *reinterpret_cast<const Vec16 *>(s);
        return gather_vec<ES>(0, [&](int) {
            const T e = *reinterpret_cast<const T *>(s);
            s += ES;
            if (++tx == tw) {  // the seam: the same row of the next tile
                tx = 0;
                s += tstep - (int64_t)tw * ES;
            }
            return e;
        });
    });
}

// grid (row chunks of the window, c); block (bx, by): bx lanes along a window row, by rows at a time.  Picture-centric: a
// workgroup's rows cross every tile of the sub-grid's row that the window meets.
template <int ES>
__global__ __launch_bounds__(TL_THREADS) void k_tile_mosaic(const TileMosaicArgs a) {
    const uint32_t ch = blockIdx.y;
    const size_t plane = (size_t)a.rh * a.rw * ES;
    const int64_t ya = (int64_t)blockIdx.x * a.rows;
    const int yb = (int)min(ya + a.rows, (int64_t)a.wh);
    for (int y = (int)ya + (int)threadIdx.y; y < yb; y += (int)blockDim.y) {
        const int Y = a.y0 + y, i = Y / a.th;
        const uint8_t *row = a.tiles + ((size_t)(i - a.i0) * a.nj * a.c + ch) * plane
                             + ((size_t)(Y - i * a.th + a.oy) * a.rw + a.ox) * ES;
        mosaic_row<ES>(a.out + (int64_t)ch * a.sc + (int64_t)y * a.sh, a.sw, row, (int64_t)((size_t)a.c * plane), (uint32_t)a.tw, a.j0,
                       a.x0, a.ww, (int)threadIdx.x, (int)blockDim.x);
    }
}

// in[T] (each taken as min(in[t], lim)) -> off[t] = the sum of those before t, out[t] = the clipped value in the other
// width.  One workgroup: 256 lengths per round, a carry between rounds.
template <typename TIN, typename TOUT>
__global__ __launch_bounds__(TL_THREADS) void k_tile_scan(const TIN *__restrict__ in, uint32_t T, uint64_t lim,
                                                          uint64_t *__restrict__ off, TOUT *__restrict__ out) {
    __shared__ uint64_t wsum[TL_THREADS / 64];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < T; base += TL_THREADS) {
        const uint32_t idx = base + threadIdx.x;
        const uint64_t v = idx < T ? min((uint64_t)in[idx], lim) : 0;
        const uint64_t before = block_scan_exclusive(v, carry, wsum);
        if (idx < T) {
            off[idx] = before;
            out[idx] = (TOUT)v;
        }
        __syncthreads();
    }
}

// grid (T, chunks of a slot).  Stream t: lens[t] bytes of slot t to packed + off[t]; nothing is written at or past cap.
__global__ __launch_bounds__(TL_THREADS) void k_tile_pack(const uint8_t *__restrict__ slots, uint64_t slot_stride,
                                                          const uint32_t *__restrict__ lens, const uint64_t *__restrict__ off,
                                                          uint8_t *__restrict__ packed, uint64_t cap) {
    const uint32_t t = blockIdx.x;
    const uint64_t o = off[t];
    if (o >= cap) return;
    const uint64_t len = min((uint64_t)lens[t], cap - o);
    const uint8_t *src = slots + (size_t)t * slot_stride;
    copy_bytes(packed + o, src, len, len, src, src + slot_stride, blockIdx.y);
}

// grid (T, chunks of a slot).  Slot t: the nbytes[t] bytes at packed + off[t] (those that lie inside the run), then zeros up
// to slot_stride.
__global__ __launch_bounds__(TL_THREADS) void k_tile_unpack(const uint8_t *__restrict__ packed, uint64_t packed_bytes,
                                                            const uint64_t *__restrict__ nbytes, const uint64_t *__restrict__ off,
                                                            uint8_t *__restrict__ slots, uint64_t slot_stride) {
    const uint32_t t = blockIdx.x;
    const uint64_t o = off[t];
    const uint64_t len = o < packed_bytes ? min(nbytes[t], packed_bytes - o) : 0;
    copy_bytes(slots + (size_t)t * slot_stride, packed + min(o, packed_bytes), slot_stride, len, packed, packed + packed_bytes,
               blockIdx.y);
}

// ---- host launchers ------------------------------------------------------------------------------------------------------

extern "C" int spiht_launch_tile_cut(const TileCutArgs *p, int es, int64_t NT, hipStream_t st) {
    return dispatch_es(es, [&](auto e) {
        constexpr int ES = decltype(e)::value;
        TileCutArgs a = *p;
        dim3 block;
        uint32_t gz;
        row_blocks(((int64_t)a.tw * ES + 15) / 16 + 1, (int64_t)a.tw * ES, a.th, &block, &a.rows, &gz);
        hipLaunchKernelGGL(k_tile_cut<ES>, dim3((uint32_t)NT, a.c, gz), block, 0, st, a);
        return (int)hipGetLastError();
    });
}

extern "C" int spiht_launch_tile_paste(const TilePasteArgs *p, int es, int64_t ntiles, hipStream_t st) {
    return dispatch_es(es, [&](auto e) {
        constexpr int ES = decltype(e)::value;
        TilePasteArgs a = *p;
        dim3 block;
        uint32_t gz;
        const int64_t n = std::min<int64_t>(a.tw, a.ww);  // the longest row piece a tile gives
        row_blocks(a.sw == ES ? (n * ES + 15) / 16 + 1 : n, n * ES, std::min<int64_t>(a.th, a.wh), &block, &a.rows, &gz);
        hipLaunchKernelGGL(k_tile_paste<ES>, dim3((uint32_t)ntiles, a.c, gz), block, 0, st, a);
        return (int)hipGetLastError();
    });
}

extern "C" int spiht_launch_tile_mosaic(const TileMosaicArgs *p, int es, hipStream_t st) {
    return dispatch_es(es, [&](auto e) {
        constexpr int ES = decltype(e)::value;
        TileMosaicArgs a = *p;
        dim3 block;
        uint32_t gz;
        window_blocks(a.sw == ES, a.ww, ES, a.wh, a.c, &block, &a.rows, &gz);  // a workgroup's rows are the window's
        hipLaunchKernelGGL(k_tile_mosaic<ES>, dim3(gz, a.c), block, 0, st, a);
        return (int)hipGetLastError();
    });
}

// d_nbytes [T] (scratch: the streams' byte lengths) -> d_off [T] (scratch), d_lens [T]; then the gather
extern "C" int spiht_launch_tile_pack(const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_nbytes, int64_t T,
                                      uint64_t *d_off, uint8_t *d_packed, uint64_t cap, uint32_t *d_lens, hipStream_t st) {
    hipLaunchKernelGGL((k_tile_scan<uint64_t, uint32_t>), dim3(1), dim3(TL_THREADS), 0, st, d_nbytes, (uint32_t)T, slot_stride, d_off,
                       d_lens);
    hipLaunchKernelGGL(k_tile_pack, dim3((uint32_t)T, slot_chunks(slot_stride)), dim3(TL_THREADS), 0, st, d_slots, slot_stride,
                       (const uint32_t *)d_lens, (const uint64_t *)d_off, d_packed, cap);
    return (int)hipGetLastError();
}
// d_lens [T] -> d_off [T] (scratch), d_nbytes [T]; then the scatter into zero-padded slots
extern "C" int spiht_launch_tile_unpack(const uint8_t *d_packed, uint64_t packed_bytes, const uint32_t *d_lens, int64_t T,
                                        uint64_t *d_off, uint8_t *d_slots, uint64_t slot_stride, uint64_t *d_nbytes,
                                        hipStream_t st) {
    hipLaunchKernelGGL((k_tile_scan<uint32_t, uint64_t>), dim3(1), dim3(TL_THREADS), 0, st, d_lens, (uint32_t)T, slot_stride, d_off,
                       d_nbytes);
    hipLaunchKernelGGL(k_tile_unpack, dim3((uint32_t)T, slot_chunks(slot_stride)), dim3(TL_THREADS), 0, st, d_packed, packed_bytes,
                       (const uint64_t *)d_nbytes, (const uint64_t *)d_off, d_slots, slot_stride);
    return (int)hipGetLastError();
}
