// Quality layers of a tiled picture (gfx950): the tiles' streams in layer-major order, so that any prefix of the run is the
// whole picture at a lower rate.  Layer q holds, tile by tile, the bytes [B(q-1, t), B(q, t)) of tile t's stream; B is
// non-decreasing in q (the allocations at growing budgets nest: spiht_amd/alloc.py, allocate_layers).
//   k_layer_table   pack: Q rows of allocated bits -> B [N][Q][T], the running maximum of min(ceil(bits / 8), slot_stride)
//   k_layer_raw     unpack: a table [Q][T] -> its running maximum over q (a table that falls still names a valid run)
//   k_layer_scan    the pieces' lengths B(q, t) - B(q-1, t) in file order -> their exclusive prefix sums (one workgroup)
//   k_layer_pack    slots -> the run: piece (q, t) of slot t to its offset; nothing at or past cap
//   k_layer_unpack  the run -> zero-padded slots: the pieces of layers < upto of a tile one behind the other, zeros behind
// Both copies are copy_bytes per piece (copy_bytes.h): chunks cut at 16-byte-aligned destination addresses, the ragged ends
// byte by byte, so neighbouring pieces write disjoint bytes.  Plain vector and byte stores; no atomics.
#include "tiles_device.h"
#include "copy_bytes.h"

// grid over the N * T tiles, one thread each.  bits [Q][NT] -> cum [N][Q][T]
__global__ __launch_bounds__(TL_THREADS) void k_layer_table(const uint64_t *__restrict__ bits, uint32_t Q, uint32_t NT, uint32_t T,
                                                            uint64_t slot_stride, uint32_t *__restrict__ cum) {
    const uint32_t i = blockIdx.x * TL_THREADS + threadIdx.x;
    if (i >= NT) return;
    const uint32_t n = i / T, t = i - n * T;
    uint64_t B = 0;
    for (uint32_t q = 0; q < Q; q++) {
        const uint64_t b = bits[(size_t)q * NT + i];
        B = max(B, min((b >> 3) + ((b & 7) != 0), slot_stride));
        cum[((size_t)n * Q + q) * T + t] = (uint32_t)B;
    }
}

// one thread per tile.  cum [Q][T] (the first `upto` rows are read) -> M [upto][T], the running maximum over q
__global__ __launch_bounds__(TL_THREADS) void k_layer_raw(const uint32_t *__restrict__ cum, uint32_t upto, uint32_t T,
                                                          uint32_t *__restrict__ M) {
    const uint32_t t = blockIdx.x * TL_THREADS + threadIdx.x;
    if (t >= T) return;
    uint32_t m = 0;
    for (uint32_t q = 0; q < upto; q++) {
        m = max(m, cum[(size_t)q * T + t]);
        M[(size_t)q * T + t] = m;
    }
}

// the length of piece e of a table [.][Q][T] that does not fall in q
__device__ __forceinline__ uint32_t piece_len(const uint32_t *__restrict__ B, uint32_t e, uint32_t Q, uint32_t T) {
    return B[e] - ((e / T) % Q ? B[e - T] : 0u);
}

// B [P][Q][T] -> off [P * Q * T]: the sum of the pieces before e in file order.  One workgroup: 256 pieces per round, a carry
// between rounds (tiles_device.h: block_scan_exclusive, as k_tile_scan).
__global__ __launch_bounds__(TL_THREADS) void k_layer_scan(const uint32_t *__restrict__ B, uint32_t n, uint32_t Q, uint32_t T,
                                                           uint64_t *__restrict__ off) {
    __shared__ uint64_t wsum[TL_THREADS / 64];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n; base += TL_THREADS) {
        const uint32_t idx = base + threadIdx.x;
        const uint64_t before = block_scan_exclusive(idx < n ? piece_len(B, idx, Q, T) : 0, carry, wsum);
        if (idx < n) off[idx] = before;
        __syncthreads();
    }
}

// grid (N * T, Q, chunks of a slot).  Piece (q, t) of picture n: bytes [B(q-1, t), B(q, t)) of slot n * T + t to
// packed + off; the workgroup of a picture's first piece also writes the picture's length.
__global__ __launch_bounds__(TL_THREADS) void k_layer_pack(const uint8_t *__restrict__ slots, uint64_t slot_stride,
                                                           const uint32_t *__restrict__ cum, const uint64_t *__restrict__ off,
                                                           uint32_t Q, uint32_t T, uint8_t *__restrict__ packed, uint64_t cap,
                                                           uint64_t *__restrict__ pic_bytes) {
    const uint32_t i = blockIdx.x, q = blockIdx.y, n = i / T, t = i - n * T;
    const uint32_t first = n * Q * T, e = first + q * T + t;
    if (t == 0 && q == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
        const uint32_t last = first + Q * T - 1;
        pic_bytes[n] = off[last] + piece_len(cum, last, Q, T) - off[first];
    }
    const uint64_t hi = cum[e], lo = hi - piece_len(cum, e, Q, T);
    const uint64_t o = off[e];
    if (hi == lo || o >= cap) return;
    const uint64_t len = min(hi - lo, cap - o);
    const uint8_t *slot = slots + (size_t)i * slot_stride;
    copy_bytes(packed + o, slot + lo, len, len, slot, slot + slot_stride, blockIdx.z);
}

// grid (S, upto + 1, chunks of a slot).  Slot s holds tile sel[s] (clamped to the table; NULL: tile s).  y < upto: piece
// (y, t) of the run (those of its bytes that lie inside the run; zeros for the others) to its place in the slot; y == upto: the
// zeros from the tile's end up to slot_stride, and the tile's length.  M: the table's running maximum (k_layer_raw).
__global__ __launch_bounds__(TL_THREADS) void k_layer_unpack(const uint8_t *__restrict__ layers, uint64_t layers_bytes,
                                                             const uint32_t *__restrict__ M, const uint64_t *__restrict__ off,
                                                             uint32_t upto, uint32_t T, const int32_t *__restrict__ sel,
                                                             uint8_t *__restrict__ slots, uint64_t slot_stride,
                                                             uint64_t *__restrict__ nbytes) {
    const uint32_t s = blockIdx.x, q = blockIdx.y;
    const uint32_t t = sel ? (uint32_t)min(max(sel[s], 0), (int32_t)T - 1) : s;
    uint8_t *slot = slots + (size_t)s * slot_stride;
    if (q == upto) {
        const uint64_t end = min((uint64_t)M[(size_t)(upto - 1) * T + t], slot_stride);
        if (blockIdx.z == 0 && threadIdx.x == 0) nbytes[s] = end;
        if (end < slot_stride) copy_bytes(slot + end, layers, slot_stride - end, 0, layers, layers + layers_bytes, blockIdx.z);
        return;
    }
    const uint32_t e = q * T + t;
    const uint64_t lo = min((uint64_t)(q ? M[e - T] : 0u), slot_stride), hi = min((uint64_t)M[e], slot_stride);
    if (hi == lo) return;
    const uint64_t o = off[e];  // the piece's first byte; lo < slot_stride, so it is the byte that goes to slot + lo
    const uint64_t have = o < layers_bytes ? min(hi - lo, layers_bytes - o) : 0;
    copy_bytes(slot + lo, layers + min(o, layers_bytes), hi - lo, have, layers, layers + layers_bytes, blockIdx.z);
}

// ---- host launchers ------------------------------------------------------------------------------------------------------

// d_off: uint64 [N * Q * T] (scratch)
extern "C" int spiht_launch_layer_pack(const uint8_t *d_slots, uint64_t slot_stride, const uint64_t *d_cum_bits, int64_t Q, int64_t N,
                                       int64_t T, uint64_t *d_off, uint8_t *d_packed, uint64_t cap, uint32_t *d_cum,
                                       uint64_t *d_pic_bytes, hipStream_t st) {
    const uint32_t NT = (uint32_t)(N * T);
    hipLaunchKernelGGL(k_layer_table, dim3((NT + TL_THREADS - 1) / TL_THREADS), dim3(TL_THREADS), 0, st, d_cum_bits, (uint32_t)Q, NT,
                       (uint32_t)T, slot_stride, d_cum);
    hipLaunchKernelGGL(k_layer_scan, dim3(1), dim3(TL_THREADS), 0, st, (const uint32_t *)d_cum, (uint32_t)(N * Q * T), (uint32_t)Q,
                       (uint32_t)T, d_off);
    hipLaunchKernelGGL(k_layer_pack, dim3(NT, (uint32_t)Q, slot_chunks(slot_stride)), dim3(TL_THREADS), 0, st, d_slots, slot_stride,
                       (const uint32_t *)d_cum, (const uint64_t *)d_off, (uint32_t)Q, (uint32_t)T, d_packed, cap, d_pic_bytes);
    return (int)hipGetLastError();
}
// d_off: uint64 [upto * T], d_M: uint32 [upto * T] (scratch)
extern "C" int spiht_launch_layer_unpack(const uint8_t *d_layers, uint64_t layers_bytes, const uint32_t *d_cum, int64_t T,
                                         int64_t upto, const int32_t *d_sel, int64_t S, uint64_t *d_off, uint32_t *d_M,
                                         uint8_t *d_slots, uint64_t slot_stride, uint64_t *d_nbytes, hipStream_t st) {
    hipLaunchKernelGGL(k_layer_raw, dim3(((uint32_t)T + TL_THREADS - 1) / TL_THREADS), dim3(TL_THREADS), 0, st, d_cum, (uint32_t)upto,
                       (uint32_t)T, d_M);
    hipLaunchKernelGGL(k_layer_scan, dim3(1), dim3(TL_THREADS), 0, st, (const uint32_t *)d_M, (uint32_t)(upto * T), (uint32_t)upto,
                       (uint32_t)T, d_off);
    hipLaunchKernelGGL(k_layer_unpack, dim3((uint32_t)S, (uint32_t)upto + 1, slot_chunks(slot_stride)), dim3(TL_THREADS), 0, st,
                       d_layers, layers_bytes, (const uint32_t *)d_M, (const uint64_t *)d_off, (uint32_t)upto, (uint32_t)T, d_sel,
                       d_slots, slot_stride, d_nbytes);
    return (int)hipGetLastError();
}
