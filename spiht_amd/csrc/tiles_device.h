// Tiled pictures: the device code that tiles.hip, tileset.hip, overlap.hip and layers.hip share -- the row store of the cut with a
// margin, the mosaic and the blend, the plain row copy of cut and paste, and the workgroup's exclusive scan.
#pragma once
#include "tiles.h"
#include "floatpx.h"

// 16 bytes, as a lane loads and stores them
typedef uint32_t Vec16 __attribute__((ext_vector_type(4)));

// The 16 bytes of elements k0 .. k0 + 16 / ES - 1, gathered one by one.
template <int ES, typename ELEM>
__device__ __forceinline__ Vec16 gather_vec(int k0, ELEM elem) {
    typename ElemOf<ES>::type e[16 / ES];
#pragma unroll
    for (int i = 0; i < 16 / ES; i++) e[i] = elem(k0 + i);
    Vec16 q;
    __builtin_memcpy(&q, e, 16);
    return q;
}

// What a float64 sample is stored as by the kernels that do arithmetic on decoded tiles (blend, resample).  8 / 16 bits: the
// decoder's conversion of a float64 sample (dwt_device.h, px8_store_value / px16_store_value): clip to [0, 1], times 255 /
// 65535, truncate; NaN -> 0 (fmax / fmin return the number of a pair with a NaN).  FK != 0: a float kind (floatpx.h: 1 float32,
// 2 float16, 3 bfloat16) -- the float64 sample rounded once to the kind, as the decoder's float store does
template <int ES, int FK = 0> __device__ __forceinline__ typename ElemOf<ES>::type px_store_value(double v) {
    if constexpr (FK != 0) {
        return (typename ElemOf<ES>::type)flt_store_value(v, FK);
    } else if constexpr (ES == 8) {
        return (uint64_t)__double_as_longlong(v);
    } else {
        const double c = fmin(fmax(v, 0.0), 1.0);
        const double s = c * (ES == 1 ? 255.0 : 65535.0);
        return (typename ElemOf<ES>::type)(uint32_t)s;
    }
}

// One row of n elements of ES bytes, element k to dst + k * ds; dst and ds are multiples of ES.  The lanes lane, lane + nlanes,
// ... of the caller share the row: consecutive lanes store consecutive vectors.  THE ALIGNMENT RULE of the copies: where the
// destination is contiguous, a lane stores 16 bytes at each 16-byte-aligned address of it whose 16 bytes all belong to the row;
// what lies in front of the first and behind the last such address goes element by element.  A strided destination (HWC, RGBA)
// goes element by element, and what lies between the elements is not written.
//   BYTES     the integer that counts the row's bytes: int for a row of a tile (at most 2^24 + 2^25 elements: api_tiles.cpp),
//             int64_t for a row of a window (up to 2^30 elements)
//   elem(k)   element k (the unsigned integer of ES bytes), 0 <= k < n
//   fill(k0)  the 16 bytes of elements k0 .. k0 + 16 / ES - 1, all of them inside the row: the caller's rule for when that is
//             one aligned 16-byte load, and how it is gathered otherwise
template <int ES, typename BYTES, typename ELEM, typename FILL>
__device__ __forceinline__ void store_row(uint8_t *dst, int64_t ds, int n, int lane, int nlanes, ELEM elem, FILL fill) {
    typedef typename ElemOf<ES>::type T;
    constexpr int EPV = 16 / ES;
    if (ds != ES) {
        for (int k = lane; k < n; k += nlanes) *reinterpret_cast<T *>(dst + (int64_t)k * ds) = elem(k);
        return;
    }
    const int a = (int)((uintptr_t)dst & 15);
    const BYTES nbytes = (BYTES)n * ES;
    const int nvec = (int)((a + nbytes + 15) >> 4);
    for (int v = lane; v < nvec; v += nlanes) {
        const BYTES p = 16 * (BYTES)v - a;  // bytes from dst; a multiple of ES, negative in the first vector of an unaligned row
        const int k0 = (int)(p / ES);
        if (p >= 0 && p + 16 <= nbytes) {
            *reinterpret_cast<Vec16 *>(dst + p) = fill(k0);
        } else {
#pragma unroll
            for (int i = 0; i < EPV; i++) {
                const int k = k0 + i;
                if (k >= 0 && k < n) *reinterpret_cast<T *>(dst + (int64_t)k * ES) = elem(k);
            }
        }
    }
}

// The plain copy of a row (cut, paste and their picture-set forms): element k from src + min(k, nvalid - 1) * ss (replication
// past nvalid); src and ss are multiples of ES.  A vector is one 16-byte load where the source is contiguous, unreplicated and
// aligned as well.  It is store_row's rule WRITTEN OUT, not a call of it: on the skeleton the 8-bit cut measured above the spread
// of this text's own runs (profiles/tile_kernels_fold.txt), so this text stays until a wording of the call compiles to its code.
template <int ES>
__device__ __forceinline__ void copy_row(uint8_t *dst, int64_t ds, const uint8_t *src, int64_t ss, int n, int nvalid, int lane,
                                         int nlanes) {
    typedef typename ElemOf<ES>::type T;
    constexpr int EPV = 16 / ES;
    if (ds != ES) {  // a strided destination (HWC, RGBA): what lies between the elements is not written
        for (int k = lane; k < n; k += nlanes)
            *reinterpret_cast<T *>(dst + (int64_t)k * ds) = *reinterpret_cast<const T *>(src + (int64_t)min(k, nvalid - 1) * ss);
        return;
    }
    const int a = (int)((uintptr_t)dst & 15), nbytes = n * ES;
    const int nvec = (a + nbytes + 15) >> 4;
    for (int v = lane; v < nvec; v += nlanes) {
        const int p = 16 * v - a;  // bytes from dst; a multiple of ES, negative in the first vector of an unaligned row
        const int k0 = p / ES;
        if (p >= 0 && p + 16 <= nbytes) {
            const uint8_t *s = src + (int64_t)k0 * ss;
            uint4 q;
            if (ss == ES && k0 + EPV <= nvalid && ((uintptr_t)s & 15) == 0) {
                q = *reinterpret_cast<const uint4 *>(s);
            } else {
                T e[EPV];
#pragma unroll
                for (int i = 0; i < EPV; i++) e[i] = *reinterpret_cast<const T *>(src + (int64_t)min(k0 + i, nvalid - 1) * ss);
                __builtin_memcpy(&q, e, 16);
            }
            *reinterpret_cast<uint4 *>(dst + p) = q;
        } else {
#pragma unroll
            for (int i = 0; i < EPV; i++) {
                const int k = k0 + i;
                if (k >= 0 && k < n)
                    *reinterpret_cast<T *>(dst + (int64_t)k * ES) = *reinterpret_cast<const T *>(src + (int64_t)min(k, nvalid - 1) * ss);
            }
        }
    }
}

// One round of an exclusive scan of uint64 in thread order by a workgroup of TL_THREADS, one value per thread and round: returns
// the sum of the earlier rounds' values (carry) and of v over the threads before this one, and adds the round's total to carry.
// wsum: TL_THREADS / 64 words of LDS; the caller puts a __syncthreads() between this call and the next that uses them.
__device__ __forceinline__ uint64_t block_scan_exclusive(uint64_t v, uint64_t &carry, uint64_t *wsum) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(x, o);
        if ((int)lane >= o) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint64_t pre = 0, total = 0;
    for (uint32_t k = 0; k < TL_THREADS / 64; k++) {
        if (k < wv) pre += wsum[k];
        total += wsum[k];
    }
    const uint64_t before = carry + pre + x - v;
    carry += total;
    return before;
}
