// The byte copy of the stream kernels (tiles.hip: pack, unpack; alloc.hip: prefix slots): device code only.
#pragma once
#include "tiles.h"

// a 16-byte load from an address that is only 4-byte aligned
struct __attribute__((packed, aligned(4))) U32x4u {
    uint32_t v[4];
};

// One workgroup's share (chunk) of n_total destination bytes at dst: byte pos is src[pos] for pos < n_copy and zero behind.
// Chunks are cut at 16-byte-aligned addresses of dst.  [lo, hi) is what may be read around src (lo 4-byte aligned): a vector
// whose source words lie inside it is loaded as aligned 32-bit words and shifted, any other byte by byte.
__device__ __forceinline__ void copy_bytes(uint8_t *dst, const uint8_t *src, uint64_t n_total, uint64_t n_copy, const uint8_t *lo,
                                           const uint8_t *hi, uint32_t chunk) {
    const int64_t nt = (int64_t)n_total, nc = (int64_t)n_copy;
    const int64_t pbase = (int64_t)chunk * TL_CHUNK - (int64_t)((uintptr_t)dst & 15);
    if (pbase >= nt) return;
#pragma unroll
    for (int r = 0; r < TL_CHUNK / 16 / TL_THREADS; r++) {
        const int64_t p = pbase + 16 * (int64_t)(r * TL_THREADS + (int)threadIdx.x);
        if (p >= nt || p + 16 <= 0) continue;
        if (p >= 0 && p + 16 <= nt) {
            uint4 q = make_uint4(0, 0, 0, 0);
            if (p + 16 <= nc) {
                const uint8_t *s = src + p;
                const uint32_t m = (uint32_t)((uintptr_t)s & 3);
                const uint8_t *sa = s - m;
                if (sa >= lo && sa + (m ? 20 : 16) <= hi) {
                    const U32x4u w = *reinterpret_cast<const U32x4u *>(sa);
                    uint32_t w4 = 0;
                    if (m) w4 = *reinterpret_cast<const uint32_t *>(sa + 16);
                    q.x = __builtin_amdgcn_alignbyte(w.v[1], w.v[0], m);
                    q.y = __builtin_amdgcn_alignbyte(w.v[2], w.v[1], m);
                    q.z = __builtin_amdgcn_alignbyte(w.v[3], w.v[2], m);
                    q.w = __builtin_amdgcn_alignbyte(w4, w.v[3], m);
                } else {
                    uint8_t e[16];
#pragma unroll
                    for (int i = 0; i < 16; i++) e[i] = s[i];
                    __builtin_memcpy(&q, e, 16);
                }
            } else if (p < nc) {
                uint8_t e[16];
#pragma unroll
                for (int i = 0; i < 16; i++) e[i] = p + i < nc ? src[p + i] : (uint8_t)0;
                __builtin_memcpy(&q, e, 16);
            }
            *reinterpret_cast<uint4 *>(dst + p) = q;
        } else {
            for (int i = 0; i < 16; i++) {
                const int64_t pos = p + i;
                if (pos >= 0 && pos < nt) dst[pos] = pos < nc ? src[pos] : (uint8_t)0;
            }
        }
    }
}
