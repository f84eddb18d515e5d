// fastdiv_check.cpp -- the host arithmetic behind the tiled forward transform's launch constants (csrc/common.h: FastDivU,
// fastdivu_make, dwt_narrow_ok), exercised on the CPU under the address and undefined-behaviour sanitizers.  Stand-alone: no
// device call, nothing of the library linked.
//
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Ispiht_amd/csrc tools/fastdiv_check.cpp -o fastdiv_check
//   ./fastdiv_check        (prints the number of divisions compared; exit status 0 when every one agreed)
//
// What is compared with / and %: the multiplier form of tile -> (column, row, plane) in the XCD order of the kernel, and of
// plane -> (image, channel), for EVERY tile index of
//   * the grids of tests/test_gpu_dwt_addressing.py: widths 123 125 251 3 5 7 x heights 19 21 43 3 5 7, filters of 2, 6 and
//     10 taps, every level down to a 1 x 1 approximation or 9 levels, batches 1 2 5 x channels 1 3 4;
//   * the benchmark's seven levels (256 pictures of 3 x 1080 x 1920, 6 taps);
// then every divisor up to 70 000 and a spread of large ones against the edge values of the 32-bit range.
#include <stdint.h>
#include <stdio.h>

#include "common.h"

#define TH 12  // dwt_device.h: DW_TH, DW_TW
#define TW 64

static uint64_t n_cmp = 0, n_bad = 0;

static void cmp(uint32_t n, const FastDivU &f, uint32_t d) {
    n_cmp++;
    if (fastdivu_host(n, f) != n / d) {
        if (n_bad++ < 10) fprintf(stderr, "mismatch: %u / %u = %u, multiplier form %u\n", n, d, n / d, fastdivu_host(n, f));
    }
}

// every tile of a launch: (out_w x out_h outputs, `planes` planes of c channels)
static void grid(int out_w, int out_h, int planes, int c) {
    const uint32_t gx = (uint32_t)((out_w + TW - 1) / TW), gy = (uint32_t)((out_h + TH - 1) / TH);
    const uint32_t nt = gx * gy * (uint32_t)planes;
    const FastDivU dgx = fastdivu_make(gx), dgy = fastdivu_make(gy), dc = fastdivu_make((uint32_t)c);
    const uint32_t q = nt >> 3, r = nt & 7u;
    for (uint32_t L = 0; L < nt; L++) {
        const uint32_t x = L & 7u, j = L >> 3;
        const uint32_t T = x * q + (x < r ? x : r) + j;  // xcd_tile_at / xcd_tile_fd
        cmp(T, dgx, gx);
        const uint32_t t2 = fastdivu_host(T, dgx);
        cmp(t2, dgy, gy);
        const uint32_t bx = T - t2 * gx, bz = fastdivu_host(t2, dgy), by = t2 - bz * gy;
        n_cmp++;
        if (bx != T % gx || by != (T / gx) % gy || bz != (T / gx) / gy || bz >= (uint32_t)planes) {
            if (n_bad++ < 10) fprintf(stderr, "tile %u of grid %u x %u x %d: (%u, %u, %u)\n", T, gx, gy, planes, bx, by, bz);
        }
        cmp(bz, dc, (uint32_t)c);
        const uint32_t img = fastdivu_host(bz, dc), k = bz - img * (uint32_t)c;
        n_cmp++;
        if (img != bz / (uint32_t)c || k != bz % (uint32_t)c) n_bad++;
    }
}

int main() {
    static const int sizes_w[] = {123, 125, 251, 3, 5, 7}, sizes_h[] = {19, 21, 43, 3, 5, 7}, taps[] = {2, 6, 10};
    static const int batches[] = {1, 2, 5}, chans[] = {1, 3, 4};
    for (int F : taps)
        for (int W : sizes_w)
            for (int H : sizes_h)
                for (int B : batches)
                    for (int c : chans) {
                        int h = H, w = W;
                        for (int l = 0; l < 9; l++) {
                            h = (h + F - 1) / 2;
                            w = (w + F - 1) / 2;
                            grid(w, h, B * c, c);
                            if (h == 1 && w == 1) break;
                        }
                    }
    {
        int h = 1080, w = 1920;
        for (int l = 0; l < 7; l++) {
            h = (h + 5) / 2;
            w = (w + 5) / 2;
            grid(w, h, 256 * 3, 3);
        }
    }
    static const uint32_t edge[] = {0u, 1u, 2u, 3u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    auto divisor = [&](uint32_t d) {
        const FastDivU f = fastdivu_make(d);
        for (uint32_t n : edge) cmp(n, f, d);
        for (uint32_t m = 0; m < 4; m++) {  // around multiples of d, low and high
            const uint64_t lo = (uint64_t)d * m, hi = (0xFFFFFFFFull / d) * d - (uint64_t)d * m;
            for (int e = -1; e <= 1; e++) {
                if ((int64_t)lo + e >= 0 && lo + e <= 0xFFFFFFFFull) cmp((uint32_t)(lo + e), f, d);
                if ((int64_t)hi + e >= 0 && hi + e <= 0xFFFFFFFFull) cmp((uint32_t)(hi + e), f, d);
            }
        }
        uint32_t s = d * 2654435761u + 12345u;  // and a few scattered values
        for (int i = 0; i < 16; i++) {
            s = s * 1664525u + 1013904223u;
            cmp(s, f, d);
        }
    };
    for (uint32_t d = 1; d <= 70000u; d++) divisor(d);
    for (uint32_t sh = 17; sh < 32; sh++)
        for (int e = -2; e <= 2; e++) divisor((1u << sh) + (uint32_t)e);
    divisor(0xFFFFFFFFu);
    divisor(0xFFFFFFFEu);
    // the launcher's choice of addressing at its limits (2^30 bytes a plane)
    const int64_t G = (int64_t)1 << 30;
    int ok = 1;
    ok &= dwt_narrow_ok(1080, 1920, 542, 962, 1111, 1949, 0, 0, 0) ? 1 : 0;
    ok &= dwt_narrow_ok(11585, 11585, 8, 8, 16, 16, 0, 0, 0) ? 1 : 0;
    ok &= dwt_narrow_ok(11586, 11586, 8, 8, 16, 16, 0, 0, 0) ? 0 : 1;
    ok &= dwt_narrow_ok(G - 1, G - 1, G - 1, G - 1, G - 1, G - 1, 2, G - 1, G - 1) ? 0 : 1;  // (no overflow on the way to "no")
    printf("%llu divisions compared, %llu differ; addressing limits %s\n", (unsigned long long)n_cmp, (unsigned long long)n_bad,
           ok ? "ok" : "WRONG");
    return (n_bad == 0 && ok) ? 0 : 1;
}
