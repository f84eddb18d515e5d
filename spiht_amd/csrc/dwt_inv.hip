// The tiled inverse DWT level (gfx950): a workgroup per tile, persistent workgroups that fetch a tile ahead, and level 1 of a
// 3-channel image with the colour model change on its stores, with their launchers (dwt_device.h: the whole picture).
#include "dwt_device.h"

// IW_TH x IW_TW (common.h): output rows / columns per tile.  Level 1 of 256 1080p images, workgroup per tile: 16 rows
// 4.02 ms, 20: 4.05, 24: 4.03, 32: 4.19, 12: 4.22, 40: 4.67, 8: 4.74; persistent kernel beside the list decoder (the
// pipelined schedule): 16 rows 7.3 ms, 20: 7.0, 24: 6.5-6.7, 28: 8.1, 32: 7.6

// ---- the filter of a thread, shared by k_idwt_level and k_idwt_level_pf -------------------------------------------------
// LOM / HIM: non-zero taps of rec_lo / rec_hi (a product with a zero tap adds exactly nothing to `ca*lo + cd*hi`, so it
// is skipped).
// `full` (wave-uniform) false: the caller knows the detail part of the sums to be +0.0 and it is not computed.  That is the
// case for a staged band row whose bit in the tile's row word (common.h: L1Flags) is clear, in a plane whose zeros
// dequantise to +0.0 (zero_ok): the row is +0.0 in the three detail bands, over every staged column, halo included.  An
// accumulator that starts at the literal 0.0 and adds products (+0.0) * tap = +-0.0 stays +0.0, so td, ua and ud are +0.0,
// th = (0.0 + 0.0) + 0.0 is +0.0, and tl = (0.0 + ta) + 0.0 is 0.0 + ta: 0.0 + ta is never -0.0, and y + 0.0 == y in every
// bit for every other y, NaN and the infinities included.  A window of such rows holds th = +0.0 only: sd is +0.0 and the
// output (0.0 + sa) + 0.0 likewise.  So skipping changes no bit, whatever further bits the word has set.
//
// IDWT_ROW: axis -1 synthesis of band row r at the thread's output column (cl: its first contributing staged column; tlo /
// thi: the taps of its parity).  Order of the additions as in pywt's upsampling_convolution_valid_sf: the approximation and
// the detail contribution are separate sums, each over j = 0..F/2-1 (tap 2j+parity against band column i-j, i.e. DEscending
// band column), and the detail sum is added to the finished approximation sum -- the result is then bit-identical to
// pywt.waverec2's.
// (A macro, not a function: through a function's reference parameters the filters of 12 taps and more come out with a quarter
// more registers -- 186 instead of 147 for 14 taps -- and a workgroup fewer per CU.)  In scope: s_b, cl, tlo, thi; F, LOM, HIM.
#define IDWT_ROW(tl, th, r, full)                                                                             \
    double tl, th;                                                                                            \
    {                                                                                                         \
        constexpr uint32_t PAIR_ = 3u; /* taps F-2-2s (even columns) and F-1-2s (odd columns): skip a product when both are zero */ \
        double ta_ = 0.0, td_ = 0.0, ua_ = 0.0, ud_ = 0.0;                                                    \
        if (full) {                                                                                           \
            _Pragma("unroll") for (int j_ = 0; j_ < F / 2; j_++) {                                            \
                const int s_ = F / 2 - 1 - j_;                                                                \
                if (((LOM >> (F - 2 - 2 * s_)) & PAIR_) != 0) {                                               \
                    ta_ += s_b[0][r][cl + s_] * tlo[s_];                                                      \
                    ua_ += s_b[2][r][cl + s_] * tlo[s_];                                                      \
                }                                                                                             \
                if (((HIM >> (F - 2 - 2 * s_)) & PAIR_) != 0) {                                               \
                    td_ += s_b[1][r][cl + s_] * thi[s_];                                                      \
                    ud_ += s_b[3][r][cl + s_] * thi[s_];                                                      \
                }                                                                                             \
            }                                                                                                 \
        } else {                                                                                              \
            _Pragma("unroll") for (int j_ = 0; j_ < F / 2; j_++) {                                            \
                const int s_ = F / 2 - 1 - j_;                                                                \
                if (((LOM >> (F - 2 - 2 * s_)) & PAIR_) != 0) ta_ += s_b[0][r][cl + s_] * tlo[s_];            \
            }                                                                                                 \
        }                                                                                                     \
        tl = (0.0 + ta_) + td_;                                                                               \
        th = (0.0 + ua_) + ud_;                                                                               \
    }
// idwt_col: output row 2kb + mp of a window wl / wh that holds band rows kb..kb+F/2-1 (index F/2-1 = newest); the same order
// along axis -2
template <int F, uint32_t LOM, uint32_t HIM>
__device__ __forceinline__ double idwt_col(const double (&wl)[F / 2], const double (&wh)[F / 2], const double *lo, const double *hi,
                                           int mp, bool full) {
    constexpr int HF = F / 2;
    double sa = 0.0, sd = 0.0;
    if (full) {
#pragma unroll
        for (int j = 0; j < HF; j++) {
            const int s = HF - 1 - j;
            if ((LOM >> (mp + F - 2 - 2 * s)) & 1u) sa += wl[s] * lo[mp + F - 2 - 2 * s];
            if ((HIM >> (mp + F - 2 - 2 * s)) & 1u) sd += wh[s] * hi[mp + F - 2 - 2 * s];
        }
    } else {
#pragma unroll
        for (int j = 0; j < HF; j++) {
            const int s = HF - 1 - j;
            if ((LOM >> (mp + F - 2 - 2 * s)) & 1u) sa += wl[s] * lo[mp + F - 2 - 2 * s];
        }
    }
    return (0.0 + sa) + sd;
}
// The filters up to 10 taps take the two paths.  The longer ones hold their windows and taps in 170 registers with one path and
// spill with two: their row words steer the loads only, and every row is filtered in full.
template <int F> constexpr bool IDWT_ROW_SKIP = F <= 10;
// The rows a thread's half of the tile walks, as a wave-uniform mask with the half's first row at bit 0: a half-tile is two
// whole wavefronts, which the compiler cannot know -- said so, the tests of the bits are scalar.
__device__ __forceinline__ uint32_t half_rows(uint32_t mask, int rbase) { return __builtin_amdgcn_readfirstlane(mask >> rbase); }

// grid: (ceil(out_w/TW), ceil(out_h/TH), planes).
template <int F, uint32_t LOM, uint32_t HIM, int PX = PX_F64>  // PX_U8 / PX_U16: level 1 into an 8- / 16-bit picture (a.px; a.out unused)
__global__ __launch_bounds__(DW_BLOCK) void k_idwt_level(IdwtKArgs a) {
    // band index k contributes to output n with tap t = n + F - 2 - 2k in [0,F):  k in [n/2, n/2 + F/2 - 1]
    constexpr int HF = F / 2;
    constexpr int KH = IW_TH / 2 + HF - 1;   // band rows staged: outputs m0..m0+TH-1 need k in [m0/2, m0/2+TH/2-1+HF-1]
    constexpr int KW = IW_TW / 2 + HF - 1;   // band cols staged
    constexpr int KHH = IW_TH / 4 + HF - 1;  // band rows one half-tile walks
    __shared__ double s_b[4][KH][KW + 1];    // aa, ad, da, dd (dequantised)
    uint32_t tbx, tby, tbz;
    xcd_tile((a.out_w + IW_TW - 1) / IW_TW, (a.out_h + IW_TH - 1) / IW_TH, a.planes, tbx, tby, tbz);
    const int plane = (int)tbz;
    const int k = plane % a.c;
    const int m0 = (int)tby * IW_TH, n0 = (int)tbx * IW_TW;
    const int kh0 = m0 / 2, kw0 = n0 / 2;
    const bool has_m = a.mults != nullptr;
    const double mk = has_m ? a.mults[k] : 1.0;
    const bool zero_ok = (!has_m || mk > 0.0) && a.q > 0.0;  // 0/m/q == +0.0 exactly: skip the divisions
    const int32_t *__restrict__ rec = a.rec + (size_t)plane * a.enc_h * a.enc_w;
    const double *__restrict__ ain = a.first ? nullptr : a.a_in + (size_t)plane * a.a_h * a.a_w;
    const int tid = threadIdx.x;
    // The mask of this tile's staged band rows that may hold a cell of a detail band: its row word; without row words every
    // row when its L1Flags word is set, none when that is still zero.  The detail bands of the other rows are not read (a zero
    // goes through the same arithmetic: same bits) and, where zeros dequantise to +0.0, not filtered either (IDWT_ROW)
    const size_t ti = ((size_t)plane * ((a.out_h + IW_TH - 1) / IW_TH) + tby) * ((a.out_w + IW_TW - 1) / IW_TW) + tbx;
    const uint32_t mask = a.flags == nullptr ? ~0u : a.rows != nullptr ? a.rows[ti] : a.flags[ti] != 0u ? ~0u : 0u;

    for (int p = tid; p < KH * KW; p += DW_BLOCK) {
        const int r = p / KW, cidx = p - r * KW;
        const int bi = kh0 + r, bj = kw0 + cidx;
        double vaa = 0.0, vad = 0.0, vda = 0.0, vdd = 0.0;
        if (bi < a.band_h && bj < a.band_w) {
            const bool occupied = (mask >> r) & 1u;
            const int32_t rad = occupied ? rec[(size_t)bi * a.enc_w + a.off_w + bj] : 0;
            const int32_t rda = occupied ? rec[(size_t)(a.off_h + bi) * a.enc_w + bj] : 0;
            const int32_t rdd = occupied ? rec[(size_t)(a.off_h + bi) * a.enc_w + a.off_w + bj] : 0;
            if (a.first) {
                const int32_t raa = rec[(size_t)bi * a.enc_w + bj];
                vaa = (raa == 0 && zero_ok) ? 0.0 : dequant(raa, mk, a.q, has_m);
            } else {
                vaa = ain[(size_t)bi * a.a_w + bj];
            }
            vad = (rad == 0 && zero_ok) ? 0.0 : dequant(rad, mk, a.q, has_m);
            vda = (rda == 0 && zero_ok) ? 0.0 : dequant(rda, mk, a.q, has_m);
            vdd = (rdd == 0 && zero_ok) ? 0.0 : dequant(rdd, mk, a.q, has_m);
        }
        s_b[0][r][cidx] = vaa; s_b[1][r][cidx] = vad; s_b[2][r][cidx] = vda; s_b[3][r][cidx] = vdd;
    }
    __syncthreads();

    // thread = (output column nn, half): walks the band rows its 16 output rows need
    const int nn = tid & (IW_TW - 1), half = tid / IW_TW;
    const int n = n0 + nn;
    const int np = n & 1;
    const int cl = nn / 2;            // first contributing band column, tile-relative (= n/2 - kw0)
    // taps along axis -1 for this column's parity: s = 0..HF-1  ->  t = np + F - 2 - 2s
    double tlo[HF], thi[HF];
#pragma unroll
    for (int s = 0; s < HF; s++) {
        tlo[s] = a.lo[np + F - 2 - 2 * s];
        thi[s] = a.hi[np + F - 2 - 2 * s];
    }
    double wl[HF], wh[HF];  // register window: tl/th of the last HF band rows (index HF-1 = newest)
#pragma unroll
    for (int s = 0; s < HF; s++) { wl[s] = 0.0; wh[s] = 0.0; }
    double *__restrict__ out = PX ? nullptr : a.out + (size_t)plane * a.out_h * a.out_w;
    uint8_t *__restrict__ out8 = PX ? a.px.out + (int64_t)(plane / a.c) * a.px.sb + (int64_t)(plane % a.c) * a.px.sc : nullptr;
    const int rbase = half * (IW_TH / 4);  // first band row (tile-relative) of this half
    // (a zero that dequantises to -0.0 or NaN: every row in full)
    const uint32_t fm = IDWT_ROW_SKIP<F> ? half_rows(zero_ok ? mask : ~0u, rbase) : ~0u;
#pragma unroll
    for (int rr = 0; rr < KHH; rr++) {
        const int r = rbase + rr;
        IDWT_ROW(tl, th, r, (fm >> rr) & 1u)
#pragma unroll
        for (int s = 0; s < HF - 1; s++) { wl[s] = wl[s + 1]; wh[s] = wh[s + 1]; }
        wl[HF - 1] = tl;
        wh[HF - 1] = th;
        if (rr >= HF - 1) {
            // window holds band rows kb..kb+HF-1 with kb = kh0 + r - (HF-1): output rows 2kb, 2kb+1
            const int m = 2 * (kh0 + r - (HF - 1));
            const bool wfull = ((fm >> (rr - (HF - 1))) & ((1u << HF) - 1u)) != 0u;  // a row of the window holds a cell
#pragma unroll
            for (int mp = 0; mp < 2; mp++) {
                const double sacc = idwt_col<F, LOM, HIM>(wl, wh, a.lo, a.hi, mp, wfull);
                if (PX) {
                    if (m + mp < a.px.h && n < a.px.w) PX_STORE(PX, out8, (int64_t)(m + mp) * a.px.sh + (int64_t)n * a.px.sw, sacc, a.px.kind);
                } else {
                    if (m + mp < a.out_h && n < a.out_w) out[(size_t)(m + mp) * a.out_w + n] = sacc;
                }
            }
        }
    }
}

// ---- the inverse level as persistent workgroups that fetch one tile ahead ---------------------------------------------
// k_idwt_level is a workgroup per tile: request the tile's bands, wait a memory latency, filter, store, exit.  With few
// workgroups resident on a CU -- three when a list decoder lives there too (the pipelined schedule of
// spiht_amd/batch.py) -- a CU has three tiles in flight and the level is bound by that latency, not by bytes: 8.5 instead
// of 4.0 ms for level 1 of 256 1080p images, and not reading the detail bands at all changed nothing.
// Here a workgroup walks a sequence of tiles and requests tile k+1's samples (into registers: 15 per thread) before it
// filters and stores tile k, so the latency of k+1 runs under the work of k.  The barriers are bare s_barrier behind an
// lgkmcnt wait: __syncthreads() would wait for the loads in flight as well.  Same arithmetic in the same order as
// k_idwt_level: bit-identical output.  grid: IWP_WG workgroups per CU at most; tiles dealt XCD-contiguously.
#ifndef IWP_WG
#define IWP_WG 4
#endif

// FLAGS: a.flags holds one word per tile (common.h: L1Flags), a.rows -- if given -- one row word; the detail bands of a tile
// whose word is zero, and with row words those of every staged row whose bit is clear, are all zero: they are not read and,
// where a zero dequantises to +0.0, neither staged nor filtered (IDWT_ROW, idwt_col).  The loads stay unconditional -- a branch around them would make every later wait a wait for
// everything -- and go through a buffer descriptor of the plane instead: an offset beyond it returns 0 without a trip
// to memory.  The word of a tile is fetched when the tile's number becomes known, a tile of work ahead of its use.
// PX_U8 / PX_U16: the output is the strided 8- / 16-bit picture a.px (common.h: PxView); the launcher sees to it that a
// plane's bytes span less than 2^31 (32-bit buffer offsets).
template <int F, uint32_t LOM, uint32_t HIM, bool FIRST, bool FLAGS = false, int PX = PX_F64>  // FIRST: coarsest level, the approximation comes from the packed array
__global__ __launch_bounds__(DW_BLOCK) void k_idwt_level_pf(IdwtKArgs a, uint32_t gx, uint32_t gy, uint32_t *ctr,
                                                                      TileBase cb) {
    static_assert(!(FIRST && FLAGS), "the flags are those of level 1 of a transform with two levels or more");
    constexpr int HF = F / 2;
    constexpr int KH = IW_TH / 2 + HF - 1, KW = IW_TW / 2 + HF - 1, KHH = IW_TH / 4 + HF - 1;
    constexpr int NE = (KH * KW + DW_BLOCK - 1) / DW_BLOCK;  // staged elements per thread
    __shared__ double s_b[4][KH][KW + 1];                    // aa, ad, da, dd (dequantised)
    const int tid = threadIdx.x;
    // this workgroup's tiles: workgroups are dealt round-robin over the 8 XCDs; XCD x owns the contiguous tile range
    // [x*q + min(x, r), ...) and its workgroups (every 8th) take the tiles of that range in turn
    const uint32_t nt = gx * gy * (uint32_t)a.planes;
    const uint32_t x = blockIdx.x & 7u, q = nt >> 3, r8 = nt & 7u;
    const uint32_t base = x * q + (x < r8 ? x : r8), cnt = q + (x < r8 ? 1u : 0u);
    // Which tile next: with a fixed stride (tile k, k + per, ...) the workgroups drift apart over a few hundred tiles,
    // the tiles in flight on an XCD stop being neighbours and the halo rows two tiles share are fetched from HBM twice
    // (PMC: 40 instead of 31.6 MB read per 1080p image).  So the XCD's workgroups draw their tiles from a counter: what
    // is in flight is always one contiguous window of the range, as with one workgroup per tile.  Thread 0 draws a
    // tile two ahead (the answer travels under a whole tile of work) and passes it on through s_next.
    __shared__ uint32_t s_next[2];
    uint32_t *const myctr = ctr + 32u * x;
    const uint32_t cbase = cb.v[x];
    // "on a CU": who waits for this launch to be resident before launching a neighbour (spiht_ctx_wait_resident) counts these
    if (tid == 0) atomicAdd(ctr + TILECTR_STARTED, 1u);
    uint32_t k, kn;  // position in the XCD's range of the tile being worked on / of the one after
    if (tid == 0) {
        s_next[0] = atomicAdd(myctr, 1u) - cbase;
        s_next[1] = atomicAdd(myctr, 1u) - cbase;
    }
    __syncthreads();
    k = __builtin_amdgcn_readfirstlane(s_next[0]);  // (workgroup-uniform; said so, the tile arithmetic stays scalar)
    kn = __builtin_amdgcn_readfirstlane(s_next[1]);
    __syncthreads();

    struct Stage {  // the samples of one tile on their way from memory: 15 registers per thread
        int32_t rad[NE], rda[NE], rdd[NE], raa[NE];
        double vaa[NE];
        double mk;  // the plane's channel scale (a load as well: it must not be waited for on its own)
    };
    // What occupancy() below loaded for a tile -> the mask of its staged detail rows: its row word, or, without row words,
    // every row when its L1Flags word is set.  Made where the mask is used, a tile of work behind the load: made at the load
    // it would wait for it there -- for everything, the stores of the tile before included.
    auto rows_of = [&](uint32_t w) -> uint32_t { return !FLAGS ? ~0u : a.rows != nullptr ? w : w != 0u ? ~0u : 0u; };
    auto request = [&](Stage &g, uint32_t T, uint32_t occw) {  // the loads of tile T (nothing waits for them here)
        const uint32_t occ = rows_of(occw);
        const uint32_t bx = T % gx, t2 = T / gx, by = t2 % gy, plane = t2 / gy;
        const int kh0 = (int)(by * IW_TH) / 2, kw0 = (int)(bx * IW_TW) / 2;
        const int32_t *__restrict__ rec = a.rec + (size_t)plane * a.enc_h * a.enc_w;
        const double *__restrict__ ain = FIRST ? nullptr : a.a_in + (size_t)plane * a.a_h * a.a_w;
        const __amdgpu_buffer_rsrc_t rrsrc = plane_rsrc(rec, (uint32_t)a.enc_h * (uint32_t)a.enc_w * 4u);  // (FLAGS only)
        // unconditional loads from clamped positions (a branch around a load makes the compiler wait for it at the
        // join); what lies outside the band is zeroed when the samples go to LDS
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int p = min(tid + e * DW_BLOCK, KH * KW - 1);
            const int rr = p / KW, cidx = p - rr * KW;
            const int bi = min(kh0 + rr, a.band_h - 1), bj = min(kw0 + cidx, a.band_w - 1);
            if (FLAGS) {
                const uint32_t o_ad = ((uint32_t)bi * (uint32_t)a.enc_w + (uint32_t)(a.off_w + bj)) * 4u;
                const uint32_t o_da = ((uint32_t)(a.off_h + bi) * (uint32_t)a.enc_w + (uint32_t)bj) * 4u;
                const bool rd = __builtin_amdgcn_ubfe(occ, (uint32_t)rr, 1u) != 0u;  // the row's bit in the tile's mask (one v_bfe_u32)
                g.rad[e] = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rd ? o_ad : BUF_OOB, 0, 0);
                g.rda[e] = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rd ? o_da : BUF_OOB, 0, 0);
                g.rdd[e] = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rd ? o_da + (uint32_t)a.off_w * 4u : BUF_OOB, 0, 0);
            } else {
                g.rad[e] = rec[(size_t)bi * a.enc_w + a.off_w + bj];
                g.rda[e] = rec[(size_t)(a.off_h + bi) * a.enc_w + bj];
                g.rdd[e] = rec[(size_t)(a.off_h + bi) * a.enc_w + a.off_w + bj];
            }
            if (FIRST) { g.raa[e] = rec[(size_t)bi * a.enc_w + bj]; g.vaa[e] = 0.0; }
            else { g.vaa[e] = ain[(size_t)bi * a.a_w + bj]; g.raa[e] = 0; }
        }
        g.mk = a.mults != nullptr ? a.mults[plane % (uint32_t)a.c] : 1.0;
    };
    // taps of axis -1 for this thread's column parity (n0 is even: the parity is the same in every tile)
    const int nn = tid & (IW_TW - 1), half = tid / IW_TW, np = nn & 1, cl = nn / 2;
    double tlo[HF], thi[HF];
#pragma unroll
    for (int s2 = 0; s2 < HF; s2++) {
        tlo[s2] = a.lo[np + F - 2 - 2 * s2];
        thi[s2] = a.hi[np + F - 2 - 2 * s2];
    }
    const bool has_m = a.mults != nullptr;
    // one tile: its samples (in g) -> LDS, then g is free and takes the loads of the next tile; filter; store
    auto tile = [&](Stage &g, uint32_t kk, uint32_t knext, uint32_t occw, uint32_t occ_next) {
        const uint32_t T = base + kk;
        const uint32_t bx = T % gx, t2 = T / gx, by = t2 % gy, plane = t2 / gy;
        const int kh0s = (int)(by * IW_TH) / 2, kw0s = (int)(bx * IW_TW) / 2;
        const double mk = g.mk;
        const bool zero_ok = (!has_m || mk > 0.0) && a.q > 0.0;  // 0/m/q == +0.0 exactly: skip the divisions
        // the rows whose detail bands the filter reads: the tile's mask, or all of them where a zero is not +0.0.  The others
        // are not written to LDS either (what an earlier tile left there is never read)
        const uint32_t fmask = !FLAGS || !IDWT_ROW_SKIP<F> || !zero_ok ? ~0u : rows_of(occw);
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int p = tid + e * DW_BLOCK;
            if (p < KH * KW) {
                const int rr = p / KW, cidx = p - rr * KW;
                const bool in = kh0s + rr < a.band_h && kw0s + cidx < a.band_w;
                const double va = FIRST ? ((g.raa[e] == 0 && zero_ok) ? 0.0 : dequant(g.raa[e], mk, a.q, has_m)) : g.vaa[e];
                s_b[0][rr][cidx] = in ? va : 0.0;
                if (!FLAGS || !IDWT_ROW_SKIP<F> || __builtin_amdgcn_ubfe(fmask, (uint32_t)rr, 1u) != 0u) {
                    s_b[1][rr][cidx] = (!in || (g.rad[e] == 0 && zero_ok)) ? 0.0 : dequant(g.rad[e], mk, a.q, has_m);
                    s_b[2][rr][cidx] = (!in || (g.rda[e] == 0 && zero_ok)) ? 0.0 : dequant(g.rda[e], mk, a.q, has_m);
                    s_b[3][rr][cidx] = (!in || (g.rdd[e] == 0 && zero_ok)) ? 0.0 : dequant(g.rdd[e], mk, a.q, has_m);
                }
            }
        }
        // the tile after `knext` is drawn here -- behind the wait for this tile's samples, ahead of the next tile's
        // loads -- and looked at only at the end of the tile (raw: a subtraction here would wait for the answer)
        uint32_t drawn = 0;
        if (tid == 0) drawn = atomicAdd(myctr, 1u);
        request(g, base + min(knext, cnt - 1u), occ_next);  // unconditional (past the end: the last tile again, never used): a
        lds_barrier();                            // branch around loads makes every later wait a wait for all of them
        // ---- thread = (output column nn, half): as k_idwt_level ----
        const int m0 = (int)by * IW_TH, n0 = (int)bx * IW_TW, kh0 = m0 / 2;
        const int n = n0 + nn;
        double wl[HF], wh[HF];
#pragma unroll
        for (int s2 = 0; s2 < HF; s2++) { wl[s2] = 0.0; wh[s2] = 0.0; }
        const int rbase = half * (IW_TH / 4);
        const uint32_t fm = FLAGS && IDWT_ROW_SKIP<F> ? half_rows(fmask, rbase) : ~0u;
        // Stores through a buffer descriptor of the plane: what falls outside the picture (rows past the plane's end by
        // the descriptor's range check, columns past out_w by an offset beyond it) is dropped by the hardware, so the
        // stores stand in straight-line code.  With branches around them the compiler cannot count them, and the wait
        // for the next tile's samples at the top of the loop becomes a wait for these stores as well.
        const uint32_t row_bytes = (uint32_t)a.out_w * 8u;
        const __amdgpu_buffer_rsrc_t orsrc = PX ? plane_rsrc(a.px.out + (int64_t)(plane / (uint32_t)a.c) * a.px.sb + (int64_t)(plane % (uint32_t)a.c) * a.px.sc,
                                                             (uint32_t)((int64_t)(a.px.h - 1) * a.px.sh + (int64_t)(a.px.w - 1) * a.px.sw + (PX == PX_FLT ? a.px.es : PX)))
                                                : plane_rsrc(a.out + (size_t)plane * a.out_h * a.out_w, (uint32_t)a.out_h * row_bytes);
        const uint32_t voff0 = n < a.out_w ? (uint32_t)(2 * (kh0 + rbase)) * row_bytes + (uint32_t)n * 8u : BUF_OOB;
        // (integer pixels) the crop: columns x >= w by an offset beyond the descriptor, rows y >= h by a compare per store
        const int y0 = 2 * (kh0 + rbase);
        const uint32_t voff8 = n < a.px.w ? (uint32_t)y0 * (uint32_t)a.px.sh + (uint32_t)n * (uint32_t)a.px.sw : BUF_OOB;
#pragma unroll
        for (int rr = 0; rr < KHH; rr++) {
            const int r = rbase + rr;
            // (the branches on the mask's bits go around LDS reads and arithmetic only: the stores below stay in the straight line)
            IDWT_ROW(tl, th, r, (fm >> rr) & 1u)
#pragma unroll
            for (int s2 = 0; s2 < HF - 1; s2++) { wl[s2] = wl[s2 + 1]; wh[s2] = wh[s2 + 1]; }
            wl[HF - 1] = tl;
            wh[HF - 1] = th;
            if (rr >= HF - 1) {
                const bool wfull = ((fm >> (rr - (HF - 1))) & ((1u << HF) - 1u)) != 0u;  // a row of the window holds a cell
#pragma unroll
                for (int mp = 0; mp < 2; mp++) {
                    const double sacc = idwt_col<F, LOM, HIM>(wl, wh, a.lo, a.hi, mp, wfull);
                    if constexpr (PX == PX_U8) {
                        const int dy = 2 * (rr - (HF - 1)) + mp;
                        __builtin_amdgcn_raw_buffer_store_b8(px8_store_value(sacc), orsrc,
                                                             y0 + dy < a.px.h ? voff8 + (uint32_t)dy * (uint32_t)a.px.sh : BUF_OOB, 0, 0);
                    } else if constexpr (PX == PX_U16) {
                        const int dy = 2 * (rr - (HF - 1)) + mp;
                        __builtin_amdgcn_raw_buffer_store_b16(px16_store_value(sacc), orsrc,
                                                              y0 + dy < a.px.h ? voff8 + (uint32_t)dy * (uint32_t)a.px.sh : BUF_OOB, 0, 0);
                    } else if constexpr (PX == PX_FLT) {
                        // both widths stand in the straight line, the one the kind does not use at an offset beyond the
                        // descriptor (dropped without a trip to memory): a branch around a store is what the kernel avoids
                        const int dy = 2 * (rr - (HF - 1)) + mp;
                        const uint32_t b = flt_store_value(sacc, a.px.kind);
                        const uint32_t vo = y0 + dy < a.px.h ? voff8 + (uint32_t)dy * (uint32_t)a.px.sh : BUF_OOB;
                        __builtin_amdgcn_raw_buffer_store_b32(b, orsrc, a.px.kind == SPIHT_FLT_F32 ? vo : BUF_OOB, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b16((uint16_t)b, orsrc, a.px.kind == SPIHT_FLT_F32 ? BUF_OOB : vo, 0, 0);
                    } else {
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, sacc), orsrc,
                                                              voff0 + (uint32_t)(2 * (rr - (HF - 1)) + mp) * row_bytes, 0, 0);
                    }
                }
            }
        }
        if (tid == 0) s_next[0] = drawn - cbase;
        lds_barrier();  // every wave has read the tile before the next one is written over it
    };
    // One tile ahead.  (Two ahead -- a second register set, 116 VGPRs -- leaves room for ONE such workgroup per CU beside
    // a decoder instead of two and was slower there: 9.2-10.6 instead of 7.2 ms for level 1.)
    Stage g0;
    if (k >= cnt) return;
    // the row word of position kk of this XCD's range (clamped as the request is), or without row words its L1Flags word: one
    // load per tile either way, not looked at here (rows_of)
    const uint32_t *const mw = FLAGS ? (a.rows != nullptr ? a.rows : a.flags) : nullptr;
    auto occupancy = [&](uint32_t kk) -> uint32_t { return FLAGS ? mw[base + min(kk, cnt - 1u)] : 1u; };
    uint32_t occ = occupancy(k);
    request(g0, base + k, occ);
    uint32_t occ_n = occupancy(kn);
    // The first tile stands outside the loop: inside it the wait for a tile's samples can then be "all but the stores
    // issued since" on every path into the loop head (with the first trip inside, nothing follows the samples' loads on
    // the path from above, and the compiler has to make it a wait for everything -- the stores of the tile before).
    tile(g0, k, kn, occ, occ_n);
    k = kn;
    kn = __builtin_amdgcn_readfirstlane(s_next[0]);  // (s_next[0] is written again only behind the
                                                                         // next tile's first barrier)
    occ = occ_n;
    occ_n = occupancy(kn);
    while (k < cnt) {
        tile(g0, k, kn, occ, occ_n);
        k = kn;
        kn = __builtin_amdgcn_readfirstlane(s_next[0]);
        occ = occ_n;
        occ_n = occupancy(kn);
    }
}

// ---- level 1 of the inverse transform of a 3-channel image with the colour model change on its stores ------------
// k_idwt_level for the three channels of a tile at once (same staging, same sums in the same order), so that the three
// values of an output pixel meet in one thread, which converts them (color3_px: three pow() per pixel) and stores the
// result: the transformed picture in the coded colour model never exists in memory.  Arithmetic-bound, so the tile is
// smaller than k_idwt_level's (IWC_TH rows: 38.6 KB of LDS for the three channels, four workgroups per CU).
#define IWC_TH 8
template <int F, uint32_t LOM, uint32_t HIM, int PX = PX_F64>  // PX_U8 / PX_U16: an 8- / 16-bit picture (a.px; a.out unused)
__global__ __launch_bounds__(DW_BLOCK) void k_idwt1_color(IdwtKArgs a) {
    constexpr int HF = F / 2;
    constexpr int KH = IWC_TH / 2 + HF - 1, KW = IW_TW / 2 + HF - 1, KHH = IWC_TH / 4 + HF - 1;
    __shared__ double s_b[3][4][KH][KW + 1];  // per channel: aa, ad, da, dd (dequantised)
    __shared__ SpowLds s_pw;
    spow_lds_fill(s_pw, threadIdx.x);      // (the barrier after the staging loop below covers it)
    uint32_t tbx, tby, tbz;
    xcd_tile((a.out_w + IW_TW - 1) / IW_TW, (a.out_h + IWC_TH - 1) / IWC_TH, a.planes / 3, tbx, tby, tbz);
    const int img = (int)tbz;
    const int m0 = (int)tby * IWC_TH, n0 = (int)tbx * IW_TW;
    const int kh0 = m0 / 2, kw0 = n0 / 2;
    const bool has_m = a.mults != nullptr;
    const int tid = threadIdx.x;
    const size_t cpl = (size_t)a.enc_h * a.enc_w, apl = (size_t)a.a_h * a.a_w, opl = (size_t)a.out_h * a.out_w;

    for (int p = tid; p < 3 * KH * KW; p += DW_BLOCK) {
        const int ch = p / (KH * KW), q = p - ch * (KH * KW);
        const int r = q / KW, cidx = q - r * KW;
        const int bi = kh0 + r, bj = kw0 + cidx;
        const double mk = has_m ? a.mults[ch] : 1.0;
        const bool zero_ok = (!has_m || mk > 0.0) && a.q > 0.0;  // 0/m/q == +0.0 exactly: skip the divisions
        const int32_t *__restrict__ rec = a.rec + ((size_t)img * 3 + ch) * cpl;
        double vaa = 0.0, vad = 0.0, vda = 0.0, vdd = 0.0;
        if (bi < a.band_h && bj < a.band_w) {
            const int32_t rad = rec[(size_t)bi * a.enc_w + a.off_w + bj];
            const int32_t rda = rec[(size_t)(a.off_h + bi) * a.enc_w + bj];
            const int32_t rdd = rec[(size_t)(a.off_h + bi) * a.enc_w + a.off_w + bj];
            if (a.first) {
                const int32_t raa = rec[(size_t)bi * a.enc_w + bj];
                vaa = (raa == 0 && zero_ok) ? 0.0 : dequant(raa, mk, a.q, has_m);
            } else {
                vaa = a.a_in[((size_t)img * 3 + ch) * apl + (size_t)bi * a.a_w + bj];
            }
            vad = (rad == 0 && zero_ok) ? 0.0 : dequant(rad, mk, a.q, has_m);
            vda = (rda == 0 && zero_ok) ? 0.0 : dequant(rda, mk, a.q, has_m);
            vdd = (rdd == 0 && zero_ok) ? 0.0 : dequant(rdd, mk, a.q, has_m);
        }
        s_b[ch][0][r][cidx] = vaa; s_b[ch][1][r][cidx] = vad; s_b[ch][2][r][cidx] = vda; s_b[ch][3][r][cidx] = vdd;
    }
    __syncthreads();

    const int nn = tid & (IW_TW - 1), half = tid / IW_TW;
    const int n = n0 + nn, np = n & 1, cl = nn / 2;
    double tlo[HF], thi[HF];
#pragma unroll
    for (int s = 0; s < HF; s++) {
        tlo[s] = a.lo[np + F - 2 - 2 * s];
        thi[s] = a.hi[np + F - 2 - 2 * s];
    }
    double wl[3][HF], wh[3][HF];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
#pragma unroll
        for (int s = 0; s < HF; s++) { wl[ch][s] = 0.0; wh[ch][s] = 0.0; }
    double *__restrict__ out = PX ? nullptr : a.out + (size_t)img * 3 * opl;
    uint8_t *__restrict__ out8 = PX ? a.px.out + (int64_t)img * a.px.sb : nullptr;
    const int rbase = half * (IWC_TH / 4);
#pragma unroll
    for (int rr = 0; rr < KHH; rr++) {
        const int r = rbase + rr;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {  // axis -1 synthesis of band row r at output column n (order: k_idwt_level)
            double ta = 0.0, td = 0.0, ua = 0.0, ud = 0.0;
#pragma unroll
            for (int j = 0; j < HF; j++) {
                const int s = HF - 1 - j;
                constexpr uint32_t PAIR = 3u;
                const bool lnz = ((LOM >> (F - 2 - 2 * s)) & PAIR) != 0, hnz = ((HIM >> (F - 2 - 2 * s)) & PAIR) != 0;
                if (lnz) {
                    ta += s_b[ch][0][r][cl + s] * tlo[s];
                    ua += s_b[ch][2][r][cl + s] * tlo[s];
                }
                if (hnz) {
                    td += s_b[ch][1][r][cl + s] * thi[s];
                    ud += s_b[ch][3][r][cl + s] * thi[s];
                }
            }
            const double tl = (0.0 + ta) + td, th = (0.0 + ua) + ud;
#pragma unroll
            for (int s = 0; s < HF - 1; s++) { wl[ch][s] = wl[ch][s + 1]; wh[ch][s] = wh[ch][s + 1]; }
            wl[ch][HF - 1] = tl;
            wh[ch][HF - 1] = th;
        }
        if (rr >= HF - 1) {
            const int m = 2 * (kh0 + r - (HF - 1));
#pragma unroll
            for (int mp = 0; mp < 2; mp++) {
                double px[3];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    double sa = 0.0, sd = 0.0;
#pragma unroll
                    for (int j = 0; j < HF; j++) {
                        const int s = HF - 1 - j;
                        const bool lnz = (LOM >> (mp + F - 2 - 2 * s)) & 1u, hnz = (HIM >> (mp + F - 2 - 2 * s)) & 1u;
                        if (lnz) sa += wl[ch][s] * a.lo[mp + F - 2 - 2 * s];
                        if (hnz) sd += wh[ch][s] * a.hi[mp + F - 2 - 2 * s];
                    }
                    px[ch] = (0.0 + sa) + sd;
                }
                if (PX ? (m + mp < a.px.h && n < a.px.w) : (m + mp < a.out_h && n < a.out_w)) {
                    double w0, w1, w2;
                    color3_px(a.col, s_pw, px[0], px[1], px[2], w0, w1, w2);
                    if (PX) {
                        const int64_t o = (int64_t)(m + mp) * a.px.sh + (int64_t)n * a.px.sw;
                        PX_STORE(PX, out8, o, w0, a.px.kind);
                        PX_STORE(PX, out8, o + a.px.sc, w1, a.px.kind);
                        PX_STORE(PX, out8, o + 2 * a.px.sc, w2, a.px.kind);
                    } else {
                        const size_t o = (size_t)(m + mp) * a.out_w + n;
                        out[o] = w0;
                        out[o + opl] = w1;
                        out[o + 2 * opl] = w2;
                    }
                }
            }
        }
    }
}

// ---- host launchers -----------------------------------------------------------------------------
// the persistent kernel of one pixel kind: coarsest level / with the L1Flags words / without
template <int F, uint32_t LOM, uint32_t HIM, int PX>
static void launch_idwt_pf(IdwtKArgs &a, uint32_t G, uint32_t pad, hipStream_t st, uint32_t gx, uint32_t gy, uint32_t *ctr, const TileBase &cb) {
    if (a.first) hipLaunchKernelGGL((k_idwt_level_pf<F, LOM, HIM, true, false, PX>), dim3(G), dim3(DW_BLOCK), pad, st, a, gx, gy, ctr, cb);
    else if (a.flags && (uint64_t)a.enc_h * a.enc_w * 4u < (1ull << 31))  // (with a.rows or without: one kernel)
        hipLaunchKernelGGL((k_idwt_level_pf<F, LOM, HIM, false, true, PX>), dim3(G), dim3(DW_BLOCK), pad, st, a, gx, gy, ctr, cb);
    else { a.flags = nullptr; a.rows = nullptr; hipLaunchKernelGGL((k_idwt_level_pf<F, LOM, HIM, false, false, PX>), dim3(G), dim3(DW_BLOCK), pad, st, a, gx, gy, ctr, cb); }
}
// a.px.out set: level 1 into an 8- or 16-bit picture (the kernels of the kind a.px.es names; a.out unused)
template <int F, uint32_t LOM, uint32_t HIM>
static int launch_idwt_FM(IdwtKArgs a, int planes, hipStream_t st, TileCtr *tc) {
    a.planes = planes;
    const int px = a.px.out == nullptr ? PX_F64 : px_kind_of(a.px);
    if (a.color) {  // level 1 of a 3-channel image, colour model change on the stores
        uint32_t ntc = (uint32_t)((a.out_w + IW_TW - 1) / IW_TW) * (uint32_t)((a.out_h + IWC_TH - 1) / IWC_TH) * (uint32_t)(planes / 3);
        with_px(px, [&](auto PX) { hipLaunchKernelGGL((k_idwt1_color<F, LOM, HIM, PX>), dim3(ntc), dim3(DW_BLOCK), 0, st, a); });
        return (int)hipGetLastError();
    }
    const uint32_t gx = (uint32_t)((a.out_w + IW_TW - 1) / IW_TW), gy = (uint32_t)((a.out_h + IW_TH - 1) / IW_TH);
    const uint32_t nt = gx * gy * (uint32_t)planes;
    // a level with several tiles per workgroup slot (20 000 tiles and more: at 1080p, level 1 of 10 images): persistent
    // workgroups that fetch a tile ahead
    constexpr uint32_t pf_min = 20000u;
    const int num_cu = tc ? tc->num_cu : 0;
    // (the persistent kernel addresses a plane with 32-bit offsets: float64 planes by their size, the 8- / 16-bit output by
    // the byte span of its strides)
    const bool off32 = px ? (uint64_t)((a.px.h - 1) * a.px.sh + (a.px.w - 1) * a.px.sw) + (uint64_t)a.px.es < (1ull << 31)
                          : (uint64_t)(a.out_h + IW_TH) * a.out_w * 8u < (1ull << 31);
    if (tc && tc->dev && num_cu >= 2 && nt >= pf_min && off32) {  // (>= 8 workgroups: one per tile range at least)
        const int g = tc->wg_per_cu > 0 ? tc->wg_per_cu : IWP_WG;
        const uint32_t G = (uint32_t)(num_cu * g);
        // A caller that asks for g < IWP_WG workgroups per CU wants the rest of the CU for somebody else -- the pipelined
        // schedule's list decoder, whose workgroup finds no registers beside four of these.  The grid is exactly g per CU,
        // but where the workgroups land is the dispatcher's business: a CU that took g + 1 while the decoder's were arriving
        // keeps a decoder workgroup waiting for the whole level (13.9 instead of 9.3 ms).  So the workgroups
        // are made too large for a (g + 1)-th: LDS they do not use (dynamic, behind the kernel's own), just over 1 / (g + 1)
        // of the CU's.  The placement is then the same whoever arrives first -- no timer between the launches.
        uint32_t pad = 0;
        if (g < IWP_WG && tc->lds_per_cu > 0) {
            constexpr int HFk = F / 2;
            constexpr uint32_t own = 4u * (IW_TH / 2 + HFk - 1) * (IW_TW / 2 + HFk) * 8u + 64u;  // s_b + s_next, rounded up
            const uint32_t want = (uint32_t)tc->lds_per_cu / (uint32_t)(g + 1) + 512u;
            if (want > own && want <= 65536u) pad = want - own;
        }
        TileBase cb;
        uint32_t *ctr = tc->dev;
        for (uint32_t x = 0; x < 8; x++) {
            cb.v[x] = tc->base[x];
            // XCD x draws one number per tile of its range and two more per workgroup (the look-ahead past the end)
            tc->base[x] += (nt >> 3) + (x < (nt & 7u) ? 1u : 0u) + 2u * ((G + 7u - x) >> 3);
        }
        tc->started += G;
        with_px(px, [&](auto PX) { launch_idwt_pf<F, LOM, HIM, PX>(a, G, pad, st, gx, gy, ctr, cb); });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {  // the launch did not happen: counters and book-keeping start over together
            (void)hipMemsetAsync(tc->dev, 0, TILECTR_WORDS * sizeof(uint32_t), st);
            for (uint32_t x = 0; x < 8; x++) tc->base[x] = 0;
            tc->started = 0;
        }
        return (int)e;
    }
    with_px(px, [&](auto PX) { hipLaunchKernelGGL((k_idwt_level<F, LOM, HIM, PX>), dim3(nt), dim3(DW_BLOCK), 0, st, a); });
    return (int)hipGetLastError();
}
template <int F, uint32_t LOM, uint32_t HIM>
static int launch_idwt_F(const IdwtKArgs &a, int planes, hipStream_t st, TileCtr *tc) {
    uint32_t lom, him;
    tap_masks(a.lo, a.hi, F, lom, him);
    if (lom == LOM && him == HIM) return launch_idwt_FM<F, LOM, HIM>(a, planes, st, tc);
    return launch_idwt_FM<F, (1u << F) - 1u, (1u << F) - 1u>(a, planes, st, tc);
}

// tc: tile counters of the calling context (nullptr: fixed-stride tile order in the persistent kernel); a->px.out set: level 1
// into an 8- or 16-bit picture
extern "C" int spiht_launch_idwt_level(const IdwtKArgs *a, int planes, hipStream_t st, TileCtr *tc) {
    switch (a->F) {
    case 2: return launch_idwt_F<2, 0x3u, 0x3u>(*a, planes, st, tc);            // haar
    case 6: return launch_idwt_F<6, 0x0Eu, 0x3Eu>(*a, planes, st, tc);          // bior2.2 rec_lo / rec_hi
    case 10: return launch_idwt_F<10, 0x0FEu, 0x3FEu>(*a, planes, st, tc);      // bior4.4
    case 18: return launch_idwt_F<18, 0x3FF8u, 0x3FFFEu>(*a, planes, st, tc);   // bior6.8
    case 4: return launch_idwt_F<4, 0xFu, 0xFu>(*a, planes, st, tc);
    case 8: return launch_idwt_F<8, 0xFFu, 0xFFu>(*a, planes, st, tc);
    case 12: return launch_idwt_F<12, 0xFFFu, 0xFFFu>(*a, planes, st, tc);
    case 14: return launch_idwt_F<14, 0x3FFFu, 0x3FFFu>(*a, planes, st, tc);
    case 16: return launch_idwt_F<16, 0xFFFFu, 0xFFFFu>(*a, planes, st, tc);
    case 20: return launch_idwt_F<20, 0xFFFFFu, 0xFFFFFu>(*a, planes, st, tc);
    default: return -1;
    }
}
