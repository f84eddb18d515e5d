// The tiled forward DWT level (gfx950): narrow and wide addressing, the overhang, the single-precision level and level 1 of a
// 3-channel image with the colour model change on its loads, with their launchers (dwt_device.h: the whole picture).
#include "dwt_device.h"

// ---- the tiled forward level ---------------------------------------------------------------------------------------
// Tile -> (bx, by, plane) of k_dwt_level in the XCD order of xcd_tile_at, with the launcher's multipliers instead of the
// two divisions (DwtKArgs::dv_gx, dv_gy: exact for every 32-bit tile index, so the same coordinates for every grid).
__device__ __forceinline__ void xcd_tile_fd(uint32_t L, const DwtKArgs &a, uint32_t &bx, uint32_t &by, uint32_t &bz) {
    const uint32_t q = a.nt >> 3, r = a.nt & 7u, x = L & 7u, j = L >> 3;
    const uint32_t T = x * q + (x < r ? x : r) + j;
    const uint32_t t2 = fdivu(T, a.dv_gx);
    bx = T - t2 * a.gx;
    bz = fdivu(t2, a.dv_gy);
    by = t2 - bz * a.gy;
}
#define OOB_ROW BUF_OOB      // row offset of a row of zeros (zero padding) ...
#define OOB_COL 0x40000000u  // ... column offset of a column of zeros: with planes under 2^30 bytes (dwt_narrow_ok) the sum
                             // of a row and a column offset is past the plane's end as soon as one of the two is a mark,
                             // and the load returns zero

// grid: (ceil(out_w/TW), ceil(out_h/TH), planes).  LOM / HIM: bit j set = tap j of dec_lo / dec_hi is non-zero;
// a zero tap contributes exactly nothing (0*x added to the running sum), so skipping it changes no bit and
// removes a third (bior2.2) to a fifth of the float64 arithmetic.
// One tile of k_dwt_level.
// PX != PX_F64: the level's input is the strided 8- or 16-bit picture a.px (common.h: PxView), converted on the loads;
// PX_FLT: the strided float32 / float16 / bfloat16 picture of kind a.px.kind, widened on the loads (nothing scaled).
// WIDE == false (the launcher's choice, dwt_narrow_ok: every plane under 2^30 bytes): the input plane, the packed array's
// plane and the approximation's plane are addressed through buffer descriptors with 32-bit byte offsets -- a load is one LDS
// word (the row's offset) + the lane's column offset, a store is an offset advanced by a launch-time constant, and rows and
// columns outside the level fall to the descriptors' range check.  WIDE == true: 64-bit addresses formed per access, for
// planes of any size.
template <int F, uint32_t LOM, uint32_t HIM, int PS, int NR, int PX = PX_F64, bool WIDE = false>
__device__ __forceinline__ void dwt_tile(const DwtKArgs &a, double (&s_lo)[2][PS], double (&s_hi)[2][PS], uint32_t tbx, uint32_t tby,
                                         uint32_t tbz) {
    constexpr int NC = 2 * DW_TW + F - 2;  // input columns needed by the tile
    constexpr int HC = (NC + 1) / 2;       // columns per parity plane
    static_assert(NC <= DWF_BLOCK, "one thread per input column");
    static_assert(NR == 2 * DW_TH + F - 2, "input rows needed");
    static_assert(DW_TH <= 64, "dwt_narrow_ok allows for 64 rows below the level's last");
    constexpr int RS = HC + 1;
    constexpr int NRP = (NR + 3) & ~3;     // row offsets in LDS, read four at a time
    const uint32_t plane = tbz;
    const uint32_t img = fdivu(plane, a.dv_c), k = plane - img * (uint32_t)a.c;
    const int oh0 = (int)tby * DW_TH, ow0 = (int)tbx * DW_TW;
    const int tid = threadIdx.x;

    // input row needed for output row o, tap j: 2*o + 1 - j ; first needed row r0 = 2*oh0 + 1 - (F-1)
    const int r0 = 2 * oh0 + 2 - F, c0 = 2 * ow0 + 2 - F;
    // the rows' offsets, worked out once per tile by NR threads.  Narrow: bytes from the plane's start (OOB_ROW: a row of
    // zeros); wide: elements / bytes as 64-bit numbers (-1: a row of zeros)
    __shared__ __attribute__((aligned(16))) uint32_t s_off[WIDE ? 4 : NRP];
    __shared__ long long s_off64[WIDE ? NR : 1];
    if (tid < NR) {
        const int gr = ext_index(r0 + tid, a.in_h, a.mode);
        if constexpr (WIDE) s_off64[tid] = gr < 0 ? -1ll : (long long)gr * (PX ? a.px.sh : (long long)a.in_w);
        else s_off[tid] = gr < 0 ? OOB_ROW : (uint32_t)gr * a.in_rb;
    }
    __shared__ uint32_t s_amax;
    if (tid == 0) s_amax = 0;
    __syncthreads();

    // ---- axis -2: thread <-> input column; all loads first, then the filter ----
    // The columns beyond the last full wavefront (NC - 128 = F - 2 of them) would have a wavefront issue the whole phase for a
    // few live lanes.  Where they fit (DWF_STRAY), that wavefront instead spreads them over its lanes as (column, output row)
    // items: an item loads its own F rows and adds the same taps in the same ascending order -- the same bits.
    constexpr int NFULL = NC / 64 * 64, NS = NC - NFULL;
    constexpr bool STRAY = DWF_STRAY && !WIDE && NS > 0 && NS * DW_TH <= 64;
    if constexpr (STRAY) {
        const int it = tid - NFULL;
        if (it >= 0 && it < NS * DW_TH) {
            const int o = it / NS, sc = NFULL + it % NS;
            const int gc = ext_index(c0 + sc, a.in_w, a.mode);
            const uint8_t *pb = PX ? a.px.in + (int64_t)img * a.px.sb + (int64_t)k * a.px.sc
                                   : reinterpret_cast<const uint8_t *>(a.in) + (uint64_t)plane * a.in_pb;
            const __amdgpu_buffer_rsrc_t rs_in = plane_rsrc(pb, a.in_pb);
            const uint32_t cb = gc < 0 ? OOB_COL : (uint32_t)gc * (PX ? a.in_cb : 8u);
            double x[F];
            if constexpr (PX != PX_F64) {
                uint32_t raw[F];
                if (PX == PX_FLT && a.px.kind == SPIHT_FLT_F32) {  // (the kind is uniform over the launch: one branch around the item's loads)
#pragma unroll
                    for (int t = 0; t < F; t++) raw[t] = __builtin_amdgcn_raw_buffer_load_b32(rs_in, s_off[2 * o + t] + cb, 0, 0);
                } else {
#pragma unroll
                    for (int t = 0; t < F; t++) {
                        if constexpr (PX == PX_U8) raw[t] = __builtin_amdgcn_raw_buffer_load_b8(rs_in, s_off[2 * o + t] + cb, 0, 0);
                        else raw[t] = __builtin_amdgcn_raw_buffer_load_b16(rs_in, s_off[2 * o + t] + cb, 0, 0);
                    }
                }
#pragma unroll
                for (int t = 0; t < F; t++) x[t] = px_value<PX>(raw[t], a.px.kind);
            } else {
#pragma unroll
                for (int t = 0; t < F; t++)
                    x[t] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs_in, s_off[2 * o + t] + cb, 0, 0));
            }
            double sl = 0.0, shh = 0.0;
#pragma unroll
            for (int j = 0; j < F; j++) {
                if ((LOM >> j) & 1u) sl += a.lo[j] * x[F - 1 - j];
                if ((HIM >> j) & 1u) shh += a.hi[j] * x[F - 1 - j];
            }
            s_lo[sc & 1][o * RS + (sc >> 1)] = sl;
            s_hi[sc & 1][o * RS + (sc >> 1)] = shh;
        }
    }
    if (tid < (STRAY ? NFULL : NC)) {
        const int gc = ext_index(c0 + tid, a.in_w, a.mode);
        double x[NR];
        // Nothing of the address arithmetic on the scalar unit: a list-coding workgroup on the same CU keeps that unit busy
        // (its sequencer wavefront issues a dependent scalar instruction whenever it can, and it is the older wavefront),
        // and 28 rows x a dozen scalar instructions per tile were what this kernel lost beside it (DESIGN.md 6, round 3:
        // one scalar-busy wavefront per CU and nothing else cost this kernel 68 %).  The row offsets come out of LDS
        // through an index the compiler cannot prove uniform, so that they stay in vector registers.
        int lz = 0;
        asm volatile("" : "+v"(lz));
        if constexpr (!WIDE) {
            // the plane's base in 64 bits once (from the tile coordinates in vector registers, read back as scalars into the
            // descriptor); per row one add of two 32-bit offsets.  Zero padding needs no case of its own: a marked row or
            // column is out of the descriptor's range and loads as 0, which is 0.0 (and the pixel 0 / 255 = 0.0).
            const uint8_t *pb = PX ? a.px.in + (int64_t)img * a.px.sb + (int64_t)k * a.px.sc
                                   : reinterpret_cast<const uint8_t *>(a.in) + (uint64_t)plane * a.in_pb;
            const __amdgpu_buffer_rsrc_t rs_in = plane_rsrc(pb, a.in_pb);
            const uint32_t cb = gc < 0 ? OOB_COL : (uint32_t)gc * (PX ? a.in_cb : 8u);
            const uint4 *so = reinterpret_cast<const uint4 *>(s_off) + lz;
            if constexpr (PX != PX_F64) {  // byte / 16-bit loads, ALL of them first (converted one by one behind its load, the
                                           // compiler waited for each load before it issued the next: level 1 took 7.1
                                           // instead of 4.3 ms), then k -> k / 255.0 (k / 65535.0)
                uint32_t raw[NRP];
                if (PX == PX_FLT && a.px.kind == SPIHT_FLT_F32) {  // a float kind: the same order -- every load, then the widening.
                                                                   // The kind is uniform over the launch, so the one branch stands
                                                                   // around all of a thread's loads, not between them
#pragma unroll
                    for (int q = 0; q < NRP / 4; q++) {
                        const uint4 o4 = so[q];
                        const uint32_t o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            if (4 * q + e >= NR) continue;
                            raw[4 * q + e] = __builtin_amdgcn_raw_buffer_load_b32(rs_in, o[e] + cb, 0, 0);
                        }
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < NRP / 4; q++) {
                        const uint4 o4 = so[q];
                        const uint32_t o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            if (4 * q + e >= NR) continue;
                            if constexpr (PX == PX_U8) raw[4 * q + e] = __builtin_amdgcn_raw_buffer_load_b8(rs_in, o[e] + cb, 0, 0);
                            else raw[4 * q + e] = __builtin_amdgcn_raw_buffer_load_b16(rs_in, o[e] + cb, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < NR; r++) x[r] = px_value<PX>(raw[r], a.px.kind);
            } else {
#pragma unroll
                for (int q = 0; q < NRP / 4; q++) {
                    const uint4 o4 = so[q];
                    const uint32_t o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if (4 * q + e >= NR) continue;
                        x[4 * q + e] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs_in, o[e] + cb, 0, 0));
                    }
                }
            }
        } else {
            const double *__restrict__ in = PX ? nullptr : a.in + (size_t)plane * a.in_h * a.in_w;
            const uint8_t *__restrict__ in8 = PX ? a.px.in + (int64_t)img * a.px.sb + (int64_t)k * a.px.sc : nullptr;
            if (PX) {
                const long long co8 = gc < 0 ? 0 : (long long)gc * a.px.sw;
                uint32_t raw[NR];
                static_assert(NR <= 64, "one bit per row");
                uint64_t okm = 0;  // bit r: row r is inside the picture (zero padding: a zero sample otherwise)
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const long long off = s_off64[r + lz];
                    const bool ok = a.mode != 3 || (gc >= 0 && off >= 0);
                    okm |= (ok ? 1ull : 0ull) << r;
                    raw[r] = px_load<PX>(in8 + (ok ? off + co8 : 0), a.px.kind);
                }
#pragma unroll
                for (int r = 0; r < NR; r++) x[r] = ((okm >> r) & 1ull) ? px_value<PX>(raw[r], a.px.kind) : 0.0;
            } else if (a.mode != 3) {  // not zero padding: every index is inside the picture
#pragma unroll
                for (int r = 0; r < NR; r++) x[r] = in[s_off64[r + lz] + gc];
            } else {
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const long long off = s_off64[r + lz];
                    const bool ok = gc >= 0 && off >= 0;
                    const double v = in[ok ? off + gc : 0];
                    x[r] = ok ? v : 0.0;
                }
            }
        }
        const int par = tid & 1, hc = tid >> 1;
#pragma unroll
        for (int o = 0; o < DW_TH; o++) {
            // out[o] = sum_j f[j] * x~[2(oh0+o)+1-j];  x~[2(oh0+o)+1-j] = x[2o + F-1-j]
            double sl = 0.0, shh = 0.0;
#pragma unroll
            for (int j = 0; j < F; j++) {
                if ((LOM >> j) & 1u) sl += a.lo[j] * x[2 * o + F - 1 - j];
                if ((HIM >> j) & 1u) shh += a.hi[j] * x[2 * o + F - 1 - j];
            }
            s_lo[par][o * RS + hc] = sl;
            s_hi[par][o * RS + hc] = shh;
        }
    }
    __syncthreads();

    // ---- axis -1 from LDS; 4 sub-bands per output position ----
    const bool has_m = a.mults != nullptr;
    const double mk = has_m ? a.mults[k] : 1.0;
    uint32_t amax = 0;
    constexpr int NU = (DW_TH * DW_TW + DWF_BLOCK - 1) / DWF_BLOCK;  // output positions per thread
    if constexpr (!WIDE) {
        // A thread's outputs lie in one column, DWF_BLOCK / DW_TW rows apart: the offset of the first is worked out once (the
        // same offset serves the top and the bottom bands: their descriptors start off_h rows apart, and the 'ad' / 'dd'
        // column offset is the instruction's scalar offset), the others follow by a constant.  The descriptors end with the
        // level's last row, so a tile's rows below it are dropped by the range check; a thread right of the last column
        // starts from the out-of-range mark and stays out of range.
        static_assert(DWF_BLOCK % DW_TW == 0 && (DW_TH * DW_TW) % DWF_BLOCK == 0, "a thread keeps its column; whole steps");
        constexpr int RSTEP = DWF_BLOCK / DW_TW;
        const int o0 = tid / DW_TW, wcol = tid % DW_TW;
        const int oh = oh0 + o0, ow = ow0 + wcol;
        const bool colok = ow < a.out_w;
        uint32_t vco = colok ? (uint32_t)oh * a.co_rb + (uint32_t)ow * 4u : BUF_OOB;
        uint32_t vll = colok ? (uint32_t)oh * a.ll_rb + (uint32_t)ow * 8u : BUF_OOB;
        uint8_t *cob = reinterpret_cast<uint8_t *>(a.coeffs) + (uint64_t)plane * a.co_pb;
        const uint32_t band_bytes = (uint32_t)a.out_h * a.co_rb;
        const __amdgpu_buffer_rsrc_t rs_top = plane_rsrc(cob, band_bytes);
        const __amdgpu_buffer_rsrc_t rs_bot = plane_rsrc(cob + (uint64_t)(uint32_t)a.off_h * a.co_rb, band_bytes);
        const __amdgpu_buffer_rsrc_t rs_ll =
            plane_rsrc(reinterpret_cast<uint8_t *>(a.ll_out) + (uint64_t)plane * a.ll_pb, a.last ? 0u : (uint32_t)a.out_h * a.ll_rb);
        const uint32_t so_w = (uint32_t)a.off_w * 4u;
        // the few outputs of the bottom / right overhang whose sum depends on PyWavelets' tap order are computed again
        // by k_dwt_edge, which overwrites them and accounts for their magnitude (ov_h <= out_h, ov_w <= out_w: an output
        // counted here is inside the level)
        const int mine_rows = ow < a.ov_w ? a.ov_h - oh : 0;  // output u is this kernel's to account for: u * RSTEP < mine_rows
#pragma unroll
        for (int u = 0; u < NU; u++) {
            const int o = o0 + u * RSTEP;
            // x~ index 2*ow+1-j  ->  tile column 2*wcol + F-1-j  ->  parity (F-1-j)&1, half-column wcol + (F-1-j)/2
            double aa = 0.0, ad = 0.0, da = 0.0, dd = 0.0;
#pragma unroll
            for (int j = 0; j < F; j++) {
                const double vl = s_lo[(F - 1 - j) & 1][o * RS + wcol + ((F - 1 - j) >> 1)];
                const double vh = s_hi[(F - 1 - j) & 1][o * RS + wcol + ((F - 1 - j) >> 1)];
                if ((LOM >> j) & 1u) { aa += a.lo[j] * vl; da += a.lo[j] * vh; }
                if ((HIM >> j) & 1u) { ad += a.hi[j] * vl; dd += a.hi[j] * vh; }
            }
            // (the channel scale is multiplied in whether there is one or not: without one mk is 1.0 and 1.0 * v is v in every
            // bit -- the product was computed either way, and picking between v and mk * v cost two selects a value)
            const int32_t qad = quant(ad, mk, a.q, true), qda = quant(da, mk, a.q, true), qdd = quant(dd, mk, a.q, true);
            uint32_t m = max(iabs_u(qad), max(iabs_u(qda), iabs_u(qdd)));
            if (a.last) {
                const int32_t qaa = quant(aa, mk, a.q, true);
                __builtin_amdgcn_raw_buffer_store_b32((uint32_t)qaa, rs_top, vco, 0, 0);
                m = max(m, iabs_u(qaa));
            } else {
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, aa), rs_ll, vll, 0, 0);
            }
            __builtin_amdgcn_raw_buffer_store_b32((uint32_t)qad, rs_top, vco, so_w, 0);  // 'ad' top-right
            __builtin_amdgcn_raw_buffer_store_b32((uint32_t)qda, rs_bot, vco, 0, 0);     // 'da' bottom-left
            __builtin_amdgcn_raw_buffer_store_b32((uint32_t)qdd, rs_bot, vco, so_w, 0);  // 'dd' bottom-right
            amax = max(amax, u * RSTEP < mine_rows ? m : 0u);
            vco += (uint32_t)RSTEP * a.co_rb;
            vll += (uint32_t)RSTEP * a.ll_rb;
        }
    } else {
        int32_t *__restrict__ co = a.coeffs + (size_t)plane * a.enc_h * a.enc_w;
        double *__restrict__ llo = a.last ? nullptr : a.ll_out + (size_t)plane * a.out_h * a.out_w;
#pragma unroll
        for (int u = 0; u < NU; u++) {
            const int p = tid + u * DWF_BLOCK;
            const int o = p / DW_TW, wcol = p % DW_TW;
            const int oh = oh0 + o, ow = ow0 + wcol;
            if (o >= DW_TH || oh >= a.out_h || ow >= a.out_w) continue;
            double aa = 0.0, ad = 0.0, da = 0.0, dd = 0.0;
#pragma unroll
            for (int j = 0; j < F; j++) {
                const double vl = s_lo[(F - 1 - j) & 1][o * RS + wcol + ((F - 1 - j) >> 1)];
                const double vh = s_hi[(F - 1 - j) & 1][o * RS + wcol + ((F - 1 - j) >> 1)];
                if ((LOM >> j) & 1u) { aa += a.lo[j] * vl; da += a.lo[j] * vh; }
                if ((HIM >> j) & 1u) { ad += a.hi[j] * vl; dd += a.hi[j] * vh; }
            }
            const int32_t qad = quant(ad, mk, a.q, has_m), qda = quant(da, mk, a.q, has_m), qdd = quant(dd, mk, a.q, has_m);
            const bool mine = oh < a.ov_h && ow < a.ov_w;
            if (a.last) {
                const int32_t qaa = quant(aa, mk, a.q, has_m);
                co[(size_t)oh * a.enc_w + ow] = qaa;
                if (mine) amax = max(amax, iabs_u(qaa));
            } else {
                llo[(size_t)oh * a.out_w + ow] = aa;
            }
            co[(size_t)oh * a.enc_w + a.off_w + ow] = qad;                 // 'ad' top-right
            co[(size_t)(a.off_h + oh) * a.enc_w + ow] = qda;               // 'da' bottom-left
            co[(size_t)(a.off_h + oh) * a.enc_w + a.off_w + ow] = qdd;     // 'dd' bottom-right
            if (mine) amax = max(amax, max(iabs_u(qad), max(iabs_u(qda), iabs_u(qdd))));
        }
    }
    if (a.maxabs != nullptr) {
        block_raise_max(&a.maxabs[img], amax, &s_amax);
    }
}

// PX_U8 / PX_U16: level 1 of an 8- / 16-bit picture (a.px; a.in unused).  WIDE: see dwt_tile
template <int F, uint32_t LOM, uint32_t HIM, int PX = PX_F64, bool WIDE = false>
__global__ __launch_bounds__(DWF_BLOCK) void k_dwt_level(DwtKArgs a) {
    constexpr int NC = 2 * DW_TW + F - 2, NR = 2 * DW_TH + F - 2, HC = (NC + 1) / 2;
    // two column-parity planes; the padding makes the plane stride an odd multiple of 16 banks, so the even and odd
    // lanes of one ds_write_b64 lane group land on different banks
    constexpr int RS = HC + 1, PS = DW_TH * RS + (24 - (DW_TH * RS) % 16) % 16;  // PS % 16 == 8
    __shared__ double s_lo[2][PS];
    __shared__ double s_hi[2][PS];
    uint32_t tbx, tby, tbz;
    // the tile's coordinates worked out in vector registers (every lane the same values): they and everything that follows
    // from them -- plane, origin, the base pointers -- then cost the scalar unit nothing (see dwt_tile)
    uint32_t lin = blockIdx.x;
    asm volatile("" : "+v"(lin));
    xcd_tile_fd(lin, a, tbx, tby, tbz);
    dwt_tile<F, LOM, HIM, PS, NR, PX, WIDE>(a, s_lo, s_hi, tbx, tby, tbz);
}

// ---- the bottom / right overhang of a float64 level, in PyWavelets' summation order -----------------------------
// pywt's downsampling_convolution adds the taps in ascending order -- except for the outputs that hang over the end
// of the input (jb = 2o+1-N >= 0, the last F/2 or so output rows and columns of a level): there the taps that read the
// signal extension come first, nearest first (tap jb down to 0), then the others ascending.  The sums differ in the
// last bits, and on 8-bit pictures with flat areas (coefficient x q exactly an integer) the truncating quantiser turns
// that into +-1 (tests/golden/blocky_pywt.npz).  k_dwt_level keeps its compile-time ascending order everywhere (the
// overhang code inside it -- as a block-uniform branch, a second instantiation for the edge tiles, one launch or two,
// a side stream -- cost the level 5 to 12 %: measured); this kernel then recomputes just the outputs whose order
// matters (ov_h / ov_w: the last row and column of a bior level), one thread each, straight from global memory, and
// overwrites them.  grid: (ceil(outputs / 256), planes).
template <int F, int PX = PX_F64>  // PX_U8 / PX_U16: level 1 of an 8- / 16-bit picture (a.px)
__global__ __launch_bounds__(256) void k_dwt_edge(DwtKArgs a) {
    __shared__ double s_f[2][F];  // taps, indexed at run time below
    if (threadIdx.x < F) { s_f[0][threadIdx.x] = a.lo[threadIdx.x]; s_f[1][threadIdx.x] = a.hi[threadIdx.x]; }
    __shared__ uint32_t s_amax;
    if (threadIdx.x == 0) s_amax = 0;
    __syncthreads();
    const int nr = a.out_h - a.ov_h, nc = a.out_w - a.ov_w;        // overhang rows / columns
    const int nA = nr * a.out_w, total = nA + a.ov_h * nc;          // all columns of those rows + the rest of those columns
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int plane = blockIdx.y;
    uint32_t amax = 0;
    if (t < total) {
        int oh, ow;
        if (t < nA) { oh = a.ov_h + t / a.out_w; ow = t % a.out_w; }
        else { const int u = t - nA; oh = u / nc; ow = a.ov_w + u % nc; }
        const double *__restrict__ in = PX ? nullptr : a.in + (size_t)plane * a.in_h * a.in_w;
        const uint8_t *__restrict__ in8 = PX ? a.px.in + (int64_t)(plane / a.c) * a.px.sb + (int64_t)(plane % a.c) * a.px.sc : nullptr;
        const int ir = 2 * oh + 1, ic = 2 * ow + 1;
        const int jbr = oh >= a.ov_h ? ir - a.in_h : -1, jbc = ow >= a.ov_w ? ic - a.in_w : -1;
        int gr[F];
#pragma unroll
        for (int r = 0; r < F; r++) gr[r] = ext_index(ir - r, a.in_h, a.mode);
        // Column by column in the order axis -1 asks for; per column the F samples are loaded first (independent loads),
        // then added in the order the row asks for -- a sample is picked by comparing indices, registers cannot be
        // indexed at run time.  (One load at a time, as a plain double loop does it, this kernel took 0.26 ms at
        // 256 x 1080p, 7 % of the level.)
        double aa = 0.0, ad = 0.0, da = 0.0, dd = 0.0;
#pragma unroll F <= 6 ? F : 1
        for (int s1 = 0; s1 < F; s1++) {
            const int j = s1 <= jbc ? jbc - s1 : s1;
            const int gc = ext_index(ic - j, a.in_w, a.mode);
            double xv[F];
#pragma unroll
            for (int r = 0; r < F; r++) {
                if (PX) xv[r] = (gc < 0 || gr[r] < 0) ? 0.0 : px_value<PX>(px_load<PX>(in8 + ((int64_t)gr[r] * a.px.sh + (int64_t)gc * a.px.sw), a.px.kind), a.px.kind);
                else xv[r] = (gc < 0 || gr[r] < 0) ? 0.0 : in[(size_t)gr[r] * a.in_w + gc];
            }
            double tl = 0.0, th = 0.0;
#pragma unroll
            for (int s2 = 0; s2 < F; s2++) {
                const int j2 = s2 <= jbr ? jbr - s2 : s2;
                double v = xv[0];
#pragma unroll
                for (int r = 1; r < F; r++) v = (j2 == r) ? xv[r] : v;
                tl += s_f[0][j2] * v;
                th += s_f[1][j2] * v;
            }
            aa += s_f[0][j] * tl; da += s_f[0][j] * th;
            ad += s_f[1][j] * tl; dd += s_f[1][j] * th;
        }
        const int k = plane % a.c;
        const bool has_m = a.mults != nullptr;
        const double mk = has_m ? a.mults[k] : 1.0;
        int32_t *__restrict__ co = a.coeffs + (size_t)plane * a.enc_h * a.enc_w;
        const int32_t qad = quant(ad, mk, a.q, has_m), qda = quant(da, mk, a.q, has_m), qdd = quant(dd, mk, a.q, has_m);
        if (a.last) {
            const int32_t qaa = quant(aa, mk, a.q, has_m);
            co[(size_t)oh * a.enc_w + ow] = qaa;
            amax = iabs_u(qaa);
        } else {
            a.ll_out[(size_t)plane * a.out_h * a.out_w + (size_t)oh * a.out_w + ow] = aa;
        }
        co[(size_t)oh * a.enc_w + a.off_w + ow] = qad;
        co[(size_t)(a.off_h + oh) * a.enc_w + ow] = qda;
        co[(size_t)(a.off_h + oh) * a.enc_w + a.off_w + ow] = qdd;
        amax = max(amax, max(iabs_u(qad), max(iabs_u(qda), iabs_u(qdd))));
    }
    if (a.maxabs != nullptr) {
        block_raise_max(&a.maxabs[plane / a.c], amax, &s_amax);
    }
}

// ---- single-precision forward level ------------------------------------------------------------------------------
// PyWavelets transforms float32 (and float16) pixels in float32 with float copies of the filters, and the wrapper
// quantises the float32 array in float32 (in float64 once per-channel scales are applied).  In float32 the order of
// the additions decides quantised coefficients, so this kernel follows pywt's (convolution.template.c,
// downsampling_convolution): ascending taps, except for outputs that hang over the right / bottom end (2o+1 >= N),
// where the taps reading the extension come first, nearest first (tap index 2o+1-N down to 0), then the rest
// ascending.  Same tiling as k_dwt_level; the overhang outputs (the last (F-1)/2 rows and columns of a level) take
// a slower path with run-time tap order.  Level inputs shorter than the filter are refused by the host (pywt runs
// yet another loop for them).  (quant_f32: dwt_device.h)
template <int F, uint32_t LOM, uint32_t HIM>
__global__ __launch_bounds__(DW_BLOCK) void k_dwt_level_f32(DwtKArgs a) {
    constexpr int NC = 2 * DW_TW + F - 2, NR = 2 * DW32_TH + F - 2, HC = (NC + 1) / 2;
    static_assert(NC <= DW_BLOCK, "one thread per input column");
    constexpr int RS = HC + 1, PS = DW32_TH * RS + 8;
    __shared__ float s_lo[2][PS];
    __shared__ float s_hi[2][PS];
    __shared__ int s_row[NR];
    __shared__ float s_flo[F], s_fhi[F];  // float copies of the filters, for the run-time-ordered overhang sums
    uint32_t tbx, tby, tbz;
    xcd_tile((a.out_w + DW_TW - 1) / DW_TW, (a.out_h + DW32_TH - 1) / DW32_TH, a.planes, tbx, tby, tbz);
    const int plane = (int)tbz;
    const int oh0 = (int)tby * DW32_TH, ow0 = (int)tbx * DW_TW;
    const float *__restrict__ in = reinterpret_cast<const float *>(a.in) + (size_t)plane * a.in_h * a.in_w;
    const int tid = threadIdx.x;
    float flo[F], fhi[F];  // (PyWavelets' single-precision filters: not always the doubles rounded -- the coiflets)
#pragma unroll
    for (int j = 0; j < F; j++) { flo[j] = a.lo_f[j]; fhi[j] = a.hi_f[j]; }

    const int r0 = 2 * oh0 + 2 - F, c0 = 2 * ow0 + 2 - F;
    if (tid < NR) s_row[tid] = ext_index(r0 + tid, a.in_h, a.mode);
    if (tid < F) { s_flo[tid] = a.lo_f[tid]; s_fhi[tid] = a.hi_f[tid]; }
    __shared__ uint32_t s_amax;
    if (tid == 0) s_amax = 0;
    __syncthreads();

    // ---- axis -2 ----
    if (tid < NC) {
        const int gc = ext_index(c0 + tid, a.in_w, a.mode);
        float x[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int gr = s_row[r];
            x[r] = (gc < 0 || gr < 0) ? 0.0f : in[(size_t)gr * a.in_w + gc];
        }
        const int par = tid & 1, hc = tid >> 1;
#pragma unroll
        for (int o = 0; o < DW32_TH; o++) {
            float sl = 0.0f, shh = 0.0f;
            const int i = 2 * (oh0 + o) + 1;
            if (i < a.in_h || a.mode == 4) {  // (constant-edge mode: pywt keeps ascending order over the overhang too)
#pragma unroll
                for (int j = 0; j < F; j++) {
                    if ((LOM >> j) & 1u) sl += flo[j] * x[2 * o + F - 1 - j];
                    if ((HIM >> j) & 1u) shh += fhi[j] * x[2 * o + F - 1 - j];
                }
            } else if (oh0 + o < a.out_h) {  // overhang: extension taps first, nearest first (reloaded: run-time order)
                const int jb = i - a.in_h;
                for (int s = 0; s < F; s++) {
                    const int j = s <= jb ? jb - s : s;
                    const int gr = s_row[2 * o + F - 1 - j];
                    const float v = (gc < 0 || gr < 0) ? 0.0f : in[(size_t)gr * a.in_w + gc];
                    sl += s_flo[j] * v;
                    shh += s_fhi[j] * v;
                }
            }
            s_lo[par][o * RS + hc] = sl;
            s_hi[par][o * RS + hc] = shh;
        }
    }
    __syncthreads();

    // ---- axis -1 from LDS ----
    const int k = plane % a.c;
    const bool has_m = a.mults != nullptr;
    const double mk = has_m ? a.mults[k] : 1.0;
    const float qf = (float)a.q;
    int32_t *__restrict__ co = a.coeffs + (size_t)plane * a.enc_h * a.enc_w;
    float *__restrict__ llo = a.last ? nullptr : reinterpret_cast<float *>(a.ll_out) + (size_t)plane * a.out_h * a.out_w;
    uint32_t amax = 0;
#pragma unroll
    for (int u = 0; u < DW32_TH * DW_TW / DW_BLOCK; u++) {
        const int p = tid + u * DW_BLOCK;
        const int o = p / DW_TW, wcol = p % DW_TW;
        const int oh = oh0 + o, ow = ow0 + wcol;
        if (oh >= a.out_h || ow >= a.out_w) continue;
        float aa = 0.0f, ad = 0.0f, da = 0.0f, dd = 0.0f;
        const int i = 2 * ow + 1;
        if (i < a.in_w || a.mode == 4) {
#pragma unroll
            for (int j = 0; j < F; j++) {
                const float vl = s_lo[(F - 1 - j) & 1][o * RS + wcol + ((F - 1 - j) >> 1)];
                const float vh = s_hi[(F - 1 - j) & 1][o * RS + wcol + ((F - 1 - j) >> 1)];
                if ((LOM >> j) & 1u) { aa += flo[j] * vl; da += flo[j] * vh; }
                if ((HIM >> j) & 1u) { ad += fhi[j] * vl; dd += fhi[j] * vh; }
            }
        } else {
            const int jb = i - a.in_w;
            for (int s = 0; s < F; s++) {
                const int j = s <= jb ? jb - s : s;
                const float vl = s_lo[(F - 1 - j) & 1][o * RS + wcol + ((F - 1 - j) >> 1)];
                const float vh = s_hi[(F - 1 - j) & 1][o * RS + wcol + ((F - 1 - j) >> 1)];
                aa += s_flo[j] * vl; da += s_flo[j] * vh;
                ad += s_fhi[j] * vl; dd += s_fhi[j] * vh;
            }
        }
        const int32_t qad = quant_f32(ad, mk, a.q, qf, has_m), qda = quant_f32(da, mk, a.q, qf, has_m),
                      qdd = quant_f32(dd, mk, a.q, qf, has_m);
        if (a.last) {
            const int32_t qaa = quant_f32(aa, mk, a.q, qf, has_m);
            co[(size_t)oh * a.enc_w + ow] = qaa;
            amax = max(amax, iabs_u(qaa));
        } else {
            llo[(size_t)oh * a.out_w + ow] = aa;
        }
        co[(size_t)oh * a.enc_w + a.off_w + ow] = qad;
        co[(size_t)(a.off_h + oh) * a.enc_w + ow] = qda;
        co[(size_t)(a.off_h + oh) * a.enc_w + a.off_w + ow] = qdd;
        amax = max(amax, max(iabs_u(qad), max(iabs_u(qda), iabs_u(qdd))));
    }
    if (a.maxabs != nullptr) {
        block_raise_max(&a.maxabs[plane / a.c], amax, &s_amax);
    }
}

// ---- level 1 of a 3-channel image with the colour model change on its loads ---------------------
// The change needs all three planes of a pixel and costs three pow() per pixel -- about as much arithmetic as the
// transform costs memory time -- so every pixel must be converted exactly once: a workgroup owns a strip of C1_SW output
// columns of ALL THREE channels and marches down C1_ROWS output rows.  Thread = input column: per step it loads the
// R, G, B samples of two new rows (C1_PF steps ahead), converts them, slides them into a register window of F rows per
// channel, and filters down the column; the low / high rows of the three channels go through a double-buffered LDS row
// to the axis -1 filter (threads 0..127: aa, ad from the low rows; 128..255: da, dd from the high rows).  One barrier per
// output row; a pixel is loaded and converted once per strip (F-2 rows of overlap between vertically adjacent strips).
// Same sums in the same order as k_dwt_level on converted pixels, overhang order included: bit-identical outputs.
#ifndef C1_PF
#define C1_PF 1   // steps of look-ahead of the raw samples.  256 x 1024x1024: 1 -> 5.6 ms, 2 -> 7.1 (spills at 128 VGPRs wait
#endif            // for the look-ahead loads in front of them); 3 waves / SIMD without spills: 6.1 - 6.3; 2: 7.7
#define C1_ROWS 136
#ifndef C1_WPE
#define C1_WPE 4
#endif
template <int F, uint32_t LOM, uint32_t HIM, int PX = PX_F64>  // PX_U8 / PX_U16: an 8- / 16-bit picture (a.px; a.in unused)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(C1_WPE, C1_WPE)))  // 128 VGPRs: left alone the compiler interleaves
void k_dwt1_color(DwtKArgs a, uint32_t gx, uint32_t gy) {                       // the six powers of a step over 173 (2 waves / SIMD)
    constexpr int SW = (256 - (F - 2)) / 2;  // output columns per strip: exactly 256 input columns
    constexpr int HC = 128 + 2;
    __shared__ double s_lo[2][3][2][HC];     // [output row parity][channel][column parity][column >> 1]
    __shared__ double s_hi[2][3][2][HC];
    __shared__ SpowLds s_pw;
    __shared__ uint32_t s_amax;
    spow_lds_fill(s_pw, threadIdx.x);
    if (threadIdx.x == 0) s_amax = 0;
    __syncthreads();
    uint32_t tbx, tby, tbz;
    xcd_tile(gx, gy, a.planes / 3, tbx, tby, tbz);
    const int img = (int)tbz;
    const int ow0 = (int)tbx * SW, oa = (int)tby * C1_ROWS;
    const int ob = min(oa + C1_ROWS, a.out_h);
    const size_t npl = (size_t)a.in_h * a.in_w;
    const double *__restrict__ in = PX ? nullptr : a.in + (size_t)img * 3 * npl;
    const uint8_t *__restrict__ in8 = PX ? a.px.in + (int64_t)img * a.px.sb : nullptr;
    const int tid = threadIdx.x;
    const int gc = ext_index(2 * ow0 + 2 - F + tid, a.in_w, a.mode);
    auto ld = [&](int r, double &u0, double &u1, double &u2) {  // raw R, G, B of (row r, this column), extension applied
        const int gr = ext_index(r, a.in_h, a.mode);
        const bool z = gc < 0 || gr < 0;
        if (PX) {  // (the pixel's three channels sc bytes apart: neighbours in an interleaved picture)
            const int64_t o = z ? 0 : (int64_t)gr * a.px.sh + (int64_t)gc * a.px.sw;
            if constexpr (PX == PX_FLT) {  // the three loads, then the widenings (the kind is uniform over the launch)
                const uint32_t r0 = px_load<PX>(in8 + o, a.px.kind), r1 = px_load<PX>(in8 + (o + a.px.sc), a.px.kind);
                const uint32_t r2 = px_load<PX>(in8 + (o + 2 * a.px.sc), a.px.kind);
                u0 = px_value<PX>(r0, a.px.kind); u1 = px_value<PX>(r1, a.px.kind); u2 = px_value<PX>(r2, a.px.kind);
            } else {
                u0 = px_value<PX>(px_load<PX>(in8 + o)); u1 = px_value<PX>(px_load<PX>(in8 + (o + a.px.sc)));
                u2 = px_value<PX>(px_load<PX>(in8 + (o + 2 * a.px.sc)));
            }
        } else {
            const size_t o = z ? 0 : (size_t)gr * a.in_w + gc;
            u0 = in[o]; u1 = in[o + npl]; u2 = in[o + 2 * npl];
        }
        if (z) { u0 = 0.0; u1 = 0.0; u2 = 0.0; }
    };
    // "zero" extension pads the CONVERTED signal with zeros (pywt extends what it is given): convert, then zero
    auto cv = [&](int r, double u0, double u1, double u2, double &w0, double &w1, double &w2) {
        color3_px(a.col, s_pw, u0, u1, u2, w0, w1, w2);
        if (gc < 0 || ext_index(r, a.in_h, a.mode) < 0) { w0 = 0.0; w1 = 0.0; w2 = 0.0; }
    };
    double win[3][F];  // rows 2o+2-F .. 2o+1 of output row o, converted
#pragma unroll
    for (int t = 0; t < F; t++) {
        double u0, u1, u2;
        ld(2 * oa + 2 - F + t, u0, u1, u2);
        cv(2 * oa + 2 - F + t, u0, u1, u2, win[0][t], win[1][t], win[2][t]);
    }
    double pq[C1_PF][2][3];  // raw samples of the two rows each of the next C1_PF steps brings in
#pragma unroll
    for (int u = 0; u < C1_PF; u++)
#pragma unroll
        for (int e = 0; e < 2; e++) ld(2 * (oa + 1 + u) + e, pq[u][e][0], pq[u][e][1], pq[u][e][2]);

    const bool has_m = a.mults != nullptr;
    double mk[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) mk[ch] = has_m ? a.mults[ch] : 1.0;
    const int role = tid >> 7, wcol = tid & 127;
    const int ow = ow0 + wcol;
    const bool wr = wcol < SW && ow < a.out_w;
    const size_t cpl = (size_t)a.enc_h * a.enc_w, lpl = (size_t)a.out_h * a.out_w;
    int32_t *__restrict__ co = a.coeffs + (size_t)img * 3 * cpl;
    double *__restrict__ llo = a.last ? nullptr : a.ll_out + (size_t)img * 3 * lpl;
    uint32_t amax = 0;
    const int par = tid & 1, hc = tid >> 1;

    for (int o0 = oa; o0 < ob; o0 += C1_PF) {
#pragma unroll
        for (int u = 0; u < C1_PF; u++) {
            const int o = o0 + u;
            // ---- axis -2 for output row o, three channels ----
            if (o < a.ov_h) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    double sl = 0.0, shh = 0.0;
#pragma unroll
                    for (int j = 0; j < F; j++) {
                        if ((LOM >> j) & 1u) sl += a.lo[j] * win[ch][F - 1 - j];
                        if ((HIM >> j) & 1u) shh += a.hi[j] * win[ch][F - 1 - j];
                    }
                    s_lo[o & 1][ch][par][hc] = sl;
                    s_hi[o & 1][ch][par][hc] = shh;
                }
            } else {  // bottom overhang: PyWavelets' order (k_dwt_level); the window element is picked with selects
                const int jb = 2 * o + 1 - a.in_h;
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    double sl = 0.0, shh = 0.0;
                    for (int s2 = 0; s2 < F; s2++) {
                        const int j = s2 <= jb ? jb - s2 : s2;
                        double v = win[ch][0];
#pragma unroll
                        for (int t = 1; t < F; t++) v = (F - 1 - j == t) ? win[ch][t] : v;
                        sl += a.lo[j] * v;
                        shh += a.hi[j] * v;
                    }
                    s_lo[o & 1][ch][par][hc] = sl;
                    s_hi[o & 1][ch][par][hc] = shh;
                }
            }
            // slide the windows: the two rows this step brings in are converted now, their successors requested
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
#pragma unroll
                for (int t = 0; t < F - 2; t++) win[ch][t] = win[ch][t + 2];
#pragma unroll
            for (int e = 0; e < 2; e++)
                cv(2 * (o + 1) + e, pq[u][e][0], pq[u][e][1], pq[u][e][2], win[0][F - 2 + e], win[1][F - 2 + e], win[2][F - 2 + e]);
#pragma unroll
            for (int e = 0; e < 2; e++) ld(2 * (o + 1 + C1_PF) + e, pq[u][e][0], pq[u][e][1], pq[u][e][2]);
            __syncthreads();
            // ---- axis -1: two sub-bands per thread and channel ----
            if (wr && o < ob) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const double(*src)[HC] = role ? s_hi[o & 1][ch] : s_lo[o & 1][ch];
                    double r0 = 0.0, r1 = 0.0;  // role 0: aa, ad   role 1: da, dd
                    if (ow < a.ov_w) {
#pragma unroll
                        for (int j = 0; j < F; j++) {
                            const double v = src[(F - 1 - j) & 1][wcol + ((F - 1 - j) >> 1)];
                            if ((LOM >> j) & 1u) r0 += a.lo[j] * v;
                            if ((HIM >> j) & 1u) r1 += a.hi[j] * v;
                        }
                    } else {  // right overhang
                        const int jb = 2 * ow + 1 - a.in_w;
                        for (int s2 = 0; s2 < F; s2++) {
                            const int j = s2 <= jb ? jb - s2 : s2;
                            const double v = src[(F - 1 - j) & 1][wcol + ((F - 1 - j) >> 1)];
                            r0 += a.lo[j] * v;
                            r1 += a.hi[j] * v;
                        }
                    }
                    int32_t *cc = co + (size_t)ch * cpl;
                    const int32_t q1 = quant(r1, mk[ch], a.q, has_m);
                    amax = max(amax, iabs_u(q1));
                    if (role == 0) {
                        if (a.last) {
                            const int32_t q0 = quant(r0, mk[ch], a.q, has_m);
                            cc[(size_t)o * a.enc_w + ow] = q0;
                            amax = max(amax, iabs_u(q0));
                        } else {
                            llo[(size_t)ch * lpl + (size_t)o * a.out_w + ow] = r0;
                        }
                        cc[(size_t)o * a.enc_w + a.off_w + ow] = q1;                      // 'ad' top-right
                    } else {
                        const int32_t q0 = quant(r0, mk[ch], a.q, has_m);
                        amax = max(amax, iabs_u(q0));
                        cc[(size_t)(a.off_h + o) * a.enc_w + ow] = q0;                     // 'da' bottom-left
                        cc[(size_t)(a.off_h + o) * a.enc_w + a.off_w + ow] = q1;           // 'dd' bottom-right
                    }
                }
            }
        }
    }
    if (a.maxabs != nullptr) {
        block_raise_max(&a.maxabs[img], amax, &s_amax);
    }
}

// ---- host launchers -----------------------------------------------------------------------------

// The launch-time constants of k_dwt_level (common.h: DwtKArgs): the tile grid with its division multipliers, and the choice
// of addressing -- 32-bit offsets into plane descriptors where every plane is small enough for them (dwt_narrow_ok), the 64-bit
// addressing otherwise (or when SPIHT_DWT_ADDR64 is set to a non-zero number: the tests run small pictures through it).
// Returns the number of tiles.
extern "C" int spiht_dwt_addr32(int64_t in_h, int64_t in_w, int64_t out_h, int64_t out_w, int64_t enc_h, int64_t enc_w, int px_es,
                                int64_t px_sh, int64_t px_sw) {
    return dwt_narrow_ok(in_h, in_w, out_h, out_w, enc_h, enc_w, px_es, px_sh, px_sw) ? 1 : 0;
}
static uint32_t dwt_set_launch_consts(DwtKArgs &a, int planes, int px) {
    a.gx = (uint32_t)((a.out_w + DW_TW - 1) / DW_TW);
    a.gy = (uint32_t)((a.out_h + DW_TH - 1) / DW_TH);
    a.nt = a.gx * a.gy * (uint32_t)planes;
    a.dv_gx = fastdivu_make(a.gx);
    a.dv_gy = fastdivu_make(a.gy);
    a.dv_c = fastdivu_make((uint32_t)a.c);
    const char *force = getenv("SPIHT_DWT_ADDR64");
    a.narrow = spiht_dwt_addr32(a.in_h, a.in_w, a.out_h, a.out_w, a.enc_h, a.enc_w, px ? a.px.es : 0, a.px.sh, a.px.sw) &&
               !(force && atoi(force) != 0);
    if (a.narrow) {
        a.in_pb = px ? (uint32_t)((a.in_h - 1) * a.px.sh + (a.in_w - 1) * a.px.sw + a.px.es) : (uint32_t)a.in_h * (uint32_t)a.in_w * 8u;
        a.in_rb = px ? (uint32_t)a.px.sh : (uint32_t)a.in_w * 8u;
        a.in_cb = px ? (uint32_t)a.px.sw : 8u;
        a.co_pb = (uint32_t)a.enc_h * (uint32_t)a.enc_w * 4u;
        a.co_rb = (uint32_t)a.enc_w * 4u;
        a.ll_pb = (uint32_t)a.out_h * (uint32_t)a.out_w * 8u;
        a.ll_rb = (uint32_t)a.out_w * 8u;
    }
    return a.nt;
}

// a.px.in set: level 1 of an 8- or 16-bit picture (the kernels of the kind a.px.es names; a.in unused)
template <int F, uint32_t LOM, uint32_t HIM>
static int launch_dwt_FM(DwtKArgs a, int planes, hipStream_t st) {
    a.planes = planes;
    const int px = a.px.in == nullptr ? PX_F64 : px_kind_of(a.px);
    a.ov_h = a.out_h;
    a.ov_w = a.out_w;
    if (a.f32) {
        uint32_t ntf = (uint32_t)((a.out_w + DW_TW - 1) / DW_TW) * (uint32_t)((a.out_h + DW32_TH - 1) / DW32_TH) * (uint32_t)planes;
        hipLaunchKernelGGL((k_dwt_level_f32<F, LOM, HIM>), dim3(ntf), dim3(DW_BLOCK), 0, st, a);
        return (int)hipGetLastError();
    }
    // Outputs summed in PyWavelets' overhang order: those with jb = 2o+1-N >= 0 (constant-edge mode keeps ascending order).
    // Inputs shorter than the filter take the same order -- right-hand extension taps first, nearest first, then ascending
    // through the signal and on into the left-hand extension (checked against PyWavelets: tests/golden/short_pywt.npz).
    // The order is tap jb, jb-1, ..., 0, jb+1, ...: with z leading taps that are zero in both filters it gives the same
    // bits as ascending order until jb >= z+2 (a zero tap adds nothing and the first two non-zero terms commute).
    int z = 0;
    while (z < F && a.lo[z] == 0.0 && a.hi[z] == 0.0) z++;
    if (a.mode != 4) a.ov_h = min(a.out_h, (a.in_h + z + 2) / 2);
    if (a.mode != 4) a.ov_w = min(a.out_w, (a.in_w + z + 2) / 2);
    if (a.color) {  // level 1 of a 3-channel image, colour model change on the loads
        constexpr int SW = (256 - (F - 2)) / 2;
        const uint32_t gx = (uint32_t)((a.out_w + SW - 1) / SW), gy = (uint32_t)((a.out_h + C1_ROWS - 1) / C1_ROWS);
        with_px(px, [&](auto PX) {
            hipLaunchKernelGGL((k_dwt1_color<F, LOM, HIM, PX>), dim3(gx * gy * (uint32_t)(planes / 3)), dim3(256), 0, st, a, gx, gy);
        });
        return (int)hipGetLastError();
    }
    const uint32_t nt = dwt_set_launch_consts(a, planes, px);
    with_px(px, [&](auto PX) {
        if (a.narrow) hipLaunchKernelGGL((k_dwt_level<F, LOM, HIM, PX>), dim3(nt), dim3(DWF_BLOCK), 0, st, a);
        else hipLaunchKernelGGL((k_dwt_level<F, LOM, HIM, PX, true>), dim3(nt), dim3(DWF_BLOCK), 0, st, a);
    });
    const int n_edge = (a.out_h - a.ov_h) * a.out_w + a.ov_h * (a.out_w - a.ov_w);
    if (n_edge > 0)
        with_px(px, [&](auto PX) { hipLaunchKernelGGL((k_dwt_edge<F, PX>), dim3((n_edge + 255) / 256, planes), dim3(256), 0, st, a); });
    return (int)hipGetLastError();
}
// specialised for the zero-tap pattern of the known filter bank of that length, generic otherwise
template <int F, uint32_t LOM, uint32_t HIM>
static int launch_dwt_F(const DwtKArgs &a, int planes, hipStream_t st) {
    uint32_t lom, him;
    tap_masks(a.lo, a.hi, F, lom, him);
    if (lom == LOM && him == HIM) return launch_dwt_FM<F, LOM, HIM>(a, planes, st);
    return launch_dwt_FM<F, (1u << F) - 1u, (1u << F) - 1u>(a, planes, st);
}

// a->px.in set: level 1 of an 8- or 16-bit picture, tiled routes only (the caller converts for the two-pass level)
extern "C" int spiht_launch_dwt_level(const DwtKArgs *a, int planes, hipStream_t st) {
    switch (a->F) {
    case 2: return launch_dwt_F<2, 0x3u, 0x3u>(*a, planes, st);            // haar
    case 6: return launch_dwt_F<6, 0x3Eu, 0x0Eu>(*a, planes, st);          // bior2.2
    case 10: return launch_dwt_F<10, 0x3FEu, 0x0FEu>(*a, planes, st);      // bior4.4
    case 18: return launch_dwt_F<18, 0x3FFFEu, 0x3FF8u>(*a, planes, st);   // bior6.8
    // every other even length up to SPIHT_MAX_TAPS (db / sym / coif / the other bior and rbio banks): all taps taken
    case 4: return launch_dwt_F<4, 0xFu, 0xFu>(*a, planes, st);
    case 8: return launch_dwt_F<8, 0xFFu, 0xFFu>(*a, planes, st);
    case 12: return launch_dwt_F<12, 0xFFFu, 0xFFFu>(*a, planes, st);
    case 14: return launch_dwt_F<14, 0x3FFFu, 0x3FFFu>(*a, planes, st);
    case 16: return launch_dwt_F<16, 0xFFFFu, 0xFFFFu>(*a, planes, st);
    case 20: return launch_dwt_F<20, 0xFFFFFu, 0xFFFFFu>(*a, planes, st);
    default: return -1;
    }
}
