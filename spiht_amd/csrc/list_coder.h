// The rules of the list coder, each written once (device code only).  Used by the two list encoders (encode.hip: one workgroup
// per image; encode_wide.hip: one image on several CUs), by the decoder for the tree (decode.hip), by metadata.hip (decomp) and
// by pyramid.hip (iabs_u).  Every rule names the lines of the reference's encoder_decoder.rs that it reproduces.
// In order: the tree, the scan, the tokens, the appends of a fired entry, the staging of bits, an encoder's image (set-up, root
// seeding, closing report).  The tokens are what the encoders WRITE; the decoder reads the same tokens and writes none: its
// parsing is decode.hip's lip_starts (LIP pass) and work_lis (the type-A token) -- a change of a token is made here and there.
// What stays apart, and why:
//   * the LIS chunk bodies: k_encode scans five counts for one entry per thread, k_encode_wide four derived counts for WIDE_U
//     entries per thread, from which it works out the other counts; one body would be neither;
//   * the flushes: k_encode's emit_bits carries the partial last word into the staging buffer of the other parity, the wide
//     kernel's flush ORs the first and the last word, which it shares with other workgroups, into the stream;
//   * the decoder beyond the tree and the shuffle: its scan has two barriers and a partial array of its own, its passes are
//     placed by the sequencer; and the wide kernel's group state (WideCtl::bad) around the closing report.
// The kernels built from this header are compared with those before it, fold by fold, in profiles/list_coder_fold.txt.
#pragma once
#include "common.h"

// ---- tree geometry on the packed array [c, h, w] ---------------------------------------------------------------------------
// x.abs() of is_element_sig / is_bit_set (encoder_decoder.rs:31-41)  (INT32_MIN -> 2^31, no signed overflow)
__device__ __forceinline__ uint32_t iabs_u(int32_t x) { return x < 0 ? 0u - (uint32_t)x : (uint32_t)x; }
// linear index -> (channel, row, column)
__device__ __forceinline__ void decomp(const Geom &g, uint32_t idx, uint32_t &k, uint32_t &i, uint32_t &j) {
    k = fdiv(idx, g.div_hw);
    uint32_t r = idx - k * g.hw;
    i = fdiv(r, g.div_w);
    j = r - i * (uint32_t)g.w;
}
// offspring (0,0) of node (i,j): row r, column cc (the others are +1 in either direction); returns its linear
// index within the image  (get_offspring, encoder_decoder.rs:43-75)
__device__ __forceinline__ uint32_t child_base(const Geom &g, uint32_t k, uint32_t i, uint32_t j, uint32_t &r, uint32_t &cc) {
    if (i < (uint32_t)g.ll_h && j < (uint32_t)g.ll_w) {
        r = (i & 1u) * (uint32_t)g.ll_h + (i & ~1u);
        cc = (j & 1u) * (uint32_t)g.ll_w + (j & ~1u);
    } else {
        r = 2 * i;
        cc = 2 * j;
    }
    return k * g.hw + r * (uint32_t)g.w + cc;
}
// linear index of offspring q = 0..3, in the order of get_offspring's array (encoder_decoder.rs:57-62, 69-74); cb = child_base
__device__ __forceinline__ uint32_t offspring(uint32_t cb, int q, uint32_t W) { return cb + (q >> 1) * W + (q & 1); }
// has_descendents_past_offspring (encoder_decoder.rs:7-12), raw coordinates
__device__ __forceinline__ bool has_grandchildren(uint32_t i, uint32_t j, uint32_t H, uint32_t W) {
    return 4 * i + 3 < H && 4 * j + 3 < W;
}
// type-A entry for child (ci,cj) with linear index idx: flagged leaf when it has no offspring of its own
// (get_offspring is None, encoder_decoder.rs:65-67; the reference queues the entry all the same, :273-278)
__device__ __forceinline__ uint32_t make_a_entry(uint32_t idx, uint32_t ci, uint32_t cj, uint32_t H, uint32_t W) {
    return idx | ENT_A | ((2 * ci + 1 < H && 2 * cj + 1 < W) ? 0u : ENT_LEAF);
}
// a fired type-B entry: the type-A entries of its four offspring at nxt[oq .. oq + 3] (encoder_decoder.rs:272-278).
// cb, cr, ccol = child_base; `orw` is ORed into each entry (the decoder's filter bits, else 0)
__device__ __forceinline__ void store_a_entries(uint32_t *nxt, uint32_t oq, uint32_t cb, uint32_t cr, uint32_t ccol, uint32_t H,
                                                uint32_t W, uint32_t orw) {
    nxt[oq] = make_a_entry(cb, cr, ccol, H, W) | orw;
    nxt[oq + 1] = make_a_entry(cb + 1, cr, ccol + 1, H, W) | orw;
    nxt[oq + 2] = make_a_entry(cb + W, cr + 1, ccol, H, W) | orw;
    nxt[oq + 3] = make_a_entry(cb + W + 1, cr + 1, ccol + 1, H, W) | orw;
}

// ---- scan --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int o) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = (uint32_t)__shfl_up((int)lo, o);
    hi = (uint32_t)__shfl_up((int)hi, o);
    return ((uint64_t)hi << 32) | lo;
}
// packed exclusive scan over the workgroup of an encoder; one __syncthreads; `par` alternates the partial buffer.  SH is the
// kernel's shared struct with `uint64_t part[2][wavefronts]`, taken by reference: handing sh.part[par] over as a pointer
// costs k_encode_wide 16 more spilled registers
template <class SH>
__device__ __forceinline__ uint64_t block_exscan_packed(uint64_t v, uint64_t &total, SH &sh, int par) {
    constexpr int NWAVES = (int)(sizeof(sh.part[0]) / sizeof(uint64_t));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint64_t t = shfl_up_u64(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sh.part[par][wave] = inc;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
#pragma unroll
    for (int wv = 0; wv < NWAVES; wv++) {
        uint64_t p = sh.part[par][wv];
        if (wv < wave) pre += p;
        tot += p;
    }
    total = tot;
    return pre + inc - v;
}

// ---- tokens, as the encoders write them (LSB first) ------------------------------------------------------------------------
// is_element_sig at plane n, T = 1 << n (encoder_decoder.rs:37-41)
__device__ __forceinline__ bool is_sig(int32_t x, uint32_t T) { return iabs_u(x) >= T; }
// the token of a significant coefficient, '1 s' with s = (x >= 0), two bits (LIP pass: encoder_decoder.rs:210-217; an offspring:
// :243-251); an insignificant one is '0', one bit
__device__ __forceinline__ uint32_t sig_token(int32_t x) { return 1u | ((x >= 0) ? 2u : 0u); }
// one offspring x = xc[q] of a fired type-A entry: its '0' | '1 s' at bit o of the entry's token, its bit of sigm, the mask of
// the significant offspring (encoder_decoder.rs:242-255)
__device__ __forceinline__ void token_a_offspring(int32_t x, uint32_t T, int q, uint32_t &bits, uint32_t &o, uint32_t &sigm) {
    if (is_sig(x, T)) {
        bits |= (1u << o) | ((x >= 0 ? 1u : 0u) << (o + 1));
        o += 2;
        sigm |= 1u << q;
    } else {
        o += 1;
    }
}
// the token of a fired type-A entry: '1', then its four offspring (encoder_decoder.rs:239-255).  Returns its bits; nb = its
// length (5 .. 9).  k_encode_wide runs this loop itself, over token_a_offspring: through token_a, in any wording, its count of
// spilled registers changes (profiles/list_coder_fold.txt)
__device__ __forceinline__ uint32_t token_a(const int32_t (&xc)[4], uint32_t T, uint32_t &nb, uint32_t &sigm) {
    uint32_t bits = 1u, o = 1;
    sigm = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) token_a_offspring(xc[q], T, q, bits, o, sigm);
    nb = o;
    return bits;
}
// refinement bit of an LSP entry at plane n: is_bit_set (encoder_decoder.rs:31-34, 286-292)
__device__ __forceinline__ uint32_t refine_bit(int32_t x, int n) { return (iabs_u(x) >> n) & 1u; }

// ---- appends of a fired type-A entry (encoder_decoder.rs:242-261) -----------------------------------------------------------
// its offspring to the LSP from os or the LIP from ol by sigm, and the entry itself to nxt[oq] as type B when it has
// grandchildren.  The offsets come by value -- popc(sigm), 4 - popc(sigm) and keep_b entries were written: with references that
// the function advances, k_encode_wide spills 79 registers instead of 24
__device__ __forceinline__ void append_fired_a(uint32_t idx, uint32_t cb, uint32_t W, uint32_t sigm, bool keep_b, uint32_t *lsp,
                                               uint32_t os, uint32_t *lip, uint32_t ol, uint32_t *nxt, uint32_t oq) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint32_t ci = offspring(cb, q, W);
        if (sigm & (1u << q)) lsp[os++] = ci; else lip[ol++] = ci;
    }
    if (keep_b) nxt[oq] = idx;  // type B
}

// ---- staging: a token's bits ORed into LDS words; chunk bit 0 lies at bit shft of wbuf[0], the chunk is cut at totv bits -------
__device__ __forceinline__ void stage_bits(uint32_t *wbuf, uint32_t bits, uint32_t nb, uint32_t off, uint32_t totv, uint32_t shft) {
    if (nb && off < totv) {
        const uint32_t nbv = (off + nb <= totv) ? nb : (totv - off);
        const uint32_t v = bits & ((1u << nbv) - 1u);  // nb <= 16
        const uint32_t p = shft + off, wi = p >> 5, bo = p & 31;
        if (v) {
            atomicOr(&wbuf[wi], v << bo);
            if (bo + nbv > 32) atomicOr(&wbuf[wi + 1], v >> (32 - bo));
        }
    }
}

// ---- one image of an encoder ---------------------------------------------------------------------------------------------
// `(max as f32).log2() as u8`  (encoder_decoder.rs:166) with the host libm's rounding (table from the host)
__device__ __forceinline__ int start_plane(uint32_t maxabs, const float *thr) {
    if (maxabs == 0) return 0;
    float m = (float)(int32_t)maxabs;
    int e = (int)((__float_as_uint(m) >> 23) & 0xffu) - 127;
    if (e + 1 <= 31 && m >= thr[e + 1]) e += 1;
    return e;
}

struct EncImage {
    const int32_t *X;         // coefficients
    const uint8_t *DM, *LM;   // the pyramid's codes of D and L (pyramid.hip)
    uint32_t *outw;           // the image's slot, as words
    uint64_t capb, max_bits;  // bits of the slot (never write past it); the budget, within the slot
};
__device__ __forceinline__ EncImage enc_image(const EncArgs &a, int b) {
    EncImage im;
    im.X = a.x + (size_t)b * a.g.n;
    im.DM = a.dmsb + (size_t)b * a.g.n;
    im.LM = a.lmsb + (size_t)b * a.g.n;
    im.outw = reinterpret_cast<uint32_t *>(a.out + (size_t)b * a.slot_stride);
    im.capb = a.slot_stride * 8;
    im.max_bits = a.max_bits < im.capb ? a.max_bits : im.capb;
    return im;
}
// max|x|, the first plane (encoder_decoder.rs:165-167), "|x| >= 2^30 is not coded".  In EncImage: 4 SGPR spills fewer (wide)
__device__ __forceinline__ int enc_first_plane(const EncArgs &a, int b, uint32_t &maxabs, bool &bad) {
    maxabs = a.maxabs[b];
    bad = maxabs >= (1u << 30);
    return start_plane(maxabs, a.log2_thresh);
}
// initial LIP / LIS from the root block (encoder_decoder.rs:169-190): i, j, then channel innermost.  `scan(v, tot)` is the
// kernel's workgroup scan, called by every thread.  Returns false when a list does not hold them.
template <uint32_t BLOCK, class Scan>
__device__ __forceinline__ bool seed_lists(const Geom &g, const ListCaps &caps, uint32_t *lip, uint32_t *lis, uint32_t &lip_len,
                                           uint32_t &lis_len, Scan scan) {
    const uint32_t tid = threadIdx.x, W = (uint32_t)g.w;
    const uint32_t nroot = (uint32_t)(g.ll_h * g.ll_w * g.c);
    for (uint32_t base = 0; base < nroot; base += BLOCK) {
        uint32_t t = base + tid;
        bool act = t < nroot;
        uint32_t k = 0, i = 0, j = 0;
        if (act) {
            uint32_t ij = t / (uint32_t)g.c;
            k = t - ij * (uint32_t)g.c;
            i = ij / (uint32_t)g.ll_w;
            j = ij - i * (uint32_t)g.ll_w;
        }
        uint32_t idx = k * g.hw + i * W + j;
        bool inlis = act && (((i | j) & 1u) != 0);
        uint64_t tot;
        uint64_t ex = scan(inlis ? 1ull : 0ull, tot);
        if (act && t < caps.lip) lip[t] = idx;
        if (inlis && lis_len + (uint32_t)ex < caps.lis) lis[lis_len + (uint32_t)ex] = idx | ENT_A;
        lis_len += (uint32_t)tot;
    }
    lip_len = nroot;
    return lip_len <= caps.lip && lis_len <= caps.lis;
}
// the closing report of an image, by one thread: the stream's length, its first plane, the error bits (1: a list capacity,
// 2: |x| >= 2^30, 4: the budget was cut by the slot).  maxabs, max_n: enc_first_plane's
__device__ __forceinline__ void enc_report(const EncArgs &a, int b, const EncImage &im, uint32_t maxabs, int max_n, uint64_t bitpos, bool bad) {
    a.out_nbits[b] = bitpos;
    a.out_maxn[b] = (uint8_t)max_n;
    if (bad) atomicOr(a.err, maxabs >= (1u << 30) ? 2u : 1u);
    if (a.max_bits > im.capb && bitpos >= im.capb) atomicOr(a.err, 4u);
}
