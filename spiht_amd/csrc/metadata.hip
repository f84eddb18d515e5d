// decode_with_metadata (gfx950): turns the position-indexed trace written by k_decode<true> into the
// reference's int32[nbits+1, 8] table (/root/reference/src/encoder_decoder.rs:616-684):
//   [action, local_h, local_w, channel, filter, depth, n, value of the coefficient before the bit is read]
// Seven of the eight columns are a pure function of the trace record (k_meta_rows).  The eighth, the running
// value of the coefficient, depends on every earlier write to the same coefficient -- and on trees with
// duplicated nodes (odd ll_h / ll_w) two list entries write the same cell -- so the records are
// stable-sorted by node index (rocPRIM radix sort; position order is kept inside a node) and one thread per node
// replays that node's few writes in stream order (k_meta_fold).  This is the sequential semantics of the
// reference for any byte string, not only for encoder-produced streams.
#include "common.h"
#include "list_coder.h"  // decomp
#include <algorithm>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#define META_KEY_NONE 0x10000000u  // sorts after every node index (< 2^28)

__global__ __launch_bounds__(256) void k_meta_keys(const uint32_t *__restrict__ tr_ent, const uint8_t *__restrict__ tr_act,
                                                   uint64_t rows, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < rows; q += (uint64_t)gridDim.x * blockDim.x) {
        keys[q] = tr_act[q] == TR_NONE ? META_KEY_NONE : (tr_ent[q] & ENT_IDX_META);
        vals[q] = (uint32_t)q;
    }
}

// Rust `f32 as i32`: toward zero, saturating, NaN -> 0
__device__ __forceinline__ int32_t f32_as_i32(float v) {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (int32_t)0x80000000u;
    return (int32_t)v;
}

// get_local_position, encoder_decoder.rs:593-613: single-precision divide, multiply, subtract, each rounded
__device__ __forceinline__ int32_t local_coord(uint32_t x, int32_t start, int32_t extent) {
    const float num = __fsub_rn((float)x, (float)start);
    const float frac = __fdiv_rn(num, (float)extent);
    return f32_as_i32(__fsub_rn(__fmul_rn(frac, 200000.0f), 100000.0f));
}

// columns 0..6 of the row of a record (the eighth, the running value, is the fold's): entry e, action | plane << 3 ac
__device__ __forceinline__ void meta_row(const Geom &g, const int32_t *slices, int32_t level, uint32_t e, uint32_t ac, int4 &r0,
                                         int4 &r1) {
    const uint32_t idx = e & ENT_IDX_META;
    const uint32_t filter = (e >> ENT_FILT_SHIFT) & 3u;
    uint32_t k, i, j;
    decomp(g, idx, k, i, j);
    // generation = halvings until the index-tree ancestor is a root (the tree is index based outside LL)
    uint32_t t = 0, ii = i, jj = j;
    while (!(ii < (uint32_t)g.ll_h && jj < (uint32_t)g.ll_w)) { ii >>= 1; jj >>= 1; t++; }
    int32_t lh, lw;
    if (t == 0) {  // :597-600: LL does not subtract the slice start
        lh = local_coord(i, 0, slices[1]);
        lw = local_coord(j, 0, slices[3]);
    } else {       // :601-609: other_slices[level-1-depth][filter-1]
        const int32_t *s = slices + 4 + ((t - 1) * 3 + (filter - 1)) * 4;
        lh = local_coord(i, s[0], s[1] - s[0]);
        lw = local_coord(j, s[2], s[3] - s[2]);
    }
    r0 = make_int4((int)(ac & 7u), lh, lw, (int)k);
    r1 = make_int4((int)filter, level - (int)t, (int)(ac >> 3), 0);
}

__global__ __launch_bounds__(256) void k_meta_rows(MetaArgs a) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.rows; q += (uint64_t)gridDim.x * blockDim.x) {
        int4 r0 = make_int4(0, 0, 0, 0), r1 = make_int4(0, 0, 0, 0);
        const uint32_t ac = a.tr_act[q];
        if (ac != TR_NONE) meta_row(a.g, a.slices, a.level, a.tr_ent[q], ac, r0, r1);
        int4 *row = reinterpret_cast<int4 *>(a.meta + q * 8);
        row[0] = r0;
        row[1] = r1;
    }
}

// encoder_decoder.rs:14-29
__device__ __forceinline__ int32_t meta_set_bit(int32_t x, uint32_t n, uint32_t bit) {
    const uint32_t m = 1u << n;
    if (x >= 0) return bit ? (int32_t)((uint32_t)x | m) : (int32_t)((uint32_t)x & ~m);
    uint32_t v = (uint32_t)(-x);
    v = bit ? (v | m) : (v & ~m);
    return -(int32_t)v;
}

// the coefficient after the operation of trace record ac (action | plane << 3) has read `bit` (action 1 / 4: sign bit ->
// +-1.5*2^n, :714-724 / :751-761; action 6: refinement bit, :825; every other action leaves it)
__device__ __forceinline__ int32_t meta_apply(int32_t x, uint32_t ac, uint32_t bit) {
    const uint32_t act = ac & 7u, n = ac >> 3;
    if (act == 1u || act == 4u) {
        const int32_t base = n == 0 ? 1 : (int32_t)((1u << (n - 1)) + (1u << n));
        return bit ? base : -base;
    }
    if (act == 6u) return meta_set_bit(x, n, bit);
    return x;
}

// one thread per node: walk the node's records in stream order, note the value before each record, apply the writes
__global__ __launch_bounds__(256) void k_meta_fold(MetaArgs a) {
    const uint64_t nbits = a.rows - 1;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.rows; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t key = a.skey[s];
        if (key == META_KEY_NONE) continue;
        if (s > 0 && a.skey[s - 1] == key) continue;  // not the first record of its node
        int32_t x = 0;
        for (uint64_t r = s; r < a.rows && a.skey[r] == key; r++) {
            const uint64_t q = a.spos[r];
            a.meta[q * 8 + 7] = x;
            if (q >= nbits) continue;  // the waiting operation never got its bit
            x = meta_apply(x, a.tr_act[q], (a.data[q >> 3] >> (q & 7)) & 1u);
        }
    }
}

// Progressive decoding to K bit budgets from ONE walk of the stream (the pattern of the reference's make_gif.py:46-61:
// decode(bytes[:k]) for many k).  The decoder's state after b bits is the state after the operations
// of stream positions < b, and the sorted trace has every node's operations in stream order: one thread per node replays
// them once and leaves the node's value in out[kk] whenever it passes budgets[kk] (ascending).  out: [K][g.n], zeroed
// by the caller (a node without operations stays 0).
__global__ __launch_bounds__(256) void k_budget_fold(MetaArgs a, const uint64_t *__restrict__ budgets, int K, int32_t *__restrict__ out) {
    const uint64_t nbits = a.rows - 1;
    const size_t n_cells = a.g.n;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.rows; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t key = a.skey[s];
        if (key == META_KEY_NONE) continue;
        if (s > 0 && a.skey[s - 1] == key) continue;  // not the first record of its node
        int32_t x = 0;
        int kk = 0;
        for (uint64_t r = s; r < a.rows && a.skey[r] == key; r++) {
            const uint64_t q = a.spos[r];
            for (; kk < K && budgets[kk] <= q; kk++)  // budgets that end in front of this operation
                if (x) out[(size_t)kk * n_cells + key] = x;
            if (q >= nbits) continue;  // the waiting operation never got its bit
            x = meta_apply(x, a.tr_act[q], (a.data[q >> 3] >> (q & 7)) & 1u);
        }
        for (; kk < K; kk++)
            if (x) out[(size_t)kk * n_cells + key] = x;
    }
}

extern "C" int spiht_meta_sort_temp_bytes(uint64_t rows, size_t *bytes) {
    size_t sz = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sz, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (size_t)rows, 0u, 29u, (hipStream_t)0);
    *bytes = sz;
    return (int)e;
}

// a->skey / a->spos must point to keys_out / vals_out
extern "C" int spiht_launch_metadata(const MetaArgs *a, uint32_t *keys_in, uint32_t *vals_in, uint32_t *keys_out,
                                     uint32_t *vals_out, void *temp, size_t temp_bytes, hipStream_t st) {
    const uint64_t rows = a->rows;
    const int grid = (int)std::min<uint64_t>((rows + 255) / 256, 1u << 16);
    hipLaunchKernelGGL(k_meta_keys, dim3(grid), dim3(256), 0, st, a->tr_ent, a->tr_act, rows, keys_in, vals_in);
    hipLaunchKernelGGL(k_meta_rows, dim3(grid), dim3(256), 0, st, *a);
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)rows, 0u, 29u, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_meta_fold, dim3(grid), dim3(256), 0, st, *a);
    return (int)hipGetLastError();
}

// the trace sorted by (node, position) as above, then k_budget_fold.  a->skey / a->spos must point to keys_out / vals_out
extern "C" int spiht_launch_budget_fold(const MetaArgs *a, uint32_t *keys_in, uint32_t *vals_in, uint32_t *keys_out,
                                        uint32_t *vals_out, void *temp, size_t temp_bytes, const uint64_t *d_budgets, int K,
                                        int32_t *d_out, hipStream_t st) {
    const uint64_t rows = a->rows;
    const int grid = (int)std::min<uint64_t>((rows + 255) / 256, 1u << 16);
    hipLaunchKernelGGL(k_meta_keys, dim3(grid), dim3(256), 0, st, a->tr_ent, a->tr_act, rows, keys_in, vals_in);
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)rows, 0u, 29u, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_budget_fold, dim3(grid), dim3(256), 0, st, *a, d_budgets, K, d_out);
    return (int)hipGetLastError();
}

// ---- the batched form: a chunk of nb images, trace of image b at b * tr_stride (spiht_decode_with_metadata_batch_i32) ----
// Per image the same three steps on that image's own records; one radix sort over the chunk on the key b * n + node keeps
// the images apart (records ordered by image, node, position).  A segmented sort on the node, a segment per image, was
// measured against it: 2.4x slower at 64 1080p pictures, 2 % faster at 1024 of 256 x 256.

// records of image b that are rows of its table: 8 * nbytes + 1, as the decoder counts them (a slot that claims more than
// slot_stride bytes is decoded as an empty stream, and flagged)
__device__ __forceinline__ uint32_t meta_valid_rows(const MetaBatchArgs &a, uint32_t b) {
    const uint64_t nby = a.nbytes[b];
    return nby > a.slot_stride ? 1u : (uint32_t)(nby * 8 + 1);
}

// grid (x, nb): image blockIdx.y
__global__ __launch_bounds__(256) void k_meta_keys_batch(MetaBatchArgs a, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint32_t base = blockIdx.y * a.tr_stride;
    const uint32_t kb = blockIdx.y * a.g.n;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < a.tr_stride; p += gridDim.x * blockDim.x) {
        const uint32_t q = base + p;
        keys[q] = a.tr_act[q] == TR_NONE ? a.key_none : kb + (a.tr_ent[q] & ENT_IDX_META);
        vals[q] = q;
    }
}

// grid (x, nb): every one of the image's meta_rows rows is written, zeros past its valid rows
__global__ __launch_bounds__(256) void k_meta_rows_batch(MetaBatchArgs a) {
    const uint32_t b = blockIdx.y;
    const uint32_t rows = meta_valid_rows(a, b);
    const uint32_t *ent = a.tr_ent + (size_t)b * a.tr_stride;
    const uint8_t *act = a.tr_act + (size_t)b * a.tr_stride;
    int4 *out = reinterpret_cast<int4 *>(a.meta + (size_t)b * a.meta_rows * 8);
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.meta_rows; p += (uint64_t)gridDim.x * blockDim.x) {
        int4 r0 = make_int4(0, 0, 0, 0), r1 = make_int4(0, 0, 0, 0);
        if (p < rows) {
            const uint32_t ac = act[p];
            if (ac != TR_NONE) meta_row(a.g, a.slices, a.level, ent[p], ac, r0, r1);
        }
        out[2 * p] = r0;
        out[2 * p + 1] = r1;
    }
}

// k_meta_fold over the chunk: a node's records are the run of one key; its image is that of the records' positions
__global__ __launch_bounds__(256) void k_meta_fold_batch(MetaBatchArgs a, uint32_t records) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < records; s += gridDim.x * blockDim.x) {
        const uint32_t key = a.skey[s];
        if (key == a.key_none) continue;
        if (s > 0 && a.skey[s - 1] == key) continue;  // not the first record of its node
        const uint32_t b = fdiv(a.spos[s], a.div_tr);
        const uint32_t base = b * a.tr_stride, nbits = meta_valid_rows(a, b) - 1;
        const uint8_t *data = a.data + (size_t)b * a.slot_stride;
        int32_t *meta = a.meta + (size_t)b * a.meta_rows * 8;
        int32_t x = 0;
        for (uint32_t r = s; r < records && a.skey[r] == key; r++) {
            const uint32_t q = a.spos[r];
            const uint32_t p = q - base;
            meta[(size_t)p * 8 + 7] = x;
            if (p >= nbits) continue;  // the waiting operation never got its bit
            x = meta_apply(x, a.tr_act[q], (data[p >> 3] >> (p & 7)) & 1u);
        }
    }
}

static hipError_t meta_batch_sort(const MetaBatchArgs &a, void *temp, size_t &temp_bytes, uint32_t *keys_in, uint32_t *vals_in,
                                  uint32_t *keys_out, uint32_t *vals_out, hipStream_t st) {
    const unsigned end_bit = 32u - (unsigned)__builtin_clz(a.key_none);  // key_none = nb * n, the largest key
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)a.nb * a.tr_stride, 0u,
                                     end_bit, st);
}

// the sort's temporary for the chunk `a` describes (nb, tr_stride, key_none)
extern "C" int spiht_meta_batch_sort_temp_bytes(const MetaBatchArgs *a, size_t *bytes) {
    size_t sz = 0;
    hipError_t e = meta_batch_sort(*a, nullptr, sz, nullptr, nullptr, nullptr, nullptr, (hipStream_t)0);
    *bytes = sz;
    return (int)e;
}

// a->skey / a->spos must point to keys_out / vals_out
extern "C" int spiht_launch_metadata_batch(const MetaBatchArgs *a, uint32_t *keys_in, uint32_t *vals_in, uint32_t *keys_out,
                                           uint32_t *vals_out, void *temp, size_t temp_bytes, hipStream_t st) {
    const uint32_t records = (uint32_t)a->nb * a->tr_stride;
    const dim3 g_tr((unsigned)std::min<uint64_t>((a->tr_stride + 255) / 256, 1024), (unsigned)a->nb);
    const dim3 g_rows((unsigned)std::min<uint64_t>((a->meta_rows + 255) / 256, 1024), (unsigned)a->nb);
    hipLaunchKernelGGL(k_meta_keys_batch, g_tr, dim3(256), 0, st, *a, keys_in, vals_in);
    hipLaunchKernelGGL(k_meta_rows_batch, g_rows, dim3(256), 0, st, *a);
    hipError_t e = meta_batch_sort(*a, temp, temp_bytes, keys_in, vals_in, keys_out, vals_out, st);
    if (e != hipSuccess) return (int)e;
    const int grid = (int)std::min<uint64_t>(((uint64_t)records + 255) / 256, 1u << 16);
    hipLaunchKernelGGL(k_meta_fold_batch, dim3(grid), dim3(256), 0, st, *a, records);
    return (int)hipGetLastError();
}
