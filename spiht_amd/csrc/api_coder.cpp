// Host side of libspiht_hip.so (include/spiht_hip.h), the coder: the coder's geometry and list scratch, and the int32 calls
// -- encode / decode of coefficient arrays, single and batched, metadata, budgets and traces, the list-coding halves.  Mirrors
// what the reference's src/lib.rs does around encode()/decode(): take a strided int32 view, run the coder, pack/unpack bytes --
// here by queueing HIP kernels.
#include "api_internal.h"

int make_geom(int64_t c, int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, Geom *g) {
    if (!(ll_h > 1) || !(ll_w > 1)) return SPIHT_ERR_LL;
    if (c <= 0 || h <= 0 || w <= 0) return SPIHT_ERR_EMPTY;
    // the reference indexes arr[(k, l, m)] for the offspring of every root node: out of bounds -> panic
    int64_t need_h = (ll_h % 2 == 0) ? 2 * ll_h : 2 * ll_h - 1;
    int64_t need_w = (ll_w % 2 == 0) ? 2 * ll_w : 2 * ll_w - 1;
    if (h < need_h || w < need_w) return SPIHT_ERR_SHAPE;
    if ((double)c * (double)h * (double)w >= 1073741824.0) return SPIHT_ERR_TOO_LARGE;
    g->c = (int32_t)c; g->h = (int32_t)h; g->w = (int32_t)w;
    g->ll_h = (int32_t)ll_h; g->ll_w = (int32_t)ll_w;
    g->hw = (uint32_t)(h * w);
    g->n = (uint32_t)(c * h * w);
    g->pad = 0;
    g->div_w = fastdiv_make((uint32_t)w);
    g->div_hw = fastdiv_make(g->hw);
    return SPIHT_OK;
}

// number of tree-node instances (duplicates counted) and of instances with offspring
static void instance_counts(const Geom &g, uint64_t *nodes, uint64_t *parents) {
    const uint64_t h = (uint64_t)g.h, w = (uint64_t)g.w;
    const uint64_t he = h & ~1ull, we = w & ~1ull;  // (i|1) < h  <=>  i < he
    const uint64_t hp = h / 2, wp = w / 2;          // has offspring <=> i < hp && j < wp
    uint64_t nn = (uint64_t)g.ll_h * g.ll_w, pp = 0;
    for (int64_t i = 0; i < g.ll_h; i++)
        for (int64_t j = 0; j < g.ll_w; j++) {
            if (i % 2 == 0 && j % 2 == 0) continue;
            pp += 1;
            uint64_t ri = (uint64_t)((i & 1) * g.ll_h + (i & ~1ll)), rj = (uint64_t)((j & 1) * g.ll_w + (j & ~1ll));
            for (int q = 0; q < 4; q++) {
                uint64_t ci = ri + (q >> 1), cj = rj + (q & 1);
                // sub-tree of (ci,cj): depth t block rows [ci<<t, (ci+1)<<t)
                for (int t = 0; t < 32; t++) {
                    uint64_t r0 = ci << t, c0 = cj << t, sz = 1ull << t;
                    uint64_t lim_h = t == 0 ? h : he, lim_w = t == 0 ? w : we;
                    uint64_t rows = r0 >= lim_h ? 0 : std::min(sz, lim_h - r0);
                    uint64_t cols = c0 >= lim_w ? 0 : std::min(sz, lim_w - c0);
                    if (rows == 0 || cols == 0) break;
                    nn += rows * cols;
                    uint64_t prow = r0 >= hp ? 0 : std::min(sz, hp - r0);
                    uint64_t pcol = c0 >= wp ? 0 : std::min(sz, wp - c0);
                    pp += prow * pcol;
                }
            }
        }
    *nodes = nn * (uint64_t)g.c;
    *parents = pp * (uint64_t)g.c;
}

uint64_t bound_bits(const Geom &g, uint32_t max_abs) {
    uint64_t nodes, parents;
    instance_counts(g, &nodes, &parents);
    int planes = 1;
    while (planes < 32 && (1ull << planes) <= (uint64_t)max_abs) planes++;
    planes += 1;  // Q1: the start plane can be one above the true msb
    // per node: <= planes LIP zeros + sig + sign + <= planes refinement bits; per parent: <= planes A bits + planes B bits
    return nodes * (2ull * planes + 2) + parents * (2ull * planes);
}

static void list_caps(const Geom &g, uint64_t max_bits, ListCaps *caps, uint64_t *nodes_out) {
    uint64_t nodes, parents;
    instance_counts(g, &nodes, &parents);
    uint64_t roots = (uint64_t)g.c * g.ll_h * g.ll_w;
    uint64_t mb = max_bits;
    uint64_t lip = nodes, lsp = nodes, lis = parents + 4 * roots;  // + leaf A entries under root B entries (Q5)
    if (mb < (1ull << 40)) {
        // what a stream of mb bits can put on the lists ... plus what ONE chunk of the encoder appends: its scans
        // give every entry of the chunk its list slots before the bit budget cuts the chunk short (encode.hip: up to 2048
        // LIP entries or 1024 LIS entries per chunk; encode_wide.hip: 8192 or 2048; at most four appends each; found by
        // tests/test_gpu_spiht.py::test_random_geometries_and_budgets)
        const uint64_t chunk_slack = 16384;
        lip = std::min(lip, roots + mb + chunk_slack);
        lsp = std::min(lsp, mb / 2 + 1 + chunk_slack);
        lis = std::min(lis, roots + 4 * mb + chunk_slack);
    }
    // multiples of 64 entries: every slot's lists start 256-byte aligned (the encoder reads entry pairs as 8-byte loads)
    caps->lip = (uint32_t)std::min<uint64_t>((lip + 127) & ~63ull, 0xFFFFFFC0ull);
    caps->lsp = (uint32_t)std::min<uint64_t>((lsp + 127) & ~63ull, 0xFFFFFFC0ull);
    caps->lis = (uint32_t)std::min<uint64_t>((lis + 127) & ~63ull, 0xFFFFFFC0ull);
    caps->pad = 0;
    if (nodes_out) *nodes_out = nodes;
}

// ------------------------------------------------------------------------------------------------
// list coder plumbing
// ------------------------------------------------------------------------------------------------

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// carve per-slot list scratch out of ctx->lists; returns pointers
struct ListPtrs {
    uint32_t *lip0, *lip1, *lsp, *lis0, *lis1, *lis2;
    int32_t *lsp_val;
};

static int alloc_lists(spiht_ctx *ctx, const ListCaps &caps, int want_slots, bool decoder, int *nslots, ListPtrs *p) {
    size_t per_slot = ((size_t)caps.lip * 2 + (size_t)caps.lsp * (decoder ? 2 : 1) + (size_t)caps.lis * 3) * 4;
    // keep the scratch under ~24 GiB
    const size_t budget = (size_t)24 << 30;
    int slots = want_slots;
    if ((size_t)slots * per_slot > budget) slots = (int)std::max<size_t>(1, budget / per_slot);
    size_t s_lip = align256((size_t)caps.lip * 4 * slots), s_lsp = align256((size_t)caps.lsp * 4 * slots),
           s_lis = align256((size_t)caps.lis * 4 * slots);
    size_t total = 2 * s_lip + (decoder ? 2 : 1) * s_lsp + 3 * s_lis;
    ctx->last_dec_valid = false;  // the lists get a new user
    CHK(ensure(ctx, ctx->lists, total));
    char *base = (char *)ctx->lists.p;
    p->lip0 = (uint32_t *)base; base += s_lip;
    p->lip1 = (uint32_t *)base; base += s_lip;
    p->lsp = (uint32_t *)base; base += s_lsp;
    p->lsp_val = nullptr;
    if (decoder) { p->lsp_val = (int32_t *)base; base += s_lsp; }
    p->lis0 = (uint32_t *)base; base += s_lis;
    p->lis1 = (uint32_t *)base; base += s_lis;
    p->lis2 = (uint32_t *)base; base += s_lis;
    *nslots = slots;
    return SPIHT_OK;
}

static int encode_lists_device(spiht_ctx *ctx, const Geom &g, const int32_t *d_x, const uint8_t *d_dmsb,
                               const uint8_t *d_lmsb, const uint32_t *d_maxabs, int B, uint64_t max_bits,
                               const ListCaps &caps, int nslots, const ListPtrs &lp, uint8_t *d_out, uint64_t slot_stride,
                               uint64_t *d_nbits, uint8_t *d_maxn);

// Encode B device-resident coefficient arrays.  max_bits already validated; queues work on ctx->stream.
int encode_device(spiht_ctx *ctx, const Geom &g, const int32_t *d_x, int B, uint64_t max_bits_in, uint8_t *d_out, uint64_t slot_stride,
                  uint64_t *d_nbits, uint8_t *d_maxn, bool have_maxabs) {
    if (slot_stride % 4 != 0) return SPIHT_ERR_ARG;
    if ((uint64_t)B * (uint64_t)g.c > 65535ull) return SPIHT_ERR_ARG;
    const uint64_t max_bits = max_bits_in == 0 ? SPIHT_MAX_BITS_UNLIMITED : max_bits_in;  // encoder_decoder.rs:196
    CHK(ensure(ctx, ctx->dmsb, (size_t)B * g.n));
    CHK(ensure(ctx, ctx->lmsb, (size_t)B * g.n));
    CHK(ensure(ctx, ctx->maxabs, (size_t)B * 4));
    ListCaps caps;
    list_caps(g, std::min<uint64_t>(max_bits, slot_stride * 8), &caps, nullptr);
    int nslots = 0;
    ListPtrs lp;
    CHK(alloc_lists(ctx, caps, std::min(B, ctx->num_cu), false, &nslots, &lp));
    if (!have_maxabs) {
        StageTimer t(ctx, ST_ABSMAX);
        LAUNCHCHK(spiht_launch_absmax(d_x, B, g.n, (uint32_t *)ctx->maxabs.p, ctx->stream));
    }
    {
        StageTimer t(ctx, ST_PYRAMID);
        LAUNCHCHK(spiht_launch_pyramid(&g, B, d_x, (uint8_t *)ctx->dmsb.p, (uint8_t *)ctx->lmsb.p, ctx->stream));
    }
    return encode_lists_device(ctx, g, d_x, (const uint8_t *)ctx->dmsb.p, (const uint8_t *)ctx->lmsb.p,
                               (const uint32_t *)ctx->maxabs.p, B, max_bits, caps, nslots, lp, d_out, slot_stride, d_nbits,
                               d_maxn);
}

// the list-coding half of the encoder: coefficient arrays + their significance pyramid -> streams
static int encode_lists_device(spiht_ctx *ctx, const Geom &g, const int32_t *d_x, const uint8_t *d_dmsb,
                               const uint8_t *d_lmsb, const uint32_t *d_maxabs, int B, uint64_t max_bits,
                               const ListCaps &caps, int nslots, const ListPtrs &lp, uint8_t *d_out, uint64_t slot_stride,
                               uint64_t *d_nbits, uint8_t *d_maxn) {
    EncArgs a;
    memset(&a, 0, sizeof(a));
    a.g = g;
    a.caps = caps;
    a.B = B;
    a.nslots = nslots;
    a.x = d_x;
    a.dmsb = d_dmsb;
    a.lmsb = d_lmsb;
    a.maxabs = d_maxabs;
    a.max_bits = max_bits;
    a.out = d_out;
    a.slot_stride = slot_stride;
    a.out_nbits = d_nbits;
    a.out_maxn = d_maxn;
    a.lip0 = lp.lip0; a.lip1 = lp.lip1; a.lsp = lp.lsp; a.lis0 = lp.lis0; a.lis1 = lp.lis1; a.lis2 = lp.lis2;
    a.err = (uint32_t *)ctx->err.p;
    memcpy(a.log2_thresh, ctx->log2_thresh, sizeof(a.log2_thresh));
    // The slots come out zero past the stream's last bit.  k_encode clears its image's slot itself before it writes into it:
    // a fill queued in front of the kernel was seen to land on words the kernel had already written when the stream had
    // just waited for events of two other streams (the pipeline's second step), which cost a stream its first few hundred
    // bytes now and then.
    // Few images per call: each on a group of G workgroups (encode_wide.hip) instead of one -- a single image's list coding
    // is bound by the one CU it runs on.  Every workgroup of a group must be resident at once: B * G within what the device
    // holds of that kernel (asked of the runtime once per context).
    int G = (int)std::min<uint64_t>(64, std::max<uint64_t>(2, g.n >> 18));
    if (ctx->opt_wide_g > 0) G = ctx->opt_wide_g;
    if (ctx->wide_per_cu < 0) ctx->wide_per_cu = std::max(0, spiht_wide_groups_per_cu());
    G = std::min(G, std::max(1, ctx->wide_per_cu) * ctx->num_cu / std::max(B, 1));
    if (ctx->opt_wide_encode && G >= 2 && (g.n >= (1u << 18) || ctx->opt_wide_encode >= 2) && nslots >= B) {
        WideArgs w;
        const uint64_t cap_max = std::max<uint64_t>(caps.lip, std::max<uint64_t>(caps.lsp, caps.lis));
        w.maxchunks = (uint32_t)(cap_max / 2048 + 2);  // (the smaller of the two chunk sizes: WIDE_U * 1024 entries)
        w.G = (uint32_t)G;
        w.solo = (uint32_t)ctx->opt_wide_solo;
        w.pad = 0;
        const size_t ctl_bytes = align256((size_t)B * sizeof(WideCtl)), desc_bytes = (size_t)B * 2 * w.maxchunks * 4 * 8;
        CHK(ensure(ctx, ctx->widebuf, ctl_bytes + desc_bytes));
        w.ctl = (WideCtl *)ctx->widebuf.p;
        w.desc = (uint64_t *)((char *)ctx->widebuf.p + ctl_bytes);
        {  // its chunks OR their first and last word into the slot: the slots start all-zero
            StageTimer t(ctx, ST_MEMSET);
            HIPCHK(hipMemsetAsync(d_out, 0, (size_t)B * slot_stride, ctx->stream));
        }
        StageTimer t(ctx, ST_ENC_LISTS);
        HIPCHK(hipMemsetAsync(ctx->widebuf.p, 0, ctl_bytes + desc_bytes, ctx->stream));
        ctx->wide_last_groups = B;
        if (ctx->opt_wide_encode == 3) {  // tests: every group finds itself given up -> k_encode<redo> codes every image
            HIPCHK(hipStreamSynchronize(ctx->stream));  // (an earlier launch may still copy from the vector)
            WideCtl gave_up;
            memset(&gave_up, 0, sizeof(gave_up));
            gave_up.bad = 2u;
            ctx->wide_forced.assign((size_t)B, gave_up);
            HIPCHK(hipMemcpyAsync(ctx->widebuf.p, ctx->wide_forced.data(), (size_t)B * sizeof(WideCtl), hipMemcpyHostToDevice, ctx->stream));
        }
        // The workgroups of a group wait for one another, so a grid should become resident as a whole: two such grids of
        // different contexts, each half resident on a full GPU, would wait for each other.  One at a time per device, by an
        // event chain between the contexts' streams (the host does not block).  What that chain cannot see -- another
        // process, another kernel holding the CUs -- ends in the group giving up after a bounded wait (encode_wide.hip), and
        // the launch of k_encode<redo> right behind codes exactly those images with one workgroup each: same bits, later.
        static std::mutex wide_mu;
        static hipEvent_t wide_last[64] = {};
        {
            std::lock_guard<std::mutex> wl(wide_mu);
            hipEvent_t &ev = wide_last[ctx->device & 63];
            if (ev) HIPCHK(hipStreamWaitEvent(ctx->stream, ev, 0));
            else HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            LAUNCHCHK(spiht_launch_encode_wide(&a, &w, B, ctx->stream));
            HIPCHK(hipEventRecord(ev, ctx->stream));
        }
        a.redo = w.ctl;
        a.nslots = B;
        LAUNCHCHK(spiht_launch_encode(&a, ctx->stream));
        return SPIHT_OK;
    }
    {
        StageTimer t(ctx, ST_ENC_LISTS);
        LAUNCHCHK(spiht_launch_encode(&a, ctx->stream));
    }
    return SPIHT_OK;
}

int decode_device(spiht_ctx *ctx, const Geom &g, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                  const uint8_t *d_maxn, int B, int32_t *d_out, uint32_t *d_tr_ent, uint8_t *d_tr_act, uint64_t tr_stride,
                  bool zero_out, DecArgs *args_out, const L1Flags *fl) {
    if (slot_stride % 4 != 0) return SPIHT_ERR_ARG;
    if (slot_stride * 8 >= 0xFFFFFF00ull) return SPIHT_ERR_TOO_LARGE;
    ListCaps caps;
    list_caps(g, slot_stride * 8, &caps, nullptr);
    int nslots = 0;
    ListPtrs lp;
    CHK(alloc_lists(ctx, caps, std::min(B, ctx->num_cu * 8), true, &nslots, &lp));
    if (zero_out) {
        StageTimer t(ctx, ST_MEMSET);
        HIPCHK(hipMemsetAsync(d_out, 0, (size_t)B * g.n * 4, ctx->stream));
    }
    DecArgs a;
    memset(&a, 0, sizeof(a));
    a.g = g;
    a.caps = caps;
    a.B = B;
    a.nslots = nslots;
    a.data = d_data;
    a.slot_stride = slot_stride;
    a.nbytes = d_nbytes;
    a.max_n = d_maxn;
    a.out = d_out;
    a.lip0 = lp.lip0; a.lip1 = lp.lip1; a.lsp_idx = lp.lsp; a.lsp_val = lp.lsp_val;
    a.lis0 = lp.lis0; a.lis1 = lp.lis1; a.lis2 = lp.lis2;
    a.err = (uint32_t *)ctx->err.p;
    a.tr_ent = d_tr_ent; a.tr_act = d_tr_act; a.tr_stride = tr_stride;
    if (fl && fl->p) {  // (zero-filled here: the decoder only ever sets words)
        a.fl = *fl;
        const size_t wb = (size_t)B * g.c * fl->gy * fl->gx * 4;
        const bool one = fl->rows == fl->p + wb / 4;  // words and row words laid out as one buffer: one fill
        HIPCHK(hipMemsetAsync(fl->p, 0, one ? 2 * wb : wb, ctx->stream));
        if (fl->rows && !one) HIPCHK(hipMemsetAsync(fl->rows, 0, wb, ctx->stream));
    }
    if (args_out) {  // the caller wants to undo the scatter later: one LSP length per slot
        CHK(ensure(ctx, ctx->lspcnt, (size_t)nslots * 4));
        a.lsp_count = (uint32_t *)ctx->lspcnt.p;
    }
    {
        StageTimer t(ctx, ST_DEC_LISTS);
        LAUNCHCHK(ctx->dec_waves == 8 ? spiht_launch_decode_w8(&a, ctx->stream) : spiht_launch_decode(&a, ctx->stream));
    }
    if (args_out) *args_out = a;
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// L2 boundary, single image, host buffers
// ------------------------------------------------------------------------------------------------

extern "C" int spiht_encode_bound(int64_t c, int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, uint32_t max_abs,
                                  uint64_t max_bits, uint64_t *bound_bytes) {
    if (!bound_bytes) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    uint64_t bits = bound_bits(g, max_abs);
    if (max_bits != 0) bits = std::min(bits, max_bits);
    *bound_bytes = ((bits + 7) / 8 + 3) & ~3ull;
    return SPIHT_OK;
}

// The result of a single encode (ctx->out, ctx->nbits, ctx->maxn) to the host; waits
int read_encoded(spiht_ctx *ctx, uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n) {
    uint64_t nbits = 0;
    uint8_t mn = 0;
    HIPCHK(hipMemcpyAsync(&nbits, ctx->nbits.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&mn, ctx->maxn.p, 1, hipMemcpyDeviceToHost, ctx->stream));
    CHK(take_err(ctx));  // synchronises
    *out_nbits = nbits;
    *max_n = mn;
    const uint64_t nbytes = (nbits + 7) / 8;
    if (nbytes > out_cap) return SPIHT_ERR_CAPACITY;
    if (nbytes) {
        StageTimer t(ctx, ST_D2H);
        HIPCHK(hipMemcpyAsync(out, ctx->out.p, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}

// One host stream for the decoder: its bytes into ctx->data, a slot of *slot bytes whose last word is zeroed first (the
// bytes past the stream in it), its length and magnitude into ctx->nbytes / ctx->maxn; waits, and returns the error an
// earlier batched call has latched, if any (take_err)
int stage_stream(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, uint64_t *slot) {
    *slot = std::max<uint64_t>(4, (nbytes + 3) & ~3ull);
    CHK(ensure(ctx, ctx->data, *slot));
    CHK(ensure(ctx, ctx->nbytes, 8));
    CHK(ensure(ctx, ctx->maxn, 4));
    CHK(take_err(ctx));
    StageTimer t(ctx, ST_H2D);
    HIPCHK(hipMemsetAsync((char *)ctx->data.p + (*slot - 4), 0, 4, ctx->stream));
    if (nbytes) HIPCHK(hipMemcpyAsync(ctx->data.p, data, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->nbytes.p, &nbytes, 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->maxn.p, &n, 1, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // &nbytes / &n are stack temporaries
    return SPIHT_OK;
}

extern "C" int spiht_encode_i32(spiht_ctx *ctx, const int32_t *x, int64_t c, int64_t h, int64_t w, int64_t stride_c,
                                int64_t stride_h, int64_t stride_w, int64_t ll_h, int64_t ll_w, uint64_t max_bits,
                                uint8_t *out, uint64_t out_cap, uint64_t *out_nbits, uint8_t *max_n) {
    if (!ctx || !out_nbits || !max_n || (!out && out_cap)) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (!x) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    // gather the strided view into a contiguous staging buffer (lib.rs:27 takes any strides)
    std::vector<int32_t> stage;
    const int32_t *src = x;
    uint32_t max_abs = 0;
    const bool contiguous = stride_w == 1 && stride_h == w && stride_c == h * w;
    if (!contiguous) {
        stage.resize(g.n);
        size_t t = 0;
        for (int64_t k = 0; k < c; k++)
            for (int64_t i = 0; i < h; i++) {
                const int32_t *row = x + k * stride_c + i * stride_h;
                for (int64_t j = 0; j < w; j++) stage[t++] = row[j * stride_w];
            }
        src = stage.data();
    }
    for (size_t t = 0; t < g.n; t++) {
        int32_t v = src[t];
        uint32_t m = v < 0 ? (uint32_t)(-(int64_t)v) : (uint32_t)v;
        if (m > max_abs) max_abs = m;
    }
    if (max_abs >= (1u << 30)) return SPIHT_ERR_MAGNITUDE;
    uint64_t bits = bound_bits(g, max_abs);
    if (max_bits != 0) bits = std::min(bits, max_bits);
    if (bits >= 0xFFFFFF00ull * 8ull) return SPIHT_ERR_TOO_LARGE;
    const uint64_t slot = std::max<uint64_t>(4, ((bits + 7) / 8 + 3) & ~3ull);
    CHK(ensure(ctx, ctx->x, (size_t)g.n * 4));
    CHK(ensure(ctx, ctx->out, slot));
    CHK(ensure(ctx, ctx->nbits, 8));
    CHK(ensure(ctx, ctx->maxn, 4));
    CHK(take_err(ctx));
    {
        StageTimer t(ctx, ST_H2D);
        HIPCHK(hipMemcpyAsync(ctx->x.p, src, (size_t)g.n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    CHK(encode_device(ctx, g, (const int32_t *)ctx->x.p, 1, max_bits, (uint8_t *)ctx->out.p, slot,
                      (uint64_t *)ctx->nbits.p, (uint8_t *)ctx->maxn.p));
    return read_encoded(ctx, out, out_cap, out_nbits, max_n);
}

extern "C" int spiht_decode_i32(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t h,
                                int64_t w, int64_t ll_h, int64_t ll_w, int32_t *out) {
    if (!ctx || !out || (!data && nbytes)) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (n > 30) return SPIHT_ERR_MAGNITUDE;
    if (nbytes * 8 >= 0xFFFFFF00ull) return SPIHT_ERR_TOO_LARGE;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->rec, (size_t)g.n * 4));
    uint64_t slot;
    CHK(stage_stream(ctx, data, nbytes, n, &slot));
    CHK(decode_device(ctx, g, (const uint8_t *)ctx->data.p, slot, (const uint64_t *)ctx->nbytes.p,
                      (const uint8_t *)ctx->maxn.p, 1, (int32_t *)ctx->rec.p));
    CHK(take_err(ctx));
    {
        StageTimer t(ctx, ST_D2H);
        HIPCHK(hipMemcpyAsync(out, ctx->rec.p, (size_t)g.n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}

// number of generations below the LL block that exist in the index-based tree (encoder_decoder.rs:43-75): the
// shallowest first-generation nodes are (0, ll_w) and (ll_h, 0); a node has offspring iff 2i+1 < h && 2j+1 < w
static int tree_generations(const Geom &g) {
    int best = 1;
    const int64_t cand[2][2] = {{0, g.ll_w}, {g.ll_h, 0}};
    for (auto &cd : cand) {
        int t = 1;
        while (t < 40 && 2 * (cd[0] << (t - 1)) + 1 < g.h && 2 * (cd[1] << (t - 1)) + 1 < g.w) t++;
        best = std::max(best, t);
    }
    return best;
}

// The decoder's trace and the sort behind it, in ctx->trace: ent[rows] u32 | 4 x u32[rows] sort buffers | act[rows] u8 |
// in_bytes of the caller's own input | sort temp.  One stream: rows = one per bit of the nbytes stream, and one more.
struct TraceScratch {
    uint64_t rows;
    uint32_t *ent, *k0, *v0, *k1, *v1;
    uint8_t *act;
    char *in, *tmp;
    size_t tmp_bytes;
    // what the metadata and budget kernels read of it (and of the stream at d_data)
    MetaArgs meta_args(const Geom &g, const void *d_data) const {
        MetaArgs ma;
        memset(&ma, 0, sizeof(ma));
        ma.g = g;
        ma.rows = rows;
        ma.tr_ent = ent;
        ma.tr_act = act;
        ma.data = (const uint8_t *)d_data;
        ma.skey = k1;
        ma.spos = v1;
        return ma;
    }
};
static int trace_layout(spiht_ctx *ctx, uint64_t rows, size_t tmp_bytes, size_t in_bytes, TraceScratch *t) {
    t->rows = rows;
    t->tmp_bytes = tmp_bytes;
    const size_t r4 = align256(t->rows * 4), o_act = 5 * r4, o_in = o_act + align256(t->rows), o_tmp = o_in + align256(in_bytes);
    CHK(ensure(ctx, ctx->trace, o_tmp + align256(t->tmp_bytes)));
    char *tb = (char *)ctx->trace.p;
    t->ent = (uint32_t *)tb;
    t->k0 = (uint32_t *)(tb + r4);
    t->v0 = (uint32_t *)(tb + 2 * r4);
    t->k1 = (uint32_t *)(tb + 3 * r4);
    t->v1 = (uint32_t *)(tb + 4 * r4);
    t->act = (uint8_t *)(tb + o_act);
    t->in = tb + o_in;
    t->tmp = tb + o_tmp;
    return SPIHT_OK;
}
static int trace_scratch(spiht_ctx *ctx, uint64_t nbytes, size_t in_bytes, TraceScratch *t) {
    size_t tmp_bytes = 0;
    if (spiht_meta_sort_temp_bytes(nbytes * 8 + 1, &tmp_bytes) != 0) return SPIHT_ERR_INTERNAL;
    return trace_layout(ctx, nbytes * 8 + 1, tmp_bytes, in_bytes, t);
}

// top_slice / other_slices of decode_with_metadata as int32 {top[4], [level][3][4]}: a value outside [0, 2^31) is
// SPIHT_ERR_ARG, a reversed slice SPIHT_ERR_SHAPE (usize underflow in end - start, encoder_decoder.rs:606-608)
static int meta_slices(const int64_t *top_slice, const int64_t *other_slices, int64_t level, std::vector<int32_t> *out) {
    std::vector<int32_t> &sl = *out;
    sl.resize(4 + (size_t)level * 12);
    for (size_t t = 0; t < sl.size(); t++) {
        const int64_t v = t < 4 ? top_slice[t] : other_slices[t - 4];
        if (v < 0 || v > 0x7FFFFFFF) return SPIHT_ERR_ARG;
        sl[t] = (int32_t)v;
    }
    for (size_t t = 4; t < sl.size(); t += 4)
        if (sl[t + 1] < sl[t] || sl[t + 3] < sl[t + 2]) return SPIHT_ERR_SHAPE;
    return SPIHT_OK;
}

extern "C" int spiht_decode_with_metadata_i32(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c,
                                              int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, const int64_t *top_slice,
                                              const int64_t *other_slices, int64_t level, int32_t *out, int32_t *meta) {
    if (!ctx || !out || !meta || (!data && nbytes) || !top_slice || level < 0 || (level > 0 && !other_slices))
        return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (g.n >= (1u << 28)) return SPIHT_ERR_TOO_LARGE;  // list entries carry the filter in bits 28-29
    if (n > 30) return SPIHT_ERR_MAGNITUDE;
    if (nbytes * 8 >= 0xFFFFFF00ull) return SPIHT_ERR_TOO_LARGE;
    if (level > 255 || tree_generations(g) > level) return SPIHT_ERR_SHAPE;  // other_slices[depth_i] out of bounds (:603)
    std::vector<int32_t> sl;
    CHK(meta_slices(top_slice, other_slices, level, &sl));
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    TraceScratch tr;
    CHK(trace_scratch(ctx, nbytes, sl.size() * 4, &tr));
    CHK(ensure(ctx, ctx->rec, (size_t)g.n * 4));
    CHK(ensure(ctx, ctx->meta, tr.rows * 32));
    uint64_t slot;
    CHK(stage_stream(ctx, data, nbytes, n, &slot));
    {
        StageTimer t(ctx, ST_H2D);
        HIPCHK(hipMemcpyAsync(tr.in, sl.data(), sl.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemsetAsync(tr.act, TR_NONE, tr.rows, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));  // (a vector temporary)
    }
    CHK(decode_device(ctx, g, (const uint8_t *)ctx->data.p, slot, (const uint64_t *)ctx->nbytes.p,
                      (const uint8_t *)ctx->maxn.p, 1, (int32_t *)ctx->rec.p, tr.ent, tr.act, tr.rows));
    MetaArgs ma = tr.meta_args(g, ctx->data.p);
    ma.level = (int32_t)level;
    ma.slices = (const int32_t *)tr.in;
    ma.meta = (int32_t *)ctx->meta.p;
    LAUNCHCHK(spiht_launch_metadata(&ma, tr.k0, tr.v0, tr.k1, tr.v1, tr.tmp, tr.tmp_bytes, ctx->stream));
    CHK(take_err(ctx));
    {
        StageTimer t(ctx, ST_D2H);
        HIPCHK(hipMemcpyAsync(out, ctx->rec.p, (size_t)g.n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(meta, ctx->meta.p, tr.rows * 32, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}

// Progressive decoding of ONE stream to K bit budgets (ascending) from one walk: out[kk] = what decode() returns for the
// first budgets[kk] bits of the stream (a budget past the end: the whole stream).  The pattern of the reference's
// make_gif.py:46-61 (`decode(original_bytes[:byte_len])` per frame), SURVEY.md 8 f-3: the K walks of K prefixes become
// one walk with the trace of decode_with_metadata, and every tree node replays its own operations once
// (metadata.hip: k_budget_fold).  d_out: device int32 [K, c, h, w], zero-filled here.  Asynchronous apart from the upload.
extern "C" int spiht_decode_budgets_dev_i32(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t h,
                                            int64_t w, int64_t ll_h, int64_t ll_w, const uint64_t *budgets_bits, int64_t K,
                                            int32_t *d_out) {
    if (!ctx || !d_out || (!data && nbytes) || !budgets_bits || K < 1 || K > 65535) return SPIHT_ERR_ARG;
    for (int64_t k = 1; k < K; k++)
        if (budgets_bits[k] < budgets_bits[k - 1]) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (g.n >= (1u << 28)) return SPIHT_ERR_TOO_LARGE;
    if (n > 30) return SPIHT_ERR_MAGNITUDE;
    if (nbytes * 8 >= 0xFFFFFF00ull) return SPIHT_ERR_TOO_LARGE;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    TraceScratch tr;
    CHK(trace_scratch(ctx, nbytes, (size_t)K * 8, &tr));
    CHK(ensure(ctx, ctx->rec, (size_t)g.n * 4));
    uint64_t slot;
    CHK(stage_stream(ctx, data, nbytes, n, &slot));
    {
        StageTimer t(ctx, ST_H2D);
        HIPCHK(hipMemcpyAsync(tr.in, budgets_bits, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemsetAsync(tr.act, TR_NONE, tr.rows, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));  // (the caller's array)
    }
    HIPCHK(hipMemsetAsync(d_out, 0, (size_t)K * g.n * 4, ctx->stream));
    CHK(decode_device(ctx, g, (const uint8_t *)ctx->data.p, slot, (const uint64_t *)ctx->nbytes.p,
                      (const uint8_t *)ctx->maxn.p, 1, (int32_t *)ctx->rec.p, tr.ent, tr.act, tr.rows));
    const MetaArgs ma = tr.meta_args(g, ctx->data.p);
    LAUNCHCHK(spiht_launch_budget_fold(&ma, tr.k0, tr.v0, tr.k1, tr.v1, tr.tmp, tr.tmp_bytes, (const uint64_t *)tr.in, (int)K,
                                       d_out, ctx->stream));
    return SPIHT_OK;
}

// ... with the K arrays brought to the host (int32 [K, c, h, w]); synchronous.
extern "C" int spiht_decode_budgets_i32(spiht_ctx *ctx, const uint8_t *data, uint64_t nbytes, uint8_t n, int64_t c, int64_t h,
                                        int64_t w, int64_t ll_h, int64_t ll_w, const uint64_t *budgets_bits, int64_t K,
                                        int32_t *out) {
    if (!ctx || !out || K < 1) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)K * g.n * 4;
    CHK(ensure(ctx, ctx->hrec, bytes));
    CHK(spiht_decode_budgets_dev_i32(ctx, data, nbytes, n, c, h, w, ll_h, ll_w, budgets_bits, K, (int32_t *)ctx->hrec.p));
    CHK(take_err(ctx));
    {
        StageTimer t(ctx, ST_D2H);
        HIPCHK(hipMemcpyAsync(out, ctx->hrec.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}

// ------------------------------------------------------------------------------------------------
// batched, device-resident
// ------------------------------------------------------------------------------------------------

extern "C" int spiht_encode_batch_i32(spiht_ctx *ctx, const int32_t *d_x, int64_t B, int64_t c, int64_t h, int64_t w,
                                      int64_t ll_h, int64_t ll_w, uint64_t max_bits, uint8_t *d_out,
                                      uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n) {
    if (!ctx || !d_x || !d_out || !d_nbits || !d_max_n || B < 0) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (c > 65535) return SPIHT_ERR_TOO_LARGE;  // (one array's planes go into grid.z of the pyramid's launches)
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    return batch_chunks(B, c, [&](int64_t b0, int nb) -> int {
        return encode_device(ctx, g, d_x + (size_t)b0 * g.n, nb, max_bits, d_out + (size_t)b0 * slot_stride, slot_stride,
                             d_nbits + b0, d_max_n + b0);
    });  // asynchronous: errors surface in spiht_ctx_synchronize()
}

extern "C" int spiht_decode_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                      const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c, int64_t h,
                                      int64_t w, int64_t ll_h, int64_t ll_w, int32_t *d_out) {
    if (!ctx || !d_data || !d_nbytes || !d_max_n || !d_out || B < 0) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    CHK(decode_device(ctx, g, d_data, slot_stride, d_nbytes, d_max_n, (int)B, d_out));
    return SPIHT_OK;  // asynchronous: errors surface in spiht_ctx_synchronize()
}

// decode_with_metadata of B device-resident streams.  In chunks of images: per chunk the traced decode of every image (trace
// of image b at b * tr_stride), then the rows, the sort and the fold of metadata.hip over the chunk.  The chunk's trace and
// sort buffers (21 bytes per record) stay within META_CHUNK_BYTES unless one image alone needs more; the keys b * n + node
// (or the record indices) stay 32-bit.  The slices go to the kernels by value: nothing is read from the host afterwards.
#define META_CHUNK_BYTES ((size_t)2 << 30)
extern "C" int spiht_decode_with_metadata_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                    const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                    int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, const int64_t *top_slice,
                                                    const int64_t *other_slices, int64_t level, int32_t *d_out, int32_t *d_meta,
                                                    uint64_t meta_rows) {
    if (!ctx || !d_data || !d_nbytes || !d_max_n || !d_meta || B < 0 || !top_slice || level < 0 || (level > 0 && !other_slices))
        return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (g.n >= (1u << 28)) return SPIHT_ERR_TOO_LARGE;  // list entries carry the filter in bits 28-29
    if (slot_stride % 4 != 0) return SPIHT_ERR_ARG;
    if (slot_stride >= (1ull << 28)) return SPIHT_ERR_TOO_LARGE;  // a chunk's record indices are 32-bit (and under 2^31)
    const uint64_t tr_stride = 8 * slot_stride + 1;
    if (meta_rows < tr_stride) return SPIHT_ERR_ARG;
    if (level > 255 || tree_generations(g) > level) return SPIHT_ERR_SHAPE;  // other_slices[depth_i] out of bounds (:603)
    std::vector<int32_t> sl;
    CHK(meta_slices(top_slice, other_slices, level, &sl));
    if (B == 0) return SPIHT_OK;
    MetaBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.g = g;
    a.level = (int32_t)level;
    a.tr_stride = (uint32_t)std::max<uint64_t>(tr_stride, 2);  // (FastDiv divides by 2 or more)
    a.div_tr = fastdiv_make(a.tr_stride);
    a.slot_stride = slot_stride;
    a.meta_rows = meta_rows;
    // the kernels read the levels the tree reaches (tree_generations <= 28 when n < 2^28)
    memcpy(a.slices, sl.data(), std::min<size_t>(sl.size(), 4 + 12 * META_MAX_GEN) * 4);
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    int64_t chunk = 65535 / c;                                             // the decoder's slots, the kernels' grid.y
    chunk = std::min<int64_t>(chunk, (int64_t)(0x80000000ull / a.tr_stride));  // record indices
    chunk = std::min<int64_t>(chunk, (int64_t)(0xFFFFFFFFull / g.n));          // keys b * n + node, and nb * n for "none"
    chunk = std::min<int64_t>(chunk, (int64_t)std::max<size_t>(1, META_CHUNK_BYTES / ((size_t)a.tr_stride * 21)));
    if (ctx->opt_meta_chunk > 0) chunk = std::min<int64_t>(chunk, ctx->opt_meta_chunk);
    chunk = std::max<int64_t>(chunk, 1);
    if (!d_out) CHK(ensure(ctx, ctx->rec, (size_t)std::min<int64_t>(chunk, B) * g.n * 4));
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (int)std::min<int64_t>(chunk, B - b0);
        a.nb = nb;
        a.key_none = (uint32_t)nb * g.n;
        size_t tmp_bytes = 0;
        if (spiht_meta_batch_sort_temp_bytes(&a, &tmp_bytes) != 0) return SPIHT_ERR_INTERNAL;
        TraceScratch tr;
        CHK(trace_layout(ctx, (uint64_t)nb * a.tr_stride, tmp_bytes, 0, &tr));
        HIPCHK(hipMemsetAsync(tr.act, TR_NONE, tr.rows, ctx->stream));
        const uint8_t *data = d_data + (size_t)b0 * slot_stride;
        int32_t *rec = d_out ? d_out + (size_t)b0 * g.n : (int32_t *)ctx->rec.p;
        CHK(decode_device(ctx, g, data, slot_stride, d_nbytes + b0, d_max_n + b0, nb, rec, tr.ent, tr.act, a.tr_stride));
        a.tr_ent = tr.ent;
        a.tr_act = tr.act;
        a.data = data;
        a.nbytes = d_nbytes + b0;
        a.meta = d_meta + (size_t)b0 * meta_rows * 8;
        a.skey = tr.k1;
        a.spos = tr.v1;
        LAUNCHCHK(spiht_launch_metadata_batch(&a, tr.k0, tr.v0, tr.k1, tr.v1, tr.tmp, tr.tmp_bytes, ctx->stream));
    }
    return SPIHT_OK;  // asynchronous: errors surface in spiht_ctx_synchronize()
}

extern "C" int spiht_pyramid_batch_i32(spiht_ctx *ctx, const int32_t *d_x, int64_t B, int64_t c, int64_t h, int64_t w,
                                       int64_t ll_h, int64_t ll_w, uint8_t *d_dmsb, uint8_t *d_lmsb,
                                       uint32_t *d_maxabs) {
    if (!ctx || !d_x || !d_dmsb || !d_lmsb || B < 0) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (B == 0) return SPIHT_OK;
    if ((uint64_t)B * (uint64_t)g.c > 65535ull) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    if (d_maxabs) {  // null: the caller has max|x| already (spiht_dwt_pyramid_batch_f64 without the pyramid)
        StageTimer t(ctx, ST_ABSMAX);
        LAUNCHCHK(spiht_launch_absmax(d_x, (int)B, g.n, d_maxabs, ctx->stream));
    }
    {
        StageTimer t(ctx, ST_PYRAMID);
        LAUNCHCHK(spiht_launch_pyramid(&g, (int)B, d_x, d_dmsb, d_lmsb, ctx->stream));
    }
    return SPIHT_OK;
}

extern "C" int spiht_encode_lists_batch_i32(spiht_ctx *ctx, const int32_t *d_x, const uint8_t *d_dmsb,
                                            const uint8_t *d_lmsb, const uint32_t *d_maxabs, int64_t B, int64_t c,
                                            int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, uint64_t max_bits_in,
                                            uint8_t *d_out, uint64_t slot_stride, uint64_t *d_nbits, uint8_t *d_max_n) {
    if (!ctx || !d_x || !d_dmsb || !d_lmsb || !d_maxabs || !d_out || !d_nbits || !d_max_n || B < 0) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    if (B == 0) return SPIHT_OK;
    if (slot_stride % 4 != 0) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t max_bits = max_bits_in == 0 ? SPIHT_MAX_BITS_UNLIMITED : max_bits_in;
    ListCaps caps;
    list_caps(g, std::min<uint64_t>(max_bits, slot_stride * 8), &caps, nullptr);
    return batch_chunks(B, c, [&](int64_t b0, int nb) -> int {
        int nslots = 0;
        ListPtrs lp;
        CHK(alloc_lists(ctx, caps, std::min(nb, ctx->num_cu), false, &nslots, &lp));
        return encode_lists_device(ctx, g, d_x + (size_t)b0 * g.n, d_dmsb + (size_t)b0 * g.n, d_lmsb + (size_t)b0 * g.n,
                                   d_maxabs + b0, nb, max_bits, caps, nslots, lp, d_out + (size_t)b0 * slot_stride, slot_stride,
                                   d_nbits + b0, d_max_n + b0);
    });
}

static int decode_lists_batch(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride, const uint64_t *d_nbytes,
                              const uint8_t *d_max_n, int64_t B, const Geom &g, int32_t *d_out_zeroed, const L1Flags *fl) {
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DecArgs da;
    CHK(decode_device(ctx, g, d_data, slot_stride, d_nbytes, d_max_n, (int)B, d_out_zeroed, nullptr, nullptr, 0, false, &da, fl));
    ctx->last_dec = da;
    ctx->last_dec_valid = da.nslots >= (int)B;  // otherwise slots were reused inside the launch
    return SPIHT_OK;
}
extern "C" int spiht_decode_lists_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                            const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                            int64_t h, int64_t w, int64_t ll_h, int64_t ll_w, int32_t *d_out_zeroed) {
    if (!ctx || !d_data || !d_nbytes || !d_max_n || !d_out_zeroed || B < 0) return SPIHT_ERR_ARG;
    Geom g;
    CHK(make_geom(c, h, w, ll_h, ll_w, &g));
    return decode_lists_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, g, d_out_zeroed, nullptr);
}
// The same for the coefficient arrays of B images of H x W pixels (the geometry spiht_geometry gives), leaving in d_flags
// (spiht_l1_flags_words(...) x B words; zero-filled by this call) the occupancy of the inverse transform's level-1 tiles
// for spiht_dequant_idwt_flags_batch_f64.  d_flags == NULL or a geometry without flags: as spiht_decode_lists_batch_i32.
extern "C" int spiht_decode_lists_flags_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                  const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                  int64_t H, int64_t W, int wavelet, int mode, int level, int32_t *d_out_zeroed,
                                                  uint32_t *d_flags) {
    return spiht_decode_lists_rows_batch_i32(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, c, H, W, wavelet, mode, level,
                                             d_out_zeroed, d_flags, nullptr);
}
// ... and in d_rows (as many words again, zero-filled by this call; one fill when d_rows == d_flags + the words' count) the
// row words of those tiles for spiht_idwt_level1_rows_batch_*: bit r of a tile's word is set when its staged band row r holds
// a decoded cell.  d_rows == NULL: as spiht_decode_lists_flags_batch_i32; without d_flags d_rows is ignored.
extern "C" int spiht_decode_lists_rows_batch_i32(spiht_ctx *ctx, const uint8_t *d_data, uint64_t slot_stride,
                                                 const uint64_t *d_nbytes, const uint8_t *d_max_n, int64_t B, int64_t c,
                                                 int64_t H, int64_t W, int wavelet, int mode, int level, int32_t *d_out_zeroed,
                                                 uint32_t *d_flags, uint32_t *d_rows) {
    if (!ctx || !d_data || !d_nbytes || !d_max_n || !d_out_zeroed || B < 0) return SPIHT_ERR_ARG;
    ImgCall k;
    int st;
    // (one picture: an empty batch has its geometry checked too; decode_lists_batch takes the context)
    if (!k.open(&st, ctx, 1, c, H, W, wavelet, mode, level, true)) return st;
    L1Flags fl;
    const bool flagged = d_flags && l1flags_geometry(k.ig, k.F, &fl);
    if (flagged) { fl.p = d_flags; fl.rows = d_rows; }
    return decode_lists_batch(ctx, d_data, slot_stride, d_nbytes, d_max_n, B, k.g, d_out_zeroed, flagged ? &fl : nullptr);
}

// Puts the zeros back into the array the context's last spiht_decode_lists_batch_i32 scattered into (after its
// consumer, the inverse transform, has read it): clears exactly the cells that call wrote, through the decoder's
// lists, instead of a zero-fill of B*c*h*w*4 bytes before the next decode.  Falls back to that zero-fill when the
// lists are gone (another list-coding call on this context in between, slots reused within the launch, a latched
// device error).  Queued on the context's stream like everything else.
extern "C" int spiht_unscatter_lists_batch_i32(spiht_ctx *ctx, int32_t *d_out, int64_t B, int64_t c, int64_t h, int64_t w) {
    if (!ctx || !d_out || B < 0 || c < 1 || h < 1 || w < 1) return SPIHT_ERR_ARG;
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    StageTimer t(ctx, ST_MEMSET);
    const DecArgs &da = ctx->last_dec;
    if (ctx->last_dec_valid && da.out == d_out && da.B == (int)B && (int64_t)da.g.n == c * h * w) {
        LAUNCHCHK(spiht_launch_unscatter(&da, ctx->stream));
    } else {
        HIPCHK(hipMemsetAsync(d_out, 0, (size_t)B * (size_t)(c * h * w) * 4, ctx->stream));
    }
    return SPIHT_OK;
}

extern "C" int spiht_nbits_to_nbytes(spiht_ctx *ctx, const uint64_t *d_nbits, int64_t B, uint64_t *d_nbytes) {
    if (!ctx || !d_nbits || !d_nbytes || B < 0) return SPIHT_ERR_ARG;
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    LAUNCHCHK(spiht_launch_nbits_to_nbytes(d_nbits, (int)B, d_nbytes, ctx->stream));
    return SPIHT_OK;
}
