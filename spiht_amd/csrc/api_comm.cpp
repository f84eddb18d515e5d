// Host side of libspiht_hip.so (include/spiht_hip.h), several GPUs: the RCCL communicator and the gather of the streams.
#include "api_internal.h"

// ------------------------------------------------------------------------------------------------
// multi-GPU: the one exchange of the path -- an all-gather of the stream slots, bit counts and start planes between
// encode and decode -- on RCCL, queued on the context's stream like every kernel.  librccl is loaded
// on first use (a single-GPU process never touches it); no link-time dependency.
// ------------------------------------------------------------------------------------------------
#include <dlfcn.h>
#include <rccl/rccl.h>

struct RcclApi {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int *) = nullptr;
    const char *(*GetLastError)(ncclComm_t) = nullptr;  // optional (newer RCCL)
};
static RcclApi g_rccl;
static std::mutex g_rccl_mu;

static std::string g_rccl_name;   // the soname that was loaded, or what was tried and why each failed

static int rccl_load() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.h) return SPIHT_OK;
    const char *names[] = {getenv("SPIHT_RCCL_LIB"), "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
    void *h = nullptr;
    std::string tried;
    for (const char *n : names) {
        if (!n || !*n) continue;
        h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (h) { g_rccl_name = n; break; }
        const char *e = dlerror();
        tried += std::string(tried.empty() ? "" : "; ") + n + ": " + (e ? e : "?");
    }
    if (!h) {
        g_rccl_name = "not loaded (" + tried + ")";
        g_hip_err = "cannot load librccl, tried " + tried;
        return SPIHT_ERR_HIP;
    }
    RcclApi a;
    a.h = h;
#define RSYM(field, name)                                                                \
    do {                                                                                  \
        *(void **)(&a.field) = dlsym(h, name);                                            \
        if (!a.field) { g_hip_err = std::string("librccl lacks ") + name; dlclose(h); return SPIHT_ERR_HIP; } \
    } while (0)
    RSYM(GetUniqueId, "ncclGetUniqueId");
    RSYM(CommInitRank, "ncclCommInitRank");
    RSYM(CommDestroy, "ncclCommDestroy");
    RSYM(AllGather, "ncclAllGather");
    RSYM(AllReduce, "ncclAllReduce");
    RSYM(GroupStart, "ncclGroupStart");
    RSYM(GroupEnd, "ncclGroupEnd");
    RSYM(GetErrorString, "ncclGetErrorString");
    RSYM(GetVersion, "ncclGetVersion");
#undef RSYM
    *(void **)(&a.GetLastError) = dlsym(h, "ncclGetLastError");
    g_rccl = a;
    return SPIHT_OK;
}

#define NCCLCHK(expr)                                                                      \
    do {                                                                                   \
        ncclResult_t _r = (expr);                                                          \
        if (_r != ncclSuccess) {                                                           \
            g_hip_err = std::string(#expr) + ": " + g_rccl.GetErrorString(_r);             \
            return SPIHT_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

struct spiht_comm {
    ncclComm_t comm = nullptr;
    int world = 1, rank = 0, device = 0;
    void *scratch = nullptr;  // 16 device bytes for the barrier / the scalar reductions
};

static_assert(SPIHT_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");

// Which RCCL library serves this process: the soname dlopen took, or -- when none could be loaded -- every candidate
// tried with the loader's reason.  Empty before the first spiht_comm_* call.
extern "C" const char *spiht_rccl_library(void) {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    return g_rccl_name.c_str();
}

extern "C" int spiht_comm_unique_id(uint8_t *id) {
    if (!id) return SPIHT_ERR_ARG;
    CHK(rccl_load());
    ncclUniqueId u;
    NCCLCHK(g_rccl.GetUniqueId(&u));
    memcpy(id, u.internal, SPIHT_COMM_ID_BYTES);
    return SPIHT_OK;
}

extern "C" int spiht_comm_create(spiht_ctx *ctx, const uint8_t *id, int world, int rank, spiht_comm **out) {
    if (!ctx || !id || !out || world < 1 || rank < 0 || rank >= world) return SPIHT_ERR_ARG;
    *out = nullptr;
    CHK(rccl_load());
    HIPCHK(hipSetDevice(ctx->device));
    ncclUniqueId u;
    memcpy(u.internal, id, SPIHT_COMM_ID_BYTES);
    spiht_comm *c = new spiht_comm();
    c->world = world;
    c->rank = rank;
    c->device = ctx->device;
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, world, u, rank);
    if (r != ncclSuccess) {
        // the result's name and, where this RCCL has it, the text of the last error it logged (the actual reason)
        g_hip_err = "ncclCommInitRank(world " + std::to_string(world) + ", rank " + std::to_string(rank) + ", device " +
                    std::to_string(ctx->device) + ", " + g_rccl_name + "): " + g_rccl.GetErrorString(r);
        if (g_rccl.GetLastError) {
            const char *le = g_rccl.GetLastError(nullptr);
            if (le && *le) g_hip_err += std::string(" -- ") + le;
        }
        delete c;
        return SPIHT_ERR_HIP;
    }
    if (hipMalloc(&c->scratch, 16) != hipSuccess) {
        (void)hipGetLastError();
        (void)g_rccl.CommDestroy(c->comm);
        delete c;
        return SPIHT_ERR_NOMEM;
    }
    *out = c;
    return SPIHT_OK;
}

extern "C" void spiht_comm_destroy(spiht_comm *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    delete c;
}

extern "C" int spiht_comm_info(spiht_comm *c, int *world, int *rank, int *rccl_version) {
    if (!c) return SPIHT_ERR_ARG;
    if (world) *world = c->world;
    if (rank) *rank = c->rank;
    if (rccl_version) {
        *rccl_version = 0;
        if (g_rccl.GetVersion) (void)g_rccl.GetVersion(rccl_version);
    }
    return SPIHT_OK;
}

// Rank r's B slots / bit counts / start planes land in rows [r*B, (r+1)*B) of the gathered arrays on every rank
// (spiht_amd/dist.py: rank-major).  Three all-gathers in one RCCL group, queued on the context's stream: ordered
// after the encoder kernels queued before and before the decoder kernels queued after; the host does not block.
extern "C" int spiht_gather_streams(spiht_ctx *ctx, spiht_comm *c, const uint8_t *d_slots, const uint64_t *d_nbits,
                                    const uint8_t *d_max_n, int64_t B, uint64_t slot_stride, uint8_t *d_all_slots,
                                    uint64_t *d_all_nbits, uint8_t *d_all_max_n) {
    if (!ctx || !c || !d_slots || !d_nbits || !d_max_n || !d_all_slots || !d_all_nbits || !d_all_max_n || B < 0)
        return SPIHT_ERR_ARG;
    if (c->device != ctx->device) return SPIHT_ERR_ARG;
    if (B == 0) return SPIHT_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    StageTimer t(ctx, ST_GATHER);  // (the exchange's own time on the stream: a first multi-GPU run explains itself)
    NCCLCHK(g_rccl.GroupStart());
    ncclResult_t r1 = g_rccl.AllGather(d_slots, d_all_slots, (size_t)B * slot_stride, ncclUint8, c->comm, ctx->stream);
    ncclResult_t r2 = g_rccl.AllGather(d_nbits, d_all_nbits, (size_t)B, ncclUint64, c->comm, ctx->stream);
    ncclResult_t r3 = g_rccl.AllGather(d_max_n, d_all_max_n, (size_t)B, ncclUint8, c->comm, ctx->stream);
    NCCLCHK(g_rccl.GroupEnd());
    NCCLCHK(r1);
    NCCLCHK(r2);
    NCCLCHK(r3);
    return SPIHT_OK;
}

// Where rank r's rows start in the gathered arrays (rank-major: rows [r*B, (r+1)*B)), in bytes from each array's start --
// what a rank's decoder reads after spiht_gather_streams.  Pure arithmetic (no device); spiht_pipeline_submit_gather uses it.
extern "C" int spiht_gather_row_offsets(int rank, int world, int64_t B, uint64_t slot_stride, uint64_t *off_slots, uint64_t *off_nbits,
                                        uint64_t *off_max_n) {
    if (world < 1 || rank < 0 || rank >= world || B < 0 || !off_slots || !off_nbits || !off_max_n) return SPIHT_ERR_ARG;
    if (slot_stride && (uint64_t)world * (uint64_t)B > UINT64_MAX / slot_stride) return SPIHT_ERR_TOO_LARGE;
    *off_slots = (uint64_t)rank * (uint64_t)B * slot_stride;
    *off_nbits = (uint64_t)rank * (uint64_t)B * sizeof(uint64_t);
    *off_max_n = (uint64_t)rank * (uint64_t)B;
    return SPIHT_OK;
}

// max over ranks of a host double (timing: the job's time is its slowest rank's); blocks until done
extern "C" int spiht_comm_allreduce_max_f64(spiht_ctx *ctx, spiht_comm *c, double *value) {
    if (!ctx || !c || !value || c->device != ctx->device) return SPIHT_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(c->scratch, value, 8, hipMemcpyHostToDevice, ctx->stream));
    NCCLCHK(g_rccl.AllReduce(c->scratch, c->scratch, 1, ncclFloat64, ncclMax, c->comm, ctx->stream));
    HIPCHK(hipMemcpyAsync(value, c->scratch, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPIHT_OK;
}

// every rank has reached this call and everything queued on its context's stream before it has finished
extern "C" int spiht_comm_barrier(spiht_ctx *ctx, spiht_comm *c) {
    double one = 1.0;
    return spiht_comm_allreduce_max_f64(ctx, c, &one);
}
