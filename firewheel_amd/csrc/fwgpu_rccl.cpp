// fwgpu_rccl.cpp — the mix bus over RCCL, behind the C ABI (include/fwgpu.h "mix bus over RCCL").
//
// north_star names the step: "a single RCCL all-reduce over xGMI for the final mix bus" — the top-level R-port SumNode of a
// voice-sharded graph (nodes/sum.rs:111-133).  Rounds 1-5 had it in the Python harness only (torch.distributed); a Rust or C host
// bound to include/fwgpu.h got libfwgpu's own one-shot exchange (fwgpu_exchange.cpp) and nothing to compare it with.  Here:
//   fwgpu_bus_allreduce_rccl     ncclAllReduce(sum) in place on the ctx stream.  Re-associates the f32 sum for more than two ranks:
//                                within 1e-6 relative of the reference, not its bits.
//   fwgpu_bus_allgather_ordered  ncclAllGather of the partial buses (+ their per-(block, channel) silence flags), then the
//                                rank-ordered sum kernel of fwgpu_bus_sum_ordered_flags: sum.rs's order, silent ports skipped on the
//                                n-port path — bit-identical to the single-process graph on every rank.
// librccl is NOT a link dependency of libfwgpu.so: it is dlopen'ed at the first fwgpu_rccl_* call (FWGPU_RCCL_LIB names another
// file: the CPU tier's in-process stand-in, tests/host_harness/fakerccl.cpp), so hosts that never shard never load it.  The
// communicator is built from a 128-byte unique id the caller carries from rank 0 to every rank through whatever side channel it
// has — the same contract as the exchange's handles.
#include "fwgpu_ctx.h"

#include <dlfcn.h>

#include <mutex>

namespace {

struct NcclUniqueId {
    char internal[128];
};
static_assert(sizeof(NcclUniqueId) == FWGPU_RCCL_UNIQUE_ID_BYTES, "ncclUniqueId is 128 bytes (rccl.h NCCL_UNIQUE_ID_BYTES)");
typedef void* NcclComm;
enum { NCCL_UINT8 = 1, NCCL_FLOAT32 = 7, NCCL_SUM = 0 };  // rccl.h: ncclDataType_t / ncclRedOp_t

struct RcclApi {
    void* so = nullptr;
    int (*GetUniqueId)(NcclUniqueId*) = nullptr;
    int (*CommInitRank)(NcclComm*, int, NcclUniqueId, int) = nullptr;
    int (*CommDestroy)(NcclComm) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, NcclComm, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, NcclComm, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    char err[256] = {0};
};
RcclApi g_api;
std::mutex g_api_mu;
char g_rccl_err[512] = "";  // fwgpu_rccl_last_error: the calls that have no ctx to report through

bool load_api() {
    std::lock_guard<std::mutex> lk(g_api_mu);
    if (g_api.so) return true;
    const char* names[] = {getenv("FWGPU_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* so = nullptr;
    for (const char* n : names) {
        if (!n || !*n) continue;
        so = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (so) break;
        snprintf(g_api.err, sizeof(g_api.err), "%s", dlerror());
    }
    if (!so) return false;
    RcclApi a;
    a.so = so;
#define SYM(field, name)                                                                   \
    *(void**)(&a.field) = dlsym(so, name);                                                 \
    if (!a.field) {                                                                        \
        snprintf(g_api.err, sizeof(g_api.err), "librccl lacks %s", name);                  \
        dlclose(so);                                                                       \
        return false;                                                                      \
    }
    SYM(GetUniqueId, "ncclGetUniqueId")
    SYM(CommInitRank, "ncclCommInitRank")
    SYM(CommDestroy, "ncclCommDestroy")
    SYM(AllReduce, "ncclAllReduce")
    SYM(AllGather, "ncclAllGather")
    SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
    g_api = a;
    return true;
}

inline void use_device(fwgpu_ctx* c) {  // (as fwgpu_abi.cpp: the thread's current device is asked first, a thread-local read)
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != c->device) (void)hipSetDevice(c->device);
}

int nccl_fail(fwgpu_ctx* c, int rc, const char* what) {
    char msg[400];
    snprintf(msg, sizeof(msg), "%s: %s (ncclResult %d)", what, g_api.GetErrorString ? g_api.GetErrorString(rc) : "?", rc);
    snprintf(g_rccl_err, sizeof(g_rccl_err), "%s", msg);
    return c ? fail(c, FWGPU_ERR_DEVICE, msg) : FWGPU_ERR_DEVICE;
}

}  // namespace

struct fwgpu_rccl_comm {
    fwgpu_ctx* ctx = nullptr;
    NcclComm comm = nullptr;
    int world = 0, rank = 0;
    DevBuf gathered;      // [world][n_floats] partial buses, rank order (all-gather target)
    DevBuf gathered_sil;  // [world][n_silence] flags
    DevBuf zero_sil;      // flags of a caller that passes none: "nothing is silent"
};

extern "C" {

const char* fwgpu_rccl_last_error(void) { return g_rccl_err; }

int fwgpu_rccl_unique_id(uint8_t* id) {
    if (!id) return FWGPU_ERR_INVALID;
    if (!load_api()) {
        snprintf(g_rccl_err, sizeof(g_rccl_err), "librccl could not be loaded: %s", g_api.err);
        return FWGPU_ERR_DEVICE;
    }
    NcclUniqueId u;
    memset(&u, 0, sizeof(u));
    const int rc = g_api.GetUniqueId(&u);
    if (rc) return nccl_fail(nullptr, rc, "ncclGetUniqueId");
    memcpy(id, &u, sizeof(u));
    return 0;
}

fwgpu_rccl_comm* fwgpu_rccl_comm_create(fwgpu_ctx* c, const uint8_t* id, uint32_t world, uint32_t rank) {
    if (!c) return nullptr;
    if (!id || world == 0 || world > FW_MAX_BUS_PARTS || rank >= world) {
        fail(c, FWGPU_ERR_INVALID, "rccl comm: a 128-byte unique id, 1..64 ranks, rank < world");
        return nullptr;
    }
    if (!load_api()) {
        char msg[400];
        snprintf(msg, sizeof(msg), "librccl could not be loaded: %s", g_api.err);
        fail(c, FWGPU_ERR_DEVICE, msg);
        return nullptr;
    }
    use_device(c);
    RtHold hold(c);  // communicator setup allocates and synchronises: no resident realtime kernel meanwhile (as fwgpu_bus_exchange_open)
    fwgpu_rccl_comm* m = new (std::nothrow) fwgpu_rccl_comm();
    if (!m) {
        fail(c, FWGPU_ERR_DEVICE, "rccl comm: out of host memory");
        return nullptr;
    }
    m->ctx = c;
    m->world = (int)world;
    m->rank = (int)rank;
    NcclUniqueId u;
    memcpy(&u, id, sizeof(u));
    const int rc = g_api.CommInitRank(&m->comm, (int)world, u, (int)rank);  // collective: every rank of the id calls it
    if (rc) {
        nccl_fail(c, rc, "ncclCommInitRank");
        delete m;
        return nullptr;
    }
    return m;
}

int fwgpu_rccl_comm_destroy(fwgpu_rccl_comm* m) {
    if (!m) return 0;
    fwgpu_ctx* c = m->ctx;
    use_device(c);
    RtHold hold(c);
    (void)hipStreamSynchronize(c->stream);  // nothing of this communicator is in flight any more
    int rc = 0;
    if (m->comm) {
        const int nrc = g_api.CommDestroy(m->comm);
        if (nrc) rc = nccl_fail(c, nrc, "ncclCommDestroy");
    }
    m->gathered.release();
    m->gathered_sil.release();
    m->zero_sil.release();
    delete m;
    return rc;
}

int fwgpu_rccl_comm_info(fwgpu_rccl_comm* m, uint32_t* world, uint32_t* rank) {
    if (!m) return FWGPU_ERR_INVALID;
    if (world) *world = (uint32_t)m->world;
    if (rank) *rank = (uint32_t)m->rank;
    return 0;
}

int fwgpu_bus_allreduce_rccl(fwgpu_rccl_comm* m, float* d_bus, uint64_t n_floats) {
    if (!m) return FWGPU_ERR_INVALID;
    fwgpu_ctx* c = m->ctx;
    AudioCallScope audio;
    use_device(c);
    if (!d_bus || n_floats == 0) return fail(c, FWGPU_ERR_INVALID, "rccl all-reduce: null bus or no floats");
    const int rc = g_api.AllReduce(d_bus, d_bus, (size_t)n_floats, NCCL_FLOAT32, NCCL_SUM, m->comm, c->stream);
    return rc ? nccl_fail(c, rc, "ncclAllReduce") : 0;
}

int fwgpu_bus_allgather_ordered(fwgpu_rccl_comm* m, const float* d_bus, const uint8_t* d_silence, float* d_out, uint8_t* d_out_silence,
                                uint64_t n_floats, uint32_t frames_per_block, uint32_t n_channels) {
    if (!m) return FWGPU_ERR_INVALID;
    fwgpu_ctx* c = m->ctx;
    AudioCallScope audio;
    use_device(c);
    if (!d_bus || !d_out || n_floats == 0 || (n_floats & 3u)) return fail(c, FWGPU_ERR_INVALID, "rccl all-gather: null bus, or a float count that is no multiple of 4");
    if (((uintptr_t)d_out & 15u)) return fail(c, FWGPU_ERR_INVALID, "output not 16-byte aligned");
    if (frames_per_block == 0 || n_channels == 0) return fail(c, FWGPU_ERR_INVALID, "the block geometry (frames, channels) is needed: silence is per (block, channel)");
    const uint64_t per = (uint64_t)frames_per_block * n_channels;
    const uint32_t n_blocks = (uint32_t)((n_floats + per - 1) / per);
    const size_t n_sil = ((size_t)n_blocks * n_channels + 15) & ~(size_t)15;  // (16-byte slots: every rank's flags start aligned)
    const size_t W = (size_t)m->world;
    if (m->gathered.cap < W * n_floats * sizeof(float) || m->gathered_sil.cap < W * n_sil) {
        RtHold hold(c);  // (first call of this size only)
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, m->gathered.ensure_n("rccl_gathered", W * n_floats * sizeof(float)));
        HIPC(c, m->gathered_sil.ensure_n("rccl_gathered_sil", W * n_sil));
        HIPC(c, hipMemsetAsync(m->gathered_sil.p, 0, W * n_sil, c->stream));
    }
    // zero_sil is sent, never written: cleared over its WHOLE capacity whenever it is (re)allocated, and tested on its own — DevBuf
    // allocates with headroom, so a later call with more blocks may fit every capacity, and whatever it sends must be zeros too
    // (a non-zero byte read as a flag clears a block, or drops a port from the n-port sum).  A size seen before costs one compare.
    if (m->zero_sil.cap < n_sil) {
        RtHold hold(c);
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, m->zero_sil.ensure_n("rccl_zero_sil", n_sil));
        HIPC(c, hipMemsetAsync(m->zero_sil.p, 0, m->zero_sil.cap, c->stream));
    }
    int rc = g_api.AllGather(d_bus, m->gathered.p, (size_t)n_floats, NCCL_FLOAT32, m->comm, c->stream);
    if (rc) return nccl_fail(c, rc, "ncclAllGather(bus)");
    // the flags travel as whole 16-byte slots; a caller without flags sends "nothing silent".  The caller's array holds
    // n_blocks * n_channels bytes: staged into a slot-sized block first so that the gather never reads past it.
    const uint8_t* sil_src = (const uint8_t*)m->zero_sil.p;
    if (d_silence) {
        uint8_t* mine = (uint8_t*)m->gathered_sil.p + (size_t)m->rank * n_sil;
        HIPC(c, hipMemcpyAsync(mine, d_silence, (size_t)n_blocks * n_channels, hipMemcpyDeviceToDevice, c->stream));
        sil_src = mine;  // (in place: rank r's slot of the receive buffer is its send buffer — ncclAllGather's in-place form)
    }
    rc = g_api.AllGather(sil_src, m->gathered_sil.p, n_sil, NCCL_UINT8, m->comm, c->stream);
    if (rc) return nccl_fail(c, rc, "ncclAllGather(silence flags)");
    BusParts bp;
    bp.n = m->world;
    const uint8_t* sil[FW_MAX_BUS_PARTS];
    for (int r = 0; r < FW_MAX_BUS_PARTS; ++r) {
        bp.part[r] = r < m->world ? (const float*)m->gathered.p + (size_t)r * n_floats : nullptr;
        sil[r] = r < m->world ? (const uint8_t*)m->gathered_sil.p + (size_t)r * n_sil : nullptr;
    }
    // (the table of flag pointers is read by the kernel: it must live in device-visible memory until the launch has run — the launch
    //  wrapper copies it into the kernel's arguments, as for fwgpu_bus_sum_ordered_flags)
    LCHK(c, launch_bus_sum_ordered(c->stream, bp, sil, d_out, d_out_silence, (size_t)n_floats, n_blocks, frames_per_block, n_channels));
    return 0;
}

}  // extern "C"
