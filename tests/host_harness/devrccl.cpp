// devrccl.cpp — GPU tier only: the six RCCL entry points libfwgpu dlopen's (fwgpu_rccl.cpp), for ranks that are THREADS of one process,
// each with its own context and stream on ONE device.  The real librccl refuses two ranks on one device, so without this the slot
// layout of fwgpu_bus_allgather_ordered (rank r's data at r * n_floats, its flags at r * n_sil, the in-place send slot) never meets
// the real k_bus_sum_ordered at world > 1.  Never linked into the product; FWGPU_RCCL_LIB points libfwgpu at it.
//
// An all-gather: synchronise the caller's stream (its send buffer is written), rendezvous, copy every peer's send buffer into the
// caller's receive buffer device-to-device on the caller's stream (not the in-place slot: source and destination coincide),
// synchronise, rendezvous again (no peer reuses a send buffer while another still reads it).
// Both rendezvous are BOUNDED: a rank that waits longer than WAIT_S gets an error code, and so does every other waiter, then and
// from then on — a rank that failed never leaves its peers blocked on a shared machine.
//
// HIP is resolved from the copy of the runtime the process already holds (PyTorch ships its own libamdhip64; a second copy in the
// process would own no device memory of the first): the loaded objects are searched for it, nothing is linked or loaded anew.
#include <dlfcn.h>
#include <link.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

namespace {
constexpr int WAIT_S = 20;
enum { RC_OK = 0, RC_UNHANDLED_HIP = 1, RC_TIMEOUT = 3, RC_INVALID_ARGUMENT = 4, RC_INVALID_USAGE = 5 };  // rccl.h ncclResult_t

struct Hip {
    decltype(&hipStreamSynchronize) StreamSynchronize = nullptr;
    decltype(&hipMemcpyAsync) MemcpyAsync = nullptr;
    bool ok = false;
};
int find_hip(struct dl_phdr_info* info, size_t, void* out) {
    if (info->dlpi_name && strstr(info->dlpi_name, "libamdhip64")) {
        *(std::string*)out = info->dlpi_name;
        return 1;
    }
    return 0;
}
const Hip& hip() {
    static const Hip h = [] {
        Hip x;
        std::string path;
        dl_iterate_phdr(find_hip, &path);
        void* so = path.empty() ? nullptr : dlopen(path.c_str(), RTLD_NOW | RTLD_NOLOAD);  // (NOLOAD: the mapped copy or nothing)
        if (!so) return x;
        *(void**)(&x.StreamSynchronize) = dlsym(so, "hipStreamSynchronize");
        *(void**)(&x.MemcpyAsync) = dlsym(so, "hipMemcpyAsync");
        x.ok = x.StreamSynchronize && x.MemcpyAsync;
        return x;
    }();
    return h;
}

struct Group {
    int world = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    bool failed = false;
    std::vector<const void*> send;
    std::vector<void*> recv;
};
struct Comm {
    std::shared_ptr<Group> g;
    int rank;
};
std::mutex g_mu;
std::map<std::string, std::shared_ptr<Group>> g_groups;
std::atomic<uint64_t> g_next{1};

int fail_group(Group& g, int rc) {
    std::lock_guard<std::mutex> lk(g.mu);
    g.failed = true;
    g.cv.notify_all();
    return rc;
}
// all `world` ranks arrive, or everybody leaves with an error
int rendezvous(Group& g, int rank, const void* send, void* recv) {
    std::unique_lock<std::mutex> lk(g.mu);
    if (g.failed) return RC_TIMEOUT;
    if (recv) {
        g.send[rank] = send;
        g.recv[rank] = recv;
    }
    if (++g.arrived == g.world) {
        g.arrived = 0;
        g.gen++;
        g.cv.notify_all();
        return RC_OK;
    }
    const uint64_t gen = g.gen;
    if (!g.cv.wait_for(lk, std::chrono::seconds(WAIT_S), [&] { return g.gen != gen || g.failed; })) {
        g.failed = true;
        g.cv.notify_all();
    }
    return g.gen != gen ? RC_OK : RC_TIMEOUT;
}
}  // namespace

struct ncclUniqueId {
    char internal[128];
};

extern "C" {
int ncclGetUniqueId(ncclUniqueId* id) {
    memset(id, 0, sizeof(*id));
    const uint64_t n = g_next++;
    memcpy(id->internal, "DEVRCCL\0", 8);
    memcpy(id->internal + 8, &n, sizeof(n));
    return RC_OK;
}
int ncclCommInitRank(void** comm, int nranks, ncclUniqueId id, int rank) {
    if (nranks < 1 || rank < 0 || rank >= nranks || memcmp(id.internal, "DEVRCCL\0", 8) != 0) return RC_INVALID_ARGUMENT;
    if (!hip().ok) return RC_UNHANDLED_HIP;
    std::lock_guard<std::mutex> lk(g_mu);
    std::shared_ptr<Group>& g = g_groups[std::string(id.internal, sizeof(id.internal))];
    if (!g) {
        g = std::make_shared<Group>();
        g->world = nranks;
        g->send.assign((size_t)nranks, nullptr);
        g->recv.assign((size_t)nranks, nullptr);
    }
    if (g->world != nranks) return RC_INVALID_ARGUMENT;
    *comm = new Comm{g, rank};
    return RC_OK;
}
int ncclCommDestroy(void* comm) {
    delete (Comm*)comm;
    return RC_OK;
}
// (libfwgpu looks the symbol up when it loads an RCCL; no test sends an all-reduce through this stand-in)
int ncclAllReduce(const void*, void*, size_t, int, int, void*, void*) { return RC_INVALID_USAGE; }
int ncclAllGather(const void* send, void* recv, size_t count, int dtype, void* comm, void* stream) {
    if ((dtype != 7 && dtype != 1) || !send || !recv || !comm) return RC_INVALID_ARGUMENT;  // ncclFloat32, ncclUint8
    const size_t bytes = count * (dtype == 7 ? 4u : 1u);
    Comm* c = (Comm*)comm;
    Group& g = *c->g;
    const Hip& h = hip();
    hipStream_t s = (hipStream_t)stream;
    if (h.StreamSynchronize(s) != hipSuccess) return fail_group(g, RC_UNHANDLED_HIP);
    int rc = rendezvous(g, c->rank, send, recv);
    if (rc) return rc;
    // (the tables are stable from here to the second rendezvous: every rank wrote its entry before it arrived at the first)
    for (int p = 0; p < g.world; ++p) {
        char* dst = (char*)recv + (size_t)p * bytes;
        if ((const void*)dst == g.send[p]) continue;  // the in-place slot: rank p's send buffer IS its slot of its own receive buffer
        if (h.MemcpyAsync(dst, g.send[p], bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail_group(g, RC_UNHANDLED_HIP);
    }
    if (h.StreamSynchronize(s) != hipSuccess) return fail_group(g, RC_UNHANDLED_HIP);
    return rendezvous(g, c->rank, nullptr, nullptr);
}
const char* ncclGetErrorString(int rc) {
    switch (rc) {
        case RC_OK: return "no error";
        case RC_UNHANDLED_HIP: return "device stand-in: a HIP call failed, or no loaded HIP runtime was found";
        case RC_TIMEOUT: return "device stand-in: a peer did not arrive within 20 s";
        case RC_INVALID_USAGE: return "device stand-in: all-reduce is not offered";
        default: return "device stand-in: invalid argument";
    }
}
}
