// avt_shard.cpp — batch split of independent frames over the GPUs of one node behind the C ABI of include/avt_shard.h
// (SURVEY.md §8e): frame f -> rank f mod W, model constants replicated, RCCL over xGMI for exactly three exchanges
// (model broadcast, cloud scatter, result all-gather), all on device buffers.  The reference has no counterpart: it is
// a single process whose parallelism are per-call std::thread pools (AvatarOptimizer.cpp:337-343, :883-889).
// Compiled with hipcc (host only).  librccl is opened with dlopen at the first use, see rccl_api().
#include <dlfcn.h>
#include <link.h>
#include <rccl/rccl.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/avt_shard.h"
#include "avt_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// partition
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int avt_shard_owner(int frame, int world) { return world > 0 ? frame % world : 0; }
extern "C" int avt_shard_local_count(int num_frames, int rank, int world) {
    if (world <= 0 || rank < 0 || rank >= world || num_frames <= rank) return 0;
    return (num_frames - rank + world - 1) / world;
}
extern "C" int avt_shard_local_index(int frame, int world) { return world > 0 ? frame / world : frame; }
extern "C" int avt_shard_global_frame(int local_index, int rank, int world) { return rank + world * local_index; }

// ---------------------------------------------------------------------------------------------------------------------
// packed model: header + the arrays of avt_model_desc, each 8-byte aligned, in declaration order
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct PackHeader {
    char magic[8];                 // "AVTMODEL"
    std::int32_t version, V, J, K, F, nnz_w, nnz_r, ncomps, ndims, pad;
    std::uint64_t bytes;           // of the whole block
};

struct PackLayout {
    size_t off[15], len[15];       // byte offset / byte length of every array (13, 14: the legacy format's joint shape regressor)
    size_t total;
};
enum { PACK_LIMIT_ONE_JOINT = 1, PACK_HAS_JSR = 2 };      // PackHeader::pad carries these flags (0 in blocks packed before they existed)

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

bool pack_layout(const PackHeader& h, PackLayout& L) {
    if (h.V <= 0 || h.J <= 0 || h.K < 0 || h.F < 0 || h.nnz_w < 0 || h.nnz_r < 0 || h.ncomps < 0 || h.ndims < 0) return false;
    if (h.J > AVT_MAX_JOINTS || h.K > AVT_MAX_SHAPE || h.V > (1 << 24) || h.F > (1 << 25) || h.ncomps > 4096 || h.ndims > 4096) return false;
    const size_t V = h.V, J = h.J, K = h.K, F = h.F, C = h.ncomps, n = h.ndims;
    const size_t lens[13] = {3 * V * 8, 3 * V * K * 8, J * 4, 3 * F * 4, (V + 1) * 4, (size_t)h.nnz_w * 4, (size_t)h.nnz_w * 8,
                             (J + 1) * 4, (size_t)h.nnz_r * 4, (size_t)h.nnz_r * 8, C * 8, C * n * 8, C * n * n * 8};
    size_t o = align8(sizeof(PackHeader));
    for (int i = 0; i < 13; ++i) { L.off[i] = o; L.len[i] = lens[i]; o = align8(o + lens[i]); }
    const bool jsr = (h.pad & PACK_HAS_JSR) != 0;
    const size_t extra[2] = {jsr ? 3 * J * 8 : 0, jsr ? 3 * J * K * 8 : 0};
    for (int i = 0; i < 2; ++i) { L.off[13 + i] = o; L.len[13 + i] = extra[i]; o = align8(o + extra[i]); }
    L.total = o;
    return (h.pad & ~(PACK_LIMIT_ONE_JOINT | PACK_HAS_JSR)) == 0;
}

bool header_of(const avt_model_desc* d, PackHeader& h) {
    if (!d || d->num_points <= 0 || d->num_joints <= 0 || !d->weights_colptr || !d->jreg_colptr) return false;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, "AVTMODEL", 8);
    h.version = 1;
    h.V = d->num_points; h.J = d->num_joints; h.K = d->num_shape_keys; h.F = d->num_faces;
    h.nnz_w = d->weights_colptr[d->num_points];
    h.nnz_r = d->jreg_colptr[d->num_joints];
    h.ncomps = d->prior_ncomps > 0 ? d->prior_ncomps : 0;
    h.ndims = h.ncomps ? d->prior_ndims : 0;
    h.pad = (d->limit_one_joint_per_point ? PACK_LIMIT_ONE_JOINT : 0) | ((d->joint_shape_reg_base && d->joint_shape_reg) ? PACK_HAS_JSR : 0);
    return true;
}

}  // namespace

extern "C" int avt_model_pack_size(const avt_model_desc* desc, size_t* bytes) {
    return avt_guard("avt_model_pack_size", [&]() -> int {
        PackHeader h; PackLayout L;
        if (!bytes || !header_of(desc, h) || !pack_layout(h, L)) { avt_set_error("avt_model_pack_size: bad model description"); return 1; }
        *bytes = L.total;
        return 0;
    });
}

extern "C" int avt_model_pack(const avt_model_desc* d, void* buf, size_t bytes) {
    return avt_guard("avt_model_pack", [&]() -> int {
        PackHeader h; PackLayout L;
        if (!buf || !header_of(d, h) || !pack_layout(h, L)) { avt_set_error("avt_model_pack: bad model description"); return 1; }
        if (bytes < L.total) { avt_set_error("avt_model_pack: buffer too small"); return 1; }
        h.bytes = L.total;
        char* b = (char*)buf;
        std::memset(b, 0, L.total);
        std::memcpy(b, &h, sizeof h);
        const void* src[15] = {d->base_cloud, d->key_clouds, d->parent, d->mesh, d->weights_colptr, d->weights_row, d->weights_val,
                               d->jreg_colptr, d->jreg_row, d->jreg_val, d->prior_weight, d->prior_mean, d->prior_cov,
                               d->joint_shape_reg_base, d->joint_shape_reg};
        for (int i = 0; i < 15; ++i) {
            if (L.len[i] == 0) continue;
            if (!src[i]) { avt_set_error("avt_model_pack: a required array of the model description is NULL"); return 1; }
            std::memcpy(b + L.off[i], src[i], L.len[i]);
        }
        return 0;
    });
}

extern "C" int avt_model_unpack(const void* buf, size_t bytes, avt_model** out) {
    return avt_guard("avt_model_unpack", [&]() -> int {
        if (!buf || !out || bytes < sizeof(PackHeader)) { avt_set_error("avt_model_unpack: block too small"); return 1; }
        PackHeader h;
        std::memcpy(&h, buf, sizeof h);
        PackLayout L;
        if (std::memcmp(h.magic, "AVTMODEL", 8) != 0 || h.version != 1 || !pack_layout(h, L) || h.bytes != L.total || bytes < L.total) {
            avt_set_error("avt_model_unpack: not a packed model (magic / version / size mismatch)");
            return 1;
        }
        const char* b = (const char*)buf;
        avt_model_desc d;
        std::memset(&d, 0, sizeof d);
        d.num_points = h.V; d.num_joints = h.J; d.num_shape_keys = h.K; d.num_faces = h.F;
        d.base_cloud = (const double*)(b + L.off[0]); d.key_clouds = (const double*)(b + L.off[1]);
        d.parent = (const int*)(b + L.off[2]); d.mesh = (const int*)(b + L.off[3]);
        d.weights_colptr = (const int*)(b + L.off[4]); d.weights_row = (const int*)(b + L.off[5]); d.weights_val = (const double*)(b + L.off[6]);
        d.jreg_colptr = (const int*)(b + L.off[7]); d.jreg_row = (const int*)(b + L.off[8]); d.jreg_val = (const double*)(b + L.off[9]);
        d.prior_ncomps = h.ncomps; d.prior_ndims = h.ndims;
        if (h.ncomps) { d.prior_weight = (const double*)(b + L.off[10]); d.prior_mean = (const double*)(b + L.off[11]); d.prior_cov = (const double*)(b + L.off[12]); }
        d.limit_one_joint_per_point = (h.pad & PACK_LIMIT_ONE_JOINT) ? 1 : 0;
        if (h.pad & PACK_HAS_JSR) { d.joint_shape_reg_base = (const double*)(b + L.off[13]); d.joint_shape_reg = (const double*)(b + L.off[14]); }
        // the column pointers index the arrays that follow them: check before avt_model_create walks them
        if (d.weights_colptr[0] != 0 || d.weights_colptr[h.V] != h.nnz_w || d.jreg_colptr[0] != 0 || d.jreg_colptr[h.J] != h.nnz_r) {
            avt_set_error("avt_model_unpack: sparse column pointers do not match the block");
            return 1;
        }
        for (int v = 0; v < h.V; ++v)
            if (d.weights_colptr[v + 1] < d.weights_colptr[v]) { avt_set_error("avt_model_unpack: weight column pointers not monotone"); return 1; }
        for (int j = 0; j < h.J; ++j)      // (all of them before any row is read: monotone from 0 to nnz_r, every index below lies in the array)
            if (d.jreg_colptr[j + 1] < d.jreg_colptr[j]) { avt_set_error("avt_model_unpack: regressor column pointers not monotone"); return 1; }
        for (int e = 0; e < h.nnz_r; ++e)
            if (d.jreg_row[e] < 0 || d.jreg_row[e] >= h.V) { avt_set_error("avt_model_unpack: regressor row out of range"); return 1; }
        return avt_model_create(&d, out);
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// RCCL, opened at run time
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct RcclApi {
    void* handle = nullptr;
    std::string path, error;
    int version = 0;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
};

int find_loaded_rccl(struct dl_phdr_info* info, size_t, void* data) {
    if (info->dlpi_name && std::strstr(info->dlpi_name, "librccl")) { *(std::string*)data = info->dlpi_name; return 1; }
    return 0;
}

RcclApi* rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (tried) {
        if (!api.handle) avt_set_error("avt_shard: cannot open librccl (" + api.error + "); set AVT_RCCL_LIB");
        return api.handle ? &api : nullptr;
    }
    tried = true;
    // one RCCL per process: if the host program (PyTorch) already mapped a librccl, use that very copy
    std::string loaded;
    dl_iterate_phdr(find_loaded_rccl, &loaded);
    std::vector<std::string> cand;
    if (const char* e = getenv("AVT_RCCL_LIB")) cand.push_back(e);
    if (!loaded.empty()) cand.push_back(loaded);
    cand.push_back("librccl.so.1"); cand.push_back("librccl.so"); cand.push_back("/opt/rocm/lib/librccl.so.1");
    for (const std::string& p : cand) {
        api.handle = dlopen(p.c_str(), RTLD_NOW | RTLD_GLOBAL);
        if (api.handle) { api.path = p; break; }
        const char* e = dlerror();              // dlerror() clears the message: read it once
        api.error = p + ": " + (e ? e : "dlopen failed");
    }
    if (!api.handle) { avt_set_error("avt_shard: cannot open librccl (" + api.error + "); set AVT_RCCL_LIB"); return nullptr; }
    bool ok = true;
    auto sym = [&](const char* n) { void* s = dlsym(api.handle, n); if (!s) { ok = false; api.error = std::string("missing symbol ") + n; } return s; };
    api.GetVersion = (decltype(api.GetVersion))sym("ncclGetVersion");
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    api.Broadcast = (decltype(api.Broadcast))sym("ncclBroadcast");
    api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
    api.Send = (decltype(api.Send))sym("ncclSend");
    api.Recv = (decltype(api.Recv))sym("ncclRecv");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    if (!ok) { avt_set_error("avt_shard: " + api.path + ": " + api.error); dlclose(api.handle); api.handle = nullptr; return nullptr; }
    Dl_info di;
    if (dladdr((void*)api.GetUniqueId, &di) && di.dli_fname) api.path = di.dli_fname;
    api.GetVersion(&api.version);
    return &api;
}

// ---------------------------------------------------------------------------------------------------------------------
// The transport: what an avt_shard asks of its communicator, counts and types as RCCL takes them.  Its destructor leaves the group.
// ---------------------------------------------------------------------------------------------------------------------
struct Transport {
    virtual ~Transport() = default;
    virtual ncclResult_t broadcast(const void* send, void* recv, size_t count, ncclDataType_t t, int root, hipStream_t st) = 0;
    virtual ncclResult_t all_gather(const void* send, void* recv, size_t count, ncclDataType_t t, hipStream_t st) = 0;
    virtual ncclResult_t send(const void* ptr, size_t count, ncclDataType_t t, int peer, hipStream_t st) = 0;
    virtual ncclResult_t recv(void* ptr, size_t count, ncclDataType_t t, int peer, hipStream_t st) = 0;
    virtual ncclResult_t group_start() = 0;
    virtual ncclResult_t group_end() = 0;
    virtual const char* error_string(ncclResult_t r) const = 0;
    virtual std::string backend() const = 0;      // avt_shard_backend
};

struct RcclTransport final : Transport {
    RcclApi* a;
    ncclComm_t comm = nullptr;
    explicit RcclTransport(RcclApi* api) : a(api) {}
    ~RcclTransport() override { if (comm) a->CommDestroy(comm); }
    ncclResult_t broadcast(const void* send, void* recv, size_t count, ncclDataType_t t, int root, hipStream_t st) override { return a->Broadcast(send, recv, count, t, root, comm, st); }
    ncclResult_t all_gather(const void* send, void* recv, size_t count, ncclDataType_t t, hipStream_t st) override { return a->AllGather(send, recv, count, t, comm, st); }
    ncclResult_t send(const void* ptr, size_t count, ncclDataType_t t, int peer, hipStream_t st) override { return a->Send(ptr, count, t, peer, comm, st); }
    ncclResult_t recv(void* ptr, size_t count, ncclDataType_t t, int peer, hipStream_t st) override { return a->Recv(ptr, count, t, peer, comm, st); }
    ncclResult_t group_start() override { return a->GroupStart(); }
    ncclResult_t group_end() override { return a->GroupEnd(); }
    const char* error_string(ncclResult_t r) const override { return a->GetErrorString(r); }
    std::string backend() const override {
        char buf[512];
        snprintf(buf, sizeof buf, "rccl %d.%d.%d, %s", a->version / 10000, (a->version / 100) % 100, a->version % 100, a->path.c_str());
        return buf;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The point-to-point front of the two transports that need no RCCL.  Sends and receives queue up until the outermost group ends (a lone
// one is a group of its own); broadcast and all-gather are made of them - the root sends to every other rank, every rank sends to and
// receives from every other rank, a rank's own part is a device-to-device copy.  A transport supplies complete(): all of `sends` and
// `recvs` (device pointers), FIFO per peer, on this stream; it returns when everything this rank sends has been taken - its buffers are
// free again - and everything it receives lies in its buffers.  Stricter than RCCL: every call completes before it returns.
// ---------------------------------------------------------------------------------------------------------------------
struct Xfer { int peer; char* ptr; size_t bytes, done; };

size_t nccl_type_bytes(ncclDataType_t t) {
    switch (t) {
        case ncclChar: case ncclUint8: return 1;
        case ncclInt32: case ncclUint32: case ncclFloat: return 4;
        case ncclInt64: case ncclUint64: case ncclDouble: return 8;
        default: return 0;
    }
}

ncclResult_t copy_now(void* dst, const void* src, size_t bytes, hipStream_t st) {
    if (bytes && dst != src && hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st) != hipSuccess) return ncclUnhandledCudaError;
    return hipStreamSynchronize(st) == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
}

struct P2pTransport : Transport {
    const int rank, world;
    int depth = 0;                         // open groups
    std::vector<Xfer> q_sends, q_recvs;    // queued by send / recv (a handle belongs to one thread)
    hipStream_t stream = nullptr;
    P2pTransport(int rank_, int world_) : rank(rank_), world(world_) {}
    virtual ncclResult_t complete(std::vector<Xfer>& sends, std::vector<Xfer>& recvs, hipStream_t st) = 0;

    ncclResult_t flush() {
        if (q_sends.empty() && q_recvs.empty()) return ncclSuccess;
        const ncclResult_t r = complete(q_sends, q_recvs, stream);
        q_sends.clear(); q_recvs.clear(); stream = nullptr;
        return r;
    }
    ncclResult_t group_start() override { ++depth; return ncclSuccess; }
    ncclResult_t group_end() override { return --depth == 0 ? flush() : ncclSuccess; }
    ncclResult_t queue(std::vector<Xfer>& q, const void* ptr, size_t bytes, int peer, hipStream_t st) {
        stream = st;
        q.push_back({peer, (char*)ptr, bytes, 0});
        return depth == 0 ? flush() : ncclSuccess;
    }
    ncclResult_t send(const void* ptr, size_t count, ncclDataType_t t, int peer, hipStream_t st) override { return queue(q_sends, ptr, count * nccl_type_bytes(t), peer, st); }
    ncclResult_t recv(void* ptr, size_t count, ncclDataType_t t, int peer, hipStream_t st) override { return queue(q_recvs, ptr, count * nccl_type_bytes(t), peer, st); }
    ncclResult_t broadcast(const void* send, void* recv, size_t count, ncclDataType_t t, int root, hipStream_t st) override {
        const size_t bytes = count * nccl_type_bytes(t);
        std::vector<Xfer> out, in;
        if (rank == root) { for (int k = 0; k < world; ++k) if (k != root) out.push_back({k, (char*)send, bytes, 0}); }
        else in.push_back({root, (char*)recv, bytes, 0});
        const ncclResult_t r = complete(out, in, st);
        return r == ncclSuccess && rank == root ? copy_now(recv, send, bytes, st) : r;
    }
    ncclResult_t all_gather(const void* send, void* recv, size_t count, ncclDataType_t t, hipStream_t st) override {
        const size_t bytes = count * nccl_type_bytes(t);
        std::vector<Xfer> out, in;
        for (int k = 0; k < world; ++k) if (k != rank) { out.push_back({k, (char*)send, bytes, 0}); in.push_back({k, (char*)recv + (size_t)k * bytes, bytes, 0}); }
        const ncclResult_t r = complete(out, in, st);
        return r == ncclSuccess ? copy_now((char*)recv + (size_t)rank * bytes, send, bytes, st) : r;
    }
};

// one reader of AVT_SHARD_LOOPBACK_TIMEOUT_S: how long an exchange may see no progress before its group is declared broken
double timeout_from_env(double default_s) {
    const char* e = getenv("AVT_SHARD_LOOPBACK_TIMEOUT_S");
    return e ? std::max(0.1, atof(e)) : default_s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Loop-back transport: the ranks are the THREADS of one process (one avt_shard per thread, any mix of devices), a transfer is a
// device-to-device copy behind a host-side rendezvous.  It exists for two reasons: a single-process host that drives several GPUs from
// threads needs no RCCL, and every line of the multi-peer exchange code below can run with W > 1 ranks on a one-GPU box
// (tests/test_gpu_shard.py) - RCCL refuses two ranks on one GPU.  A rank that never arrives makes its peers fail after a time-out
// instead of hanging (ncclSystemError), and the group stays broken.
// ---------------------------------------------------------------------------------------------------------------------
struct LoopMail { const void* ptr; size_t bytes; int state; };   // 0 posted, 1 taken by the receiver, 2 copied
struct LoopGroup {
    std::string name;
    int world = 0, joined = 0, refs = 0;
    std::mutex m;
    std::condition_variable cv;
    bool broken = false;
    double timeout_s = 20.0;
    std::vector<std::deque<LoopMail>> mail;        // [source * world + destination] posted sends, oldest first
    std::vector<int> outstanding;                  // per source rank: posted sends not yet copied out by their receivers
    std::vector<char> present;                     // per rank: a member with this rank exists
};

std::mutex loop_registry_mutex;
std::map<std::string, LoopGroup*> loop_registry;

struct LoopTransport final : P2pTransport {
    LoopGroup* g;
    LoopTransport(LoopGroup* g_, int rank_) : P2pTransport(rank_, g_->world), g(g_) {}
    ~LoopTransport() override {
        std::lock_guard<std::mutex> lk(loop_registry_mutex);
        --g->joined;
        g->present[rank] = 0;
        if (--g->refs == 0) {
            auto it = loop_registry.find(g->name);
            if (it != loop_registry.end() && it->second == g) loop_registry.erase(it);      // (a broken group was already taken out of the registry)
            delete g;
        }
    }
    const char* error_string(ncclResult_t r) const override {
        return r == ncclSuccess ? "no error" : r == ncclSystemError ? "loop-back transport: a rank did not arrive (time-out); the group is broken" : "loop-back transport: device copy failed";
    }
    std::string backend() const override { return "loop-back (threads of one process), group " + g->name; }
    // Only the two ends of a transfer meet - a rank with nothing to send or receive meets nobody - through a mailbox per (source,
    // destination) pair: the sender posts (pointer, size), the receiver takes the oldest posted entry of its pair, copies device-to-device
    // on its own stream and marks it done; the sender returns when all its entries are done.  All posts happen before any wait, so W ranks
    // that all send to each other cannot deadlock.
    ncclResult_t complete(std::vector<Xfer>& sends, std::vector<Xfer>& recvs, hipStream_t st) override {
        const int me = rank, W = world;
        ncclResult_t r = hipStreamSynchronize(st) == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;   // what I send is ready
        const auto limit = std::chrono::duration<double>(g->timeout_s);
        {
            std::lock_guard<std::mutex> lk(g->m);
            for (const Xfer& sd : sends) { g->mail[(size_t)me * W + sd.peer].push_back({sd.ptr, sd.bytes, 0}); ++g->outstanding[me]; }
            g->cv.notify_all();
        }
        for (const Xfer& rc : recvs) {
            if (r != ncclSuccess) break;
            std::deque<LoopMail>& box = g->mail[(size_t)rc.peer * W + me];
            LoopMail* m = nullptr;
            {
                std::unique_lock<std::mutex> lk(g->m);
                const bool ok = g->cv.wait_for(lk, limit, [&] {
                    if (g->broken) return true;
                    for (LoopMail& e : box) if (e.state == 0) { m = &e; return true; }
                    return false;
                });
                if (!ok || g->broken || !m) { g->broken = true; g->cv.notify_all(); r = ncclSystemError; break; }
                if (m->bytes != rc.bytes) { g->broken = true; g->cv.notify_all(); r = ncclInvalidUsage; break; }
                m->state = 1;                                   // taken (deque references stay valid: only the front is ever popped)
            }
            const ncclResult_t cr = copy_now(rc.ptr, m->ptr, rc.bytes, st);
            {
                std::lock_guard<std::mutex> lk(g->m);
                m->state = 2;
                while (!box.empty() && box.front().state == 2) box.pop_front();
                --g->outstanding[rc.peer];
                g->cv.notify_all();
            }
            if (cr != ncclSuccess) r = cr;
        }
        {
            std::unique_lock<std::mutex> lk(g->m);
            const bool ok = g->cv.wait_for(lk, limit, [&] { return g->broken || g->outstanding[me] == 0; });
            if ((!ok || g->broken) && r == ncclSuccess) { g->broken = true; g->cv.notify_all(); r = ncclSystemError; }
        }
        return r;
    }
};

// the group registry: the first rank to name a group creates it, the others join
int loop_join(const char* group, int rank, int world, std::unique_ptr<Transport>& out) {
    std::lock_guard<std::mutex> lk(loop_registry_mutex);
    LoopGroup* g = nullptr;
    auto it = loop_registry.find(group);
    if (it != loop_registry.end() && it->second->broken) {      // a group that timed out stays broken for its members; a fresh create under the same name starts clean
        loop_registry.erase(it);
        it = loop_registry.end();
    }
    if (it == loop_registry.end()) {
        g = new LoopGroup();
        g->name = group; g->world = world; g->present.assign(world, 0); g->mail.resize((size_t)world * world); g->outstanding.assign(world, 0);
        g->timeout_s = timeout_from_env(20.0);
        loop_registry[group] = g;
    } else {
        g = it->second;
        if (g->world != world || g->joined >= world) { avt_set_error("avt_shard_create_loopback: group exists with another world size, or is full"); return 1; }
        if (g->present[rank]) { avt_set_error("avt_shard_create_loopback: this rank is already a member of the group"); return 1; }
    }
    ++g->joined; ++g->refs; g->present[rank] = 1;
    out.reset(new LoopTransport(g, rank));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Shared-memory transport: the ranks are PROCESSES of one node, a transfer is staged through a POSIX shared-memory segment
// (device -> segment -> device).  RCCL refuses two ranks on one GPU ("Duplicate GPU detected"), so on a one-GPU box
// the launch path a real node takes - bench.py --gpus N -> torch.distributed.run -> one process per rank -> avt_shard ->
// scatter -> optimize -> all-gather - could never run with N > 1; with this transport it does (tests/test_gpu_bench_ranks.py,
// AVT_BENCH_SHARE_GPU0=1), and a node without RCCL still has a batch split.  It is NOT the fast path: every byte crosses
// the host twice.
// Layout: a header, then one mailbox per ordered pair (source, destination): two sequence counters and SHM_CHUNK bytes.
// A message travels as chunks (a chunk never spans messages); chunk i of a box is written when chunk i - 1 has been taken
// (seq_empty == i) and published by seq_full = i + 1.
// One progress loop serves all pending sends and receives of a call, so grouped exchanges cannot deadlock; a peer that
// never arrives makes the call fail after AVT_SHARD_LOOPBACK_TIMEOUT_S (default 60 s here) and marks the segment broken.
// ---------------------------------------------------------------------------------------------------------------------
constexpr size_t SHM_CHUNK = 1u << 20;
constexpr unsigned SHM_MAGIC = 0x41565453u;      // "AVTS"
struct ShmHeader {
    std::atomic<unsigned> magic;
    std::atomic<int> attached, broken;
    int world;
    unsigned long long chunk;
    char pad[40];
};
struct ShmBox {
    std::atomic<unsigned long long> seq_full, seq_empty;      // chunks published by the source / taken by the destination
    unsigned long long bytes;                                  // payload of the chunk in flight
    char pad[40];
};
static_assert(sizeof(ShmHeader) == 64 && sizeof(ShmBox) == 64, "shared-memory transport: 64-byte records");
size_t shm_bytes(int world) { return sizeof(ShmHeader) + (sizeof(ShmBox) + SHM_CHUNK) * (size_t)world * world; }

struct ShmTransport final : P2pTransport {
    void* base; size_t map_bytes;
    double timeout_s;
    std::vector<unsigned long long> sent, taken;              // per peer: chunks I published to it / took from it
    ShmTransport(void* base_, size_t map_bytes_, int rank_, int world_, double timeout_s_)
        : P2pTransport(rank_, world_), base(base_), map_bytes(map_bytes_), timeout_s(timeout_s_), sent(world_, 0), taken(world_, 0) {}
    ~ShmTransport() override { munmap(base, map_bytes); }
    ShmHeader* hdr() const { return (ShmHeader*)base; }
    ShmBox* box(int src, int dst) const { return (ShmBox*)((char*)base + sizeof(ShmHeader)) + (size_t)src * world + dst; }
    char* payload(int src, int dst) const { return (char*)base + sizeof(ShmHeader) + sizeof(ShmBox) * (size_t)world * world + ((size_t)src * world + dst) * SHM_CHUNK; }
    const char* error_string(ncclResult_t r) const override {
        return r == ncclSuccess ? "no error" : r == ncclSystemError ? "shared-memory transport: a rank did not arrive (time-out); the segment is broken"
             : r == ncclInvalidUsage ? "shared-memory transport: the two ends of a transfer disagree about its size" : "shared-memory transport: device copy failed";
    }
    std::string backend() const override { return "shared memory (processes of one node, staged through the host)"; }
    ncclResult_t complete(std::vector<Xfer>& sends, std::vector<Xfer>& recvs, hipStream_t st) override {
        if (hipStreamSynchronize(st) != hipSuccess) return ncclUnhandledCudaError;      // what I send is ready
        if (hdr()->broken.load(std::memory_order_acquire)) return ncclSystemError;
        auto t0 = std::chrono::steady_clock::now();
        size_t left = 0;
        for (auto& x : sends) left += x.bytes == 0 ? 0 : 1;
        for (auto& x : recvs) left += x.bytes == 0 ? 0 : 1;
        std::vector<char> busy_send(world), busy_recv(world);
        while (left) {
            bool moved = false;
            std::fill(busy_send.begin(), busy_send.end(), 0); std::fill(busy_recv.begin(), busy_recv.end(), 0);
            for (auto& x : sends) {
                if (x.done == x.bytes) continue;
                if (busy_send[x.peer]) continue;                     // an earlier message to this peer goes first
                busy_send[x.peer] = 1;
                ShmBox* b = box(rank, x.peer);
                if (b->seq_empty.load(std::memory_order_acquire) != sent[x.peer]) continue;      // the previous chunk is still in the box
                const size_t n = std::min(SHM_CHUNK, x.bytes - x.done);
                if (hipMemcpy(payload(rank, x.peer), x.ptr + x.done, n, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
                b->bytes = n;
                b->seq_full.store(++sent[x.peer], std::memory_order_release);
                x.done += n; moved = true;
                if (x.done == x.bytes) --left;
            }
            for (auto& x : recvs) {
                if (x.done == x.bytes) continue;
                if (busy_recv[x.peer]) continue;
                busy_recv[x.peer] = 1;
                ShmBox* b = box(x.peer, rank);
                if (b->seq_full.load(std::memory_order_acquire) != taken[x.peer] + 1) continue;   // nothing new from this peer
                const size_t n = (size_t)b->bytes;
                if (n != std::min(SHM_CHUNK, x.bytes - x.done)) { hdr()->broken.store(1, std::memory_order_release); return ncclInvalidUsage; }   // the two ends disagree about a message size
                if (hipMemcpy(x.ptr + x.done, payload(x.peer, rank), n, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
                b->seq_empty.store(++taken[x.peer], std::memory_order_release);
                x.done += n; moved = true;
                if (x.done == x.bytes) --left;
            }
            if (!left) break;
            if (moved) t0 = std::chrono::steady_clock::now();      //  the time-out bounds INACTIVITY, not the length of a long exchange
            else {
                if (hdr()->broken.load(std::memory_order_acquire)) return ncclSystemError;
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
                    hdr()->broken.store(1, std::memory_order_release);
                    return ncclSystemError;
                }
                std::this_thread::sleep_for(std::chrono::microseconds(20));
            }
        }
        return ncclSuccess;
    }
};

// the segment rendezvous: rank 0 creates and initialises the segment named after the rendezvous bytes, everybody maps it, and all wait
// until all are attached (creation is collective, like ncclCommInitRank)
int shm_attach(const char id[AVT_SHARD_ID_BYTES], int rank, int world, std::unique_ptr<Transport>& out) {
    unsigned long long h = 1469598103934665603ull;      // FNV-1a of the rendezvous bytes names the segment
    for (int i = 0; i < AVT_SHARD_ID_BYTES; ++i) { h ^= (unsigned char)id[i]; h *= 1099511628211ull; }
    char name[64];
    snprintf(name, sizeof name, "/avt_shard_%016llx", h);
    const double timeout_s = timeout_from_env(60.0);
    const size_t bytes = shm_bytes(world);
    const auto t0 = std::chrono::steady_clock::now();
    auto late = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s; };
    int fd = -1;
    if (rank == 0) {
        fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
        if (fd < 0 || ftruncate(fd, (off_t)bytes) != 0) {
            avt_set_error(std::string("avt_shard_create_shm: cannot create the segment ") + name + ": " + strerror(errno));
            if (fd >= 0) { close(fd); shm_unlink(name); }
            return 1;
        }
    } else {
        struct stat sb;
        while (true) {      // rank 0 creates and sizes it
            fd = shm_open(name, O_RDWR, 0600);
            if (fd >= 0 && fstat(fd, &sb) == 0 && (size_t)sb.st_size >= bytes) break;
            if (fd >= 0) { close(fd); fd = -1; }
            if (late()) { avt_set_error(std::string("avt_shard_create_shm: rank 0 never created the segment ") + name); return 1; }
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
    }
    void* base = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (base == MAP_FAILED) { avt_set_error(std::string("avt_shard_create_shm: mmap: ") + strerror(errno)); if (rank == 0) shm_unlink(name); return 1; }
    std::unique_ptr<ShmTransport> sc(new ShmTransport(base, bytes, rank, world, timeout_s));      // (unmaps when it goes)
    ShmHeader* hd = sc->hdr();
    if (rank == 0) {      // (a fresh segment is zero-filled: counters start at 0)
        hd->world = world; hd->chunk = SHM_CHUNK;
        hd->magic.store(SHM_MAGIC, std::memory_order_release);
    } else {
        while (hd->magic.load(std::memory_order_acquire) != SHM_MAGIC) {
            if (late()) { avt_set_error("avt_shard_create_shm: the segment was never initialised"); return 1; }
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
        if (hd->world != world || hd->chunk != SHM_CHUNK) { avt_set_error("avt_shard_create_shm: the segment belongs to a group of another shape"); return 1; }
    }
    hd->attached.fetch_add(1, std::memory_order_acq_rel);
    while (hd->attached.load(std::memory_order_acquire) < world) {
        if (late()) {
            avt_set_error("avt_shard_create_shm: not every rank attached in time");
            if (rank == 0) shm_unlink(name);
            return 1;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    if (rank == 0) shm_unlink(name);      // everybody holds a mapping: the name can go, the memory lives until the last unmap
    out = std::move(sc);
    return 0;
}

}  // namespace

struct avt_shard {
    std::unique_ptr<Transport> tr;
    int device = 0, rank = 0, world = 1;
    hipStream_t stream = nullptr;          // exchanges that happen before a context exists (model broadcast)
    std::string backend;
    // result gather: per-rank send block and the gathered block, device
    DevBuf<double> d_send, d_recv;         // one rank block / `world` of them, in doubles
    const double* gathered = nullptr;      // where the last gather left every rank's block (d_recv; one rank: the context's own result records)
    DevBuf<char> d_stage, d_stage2;        // scatter / broadcast staging, bytes
    hipStream_t gather_stream = nullptr;   // the stream the last all-gather was enqueued on
    bool self_exchange = false;            // avt_shard_set_self_exchange: a rank's own blocks go through the transport as well (dry runs)
};

namespace {

// a transport's status: anything but success becomes the last error, "<what>: <the transport's text>", and 1
int nccl_ok(const avt_shard* s, const char* what, ncclResult_t r) {
    if (r == ncclSuccess) return 0;
    avt_set_error(std::string(what) + ": " + s->tr->error_string(r));
    return 1;
}
#define NCCL_OK(s, expr) do { if (nccl_ok((s), #expr, (expr))) return 1; } while (0)

// a staging block of at least `bytes` (discarded when it grows); never under 256, so that the control words of successive
// calls (64, 8 (world + 1) .. bytes) share one allocation
int grow(DevBuf<char>& b, size_t bytes) { return b.reserve(std::max<size_t>(bytes, 256)); }

// the clouds of n points in a staging block: [3 n doubles | n ints] (+ 64 bytes of slack)
struct CloudBlock { double* data = nullptr; int* lab = nullptr; };
int carve(DevBuf<char>& b, size_t n, CloudBlock& out) {
    if (grow(b, n * 28 + 64)) return 1;
    out.data = (double*)b.p; out.lab = (int*)(b.p + n * 24);
    return 0;
}

// One round of control words through the device block `dev` on `st`: `up_bytes` host bytes up to dev + up_at, the collective, `down_bytes`
// down from dev, ONE synchronise.  (0 bytes: that copy is not made.)
template <class F>
int exchange_words(avt_shard* s, hipStream_t st, const char* what, char* dev, size_t up_at, const void* up, size_t up_bytes, F&& collective,
                   void* down, size_t down_bytes) {
    if (up_bytes) AVT_HIP(hipMemcpyAsync(dev + up_at, up, up_bytes, hipMemcpyHostToDevice, st));
    if (nccl_ok(s, what, collective())) return 1;
    if (down_bytes) AVT_HIP(hipMemcpyAsync(down, dev, down_bytes, hipMemcpyDeviceToHost, st));
    AVT_HIP(hipStreamSynchronize(st));
    return 0;
}

// the shape of a result gather of B frames: rows of a rank block, doubles of a row, doubles of a rank block
struct GatherShape {
    int per, stride;
    size_t blk;
    GatherShape(const avt_shard* s, const avt_ctx* c, int B) : per((B + s->world - 1) / s->world), stride(result_stride(c->dm.d)), blk((size_t)per * stride) {}
};

// what every create checks first, with the entry point's name in its texts.  1: bad argument (or, need_rccl, no librccl); 2: no such device
int check_create(const char* who, int device, int rank, int world, const void* rendezvous, avt_shard** out, bool need_rccl = false) {
    if (!rendezvous || !out || world <= 0 || rank < 0 || rank >= world) { avt_set_error(std::string(who) + ": bad argument"); return 1; }
    if (need_rccl && !rccl_api()) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { avt_set_error(std::string(who) + ": device index out of range"); return 2; }
    return 0;
}

// the handle around its transport: on `device`, where `connect` builds the transport (the last error is its to set), with the stream;
// whatever fails, everything made so far is released
template <class F>
int finish_create(const char* who, int device, int rank, int world, avt_shard** out, F&& connect) {
    AVT_HIP(hipSetDevice(device));
    std::unique_ptr<avt_shard> s(new avt_shard());
    s->device = device; s->rank = rank; s->world = world;
    if (connect(s->tr)) return 1;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { avt_set_error(std::string(who) + ": hipStreamCreate failed"); return 1; }
    s->backend = s->tr->backend();
    *out = s.release();
    return 0;
}

}  // namespace

extern "C" int avt_shard_unique_id(char id[AVT_SHARD_ID_BYTES]) {
    return avt_guard("avt_shard_unique_id", [&]() -> int {
        RcclApi* a = rccl_api();
        if (!a) return 1;
        if (!id) { avt_set_error("avt_shard_unique_id: null argument"); return 1; }
        static_assert(AVT_SHARD_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
        ncclUniqueId u;
        const ncclResult_t r = a->GetUniqueId(&u);
        if (r != ncclSuccess) { avt_set_error(std::string("ncclGetUniqueId: ") + a->GetErrorString(r)); return 1; }
        std::memcpy(id, u.internal, AVT_SHARD_ID_BYTES);
        return 0;
    });
}

extern "C" int avt_shard_create(int device, int rank, int world, const char id[AVT_SHARD_ID_BYTES], avt_shard** out) {
    return avt_guard("avt_shard_create", [&]() -> int {
        if (const int rc = check_create("avt_shard_create", device, rank, world, id, out, true)) return rc;
        return finish_create("avt_shard_create", device, rank, world, out, [&](std::unique_ptr<Transport>& tr) {
            std::unique_ptr<RcclTransport> t(new RcclTransport(rccl_api()));
            ncclUniqueId u;
            std::memcpy(u.internal, id, AVT_SHARD_ID_BYTES);
            const ncclResult_t r = t->a->CommInitRank(&t->comm, world, u, rank);
            if (r != ncclSuccess) { avt_set_error(std::string("ncclCommInitRank: ") + t->a->GetErrorString(r)); return 1; }
            tr = std::move(t);
            return 0;
        });
    });
}

extern "C" int avt_shard_create_loopback(int device, int rank, int world, const char* group, avt_shard** out) {
    return avt_guard("avt_shard_create_loopback", [&]() -> int {
        if (const int rc = check_create("avt_shard_create_loopback", device, rank, world, group, out)) return rc;
        return finish_create("avt_shard_create_loopback", device, rank, world, out, [&](std::unique_ptr<Transport>& tr) { return loop_join(group, rank, world, tr); });
    });
}

extern "C" int avt_shard_create_shm(int device, int rank, int world, const char id[AVT_SHARD_ID_BYTES], avt_shard** out) {
    return avt_guard("avt_shard_create_shm", [&]() -> int {
        if (world > 64) { avt_set_error("avt_shard_create_shm: bad argument"); return 1; }      // (a segment holds world x world mailboxes of 1 MiB)
        if (const int rc = check_create("avt_shard_create_shm", device, rank, world, id, out)) return rc;
        return finish_create("avt_shard_create_shm", device, rank, world, out, [&](std::unique_ptr<Transport>& tr) { return shm_attach(id, rank, world, tr); });
    });
}

extern "C" void avt_shard_destroy(avt_shard* s) {
    if (!s) return;
    (void)avt_guard("avt_shard_destroy", [&]() -> int {
        (void)hipSetDevice(s->device);
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        s->tr.reset();
        // the blocks go with `delete`, after the stream: hipFree waits for the device, so nothing is queued on them either way
        if (s->stream) (void)hipStreamDestroy(s->stream);
        delete s;
        return 0;
    });
}

extern "C" int avt_shard_rank(const avt_shard* s) { return s ? s->rank : -1; }
extern "C" int avt_shard_world(const avt_shard* s) { return s ? s->world : 0; }
extern "C" const char* avt_shard_backend(const avt_shard* s) { return s ? s->backend.c_str() : ""; }

extern "C" int avt_shard_broadcast_model(avt_shard* s, int root, const avt_model_desc* desc, avt_model** out) {
    return avt_guard("avt_shard_broadcast_model", [&]() -> int {
        if (!s || !out || root < 0 || root >= s->world) { avt_set_error("avt_shard_broadcast_model: bad argument"); return 1; }
        AVT_HIP(hipSetDevice(s->device));
        // 1. size of the packed block (8 bytes), 2. the block itself; both as device-buffer broadcasts
        unsigned long long nbytes = 0;
        std::vector<char> host;
        if (s->rank == root) {
            size_t n = 0;
            if (avt_model_pack_size(desc, &n)) return 1;
            host.resize(n);
            if (avt_model_pack(desc, host.data(), n)) return 1;
            nbytes = n;
        }
        if (grow(s->d_stage2, 64)) return 1;
        if (exchange_words(s, s->stream, "ncclBroadcast of the model's size", s->d_stage2, 0, &nbytes, 8,
                           [&] { return s->tr->broadcast(s->d_stage2, s->d_stage2, 8, ncclChar, root, s->stream); }, &nbytes, 8)) return 1;
        if (nbytes < sizeof(PackHeader) || nbytes > (1ull << 32)) { avt_set_error("avt_shard_broadcast_model: implausible model size received"); return 1; }
        if (grow(s->d_stage, nbytes)) return 1;
        host.resize(nbytes);
        if (exchange_words(s, s->stream, "ncclBroadcast of the packed model", s->d_stage, 0, host.data(), s->rank == root ? nbytes : 0,
                           [&] { return s->tr->broadcast(s->d_stage, s->d_stage, nbytes, ncclChar, root, s->stream); }, host.data(), nbytes)) return 1;
        return avt_model_unpack(host.data(), host.size(), out);
    });
}

namespace {

// one avt_shard_scatter_frames call: its arguments and what each step leaves for the next
struct Scatter {
    avt_shard* s; avt_ctx* c;
    int root, B;
    const double* data; const int *labels, *offs; const double *p, *q, *w;      // the root's host arrays
    std::vector<double> tab;            // [B point counts as doubles | B x xsize states]; on every rank after the table step
    std::vector<int> cnt;               // points of every frame
    std::vector<long long> rank_pts;    // points of every rank's share
    std::string my_error;               // what THIS rank holds against the batch
    CloudBlock share;                   // this rank's clouds on the device, after the cloud step
    bool is_root() const { return s->rank == root; }

    // ---- 1. frame table and start states: one small broadcast, and what this rank holds against the batch
    int table() {
        const AvtDims& d = c->dm.d;
        const int W = s->world, xs = d.xsize;
        const size_t tab_n = (size_t)B * (1 + xs);
        tab.assign(tab_n, 0.0);
        if (is_root()) {
            if (!data || !labels || !offs || !p || !q || !w) my_error = "avt_shard_scatter_frames: root needs all host arrays";
            for (int f = 0; f < B && my_error.empty(); ++f) {
                const int n = offs[f + 1] - offs[f];
                if (n < 0) { my_error = "avt_shard_scatter_frames: frame_offsets not monotone"; break; }
                tab[f] = (double)n;
                pack_state_row(d, &tab[(size_t)B + (size_t)f * xs], p, q, w, f);
            }
            if (!my_error.empty()) tab[0] = -1.0;          // a point count cannot be negative: "the root's batch is unusable"
        }
        if (grow(s->d_stage2, std::max<size_t>(tab_n, (size_t)W + 1) * 8)) return 1;   // (allocation failure: nothing a peer could wait for has begun)
        if (exchange_words(s, c->stream, "ncclBroadcast of the frame table", s->d_stage2, 0, tab.data(), is_root() ? tab_n * 8 : 0,
                           [&] { return s->tr->broadcast(s->d_stage2, s->d_stage2, tab_n, ncclDouble, root, c->stream); }, tab.data(), tab_n * 8)) return 1;
        cnt.assign(B, 0);
        rank_pts.assign(W, 0);
        const bool root_bad = tab[0] < 0.0;
        if (root_bad && my_error.empty()) my_error = "avt_shard_scatter_frames: the root rank rejected the batch";
        if (my_error.empty() && avt_shard_local_count(B, s->rank, W) > c->fb.max_frames) my_error = "avt_shard_scatter_frames: this rank's share exceeds the context's max_frames";
        for (int f = 0; f < B && !root_bad; ++f) {
            cnt[f] = (int)tab[f];
            // every rank checks ITS frames against ITS context (contexts may differ in size)
            if (f % W == s->rank && my_error.empty() && (cnt[f] < 0 || cnt[f] > c->fb.max_points))
                my_error = "avt_shard_scatter_frames: a frame has more points than max_points_per_frame";
            rank_pts[f % W] += std::max(cnt[f], 0);
        }
        return 0;
    }

    // ---- 2. agreement: one double per rank (0 = fine), everybody sees everybody's; one bad rank and every rank leaves with nothing exchanged
    int agree() {
        const int W = s->world;
        std::vector<double> flags((size_t)W + 1, 0.0);
        flags[W] = my_error.empty() ? 0.0 : 1.0;
        double* dflag = (double*)s->d_stage2.p;
        if (exchange_words(s, c->stream, "ncclAllGather of the agreement flags", s->d_stage2, (size_t)W * 8, &flags[W], 8,
                           [&] { return s->tr->all_gather(dflag + W, dflag, 1, ncclDouble, c->stream); }, flags.data(), (size_t)W * 8)) return 1;
        int bad_rank = -1;
        for (int r = 0; r < W; ++r) if (flags[r] != 0.0 && bad_rank < 0) bad_rank = r;
        if (bad_rank < 0) return 0;
        c->nframes = 0; c->frames_valid = c->state_valid = false;
        avt_set_error(!my_error.empty() ? my_error : "avt_shard_scatter_frames: rank " + std::to_string(bad_rank) + " rejected the batch; nothing was exchanged");
        return 1;
    }

    // ---- 3. clouds: the root permutes the batch so that every rank's frames are contiguous (rank-major, then local order), uploads it once
    // and sends each rank its block: [3 n doubles | n ints] -> two sends per peer, one group
    int clouds() {
        const int W = s->world;
        hipStream_t st = c->stream;
        std::vector<long long> rank_off(W + 1, 0);
        for (int r = 0; r < W; ++r) rank_off[r + 1] = rank_off[r] + rank_pts[r];
        const long long total = rank_off[W], mine = rank_pts[s->rank];
        CloudBlock all;            // the root: the whole permuted batch; another rank: its share
        if (is_root()) {
            std::vector<double> hd((size_t)total * 3);
            std::vector<int> hl((size_t)total);
            std::vector<long long> cur(rank_off.begin(), rank_off.end() - 1);
            for (int f = 0; f < B; ++f) {
                const int r = f % W, n = cnt[f];
                std::memcpy(&hd[(size_t)cur[r] * 3], data + (size_t)offs[f] * 3, (size_t)n * 24);
                std::memcpy(&hl[(size_t)cur[r]], labels + offs[f], (size_t)n * 4);
                cur[r] += n;
            }
            if (carve(s->d_stage, (size_t)total, all)) return 1;
            if (total) {
                AVT_HIP(hipMemcpyAsync(all.data, hd.data(), (size_t)total * 24, hipMemcpyHostToDevice, st));
                AVT_HIP(hipMemcpyAsync(all.lab, hl.data(), (size_t)total * 4, hipMemcpyHostToDevice, st));
            }
            AVT_HIP(hipStreamSynchronize(st));   // the host vectors go out of scope below
            share.data = all.data + rank_off[s->rank] * 3; share.lab = all.lab + rank_off[s->rank];
        } else {
            if (carve(s->d_stage, (size_t)mine, all)) return 1;
            share = all;
        }
        // dry runs (avt_shard_set_self_exchange): push the root's own block through the transport too, into the control words' block
        const bool self_loop = is_root() && s->self_exchange && mine;
        CloudBlock loop;
        if (self_loop && carve(s->d_stage2, (size_t)mine, loop)) return 1;
        NCCL_OK(s, s->tr->group_start());
        if (is_root()) {
            for (int r = 0; r < W; ++r) {
                if (rank_pts[r] == 0 || (r == s->rank && !s->self_exchange)) continue;
                NCCL_OK(s, s->tr->send(all.data + rank_off[r] * 3, (size_t)rank_pts[r] * 3, ncclDouble, r, st));
                NCCL_OK(s, s->tr->send(all.lab + rank_off[r], (size_t)rank_pts[r], ncclInt32, r, st));
            }
            if (self_loop) share = loop;
        }
        if ((!is_root() || self_loop) && mine) {
            NCCL_OK(s, s->tr->recv(share.data, (size_t)mine * 3, ncclDouble, root, st));
            NCCL_OK(s, s->tr->recv(share.lab, (size_t)mine, ncclInt32, root, st));
        }
        NCCL_OK(s, s->tr->group_end());
        return 0;
    }

    // ---- 4. install this rank's frames in the context's resident buffers (device-to-device) and its start states
    int install() {
        const AvtDims& d = c->dm.d;
        const int W = s->world, nloc = avt_shard_local_count(B, s->rank, W);
        std::vector<int> lcnt(nloc);
        std::vector<double> lp((size_t)nloc * 3), lq((size_t)nloc * 4 * d.J), lw((size_t)nloc * d.K);
        for (int i = 0; i < nloc; ++i) {
            const int f = avt_shard_global_frame(i, s->rank, W);
            lcnt[i] = cnt[f];
            unpack_state_row(d, &tab[(size_t)B + (size_t)f * d.xsize], lp.data(), lq.data(), lw.data(), i);
        }
        if (nloc == 0) {       // a rank without frames (B < W): nothing resident, and a later gather must see exactly that
            c->nframes = 0; c->frames_valid = c->state_valid = false;
        } else {
            if (avt_internal_install_frames(c, nloc, lcnt.data(), share.data, share.lab, 1)) return 1;
            if (avt_state_upload(c, nloc, lp.data(), lq.data(), lw.data())) return 1;
        }
        AVT_HIP(hipStreamSynchronize(c->stream));
        return 0;
    }
};

}  // namespace

extern "C" int avt_shard_scatter_frames(avt_shard* s, avt_ctx* c, int root, int B, const double* data, const int* labels,
                                        const int* offs, const double* p, const double* q, const double* w) {
    return avt_guard("avt_shard_scatter_frames", [&]() -> int {
        if (!s || !c || root < 0 || root >= s->world || B <= 0) { avt_set_error("avt_shard_scatter_frames: bad argument"); return 1; }
        AVT_HIP(hipSetDevice(s->device));
        // A rank that leaves before a collective its peers enter blocks them for ever.  Everything that can be wrong on ONE rank
        // only - the root's arguments, a context too small for this rank's share - is therefore carried INTO the exchange and all
        // ranks leave together: the root marks a bad batch in the table it broadcasts, and every rank contributes an ok / not-ok
        // word to a one-double all-gather before any cloud moves.
        Scatter x{s, c, root, B, data, labels, offs, p, q, w};
        if (x.table() || x.agree() || x.clouds()) return 1;
        return x.install();
    });
}

extern "C" int avt_shard_gather_enqueue(avt_shard* s, avt_ctx* c, int B) {
    return avt_guard("avt_shard_gather_enqueue", [&]() -> int {
        if (!s || !c || B <= 0) { avt_set_error("avt_shard_gather_enqueue: bad argument"); return 1; }
        const GatherShape g(s, c, B);
        const int W = s->world, per = g.per, stride = g.stride;
        const size_t blk = g.blk;
        const int nloc = avt_shard_local_count(B, s->rank, W);
        // (a rank whose context does not hold its share still takes part in the all-gather - its peers are on their way into it - with
        // its rows marked faulty, and reports the error afterwards; every rank's download then fails on those rows)
        const bool mismatch = nloc != (c->frames_valid ? c->nframes : 0);
        AVT_HIP(hipSetDevice(s->device));
        if (s->d_send.cap < blk || s->d_recv.cap < blk * W) {   // each on its own: a failed allocation leaves that block empty
            AVT_HIP(hipStreamSynchronize(c->stream));
            AVT_HIP(hipStreamSynchronize(s->stream));
            if (s->d_send.reserve(blk) || s->d_recv.reserve(blk * W)) return 1;
            AVT_HIP(hipMemsetAsync(s->d_send, 0, blk * 8, c->stream));
        }
        // Packing kernel and all-gather go behind optimize() on the context's stream.  Measured on one MI355X (bench.py, one frame
        // per step, 0.62 ms): this costs 6 us per step; putting the all-gather on the shard's own stream instead - so that the
        // exchange of step k overlaps step k+1 - costs 25 us, because the event record / cross-stream wait the hand-over needs
        // sit in the context stream's critical path (double-buffering the send block and waiting on the host: 24 us).
        // (avt_shard_set_self_exchange - the dry-run switch that pushes a lone rank's own blocks through the transport - keeps the one-rank all-gather too)
        const bool direct = W == 1 && !mismatch && !s->self_exchange;
        if (mismatch) {
            std::vector<double> rows(blk, 0.0);
            for (int i = 0; i < per; ++i) rows[(size_t)i * stride + c->dm.d.xsize + AVT_RESULT_FAULT] = (double)AVT_FAULT_NOT_RESIDENT;
            AVT_HIP(hipMemcpyAsync(s->d_send, rows.data(), blk * 8, hipMemcpyHostToDevice, c->stream));
            AVT_HIP(hipStreamSynchronize(c->stream));
        } else if (nloc && !c->results_fresh) {      // (no optimize() in front: the records are made now)
            launch_pack_results(c, nloc);
            c->results_fresh = true;
        }
        // The result records (p, q, w, statistics, fault word per resident frame) are written by the k_lbs launch that closes optimize()
        // (FrameBuffers::results): they ARE the send block.  One rank: they are the gathered block as well - an all-gather over one rank is a
        // device-to-device copy kernel on the stream, 4.3 us per step for the identity.
        const double* send = (mismatch || (size_t)per > (size_t)c->fb.max_frames) ? s->d_send.p : c->fb.results;
        if (!mismatch && send == s->d_send && nloc) AVT_HIP(hipMemcpyAsync(s->d_send, c->fb.results, (size_t)nloc * stride * 8, hipMemcpyDeviceToDevice, c->stream));
        //  ... as a SNAPSHOT, like every other world size: enqueue -> optimize -> download returns the rows of the call the gather was enqueued
        // behind, not the later call's (include/avt_shard.h: "into a device buffer owned by the shard"); one rank: a plain device-to-device copy
        if (!direct) NCCL_OK(s, s->tr->all_gather(send, s->d_recv, blk, ncclDouble, c->stream));
        else if (nloc) AVT_HIP(hipMemcpyAsync(s->d_recv, send, (size_t)nloc * stride * 8, hipMemcpyDeviceToDevice, c->stream));
        s->gathered = s->d_recv;
        s->gather_stream = c->stream;
        if (mismatch) { avt_set_error("avt_shard_gather_enqueue: resident frames differ from this rank's share of the batch (its rows were gathered as faulty)"); return 1; }
        return 0;
    });
}

extern "C" int avt_shard_set_self_exchange(avt_shard* s, int on) {
    return avt_guard("avt_shard_set_self_exchange", [&]() -> int {
        if (!s) { avt_set_error("avt_shard_set_self_exchange: null argument"); return 1; }
        s->self_exchange = on != 0;
        return 0;
    });
}

extern "C" int avt_shard_gather_wait(avt_shard* s) {
    return avt_guard("avt_shard_gather_wait", [&]() -> int {
        if (!s) { avt_set_error("avt_shard_gather_wait: null argument"); return 1; }
        AVT_HIP(hipSetDevice(s->device));
        if (s->gather_stream) AVT_HIP(hipStreamSynchronize(s->gather_stream));
        return 0;
    });
}

extern "C" int avt_shard_gather_download(avt_shard* s, avt_ctx* c, int B, double* p, double* q, double* w, avt_stats* stats) {
    return avt_guard("avt_shard_gather_download", [&]() -> int {
        if (!s || !c || B <= 0) { avt_set_error("avt_shard_gather_download: bad argument"); return 1; }
        const AvtDims& d = c->dm.d;
        const GatherShape g(s, c, B);
        const int W = s->world;
        if (s->d_recv.cap < g.blk * W || !s->gathered) { avt_set_error("avt_shard_gather_download: nothing was gathered"); return 1; }
        AVT_HIP(hipSetDevice(s->device));
        std::vector<double> host(g.blk * W);
        AVT_HIP(hipMemcpyAsync(host.data(), s->gathered, host.size() * 8, hipMemcpyDeviceToHost, c->stream));   // behind the all-gather
        AVT_HIP(hipStreamSynchronize(c->stream));
        int bad = -1;
        for (int f = 0; f < B; ++f)       // the owning rank's device fault bits travelled with the result
            if (unpack_result_row(d, &host[(size_t)(f % W) * g.blk + (size_t)(f / W) * g.stride], p, q, w, stats, f) && bad < 0) bad = f;
        if (bad >= 0) {
            (void)avt_internal_clear_faults(c);      // reported once
            avt_set_error("avt_shard_gather_download: frame " + std::to_string(bad) + " carries a device fault (rank " + std::to_string(bad % W) + "); its result is not valid");
            return AVT_STATUS_DEVICE_FAULT;
        }
        return 0;
    });
}

extern "C" int avt_shard_gather_results(avt_shard* s, avt_ctx* c, int B, double* p, double* q, double* w, avt_stats* stats) {
    if (avt_shard_gather_enqueue(s, c, B)) return 1;
    return avt_shard_gather_download(s, c, B, p, q, w, stats);
}

extern "C" int avt_shard_barrier(avt_shard* s, avt_ctx* c) {
    return avt_guard("avt_shard_barrier", [&]() -> int {
        if (!s) { avt_set_error("avt_shard_barrier: null argument"); return 1; }
        AVT_HIP(hipSetDevice(s->device));
        hipStream_t st = c ? c->stream : s->stream;
        if (grow(s->d_stage2, (size_t)(s->world + 1) * 8)) return 1;
        double* b = (double*)s->d_stage2.p;
        return exchange_words(s, st, "ncclAllGather of the barrier", s->d_stage2, 0, nullptr, 0,
                              [&] { return s->tr->all_gather(b + s->world, b, 1, ncclDouble, st); }, nullptr, 0);
    });
}
