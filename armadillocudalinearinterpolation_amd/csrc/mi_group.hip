// Multi-GPU behind the C ABI: one host process drives the GPUs of a node (the reference is single-GPU,
// EventDrivenMap.cu:80-94, Driver.cu:20).  A group holds one context (device + stream of its own) per shard.
//   * table interpolation: contiguous query shards, the table replicated on every device, no exchange unless the
//     caller wants every device to hold the whole result vector -- then an RCCL all-gather over xGMI
//     (ncclAllGather on the per-device communicators of ncclCommInitAll, one ncclGroupStart/End section);
//   * EventDrivenMap::ComputeF: realisation shards (the realisation is already the unit of work, EventDrivenMap.cu:196),
//     exchange = the partial block of MI_EDM_PARTIAL_LEN(S) doubles per shard.  In one process the blocks are already
//     on the host (pinned D2H at the end of each shard's pipeline), so the default adds them there in shard order;
//     MI_GROUP_REDUCE_RCCL does the same sum with ncclAllReduce on the devices (what one-process-per-GPU callers do
//     with torch.distributed, sharding.py).
// RCCL is bound at run time (dlopen): the library must not drag a second RCCL into a process that already carries
// PyTorch's.  A group may name the same device several times (rehearsal of the shard arithmetic on a box with fewer
// GPUs than shards): RCCL cannot form a communicator over duplicates, so such a group gathers with device-to-device
// copies and reduces on the host.
#include <dlfcn.h>

#include <cstdlib>
#include <initializer_list>
#include <new>
#include <set>
#include <type_traits>
#include <vector>

#include "mi_common.hpp"

// the few RCCL declarations used (rccl.h:236,260,339,611,678; kept local so that the header is not a build dependency)
typedef struct ncclComm* ncclComm_t;
typedef int ncclResult_t;
enum { mi_ncclFloat64 = 8, mi_ncclSum = 0 };

struct mi_group {
    std::vector<int> dev;
    std::vector<mi_ctx*> ctx;
    std::vector<hipEvent_t> done;      // per shard: its kernels of the current call have been enqueued up to here
    // created on first use (a group that never takes device-resident shards never has them):
    std::vector<hipEvent_t> pre;       // per shard: the caller's stream has been enqueued up to here (mi_group_wait_stream)
    std::vector<hipEvent_t> copied;    // per shard, repeated devices: its gather copies have been enqueued up to here
    bool distinct = true;
    int reduce_mode = 0;
    // RCCL, bound lazily
    void* lib = nullptr;
    bool rccl_tried = false;
    std::vector<ncclComm_t> comms;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    std::vector<double*> red_dev;      // MI_EDM partial blocks on the devices (RCCL reduce mode)
    // chunked gather (mi_group_set_gather_chunks): a second stream per member for the exchange, one event per chunk
    int gather_chunks = 1;
    std::vector<hipStream_t> gstream;
    std::vector<std::vector<hipEvent_t>> cdone;   // [member][chunk]: the chunk's kernel has been enqueued up to here
    std::vector<hipEvent_t> gdone;                // [member]: its exchange stream has been enqueued up to here
};

struct mi_group_grid1 {
    mi_group* g;
    std::vector<mi_grid1*> grid;
};

struct mi_group_grid2 {
    mi_group* g;
    std::vector<mi_grid2*> grid;
};

struct mi_group_edm {
    mi_group* g;
    mi_edm_params total;
    std::vector<mi_edm*> shard;
    std::vector<size_t> lo, hi;
};

namespace {

constexpr int kMaxSpikesG = 8;

mi_status bind_rccl(mi_group* g)
{
    if (g->comms.size() == g->dev.size()) return MI_OK;
    if (!g->distinct)
        return mi::fail(nullptr, MI_ERR_INVALID_ARG, "mi_group: RCCL needs distinct devices (this group repeats one)");
    if (!g->rccl_tried) {
        g->rccl_tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            g->lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (g->lib) break;
        }
        if (g->lib) {
            g->CommInitAll = (decltype(g->CommInitAll))dlsym(g->lib, "ncclCommInitAll");
            g->CommDestroy = (decltype(g->CommDestroy))dlsym(g->lib, "ncclCommDestroy");
            g->GetErrorString = (decltype(g->GetErrorString))dlsym(g->lib, "ncclGetErrorString");
            g->AllReduce = (decltype(g->AllReduce))dlsym(g->lib, "ncclAllReduce");
            g->AllGather = (decltype(g->AllGather))dlsym(g->lib, "ncclAllGather");
            g->GroupStart = (decltype(g->GroupStart))dlsym(g->lib, "ncclGroupStart");
            g->GroupEnd = (decltype(g->GroupEnd))dlsym(g->lib, "ncclGroupEnd");
            g->CommCount = (decltype(g->CommCount))dlsym(g->lib, "ncclCommCount");
            g->Broadcast = (decltype(g->Broadcast))dlsym(g->lib, "ncclBroadcast");
        }
    }
    if (!g->lib || !g->CommInitAll || !g->CommDestroy || !g->AllReduce || !g->AllGather || !g->GroupStart || !g->GroupEnd)
        return mi::fail(nullptr, MI_ERR_HIP, "mi_group: librccl.so could not be loaded (%s)", g->lib ? "symbol missing" : dlerror());
    g->comms.assign(g->dev.size(), nullptr);
    const ncclResult_t r = g->CommInitAll(g->comms.data(), (int)g->dev.size(), g->dev.data());
    if (r != 0) {
        g->comms.clear();
        return mi::fail(nullptr, MI_ERR_HIP, "ncclCommInitAll over %zu devices failed: %s", g->dev.size(),
                        g->GetErrorString ? g->GetErrorString(r) : "?");
    }
    return MI_OK;
}

// member r's event of a per-member vector that is filled on first use (the device of member r is current)
mi_status member_event(mi_group* g, std::vector<hipEvent_t>& v, size_t r, hipEvent_t* out)
{
    if (v.size() != g->ctx.size()) v.assign(g->ctx.size(), nullptr);
    if (!v[r]) MI_HIP(g->ctx[r], hipEventCreateWithFlags(&v[r], hipEventDisableTiming));
    *out = v[r];
    return MI_OK;
}

#define MI_NCCL(g, call)                                                                              \
    do {                                                                                              \
        const ncclResult_t r_ = (call);                                                               \
        if (r_ != 0)                                                                                  \
            return mi::fail(nullptr, MI_ERR_HIP, "%s failed: %s", #call,                              \
                            (g)->GetErrorString ? (g)->GetErrorString(r_) : "?");                     \
    } while (0)

// ---- host calls sharded over the members ---------------------------------------------------------------------------

struct HostRange {
    const void* p;
    size_t bytes;
};

// The ranges one call page-locked: add() keeps a range only when mi::pin_host gave this call a reference, release() gives
// back exactly those, once.  Only sharded_host_call holds one, and it releases behind its drain; the destructor is a backstop.
class HostPins {
public:
    HostPins() = default;
    HostPins(const HostPins&) = delete;
    HostPins& operator=(const HostPins&) = delete;
    ~HostPins() { release(); }
    void add(const HostRange& h)
    {
        // a range beyond kMax stays pageable: its copies take hipMemcpyAsync's blocking path
        if (count_ < kMax && mi::pin_host(h.p, h.bytes)) held_[count_++] = h.p;
    }
    void release()
    {
        for (int k = 0; k < count_; ++k) mi::unpin_host(held_[k]);
        count_ = 0;
    }

private:
    static constexpr int kMax = 4;
    const void* held_[kMax];
    int count_ = 0;
};

// scratch slots 0-2 of a member at the sizes its step needs (0: the slot is not used)
mi_status grow_slots(mi_ctx* c, size_t bytes0, size_t bytes1, size_t bytes2)
{
    mi_status st = mi::ensure_scratch(c, 0, bytes0);
    if (st == MI_OK) st = mi::ensure_scratch(c, 1, bytes1);
    if (st == MI_OK) st = mi::ensure_scratch(c, 2, bytes2);
    return st;
}

// The frame of every mi_group_*_host entry point (`who`).  `ranges` are page-locked when `pin`.  Members are visited in
// rank order; member r gets [lo, hi) = mi_shard_bounds(count, r, P), one with an empty shard is skipped, and
// enqueue(r, ctx, lo, hi, herr) runs with the member's device current: everything on the member's stream, nothing waits.
// It returns a callee's status and leaves a failed copy in herr.  The first failure of either kind (or of hipSetDevice, a
// copy error) ends the loop; afterwards(...), if given, is a second pass of the same shape that runs only when everything
// before it succeeded.  Then every member's stream is drained, whatever happened, and only then the pins go.  Reported:
// the callee's status with its own text, else the copy error, else the first failed synchronisation.
// MI_TEST_FAIL_GROUP_SHARD (error-path test hook): a copy error instead of the second member that has work, with the
// first one's copies and kernel enqueued.
template <class Enqueue, class Afterwards = std::nullptr_t>
mi_status sharded_host_call(mi_group* g, const char* who, size_t count, bool pin, std::initializer_list<HostRange> ranges,
                            Enqueue enqueue, Afterwards afterwards = nullptr)
{
    const int P = (int)g->ctx.size();
    HostPins pins;
    if (pin)
        for (const HostRange& h : ranges) pins.add(h);
    mi_status st = MI_OK;
    hipError_t herr = hipSuccess;
    const char* what = "";
    auto pass = [&](auto& step, bool fail_hook) {
        int busy = 0;
        for (int r = 0; r < P && st == MI_OK && herr == hipSuccess; ++r) {
            size_t lo, hi;
            mi_shard_bounds(count, r, P, &lo, &hi);
            if (hi == lo) continue;
            if (fail_hook && busy++ == 1) { herr = hipErrorUnknown; what = "MI_TEST_FAIL_GROUP_SHARD (error-path test hook): "; break; }
            herr = hipSetDevice(g->dev[r]);
            if (herr == hipSuccess) st = step(r, g->ctx[r], lo, hi, herr);
        }
    };
    pass(enqueue, getenv("MI_TEST_FAIL_GROUP_SHARD") != nullptr);
    if constexpr (!std::is_same<Afterwards, std::nullptr_t>::value) pass(afterwards, false);
    hipError_t esync = hipSuccess;
    for (int r = 0; r < P; ++r) {   // drain every stream before the ranges are released, on success or error
        (void)hipSetDevice(g->dev[r]);
        const hipError_t e = hipStreamSynchronize(g->ctx[r]->stream);
        if (e != hipSuccess && esync == hipSuccess) esync = e;
    }
    pins.release();
    if (st != MI_OK) return st;
    if (herr != hipSuccess) return mi::fail(nullptr, MI_ERR_HIP, "%s: copy failed: %s%s", who, what, hipGetErrorString(herr));
    if (esync != hipSuccess) return mi::fail(nullptr, MI_ERR_HIP, "%s: %s", who, hipGetErrorString(esync));
    return MI_OK;
}

}  // namespace

static mi_status gather_shards(mi_group* g, double* const* part_dev, double* const* gathered_dev, size_t n_per_shard);
static mi_status interp1_chunked_gather(mi_group* g, const mi_group_grid1* t, const double* const* xq_dev, double* const* yq_dev,
                                        size_t nq_per_shard, double extrap, double* const* gathered_dev);

extern "C" {

void mi_shard_bounds(size_t n, int rank, int world, size_t* lo, size_t* hi)
{
    // contiguous, balanced: the first n % world shards get one extra unit (= sharding.shard_bounds)
    const size_t w = world > 0 ? (size_t)world : 1, r = rank > 0 ? (size_t)rank : 0;
    const size_t base = n / w, rem = n % w;
    const size_t a = r * base + (r < rem ? r : rem);
    if (lo) *lo = a;
    if (hi) *hi = a + base + (r < rem ? 1 : 0);
}

mi_status mi_group_create(int ndev, const int* devices, mi_group** out)
{
    MI_REQUIRE(nullptr, out != nullptr, "mi_group_create: out is NULL");
    *out = nullptr;
    MI_REQUIRE(nullptr, ndev >= 1 && ndev <= 64, "mi_group_create: ndev=%d not in [1,64]", ndev);
    mi_group* g = new (std::nothrow) mi_group();
    if (!g) return mi::fail(nullptr, MI_ERR_NOMEM, "mi_group_create: out of host memory");
    std::set<int> seen;
    for (int r = 0; r < ndev; ++r) {
        const int d = devices ? devices[r] : r;
        g->dev.push_back(d);
        if (!seen.insert(d).second) g->distinct = false;
    }
    for (int r = 0; r < ndev; ++r) {
        mi_ctx* c = nullptr;
        mi_status st = mi_ctx_create(g->dev[r], &c);
        if (st == MI_OK) st = mi_ctx_own_stream(c);
        hipEvent_t ev = nullptr;
        if (st == MI_OK && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
            st = mi::fail(nullptr, MI_ERR_HIP, "mi_group_create: hipEventCreate failed on device %d", g->dev[r]);
        if (st != MI_OK) {
            if (c) mi_ctx_destroy(c);
            mi_group_destroy(g);
            return st;
        }
        // a group member works on the queries it is handed, in whatever order: no probe traffic between devices' calls
        g->ctx.push_back(c);
        g->done.push_back(ev);
    }
    *out = g;
    return MI_OK;
}

mi_status mi_group_destroy(mi_group* g)
{
    if (!g) return MI_OK;
    // Every stream of every member drained BEFORE any communicator goes: the chunked gather leaves its broadcasts on the
    // members' second streams, and a communicator must not be torn down under work that still refers to it.
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        (void)hipSetDevice(g->dev[r]);
        (void)hipStreamSynchronize(g->ctx[r]->stream);
        if (r < g->gstream.size() && g->gstream[r]) (void)hipStreamSynchronize(g->gstream[r]);
    }
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        (void)hipSetDevice(g->dev[r]);
        if (r < g->comms.size() && g->comms[r] && g->CommDestroy) (void)g->CommDestroy(g->comms[r]);
    }
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        (void)hipSetDevice(g->dev[r]);
        if (r < g->red_dev.size() && g->red_dev[r]) (void)hipFree(g->red_dev[r]);
        if (g->done[r]) (void)hipEventDestroy(g->done[r]);
        if (r < g->pre.size() && g->pre[r]) (void)hipEventDestroy(g->pre[r]);
        if (r < g->copied.size() && g->copied[r]) (void)hipEventDestroy(g->copied[r]);
        if (r < g->gstream.size() && g->gstream[r]) (void)hipStreamDestroy(g->gstream[r]);
        if (r < g->gdone.size() && g->gdone[r]) (void)hipEventDestroy(g->gdone[r]);
        if (r < g->cdone.size())
            for (hipEvent_t e : g->cdone[r])
                if (e) (void)hipEventDestroy(e);
        mi_ctx_destroy(g->ctx[r]);
    }
    // the RCCL handle stays open for the life of the process (communicator teardown may still use it)
    delete g;
    return MI_OK;
}

int mi_group_size(const mi_group* g) { return g ? (int)g->ctx.size() : 0; }

mi_ctx* mi_group_ctx(mi_group* g, int rank)
{
    if (!g || rank < 0 || rank >= (int)g->ctx.size()) return nullptr;
    return g->ctx[rank];
}

int mi_group_rccl_ranks(mi_group* g)
{
    // the size RCCL itself reports for the group's communicator (ncclCommCount of shard 0's handle), forming the
    // communicator first if no collective has needed it yet; 0 when the group cannot use RCCL (repeated devices,
    // library missing) -- the error text is then in mi_last_error(NULL)
    if (!g || bind_rccl(g) != MI_OK || g->comms.empty() || !g->CommCount) return 0;
    int n = 0;
    if (g->CommCount(g->comms[0], &n) != 0) return 0;
    return n;
}

mi_status mi_group_set_gather_chunks(mi_group* g, int chunks)
{
    MI_REQUIRE(nullptr, g != nullptr, "mi_group_set_gather_chunks: group is NULL");
    MI_REQUIRE(nullptr, chunks >= 1 && chunks <= 64, "mi_group_set_gather_chunks: chunks=%d not in [1,64]", chunks);
    g->gather_chunks = chunks;
    return MI_OK;
}

mi_status mi_group_set_reduce(mi_group* g, int mode)
{
    MI_REQUIRE(nullptr, g != nullptr, "mi_group_set_reduce: group is NULL");
    MI_REQUIRE(nullptr, mode == MI_GROUP_REDUCE_HOST || mode == MI_GROUP_REDUCE_RCCL, "mi_group_set_reduce: unknown mode %d", mode);
    if (mode == MI_GROUP_REDUCE_RCCL) {
        mi_status st = bind_rccl(g);
        if (st != MI_OK) return st;
    }
    g->reduce_mode = mode;
    return MI_OK;
}

mi_status mi_group_synchronize(mi_group* g)
{
    MI_REQUIRE(nullptr, g != nullptr, "mi_group_synchronize: group is NULL");
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        mi_status st = mi_ctx_synchronize(g->ctx[r]);
        if (st != MI_OK) return st;
    }
    return MI_OK;
}

mi_status mi_group_wait_stream(mi_group* g, int rank, void* stream)
{
    MI_REQUIRE(nullptr, g != nullptr, "mi_group_wait_stream: group is NULL");
    MI_REQUIRE(nullptr, rank >= 0 && rank < (int)g->ctx.size(), "mi_group_wait_stream: rank=%d not in [0,%zu)", rank, g->ctx.size());
    // stream-ordered, no host wait: an event on the caller's stream (NULL: the device's default stream), and the member's
    // stream behind it.  The exchange stream of the chunked gather starts behind the member's stream, so it is covered.
    mi_ctx* c = g->ctx[rank];
    MI_HIP(c, hipSetDevice(g->dev[rank]));
    // nothing pending there (the timed loop of bench.py --backend group): nothing to order behind, and the member's queue
    // is spared a barrier per call.  hipStreamQuery does not wait; any answer but "idle" takes the ordered path.
    if (hipStreamQuery((hipStream_t)stream) == hipSuccess) return MI_OK;
    (void)hipGetLastError();   // hipErrorNotReady is an answer, not a failure
    hipEvent_t pre = nullptr;
    const mi_status st = member_event(g, g->pre, (size_t)rank, &pre);
    if (st != MI_OK) return st;
    MI_HIP(c, hipEventRecord(pre, (hipStream_t)stream));
    MI_HIP(c, hipStreamWaitEvent(c->stream, pre, 0));
    return MI_OK;
}

// ---- table interpolation ------------------------------------------------------------------------------------------

mi_status mi_group_grid1_create(mi_group* g, const double* x, const double* y, size_t n, unsigned flags, mi_group_grid1** out)
{
    MI_REQUIRE(nullptr, g && out, "mi_group_grid1_create: NULL argument");
    *out = nullptr;
    MI_REQUIRE(nullptr, (flags & MI_GRID_DEVICE_PTRS) == 0, "mi_group_grid1_create: the table is given in host memory (it is replicated on every device)");
    mi_group_grid1* t = new (std::nothrow) mi_group_grid1();
    if (!t) return mi::fail(nullptr, MI_ERR_NOMEM, "mi_group_grid1_create: out of host memory");
    t->g = g;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        mi_grid1* gr = nullptr;
        const mi_status st = mi_grid1_create(g->ctx[r], x, y, n, flags, &gr);
        if (st != MI_OK) {
            mi_group_grid1_destroy(t);
            return st;
        }
        t->grid.push_back(gr);
    }
    *out = t;
    return MI_OK;
}

mi_status mi_group_grid1_destroy(mi_group_grid1* t)
{
    if (!t) return MI_OK;
    for (mi_grid1* gr : t->grid) mi_grid1_destroy(gr);
    delete t;
    return MI_OK;
}

mi_status mi_group_interp1_f64_dev(mi_group* g, const mi_group_grid1* t, const double* const* xq_dev, double* const* yq_dev,
                                   size_t nq_per_shard, double extrap, double* const* gathered_dev)
{
    MI_REQUIRE(nullptr, g && t && xq_dev && yq_dev, "mi_group_interp1_f64_dev: NULL argument");
    MI_REQUIRE(nullptr, t->g == g && t->grid.size() == g->ctx.size(), "mi_group_interp1_f64_dev: the table belongs to another group");
    const size_t P = g->ctx.size();
    if (gathered_dev && g->distinct) {
        const mi_status st = bind_rccl(g);
        if (st != MI_OK) return st;
    }
    if (gathered_dev && g->gather_chunks > 1 && nq_per_shard >= 2 * (size_t)g->gather_chunks)
        return interp1_chunked_gather(g, t, xq_dev, yq_dev, nq_per_shard, extrap, gathered_dev);
    for (size_t r = 0; r < P; ++r) {
        const mi_status st = mi_interp1_f64_dev_v2(g->ctx[r], t->grid[r], xq_dev[r], yq_dev[r], nq_per_shard, extrap);
        if (st != MI_OK) return st;
        if (gathered_dev && !g->distinct) MI_HIP(g->ctx[r], hipEventRecord(g->done[r], g->ctx[r]->stream));
    }
    if (!gathered_dev || nq_per_shard == 0) return MI_OK;
    // every device receives the P shards, shard s at offset s * nq_per_shard (in place when yq_dev[r] already points
    // there): one all-gather over xGMI, enqueued behind each device's kernel on its own stream -- or, in a rehearsal
    // group (a device named more than once), the same data movement with device-to-device copies
    return gather_shards(g, yq_dev, gathered_dev, nq_per_shard);
}

mi_status mi_group_interp1_f64_host(mi_group* g, const mi_group_grid1* t, const double* xq, double* yq, size_t nq, double extrap)
{
    MI_REQUIRE(nullptr, g && t, "mi_group_interp1_f64_host: NULL argument");
    MI_REQUIRE(nullptr, t->g == g && t->grid.size() == g->ctx.size(), "mi_group_interp1_f64_host: the table belongs to another group");
    if (nq == 0) return MI_OK;
    MI_REQUIRE(nullptr, xq && yq, "mi_group_interp1_f64_host: NULL query/result pointer");
    // every shard: upload, kernel, download on its device's own stream; nothing waits until all are enqueued
    return sharded_host_call(g, "mi_group_interp1_f64_host", nq, true, {{xq, nq * sizeof(double)}, {yq, nq * sizeof(double)}},
        [&](int r, mi_ctx* c, size_t lo, size_t hi, hipError_t& herr) -> mi_status {
            const size_t bytes = (hi - lo) * sizeof(double);
            mi_status st = grow_slots(c, bytes, bytes, 0);
            if (st != MI_OK) return st;
            herr = hipMemcpyAsync(c->scratch[0], xq + lo, bytes, hipMemcpyHostToDevice, c->stream);
            if (herr != hipSuccess) return MI_OK;
            st = mi_interp1_f64_dev_v2(c, t->grid[r], (const double*)c->scratch[0], (double*)c->scratch[1], hi - lo, extrap);
            if (st == MI_OK) herr = hipMemcpyAsync(yq + lo, c->scratch[1], bytes, hipMemcpyDeviceToHost, c->stream);
            return st;
        });
}

// ---- 2-D table interpolation (BASELINE config 3 over several GPUs: scattered query shards, the table replicated) ------

mi_status mi_group_grid2_create(mi_group* g, const double* x, size_t nx, const double* y, size_t ny, const double* z,
                                unsigned flags, mi_group_grid2** out)
{
    MI_REQUIRE(nullptr, g && out, "mi_group_grid2_create: NULL argument");
    *out = nullptr;
    MI_REQUIRE(nullptr, (flags & MI_GRID_DEVICE_PTRS) == 0, "mi_group_grid2_create: the table is given in host memory (it is replicated on every device)");
    mi_group_grid2* t = new (std::nothrow) mi_group_grid2();
    if (!t) return mi::fail(nullptr, MI_ERR_NOMEM, "mi_group_grid2_create: out of host memory");
    t->g = g;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        mi_grid2* gr = nullptr;
        const mi_status st = mi_grid2_create(g->ctx[r], x, nx, y, ny, z, flags, &gr);
        if (st != MI_OK) {
            mi_group_grid2_destroy(t);
            return st;
        }
        t->grid.push_back(gr);
    }
    *out = t;
    return MI_OK;
}

mi_status mi_group_grid2_destroy(mi_group_grid2* t)
{
    if (!t) return MI_OK;
    for (mi_grid2* gr : t->grid) mi_grid2_destroy(gr);
    delete t;
    return MI_OK;
}

// results of every shard to every device: RCCL all-gather (distinct devices) or device-to-device copies (rehearsal group)
static mi_status gather_shards(mi_group* g, double* const* part_dev, double* const* gathered_dev, size_t n_per_shard)
{
    const size_t P = g->ctx.size();
    if (g->distinct) {
        MI_NCCL(g, g->GroupStart());
        for (size_t r = 0; r < P; ++r) {
            const ncclResult_t rc = g->AllGather(part_dev[r], gathered_dev[r], n_per_shard, mi_ncclFloat64, g->comms[r], g->ctx[r]->stream);
            if (rc != 0) {
                (void)g->GroupEnd();
                return mi::fail(nullptr, MI_ERR_HIP, "ncclAllGather failed: %s", g->GetErrorString ? g->GetErrorString(rc) : "?");
            }
        }
        MI_NCCL(g, g->GroupEnd());
        return MI_OK;
    }
    for (size_t r = 0; r < P; ++r) {
        MI_HIP(g->ctx[r], hipSetDevice(g->dev[r]));
        for (size_t s = 0; s < P; ++s) {
            double* dst = gathered_dev[r] + s * n_per_shard;
            if (dst == part_dev[s]) continue;
            MI_HIP(g->ctx[r], hipStreamWaitEvent(g->ctx[r]->stream, g->done[s], 0));
            MI_HIP(g->ctx[r], hipMemcpyAsync(dst, part_dev[s], n_per_shard * sizeof(double), hipMemcpyDeviceToDevice, g->ctx[r]->stream));
        }
        hipEvent_t copied = nullptr;
        const mi_status st = member_event(g, g->copied, r, &copied);
        if (st != MI_OK) return st;
        MI_HIP(g->ctx[r], hipEventRecord(copied, g->ctx[r]->stream));
    }
    // member r's copies read every other member's part_dev[s]: member s's stream ends behind them, so that a later call
    // that writes part_dev[s] again is ordered behind the reads without a synchronisation in between
    for (size_t s = 0; s < P; ++s)
        for (size_t r = 0; r < P; ++r)
            if (r != s) MI_HIP(g->ctx[s], hipStreamWaitEvent(g->ctx[s]->stream, g->copied[r], 0));
    return MI_OK;
}

// The all-gather hidden behind the kernels (north_star: "an RCCL all-gather over xGMI to reassemble the residual vector";
// at 8 GPUs the exchange of a 1e8-query call is 0.65 ms per link against 0.1 ms of kernel): every
// shard is cut into `gather_chunks` contiguous chunks; the kernel of chunk k+1 runs on the member's own stream while chunk k
// travels on the member's exchange stream.  A chunk of every shard has to land at its place INSIDE that shard's slot of the
// gathered vector (shard s at s * nq_per_shard), which ncclAllGather cannot do (it packs the pieces back to back), so a chunk
// is exchanged as P grouped ncclBroadcast calls, root s sending its piece of the chunk (in place where yq_dev already points
// into gathered_dev).  Repeated devices (rehearsal): the same schedule with device-to-device copies.  Results are those of the
// unchunked call bit for bit (tests/test_group_gpu.py); the timing on a real 8-GPU node is unmeasured.
static mi_status interp1_chunked_gather(mi_group* g, const mi_group_grid1* t, const double* const* xq_dev, double* const* yq_dev,
                                        size_t nq_per_shard, double extrap, double* const* gathered_dev)
{
    const size_t P = g->ctx.size();
    const size_t K = (size_t)g->gather_chunks;
    if (g->distinct && !g->Broadcast) return mi::fail(nullptr, MI_ERR_HIP, "mi_group: ncclBroadcast is not exported by the loaded librccl");
    // exchange streams and events, created on first use
    if (g->gstream.size() != P) {
        g->gstream.assign(P, nullptr);
        g->gdone.assign(P, nullptr);
        g->cdone.assign(P, std::vector<hipEvent_t>());
    }
    for (size_t r = 0; r < P; ++r) {
        MI_HIP(g->ctx[r], hipSetDevice(g->dev[r]));
        if (!g->gstream[r]) MI_HIP(g->ctx[r], hipStreamCreateWithFlags(&g->gstream[r], hipStreamNonBlocking));
        if (!g->gdone[r]) MI_HIP(g->ctx[r], hipEventCreateWithFlags(&g->gdone[r], hipEventDisableTiming));
        while (g->cdone[r].size() < K) {
            hipEvent_t e = nullptr;
            MI_HIP(g->ctx[r], hipEventCreateWithFlags(&e, hipEventDisableTiming));
            g->cdone[r].push_back(e);
        }
        // the exchange stream starts behind whatever the member's stream already holds (an earlier call may still read
        // or write the buffers)
        MI_HIP(g->ctx[r], hipEventRecord(g->gdone[r], g->ctx[r]->stream));
        MI_HIP(g->ctx[r], hipStreamWaitEvent(g->gstream[r], g->gdone[r], 0));
    }
    size_t c = (nq_per_shard + K - 1) / K;
    c += c & 1;                                        // even: 16-byte aligned chunk starts for the vector kernels
    for (size_t k = 0; k * c < nq_per_shard; ++k) {
        const size_t off = k * c, len = std::min(c, nq_per_shard - off);
        for (size_t r = 0; r < P; ++r) {
            const mi_status st = mi_interp1_f64_dev_v2(g->ctx[r], t->grid[r], xq_dev[r] + off, yq_dev[r] + off, len, extrap);
            if (st != MI_OK) return st;
            MI_HIP(g->ctx[r], hipEventRecord(g->cdone[r][k], g->ctx[r]->stream));
        }
        if (g->distinct) {
            for (size_t r = 0; r < P; ++r) {
                MI_HIP(g->ctx[r], hipSetDevice(g->dev[r]));
                MI_HIP(g->ctx[r], hipStreamWaitEvent(g->gstream[r], g->cdone[r][k], 0));
            }
            MI_NCCL(g, g->GroupStart());
            for (size_t s = 0; s < P; ++s) {
                for (size_t r = 0; r < P; ++r) {
                    const ncclResult_t rc = g->Broadcast(yq_dev[r] + off, gathered_dev[r] + s * nq_per_shard + off, len, mi_ncclFloat64,
                                                         (int)s, g->comms[r], g->gstream[r]);
                    if (rc != 0) {
                        (void)g->GroupEnd();
                        return mi::fail(nullptr, MI_ERR_HIP, "ncclBroadcast failed: %s", g->GetErrorString ? g->GetErrorString(rc) : "?");
                    }
                }
            }
            MI_NCCL(g, g->GroupEnd());
        } else {
            for (size_t r = 0; r < P; ++r) {
                MI_HIP(g->ctx[r], hipSetDevice(g->dev[r]));
                for (size_t s = 0; s < P; ++s) {
                    double* dst = gathered_dev[r] + s * nq_per_shard + off;
                    if (dst == yq_dev[s] + off) continue;
                    MI_HIP(g->ctx[r], hipStreamWaitEvent(g->gstream[r], g->cdone[s][k], 0));
                    MI_HIP(g->ctx[r], hipMemcpyAsync(dst, yq_dev[s] + off, len * sizeof(double), hipMemcpyDeviceToDevice, g->gstream[r]));
                }
            }
        }
    }
    // the member's own stream ends behind its exchange stream: mi_group_synchronize (and any later call) covers the gather
    for (size_t r = 0; r < P; ++r) {
        MI_HIP(g->ctx[r], hipSetDevice(g->dev[r]));
        MI_HIP(g->ctx[r], hipEventRecord(g->gdone[r], g->gstream[r]));
        MI_HIP(g->ctx[r], hipStreamWaitEvent(g->ctx[r]->stream, g->gdone[r], 0));
    }
    // repeated devices: member r's exchange stream copied out of every other member's yq_dev[s], so member s's stream ends
    // behind those reads too (with RCCL the broadcasts of member s's own communicator rank are what reads its buffer)
    if (!g->distinct)
        for (size_t s = 0; s < P; ++s)
            for (size_t r = 0; r < P; ++r)
                if (r != s) MI_HIP(g->ctx[s], hipStreamWaitEvent(g->ctx[s]->stream, g->gdone[r], 0));
    return MI_OK;
}

mi_status mi_group_interp2_f64_dev(mi_group* g, const mi_group_grid2* t, const double* const* xq_dev, const double* const* yq_dev,
                                   double* const* zq_dev, size_t nq_per_shard, double extrap, double* const* gathered_dev)
{
    MI_REQUIRE(nullptr, g && t && xq_dev && yq_dev && zq_dev, "mi_group_interp2_f64_dev: NULL argument");
    MI_REQUIRE(nullptr, t->g == g && t->grid.size() == g->ctx.size(), "mi_group_interp2_f64_dev: the table belongs to another group");
    const size_t P = g->ctx.size();
    if (gathered_dev && g->distinct) {
        const mi_status st = bind_rccl(g);
        if (st != MI_OK) return st;
    }
    for (size_t r = 0; r < P; ++r) {
        const mi_status st = mi_interp2_f64_dev(g->ctx[r], t->grid[r], xq_dev[r], yq_dev[r], zq_dev[r], nq_per_shard, extrap);
        if (st != MI_OK) return st;
        if (gathered_dev && !g->distinct) MI_HIP(g->ctx[r], hipEventRecord(g->done[r], g->ctx[r]->stream));
    }
    if (!gathered_dev || nq_per_shard == 0) return MI_OK;
    return gather_shards(g, zq_dev, gathered_dev, nq_per_shard);
}

mi_status mi_group_interp2_f64_host(mi_group* g, const mi_group_grid2* t, const double* xq, const double* yq, double* zq, size_t nq,
                                    double extrap)
{
    MI_REQUIRE(nullptr, g && t, "mi_group_interp2_f64_host: NULL argument");
    MI_REQUIRE(nullptr, t->g == g && t->grid.size() == g->ctx.size(), "mi_group_interp2_f64_host: the table belongs to another group");
    if (nq == 0) return MI_OK;
    MI_REQUIRE(nullptr, xq && yq && zq, "mi_group_interp2_f64_host: NULL query/result pointer");
    const size_t all = nq * sizeof(double);
    return sharded_host_call(g, "mi_group_interp2_f64_host", nq, true, {{xq, all}, {yq, all}, {zq, all}},
        [&](int r, mi_ctx* c, size_t lo, size_t hi, hipError_t& herr) -> mi_status {
            const size_t bytes = (hi - lo) * sizeof(double);
            mi_status st = grow_slots(c, bytes, bytes, bytes);
            if (st != MI_OK) return st;
            herr = hipMemcpyAsync(c->scratch[0], xq + lo, bytes, hipMemcpyHostToDevice, c->stream);
            if (herr == hipSuccess) herr = hipMemcpyAsync(c->scratch[1], yq + lo, bytes, hipMemcpyHostToDevice, c->stream);
            if (herr != hipSuccess) return MI_OK;
            st = mi_interp2_f64_dev(c, t->grid[r], (const double*)c->scratch[0], (const double*)c->scratch[1], (double*)c->scratch[2],
                                    hi - lo, extrap);
            if (st == MI_OK) herr = hipMemcpyAsync(zq + lo, c->scratch[2], bytes, hipMemcpyDeviceToHost, c->stream);
            return st;
        });
}

mi_status mi_group_interp2_grid_f64_host(mi_group* g, const mi_group_grid2* t, const double* xi, size_t nxi, const double* yi,
                                         size_t nyi, double* zi, double extrap)
{
    MI_REQUIRE(nullptr, g && t, "mi_group_interp2_grid_f64_host: NULL argument");
    MI_REQUIRE(nullptr, t->g == g && t->grid.size() == g->ctx.size(), "mi_group_interp2_grid_f64_host: the table belongs to another group");
    if (nxi == 0 || nyi == 0) return MI_OK;
    MI_REQUIRE(nullptr, xi && yi && zi, "mi_group_interp2_grid_f64_host: NULL query/result pointer");
    MI_REQUIRE(nullptr, nxi <= SIZE_MAX / sizeof(double) / nyi, "mi_group_interp2_grid_f64_host: nxi=%zu x nyi=%zu too large", nxi, nyi);
    // the columns are sharded: member r's [lo, hi) is one contiguous slice of the column-major zi
    return sharded_host_call(g, "mi_group_interp2_grid_f64_host", nxi, true,
        {{xi, nxi * sizeof(double)}, {yi, nyi * sizeof(double)}, {zi, nxi * nyi * sizeof(double)}},
        [&](int r, mi_ctx* c, size_t lo, size_t hi, hipError_t& herr) -> mi_status {
            const size_t m = hi - lo;
            mi_status st = grow_slots(c, m * sizeof(double), nyi * sizeof(double), m * nyi * sizeof(double));
            if (st != MI_OK) return st;
            herr = hipMemcpyAsync(c->scratch[0], xi + lo, m * sizeof(double), hipMemcpyHostToDevice, c->stream);
            if (herr == hipSuccess) herr = hipMemcpyAsync(c->scratch[1], yi, nyi * sizeof(double), hipMemcpyHostToDevice, c->stream);
            if (herr != hipSuccess) return MI_OK;
            st = mi_interp2_grid_f64_dev(c, t->grid[r], (const double*)c->scratch[0], m, (const double*)c->scratch[1], nyi,
                                         (double*)c->scratch[2], extrap);
            if (st == MI_OK) herr = hipMemcpyAsync(zi + lo * nyi, c->scratch[2], m * nyi * sizeof(double), hipMemcpyDeviceToHost, c->stream);
            return st;
        });
}

// interp1 over the columns of a matrix (mi_cols1.hip), columns sharded: member r takes [lo, hi) = mi_shard_bounds(ncols, r, P).
// X and XI are replicated; each member gets an axis of its own for the duration of the call.  Device copies are compact
// (leading dimensions n and nxi): slot 0 XI, slot 1 the member's columns of Y, slot 2 its columns of YI.
static hipError_t group_copy_cols(double* dst, size_t ld_dst, const double* src, size_t ld_src, size_t rows, size_t ncols,
                                  hipMemcpyKind kind, hipStream_t stream)
{
    if (ld_dst == rows && ld_src == rows) return hipMemcpyAsync(dst, src, rows * ncols * sizeof(double), kind, stream);
    return hipMemcpy2DAsync(dst, ld_dst * sizeof(double), src, ld_src * sizeof(double), rows * sizeof(double), ncols, kind, stream);
}

mi_status mi_group_interp1_cols_f64_host(mi_group* g, const double* x, size_t n, const double* y, size_t ldy, size_t ncols,
                                         const double* xi, size_t nxi, double* yi, size_t ldyi, double extrap)
{
    MI_REQUIRE(nullptr, g && x, "mi_group_interp1_cols_f64_host: NULL argument");
    const int P = (int)g->ctx.size();
    // one axis per member: validates X (MI_ERR_GRID) whatever ncols and nxi are
    std::vector<mi_axis1*> axis(P, nullptr);
    mi_status st = MI_OK;
    for (int r = 0; r < P && st == MI_OK; ++r) {
        if (hipSetDevice(g->dev[r]) != hipSuccess) st = mi::fail(nullptr, MI_ERR_HIP, "mi_group_interp1_cols_f64_host: hipSetDevice(%d) failed", g->dev[r]);
        else st = mi_axis1_create(g->ctx[r], x, n, 0, &axis[r]);   // a failure's text is also the calling thread's last error
    }
    if (st == MI_OK && ncols != 0 && nxi != 0) {
        if (!(y && xi && yi)) st = mi::fail(nullptr, MI_ERR_INVALID_ARG, "mi_group_interp1_cols_f64_host: NULL table/query/result pointer");
        else if (ldy < n) st = mi::fail(nullptr, MI_ERR_INVALID_ARG, "mi_group_interp1_cols_f64_host: ldy=%zu is smaller than the axis (n=%zu)", ldy, n);
        else if (ldyi < nxi) st = mi::fail(nullptr, MI_ERR_INVALID_ARG, "mi_group_interp1_cols_f64_host: ldyi=%zu is smaller than nxi=%zu", ldyi, nxi);
        else if (ldy > SIZE_MAX / sizeof(double) / ncols || ldyi > SIZE_MAX / sizeof(double) / ncols)
            st = mi::fail(nullptr, MI_ERR_INVALID_ARG, "mi_group_interp1_cols_f64_host: ncols=%zu x (ldy=%zu, ldyi=%zu) too large", ncols, ldy, ldyi);
    }
    if (st == MI_OK && ncols != 0 && nxi != 0)
        st = sharded_host_call(g, "mi_group_interp1_cols_f64_host", ncols, true,
            {{xi, nxi * sizeof(double)}, {y, ((ncols - 1) * ldy + n) * sizeof(double)}, {yi, ((ncols - 1) * ldyi + nxi) * sizeof(double)}},
            [&](int r, mi_ctx* c, size_t lo, size_t hi, hipError_t& herr) -> mi_status {
                const size_t m = hi - lo;
                mi_status s = grow_slots(c, nxi * sizeof(double), m * n * sizeof(double), m * nxi * sizeof(double));
                if (s != MI_OK) return s;
                double *dxi = (double*)c->scratch[0], *dy = (double*)c->scratch[1], *dyi = (double*)c->scratch[2];
                herr = hipMemcpyAsync(dxi, xi, nxi * sizeof(double), hipMemcpyHostToDevice, c->stream);
                if (herr == hipSuccess) herr = group_copy_cols(dy, n, y + lo * ldy, ldy, n, m, hipMemcpyHostToDevice, c->stream);
                if (herr != hipSuccess) return MI_OK;
                s = mi_interp1_cols_f64_dev(c, axis[r], dy, n, m, dxi, nxi, dyi, nxi, extrap);
                if (s == MI_OK) herr = group_copy_cols(yi + lo * ldyi, ldyi, dyi, nxi, nxi, m, hipMemcpyDeviceToHost, c->stream);
                return s;
            });
    for (int r = 0; r < P; ++r) mi_axis1_destroy(axis[r]);
    return st;
}

// The two paired-column forms (`who`), columns sharded as above.  each_form: the call is mi_group_interp1_each_f64_host,
// which has an ldxi to check and to name, and hands its shards to mi_interp1_each_f64_dev; pairs passes ldxi = 0.
// Device copies are compact and sub-allocated as in the single-context host forms: slot 0 the member's columns of X then
// of Y, slot 1 XI (one vector, or the member's columns when ldxi > 0), len, col_ok, slot 2 its columns of YI; slot 3
// stays with the device call.
static mi_status group_paired_host(mi_group* g, const char* who, bool each_form, const double* x, size_t ldx, const double* y,
                                   size_t ldy, size_t n, const uint32_t* len, size_t ncols, const double* xi, size_t ldxi,
                                   size_t nxi, double* yi, size_t ldyi, double extrap, uint32_t* col_ok)
{
    MI_REQUIRE(nullptr, g, "%s: NULL group", who);
    if (ncols == 0 || nxi == 0) return MI_OK;
    MI_REQUIRE(nullptr, x && y && xi && yi, "%s: NULL table/query/result pointer", who);
    MI_REQUIRE(nullptr, n >= 2 && n < 0x7ffffff0u, "%s: need 2 <= n < 2^31 - 16 (n=%zu)", who, n);
    MI_REQUIRE(nullptr, ldx >= n, "%s: ldx=%zu is smaller than n=%zu", who, ldx, n);
    MI_REQUIRE(nullptr, ldy >= n, "%s: ldy=%zu is smaller than n=%zu", who, ldy, n);
    MI_REQUIRE(nullptr, ldyi >= nxi, "%s: ldyi=%zu is smaller than nxi=%zu", who, ldyi, nxi);
    const size_t lim = SIZE_MAX / (2 * sizeof(double)) / ncols;
    const bool fits = ldx <= lim && ldy <= lim && ldyi <= lim && ldxi <= lim && nxi <= lim;
    if (each_form) {
        MI_REQUIRE(nullptr, ldxi == 0 || ldxi >= nxi, "%s: ldxi=%zu is smaller than nxi=%zu (0: one xi for every column)", who, ldxi, nxi);
        MI_REQUIRE(nullptr, fits, "%s: ncols=%zu x (ldx=%zu, ldy=%zu, ldxi=%zu, ldyi=%zu) too large", who, ncols, ldx, ldy, ldxi, ldyi);
    } else {
        MI_REQUIRE(nullptr, fits, "%s: ncols=%zu x (ldx=%zu, ldy=%zu, ldyi=%zu) too large", who, ncols, ldx, ldy, ldyi);
    }
    const bool per_col = ldxi > 0;          // XI goes with its columns; otherwise one vector, replicated
    std::vector<uint32_t> ok_own;
    if (!col_ok) ok_own.resize(ncols);
    uint32_t* const hok = col_ok ? col_ok : ok_own.data();
    // the caller's arrays are page-locked above the size at which the single-context host forms start to chunk (2 x 8 M
    // elements): below it registering four ranges costs more than the members' copies gain by overlapping, and the
    // copies take hipMemcpyAsync's path for pageable memory
    const bool big = std::max(n, nxi) > 2 * ((size_t)8 << 20) / ncols;
    std::vector<const uint32_t*> dok_of(g->ctx.size(), nullptr);   // where each member's step put its col_ok
    const mi_status st = sharded_host_call(g, who, ncols, big,
        {{xi, ((ncols - 1) * ldxi + nxi) * sizeof(double)}, {x, ((ncols - 1) * ldx + n) * sizeof(double)},
         {y, ((ncols - 1) * ldy + n) * sizeof(double)}, {yi, ((ncols - 1) * ldyi + nxi) * sizeof(double)}},
        [&](int r, mi_ctx* c, size_t lo, size_t hi, hipError_t& herr) -> mi_status {
            const size_t m = hi - lo, xi_bytes = (per_col ? m * nxi : nxi) * sizeof(double);
            mi_status s = grow_slots(c, 2 * m * n * sizeof(double), xi_bytes + 2 * m * sizeof(uint32_t), m * nxi * sizeof(double));
            if (s != MI_OK) return s;
            double *dx = (double*)c->scratch[0], *dy = dx + m * n, *dxi = (double*)c->scratch[1], *dyi = (double*)c->scratch[2];
            uint32_t *dlen = (uint32_t*)((char*)c->scratch[1] + xi_bytes), *dok = dlen + m;
            dok_of[r] = dok;
            if (per_col) herr = group_copy_cols(dxi, nxi, xi + lo * ldxi, ldxi, nxi, m, hipMemcpyHostToDevice, c->stream);
            else herr = hipMemcpyAsync(dxi, xi, xi_bytes, hipMemcpyHostToDevice, c->stream);
            if (herr == hipSuccess && len) herr = hipMemcpyAsync(dlen, len + lo, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
            if (herr == hipSuccess) herr = group_copy_cols(dx, n, x + lo * ldx, ldx, n, m, hipMemcpyHostToDevice, c->stream);
            if (herr == hipSuccess) herr = group_copy_cols(dy, n, y + lo * ldy, ldy, n, m, hipMemcpyHostToDevice, c->stream);
            if (herr != hipSuccess) return MI_OK;
            if (each_form) s = mi_interp1_each_f64_dev(c, dx, n, dy, n, n, len ? dlen : nullptr, m, dxi, per_col ? nxi : 0, nxi, dyi, nxi, extrap, dok);
            else s = mi_interp1_pairs_f64_dev(c, dx, n, dy, n, n, len ? dlen : nullptr, m, dxi, nxi, dyi, nxi, extrap, dok);
            if (s == MI_OK) herr = group_copy_cols(yi + lo * ldyi, ldyi, dyi, nxi, nxi, m, hipMemcpyDeviceToHost, c->stream);
            return s;
        },
        // the flags last: their host side is not pinned, so this copy waits for the member's stream
        [&](int r, mi_ctx* c, size_t lo, size_t hi, hipError_t& herr) -> mi_status {
            herr = hipMemcpyAsync(hok + lo, dok_of[r], (hi - lo) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
            return MI_OK;
        });
    if (st != MI_OK || col_ok) return st;
    for (size_t c = 0; c < ncols; ++c)
        if (!hok[c])
            return mi::fail(nullptr, MI_ERR_GRID, "%s: column %zu is bad (len outside [2, n], or X not finite and strictly "
                            "increasing; X is not sorted for the caller); its outputs are NaN", who, c);
    return MI_OK;
}

// interp1 over paired columns (mi_pairs1.hip); XI is replicated
mi_status mi_group_interp1_pairs_f64_host(mi_group* g, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                          const uint32_t* len, size_t ncols, const double* xi, size_t nxi, double* yi,
                                          size_t ldyi, double extrap, uint32_t* col_ok)
{
    return group_paired_host(g, "mi_group_interp1_pairs_f64_host", false, x, ldx, y, ldy, n, len, ncols, xi, 0, nxi, yi, ldyi, extrap,
                             col_ok);
}

// interp1 over paired columns with a query vector per column (mi_each1.hip); XI goes with its columns when ldxi > 0 and is
// replicated when ldxi == 0
mi_status mi_group_interp1_each_f64_host(mi_group* g, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                         const uint32_t* len, size_t ncols, const double* xi, size_t ldxi, size_t nxi,
                                         double* yi, size_t ldyi, double extrap, uint32_t* col_ok)
{
    return group_paired_host(g, "mi_group_interp1_each_f64_host", true, x, ldx, y, ldy, n, len, ncols, xi, ldxi, nxi, yi, ldyi, extrap,
                             col_ok);
}

// ---- EventDrivenMap -----------------------------------------------------------------------------------------------

static mi_status edm_shard_params(const mi_group_edm* e, int r, mi_edm_params* p)
{
    *p = e->total;
    p->n_real = (uint32_t)(e->hi[r] - e->lo[r]);
    p->real_offset = e->total.real_offset + (uint32_t)e->lo[r];
    return MI_OK;
}

static mi_status edm_layout(mi_group_edm* e, const mi_edm_params* p)
{
    const int P = (int)e->g->ctx.size();
    MI_REQUIRE(nullptr, p->n_real >= (uint32_t)P, "mi_group_edm: %u realisations cannot be split over %d shards", p->n_real, P);
    e->total = *p;
    e->lo.resize(P);
    e->hi.resize(P);
    for (int r = 0; r < P; ++r) mi_shard_bounds(p->n_real, r, P, &e->lo[r], &e->hi[r]);
    return MI_OK;
}

mi_status mi_group_edm_create(mi_group* g, const mi_edm_params* p, mi_group_edm** out)
{
    MI_REQUIRE(nullptr, g && p && out, "mi_group_edm_create: NULL argument");
    *out = nullptr;
    mi_group_edm* e = new (std::nothrow) mi_group_edm();
    if (!e) return mi::fail(nullptr, MI_ERR_NOMEM, "mi_group_edm_create: out of host memory");
    e->g = g;
    mi_status st = edm_layout(e, p);
    for (size_t r = 0; st == MI_OK && r < g->ctx.size(); ++r) {
        mi_edm_params ps;
        edm_shard_params(e, (int)r, &ps);
        mi_edm* s = nullptr;
        st = mi_edm_create(g->ctx[r], &ps, &s);
        if (st == MI_OK) e->shard.push_back(s);
    }
    if (st != MI_OK) {
        mi_group_edm_destroy(e);
        return st;
    }
    *out = e;
    return MI_OK;
}

mi_status mi_group_edm_destroy(mi_group_edm* e)
{
    if (!e) return MI_OK;
    for (mi_edm* s : e->shard) mi_edm_destroy(s);
    delete e;
    return MI_OK;
}

mi_status mi_group_edm_set_params(mi_group_edm* e, const mi_edm_params* p)
{
    MI_REQUIRE(nullptr, e && p, "mi_group_edm_set_params: NULL argument");
    mi_status st = edm_layout(e, p);
    for (size_t r = 0; st == MI_OK && r < e->shard.size(); ++r) {
        mi_edm_params ps;
        edm_shard_params(e, (int)r, &ps);
        st = mi_edm_set_params(e->shard[r], &ps);
    }
    return st;
}

mi_edm* mi_group_edm_shard(mi_group_edm* e, int rank)
{
    if (!e || rank < 0 || rank >= (int)e->shard.size()) return nullptr;
    return e->shard[rank];
}

mi_status mi_group_edm_shard_bounds(const mi_group_edm* e, int rank, size_t* lo, size_t* hi)
{
    MI_REQUIRE(nullptr, e && rank >= 0 && rank < (int)e->shard.size(), "mi_group_edm_shard_bounds: bad argument");
    if (lo) *lo = e->lo[rank];
    if (hi) *hi = e->hi[rank];
    return MI_OK;
}

mi_status mi_group_edm_compute_f(mi_group_edm* e, const double* z, double* f, double* partial_total)
{
    MI_REQUIRE(nullptr, e && z && f, "mi_group_edm_compute_f: NULL argument");
    mi_group* g = e->g;
    const size_t P = e->shard.size();
    const uint32_t S = e->total.n_spikes;
    const uint32_t L = 2 * S + 1;
    // every shard's whole pipeline is enqueued before any is waited for: the devices run concurrently
    for (size_t r = 0; r < P; ++r) {
        const mi_status st = mi_edm_compute_f_begin(e->shard[r], z);
        if (st != MI_OK) {
            double fr[kMaxSpikesG];
            for (size_t q = 0; q < r; ++q) (void)mi_edm_compute_f_end(e->shard[q], fr, nullptr);   // nothing stays pending
            return st;
        }
    }
    double tot[2 * kMaxSpikesG + 1] = {0};
    std::vector<double> parts(P * L);
    mi_status first = MI_OK;
    for (size_t r = 0; r < P; ++r) {
        double fr[kMaxSpikesG];
        const mi_status st = mi_edm_compute_f_end(e->shard[r], fr, &parts[r * L]);
        if (st != MI_OK && first == MI_OK) first = st;
    }
    if (first != MI_OK) return first;
    if (g->reduce_mode == MI_GROUP_REDUCE_RCCL && P > 1) {
        // the same sum on the devices: all-reduce of 2S+1 doubles over xGMI (what one-process-per-GPU callers do)
        mi_status st = bind_rccl(g);
        if (st != MI_OK) return st;
        if (g->red_dev.size() != P) {
            g->red_dev.assign(P, nullptr);
            for (size_t r = 0; r < P; ++r) {
                MI_HIP(g->ctx[r], hipSetDevice(g->dev[r]));
                MI_HIP(g->ctx[r], hipMalloc(&g->red_dev[r], (2 * kMaxSpikesG + 1) * sizeof(double)));
            }
        }
        for (size_t r = 0; r < P; ++r) {
            MI_HIP(g->ctx[r], hipSetDevice(g->dev[r]));
            MI_HIP(g->ctx[r], hipMemcpyAsync(g->red_dev[r], &parts[r * L], L * sizeof(double), hipMemcpyHostToDevice, g->ctx[r]->stream));
        }
        MI_NCCL(g, g->GroupStart());
        for (size_t r = 0; r < P; ++r) {
            const ncclResult_t rc = g->AllReduce(g->red_dev[r], g->red_dev[r], L, mi_ncclFloat64, mi_ncclSum, g->comms[r], g->ctx[r]->stream);
            if (rc != 0) {
                (void)g->GroupEnd();
                return mi::fail(nullptr, MI_ERR_HIP, "ncclAllReduce failed: %s", g->GetErrorString ? g->GetErrorString(rc) : "?");
            }
        }
        MI_NCCL(g, g->GroupEnd());
        MI_HIP(g->ctx[0], hipSetDevice(g->dev[0]));
        MI_HIP(g->ctx[0], hipMemcpyAsync(tot, g->red_dev[0], L * sizeof(double), hipMemcpyDeviceToHost, g->ctx[0]->stream));
        for (size_t r = 0; r < P; ++r) {
            MI_HIP(g->ctx[r], hipSetDevice(g->dev[r]));
            MI_HIP(g->ctx[r], hipStreamSynchronize(g->ctx[r]->stream));
        }
    } else {
        for (size_t r = 0; r < P; ++r)           // fixed order: the sum is reproducible run to run
            for (uint32_t k = 0; k < L; ++k) tot[k] += parts[r * L + k];
    }
    if (partial_total)
        for (uint32_t k = 0; k < L; ++k) partial_total[k] = tot[k];
    return mi_edm_residual_from_sums(&e->total, z, tot, f);
}

}  // extern "C"
