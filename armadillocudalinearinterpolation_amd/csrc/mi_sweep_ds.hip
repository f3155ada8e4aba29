// Region sweep, pipelined form, with deferred result stores: mi_interp1_f64_dev_v2.
//
// interp1_sweep_ds_kernel is interp1_sweep_pipe_kernel (mi_interp1_sweep.hpp) in every respect but the hand-over of
// results.  There, the group that has just gathered a tile stores its 16 result vectors per lane and loads the 16
// query vectors of its next tile in the gap while the other group scatters: 256 KiB per CU through HBM with no gather
// in flight.  Here it stores only 16 - DEFER vectors in the gap (their registers become load destinations), issues all
// 16 loads (they stay in the gap: every measurement of moved loads lost), and keeps DEFER result vectors in registers
// until the start of its next (prepare) step, where they go out beside the other group's gather rounds
// (profiles/r02_exp_mix_stream_beside_gathers.log: streamed stores cost gathers 3 %).
// Same tiles, same sort, same arithmetic (eval_batch), same store addresses, width and nt policy: the output is
// bit-identical to the pipelined form's.  No wait of one workgroup on another; the only spin is the group counter.
// Timings of every DEFER value and of both placements of the held-back stores, and which of them fit the 128 registers
// of a 1024-lane workgroup without scratch: profiles/r08_sweep_deferred_stores.log.
//
// The sources of the interp1 kernel family are included as they are.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

#include "mi_interp1_sweep.hpp"

using namespace mi_interp1;

namespace {

// result vectors held back per lane and tile, by table mode: what fits the 128 registers without scratch ({x,y} tables
// have less room: their gather rounds keep more alive)
constexpr int ds_defer(int mode) { return mode == 0 ? 8 : 4; }

typedef __attribute__((address_space(3))) volatile unsigned lds_vu32;

template <int MODE, int FORMULA, int DEFER>
__global__ __launch_bounds__(kPipeThreads) void interp1_sweep_ds_kernel(G1Dev g, const double* __restrict__ xq,
                                                                        double* __restrict__ yq, size_t ntiles,
                                                                        double extrap, double bscale,
                                                                        const int* __restrict__ order_flag,
                                                                        size_t tail, ProbeArgs probe)
{
    constexpr int kVec = kSweepK / 2;                      // result vectors per lane and tile
    static_assert(DEFER > 0 && DEFER <= kVec, "DEFER counts result vectors of a lane");
    constexpr int kNow = kVec - DEFER;                     // stored in the gap, as before
    __shared__ double sq[kSweepTile];
    __shared__ unsigned hist[2][kSweepBins];
    __shared__ unsigned gbar[2];
    if (*order_flag != 0) return;            // queries already ordered locally: the streaming kernel does the work
    if (threadIdx.x < 2) gbar[threadIdx.x] = 0;
    const int tid = threadIdx.x & (kPipeGroup - 1);
    const int grp = threadIdx.x >> 9;        // wave-uniform: waves 0-7 / 8-15
    const bool last_wg = blockIdx.x == gridDim.x - 1;
    if (probe.host_mailbox && last_wg && threadIdx.x >= kPipeThreads - 64) order_probe_wave(probe);   // for the next call
    const long nloc = ntiles > blockIdx.x ? (long)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x) : 0;
    double q[kSweepK];                       // preparer: the tile's queries; gatherer: the results that leave in the gap
    double held[2 * DEFER];                  // results held back from the gap to this group's next step
    unsigned sp2[kSweepK / 2];               // sorted positions of this group's tile, two per register
    // `held` carries values from a gather step to the next prepare step only.  Zeros (constants, no register) on every
    // other path, the way out of the loops included, so that the allocator has these registers for the sort.
    auto drop_held = [&]() {
#pragma unroll
        for (int u = 0; u < 2 * DEFER; ++u) held[u] = 0.0;
    };
    drop_held();
    // vector u of this lane in local tile `it` of a stream: a wave-uniform base and one 32-bit lane offset that the
    // query and the result stream share (scalar-base addressing: no 64-bit lane address is kept across the loop)
    const unsigned lane_bytes = (unsigned)tid * (unsigned)sizeof(d2);
    auto vec_at = [&](const double* base, long it, int u) {
        const char* row = reinterpret_cast<const char*>(base + ((size_t)blockIdx.x + (size_t)it * gridDim.x) * kSweepTile) +
                          (size_t)u * kPipeGroup * sizeof(d2);
        return reinterpret_cast<d2*>(const_cast<char*>(row + lane_bytes));
    };
    auto load_tile = [&](long it) {                          // the 16 vectors per lane of this group's next tile
#pragma unroll
        for (int u = 0; u < kVec; ++u) {
            const d2 v = stream_load(vec_at(xq, it, u));
            q[2 * u] = v.x;
            q[2 * u + 1] = v.y;
        }
    };
    auto store_now = [&](long it) {                          // vectors 0 .. kNow-1 of the tile, in the gap
#pragma unroll
        for (int u = 0; u < kNow; ++u) {
            d2 v;
            v.x = q[2 * u];
            v.y = q[2 * u + 1];
            stream_store(v, vec_at(yq, it, u));
        }
    };
    auto store_held = [&](long it) {                         // vectors kNow .. 15 of tile `it`, one step later
        if (it < 0) return;                                  // (nothing gathered yet)
#pragma unroll
        for (int u = 0; u < DEFER; ++u) {
            d2 v;
            v.x = held[2 * u];
            v.y = held[2 * u + 1];
            stream_store(v, vec_at(yq, it, kNow + u));
        }
    };
    for (int b = threadIdx.x; b < 2 * kSweepBins; b += kPipeThreads) (&hist[0][0])[b] = 0;
    if (grp == 0 && nloc > 0) load_tile(0);
    pipe_barrier();
    unsigned* const myhist = hist[grp];
    // barrier among the 8 waves of this group only: a monotonic arrival counter in LDS
    unsigned gb_target = 0;
    auto group_barrier = [&]() {
        gb_target += kPipeGroup / 64;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if ((threadIdx.x & 63) == 0) atomicAdd(&gbar[grp], 1u);
        // polled with an LDS load proper: a flat load counts as vector memory too, and waiting for its result would
        // wait for every result store this wave has in flight
        while (*(lds_vu32*)&gbar[grp] < gb_target) __builtin_amdgcn_s_sleep(2);
        asm volatile("" ::: "memory");
    };
    // The schedule of interp1_sweep_pipe_kernel: in step `it` the owner of tile `it` (group it & 1) gathers it and the
    // owner of tile it+1 prepares it; each group alternates strictly between the two roles.
    auto gather_step = [&](long it) {        // this group owns tile `it` (it = -1: nothing yet, barriers only)
        const bool act = it >= 0;
        const bool rev = (it & 1) != 0;      // regions are swept up, down, up, ...
        const int stride = rev ? -kPipeGroup : kPipeGroup;
        int first = rev ? kSweepTile - 1 - tid : tid;
        if (act) {
#pragma unroll 1
            for (int iv = 0; iv < 4; ++iv) { // eight rounds; the other group prepares its tile meanwhile
                pipe_gather_rounds<MODE, FORMULA>(g, sq, first, stride, extrap);
                first += 8 * stride;
            }
        }
        pipe_barrier();                      // (the preparer is done with its sort)
        if (act) {                           // results out of the tile: into q (stored in the gap) or held (next step)
#pragma unroll
            for (int u = 0; u < kSweepK; u += 2) {
                const double a = sq[sp2[u / 2] & 0xffffu], b = sq[sp2[u / 2] >> 16];
                if (u / 2 < kNow) {
                    q[u] = a;
                    q[u + 1] = b;
                } else {
                    held[u - 2 * kNow] = a;
                    held[u + 1 - 2 * kNow] = b;
                }
                if ((u & 6) == 6) __builtin_amdgcn_sched_barrier(0);   // eight at a time: bounded register pressure
            }
        } else {
#pragma unroll
            for (int u = 0; u < kSweepK; ++u) q[u] = 0.0;   // explicit definition on every path: q is dead during the rounds
#pragma unroll
            for (int u = 0; u < 2 * DEFER; ++u) held[u] = 0.0;
        }
        pipe_barrier();
        if (act) store_now(it);              // nothing waited for; the registers of these vectors take the loads below
        __builtin_amdgcn_sched_barrier(0);   // stores first: their registers are free when the loads want them
        if (it + 2 < nloc) {                 // (it = -1: group 1's first tile)
            load_tile(it + 2);               // all 16 loads stay in the gap, where nobody gathers
        } else {
#pragma unroll
            for (int u = 0; u < kSweepK; ++u) q[u] = 0.0;
        }
        pipe_barrier();
    };
    auto prep_step = [&](long it) {          // this group owns tile it+1 (past the last tile: barriers only)
        const bool act = it + 1 < nloc;
        // The results held back from tile it-1, which this group gathered in the previous step, go out here, beside the
        // first gather rounds of the other group and behind this group's own loads, which are still landing.  (After
        // the sort, in the slack before the barrier, the registers do not last: profiles/r08_sweep_deferred_stores.log.)
        store_held(it - 1);
        drop_held();
        unsigned rank2[kSweepK / 2];         // rank inside the region (histogram ticket), two per register
#pragma unroll
        for (int u = 0; u < kSweepK / 2; ++u) rank2[u] = 0;
        if (act) {
            // region histogram (own histogram, cleared in the previous step)
#pragma unroll
            for (int u = 0; u < kSweepK; u += 2) {
                const unsigned r0 = atomicAdd(&myhist[sweep_bin(q[u], g.xmin, bscale)], 1u);
                const unsigned r1 = atomicAdd(&myhist[sweep_bin(q[u + 1], g.xmin, bscale)], 1u);
                rank2[u / 2] = r0 | (r1 << 16);
                if ((u & 6) == 6) __builtin_amdgcn_sched_barrier(0);
            }
            group_barrier();
            if (tid < 64) {                  // exclusive prefix over the regions (one wave, 64 at a time)
                unsigned run = 0;
#pragma unroll
                for (int base = 0; base < kSweepBins; base += 64) {
                    const unsigned v = myhist[base + tid];
                    unsigned incl = v;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const unsigned o = __shfl_up(incl, off, 64);
                        if (tid >= off) incl += o;
                    }
                    myhist[base + tid] = run + incl - v;
                    run += __shfl(incl, 63, 64);
                }
            }
            group_barrier();
#pragma unroll
            for (int u = 0; u < kSweepK; u += 2) {   // sorted positions
                // the region is recomputed from the query rather than kept (see interp1_sweep_pipe_kernel)
                double qa = q[u], qb = q[u + 1];
                asm volatile("" : "+v"(qa), "+v"(qb));
                const unsigned p0 = myhist[sweep_bin(qa, g.xmin, bscale)] + (rank2[u / 2] & 0xffffu);
                const unsigned p1 = myhist[sweep_bin(qb, g.xmin, bscale)] + (rank2[u / 2] >> 16);
                sp2[u / 2] = p0 | (p1 << 16);
                if ((u & 6) == 6) __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int u = 0; u < kSweepK / 2; ++u) sp2[u] = 0;
        }
        pipe_barrier();                      // the gather rounds of the other group are over
        if (act) {
            for (int b = tid; b < kSweepBins; b += kPipeGroup) myhist[b] = 0;   // every lane read its region bases before the barrier
        }
        pipe_barrier();                      // (the gatherer has taken its results out of the tile)
        if (act) {                           // this group's tile goes in
#pragma unroll
            for (int u = 0; u < kSweepK; u += 2) {
                sq[sp2[u / 2] & 0xffffu] = q[u];
                sq[sp2[u / 2] >> 16] = q[u + 1];
                if ((u & 6) == 6) __builtin_amdgcn_sched_barrier(0);
            }
        }
        pipe_barrier();
    };
    if (grp == 0) {
        for (long it = -1;;) {
            prep_step(it);
            if (++it >= nloc) break;
            gather_step(it);
            if (++it >= nloc) break;
        }
    } else {
        for (long it = -1;;) {
            gather_step(it);
            if (++it >= nloc) break;
            prep_step(it);
            if (++it >= nloc) break;
        }
    }
    // the group that gathered the workgroup's last tile has no prepare step left to store in
    if (nloc > 0 && grp == (int)((nloc - 1) & 1)) store_held(nloc - 1);
    if (tail && last_wg && grp == 0) {       // ragged tail (< one tile), four queries per lane at a time
        const double* tq = xq + ntiles * kSweepTile;
        double* to = yq + ntiles * kSweepTile;
#pragma unroll 1
        for (int u = 0; u < kSweepK; u += 4) {
            double qq[4], rr[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const size_t i = (size_t)tid + (size_t)(u + w) * kPipeGroup;
                qq[w] = i < tail ? tq[i] : 0.0;
            }
            eval_batch<MODE, 4, FORMULA, kSweepWin>(g, qq, rr, extrap);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const size_t i = (size_t)tid + (size_t)(u + w) * kPipeGroup;
                if (i < tail) to[i] = rr[w];
            }
        }
    }
}

// launch_mode's window for the whole-table-in-LDS kernel, which it tries before the sweep (the constants of
// mi_interp1_stream.hpp; that header defines a kernel and belongs to mi_interp1.hip alone)
constexpr size_t kLdsMaxTableBytes = 128 * 1024, kLdsMinTableBytes0 = 32 * 1024, kLdsMinTableBytes3 = 2 * 1024;
constexpr size_t kLdsQueriesPerBlock = 1u << 17;

// environment hooks, each read ONCE per process; the first three mean what they mean to mi_interp1_f64_dev
struct DsEnv {
    long min_bytes;          // MI_SWEEP_MIN_BYTES
    size_t min_tiles_per_cu; // MI_SWEEP_MIN_TILES_PER_CU
    int variant;             // MI_SWEEP_VARIANT
    bool variant_forced;
    int defer;               // MI_SWEEP_DEFER: 0 = every call goes to mi_interp1_f64_dev (A/B switch inside one library)
};
const DsEnv& ds_env()
{
    static const DsEnv e = [] {
        DsEnv v{-1, kSweepMinTilesPerCu, 2, false, 1};
        if (const char* s = getenv("MI_SWEEP_MIN_BYTES")) v.min_bytes = (long)strtoull(s, nullptr, 10);
        if (const char* s = getenv("MI_SWEEP_MIN_TILES_PER_CU")) v.min_tiles_per_cu = (size_t)strtoull(s, nullptr, 10);
        if (const char* s = getenv("MI_SWEEP_VARIANT")) {
            const int x = atoi(s);
            v.variant = (x == 1 || x == 2) ? x : 2;
            v.variant_forced = true;
        }
        if (const char* s = getenv("MI_SWEEP_DEFER")) v.defer = atoi(s);
        return v;
    }();
    return e;
}

// Would launch_mode (mi_interp1.hip) take the pipelined form as its only launch (plan 0)?  Its rules, in its order.
template <int MODE>
bool takes_pipelined_sweep(const mi_ctx* ctx, const G1Dev& d, size_t table_bytes, const double* xq, const double* yq,
                           size_t nq, ProbeArgs& probe)
{
    if (((reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(yq)) & 15u) != 0) return false;
    if (ctx->query_order == MI_QUERIES_ORDERED) return false;
    const bool span_ok = std::isfinite(d.xmax - d.xmin) && (d.xmax - d.xmin) > 0.0;
    if (!span_ok) return false;
    const unsigned cus = (unsigned)(ctx->compute_units > 0 ? ctx->compute_units : 256);
    const size_t ntiles = nq / kSweepTile;
    if (ntiles == 0) return false;
    bool size_ok = table_bytes >= ((size_t)5 << 20);
    if (MODE == 3) size_ok = table_bytes > kLdsMaxTableBytes && !(table_bytes > 2600000 && table_bytes < 3900000);
    if (ds_env().min_bytes >= 0) size_ok = table_bytes >= (size_t)ds_env().min_bytes;
    if constexpr (MODE == 0 || MODE == 3) {  // the whole-table-in-LDS kernel comes first
        const size_t ybytes = ((size_t)d.n + 1) * (MODE == 0 ? sizeof(double) : sizeof(d2));
        if (ybytes > (MODE == 0 ? kLdsMinTableBytes0 : kLdsMinTableBytes3) && ybytes <= kLdsMaxTableBytes && nq >= 8 * kLdsQueriesPerBlock)
            return false;
    }
    if (!size_ok || ntiles < (size_t)cus * ds_env().min_tiles_per_cu) return false;
    if (!(ds_env().variant == 2 && (ds_env().variant_forced || ntiles >= (size_t)cus * 16))) return false;
    probe = ProbeArgs{};
    if (ctx->query_order == MI_QUERIES_AUTO) {
        if (*reinterpret_cast<volatile int*>(ctx->probe_host) != 0) return false;   // predicts ordered, or no verdict yet
        probe = ProbeArgs{xq, nq, d.xmin, (double)kSweepBins / (d.xmax - d.xmin), nullptr, ctx->probe_host_dev};
    }
    return true;
}

std::atomic<size_t> g_ds_launches{0};      // mi_debug_sweep_ds_launches (test hook)

template <int MODE, int FORMULA, int DEFER>
mi_status launch_ds(mi_ctx* ctx, const G1Dev& d, const double* xq, double* yq, size_t nq, double extrap, const ProbeArgs& probe)
{
    const unsigned cus = (unsigned)(ctx->compute_units > 0 ? ctx->compute_units : 256);
    const size_t ntiles = nq / kSweepTile;
    const double bscale = (double)kSweepBins / (d.xmax - d.xmin);
    const int* flags = reinterpret_cast<const int*>(static_cast<const char*>(ctx->reduce_ws) + mi_ctx::kFlagOffset);   // flags[0] is a constant 0
    const unsigned pgrid = (unsigned)std::min<size_t>(ntiles, (size_t)cus);   // one 1024-lane workgroup per CU
    hipLaunchKernelGGL((interp1_sweep_ds_kernel<MODE, FORMULA, DEFER>), dim3(pgrid), dim3(kPipeThreads), 0, ctx->stream, d, xq, yq,
                       ntiles, extrap, bscale, flags, nq - ntiles * kSweepTile, probe);
    MI_LAUNCH_CHECK(ctx, "interp1 pipelined region-sweep kernel (deferred stores)");
    g_ds_launches.fetch_add(1, std::memory_order_relaxed);
    return MI_OK;
}

template <int MODE, int FORMULA = 0>
mi_status dispatch_ds(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq, size_t nq, double extrap)
{
    ProbeArgs probe{};
    const int defer = ds_env().defer;
    if (defer == 0 || !takes_pipelined_sweep<MODE>(ctx, g->d, g->table_bytes, xq, yq, nq, probe))
        return mi_interp1_f64_dev(ctx, g, xq, yq, nq, extrap);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    return launch_ds<MODE, FORMULA, ds_defer(MODE)>(ctx, g->d, xq, yq, nq, extrap, probe);
}

}  // namespace

extern "C" size_t mi_debug_sweep_ds_launches(void) { return g_ds_launches.load(std::memory_order_relaxed); }

extern "C" mi_status mi_interp1_f64_dev_v2(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq, size_t nq, double extrap)
{
    // argument errors, empty calls and pointers that are not even 8-byte aligned: mi_interp1_f64_dev's own answers
    if (!ctx || !g || nq == 0 || !xq || !yq) return mi_interp1_f64_dev(ctx, g, xq, yq, nq, extrap);
    switch (g->mode) {
        case 0:
            if (g->d.formula == 1) return dispatch_ds<0, 1>(ctx, g, xq, yq, nq, extrap);
            if (g->d.formula == 2) return dispatch_ds<0, 2>(ctx, g, xq, yq, nq, extrap);
            if (g->d.formula == 3) return dispatch_ds<0, 3>(ctx, g, xq, yq, nq, extrap);
            return dispatch_ds<0, 0>(ctx, g, xq, yq, nq, extrap);
        case 1:
            if (g->d.centred) return dispatch_ds<3>(ctx, g, xq, yq, nq, extrap);
            return dispatch_ds<1>(ctx, g, xq, yq, nq, extrap);
        default: return dispatch_ds<2>(ctx, g, xq, yq, nq, extrap);
    }
}
