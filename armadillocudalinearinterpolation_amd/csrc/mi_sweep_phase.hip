// Region sweep with the XCD groups out of phase (gfx950): the exported mi_interp1_f64_dev_v2 and
// mi_debug_sweep_ds_launches.  Hand-written HIP; memory-bound, no MFMA.
//
// The files of the interp1 kernel family are pinned by digest (tests/test_interp1_cols_cpu.py), so this unit stands
// beside them the way mi_nearest1.hip does: mi_interp1.hip is compiled with its two exported names renamed to
// mi_interp1_f64_dev_v2_base and mi_debug_sweep_ds_launches_base (_build.PER_SOURCE_FLAGS), and the names themselves are
// defined here.  mi_interp1_sweep.hpp is included as it is, for eval_batch, the prefix, the stream accessors, the
// gather rounds, the ragged tail and the probe.
//
// interp1_phased_sweep_kernel<FORMULA, DEFER> restates interp1_sweep_pipe_kernel<0, FORMULA, DEFER> (pipelined form,
// closed-form tables, part of each tile's result stores held back): same tile, same two groups of 8 waves, same
// barriers, same eval_batch, same store addresses, widths and nt policy -- the output is bit for bit that kernel's.
// One addition.  In the parent all workgroups run in step, so every CU of every XCD streams its 256 KiB per tile at
// the same moment (HBM-limited) and then nobody streams while everybody gathers (limited by each XCD's L2 request
// path).  The in-step sweep is needed only WITHIN an XCD, whose L2 the table regions live in; two XCDs share nothing
// but the fabric and HBM.  Workgroups are dealt round-robin over the 8 XCDs, so workgroups with equal blockIdx % 8
// share an XCD; class c = blockIdx % P (P = 1, 2, 4, 8 divides 8, so this is (blockIdx % 8) % P) starts its first tile
// c/P of a tile period late and the stream bursts of one class meet the gather rounds of the others.  A wrong guess
// about the dealing costs speed only, never a result.
//   The delay is a bounded wait on the constant-rate wall clock before the workgroup's first load: it depends on the
//   clock alone, never on another workgroup, and ends after a fixed number of polls whatever the clock says.
//   Tiles: workgroups are ranked by (class, blockIdx); rank s owns tiles s, s + grid, s + 2 grid, ...  So no workgroup
//   of a later class has more tiles than one of an earlier class, and the ntiles % grid leftover tiles go to the
//   earliest class.  The workgroup of the last rank has the fewest tiles and takes the probe and the ragged tail.
// Measurements and the phase count shipped: DESIGN.md section 4.2, profiles/r10_sweep_xcd_phases.log.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

#include "mi_interp1_sweep.hpp"

using namespace mi_interp1;

namespace {

// Tile period of interp1_sweep_pipe_kernel<0, F, 8> on MI355X: a MEASURED figure (0.65 ms for 23.8 tiles per CU at 1e8
// queries over the 1e6-node table, profiles/r08_sweep_deferred_stores.log), not a derived one.
constexpr unsigned kTilePeriodNs = 27000;
constexpr unsigned kMaxPeriodNs = 1000000;      // what MI_SWEEP_XCD_PHASES may ask for at most
constexpr int kPhaseWaitPolls = 4096;           // upper bound of the clock wait's polls (about 0.2 us each)
constexpr int kPhasesDefault = 4;          // measured: 1, 2, 4, 8 classes 0.651, 0.621, 0.618, 0.623 ms against 0.651 (profiles/r10_sweep_xcd_phases.log)

template <int FORMULA, int DEFER>
__global__ __launch_bounds__(kPipeThreads) void interp1_phased_sweep_kernel(G1Dev g, const double* __restrict__ xq,
                                                                            double* __restrict__ yq, size_t ntiles,
                                                                            double extrap, double bscale,
                                                                            const int* __restrict__ order_flag,
                                                                            size_t tail, ProbeArgs probe,
                                                                            unsigned phase_shift, unsigned class_ticks)
{
    constexpr int kVec = kSweepK / 2;                      // result vectors per lane and tile
    static_assert(DEFER > 0 && DEFER <= kVec, "DEFER counts result vectors of a lane");
    constexpr int kNow = kVec - DEFER;                     // stored in the gap
    constexpr int kHeld = 2 * DEFER;
    __shared__ double sq[kSweepTile];
    __shared__ unsigned hist[2][kSweepBins];
    __shared__ unsigned gbar[2];
    if (*order_flag != 0) return;            // queries already ordered locally: the streaming kernel does the work
    if (threadIdx.x < 2) gbar[threadIdx.x] = 0;
    const int tid = threadIdx.x & (kPipeGroup - 1);
    const int grp = threadIdx.x >> 9;        // wave-uniform: waves 0-7 / 8-15
    // phase class and rank (all scalar): rank = workgroups of earlier classes + earlier workgroups of this class
    const unsigned nwg = gridDim.x;
    const unsigned phases = 1u << phase_shift;   // a power of two: shifts and masks, no integer division
    const unsigned cls = blockIdx.x & (phases - 1);
    unsigned rank = blockIdx.x >> phase_shift;
    for (unsigned k = 0; k < cls; ++k) rank += nwg > k ? (nwg - k + phases - 1) >> phase_shift : 0;
    const bool last_wg = rank == nwg - 1;
    if (probe.host_mailbox && last_wg && threadIdx.x >= kPipeThreads - 64) order_probe_wave(probe);   // for the next call
    const long nloc = ntiles > rank ? (long)((ntiles - rank + nwg - 1) / nwg) : 0;
    if (cls != 0) {
        // the delay of this class: every wave waits on the clock by itself, bounded by the poll count
        const unsigned long long t0 = wall_clock64(), want = (unsigned long long)cls * class_ticks;
        for (int poll = 0; poll < kPhaseWaitPolls && wall_clock64() - t0 < want; ++poll) __builtin_amdgcn_s_sleep(8);
    }
    double q[kSweepK];                       // preparer: the tile's queries; gatherer: the results that leave in the gap
    double held[kHeld];                      // results held back from the gap to this group's next step
    unsigned sp2[kSweepK / 2];               // sorted positions of this group's tile, two per register
    // `held` carries values from a gather step to the next prepare step only.  Zeros (constants, no register) on every
    // other path, the way out of the loops included, so that the allocator has these registers for the sort.
    auto drop_held = [&]() {
#pragma unroll
        for (int u = 0; u < kHeld; ++u) held[u] = 0.0;
    };
    drop_held();
    // vector u of this lane in local tile `it` of a stream: a wave-uniform base and one 32-bit lane offset that the
    // query and the result stream share (scalar-base addressing: no 64-bit lane address is kept across the loop)
    const unsigned lane_bytes = (unsigned)tid * (unsigned)sizeof(d2);
    auto vec_at = [&](const double* base, long it, int u) {
        const char* row = reinterpret_cast<const char*>(base + ((size_t)rank + (size_t)it * nwg) * kSweepTile) +
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
    // One step of the schedule: in step `it` the owner of tile `it` (group it & 1) gathers it and the owner of tile
    // it+1 prepares it; the two roles are separate code paths run in strict alternation by each group.
    auto gather_step = [&](long it) {        // this group owns tile `it` (it = -1: nothing yet, barriers only)
        const bool act = it >= 0;
        // regions are swept up, down, up, ...: lane j of round u handles sorted position j + 512 u (up) or
        // 16383 - j - 512 u (down)
        const bool rev = (it & 1) != 0;
        const int stride = rev ? -kPipeGroup : kPipeGroup;
        int first = rev ? kSweepTile - 1 - tid : tid;
        if (act) {
#pragma unroll 1
            for (int iv = 0; iv < 4; ++iv) { // eight rounds; the other group prepares its tile meanwhile
                pipe_gather_rounds<0, FORMULA>(g, sq, first, stride, extrap);
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
            drop_held();
        }
        pipe_barrier();
        if (act) store_now(it);              // nothing waited for; the registers of these vectors take the loads below
        __builtin_amdgcn_sched_barrier(0);   // stores first: their registers are free when the loads want them
        if (it + 2 < nloc) {                 // (it = -1: group 1's first tile)
            load_tile(it + 2);               // all 16 loads stay in the gap, where nobody of this workgroup gathers
        } else {
#pragma unroll
            for (int u = 0; u < kSweepK; ++u) q[u] = 0.0;
        }
        pipe_barrier();
    };
    auto prep_step = [&](long it) {          // this group owns tile it+1 (past the last tile: barriers only)
        const bool act = it + 1 < nloc;
        // the results held back from tile it-1 go out here, beside the first gather rounds of the other group
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
            if (tid < 64) sweep_prefix_wave(myhist, tid);
            group_barrier();
#pragma unroll
            for (int u = 0; u < kSweepK; u += 2) {   // sorted positions
                // the region is recomputed from the query rather than kept: handed through an empty asm so that the
                // compiler does not keep the 32 fp64 products of the histogram pass alive
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
    if (tail && last_wg && grp == 0) pipe_tail<0, FORMULA>(g, xq + ntiles * kSweepTile, yq + ntiles * kSweepTile, tail, tid, extrap);
}

// MI_SWEEP_XCD_PHASES = P or P:period_ns, read ONCE per process.  P = 0 forwards every call to the family's own kernels,
// 1, 2, 4, 8 is the number of phase classes; anything else is the default.  The family's own tuning hooks mean "run the
// family's own forms" to the tests and scripts that set them: any of them present forwards every call as well.
struct PhaseEnv {
    int phases;
    unsigned period_ns;
    bool family_hooks;
};
const PhaseEnv& phase_env()
{
    static const PhaseEnv e = [] {
        PhaseEnv v{kPhasesDefault, kTilePeriodNs, false};
        if (const char* s = getenv("MI_SWEEP_XCD_PHASES")) {
            char* end = nullptr;
            const long p = strtol(s, &end, 10);
            if (end != s && (p == 0 || p == 1 || p == 2 || p == 4 || p == 8)) v.phases = (int)p;
            if (end != s && *end == ':') {
                const long ns = strtol(end + 1, nullptr, 10);
                if (ns >= 0 && ns <= (long)kMaxPeriodNs) v.period_ns = (unsigned)ns;
            }
        }
        v.family_hooks = getenv("MI_SWEEP_MIN_BYTES") || getenv("MI_SWEEP_MIN_TILES_PER_CU") || getenv("MI_SWEEP_VARIANT") ||
                         getenv("MI_SWEEP_DEFER");
        return v;
    }();
    return e;
}

std::atomic<size_t> g_phased_launches{0};

// ticks of the wall clock between the starts of two consecutive classes (the whole delay stays below one period)
unsigned class_ticks(const mi_ctx* ctx, unsigned period_ns, int phases)
{
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || khz <= 0) khz = 100000;
    return (unsigned)((double)period_ns * (double)khz * 1e-6 / (double)phases);
}

template <int FORMULA>
mi_status launch_phased(mi_ctx* ctx, const G1Dev& d, const double* xq, double* yq, size_t nq, double extrap, int phases,
                        unsigned period_ns, unsigned max_wg, const ProbeArgs& probe)
{
    const size_t ntiles = nq / kSweepTile, head = ntiles * kSweepTile;
    const double bscale = (double)kSweepBins / (d.xmax - d.xmin);
    const int* flags = reinterpret_cast<const int*>(static_cast<const char*>(ctx->reduce_ws) + mi_ctx::kFlagOffset);   // flags[0]: constant 0
    const unsigned cus = (unsigned)(ctx->compute_units > 0 ? ctx->compute_units : 256);
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(ntiles, (size_t)std::min(cus, max_wg)));
    hipLaunchKernelGGL((interp1_phased_sweep_kernel<FORMULA, kSweepDefer(0)>), dim3(grid), dim3(kPipeThreads), 0, ctx->stream, d,
                       xq, yq, ntiles, extrap, bscale, flags, nq - head, probe, (unsigned)(phases == 8 ? 3 : phases == 4 ? 2 : phases == 2 ? 1 : 0),
                       class_ticks(ctx, period_ns, phases));
    MI_LAUNCH_CHECK(ctx, "interp1 phased region-sweep kernel");
    g_phased_launches.fetch_add(1, std::memory_order_relaxed);
    return MI_OK;
}

mi_status launch_phased_formula(mi_ctx* ctx, const G1Dev& d, const double* xq, double* yq, size_t nq, double extrap, int phases,
                                unsigned period_ns, unsigned max_wg, const ProbeArgs& probe)
{
    if (d.formula == 1) return launch_phased<1>(ctx, d, xq, yq, nq, extrap, phases, period_ns, max_wg, probe);
    if (d.formula == 2) return launch_phased<2>(ctx, d, xq, yq, nq, extrap, phases, period_ns, max_wg, probe);
    if (d.formula == 3) return launch_phased<3>(ctx, d, xq, yq, nq, extrap, phases, period_ns, max_wg, probe);
    return launch_phased<0>(ctx, d, xq, yq, nq, extrap, phases, period_ns, max_wg, probe);
}

bool aligned16(const double* xq, const double* yq)
{
    return ((reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(yq)) & 15u) == 0;
}

bool span_ok(const G1Dev& d) { return std::isfinite(d.xmax - d.xmin) && (d.xmax - d.xmin) > 0.0; }

}  // namespace

extern "C" {

size_t mi_debug_sweep_ds_launches(void)
{
    return mi_debug_sweep_ds_launches_base() + g_phased_launches.load(std::memory_order_relaxed);
}

// The phased kernel exactly where the family's dispatcher (launch_mode, mi_interp1.hip) would launch
// interp1_sweep_pipe_kernel<0, F, 8> as the call's only kernel; every other call, argument errors included, is the
// family's, message texts and all.
mi_status mi_interp1_f64_dev_v2(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq, size_t nq, double extrap)
{
    const PhaseEnv& e = phase_env();
    bool take = e.phases != 0 && !e.family_hooks && ctx && g && xq && yq && g->mode == 0 && aligned16(xq, yq) &&
                g->table_bytes >= ((size_t)5 << 20) && span_ok(g->d) && ctx->query_order != MI_QUERIES_ORDERED;
    if (take) {
        const size_t cus = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256);
        take = nq / kSweepTile >= cus * 16;
    }
    ProbeArgs probe{};   // host_mailbox == nullptr: no probe
    if (take && ctx->query_order == MI_QUERIES_AUTO) {
        // the verdict of an earlier call's probe (never waited for): only "unordered" makes the sweep the only launch
        take = *reinterpret_cast<volatile int*>(ctx->probe_host) == 0;
        probe = ProbeArgs{xq, nq, g->d.xmin, (double)kSweepBins / (g->d.xmax - g->d.xmin), nullptr, ctx->probe_host_dev};
    }
    if (!take) return mi_interp1_f64_dev_v2_base(ctx, g, xq, yq, nq, extrap);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    return launch_phased_formula(ctx, g->d, xq, yq, nq, extrap, e.phases, e.period_ns, ~0u, probe);
}

mi_status mi_debug_interp1_phased_sweep(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq, size_t nq, double extrap,
                                        int phases, int max_workgroups)
{
    MI_REQUIRE(ctx, ctx && g, "mi_debug_interp1_phased_sweep: NULL context or grid");
    MI_REQUIRE(ctx, g->mode == 0 && span_ok(g->d), "mi_debug_interp1_phased_sweep: closed-form tables (mode 0) of positive finite span only");
    MI_REQUIRE(ctx, phases == 1 || phases == 2 || phases == 4 || phases == 8, "mi_debug_interp1_phased_sweep: phases=%d is not 1, 2, 4 or 8", phases);
    MI_REQUIRE(ctx, max_workgroups >= 1, "mi_debug_interp1_phased_sweep: max_workgroups=%d", max_workgroups);
    if (nq == 0) return MI_OK;
    MI_REQUIRE(ctx, xq && yq && aligned16(xq, yq), "mi_debug_interp1_phased_sweep: pointers must be non-NULL and 16-byte aligned");
    MI_HIP(ctx, hipSetDevice(ctx->device));
    ProbeArgs probe{};
    if (ctx->query_order == MI_QUERIES_AUTO && nq >= 4098)
        probe = ProbeArgs{xq, nq, g->d.xmin, (double)kSweepBins / (g->d.xmax - g->d.xmin), nullptr, ctx->probe_host_dev};
    return launch_phased_formula(ctx, g->d, xq, yq, nq, extrap, phases, phase_env().period_ns, (unsigned)max_workgroups, probe);
}

}  // extern "C"
