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
// Two forms of the offset; workgroups are ranked by (class, blockIdx) in both, and the workgroup of the last rank has the
// least work and takes the order probe and the ragged tail.
//   By work (shipped for 4 classes): the queries are dealt in units of 4096, a quarter of a tile and one pass of the gather
//   loop; a workgroup of class c starts with a tile of first_units[c] units, goes on with full tiles and ends with one of
//   1..4 units (mi_sweep_partition.hpp: one function for the kernel and the host).  Nobody waits, no period is assumed.
//   Every tile carries its unit count in a scalar register and the loops skip the units it does not have.
//   By the clock (P = 8, MI_SWEEP_XCD_PHASES=P:period_ns, mi_debug_interp1_phased_sweep): a bounded wait on the
//   constant-rate wall clock before the workgroup's first load; it depends on the clock alone, never on another
//   workgroup, and ends after a fixed number of polls whatever the clock says.  Rank s owns tiles s, s + grid, ...
// Measurements, the phase count and the first-tile table shipped: DESIGN.md section 4.2,
// profiles/r10_sweep_xcd_phases.log, profiles/r17_sweep_work_shift.log.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "mi_interp1_sweep.hpp"
#include "mi_sweep_partition.hpp"

using namespace mi_interp1;

namespace {

// Tile period of interp1_sweep_pipe_kernel<0, F, 8> on MI355X: a MEASURED figure (0.65 ms for 23.8 tiles per CU at 1e8
// queries over the 1e6-node table, profiles/r08_sweep_deferred_stores.log), not a derived one.
constexpr unsigned kTilePeriodNs = 27000;
constexpr unsigned kMaxPeriodNs = 1000000;      // what MI_SWEEP_XCD_PHASES may ask for at most
constexpr int kPhaseWaitPolls = 4096;           // upper bound of the clock wait's polls (about 0.2 us each)
constexpr int kPhasesDefault = 4;          // measured: 1, 2, 4, 8 classes 0.651, 0.621, 0.618, 0.623 ms against 0.651 (profiles/r10_sweep_xcd_phases.log)
constexpr size_t kMaxQueries = (size_t)1 << 43;   // the kernel counts 4096-query units in 32 bits (2^31 of them: 64 TiB of queries)
constexpr unsigned kFirstUnits4 = 1234;    // first-tile table shipped for 4 classes, a decimal digit per class (0: the clock form).  Measured against the
                                           // clock form 0.6037-0.6064 against 0.6122-0.6158 ms; {4,1,2,3} 0.6060-0.6102 (profiles/r17_sweep_work_shift.log)
constexpr unsigned kFirstUnits2 = 0;       // ... and for 2 classes: the clock form stays ({4,2} did not beat it)

// The units of a tile, each a group of eight registers per lane: body(j) for the units the tile has, skip(j) for the
// others.  nu is wave-uniform, so the guards are scalar branches at the unit boundaries, which the loops that use this
// already mark with a sched_barrier; a full tile runs the vector instructions it always ran.  (A separate straight
// path for nu == 4 beside the guarded one was compiled too: 12-13 registers per lane go to scratch with it.)
template <int J>
using unit_c = std::integral_constant<int, J>;
template <class Body, class Skip>
__device__ __forceinline__ void for_units(unsigned nu, Body&& body, Skip&& skip)
{
    if (nu > 0) body(unit_c<0>{}); else skip(unit_c<0>{});
    if (nu > 1) body(unit_c<1>{}); else skip(unit_c<1>{});
    if (nu > 2) body(unit_c<2>{}); else skip(unit_c<2>{});
    if (nu > 3) body(unit_c<3>{}); else skip(unit_c<3>{});
}

// first_units == 0: ownership by whole tiles (rank s owns tiles s, s + grid, ...), class c waits c * class_ticks on the
// clock.  Otherwise first_units is the first-tile table (mi_sweep::pack_first_units) and the ownership is
// mi_sweep::sweep_partition's; class_ticks is normally 0 then.
// STAMP: lane 0 of the workgroup stores the wall clock at entry (slot 0) and at exit (slot 1 + tiles), lane 0 of the
// gathering group at the start of the gather step of tile i (slot 1 + i), into stamps[blockIdx * stamp_cap + slot];
// plain stores, nothing waits for them.  Off in every instance the library's own calls launch.
template <int FORMULA, int DEFER, bool STAMP>
__global__ __launch_bounds__(kPipeThreads) void interp1_phased_sweep_kernel(G1Dev g, const double* __restrict__ xq,
                                                                            double* __restrict__ yq, size_t nq,
                                                                            double extrap, double bscale,
                                                                            const int* __restrict__ order_flag,
                                                                            ProbeArgs probe, unsigned phase_shift,
                                                                            unsigned class_ticks, unsigned first_units,
                                                                            unsigned long long* __restrict__ stamps,
                                                                            unsigned stamp_cap)
{
    constexpr int kVec = kSweepK / 2;                      // result vectors per lane and tile
    constexpr int kUnitVec = kVec / (int)mi_sweep::kTileUnits;   // vectors per lane and unit
    static_assert(DEFER > 0 && DEFER <= kVec, "DEFER counts result vectors of a lane");
    static_assert(kSweepTile == (int)(mi_sweep::kTileUnits * mi_sweep::kUnitQueries) && kUnitVec == 4, "a unit is a quarter of a tile");
    constexpr int kNow = kVec - DEFER;                     // stored in the gap
    constexpr int kHeld = 2 * DEFER;
    __shared__ double sq[kSweepTile];
    __shared__ unsigned hist[2][kSweepBins];
    __shared__ unsigned gbar[2];
    if (*order_flag != 0) return;            // queries already ordered locally: the streaming kernel does the work
    auto stamp = [&](unsigned slot) __attribute__((always_inline)) {
        if constexpr (STAMP) {
            if (slot < stamp_cap) stamps[(size_t)blockIdx.x * stamp_cap + slot] = wall_clock64();
        }
    };
    if (threadIdx.x == 0) stamp(0);
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
    // This workgroup's tiles, in units of 4096 queries (the host keeps nq below 2^43, so 32 bits hold them): tile `it`
    // starts at org + (it - 1) step, the first and the last two tiles a correction further (mod 2^32).  The integer
    // division of the partition runs on the vector ALU; its results are uniform and are put back into scalar
    // registers here, where they stay for the whole kernel.
    auto scalar = [](unsigned v) __attribute__((always_inline)) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
    const unsigned step = mi_sweep::kTileUnits * nwg;
    unsigned ntl, org, nus = mi_sweep::kTileUnits | (mi_sweep::kTileUnits << 4), d_first = 0, d_pen = 0, d_last = 0;   // nus: units of the first tile | of the last << 4
    if (first_units == 0) {
        const unsigned ntiles = (unsigned)(nq / kSweepTile);
        ntl = scalar(ntiles > rank ? (ntiles - rank + nwg - 1) / nwg : 0);
        org = mi_sweep::kTileUnits * rank + step;
    } else {
        const mi_sweep::PartitionT<unsigned> part =
            mi_sweep::sweep_partition<unsigned>((unsigned)(nq / mi_sweep::kUnitQueries), nwg, phases, first_units, rank);
        ntl = scalar(part.ntiles);
        nus = scalar(part.first_units | (part.last_units << 4));
        org = scalar(part.mid_origin);
        d_first = scalar(part.first_start - (part.mid_origin - step));
        if (part.ntiles >= 2) d_last = scalar(part.last_start - (part.mid_origin + (part.ntiles - 2) * step));
        if (part.ntiles >= 3) d_pen = scalar(part.pen_start - (part.mid_origin + (part.ntiles - 3) * step));
    }
    const long nloc = (long)ntl;
    // (copies, captured by value: a choice among captured references is a choice among addresses, which puts the
    // variables into memory.  The tile index is uniform but the compiler cannot know: it is put into a scalar register,
    // so that everything chosen by it -- unit counts, hence the guards, and addresses -- stays scalar.)
    const unsigned k_org = org, k_nus = nus, k_first = d_first, k_pen = d_pen, k_last = d_last;
    auto tile_units = [scalar, ntl, k_nus](long it) __attribute__((always_inline)) {         // (of a tile the workgroup has)
        const unsigned i = scalar((unsigned)it);
        return i == 0 ? k_nus & 15u : i == ntl - 1 ? k_nus >> 4 : mi_sweep::kTileUnits;
    };
    auto tile_at = [scalar, ntl, step, k_org, k_first, k_pen, k_last](long it) __attribute__((always_inline)) {
        const unsigned i = scalar((unsigned)it);
        const unsigned fix = i == 0 ? k_first : i == ntl - 1 ? k_last : i == ntl - 2 ? k_pen : 0u;
        return k_org + (i - 1u) * step + fix;
    };
    if (cls != 0 && class_ticks != 0) {
        // the delay of this class: every wave waits on the clock by itself, bounded by the poll count
        const unsigned long long t0 = wall_clock64(), want = (unsigned long long)cls * class_ticks;
        for (int poll = 0; poll < kPhaseWaitPolls && wall_clock64() - t0 < want; ++poll) __builtin_amdgcn_s_sleep(8);
    }
    double q[kSweepK];                       // preparer: the tile's queries; gatherer: the results that leave in the gap
    double held[kHeld];                      // results held back from the gap to this group's next step
    unsigned sp2[kSweepK / 2];               // sorted positions of this group's tile, two per register
    // `held` carries values from a gather step to the next prepare step only.  Zeros (constants, no register) on every
    // other path, the way out of the loops included, so that the allocator has these registers for the sort.
    auto drop_held = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < kHeld; ++u) held[u] = 0.0;
    };
    drop_held();
    // vector u of this lane in local tile `it` of a stream: a wave-uniform base and one 32-bit lane offset that the
    // query and the result stream share (scalar-base addressing: no 64-bit lane address is kept across the loop)
    const unsigned lane_bytes = (unsigned)tid * (unsigned)sizeof(d2);
    auto vec_at = [&](const double* base, long it, int u) __attribute__((always_inline)) {
        // (the tile's base is handed through an empty asm in a scalar register pair: otherwise base + lane offset is
        // formed once in front of the loops, as a 64-bit lane address that lives through the whole kernel)
        const char* row = reinterpret_cast<const char*>(base + (size_t)tile_at(it) * mi_sweep::kUnitQueries);
        asm("" : "+s"(row));
        return reinterpret_cast<d2*>(const_cast<char*>(row + (size_t)u * kPipeGroup * sizeof(d2) + lane_bytes));
    };
    auto load_tile = [&](long it) __attribute__((always_inline)) {                          // the 16 vectors per lane of this group's next tile (4 per unit)
        for_units(tile_units(it),
                  [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                      for (int u = kUnitVec * J; u < kUnitVec * (J + 1); ++u) {
                          const d2 v = stream_load(vec_at(xq, it, u));
                          q[2 * u] = v.x;
                          q[2 * u + 1] = v.y;
                      }
                  },
                  [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                      for (int u = 2 * kUnitVec * J; u < 2 * kUnitVec * (J + 1); ++u) q[u] = 0.0;
                  });
    };
    auto store_now = [&](long it) __attribute__((always_inline)) {                          // vectors 0 .. kNow-1 of the tile, in the gap
        for_units(tile_units(it),
                  [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                      for (int u = kUnitVec * J; u < kUnitVec * (J + 1); ++u) {
                          if (u < kNow) {
                              d2 v;
                              v.x = q[2 * u];
                              v.y = q[2 * u + 1];
                              stream_store(v, vec_at(yq, it, u));
                          }
                      }
                  },
                  [&](auto) __attribute__((always_inline)) {});
    };
    auto store_held = [&](long it) __attribute__((always_inline)) {                         // vectors kNow .. 15 of tile `it`, one step later
        if (it < 0) return;                                  // (nothing gathered yet)
        for_units(tile_units(it),
                  [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                      for (int u = kUnitVec * J; u < kUnitVec * (J + 1); ++u) {
                          if (u >= kNow) {
                              d2 v;
                              v.x = held[2 * (u - kNow)];
                              v.y = held[2 * (u - kNow) + 1];
                              stream_store(v, vec_at(yq, it, u));
                          }
                      }
                  },
                  [&](auto) __attribute__((always_inline)) {});
    };
    for (int b = threadIdx.x; b < 2 * kSweepBins; b += kPipeThreads) (&hist[0][0])[b] = 0;
    if (grp == 0 && nloc > 0) load_tile(0);
    pipe_barrier();
    // The order probe for the next call: the last wave of the last-ranked workgroup, here, where its group has nothing to
    // gather yet and only waits for the other group's first sort.  In front of the first barrier the probe's two rounds
    // of scattered loads held the whole workgroup back by a few microseconds; a workgroup that far behind the others of
    // its XCD stays behind, misses the table regions they share in L2 and ends the kernel late (measured without a clock
    // wait to hide it: 0.637 against 0.592 ms, profiles/r17_sweep_work_shift.log).
    if (probe.host_mailbox && last_wg && threadIdx.x >= kPipeThreads - 64) order_probe_wave(probe);
    unsigned* const myhist = hist[grp];
    // barrier among the 8 waves of this group only: a monotonic arrival counter in LDS
    unsigned gb_target = 0;
    auto group_barrier = [&]() __attribute__((always_inline)) {
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
    auto gather_step = [&](long it) __attribute__((always_inline)) {        // this group owns tile `it` (it = -1: nothing yet, barriers only)
        const bool act = it >= 0;
        const unsigned nu = act ? tile_units(it) : 0;
        // regions are swept up, down, up, ...: lane j of round u handles sorted position j + 512 u (up) or
        // 4096 nu - 1 - j - 512 u (down); a tile of nu units holds sorted positions 0 .. 4096 nu - 1
        const bool rev = (it & 1) != 0;
        const int stride = rev ? -kPipeGroup : kPipeGroup;
        int first = rev ? (int)(nu * mi_sweep::kUnitQueries) - 1 - tid : tid;
        if (act) {
            if (tid == 0) stamp(1u + (unsigned)it);
#pragma unroll 1
            for (int iv = 0; iv < (int)nu; ++iv) { // two rounds per unit; the other group prepares its tile meanwhile
                pipe_gather_rounds<0, FORMULA>(g, sq, first, stride, extrap);
                first += 8 * stride;
            }
        }
        pipe_barrier();                      // (the preparer is done with its sort)
        if (act) {                           // results out of the tile: into q (stored in the gap) or held (next step)
            for_units(nu,
                      [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                          for (int u = 8 * J; u < 8 * (J + 1); u += 2) {
                              const double a = sq[sp2[u / 2] & 0xffffu], b = sq[sp2[u / 2] >> 16];
                              if (u / 2 < kNow) {
                                  q[u] = a;
                                  q[u + 1] = b;
                              } else {
                                  held[u - 2 * kNow] = a;
                                  held[u + 1 - 2 * kNow] = b;
                              }
                          }
                          __builtin_amdgcn_sched_barrier(0);   // eight at a time: bounded register pressure
                      },
                      [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                          for (int u = 8 * J; u < 8 * (J + 1); ++u) {
                              if (u / 2 < kNow) q[u] = 0.0;
                              else held[u - 2 * kNow] = 0.0;
                          }
                      });
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
    auto prep_step = [&](long it) __attribute__((always_inline)) {          // this group owns tile it+1 (past the last tile: barriers only)
        const bool act = it + 1 < nloc;
        const unsigned nu = act ? tile_units(it + 1) : 0;
        // the results held back from tile it-1 go out here, beside the first gather rounds of the other group
        store_held(it - 1);
        drop_held();
        unsigned rank2[kSweepK / 2];         // rank inside the region (histogram ticket), two per register
#pragma unroll
        for (int u = 0; u < kSweepK / 2; ++u) rank2[u] = 0;
        if (act) {
            // region histogram (own histogram, cleared in the previous step)
            for_units(nu,
                      [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                          for (int u = 8 * J; u < 8 * (J + 1); u += 2) {
                              const unsigned r0 = atomicAdd(&myhist[sweep_bin(q[u], g.xmin, bscale)], 1u);
                              const unsigned r1 = atomicAdd(&myhist[sweep_bin(q[u + 1], g.xmin, bscale)], 1u);
                              rank2[u / 2] = r0 | (r1 << 16);
                          }
                          __builtin_amdgcn_sched_barrier(0);
                      },
                      [&](auto) __attribute__((always_inline)) {});
            group_barrier();
            if (tid < 64) sweep_prefix_wave(myhist, tid);
            group_barrier();
            for_units(nu,
                      [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                          for (int u = 8 * J; u < 8 * (J + 1); u += 2) {   // sorted positions
                              // the region is recomputed from the query rather than kept: handed through an empty asm so
                              // that the compiler does not keep the 32 fp64 products of the histogram pass alive
                              double qa = q[u], qb = q[u + 1];
                              asm volatile("" : "+v"(qa), "+v"(qb));
                              const unsigned p0 = myhist[sweep_bin(qa, g.xmin, bscale)] + (rank2[u / 2] & 0xffffu);
                              const unsigned p1 = myhist[sweep_bin(qb, g.xmin, bscale)] + (rank2[u / 2] >> 16);
                              sp2[u / 2] = p0 | (p1 << 16);
                          }
                          __builtin_amdgcn_sched_barrier(0);
                      },
                      [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                          for (int u = 4 * J; u < 4 * (J + 1); ++u) sp2[u] = 0;
                      });
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
            for_units(nu,
                      [&](auto j) __attribute__((always_inline)) {
                      constexpr int J = decltype(j)::value;
#pragma unroll
                          for (int u = 8 * J; u < 8 * (J + 1); u += 2) {
                              sq[sp2[u / 2] & 0xffffu] = q[u];
                              sq[sp2[u / 2] >> 16] = q[u + 1];
                          }
                          __builtin_amdgcn_sched_barrier(0);
                      },
                      [&](auto) __attribute__((always_inline)) {});
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
    const size_t tail = nq & (size_t)((first_units ? mi_sweep::kUnitQueries : (unsigned)kSweepTile) - 1u), whole = nq - tail;
    if (tail && last_wg && grp == 0) pipe_tail<0, FORMULA>(g, xq + whole, yq + whole, tail, tid, extrap);
    if (threadIdx.x == 0) stamp(1u + (unsigned)nloc);
}

// How the classes are set apart: by a wait on the clock (first_units == 0, whole tiles) or by work (first_units: the
// first-tile table as mi_sweep::pack_first_units returns it; period_ns is normally 0 then).
struct PhaseForm {
    int phases;
    unsigned period_ns;
    unsigned first_units;
};

// The first-tile table shipped for P classes, a decimal digit per class; 0: the clock form.  Measured:
// profiles/r17_sweep_work_shift.log, DESIGN.md section 4.2.
constexpr unsigned first_units_default(int phases) { return phases == 4 ? kFirstUnits4 : phases == 2 ? kFirstUnits2 : 0; }

// MI_SWEEP_XCD_PHASES = P[:period_ns[:units]], read ONCE per process.  P = 0 forwards every call to the family's own
// kernels, 1, 2, 4, 8 is the number of phase classes; anything else is the default.  units: the first-tile table of the
// shift by work, a digit 1..4 per class (4:0:4123); it needs P = 1, 2 or 4 -- an eighth of a tile is no whole gather
// pass -- and is ignored otherwise.  No units field: period_ns > 0 asks for the clock form with that period, otherwise
// the shipped form of P runs.  The family's own tuning hooks mean "run the family's own forms" to the tests and scripts
// that set them: any of them present forwards every call as well.
struct PhaseEnv {
    PhaseForm form;
    bool family_hooks;
};
PhaseForm clock_form(int phases, unsigned period_ns) { return PhaseForm{phases, period_ns, 0}; }
PhaseForm shipped_form(int phases)
{
    const unsigned packed = phases < 8 ? mi_sweep::pack_first_units(first_units_default(phases), (unsigned)phases) : 0;
    return packed ? PhaseForm{phases, 0, packed} : clock_form(phases, kTilePeriodNs);
}
const PhaseEnv& phase_env()
{
    static const PhaseEnv e = [] {
        PhaseEnv v{shipped_form(kPhasesDefault), false};
        if (const char* s = getenv("MI_SWEEP_XCD_PHASES")) {
            char* end = nullptr;
            const long p = strtol(s, &end, 10);
            int phases = kPhasesDefault;
            if (end != s && (p == 0 || p == 1 || p == 2 || p == 4 || p == 8)) phases = (int)p;
            v.form = shipped_form(phases);
            if (end != s && *end == ':') {
                char* end2 = nullptr;
                const long ns = strtol(end + 1, &end2, 10);
                const bool ns_ok = end2 != end + 1 && ns >= 0 && ns <= (long)kMaxPeriodNs;
                unsigned packed = 0;
                if (*end2 == ':' && phases >= 1 && phases < 8) {
                    const long units = strtol(end2 + 1, nullptr, 10);
                    if (units > 0 && units <= 44444444) packed = mi_sweep::pack_first_units((unsigned)units, (unsigned)phases);
                }
                if (packed) v.form = PhaseForm{phases, ns_ok ? (unsigned)ns : 0u, packed};
                else if (ns_ok && (ns > 0 || v.form.first_units == 0)) v.form = clock_form(phases, (unsigned)ns);
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
    if (period_ns == 0) return 0;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || khz <= 0) khz = 100000;
    return (unsigned)((double)period_ns * (double)khz * 1e-6 / (double)phases);
}

struct StampArgs {
    unsigned long long* buf;   // nullptr: the product instance, no stamps
    unsigned cap;              // slots per workgroup
};

template <int FORMULA>
mi_status launch_phased(mi_ctx* ctx, const G1Dev& d, const double* xq, double* yq, size_t nq, double extrap, const PhaseForm& f,
                        unsigned max_wg, const ProbeArgs& probe, const StampArgs& st)
{
    // workgroups: one per CU, and no more than there are tiles (clock form) or units (work form)
    const size_t pieces = f.first_units ? nq / mi_sweep::kUnitQueries : nq / kSweepTile;
    const double bscale = (double)kSweepBins / (d.xmax - d.xmin);
    const int* flags = reinterpret_cast<const int*>(static_cast<const char*>(ctx->reduce_ws) + mi_ctx::kFlagOffset);   // flags[0]: constant 0
    const unsigned cus = (unsigned)(ctx->compute_units > 0 ? ctx->compute_units : 256);
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(pieces, (size_t)std::min(cus, max_wg)));
    const unsigned shift = (unsigned)(f.phases == 8 ? 3 : f.phases == 4 ? 2 : f.phases == 2 ? 1 : 0);
    const unsigned ticks = class_ticks(ctx, f.period_ns, f.phases);
    if (st.buf)
        hipLaunchKernelGGL((interp1_phased_sweep_kernel<FORMULA, kSweepDefer(0), true>), dim3(grid), dim3(kPipeThreads), 0, ctx->stream, d,
                           xq, yq, nq, extrap, bscale, flags, probe, shift, ticks, f.first_units, st.buf, st.cap);
    else
        hipLaunchKernelGGL((interp1_phased_sweep_kernel<FORMULA, kSweepDefer(0), false>), dim3(grid), dim3(kPipeThreads), 0, ctx->stream, d,
                           xq, yq, nq, extrap, bscale, flags, probe, shift, ticks, f.first_units, (unsigned long long*)nullptr, 0u);
    MI_LAUNCH_CHECK(ctx, "interp1 phased region-sweep kernel");
    g_phased_launches.fetch_add(1, std::memory_order_relaxed);
    return MI_OK;
}

mi_status launch_phased_formula(mi_ctx* ctx, const G1Dev& d, const double* xq, double* yq, size_t nq, double extrap, const PhaseForm& f,
                                unsigned max_wg, const ProbeArgs& probe, const StampArgs& st = StampArgs{nullptr, 0})
{
    if (d.formula == 1) return launch_phased<1>(ctx, d, xq, yq, nq, extrap, f, max_wg, probe, st);
    if (d.formula == 2) return launch_phased<2>(ctx, d, xq, yq, nq, extrap, f, max_wg, probe, st);
    if (d.formula == 3) return launch_phased<3>(ctx, d, xq, yq, nq, extrap, f, max_wg, probe, st);
    return launch_phased<0>(ctx, d, xq, yq, nq, extrap, f, max_wg, probe, st);
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
    bool take = e.form.phases != 0 && !e.family_hooks && ctx && g && xq && yq && g->mode == 0 && aligned16(xq, yq) &&
                g->table_bytes >= ((size_t)5 << 20) && span_ok(g->d) && ctx->query_order != MI_QUERIES_ORDERED;
    if (take) {
        const size_t cus = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256);
        take = nq / kSweepTile >= cus * 16 && nq <= kMaxQueries;
    }
    ProbeArgs probe{};   // host_mailbox == nullptr: no probe
    if (take && ctx->query_order == MI_QUERIES_AUTO) {
        // the verdict of an earlier call's probe (never waited for): only "unordered" makes the sweep the only launch
        take = *reinterpret_cast<volatile int*>(ctx->probe_host) == 0;
        probe = ProbeArgs{xq, nq, g->d.xmin, (double)kSweepBins / (g->d.xmax - g->d.xmin), nullptr, ctx->probe_host_dev};
    }
    if (!take) return mi_interp1_f64_dev_v2_base(ctx, g, xq, yq, nq, extrap);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    return launch_phased_formula(ctx, g->d, xq, yq, nq, extrap, e.form, ~0u, probe);
}

// the clock form, with the period of the environment if it names one
mi_status mi_debug_interp1_phased_sweep(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq, size_t nq, double extrap,
                                        int phases, int max_workgroups)
{
    MI_REQUIRE(ctx, ctx && g, "mi_debug_interp1_phased_sweep: NULL context or grid");
    MI_REQUIRE(ctx, g->mode == 0 && span_ok(g->d), "mi_debug_interp1_phased_sweep: closed-form tables (mode 0) of positive finite span only");
    MI_REQUIRE(ctx, phases == 1 || phases == 2 || phases == 4 || phases == 8, "mi_debug_interp1_phased_sweep: phases=%d is not 1, 2, 4 or 8", phases);
    MI_REQUIRE(ctx, max_workgroups >= 1, "mi_debug_interp1_phased_sweep: max_workgroups=%d", max_workgroups);
    if (nq == 0) return MI_OK;
    MI_REQUIRE(ctx, nq <= kMaxQueries, "mi_debug_interp1_phased_sweep: nq=%zu is more than the kernel counts in 32 bits", nq);
    MI_REQUIRE(ctx, xq && yq && aligned16(xq, yq), "mi_debug_interp1_phased_sweep: pointers must be non-NULL and 16-byte aligned");
    MI_HIP(ctx, hipSetDevice(ctx->device));
    ProbeArgs probe{};
    if (ctx->query_order == MI_QUERIES_AUTO && nq >= 4098)
        probe = ProbeArgs{xq, nq, g->d.xmin, (double)kSweepBins / (g->d.xmax - g->d.xmin), nullptr, ctx->probe_host_dev};
    const PhaseForm& env = phase_env().form;
    return launch_phased_formula(ctx, g->d, xq, yq, nq, extrap, clock_form(phases, env.first_units ? kTilePeriodNs : env.period_ns),
                                 (unsigned)max_workgroups, probe);
}

// first_units: the first-tile table, a decimal digit 1..4 per class (4123), for the shift by work (phases 1, 2, 4; no
// clock wait); 0: the clock form, as above.  stamps: NULL, or room for max_workgroups * stamp_cap clock values on the
// device (the stamping instance of the kernel runs then; slots nobody writes keep what they held).
mi_status mi_debug_interp1_phased_sweep_ex(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq, size_t nq, double extrap,
                                           int phases, int max_workgroups, unsigned first_units, unsigned long long* stamps,
                                           unsigned stamp_cap)
{
    MI_REQUIRE(ctx, ctx && g, "mi_debug_interp1_phased_sweep_ex: NULL context or grid");
    MI_REQUIRE(ctx, g->mode == 0 && span_ok(g->d), "mi_debug_interp1_phased_sweep_ex: closed-form tables (mode 0) of positive finite span only");
    MI_REQUIRE(ctx, phases == 1 || phases == 2 || phases == 4 || phases == 8, "mi_debug_interp1_phased_sweep_ex: phases=%d is not 1, 2, 4 or 8", phases);
    MI_REQUIRE(ctx, max_workgroups >= 1, "mi_debug_interp1_phased_sweep_ex: max_workgroups=%d", max_workgroups);
    const unsigned packed = first_units && phases < 8 ? mi_sweep::pack_first_units(first_units, (unsigned)phases) : 0;
    MI_REQUIRE(ctx, first_units == 0 || packed != 0, "mi_debug_interp1_phased_sweep_ex: first_units=%u is not %d digits in 1..4 (and phases 1, 2 or 4)",
               first_units, phases);
    MI_REQUIRE(ctx, stamps == nullptr || stamp_cap >= 2, "mi_debug_interp1_phased_sweep_ex: stamp_cap=%u with a stamp buffer", stamp_cap);
    if (nq == 0) return MI_OK;
    MI_REQUIRE(ctx, nq <= kMaxQueries, "mi_debug_interp1_phased_sweep_ex: nq=%zu is more than the kernel counts in 32 bits", nq);
    MI_REQUIRE(ctx, xq && yq && aligned16(xq, yq), "mi_debug_interp1_phased_sweep_ex: pointers must be non-NULL and 16-byte aligned");
    MI_HIP(ctx, hipSetDevice(ctx->device));
    ProbeArgs probe{};
    if (ctx->query_order == MI_QUERIES_AUTO && nq >= 4098)
        probe = ProbeArgs{xq, nq, g->d.xmin, (double)kSweepBins / (g->d.xmax - g->d.xmin), nullptr, ctx->probe_host_dev};
    const PhaseForm& env = phase_env().form;
    const PhaseForm f = packed ? PhaseForm{phases, 0, packed} : clock_form(phases, env.first_units ? kTilePeriodNs : env.period_ns);
    return launch_phased_formula(ctx, g->d, xq, yq, nq, extrap, f, (unsigned)max_workgroups, probe, StampArgs{stamps, stamp_cap});
}

// The ownership of the shift by work for one workgroup (csrc/mi_sweep_partition.hpp; no device is touched).  Starts in
// units of 4096 queries.  Returns 0, or 1 if phases is not 1, 2 or 4, first_units not its table, or rank >= nwg.
mi_status mi_debug_sweep_partition(size_t nq, unsigned nwg, int phases, unsigned first_units, unsigned rank, unsigned* ntiles,
                             unsigned* first_tile_units, unsigned* last_tile_units, size_t* work, size_t* first_start,
                             size_t* mid_origin, size_t* mid_step, size_t* pen_start, size_t* last_start)
{
    if (!(phases == 1 || phases == 2 || phases == 4) || nwg == 0 || rank >= nwg) return MI_ERR_INVALID_ARG;
    const unsigned packed = mi_sweep::pack_first_units(first_units, (unsigned)phases);
    if (!packed) return MI_ERR_INVALID_ARG;
    const mi_sweep::Partition p = mi_sweep::sweep_partition<size_t>(nq / mi_sweep::kUnitQueries, nwg, (unsigned)phases, packed, rank);
    if (ntiles) *ntiles = p.ntiles;
    if (first_tile_units) *first_tile_units = p.first_units;
    if (last_tile_units) *last_tile_units = p.last_units;
    if (work) *work = p.work;
    if (first_start) *first_start = p.first_start;
    if (mid_origin) *mid_origin = p.mid_origin;
    if (mid_step) *mid_step = p.mid_step;
    if (pen_start) *pen_start = p.pen_start;
    if (last_start) *last_start = p.last_start;
    return MI_OK;
}

}  // extern "C"
