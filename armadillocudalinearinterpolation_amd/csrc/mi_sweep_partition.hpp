// Which queries a workgroup of the phased region sweep owns when the phase classes are shifted by WORK: one pure
// function, the same on the host (mi_debug_sweep_partition, tests/test_sweep_work_cpu.py) and in the kernel
// (interp1_phased_sweep_kernel, mi_sweep_phase.hip), scalar integer arithmetic only, nothing uploaded.
//
// Everything is counted in units of 4096 queries, a quarter of a tile: one pass of the kernel's gather loop.  The
// U = nq / 4096 whole units are dealt to the nwg workgroups by rank (rank = workgroups of earlier classes + earlier
// workgroups of the same class, class = blockIdx % P): rank s gets w_s = U / nwg units and one more if s < U % nwg.  A
// workgroup of class c cuts its share into a first tile of min(first_units[c], w_s) units, full tiles of 4 units and a
// last tile of 1..4 units, so the classes reach their stream bursts first_units apart without anybody waiting.
//
// Where the tiles lie (in units, from the start of the arrays):
//   [ first tiles of all ranks, in rank order ]
//   [ row 1 ] ... [ row R ]   R = the number of full tiles behind the first that EVERY rank has; a row holds one full
//                             tile of every rank, in rank order: tile i of rank s starts at origin + (i - 1) step, with
//                             origin = (end of the first tiles) + 4 s and step = 4 nwg -- the access pattern of the
//                             ownership by whole tiles (rank s owns tiles s, s + nwg, ...)
//   [ row R+1 ]               what is left to a rank is l_s = w_s - first - 4 R units, 0..7 of them (the shares differ
//                             by at most 1 and the first tiles by at most 3): min(l_s, 4) units here, in rank order ...
//   [ row R+2 ]               ... and the l_s - 4 units beyond a full tile here, in rank order
//   [ tail ]                  nq % 4096 queries: the last rank's, outside this function
// So a workgroup's tiles are: the first, a regular run, and at most two tiles off the regular grid at its end.  The
// function returns the start of the tile before the last explicitly for that reason; tile i of a workgroup with n tiles
// starts at  i == 0 ? first_start : i == n-1 ? last_start : i == n-2 ? pen_start : mid_origin + (i-1) mid_step  and has
// i == 0 ? first_units : i == n-1 ? last_units : 4  units.
#pragma once
#include <cstddef>

namespace mi_sweep {

constexpr unsigned kUnitQueries = 4096;
constexpr unsigned kTileUnits = 4;
constexpr unsigned kMaxPhases = 8;

// I: the integer that holds a count of units -- size_t on the host, 32 bits in the kernel (one scalar register each;
// the host launches the kernel only where they suffice)
template <class I>
struct PartitionT {
    unsigned ntiles;        // tiles of this workgroup
    unsigned first_units;   // units of tile 0 (0 if the workgroup has no tile)
    unsigned last_units;    // units of tile ntiles - 1 (first_units if ntiles == 1)
    I work;                 // w_s: units of this workgroup
    I first_start;          // starts, in units
    I mid_origin;
    I mid_step;
    I pen_start;            // tile ntiles - 2 (first_start if ntiles < 2)
    I last_start;           // tile ntiles - 1
};
using Partition = PartitionT<size_t>;

// The first-tile table travels as one number.  Outside (environment, C ABI): a decimal digit per class, class 0 first
// (4123 = {4, 1, 2, 3}).  Inside: four bits per class, class k at bits 4k .. 4k+3, so that the kernel indexes it with a
// shift and keeps no array.  Returns 0 unless the decimal number has exactly P digits, all in 1..4.
__host__ __device__ inline unsigned pack_first_units(unsigned decimal, unsigned P)
{
    if (P == 0 || P > kMaxPhases) return 0;
    unsigned nibbles = 0;
    for (unsigned k = P; k-- > 0;) {
        const unsigned digit = decimal % 10u;
        decimal /= 10u;
        if (digit < 1 || digit > kTileUnits) return 0;
        nibbles |= digit << (4 * k);
    }
    return decimal == 0 ? nibbles : 0;
}
__host__ __device__ inline unsigned first_units_of(unsigned nibbles, unsigned k) { return (nibbles >> (4 * k)) & 15u; }

// number of workgroups of class k among nwg (blockIdx % P == k)
__host__ __device__ inline unsigned class_size(unsigned nwg, unsigned P, unsigned k) { return nwg > k ? (nwg - k + P - 1) / P : 0; }

namespace detail {

template <class I>
struct Sums {
    I first, row1, row2;   // units in first tiles, in row R+1 and in row R+2, of the ranks counted
};

template <class I>
__host__ __device__ inline I min_sz(I a, I b) { return a < b ? a : b; }

// the three sums over ranks 0 .. upto-1; R = regular rows.  A class is a run of consecutive ranks, and inside it the
// ranks below `rem` have the larger share: two terms per class.
template <class I>
__host__ __device__ inline Sums<I> sums_below(unsigned upto, unsigned nwg, unsigned P, unsigned fu, I w, unsigned rem, I R)
{
    Sums<I> s{0, 0, 0};
    unsigned a = 0;
    for (unsigned k = 0; k < P; ++k) {
        const unsigned b = a + class_size(nwg, P, k), hi = b < upto ? b : upto;
        if (hi > a) {
            const unsigned n1 = rem > a ? (rem < hi ? rem - a : hi - a) : 0;
            for (unsigned more = 0; more < 2; ++more) {
                const I cnt = more ? n1 : hi - a - n1;
                if (cnt == 0) continue;
                const I share = w + more, f = min_sz<I>(first_units_of(fu, k), share), left = share - f - kTileUnits * R;
                s.first += cnt * f;
                s.row1 += cnt * min_sz<I>(left, kTileUnits);
                s.row2 += cnt * (left > kTileUnits ? left - kTileUnits : 0);
            }
        }
        a = b;
    }
    return s;
}

}  // namespace detail

// U: whole units, nq / 4096
template <class I>
__host__ __device__ inline PartitionT<I> sweep_partition(I U, unsigned nwg, unsigned P, unsigned first_units, unsigned rank)
{
    PartitionT<I> p{};
    if (nwg == 0 || rank >= nwg || P == 0 || P > kMaxPhases) return p;
    const I w = U / nwg;
    const unsigned rem = (unsigned)(U % nwg);
    // R: full tiles behind the first that every rank has = (the least of w_s - first over all ranks) / 4
    I least = ~(I)0;
    unsigned a = 0, cls = 0;
    for (unsigned k = 0; k < P; ++k) {
        const unsigned b = a + class_size(nwg, P, k);
        if (b > a) {
            if (rem > a) least = detail::min_sz<I>(least, w + 1 - detail::min_sz<I>(first_units_of(first_units, k), w + 1));
            if (rem < b) least = detail::min_sz<I>(least, w - detail::min_sz<I>(first_units_of(first_units, k), w));
            if (rank >= a && rank < b) cls = k;
        }
        a = b;
    }
    const I R = least / kTileUnits;
    const detail::Sums<I> all = detail::sums_below<I>(nwg, nwg, P, first_units, w, rem, R);
    const detail::Sums<I> low = detail::sums_below<I>(rank, nwg, P, first_units, w, rem, R);
    p.work = w + (rank < rem ? 1 : 0);
    const I f = detail::min_sz<I>(first_units_of(first_units, cls), p.work), left = p.work - f - kTileUnits * R;
    const unsigned t1 = (unsigned)detail::min_sz<I>(left, kTileUnits), t2 = left > kTileUnits ? (unsigned)(left - kTileUnits) : 0;
    p.first_units = (unsigned)f;
    p.first_start = low.first;
    p.mid_origin = all.first + (I)kTileUnits * rank;
    p.mid_step = (I)kTileUnits * nwg;
    if (f == 0) return p;                                    // no unit at all (the origin and step are still the grid's)
    const I row1 = all.first + p.mid_step * R + low.row1, row2 = all.first + p.mid_step * R + all.row1 + low.row2;
    const I ntiles = 1 + R + (t1 ? 1 : 0) + (t2 ? 1 : 0);
    p.ntiles = (unsigned)ntiles;
    // tile i: 0 the first, 1..R the regular rows, R+1 and R+2 what is left
    auto start_of = [&](I i) { return i == 0 ? p.first_start : i <= R ? p.mid_origin + (i - 1) * p.mid_step : i == R + 1 ? row1 : row2; };
    auto units_of = [&](I i) { return i == 0 ? (unsigned)f : i <= R ? kTileUnits : i == R + 1 ? t1 : t2; };
    p.last_start = start_of(ntiles - 1);
    p.last_units = units_of(ntiles - 1);
    p.pen_start = ntiles >= 2 ? start_of(ntiles - 2) : p.first_start;
    return p;
}

}  // namespace mi_sweep
