// What the two paired-column interp1 units share (mi_pairs1.hip: one query vector for all columns; mi_each1.hip: one per
// column) on the device: the shape of a unit of work, the layouts of X in LDS, the staging of a column into LDS with the
// validation of X on the way, the length rule and the bracket search.  Every kernel of both units compiles to the
// instructions it had when each unit carried its own copy.  The kernels, the blend, the validation
// pass of the direct form and the whole host side stay in the two units.  This header defines no kernel.
#pragma once
#include <cstdint>

#include "mi_interp2_eval.hpp"

namespace mi_paired {

using mi_interp2::kBlock;

constexpr int kQIter = 4;                            // 512-row slices per row block: 8 queries per lane in registers
constexpr int kPrefetch = 2;                         // 16-B vectors per lane and array held in registers for the next column
constexpr int kWaves = kBlock / 64;
constexpr size_t kFlagBytes = 4 * kWaves * sizeof(int);   // per wave: a validation flag for each buffer pair, the query-order flag, padding

typedef __attribute__((address_space(3))) double lds_double;
typedef __attribute__((address_space(3))) int lds_int;

// X in LDS, two layouts (mi_pairs1.hip chooses per unit of work from the unit's queries, the same in all its columns;
// mi_each1.hip always stages skewed):
//   plain   element i at i: when XI ascends along the rows of the unit, the lanes of a wave probe the same or
//           neighbouring nodes at every step of the search: broadcasts and distinct banks, and the cheapest address.
//   skewed  element i at i + (i >> 5), one padding slot per 32 elements (one 256-B bank row of 8-B slots).  The probes
//           of a binary search sit at odd multiples of a power of two; plain, every probe of a step with a stride of 16
//           elements or more falls into the same bank pair, and lanes with unrelated brackets (unsorted XI) serialise up
//           to 32-fold (measured: 12 x the conflict cycles of sorted XI).  Skewed, the probes of different 32-element
//           blocks land in different banks -- at two more address instructions per probe, which a kernel bound by
//           instruction issue feels (sorted XI: 13 % slower than plain), hence the choice.
// Y is not searched and is always plain.
__host__ __device__ inline int skew(int i) { return i + (i >> 5); }
__host__ __device__ inline size_t x_stride(size_t n) { return n + (n >> 5) + 2; }
__host__ __device__ inline size_t lds_bytes_for(size_t n) { return 2 * (x_stride(n) + n + 2) * sizeof(double) + kFlagBytes; }

template <bool SKEW>
struct LdsX {                                        // the staged X of one column
    lds_double* p;
    __device__ __forceinline__ double operator[](int i) const { return p[SKEW ? skew(i) : i]; }
};

// A column on its way into LDS (mi_cols1.hip's ColLoad).  The 16-B vectors start at the column's first 16-B aligned
// element (h = 0 or 1 elements in): vector k holds elements h + 2k, h + 2k + 1, k < nv = (n - h) / 2.  Elements 0 and
// n-1 are fetched by every lane (one line each, broadcast) and cover the head, an odd tail and the padding element.
// For the validation of X: before = element n-2, and in lane 0 of each wave seam[k] = the element in front of its vector.
struct ColLoad {
    d2 v[kPrefetch];
    double seam[kPrefetch];
    double first, last, before;
    int h;
    int nv;
};

// n == 0: nothing is staged (a column whose length is out of range)
template <bool CHECK>
__device__ __forceinline__ void col_issue(ColLoad& L, const double* __restrict__ col, int n)
{
    L.h = (int)((reinterpret_cast<uintptr_t>(col) >> 3) & 1u);
    L.nv = n > 0 ? (n - L.h) >> 1 : 0;
    const d2* p = reinterpret_cast<const d2*>(col + L.h);
    const bool lane0 = (threadIdx.x & 63u) == 0;
#pragma unroll
    for (int k = 0; k < kPrefetch; ++k) {
        const int j = (int)threadIdx.x + k * kBlock;
        L.v[k].x = 0.0;
        L.v[k].y = 0.0;
        L.seam[k] = -__builtin_inf();
        if (j < L.nv) {
            L.v[k] = __builtin_nontemporal_load(p + j);
            if (CHECK && lane0 && L.h + 2 * j > 0) L.seam[k] = col[L.h + 2 * j - 1];
        }
    }
    L.first = L.last = L.before = 0.0;
    if (n > 0) {
        L.first = col[0];
        L.last = col[n - 1];
        if (CHECK) L.before = col[n - 2];
    }
}

// one staged vector against its predecessor: prev < v.x < v.y < +inf
__device__ __forceinline__ bool vec_bad(double prev, d2 v)
{
    return !(prev < v.x) | !(v.x < v.y) | !(v.y < __builtin_inf());
}

// buf: n + 1 elements (index n = padding = the last element).  CHECK: X; returns whether this lane saw the chain broken.
template <bool CHECK, bool SKEW>
__device__ __forceinline__ bool col_commit(const ColLoad& L, const double* __restrict__ col, int n, lds_double* buf)
{
    bool bad = false;
    auto at = [](int i) { return SKEW ? skew(i) : i; };
    const bool lane0 = (threadIdx.x & 63u) == 0;
#pragma unroll
    for (int k = 0; k < kPrefetch; ++k) {
        const int j = (int)threadIdx.x + k * kBlock;
        double prev = 0.0;
        if (CHECK) prev = __shfl_up(L.v[k].y, 1);           // every lane takes part; lane t-1 holds vector j-1
        if (j < L.nv) {
            buf[at(L.h + 2 * j)] = L.v[k].x;
            buf[at(L.h + 2 * j + 1)] = L.v[k].y;
            if (CHECK) bad |= vec_bad(lane0 ? L.seam[k] : prev, L.v[k]);
        }
    }
    const d2* p = reinterpret_cast<const d2*>(col + L.h);
    for (int j0 = kPrefetch * kBlock; j0 < L.nv; j0 += kBlock) {   // the rest of a long column (uniform trip count)
        const int j = j0 + (int)threadIdx.x;
        d2 v;
        v.x = 0.0;
        v.y = 0.0;
        if (j < L.nv) v = __builtin_nontemporal_load(p + j);
        double prev = 0.0;
        if (CHECK) prev = __shfl_up(v.y, 1);
        if (j < L.nv) {
            buf[at(L.h + 2 * j)] = v.x;
            buf[at(L.h + 2 * j + 1)] = v.y;
            if (CHECK) bad |= vec_bad(lane0 ? col[L.h + 2 * j - 1] : prev, v);
        }
    }
    if (threadIdx.x == 0 && n > 0) {
        buf[0] = L.first;
        buf[at(n - 1)] = L.last;
        buf[at(n)] = L.last;
        // the head in front of the first vector, an odd tail behind the last one, and both ends finite
        if (CHECK) bad |= !(-__builtin_inf() < L.first) | !(L.before < L.last) | !(L.last < __builtin_inf());
    }
    return bad;
}

__device__ __forceinline__ int col_len(const uint32_t* __restrict__ len, size_t c, int n)
{
    if (!len) return n;
    const uint32_t m = len[c];
    return (m >= 2u && m <= (uint32_t)n) ? (int)m : 0;     // 0: out of range, the column is bad and nothing of it is read
}

// largest l in [0, nc) with X[l] <= q for each of the lane's 2*kQIter queries (X[0] <= q assumed; any l in range
// otherwise).  Branch-free, the trip count depends on nc alone; the searches of a lane are independent, so their loads
// overlap.
template <typename XP>
__device__ __forceinline__ void search(XP X, int nc, const double (&qa)[kQIter], const double (&qb)[kQIter], int (&la)[kQIter],
                                       int (&lb)[kQIter])
{
#pragma unroll
    for (int j = 0; j < kQIter; ++j) la[j] = lb[j] = 0;
    for (int span = nc; span > 1;) {
        const int half = span >> 1;
#pragma unroll
        for (int j = 0; j < kQIter; ++j) {
            const double xa = X[la[j] + half], xb = X[lb[j] + half];
            la[j] = (xa <= qa[j]) ? la[j] + half : la[j];
            lb[j] = (xb <= qb[j]) ? lb[j] + half : lb[j];
        }
        span -= half;
    }
}

}  // namespace mi_paired
