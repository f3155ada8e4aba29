// interp1 over paired rows: every ROW of Y has an X row of its own.  X and Y column-major m x n (leading dimensions ldx,
// ldy >= m), X(r, k) = x[r + k*ldx], an optional fill count len[r] (valid leading nodes of row r, 2 <= len[r] <= n; NULL:
// n everywhere), queries XI (nxi, any order, shared by every row) -> YI column-major m x nxi (leading dimension ldyi >= m),
//     YI[r + i*ldyi] == mi_interp1_f64_dev's result for XI[i] on the table (X(r, 0:len[r]), Y(r, 0:len[r])),  bit for bit.
// An ensemble stored realisation-fastest ([time level][realisation], the reference's event arrays, index m*R + r), every
// trajectory recorded at its own times, resampled onto one common mesh without a transpose; with n = 2 and nxi = 1 it is
// the shape of the reference's RestrictKernel in fp64.  mi_interp1_pairs_f64_dev's contract with rows for columns.
//
// X is validated on the device at every call with mi_axis1_create's rule: a row is bad when len[r] < 2, len[r] > n, or
// X(r, 0:len[r]) is not finite and strictly increasing -- the chain -inf < X(r,0) < X(r,1) < ... < X(r,len-1) < +inf of
// true comparisons (equal nodes and the pair -0.0, 0.0 are bad).  A bad row's outputs are all NaN; row_ok[r] (optional)
// is 1 for a good row, 0 for a bad one.
//
// The weight is mi_interp2_eval.hpp's weight(), the blend is interp1's (1-w)*Y[l] + w*Y[r], and this file is compiled
// with -ffp-contract=off like every other, so every product and sum rounds.
//
// In this layout the contiguous direction runs across the rows: at one node index k, 64 neighbouring rows are 512
// contiguous bytes of x and of y.  So a lane owns a row.  The work is cut as mi_rows1.hip cuts it: a unit is (block of
// kBlock consecutive rows) x (run of consecutive queries), workgroups of kBlock lanes stride over the units, and the
// queries are cut into runs only as far as filling the machine needs.
//   march   the lanes of a wave walk the run's queries together: XI[i] is the same for all of them and comes down the
//           scalar path.  Each lane keeps the bracket l of its own row with X(r,l), X(r,l+1), Y(r,l), Y(r,l+1) in
//           registers, and X(r,l+2), Y(r,l+2) requested ahead.  For a query the lane keeps its bracket, or advances by
//           one node (the values requested ahead move over, the next pair is requested), or re-locates: a few doubling
//           steps away from the bracket, forward or backward, then a binary search of what is left (the whole row for the
//           first query of a run).  Whatever the path, l is the largest index with X(r,l) <= XI[i] and the four values
//           are those of the row, so the result depends on neither the query order nor the run length nor the grid.
//           Sorted queries make it one pass over each row.  The 64 lanes store YI[r + i*ldyi] for the same i: every
//           store of a wave is one 512-B piece, written non-temporally.
//   short rows (n <= kThinN, form 0): one launch.  Every unit checks its lanes' whole rows first (n coalesced loads per
//           lane); the units of the first run write row_ok.  No workspace: the call never allocates.
//   long rows (form 1): a validation pass first, a lane per row with k ascending (coalesced), writes one flag per row
//           -- into row_ok when the caller gave one, else into context scratch slot 3, which the gridded, shared-axis
//           and long-column paired calls use in stream order on the same stream -- and the march reads the flag.
// Every index into x, y and yi is 64-bit; no grid dimension depends on m, n or nxi.
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "mi_interp2_eval.hpp"

namespace mi_rowpairs1 {

using mi_interp2::kBlock;

constexpr size_t kThinN = 32;                        // rows up to here are validated inside the march kernel (form 0)
constexpr size_t kMinRun = 64;                       // queries per run, at least (but for the last run): a run starts with a search
// Workgroups per CU the grid is cut for -- fewer than the eight that fit.  The lanes of a wave sit at different nodes, so
// a wave's load touches several columns and uses a few bytes of each line it brings in; the other rows of those lines
// come by a little later.  What a CU has in flight must stay in its share of L2 until then: measured on 125 000 x 1024
// onto 2048 sorted points, 8 / 4 / 3 / 2 workgroups per CU take 3.62 / 2.60 / 2.45 / 2.76 ms.
constexpr int kGroupsPerCu = 3;
constexpr int kGallop = 4;                           // doubling steps around the bracket before a re-locate searches the rest of the row
constexpr int kCheckAhead = 8;                      // nodes per lane in flight in the validation pass

// process-wide call counts by form (mi_debug_rowpairs_launches): 0 short rows, 1 long rows
std::atomic<size_t> g_launches[2];

typedef __attribute__((address_space(4))) const double const_double;

// valid nodes of row r; 0: out of range, the row is bad and nothing of it is read
__device__ __forceinline__ int row_len(const uint32_t* __restrict__ len, size_t r, int n)
{
    if (!len) return n;
    const uint32_t c = len[r];
    return (c >= 2u && c <= (uint32_t)n) ? (int)c : 0;
}

// one node against its predecessor: prev < v < +inf
__device__ __forceinline__ bool node_bad(double prev, double v)
{
    return !(prev < v && v < __builtin_inf());
}

// long rows, first pass: flag[r] = 1 when row r is good, 0 when it is bad.  A lane per row, k ascending: a wave's load
// is 512 contiguous bytes; kCheckAhead of them are requested before the first is compared.
__global__ __launch_bounds__(kBlock) void rowpairs1_validate_kernel(const double* __restrict__ x, size_t ldx, size_t m, int n,
                                                                    const uint32_t* __restrict__ len,
                                                                    uint32_t* __restrict__ flag)
{
    const size_t nrb = (m + kBlock - 1) / kBlock;
    for (size_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const size_t r = rb * kBlock + threadIdx.x;
        if (r >= m) continue;
        const int nr = row_len(len, r, n);
        const double* const xr = x + r;
        bool bad = nr == 0;
        double prev = -__builtin_inf();
        int k = 0;
        for (; k + kCheckAhead <= nr; k += kCheckAhead) {
            double v0 = xr[(size_t)(k + 0) * ldx], v1 = xr[(size_t)(k + 1) * ldx], v2 = xr[(size_t)(k + 2) * ldx],
                   v3 = xr[(size_t)(k + 3) * ldx], v4 = xr[(size_t)(k + 4) * ldx], v5 = xr[(size_t)(k + 5) * ldx],
                   v6 = xr[(size_t)(k + 6) * ldx], v7 = xr[(size_t)(k + 7) * ldx];
            static_assert(kCheckAhead == 8, "eight loads are written out");
            bad |= node_bad(prev, v0);
            bad |= node_bad(v0, v1);
            bad |= node_bad(v1, v2);
            bad |= node_bad(v2, v3);
            bad |= node_bad(v3, v4);
            bad |= node_bad(v4, v5);
            bad |= node_bad(v5, v6);
            bad |= node_bad(v6, v7);
            prev = v7;
        }
        for (; k < nr; ++k) {
            const double v = xr[(size_t)k * ldx];
            bad |= node_bad(prev, v);
            prev = v;
        }
        flag[r] = bad ? 0u : 1u;
    }
}

// THIN: short rows, validated here; flag = row_ok, written by the units of the first run (may be null).
// Long rows: flag = the validation pass's flags, read.
// unit u = (row block u % nrb, query run u / nrb): consecutive workgroups take neighbouring row blocks of the same queries.
template <bool THIN>
__global__ __launch_bounds__(kBlock) void rowpairs1_march_kernel(const double* __restrict__ x, size_t ldx,
                                                                 const double* __restrict__ y, size_t ldy, size_t m, int n,
                                                                 const uint32_t* __restrict__ len, const double* __restrict__ xi,
                                                                 size_t nxi, size_t run, size_t nrb, size_t nunits,
                                                                 double* __restrict__ yi, size_t ldyi, double extrap,
                                                                 uint32_t* flag)
{
    // XI is read through the constant address space (nothing in this kernel writes it): the query of an iteration is the
    // same for every lane and stays on the scalar path, where it waits for none of the lanes' loads and stores
    const const_double* const cxi = (const const_double*)xi;
    const double inf = __builtin_inf();
    for (size_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const size_t s = u / nrb, rb = u - s * nrb;
        const size_t c0 = s * run, c1 = min(c0 + run, nxi);
        const size_t r = rb * kBlock + threadIdx.x;
        const bool active = r < m;
        const int nr = active ? row_len(len, r, n) : 0;
        const int last = nr - 1;
        const double* const xrow = x + r;
        const double* const yrow = y + r;
        double* const orow = yi + r;
        bool ok;
        double x0 = 0.0, x1 = 0.0;
        if constexpr (THIN) {
            bool bad = nr == 0;
            double prev = -inf;
#pragma unroll 4
            for (int k = 0; k < n; ++k) {                    // (n is uniform and small; a shorter row stops taking part)
                if (k < nr) {
                    const double v = xrow[(size_t)k * ldx];
                    bad |= node_bad(prev, v);
                    if (k == 0) x0 = v;
                    prev = v;
                }
            }
            x1 = prev;
            ok = !bad;
            if (flag && s == 0 && active) flag[r] = ok ? 1u : 0u;
        } else {
            ok = active && flag[r] != 0;
            if (ok) {
                x0 = xrow[0];
                x1 = xrow[(size_t)last * ldx];
            }
        }
        // the bracket held: l, the nodes l and rr = min(l+1, last), and node min(l+2, last) requested ahead.
        // Nothing is held at first: l = nr and +inf send the run's first query in range to the search over the whole row.
        int l = nr;
        double xl = inf, xr = inf, yl = 0.0, yr = 0.0, xn = inf, yn = 0.0;
        for (size_t i = c0; i < c1; ++i) {
            const double q = cxi[i];
            double v = (q != q) ? __builtin_nan("") : extrap;
            if (ok && q >= x0 && q <= x1) {
                const bool keep = q >= xl && (q < xr || l == last);
                if (!keep) {
                    const bool advance = l < last && q >= xr && (q < xn || l + 1 == last);
                    if (advance) {
                        ++l;
                        xl = xr;
                        yl = yr;
                        xr = xn;
                        yr = yn;
                    } else {
                        // the new l is the largest index in [lo, lo + span) with X <= q, X[lo] <= q known.  Nothing held: the
                        // whole row.  Otherwise the neighbourhood first, in doubling steps away from the bracket (the nodes
                        // the neighbouring lanes are at, so mostly lines that are in the cache), then the rest of the row.
                        int lo = 0, span = nr;
                        if (q >= xl) {                       // in front: X[l+2] <= q (it is neither kept nor advanced)
                            lo = l + 2;
                            span = nr - lo;
                            int step = 2;
                            for (int g = 0; g < kGallop; ++g) {
                                const int p = lo + step;
                                if (p > last) break;
                                if (!(xrow[(size_t)p * ldx] <= q)) {
                                    span = step;
                                    break;
                                }
                                lo = p;
                                span = nr - lo;
                                step <<= 1;
                            }
                        } else if (l != nr) {                // behind: q < X[hi]
                            int hi = l, step = 1;
                            span = hi;
                            for (int g = 0; g < kGallop; ++g) {
                                const int p = hi - step;
                                if (p <= 0) break;
                                if (xrow[(size_t)p * ldx] <= q) {
                                    lo = p;
                                    span = hi - p;
                                    break;
                                }
                                hi = p;
                                span = hi;
                                step <<= 1;
                            }
                        }
                        while (span > 1) {
                            const int half = span >> 1;
                            const double xv = xrow[(size_t)(lo + half) * ldx];
                            lo = (xv <= q) ? lo + half : lo;
                            span -= half;
                        }
                        l = lo;
                        const int rr = min(l + 1, last);
                        xl = xrow[(size_t)l * ldx];
                        yl = yrow[(size_t)l * ldy];
                        xr = xrow[(size_t)rr * ldx];
                        yr = yrow[(size_t)rr * ldy];
                    }
                    const int k2 = min(l + 2, last);
                    xn = xrow[(size_t)k2 * ldx];
                    yn = yrow[(size_t)k2 * ldy];
                }
                const double w = mi_interp2::weight(xl, xr, q);
                v = (1.0 - w) * yl + w * yr;
            }
            if (!ok) v = __builtin_nan("");
            if (active) __builtin_nontemporal_store(v, orow + i * ldyi);
        }
    }
}

// the argument rules of the entry point, in mi_pairs1.hip's words with rows for columns
mi_status check_args(const mi_ctx* ctx, const char* who, const double* x, size_t ldx, const double* y, size_t ldy, size_t m,
                     size_t n, const uint32_t* len, const double* xi, size_t nxi, const double* yi, size_t ldyi,
                     const uint32_t* row_ok)
{
    MI_REQUIRE(ctx, x && y && xi && yi, "%s: NULL table/query/result pointer", who);
    const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xi) |
                         reinterpret_cast<uintptr_t>(yi);
    MI_REQUIRE(ctx, (al & 7u) == 0, "%s: x, y, xi, yi must be 8-byte aligned", who);
    const uintptr_t al4 = reinterpret_cast<uintptr_t>(len) | reinterpret_cast<uintptr_t>(row_ok);
    MI_REQUIRE(ctx, (al4 & 3u) == 0, "%s: len, row_ok must be 4-byte aligned", who);
    MI_REQUIRE(ctx, n >= 2, "%s: need at least two nodes per row (n=%zu)", who, n);
    MI_REQUIRE(ctx, n < 0x7ffffff0u, "%s: n=%zu exceeds 2^31 - 16", who, n);
    MI_REQUIRE(ctx, ldx >= m, "%s: ldx=%zu is smaller than m=%zu", who, ldx, m);
    MI_REQUIRE(ctx, ldy >= m, "%s: ldy=%zu is smaller than m=%zu", who, ldy, m);
    MI_REQUIRE(ctx, ldyi >= m, "%s: ldyi=%zu is smaller than m=%zu", who, ldyi, m);
    const size_t lim = SIZE_MAX / (2 * sizeof(double));
    MI_REQUIRE(ctx, ldx <= lim / n && ldy <= lim / n && ldyi <= lim / nxi && m <= lim,
               "%s: m=%zu, or ldx=%zu, ldy=%zu x n=%zu, or ldyi=%zu x nxi=%zu too large", who, m, ldx, ldy, n, ldyi, nxi);
    return MI_OK;
}

}  // namespace mi_rowpairs1

using namespace mi_rowpairs1;

extern "C" {

size_t mi_debug_rowpairs_launches(int form)
{
    return (form >= 0 && form < 2) ? g_launches[form].load(std::memory_order_relaxed) : 0;
}

mi_status mi_interp1_rowpairs_f64_dev(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, size_t m, size_t n,
                                      const uint32_t* len, const double* xi, size_t nxi, double* yi, size_t ldyi, double extrap,
                                      uint32_t* row_ok)
{
    MI_REQUIRE(ctx, ctx, "mi_interp1_rowpairs_f64_dev: NULL context");
    if (m == 0 || nxi == 0) return MI_OK;
    mi_status st = check_args(ctx, "mi_interp1_rowpairs_f64_dev", x, ldx, y, ldy, m, n, len, xi, nxi, yi, ldyi, row_ok);
    if (st != MI_OK) return st;
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    // units: row blocks x query runs.  kGroupsPerCu workgroups per CU are launched at most; when the rows alone give
    // fewer units than two per such workgroup the queries are cut into runs, never below kMinRun queries (every run
    // begins with a search of its rows): a small call leaves workgroups idle rather than searching more than it marches
    const size_t resident = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * kGroupsPerCu;
    const size_t target = resident * 2;
    const size_t nrb = (m + kBlock - 1) / kBlock;
    const size_t want_runs = std::max<size_t>(1, std::min(target / nrb, (nxi + kMinRun - 1) / kMinRun));
    const size_t run = (nxi + want_runs - 1) / want_runs;
    const size_t nruns = (nxi + run - 1) / run;
    MI_REQUIRE(ctx, nrb <= SIZE_MAX / nruns, "mi_interp1_rowpairs_f64_dev: m=%zu x nxi=%zu too large", m, nxi);
    const size_t nunits = nrb * nruns;
    const unsigned grid = (unsigned)std::min(nunits, resident);   // workgroups stride over the units beyond that
    if (n <= kThinN) {
        hipLaunchKernelGGL(rowpairs1_march_kernel<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, x, ldx, y, ldy, m, (int)n, len, xi,
                           nxi, run, nrb, nunits, yi, ldyi, extrap, row_ok);
        MI_LAUNCH_CHECK(ctx, "interp1 rowpairs kernel");
        g_launches[0].fetch_add(1, std::memory_order_relaxed);
        return MI_OK;
    }
    uint32_t* flag = row_ok;
    if (!flag) {
        st = mi::ensure_scratch(ctx, 3, m * sizeof(uint32_t));
        if (st != MI_OK) return st;
        flag = (uint32_t*)ctx->scratch[3];
    }
    hipLaunchKernelGGL(rowpairs1_validate_kernel, dim3(mi::stream_grid(ctx, m, kBlock)), dim3(kBlock), 0, ctx->stream, x, ldx, m,
                       (int)n, len, flag);
    MI_LAUNCH_CHECK(ctx, "interp1 rowpairs validation kernel");
    hipLaunchKernelGGL(rowpairs1_march_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, x, ldx, y, ldy, m, (int)n, len, xi,
                       nxi, run, nrb, nunits, yi, ldyi, extrap, flag);
    MI_LAUNCH_CHECK(ctx, "interp1 rowpairs kernel");
    g_launches[1].fetch_add(1, std::memory_order_relaxed);
    return MI_OK;
}

}  // extern "C"
