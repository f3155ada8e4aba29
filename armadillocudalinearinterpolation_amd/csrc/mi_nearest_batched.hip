// arma::interp1's "nearest" method for the two batched shapes whose tables do not lie along a column of one shared
// axis: one table per ROW of a matrix (mi_interp1_rows_nearest_f64_dev: one mi_axis1, Y column-major m x n -- the
// [time level][realisation] layout, or the slices of a cube) and paired columns (mi_interp1_pairs_nearest_f64_dev: every
// column of Y with an X column of its own).  Hand-written HIP for gfx950; memory-bound, no MFMA.
//
// Nearest rule (include/mi355_interp.h): the bracket l is the linear call's (largest node with X[l] <= q), r = min(l+1, n-1),
//     a = q - X[l];  b = X[r] - q;  k = (b < a) ? r : l;  out = Y[k]
// -- a tie keeps the left node, the decision comes from a and b themselves, and the value is copied: no arithmetic
// touches it.  q outside [X[0], X[n-1]] -> extrap, q = NaN -> NaN.
//
// This unit stands beside the linear twins (the rows and the paired-column units) and the first nearest unit rather than
// inside them: tests pin those files on their text and on the kernels their namespaces hold.  What it needs of them is
// restated here and held to the originals by tests/test_nearest_batched_cpu.py: take_right, col_load / col_store, the
// unit arithmetic of both host sides, the validation pass of long paired columns and check_args.  mi_axis1.hpp,
// mi_interp2_eval.hpp (AxisDev, axis_locate, axis_node, kBlock) and mi_paired_cols.hpp (the LDS layouts, the staging of
// a column with the validation of X on the way, col_len, search) are used as they are.
//
// Rows, two launches on the context's stream:
//   locate  every XI[i] -> one int32 (k >= 0 the nearest node, -1 out of range, -2 NaN) into context scratch slot 3,
//           the record workspace of the linear calls, in stream order with them.
//   rows    the linear call's units: (block of kRowBlock consecutive rows) x (run of consecutive output columns),
//           workgroups of 256 lanes striding over the units.  An output column is ONE input column, copied.
//     tile body (m >= kThinM): a lane owns kLaneRows rows of the block (16-B form: rows 2t, 2t+1, 512+2t, 513+2t; 8-B
//           form: rows t + 256 j) and keeps one column of Y, hk, in registers, and one on its way, nk, wanted at output
//           column jn.  The walk over the records that finds jn -- the next output whose k >= 0 and k != hk -- runs on
//           the scalar path, and the load of column nk is issued before the outputs of hk are stored.  A flagged record
//           stores NaN / extrap and leaves the held column alone; k == hk loads nothing.  With sorted XI every column
//           of Y some query is nearest to is read once per row block and run; the others are never read.
//     flat body (m < kThinM): the linear flat body's indexing, one 8-B load y[k*ldy + r] per output.
// Pairs, the linear call's units (row block of kPairRowBlock outputs x run of columns), no records:
//   LDS form (n <= kLdsMaxN): X[:, c] and Y[:, c] staged into one of two LDS buffer pairs, X validated on the way, the
//           next column's loads in flight while this one is served, one barrier per column, X plain or skewed per
//           unit.  After the bracket search one output is take_right(X[l], X[l+1], q) and ONE read Y[l + right]: two
//           subtractions, a compare and an LDS read where the linear call divides and blends.  The padding element at
//           index n_c holds the last node, so at l = n_c-1 both differences are 0 and the left node is kept.
//   direct form (longer columns): a validation pass writes one flag per column (into col_ok when given, else into
//           scratch slot 3); the column kernel searches x[:, c] through L2 and gathers y[k, c] once.
// YI is written with coalesced non-temporal stores, 16 B where the pointers and leading dimensions allow.
// Every index into x, y and yi is 64-bit; no grid dimension depends on m, n, B or nxi.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <type_traits>

#include "mi_axis1.hpp"
#include "mi_interp2_eval.hpp"
#include "mi_paired_cols.hpp"

namespace mi_nearest_batched {

using mi_interp2::kBlock;
using namespace mi_paired;   // the LDS layouts, the staging of a column (ColLoad ...), col_len and search, as they are

// ---- restated from the rows unit (the same expressions; a CPU test compares them) ----------------------------------
constexpr int kLaneRows = 4;                         // rows of a block per lane (tile body)
constexpr size_t kRowBlock = 1024;                   // = kLaneRows * kBlock rows per unit of the tile body: 8 KiB of a column
constexpr size_t kThinM = kBlock;                    // m below: flat body
constexpr int kFlatStep = 2 * kBlock;                // outputs per step of the flat body
constexpr size_t kMaxFlatRun = (size_t)1 << 23;      // columns per run of the flat body: run * m stays below 2^31
constexpr size_t kMinRun = 16;                       // output columns per run of the tile body, at least (but for the last run)
constexpr size_t kMinFlatUnit = 4 * kFlatStep;       // outputs per run of the flat body, about as many at least
static_assert(kRowBlock == (size_t)kLaneRows * kBlock, "a lane owns kLaneRows rows of a block");
// ---- restated from the paired-column unit ---------------------------------------------------------------------------
constexpr size_t kPairRowBlock = 2 * kBlock * kQIter;    // 2048 outputs of one column per unit
constexpr size_t kLdsMaxN = 4096;                    // LDS form up to here: 2 pairs x (2 n + n/32 + 4) x 8 B + flags = 133248 B of the CU's 160 KiB

// mi_debug_nearest_batched_launches: 0 rows tile 16-B, 1 rows tile 8-B, 2 rows flat, 3 pairs LDS form, 4 pairs direct form
std::atomic<size_t> g_launches[5];
inline void count(int form) { g_launches[form].fetch_add(1, std::memory_order_relaxed); }

// k = (b < a) ? r : l on the values the caller holds for both nodes
__device__ __forceinline__ bool take_right(double xl, double xr, double q)
{
    const double a = q - xl;
    const double b = xr - q;
    return b < a;
}

// ---- rows -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void nb_rows_locate_kernel(AxisDev ax, const double* __restrict__ xi, size_t nxi,
                                                                int* __restrict__ idx)
{
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < nxi; k += (size_t)gridDim.x * kBlock) {
        const double q = xi[k];
        int r;
        if (!(q >= ax.xmin && q <= ax.xmax)) {
            r = (q != q) ? -2 : -1;
        } else {
            const int l = mi_interp2::axis_locate(ax, q);
            const int rr = min(l + 1, ax.n - 1);
            r = take_right(mi_interp2::axis_node(ax, l), mi_interp2::axis_node(ax, rr), q) ? rr : l;
        }
        idx[k] = r;
    }
}

// The lane's kLaneRows elements of one column of a row block; p: the column at the block's first row, rows: rows of the
// block that exist (1..kRowBlock).  VEC: p is 16-B aligned.  FULL: rows == kRowBlock, nothing to test.  Elements of rows
// that do not exist are left alone.
template <bool VEC, bool FULL>
__device__ __forceinline__ void col_load(double (&v)[kLaneRows], const double* __restrict__ p, int t, int rows)
{
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < kLaneRows / 2; ++j) {
            const int r = 2 * t + j * 2 * kBlock;
            if (FULL || r + 1 < rows) {
                const d2 x = *reinterpret_cast<const d2*>(p + r);
                v[2 * j] = x.x;
                v[2 * j + 1] = x.y;
            } else if (r < rows) {
                v[2 * j] = p[r];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kLaneRows; ++j) {
            const int r = t + j * kBlock;
            if (FULL || r < rows) v[j] = p[r];
        }
    }
}

template <bool VEC, bool FULL>
__device__ __forceinline__ void col_store(const double (&v)[kLaneRows], double* __restrict__ p, int t, int rows)
{
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < kLaneRows / 2; ++j) {
            const int r = 2 * t + j * 2 * kBlock;
            if (FULL || r + 1 < rows) {
                d2 x;
                x.x = v[2 * j];
                x.y = v[2 * j + 1];
                __builtin_nontemporal_store(x, reinterpret_cast<d2*>(p + r));
            } else if (r < rows) {
                __builtin_nontemporal_store(v[2 * j], p + r);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kLaneRows; ++j) {
            const int r = t + j * kBlock;
            if (FULL || r < rows) __builtin_nontemporal_store(v[j], p + r);
        }
    }
}

// the records through the constant address space (they were written by the locate kernel, before this one began): that
// keeps their reads on the scalar path, where they wait for nothing but themselves -- as vector loads they would wait
// for every store and every column in flight
typedef __attribute__((address_space(4))) int const_idx;

// the first output column j in [j, c1) whose record is a node other than hk; that node in nk.  c1 when there is none.
// Uniform: every lane walks the same records.
__device__ __forceinline__ size_t next_column(const const_idx* cidx, size_t j, size_t c1, int hk, int& nk)
{
    for (; j < c1; ++j) {
        const int k = cidx[j];
        if (k >= 0 && k != hk) {
            nk = k;
            break;
        }
    }
    return j;
}

// One unit of the tile body: output columns [c0, c1) of one row block; yb, ob: y and yi at the block's first row.
// FULL: all kRowBlock rows exist.  A block cut short by m tests its rows per access; `rows` is then passed through an empty
// asm statement inside the loops, so that the tests stay where they are: hoisted out of a loop as lane-dependent loop
// versions, they would take the uniform (scalar) record path away from everything below.
template <bool VEC, bool FULL>
__device__ __forceinline__ void tile_unit(const int* __restrict__ idx, const double* __restrict__ yb, size_t ldy, size_t c0,
                                          size_t c1, double* __restrict__ ob, size_t ldyi, double extrap, int t, int rows)
{
    const const_idx* const cidx = (const const_idx*)idx;
    // the outputs [i, j) of the column held in a (flagged ones among them: NaN / extrap): no load in here
    auto emit = [&](const double (&a)[kLaneRows], size_t i, size_t j) {
        for (; i < j; ++i) {
            if constexpr (!FULL) asm volatile("" : "+v"(rows));
            const int k = cidx[i];                               // uniform; flagged, or the node held
            if (k < 0) {
                const double f = (k == -2) ? __builtin_nan("") : extrap;
                double v[kLaneRows];
#pragma unroll
                for (int e = 0; e < kLaneRows; ++e) v[e] = f;
                col_store<VEC, FULL>(v, ob + i * ldyi, t, rows);
            } else {
                col_store<VEC, FULL>(a, ob + i * ldyi, t, rows);
            }
        }
    };
    // a: column hk of Y, this lane's rows; p: column nk on its way, wanted at output column jn
    double a[kLaneRows], p[kLaneRows];
#pragma unroll
    for (int k = 0; k < kLaneRows; ++k) a[k] = p[k] = 0.0;
    int hk = -1, nk = -1;
    size_t jn = next_column(cidx, c0, c1, hk, nk);
    if (jn >= c1) {                                              // a run without any column: every output is flagged
        emit(a, c0, c1);
        return;
    }
    col_load<VEC, FULL>(p, yb + (size_t)nk * ldy, t, rows);
    emit(a, c0, jn);                                             // the flagged outputs in front of the first column
    // One trip per column held.  The order inside a trip is the point: the column on its way becomes the one held (the
    // wait for its load is here), the column after it is looked up in the records and requested, and only then are
    // the outputs of the one held stored -- the next load is in flight while they issue.  The load is unconditional
    // on the way round the loop (the last trip leaves through the break before it): a load under a condition ends in
    // a register copy at the join, and the wait for the load with it, in front of the stores.
    for (size_t i = jn;;) {
        if constexpr (!FULL) asm volatile("" : "+v"(rows));
#pragma unroll
        for (int e = 0; e < kLaneRows; ++e) a[e] = p[e];
        hk = nk;
        jn = next_column(cidx, i + 1, c1, hk, nk);
        if (jn >= c1) {
            emit(a, i, c1);
            break;
        }
        col_load<VEC, FULL>(p, yb + (size_t)nk * ldy, t, rows);
        emit(a, i, jn);
        i = jn;
    }
}

// Tile body.  VEC: 16-B accesses (y, yi 16-B aligned, ldy, ldyi even) / 8-B accesses.
// unit u = (row block u % nrb, column run u / nrb): consecutive workgroups take neighbouring row blocks of the same columns.
template <bool VEC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void nb_rows_tile_kernel(
    const int* __restrict__ idx, const double* __restrict__ y, size_t ldy, size_t m, size_t nxi, size_t run, size_t nrb,
    size_t nunits, double* __restrict__ yi, size_t ldyi, double extrap)
{
    const int t = (int)threadIdx.x;
    for (size_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const size_t s = u / nrb, rb = u - s * nrb;
        const size_t c0 = s * run, c1 = min(c0 + run, nxi);
        const size_t row0 = rb * kRowBlock;
        const int rows = (int)min(kRowBlock, m - row0);
        if (rows == (int)kRowBlock) tile_unit<VEC, true>(idx, y + row0, ldy, c0, c1, yi + row0, ldyi, extrap, t, rows);
        else tile_unit<VEC, false>(idx, y + row0, ldy, c0, c1, yi + row0, ldyi, extrap, t, rows);
    }
}

// Flat body: unit u = run u of output columns, all m rows.
__global__ __launch_bounds__(kBlock) void nb_rows_flat_kernel(const int* __restrict__ idx, const double* __restrict__ y, size_t ldy,
                                                              uint32_t m, size_t nxi, size_t run, size_t nunits,
                                                              double* __restrict__ yi, size_t ldyi, double extrap)
{
    const uint32_t t = threadIdx.x;
    const uint32_t qs = (uint32_t)kFlatStep / m, rs = (uint32_t)kFlatStep - qs * m;   // a step in (columns, rows)
    uint32_t qo[2], ro[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t o = t + (uint32_t)h * kBlock;
        qo[h] = o / m;
        ro[h] = o - qo[h] * m;
    }
    for (size_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const size_t c0 = u * run, c1 = min(c0 + run, nxi);
        // outputs k = r + (i - c0)*m of the run; this lane's two of a step: t and t + 256 into it
        const uint32_t total = (uint32_t)(c1 - c0) * m;
        uint32_t jb = 0, ib = 0;                             // column and row of the step's first output
        for (uint32_t k0 = 0; k0 < total; k0 += kFlatStep) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (k0 + t + (uint32_t)h * kBlock < total) {
                    uint32_t r = ib + ro[h], dj = jb + qo[h];
                    if (r >= m) {
                        r -= m;
                        ++dj;
                    }
                    const size_t i = c0 + dj;
                    const int k = idx[i];
                    double v = (k == -2) ? __builtin_nan("") : extrap;
                    if (k >= 0) v = y[(size_t)k * ldy + r];
                    __builtin_nontemporal_store(v, yi + i * ldyi + r);
                }
            }
            jb += qs;
            ib += rs;
            if (ib >= m) {
                ib -= m;
                ++jb;
            }
        }
    }
}

// ---- pairs ----------------------------------------------------------------------------------------------------------

// one output: X, Y readable at l and at l + 1 (LDS form: the padding element) or at r = min(l+1, nc-1) (direct form)
template <bool LDSF, typename XP, typename YP>
__device__ __forceinline__ double pick(XP X, YP Y, int nc, int l, double q, double x0, double x1, double extrap)
{
    const int r = LDSF ? l + 1 : min(l + 1, nc - 1);
    double v = Y[take_right(X[l], X[r], q) ? r : l];
    if (!(q >= x0 && q <= x1)) v = (q != q) ? __builtin_nan("") : extrap;
    return v;
}

// direct form, first pass: flag[c] = 1 when column c is good, 0 when it is bad; workgroups stride over the columns
__global__ __launch_bounds__(kBlock) void nb_pairs_validate_kernel(const double* __restrict__ x, size_t ldx, int n,
                                                                   const uint32_t* __restrict__ len, size_t ncols,
                                                                   uint32_t* __restrict__ flag)
{
    __shared__ int wave_bad[kWaves];
    for (size_t c = blockIdx.x; c < ncols; c += gridDim.x) {
        const double* const col = x + c * ldx;
        const int nc = col_len(len, c, n);
        bool bad = nc == 0;
        for (int k = (int)threadIdx.x; k < nc; k += kBlock) {
            const double xv = col[k];
            const double prev = k > 0 ? col[k - 1] : -__builtin_inf();
            bad |= !(prev < xv) | !(xv < __builtin_inf());
        }
        const bool wb = __any(bad);
        if ((threadIdx.x & 63u) == 0) wave_bad[threadIdx.x >> 6] = wb;
        __syncthreads();
        if (threadIdx.x == 0) {
            int any = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) any |= wave_bad[w];
            flag[c] = any ? 0u : 1u;
        }
        __syncthreads();
    }
}

// LDSF: LDS form / direct form.  VEC: 16-B stores (yi 16-B aligned, ldyi even) / 8-B stores.
// unit u = (row block u % nrb, column run u / nrb): consecutive workgroups share a run's columns (L2) in the LDS form.
// flag: LDS form: col_ok, written (may be null); direct form: the validation pass's flags, read.
template <bool LDSF, bool VEC>
__global__ __launch_bounds__(kBlock) void nb_pairs_kernel(const double* __restrict__ x, size_t ldx, const double* __restrict__ y,
                                                          size_t ldy, int n, const uint32_t* __restrict__ len, size_t ncols,
                                                          size_t run, const double* __restrict__ xi, size_t nxi, size_t nrb,
                                                          size_t nunits, double* __restrict__ yi, size_t ldyi, double extrap,
                                                          uint32_t* flag)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    lds_double* const lds = (lds_double*)smem;
    const int sx = (int)x_stride((size_t)n);                // elements of a staged X (room for the skew), then n + 2 of its Y
    const int pair = sx + n + 2;
    lds_int* const wflag = (lds_int*)(lds + 2 * (size_t)pair);   // [2 buffer pairs][kWaves] validation, then [kWaves] query order
    const int t = (int)threadIdx.x;
    for (size_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const size_t rb = u % nrb, s = u / nrb;
        const size_t c0 = s * run, c1 = min(c0 + run, ncols);
        const size_t row0 = rb * kPairRowBlock;
        // this lane's rows, (ia, ib) + j*512 for j < kQIter, and their queries (NaN where there is no such row)
        const size_t ia = row0 + (VEC ? 2 * t : t), ib = ia + (VEC ? 1 : kBlock);
        double qa[kQIter], qb[kQIter];
#pragma unroll
        for (int j = 0; j < kQIter; ++j) {
            const size_t o = (size_t)j * (2 * kBlock);
            qa[j] = (ia + o < nxi) ? xi[ia + o] : __builtin_nan("");
            qb[j] = (ib + o < nxi) ? xi[ib + o] : __builtin_nan("");
        }
        // the layout of X in LDS for this unit: plain when every wave's queries ascend along the rows (NaN is neutral)
        bool plain = true;
        if constexpr (LDSF) {
            bool asc = true;
#pragma unroll
            for (int j = 0; j < kQIter; ++j) {
                const double na = __shfl_down(qa[j], 1), nb = __shfl_down(qb[j], 1);   // the next lane's rows
                const bool last = (t & 63) == 63;
                if (VEC) asc &= !(qa[j] > qb[j]) & (last | !(qb[j] > na));
                else asc &= (last | (!(qa[j] > na) & !(qb[j] > nb)));
            }
            const bool wasc = __all(asc);
            if ((t & 63) == 0) wflag[2 * kWaves + (t >> 6)] = wasc;
            __syncthreads();
            int all = 1;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) all &= wflag[2 * kWaves + w];
            plain = all != 0;
        }
        auto unit = [&](auto skew_tag) {
            constexpr bool SKEW = decltype(skew_tag)::value;
            ColLoad LX, LY;
            int nc_next = 0;
            if constexpr (LDSF) {
                // (every column of the previous unit ended on a barrier: both buffer pairs are free)
                nc_next = col_len(len, c0, n);
                col_issue<true>(LX, x + c0 * ldx, nc_next);
                col_issue<false>(LY, y + c0 * ldy, nc_next);
                const bool bad = col_commit<true, SKEW>(LX, x + c0 * ldx, nc_next, lds) | (nc_next == 0);
                col_commit<false, false>(LY, y + c0 * ldy, nc_next, lds + sx);
                const bool wb = __any(bad);
                if ((t & 63) == 0) wflag[t >> 6] = wb;
                __syncthreads();
            }
            for (size_t c = c0; c < c1; ++c) {
                const int cb = (int)((c - c0) & 1);
                const bool more = c + 1 < c1;
                const double* const xcol = x + c * ldx;
                const double* const ycol = y + c * ldy;
                int nc;
                bool ok;
                if constexpr (LDSF) {
                    nc = nc_next;
                    if (more) {                                  // in flight while this column is searched and served
                        nc_next = col_len(len, c + 1, n);
                        col_issue<true>(LX, xcol + ldx, nc_next);
                        col_issue<false>(LY, ycol + ldy, nc_next);
                    }
                    int any = 0;
#pragma unroll
                    for (int w = 0; w < kWaves; ++w) any |= wflag[cb * kWaves + w];
                    ok = any == 0;
                    if (flag && rb == 0 && t == 0) flag[c] = ok ? 1u : 0u;
                } else {
                    nc = col_len(len, c, n);
                    ok = flag[c] != 0;
                }
                double* const out = yi + c * ldyi;
                int la[kQIter], lb[kQIter];
                double x0 = 0.0, x1 = 0.0;
                const LdsX<SKEW> curx = {lds + (size_t)cb * pair};
                lds_double* const cury = curx.p + sx;
                if (ok) {                                        // (uniform; a bad column is not searched: nc may be 0)
                    if constexpr (LDSF) {
                        x0 = curx[0];
                        x1 = curx[nc - 1];
                        search(curx, nc, qa, qb, la, lb);
                    } else {
                        x0 = xcol[0];
                        x1 = xcol[nc - 1];
                        search(xcol, nc, qa, qb, la, lb);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < kQIter; ++j) la[j] = lb[j] = 0;
                }
#pragma unroll
                for (int j = 0; j < kQIter; ++j) {
                    const size_t o = (size_t)j * (2 * kBlock);
                    if (!(ia + o < nxi)) continue;
                    const bool hb = ib + o < nxi;
                    double* const oa = out + ia + o;
                    double va = __builtin_nan(""), vb = va;
                    if (ok) {
                        if constexpr (LDSF) {
                            va = pick<true>(curx, cury, nc, la[j], qa[j], x0, x1, extrap);
                            vb = pick<true>(curx, cury, nc, lb[j], qb[j], x0, x1, extrap);
                        } else {
                            va = pick<false>(xcol, ycol, nc, la[j], qa[j], x0, x1, extrap);
                            vb = pick<false>(xcol, ycol, nc, lb[j], qb[j], x0, x1, extrap);
                        }
                    }
                    if (VEC && hb) {
                        d2 o2;
                        o2.x = va;
                        o2.y = vb;
                        __builtin_nontemporal_store(o2, reinterpret_cast<d2*>(oa));
                    } else {
                        __builtin_nontemporal_store(va, oa);
                        if (hb) __builtin_nontemporal_store(vb, oa + (ib - ia));
                    }
                }
                if constexpr (LDSF) {
                    if (more) {
                        lds_double* const nx = lds + (size_t)(cb ^ 1) * pair;
                        const bool bad = col_commit<true, SKEW>(LX, xcol + ldx, nc_next, nx) | (nc_next == 0);
                        col_commit<false, false>(LY, ycol + ldy, nc_next, nx + sx);
                        const bool wb = __any(bad);
                        if ((t & 63) == 0) wflag[(cb ^ 1) * kWaves + (t >> 6)] = wb;
                    }
                    __syncthreads();
                }
            }
        };
        if (plain) unit(std::false_type{});
        else unit(std::true_type{});
    }
}

template <bool LDSF, bool VEC>
mi_status launch_pairs(mi_ctx* ctx, unsigned grid, size_t lds_bytes, const double* x, size_t ldx, const double* y, size_t ldy, int n,
                       const uint32_t* len, size_t ncols, size_t run, const double* xi, size_t nxi, size_t nrb, size_t nunits,
                       double* yi, size_t ldyi, double extrap, uint32_t* flag)
{
    if (lds_bytes > 64 * 1024)   // above the default limit of dynamic LDS (per device: asked for at every such launch)
        MI_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&nb_pairs_kernel<LDSF, VEC>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes_for(kLdsMaxN)));
    hipLaunchKernelGGL((nb_pairs_kernel<LDSF, VEC>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, x, ldx, y, ldy, n, len, ncols,
                       run, xi, nxi, nrb, nunits, yi, ldyi, extrap, flag);
    MI_LAUNCH_CHECK(ctx, "interp1 pairs nearest kernel");
    count(LDSF ? 3 : 4);
    return MI_OK;
}

// the argument rules of the paired-column device call (who: the entry point's name)
mi_status check_args(const mi_ctx* ctx, const char* who, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                     const uint32_t* len, size_t ncols, const double* xi, size_t nxi, const double* yi, size_t ldyi,
                     const uint32_t* col_ok)
{
    MI_REQUIRE(ctx, x && y && xi && yi, "%s: NULL table/query/result pointer", who);
    const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xi) |
                         reinterpret_cast<uintptr_t>(yi);
    MI_REQUIRE(ctx, (al & 7u) == 0, "%s: x, y, xi, yi must be 8-byte aligned", who);
    const uintptr_t al4 = reinterpret_cast<uintptr_t>(len) | reinterpret_cast<uintptr_t>(col_ok);
    MI_REQUIRE(ctx, (al4 & 3u) == 0, "%s: len, col_ok must be 4-byte aligned", who);
    MI_REQUIRE(ctx, n >= 2, "%s: need at least two nodes per column (n=%zu)", who, n);
    MI_REQUIRE(ctx, n < 0x7ffffff0u, "%s: n=%zu exceeds 2^31 - 16", who, n);
    MI_REQUIRE(ctx, ldx >= n, "%s: ldx=%zu is smaller than n=%zu", who, ldx, n);
    MI_REQUIRE(ctx, ldy >= n, "%s: ldy=%zu is smaller than n=%zu", who, ldy, n);
    MI_REQUIRE(ctx, ldyi >= nxi, "%s: ldyi=%zu is smaller than nxi=%zu", who, ldyi, nxi);
    const size_t lim = SIZE_MAX / (2 * sizeof(double)) / ncols;
    MI_REQUIRE(ctx, ldx <= lim && ldy <= lim && ldyi <= lim && nxi <= lim,
               "%s: ncols=%zu x (ldx=%zu, ldy=%zu, ldyi=%zu) too large", who, ncols, ldx, ldy, ldyi);
    return MI_OK;
}

}  // namespace mi_nearest_batched

using namespace mi_nearest_batched;

extern "C" {

size_t mi_debug_nearest_batched_launches(int form)
{
    return (form >= 0 && form < 5) ? g_launches[form].load(std::memory_order_relaxed) : 0;
}

mi_status mi_interp1_rows_nearest_f64_dev(mi_ctx* ctx, const mi_axis1* ax, const double* y, size_t ldy, size_t m, const double* xi,
                                          size_t nxi, double* yi, size_t ldyi, double extrap)
{
    MI_REQUIRE(ctx, ctx && ax, "mi_interp1_rows_nearest_f64_dev: NULL context or axis");
    MI_REQUIRE(ctx, ax->device == ctx->device, "mi_interp1_rows_nearest_f64_dev: the axis lives on device %d, the context on device %d",
               ax->device, ctx->device);
    if (m == 0 || nxi == 0) return MI_OK;
    MI_REQUIRE(ctx, y && xi && yi, "mi_interp1_rows_nearest_f64_dev: NULL table/query/result pointer");
    const uintptr_t al = reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(yi);
    MI_REQUIRE(ctx, (al & 7u) == 0, "mi_interp1_rows_nearest_f64_dev: pointers must be 8-byte aligned");
    const size_t n = ax->n;
    MI_REQUIRE(ctx, ldy >= m, "mi_interp1_rows_nearest_f64_dev: ldy=%zu is smaller than m=%zu", ldy, m);
    MI_REQUIRE(ctx, ldyi >= m, "mi_interp1_rows_nearest_f64_dev: ldyi=%zu is smaller than m=%zu", ldyi, m);
    MI_REQUIRE(ctx, nxi <= SIZE_MAX / sizeof(int) && ldy <= SIZE_MAX / sizeof(double) / n && ldyi <= SIZE_MAX / sizeof(double) / nxi,
               "mi_interp1_rows_nearest_f64_dev: ldy=%zu x n=%zu or ldyi=%zu x nxi=%zu too large", ldy, n, ldyi, nxi);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    const mi_status st = mi::ensure_scratch(ctx, 3, nxi * sizeof(int));
    if (st != MI_OK) return st;
    int* idx = (int*)ctx->scratch[3];
    hipLaunchKernelGGL(nb_rows_locate_kernel, dim3(mi::stream_grid(ctx, nxi, kBlock)), dim3(kBlock), 0, ctx->stream, ax->a, xi, nxi, idx);
    MI_LAUNCH_CHECK(ctx, "interp1 rows nearest locate kernel");
    // units: row blocks x column runs, at most 4 per resident workgroup (8 per CU).  The columns are cut into runs only as
    // far as that needs and never below kMinRun columns (tile body: every run reads its first column anew) or about
    // kMinFlatUnit outputs (flat body): a small call leaves workgroups idle rather than reading Y several times
    const bool thin = m < kThinM;
    const size_t resident = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * 8;
    const size_t target = resident * 4;
    const size_t nrb = thin ? 1 : (m + kRowBlock - 1) / kRowBlock;
    const size_t min_run = thin ? (kMinFlatUnit + m - 1) / m : kMinRun;
    size_t want_runs = std::max<size_t>(1, std::min(target / nrb, (nxi + min_run - 1) / min_run));
    if (thin) want_runs = std::max(want_runs, (nxi + kMaxFlatRun - 1) / kMaxFlatRun);
    const size_t run = (nxi + want_runs - 1) / want_runs;
    const size_t nruns = (nxi + run - 1) / run;
    MI_REQUIRE(ctx, nrb <= SIZE_MAX / nruns, "mi_interp1_rows_nearest_f64_dev: m=%zu x nxi=%zu too large", m, nxi);
    const size_t nunits = nrb * nruns;
    const unsigned grid = (unsigned)std::min(nunits, resident);   // workgroups stride over the units beyond that
    int form;
    if (thin) {
        form = 2;
        hipLaunchKernelGGL(nb_rows_flat_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, idx, y, ldy, (uint32_t)m, nxi, run, nunits, yi,
                           ldyi, extrap);
    } else if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(yi)) & 15u) == 0 && ((ldy | ldyi) & 1) == 0) {
        form = 0;
        hipLaunchKernelGGL(nb_rows_tile_kernel<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, idx, y, ldy, m, nxi, run, nrb, nunits, yi,
                           ldyi, extrap);
    } else {
        form = 1;
        hipLaunchKernelGGL(nb_rows_tile_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, idx, y, ldy, m, nxi, run, nrb, nunits, yi,
                           ldyi, extrap);
    }
    MI_LAUNCH_CHECK(ctx, "interp1 rows nearest kernel");
    count(form);
    return MI_OK;
}

mi_status mi_interp1_pairs_nearest_f64_dev(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                           const uint32_t* len, size_t ncols, const double* xi, size_t nxi, double* yi, size_t ldyi,
                                           double extrap, uint32_t* col_ok)
{
    MI_REQUIRE(ctx, ctx, "mi_interp1_pairs_nearest_f64_dev: NULL context");
    if (ncols == 0 || nxi == 0) return MI_OK;
    mi_status st = check_args(ctx, "mi_interp1_pairs_nearest_f64_dev", x, ldx, y, ldy, n, len, ncols, xi, nxi, yi, ldyi, col_ok);
    if (st != MI_OK) return st;
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    // units: row blocks x column runs, about 16 workgroups of work per CU when the shape has that much
    const size_t nrb = (nxi + kPairRowBlock - 1) / kPairRowBlock;
    const size_t target = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * 16;
    const size_t want_runs = std::min(ncols, std::max<size_t>(1, (target + nrb - 1) / nrb));
    const size_t run = (ncols + want_runs - 1) / want_runs;
    const size_t nruns = (ncols + run - 1) / run;
    MI_REQUIRE(ctx, nrb <= SIZE_MAX / nruns, "mi_interp1_pairs_nearest_f64_dev: nxi=%zu x ncols=%zu too large", nxi, ncols);
    const size_t nunits = nrb * nruns;
    const unsigned grid = (unsigned)std::min(nunits, target);   // workgroups stride over the units beyond that
    const bool vec = (reinterpret_cast<uintptr_t>(yi) & 15u) == 0 && (ldyi & 1) == 0;
    if (n <= kLdsMaxN) {
        const size_t lds_bytes = lds_bytes_for(n);
        return vec ? launch_pairs<true, true>(ctx, grid, lds_bytes, x, ldx, y, ldy, (int)n, len, ncols, run, xi, nxi, nrb, nunits, yi, ldyi, extrap, col_ok)
                   : launch_pairs<true, false>(ctx, grid, lds_bytes, x, ldx, y, ldy, (int)n, len, ncols, run, xi, nxi, nrb, nunits, yi, ldyi, extrap, col_ok);
    }
    uint32_t* flag = col_ok;
    if (!flag) {
        st = mi::ensure_scratch(ctx, 3, ncols * sizeof(uint32_t));
        if (st != MI_OK) return st;
        flag = (uint32_t*)ctx->scratch[3];
    }
    hipLaunchKernelGGL(nb_pairs_validate_kernel, dim3(mi::stream_grid(ctx, ncols * kBlock, kBlock)), dim3(kBlock), 0, ctx->stream, x, ldx,
                       (int)n, len, ncols, flag);
    MI_LAUNCH_CHECK(ctx, "interp1 pairs nearest validation kernel");
    return vec ? launch_pairs<false, true>(ctx, grid, 0, x, ldx, y, ldy, (int)n, len, ncols, run, xi, nxi, nrb, nunits, yi, ldyi, extrap, flag)
               : launch_pairs<false, false>(ctx, grid, 0, x, ldx, y, ldy, (int)n, len, ncols, run, xi, nxi, nrb, nunits, yi, ldyi, extrap, flag);
}

}  // extern "C"
