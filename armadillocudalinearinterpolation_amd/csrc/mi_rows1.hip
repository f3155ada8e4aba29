// Batched interp1 along the rows of a matrix: one axis X (n nodes), Y column-major m x n (leading dimension ldy), one table
// per ROW, queries XI (nxi, any order) -> YI column-major m x nxi (leading dimension ldyi),
//     YI[r + i*ldyi] == mi_interp1_f64_dev's result for XI[i] on the table (X, Y(r, :)),   bit for bit.
// An ensemble stored realisation-fastest ([time level][realisation]), or interpolation across the slices of a cube
// (m = ny * nx rows, one column per slice).  The bracket and the weight of a query are the same for every row, and a
// column of Y is a contiguous stream: an output column is a blend of two input columns, element by element.
//
// The locate / weight code is mi_interp2_eval.hpp's (AxisDev, axis_record, AxRec), used as it is; the blend below is
// interp1's (1-w)*Y[l] + w*Y[r], and this file is compiled with -ffp-contract=off like every other, so every product and
// sum rounds.
//
// Two launches on the context's stream:
//   locate  every XI[i] -> {w, l, r} record, once per call, into context scratch slot 3 (shared in stream order with the
//           other record users: mi_interp2_grid_f64_dev, mi_interp1_cols_f64_dev, mi_interp2_slices_f64_dev and the
//           long-column forms of the paired-column calls).
//   rows    the work is cut into units = (block of kRowBlock consecutive rows) x (run of consecutive output columns);
//           workgroups of 256 lanes stride over the units.  The record of an output column is the same for the whole
//           workgroup and is read once per column on the uniform path.
//     tile body (m >= kThinM): a lane owns kLaneRows rows of the block (16-B form, y and yi 16-B aligned and ldy, ldyi
//           even: rows 2t, 2t+1, 512+2t, 513+2t; 8-B form: rows t + 256 j), so a column access of the workgroup is 8 KiB.
//           The lane keeps the values of the two bracketing columns hl, hr in registers.  For the next output column a
//           flagged record stores NaN / extrap and leaves the cache alone; l == hl loads nothing; l == hr moves the right
//           column over and loads one column; anything else loads both; at the last node (l == r) the right value is the
//           left value.  The branches are uniform: with sorted XI every column of Y a query brackets is read once per row
//           block and run, and columns no query brackets are never read.  The loads of the NEXT bracket (found by looking
//           ahead in the records) are issued before the current output is blended and stay in registers until the
//           output that needs them: a workgroup has up to two columns (16 KiB) in flight while it blends and stores.
//     flat body (m < kThinM, where the tile body would leave most lanes idle): a flat index over the run's m x columns
//           outputs, 512 per step, column and row recovered without a division in the loop; the record is taken per
//           output; two 8-B loads, the blend, one 8-B store.
//   YI is written with non-temporal stores.
// Every index into y and yi is 64-bit; no grid dimension depends on m, n or nxi.
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "mi_interp2_eval.hpp"
#include "mi_axis1.hpp"

namespace mi_rows1 {

using mi_interp2::AxRec;
using mi_interp2::kBlock;

constexpr int kLaneRows = 4;                         // rows of a block per lane (tile body)
constexpr size_t kRowBlock = 1024;                   // = kLaneRows * kBlock rows per unit of the tile body: 8 KiB of a column
constexpr size_t kThinM = kBlock;                    // m below: flat body
constexpr int kFlatStep = 2 * kBlock;                // outputs per step of the flat body
constexpr size_t kMaxFlatRun = (size_t)1 << 23;      // columns per run of the flat body: run * m stays below 2^31
constexpr size_t kMinRun = 16;                       // output columns per run of the tile body, at least (but for the last run)
constexpr size_t kMinFlatUnit = 4 * kFlatStep;       // outputs per run of the flat body, about as many at least
static_assert(kRowBlock == (size_t)kLaneRows * kBlock, "a lane owns kLaneRows rows of a block");

// process-wide call counts by form (mi_debug_rows1_launches): 0 tile body 16-B, 1 tile body 8-B, 2 flat body
std::atomic<size_t> g_launches[3];

__global__ __launch_bounds__(kBlock) void rows1_locate_kernel(AxisDev ax, const double* __restrict__ xi, size_t nxi,
                                                              AxRec* __restrict__ rec)
{
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < nxi; k += (size_t)gridDim.x * kBlock)
        rec[k] = mi_interp2::axis_record(ax, xi[k]);
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

typedef __attribute__((address_space(4))) AxRec const_rec;

// the first output column j in [j, c1) whose record is not flagged and whose bracket starts at another column than hl;
// its bracket in (nl, nr).  c1 when there is none.  Uniform: every lane walks the same records.
__device__ __forceinline__ size_t next_bracket(const AxRec* __restrict__ rec, size_t j, size_t c1, int hl, int& nl, int& nr)
{
    // read through the constant address space (the records were written by the locate kernel, before this one began):
    // that keeps the walk on the scalar path, where it waits for nothing but its own loads -- as a vector load it would
    // wait for every store and every column in flight
    const const_rec* const crec = (const const_rec*)rec;
    for (; j < c1; ++j) {
        const int l = crec[j].l, r = crec[j].r;
        if (r >= 0 && l != hl) {
            nl = l;
            nr = r;
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
__device__ __forceinline__ void tile_unit(const AxRec* __restrict__ rec, const double* __restrict__ yb, size_t ldy, size_t c0,
                                          size_t c1, double* __restrict__ ob, size_t ldyi, double extrap, int t, int rows)
{
    // a, b: columns hl, hr of Y, this lane's rows; pa, pb: columns nl, nr on their way, wanted at output column jn
    double a[kLaneRows], b[kLaneRows], pa[kLaneRows], pb[kLaneRows];
#pragma unroll
    for (int k = 0; k < kLaneRows; ++k) a[k] = b[k] = pa[k] = pb[k] = 0.0;
    int hl = -1, hr = -1, nl = -1, nr = -1;
    size_t jn = next_bracket(rec, c0, c1, hl, nl, nr);
    if (jn < c1) {
        col_load<VEC, FULL>(pa, yb + (size_t)nl * ldy, t, rows);
        if (nr != nl) col_load<VEC, FULL>(pb, yb + (size_t)nr * ldy, t, rows);
    }
    size_t i = c0;
    for (;;) {
        // the outputs of the bracket held: no load in here, the next bracket's columns stay in flight
        for (; i < jn; ++i) {
            if constexpr (!FULL) asm volatile("" : "+v"(rows));
            const AxRec R = rec[i];                          // uniform; flagged, or l == hl
            double v[kLaneRows];
            const double f = (R.r == -2) ? __builtin_nan("") : extrap;
#pragma unroll
            for (int k = 0; k < kLaneRows; ++k) {
                const double e = (1.0 - R.w) * a[k] + R.w * b[k];
                v[k] = (R.r < 0) ? f : e;
            }
            col_store<VEC, FULL>(v, ob + i * ldyi, t, rows);
        }
        if (i >= c1) break;
        if constexpr (!FULL) asm volatile("" : "+v"(rows));
        // output column i starts another bracket: the columns on their way become the ones held
#pragma unroll
        for (int k = 0; k < kLaneRows; ++k) a[k] = (nl == hr) ? b[k] : pa[k];
#pragma unroll
        for (int k = 0; k < kLaneRows; ++k) b[k] = (nr == nl) ? a[k] : pb[k];
        hl = nl;
        hr = nr;
        // and the bracket after it is looked up in the records and requested before anything of this one is blended
        jn = next_bracket(rec, i + 1, c1, hl, nl, nr);
        if (jn < c1) {
            if (nl != hr) col_load<VEC, FULL>(pa, yb + (size_t)nl * ldy, t, rows);
            if (nr != nl) col_load<VEC, FULL>(pb, yb + (size_t)nr * ldy, t, rows);
        }
    }
}

// Tile body.  VEC: 16-B accesses (y, yi 16-B aligned, ldy, ldyi even) / 8-B accesses.
// unit u = (row block u % nrb, column run u / nrb): consecutive workgroups take neighbouring row blocks of the same columns.
template <bool VEC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(VEC ? 8 : 6, 8))) void rows1_tile_kernel(const AxRec* __restrict__ rec, const double* __restrict__ y, size_t ldy,
                                                            size_t m, size_t nxi, size_t run, size_t nrb, size_t nunits,
                                                            double* __restrict__ yi, size_t ldyi, double extrap)
{
    const int t = (int)threadIdx.x;
    for (size_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const size_t s = u / nrb, rb = u - s * nrb;
        const size_t c0 = s * run, c1 = min(c0 + run, nxi);
        const size_t row0 = rb * kRowBlock;
        const int rows = (int)min(kRowBlock, m - row0);
        if (rows == (int)kRowBlock) tile_unit<VEC, true>(rec, y + row0, ldy, c0, c1, yi + row0, ldyi, extrap, t, rows);
        else tile_unit<VEC, false>(rec, y + row0, ldy, c0, c1, yi + row0, ldyi, extrap, t, rows);
    }
}

// Flat body: unit u = run u of output columns, all m rows.
__global__ __launch_bounds__(kBlock) void rows1_flat_kernel(const AxRec* __restrict__ rec, const double* __restrict__ y, size_t ldy,
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
                    const AxRec R = rec[i];
                    double v = (R.r == -2) ? __builtin_nan("") : extrap;
                    if (R.r >= 0) {
                        const double a = y[(size_t)R.l * ldy + r], b = y[(size_t)R.r * ldy + r];
                        v = (1.0 - R.w) * a + R.w * b;
                    }
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

}  // namespace mi_rows1

using namespace mi_rows1;

extern "C" {

size_t mi_debug_rows1_launches(int form)
{
    return (form >= 0 && form < 3) ? g_launches[form].load(std::memory_order_relaxed) : 0;
}

mi_status mi_interp1_rows_f64_dev(mi_ctx* ctx, const mi_axis1* ax, const double* y, size_t ldy, size_t m, const double* xi,
                                  size_t nxi, double* yi, size_t ldyi, double extrap)
{
    MI_REQUIRE(ctx, ctx && ax, "mi_interp1_rows_f64_dev: NULL context or axis");
    MI_REQUIRE(ctx, ax->device == ctx->device, "mi_interp1_rows_f64_dev: the axis lives on device %d, the context on device %d",
               ax->device, ctx->device);
    if (m == 0 || nxi == 0) return MI_OK;
    MI_REQUIRE(ctx, y && xi && yi, "mi_interp1_rows_f64_dev: NULL table/query/result pointer");
    const uintptr_t al = reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(yi);
    MI_REQUIRE(ctx, (al & 7u) == 0, "mi_interp1_rows_f64_dev: pointers must be 8-byte aligned");
    const size_t n = ax->n;
    MI_REQUIRE(ctx, ldy >= m, "mi_interp1_rows_f64_dev: ldy=%zu is smaller than m=%zu", ldy, m);
    MI_REQUIRE(ctx, ldyi >= m, "mi_interp1_rows_f64_dev: ldyi=%zu is smaller than m=%zu", ldyi, m);
    MI_REQUIRE(ctx, nxi <= SIZE_MAX / sizeof(AxRec) && ldy <= SIZE_MAX / sizeof(double) / n && ldyi <= SIZE_MAX / sizeof(double) / nxi,
               "mi_interp1_rows_f64_dev: ldy=%zu x n=%zu or ldyi=%zu x nxi=%zu too large", ldy, n, ldyi, nxi);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    const mi_status st = mi::ensure_scratch(ctx, 3, nxi * sizeof(AxRec));
    if (st != MI_OK) return st;
    AxRec* rec = (AxRec*)ctx->scratch[3];
    hipLaunchKernelGGL(rows1_locate_kernel, dim3(mi::stream_grid(ctx, nxi, kBlock)), dim3(kBlock), 0, ctx->stream, ax->a, xi, nxi, rec);
    MI_LAUNCH_CHECK(ctx, "interp1 rows locate kernel");
    // units: row blocks x column runs, at most 4 per resident workgroup (8 per CU).  The columns are cut into runs only as
    // far as that needs and never below kMinRun columns (tile body: every run reads its first bracket anew) or about
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
    MI_REQUIRE(ctx, nrb <= SIZE_MAX / nruns, "mi_interp1_rows_f64_dev: m=%zu x nxi=%zu too large", m, nxi);
    const size_t nunits = nrb * nruns;
    const unsigned grid = (unsigned)std::min(nunits, resident);   // workgroups stride over the units beyond that
    int form;
    if (thin) {
        form = 2;
        hipLaunchKernelGGL(rows1_flat_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, rec, y, ldy, (uint32_t)m, nxi, run, nunits, yi,
                           ldyi, extrap);
    } else if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(yi)) & 15u) == 0 && ((ldy | ldyi) & 1) == 0) {
        form = 0;
        hipLaunchKernelGGL(rows1_tile_kernel<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, rec, y, ldy, m, nxi, run, nrb, nunits, yi,
                           ldyi, extrap);
    } else {
        form = 1;
        hipLaunchKernelGGL(rows1_tile_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, rec, y, ldy, m, nxi, run, nrb, nunits, yi,
                           ldyi, extrap);
    }
    MI_LAUNCH_CHECK(ctx, "interp1 rows kernel");
    g_launches[form].fetch_add(1, std::memory_order_relaxed);
    return MI_OK;
}

}  // extern "C"
