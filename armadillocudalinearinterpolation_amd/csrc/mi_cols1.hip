// Batched interp1 over the columns of a matrix: one axis X (n nodes), Y column-major n x B (leading dimension ldy),
// queries XI (nxi, any order) -> YI column-major nxi x B (leading dimension ldyi),
//     YI[i + c*ldyi] == mi_interp1_f64_dev's result for XI[i] on the table (X, Y[:, c]),   bit for bit.
// MATLAB's interp1 with a matrix Y; in Armadillo terms the loop over the columns of an arma::mat that arma::interp1
// (vectors only) leaves to its caller.  X is taken as it is (Armadillo's "*linear" contract: strictly increasing and
// finite, else MI_ERR_GRID) -- sorting it would mean permuting the rows of every Y.
//
// The locate / weight code is mi_interp2_eval.hpp's (AxisDev, axis_locate, weight, axis_record), used as it is: the
// weight is interp1's  a > 0 ? a/(a+b) : 0, the blend below is interp1's (1-w)*Y[l] + w*Y[r], and this file is compiled
// with -ffp-contract=off like every other, so every product and sum rounds.
//
// Two launches on the context's stream:
//   locate   every XI[i] -> {w, l, r} record (AxRec), once per call, into context scratch slot 3.  The gridded
//            bilinear call (mi_interp2_grid_f64_dev) keeps its records in the same slot: both calls fill and read it
//            in stream order on the context's stream, so back-to-back calls of either kind do not disturb each other.
//   columns  one kernel, two forms, chosen from n alone; the work is cut into units = (row block of kRowBlock
//            consecutive outputs) x (run of consecutive columns), workgroups stride over the units, and a lane keeps
//            the records of its 2*kRecIter rows in registers across the run's columns.
//     LDS form (n <= kLdsMaxN, a column of at most 64 KiB): a column is read once, 16 B per lane and coalesced, into one
//            of two LDS buffers (one padding element holding Y[n-1], so that l+1 never leaves the buffer and equals
//            Y[r] at the last node); the loads of the next column are issued before the current column is blended
//            (the first kPrefetch*512 elements wait in registers, the rest of a longer column follows the blend);
//            one barrier per column.  Y[l], Y[l+1] come from LDS.
//     direct form (longer columns): Y[l], Y[r] are gathered from the column through L2.  Sorted XI makes neighbouring
//            lanes share lines; permuted XI is gather-bound.
//   YI is written with coalesced non-temporal stores: 16 B per lane (rows 2t, 2t+1) when yi is 16-B aligned and ldyi is
//   even, otherwise 8 B per lane (rows t, t+256: one contiguous 2-KiB run per workgroup each).
// Every index into y and yi is 64-bit; no grid dimension depends on B, n or nxi.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <vector>

#include "mi_interp2_eval.hpp"
#include "mi_axis1.hpp"

namespace mi_cols1 {

using mi_interp2::AxRec;
using mi_interp2::kBlock;

constexpr int kRecIter = 4;                          // 512-row slices per row block: 8 records per lane in registers
constexpr size_t kRowBlock = 2 * kBlock * kRecIter;  // 2048 outputs of one column per unit
constexpr size_t kLdsMaxN = 8192;                    // LDS form up to here: 2 x (n + 2) x 8 B <= 131104 B of the CU's 160 KiB
constexpr int kPrefetch = 4;                         // 16-B vectors per lane held in registers for the next column

typedef __attribute__((address_space(3))) double lds_double;

__global__ __launch_bounds__(kBlock) void cols1_locate_kernel(AxisDev ax, const double* __restrict__ xi, size_t nxi,
                                                              AxRec* __restrict__ rec)
{
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < nxi; k += (size_t)gridDim.x * kBlock)
        rec[k] = mi_interp2::axis_record(ax, xi[k]);
}

// A column on its way into LDS.  The 16-B vectors start at the column's first 16-B aligned element (h = 0 or 1
// elements in): vector k holds elements h + 2k, h + 2k + 1, k < nv = (n - h) / 2.  Elements 0 and n-1 are fetched by
// every lane (one line each, broadcast) and cover the head, an odd tail and the padding element.
struct ColLoad {
    d2 v[kPrefetch];
    double first, last;
    int h;
    int nv;
};

__device__ __forceinline__ void col_issue(ColLoad& L, const double* __restrict__ col, int n)
{
    L.h = (int)((reinterpret_cast<uintptr_t>(col) >> 3) & 1u);
    L.nv = (n - L.h) >> 1;
    const d2* p = reinterpret_cast<const d2*>(col + L.h);
#pragma unroll
    for (int k = 0; k < kPrefetch; ++k) {
        const int j = (int)threadIdx.x + k * kBlock;
        if (j < L.nv) L.v[k] = __builtin_nontemporal_load(p + j);
    }
    L.first = col[0];
    L.last = col[n - 1];
}

// buf: n + 1 elements (index n = padding = Y[n-1])
__device__ __forceinline__ void col_commit(const ColLoad& L, const double* __restrict__ col, int n, lds_double* buf)
{
#pragma unroll
    for (int k = 0; k < kPrefetch; ++k) {
        const int j = (int)threadIdx.x + k * kBlock;
        if (j < L.nv) {
            buf[L.h + 2 * j] = L.v[k].x;
            buf[L.h + 2 * j + 1] = L.v[k].y;
        }
    }
    const d2* p = reinterpret_cast<const d2*>(col + L.h);
    for (int j = (int)threadIdx.x + kPrefetch * kBlock; j < L.nv; j += kBlock) {   // the rest of a long column
        const d2 v = __builtin_nontemporal_load(p + j);
        buf[L.h + 2 * j] = v.x;
        buf[L.h + 2 * j + 1] = v.y;
    }
    if (threadIdx.x == 0) {
        buf[0] = L.first;
        buf[n - 1] = L.last;
        buf[n] = L.last;
    }
}

// LDSF: LDS form / direct form.  VEC: 16-B stores (yi 16-B aligned, ldyi even) / 8-B stores.
// unit u = (row block u % nrb, column run u / nrb): consecutive workgroups share a run's columns (L2) in the LDS form.
template <bool LDSF, bool VEC>
__global__ __launch_bounds__(kBlock) void cols1_kernel(const AxRec* __restrict__ rec, int n, const double* __restrict__ y,
                                                       size_t ldy, size_t ncols, size_t run, size_t nxi, size_t nrb,
                                                       size_t nunits, double* __restrict__ yi, size_t ldyi, double extrap)
{
    extern __shared__ double smem[];
    lds_double* const lds = (lds_double*)smem;
    const int stride = n + 2;                               // elements per LDS buffer (n + 1 used)
    const int t = (int)threadIdx.x;
    for (size_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const size_t rb = u % nrb, s = u / nrb;
        const size_t c0 = s * run, c1 = min(c0 + run, ncols);
        const size_t row0 = rb * kRowBlock;
        // this lane's rows, (ia, ib) + j*512 for j < kRecIter, and their records
        const size_t ia = row0 + (VEC ? 2 * t : t), ib = ia + (VEC ? 1 : kBlock);
        double wa[kRecIter], wb[kRecIter];
        int la[kRecIter], lb[kRecIter], ra[kRecIter], rb_[kRecIter];   // r = -3: no such row
#pragma unroll
        for (int j = 0; j < kRecIter; ++j) {
            const size_t o = (size_t)j * (2 * kBlock);
            AxRec A, B;
            A.w = 0.0; A.l = 0; A.r = -3;
            B = A;
            if (ia + o < nxi) A = rec[ia + o];
            if (ib + o < nxi) B = rec[ib + o];
            wa[j] = A.w; la[j] = A.l; ra[j] = A.r;
            wb[j] = B.w; lb[j] = B.l; rb_[j] = B.r;
        }
        ColLoad L;
        if constexpr (LDSF) {
            // (every column of the previous unit ended on a barrier: both buffers are free)
            const double* col = y + c0 * ldy;
            col_issue(L, col, n);
            col_commit(L, col, n, lds);
            __syncthreads();
        }
        for (size_t c = c0; c < c1; ++c) {
            lds_double* const cur = lds + (size_t)((c - c0) & 1) * stride;
            lds_double* const nxt = lds + (size_t)(((c - c0) & 1) ^ 1) * stride;
            const double* const col = y + c * ldy;
            const bool more = c + 1 < c1;
            if constexpr (LDSF) {
                if (more) col_issue(L, col + ldy, n);       // in flight while this column is blended
            }
            double* const out = yi + c * ldyi;
#pragma unroll
            for (int j = 0; j < kRecIter; ++j) {
                if (ra[j] == -3) continue;
                const bool hb = rb_[j] != -3;
                double* const oa = out + ia + (size_t)j * (2 * kBlock);
                double a0, a1, b0, b1;
                if constexpr (LDSF) {
                    a0 = cur[la[j]];
                    a1 = cur[la[j] + 1];
                    b0 = cur[lb[j]];
                    b1 = cur[lb[j] + 1];
                } else {
                    a0 = col[la[j]];
                    a1 = col[max(ra[j], 0)];
                    b0 = col[lb[j]];
                    b1 = col[max(rb_[j], 0)];
                }
                double va = (1.0 - wa[j]) * a0 + wa[j] * a1;
                double vb = (1.0 - wb[j]) * b0 + wb[j] * b1;
                if (ra[j] < 0) va = (ra[j] == -2) ? __builtin_nan("") : extrap;
                if (rb_[j] < 0) vb = (rb_[j] == -2) ? __builtin_nan("") : extrap;
                if (VEC && hb) {
                    d2 o;
                    o.x = va;
                    o.y = vb;
                    __builtin_nontemporal_store(o, reinterpret_cast<d2*>(oa));
                } else {
                    __builtin_nontemporal_store(va, oa);
                    if (hb) __builtin_nontemporal_store(vb, oa + (ib - ia));
                }
            }
            if constexpr (LDSF) {
                if (more) col_commit(L, col + ldy, n, nxt);
                __syncthreads();
            }
        }
    }
}

mi_status fill_explicit(mi_ctx* ctx, const std::vector<double>& xs, void** dev, AxisDev* a)
{
    const size_t n = xs.size();
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(xs[i])) return mi::fail(ctx, MI_ERR_GRID, "mi_axis1_create: X[%zu] is not finite", i);
    for (size_t i = 1; i < n; ++i)
        if (!(xs[i - 1] < xs[i]))
            return mi::fail(ctx, MI_ERR_GRID, "mi_axis1_create: X not strictly increasing at %zu (X is not sorted for the caller)", i);
    memset(a, 0, sizeof(*a));
    a->n = (int)n;
    a->xmin = xs[0];
    a->xmax = xs[n - 1];
    // analytic guess + bounded walk where the guess stays within kMaxWalk nodes of every node, else binary search:
    // a matter of time only, axis_locate returns the largest l with X[l] <= q either way
    const double scale = (double)(n - 1) / (a->xmax - a->xmin);
    const bool ok = std::isfinite(scale) && scale > 0.0;
    long e_lo = 0, e_hi = 0;
    if (ok) {
        for (size_t i = 0; i < n; ++i) {
            long gi = (long)(int)((xs[i] - a->xmin) * scale);
            gi = std::min<long>(std::max<long>(gi, 0), (long)n - 1);
            e_lo = std::min(e_lo, gi - (long)i);
            e_hi = std::max(e_hi, gi - (long)i);
        }
    }
    a->use_guess = ok && (e_hi - e_lo + 1) <= mi_interp2::kMaxWalk;
    a->scale = ok ? scale : 0.0;
    const hipError_t e = hipMalloc(dev, n * sizeof(double));
    if (e != hipSuccess) return mi::fail(ctx, MI_ERR_NOMEM, "mi_axis1_create: hipMalloc failed: %s", hipGetErrorString(e));
    MI_HIP(ctx, hipMemcpy(*dev, xs.data(), n * sizeof(double), hipMemcpyHostToDevice));
    a->nodes = (const double*)*dev;
    return MI_OK;
}

// ncols columns of `rows` doubles between a compact device buffer and a host matrix with leading dimension ld
hipError_t copy_cols(double* dst, size_t ld_dst, const double* src, size_t ld_src, size_t rows, size_t ncols, hipMemcpyKind kind,
                     hipStream_t stream)
{
    if (ld_dst == rows && ld_src == rows) return hipMemcpyAsync(dst, src, rows * ncols * sizeof(double), kind, stream);
    return hipMemcpy2DAsync(dst, ld_dst * sizeof(double), src, ld_src * sizeof(double), rows * sizeof(double), ncols, kind, stream);
}

template <bool LDSF, bool VEC>
mi_status launch(mi_ctx* ctx, unsigned grid, size_t lds_bytes, const AxRec* rec, int n, const double* y, size_t ldy,
                 size_t ncols, size_t run, size_t nxi, size_t nrb, size_t nunits, double* yi, size_t ldyi, double extrap)
{
    if (lds_bytes > 64 * 1024)   // above the default limit of dynamic LDS (per device: asked for at every such launch)
        MI_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&cols1_kernel<LDSF, VEC>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)((kLdsMaxN + 2) * 2 * sizeof(double))));
    hipLaunchKernelGGL((cols1_kernel<LDSF, VEC>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, rec, n, y, ldy, ncols, run,
                       nxi, nrb, nunits, yi, ldyi, extrap);
    MI_LAUNCH_CHECK(ctx, "interp1 cols kernel");
    return MI_OK;
}

}  // namespace mi_cols1

using namespace mi_cols1;

extern "C" {

mi_status mi_axis1_create(mi_ctx* ctx, const double* x, size_t n, unsigned flags, mi_axis1** out)
{
    MI_REQUIRE(ctx, ctx && x && out, "mi_axis1_create: NULL argument");
    MI_REQUIRE(ctx, (flags & ~MI_GRID_DEVICE_PTRS) == 0, "mi_axis1_create: unknown flags 0x%x", flags);
    *out = nullptr;
    if (n < 2) return mi::fail(ctx, MI_ERR_GRID, "mi_axis1_create: need at least two nodes (n=%zu)", n);
    MI_REQUIRE(ctx, n < 0x7ffffff0u, "mi_axis1_create: n=%zu exceeds 2^31", n);
    MI_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> xs(n);
    if (flags & MI_GRID_DEVICE_PTRS) {
        MI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        MI_HIP(ctx, hipMemcpy(xs.data(), x, n * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        memcpy(xs.data(), x, n * sizeof(double));
    }
    mi_axis1* ax = new (std::nothrow) mi_axis1();
    if (!ax) return mi::fail(ctx, MI_ERR_NOMEM, "mi_axis1_create: out of host memory");
    ax->ctx = ctx;
    ax->device = ctx->device;
    ax->dev_x = nullptr;
    ax->n = n;
    const mi_status st = fill_explicit(ctx, xs, &ax->dev_x, &ax->a);
    if (st != MI_OK) {
        mi_axis1_destroy(ax);
        return st;
    }
    *out = ax;
    return MI_OK;
}

mi_status mi_axis1_create_uniform(mi_ctx* ctx, double x0, double dx, size_t n, mi_axis1** out)
{
    MI_REQUIRE(ctx, ctx && out, "mi_axis1_create_uniform: NULL argument");
    *out = nullptr;
    if (n < 2) return mi::fail(ctx, MI_ERR_GRID, "mi_axis1_create_uniform: need at least two nodes (n=%zu)", n);
    MI_REQUIRE(ctx, n < 0x7ffffff0u, "mi_axis1_create_uniform: n=%zu exceeds 2^31", n);
    if (!(dx > 0.0) || !std::isfinite(dx) || !std::isfinite(x0) || !std::isfinite(std::fma((double)(n - 1), dx, x0)))
        return mi::fail(ctx, MI_ERR_GRID, "mi_axis1_create_uniform: need finite x0 and dx > 0");
    if (!(std::fma(1.0, dx, x0) > x0))
        return mi::fail(ctx, MI_ERR_GRID, "mi_axis1_create_uniform: dx too small relative to x0");
    mi_axis1* ax = new (std::nothrow) mi_axis1();
    if (!ax) return mi::fail(ctx, MI_ERR_NOMEM, "mi_axis1_create_uniform: out of host memory");
    ax->ctx = ctx;
    ax->device = ctx->device;
    ax->dev_x = nullptr;
    ax->n = n;
    AxisDev& a = ax->a;
    memset(&a, 0, sizeof(a));
    a.n = (int)n;
    a.x0 = x0;
    a.dx = dx;
    a.xmin = x0;
    a.xmax = std::fma((double)(n - 1), dx, x0);
    a.scale = 1.0 / dx;
    *out = ax;
    return MI_OK;
}

mi_status mi_axis1_destroy(mi_axis1* ax)
{
    if (!ax) return MI_OK;
    (void)hipSetDevice(ax->device);
    if (ax->dev_x) (void)hipFree(ax->dev_x);
    delete ax;
    return MI_OK;
}

mi_status mi_interp1_cols_f64_dev(mi_ctx* ctx, const mi_axis1* ax, const double* y, size_t ldy, size_t ncols, const double* xi,
                                  size_t nxi, double* yi, size_t ldyi, double extrap)
{
    MI_REQUIRE(ctx, ctx && ax, "mi_interp1_cols_f64_dev: NULL context or axis");
    MI_REQUIRE(ctx, ax->device == ctx->device, "mi_interp1_cols_f64_dev: the axis lives on device %d, the context on device %d",
               ax->device, ctx->device);
    if (ncols == 0 || nxi == 0) return MI_OK;
    MI_REQUIRE(ctx, y && xi && yi, "mi_interp1_cols_f64_dev: NULL table/query/result pointer");
    const uintptr_t al = reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(yi);
    MI_REQUIRE(ctx, (al & 7u) == 0, "mi_interp1_cols_f64_dev: pointers must be 8-byte aligned");
    const size_t n = ax->n;
    MI_REQUIRE(ctx, ldy >= n, "mi_interp1_cols_f64_dev: ldy=%zu is smaller than the axis (n=%zu)", ldy, n);
    MI_REQUIRE(ctx, ldyi >= nxi, "mi_interp1_cols_f64_dev: ldyi=%zu is smaller than nxi=%zu", ldyi, nxi);
    MI_REQUIRE(ctx, nxi <= SIZE_MAX / sizeof(AxRec) && ldy <= SIZE_MAX / sizeof(double) / ncols && ldyi <= SIZE_MAX / sizeof(double) / ncols,
               "mi_interp1_cols_f64_dev: ncols=%zu x (ldy=%zu, ldyi=%zu) too large", ncols, ldy, ldyi);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    const mi_status st = mi::ensure_scratch(ctx, 3, nxi * sizeof(AxRec));
    if (st != MI_OK) return st;
    AxRec* rec = (AxRec*)ctx->scratch[3];
    hipLaunchKernelGGL(cols1_locate_kernel, dim3(mi::stream_grid(ctx, nxi, kBlock)), dim3(kBlock), 0, ctx->stream, ax->a, xi, nxi, rec);
    MI_LAUNCH_CHECK(ctx, "interp1 cols locate kernel");
    // units: row blocks x column runs, about 16 workgroups of work per CU when the shape has that much
    const size_t nrb = (nxi + kRowBlock - 1) / kRowBlock;
    const size_t target = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * 16;
    const size_t want_runs = std::min(ncols, std::max<size_t>(1, (target + nrb - 1) / nrb));
    const size_t run = (ncols + want_runs - 1) / want_runs;
    const size_t nruns = (ncols + run - 1) / run;
    MI_REQUIRE(ctx, nrb <= SIZE_MAX / nruns, "mi_interp1_cols_f64_dev: nxi=%zu x ncols=%zu too large", nxi, ncols);
    const size_t nunits = nrb * nruns;
    const unsigned grid = (unsigned)std::min(nunits, target);   // workgroups stride over the units beyond that
    const bool vec = (reinterpret_cast<uintptr_t>(yi) & 15u) == 0 && (ldyi & 1) == 0;
    if (n <= kLdsMaxN) {
        const size_t lds_bytes = 2 * (n + 2) * sizeof(double);
        return vec ? launch<true, true>(ctx, grid, lds_bytes, rec, (int)n, y, ldy, ncols, run, nxi, nrb, nunits, yi, ldyi, extrap)
                   : launch<true, false>(ctx, grid, lds_bytes, rec, (int)n, y, ldy, ncols, run, nxi, nrb, nunits, yi, ldyi, extrap);
    }
    return vec ? launch<false, true>(ctx, grid, 0, rec, (int)n, y, ldy, ncols, run, nxi, nrb, nunits, yi, ldyi, extrap)
               : launch<false, false>(ctx, grid, 0, rec, (int)n, y, ldy, ncols, run, nxi, nrb, nunits, yi, ldyi, extrap);
}

mi_status mi_interp1_cols_f64_host(mi_ctx* ctx, const mi_axis1* ax, const double* y, size_t ldy, size_t ncols, const double* xi,
                                   size_t nxi, double* yi, size_t ldyi, double extrap)
{
    MI_REQUIRE(ctx, ctx && ax, "mi_interp1_cols_f64_host: NULL context or axis");
    if (ncols == 0 || nxi == 0) return MI_OK;
    MI_REQUIRE(ctx, y && xi && yi, "mi_interp1_cols_f64_host: NULL table/query/result pointer");
    const size_t n = ax->n;
    MI_REQUIRE(ctx, ldy >= n, "mi_interp1_cols_f64_host: ldy=%zu is smaller than the axis (n=%zu)", ldy, n);
    MI_REQUIRE(ctx, ldyi >= nxi, "mi_interp1_cols_f64_host: ldyi=%zu is smaller than nxi=%zu", ldyi, nxi);
    MI_REQUIRE(ctx, ldy <= SIZE_MAX / sizeof(double) / ncols && ldyi <= SIZE_MAX / sizeof(double) / ncols,
               "mi_interp1_cols_f64_host: ncols=%zu x (ldy=%zu, ldyi=%zu) too large", ncols, ldy, ldyi);
    MI_HIP(ctx, hipSetDevice(ctx->device));
    // device copies are compact (leading dimensions n and nxi): slot 0 XI, slot 1 Y, slot 2 YI
    mi_status st = mi::ensure_scratch(ctx, 0, nxi * sizeof(double));
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 1, n * ncols * sizeof(double));
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 2, nxi * ncols * sizeof(double));
    if (st != MI_OK) return st;
    double *dxi = (double*)ctx->scratch[0], *dy = (double*)ctx->scratch[1], *dyi = (double*)ctx->scratch[2];
    const size_t chunk = (size_t)8 << 20;   // elements, as the 8 M-query chunks of mi_interp1_f64_host
    const size_t per_col = std::max(n, nxi);
    if (per_col <= 2 * chunk / ncols) {
        MI_HIP(ctx, hipMemcpyAsync(dxi, xi, nxi * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        MI_HIP(ctx, copy_cols(dy, n, y, ldy, n, ncols, hipMemcpyHostToDevice, ctx->stream));
        st = mi_interp1_cols_f64_dev(ctx, ax, dy, n, ncols, dxi, nxi, dyi, nxi, extrap);
        if (st != MI_OK) return st;
        MI_HIP(ctx, copy_cols(yi, ldyi, dyi, nxi, nxi, ncols, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return MI_OK;
    }
    // column chunks of about `chunk` elements, pinned like mi_interp1_f64_host: the copy back of chunk k (on the aux
    // stream) overlaps the upload and the kernels of chunk k+1
    st = mi::ensure_aux_stream(ctx);
    if (st != MI_OK) return st;
    const size_t y_bytes = ((ncols - 1) * ldy + n) * sizeof(double), yi_bytes = ((ncols - 1) * ldyi + nxi) * sizeof(double);
    const bool pin_x = mi::pin_host(xi, nxi * sizeof(double)), pin_y = mi::pin_host(y, y_bytes), pin_o = mi::pin_host(yi, yi_bytes);
    // as in mi_interp1_f64_host: no early return before both streams are drained and the ranges released
    hipError_t herr = hipMemcpyAsync(dxi, xi, nxi * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    const char* what = "upload of the queries";
    const size_t cols = std::max<size_t>(1, chunk / per_col);
    const bool fail_hook = getenv("MI_TEST_FAIL_COLS_CHUNK") != nullptr;
    for (size_t c0 = 0; c0 < ncols && herr == hipSuccess && st == MI_OK; c0 += cols) {
        const size_t m = std::min(cols, ncols - c0);
        if (fail_hook && c0 > 0) { herr = hipErrorUnknown; what = "MI_TEST_FAIL_COLS_CHUNK (error-path test hook)"; break; }
        herr = copy_cols(dy + c0 * n, n, y + c0 * ldy, ldy, n, m, hipMemcpyHostToDevice, ctx->stream);
        if (herr != hipSuccess) { what = "upload of a column chunk"; break; }
        st = mi_interp1_cols_f64_dev(ctx, ax, dy + c0 * n, n, m, dxi, nxi, dyi + c0 * nxi, nxi, extrap);
        if (st != MI_OK) break;
        herr = hipEventRecord(ctx->aux_event, ctx->stream);
        if (herr == hipSuccess) herr = hipStreamWaitEvent(ctx->aux_stream, ctx->aux_event, 0);
        if (herr == hipSuccess)
            herr = copy_cols(yi + c0 * ldyi, ldyi, dyi + c0 * nxi, nxi, nxi, m, hipMemcpyDeviceToHost, ctx->aux_stream);
        if (herr != hipSuccess) what = "download of a result chunk";
    }
    const hipError_t e1 = hipStreamSynchronize(ctx->stream), e2 = hipStreamSynchronize(ctx->aux_stream);
    if (pin_x) mi::unpin_host(xi);
    if (pin_y) mi::unpin_host(y);
    if (pin_o) mi::unpin_host(yi);
    if (st != MI_OK) return st;
    if (herr != hipSuccess) return mi::fail(ctx, MI_ERR_HIP, "mi_interp1_cols_f64_host: %s failed: %s", what, hipGetErrorString(herr));
    MI_HIP(ctx, e1);
    MI_HIP(ctx, e2);
    return MI_OK;
}

}  // extern "C"
