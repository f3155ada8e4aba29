// interp1 over paired columns with a query vector per column: X, Y column-major n x B as in mi_pairs1.hip (leading
// dimensions ldx, ldy, optional fill counts len), XI column-major nxi x B (leading dimension ldxi >= nxi) -> YI
// column-major nxi x B,
//     YI[i + c*ldyi] == mi_interp1_f64_dev's result for XI[i + c*ldxi] on the table (X[0:len[c], c], Y[0:len[c], c]),
// bit for bit.  ldxi == 0: one XI vector for every column (mi_interp1_pairs_f64_dev's contract and bits).
// Inverse-CDF sampling from B distributions, every trajectory resampled onto a mesh of its own, Restrict with a horizon
// per realisation.  Validation, bad columns, col_ok and the blend are mi_pairs1.hip's, word for word; this file is
// compiled with -ffp-contract=off like every other.
//
// Three forms, chosen by the dispatcher from n, nxi and ldxi alone:
//   thin form   (n <= kThinMaxN and nxi <= kThinMaxQ, any ldxi): one lane per column, one workgroup per block of kBlock
//               consecutive columns, workgroups stride over the blocks.  A lane walks down its column once, 16 B at a
//               time where x, y are 16-B aligned and ldx, ldy even (compact two-node columns: one 16-B load each, the
//               block's 4 KiB contiguous), and keeps per query the running bracket: the last node <= q and the node
//               behind it.  That is a branch-free count of the nodes <= q whose trip count depends on n alone -- no
//               register array is indexed, nothing goes through LDS, there is no barrier.  The chain
//               -inf < X[0] < ... < X[len-1] < +inf is checked on the way.
//   LDS form    (n <= kLdsMaxN, ldxi > 0, not thin): mi_pairs1.hip's unit structure -- (row block) x (run of columns),
//               double-buffered staging of X and Y with the validation on the way into LDS, branch-free binary search,
//               non-temporal stores -- but a lane's 2*kQIter queries are reloaded for every column, and the loads of
//               the next column's queries are issued with the loads of its X and Y.  X is always staged skewed:
//               per-column queries are unordered in the expected use, and a layout chosen per unit would have to be
//               chosen per column here.  Results never depend on the layout.
//   direct form (n > kLdsMaxN, ldxi > 0): the validation pass (flags into col_ok or context scratch slot 3), then the
//               column kernel on the column itself, reading its queries from xi + c*ldxi.
// ldxi == 0 and not thin is mi_interp1_pairs_f64_dev's own case and is forwarded to it.
// The LDS layout and the staging helpers (ColLoad, col_issue, col_commit, col_len, search, skew) are mi_paired_cols.hpp's,
// shared with mi_pairs1.hip; the blend, the validation pass and the host side are still copies of that file's.
// Every index into x, y, xi and yi is 64-bit; no grid dimension depends on B, n or nxi.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "mi_interp2_eval.hpp"
#include "mi_paired_cols.hpp"

namespace mi_each1 {

using mi_interp2::kBlock;
using namespace mi_paired;

// The thin form's limits.  kThinMaxQ is the number of per-query register sets of the widest thin kernel (123 VGPRs, four
// waves per SIMD).  Measured (scripts/gpu_interp1_each_timing.py): at n = 32, nxi = 8 the thin form is
// still 4.5 x faster than the LDS form (113 x at n = 2, nxi = 1); the crossover above 32 nodes is not located.
constexpr size_t kThinMaxN = 32;
constexpr size_t kThinMaxQ = 8;

constexpr size_t kRowBlock = 2 * kBlock * kQIter;    // 2048 outputs of one column per unit
constexpr size_t kLdsMaxN = 4096;                    // LDS form up to here (mi_pairs1.hip's limit and LDS budget: 133248 B)

// process-wide launch counts by form (mi_debug_each_launches): 0 thin, 1 LDS, 2 direct, 3 forwarded
std::atomic<size_t> g_launches[4];

// the blend and the range rule of interp1 on one located bracket
__device__ __forceinline__ double finish(double xl, double xr, double yl, double yr, double q, double x0, double x1, double extrap)
{
    const double w = mi_interp2::weight(xl, xr, q);
    double v = (1.0 - w) * yl + w * yr;
    if (!(q >= x0 && q <= x1)) v = (q != q) ? __builtin_nan("") : extrap;
    return v;
}

template <bool LDSF, typename XP, typename YP>
__device__ __forceinline__ double blend(XP X, YP Y, int nc, int l, double q, double x0, double x1, double extrap)
{
    const int r = LDSF ? l + 1 : min(l + 1, nc - 1);       // LDS form: the padding element at nc holds the last node
    return finish(X[l], X[r], Y[l], Y[r], q, x0, x1, extrap);
}

// ---- thin form ------------------------------------------------------------------------------------------------------
// Q: per-query register sets (nxi <= Q).  One lane per column; a lane's state per query is the bracket so far:
// (xl, yl) the last node <= q, (xr, yr) the node behind it, or the last node of the column.
template <int Q>
__global__ __launch_bounds__(kBlock) void each1_thin_kernel(const double* __restrict__ x, size_t ldx, const double* __restrict__ y,
                                                            size_t ldy, int n, const uint32_t* __restrict__ len, size_t ncols,
                                                            const double* __restrict__ xi, size_t ldxi, int nxi,
                                                            double* __restrict__ yi, size_t ldyi, double extrap,
                                                            uint32_t* __restrict__ col_ok, int vec)
{
    const size_t nblocks = (ncols + kBlock - 1) / kBlock;
    for (size_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const size_t c = b * kBlock + threadIdx.x;
        if (c >= ncols) continue;                            // (no barrier anywhere: lanes are independent)
        const double* const xc = x + c * ldx;
        const double* const yc = y + c * ldy;
        const int nc = col_len(len, c, n);
        double q[Q], xl[Q], yl[Q], xr[Q], yr[Q];
        bool took[Q];                                        // node k-1 was <= q (true in front of the column)
#pragma unroll
        for (int i = 0; i < Q; ++i) {
            q[i] = (i < nxi) ? xi[c * ldxi + i] : __builtin_nan("");
            xl[i] = yl[i] = xr[i] = yr[i] = 0.0;
            took[i] = true;
        }
        double x0 = 0.0, x1 = 0.0, prev = -__builtin_inf();
        bool bad = nc == 0;
        auto node = [&](int k, double xk, double yk) {
            const bool in = k < nc;
            bad |= in & (!(prev < xk) | !(xk < __builtin_inf()));
            prev = xk;
            if (k == 0) x0 = xk;
            x1 = in ? xk : x1;
#pragma unroll
            for (int i = 0; i < Q; ++i) {
                const bool behind = in & took[i];            // k <= l + 1: ends on r = min(l + 1, nc - 1)
                xr[i] = behind ? xk : xr[i];
                yr[i] = behind ? yk : yr[i];
                const bool take = behind & (xk <= q[i]);     // k <= l  (k == 0 is taken as "any l in range" below x0)
                const bool keep = take | (k == 0);
                xl[i] = keep ? xk : xl[i];
                yl[i] = keep ? yk : yl[i];
                took[i] = take;
            }
        };
        if (vec) {
            int k = 0;
            for (; k + 1 < n; k += 2) {
                const d2 xv = *reinterpret_cast<const d2*>(xc + k), yv = *reinterpret_cast<const d2*>(yc + k);
                node(k, xv.x, yv.x);
                node(k + 1, xv.y, yv.y);
            }
            if (k < n) node(k, xc[k], yc[k]);
        } else {
            for (int k = 0; k < n; ++k) node(k, xc[k], yc[k]);
        }
        double* const out = yi + c * ldyi;
#pragma unroll
        for (int i = 0; i < Q; ++i)
            if (i < nxi) out[i] = bad ? __builtin_nan("") : finish(xl[i], xr[i], yl[i], yr[i], q[i], x0, x1, extrap);
        if (col_ok) col_ok[c] = bad ? 0u : 1u;
    }
}

// ---- direct form, first pass (mi_pairs1.hip's) ------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void each1_validate_kernel(const double* __restrict__ x, size_t ldx, int n,
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

// ---- LDS form and direct form with per-column queries -----------------------------------------------------------------
// LDSF: LDS form / direct form.  VEC: 16-B stores (yi 16-B aligned, ldyi even) / 8-B stores.
// unit u = (row block u % nrb, column run u / nrb).  flag: LDS form: col_ok, written (may be null); direct form: read.
template <bool LDSF, bool VEC>
__global__ __launch_bounds__(kBlock) void each1_kernel(const double* __restrict__ x, size_t ldx, const double* __restrict__ y,
                                                       size_t ldy, int n, const uint32_t* __restrict__ len, size_t ncols,
                                                       size_t run, const double* __restrict__ xi, size_t ldxi, size_t nxi,
                                                       size_t nrb, size_t nunits, double* __restrict__ yi, size_t ldyi,
                                                       double extrap, uint32_t* flag)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    lds_double* const lds = (lds_double*)smem;
    const int sx = (int)x_stride((size_t)n);
    const int pair = sx + n + 2;
    lds_int* const wflag = (lds_int*)(lds + 2 * (size_t)pair);   // [2 buffer pairs][kWaves] validation
    const int t = (int)threadIdx.x;
    for (size_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const size_t rb = u % nrb, s = u / nrb;
        const size_t c0 = s * run, c1 = min(c0 + run, ncols);
        const size_t row0 = rb * kRowBlock;
        // this lane's rows, (ia, ib) + j*512 for j < kQIter
        const size_t ia = row0 + (VEC ? 2 * t : t), ib = ia + (VEC ? 1 : kBlock);
        double qa[kQIter], qb[kQIter], na[kQIter], nb[kQIter];
        auto queries = [&](size_t c, double (&a)[kQIter], double (&b)[kQIter]) {     // NaN where there is no such row
            const double* const qc = xi + c * ldxi;
#pragma unroll
            for (int j = 0; j < kQIter; ++j) {
                const size_t o = (size_t)j * (2 * kBlock);
                a[j] = (ia + o < nxi) ? __builtin_nontemporal_load(qc + ia + o) : __builtin_nan("");
                b[j] = (ib + o < nxi) ? __builtin_nontemporal_load(qc + ib + o) : __builtin_nan("");
            }
        };
        ColLoad LX, LY;
        int nc_next = 0;
        queries(c0, na, nb);
        if constexpr (LDSF) {
            // (every column of the previous unit ended on a barrier: both buffer pairs are free)
            nc_next = col_len(len, c0, n);
            col_issue<true>(LX, x + c0 * ldx, nc_next);
            col_issue<false>(LY, y + c0 * ldy, nc_next);
            const bool bad = col_commit<true, true>(LX, x + c0 * ldx, nc_next, lds) | (nc_next == 0);
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
#pragma unroll
            for (int j = 0; j < kQIter; ++j) {
                qa[j] = na[j];
                qb[j] = nb[j];
            }
            int nc;
            bool ok;
            if constexpr (LDSF) {
                nc = nc_next;
                if (more) {                                  // in flight while this column is searched and blended
                    nc_next = col_len(len, c + 1, n);
                    col_issue<true>(LX, xcol + ldx, nc_next);
                    col_issue<false>(LY, ycol + ldy, nc_next);
                    queries(c + 1, na, nb);
                }
                int any = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) any |= wflag[cb * kWaves + w];
                ok = any == 0;
                if (flag && rb == 0 && t == 0) flag[c] = ok ? 1u : 0u;
            } else {
                nc = col_len(len, c, n);
                ok = flag[c] != 0;
                if (more) queries(c + 1, na, nb);
            }
            double* const out = yi + c * ldyi;
            int la[kQIter], lb[kQIter];
            double x0 = 0.0, x1 = 0.0;
            const LdsX<true> curx = {lds + (size_t)cb * pair};
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
                        va = blend<true>(curx, cury, nc, la[j], qa[j], x0, x1, extrap);
                        vb = blend<true>(curx, cury, nc, lb[j], qb[j], x0, x1, extrap);
                    } else {
                        va = blend<false>(xcol, ycol, nc, la[j], qa[j], x0, x1, extrap);
                        vb = blend<false>(xcol, ycol, nc, lb[j], qb[j], x0, x1, extrap);
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
                    const bool bad = col_commit<true, true>(LX, xcol + ldx, nc_next, nx) | (nc_next == 0);
                    col_commit<false, false>(LY, ycol + ldy, nc_next, nx + sx);
                    const bool wb = __any(bad);
                    if ((t & 63) == 0) wflag[(cb ^ 1) * kWaves + (t >> 6)] = wb;
                }
                __syncthreads();
            }
        }
    }
}

template <bool LDSF, bool VEC>
mi_status launch(mi_ctx* ctx, unsigned grid, size_t lds_bytes, const double* x, size_t ldx, const double* y, size_t ldy, int n,
                 const uint32_t* len, size_t ncols, size_t run, const double* xi, size_t ldxi, size_t nxi, size_t nrb,
                 size_t nunits, double* yi, size_t ldyi, double extrap, uint32_t* flag)
{
    if (lds_bytes > 64 * 1024)   // above the default limit of dynamic LDS (per device: asked for at every such launch)
        MI_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&each1_kernel<LDSF, VEC>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes_for(kLdsMaxN)));
    hipLaunchKernelGGL((each1_kernel<LDSF, VEC>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, x, ldx, y, ldy, n, len, ncols,
                       run, xi, ldxi, nxi, nrb, nunits, yi, ldyi, extrap, flag);
    MI_LAUNCH_CHECK(ctx, "interp1 each kernel");
    return MI_OK;
}

template <int Q>
mi_status launch_thin(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, int n, const uint32_t* len,
                      size_t ncols, const double* xi, size_t ldxi, int nxi, double* yi, size_t ldyi, double extrap,
                      uint32_t* col_ok)
{
    const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0 && ((ldx | ldy) & 1) == 0;
    hipLaunchKernelGGL((each1_thin_kernel<Q>), dim3(mi::stream_grid(ctx, ncols, kBlock)), dim3(kBlock), 0, ctx->stream, x, ldx, y,
                       ldy, n, len, ncols, xi, ldxi, nxi, yi, ldyi, extrap, col_ok, vec);
    MI_LAUNCH_CHECK(ctx, "interp1 each thin kernel");
    return MI_OK;
}

// the argument rules shared by the entry points (who: the entry point's name); dev: alignment is checked too
mi_status check_args(const mi_ctx* ctx, const char* who, bool dev, const double* x, size_t ldx, const double* y, size_t ldy,
                     size_t n, const uint32_t* len, size_t ncols, const double* xi, size_t ldxi, size_t nxi, const double* yi,
                     size_t ldyi, const uint32_t* col_ok)
{
    MI_REQUIRE(ctx, x && y && xi && yi, "%s: NULL table/query/result pointer", who);
    if (dev) {
        const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xi) |
                             reinterpret_cast<uintptr_t>(yi);
        MI_REQUIRE(ctx, (al & 7u) == 0, "%s: x, y, xi, yi must be 8-byte aligned", who);
        const uintptr_t al4 = reinterpret_cast<uintptr_t>(len) | reinterpret_cast<uintptr_t>(col_ok);
        MI_REQUIRE(ctx, (al4 & 3u) == 0, "%s: len, col_ok must be 4-byte aligned", who);
    }
    MI_REQUIRE(ctx, n >= 2, "%s: need at least two nodes per column (n=%zu)", who, n);
    MI_REQUIRE(ctx, n < 0x7ffffff0u, "%s: n=%zu exceeds 2^31 - 16", who, n);
    MI_REQUIRE(ctx, ldx >= n, "%s: ldx=%zu is smaller than n=%zu", who, ldx, n);
    MI_REQUIRE(ctx, ldy >= n, "%s: ldy=%zu is smaller than n=%zu", who, ldy, n);
    MI_REQUIRE(ctx, ldyi >= nxi, "%s: ldyi=%zu is smaller than nxi=%zu", who, ldyi, nxi);
    MI_REQUIRE(ctx, ldxi == 0 || ldxi >= nxi, "%s: ldxi=%zu is smaller than nxi=%zu (0: one xi for every column)", who, ldxi, nxi);
    const size_t lim = SIZE_MAX / (2 * sizeof(double)) / ncols;
    MI_REQUIRE(ctx, ldx <= lim && ldy <= lim && ldyi <= lim && ldxi <= lim && nxi <= lim,
               "%s: ncols=%zu x (ldx=%zu, ldy=%zu, ldxi=%zu, ldyi=%zu) too large", who, ncols, ldx, ldy, ldxi, ldyi);
    return MI_OK;
}

// ncols columns of `rows` doubles between a compact device buffer and a host matrix with leading dimension ld
hipError_t copy_cols(double* dst, size_t ld_dst, const double* src, size_t ld_src, size_t rows, size_t ncols, hipMemcpyKind kind,
                     hipStream_t stream)
{
    if (ld_dst == rows && ld_src == rows) return hipMemcpyAsync(dst, src, rows * ncols * sizeof(double), kind, stream);
    return hipMemcpy2DAsync(dst, ld_dst * sizeof(double), src, ld_src * sizeof(double), rows * sizeof(double), ncols, kind, stream);
}

}  // namespace mi_each1

using namespace mi_each1;

extern "C" {

size_t mi_debug_each_launches(int form)
{
    return (form >= 0 && form < 4) ? g_launches[form].load(std::memory_order_relaxed) : 0;
}

mi_status mi_interp1_each_f64_dev(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                  const uint32_t* len, size_t ncols, const double* xi, size_t ldxi, size_t nxi, double* yi,
                                  size_t ldyi, double extrap, uint32_t* col_ok)
{
    MI_REQUIRE(ctx, ctx, "mi_interp1_each_f64_dev: NULL context");
    if (ncols == 0 || nxi == 0) return MI_OK;
    mi_status st = check_args(ctx, "mi_interp1_each_f64_dev", true, x, ldx, y, ldy, n, len, ncols, xi, ldxi, nxi, yi, ldyi, col_ok);
    if (st != MI_OK) return st;
    if (n <= kThinMaxN && nxi <= kThinMaxQ) {
        MI_HIP(ctx, hipSetDevice(ctx->device));
        const int q = (int)nxi;
        st = q <= 1 ? launch_thin<1>(ctx, x, ldx, y, ldy, (int)n, len, ncols, xi, ldxi, q, yi, ldyi, extrap, col_ok)
           : q <= 2 ? launch_thin<2>(ctx, x, ldx, y, ldy, (int)n, len, ncols, xi, ldxi, q, yi, ldyi, extrap, col_ok)
           : q <= 4 ? launch_thin<4>(ctx, x, ldx, y, ldy, (int)n, len, ncols, xi, ldxi, q, yi, ldyi, extrap, col_ok)
                    : launch_thin<(int)kThinMaxQ>(ctx, x, ldx, y, ldy, (int)n, len, ncols, xi, ldxi, q, yi, ldyi, extrap, col_ok);
        if (st == MI_OK) g_launches[0].fetch_add(1, std::memory_order_relaxed);
        return st;
    }
    if (ldxi == 0) {   // one XI for every column: the existing call's own case
        st = mi_interp1_pairs_f64_dev(ctx, x, ldx, y, ldy, n, len, ncols, xi, nxi, yi, ldyi, extrap, col_ok);
        if (st == MI_OK) g_launches[3].fetch_add(1, std::memory_order_relaxed);
        return st;
    }
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    // units: row blocks x column runs, about 16 workgroups of work per CU when the shape has that much (mi_pairs1.hip's cut)
    const size_t nrb = (nxi + kRowBlock - 1) / kRowBlock;
    const size_t target = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * 16;
    const size_t want_runs = std::min(ncols, std::max<size_t>(1, (target + nrb - 1) / nrb));
    const size_t run = (ncols + want_runs - 1) / want_runs;
    const size_t nruns = (ncols + run - 1) / run;
    MI_REQUIRE(ctx, nrb <= SIZE_MAX / nruns, "mi_interp1_each_f64_dev: nxi=%zu x ncols=%zu too large", nxi, ncols);
    const size_t nunits = nrb * nruns;
    const unsigned grid = (unsigned)std::min(nunits, target);   // workgroups stride over the units beyond that
    const bool vec = (reinterpret_cast<uintptr_t>(yi) & 15u) == 0 && (ldyi & 1) == 0;
    if (n <= kLdsMaxN) {
        const size_t lds_bytes = lds_bytes_for(n);
        st = vec ? launch<true, true>(ctx, grid, lds_bytes, x, ldx, y, ldy, (int)n, len, ncols, run, xi, ldxi, nxi, nrb, nunits, yi, ldyi, extrap, col_ok)
                 : launch<true, false>(ctx, grid, lds_bytes, x, ldx, y, ldy, (int)n, len, ncols, run, xi, ldxi, nxi, nrb, nunits, yi, ldyi, extrap, col_ok);
        if (st == MI_OK) g_launches[1].fetch_add(1, std::memory_order_relaxed);
        return st;
    }
    uint32_t* flag = col_ok;
    if (!flag) {
        st = mi::ensure_scratch(ctx, 3, ncols * sizeof(uint32_t));
        if (st != MI_OK) return st;
        flag = (uint32_t*)ctx->scratch[3];
    }
    hipLaunchKernelGGL(each1_validate_kernel, dim3(mi::stream_grid(ctx, ncols * kBlock, kBlock)), dim3(kBlock), 0, ctx->stream, x, ldx,
                       (int)n, len, ncols, flag);
    MI_LAUNCH_CHECK(ctx, "interp1 each validation kernel");
    st = vec ? launch<false, true>(ctx, grid, 0, x, ldx, y, ldy, (int)n, len, ncols, run, xi, ldxi, nxi, nrb, nunits, yi, ldyi, extrap, flag)
             : launch<false, false>(ctx, grid, 0, x, ldx, y, ldy, (int)n, len, ncols, run, xi, ldxi, nxi, nrb, nunits, yi, ldyi, extrap, flag);
    if (st == MI_OK) g_launches[2].fetch_add(1, std::memory_order_relaxed);
    return st;
}

mi_status mi_interp1_each_f64_host(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                   const uint32_t* len, size_t ncols, const double* xi, size_t ldxi, size_t nxi, double* yi,
                                   size_t ldyi, double extrap, uint32_t* col_ok)
{
    MI_REQUIRE(ctx, ctx, "mi_interp1_each_f64_host: NULL context");
    if (ncols == 0 || nxi == 0) return MI_OK;
    mi_status st = check_args(ctx, "mi_interp1_each_f64_host", false, x, ldx, y, ldy, n, len, ncols, xi, ldxi, nxi, yi, ldyi, col_ok);
    if (st != MI_OK) return st;
    MI_HIP(ctx, hipSetDevice(ctx->device));
    // device copies are compact (leading dimensions n and nxi), sub-allocated so that slot 3 stays with the device call:
    // slot 0 X then Y, slot 1 XI (one vector, or nxi x ncols: as large as YI) then len then col_ok, slot 2 YI
    const bool each = ldxi > 0;
    const size_t xi_bytes = (each ? nxi * ncols : nxi) * sizeof(double), u32_bytes = ncols * sizeof(uint32_t);
    st = mi::ensure_scratch(ctx, 0, 2 * n * ncols * sizeof(double));
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 1, xi_bytes + 2 * u32_bytes);
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 2, nxi * ncols * sizeof(double));
    if (st != MI_OK) return st;
    double *dx = (double*)ctx->scratch[0], *dy = dx + n * ncols, *dxi = (double*)ctx->scratch[1], *dyi = (double*)ctx->scratch[2];
    uint32_t *dlen = (uint32_t*)((char*)ctx->scratch[1] + xi_bytes), *dok = dlen + ncols;
    std::vector<uint32_t> ok_own;
    if (!col_ok) ok_own.resize(ncols);
    uint32_t* const hok = col_ok ? col_ok : ok_own.data();
    const size_t chunk = (size_t)8 << 20;   // elements, as mi_interp1_pairs_f64_host
    const size_t per_col = std::max(n, nxi);
    // above the threshold: pinned column chunks of about `chunk` elements; the copy back of chunk k (on the aux stream)
    // overlaps the upload and the kernels of chunk k+1
    const bool chunked = per_col > 2 * chunk / ncols;
    if (chunked) {
        st = mi::ensure_aux_stream(ctx);
        if (st != MI_OK) return st;
    }
    const size_t x_bytes = ((ncols - 1) * ldx + n) * sizeof(double), y_bytes = ((ncols - 1) * ldy + n) * sizeof(double),
                 yi_bytes = ((ncols - 1) * ldyi + nxi) * sizeof(double), q_bytes = ((ncols - 1) * ldxi + nxi) * sizeof(double);
    const bool pin_q = chunked && mi::pin_host(xi, q_bytes), pin_x = chunked && mi::pin_host(x, x_bytes),
               pin_y = chunked && mi::pin_host(y, y_bytes), pin_o = chunked && mi::pin_host(yi, yi_bytes);
    // no early return before both streams are drained and the ranges released
    hipStream_t back = chunked ? ctx->aux_stream : ctx->stream;
    hipError_t herr = hipSuccess;
    const char* what = "upload of the queries";
    if (!each) herr = hipMemcpyAsync(dxi, xi, xi_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (herr == hipSuccess && len) {
        herr = hipMemcpyAsync(dlen, len, u32_bytes, hipMemcpyHostToDevice, ctx->stream);
        what = "upload of the column lengths";
    }
    const size_t cols = chunked ? std::max<size_t>(1, chunk / per_col) : ncols;
    const bool fail_hook = getenv("MI_TEST_FAIL_EACH_CHUNK") != nullptr;
    for (size_t c0 = 0; c0 < ncols && herr == hipSuccess && st == MI_OK; c0 += cols) {
        const size_t m = std::min(cols, ncols - c0);
        if (fail_hook && c0 > 0) { herr = hipErrorUnknown; what = "MI_TEST_FAIL_EACH_CHUNK (error-path test hook)"; break; }
        herr = copy_cols(dx + c0 * n, n, x + c0 * ldx, ldx, n, m, hipMemcpyHostToDevice, ctx->stream);
        if (herr == hipSuccess) herr = copy_cols(dy + c0 * n, n, y + c0 * ldy, ldy, n, m, hipMemcpyHostToDevice, ctx->stream);
        if (herr == hipSuccess && each)   // XI travels with its columns
            herr = copy_cols(dxi + c0 * nxi, nxi, xi + c0 * ldxi, ldxi, nxi, m, hipMemcpyHostToDevice, ctx->stream);
        if (herr != hipSuccess) { what = "upload of a column chunk"; break; }
        st = mi_interp1_each_f64_dev(ctx, dx + c0 * n, n, dy + c0 * n, n, n, len ? dlen + c0 : nullptr, m, each ? dxi + c0 * nxi : dxi,
                                     each ? nxi : 0, nxi, dyi + c0 * nxi, nxi, extrap, dok + c0);
        if (st != MI_OK) break;
        if (chunked) {
            herr = hipEventRecord(ctx->aux_event, ctx->stream);
            if (herr == hipSuccess) herr = hipStreamWaitEvent(ctx->aux_stream, ctx->aux_event, 0);
        }
        if (herr == hipSuccess) herr = copy_cols(yi + c0 * ldyi, ldyi, dyi + c0 * nxi, nxi, nxi, m, hipMemcpyDeviceToHost, back);
        if (herr != hipSuccess) what = "download of a result chunk";
    }
    if (herr == hipSuccess && st == MI_OK) {
        herr = hipMemcpyAsync(hok, dok, u32_bytes, hipMemcpyDeviceToHost, ctx->stream);
        what = "download of the column flags";
    }
    const hipError_t e1 = hipStreamSynchronize(ctx->stream), e2 = chunked ? hipStreamSynchronize(ctx->aux_stream) : hipSuccess;
    if (pin_q) mi::unpin_host(xi);
    if (pin_x) mi::unpin_host(x);
    if (pin_y) mi::unpin_host(y);
    if (pin_o) mi::unpin_host(yi);
    if (st != MI_OK) return st;
    if (herr != hipSuccess) return mi::fail(ctx, MI_ERR_HIP, "mi_interp1_each_f64_host: %s failed: %s", what, hipGetErrorString(herr));
    MI_HIP(ctx, e1);
    MI_HIP(ctx, e2);
    if (!col_ok)   // the caller has no other way to learn it; every output is complete (NaN in the bad columns)
        for (size_t c = 0; c < ncols; ++c)
            if (!hok[c])
                return mi::fail(ctx, MI_ERR_GRID, "mi_interp1_each_f64_host: column %zu is bad (len outside [2, n], or X not finite "
                                "and strictly increasing; X is not sorted for the caller); its outputs are NaN", c);
    return MI_OK;
}

}  // extern "C"
