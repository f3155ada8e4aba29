// interp1 over paired columns: every column of Y has an X column of its own.  X and Y column-major n x B (leading
// dimensions ldx, ldy), an optional fill count len[c] (valid leading rows of column c, 2 <= len[c] <= n; NULL: n
// everywhere), queries XI (nxi, any order, shared by every column) -> YI column-major nxi x B (leading dimension ldyi),
//     YI[i + c*ldyi] == mi_interp1_f64_dev's result for XI[i] on the table (X[0:len[c], c], Y[0:len[c], c]),  bit for bit.
// An ensemble of trajectories, each sampled at its own (event) times, resampled onto one common mesh; with n = 2 and
// nxi = 1 it is the shape of the reference's RestrictKernel (EventDrivenMap.cu:769-785).
//
// X lives on the device and changes from call to call, so it is validated on the device, always, with mi_axis1_create's
// rule: a column is bad when len[c] < 2, len[c] > n, or X[0:len[c], c] is not finite and strictly increasing
// (!(X[k-1] < X[k]): equal nodes and the pair -0.0, 0.0 are bad).  A bad column's outputs are all NaN; col_ok[c] (optional)
// is 1 for a good column, 0 for a bad one.  A chain  -inf < X[0] < X[1] < ... < X[len-1] < +inf  of true comparisons is
// that rule exactly: a NaN fails both comparisons it takes part in, an infinity fails one of them.
//
// The weight is mi_interp2_eval.hpp's weight(), a > 0 ? a/(a+b) : 0, the blend is interp1's (1-w)*Y[l] + w*Y[r], and
// this file is compiled with -ffp-contract=off like every other, so every product and sum rounds.
//
// The work is cut as mi_cols1.hip cuts it: a unit is (row block of kRowBlock consecutive outputs) x (run of consecutive
// columns), workgroups stride over the units, and a lane keeps its 2*kQIter queries in registers across the run's
// columns.  There are no records: with an X per column nothing located for one column serves another, so the bracket
// search runs inside the column kernel, once per output.
//   LDS form (n <= kLdsMaxN): X[:, c] and Y[:, c] are each read once, 16 B per lane and coalesced, into one of two LDS
//            buffer pairs (one padding element at index len[c] holding the last node, so that l+1 never leaves the
//            buffer and equals the value at r = min(l+1, len-1); X plain or skewed, see mi_paired_cols.hpp);
//            the loads of the next column are issued before the current one is searched and blended; one barrier
//            per column.  Every workgroup that stages a column checks
//            its staged X on the way into LDS (each element against its predecessor: the other half of its own 16-B
//            vector, the neighbouring lane's by a wave shuffle, the neighbouring wave's by one 8-B load per wave) and
//            leaves one flag per wave beside the buffers -- no extra pass, no traffic between workgroups.  The bracket
//            is a branch-free binary search over X in LDS, the 2*kQIter searches of a lane interleaved.
//   direct form (longer columns): a streaming pass (one workgroup per column at a time) validates every column first
//            and writes its flag -- into col_ok when the caller gave one, else into context scratch slot 3, which the
//            gridded and shared-axis calls use in stream order on the same stream -- and the column kernel reads the
//            flag, searches X and gathers X[l], X[r], Y[l], Y[r] on the column itself through L2.
//   YI is written with coalesced non-temporal stores: 16 B per lane (rows 2t, 2t+1) when yi is 16-B aligned and ldyi is
//   even, otherwise 8 B per lane (rows t, t+256).
// Every index into x, y and yi is 64-bit; no grid dimension depends on B, n or nxi.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "mi_interp2_eval.hpp"
#include "mi_paired_cols.hpp"

namespace mi_pairs1 {

using mi_interp2::kBlock;
using namespace mi_paired;   // the LDS layouts, the staging of a column (ColLoad ...), col_len and search, shared with mi_each1.hip

constexpr size_t kRowBlock = 2 * kBlock * kQIter;    // 2048 outputs of one column per unit
constexpr size_t kLdsMaxN = 4096;                    // LDS form up to here: 2 pairs x (2 n + n/32 + 4) x 8 B + flags = 133248 B of the CU's 160 KiB

// one output: X, Y readable at l and at l + 1 (LDS form: the padding element) or at r = min(l+1, nc-1) (direct form)
template <bool LDSF, typename XP, typename YP>
__device__ __forceinline__ double blend(XP X, YP Y, int nc, int l, double q, double x0, double x1, bool ok, double extrap)
{
    const int r = LDSF ? l + 1 : min(l + 1, nc - 1);
    const double w = mi_interp2::weight(X[l], X[r], q);
    double v = (1.0 - w) * Y[l] + w * Y[r];
    if (!(q >= x0 && q <= x1)) v = (q != q) ? __builtin_nan("") : extrap;
    return ok ? v : __builtin_nan("");
}

// direct form, first pass: flag[c] = 1 when column c is good, 0 when it is bad; workgroups stride over the columns
__global__ __launch_bounds__(kBlock) void pairs1_validate_kernel(const double* __restrict__ x, size_t ldx, int n,
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
__global__ __launch_bounds__(kBlock) void pairs1_kernel(const double* __restrict__ x, size_t ldx, const double* __restrict__ y,
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
        const size_t row0 = rb * kRowBlock;
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
                    if (more) {                                  // in flight while this column is searched and blended
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
                            va = blend<true>(curx, cury, nc, la[j], qa[j], x0, x1, true, extrap);
                            vb = blend<true>(curx, cury, nc, lb[j], qb[j], x0, x1, true, extrap);
                        } else {
                            va = blend<false>(xcol, ycol, nc, la[j], qa[j], x0, x1, true, extrap);
                            vb = blend<false>(xcol, ycol, nc, lb[j], qb[j], x0, x1, true, extrap);
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
mi_status launch(mi_ctx* ctx, unsigned grid, size_t lds_bytes, const double* x, size_t ldx, const double* y, size_t ldy, int n,
                 const uint32_t* len, size_t ncols, size_t run, const double* xi, size_t nxi, size_t nrb, size_t nunits,
                 double* yi, size_t ldyi, double extrap, uint32_t* flag)
{
    if (lds_bytes > 64 * 1024)   // above the default limit of dynamic LDS (per device: asked for at every such launch)
        MI_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&pairs1_kernel<LDSF, VEC>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes_for(kLdsMaxN)));
    hipLaunchKernelGGL((pairs1_kernel<LDSF, VEC>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, x, ldx, y, ldy, n, len, ncols,
                       run, xi, nxi, nrb, nunits, yi, ldyi, extrap, flag);
    MI_LAUNCH_CHECK(ctx, "interp1 pairs kernel");
    return MI_OK;
}

// the argument rules shared by the three entry points (who: the entry point's name); dev: alignment is checked too
mi_status check_args(const mi_ctx* ctx, const char* who, bool dev, const double* x, size_t ldx, const double* y, size_t ldy,
                     size_t n, const uint32_t* len, size_t ncols, const double* xi, size_t nxi, const double* yi, size_t ldyi,
                     const uint32_t* col_ok)
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
    const size_t lim = SIZE_MAX / (2 * sizeof(double)) / ncols;
    MI_REQUIRE(ctx, ldx <= lim && ldy <= lim && ldyi <= lim && nxi <= lim,
               "%s: ncols=%zu x (ldx=%zu, ldy=%zu, ldyi=%zu) too large", who, ncols, ldx, ldy, ldyi);
    return MI_OK;
}

// ncols columns of `rows` doubles between a compact device buffer and a host matrix with leading dimension ld
hipError_t copy_cols(double* dst, size_t ld_dst, const double* src, size_t ld_src, size_t rows, size_t ncols, hipMemcpyKind kind,
                     hipStream_t stream)
{
    if (ld_dst == rows && ld_src == rows) return hipMemcpyAsync(dst, src, rows * ncols * sizeof(double), kind, stream);
    return hipMemcpy2DAsync(dst, ld_dst * sizeof(double), src, ld_src * sizeof(double), rows * sizeof(double), ncols, kind, stream);
}

}  // namespace mi_pairs1

using namespace mi_pairs1;

extern "C" {

mi_status mi_interp1_pairs_f64_dev(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                   const uint32_t* len, size_t ncols, const double* xi, size_t nxi, double* yi, size_t ldyi,
                                   double extrap, uint32_t* col_ok)
{
    MI_REQUIRE(ctx, ctx, "mi_interp1_pairs_f64_dev: NULL context");
    if (ncols == 0 || nxi == 0) return MI_OK;
    mi_status st = check_args(ctx, "mi_interp1_pairs_f64_dev", true, x, ldx, y, ldy, n, len, ncols, xi, nxi, yi, ldyi, col_ok);
    if (st != MI_OK) return st;
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    // units: row blocks x column runs, about 16 workgroups of work per CU when the shape has that much
    const size_t nrb = (nxi + kRowBlock - 1) / kRowBlock;
    const size_t target = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * 16;
    const size_t want_runs = std::min(ncols, std::max<size_t>(1, (target + nrb - 1) / nrb));
    const size_t run = (ncols + want_runs - 1) / want_runs;
    const size_t nruns = (ncols + run - 1) / run;
    MI_REQUIRE(ctx, nrb <= SIZE_MAX / nruns, "mi_interp1_pairs_f64_dev: nxi=%zu x ncols=%zu too large", nxi, ncols);
    const size_t nunits = nrb * nruns;
    const unsigned grid = (unsigned)std::min(nunits, target);   // workgroups stride over the units beyond that
    const bool vec = (reinterpret_cast<uintptr_t>(yi) & 15u) == 0 && (ldyi & 1) == 0;
    if (n <= kLdsMaxN) {
        const size_t lds_bytes = lds_bytes_for(n);
        return vec ? launch<true, true>(ctx, grid, lds_bytes, x, ldx, y, ldy, (int)n, len, ncols, run, xi, nxi, nrb, nunits, yi, ldyi, extrap, col_ok)
                   : launch<true, false>(ctx, grid, lds_bytes, x, ldx, y, ldy, (int)n, len, ncols, run, xi, nxi, nrb, nunits, yi, ldyi, extrap, col_ok);
    }
    uint32_t* flag = col_ok;
    if (!flag) {
        st = mi::ensure_scratch(ctx, 3, ncols * sizeof(uint32_t));
        if (st != MI_OK) return st;
        flag = (uint32_t*)ctx->scratch[3];
    }
    hipLaunchKernelGGL(pairs1_validate_kernel, dim3(mi::stream_grid(ctx, ncols * kBlock, kBlock)), dim3(kBlock), 0, ctx->stream, x, ldx,
                       (int)n, len, ncols, flag);
    MI_LAUNCH_CHECK(ctx, "interp1 pairs validation kernel");
    return vec ? launch<false, true>(ctx, grid, 0, x, ldx, y, ldy, (int)n, len, ncols, run, xi, nxi, nrb, nunits, yi, ldyi, extrap, flag)
               : launch<false, false>(ctx, grid, 0, x, ldx, y, ldy, (int)n, len, ncols, run, xi, nxi, nrb, nunits, yi, ldyi, extrap, flag);
}

mi_status mi_interp1_pairs_f64_host(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                    const uint32_t* len, size_t ncols, const double* xi, size_t nxi, double* yi, size_t ldyi,
                                    double extrap, uint32_t* col_ok)
{
    MI_REQUIRE(ctx, ctx, "mi_interp1_pairs_f64_host: NULL context");
    if (ncols == 0 || nxi == 0) return MI_OK;
    mi_status st = check_args(ctx, "mi_interp1_pairs_f64_host", false, x, ldx, y, ldy, n, len, ncols, xi, nxi, yi, ldyi, col_ok);
    if (st != MI_OK) return st;
    MI_HIP(ctx, hipSetDevice(ctx->device));
    // device copies are compact (leading dimensions n and nxi), sub-allocated so that slot 3 stays with the device call:
    // slot 0 X then Y, slot 1 XI then len then col_ok, slot 2 YI
    const size_t xi_bytes = nxi * sizeof(double), u32_bytes = ncols * sizeof(uint32_t);
    st = mi::ensure_scratch(ctx, 0, 2 * n * ncols * sizeof(double));
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 1, xi_bytes + 2 * u32_bytes);
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 2, nxi * ncols * sizeof(double));
    if (st != MI_OK) return st;
    double *dx = (double*)ctx->scratch[0], *dy = dx + n * ncols, *dxi = (double*)ctx->scratch[1], *dyi = (double*)ctx->scratch[2];
    uint32_t *dlen = (uint32_t*)((char*)ctx->scratch[1] + xi_bytes), *dok = dlen + ncols;
    std::vector<uint32_t> ok_own;
    if (!col_ok) ok_own.resize(ncols);
    uint32_t* const hok = col_ok ? col_ok : ok_own.data();
    const size_t chunk = (size_t)8 << 20;   // elements, as the 8 M-query chunks of mi_interp1_f64_host
    const size_t per_col = std::max(n, nxi);
    // above the threshold: column chunks of about `chunk` elements, pinned like mi_interp1_cols_f64_host: the copy back
    // of chunk k (on the aux stream) overlaps the upload and the kernels of chunk k+1
    const bool chunked = per_col > 2 * chunk / ncols;
    if (chunked) {
        st = mi::ensure_aux_stream(ctx);
        if (st != MI_OK) return st;
    }
    const size_t x_bytes = ((ncols - 1) * ldx + n) * sizeof(double), y_bytes = ((ncols - 1) * ldy + n) * sizeof(double),
                 yi_bytes = ((ncols - 1) * ldyi + nxi) * sizeof(double);
    const bool pin_q = chunked && mi::pin_host(xi, xi_bytes), pin_x = chunked && mi::pin_host(x, x_bytes),
               pin_y = chunked && mi::pin_host(y, y_bytes), pin_o = chunked && mi::pin_host(yi, yi_bytes);
    // no early return before both streams are drained and the ranges released
    hipStream_t back = chunked ? ctx->aux_stream : ctx->stream;
    hipError_t herr = hipMemcpyAsync(dxi, xi, xi_bytes, hipMemcpyHostToDevice, ctx->stream);
    const char* what = "upload of the queries";
    if (herr == hipSuccess && len) {
        herr = hipMemcpyAsync(dlen, len, u32_bytes, hipMemcpyHostToDevice, ctx->stream);
        what = "upload of the column lengths";
    }
    const size_t cols = chunked ? std::max<size_t>(1, chunk / per_col) : ncols;
    const bool fail_hook = getenv("MI_TEST_FAIL_PAIRS_CHUNK") != nullptr;
    for (size_t c0 = 0; c0 < ncols && herr == hipSuccess && st == MI_OK; c0 += cols) {
        const size_t m = std::min(cols, ncols - c0);
        if (fail_hook && c0 > 0) { herr = hipErrorUnknown; what = "MI_TEST_FAIL_PAIRS_CHUNK (error-path test hook)"; break; }
        herr = copy_cols(dx + c0 * n, n, x + c0 * ldx, ldx, n, m, hipMemcpyHostToDevice, ctx->stream);
        if (herr == hipSuccess) herr = copy_cols(dy + c0 * n, n, y + c0 * ldy, ldy, n, m, hipMemcpyHostToDevice, ctx->stream);
        if (herr != hipSuccess) { what = "upload of a column chunk"; break; }
        st = mi_interp1_pairs_f64_dev(ctx, dx + c0 * n, n, dy + c0 * n, n, n, len ? dlen + c0 : nullptr, m, dxi, nxi, dyi + c0 * nxi,
                                      nxi, extrap, dok + c0);
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
    if (herr != hipSuccess) return mi::fail(ctx, MI_ERR_HIP, "mi_interp1_pairs_f64_host: %s failed: %s", what, hipGetErrorString(herr));
    MI_HIP(ctx, e1);
    MI_HIP(ctx, e2);
    if (!col_ok)   // the caller has no other way to learn it; every output is complete (NaN in the bad columns)
        for (size_t c = 0; c < ncols; ++c)
            if (!hok[c])
                return mi::fail(ctx, MI_ERR_GRID, "mi_interp1_pairs_f64_host: column %zu is bad (len outside [2, n], or X not finite "
                                "and strictly increasing; X is not sorted for the caller); its outputs are NaN", c);
    return MI_OK;
}

}  // extern "C"
