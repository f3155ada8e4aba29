// Gridded bilinear interpolation, arma::interp2(X, Y, Z, XI, YI, ZI): ZI(i, j) = Z at (XI[j], YI[i]), ZI column-major
// nyi x nxi (zi[i + j*nyi]), over the resident tables of mi_interp2.hip.  Bit-identical to mi_interp2_f64_dev on the
// pair (XI[j], YI[i]): the same locate / weight / blend code (mi_interp2_eval.hpp), compiled with -ffp-contract=off.
//
// Two launches on the context's stream:
//   locate  every XI[j] and YI[i] -> {w, l, r} record (AxRec), once per call, into context scratch slot 3
//           (slots 0-2 belong to the host-convenience paths, which call this with their uploads there);
//   grid    the records and the table -> ZI.  The only stream that scales with the output is its 8-B store.
//     tile form (nyi >= kThinRows): a workgroup owns kTileRows consecutive rows (two per lane) and a strip of
//           columns; the row records stay in registers across the strip, the column record is wave-uniform, and the
//           lane's two cells are re-read only when the column's bracket lx changes.  Column starts are 16-B aligned
//           when zi is and nyi is even: then rows 2t, 2t+1 -> one 16-B store per lane; otherwise rows t, t+256 -> two
//           8-B stores, each one contiguous 512-B run per wave.
//     flat form (nyi < kThinRows, where the tile form would leave most lanes idle): the flat output index, 512
//           consecutive outputs per workgroup; per output a 32-bit division by nyi, two record loads (L1/L2) and the
//           cell.  16-B stores when zi is 16-B aligned.
// Every index into zi is 64-bit; workgroups stride over the work, so no grid dimension depends on nxi or nyi.
#include <algorithm>
#include <cstdint>

#include "mi_interp2_eval.hpp"

namespace mi_interp2 {

constexpr int kTileRows = 2 * kBlock;      // rows per workgroup of the tile form, outputs per workgroup of the flat one
constexpr size_t kThinRows = kBlock;       // below: flat form
constexpr size_t kMaxGrid = (size_t)1 << 20;

__global__ __launch_bounds__(kBlock) void interp2_grid_locate_kernel(AxisDev ax, AxisDev ay, const double* __restrict__ xi,
                                                                     size_t nxi, const double* __restrict__ yi, size_t nyi,
                                                                     AxRec* __restrict__ rec)
{
    const size_t n = nxi + nyi;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock)
        rec[k] = k < nxi ? axis_record(ax, xi[k]) : axis_record(ay, yi[k - nxi]);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void interp2_grid_tile_kernel(G2Dev g, const AxRec* __restrict__ cols,
                                                                   const AxRec* __restrict__ rows, size_t nxi, size_t nyi,
                                                                   size_t strip, size_t nrb, size_t nwork,
                                                                   double* __restrict__ zi, double extrap)
{
    for (size_t b = blockIdx.x; b < nwork; b += gridDim.x) {
        const size_t rb = b % nrb, s = b / nrb;             // consecutive workgroups: consecutive row blocks of a strip
        const size_t i0 = rb * kTileRows + (VEC ? 2 * threadIdx.x : threadIdx.x);
        const size_t i1 = i0 + (VEC ? 1 : kBlock);
        if (i0 >= nyi) continue;
        const bool has1 = i1 < nyi;                        // always true in the VEC form (nyi even)
        const AxRec R0 = rows[i0];
        const AxRec R1 = has1 ? rows[i1] : R0;
        const size_t j0 = s * strip, j1 = min(j0 + strip, nxi);
        int lx = -1;
        d2v lo0, hi0, lo1, hi1;
        for (size_t j = j0; j < j1; ++j) {
            const AxRec X = cols[j];                         // wave-uniform
            double v0, v1;
            if (X.r < 0) {
                v0 = flagged_result(X.r, R0.r, extrap);
                v1 = flagged_result(X.r, R1.r, extrap);
            } else {
                if (X.l != lx) {                             // uniform branch: a new table column
                    lx = X.l;
                    const d2v* c0 = cell_ptr(g, lx, R0.l);
                    const d2v* c1 = cell_ptr(g, lx, R1.l);
                    lo0 = c0[0];
                    hi0 = c0[1];
                    lo1 = c1[0];
                    hi1 = c1[1];
                }
                v0 = blend_records(lo0, hi0, X, R0, extrap);
                v1 = blend_records(lo1, hi1, X, R1, extrap);
            }
            double* col = zi + j * nyi;
            if constexpr (VEC) {
                d2 o;
                o.x = v0;
                o.y = v1;
                __builtin_nontemporal_store(o, reinterpret_cast<d2*>(col + i0));
            } else {
                __builtin_nontemporal_store(v0, col + i0);
                if (has1) __builtin_nontemporal_store(v1, col + i1);
            }
        }
    }
}

__device__ __forceinline__ double grid_point(const G2Dev& g, const AxRec* __restrict__ cols, const AxRec* __restrict__ rows,
                                             size_t jb, uint32_t ib, uint32_t o, uint32_t nyi, double extrap)
{
    const uint32_t u = ib + o;                               // < nyi + kTileRows: no overflow for a thin output
    const uint32_t dj = u / nyi;
    const AxRec X = cols[jb + dj], Y = rows[u - dj * nyi];
    if (X.r < 0 || Y.r < 0) return flagged_result(X.r, Y.r, extrap);
    const d2v* c = cell_ptr(g, X.l, Y.l);
    return blend_records(c[0], c[1], X, Y, extrap);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void interp2_grid_flat_kernel(G2Dev g, const AxRec* __restrict__ cols,
                                                                   const AxRec* __restrict__ rows, uint32_t nyi, size_t total,
                                                                   size_t nwork, double* __restrict__ zi, double extrap)
{
    for (size_t b = blockIdx.x; b < nwork; b += gridDim.x) {
        const size_t k0 = b * kTileRows;
        const size_t jb = k0 / nyi;                          // once per workgroup
        const uint32_t ib = (uint32_t)(k0 - jb * nyi);
        const uint32_t o0 = VEC ? 2 * threadIdx.x : threadIdx.x;
        const uint32_t o1 = VEC ? o0 + 1 : o0 + kBlock;
        const bool has0 = k0 + o0 < total, has1 = k0 + o1 < total;
        if (!has0) continue;
        const double v0 = grid_point(g, cols, rows, jb, ib, o0, nyi, extrap);
        const double v1 = has1 ? grid_point(g, cols, rows, jb, ib, o1, nyi, extrap) : 0.0;
        if (VEC && has1) {
            d2 o;
            o.x = v0;
            o.y = v1;
            __builtin_nontemporal_store(o, reinterpret_cast<d2*>(zi + k0 + o0));
        } else {
            __builtin_nontemporal_store(v0, zi + k0 + o0);
            if (has1) __builtin_nontemporal_store(v1, zi + k0 + o1);
        }
    }
}

}  // namespace mi_interp2

using namespace mi_interp2;

extern "C" {

mi_status mi_interp2_grid_f64_dev(mi_ctx* ctx, const mi_grid2* g, const double* xi, size_t nxi, const double* yi, size_t nyi,
                                  double* zi, double extrap)
{
    MI_REQUIRE(ctx, ctx && g, "mi_interp2_grid_f64_dev: NULL context or grid");
    if (nxi == 0 || nyi == 0) return MI_OK;
    MI_REQUIRE(ctx, xi && yi && zi, "mi_interp2_grid_f64_dev: NULL query/result pointer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(yi) | reinterpret_cast<uintptr_t>(zi);
    MI_REQUIRE(ctx, (a & 7u) == 0, "mi_interp2_grid_f64_dev: pointers must be 8-byte aligned");
    MI_REQUIRE(ctx, nxi < SIZE_MAX / sizeof(AxRec) - nyi && nxi <= SIZE_MAX / sizeof(double) / nyi,
               "mi_interp2_grid_f64_dev: nxi=%zu x nyi=%zu too large", nxi, nyi);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    const mi_status st = mi::ensure_scratch(ctx, 3, (nxi + nyi) * sizeof(AxRec));
    if (st != MI_OK) return st;
    AxRec* cols = (AxRec*)ctx->scratch[3];
    AxRec* rows = cols + nxi;
    hipLaunchKernelGGL(interp2_grid_locate_kernel, dim3(mi::stream_grid(ctx, nxi + nyi, kBlock)), dim3(kBlock), 0,
                       ctx->stream, g->d.ax, g->d.ay, xi, nxi, yi, nyi, cols);
    MI_LAUNCH_CHECK(ctx, "interp2 grid locate kernel");
    const size_t total = nxi * nyi;
    if (nyi < kThinRows) {
        const size_t nwork = (total + kTileRows - 1) / kTileRows;
        const unsigned grid = (unsigned)std::min(nwork, kMaxGrid);
        if ((reinterpret_cast<uintptr_t>(zi) & 15u) == 0)
            hipLaunchKernelGGL((interp2_grid_flat_kernel<true>), dim3(grid), dim3(kBlock), 0, ctx->stream, g->d, cols, rows,
                               (uint32_t)nyi, total, nwork, zi, extrap);
        else
            hipLaunchKernelGGL((interp2_grid_flat_kernel<false>), dim3(grid), dim3(kBlock), 0, ctx->stream, g->d, cols, rows,
                               (uint32_t)nyi, total, nwork, zi, extrap);
    } else {
        // about 32 workgroups of work per CU: strips of columns over the row blocks
        const size_t nrb = (nyi + kTileRows - 1) / kTileRows;
        const size_t target = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * 32;
        const size_t want_strips = std::min(nxi, std::max<size_t>(1, (target + nrb - 1) / nrb));
        const size_t strip = (nxi + want_strips - 1) / want_strips;
        const size_t nwork = nrb * ((nxi + strip - 1) / strip);
        const unsigned grid = (unsigned)std::min(nwork, kMaxGrid);
        if ((reinterpret_cast<uintptr_t>(zi) & 15u) == 0 && (nyi & 1) == 0)
            hipLaunchKernelGGL((interp2_grid_tile_kernel<true>), dim3(grid), dim3(kBlock), 0, ctx->stream, g->d, cols, rows,
                               nxi, nyi, strip, nrb, nwork, zi, extrap);
        else
            hipLaunchKernelGGL((interp2_grid_tile_kernel<false>), dim3(grid), dim3(kBlock), 0, ctx->stream, g->d, cols, rows,
                               nxi, nyi, strip, nrb, nwork, zi, extrap);
    }
    MI_LAUNCH_CHECK(ctx, "interp2 grid kernel");
    return MI_OK;
}

mi_status mi_interp2_grid_f64_host(mi_ctx* ctx, const mi_grid2* g, const double* xi, size_t nxi, const double* yi, size_t nyi,
                                   double* zi, double extrap)
{
    MI_REQUIRE(ctx, ctx && g, "mi_interp2_grid_f64_host: NULL context or grid");
    if (nxi == 0 || nyi == 0) return MI_OK;
    MI_REQUIRE(ctx, xi && yi && zi, "mi_interp2_grid_f64_host: NULL query/result pointer");
    MI_REQUIRE(ctx, nxi <= SIZE_MAX / sizeof(double) / nyi, "mi_interp2_grid_f64_host: nxi=%zu x nyi=%zu too large", nxi, nyi);
    MI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t total = nxi * nyi;
    mi_status st = mi::ensure_scratch(ctx, 0, nxi * sizeof(double));
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 1, nyi * sizeof(double));
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 2, total * sizeof(double));
    if (st != MI_OK) return st;
    double *dx = (double*)ctx->scratch[0], *dy = (double*)ctx->scratch[1], *dz = (double*)ctx->scratch[2];
    const size_t chunk = (size_t)8 << 20;
    if (total <= 2 * chunk) {
        MI_HIP(ctx, hipMemcpyAsync(dx, xi, nxi * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        MI_HIP(ctx, hipMemcpyAsync(dy, yi, nyi * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        st = mi_interp2_grid_f64_dev(ctx, g, dx, nxi, dy, nyi, dz, extrap);
        if (st != MI_OK) return st;
        MI_HIP(ctx, hipMemcpyAsync(zi, dz, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return MI_OK;
    }
    // column chunks of about `chunk` outputs, pinned like mi_interp2_f64_host: the copy back of chunk k (on the aux
    // stream) overlaps the kernels of chunk k+1
    st = mi::ensure_aux_stream(ctx);
    if (st != MI_OK) return st;
    const bool pin_z = mi::pin_host(zi, total * sizeof(double));
    // as in mi_interp2_f64_host: no early return before both streams are drained and the range released
    hipError_t herr = hipMemcpyAsync(dx, xi, nxi * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    const char* what = "upload of the query axes";
    if (herr == hipSuccess) herr = hipMemcpyAsync(dy, yi, nyi * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    const size_t cols = std::max<size_t>(1, chunk / nyi);
    for (size_t c0 = 0; c0 < nxi && herr == hipSuccess && st == MI_OK; c0 += cols) {
        const size_t m = std::min(cols, nxi - c0);
        st = mi_interp2_grid_f64_dev(ctx, g, dx + c0, m, dy, nyi, dz + c0 * nyi, extrap);
        if (st != MI_OK) break;
        herr = hipEventRecord(ctx->aux_event, ctx->stream);
        if (herr == hipSuccess) herr = hipStreamWaitEvent(ctx->aux_stream, ctx->aux_event, 0);
        if (herr == hipSuccess)
            herr = hipMemcpyAsync(zi + c0 * nyi, dz + c0 * nyi, m * nyi * sizeof(double), hipMemcpyDeviceToHost, ctx->aux_stream);
        if (herr != hipSuccess) what = "download of a result chunk";
    }
    const hipError_t e1 = hipStreamSynchronize(ctx->stream), e2 = hipStreamSynchronize(ctx->aux_stream);
    if (pin_z) mi::unpin_host(zi);
    if (st != MI_OK) return st;
    if (herr != hipSuccess) return mi::fail(ctx, MI_ERR_HIP, "mi_interp2_grid_f64_host: %s failed: %s", what, hipGetErrorString(herr));
    MI_HIP(ctx, e1);
    MI_HIP(ctx, e2);
    return MI_OK;
}

}  // extern "C"
