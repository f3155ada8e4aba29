// arma::interp2's "nearest" method: scattered pairs and the gridded output on the resident tables of mi_interp2.hip
// (mi_interp2_nearest_f64_dev, mi_interp2_grid_nearest_f64_dev / _host), and the gridded output over the slices of a cube
// read in place (mi_interp2_slices_nearest_f64_dev).  Hand-written HIP for gfx950; memory-bound, no MFMA.
//
// 2-D nearest rule (include/mi355_interp.h): Armadillo's method is separable -- interp2_helper_nearest along one axis,
// then along the other -- so the 1-D rule per axis is the 2-D rule:
//     kx = nearest-rule node of XI[j] on the x axis, ky = nearest-rule node of YI[i] on the y axis, each by
//         l = largest node with X[l] <= q, r = min(l+1, n-1), a = q - X[l]; b = X[r] - q; k = (b < a) ? r : l
//     either coordinate NaN -> NaN; else either coordinate out of range -> extrap; else Z(ky, kx), the stored 64 bits.
// A tie keeps the left node, the decision comes from a and b themselves, and the value is copied: no arithmetic
// touches it, so inf, NaN, -0.0 and denormals in Z reach exactly the outputs whose (ky, kx) is their node.
//
// This unit stands beside the linear twins (mi_interp2.hip, mi_interp2_grid.hip, mi_slices2.hip) rather than inside them:
// tests pin those files on their text, and the committed traffic profiles are stamped with the interp2 family's sources.
// What it needs of them is restated here and held to the originals by tests/test_interp2_nearest_cpu.py: take_right
// (mi_nearest_batched.hip), the constants and the unit arithmetic of the gridded and the slices host sides, mul_sat and
// the check_args rules of the slices call.  mi_interp2_eval.hpp (AxisDev, G2Dev, mi_grid2, axis_locate, axis_node,
// kBlock) and mi_axis1.hpp are used as they are.
//
// Z on a mi_grid2: only the repacked table is resident.  In both layouts the first 8 B of cell (ky, kx) are Z(ky, kx):
//     ((const double*)g.zp)[(g.quads ? 4 : 2) * ((size_t)kx * ny + ky)],   below ny*nx cells, inside the allocation.
//
// Scattered: interp2_kernel's launch shape (one 16-B vector of each coordinate stream per lane when the pointers allow);
//   both axes located, take_right on each, one 8-B gather, non-temporal store.  A flagged query is located at the
//   grid's origin (as locate2 does), so no address is formed from its coordinates.
// Gridded and slices, two launches on the context's stream:
//   locate  every XI[j] and YI[i] -> one int32 (k >= 0 the nearest node, -1 out of range, -2 NaN), 4-B records in
//           context scratch slot 3 -- the record workspace of the linear calls, in stream order with them -- once per
//           call and for all slices.
//   body    the linear call's work split (gridded: row blocks of 512 x strips of columns; slices: units = (slice, column
//           strip, row block)), workgroups striding over it.
//     tile body (nyi >= kThinRows): a lane keeps ky of its two rows in registers; kx[j] is wave-uniform, read on the
//           scalar path; the lane's two values are re-read only when kx changes (a uniform branch: upsampling reuses a
//           table column for every output column that maps to it), and a flagged column leaves them alone.  16-B stores
//           (rows 2t, 2t+1) when zi (and ldzi, the slice stride) allow, else two 8-B stores (rows t, t+256).
//     flat body (nyi < kThinRows): the linear flat kernels' indexing, one 8-B gather per output; gridded: 16-B stores when
//           zi is 16-B aligned; slices: 8-B stores (an output column does not start where the previous one ends).
//   The slices call has the direct (through-L2) form only: one 8-B read per output where the linear call reads four.
// Every index into z and zi is 64-bit; no grid dimension depends on nslices, nxi or nyi.
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "mi_axis1.hpp"
#include "mi_interp2_eval.hpp"

namespace mi_nearest2 {

using mi_interp2::kBlock;

// ---- restated from the gridded and the slices units (the same expressions; a CPU test compares them) ----------------
constexpr int kTileRows = 2 * kBlock;          // output rows per unit of the tile body, outputs per step of the flat body
constexpr size_t kThinRows = kBlock;           // nyi below: flat body
constexpr size_t kMaxGrid = (size_t)1 << 20;
constexpr size_t kMaxFlatStrip = (size_t)1 << 23;   // columns per strip of the flat body: strip * nyi stays below 2^31
// the overflow rules are the linear twins', word for word: they count their 16-B records (sizeof(AxRec)), so the same
// sizes are refused here, where a record is 4 B
constexpr size_t kTwinRecBytes = 16;

// mi_debug_nearest2_launches: 0 scattered; gridded: 1 tile 16-B, 2 tile 8-B, 3 flat 16-B, 4 flat 8-B; slices: 5 tile 16-B,
// 6 tile 8-B, 7 flat
std::atomic<size_t> g_launches[8];
inline void count(int form) { g_launches[form].fetch_add(1, std::memory_order_relaxed); }

// k = (b < a) ? r : l on the values the caller holds for both nodes (mi_nearest_batched.hip)
__device__ __forceinline__ bool take_right(double xl, double xr, double q)
{
    const double a = q - xl;
    const double b = xr - q;
    return b < a;
}

// nearest-rule node of q, q inside [xmin, xmax]
__device__ __forceinline__ int nearest_node(const AxisDev& a, double q)
{
    const int l = mi_interp2::axis_locate(a, q);
    const int r = min(l + 1, a.n - 1);
    return take_right(mi_interp2::axis_node(a, l), mi_interp2::axis_node(a, r), q) ? r : l;
}

// one coordinate of the gridded calls: the node, or -1 out of range / -2 NaN
__device__ __forceinline__ int axis_index(const AxisDev& a, double q)
{
    if (!(q >= a.xmin && q <= a.xmax)) return (q != q) ? -2 : -1;
    return nearest_node(a, q);
}

// result of an output whose column or row record is flagged: NaN wins over out-of-range (flagged_result of the linear calls)
__device__ __forceinline__ double flagged(int kx, int ky, double extrap)
{
    return (kx == -2 || ky == -2) ? __builtin_nan("") : extrap;
}

// the resident table of a mi_grid2 as doubles: Z(ky, kx) = p[cell * (kx*ny + ky)]
struct TableDev {
    const double* p;
    size_t ny;
    size_t cell;           // doubles per cell: 4 (quads) or 2 (column pairs)
};

inline TableDev table_of(const G2Dev& g)
{
    TableDev T;
    T.p = reinterpret_cast<const double*>(g.zp);
    T.ny = (size_t)g.ay.n;
    T.cell = g.quads ? 4 : 2;
    return T;
}

// ---- scattered ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double eval_nearest(const G2Dev& g, double qx, double qy, double extrap)
{
    const bool oor = !(qx >= g.ax.xmin && qx <= g.ax.xmax && qy >= g.ay.xmin && qy <= g.ay.xmax);
    const double sx = oor ? g.ax.xmin : qx;                  // a flagged query: node 0 of both axes, its result replaced
    const double sy = oor ? g.ay.xmin : qy;
    const int kx = nearest_node(g.ax, sx);
    const int ky = nearest_node(g.ay, sy);
    const size_t k = (size_t)kx * (size_t)g.ay.n + (size_t)ky;
    const double v = reinterpret_cast<const double*>(g.zp)[(g.quads ? 4 : 2) * k];
    if (oor) return (qx != qx || qy != qy) ? __builtin_nan("") : extrap;
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void nearest2_kernel(G2Dev g, const double* __restrict__ xq, const double* __restrict__ yq,
                                                          double* __restrict__ zq, size_t nq, double extrap)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (VEC) {
        const size_t nvec = nq >> 1;
        if (i < nvec) {
            const d2 vx = __builtin_nontemporal_load(reinterpret_cast<const d2*>(xq) + i);
            const d2 vy = __builtin_nontemporal_load(reinterpret_cast<const d2*>(yq) + i);
            d2 o;
            o.x = eval_nearest(g, vx.x, vy.x, extrap);
            o.y = eval_nearest(g, vx.y, vy.y, extrap);
            __builtin_nontemporal_store(o, reinterpret_cast<d2*>(zq) + i);
        }
        if ((nq & 1) && i == nvec) __builtin_nontemporal_store(eval_nearest(g, xq[nq - 1], yq[nq - 1], extrap), zq + (nq - 1));
    } else {
        if (i < nq) __builtin_nontemporal_store(eval_nearest(g, xq[i], yq[i], extrap), zq + i);
    }
}

// ---- locate (gridded and slices) --------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void nearest2_locate_kernel(AxisDev ax, AxisDev ay, const double* __restrict__ xi, size_t nxi,
                                                                 const double* __restrict__ yi, size_t nyi, int* __restrict__ idx)
{
    const size_t n = nxi + nyi;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock)
        idx[k] = k < nxi ? axis_index(ax, xi[k]) : axis_index(ay, yi[k - nxi]);
}

// the column records through the constant address space (they were written by the locate kernel, before this one began):
// that keeps their reads on the scalar path (mi_nearest_batched.hip)
typedef __attribute__((address_space(4))) int const_idx;

// Columns [j0, j1) of one row block, tile body.  src(ky, kx): the table value; col(j): the output column at row 0.
// VEC: rows i0, i0+1 -> one 16-B store (has1 always true); else rows i0, i0+256 -> two 8-B stores.
template <bool VEC, typename SrcF, typename ColF>
__device__ __forceinline__ void tile_columns(const int* __restrict__ cols, int ky0, int ky1, bool has1, size_t i0, size_t i1,
                                             size_t j0, size_t j1, double extrap, SrcF src, ColF col)
{
    const const_idx* const ccols = (const const_idx*)cols;
    // (a flagged row reads node 0 and its result is replaced)
    const int r0 = max(ky0, 0), r1 = max(ky1, 0);
    int hx = -1;                                             // the table column held
    double a0 = 0.0, a1 = 0.0;
    for (size_t j = j0; j < j1; ++j) {
        const int kx = ccols[j];                             // wave-uniform
        double v0, v1;
        if (kx < 0) {                                        // the held values survive a flagged column
            v0 = flagged(kx, ky0, extrap);
            v1 = flagged(kx, ky1, extrap);
        } else {
            if (kx != hx) {                                  // uniform branch: a new table column
                hx = kx;
                a0 = src(r0, kx);
                a1 = src(r1, kx);
            }
            v0 = ky0 < 0 ? flagged(kx, ky0, extrap) : a0;
            v1 = ky1 < 0 ? flagged(kx, ky1, extrap) : a1;
        }
        double* const c = col(j);
        if (VEC && has1) {
            d2 o;
            o.x = v0;
            o.y = v1;
            __builtin_nontemporal_store(o, reinterpret_cast<d2*>(c + i0));
        } else {
            __builtin_nontemporal_store(v0, c + i0);
            if (has1) __builtin_nontemporal_store(v1, c + i1);
        }
    }
}

// ---- gridded, on a mi_grid2 -------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kBlock) void nearest2_grid_tile_kernel(TableDev T, const int* __restrict__ cols,
                                                                    const int* __restrict__ rows, size_t nxi, size_t nyi,
                                                                    size_t strip, size_t nrb, size_t nwork, double* __restrict__ zi,
                                                                    double extrap)
{
    for (size_t b = blockIdx.x; b < nwork; b += gridDim.x) {
        const size_t rb = b % nrb, s = b / nrb;             // consecutive workgroups: consecutive row blocks of a strip
        const size_t i0 = rb * kTileRows + (VEC ? 2 * threadIdx.x : threadIdx.x);
        const size_t i1 = i0 + (VEC ? 1 : kBlock);
        if (i0 >= nyi) continue;
        const bool has1 = i1 < nyi;                        // always true in the VEC form (nyi even)
        const int ky0 = rows[i0];
        const int ky1 = has1 ? rows[i1] : ky0;
        const size_t j0 = s * strip, j1 = min(j0 + strip, nxi);
        tile_columns<VEC>(
            cols, ky0, ky1, has1, i0, i1, j0, j1, extrap,
            [&](int ky, int kx) { return T.p[T.cell * ((size_t)kx * T.ny + (size_t)ky)]; },
            [&](size_t j) { return zi + j * nyi; });
    }
}

__device__ __forceinline__ double grid_point(const TableDev& T, const int* __restrict__ cols, const int* __restrict__ rows,
                                             size_t jb, uint32_t ib, uint32_t o, uint32_t nyi, double extrap)
{
    const uint32_t u = ib + o;                               // < nyi + kTileRows: no overflow for a thin output
    const uint32_t dj = u / nyi;
    const int kx = cols[jb + dj], ky = rows[u - dj * nyi];
    if (kx < 0 || ky < 0) return flagged(kx, ky, extrap);
    return T.p[T.cell * ((size_t)kx * T.ny + (size_t)ky)];
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void nearest2_grid_flat_kernel(TableDev T, const int* __restrict__ cols,
                                                                    const int* __restrict__ rows, uint32_t nyi, size_t total,
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
        const double v0 = grid_point(T, cols, rows, jb, ib, o0, nyi, extrap);
        const double v1 = has1 ? grid_point(T, cols, rows, jb, ib, o1, nyi, extrap) : 0.0;
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

// ---- slices -----------------------------------------------------------------------------------------------------------

struct Shape {
    size_t ldz, zstride, nslices;
    size_t nxi, nyi, ldzi, zistride;
    size_t strip, nstrips, nrb, nunits;        // units: u = rb + nrb * (strip index + nstrips * slice)
};

// THIN: flat body / tile body.  VEC (tile body only): 16-B / 8-B stores.
template <bool THIN, bool VEC>
__global__ __launch_bounds__(kBlock) void nearest2_slices_kernel(const int* __restrict__ cols, const int* __restrict__ rows, Shape S,
                                                                 const double* __restrict__ z, double* __restrict__ zi, double extrap)
{
    const int t = (int)threadIdx.x;
    const size_t per_slice = S.nrb * S.nstrips;
    for (size_t u = blockIdx.x; u < S.nunits; u += gridDim.x) {
        const size_t s = u / per_slice, v = u - s * per_slice;
        const size_t sj = v / S.nrb, rb = v - sj * S.nrb;
        const size_t j0 = sj * S.strip, j1 = min(j0 + S.strip, S.nxi);
        const double* const zs = z + s * S.zstride;
        double* const zis = zi + s * S.zistride;
        if constexpr (THIN) {
            // outputs k = i + (j - j0)*nyi of the strip, 512 per step; this lane's two: o = t and t + 256 into the step
            const uint32_t nyi = (uint32_t)S.nyi;
            const uint32_t total = (uint32_t)(j1 - j0) * nyi;
            const uint32_t qs = (uint32_t)kTileRows / nyi, rs = (uint32_t)kTileRows - qs * nyi;   // a step in (columns, rows)
            uint32_t qo[2], ro[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t o = (uint32_t)t + (uint32_t)h * kBlock;
                qo[h] = o / nyi;
                ro[h] = o - qo[h] * nyi;
            }
            uint32_t jb = 0, ib = 0;                           // column and row of the step's first output
            for (uint32_t k0 = 0; k0 < total; k0 += kTileRows) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (k0 + (uint32_t)t + (uint32_t)h * kBlock < total) {
                        uint32_t i = ib + ro[h], dj = jb + qo[h];
                        if (i >= nyi) {
                            i -= nyi;
                            ++dj;
                        }
                        const size_t j = j0 + dj;
                        const int kx = cols[j], ky = rows[i];
                        double r = flagged(kx, ky, extrap);
                        if (kx >= 0 && ky >= 0) r = zs[(size_t)ky + (size_t)kx * S.ldz];
                        __builtin_nontemporal_store(r, zis + j * S.ldzi + i);
                    }
                }
                jb += qs;
                ib += rs;
                if (ib >= nyi) {
                    ib -= nyi;
                    ++jb;
                }
            }
        } else {
            const size_t i0 = rb * kTileRows + (VEC ? 2 * t : t), i1 = i0 + (VEC ? 1 : kBlock);
            if (i0 < S.nyi) {
                const bool has1 = i1 < S.nyi;
                const int ky0 = rows[i0];
                const int ky1 = has1 ? rows[i1] : ky0;
                tile_columns<VEC>(
                    cols, ky0, ky1, has1, i0, i1, j0, j1, extrap,
                    [&](int ky, int kx) { return zs[(size_t)ky + (size_t)kx * S.ldz]; },
                    [&](size_t j) { return zis + j * S.ldzi; });
            }
        }
    }
}

template <bool THIN, bool VEC>
mi_status launch_slices(mi_ctx* ctx, unsigned grid, const int* cols, const int* rows, const Shape& S, const double* z, double* zi,
                        double extrap)
{
    hipLaunchKernelGGL((nearest2_slices_kernel<THIN, VEC>), dim3(grid), dim3(kBlock), 0, ctx->stream, cols, rows, S, z, zi, extrap);
    MI_LAUNCH_CHECK(ctx, "interp2 slices nearest kernel");
    return MI_OK;
}

// a * b, or SIZE_MAX when that overflows (the slices unit)
inline size_t mul_sat(size_t a, size_t b) { return (a != 0 && b > SIZE_MAX / a) ? SIZE_MAX : a * b; }

// the argument rules of the slices call (who: the entry point's name); dev: alignment is checked too
mi_status check_args(const mi_ctx* ctx, const char* who, bool dev, size_t nx, size_t ny, const double* z, size_t ldz, size_t zstride,
                     size_t nslices, const double* xi, size_t nxi, const double* yi, size_t nyi, const double* zi, size_t ldzi,
                     size_t zistride)
{
    MI_REQUIRE(ctx, z && xi && yi && zi, "%s: NULL table/query/result pointer", who);
    if (dev) {
        const uintptr_t al = reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(yi) |
                             reinterpret_cast<uintptr_t>(zi);
        MI_REQUIRE(ctx, (al & 7u) == 0, "%s: z, xi, yi, zi must be 8-byte aligned", who);
    }
    MI_REQUIRE(ctx, ldz >= ny, "%s: ldz=%zu is smaller than the y axis (ny=%zu)", who, ldz, ny);
    MI_REQUIRE(ctx, ldzi >= nyi, "%s: ldzi=%zu is smaller than nyi=%zu", who, ldzi, nyi);
    const size_t zmat = mul_sat(ldz, nx), zimat = mul_sat(ldzi, nxi);
    const size_t lim = SIZE_MAX / sizeof(double) / nslices;
    MI_REQUIRE(ctx, zmat <= lim && zimat <= lim && nxi < SIZE_MAX / kTwinRecBytes - nyi && nyi <= SIZE_MAX / sizeof(double) / nxi,
               "%s: nslices=%zu x (ldz=%zu x nx=%zu, ldzi=%zu x nxi=%zu) too large", who, nslices, ldz, nx, ldzi, nxi);
    if (nslices > 1) {
        MI_REQUIRE(ctx, zstride >= zmat, "%s: z_slice_stride=%zu is smaller than ldz*nx=%zu", who, zstride, zmat);
        MI_REQUIRE(ctx, zistride >= zimat, "%s: zi_slice_stride=%zu is smaller than ldzi*nxi=%zu", who, zistride, zimat);
        MI_REQUIRE(ctx, zstride <= lim && zistride <= lim, "%s: nslices=%zu x (z_slice_stride=%zu, zi_slice_stride=%zu) too large", who,
                   nslices, zstride, zistride);
    }
    return MI_OK;
}

// the records of one call in scratch slot 3, located: cols = the nxi column records, the nyi row records behind them
mi_status locate(mi_ctx* ctx, const AxisDev& ax, const AxisDev& ay, const double* xi, size_t nxi, const double* yi, size_t nyi,
                 const char* what, int** cols)
{
    const mi_status st = mi::ensure_scratch(ctx, 3, (nxi + nyi) * sizeof(int));
    if (st != MI_OK) return st;
    *cols = (int*)ctx->scratch[3];
    hipLaunchKernelGGL(nearest2_locate_kernel, dim3(mi::stream_grid(ctx, nxi + nyi, kBlock)), dim3(kBlock), 0, ctx->stream, ax, ay, xi,
                       nxi, yi, nyi, *cols);
    MI_LAUNCH_CHECK(ctx, what);
    return MI_OK;
}

}  // namespace mi_nearest2

using namespace mi_nearest2;

extern "C" {

size_t mi_debug_nearest2_launches(int form)
{
    return (form >= 0 && form < 8) ? g_launches[form].load(std::memory_order_relaxed) : 0;
}

mi_status mi_interp2_nearest_f64_dev(mi_ctx* ctx, const mi_grid2* g, const double* xq, const double* yq, double* zq, size_t nq,
                                     double extrap)
{
    MI_REQUIRE(ctx, ctx && g, "mi_interp2_nearest_f64_dev: NULL context or grid");
    if (nq == 0) return MI_OK;
    MI_REQUIRE(ctx, xq && yq && zq, "mi_interp2_nearest_f64_dev: NULL query/result pointer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(yq) | reinterpret_cast<uintptr_t>(zq);
    MI_REQUIRE(ctx, (a & 7u) == 0, "mi_interp2_nearest_f64_dev: pointers must be 8-byte aligned");
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    const bool vec = (a & 15u) == 0;
    const size_t lanes = vec ? (nq >> 1) + (nq & 1) : nq;
    const size_t grid = (lanes + kBlock - 1) / kBlock;
    if (grid > 0x7fffffffull) return mi::fail(ctx, MI_ERR_INVALID_ARG, "mi_interp2_nearest_f64_dev: nq=%zu too large for one launch", nq);
    if (vec)
        hipLaunchKernelGGL((nearest2_kernel<true>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, g->d, xq, yq, zq, nq, extrap);
    else
        hipLaunchKernelGGL((nearest2_kernel<false>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, g->d, xq, yq, zq, nq, extrap);
    MI_LAUNCH_CHECK(ctx, "interp2 nearest kernel");
    count(0);
    return MI_OK;
}

mi_status mi_interp2_grid_nearest_f64_dev(mi_ctx* ctx, const mi_grid2* g, const double* xi, size_t nxi, const double* yi, size_t nyi,
                                          double* zi, double extrap)
{
    MI_REQUIRE(ctx, ctx && g, "mi_interp2_grid_nearest_f64_dev: NULL context or grid");
    if (nxi == 0 || nyi == 0) return MI_OK;
    MI_REQUIRE(ctx, xi && yi && zi, "mi_interp2_grid_nearest_f64_dev: NULL query/result pointer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(yi) | reinterpret_cast<uintptr_t>(zi);
    MI_REQUIRE(ctx, (a & 7u) == 0, "mi_interp2_grid_nearest_f64_dev: pointers must be 8-byte aligned");
    MI_REQUIRE(ctx, nxi < SIZE_MAX / kTwinRecBytes - nyi && nxi <= SIZE_MAX / sizeof(double) / nyi,
               "mi_interp2_grid_nearest_f64_dev: nxi=%zu x nyi=%zu too large", nxi, nyi);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    int* cols = nullptr;
    const mi_status st = locate(ctx, g->d.ax, g->d.ay, xi, nxi, yi, nyi, "interp2 grid nearest locate kernel", &cols);
    if (st != MI_OK) return st;
    const int* rows = cols + nxi;
    const TableDev T = table_of(g->d);
    const size_t total = nxi * nyi;
    int form;
    if (nyi < kThinRows) {
        const size_t nwork = (total + kTileRows - 1) / kTileRows;
        const unsigned grid = (unsigned)std::min(nwork, kMaxGrid);
        if ((reinterpret_cast<uintptr_t>(zi) & 15u) == 0) {
            form = 3;
            hipLaunchKernelGGL((nearest2_grid_flat_kernel<true>), dim3(grid), dim3(kBlock), 0, ctx->stream, T, cols, rows, (uint32_t)nyi,
                               total, nwork, zi, extrap);
        } else {
            form = 4;
            hipLaunchKernelGGL((nearest2_grid_flat_kernel<false>), dim3(grid), dim3(kBlock), 0, ctx->stream, T, cols, rows, (uint32_t)nyi,
                               total, nwork, zi, extrap);
        }
    } else {
        // about 32 workgroups of work per CU: strips of columns over the row blocks
        const size_t nrb = (nyi + kTileRows - 1) / kTileRows;
        const size_t target = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * 32;
        const size_t want_strips = std::min(nxi, std::max<size_t>(1, (target + nrb - 1) / nrb));
        const size_t strip = (nxi + want_strips - 1) / want_strips;
        const size_t nwork = nrb * ((nxi + strip - 1) / strip);
        const unsigned grid = (unsigned)std::min(nwork, kMaxGrid);
        if ((reinterpret_cast<uintptr_t>(zi) & 15u) == 0 && (nyi & 1) == 0) {
            form = 1;
            hipLaunchKernelGGL((nearest2_grid_tile_kernel<true>), dim3(grid), dim3(kBlock), 0, ctx->stream, T, cols, rows, nxi, nyi, strip,
                               nrb, nwork, zi, extrap);
        } else {
            form = 2;
            hipLaunchKernelGGL((nearest2_grid_tile_kernel<false>), dim3(grid), dim3(kBlock), 0, ctx->stream, T, cols, rows, nxi, nyi, strip,
                               nrb, nwork, zi, extrap);
        }
    }
    MI_LAUNCH_CHECK(ctx, "interp2 grid nearest kernel");
    count(form);
    return MI_OK;
}

mi_status mi_interp2_grid_nearest_f64_host(mi_ctx* ctx, const mi_grid2* g, const double* xi, size_t nxi, const double* yi, size_t nyi,
                                           double* zi, double extrap)
{
    MI_REQUIRE(ctx, ctx && g, "mi_interp2_grid_nearest_f64_host: NULL context or grid");
    if (nxi == 0 || nyi == 0) return MI_OK;
    MI_REQUIRE(ctx, xi && yi && zi, "mi_interp2_grid_nearest_f64_host: NULL query/result pointer");
    MI_REQUIRE(ctx, nxi <= SIZE_MAX / sizeof(double) / nyi, "mi_interp2_grid_nearest_f64_host: nxi=%zu x nyi=%zu too large", nxi, nyi);
    MI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t total = nxi * nyi;
    // up to 2 x 8 Mi outputs in one piece; beyond that column chunks of about 8 Mi outputs, each one the same three steps
    // (device call into slot 2, download) on the context's own stream.  No pinning and no second stream: the path is
    // PCIe-bound either way.
    const size_t chunk = (size_t)8 << 20;
    const size_t cols = total <= 2 * chunk ? nxi : std::max<size_t>(1, chunk / nyi);
    mi_status st = mi::ensure_scratch(ctx, 0, nxi * sizeof(double));
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 1, nyi * sizeof(double));
    if (st == MI_OK) st = mi::ensure_scratch(ctx, 2, cols * nyi * sizeof(double));
    if (st != MI_OK) return st;
    double *dx = (double*)ctx->scratch[0], *dy = (double*)ctx->scratch[1], *dz = (double*)ctx->scratch[2];
    MI_HIP(ctx, hipMemcpyAsync(dx, xi, nxi * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(ctx, hipMemcpyAsync(dy, yi, nyi * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    for (size_t c0 = 0; c0 < nxi; c0 += cols) {
        const size_t m = std::min(cols, nxi - c0);
        st = mi_interp2_grid_nearest_f64_dev(ctx, g, dx + c0, m, dy, nyi, dz, extrap);
        if (st != MI_OK) break;
        // (in stream order: the next chunk's kernels overwrite dz only after this copy has read it)
        const hipError_t e = hipMemcpyAsync(zi + c0 * nyi, dz, m * nyi * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->stream);
            return mi::fail(ctx, MI_ERR_HIP, "mi_interp2_grid_nearest_f64_host: download of a result chunk failed: %s", hipGetErrorString(e));
        }
    }
    const hipError_t e1 = hipStreamSynchronize(ctx->stream);   // also after a failed chunk: nothing of this call is left in flight
    if (st != MI_OK) return st;
    MI_HIP(ctx, e1);
    return MI_OK;
}

mi_status mi_interp2_slices_nearest_f64_dev(mi_ctx* ctx, const mi_axis1* ax, const mi_axis1* ay, const double* z, size_t ldz,
                                            size_t zstride, size_t nslices, const double* xi, size_t nxi, const double* yi,
                                            size_t nyi, double* zi, size_t ldzi, size_t zistride, double extrap)
{
    MI_REQUIRE(ctx, ctx && ax && ay, "mi_interp2_slices_nearest_f64_dev: NULL context or axis");
    MI_REQUIRE(ctx, ax->device == ctx->device && ay->device == ctx->device,
               "mi_interp2_slices_nearest_f64_dev: the axes live on devices %d and %d, the context on device %d", ax->device, ay->device,
               ctx->device);
    if (nslices == 0 || nxi == 0 || nyi == 0) return MI_OK;
    const size_t nx = ax->n, ny = ay->n;
    mi_status st = check_args(ctx, "mi_interp2_slices_nearest_f64_dev", true, nx, ny, z, ldz, zstride, nslices, xi, nxi, yi, nyi, zi, ldzi, zistride);
    if (st != MI_OK) return st;
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    int* cols = nullptr;
    st = locate(ctx, ax->a, ay->a, xi, nxi, yi, nyi, "interp2 slices nearest locate kernel", &cols);
    if (st != MI_OK) return st;
    const int* rows = cols + nxi;

    const size_t cus = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256);
    const bool thin = nyi < kThinRows;
    // workgroups that can be resident: 8 per CU (the direct form of the linear call)
    const size_t resident = cus * 8;
    // units: about 4 per resident workgroup when the shape has that much; column strips are cut only as far as that needs
    Shape S;
    S.ldz = ldz;
    S.zstride = nslices > 1 ? zstride : 0;
    S.nslices = nslices;
    S.nxi = nxi;
    S.nyi = nyi;
    S.ldzi = ldzi;
    S.zistride = nslices > 1 ? zistride : 0;
    S.nrb = thin ? 1 : (nyi + kTileRows - 1) / kTileRows;
    const size_t target = resident * 4;
    const size_t blocks = mul_sat(nslices, S.nrb);
    size_t want_strips = std::min(nxi, std::max<size_t>(1, (target + blocks - 1) / blocks));
    if (thin) want_strips = std::max(want_strips, (nxi + kMaxFlatStrip - 1) / kMaxFlatStrip);
    S.strip = (nxi + want_strips - 1) / want_strips;
    S.nstrips = (nxi + S.strip - 1) / S.strip;
    MI_REQUIRE(ctx, blocks <= SIZE_MAX / S.nstrips, "mi_interp2_slices_nearest_f64_dev: nslices=%zu x nxi=%zu x nyi=%zu too large", nslices, nxi, nyi);
    S.nunits = blocks * S.nstrips;
    const unsigned grid = (unsigned)std::min(S.nunits, resident);   // workgroups stride over the units beyond that
    const bool vec = (reinterpret_cast<uintptr_t>(zi) & 15u) == 0 && (ldzi & 1) == 0 && (S.zistride & 1) == 0;
    const int form = thin ? 7 : vec ? 5 : 6;
    st = thin ? launch_slices<true, false>(ctx, grid, cols, rows, S, z, zi, extrap)
       : vec  ? launch_slices<false, true>(ctx, grid, cols, rows, S, z, zi, extrap)
              : launch_slices<false, false>(ctx, grid, cols, rows, S, z, zi, extrap);
    if (st == MI_OK) count(form);
    return st;
}

}  // extern "C"
