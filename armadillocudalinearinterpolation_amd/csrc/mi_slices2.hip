// Gridded bilinear interpolation over the slices of a cube, Z read where it lies: two axes (mi_axis1: nx and ny nodes), Z a
// stack of nslices column-major ny x nx matrices (leading dimension ldz, slice stride z_slice_stride: the layout of
// arma::cube(ny, nx, nslices).memptr()), queries XI (nxi) and YI (nyi) in any order -> ZI, nslices column-major nyi x nxi
// matrices (ldzi, zi_slice_stride),
//     ZI_s(i, j) == mi_interp2_grid_f64_dev's result at (XI[j], YI[i]) on a mi_grid2 built from (X, Y, Z_s),   bit for bit.
// The loop over the slices of a cube around arma::interp2; a field that changes on the device from step to step, regridded
// without the allocation, the repacking pass and the synchronisation of mi_grid2_create.
//
// The locate / weight / blend code is mi_interp2_eval.hpp's (AxisDev, axis_record, AxRec, blend_records =
// MI_INTERP2_BLEND + flagged_result), used as it is, and this file is compiled with -ffp-contract=off like every other.
//
// Two launches on the context's stream:
//   locate  every XI[j] and YI[i] -> {w, l, r} record, once per call and for all slices, into context scratch slot 3
//           (shared in stream order with mi_interp2_grid_f64_dev and mi_interp1_cols_f64_dev).
//   slices  one kernel.  The work is cut into units = (slice, strip of output columns, block of kTileRows output rows);
//           workgroups stride over the units.  Z has its native layout, so the corners Z(l, c), Z(r, c) are two 8-B
//           elements of one column.  Where they come from is the form, chosen on the host from the shapes and the CU
//           count alone:
//     LDS form    (ny * nx <= kLdsMaxElems, a slice of at most 64 KiB): the slice is read from HBM once, coalesced (16 B
//           per lane when ldz == ny, else 8 B), into one of two LDS buffers as a compact ny x nx image; when the
//           workgroup's next unit lies in another slice, that slice's loads are issued before the current unit is blended
//           (ldz == ny: the first 2 * kPrefetch * 256 elements wait in registers, the rest of a larger slice and every
//           padded slice follow the blend), one barrier per change of slice.  All corners come from LDS.
//     direct form (larger slices): the corners are read from the slice through L2.
//   Inside a unit, either way:
//     tile body (nyi >= kThinRows): a lane owns two output rows and keeps their records in registers across the strip;
//           the column record is wave-uniform; the four corner values per row are reloaded only when the column bracket
//           lx changes, and when the new lx is the old rx the loaded column moves over and one new column is loaded (a
//           wave-uniform branch: with sorted XI every table column is read once per row block).  16-B stores (rows 2t,
//           2t+1) when zi, ldzi and the slice stride allow, else 8-B stores (rows t, t+256).
//     flat body (nyi < kThinRows, where the tile body would leave most lanes idle): a flat index over the strip's
//           outputs, 512 per step, column and row recovered without a division in the loop; 8-B stores.
// Every index into z and zi is 64-bit; no grid dimension depends on nslices, nxi or nyi.
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "mi_interp2_eval.hpp"
#include "mi_axis1.hpp"

namespace mi_slices2 {

using mi_interp2::AxRec;
using mi_interp2::kBlock;

constexpr int kTileRows = 2 * kBlock;          // output rows per unit of the tile body, outputs per step of the flat body
constexpr size_t kThinRows = kBlock;           // nyi below: flat body
constexpr size_t kLdsMaxElems = 8192;          // LDS form up to here: 2 buffers x 8192 x 8 B = 131072 B of the CU's 160 KiB
constexpr int kPrefetch = 8;                   // 16-B vectors per lane held in registers for the next slice (a 64 x 64 slice)
constexpr size_t kMaxFlatStrip = (size_t)1 << 23;   // columns per strip of the flat body: strip * nyi stays below 2^31

typedef __attribute__((address_space(3))) double lds_double;

// process-wide call counts by form (mi_debug_slices2_launches): 0 LDS tile, 1 LDS flat, 2 direct tile, 3 direct flat
std::atomic<size_t> g_launches[4];

__global__ __launch_bounds__(kBlock) void slices2_locate_kernel(AxisDev ax, AxisDev ay, const double* __restrict__ xi, size_t nxi,
                                                                const double* __restrict__ yi, size_t nyi, AxRec* __restrict__ rec)
{
    const size_t n = nxi + nyi;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock)
        rec[k] = k < nxi ? mi_interp2::axis_record(ax, xi[k]) : mi_interp2::axis_record(ay, yi[k - nxi]);
}

// ---- a slice on its way into LDS ------------------------------------------------------------------------------------
// ne = ny * nx elements, compact in LDS (element (i, j) at i + j*ny).  contig (ldz == ny): the slice is one run of ne
// doubles; the 16-B vectors start at its first 16-B aligned element (h = 0 or 1 elements in), vector k holds elements
// h + 2k, h + 2k + 1, k < nv = (ne - h) / 2; the first kPrefetch vectors of a lane wait in registers between issue and
// commit; elements 0 and ne-1 are fetched by every lane (broadcast) and cover the head and an odd tail.  A padded slice
// (ldz > ny) is not held in registers: commit reads element e = i + j*ny from zs[i + j*ldz], 8 B per lane, and the other
// workgroups of the CU cover the latency.
struct SliceLoad {
    d2 v[kPrefetch];
    double first, last;
    int h, nv;
};

__device__ __forceinline__ void slice_issue(SliceLoad& L, const double* __restrict__ zs, int ne, bool contig)
{
    const int t = (int)threadIdx.x;
    L.h = (int)((reinterpret_cast<uintptr_t>(zs) >> 3) & 1u);
    L.nv = contig ? (ne - L.h) >> 1 : 0;
    const d2* p = reinterpret_cast<const d2*>(zs + L.h);
#pragma unroll
    for (int k = 0; k < kPrefetch; ++k) {
        const int j = t + k * kBlock;
        L.v[k].x = 0.0;
        L.v[k].y = 0.0;
        if (j < L.nv) L.v[k] = __builtin_nontemporal_load(p + j);
    }
    L.first = zs[0];
    L.last = contig ? zs[ne - 1] : 0.0;
}

__device__ __forceinline__ void slice_commit(const SliceLoad& L, const double* __restrict__ zs, int ny, int ne, size_t ldz,
                                             bool contig, lds_double* buf)
{
    const int t = (int)threadIdx.x;
    if (contig) {
#pragma unroll
        for (int k = 0; k < kPrefetch; ++k) {
            const int j = t + k * kBlock;
            if (j < L.nv) {
                buf[L.h + 2 * j] = L.v[k].x;
                buf[L.h + 2 * j + 1] = L.v[k].y;
            }
        }
        const d2* p = reinterpret_cast<const d2*>(zs + L.h);
        for (int j = t + kPrefetch * kBlock; j < L.nv; j += kBlock) {   // the rest of a larger slice
            const d2 v = __builtin_nontemporal_load(p + j);
            buf[L.h + 2 * j] = v.x;
            buf[L.h + 2 * j + 1] = v.y;
        }
        if (t == 0) {
            buf[0] = L.first;
            buf[ne - 1] = L.last;
        }
    } else {
        for (int e = t; e < ne; e += kBlock) {
            const unsigned j = (unsigned)e / (unsigned)ny;
            buf[e] = __builtin_nontemporal_load(zs + ((size_t)((unsigned)e - j * (unsigned)ny) + (size_t)j * ldz));
        }
    }
}

// where the corners of one slice come from: its LDS image or the slice itself
template <bool LDSF>
struct Src {
    const double* g;
    size_t ldz;
    lds_double* s;
    int ny;
    __device__ __forceinline__ double at(int i, int j) const
    {
        if constexpr (LDSF) return s[i + j * ny];
        else return g[(size_t)i + (size_t)j * ldz];
    }
};

struct Shape {
    int nx, ny;
    size_t ldz, zstride, nslices;
    size_t nxi, nyi, ldzi, zistride;
    size_t strip, nstrips, nrb, nunits;        // units: u = rb + nrb * (strip index + nstrips * slice)
    int contig;
};

// LDSF: LDS form / direct form.  THIN: flat body / tile body.  VEC (tile body only): 16-B / 8-B stores.
template <bool LDSF, bool THIN, bool VEC>
__global__ __launch_bounds__(kBlock) void slices2_kernel(const AxRec* __restrict__ cols, const AxRec* __restrict__ rows, Shape S,
                                                         const double* __restrict__ z, double* __restrict__ zi, double extrap)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    lds_double* const lds = (lds_double*)smem;
    const int ne = S.nx * S.ny;                              // (LDS form: <= kLdsMaxElems)
    const int bufstride = (ne + 1) & ~1;
    const int t = (int)threadIdx.x;
    const size_t per_slice = S.nrb * S.nstrips;
    int cb = 0;                                              // the LDS buffer that holds slice `held`
    size_t held = (size_t)-1;
    SliceLoad L;
    for (size_t u = blockIdx.x; u < S.nunits; u += gridDim.x) {
        const size_t s = u / per_slice, v = u - s * per_slice;
        const size_t sj = v / S.nrb, rb = v - sj * S.nrb;
        const size_t j0 = sj * S.strip, j1 = min(j0 + S.strip, S.nxi);
        const double* const zs = z + s * S.zstride;
        double* const zis = zi + s * S.zistride;
        size_t snext = s;
        if constexpr (LDSF) {
            if (held != s) {                                 // the workgroup's first unit (later slices arrive below)
                slice_issue(L, zs, ne, S.contig);
                slice_commit(L, zs, S.ny, ne, S.ldz, S.contig, lds + cb * bufstride);
                __syncthreads();
                held = s;
            }
            const size_t un = u + gridDim.x;
            if (un < S.nunits) snext = un / per_slice;
            if (snext != s) slice_issue(L, z + snext * S.zstride, ne, S.contig);   // in flight while this unit is blended
        }
        const Src<LDSF> src = {zs, S.ldz, lds + cb * bufstride, S.ny};
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
                        const AxRec X = cols[j], Y = rows[i];
                        double r = mi_interp2::flagged_result(X.r, Y.r, extrap);
                        if (X.r >= 0 && Y.r >= 0) {
                            d2v lo, hi;
                            lo.x = src.at(Y.l, X.l);
                            hi.x = src.at(Y.r, X.l);
                            lo.y = src.at(Y.l, X.r);
                            hi.y = src.at(Y.r, X.r);
                            r = mi_interp2::blend_records(lo, hi, X, Y, extrap);
                        }
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
                const AxRec R0 = rows[i0];
                const AxRec R1 = has1 ? rows[i1] : R0;
                // (a flagged row has l = 0, r < 0: its corners are read at row 0 and its result replaced)
                const int l0 = R0.l, r0 = max(R0.r, 0), l1 = R1.l, r1 = max(R1.r, 0);
                int lx = -1, rx = -1;
                d2v lo0, hi0, lo1, hi1;                      // .x: column lx, .y: column rx; lo: row l, hi: row r
                lo0.x = lo0.y = hi0.x = hi0.y = lo1.x = lo1.y = hi1.x = hi1.y = 0.0;
                for (size_t j = j0; j < j1; ++j) {
                    const AxRec X = cols[j];                 // wave-uniform
                    double v0, v1;
                    if (X.r < 0) {
                        v0 = mi_interp2::flagged_result(X.r, R0.r, extrap);
                        v1 = mi_interp2::flagged_result(X.r, R1.r, extrap);
                    } else {
                        if (X.l != lx) {                     // uniform branch: a new column bracket
                            if (X.l == rx) {                 // the right column becomes the left one
                                lo0.x = lo0.y; hi0.x = hi0.y; lo1.x = lo1.y; hi1.x = hi1.y;
                            } else {
                                lo0.x = src.at(l0, X.l); hi0.x = src.at(r0, X.l);
                                lo1.x = src.at(l1, X.l); hi1.x = src.at(r1, X.l);
                            }
                            if (X.r == X.l) {                // the last node: one column
                                lo0.y = lo0.x; hi0.y = hi0.x; lo1.y = lo1.x; hi1.y = hi1.x;
                            } else {
                                lo0.y = src.at(l0, X.r); hi0.y = src.at(r0, X.r);
                                lo1.y = src.at(l1, X.r); hi1.y = src.at(r1, X.r);
                            }
                            lx = X.l;
                            rx = X.r;
                        }
                        v0 = mi_interp2::blend_records(lo0, hi0, X, R0, extrap);
                        v1 = mi_interp2::blend_records(lo1, hi1, X, R1, extrap);
                    }
                    double* const col = zis + j * S.ldzi;
                    if (VEC && has1) {
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
        if constexpr (LDSF) {
            if (snext != s) {                                // (uniform)
                cb ^= 1;
                slice_commit(L, z + snext * S.zstride, S.ny, ne, S.ldz, S.contig, lds + cb * bufstride);
                __syncthreads();
                held = snext;
            }
        }
    }
}

template <bool LDSF, bool THIN, bool VEC>
mi_status launch(mi_ctx* ctx, unsigned grid, size_t lds_bytes, const AxRec* cols, const AxRec* rows, const Shape& S, const double* z,
                 double* zi, double extrap)
{
    if (lds_bytes > 64 * 1024)   // above the default limit of dynamic LDS (per device: asked for at every such launch)
        MI_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&slices2_kernel<LDSF, THIN, VEC>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * kLdsMaxElems * sizeof(double))));
    hipLaunchKernelGGL((slices2_kernel<LDSF, THIN, VEC>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, cols, rows, S, z, zi, extrap);
    MI_LAUNCH_CHECK(ctx, "interp2 slices kernel");
    return MI_OK;
}

// a * b, or SIZE_MAX when that overflows
inline size_t mul_sat(size_t a, size_t b) { return (a != 0 && b > SIZE_MAX / a) ? SIZE_MAX : a * b; }

// the argument rules (who: the entry point's name); dev: alignment is checked too
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
    MI_REQUIRE(ctx, zmat <= lim && zimat <= lim && nxi < SIZE_MAX / sizeof(AxRec) - nyi && nyi <= SIZE_MAX / sizeof(double) / nxi,
               "%s: nslices=%zu x (ldz=%zu x nx=%zu, ldzi=%zu x nxi=%zu) too large", who, nslices, ldz, nx, ldzi, nxi);
    if (nslices > 1) {
        MI_REQUIRE(ctx, zstride >= zmat, "%s: z_slice_stride=%zu is smaller than ldz*nx=%zu", who, zstride, zmat);
        MI_REQUIRE(ctx, zistride >= zimat, "%s: zi_slice_stride=%zu is smaller than ldzi*nxi=%zu", who, zistride, zimat);
        MI_REQUIRE(ctx, zstride <= lim && zistride <= lim, "%s: nslices=%zu x (z_slice_stride=%zu, zi_slice_stride=%zu) too large", who,
                   nslices, zstride, zistride);
    }
    return MI_OK;
}

}  // namespace mi_slices2

using namespace mi_slices2;

extern "C" {

size_t mi_debug_slices2_launches(int form)
{
    return (form >= 0 && form < 4) ? g_launches[form].load(std::memory_order_relaxed) : 0;
}

mi_status mi_interp2_slices_f64_dev(mi_ctx* ctx, const mi_axis1* ax, const mi_axis1* ay, const double* z, size_t ldz,
                                    size_t zstride, size_t nslices, const double* xi, size_t nxi, const double* yi, size_t nyi,
                                    double* zi, size_t ldzi, size_t zistride, double extrap)
{
    MI_REQUIRE(ctx, ctx && ax && ay, "mi_interp2_slices_f64_dev: NULL context or axis");
    MI_REQUIRE(ctx, ax->device == ctx->device && ay->device == ctx->device,
               "mi_interp2_slices_f64_dev: the axes live on devices %d and %d, the context on device %d", ax->device, ay->device,
               ctx->device);
    if (nslices == 0 || nxi == 0 || nyi == 0) return MI_OK;
    const size_t nx = ax->n, ny = ay->n;
    mi_status st = check_args(ctx, "mi_interp2_slices_f64_dev", true, nx, ny, z, ldz, zstride, nslices, xi, nxi, yi, nyi, zi, ldzi, zistride);
    if (st != MI_OK) return st;
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    st = mi::ensure_scratch(ctx, 3, (nxi + nyi) * sizeof(AxRec));
    if (st != MI_OK) return st;
    AxRec* cols = (AxRec*)ctx->scratch[3];
    AxRec* rows = cols + nxi;
    hipLaunchKernelGGL(slices2_locate_kernel, dim3(mi::stream_grid(ctx, nxi + nyi, kBlock)), dim3(kBlock), 0, ctx->stream, ax->a, ay->a,
                       xi, nxi, yi, nyi, cols);
    MI_LAUNCH_CHECK(ctx, "interp2 slices locate kernel");

    const size_t cus = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256);
    const bool ldsf = nx <= kLdsMaxElems && ny <= kLdsMaxElems / nx;
    const bool thin = nyi < kThinRows;
    const size_t ne = ldsf ? nx * ny : 0;
    const size_t lds_bytes = 2 * ((ne + 1) & ~(size_t)1) * sizeof(double);
    // workgroups that can be resident: LDS form by its two buffers (160 KiB per CU), at most 8 per CU either way
    const size_t resident = cus * (ldsf ? std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / std::max<size_t>(lds_bytes, 1))) : 8);
    // units: about 4 per resident workgroup when the shape has that much; column strips are cut only as far as that needs
    Shape S;
    S.nx = (int)nx;
    S.ny = (int)ny;
    S.ldz = ldz;
    S.zstride = nslices > 1 ? zstride : 0;
    S.nslices = nslices;
    S.nxi = nxi;
    S.nyi = nyi;
    S.ldzi = ldzi;
    S.zistride = nslices > 1 ? zistride : 0;
    S.contig = ldz == ny;
    S.nrb = thin ? 1 : (nyi + kTileRows - 1) / kTileRows;
    const size_t target = resident * 4;
    const size_t blocks = mul_sat(nslices, S.nrb);
    size_t want_strips = std::min(nxi, std::max<size_t>(1, (target + blocks - 1) / blocks));
    if (thin) want_strips = std::max(want_strips, (nxi + kMaxFlatStrip - 1) / kMaxFlatStrip);
    S.strip = (nxi + want_strips - 1) / want_strips;
    S.nstrips = (nxi + S.strip - 1) / S.strip;
    MI_REQUIRE(ctx, blocks <= SIZE_MAX / S.nstrips, "mi_interp2_slices_f64_dev: nslices=%zu x nxi=%zu x nyi=%zu too large", nslices, nxi, nyi);
    S.nunits = blocks * S.nstrips;
    const unsigned grid = (unsigned)std::min(S.nunits, resident);   // workgroups stride over the units beyond that
    const bool vec = (reinterpret_cast<uintptr_t>(zi) & 15u) == 0 && (ldzi & 1) == 0 && (S.zistride & 1) == 0;
    int form;
    if (ldsf) {
        form = thin ? 1 : 0;
        st = thin ? launch<true, true, false>(ctx, grid, lds_bytes, cols, rows, S, z, zi, extrap)
           : vec  ? launch<true, false, true>(ctx, grid, lds_bytes, cols, rows, S, z, zi, extrap)
                  : launch<true, false, false>(ctx, grid, lds_bytes, cols, rows, S, z, zi, extrap);
    } else {
        form = thin ? 3 : 2;
        st = thin ? launch<false, true, false>(ctx, grid, 0, cols, rows, S, z, zi, extrap)
           : vec  ? launch<false, false, true>(ctx, grid, 0, cols, rows, S, z, zi, extrap)
                  : launch<false, false, false>(ctx, grid, 0, cols, rows, S, z, zi, extrap);
    }
    if (st == MI_OK) g_launches[form].fetch_add(1, std::memory_order_relaxed);
    return st;
}

}  // extern "C"
