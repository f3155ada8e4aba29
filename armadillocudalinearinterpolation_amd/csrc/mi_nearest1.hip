// arma::interp1's "nearest" method on MI355X (gfx950): table lookup over a resident mi_grid1 (the handles, table modes
// and closed forms of the linear calls, as they are) and over the columns of a matrix (one mi_axis1, many Y).
// Hand-written HIP; memory-bound, no MFMA.
//
// Nearest rule (include/mi355_interp.h): the bracket l is the linear call's (largest node with X[l] <= q), r = min(l+1, n-1),
//     a = q - X[l];  b = X[r] - q;  k = (b < a) ? r : l;  out = Y[k]
// -- a tie keeps the left node, the decision comes from a and b themselves (never from the rounded weight a/(a+b)), and
// the value is copied: no arithmetic touches it.  q outside [X[0], X[n-1]] -> extrap, q = NaN -> NaN.
//
// The evaluator below stands beside mi_interp1::eval_batch_from (mi_interp1_eval.hpp) rather than inside it: the files
// of the interp1 kernel family are pinned by digest (tests/test_interp1_cols_cpu.py), so the bracket code is restated
// here step for step from that function's guess expressions, with its unode / load_node helpers used as they are.
//
// Table kernels (one evaluator, so the three forms agree bit for bit):
//   nearest1_vec_kernel      streaming: 16-B query and result vectors, kVecVpl vectors per lane, full-size grid.
//   nearest1_lds_kernel      the whole table in LDS (the linear LDS kernel's window and nq threshold).
//   nearest1_scalar_kernel   pointers that are 8-B but not 16-B aligned.
// Mode 0 (closed-form abscissae) gathers ONE 8-B value per query after the select -- the linear blend needs 16 B.
// Kernel choice: alignment, table size and mi_ctx_set_query_order only; the order probe's mailbox and flags are never
// read or written here, and there is no region-sweep form.
//
// Columns (mi_interp1_cols_nearest_f64_dev), two launches as in mi_cols1.hip:
//   locate   every XI[i] -> one int32 (k >= 0 the nearest node, -1 out of range, -2 NaN) into context scratch slot 3,
//            the record workspace the linear calls use, in stream order.
//   columns  mi_cols1.hip's unit structure: a row block of kRowBlock outputs x a run of columns, the lane's indices in
//            registers across the run.  LDS form (n <= kLdsMaxN): a column is staged once into one of two LDS buffers
//            (mi_paired_cols.hpp's col_issue / col_commit without the X validation); direct form: col[k] through L2.
//            Coalesced non-temporal stores, 16 B where yi and ldyi allow, else 8 B.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>

#include "mi_axis1.hpp"
#include "mi_interp1_eval.hpp"
#include "mi_paired_cols.hpp"

namespace mi_nearest1 {

using namespace mi_interp1;

// The launch shapes and the LDS window of the linear kernels, restated: mi_interp1_stream.hpp, which holds them, also
// defines the (non-template) order-probe kernel and can be part of one translation unit only.
// tests/test_interp1_nearest_cpu.py holds these to that header's values.
constexpr int kBlock = 256;
constexpr int kVecVpl = 2;                          // 16-B vectors per lane
constexpr int kLdsBlock = 1024;
constexpr size_t kLdsMaxTableBytes = 128 * 1024;
constexpr size_t kLdsMinTableBytes0 = 32 * 1024;    // mode 0: smaller tables live in L1
constexpr size_t kLdsMinTableBytes3 = 2 * 1024;     // mode 3
constexpr size_t kLdsQueriesPerBlock = 1u << 17;
static_assert(kBlock == mi_paired::kBlock, "the column staging helpers assume this workgroup size");

// k = (b < a) ? r : l on the values the caller holds for both nodes
__device__ __forceinline__ bool take_right(double xl, double xr, double q)
{
    const double a = q - xl;
    const double b = xr - q;
    return b < a;
}

// eval_batch_from's shape: all guesses first, then all gathers, then the rare walks and the select
template <int MODE, int NQ, int FORMULA = 0, bool WIN = false, bool LDSY = false>
__device__ __forceinline__ void nearest_batch_from(const G1Dev& g, const double (&q)[NQ], double (&out)[NQ], double extrap,
                                                   const double* ytab)
{
    double qs[NQ];
    int l[NQ];
    bool oor[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        oor[k] = !(q[k] >= g.xmin && q[k] <= g.xmax);   // true for NaN as well
        qs[k] = oor[k] ? g.xmin : q[k];
    }
    if constexpr (MODE == 0) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            int i = (int)((qs[k] - g.x0) * g.scale);
            i = min(max(i, 0), g.n - 1);
            double a = unode<FORMULA>(g, i), b = unode<FORMULA>(g, min(i + 1, g.n - 1));
            while (i > 0 && a > qs[k]) { --i; b = a; a = unode<FORMULA>(g, i); }
            while (i < g.n - 1 && b <= qs[k]) { ++i; a = b; b = unode<FORMULA>(g, min(i + 1, g.n - 1)); }
            l[k] = take_right(a, b, qs[k]) ? min(i + 1, g.n - 1) : i;   // the nearest node
        }
#pragma unroll
        for (int k = 0; k < NQ; ++k) {   // one 8-B gather per query
            if constexpr (LDSY) out[k] = *(const lds_cdouble*)(ytab + l[k]);
            else out[k] = ytab[l[k]];
        }
    } else if constexpr (MODE == 3) {
        d2 nm[NQ], n0[NQ], n1[NQ];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const int i = (int)((qs[k] - g.gorg) * g.scale);
            l[k] = min(max(i, 0), g.n - 1);
        }
        if constexpr (WIN) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                nm[k] = load_node<LDSY>(ytab, max(l[k] - 1, 0));
                n0[k] = load_node<LDSY>(ytab, l[k]);
                n1[k] = load_node<LDSY>(ytab, l[k] + 1);        // index n is the padding node (a copy of node n-1)
            }
        } else {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                n0[k] = load_node<LDSY>(ytab, l[k]);
                n1[k] = load_node<LDSY>(ytab, l[k] + 1);
            }
#pragma unroll   // node G-1 only where the comparison asks for it
            for (int k = 0; k < NQ; ++k) nm[k] = (qs[k] < n0[k].x) ? load_node<LDSY>(ytab, max(l[k] - 1, 0)) : n0[k];
        }
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const bool down = qs[k] < n0[k].x;   // then l = G-1 >= 0 (G = 0 has X_0 <= q)
            const d2 a = down ? nm[k] : n0[k], b = down ? n0[k] : n1[k];
            out[k] = take_right(a.x, b.x, qs[k]) ? b.y : a.y;
        }
    } else {
        d2 n0[NQ], n1[NQ];
        if constexpr (MODE == 1) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                int i = (int)((qs[k] - g.xmin) * g.scale);
                l[k] = min(max(i, 0), g.n - 2);
            }
        } else {
            uint32_t lo[NQ], hi[NQ];
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                int b = (int)((qs[k] - g.xmin) * g.scale);
                b = min(max(b, 0), g.nb - 1);
                lo[k] = g.s[b];
                hi[k] = g.s[b + 1];
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                uint32_t a = lo[k], c = hi[k];       // bracket index is in [a, c]
                while (c > a) {
                    const uint32_t mid = (a + c + 1u) >> 1;
                    if (g.nodes[mid].x <= qs[k]) a = mid; else c = mid - 1u;
                }
                l[k] = (int)a;
            }
        }
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            n0[k] = g.nodes[l[k]];
            n1[k] = g.nodes[l[k] + 1];
        }
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            if constexpr (MODE == 1) {
                int i = l[k];
                while (qs[k] < n0[k].x && i > 0) { --i; n1[k] = n0[k]; n0[k] = g.nodes[i]; }
                while (qs[k] >= n1[k].x && i < g.n - 1) { ++i; n0[k] = n1[k]; n1[k] = g.nodes[i + 1]; }
            }
            out[k] = take_right(n0[k].x, n1[k].x, qs[k]) ? n1[k].y : n0[k].y;
        }
    }
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        if (oor[k]) out[k] = (q[k] != q[k]) ? __builtin_nan("") : extrap;
    }
}

template <int MODE, int NQ, int FORMULA = 0, bool WIN = false>
__device__ __forceinline__ void nearest_batch(const G1Dev& g, const double (&q)[NQ], double (&out)[NQ], double extrap)
{
    nearest_batch_from<MODE, NQ, FORMULA, WIN>(g, q, out, extrap, MODE == 0 ? g.y : reinterpret_cast<const double*>(g.nodes));
}

// interp1_vec_kernel's shape (mi_interp1_stream.hpp) without the gate and the probe
template <int MODE, int FORMULA>
__global__ __launch_bounds__(kBlock) void nearest1_vec_kernel(G1Dev g, const double* __restrict__ xq, double* __restrict__ yq,
                                                              size_t nq, double extrap)
{
    constexpr int VPL = kVecVpl;
    const size_t nvec = nq >> 1;
    const size_t base = (size_t)blockIdx.x * (kBlock * VPL) + threadIdx.x;
    double q[2 * VPL], r[2 * VPL];
    const bool full = base + (size_t)(VPL - 1) * kBlock < nvec;
    if (full) {
#pragma unroll
        for (int u = 0; u < VPL; ++u) {
            const d2 v = __builtin_nontemporal_load(reinterpret_cast<const d2*>(xq) + base + (size_t)u * kBlock);
            q[2 * u] = v.x;
            q[2 * u + 1] = v.y;
        }
        nearest_batch<MODE, 2 * VPL, FORMULA, true>(g, q, r, extrap);
#pragma unroll
        for (int u = 0; u < VPL; ++u) {
            d2 o;
            o.x = r[2 * u];
            o.y = r[2 * u + 1];
            __builtin_nontemporal_store(o, reinterpret_cast<d2*>(yq) + base + (size_t)u * kBlock);
        }
    } else {
        for (int u = 0; u < VPL; ++u) {
            const size_t i = base + (size_t)u * kBlock;
            if (i < nvec) {
                const d2 v = __builtin_nontemporal_load(reinterpret_cast<const d2*>(xq) + i);
                double q1[2] = {v.x, v.y}, r1[2];
                nearest_batch<MODE, 2, FORMULA>(g, q1, r1, extrap);
                d2 o;
                o.x = r1[0];
                o.y = r1[1];
                __builtin_nontemporal_store(o, reinterpret_cast<d2*>(yq) + i);
            } else if ((nq & 1) && i == nvec) {   // odd tail element, handled by the first lane past the vectors
                double q1[1] = {xq[nq - 1]}, r1[1];
                nearest_batch<MODE, 1, FORMULA>(g, q1, r1, extrap);
                yq[nq - 1] = r1[0];
            }
        }
    }
}

// interp1_lds_kernel's shape: one 1024-lane workgroup copies the table and evaluates kLdsQueriesPerBlock queries
template <int MODE, int FORMULA>
__global__ __launch_bounds__(kLdsBlock) void nearest1_lds_kernel(G1Dev g, const double* __restrict__ xq, double* __restrict__ yq,
                                                                 size_t nq, double extrap)
{
    extern __shared__ __attribute__((aligned(16))) double ys[];
    {   // n + 1 entries (padding node) of 8 B (mode 0: Y) or 16 B (mode 3: {x,y})
        const double* src = MODE == 0 ? g.y : reinterpret_cast<const double*>(g.nodes);
        const int words = (MODE == 0 ? 1 : 2) * (g.n + 1);
        for (int i = threadIdx.x; i < words; i += kLdsBlock) ys[i] = src[i];
    }
    __syncthreads();
    const size_t q0 = (size_t)blockIdx.x * kLdsQueriesPerBlock;
    const size_t q1 = min(nq, q0 + kLdsQueriesPerBlock);
    const size_t nvec = (q1 - q0) >> 1;                                     // q0 is even: 16-B aligned vectors
    const d2* in = reinterpret_cast<const d2*>(xq + q0);
    d2* out = reinterpret_cast<d2*>(yq + q0);
    size_t v = threadIdx.x;
    for (; v + kLdsBlock < nvec; v += 2 * kLdsBlock) {                      // two vectors (four queries) per lane per trip
        const d2 a = __builtin_nontemporal_load(in + v), b = __builtin_nontemporal_load(in + v + kLdsBlock);
        const double q[4] = {a.x, a.y, b.x, b.y};
        double r[4];
        nearest_batch_from<MODE, 4, FORMULA, true, true>(g, q, r, extrap, ys);
        d2 o0, o1;
        o0.x = r[0]; o0.y = r[1]; o1.x = r[2]; o1.y = r[3];
        __builtin_nontemporal_store(o0, out + v);
        __builtin_nontemporal_store(o1, out + v + kLdsBlock);
    }
    for (; v < nvec; v += kLdsBlock) {
        const d2 a = __builtin_nontemporal_load(in + v);
        const double q[2] = {a.x, a.y};
        double r[2];
        nearest_batch_from<MODE, 2, FORMULA, true, true>(g, q, r, extrap, ys);
        d2 o;
        o.x = r[0]; o.y = r[1];
        __builtin_nontemporal_store(o, out + v);
    }
    if (((q1 - q0) & 1) && threadIdx.x == 0) {                              // odd tail element of the last chunk
        const double q[1] = {xq[q1 - 1]};
        double r[1];
        nearest_batch_from<MODE, 1, FORMULA, true, true>(g, q, r, extrap, ys);
        yq[q1 - 1] = r[0];
    }
}

template <int MODE, int FORMULA>
__global__ __launch_bounds__(kBlock) void nearest1_scalar_kernel(G1Dev g, const double* __restrict__ xq, double* __restrict__ yq,
                                                                 size_t nq, double extrap)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < nq) {
        double q[1] = {xq[i]}, r[1];
        nearest_batch<MODE, 1, FORMULA>(g, q, r, extrap);
        yq[i] = r[0];
    }
}

// mi_debug_nearest_launches: 0 streaming, 1 table in LDS, 2 scalar, 3 columns LDS form, 4 columns direct form
std::atomic<size_t> g_launches[5];
inline void count(int form) { g_launches[form].fetch_add(1, std::memory_order_relaxed); }

template <int MODE, int FORMULA = 0>
mi_status launch_mode(mi_ctx* ctx, const G1Dev& d, const double* xq, double* yq, size_t nq, double extrap)
{
    const bool aligned = ((reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(yq)) & 15u) == 0;
    if (!aligned) {
        const size_t grid = (nq + kBlock - 1) / kBlock;
        if (grid > 0x7fffffffull) return mi::fail(ctx, MI_ERR_INVALID_ARG, "mi_interp1_nearest_f64_dev: nq=%zu too large for one launch", nq);
        hipLaunchKernelGGL((nearest1_scalar_kernel<MODE, FORMULA>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, d, xq, yq, nq,
                           extrap);
        MI_LAUNCH_CHECK(ctx, "interp1 nearest scalar kernel");
        count(2);
        return MI_OK;
    }
    if constexpr (MODE == 0 || MODE == 3) {
        // the linear dispatcher's window (mi_interp1.hip, launch_mode): unordered queries over a table that fits LDS;
        // AUTO takes it too -- the verdict of the order probe is the linear calls' and is not consulted here
        const size_t ybytes = ((size_t)d.n + 1) * (MODE == 0 ? sizeof(double) : sizeof(d2));
        if (ctx->query_order != MI_QUERIES_ORDERED && ybytes > (MODE == 0 ? kLdsMinTableBytes0 : kLdsMinTableBytes3) && ybytes <= kLdsMaxTableBytes &&
            nq >= 8 * kLdsQueriesPerBlock && std::isfinite(d.xmax - d.xmin) && (d.xmax - d.xmin) > 0.0) {
            MI_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&nearest1_lds_kernel<MODE, FORMULA>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMaxTableBytes));
            const size_t grid = (nq + kLdsQueriesPerBlock - 1) / kLdsQueriesPerBlock;
            hipLaunchKernelGGL((nearest1_lds_kernel<MODE, FORMULA>), dim3((unsigned)grid), dim3(kLdsBlock), ybytes, ctx->stream, d, xq,
                               yq, nq, extrap);
            MI_LAUNCH_CHECK(ctx, "interp1 nearest LDS-table kernel");
            count(1);
            return MI_OK;
        }
    }
    const size_t lanes = (nq >> 1) + (nq & 1);                 // one lane per vector (+ one for an odd tail)
    const size_t per_block = (size_t)kBlock * kVecVpl;
    const size_t grid = (lanes + per_block - 1) / per_block;
    if (grid > 0x7fffffffull) return mi::fail(ctx, MI_ERR_INVALID_ARG, "mi_interp1_nearest_f64_dev: nq=%zu too large for one launch", nq);
    hipLaunchKernelGGL((nearest1_vec_kernel<MODE, FORMULA>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, d, xq, yq, nq, extrap);
    MI_LAUNCH_CHECK(ctx, "interp1 nearest streaming kernel");
    count(0);
    return MI_OK;
}

// ---- columns ------------------------------------------------------------------------------------------------------
using mi_paired::ColLoad;
using mi_paired::lds_double;

constexpr int kRecIter = 4;                          // 512-row slices per row block: 8 indices per lane in registers
constexpr size_t kRowBlock = 2 * kBlock * kRecIter;  // 2048 outputs of one column per unit (mi_cols1.hip's)
constexpr size_t kLdsMaxN = 8192;                    // LDS form up to here: 2 x (n + 2) x 8 B <= 131104 B of the CU's 160 KiB
constexpr int kNoRow = -3;

__global__ __launch_bounds__(kBlock) void nearest_cols_locate_kernel(AxisDev ax, const double* __restrict__ xi, size_t nxi,
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

// LDSF: LDS form / direct form.  VEC: 16-B stores (yi 16-B aligned, ldyi even) / 8-B stores.
// unit u = (row block u % nrb, column run u / nrb), as in cols1_kernel
template <bool LDSF, bool VEC>
__global__ __launch_bounds__(kBlock) void nearest_cols_kernel(const int* __restrict__ idx, int n, const double* __restrict__ y,
                                                              size_t ldy, size_t ncols, size_t run, size_t nxi, size_t nrb,
                                                              size_t nunits, double* __restrict__ yi, size_t ldyi, double extrap)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    lds_double* const lds = (lds_double*)smem;
    const int stride = n + 2;                               // elements per LDS buffer (n + 1 used)
    const int t = (int)threadIdx.x;
    for (size_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const size_t rb = u % nrb, s = u / nrb;
        const size_t c0 = s * run, c1 = min(c0 + run, ncols);
        const size_t row0 = rb * kRowBlock;
        // this lane's rows, (ia, ib) + j*512 for j < kRecIter, and their node indices
        const size_t ia = row0 + (VEC ? 2 * t : t), ib = ia + (VEC ? 1 : kBlock);
        int ka[kRecIter], kb[kRecIter];
#pragma unroll
        for (int j = 0; j < kRecIter; ++j) {
            const size_t o = (size_t)j * (2 * kBlock);
            ka[j] = (ia + o < nxi) ? idx[ia + o] : kNoRow;
            kb[j] = (ib + o < nxi) ? idx[ib + o] : kNoRow;
        }
        ColLoad L;
        if constexpr (LDSF) {
            // (every column of the previous unit ended on a barrier: both buffers are free)
            const double* col = y + c0 * ldy;
            mi_paired::col_issue<false>(L, col, n);
            mi_paired::col_commit<false, false>(L, col, n, lds);
            __syncthreads();
        }
        for (size_t c = c0; c < c1; ++c) {
            lds_double* const cur = lds + (size_t)((c - c0) & 1) * stride;
            lds_double* const nxt = lds + (size_t)(((c - c0) & 1) ^ 1) * stride;
            const double* const col = y + c * ldy;
            const bool more = c + 1 < c1;
            if constexpr (LDSF) {
                if (more) mi_paired::col_issue<false>(L, col + ldy, n);       // in flight while this column is served
            }
            double* const out = yi + c * ldyi;
#pragma unroll
            for (int j = 0; j < kRecIter; ++j) {
                if (ka[j] == kNoRow) continue;
                const bool hb = kb[j] != kNoRow;
                double* const oa = out + ia + (size_t)j * (2 * kBlock);
                double va, vb;
                if constexpr (LDSF) {
                    va = cur[max(ka[j], 0)];
                    vb = cur[max(kb[j], 0)];
                } else {
                    va = col[max(ka[j], 0)];
                    vb = col[max(kb[j], 0)];
                }
                if (ka[j] < 0) va = (ka[j] == -2) ? __builtin_nan("") : extrap;
                if (kb[j] < 0) vb = (kb[j] == -2) ? __builtin_nan("") : extrap;
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
                if (more) mi_paired::col_commit<false, false>(L, col + ldy, n, nxt);
                __syncthreads();
            }
        }
    }
}

template <bool LDSF, bool VEC>
mi_status launch_cols(mi_ctx* ctx, unsigned grid, size_t lds_bytes, const int* idx, int n, const double* y, size_t ldy, size_t ncols,
                      size_t run, size_t nxi, size_t nrb, size_t nunits, double* yi, size_t ldyi, double extrap)
{
    if (lds_bytes > 64 * 1024)   // above the default limit of dynamic LDS (per device: asked for at every such launch)
        MI_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&nearest_cols_kernel<LDSF, VEC>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)((kLdsMaxN + 2) * 2 * sizeof(double))));
    hipLaunchKernelGGL((nearest_cols_kernel<LDSF, VEC>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, idx, n, y, ldy, ncols, run,
                       nxi, nrb, nunits, yi, ldyi, extrap);
    MI_LAUNCH_CHECK(ctx, "interp1 nearest cols kernel");
    count(LDSF ? 3 : 4);
    return MI_OK;
}

}  // namespace mi_nearest1

using namespace mi_nearest1;

extern "C" {

size_t mi_debug_nearest_launches(int form)
{
    return (form >= 0 && form < 5) ? g_launches[form].load(std::memory_order_relaxed) : 0;
}

mi_status mi_interp1_nearest_f64_dev(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq, size_t nq, double extrap)
{
    MI_REQUIRE(ctx, ctx && g, "mi_interp1_nearest_f64_dev: NULL context or grid");
    if (nq == 0) return MI_OK;
    MI_REQUIRE(ctx, xq && yq, "mi_interp1_nearest_f64_dev: NULL query/result pointer");
    MI_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(yq)) & 7u) == 0,
               "mi_interp1_nearest_f64_dev: pointers must be 8-byte aligned");
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    switch (g->mode) {
        case 0:
            if (g->d.formula == 1) return launch_mode<0, 1>(ctx, g->d, xq, yq, nq, extrap);
            if (g->d.formula == 2) return launch_mode<0, 2>(ctx, g->d, xq, yq, nq, extrap);
            if (g->d.formula == 3) return launch_mode<0, 3>(ctx, g->d, xq, yq, nq, extrap);
            return launch_mode<0, 0>(ctx, g->d, xq, yq, nq, extrap);
        case 1:
            if (g->d.centred) return launch_mode<3>(ctx, g->d, xq, yq, nq, extrap);
            return launch_mode<1>(ctx, g->d, xq, yq, nq, extrap);
        default: return launch_mode<2>(ctx, g->d, xq, yq, nq, extrap);
    }
}

// The chunked, pinned path of mi_interp1_f64_host (mi_interp1.hip) around the nearest device call.  A second copy and
// not a shared one: that file belongs to the digest-pinned interp1 family.  No error-path hook here.
mi_status mi_interp1_nearest_f64_host(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq, size_t nq, double extrap)
{
    MI_REQUIRE(ctx, ctx && g, "mi_interp1_nearest_f64_host: NULL context or grid");
    if (nq == 0) return MI_OK;
    MI_REQUIRE(ctx, xq && yq, "mi_interp1_nearest_f64_host: NULL query/result pointer");
    MI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = nq * sizeof(double);
    mi_status st = mi::ensure_scratch(ctx, 0, bytes);
    if (st != MI_OK) return st;
    st = mi::ensure_scratch(ctx, 1, bytes);
    if (st != MI_OK) return st;
    const size_t chunk = (size_t)8 << 20;   // as mi_interp1_f64_host: small calls keep the single-shot form
    if (nq <= 2 * chunk) {
        MI_HIP(ctx, hipMemcpyAsync(ctx->scratch[0], xq, bytes, hipMemcpyHostToDevice, ctx->stream));
        st = mi_interp1_nearest_f64_dev(ctx, g, (const double*)ctx->scratch[0], (double*)ctx->scratch[1], nq, extrap);
        if (st != MI_OK) return st;
        MI_HIP(ctx, hipMemcpyAsync(yq, ctx->scratch[1], bytes, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return MI_OK;
    }
    st = mi::ensure_aux_stream(ctx);
    if (st != MI_OK) return st;
    const bool pin_in = mi::pin_host(xq, bytes), pin_out = mi::pin_host(yq, bytes);
    const double* din = (const double*)ctx->scratch[0];
    double* dout = (double*)ctx->scratch[1];
    // No early return between here and the unpinning below: a failing call leaves the loop, both streams are
    // drained (copies already queued still write into the caller's arrays), and only then are the ranges released.
    hipError_t herr = hipSuccess;
    const char* what = "";
    for (size_t off = 0; off < nq && herr == hipSuccess && st == MI_OK; off += chunk) {
        const size_t m = std::min(chunk, nq - off);
        herr = hipMemcpyAsync((void*)(din + off), xq + off, m * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (herr != hipSuccess) { what = "upload of a query chunk"; break; }
        st = mi_interp1_nearest_f64_dev(ctx, g, din + off, dout + off, m, extrap);
        if (st != MI_OK) break;
        herr = hipEventRecord(ctx->aux_event, ctx->stream);
        if (herr == hipSuccess) herr = hipStreamWaitEvent(ctx->aux_stream, ctx->aux_event, 0);
        if (herr == hipSuccess) herr = hipMemcpyAsync(yq + off, dout + off, m * sizeof(double), hipMemcpyDeviceToHost, ctx->aux_stream);
        if (herr != hipSuccess) what = "download of a result chunk";
    }
    const hipError_t e1 = hipStreamSynchronize(ctx->stream), e2 = hipStreamSynchronize(ctx->aux_stream);
    if (pin_in) mi::unpin_host(xq);
    if (pin_out) mi::unpin_host(yq);
    if (st != MI_OK) return st;
    if (herr != hipSuccess) return mi::fail(ctx, MI_ERR_HIP, "mi_interp1_nearest_f64_host: %s failed: %s", what, hipGetErrorString(herr));
    MI_HIP(ctx, e1);
    MI_HIP(ctx, e2);
    return MI_OK;
}

mi_status mi_interp1_nearest_f64(mi_ctx* ctx, const double* x, const double* y, size_t n, const double* xq, double* yq, size_t nq,
                                 double extrap)
{
    MI_REQUIRE(ctx, ctx, "mi_interp1_nearest_f64: NULL context");
    mi_grid1* g = nullptr;
    mi_status st = mi_grid1_create(ctx, x, y, n, MI_GRID_SANITISE, &g);
    if (st != MI_OK) return st;
    st = mi_interp1_nearest_f64_host(ctx, g, xq, yq, nq, extrap);
    mi_grid1_destroy(g);
    return st;
}

mi_status mi_interp1_cols_nearest_f64_dev(mi_ctx* ctx, const mi_axis1* ax, const double* y, size_t ldy, size_t ncols,
                                          const double* xi, size_t nxi, double* yi, size_t ldyi, double extrap)
{
    MI_REQUIRE(ctx, ctx && ax, "mi_interp1_cols_nearest_f64_dev: NULL context or axis");
    MI_REQUIRE(ctx, ax->device == ctx->device, "mi_interp1_cols_nearest_f64_dev: the axis lives on device %d, the context on device %d",
               ax->device, ctx->device);
    if (ncols == 0 || nxi == 0) return MI_OK;
    MI_REQUIRE(ctx, y && xi && yi, "mi_interp1_cols_nearest_f64_dev: NULL table/query/result pointer");
    const uintptr_t al = reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(yi);
    MI_REQUIRE(ctx, (al & 7u) == 0, "mi_interp1_cols_nearest_f64_dev: pointers must be 8-byte aligned");
    const size_t n = ax->n;
    MI_REQUIRE(ctx, ldy >= n, "mi_interp1_cols_nearest_f64_dev: ldy=%zu is smaller than the axis (n=%zu)", ldy, n);
    MI_REQUIRE(ctx, ldyi >= nxi, "mi_interp1_cols_nearest_f64_dev: ldyi=%zu is smaller than nxi=%zu", ldyi, nxi);
    MI_REQUIRE(ctx, nxi <= SIZE_MAX / sizeof(int) && ldy <= SIZE_MAX / sizeof(double) / ncols && ldyi <= SIZE_MAX / sizeof(double) / ncols,
               "mi_interp1_cols_nearest_f64_dev: ncols=%zu x (ldy=%zu, ldyi=%zu) too large", ncols, ldy, ldyi);
    MI_HIP(ctx, hipSetDevice(ctx->device));   // a process may hold contexts on several devices (mi_group)
    const mi_status st = mi::ensure_scratch(ctx, 3, nxi * sizeof(int));
    if (st != MI_OK) return st;
    int* idx = (int*)ctx->scratch[3];
    hipLaunchKernelGGL(nearest_cols_locate_kernel, dim3(mi::stream_grid(ctx, nxi, kBlock)), dim3(kBlock), 0, ctx->stream, ax->a, xi, nxi,
                       idx);
    MI_LAUNCH_CHECK(ctx, "interp1 nearest cols locate kernel");
    // units: row blocks x column runs, about 16 workgroups of work per CU when the shape has that much (mi_cols1.hip)
    const size_t nrb = (nxi + kRowBlock - 1) / kRowBlock;
    const size_t target = (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256) * 16;
    const size_t want_runs = std::min(ncols, std::max<size_t>(1, (target + nrb - 1) / nrb));
    const size_t run = (ncols + want_runs - 1) / want_runs;
    const size_t nruns = (ncols + run - 1) / run;
    MI_REQUIRE(ctx, nrb <= SIZE_MAX / nruns, "mi_interp1_cols_nearest_f64_dev: nxi=%zu x ncols=%zu too large", nxi, ncols);
    const size_t nunits = nrb * nruns;
    const unsigned grid = (unsigned)std::min(nunits, target);   // workgroups stride over the units beyond that
    const bool vec = (reinterpret_cast<uintptr_t>(yi) & 15u) == 0 && (ldyi & 1) == 0;
    if (n <= kLdsMaxN) {
        const size_t lds_bytes = 2 * (n + 2) * sizeof(double);
        return vec ? launch_cols<true, true>(ctx, grid, lds_bytes, idx, (int)n, y, ldy, ncols, run, nxi, nrb, nunits, yi, ldyi, extrap)
                   : launch_cols<true, false>(ctx, grid, lds_bytes, idx, (int)n, y, ldy, ncols, run, nxi, nrb, nunits, yi, ldyi, extrap);
    }
    return vec ? launch_cols<false, true>(ctx, grid, 0, idx, (int)n, y, ldy, ncols, run, nxi, nrb, nunits, yi, ldyi, extrap)
               : launch_cols<false, false>(ctx, grid, 0, idx, (int)n, y, ldy, ncols, run, nxi, nrb, nunits, yi, ldyi, extrap);
}

}  // extern "C"
