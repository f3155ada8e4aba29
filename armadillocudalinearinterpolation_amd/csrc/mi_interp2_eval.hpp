// Bilinear interpolation over an HBM-resident 2-D table on MI355X (gfx950): the table handle, its resident layouts
// (mi_interp2.hip) and the locate-and-blend arithmetic every interp2 kernel shares, so that the scattered kernel
// (mi_interp2.hip) and the gridded ones (mi_interp2_grid.hip) give bit-identical results.
// Semantics: oracle/interp_oracle.c orc_interp2_bilinear[_uniform]; blend along y inside the two bracketing columns,
// then along x.  Every TU that includes this is compiled with -ffp-contract=off (every product/sum rounds separately).
#pragma once
#include "mi_common.hpp"

typedef double d2 __attribute__((ext_vector_type(2)));

struct AxisDev {
    const double* nodes;   // explicit axis (null when implicit)
    int n;
    int use_guess;         // explicit: analytic guess + walk (1) or binary search (0)
    double xmin, xmax, scale;
    double x0, dx;         // implicit: node_i = fma(i, dx, x0)
};

typedef double d2v __attribute__((ext_vector_type(2)));

struct G2Dev {
    AxisDev ax, ay;
    const d2v* zp;         // (ny*nx + 1) column pairs {Z(l,c), Z(l,c+1)}, index l + c*ny
    int quads;             // 1: zp holds 2*ny*nx d2v: cell (l,c) = {Z(l,c), Z(l,rx)}, {Z(ry,c), Z(ry,rx)} (32 B)
};

struct mi_grid2 {
    mi_ctx* ctx;
    int device;            // copied at creation: destroy must not dereference a context that may be gone
    void* dev_x;
    void* dev_y;
    void* dev_z;
    G2Dev d;
    size_t table_bytes = 0;
};

namespace mi_interp2 {

constexpr int kBlock = 256;
constexpr int kMaxWalk = 4;

// IMPL: the axis is known to be implicit (uniform) at compile time -- no node loads, no search branches; the arithmetic
// is the one the general form takes for such an axis
template <bool IMPL = false>
__device__ __forceinline__ double axis_node(const AxisDev& a, int i)
{
    if constexpr (IMPL) return fma((double)i, a.dx, a.x0);
    return a.nodes ? a.nodes[i] : fma((double)i, a.dx, a.x0);
}

// largest l with node_l <= q (q inside [xmin, xmax])
template <bool IMPL = false>
__device__ __forceinline__ int axis_locate(const AxisDev& a, double q)
{
    if (!IMPL && a.nodes && !a.use_guess) {
        int lo = 0, hi = a.n;
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (a.nodes[mid] <= q) lo = mid; else hi = mid;
        }
        return lo;
    }
    int i = (int)((q - a.xmin) * a.scale);
    i = min(max(i, 0), a.n - 1);
    while (i > 0 && axis_node<IMPL>(a, i) > q) --i;
    while (i < a.n - 1 && axis_node<IMPL>(a, i + 1) <= q) ++i;
    return i;
}

__device__ __forceinline__ double weight(double xa, double xb, double q)
{
    const double a = q - xa, b = xb - q;
    return (a > 0.0) ? a / (a + b) : 0.0;
}

// the y blend inside the two bracketing columns: {c0, c1} = column lx, column rx at the query's y.  lo = {Z(ly,lx),
// Z(ly,rx)}, hi = {Z(ry,lx), Z(ry,rx)}; two_rows = (ry != ly) (at the last node hi is not a row of the cell)
__device__ __forceinline__ d2v blend_y(d2v lo, d2v hi, double wy, bool two_rows)
{
    const double z01 = two_rows ? hi.x : lo.x;
    const double z11 = two_rows ? hi.y : lo.y;
    d2v c;
    c.x = (1.0 - wy) * lo.x + wy * z01;
    c.y = (1.0 - wy) * lo.y + wy * z11;
    return c;
}

// then along x
__device__ __forceinline__ double blend_x(d2v c, double wx)
{
    return (1.0 - wx) * c.x + wx * c.y;
}

// The blend, written once for every interp2 kernel: along y inside the two bracketing columns, then along x, every
// product and sum rounded.  lo = {Z(ly,lx), Z(ly,rx)}, hi = {Z(ry,lx), Z(ry,rx)}; at the last node (ry == ly) hi is not
// a row of the cell and lo is used twice.  Declares `const double r`.  A macro rather than an inline function: the
// scattered kernel's code is pinned (tests/test_interp2_grid_cpu.py), and an extra call level, inlined or not, changes
// its instruction schedule.
#define MI_INTERP2_BLEND(lo, hi, two_rows, wx, wy, r)                \
    const double z01_ = (two_rows) ? (hi).x : (lo).x;                \
    const double z11_ = (two_rows) ? (hi).y : (lo).y;                \
    const double c0_ = (1.0 - (wy)) * (lo).x + (wy) * z01_;          \
    const double c1_ = (1.0 - (wy)) * (lo).y + (wy) * z11_;          \
    const double r = (1.0 - (wx)) * c0_ + (wx) * c1_

// eval2 in three steps, so that a kernel can put the cell loads of several queries in flight together
// (interp2_blocks_kernel); the direct kernel runs them back to back.  Same operations in the same order either way.
struct Loc2 {
    double sx, sy;       // the query, or the grid's origin for an out-of-range / NaN query (its result is replaced)
    int lx, ly, rx, ry;
    bool oor;
    const d2v* cell;     // two consecutive 16-B elements: {Z(ly,lx), Z(ly,rx)}, then the next row's pair / the quad's second half
};

template <bool IMPL = false>
__device__ __forceinline__ Loc2 locate2(const G2Dev& g, double qx, double qy)
{
    Loc2 L;
    L.oor = !(qx >= g.ax.xmin && qx <= g.ax.xmax && qy >= g.ay.xmin && qy <= g.ay.xmax);
    L.sx = L.oor ? g.ax.xmin : qx;
    L.sy = L.oor ? g.ay.xmin : qy;
    L.lx = axis_locate<IMPL>(g.ax, L.sx);
    L.ly = axis_locate<IMPL>(g.ay, L.sy);
    L.rx = min(L.lx + 1, g.ax.n - 1);
    L.ry = min(L.ly + 1, g.ay.n - 1);
    const size_t k = (size_t)L.lx * (size_t)g.ay.n + L.ly;
    L.cell = g.quads ? g.zp + 2 * k : g.zp + k;
    return L;
}

// lo = cell[0] = {Z(ly,lx), Z(ly,rx)}; hi = cell[1]: pairs: next row (padding past the last); quads: {Z(ry,lx), Z(ry,rx)}
template <bool IMPL = false>
__device__ __forceinline__ double blend2(const G2Dev& g, const Loc2& L, d2v lo, d2v hi, double qx, double qy, double extrap)
{
    const double wx = weight(axis_node<IMPL>(g.ax, L.lx), axis_node<IMPL>(g.ax, L.rx), L.sx);
    const double wy = weight(axis_node<IMPL>(g.ay, L.ly), axis_node<IMPL>(g.ay, L.ry), L.sy);
    MI_INTERP2_BLEND(lo, hi, L.ry != L.ly, wx, wy, r);
    if (L.oor) return (qx != qx || qy != qy) ? __builtin_nan("") : extrap;
    return r;
}

__device__ __forceinline__ double eval2(const G2Dev& g, double qx, double qy, double extrap)
{
    const Loc2 L = locate2(g, qx, qy);
    const d2v lo = L.cell[0], hi = L.cell[1];
    return blend2(g, L, lo, hi, qx, qy, extrap);
}

// ---- gridded form (mi_interp2_grid.hip): each query coordinate located once per call ----------------------------
// One axis coordinate of the gridded call: the bracket l..r and the weight w, computed by the calls locate2 / blend2
// make for an in-range query (so the bits cannot drift); r < 0 flags a coordinate outside [xmin, xmax] (-1) or NaN (-2),
// with l = 0 so that a cell address formed from it stays inside the table.
struct AxRec {
    double w;
    int l, r;
};

__device__ __forceinline__ AxRec axis_record(const AxisDev& a, double q)
{
    AxRec R;
    if (!(q >= a.xmin && q <= a.xmax)) {
        R.w = 0.0;
        R.l = 0;
        R.r = (q != q) ? -2 : -1;
        return R;
    }
    R.l = axis_locate(a, q);
    R.r = min(R.l + 1, a.n - 1);
    R.w = weight(axis_node(a, R.l), axis_node(a, R.r), q);
    return R;
}

// result of an output whose column or row record is flagged (blend2's out-of-range rule)
__device__ __forceinline__ double flagged_result(int rx, int ry, double extrap)
{
    return (rx == -2 || ry == -2) ? __builtin_nan("") : extrap;
}

// the two 16-B elements of cell (ly, lx) in either resident layout (locate2)
__device__ __forceinline__ const d2v* cell_ptr(const G2Dev& g, int lx, int ly)
{
    const size_t k = (size_t)lx * (size_t)g.ay.n + ly;
    return g.quads ? g.zp + 2 * k : g.zp + k;
}

// one output from its two records: blend2's arithmetic with the weights located once per call
__device__ __forceinline__ double blend_records(d2v lo, d2v hi, const AxRec& X, const AxRec& Y, double extrap)
{
    MI_INTERP2_BLEND(lo, hi, Y.r != Y.l, X.w, Y.w, r);
    return (X.r < 0 || Y.r < 0) ? flagged_result(X.r, Y.r, extrap) : r;
}

}  // namespace mi_interp2

