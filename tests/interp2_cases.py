"""Shared cases for the bilinear kernels (csrc/mi_interp2.hip, csrc/mi_interp2_grid.hip, csrc/mi_interp2_eval.hpp): seven
tables whose Z holds inf, NaN, -0.0 and denormals at the places where a kernel must SELECT a table element away rather
than multiply it by a zero weight, and query sets that put a query on every node, on both its ulp neighbours and on
every cell midpoint of both axes.

Plain numpy plus the CPU oracle: no torch, no GPU.  tests/test_interp2_cases_cpu.py checks the reference on these cases
(oracle.interp2_bilinear against a literal pure-Python scan, against the exact rational result, and the reach property);
tests/test_interp2_edges_gpu.py holds the scattered and the gridded kernels to oracle.interp2_bilinear on every element,
bit for bit, the sign of zero included.

Tables (TABLES; Z is (ny, nx), Z[i, j] at (yg[i], xg[j])):
    t2x2           2 x 2
    t2rows         ny = 2, nx = 67
    t2cols         nx = 2, ny = 131
    guess_bsearch  nx = 37 nodes jittered within a third of a cell (analytic guess + bounded walk); ny = 29 clustered
                   nodes, made unique AFTER the shift by 1e3, the closest ones one ulp apart (binary search)
    uniform        implicit axes x_j = fma(j, 0.0317, -1), y_i = fma(i, 0.0641, 0.5), 64 x 48 (steps with dense binary
                   digits: most nodes are inexact)
    huge_tiny      x from uniform(-1e307, 1e307), y from uniform(-1e-300, 1e-300), 33 x 21
    span_overflow  x = [-1.7e308, 0, 1.7e308] (xmax - xmin = inf: scale 0, binary search), y = [-0.0, 5e-324, 1e-323, 1]

Z = seeded normal times a per-element choice of {1, 1e150, 1e-150} (nothing larger: a blend of finite corners cannot
overflow), kept as "Zfinite"; "Z" is that with the specials of special_places() written over it.  Why each place:
    the last row           in the compact layout the second cell element of row ny-1 is the NEXT column's first row: so
                           Z[ny-1, c] is -0.0 / 5e-324 (finite, its sign visible) and Z[0, c+1] is NaN / +inf
    the last corner        -0.0: its second cell element is the compact layout's zero padding element
    the last column        the quad layout duplicates it (and the last row)
    the first corner       an out-of-range query is evaluated at (xmin, ymin) and then replaced: +inf there
    interior               +inf over -inf, +inf beside -inf, one NaN, one whole cell of -0.0, +-5e-324
"""
import functools
from fractions import Fraction

import numpy as np

import oracle
from sweep_cases import same_bits  # noqa: F401  (re-exported: the comparison of every interp2 edge test)

TABLES = ["t2x2", "t2rows", "t2cols", "guess_bsearch", "uniform", "huge_tiny", "span_overflow"]
SCALES = (1.0, 1e150, 1e-150)
KMAX_WALK = 4              # csrc/mi_interp2_eval.hpp kMaxWalk: spread of the analytic guess up to which it is used


def _fma(i, dx, x0):
    """fma(i, dx, x0): the exact rational value, rounded once"""
    return float(Fraction(int(i)) * Fraction(float(dx)) + Fraction(float(x0)))


def uniform_nodes(x0, dx, n):
    return np.array([_fma(i, dx, x0) for i in range(n)], dtype=np.float64)


def axis_uses_guess(nodes):
    """the rule make_explicit_axis (csrc/mi_interp2.hip) picks the search by: analytic guess + walk when the guess is
    never more than KMAX_WALK nodes wide of the truth, binary search otherwise (and when the span is not finite)"""
    nodes = np.asarray(nodes, dtype=np.float64)
    n = nodes.size
    with np.errstate(all="ignore"):
        scale = (n - 1) / (nodes[-1] - nodes[0])
        if not (np.isfinite(scale) and scale > 0.0):
            return False
        gi = np.clip(((nodes - nodes[0]) * scale).astype(np.int64), 0, n - 1)
    e = gi - np.arange(n)
    return int(e.max() - e.min() + 1) <= KMAX_WALK


def _axes(name):
    u = oracle.splitmix_uniform(31, 256)
    rng = np.random.default_rng([0x1E2, TABLES.index(name)])
    uni = None
    if name == "t2x2":
        xg, yg = np.array([-1.0, 2.5]), np.array([-0.5, 0.75])
    elif name == "t2rows":
        xg, yg = -3.0 + np.cumsum(0.05 + u[:67]), np.array([0.0, 1.0])
    elif name == "t2cols":
        xg, yg = np.array([0.25, 0.75]), -40.0 + np.cumsum(0.05 + u[:131])
    elif name == "guess_bsearch":
        xg = -2.0 + 3.0 * (np.arange(37) + (u[:37] - 0.5) / 3.0) / 36.0
        near = [1e-13, 2e-13, 0.3, 0.3 + 1e-13, 0.3 + 2e-13]            # 1e3 + these: one ulp (1.14e-13) apart
        yg = np.unique(1e3 + np.sort(np.concatenate([u[40:64] ** 3, near])))
    elif name == "uniform":
        uni = (-1.0, 0.0317, 0.5, 0.0641)
        xg, yg = uniform_nodes(uni[0], uni[1], 64), uniform_nodes(uni[2], uni[3], 48)
    elif name == "huge_tiny":
        xg, yg = np.sort(rng.uniform(-1e307, 1e307, 33)), np.sort(rng.uniform(-1e-300, 1e-300, 21))
    elif name == "span_overflow":
        xg, yg = np.array([-1.7e308, 0.0, 1.7e308]), np.array([-0.0, 5e-324, 1e-323, 1.0])
    else:
        raise ValueError(name)
    xg, yg = np.ascontiguousarray(xg, dtype=np.float64), np.ascontiguousarray(yg, dtype=np.float64)
    assert np.all(np.diff(xg) > 0) and np.all(np.diff(yg) > 0) and np.all(np.isfinite(xg)) and np.all(np.isfinite(yg))
    return xg, yg, uni


def special_places(ny, nx):
    """{(row, column): value} of the specials written over Z (module docstring).  Tables with fewer than 5 nodes on an
    axis get one special at a corner -- more would leave no finite output -- except span_overflow (4 x 3), whose six
    cells take a NaN at the last corner, one cell of -0.0 and a denormal."""
    inf, nan = np.inf, np.nan
    if (ny, nx) == (2, 2):
        return {(1, 1): -0.0}
    if ny == 2:
        return {(0, nx - 1): inf}
    if nx == 2:
        return {(ny - 1, 0): nan}
    if (ny, nx) == (4, 3):
        return {(3, 2): nan, (0, 0): -0.0, (1, 0): -0.0, (0, 1): -0.0, (1, 1): -0.0, (2, 1): 5e-324}
    assert ny >= 16 and nx >= 16
    c, c2 = nx // 3, (2 * nx) // 3
    p = [((0, 0), inf), ((0, nx - 1), -inf), ((ny - 1, 0), nan), ((ny - 1, nx - 1), -0.0),
         ((ny - 1, c), -0.0), ((0, c + 1), nan),                         # last row / the next column's first row
         ((ny - 1, c2), 5e-324), ((0, c2 + 1), inf),
         ((ny // 2, nx - 1), inf),                                       # last column
         ((ny // 4, nx // 4), inf), ((ny // 4 + 1, nx // 4), -inf),      # +inf with -inf directly below
         ((ny // 2, nx // 2), inf), ((ny // 2, nx // 2 + 1), -inf),      # and side by side
         ((3 * ny // 4, nx // 5), nan),
         ((ny // 3, 3 * nx // 4), -0.0), ((ny // 3 + 1, 3 * nx // 4), -0.0),
         ((ny // 3, 3 * nx // 4 + 1), -0.0), ((ny // 3 + 1, 3 * nx // 4 + 1), -0.0),
         ((2, nx // 2), 5e-324), ((3, nx // 2), -5e-324)]
    places = dict(p)
    assert len(places) == len(p)                                         # no place named twice
    return places


@functools.lru_cache(maxsize=None)
def table(name):
    """{"name", "xg", "yg", "Z", "Zfinite", "uniform": None | (x0, dx, y0, dy)} (arrays are shared: do not modify)"""
    xg, yg, uni = _axes(name)
    ny, nx = yg.size, xg.size
    rng = np.random.default_rng([0x2D, TABLES.index(name)])
    Zf = rng.standard_normal((ny, nx)) * rng.choice(SCALES, size=(ny, nx))
    Z = Zf.copy()
    for (i, j), v in special_places(ny, nx).items():
        Z[i, j] = v
    for a in (xg, yg, Z, Zf):
        a.setflags(write=False)
    return {"name": name, "xg": xg, "yg": yg, "Z": Z, "Zfinite": Zf, "uniform": uni}


# ---------------------------------------------------------------------------------------------- queries
def _distinct(values):
    """the values in their order, each 64-bit pattern once (-0.0 and 0.0 are two; NaN is one)"""
    q = np.array(values, dtype=np.float64)
    q[np.isnan(q)] = np.nan
    _, first = np.unique(q.view(np.int64), return_index=True)
    return q[np.sort(first)]


def _beyond(nodes):
    """one value beyond each end (+-inf where the axis leaves no finite one that far out)"""
    lo, hi = float(nodes[0]), float(nodes[-1])
    with np.errstate(over="ignore"):
        d = max(0.25 * (0.5 * hi - 0.5 * lo) * 2.0, 1e-310)
        return lo - d, hi + d


def axis_queries(nodes):
    """every node and both its ulp neighbours, the midpoints of neighbouring nodes, NaN, +-inf, one value beyond each
    end, and -0.0, 0.0, +-5e-324 where 0 is in range"""
    nodes = np.asarray(nodes, dtype=np.float64)
    below, above = _beyond(nodes)
    q = [nodes, np.nextafter(nodes, -np.inf), np.nextafter(nodes, np.inf), 0.5 * nodes[:-1] + 0.5 * nodes[1:],
         [nodes[0], nodes[-1], np.nan, np.inf, -np.inf, below, above]]
    if nodes[0] <= 0.0 <= nodes[-1]:
        q.append([-0.0, 0.0, 5e-324, -5e-324])
    return _distinct(np.concatenate([np.asarray(a, dtype=np.float64) for a in q]))


@functools.lru_cache(maxsize=None)
def scattered(name):
    """(xq, yq): the full cross product of the two axis sets in a seeded order, of odd length (the first pair once more
    where the product is even)"""
    t = table(name)
    ax, ay = axis_queries(t["xg"]), axis_queries(t["yg"])
    XX, YY = np.meshgrid(ax, ay)
    perm = np.random.default_rng([0x5CA7, TABLES.index(name)]).permutation(XX.size)
    xq, yq = XX.ravel()[perm], YY.ravel()[perm]
    if xq.size % 2 == 0:
        xq, yq = np.append(xq, xq[0]), np.append(yq, yq[0])
    xq.setflags(write=False)
    yq.setflags(write=False)
    return xq, yq


def cache_xi(xg):
    """Columns for the gridded tile kernel, which keeps a lane's two cells in registers while the column bracket lx is
    unchanged: runs inside one cell c interrupted by flagged columns (NaN, below, above, +-inf), by a column of cell
    c + 1 and by xmax, for the first, second, middle and last cells.  A period of 18 columns per cell."""
    xg = np.asarray(xg, dtype=np.float64)
    nx = xg.size
    below, above = _beyond(xg)
    out = []
    for c in _distinct([0, 1, (nx - 1) // 2, nx - 3, nx - 2]).astype(np.int64):
        if not 0 <= c <= nx - 2:
            continue
        a, b = xg[c], xg[c + 1]
        mid, quarter, last = 0.5 * a + 0.5 * b, 0.75 * a + 0.25 * b, np.nextafter(b, -np.inf)
        nxt = xg[-1] if c + 2 > nx - 1 else 0.5 * xg[c + 1] + 0.5 * xg[c + 2]      # a column of cell c + 1
        out += [mid, np.nan, quarter, below, a, nxt, last, xg[-1], mid, above, quarter, np.inf, mid, -np.inf, a, b, last, quarter]
    return np.array(out, dtype=np.float64)


def grid_xi(xg):
    """the unsorted XI of the gridded cases: cache_xi, then the rest of the axis set"""
    return np.concatenate([cache_xi(xg), axis_queries(xg)])


def grid_yi(yg, nyi, seed=0):
    """the y axis set in a seeded order, resized (repeated or cut) to nyi"""
    q = axis_queries(yg)
    return np.resize(q[np.random.default_rng([0x71, seed]).permutation(q.size)], nyi)


def mesh_pairs(xi, yi):
    """the meshgrid pairs in the column-major order of ZI: k = i + j * nyi"""
    XX, YY = np.meshgrid(xi, yi)
    return XX.ravel("F"), YY.ravel("F")


# ---------------------------------------------------------------------------------------------- references
def in_range(xq, yq, xg, yg):
    xq, yq = np.asarray(xq, dtype=np.float64), np.asarray(yq, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (xq >= xg[0]) & (xq <= xg[-1]) & (yq >= yg[0]) & (yq <= yg[-1])


def brackets(nodes, q):
    """(l, r) of in-range queries: l the largest index with nodes[l] <= q, r = min(l + 1, n - 1)"""
    l = np.searchsorted(nodes, q, side="right") - 1
    assert np.all(l >= 0)
    return l, np.minimum(l + 1, nodes.size - 1)


def with_extrap(ref_nan, xq, yq, xg, yg, extrap):
    """the reference under another extrapolation value, from the one computed with extrap = NaN: queries that are out of
    range and have no NaN coordinate get `extrap` (NaN wins; the CPU file holds the oracle to this)"""
    xq, yq = np.asarray(xq, dtype=np.float64), np.asarray(yq, dtype=np.float64)
    out = np.array(ref_nan, dtype=np.float64, copy=True)
    out[~in_range(xq, yq, xg, yg) & ~np.isnan(xq) & ~np.isnan(yq)] = extrap
    return out


def reference(name, xq, yq, extrap=np.nan, Z=None, nthreads=4):
    """the oracle on table `name` (its implicit-axes entry point for the uniform table)"""
    t = table(name)
    Z = t["Z"] if Z is None else Z
    if t["uniform"]:
        x0, dx, y0, dy = t["uniform"]
        return oracle.interp2_bilinear_uniform(x0, dx, t["xg"].size, y0, dy, t["yg"].size, Z, xq, yq, extrap, nthreads)
    return oracle.interp2_bilinear(t["xg"], t["yg"], Z, xq, yq, extrap, nthreads)


def _scan(nodes, q):
    l = 0
    for k in range(len(nodes)):
        if nodes[k] <= q:
            l = k
        else:
            break
    return l, min(l + 1, len(nodes) - 1)


def literal_bilinear(xg, yg, Z, xq, yq, extrap=float("nan")):
    """per query: a forward scan for each bracket and the blend written out with Python floats (IEEE doubles, every
    product and sum rounded once).  Shares no code with oracle/."""
    xs, ys = [float(v) for v in xg], [float(v) for v in yg]
    z = [[float(v) for v in row] for row in np.asarray(Z)]
    out = np.empty(len(xq), dtype=np.float64)
    for k, (qx, qy) in enumerate(zip(np.asarray(xq).tolist(), np.asarray(yq).tolist())):
        if qx != qx or qy != qy:
            out[k] = float("nan")
            continue
        if qx < xs[0] or qx > xs[-1] or qy < ys[0] or qy > ys[-1]:
            out[k] = extrap
            continue
        lx, rx = _scan(xs, qx)
        ly, ry = _scan(ys, qy)
        ax, bx = qx - xs[lx], xs[rx] - qx
        ay, by = qy - ys[ly], ys[ry] - qy
        wx = ax / (ax + bx) if ax > 0.0 else 0.0
        wy = ay / (ay + by) if ay > 0.0 else 0.0
        c0 = (1.0 - wy) * z[ly][lx] + wy * z[ry][lx]
        c1 = (1.0 - wy) * z[ly][rx] + wy * z[ry][rx]
        out[k] = (1.0 - wx) * c0 + wx * c1
    return out


def exact_bilinear(xg, yg, Z, qx, qy):
    """the exact rational bilinear interpolant at one in-range query, and the sum of its four corner magnitudes"""
    qx, qy = float(qx), float(qy)
    (lx,), (rx,) = brackets(xg, np.array([qx]))
    (ly,), (ry,) = brackets(yg, np.array([qy]))
    F = lambda v: Fraction(float(v))  # noqa: E731
    wx = (F(qx) - F(xg[lx])) / (F(xg[rx]) - F(xg[lx])) if rx != lx else Fraction(0)
    wy = (F(qy) - F(yg[ly])) / (F(yg[ry]) - F(yg[ly])) if ry != ly else Fraction(0)
    z00, z01, z10, z11 = F(Z[ly, lx]), F(Z[ry, lx]), F(Z[ly, rx]), F(Z[ry, rx])
    ex = (1 - wx) * ((1 - wy) * z00 + wy * z01) + wx * ((1 - wy) * z10 + wy * z11)
    return ex, abs(z00) + abs(z01) + abs(z10) + abs(z11)


BILINEAR_BOUND_UNITS = 16  # |oracle - exact| <= 16 * 2^-53 * (sum of the corner magnitudes): tests/test_interp2_cases_cpu.py


def bilinear_error_units(xg, yg, Z, qx, qy, got):
    """|got - exact| in units of 2^-53 * (|z00| + |z01| + |z10| + |z11|)"""
    ex, S = exact_bilinear(xg, yg, Z, qx, qy)
    err = abs(Fraction(float(got)) - ex)
    if S == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / (Fraction(1, 2 ** 53) * S))


def corners_finite(xg, yg, Z, xq, yq):
    """for in-range queries: are all four bracket corners finite?"""
    lx, rx = brackets(xg, xq)
    ly, ry = brackets(yg, yq)
    return np.isfinite(Z[ly, lx]) & np.isfinite(Z[ry, lx]) & np.isfinite(Z[ly, rx]) & np.isfinite(Z[ry, rx])
