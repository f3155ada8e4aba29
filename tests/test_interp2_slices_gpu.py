"""Gridded interp2 over the slices of a cube, Z read in place (mi_interp2_slices_f64_dev, interp2_slices): slice s of the
result is bit-identical to the oracle on the meshgrid pairs over (x, y, Z_s) and to the existing gridded call on a
mi_grid2 built from that slice, for every form of the slice kernel (LDS / direct, tile / flat body, 16-B / 8-B stores),
padded and gapped layouts, every table form and non-finite table values."""
import ctypes as C
import math

import numpy as np
import pytest

import interp2_cases as cases
import oracle

pytestmark = pytest.mark.gpu

LDS_MAX_ELEMS = 8192      # kLdsMaxElems in csrc/mi_slices2.hip: the LDS form up to here, the direct form beyond
THIN_ROWS = 256           # kThinRows: nyi below takes the flat body
LDS_TILE, LDS_FLAT, DIRECT_TILE, DIRECT_FLAT = 0, 1, 2, 3

# (ny, nx, nyi, nxi, S): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (2, 2, 5, 7, 3),
    (2, 67, 3, 300, 5),
    (131, 2, 700, 2, 5),
    (29, 37, 255, 9, 7), (29, 37, 257, 33, 7),          # either side of the flat / tile switch, odd nyi
    (41, 53, 513, 64, 3),                               # two row blocks, the second with one row
    (64, 64, 128, 128, 9),
    (64, 128, 257, 20, 5), (64, 129, 257, 20, 5),       # a slice of exactly the LDS limit, then one column more
    (64, 128, 60, 33, 5), (64, 129, 60, 33, 5),         # the same pair under the flat body
]


def _form(ny, nx, nyi):
    lds = ny * nx <= LDS_MAX_ELEMS
    thin = nyi < THIN_ROWS
    return (LDS_FLAT if thin else LDS_TILE) if lds else (DIRECT_FLAT if thin else DIRECT_TILE)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _cube(Z):
    """(ny, nx, S) numpy array -> CUDA tensor of that shape laid out like an arma::cube"""
    return _t(np.ascontiguousarray(Z.transpose(2, 1, 0))).permute(2, 1, 0)


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _pairs(xi, yi):
    """the meshgrid pairs in the column-major order of ZI: k = i + j*nyi"""
    XX, YY = np.meshgrid(xi, yi)                     # (nyi, nxi)
    return XX.ravel("F"), YY.ravel("F")


def _ref(xg, yg, Z, xi, yi, extrap=np.nan):
    """the oracle on every slice of Z (ny, nx, S) -> (nyi, nxi, S)"""
    px, py = _pairs(xi, yi)
    out = np.empty((yi.size, xi.size, Z.shape[2]))
    for s in range(Z.shape[2]):
        out[:, :, s] = oracle.interp2_bilinear(xg, yg, Z[:, :, s], px, py, extrap, nthreads=8).reshape(yi.size, xi.size, order="F")
    return out


def _axis_queries(rng, nodes, n):
    """unsorted queries over the axis in the manner of tests/test_interp2_grid_gpu.py -- exact nodes, both end nodes, one
    NaN (n >= 5), points out of range (n >= 7: about a sixth of them, on both sides from n >= 12) -- but each kind at
    positions of its own, so that at least 5/7 of an axis of five or more queries is in range whatever the seed"""
    lo, hi = nodes[0], nodes[-1]
    q = rng.uniform(lo, hi, n)
    free = list(rng.permutation(n))
    if n >= 5:
        q[free.pop()] = np.nan
    if n >= 7:
        k = max(1, n // 6)
        sides = rng.permutation(2) if k == 1 else (0, 1)
        for side, count in zip(sides, (k - k // 2, k // 2)):
            for _ in range(count):
                d = rng.uniform(0.001, 0.1) * (hi - lo)
                q[free.pop()] = lo - d if side == 0 else hi + d
    if n >= 2:
        q[free.pop()] = hi
        q[free.pop()] = lo
    for _ in range(min(len(free), max(1, n // 5))):
        q[free.pop()] = nodes[rng.integers(0, nodes.size)]
    return q


def _table(rng, ny, nx, S):
    xg = np.cumsum(rng.uniform(0.2, 1.0, nx))
    yg = np.cumsum(rng.uniform(0.1, 2.0, ny)) - 3.0
    return xg, yg, rng.standard_normal((ny, nx, S))


def _assert_not_trivial(xg, yg, xi, yi):
    """a case must not pass on nothing but extrap_val: at least half of the outputs in range, one out of range, one NaN"""
    px, py = _pairs(xi, yi)
    inr = cases.in_range(px, py, xg, yg)
    nan = np.isnan(px) | np.isnan(py)
    assert inr.mean() >= 0.5 and (~inr & ~nan).any() and nan.any(), (inr.mean(), (~inr & ~nan).sum(), nan.sum())


def _case(shape, seed=0):
    ny, nx, nyi, nxi, S = shape
    rng = np.random.default_rng([20261018, seed, ny, nx, nyi, nxi, S])
    xg, yg, Z = _table(rng, ny, nx, S)
    xi, yi = _axis_queries(rng, xg, nxi), _axis_queries(rng, yg, nyi)
    if nxi >= 5 and nyi >= 5:
        _assert_not_trivial(xg, yg, xi, yi)
    return xg, yg, Z, xi, yi


def _axes(mi_ctx, xg, yg):
    import armadillocudalinearinterpolation_amd as mi
    return mi.Axis1.from_nodes(mi_ctx, xg), mi.Axis1.from_nodes(mi_ctx, yg)


def _launches(L):
    return [int(L.mi_debug_slices2_launches(f)) for f in range(4)]


def _grid_per_slice(mi_ctx, xg, yg, Z, xi, yi, extrap=math.nan):
    """the existing gridded call on a mi_grid2 built from each slice"""
    import armadillocudalinearinterpolation_amd as mi
    out = np.empty((yi.size, xi.size, Z.shape[2]))
    xd, yd = _t(xi), _t(yi)
    for s in range(Z.shape[2]):
        g = mi.Grid2.from_axes(mi_ctx, xg, yg, Z[:, :, s])
        out[:, :, s] = g.interp_grid(xd, yd, extrap=extrap).cpu().numpy()
        g.close()
    return out


def test_one_query_in_range(mi_ctx):
    """(2, 2, 1, 1, 1): the smallest call there is, its single query placed inside the cell by hand"""
    import armadillocudalinearinterpolation_amd as mi
    xg, yg = np.array([-1.0, 2.5]), np.array([-0.5, 0.75])
    Z = np.array([[1.0, -2.0], [0.5, 4.0]]).reshape(2, 2, 1)
    xi, yi = np.array([0.3]), np.array([0.1])
    ax, ay = _axes(mi_ctx, xg, yg)
    before = _launches(mi_ctx._L)
    got = mi.interp2_slices(mi_ctx, ax, ay, _cube(Z), _t(xi), _t(yi)).cpu().numpy()
    assert [a - b for a, b in zip(_launches(mi_ctx._L), before)] == [0, 1, 0, 0]
    ref = _ref(xg, yg, Z, xi, yi)
    assert got.shape == (1, 1, 1) and np.isfinite(ref).all() and _eq(got, ref)
    assert _eq(got, _grid_per_slice(mi_ctx, xg, yg, Z, xi, yi))
    wx, wy = (0.3 + 1.0) / 3.5, (0.1 + 0.5) / 1.25               # not the oracle: the bilinear formula itself
    plain = (1 - wx) * ((1 - wy) * 1.0 + wy * 0.5) + wx * ((1 - wy) * -2.0 + wy * 4.0)
    assert abs(got[0, 0, 0] - plain) < 1e-14


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_against_oracle_and_the_gridded_call(mi_ctx, shape):
    import armadillocudalinearinterpolation_amd as mi
    ny, nx, nyi, nxi, S = shape
    xg, yg, Z, xi, yi = _case(shape)
    ax, ay = _axes(mi_ctx, xg, yg)
    Zd, xd, yd = _cube(Z), _t(xi), _t(yi)
    before = _launches(mi_ctx._L)
    got = mi.interp2_slices(mi_ctx, ax, ay, Zd, xd, yd)
    assert tuple(got.shape) == (nyi, nxi, S) and got.permute(2, 1, 0).is_contiguous()
    took = [a - b for a, b in zip(_launches(mi_ctx._L), before)]
    assert took == [int(f == _form(ny, nx, nyi)) for f in range(4)], took
    got = got.cpu().numpy()
    assert _eq(got, _ref(xg, yg, Z, xi, yi))
    assert _eq(got, _grid_per_slice(mi_ctx, xg, yg, Z, xi, yi))
    got = mi.interp2_slices(mi_ctx, ax, ay, Zd, xd, yd, extrap=-3.25).cpu().numpy()
    assert _eq(got, _ref(xg, yg, Z, xi, yi, -3.25))


@pytest.mark.parametrize("ny,nx", [(41, 53), (100, 90)])
def test_sorted_queries_denser_than_the_nodes(mi_ctx, ny, nx):
    """sorted XI, several columns per cell and every cell visited: the tile body moves the right column over to the left
    and loads one new column; reversed, it never can.  In the LDS form and in the direct form."""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng([7, ny, nx])
    xg, yg, Z = _table(rng, ny, nx, 3)
    span = xg[-1] - xg[0]
    xi = np.sort(np.concatenate([np.linspace(xg[0] - 0.02 * span, xg[-1] + 0.02 * span, 3 * nx + 1), xg[::7], [np.nan]]))
    yi = _axis_queries(rng, yg, 300)
    _assert_not_trivial(xg, yg, xi, yi)
    ax, ay = _axes(mi_ctx, xg, yg)
    before = _launches(mi_ctx._L)
    for q in (xi, xi[::-1].copy()):
        got = mi.interp2_slices(mi_ctx, ax, ay, _cube(Z), _t(q), _t(yi), extrap=0.5).cpu().numpy()
        assert _eq(got, _ref(xg, yg, Z, q, yi, 0.5))
        assert _eq(got, _grid_per_slice(mi_ctx, xg, yg, Z, q, yi, 0.5))
    took = [a - b for a, b in zip(_launches(mi_ctx._L), before)]
    assert took[_form(ny, nx, 300)] == 2 and sum(took) == 2


LAYOUTS = {   # (ldz - ny, z gap, parity of ldzi, zi gap, output offset in elements)
    "odd_ldzi_offset_8B": (3, 5, 1, 7, 1),
    "even_ldzi_aligned": (1, 1, 0, 4, 0),
    "odd_slice_stride": (0, 3, 0, 5, 0),
    "z_gap_only": (0, 2, 0, 0, 0),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("shape", [(29, 37, 257, 33, 7), (29, 37, 255, 9, 7), (64, 129, 257, 20, 5), (64, 129, 60, 33, 5)],
                         ids=lambda s: "x".join(map(str, s)))
def test_padding_gaps_and_alignment(mi_ctx, shape, layout):
    """ldz > ny with NaN in the padding rows, NaN in the gap between slices; ldzi > nyi and a zi gap whose sentinel must
    survive; zi 8-B but not 16-B aligned; odd ldzi; an odd zi slice stride"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    ny, nx, nyi, nxi, S = shape
    pad_z, gap_z, parity, gap_zi, off = LAYOUTS[layout]
    xg, yg, Z, xi, yi = _case(shape, seed=1)
    ldz, ldzi = ny + pad_z, nyi + 1 + ((nyi + 1 + parity) & 1)
    assert ldzi > nyi and ldzi % 2 == parity
    zstride, zistride = ldz * nx + gap_z, ldzi * nxi + gap_zi
    zbuf = torch.full((S * zstride,), math.nan, dtype=torch.float64, device="cuda")
    Zd = torch.as_strided(zbuf, (ny, nx, S), (1, ldz, zstride))
    Zd.copy_(torch.from_numpy(Z).cuda())
    obuf = torch.full((off + S * zistride + 2,), 123.0, dtype=torch.float64, device="cuda")
    out = torch.as_strided(obuf, (nyi, nxi, S), (1, ldzi, zistride), off)
    assert (out.data_ptr() % 16 == 8) == (off == 1)
    ax, ay = _axes(mi_ctx, xg, yg)
    before = _launches(mi_ctx._L)
    ret = mi.interp2_slices(mi_ctx, ax, ay, Zd, _t(xi), _t(yi), out=out, extrap=-1.0)
    assert ret.data_ptr() == out.data_ptr()
    assert [a - b for a, b in zip(_launches(mi_ctx._L), before)][_form(ny, nx, nyi)] == 1
    assert _eq(out.cpu().numpy(), _ref(xg, yg, Z, xi, yi, -1.0))
    written = torch.zeros_like(obuf, dtype=torch.bool)
    torch.as_strided(written, (nyi, nxi, S), (1, ldzi, zistride), off).fill_(True)
    untouched = obuf[~written].cpu().numpy()
    assert untouched.size == obuf.numel() - nyi * nxi * S and np.all(untouched == 123.0)


def test_explicit_axes_guess_and_binary_search_and_uniform_axes(mi_ctx):
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(3)
    t = cases.table("guess_bsearch")
    xg, yg = t["xg"], t["yg"]
    assert cases.axis_uses_guess(xg) and not cases.axis_uses_guess(yg)       # one axis of each search
    Z = rng.standard_normal((yg.size, xg.size, 4))
    ax, ay = _axes(mi_ctx, xg, yg)
    for nyi in (40, 300):
        xi, yi = _axis_queries(rng, xg, 70), _axis_queries(rng, yg, nyi)
        _assert_not_trivial(xg, yg, xi, yi)
        got = mi.interp2_slices(mi_ctx, ax, ay, _cube(Z), _t(xi), _t(yi)).cpu().numpy()
        assert _eq(got, _ref(xg, yg, Z, xi, yi))
    nx, ny = 40, 33
    x0, dx, y0, dy = -0.5, 2.0 / nx, 1.0, 3.0 / ny
    ux, uy = mi.Axis1.uniform(mi_ctx, x0, dx, nx), mi.Axis1.uniform(mi_ctx, y0, dy, ny)
    Z = rng.standard_normal((ny, nx, 3))
    for nyi in (33, 270):
        xi = _axis_queries(rng, x0 + dx * np.arange(nx), 50)
        yi = _axis_queries(rng, y0 + dy * np.arange(ny), nyi)
        px, py = _pairs(xi, yi)
        got = mi.interp2_slices(mi_ctx, ux, uy, _cube(Z), _t(xi), _t(yi), extrap=2.5).cpu().numpy()
        for s in range(3):
            ref = oracle.interp2_bilinear_uniform(x0, dx, nx, y0, dy, ny, Z[:, :, s], px, py, 2.5).reshape(nyi, 50, order="F")
            assert _eq(got[:, :, s], ref), s
            g = mi.Grid2.uniform(mi_ctx, x0, dx, nx, y0, dy, ny, Z[:, :, s])
            assert _eq(g.interp_grid(_t(xi), _t(yi), extrap=2.5).cpu().numpy(), got[:, :, s])
            g.close()


@pytest.mark.parametrize("nyi", [7, 300])
@pytest.mark.parametrize("name", cases.TABLES)
def test_edge_tables_as_slices(mi_ctx, name, nyi):
    """the tables of tests/interp2_cases.py (inf, NaN, -0.0 and denormals where a kernel must select, not multiply; ulp
    neighbours of every node as queries), each as every slice of a 3-slice stack with a different Z per slice: the sign
    of zero included"""
    import armadillocudalinearinterpolation_amd as mi
    t = cases.table(name)
    xg, yg = t["xg"], t["yg"]
    Z = np.stack([t["Z"], t["Zfinite"], np.ascontiguousarray(t["Z"][::-1, ::-1])], axis=2)
    if t["uniform"]:
        x0, dx, y0, dy = t["uniform"]
        ax, ay = mi.Axis1.uniform(mi_ctx, x0, dx, xg.size), mi.Axis1.uniform(mi_ctx, y0, dy, yg.size)
    else:
        ax, ay = _axes(mi_ctx, xg, yg)
    xi, yi = cases.grid_xi(xg), cases.grid_yi(yg, nyi, seed=nyi)
    px, py = cases.mesh_pairs(xi, yi)
    for extrap in (math.nan, -7.5):
        got = mi.interp2_slices(mi_ctx, ax, ay, _cube(Z), _t(xi), _t(yi), extrap=extrap).cpu().numpy()
        for s in range(3):
            ref = cases.reference(name, px, py, extrap, Z=Z[:, :, s]).reshape(nyi, xi.size, order="F")
            assert _eq(got[:, :, s], ref), (s, extrap)
            assert cases.same_bits(got[:, :, s], ref), (s, extrap)


@pytest.mark.parametrize("extrap", [-2.0, math.inf, math.nan])
@pytest.mark.parametrize("shape", [(29, 37, 300, 80, 3), (29, 37, 90, 80, 3), (100, 90, 300, 80, 3), (100, 90, 90, 80, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_non_finite_values_stay_in_their_slice_and_their_cells(mi_ctx, shape, extrap):
    """inf, NaN and -0.0 planted in slice 1 at special_places: the other slices are bit-equal to a run without them, and
    inside the slice only outputs whose four corners touch a planted value differ"""
    import armadillocudalinearinterpolation_amd as mi
    ny, nx, nyi, nxi, S = shape
    xg, yg, Z, xi, yi = _case(shape, seed=2)
    planted = Z.copy()
    places = cases.special_places(ny, nx)
    for (i, j), v in places.items():
        planted[i, j, 1] = v
    ax, ay = _axes(mi_ctx, xg, yg)
    clean = mi.interp2_slices(mi_ctx, ax, ay, _cube(Z), _t(xi), _t(yi), extrap=extrap).cpu().numpy()
    got = mi.interp2_slices(mi_ctx, ax, ay, _cube(planted), _t(xi), _t(yi), extrap=extrap).cpu().numpy()
    assert _eq(got, _ref(xg, yg, planted, xi, yi, extrap))
    for s in (0, 2):
        assert cases.same_bits(got[:, :, s], clean[:, :, s]), s
    px, py = _pairs(xi, yi)
    inr = cases.in_range(px, py, xg, yg)
    lx, rx = cases.brackets(xg, px[inr])
    ly, ry = cases.brackets(yg, py[inr])
    special = np.zeros((ny, nx), dtype=bool)
    for (i, j) in places:
        special[i, j] = True
    touched = np.zeros(px.size, dtype=bool)
    touched[inr] = special[ly, lx] | special[ry, lx] | special[ly, rx] | special[ry, rx]
    touched = touched.reshape(nyi, nxi, order="F")
    assert touched.any() and not touched.all()
    same = got[:, :, 1].view(np.int64) == clean[:, :, 1].view(np.int64)
    assert np.all(same[~touched])


def test_empty_calls_touch_nothing(mi_ctx):
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, h = mi_ctx._L, mi_ctx._h
    xg, yg, Z, xi, yi = _case((5, 6, 8, 9, 2))
    ax, ay = _axes(mi_ctx, xg, yg)
    Zd, xd, yd = _cube(Z), _t(xi), _t(yi)
    zi = torch.full((8 * 9 * 2,), 123.0, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    before = _launches(L)
    assert L.mi_interp2_slices_f64_dev(h, ax._h, ay._h, p(Zd), 5, 30, 0, p(xd), 9, p(yd), 8, p(zi), 8, 72, 0.0) == 0
    assert L.mi_interp2_slices_f64_dev(h, ax._h, ay._h, p(Zd), 5, 30, 2, p(xd), 0, p(yd), 8, p(zi), 8, 72, 0.0) == 0
    assert L.mi_interp2_slices_f64_dev(h, ax._h, ay._h, p(Zd), 5, 30, 2, p(xd), 9, p(yd), 0, p(zi), 8, 72, 0.0) == 0
    assert L.mi_interp2_slices_f64_dev(h, ax._h, ay._h, None, 0, 0, 0, None, 0, None, 0, None, 0, 0, 0.0) == 0
    torch.cuda.synchronize()
    assert _launches(L) == before and bool((zi == 123.0).all())
    empty = torch.empty(0, dtype=torch.float64, device="cuda")
    assert tuple(mi.interp2_slices(mi_ctx, ax, ay, Zd, empty, yd).shape) == (8, 0, 2)
    assert tuple(mi.interp2_slices(mi_ctx, ax, ay, Zd, xd, empty).shape) == (0, 9, 2)
    assert tuple(mi.interp2_slices(mi_ctx, ax, ay, Zd[:, :, :0], xd, yd).shape) == (8, 9, 0)
    # the strides of a single slice are ignored
    one = torch.full((8 * 9,), 123.0, dtype=torch.float64, device="cuda")
    assert L.mi_interp2_slices_f64_dev(h, ax._h, ay._h, p(Zd), 5, 0, 1, p(xd), 9, p(yd), 8, p(one), 8, 0, 0.0) == 0
    assert _eq(one.cpu().numpy().reshape(8, 9, order="F"), _ref(xg, yg, Z[:, :, :1], xi, yi, 0.0)[:, :, 0])


def test_argument_errors(mi_ctx):
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, h = mi_ctx._L, mi_ctx._h
    xg, yg, Z, xi, yi = _case((5, 6, 8, 9, 2))
    ax, ay = _axes(mi_ctx, xg, yg)
    a, b = ax._h, ay._h
    z, x, y = _cube(Z), _t(xi), _t(yi)
    zi = torch.full((8 * 9 * 2 + 2,), 123.0, dtype=torch.float64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    dev = L.mi_interp2_slices_f64_dev
    big = 2 ** 62
    cases_ = [
        ("mi_interp2_slices_f64_dev", lambda: dev(h, None, b, p(z), 5, 30, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, None, p(z), 5, 30, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, None, 5, 30, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, None, 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, p(x), 9, None, 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, p(x), 9, p(y), 8, None, 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z, 4), 5, 30, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, p(x, 4), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, p(x), 9, p(y, 4), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, p(x), 9, p(y), 8, p(zi, 4), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 4, 30, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),        # ldz < ny
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, p(x), 9, p(y), 8, p(zi), 7, 72, 0.0)),        # ldzi < nyi
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 29, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),        # z stride
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, p(x), 9, p(y), 8, p(zi), 8, 71, 0.0)),        # zi stride
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, 2, p(x), big, p(y), big, p(zi), big, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), big, 30, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, 30, big, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_f64_dev", lambda: dev(h, a, b, p(z), 5, big, 2, p(x), 9, p(y), 8, p(zi), 8, big, 0.0)),
    ]
    for name, call in cases_:
        assert call() == 1                                  # MI_ERR_INVALID_ARG
        assert name in L.mi_last_error(h).decode()
    torch.cuda.synchronize()
    assert bool((zi == 123.0).all())                        # nothing was written by a refused call
    with pytest.raises(ValueError):
        mi.interp2_slices(mi_ctx, ax, ay, _cube(Z).contiguous(), x, y)       # C order: not a cube layout
    with pytest.raises(ValueError):
        mi.interp2_slices(mi_ctx, ay, ax, _cube(Z), x, y)                    # the axes swapped: Z is (ny, nx, S)


def test_one_axis_object_for_both_axes(mi_ctx):
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(17)
    xg, _, Z = _table(rng, 31, 31, 3)
    ax = mi.Axis1.from_nodes(mi_ctx, xg)
    for nyi in (50, 280):
        xi, yi = _axis_queries(rng, xg, 45), _axis_queries(rng, xg, nyi)
        got = mi.interp2_slices(mi_ctx, ax, ax, _cube(Z), _t(xi), _t(yi)).cpu().numpy()
        assert _eq(got, _ref(xg, xg, Z, xi, yi))


def test_back_to_back_with_the_other_users_of_the_record_workspace(mi_ctx):
    """mi_interp2_grid_f64_dev and mi_interp1_cols_f64_dev keep their records in the same context slot: alternating
    calls on one stream, of growing and shrinking sizes, with no synchronisation in between"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(23)
    xg, yg, Z = _table(rng, 33, 45, 4)
    ax, ay = _axes(mi_ctx, xg, yg)
    grid = mi.Grid2.from_axes(mi_ctx, xg, yg, Z[:, :, 2])
    Zd = _cube(Z)
    Ycols = _t(Z[:, :, 0].T.copy()).T                       # (33, 45): 45 columns over the y axis
    results = []
    for nxi, nyi in ((40, 300), (900, 20), (7, 7), (300, 300), (64, 257)):
        xi, yi = _axis_queries(rng, xg, nxi), _axis_queries(rng, yg, nyi)
        xd, yd = _t(xi), _t(yi)
        s1 = mi.interp2_slices(mi_ctx, ax, ay, Zd, xd, yd, extrap=1.5)
        g = grid.interp_grid(xd, yd, extrap=1.5)
        c = ay.interp_cols(Ycols, yd, extrap=1.5)
        s2 = mi.interp2_slices(mi_ctx, ax, ay, Zd, xd, yd, extrap=1.5)
        results.append((xi, yi, s1, g, c, s2))
    for xi, yi, s1, g, c, s2 in results:
        ref = _ref(xg, yg, Z, xi, yi, 1.5)
        assert _eq(s1.cpu().numpy(), ref) and _eq(s2.cpu().numpy(), ref)
        assert _eq(g.cpu().numpy(), ref[:, :, 2])
        col = np.stack([oracle.interp1_arma(yg, Z[:, j, 0], yi, 1.5) for j in (0, 44)], axis=1)
        assert _eq(c.cpu().numpy()[:, [0, 44]], col)
    grid.close()


def test_every_form_runs_and_is_counted(mi_ctx):
    import armadillocudalinearinterpolation_amd as mi
    L = mi_ctx._L
    assert L.mi_debug_slices2_launches(-1) == 0 and L.mi_debug_slices2_launches(4) == 0
    for form, shape in ((LDS_TILE, (16, 16, 256, 9, 2)), (LDS_FLAT, (16, 16, 255, 9, 2)),
                        (DIRECT_TILE, (91, 91, 256, 9, 2)), (DIRECT_FLAT, (91, 91, 255, 9, 2))):
        xg, yg, Z, xi, yi = _case(shape)
        ax, ay = _axes(mi_ctx, xg, yg)
        before = _launches(L)
        got = mi.interp2_slices(mi_ctx, ax, ay, _cube(Z), _t(xi), _t(yi)).cpu().numpy()
        assert [a - b for a, b in zip(_launches(L), before)] == [int(f == form) for f in range(4)]
        assert _eq(got, _ref(xg, yg, Z, xi, yi))
    assert all(n > 0 for n in _launches(L))
