"""arma::interp2's gridded form (mi_interp2_grid_f64_dev / _host, mi_group_interp2_grid_f64_host, Grid2.interp_grid,
mi355::interp2 with an arma::mat ZI): ZI[i, j] = Z at (XI[j], YI[i]), bit-identical to the scattered call and to the
oracle on the meshgrid pairs, for every output shape, both table layouts, explicit and uniform axes."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "host")


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _pairs(xi, yi):
    """the meshgrid pairs in the column-major order of ZI: k = i + j*nyi"""
    XX, YY = np.meshgrid(xi, yi)                     # (nyi, nxi)
    return XX.ravel("F"), YY.ravel("F")


def _ref(xg, yg, Z, xi, yi, extrap=np.nan):
    px, py = _pairs(xi, yi)
    return oracle.interp2_bilinear(xg, yg, Z, px, py, extrap, nthreads=8).reshape(yi.size, xi.size, order="F")


def _axis_queries(rng, nodes, n):
    """unsorted queries over the axis, with points out of range on both sides, NaN and exact nodes"""
    lo, hi = nodes[0], nodes[-1]
    q = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n)
    if n >= 2:
        q[rng.integers(0, n, max(1, n // 5))] = nodes[rng.integers(0, nodes.size, max(1, n // 5))]
        q[rng.integers(0, n)] = hi
        q[rng.integers(0, n)] = lo
    if n >= 5:
        q[rng.integers(0, n)] = np.nan
    return q


def _table(rng, nx, ny):
    xg = np.cumsum(rng.uniform(0.2, 1.0, nx))
    yg = np.cumsum(rng.uniform(0.1, 2.0, ny)) - 3.0
    Z = rng.standard_normal((ny, nx))
    return xg, yg, Z


@pytest.fixture(scope="module")
def tables(mi_ctx):
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(20261016)
    xg, yg, Z = _table(rng, 53, 41)
    return {"xg": xg, "yg": yg, "Z": Z, "quad": mi.Grid2.from_axes(mi_ctx, xg, yg, Z),
            "compact": mi.Grid2.from_axes(mi_ctx, xg, yg, Z, compact=True)}


def test_golden_table(mi_ctx, golden_dir):
    import armadillocudalinearinterpolation_amd as mi
    g = np.load(os.path.join(golden_dir, "interp2_bilinear.npz"))
    xi, yi = g["XQ"][:300], g["YQ"][300:550]
    grid = mi.Grid2.from_axes(mi_ctx, g["xg"], g["yg"], g["Z"])
    got = grid.interp_grid(_t(xi), _t(yi)).cpu().numpy()
    assert got.shape == (yi.size, xi.size)
    assert _eq(got, _ref(g["xg"], g["yg"], g["Z"], xi, yi))
    px, py = _pairs(xi, yi)
    scattered = grid.interp(_t(px), _t(py)).cpu().numpy().reshape(yi.size, xi.size, order="F")
    assert _eq(got, scattered)
    assert _eq(grid.interp_grid_host(xi, yi), got)


@pytest.mark.parametrize("nxi", [1, 2, 7, 70001])
@pytest.mark.parametrize("nyi", [1, 2, 3, 63, 64, 65, 513])
def test_shapes_layouts_extrap(mi_ctx, tables, nxi, nyi):
    rng = np.random.default_rng(nxi * 1000 + nyi)
    xg, yg, Z = tables["xg"], tables["yg"], tables["Z"]
    xi, yi = _axis_queries(rng, xg, nxi), _axis_queries(rng, yg, nyi)
    for extrap in (math.nan, -3.25):
        ref = _ref(xg, yg, Z, xi, yi, extrap)
        for layout in ("quad", "compact"):
            got = tables[layout].interp_grid(_t(xi), _t(yi), extrap=extrap)
            assert tuple(got.shape) == (nyi, nxi) and got.T.is_contiguous()
            assert _eq(got.cpu().numpy(), ref), (layout, extrap)


@pytest.mark.parametrize("nxi,nyi", [(1, 1), (7, 3), (70001, 2), (5, 64), (9, 65), (3, 513), (2, 1030)])
def test_uniform_tables(mi_ctx, nxi, nyi):
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(nxi + 7 * nyi)
    nx, ny = 40, 33
    x0, dx, y0, dy = -0.5, 2.0 / nx, 1.0, 3.0 / ny
    Z = rng.standard_normal((ny, nx))
    xi = _axis_queries(rng, x0 + dx * np.arange(nx), nxi)
    yi = _axis_queries(rng, y0 + dy * np.arange(ny), nyi)
    px, py = _pairs(xi, yi)
    for compact in (False, True):
        g = mi.Grid2.uniform(mi_ctx, x0, dx, nx, y0, dy, ny, Z, compact=compact)
        for extrap in (math.nan, 2.5):
            ref = oracle.interp2_bilinear_uniform(x0, dx, nx, y0, dy, ny, Z, px, py, extrap).reshape(nyi, nxi, order="F")
            assert _eq(g.interp_grid(_t(xi), _t(yi), extrap=extrap).cpu().numpy(), ref), (compact, extrap)


@pytest.mark.parametrize("nxi,nyi", [(5, 1), (33, 3), (301, 64), (17, 513), (4, 1024)])
def test_output_offset_by_8_bytes(mi_ctx, tables, nxi, nyi):
    """a result pointer that is 8-B but not 16-B aligned: the 8-B store forms of both kernels"""
    import torch
    from armadillocudalinearinterpolation_amd._lib import check
    rng = np.random.default_rng(nxi * nyi)
    xg, yg, Z = tables["xg"], tables["yg"], tables["Z"]
    xi, yi = _axis_queries(rng, xg, nxi), _axis_queries(rng, yg, nyi)
    buf = torch.full((nxi * nyi + 2,), 123.0, dtype=torch.float64, device="cuda")
    grid = tables["quad"]
    L = grid._L
    xd, yd = _t(xi), _t(yi)
    check(L.mi_interp2_grid_f64_dev(mi_ctx._h, grid._h, C.c_void_p(xd.data_ptr()), nxi, C.c_void_p(yd.data_ptr()), nyi,
                                    C.c_void_p(buf.data_ptr() + 8), -1.0), mi_ctx._h)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert b[0] == 123.0 and b[-1] == 123.0                  # nothing written outside [1, 1 + nxi*nyi)
    assert _eq(b[1:-1].reshape(nyi, nxi, order="F"), _ref(xg, yg, Z, xi, yi, -1.0))


def test_empty_axes(mi_ctx, tables):
    import torch
    grid = tables["quad"]
    x = _t(np.array([1.0, 2.0, 3.0]))
    empty = torch.empty(0, dtype=torch.float64, device="cuda")
    assert tuple(grid.interp_grid(empty, x).shape) == (3, 0)
    assert tuple(grid.interp_grid(x, empty).shape) == (0, 3)
    assert grid.interp_grid_host(np.empty(0), np.ones(4)).shape == (4, 0)
    L = grid._L
    assert L.mi_interp2_grid_f64_dev(mi_ctx._h, grid._h, None, 0, None, 5, None, 0.0) == 0     # nothing launched


def test_against_independent_numpy_bilinear(mi_ctx):
    """not the oracle: a direct numpy bilinear on a smooth table, in-range points only, to 1e-12 relative"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(5)
    xg = np.sort(np.concatenate([[0.0, 4.0], rng.uniform(0.0, 4.0, 70)]))
    yg = np.sort(np.concatenate([[-2.0, 3.0], rng.uniform(-2.0, 3.0, 50)]))
    Z = np.exp(-0.1 * xg)[None, :] * (1.0 + np.cos(yg))[:, None] + 3.0
    xi, yi = rng.uniform(0.0, 4.0, 301), rng.uniform(-2.0, 3.0, 257)
    ix = np.clip(np.searchsorted(xg, xi, side="right") - 1, 0, xg.size - 2)
    iy = np.clip(np.searchsorted(yg, yi, side="right") - 1, 0, yg.size - 2)
    tx = (xi - xg[ix]) / (xg[ix + 1] - xg[ix])
    ty = (yi - yg[iy]) / (yg[iy + 1] - yg[iy])
    z00 = Z[iy[:, None], ix[None, :]]
    z01 = Z[iy[:, None] + 1, ix[None, :]]
    z10 = Z[iy[:, None], ix[None, :] + 1]
    z11 = Z[iy[:, None] + 1, ix[None, :] + 1]
    ty2, tx2 = ty[:, None], tx[None, :]
    ref = (1 - tx2) * ((1 - ty2) * z00 + ty2 * z01) + tx2 * ((1 - ty2) * z10 + ty2 * z11)
    for compact in (False, True):
        got = mi.Grid2.from_axes(mi_ctx, xg, yg, Z, compact=compact).interp_grid(_t(xi), _t(yi)).cpu().numpy()
        assert np.max(np.abs(got - ref) / np.abs(ref)) < 1e-12


def test_host_chunked_path_equals_dev(mi_ctx, tables):
    """more than 16.8 M outputs: the host call takes its chunked, pinned path (column chunks, copy back overlapped)"""
    rng = np.random.default_rng(11)
    xg, yg = tables["xg"], tables["yg"]
    grid = tables["compact"]
    for nxi, nyi in ((4100, 4096), (3, 6_000_001)):
        xi, yi = _axis_queries(rng, xg, nxi), _axis_queries(rng, yg, nyi)
        host = grid.interp_grid_host(xi, yi, extrap=0.5)
        dev = grid.interp_grid(_t(xi), _t(yi), extrap=0.5).cpu().numpy()
        assert host.shape == (nyi, nxi) and host.flags["F_CONTIGUOUS"]
        assert _eq(host, dev)
    assert mi_ctx._L.mi_debug_pinned_ranges() == 0


def test_argument_errors(mi_ctx, tables):
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, grid, h = mi_ctx._L, tables["quad"], mi_ctx._h
    x = torch.zeros(8, dtype=torch.float64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    cases = [
        ("mi_interp2_grid_f64_dev", lambda: L.mi_interp2_grid_f64_dev(h, None, p(x), 2, p(x), 2, p(x), 0.0)),
        ("mi_interp2_grid_f64_dev", lambda: L.mi_interp2_grid_f64_dev(h, grid._h, None, 2, p(x), 2, p(x), 0.0)),
        ("mi_interp2_grid_f64_dev", lambda: L.mi_interp2_grid_f64_dev(h, grid._h, p(x), 2, p(x), 2, None, 0.0)),
        ("mi_interp2_grid_f64_dev", lambda: L.mi_interp2_grid_f64_dev(h, grid._h, p(x, 4), 2, p(x), 2, p(x), 0.0)),
        ("mi_interp2_grid_f64_dev", lambda: L.mi_interp2_grid_f64_dev(h, grid._h, p(x), 2, p(x), 2, p(x, 4), 0.0)),
        ("mi_interp2_grid_f64_dev", lambda: L.mi_interp2_grid_f64_dev(h, grid._h, p(x), 2**62, p(x), 2**62, p(x), 0.0)),
        ("mi_interp2_grid_f64_host", lambda: L.mi_interp2_grid_f64_host(h, grid._h, None, 2, None, 2, None, 0.0)),
        ("mi_interp2_grid_f64_host", lambda: L.mi_interp2_grid_f64_host(h, None, None, 2, None, 2, None, 0.0)),
    ]
    for name, call in cases:
        assert call() == 1                                  # MI_ERR_INVALID_ARG
        assert name in L.mi_last_error(h).decode()
    grp = mi.Group([0])
    try:
        assert L.mi_group_interp2_grid_f64_host(grp._h, None, None, 2, None, 2, None, 0.0) == 1
        assert "mi_group_interp2_grid_f64_host" in L.mi_last_error(None).decode()
    finally:
        grp.close()


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
@pytest.mark.parametrize("nxi", [1, 2, 5, 1000])
def test_group_equals_single_context(mi_ctx, tables, devices, nxi):
    """columns sharded over the group (fewer and more columns than members): bit-equal to one context"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(nxi + len(devices))
    xg, yg, Z = tables["xg"], tables["yg"], tables["Z"]
    xi, yi = _axis_queries(rng, xg, nxi), _axis_queries(rng, yg, 300)
    single = tables["quad"].interp_grid(_t(xi), _t(yi), extrap=-2.0).cpu().numpy()
    grp = mi.Group(devices)
    try:
        gt = grp.grid2(xg, yg, Z)
        got = gt.interp_grid_host(xi, yi, extrap=-2.0)
        assert got.shape == (300, nxi)
        assert _eq(got, single)
        gt.close()
    finally:
        grp.close()


def test_cpp_arma_interp2_grid(tmp_path):
    """mi355::interp2(X, Y, Z, XI, YI, arma::mat& ZI) and GroupInterp2Table's gridded operator() from C++: ZI is
    YI.n_elem x XI.n_elem and bit-equal to the oracle; an arma::vec ZI still gets the scattered result"""
    from armadillocudalinearinterpolation_amd import _build as b
    b.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST, "arma_interp2_grid_test"])
    out = subprocess.run([os.path.join(HOST, "arma_interp2_grid_test"), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    dims = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in out.stdout.splitlines() if ln[:2] in ("ZI", "ZE", "ZS", "ZG")}
    rd = lambda f: np.fromfile(os.path.join(tmp_path, "g_%s.bin" % f), dtype=np.float64)  # noqa: E731
    X, Y, XI, YI = rd("X"), rd("Y"), rd("XI"), rd("YI")
    nxi, nyi = XI.size, YI.size
    Z = rd("Z").reshape(Y.size, X.size, order="F")
    assert dims["ZI"] == (nyi, nxi) and dims["ZE"] == (nyi, nxi) and dims["ZG"] == (nyi, nxi)
    assert dims["ZS"] == (nxi * nyi, 1)
    px, py = _pairs(XI, YI)
    ref = oracle.interp2_bilinear(X, Y, Z, px, py)
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    assert _eq(rd("ZI"), ref)
    assert _eq(rd("ZE"), oracle.interp2_bilinear(X, Y, Z, px, py, -7.5))
    assert _eq(rd("ZS"), ref)
    assert _eq(rd("ZG"), ref)
