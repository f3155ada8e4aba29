"""interp1 over the columns of a matrix (mi_axis1_*, mi_interp1_cols_f64_dev / _host, mi_group_interp1_cols_f64_host,
Axis1.interp_cols, mi355::Interp1Axis): YI[:, c] is interp1 of XI on the table (X, Y[:, c]).  The reference is the CPU
oracle column by column, oracle.interp1_bracket(X, Y[:, c], XI, extrap), and -- where B <= 64 -- a host-built
Grid1.from_nodes(X, Y[:, c], sanitise=False).interp(XI) on the device.  Both comparisons are
np.array_equal(..., equal_nan=True) on every output (plus the sign of zeros): no tolerance, no sampling.

Matrices are kept as C-contiguous (B, ld) buffers here: row c of the buffer is column c of the column-major matrix."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "host")
LDS_MAX_N = 8192          # kLdsMaxN in csrc/mi_cols1.hip: the LDS form up to here, the direct form beyond
ROW_BLOCK = 2048          # kRowBlock: outputs of one column per unit of work
SENTINEL = -12345.678


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _eq(a, b):
    """every element equal (NaN == NaN), and zeros carry the same sign"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & (a == 0), np.signbit(b) & (b == 0))


def _axis_queries(rng, nodes, n):
    """unsorted queries over the axis, with points out of range on both sides, NaN, both end nodes and interior nodes"""
    lo, hi = nodes[0], nodes[-1]
    q = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n)
    if n >= 2:
        q[rng.integers(0, n, max(1, n // 5))] = nodes[rng.integers(0, nodes.size, max(1, n // 5))]
        q[rng.integers(0, n)] = hi
        q[rng.integers(0, n)] = lo
    if n >= 5:
        q[rng.integers(0, n)] = np.nan
    return q


def _jittered(rng, n):
    return np.cumsum(rng.uniform(0.2, 1.0, n)) - 3.0


def _oracle_cols(X, Yb, xi, extrap=np.nan):
    """(B, nxi): row c = the oracle's interp1 on column c"""
    return np.stack([oracle.interp1_bracket(X, Yb[c], xi, extrap) for c in range(Yb.shape[0])]) if Yb.shape[0] else \
        np.empty((0, xi.size))


def _grid1_cols(ctx, X, Yb, xi, extrap=np.nan):
    """the same through a host-built 1-D table per column on the device"""
    import armadillocudalinearinterpolation_amd as mi
    xd = _t(xi)
    rows = []
    for c in range(Yb.shape[0]):
        g = mi.Grid1.from_nodes(ctx, X, Yb[c], sanitise=False)
        rows.append(g.interp(xd, extrap=extrap).cpu().numpy())
        g.close()
    return np.stack(rows)


def _run(ctx, axis, Yb, xi, extrap=np.nan, ldy_pad=0, ldyi_pad=0, misalign=False):
    """the device call on column-major views with padded leading dimensions: NaN below each column of Y (must not leak),
    a sentinel below each column of YI (must survive); misalign: yi 8-B but not 16-B aligned.  Returns (B, nxi)."""
    import torch
    B, n = Yb.shape
    nxi = xi.size
    buf = np.full((B, n + ldy_pad), np.nan)
    buf[:, :n] = Yb
    yd = _t(buf)
    ldyi = nxi + ldyi_pad
    flat = torch.full((B * ldyi + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    off = 0 if (flat.data_ptr() % 16 == 0) != misalign else 1
    ob = flat[off:off + B * ldyi].view(B, ldyi)
    assert (ob.data_ptr() % 16 != 0) == misalign
    got = axis.interp_cols(yd[:, :n].T, _t(xi), out=ob[:, :nxi].T, extrap=extrap)
    assert tuple(got.shape) == (nxi, B)
    h = flat.cpu().numpy()
    body = h[off:off + B * ldyi].reshape(B, ldyi)
    assert np.all(body[:, nxi:] == SENTINEL), "padding rows of YI were written"
    assert np.all(h[:off] == SENTINEL) and np.all(h[off + B * ldyi:] == SENTINEL), "wrote outside YI"
    return body[:, :nxi].copy()


def _check(ctx, axis, X, Yb, xi, extrap=np.nan, **kw):
    got = _run(ctx, axis, Yb, xi, extrap, **kw)
    assert _eq(got, _oracle_cols(X, Yb, xi, extrap))
    if Yb.shape[0] <= 64:
        assert _eq(got, _grid1_cols(ctx, X, Yb, xi, extrap))
    return got


@pytest.mark.parametrize("n", [2, 3, 1024, LDS_MAX_N - 1, LDS_MAX_N, LDS_MAX_N + 1, LDS_MAX_N + 2, 50_001])
def test_both_forms_and_the_switch_between_them(mi_ctx, n):
    """jittered explicit axes across the LDS-form limit; even and odd column lengths, so both load alignments run"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(100 + n)
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    for B, nxi, ldy_pad in [(5, 1500, 0), (4, 3001, 1)]:
        Yb = rng.standard_normal((B, n))
        _check(mi_ctx, axis, X, Yb, _axis_queries(rng, X, nxi), ldy_pad=ldy_pad)
    axis.close()


def test_closed_form_and_uniform_axes(mi_ctx):
    """a linspace-like explicit axis (mi_grid1 stores it in closed form: the bits must still agree), a device-resident
    explicit axis, and uniform axes (nodes fma(i, dx, x0); dx a power of two, so that x0 + i*dx is the same double)"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(7)
    for n in (1024, 20_000):
        X = np.linspace(-1.0, 2.0, n)
        Yb = rng.standard_normal((6, n))
        xi = _axis_queries(rng, X, 2500)
        g = mi.Grid1.from_nodes(mi_ctx, X, Yb[0], sanitise=False)
        assert g.info()["mode"] == 0, "the comparison table is meant to be a closed-form one"
        g.close()
        for axis in (mi.Axis1.from_nodes(mi_ctx, X), mi.Axis1.from_device_nodes(mi_ctx, _t(X))):
            _check(mi_ctx, axis, X, Yb, xi)
            axis.close()
        x0, dx = -3.0, 2.0 ** -6
        Xu = x0 + dx * np.arange(n)
        axis = mi.Axis1.uniform(mi_ctx, x0, dx, n)
        xi = _axis_queries(rng, Xu, 1777)
        got = _check(mi_ctx, axis, Xu, Yb, xi, extrap=4.25)
        xd = _t(xi)
        for c in range(Yb.shape[0]):
            gu = mi.Grid1.uniform(mi_ctx, x0, dx, Yb[c])
            assert _eq(got[c], gu.interp(xd, extrap=4.25).cpu().numpy())
            gu.close()
        axis.close()


@pytest.mark.parametrize("B", [1, 2, 3, 37, 1000])
@pytest.mark.parametrize("n", [257, 9000])
def test_column_counts(mi_ctx, B, n):
    """1, 2, 3 columns, counts that are no multiple of a workgroup's run of columns, in both forms"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(B * 31 + n)
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Yb = rng.standard_normal((B, n))
    _check(mi_ctx, axis, X, Yb, _axis_queries(rng, X, 700), extrap=-1.5)
    if B >= 37:   # several row blocks too: the run of columns per workgroup changes with nxi
        _check(mi_ctx, axis, X, Yb, _axis_queries(rng, X, 2 * ROW_BLOCK + 10), ldyi_pad=2)
    axis.close()


@pytest.mark.parametrize("n,B,nxi", [(64, 2 * 1366, 2 * ROW_BLOCK + 10), (1000, 2, ROW_BLOCK * 5000 + 3),
                                      (LDS_MAX_N + 8, 2, ROW_BLOCK * 5000 + 3)])
def test_workgroups_stride_over_the_work(mi_ctx, n, B, nxi):
    """more units of work than the launch has workgroups (16 per compute unit): by the column count on a 256-CU device
    (3 row blocks x 1366 runs = 4098 units), and by the row count on any device (5001 row blocks x 2 columns)"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(n + B)
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Yb = rng.standard_normal((B, n))
    xi = _axis_queries(rng, X, nxi)
    got = axis.interp_cols(_t(Yb).T, _t(xi)).T.cpu().numpy()
    assert got.shape == (B, nxi)
    for c in range(B):
        assert _eq(got[c], oracle.interp1_bracket(X, Yb[c], xi, np.nan, nthreads=8))
    axis.close()


@pytest.mark.parametrize("nxi", [1, 2, 7, 255, 256, 257, 511, 513, 2047, 2049, 5000])
def test_query_counts_leading_dimensions_and_store_widths(mi_ctx, nxi):
    """nxi of 1, odd, either side of 256 and of a row block, larger and smaller than n; ldy > n; ldyi > nxi odd and even
    and a yi that is 8-B but not 16-B aligned, so that both store widths run; padding rows checked by _run"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(nxi)
    for n in (600, 10_000):
        X = _jittered(rng, n)
        axis = mi.Axis1.from_nodes(mi_ctx, X)
        Yb = rng.standard_normal((7, n))
        xi = _axis_queries(rng, X, nxi)
        for ldy_pad, ldyi_pad, misalign in [(0, 0, False), (3, 1, False), (2, 2, False), (1, 0, True), (0, 3, True),
                                            (4, nxi % 2, False)]:
            _check(mi_ctx, axis, X, Yb, xi, extrap=9.0, ldy_pad=ldy_pad, ldyi_pad=ldyi_pad, misalign=misalign)
        axis.close()


@pytest.mark.parametrize("n", [500, 9001])
def test_inf_nan_and_negative_zero_stay_inside_their_column(mi_ctx, n):
    """inf, NaN and -0.0 at and beside bracket nodes go through the two-term blend as interp1 passes them (the oracle
    column by column), and the neighbouring columns' outputs are those of a call that never saw them"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(n)
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    B = 9
    clean = rng.standard_normal((B, n))
    Yb = clean.copy()
    k = n // 3
    Yb[1, k] = np.inf
    Yb[1, 0] = -np.inf
    Yb[3, k] = np.nan
    Yb[3, n - 1] = np.nan
    Yb[5, k] = -0.0
    Yb[5, k + 1] = -0.0
    Yb[5, n - 1] = -0.0
    Yb[5, 0] = -0.0
    Yb[7, n - 1] = np.inf
    Yb[7, n - 2] = -0.0
    xi = _axis_queries(rng, X, 1200)
    # at, beside and between the special nodes
    xi[:12] = [X[k], X[k - 1], X[k + 1], 0.5 * (X[k] + X[k + 1]), 0.5 * (X[k - 1] + X[k]), X[0], X[n - 1], X[n - 2],
               0.5 * (X[n - 2] + X[n - 1]), np.nextafter(X[k], np.inf), np.nextafter(X[k], -np.inf), 0.5 * (X[0] + X[1])]
    got = _check(mi_ctx, axis, X, Yb, xi, extrap=np.inf)
    assert np.isinf(got[1]).any() and np.isnan(got[3]).any() and (np.signbit(got[5]) & (got[5] == 0)).any()
    base = _run(mi_ctx, axis, clean, xi, np.inf)
    for c in (0, 2, 4, 6, 8):
        assert _eq(got[c], base[c])
    axis.close()


@pytest.mark.parametrize("extrap", [2.5, -0.0, np.inf, -np.inf, np.nan])
def test_extrapolation_values(mi_ctx, extrap):
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(5)
    for n in (300, 8500):
        X = _jittered(rng, n)
        axis = mi.Axis1.from_nodes(mi_ctx, X)
        xi = _axis_queries(rng, X, 900)
        got = _check(mi_ctx, axis, X, rng.standard_normal((4, n)), xi, extrap=extrap)
        oor = (xi < X[0]) | (xi > X[-1])
        assert oor.any() and np.isnan(got[:, np.isnan(xi)]).all()
        if not np.isnan(extrap):
            assert np.all(got[:, oor] == extrap) and np.all(np.signbit(got[:, oor]) == np.signbit(extrap))
        axis.close()


def test_empty_calls_and_argument_errors(mi_ctx):
    """B == 0 or nxi == 0 is MI_OK with nothing launched; MI_ERR_GRID for a non-increasing and for a NaN X;
    MI_ERR_INVALID_ARG for ldy < n, ldyi < nxi, misaligned or NULL pointers -- each with a mi_last_error text"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, ch = mi_ctx._L, mi_ctx._h
    n, B, nxi = 50, 4, 30
    X = np.linspace(0.0, 1.0, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    y = torch.zeros(B * n + 1, dtype=torch.float64, device="cuda")
    xi = torch.full((nxi + 1,), 0.5, dtype=torch.float64, device="cuda")
    yi = torch.full((B * nxi + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    p = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)  # noqa: E731

    def call(fn=L.mi_interp1_cols_f64_dev, yp=p(y), ldy=n, ncols=B, xp=p(xi), m=nxi, op=p(yi), ldyi=nxi):
        return fn(ch, axis._h, yp, ldy, ncols, xp, m, op, ldyi, 0.0)

    def err():
        return (L.mi_last_error(ch) or b"").decode()

    assert call() == 0
    torch.cuda.synchronize()
    yi.fill_(SENTINEL)
    assert call(ncols=0) == 0 and call(m=0) == 0 and call(ncols=0, yp=None, op=None) == 0 and call(m=0, xp=None) == 0
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()), "an empty call wrote something"
    hy, hx, ho = np.zeros(B * n), np.full(nxi, 0.5), np.full(B * nxi, SENTINEL)
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert call(L.mi_interp1_cols_f64_host, hp(hy), n, 0, hp(hx), nxi, hp(ho), nxi) == 0
    assert call(L.mi_interp1_cols_f64_host, hp(hy), n, B, hp(hx), 0, hp(ho), nxi) == 0
    assert np.all(ho == SENTINEL)
    INVALID, GRID = 1, 2
    for kw, word in [(dict(ldy=n - 1), "ldy"), (dict(ldyi=nxi - 1), "ldyi"), (dict(yp=p(y, 4)), "aligned"),
                     (dict(xp=p(xi, 4)), "aligned"), (dict(op=p(yi, 4)), "aligned"), (dict(yp=None), "NULL"),
                     (dict(xp=None), "NULL"), (dict(op=None), "NULL")]:
        assert call(**kw) == INVALID, kw
        assert word in err(), (kw, err())
    assert L.mi_interp1_cols_f64_dev(ch, None, p(y), n, B, p(xi), nxi, p(yi), nxi, 0.0) == INVALID and "NULL" in err()
    for fn in (L.mi_interp1_cols_f64_host,):
        assert call(fn, hp(hy), n - 1, B, hp(hx), nxi, hp(ho), nxi) == INVALID and "ldy" in err()
        assert call(fn, hp(hy), n, B, hp(hx), nxi, hp(ho), nxi - 1) == INVALID and "ldyi" in err()
        assert call(fn, None, n, B, hp(hx), nxi, hp(ho), nxi) == INVALID and "NULL" in err()
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()) and np.all(ho == SENTINEL), "a refused call wrote something"
    # 8-B aligned pointers that are not 16-B aligned are fine
    assert call(yp=p(y, 8), xp=p(xi, 8), op=p(yi, 8)) == 0
    torch.cuda.synchronize()
    # the axis: X is not sorted or de-duplicated for the caller
    h = C.c_void_p()
    for bad, word in [(np.array([0.0, 1.0, 1.0, 2.0]), "increasing"), (np.array([0.0, 2.0, 1.0, 3.0]), "increasing"),
                      (np.array([0.0, np.nan, 1.0]), "finite"), (np.array([0.0, 1.0, np.inf]), "finite"),
                      (np.array([1.0]), "two nodes")]:
        assert L.mi_axis1_create(ch, hp(bad), bad.size, 0, C.byref(h)) == GRID, bad
        assert word in err() and not h.value
        with pytest.raises(mi.MiError):
            mi.Axis1.from_nodes(mi_ctx, bad)
    assert L.mi_axis1_create(ch, hp(X), n, 0x1, C.byref(h)) == INVALID and "flags" in err()      # no MI_GRID_SANITISE here
    assert L.mi_axis1_create(ch, None, n, 0, C.byref(h)) == INVALID and "NULL" in err()
    assert L.mi_axis1_create_uniform(ch, 0.0, 0.0, 10, C.byref(h)) == GRID and L.mi_axis1_create_uniform(ch, 0.0, -1.0, 10, C.byref(h)) == GRID
    assert L.mi_axis1_create_uniform(ch, np.nan, 1.0, 10, C.byref(h)) == GRID and "mi_axis1_create_uniform" in err()
    assert L.mi_axis1_create_uniform(ch, 0.0, 1.0, 1, C.byref(h)) == GRID
    assert L.mi_axis1_destroy(None) == 0
    with pytest.raises(ValueError):
        axis.interp_cols(torch.zeros((B, n), dtype=torch.float64, device="cuda"), xi[:nxi])          # (B, n), not (n, B)
    with pytest.raises(ValueError):
        axis.interp_cols(torch.zeros((n, B), dtype=torch.float64, device="cuda"), xi[:nxi])          # row-major (n, B)
    axis.close()


def test_ensemble_at_scale(mi_ctx):
    """the shape the call is for: 125 000 realisations of a 1024-point state moved to a 2048-point mesh (1 GB in, 2 GB
    out on the device), every output against the oracle"""
    import armadillocudalinearinterpolation_amd as mi
    n, B, nxi = 1024, 125_000, 2048
    rng = np.random.default_rng(2026)
    X = _jittered(rng, n)
    Yb = rng.standard_normal((B, n))                    # column c of the matrix = row c of this buffer
    xi = _axis_queries(rng, X, nxi)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    got = axis.interp_cols(_t(Yb).T, _t(xi), extrap=-2.0).T.cpu().numpy()
    assert got.shape == (B, nxi)
    bad = [c for c in range(B) if not _eq(got[c], oracle.interp1_bracket(X, Yb[c], xi, -2.0))]
    assert not bad, "%d columns differ, first %s" % (len(bad), bad[:5])
    axis.close()


def test_back_to_back_with_the_gridded_interp2_call(mi_ctx):
    """both calls keep their records in context scratch slot 3: interleaved on one context and stream, without a
    synchronisation in between, each still gives its own result"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(33)
    nx, ny = 70, 90
    xg, yg = np.cumsum(rng.uniform(0.2, 1.0, nx)), np.cumsum(rng.uniform(0.1, 2.0, ny)) - 3.0
    Z = rng.standard_normal((ny, nx))
    g2 = mi.Grid2.from_axes(mi_ctx, xg, yg, Z)
    gx, gy = _axis_queries(rng, xg, 3000), _axis_queries(rng, yg, 700)
    n, B = 1500, 40
    X = _jittered(rng, n)
    Yb = rng.standard_normal((B, n))
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    xi_small, xi_big = _axis_queries(rng, X, 100), _axis_queries(rng, X, 6000)
    yd, gxd, gyd, xs, xb = _t(Yb), _t(gx), _t(gy), _t(xi_small), _t(xi_big)
    torch.cuda.synchronize()
    a1 = axis.interp_cols(yd.T, xb)
    z1 = g2.interp_grid(gxd, gyd)
    a2 = axis.interp_cols(yd.T, xs)
    z2 = g2.interp_grid(gxd, gyd)
    a3 = axis.interp_cols(yd.T, xb)
    torch.cuda.synchronize()
    XX, YY = np.meshgrid(gx, gy)
    zref = oracle.interp2_bilinear(xg, yg, Z, XX.ravel("F"), YY.ravel("F"), np.nan, nthreads=8).reshape(gy.size, gx.size, order="F")
    assert _eq(z1.cpu().numpy(), zref) and _eq(z2.cpu().numpy(), zref)
    assert _eq(a1.T.cpu().numpy(), _oracle_cols(X, Yb, xi_big)) and _eq(a3.T.cpu().numpy(), _oracle_cols(X, Yb, xi_big))
    assert _eq(a2.T.cpu().numpy(), _oracle_cols(X, Yb, xi_small))
    axis.close()
    g2.close()


def test_host_path_below_and_above_its_chunking_threshold(mi_ctx, monkeypatch):
    """one-shot and chunked (more than 2 x 8 M elements: pinned, pipelined column chunks) host calls equal the device
    call; nothing stays pinned afterwards, also after a failure forced in the middle of the chunk loop"""
    import armadillocudalinearinterpolation_amd as mi
    L = mi_ctx._L
    rng = np.random.default_rng(11)
    n, nxi = 1024, 2048
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    xi = _axis_queries(rng, X, nxi)
    assert L.mi_debug_pinned_ranges() == 0
    for B in (50, 9001):                                # 9001 x 2048 > 2 x 8 M: three chunks of 4096 columns
        Yb = rng.standard_normal((B, n))
        dev = axis.interp_cols(_t(Yb).T, _t(xi), extrap=1.5).T.cpu().numpy()
        got = axis.interp_cols_host(Yb.T, xi, extrap=1.5)
        assert got.shape == (nxi, B) and got.flags["F_CONTIGUOUS"]
        assert _eq(got.T, dev) and L.mi_debug_pinned_ranges() == 0
        idx = np.arange(0, B, 97)
        assert _eq(dev[idx], _oracle_cols(X, Yb[idx], xi, 1.5))
        # padded leading dimensions on the host side
        ldy, ldyi = n + 3, nxi + 5
        hy = np.full((B, ldy), np.nan)
        hy[:, :n] = Yb
        ho = np.full((B, ldyi), SENTINEL)
        st = L.mi_interp1_cols_f64_host(mi_ctx._h, axis._h, C.c_void_p(hy.ctypes.data), ldy, B, C.c_void_p(xi.ctypes.data), nxi,
                                        C.c_void_p(ho.ctypes.data), ldyi, 1.5)
        assert st == 0 and L.mi_debug_pinned_ranges() == 0
        assert _eq(ho[:, :nxi], dev) and np.all(ho[:, nxi:] == SENTINEL)
    monkeypatch.setenv("MI_TEST_FAIL_COLS_CHUNK", "1")
    with pytest.raises(mi.MiError) as e:
        axis.interp_cols_host(Yb.T, xi)
    assert "MI_TEST_FAIL_COLS_CHUNK" in str(e.value) and L.mi_debug_pinned_ranges() == 0
    monkeypatch.delenv("MI_TEST_FAIL_COLS_CHUNK")
    assert _eq(axis.interp_cols_host(Yb.T, xi, extrap=1.5).T, dev) and L.mi_debug_pinned_ranges() == 0
    axis.close()


def _group_devices():
    import torch
    return {"single": [0], "rehearsal": [0, 0, 0], "all_gpus": list(range(max(1, torch.cuda.device_count())))}


@pytest.mark.parametrize("which", ["single", "rehearsal", "all_gpus"])
def test_group_call_shards_the_columns(mi_ctx, which):
    """member r takes the columns mi_shard_bounds(B, r, P); B smaller than, equal to and not divisible by P; bit-equal
    to the single-device call.  all_gpus is [0, 1, ..] over every device of the machine ([0] on a single-GPU one)"""
    import armadillocudalinearinterpolation_amd as mi
    devices = _group_devices()[which]
    P = len(devices)
    grp = mi.Group(devices)
    rng = np.random.default_rng(P)
    for n in (400, 9000):
        X = _jittered(rng, n)
        axis = mi.Axis1.from_nodes(mi_ctx, X)
        xi = _axis_queries(rng, X, 1300)
        for B in sorted({1, max(P - 1, 1), P, 2 * P, 37, 8 * P + 3}):
            Yb = rng.standard_normal((B, n))
            one = axis.interp_cols(_t(Yb).T, _t(xi), extrap=-4.0).T.cpu().numpy()
            got = grp.interp_cols_host(X, Yb.T, xi, extrap=-4.0)
            assert got.shape == (xi.size, B)
            assert _eq(got.T, one) and _eq(one, _oracle_cols(X, Yb, xi, -4.0))
        axis.close()
    assert mi_ctx._L.mi_debug_pinned_ranges() == 0
    with pytest.raises(mi.MiError) as e:
        grp.interp_cols_host(np.array([0.0, 1.0, 1.0]), np.zeros((3, 2)), np.array([0.5]))
    assert e.value.code == 2 and "increasing" in str(e.value)
    assert grp.interp_cols_host(X, np.zeros((n, 0)), xi).shape == (xi.size, 0)
    grp.close()


def test_cpp_arma_interp1_cols(tmp_path):
    """mi355::Interp1Axis, mi355::interp1 with matrices and GroupInterp1Axis from C++: YI is XI.n_elem x Y.n_cols and
    bit-equal to the oracle and to the arma::vec overload column by column"""
    from armadillocudalinearinterpolation_amd import _build as b
    b.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST, "arma_interp1_cols_test"])
    out = subprocess.run([os.path.join(HOST, "arma_interp1_cols_test"), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    dims = {w[0]: (int(w[1]), int(w[2])) for w in lines if w and w[0] in ("YA", "YE", "YO", "YG")}
    assert ["threw", "1"] in lines, "a Y with the wrong row count must throw std::invalid_argument"
    rd = lambda f: np.fromfile(os.path.join(tmp_path, "c_%s.bin" % f), dtype=np.float64)  # noqa: E731
    X, XI = rd("X"), rd("XI")
    n, nxi = X.size, XI.size
    Yb = rd("Y").reshape(-1, n)                        # column-major n x B on disk = (B, n) rows
    B = Yb.shape[0]
    assert all(dims[k] == (nxi, B) for k in ("YA", "YE", "YO", "YG"))
    ref = _oracle_cols(X, Yb, XI)
    assert np.isnan(ref).any() and not np.isnan(ref).all() and np.isinf(ref).any()
    for k in ("YA", "YO", "YV", "YG"):
        assert _eq(rd(k).reshape(B, nxi), ref), k
    assert _eq(rd("YE").reshape(B, nxi), _oracle_cols(X, Yb, XI, -7.5))
