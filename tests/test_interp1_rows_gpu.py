"""interp1 along the rows of a matrix (mi_interp1_rows_f64_dev, mi_debug_rows1_launches, Axis1.interp_rows,
Axis1.interp_stack): YI[r, :] is interp1 of XI on the table (X, Y[r, :]).  The reference is the CPU oracle row by row,
oracle.interp1_bracket(X, Y[r, :], XI, extrap), for EVERY row, and -- where a test says so -- Axis1.interp_cols on the
transposed matrix.  Both comparisons are np.array_equal(..., equal_nan=True) on every output plus the sign of zeros: no
tolerance, no sampling.

Matrices are (m, n) numpy arrays here; on the device they are C-contiguous (n, ld) "time-major" buffers, row k of the
buffer being column k of the column-major matrix."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "csrc")
SENTINEL = -12345.678


def _constants():
    """kRowBlock and kThinM as csrc/mi_rows1.hip states them"""
    text = open(os.path.join(CSRC, "mi_rows1.hip")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(CSRC, "mi_interp2_eval.hpp")).read()).group(1))
    rb = int(re.search(r"^constexpr size_t kRowBlock = (\d+);", text, flags=re.M).group(1))
    thin = re.search(r"^constexpr size_t kThinM = (\w+);", text, flags=re.M).group(1)
    return rb, (block if thin == "kBlock" else int(thin))


RB, T = _constants()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _eq(a, b):
    """every element equal (NaN == NaN), and zeros carry the same sign"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & (a == 0), np.signbit(b) & (b == 0))


def _jittered(rng, n):
    return np.cumsum(rng.uniform(0.2, 1.0, n)) - 3.0


def _mixed_queries(rng, nodes, n):
    """unsorted queries over the axis, with points out of range on both sides, NaN, both end nodes and interior nodes"""
    lo, hi = nodes[0], nodes[-1]
    q = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n)
    if n >= 8:
        k = np.arange(n)
        rng.shuffle(k)
        q[k[0]], q[k[1]], q[k[2]], q[k[3]], q[k[4]] = lo, hi, np.nan, lo - 1.0, hi + 1.0
        q[k[5]] = nodes[nodes.size // 2]
        q[k[6]] = nodes[1 if nodes.size > 2 else 0]
        q[k[7]] = nodes[-2]
    return q


def _oracle_rows(X, Y, xi, extrap=np.nan):
    """(m, nxi): row r = the oracle's interp1 on the table (X, Y[r, :]), every row"""
    return np.stack([oracle.interp1_bracket(X, Y[r], xi, extrap) for r in range(Y.shape[0])]) if Y.shape[0] else \
        np.empty((0, xi.size))


def _forms(ctx):
    return [int(ctx._L.mi_debug_rows1_launches(f)) for f in range(3)]


def _run(ctx, axis, Y, xi, extrap=np.nan, ldy_pad=0, ldyi_pad=0, misalign=False, form=None):
    """the device call on column-major views with padded leading dimensions: NaN in the padding rows of y (must not
    leak), a sentinel in the padding rows of yi and around the buffer (must survive); misalign: y and yi 8-B but not
    16-B aligned.  form: the one counter of mi_debug_rows1_launches that must move, by one.  Returns (m, nxi)."""
    import torch
    m, n = Y.shape
    nxi = xi.size
    ldy, ldyi = m + ldy_pad, m + ldyi_pad
    yflat = torch.full((n * ldy + 2,), np.nan, dtype=torch.float64, device="cuda")
    yoff = 0 if (yflat.data_ptr() % 16 == 0) != misalign else 1
    hy = np.full((n, ldy), np.nan)
    hy[:, :m] = Y.T
    yb = yflat[yoff:yoff + n * ldy].view(n, ldy)
    yb.copy_(_t(hy))
    flat = torch.full((nxi * ldyi + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    off = 0 if (flat.data_ptr() % 16 == 0) != misalign else 1
    ob = flat[off:off + nxi * ldyi].view(nxi, ldyi)
    assert (ob.data_ptr() % 16 != 0) == misalign and (yb.data_ptr() % 16 != 0) == misalign
    before = _forms(ctx)
    got = axis.interp_rows(yb[:, :m].T, _t(xi), out=ob[:, :m].T, extrap=extrap)
    assert tuple(got.shape) == (m, nxi)
    h = flat.cpu().numpy()
    after = _forms(ctx)
    if form is not None:
        assert [a - b for a, b in zip(after, before)] == [int(f == form) for f in range(3)], (before, after, form)
    body = h[off:off + nxi * ldyi].reshape(nxi, ldyi)
    assert np.all(body[:, m:] == SENTINEL), "padding rows of YI were written"
    assert np.all(h[:off] == SENTINEL) and np.all(h[off + nxi * ldyi:] == SENTINEL), "wrote outside YI"
    return body[:, :m].T.copy()


def _cols(axis, Y, xi, extrap=np.nan):
    """(m, nxi) through Axis1.interp_cols on the transposed matrix: Y's rows as the columns of an (n, m) matrix"""
    return axis.interp_cols(_t(Y).T, _t(xi), extrap=extrap).T.cpu().numpy()


@pytest.mark.parametrize("m", [1, 2, 3, T - 1, T, T + 1, RB - 1, RB, RB + 1, 2 * RB + 3])
def test_row_counts_and_forms(mi_ctx, m):
    """row counts around the flat / tile threshold and around a row block, each with dense, padded and misaligned
    operands: the flat body below kThinM; the tile body with 16-B accesses when y and yi are 16-B aligned and both leading
    dimensions even, with 8-B accesses otherwise -- mi_debug_rows1_launches moves by one in exactly that form"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(1000 + m)
    n, nxi = 7, 37
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Y = rng.standard_normal((m, n))
    xi = _mixed_queries(rng, X, nxi)
    want = _oracle_rows(X, Y, xi, -7.25)
    for ldy_pad, ldyi_pad, misalign in [(0, 0, False), (1, 0, False), (0, 1, False), (3, 5, True)]:
        even = (m + ldy_pad) % 2 == 0 and (m + ldyi_pad) % 2 == 0
        form = 2 if m < T else (0 if even and not misalign else 1)
        got = _run(mi_ctx, axis, Y, xi, -7.25, ldy_pad, ldyi_pad, misalign, form=form)
        assert _eq(got, want), (m, ldy_pad, ldyi_pad, misalign)
    axis.close()


def _cache_sequences(X):
    n = X.size
    mid = lambda k, f=0.3: X[k] + f * (X[k + 1] - X[k])  # noqa: E731
    below, above, nan = X[0] - 1.0, X[-1] + 1.0, np.nan
    return {
        "ascending with repeats inside a cell": [mid(0, .1), mid(0, .5), mid(0, .5), mid(1), mid(1, .7), mid(1, .9), mid(3), mid(4), mid(4, .8)],
        "every node exactly, in order": list(X),
        "the last node three times, then the cell before it": [X[-1], X[-1], X[-1], mid(n - 2), mid(n - 2, .9)],
        "strictly descending": [X[-1]] + [mid(k) for k in range(n - 2, -1, -1)] + [X[0]],
        "alternating first and last cell": [mid(0), mid(n - 2), mid(0, .6), mid(n - 2, .2), mid(0), mid(n - 2)],
        "flagged between two queries of the same cell": [mid(2), nan, mid(2, .6), below, mid(2, .7), above, mid(2, .1)],
        "flagged between two queries of adjacent cells": [mid(1), nan, mid(2), below, mid(3), above, mid(4)],
        "all flagged": [nan, below, above, nan],
        "a single query": [mid(3)],
        "a single flagged query": [below],
    }


@pytest.mark.parametrize("which", range(10))
def test_register_cache_sequences(mi_ctx, which):
    """hand-written query sequences through every branch of the tile body's two-column cache: nothing to load, the
    right column moving over, both columns new, the last node (one column), flagged records in between"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(77)
    n, m = 6, RB + 1
    X = _jittered(rng, n)
    name, xi = list(_cache_sequences(X).items())[which]
    xi = np.array(xi)
    Y = rng.standard_normal((m, n))
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    want = _oracle_rows(X, Y, xi, 3.5)
    assert _eq(_run(mi_ctx, axis, Y, xi, 3.5, form=1), want), name                     # m odd: 8-B accesses
    # (a single output column has no leading dimension of its own: the wrapper passes ldyi = m, which is odd here)
    assert _eq(_run(mi_ctx, axis, Y, xi, 3.5, ldy_pad=1, ldyi_pad=3, form=0 if xi.size > 1 else 1), want), name
    assert _eq(_run(mi_ctx, axis, Y[:5], xi, 3.5, form=2), want[:5]), name             # and the flat body
    axis.close()


@pytest.mark.parametrize("n,nxi,m,order", [(1024, 5000, 600, "sorted"), (1024, 5000, 600, "permuted"),
                                           (50, 20_000, 5, "sorted"), (50, 20_000, RB + 1, "sorted"),
                                           (50, 20_000, RB + 1, "permuted")])
def test_long_runs_and_run_boundaries(mi_ctx, n, nxi, m, order):
    """more output columns than one workgroup takes: the columns are cut into runs, and every run starts with an empty
    cache; against the oracle and against interp_cols on the transpose"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(n + nxi + m)
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Y = rng.standard_normal((m, n))
    xi = np.sort(rng.uniform(X[0], X[-1], nxi))
    xi[0], xi[-1] = X[0], X[-1]
    if order == "permuted":
        xi = rng.permutation(xi)
    got = _run(mi_ctx, axis, Y, xi, form=2 if m < T else None)
    assert _eq(got, _oracle_rows(X, Y, xi))
    assert _eq(got, _cols(axis, Y, xi))
    axis.close()


@pytest.mark.parametrize("kind", ["two nodes", "uniform", "linspace", "clustered", "device"])
def test_axes(mi_ctx, kind):
    """n = 2; a uniform axis with dx a power of two (fma(i, dx, x0) is then x0 + i*dx exactly); a linspace-like explicit
    axis; a clustered axis, which takes the binary search; an axis whose nodes are already on the device"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(len(kind))
    if kind == "two nodes":
        X = np.array([-1.5, 2.25])
        axis = mi.Axis1.from_nodes(mi_ctx, X)
    elif kind == "uniform":
        x0, dx, n = -3.0, 2.0 ** -4, 33
        X = x0 + dx * np.arange(n)
        axis = mi.Axis1.uniform(mi_ctx, x0, dx, n)
    elif kind == "linspace":
        X = np.linspace(-1.0, 2.0, 41)
        axis = mi.Axis1.from_nodes(mi_ctx, X)
    elif kind == "clustered":
        X = np.concatenate([np.linspace(0.0, 1e-3, 40), np.linspace(1.0, 2.0, 5), 100.0 + np.linspace(0.0, 1e-6, 30)])
        axis = mi.Axis1.from_nodes(mi_ctx, X)
    else:
        X = _jittered(rng, 19)
        axis = mi.Axis1.from_device_nodes(mi_ctx, _t(X))
    for m in (T + 3, 3):
        Y = rng.standard_normal((m, X.size))
        xi = _mixed_queries(rng, X, 301)
        got = _run(mi_ctx, axis, Y, xi, 0.5)
        assert _eq(got, _oracle_rows(X, Y, xi, 0.5)), (kind, m)
        assert _eq(got, _cols(axis, Y, xi, 0.5)), (kind, m)
    axis.close()


@pytest.mark.parametrize("m", [T + 3, 3])
def test_non_finite_values_stay_inside_their_row(mi_ctx, m):
    """inf, -inf, NaN and -0.0 at the first, an interior and the last node of a few rows go through the two-term blend as
    interp1 passes them (the oracle row by row); every other row equals the run that never saw them"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(m)
    n = 9
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    clean = rng.standard_normal((m, n))
    Y = clean.copy()
    k = n // 2
    rows = [0, m - 1] if m == 3 else [1, 2, m - 1, T, 64]
    specials = [np.inf, -np.inf, np.nan, -0.0]
    for j, r in enumerate(rows):
        Y[r, 0] = specials[j % 4]
        Y[r, k] = specials[(j + 1) % 4]
        Y[r, n - 1] = specials[(j + 2) % 4]
    Y[rows[0], k + 1] = -0.0
    Y[rows[0], k] = -0.0
    xi = _mixed_queries(rng, X, 200)
    xi[:12] = [X[k], X[k - 1], X[k + 1], 0.5 * (X[k] + X[k + 1]), 0.5 * (X[k - 1] + X[k]), X[0], X[n - 1], X[n - 2],
               0.5 * (X[n - 2] + X[n - 1]), np.nextafter(X[k], np.inf), np.nextafter(X[k], -np.inf), 0.5 * (X[0] + X[1])]
    got = _run(mi_ctx, axis, Y, xi, 1.25)
    want = _oracle_rows(X, Y, xi, 1.25)
    assert _eq(got, want)
    assert np.isinf(got[rows]).any() and np.isnan(got[rows][:, ~np.isnan(xi)]).any() and (np.signbit(got[rows]) & (got[rows] == 0)).any()
    base = _run(mi_ctx, axis, clean, xi, 1.25)
    others = [r for r in range(m) if r not in rows]
    assert _eq(got[others], base[others])
    axis.close()


@pytest.mark.parametrize("extrap", [2.5, np.inf, None])
def test_extrapolation_values(mi_ctx, extrap):
    """a finite value, inf, and the default (NaN) outside [x[0], x[n-1]]; NaN for a NaN query whatever extrap is"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(5)
    X = _jittered(rng, 12)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    xi = _mixed_queries(rng, X, 90)
    oor = (xi < X[0]) | (xi > X[-1])
    assert oor.any() and np.isnan(xi).any()
    for m in (T + 1, 4):
        Y = rng.standard_normal((m, X.size))
        if extrap is None:
            got = axis.interp_rows(_t(Y.T).T, _t(xi)).cpu().numpy()
            assert np.isnan(got[:, oor]).all()
            assert _eq(got, _oracle_rows(X, Y, xi))
        else:
            got = _run(mi_ctx, axis, Y, xi, extrap)
            assert np.all(got[:, oor] == extrap)
            assert _eq(got, _oracle_rows(X, Y, xi, extrap))
        assert np.isnan(got[:, np.isnan(xi)]).all()
    axis.close()


def test_empty_and_refused_calls(mi_ctx):
    """m == 0 or nxi == 0 is MI_OK with nothing written; MI_ERR_INVALID_ARG through the raw binding for each NULL pointer,
    a pointer off by 4 bytes, ldy < m, ldyi < m and an m whose byte count overflows -- nothing launched, nothing written"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, ch = mi_ctx._L, mi_ctx._h
    n, m, nxi = 5, 300, 30
    axis = mi.Axis1.from_nodes(mi_ctx, np.linspace(0.0, 1.0, n))
    y = torch.zeros(m * n + 1, dtype=torch.float64, device="cuda")
    xi = torch.full((nxi + 1,), 0.5, dtype=torch.float64, device="cuda")
    yi = torch.full((m * nxi + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    p = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)  # noqa: E731

    def call(ax=axis._h, yp=p(y), ldy=m, rows=m, xp=p(xi), q=nxi, op=p(yi), ldyi=m):
        return L.mi_interp1_rows_f64_dev(ch, ax, yp, ldy, rows, xp, q, op, ldyi, 0.0)

    def err():
        return (L.mi_last_error(ch) or b"").decode()

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((yi[:m * nxi] == 0.0).all()) and float(yi[m * nxi]) == SENTINEL
    yi.fill_(SENTINEL)
    before = _forms(mi_ctx)
    assert call(rows=0) == 0 and call(q=0) == 0 and call(rows=0, yp=None, op=None) == 0 and call(q=0, xp=None) == 0
    INVALID = 1
    for kw, word in [(dict(yp=None), "NULL"), (dict(xp=None), "NULL"), (dict(op=None), "NULL"), (dict(ax=None), "NULL"),
                     (dict(yp=p(y, 4)), "aligned"), (dict(xp=p(xi, 4)), "aligned"), (dict(op=p(yi, 4)), "aligned"),
                     (dict(ldy=m - 1), "ldy"), (dict(ldyi=m - 1), "ldyi"),
                     (dict(rows=2 ** 62, ldy=2 ** 62, ldyi=2 ** 62), "too large"),
                     (dict(q=2 ** 62), "too large")]:
        assert call(**kw) == INVALID, kw
        assert word in err(), (kw, err())
    assert L.mi_interp1_rows_f64_dev(None, axis._h, p(y), m, m, p(xi), nxi, p(yi), m, 0.0) == INVALID
    assert _forms(mi_ctx) == before, "an empty or refused call launched a kernel"
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()), "an empty or refused call wrote something"
    # 8-B aligned pointers that are not 16-B aligned are fine
    assert call(yp=p(y, 8), xp=p(xi, 8), op=p(yi, 8)) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        axis.interp_rows(torch.zeros((m, n), dtype=torch.float64, device="cuda"), xi[:nxi])          # C-ordered (m, n)
    with pytest.raises(ValueError):
        axis.interp_rows(torch.zeros((n + 1, m), dtype=torch.float64, device="cuda").T, xi[:nxi])    # wrong n
    axis.close()


@pytest.mark.parametrize("m", [5, RB + 2])
def test_hipgraph_capture(mi_ctx, m):
    """the call is two kernels on the context's stream and, once the record workspace has grown, allocates nothing:
    captured once on a side stream, replayed twice with new Y in the same buffer, equal to the oracle each time"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(8)
    n, nxi = 11, 700
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    xi = _mixed_queries(rng, X, nxi)
    yd, qd = _t(rng.standard_normal((n, m))), _t(xi)
    out = torch.full((nxi, m), SENTINEL, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mi_ctx.use_torch_stream()
        axis.interp_rows(yd.T, qd, out=out.T)                             # warm call: grows the workspace
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mi_ctx.use_torch_stream()
            axis.interp_rows(yd.T, qd, out=out.T)
    torch.cuda.current_stream().wait_stream(side)
    mi_ctx.use_torch_stream()
    for rep in range(2):
        Y = rng.standard_normal((m, n))
        yd.copy_(_t(Y.T))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert _eq(out.cpu().numpy().T, _oracle_rows(X, Y, xi))
    axis.close()


@pytest.mark.parametrize("padded", [False, True])
def test_interp_stack(mi_ctx, padded):
    """a cube of S = 4 fields of 5 x 7 onto 9 times, dense and with a padded slice stride: element for element the oracle
    along the slice index, and interp_rows on the cube seen as a (ny*nx, S) matrix"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(3)
    ny, nx, S, nti = 5, 7, 4, 9
    X = _jittered(rng, S)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Z = rng.standard_normal((ny, nx, S))
    ti = np.array([X[0], X[-1], X[1], 0.5 * (X[1] + X[2]), np.nan, X[0] - 1.0, X[-1] + 1.0, 0.25 * X[0] + 0.75 * X[1], X[2]])
    stride = ny * nx + (5 if padded else 0)
    buf = torch.full((S, stride), np.nan, dtype=torch.float64, device="cuda")
    buf[:, :ny * nx] = _t(Z.transpose(2, 1, 0).reshape(S, nx * ny))
    cube = buf[:, :ny * nx].view(S, nx, ny).permute(2, 1, 0) if not padded else \
        torch.as_strided(buf, (ny, nx, S), (1, ny, stride))
    assert tuple(cube.shape) == (ny, nx, S) and _eq(cube.cpu().numpy(), Z)
    got = axis.interp_stack(cube, _t(ti), extrap=-3.0)
    assert tuple(got.shape) == (ny, nx, nti)
    g = got.cpu().numpy()
    for i in range(ny):
        for j in range(nx):
            assert _eq(g[i, j], oracle.interp1_bracket(X, Z[i, j], ti, -3.0)), (i, j)
    rows = axis.interp_rows(buf[:, :ny * nx].T, _t(ti), extrap=-3.0).cpu().numpy()         # (ny*nx, nti), row i + j*ny
    assert _eq(g.transpose(2, 1, 0).reshape(nti, nx * ny).T, rows)
    # into a caller's cube with a padded slice stride
    obuf = torch.full((nti, ny * nx + 3), SENTINEL, dtype=torch.float64, device="cuda")
    out = torch.as_strided(obuf, (ny, nx, nti), (1, ny, ny * nx + 3))
    axis.interp_stack(cube, _t(ti), out=out, extrap=-3.0)
    ho = obuf.cpu().numpy()
    assert _eq(ho[:, :ny * nx].reshape(nti, nx, ny).transpose(2, 1, 0), g) and np.all(ho[:, ny * nx:] == SENTINEL)
    with pytest.raises(ValueError, match="ldz"):
        axis.interp_stack(torch.zeros((S, nx, ny + 1), dtype=torch.float64, device="cuda").permute(2, 1, 0)[:ny], _t(ti))
    with pytest.raises(ValueError):
        axis.interp_stack(torch.zeros((S + 1, nx, ny), dtype=torch.float64, device="cuda").permute(2, 1, 0), _t(ti))
    axis.close()
