"""arma::interp1's "nearest" method along matrix rows and over paired columns (mi_interp1_rows_nearest_f64_dev,
mi_interp1_pairs_nearest_f64_dev, mi_debug_nearest_batched_launches; Axis1.interp_rows_nearest,
Axis1.interp_stack_nearest, interp_pairs_nearest).  The reference of every value is nearest_cases.nearest_rule, applied
per row or per column to EVERY output element and compared with nearest_cases._eq_bits: the same 64 bits, no tolerance,
no sampling.  Where a test says so the result also equals Axis1.interp_cols_nearest on the transposed or shared data.

Inputs come from tests/nearest_batched_cases.py: nodes on a grid of 1/8, so that midpoint queries are exact ties; a test
that claims to exercise the select asserts from its own inputs that it holds at least 8 exact ties and that both the left
and the right node are picked (assert_select).

Rows matrices are (m, n) numpy arrays here and C-contiguous (n, ld) buffers on the device; paired matrices are kept as
C-contiguous (B, ld) buffers: row c of the buffer is column c of the column-major matrix."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nearest_batched_cases as bc
import nearest_cases as nc
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "csrc")
SENTINEL = -12345.678
INVALID = 1


def _constants():
    """kRowBlock, kThinM, kPairRowBlock and kLdsMaxN as csrc/mi_nearest_batched.hip states them"""
    text = open(os.path.join(CSRC, "mi_nearest_batched.hip")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(CSRC, "mi_interp2_eval.hpp")).read()).group(1))
    qiter = int(re.search(r"constexpr int kQIter = (\d+);", open(os.path.join(CSRC, "mi_paired_cols.hpp")).read()).group(1))
    rb = int(re.search(r"^constexpr size_t kRowBlock = (\d+);", text, flags=re.M).group(1))
    thin = re.search(r"^constexpr size_t kThinM = (\w+);", text, flags=re.M).group(1)
    assert re.search(r"^constexpr size_t kPairRowBlock = 2 \* kBlock \* kQIter;", text, flags=re.M)
    lds = int(re.search(r"^constexpr size_t kLdsMaxN = (\d+);", text, flags=re.M).group(1))
    return rb, (block if thin == "kBlock" else int(thin)), 2 * block * qiter, lds


RB, T, PRB, LDS_MAX_N = _constants()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _forms(ctx):
    return [int(ctx._L.mi_debug_nearest_batched_launches(f)) for f in range(5)]


def _moved(before, after, form):
    assert [a - b for a, b in zip(after, before)] == [int(f == form) for f in range(5)], (before, after, form)


# ---- rows -------------------------------------------------------------------------------------------------------------

def _run(ctx, axis, Y, xi, extrap=np.nan, ldy_pad=0, ldyi_pad=0, misalign=False, form=None):
    """the device call on column-major views with padded leading dimensions: NaN in the padding rows of y (must not
    leak), a sentinel in the padding rows of yi and around the buffer (must survive); misalign: y and yi 8-B but not
    16-B aligned.  form: the one counter of the hook that must move, by one.  Returns (m, nxi)."""
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
    got = axis.interp_rows_nearest(yb[:, :m].T, _t(xi), out=ob[:, :m].T, extrap=extrap)
    assert tuple(got.shape) == (m, nxi)
    h = flat.cpu().numpy()
    if form is not None:
        _moved(before, _forms(ctx), form)
    body = h[off:off + nxi * ldyi].reshape(nxi, ldyi)
    assert np.all(body[:, m:] == SENTINEL), "padding rows of YI were written"
    assert np.all(h[:off] == SENTINEL) and np.all(h[off + nxi * ldyi:] == SENTINEL), "wrote outside YI"
    return body[:, :m].T.copy()


def _cols(axis, Y, xi, extrap=np.nan):
    """(m, nxi) through Axis1.interp_cols_nearest on the transposed matrix"""
    return axis.interp_cols_nearest(_t(Y).T, _t(xi), extrap=extrap).T.cpu().numpy()


@pytest.mark.parametrize("m", [1, 2, 3, T - 1, T, T + 1, RB - 1, RB, RB + 1, 2 * RB + 3])
def test_rows_row_counts_and_forms(mi_ctx, m):
    """row counts around the flat / tile threshold and around a row block, each dense, with padded ldy, with padded ldyi
    and misaligned: the flat body below kThinM; the tile body with 16-B accesses when y and yi are 16-B aligned and both
    leading dimensions even, with 8-B accesses otherwise -- the hook moves by one in exactly that form"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(1000 + m)
    n, nxi = 7, 37
    X = bc.nodes(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Y = rng.standard_normal((m, n))
    xi = bc.queries(rng, X, nxi)
    bc.assert_select(X, xi)
    want = bc.ref_rows(X, Y, xi, -7.25)
    for ldy_pad, ldyi_pad, misalign in [(0, 0, False), (1, 0, False), (0, 1, False), (3, 5, True)]:
        even = (m + ldy_pad) % 2 == 0 and (m + ldyi_pad) % 2 == 0
        form = 2 if m < T else (0 if even and not misalign else 1)
        got = _run(mi_ctx, axis, Y, xi, -7.25, ldy_pad, ldyi_pad, misalign, form=form)
        assert nc._eq_bits(got, want), (m, ldy_pad, ldyi_pad, misalign)
    axis.close()


@pytest.mark.parametrize("which", range(10))
def test_rows_held_column_sequences(mi_ctx, which):
    """hand-written query sequences through every branch of the tile body's one-column cache: nothing to load, a new
    column, flagged records in between and at both ends, a run without any column -- through the 8-B form, the 16-B
    form and the flat form"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(77)
    n, m = 6, RB + 1
    X = bc.nodes(rng, n)
    name, seq = list(bc.sequences(X).items())[which]
    Y = rng.standard_normal((m, n))
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    for xi in ([np.array(seq)] if seq is not None else [np.array([0.5 * X[3] + 0.5 * X[4]]), np.array([X[0] - 1.0])]):
        want = bc.ref_rows(X, Y, xi, 3.5)
        assert nc._eq_bits(_run(mi_ctx, axis, Y, xi, 3.5, form=1), want), name                     # m odd: 8-B accesses
        # (a single output column has no leading dimension of its own: the wrapper passes ldyi = m, which is odd here)
        assert nc._eq_bits(_run(mi_ctx, axis, Y, xi, 3.5, ldy_pad=1, ldyi_pad=3, form=0 if xi.size > 1 else 1), want), name
        assert nc._eq_bits(_run(mi_ctx, axis, Y[:5], xi, 3.5, form=2), want[:5]), name             # and the flat body
    if which in (0, 3):
        k = nc.rule_index(X, np.array(seq))
        assert (which == 3 and np.array_equal(k, np.arange(n - 1))) or (which == 0 and len(set(k)) < k.size)
    axis.close()


@pytest.mark.parametrize("n,nxi,m,order", [(50, 20_000, RB + 1, "sorted"), (50, 20_000, RB + 1, "permuted"), (50, 20_000, 5, "sorted")])
def test_rows_run_boundaries(mi_ctx, n, nxi, m, order):
    """more output columns than one workgroup takes: the columns are cut into runs, and every run starts without a held
    column; against the rule and against interp_cols_nearest on the transpose"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(n + nxi + m)
    X = bc.nodes(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Y = rng.standard_normal((m, n))
    xi = np.sort(bc.queries(rng, X, nxi))                 # NaN last
    if order == "permuted":
        xi = rng.permutation(xi)
    bc.assert_select(X, xi)
    got = _run(mi_ctx, axis, Y, xi, form=2 if m < T else 1)
    assert nc._eq_bits(got, bc.ref_rows(X, Y, xi))
    assert nc._eq_bits(got, _cols(axis, Y, xi))
    axis.close()


@pytest.mark.parametrize("kind", ["two nodes", "uniform", "linspace", "clustered", "device"])
def test_rows_axis_kinds(mi_ctx, kind):
    """n = 2; a uniform handle with dx a power of two (fma(i, dx, x0) is then x0 + i*dx exactly); a linspace-like explicit
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
        X = np.concatenate([np.arange(40) * 2.0 ** -15, 1.0 + np.arange(5) / 4.0, 100.0 + np.arange(30) * 2.0 ** -20])
        axis = mi.Axis1.from_nodes(mi_ctx, X)
    else:
        X = bc.nodes(rng, 19)
        axis = mi.Axis1.from_device_nodes(mi_ctx, _t(X))
    for m in (T + 3, 3):
        Y = rng.standard_normal((m, X.size))
        xi = bc.queries(rng, X, 301)
        if kind != "linspace":                            # (its midpoints need not be exact)
            bc.assert_select(X, xi)
        got = _run(mi_ctx, axis, Y, xi, 0.5)
        assert nc._eq_bits(got, bc.ref_rows(X, Y, xi, 0.5)), (kind, m)
        assert nc._eq_bits(got, _cols(axis, Y, xi, 0.5)), (kind, m)
    axis.close()


@pytest.mark.parametrize("m", [T + 3, 3])
def test_rows_non_finite_values_come_back_as_stored(mi_ctx, m):
    """inf, -inf, NaN and -0.0 at the first, an interior and the last node of a few rows come back with the stored bits,
    for the queries nearest to their node only and never in another row; a NaN node makes NaN exactly its own half-cells"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(m)
    n = 10
    X = np.arange(float(n))
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    clean = 1.0 + rng.random((m, n))
    Y = clean.copy()
    k = 4
    rows = [0, m - 1] if m == 3 else [1, 2, m - 1, T, 64]
    specials = [np.inf, -np.inf, np.nan, -0.0]
    for j, r in enumerate(rows):
        Y[r, 0] = specials[j % 4]
        Y[r, k] = specials[(j + 1) % 4]
        Y[r, n - 1] = specials[(j + 2) % 4]
    nan_row = rows[1]                                     # Y[nan_row, k] is NaN
    assert np.isnan(Y[nan_row, k])
    xi = np.concatenate([np.arange(0.0, 9.0 + 1e-9, 0.125), np.nextafter([3.5, 4.5], -np.inf), np.nextafter([3.5, 4.5], np.inf),
                         [np.nan, -1.0, 10.0]])
    bc.assert_select(X, xi)
    got = _run(mi_ctx, axis, Y, xi, 1.25)
    assert nc._eq_bits(got, bc.ref_rows(X, Y, xi, 1.25))
    kk = nc.rule_index(X, xi)
    for r in rows:                                        # a stored special is seen by the queries of its node, by no other
        for node in (0, k, n - 1):
            v = got[r][kk == node]
            assert v.size and nc._eq_bits(v, np.full(v.size, Y[r, node]))
        rest = got[r][(kk >= 0) & ~np.isin(kk, (0, k, n - 1))]
        assert np.all(np.isfinite(rest)) and not np.any(np.signbit(rest))
    own = (xi > 3.5) & (xi <= 4.5)
    assert np.array_equal(np.isnan(got[nan_row]) & (kk >= 0), own)                 # exactly its own half-cells
    base = _run(mi_ctx, axis, clean, xi, 1.25)
    others = [r for r in range(m) if r not in rows]
    assert nc._eq_bits(got[others], base[others])
    axis.close()


@pytest.mark.parametrize("extrap", [2.5, -0.0, np.inf, np.nan])
def test_rows_extrapolation_values(mi_ctx, extrap):
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(5)
    X = bc.nodes(rng, 12)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    xi = bc.queries(rng, X, 90)
    oor = (xi < X[0]) | (xi > X[-1])
    assert oor.sum() >= 4 and np.isnan(xi).any()
    for m in (T + 1, 4):
        Y = rng.standard_normal((m, X.size))
        got = _run(mi_ctx, axis, Y, xi, extrap)
        assert nc._eq_bits(got[:, oor], np.full((m, oor.sum()), extrap))
        assert nc._eq_bits(got, bc.ref_rows(X, Y, xi, extrap))
        assert np.isnan(got[:, np.isnan(xi)]).all()
    axis.close()


def test_rows_empty_and_refused_calls(mi_ctx):
    """m == 0 or nxi == 0 is MI_OK with nothing written; MI_ERR_INVALID_ARG through the raw binding for each NULL pointer,
    a pointer off by 4 bytes, ldy < m, ldyi < m and sizes whose byte count overflows -- every text names this function,
    nothing launched, nothing written"""
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
        return L.mi_interp1_rows_nearest_f64_dev(ch, ax, yp, ldy, rows, xp, q, op, ldyi, 0.0)

    def err():
        return (L.mi_last_error(ch) or b"").decode()

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((yi[:m * nxi] == 0.0).all()) and float(yi[m * nxi]) == SENTINEL
    yi.fill_(SENTINEL)
    before = _forms(mi_ctx)
    assert call(rows=0) == 0 and call(q=0) == 0 and call(rows=0, yp=None, op=None) == 0 and call(q=0, xp=None) == 0
    for kw, word in [(dict(yp=None), "NULL"), (dict(xp=None), "NULL"), (dict(op=None), "NULL"), (dict(ax=None), "NULL"),
                     (dict(yp=p(y, 4)), "aligned"), (dict(xp=p(xi, 4)), "aligned"), (dict(op=p(yi, 4)), "aligned"),
                     (dict(ldy=m - 1), "ldy"), (dict(ldyi=m - 1), "ldyi"),
                     (dict(rows=2 ** 62, ldy=2 ** 62, ldyi=2 ** 62), "too large"),
                     (dict(q=2 ** 62), "too large")]:
        assert call(**kw) == INVALID, kw
        assert word in err() and err().startswith("mi_interp1_rows_nearest_f64_dev:"), (kw, err())
    assert L.mi_interp1_rows_nearest_f64_dev(None, axis._h, p(y), m, m, p(xi), nxi, p(yi), m, 0.0) == INVALID
    assert _forms(mi_ctx) == before, "an empty or refused call launched a kernel"
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()), "an empty or refused call wrote something"
    assert call(yp=p(y, 8), xp=p(xi, 8), op=p(yi, 8)) == 0          # 8-B aligned pointers that are not 16-B aligned are fine
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        axis.interp_rows_nearest(torch.zeros((m, n), dtype=torch.float64, device="cuda"), xi[:nxi])          # C-ordered (m, n)
    axis.close()


def test_rows_slot_3_back_to_back_with_the_other_record_users(mi_ctx):
    """interp_rows (16-B records), interp_rows_nearest (4-B), interp_cols_nearest (4-B) and interp_rows again, queued on
    one context without a synchronisation in between and with different query counts: each result is correct"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(31)
    n, m = 9, T + 40
    X = bc.nodes(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Y = rng.standard_normal((m, n))
    qs = [bc.queries(rng, X, k) for k in (500, 3000, 1200, 800)]
    bc.assert_select(X, qs[1])
    yd = _t(Y.T)                                           # (n, m): rows layout; its .T view is (m, n) column-major
    a = axis.interp_rows(yd.T, _t(qs[0]), extrap=2.0)
    b = axis.interp_rows_nearest(yd.T, _t(qs[1]), extrap=2.0)
    c = axis.interp_cols_nearest(_t(Y).T, _t(qs[2]), extrap=2.0)
    d = axis.interp_rows(yd.T, _t(qs[3]), extrap=2.0)
    torch.cuda.synchronize()
    lin = lambda q: np.stack([oracle.interp1_bracket(X, Y[r], q, 2.0) for r in range(m)])  # noqa: E731
    assert np.array_equal(a.cpu().numpy(), lin(qs[0]), equal_nan=True)
    assert nc._eq_bits(b.cpu().numpy(), bc.ref_rows(X, Y, qs[1], 2.0))
    assert nc._eq_bits(c.T.cpu().numpy(), bc.ref_rows(X, Y, qs[2], 2.0))
    assert np.array_equal(d.cpu().numpy(), lin(qs[3]), equal_nan=True)
    axis.close()


@pytest.mark.parametrize("m", [5, RB + 2])
def test_rows_hipgraph_capture(mi_ctx, m):
    """the call is two kernels on the context's stream and, once the record workspace has grown, allocates nothing:
    captured once on a side stream after a warm-up call, replayed twice with new Y in the same buffer"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(8)
    n, nxi = 11, 700
    X = bc.nodes(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    xi = bc.queries(rng, X, nxi)
    bc.assert_select(X, xi)
    yd, qd = _t(rng.standard_normal((n, m))), _t(xi)
    out = torch.full((nxi, m), SENTINEL, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mi_ctx.use_torch_stream()
        axis.interp_rows_nearest(yd.T, qd, out=out.T)                     # warm call: grows the workspace
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mi_ctx.use_torch_stream()
            axis.interp_rows_nearest(yd.T, qd, out=out.T)
    torch.cuda.current_stream().wait_stream(side)
    mi_ctx.use_torch_stream()
    for rep in range(2):
        Y = rng.standard_normal((m, n))
        yd.copy_(_t(Y.T))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert nc._eq_bits(out.cpu().numpy().T, bc.ref_rows(X, Y, xi))
    axis.close()


@pytest.mark.parametrize("padded", [False, True])
def test_interp_stack_nearest(mi_ctx, padded):
    """a cube of S = 6 fields of 9 x 5 onto 40 times, dense and with a padded slice stride: element for element the rule
    along the slice index, and interp_rows_nearest on the cube seen as a (ny*nx, S) matrix"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(3)
    ny, nx, S, nti = 9, 5, 6, 40
    X = bc.nodes(rng, S)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Z = rng.standard_normal((ny, nx, S))
    ti = bc.queries(rng, X, nti)
    bc.assert_select(X, ti)
    stride = ny * nx + (5 if padded else 0)
    buf = torch.full((S, stride), np.nan, dtype=torch.float64, device="cuda")
    buf[:, :ny * nx] = _t(Z.transpose(2, 1, 0).reshape(S, nx * ny))
    cube = torch.as_strided(buf, (ny, nx, S), (1, ny, stride))
    assert nc._eq_bits(cube.cpu().numpy(), Z)
    got = axis.interp_stack_nearest(cube, _t(ti), extrap=-3.0)
    assert tuple(got.shape) == (ny, nx, nti)
    g = got.cpu().numpy()
    for i in range(ny):
        for j in range(nx):
            assert nc._eq_bits(g[i, j], nc.nearest_rule(X, Z[i, j], ti, -3.0)), (i, j)
    rows = axis.interp_rows_nearest(buf[:, :ny * nx].T, _t(ti), extrap=-3.0).cpu().numpy()     # (ny*nx, nti), row i + j*ny
    assert nc._eq_bits(g.transpose(2, 1, 0).reshape(nti, nx * ny).T, rows)
    obuf = torch.full((nti, ny * nx + 3), SENTINEL, dtype=torch.float64, device="cuda")          # a caller's padded cube
    out = torch.as_strided(obuf, (ny, nx, nti), (1, ny, ny * nx + 3))
    axis.interp_stack_nearest(cube, _t(ti), out=out, extrap=-3.0)
    ho = obuf.cpu().numpy()
    assert nc._eq_bits(ho[:, :ny * nx].reshape(nti, nx, ny).transpose(2, 1, 0), g) and np.all(ho[:, ny * nx:] == SENTINEL)
    with pytest.raises(ValueError, match="ldz"):
        axis.interp_stack_nearest(torch.zeros((S, nx, ny + 1), dtype=torch.float64, device="cuda").permute(2, 1, 0)[:ny], _t(ti))
    axis.close()


# ---- pairs ------------------------------------------------------------------------------------------------------------

def _prun(ctx, Xb, Yb, xi, extrap=np.nan, lens=None, ldx_pad=0, ldy_pad=0, ldyi_pad=0, misalign=False, want_ok=True,
          x_misalign=False, form="auto"):
    """the device call on column-major views with padded leading dimensions: NaN below each column of X and of Y (must
    not leak), a sentinel below each column of YI (must survive); misalign: yi 8-B but not 16-B aligned; x_misalign: the
    first column of X starts 8 B off a 16-B boundary.  The hook must move by one, in the form n asks for.
    Returns ((B, nxi) outputs, (B,) col_ok or None)."""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    B, n = Xb.shape
    nxi = xi.size
    bx = np.full(B * (n + ldx_pad) + 2, np.nan)
    xd_flat = _t(bx)
    xoff = 0 if (xd_flat.data_ptr() % 16 == 0) != x_misalign else 1
    xv = xd_flat[xoff:xoff + B * (n + ldx_pad)].view(B, n + ldx_pad)
    xv[:, :n] = _t(Xb)
    by = np.full((B, n + ldy_pad), np.nan)
    by[:, :n] = Yb
    yd = _t(by)
    ldyi = nxi + ldyi_pad
    flat = torch.full((B * ldyi + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    off = 0 if (flat.data_ptr() % 16 == 0) != misalign else 1
    ob = flat[off:off + B * ldyi].view(B, ldyi)
    assert (ob.data_ptr() % 16 != 0) == misalign
    ld = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.int64).astype(np.int32)).cuda()
    before = _forms(ctx)
    res = mi.interp_pairs_nearest(ctx, xv[:, :n].T, yd[:, :n].T, _t(xi), lens=ld, out=ob[:, :nxi].T, extrap=extrap, want_ok=want_ok)
    got, ok = res if want_ok else (res, None)
    assert tuple(got.shape) == (nxi, B)
    h = flat.cpu().numpy()
    _moved(before, _forms(ctx), (3 if n <= LDS_MAX_N else 4) if form == "auto" else form)
    body = h[off:off + B * ldyi].reshape(B, ldyi)
    assert np.all(body[:, nxi:] == SENTINEL), "padding rows of YI were written"
    assert np.all(h[:off] == SENTINEL) and np.all(h[off + B * ldyi:] == SENTINEL), "wrote outside YI"
    return body[:, :nxi].copy(), (None if ok is None else ok.cpu().numpy().astype(np.int64))


def _pcheck(ctx, Xb, Yb, xi, extrap=np.nan, lens=None, **kw):
    got, ok = _prun(ctx, Xb, Yb, xi, extrap, lens, **kw)
    want, wok = bc.ref_pairs(Xb, Yb, xi, extrap, lens)
    differ = [c for c in range(Xb.shape[0]) if not nc._eq_bits(got[c], want[c])]
    assert not differ, "%d columns differ from the rule, first %s" % (len(differ), differ[:5])
    if ok is not None:
        assert np.array_equal(ok, wok), "col_ok differs at %s" % np.nonzero(ok != wok)[0][:5]
    return got


@pytest.mark.parametrize("n", [2, 3, 1024, LDS_MAX_N - 1, LDS_MAX_N, LDS_MAX_N + 1, 50_001])
def test_pairs_column_lengths_and_forms(mi_ctx, n):
    """column lengths across the LDS-form limit, even and odd, so both load alignments run; the Restrict shape n = 2
    goes through the LDS form; the hook says 3 or 4 accordingly (checked in _prun)"""
    rng = np.random.default_rng(100 + n)
    for B, nxi, pads in [(5, 1500, (0, 0)), (4, 3001, (1, 2))]:
        Xb, Yb = bc.pairs(rng, B, n)
        xi = bc.pair_queries(rng, Xb, nxi)
        bc.assert_select(bc.valid_tables(Xb), xi)
        _pcheck(mi_ctx, Xb, Yb, xi, ldx_pad=pads[0], ldy_pad=pads[1])
        _pcheck(mi_ctx, Xb, Yb, xi, ldx_pad=pads[1], ldy_pad=pads[0], x_misalign=True)


@pytest.mark.parametrize("B", [1, 2, 3, 37])
@pytest.mark.parametrize("n", [257, 5000])
def test_pairs_column_counts(mi_ctx, B, n):
    rng = np.random.default_rng(B * 31 + n)
    Xb, Yb = bc.pairs(rng, B, n)
    xi = bc.pair_queries(rng, Xb, 700)
    bc.assert_select(bc.valid_tables(Xb), xi)
    _pcheck(mi_ctx, Xb, Yb, xi, extrap=-1.5)
    if B >= 37:   # several row blocks too: the run of columns per workgroup changes with nxi
        _pcheck(mi_ctx, Xb, Yb, bc.pair_queries(rng, Xb, 2 * PRB + 10), ldyi_pad=2)


@pytest.mark.parametrize("nxi", [1, 2, 7, 255, 256, 257, 2047, 2049, 5000])
def test_pairs_query_counts_and_store_widths(mi_ctx, nxi):
    """nxi of 1, odd, either side of 256 and of a row block; ldyi > nxi odd and even and a yi that is 8-B but not 16-B
    aligned, so that both store widths run; padding rows checked by _prun"""
    rng = np.random.default_rng(nxi)
    for n in (600, 5000):
        Xb, Yb = bc.pairs(rng, 7, n)
        xi = bc.pair_queries(rng, Xb, nxi)
        if nxi >= 255:
            bc.assert_select(bc.valid_tables(Xb), xi)
        for ldx_pad, ldy_pad, ldyi_pad, misalign in [(0, 0, 0, False), (1, 3, 1, False), (2, 5, 2, False), (3, 1, 0, True),
                                                     (0, 2, 3, True), (4, 1, nxi % 2, False)]:
            _pcheck(mi_ctx, Xb, Yb, xi, extrap=9.0, ldx_pad=ldx_pad, ldy_pad=ldy_pad, ldyi_pad=ldyi_pad, misalign=misalign)


def test_pairs_more_units_than_workgroups(mi_ctx):
    """3 row blocks x 1366 runs = 4098 units against 16 workgroups per compute unit on a 256-CU device"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(64)
    n, B, nxi = 64, 2 * 1366, 2 * PRB + 10
    assert (B, nxi) == (2732, 4106)
    Xb, Yb = bc.pairs(rng, B, n)
    xi = bc.pair_queries(rng, Xb, nxi)
    bc.assert_select(bc.valid_tables(Xb), xi)
    got = mi.interp_pairs_nearest(mi_ctx, _t(Xb).T, _t(Yb).T, _t(xi)).T.cpu().numpy()
    want, wok = bc.ref_pairs(Xb, Yb, xi)
    assert wok.all() and nc._eq_bits(got, want)


@pytest.mark.parametrize("n", [700, LDS_MAX_N + 100])
def test_pairs_sorted_and_permuted_queries_give_the_same_bits(mi_ctx, n):
    """sorted queries stage X plain, permuted ones skewed (LDS form): the same data, the same bits, query by query"""
    rng = np.random.default_rng(n + 7)
    B, nxi = 9, 2 * PRB + 300
    Xb, Yb = bc.pairs(rng, B, n)
    xs = np.sort(bc.pair_queries(rng, Xb, nxi))            # NaN last
    perm = rng.permutation(nxi)
    bc.assert_select(bc.valid_tables(Xb), xs)
    a = _pcheck(mi_ctx, Xb, Yb, xs, extrap=0.75)
    b = _pcheck(mi_ctx, Xb, Yb, xs[perm], extrap=0.75)
    assert nc._eq_bits(a[:, perm], b)


@pytest.mark.parametrize("n", [1500, LDS_MAX_N + 500])
def test_pairs_ragged_columns(mi_ctx, n):
    """len of 2, 3, n and random values between; the rows behind n_c hold NaN (X and Y): they reach no result and make no
    column bad; len = NULL equals len = n"""
    rng = np.random.default_rng(n + 1)
    B = 41
    Xb, Yb = bc.pairs(rng, B, n)
    lens = rng.integers(2, n + 1, B)
    lens[:6] = [2, 3, n, n - 1, 2, n]
    xi = bc.pair_queries(rng, Xb, 3000, lens)
    bc.assert_select(bc.valid_tables(Xb, lens), xi)
    Xf, Yf = Xb.copy(), Yb.copy()
    for c in range(B):
        Xf[c, lens[c]:] = np.nan
        Yf[c, lens[c]:] = np.nan
    got = _pcheck(mi_ctx, Xf, Yf, xi, 7.0, lens, ldx_pad=1)
    want, wok = bc.ref_pairs(Xb, Yb, xi, 7.0, lens)
    assert wok.all() and nc._eq_bits(got, want)
    full = np.full(B, n)
    assert nc._eq_bits(_pcheck(mi_ctx, Xb, Yb, xi, 7.0, full), _pcheck(mi_ctx, Xb, Yb, xi, 7.0, None))


def _defects(Xb, lens):
    """one defect per odd column (a good column between two bad ones): equal nodes, the pair -0.0 / 0.0, an inf node, a
    NaN node, and a descending pair at both 16-B vector seams and both sides of a wave seam.  Returns the bad columns."""
    n = Xb.shape[1]
    plan = [("equal", 5), ("equal", "last"), ("zeros", 7), ("inf", "last"), ("nan", 11), ("nan", 0),
            ("down", 1), ("down", 2), ("down", 126), ("down", 127), ("down", 128), ("down", 511), ("down", 512)]
    bad = []
    for j, (kind, k) in enumerate(plan):
        c = 2 * j + 1
        nc_ = bc.col_len(lens, c, n)
        kk = nc_ - 2 if k == "last" else k
        assert 0 <= kk <= nc_ - 2
        x = Xb[c]
        if kind == "equal":
            x[kk + 1] = x[kk]
        elif kind == "zeros":
            x[:] = x - x[kk + 1]
            assert x[kk + 1] == 0.0 and x[kk] < 0.0 and x[kk - 1] < 0.0
            x[kk] = -0.0
        elif kind == "inf":
            x[nc_ - 1] = np.inf
        elif kind == "nan":
            x[kk] = np.nan
        else:
            x[kk + 1] = np.nextafter(x[kk], -np.inf)
        bad.append(c)
    assert 2 * len(plan) + 1 <= Xb.shape[0]
    return bad


@pytest.mark.parametrize("n", [1500, LDS_MAX_N + 500])
def test_pairs_bad_columns(mi_ctx, n):
    """every kind of bad column, in both forms, with 16-B aligned and 8-B odd column starts: such a column is all NaN
    with col_ok 0; every other column has col_ok 1 and equals the rule; col_ok = NULL gives the same outputs"""
    rng = np.random.default_rng(n * 2)
    B = 34
    clean, Yb = bc.pairs(rng, B, n)
    for ragged in (False, True):
        Xb = clean.copy()
        lens = rng.integers(1030, n + 1, B) if ragged else None
        bad = _defects(Xb, lens)
        xi = bc.pair_queries(rng, clean, 2100, lens)
        bc.assert_select(bc.valid_tables(Xb, lens), xi)
        if ragged:
            lens[B - 2], lens[B - 4], lens[B - 6] = 0, 1, n + 1
            bad += [B - 2, B - 4, B - 6]
        for xm, pad in ((False, 0), (True, 1)):
            got, ok = _prun(mi_ctx, Xb, Yb, xi, 3.5, lens, ldx_pad=pad, x_misalign=xm)
            want, wok = bc.ref_pairs(Xb, Yb, xi, 3.5, lens)
            assert sorted(np.nonzero(wok == 0)[0].tolist()) == sorted(bad)
            assert np.array_equal(ok, wok), "col_ok differs at %s" % np.nonzero(ok != wok)[0][:8]
            assert np.isnan(got[bad]).all()
            assert nc._eq_bits(got, want)                  # every neighbouring column untouched
            blind, none = _prun(mi_ctx, Xb, Yb, xi, 3.5, lens, ldx_pad=pad, x_misalign=xm, want_ok=False)
            assert none is None and nc._eq_bits(blind, got)


@pytest.mark.parametrize("n", [700, LDS_MAX_N + 100])
def test_pairs_identical_columns_equal_the_shared_axis_call(mi_ctx, n):
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(n)
    X = bc.nodes(rng, n)
    B = 33
    Xb = np.tile(X, (B, 1))
    Yb = rng.standard_normal((B, n))
    xi = bc.queries(rng, X, 2500)
    bc.assert_select(X, xi)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    shared = axis.interp_cols_nearest(_t(Yb).T, _t(xi), extrap=0.25).T.cpu().numpy()
    assert nc._eq_bits(_pcheck(mi_ctx, Xb, Yb, xi, extrap=0.25), shared)
    axis.close()


@pytest.mark.parametrize("n", [500, LDS_MAX_N + 905])
def test_pairs_non_finite_values_come_back_as_stored(mi_ctx, n):
    """inf, -inf, NaN and -0.0 inside a few columns of Y come back with the stored bits and never reach another column"""
    rng = np.random.default_rng(n)
    B = 12
    Xb, clean = bc.pairs(rng, B, n)
    clean = 1.0 + np.abs(clean)
    Yb = clean.copy()
    cols = [1, 4, 7, 10]
    specials = [np.inf, -np.inf, np.nan, -0.0]
    for j, c in enumerate(cols):
        Yb[c, 0], Yb[c, n // 2], Yb[c, n - 1] = specials[j % 4], specials[(j + 1) % 4], specials[(j + 2) % 4]
    xi = bc.pair_queries(rng, Xb, 1200)
    k = n // 2
    extra = [v for c in cols for v in (Xb[c, k], 0.5 * Xb[c, k] + 0.5 * Xb[c, k + 1], 0.5 * Xb[c, k - 1] + 0.5 * Xb[c, k],
                                       Xb[c, 0], Xb[c, n - 1], 0.5 * Xb[c, n - 2] + 0.5 * Xb[c, n - 1])]
    xi[:len(extra)] = extra
    bc.assert_select(bc.valid_tables(Xb), xi)
    got = _pcheck(mi_ctx, Xb, Yb, xi, 1.25)
    for c in cols:
        kk = nc.rule_index(Xb[c], xi)
        for node in (0, k, n - 1):
            v = got[c][kk == node]
            assert v.size and nc._eq_bits(v, np.full(v.size, Yb[c, node])), (c, node)
    base = _pcheck(mi_ctx, Xb, clean, xi, 1.25)
    others = [c for c in range(B) if c not in cols]
    assert nc._eq_bits(got[others], base[others]) and np.isfinite(base[:, ~np.isnan(xi)]).all()


@pytest.mark.parametrize("extrap", [2.5, -0.0, np.inf, np.nan])
def test_pairs_extrapolation_values(mi_ctx, extrap):
    rng = np.random.default_rng(5)
    for n in (300, LDS_MAX_N + 10):
        Xb, Yb = bc.pairs(rng, 6, n)
        xi = bc.pair_queries(rng, Xb, 400)
        got = _pcheck(mi_ctx, Xb, Yb, xi, extrap)
        for c in range(6):
            oor = (xi < Xb[c, 0]) | (xi > Xb[c, -1])
            assert oor.sum() >= 2 and nc._eq_bits(got[c][oor], np.full(oor.sum(), extrap))
        assert np.isnan(got[:, np.isnan(xi)]).all()


def test_pairs_empty_and_refused_calls(mi_ctx):
    """B == 0 or nxi == 0 is MI_OK with nothing launched or written; MI_ERR_INVALID_ARG for NULL or misaligned pointers,
    ldx < n, ldy < n, ldyi < nxi, n < 2 and overflowing sizes -- each text names this function and the culprit, no hook
    moves, nothing is written"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, ch = mi_ctx._L, mi_ctx._h
    n, B, nxi = 50, 4, 30
    x = torch.arange(B * n + 1, dtype=torch.float64, device="cuda")
    y = torch.zeros(B * n + 1, dtype=torch.float64, device="cuda")
    xi = torch.full((nxi + 1,), 0.5, dtype=torch.float64, device="cuda")
    yi = torch.full((B * nxi + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    ln = torch.full((B + 1,), n, dtype=torch.int32, device="cuda")
    okt = torch.full((B + 1,), 77, dtype=torch.int32, device="cuda")
    p = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)  # noqa: E731

    def call(xp=p(x), ldx=n, yp=p(y), ldy=n, nn=n, lp=p(ln), ncols=B, qp=p(xi), m=nxi, op=p(yi), ldyi=nxi, kp=p(okt)):
        return L.mi_interp1_pairs_nearest_f64_dev(ch, xp, ldx, yp, ldy, nn, lp, ncols, qp, m, op, ldyi, 0.0, kp)

    def err():
        return (L.mi_last_error(ch) or b"").decode()

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((okt[:B] == 1).all()) and int(okt[B]) == 77
    yi.fill_(SENTINEL)
    okt.fill_(77)
    before = _forms(mi_ctx)
    assert call(ncols=0) == 0 and call(m=0) == 0 and call(ncols=0, xp=None, yp=None, op=None) == 0 and call(m=0, qp=None) == 0
    for kw, word in [(dict(ldx=n - 1), "ldx"), (dict(ldy=n - 1), "ldy"), (dict(ldyi=nxi - 1), "ldyi"), (dict(nn=1, ldx=1, ldy=1), "n=1"),
                     (dict(xp=p(x, 4)), "aligned"), (dict(yp=p(y, 4)), "aligned"), (dict(qp=p(xi, 4)), "aligned"),
                     (dict(op=p(yi, 4)), "aligned"), (dict(lp=p(ln, 2)), "aligned"), (dict(kp=p(okt, 2)), "aligned"),
                     (dict(xp=None), "NULL"), (dict(yp=None), "NULL"), (dict(qp=None), "NULL"), (dict(op=None), "NULL"),
                     (dict(ncols=2 ** 62), "too large"), (dict(ldyi=2 ** 61), "too large")]:
        assert call(**kw) == INVALID, kw
        assert word in err() and err().startswith("mi_interp1_pairs_nearest_f64_dev:"), (kw, err())
    assert L.mi_interp1_pairs_nearest_f64_dev(None, p(x), n, p(y), n, n, None, B, p(xi), nxi, p(yi), nxi, 0.0, None) == INVALID
    assert _forms(mi_ctx) == before, "an empty or refused call launched a kernel"
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()) and bool((okt == 77).all()), "an empty or refused call wrote something"
    # 8-B aligned pointers that are not 16-B aligned, 4-B aligned counts and flags are fine; len and col_ok may be NULL
    assert call(xp=p(x, 8), yp=p(y, 8), qp=p(xi, 8), op=p(yi, 8), lp=p(ln, 4), kp=p(okt, 4)) == 0
    assert call(lp=None, kp=None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        mi.interp_pairs_nearest(mi_ctx, torch.zeros((n, B), dtype=torch.float64, device="cuda"),
                                torch.zeros((n, B), dtype=torch.float64, device="cuda"), xi[:nxi])      # row-major (n, B)


def test_pairs_hipgraph_capture_of_the_lds_form(mi_ctx):
    """the LDS-form call is one kernel on the context's stream and allocates nothing: captured once with col_ok given,
    replayed twice with X, Y and xi overwritten in place between the replays"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(8)
    n, B, nxi = 1024, 60, 2500
    Xb, Yb = bc.pairs(rng, B, n)
    xd, yd, xid = _t(Xb), _t(Yb), _t(bc.pair_queries(rng, Xb, nxi))
    out = torch.full((B, nxi), SENTINEL, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mi_ctx.use_torch_stream()
        mi.interp_pairs_nearest(mi_ctx, xd.T, yd.T, xid, out=out.T)       # warm-up outside capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mi_ctx.use_torch_stream()
            _, ok = mi.interp_pairs_nearest(mi_ctx, xd.T, yd.T, xid, out=out.T, want_ok=True)
    torch.cuda.current_stream().wait_stream(side)
    mi_ctx.use_torch_stream()
    for rep in range(2):
        Xn, Yn = bc.pairs(rng, B, n)
        Xn[rep + 5, 700] = Xn[rep + 5, 699]
        xin = bc.pair_queries(rng, Xn, nxi)
        bc.assert_select(bc.valid_tables(Xn), xin)
        xd.copy_(_t(Xn))
        yd.copy_(_t(Yn))
        xid.copy_(_t(xin))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want, wok = bc.ref_pairs(Xn, Yn, xin)
        assert nc._eq_bits(out.cpu().numpy(), want)
        assert np.array_equal(ok.cpu().numpy(), wok) and not wok[rep + 5]


# ---- a seeded sweep -----------------------------------------------------------------------------------------------------

def test_rows_seeded_sweep(mi_ctx):
    """40 seeded cases: sizes up to 20 000 table elements and 20 000 outputs, random leading dimensions and alignments,
    every element compared"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(0x4EA3)
    ties = 0
    for case in range(40):
        n = int(rng.integers(2, 60))
        m = int(rng.choice([rng.integers(1, T), rng.integers(T, 20_000 // n + 1)])) if 20_000 // n > T else int(rng.integers(1, 20_000 // n + 1))
        nxi = int(rng.integers(1, max(2, min(4000, 20_000 // m) + 1)))
        X = bc.nodes(rng, n, origin=float(rng.integers(-40, 40)))
        axis = mi.Axis1.from_nodes(mi_ctx, X)
        Y = rng.standard_normal((m, n))
        xi = bc.queries(rng, X, nxi)
        if rng.random() < 0.5:
            xi = np.sort(xi)
        ties += bc.select_counts(X, xi)[0]
        extrap = float(rng.choice([np.nan, 2.5, -0.0, np.inf]))
        got = _run(mi_ctx, axis, Y, xi, extrap, int(rng.integers(0, 4)), int(rng.integers(0, 4)), bool(rng.integers(0, 2)))
        assert nc._eq_bits(got, bc.ref_rows(X, Y, xi, extrap)), (case, n, m, nxi)
        axis.close()
    assert ties >= 8


def test_pairs_seeded_sweep(mi_ctx):
    """40 seeded cases in both forms: sizes up to 20 000 table elements and 20 000 outputs, ragged or not, random leading
    dimensions and alignments, every element compared"""
    rng = np.random.default_rng(0x4EA4)
    ties = 0
    for case in range(40):
        n = int(rng.choice([rng.integers(2, 40), rng.integers(40, LDS_MAX_N + 1), rng.integers(LDS_MAX_N + 1, 10_000)]))
        B = int(rng.integers(1, max(2, min(64, 20_000 // n) + 1)))
        nxi = int(rng.integers(1, max(2, min(6000, 20_000 // B) + 1)))
        Xb, Yb = bc.pairs(rng, B, n)
        lens = rng.integers(2, n + 1, B) if rng.random() < 0.5 else None
        xi = bc.pair_queries(rng, Xb, nxi, lens)
        if rng.random() < 0.5:
            xi = np.sort(xi)
        ties += sum(bc.select_counts(X, xi)[0] for X in bc.valid_tables(Xb, lens, 4))
        extrap = float(rng.choice([np.nan, 2.5, -0.0, np.inf]))
        _pcheck(mi_ctx, Xb, Yb, xi, extrap, lens, ldx_pad=int(rng.integers(0, 4)), ldy_pad=int(rng.integers(0, 4)),
                ldyi_pad=int(rng.integers(0, 4)), misalign=bool(rng.integers(0, 2)), x_misalign=bool(rng.integers(0, 2)),
                want_ok=bool(rng.integers(0, 2)))
    assert ties >= 8
