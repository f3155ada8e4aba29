"""interp1 over paired columns with a query vector per column (mi_interp1_each_f64_dev / _host,
mi_group_interp1_each_f64_host, mi.interp_each, mi355::interp1_each): YI[:, c] is interp1 of XI[:, c] on the table
(X[0:n_c, c], Y[0:n_c, c]), NaN for a bad column; a 1-D XI (ldxi = 0) is shared by every column.  The references are the
CPU oracle column by column, oracle.interp1_bracket on the first n_c rows and that column's queries; where B <= 64 a
host-built Grid1.from_nodes(X[:n_c, c], Y[:n_c, c], sanitise=False).interp(XI[:, c]) on the device; and for a shared XI
mi.interp_pairs on the same inputs.  Every comparison is np.array_equal(..., equal_nan=True) on every output plus the
sign of zeros: no tolerance, no sampling.  After every device call the launch counters say which form ran.

Matrices are kept as C-contiguous (B, ld) buffers here: row c of the buffer is column c of the column-major matrix."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "host")
_SRC = open(os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "csrc", "mi_each1.hip")).read()
THIN_N = int(re.search(r"constexpr\s+\w+\s+kThinMaxN = (\d+);", _SRC).group(1))     # thin form: n <= THIN_N and nxi <= THIN_Q
THIN_Q = int(re.search(r"constexpr\s+\w+\s+kThinMaxQ = (\d+);", _SRC).group(1))
LDS_MAX_N = int(re.search(r"kLdsMaxN = (\d+);", _SRC).group(1))                       # LDS form up to here, direct beyond
ROW_BLOCK = 2048          # kRowBlock: outputs of one column per unit of work
BLOCK = 256               # columns per workgroup of the thin form
SENTINEL = -12345.678
THIN, LDS, DIRECT, FORWARDED = 0, 1, 2, 3


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _eq(a, b):
    """every element equal (NaN == NaN), and zeros carry the same sign"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & (a == 0), np.signbit(b) & (b == 0))


def _pairs(rng, B, n):
    """(B, n) nodes and values: jittered increments, a scale and an offset per column, so that a query in range in one
    column is out of range in the next"""
    Xb = np.cumsum(rng.uniform(0.2, 1.0, (B, n)), axis=1)
    Xb = Xb * rng.uniform(0.5, 1.5, (B, 1)) + (3.0 * n) * np.arange(B)[:, None] * rng.choice([-1.0, 1.0])
    return Xb, rng.standard_normal((B, n))


def _col_len(lens, c, n):
    return n if lens is None else int(lens[c])


def _queries(rng, Xb, nxi, lens=None, order="permuted"):
    """(B, nxi) queries, each column's drawn around that column's own range (the ranges of two columns are disjoint, so
    reading another column's queries gives extrap or a wrong value).  Every column gets its own end nodes, interior
    nodes, the points just outside, NaN and +-inf; with fewer rows than specials the specials rotate over the columns."""
    B, n = Xb.shape
    Q = np.empty((B, nxi))
    for c in range(B):
        nc = min(max(_col_len(lens, c, n), 2), n)
        x = Xb[c, :nc]
        lo, hi = x[0], x[-1]
        q = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), nxi)
        special = [lo, hi, x[nc // 2], x[(nc - 1) // 3], np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), np.nan, np.inf,
                   -np.inf, np.nextafter(hi, -np.inf), np.nextafter(lo, np.inf), 0.5 * (x[0] + x[1])]
        if nxi >= 2 * len(special):
            q[rng.choice(nxi, len(special), replace=False)] = special
        else:
            for i in range(nxi):
                k = (c * nxi + i) % (len(special) + 3)
                if k < len(special):
                    q[i] = special[k]
        if order == "sorted":
            q = np.sort(q)                                   # (NaN last)
        Q[c] = q
    return Q


def _is_bad(x):
    """mi_axis1_create's rule on the valid rows of a column"""
    return x.size < 2 or not np.all(np.isfinite(x)) or not np.all(x[:-1] < x[1:])


def _oracle_each(Xb, Yb, XI, extrap=np.nan, lens=None):
    """(B, nxi) expected outputs and the (B,) expected col_ok; XI (B, nxi), or 1-D: shared"""
    B, n = Xb.shape
    nxi = XI.shape[-1]
    want = np.full((B, nxi), np.nan)
    ok = np.zeros(B, dtype=np.int64)
    for c in range(B):
        nc = _col_len(lens, c, n)
        if nc < 2 or nc > n or _is_bad(Xb[c, :nc]):
            continue
        ok[c] = 1
        want[c] = oracle.interp1_bracket(Xb[c, :nc], Yb[c, :nc], np.ascontiguousarray(XI if XI.ndim == 1 else XI[c]), extrap)
    return want, ok


def _grid1_each(ctx, Xb, Yb, XI, extrap, lens, ok):
    """the good columns through a host-built 1-D table per column on the device"""
    import armadillocudalinearinterpolation_amd as mi
    rows = np.full((Xb.shape[0], XI.shape[-1]), np.nan)
    for c in range(Xb.shape[0]):
        if ok[c]:
            nc = _col_len(lens, c, Xb.shape[1])
            g = mi.Grid1.from_nodes(ctx, Xb[c, :nc], Yb[c, :nc], sanitise=False)
            rows[c] = g.interp(_t(XI if XI.ndim == 1 else XI[c]), extrap=extrap).cpu().numpy()
            g.close()
    return rows


def _counts(ctx):
    return [int(ctx._L.mi_debug_each_launches(f)) for f in range(4)]


def _form(n, nxi, shared):
    if n <= THIN_N and nxi <= THIN_Q:
        return THIN
    if shared:
        return FORWARDED
    return LDS if n <= LDS_MAX_N else DIRECT


def _padded(rows, width, pad, fill, misalign):
    """a (rows, width) view with leading dimension width + pad inside a flat device buffer filled with `fill`; misalign:
    the first element sits 8 B off a 16-B boundary.  Returns (flat, offset, view)."""
    import torch
    ld = width + pad
    flat = torch.full((rows * ld + 2,), fill, dtype=torch.float64, device="cuda")
    off = 0 if (flat.data_ptr() % 16 == 0) != misalign else 1
    view = flat[off:off + rows * ld].view(rows, ld)
    assert (view.data_ptr() % 16 != 0) == misalign
    return flat, off, view


def _run(ctx, Xb, Yb, XI, extrap=np.nan, lens=None, ldx_pad=0, ldy_pad=0, ldxi_pad=0, ldyi_pad=0, misalign=False, want_ok=True):
    """the device call on column-major views with padded leading dimensions: NaN below each column of X, Y and XI (must
    not leak), a sentinel below each column of YI (must survive); misalign: x, y, xi and yi each 8-B but not 16-B
    aligned.  XI (B, nxi) or 1-D (shared, ldxi = 0).  Checks that exactly the expected form was launched.
    Returns ((B, nxi) outputs, (B,) col_ok or None)."""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    B, n = Xb.shape
    shared = XI.ndim == 1
    nxi = XI.shape[-1]
    _, _, xv = _padded(B, n, ldx_pad, np.nan, misalign)
    xv[:, :n] = _t(Xb)
    _, _, yv = _padded(B, n, ldy_pad, np.nan, misalign)
    yv[:, :n] = _t(Yb)
    if shared:
        _, _, qv = _padded(1, nxi, 0, np.nan, misalign)
        qv[0, :] = _t(XI)
        qarg = qv[0]
    else:
        _, _, qv = _padded(B, nxi, ldxi_pad, np.nan, misalign)
        qv[:, :nxi] = _t(XI)
        qarg = qv[:, :nxi].T
    ldyi = nxi + ldyi_pad
    flat, off, ob = _padded(B, nxi, ldyi_pad, SENTINEL, misalign)
    ld = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.int64).astype(np.int32)).cuda()
    before = _counts(ctx)
    res = mi.interp_each(ctx, xv[:, :n].T, yv[:, :n].T, qarg, lens=ld, out=ob[:, :nxi].T, extrap=extrap, want_ok=want_ok)
    delta = [a - b for a, b in zip(_counts(ctx), before)]
    want_delta = [0, 0, 0, 0]
    want_delta[_form(n, nxi, shared)] = 1
    assert delta == want_delta, "n=%d nxi=%d shared=%s launched %s" % (n, nxi, shared, delta)
    got, ok = res if want_ok else (res, None)
    assert tuple(got.shape) == (nxi, B)
    h = flat.cpu().numpy()
    body = h[off:off + B * ldyi].reshape(B, ldyi)
    assert np.all(body[:, nxi:] == SENTINEL), "padding rows of YI were written"
    assert np.all(h[:off] == SENTINEL) and np.all(h[off + B * ldyi:] == SENTINEL), "wrote outside YI"
    return body[:, :nxi].copy(), (None if ok is None else ok.cpu().numpy().astype(np.int64))


def _check(ctx, Xb, Yb, XI, extrap=np.nan, lens=None, **kw):
    import armadillocudalinearinterpolation_amd as mi
    got, ok = _run(ctx, Xb, Yb, XI, extrap, lens, **kw)
    want, wok = _oracle_each(Xb, Yb, XI, extrap, lens)
    differ = [c for c in range(Xb.shape[0]) if not _eq(got[c], want[c])]
    assert not differ, "%d columns differ from the oracle, first %s" % (len(differ), differ[:5])
    if ok is not None:
        assert np.array_equal(ok, wok), "col_ok differs at %s" % np.nonzero(ok != wok)[0][:5]
    if Xb.shape[0] <= 64:
        assert _eq(got, _grid1_each(ctx, Xb, Yb, XI, extrap, lens, wok))
    if XI.ndim == 1:
        import torch
        ld = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.int64).astype(np.int32)).cuda()
        shared = mi.interp_pairs(ctx, _t(Xb).T, _t(Yb).T, _t(XI), lens=ld, extrap=extrap).T.cpu().numpy()
        assert _eq(got, shared), "differs from interp_pairs on the same inputs"
    return got


# the three forms: (n, nxi) that the dispatcher sends to each of them with per-column queries
FORMS = {"thin": (8, 8), "lds": (1500, 700), "direct": (LDS_MAX_N + 500, 700)}


@pytest.mark.parametrize("n", [2, 3, 8, THIN_N - 1, THIN_N, THIN_N + 1])
def test_thin_form_and_its_thresholds(mi_ctx, n):
    """either side of both thin thresholds, column counts around the wave and the workgroup's block of columns, a
    shared and a per-column XI; past a threshold the call is the LDS form (per-column) or forwarded (shared)"""
    rng = np.random.default_rng(1000 + n)
    for nxi in (1, 2, THIN_Q, THIN_Q + 1):
        for B in (1, 63, 64, 65, 255, 256, 257, 1000):
            Xb, Yb = _pairs(rng, B, n)
            Q = _queries(rng, Xb, nxi)
            _check(mi_ctx, Xb, Yb, Q, extrap=-3.25)
            # a shared vector: the queries of the columns B // 2 and 0 interleaved
            shared = np.where(np.arange(nxi) % 2 == 0, Q[B // 2], Q[0])
            _check(mi_ctx, Xb, Yb, np.ascontiguousarray(shared), extrap=-3.25)


def _two_node_formula(x0, x1, y0, y1, q, extrap):
    """interp1 on the table ((x0, x1), (y0, y1)), vectorised over columns: the bracket is l = 0 for x0 <= q < x1 (r = 1)
    and l = r = 1 at q == x1, where the blend is 1*y1 + 0*y1"""
    with np.errstate(all="ignore"):
        a, b = q - x0, x1 - q
        w = np.where(a > 0, a / (a + b), 0.0)
        v = (1.0 - w) * y0 + w * y1
        last = q == x1
        v = np.where(last, 1.0 * y1 + 0.0 * y1, v)
        v = np.where((q >= x0) & (q <= x1), v, np.where(np.isnan(q), np.nan, extrap))
        bad = ~(np.isfinite(x0) & np.isfinite(x1) & (x0 < x1))
        return np.where(bad, np.nan, v), (~bad).astype(np.int64)


def test_thin_form_workgroups_stride_over_the_blocks(mi_ctx):
    """more columns than one pass of the thin form's grid covers (8 workgroups per compute unit, 256 columns each), two
    nodes and one query of its own per column; the reference is the vectorised two-node formula, asserted bit-equal to
    the oracle column by column on a few thousand of these columns first"""
    import armadillocudalinearinterpolation_amd as mi
    cus = mi_ctx.device_info()["compute_units"]
    B = (cus if cus > 0 else 256) * 8 * BLOCK + 3 * BLOCK + 77
    rng = np.random.default_rng(77)
    x0 = rng.uniform(-5.0, 5.0, B) + 20.0 * np.arange(B)
    x1 = x0 + rng.uniform(0.1, 3.0, B)
    y0, y1 = rng.standard_normal(B), rng.standard_normal(B)
    q = x0 + rng.uniform(-0.1, 1.1, B) * (x1 - x0)
    pick = rng.integers(0, 24, B)
    q = np.where(pick == 0, x0, np.where(pick == 1, x1, np.where(pick == 2, np.nan, np.where(pick == 3, np.inf, np.where(pick == 4, -np.inf, q)))))
    y0 = np.where(pick == 5, np.inf, np.where(pick == 6, -0.0, np.where(pick == 7, np.nan, y0)))
    y1 = np.where(pick == 8, -np.inf, np.where(pick == 9, 0.0, np.where(pick == 10, np.nan, np.where(pick == 6, -0.0, y1))))
    x0 = np.where(pick == 11, -0.0, x0)                       # (a wide bracket: the column stays good)
    x1 = np.where(pick == 12, x0, np.where(pick == 13, np.inf, np.where(pick == 14, np.nan, x1)))
    q[B - 1], q[B - BLOCK] = x1[B - 1], x0[B - BLOCK]
    for extrap in (7.5,):
        want, wok = _two_node_formula(x0, x1, y0, y1, q, extrap)
        idx = np.concatenate([np.arange(0, 1500), rng.choice(B, 2500, replace=False), np.arange(B - 300, B)])
        for c in idx:
            x = np.array([x0[c], x1[c]])
            ref = oracle.interp1_bracket(x, np.array([y0[c], y1[c]]), np.array([q[c]]), extrap)[0] if not _is_bad(x) else np.nan
            assert _eq(np.array([want[c]]), np.array([ref])), (c, want[c], ref)
        assert 0 < wok.sum() < B and (pick[idx] < 15).any()
        Xb, Yb = np.stack([x0, x1], axis=1), np.stack([y0, y1], axis=1)
        before = _counts(mi_ctx)
        got, ok = mi.interp_each(mi_ctx, _t(Xb).T, _t(Yb).T, _t(q[:, None]).T, extrap=extrap, want_ok=True)
        assert [a - b for a, b in zip(_counts(mi_ctx), before)] == [1, 0, 0, 0]
        got, ok = got.T.cpu().numpy()[:, 0], ok.cpu().numpy()
        wrong = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))) | (np.signbit(got) != np.signbit(want)) & (want == 0))[0]
        assert wrong.size == 0, "%d columns differ, first %s" % (wrong.size, wrong[:5])
        assert np.array_equal(ok, wok)


@pytest.mark.parametrize("n", [THIN_N + 1, 1024, LDS_MAX_N - 1, LDS_MAX_N])
def test_lds_form(mi_ctx, n):
    """per-column queries through the LDS form: row counts either side of 256 and of a row block, 1, 2, 3 and 37
    columns, queries sorted and in random order"""
    rng = np.random.default_rng(2000 + n)
    for nxi in (1, 255, 2047, 2048, 2049, 5000):
        for B in (1, 2, 3, 37):
            Xb, Yb = _pairs(rng, B, n)
            for order in ("sorted", "permuted"):
                _check(mi_ctx, Xb, Yb, _queries(rng, Xb, nxi, order=order), extrap=0.5, ldyi_pad=B % 2)


def test_lds_form_workgroups_stride_over_the_units(mi_ctx):
    """more units of work than the launch has workgroups (16 per compute unit) on a 256-CU device: 3 row blocks x 1366
    column runs = 4098 units"""
    import armadillocudalinearinterpolation_amd as mi
    n, B, nxi = 64, 2 * 1366, 2 * ROW_BLOCK + 10
    rng = np.random.default_rng(n + B)
    Xb, Yb = _pairs(rng, B, n)
    lo, hi = Xb[:, :1], Xb[:, -1:]
    Q = lo - 0.05 * (hi - lo) + rng.uniform(0.0, 1.1, (B, nxi)) * (hi - lo)
    Q[:, 5], Q[:, nxi - 1], Q[:, 2048], Q[:, 17] = Xb[:, 0], Xb[:, -1], Xb[:, n // 2], np.nan
    before = _counts(mi_ctx)
    got = mi.interp_each(mi_ctx, _t(Xb).T, _t(Yb).T, _t(Q).T, extrap=-1.0).T.cpu().numpy()
    assert [a - b for a, b in zip(_counts(mi_ctx), before)] == [0, 1, 0, 0]
    assert got.shape == (B, nxi)
    wrong = [c for c in range(B) if not _eq(got[c], oracle.interp1_bracket(Xb[c], Yb[c], np.ascontiguousarray(Q[c]), -1.0))]
    assert not wrong, "%d columns differ, first %s" % (len(wrong), wrong[:5])


@pytest.mark.parametrize("n", [LDS_MAX_N + 1, LDS_MAX_N + 2, 50_001])
def test_direct_form(mi_ctx, n):
    """columns longer than the LDS form takes, even and odd, with col_ok (flags in the caller's array) and without
    (flags in the context's workspace)"""
    rng = np.random.default_rng(3000 + n)
    for B, nxi in [(5, 1500), (4, 3001), (1, 1)]:
        Xb, Yb = _pairs(rng, B, n)
        Q = _queries(rng, Xb, nxi)
        got = _check(mi_ctx, Xb, Yb, Q, extrap=-8.0)
        blind, none = _run(mi_ctx, Xb, Yb, Q, -8.0, want_ok=False)
        assert none is None and _eq(blind, got)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_padded_leading_dimensions_and_alignment(mi_ctx, form):
    """ldx, ldy, ldxi and ldyi padded differently (NaN below the columns of x, y and xi, a sentinel below those of yi,
    checked by _run), odd and even, and x, y, xi, yi each 8-B but not 16-B aligned, so that both load and both store
    widths run"""
    n, nxi = FORMS[form]
    rng = np.random.default_rng(len(form))
    for nn, mm in [(n, nxi), (n - 1, nxi - 1)]:
        Xb, Yb = _pairs(rng, 7, nn)
        Q = _queries(rng, Xb, mm)
        for ldx_pad, ldy_pad, ldxi_pad, ldyi_pad, misalign in [(0, 0, 0, 0, False), (1, 3, 2, 1, False), (2, 4, 1, 2, False),
                                                               (3, 1, 5, 0, True), (0, 2, 0, 3, True), (4, 2, 3, mm % 2, False),
                                                               (2, 2, 2, 2, True)]:
            _check(mi_ctx, Xb, Yb, Q, extrap=9.0, ldx_pad=ldx_pad, ldy_pad=ldy_pad, ldxi_pad=ldxi_pad, ldyi_pad=ldyi_pad,
                   misalign=misalign)
        _check(mi_ctx, Xb, Yb, np.ascontiguousarray(Q[3]), extrap=9.0, ldx_pad=1, ldy_pad=2, ldyi_pad=1, misalign=True)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_ragged_columns(mi_ctx, form):
    """len of 2, 3, n and random values between; the rows past n_c hold NaN in one run and decreasing finite values in
    another: neither changes a bit or makes a column bad; len = NULL equals len = n"""
    n, nxi = FORMS[form]
    rng = np.random.default_rng(n + 1)
    B = 41
    Xb, Yb = _pairs(rng, B, n)
    lens = rng.integers(2, n + 1, B)
    lens[:6] = [2, 3, n, n - 1, 2, n]
    Q = _queries(rng, Xb, nxi, lens)
    want, wok = _oracle_each(Xb, Yb, Q, 7.0, lens)
    assert wok.all()
    for fill in ("nan", "decreasing"):
        Xf, Yf = Xb.copy(), Yb.copy()
        for c in range(B):
            m = n - lens[c]
            Xf[c, lens[c]:] = np.nan if fill == "nan" else Xb[c, lens[c] - 1] - 1.0 - np.arange(m)
            Yf[c, lens[c]:] = np.nan if fill == "nan" else 1e300
        got = _check(mi_ctx, Xf, Yf, Q, extrap=7.0, lens=lens, ldx_pad=1)
        assert _eq(got, want)
    a, _ = _run(mi_ctx, Xb, Yb, Q, 7.0, np.full(B, n))
    b, _ = _run(mi_ctx, Xb, Yb, Q, 7.0, None)
    assert _eq(a, b)


def _defects(Xb, lens):
    """one defect per column, a good column between two bad ones: equal neighbours, a decrease by one ulp, the pair
    -0.0, 0.0, a NaN, +inf and -inf nodes -- each at the first pair, a middle pair and the last valid pair.  Returns the
    bad columns."""
    bad = []
    c = 1
    n = Xb.shape[1]
    for kind in ("equal", "decrease", "zeros", "nan", "inf", "ninf"):
        for where in ("first", "middle", "last"):
            nc = _col_len(lens, c, n)
            k = {"first": 0, "middle": (nc - 2) // 2, "last": nc - 2}[where]
            x = Xb[c]
            if kind == "equal":
                x[k + 1] = x[k]
            elif kind == "decrease":
                x[k + 1] = np.nextafter(x[k], -np.inf)
            elif kind == "zeros":
                x[:] = x - x[k + 1]
                assert x[k + 1] == 0.0 and (k == 0 or x[k - 1] < 0.0)
                x[k] = -0.0
            elif kind == "nan":
                x[k + (c >> 1 & 1)] = np.nan
            elif kind == "inf":
                x[nc - 1 if where == "last" else k + 1] = np.inf       # (inside the column it also breaks the order)
            else:
                x[0 if where == "first" else k] = -np.inf
            bad.append(c)
            c += 2
    assert c <= Xb.shape[0]
    return bad


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("ldx_pad", [0, 1])
def test_bad_columns(mi_ctx, form, ldx_pad):
    """every kind of broken column at the first, a middle and the last valid pair, with and without ragged lengths, and
    len of 0, 1 and n + 1: such a column is all NaN whatever extrap is, with col_ok 0; every other column has col_ok 1
    and is bit-equal to a call that never saw the bad ones; col_ok = NULL gives the same outputs"""
    n, nxi = FORMS[form]
    rng = np.random.default_rng(n * 2 + ldx_pad)
    B = 2 * 18 + 10
    Xb, Yb = _pairs(rng, B, n)
    clean = Xb.copy()
    for ragged in (False, True):
        Xb = clean.copy()
        lens = None
        if ragged:
            lens = rng.integers(max(4, n // 2), n + 1, B)
        bad = _defects(Xb, lens)
        Q = _queries(rng, clean, nxi, lens)
        if ragged:
            lens[B - 2], lens[B - 4], lens[B - 6] = 0, 1, n + 1
            bad += [B - 2, B - 4, B - 6]
        for extrap in (3.5, np.inf):
            got, ok = _run(mi_ctx, Xb, Yb, Q, extrap, lens, ldx_pad=ldx_pad)
            want, wok = _oracle_each(Xb, Yb, Q, extrap, lens)
            assert sorted(np.nonzero(wok == 0)[0].tolist()) == sorted(bad)
            assert np.array_equal(ok, wok), "col_ok differs at %s" % np.nonzero(ok != wok)[0][:8]
            assert np.isnan(got[bad]).all()
            assert _eq(got, want)
        good = np.nonzero(wok)[0]
        base, bok = _run(mi_ctx, clean[good], Yb[good], Q[good], extrap, None if lens is None else lens[good], ldx_pad=ldx_pad)
        assert bok.all() and _eq(got[good], base)
        blind, none = _run(mi_ctx, Xb, Yb, Q, extrap, lens, ldx_pad=ldx_pad, want_ok=False)
        assert none is None and _eq(blind, got)
    if form == "thin":   # two-node columns have one pair only: each kind once, and the shared-XI route
        Xb, Yb = _pairs(rng, 16, 2)
        Q = _queries(rng, Xb, 3)
        Xb[1, 1] = Xb[1, 0]
        Xb[3, 1] = np.nextafter(Xb[3, 0], -np.inf)
        Xb[5] = [-0.0, 0.0]
        Xb[7, 0] = np.nan
        Xb[9, 1] = np.inf
        Xb[11, 0] = -np.inf
        Xb[13, 1] = np.nan
        for XI in (Q, np.ascontiguousarray(Q[2])):
            got = _check(mi_ctx, Xb, Yb, XI, extrap=1.0)
            assert np.isnan(got[1::2][:7]).all() and not np.isnan(got[0::2]).all()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_inf_nan_and_negative_zero_stay_inside_their_column(mi_ctx, form):
    """inf, NaN and -0.0 in Y at and beside bracket nodes go through the two-term blend as interp1 passes them (the
    oracle column by column), and the neighbouring columns' outputs are those of a call that never saw them"""
    n, nxi = FORMS[form]
    rng = np.random.default_rng(n)
    B = 9
    Xb, clean = _pairs(rng, B, n)
    Yb = clean.copy()
    k = n // 3
    Yb[1, k], Yb[1, 0] = np.inf, -np.inf
    Yb[3, k], Yb[3, n - 1] = np.nan, np.nan
    Yb[5, k], Yb[5, k + 1], Yb[5, n - 1], Yb[5, 0] = -0.0, -0.0, -0.0, -0.0
    Yb[7, n - 1], Yb[7, n - 2] = np.inf, -0.0
    Q = _queries(rng, Xb, nxi)
    for c in (1, 3, 5, 7):   # at, beside and between the special nodes
        X = Xb[c]
        at = [X[k], X[k - 1], X[k + 1], 0.5 * (X[k] + X[k + 1]), 0.5 * (X[k - 1] + X[k]), X[0], X[n - 1], X[n - 2],
              0.5 * (X[n - 2] + X[n - 1]), np.nextafter(X[k], np.inf), np.nextafter(X[k], -np.inf), 0.5 * (X[0] + X[1])]
        Q[c, :min(len(at), nxi)] = at[:nxi]
    got = _check(mi_ctx, Xb, Yb, Q, extrap=np.inf)
    assert np.isinf(got[1]).any() and np.isnan(got[3]).any() and (np.signbit(got[5]) & (got[5] == 0)).any()
    base, _ = _run(mi_ctx, Xb, clean, Q, np.inf)
    for c in (0, 2, 4, 6, 8):
        assert _eq(got[c], base[c])


@pytest.mark.parametrize("extrap", [2.5, -0.0, np.inf, -np.inf, np.nan])
def test_extrapolation_values(mi_ctx, extrap):
    rng = np.random.default_rng(5)
    for n, nxi in FORMS.values():
        Xb, Yb = _pairs(rng, 14, n)
        Q = _queries(rng, Xb, nxi)
        got = _check(mi_ctx, Xb, Yb, Q, extrap=extrap)
        oor = (Q < Xb[:, :1]) | (Q > Xb[:, -1:])
        assert oor.any() and np.isnan(got[np.isnan(Q)]).all()
        if not np.isnan(extrap):
            assert np.all(got[oor] == extrap) and np.all(np.signbit(got[oor]) == np.signbit(extrap))


def test_empty_calls_and_argument_errors(mi_ctx):
    """B == 0 or nxi == 0 is MI_OK with nothing launched or written; MI_ERR_INVALID_ARG for NULL or misaligned
    pointers, ldx < n, ldy < n, ldyi < nxi, 0 < ldxi < nxi, n < 2 and overflowing sizes -- each with a mi_last_error
    text that names the culprit, none writing or launching anything"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, ch = mi_ctx._L, mi_ctx._h
    n, B, nxi = 50, 4, 30
    x = torch.arange(B * n + 1, dtype=torch.float64, device="cuda")
    y = torch.zeros(B * n + 1, dtype=torch.float64, device="cuda")
    xi = torch.full((B * nxi + 1,), 0.5, dtype=torch.float64, device="cuda")
    yi = torch.full((B * nxi + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    ln = torch.full((B + 1,), n, dtype=torch.int32, device="cuda")
    okt = torch.full((B + 1,), 77, dtype=torch.int32, device="cuda")
    p = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)  # noqa: E731

    def call(fn=L.mi_interp1_each_f64_dev, xp=p(x), ldx=n, yp=p(y), ldy=n, nn=n, lp=p(ln), ncols=B, qp=p(xi), ldxi=nxi, m=nxi,
             op=p(yi), ldyi=nxi, kp=p(okt)):
        return fn(ch, xp, ldx, yp, ldy, nn, lp, ncols, qp, ldxi, m, op, ldyi, 0.0, kp)

    def err():
        return (L.mi_last_error(ch) or b"").decode()

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((okt[:B] == 1).all()) and int(okt[B]) == 77
    yi.fill_(SENTINEL)
    okt.fill_(77)
    before = _counts(mi_ctx)
    assert call(ncols=0) == 0 and call(m=0) == 0 and call(ncols=0, xp=None, yp=None, op=None) == 0 and call(m=0, qp=None) == 0
    assert call(m=0, ldxi=0) == 0 and call(ncols=0, ldxi=0) == 0
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()) and bool((okt == 77).all()), "an empty call wrote something"
    hx, hy, hq, ho = np.arange(B * n, dtype=np.float64), np.zeros(B * n), np.full(B * nxi, 0.5), np.full(B * nxi, SENTINEL)
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    host = L.mi_interp1_each_f64_host
    assert host(ch, hp(hx), n, hp(hy), n, n, None, 0, hp(hq), nxi, nxi, hp(ho), nxi, 0.0, None) == 0
    assert host(ch, hp(hx), n, hp(hy), n, n, None, B, hp(hq), nxi, 0, hp(ho), nxi, 0.0, None) == 0
    assert np.all(ho == SENTINEL)
    INVALID = 1
    for kw, word in [(dict(ldx=n - 1), "ldx"), (dict(ldy=n - 1), "ldy"), (dict(ldyi=nxi - 1), "ldyi"), (dict(ldxi=nxi - 1), "ldxi"),
                     (dict(ldxi=1), "ldxi"), (dict(nn=1, ldx=1, ldy=1), "n=1"),
                     (dict(xp=p(x, 4)), "aligned"), (dict(yp=p(y, 4)), "aligned"), (dict(qp=p(xi, 4)), "aligned"),
                     (dict(op=p(yi, 4)), "aligned"), (dict(lp=p(ln, 2)), "aligned"), (dict(kp=p(okt, 2)), "aligned"),
                     (dict(xp=None), "NULL"), (dict(yp=None), "NULL"), (dict(qp=None), "NULL"), (dict(op=None), "NULL"),
                     (dict(ncols=2 ** 62), "too large"), (dict(ldyi=2 ** 61), "too large"), (dict(ldxi=2 ** 61), "too large")]:
        assert call(**kw) == INVALID, kw
        assert word in err(), (kw, err())
    assert L.mi_interp1_each_f64_dev(None, p(x), n, p(y), n, n, None, B, p(xi), nxi, nxi, p(yi), nxi, 0.0, None) == INVALID
    for args, word in [((hp(hx), n - 1, hp(hy), n), "ldx"), ((hp(hx), n, hp(hy), n - 1), "ldy"), ((None, n, hp(hy), n), "NULL")]:
        assert host(ch, *args, n, None, B, hp(hq), nxi, nxi, hp(ho), nxi, 0.0, None) == INVALID and word in err()
    assert host(ch, hp(hx), n, hp(hy), n, n, None, B, hp(hq), nxi, nxi, hp(ho), nxi - 1, 0.0, None) == INVALID and "ldyi" in err()
    assert host(ch, hp(hx), n, hp(hy), n, n, None, B, hp(hq), nxi - 1, nxi, hp(ho), nxi, 0.0, None) == INVALID and "ldxi" in err()
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()) and np.all(ho == SENTINEL) and bool((okt == 77).all()), "a refused call wrote something"
    assert _counts(mi_ctx) == before, "an empty or a refused call launched something"
    # 8-B aligned pointers that are not 16-B aligned, 4-B aligned counts and flags are fine; len and col_ok may be NULL;
    # ldxi == 0 shares the first nxi queries
    assert call(xp=p(x, 8), yp=p(y, 8), qp=p(xi, 8), op=p(yi, 8), lp=p(ln, 4), kp=p(okt, 4)) == 0
    assert call(lp=None, kp=None) == 0 and call(ldxi=0) == 0
    torch.cuda.synchronize()
    X, Y = x[:B * n].view(B, n), y[:B * n].view(B, n)
    with pytest.raises(ValueError):
        mi.interp_each(mi_ctx, torch.zeros((n, B), dtype=torch.float64, device="cuda"),
                       torch.zeros((n, B), dtype=torch.float64, device="cuda"), xi[:nxi])                # row-major (n, B)
    with pytest.raises(ValueError):
        mi.interp_each(mi_ctx, X.T, Y.T, xi[:B * nxi].view(nxi, B))                                      # row-major XI
    with pytest.raises(ValueError):
        mi.interp_each(mi_ctx, X.T, Y.T, xi[:(B - 1) * nxi].view(B - 1, nxi).T)                          # XI: B - 1 columns
    with pytest.raises(ValueError):
        mi.interp_each(mi_ctx, X.T, y[:(B - 1) * n].view(B - 1, n).T, xi[:nxi])                          # shapes differ
    with pytest.raises(ValueError):
        mi.interp_each(mi_ctx, X.T, Y.T, xi[:2 * nxi:2])                                                 # strided shared XI


@pytest.mark.parametrize("form", ["thin", "lds"])
def test_hipgraph_capture(mi_ctx, form):
    """a thin-form and an LDS-form call are one kernel each on the context's stream and allocate nothing: captured
    once, replayed twice with X, Y and XI overwritten in place between the replays, equal to the eager call each time"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(8)
    n, B, nxi = {"thin": (2, 3000, 1), "lds": (1024, 300, 2500)}[form]
    Xb, Yb = _pairs(rng, B, n)
    xd, yd, qd = _t(Xb), _t(Yb), _t(_queries(rng, Xb, nxi))
    out = torch.full((B, nxi), SENTINEL, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mi_ctx.use_torch_stream()
        mi.interp_each(mi_ctx, xd.T, yd.T, qd.T, out=out.T)               # warm-up outside capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mi_ctx.use_torch_stream()
            _, ok = mi.interp_each(mi_ctx, xd.T, yd.T, qd.T, out=out.T, want_ok=True)
    torch.cuda.current_stream().wait_stream(side)
    mi_ctx.use_torch_stream()
    for rep in range(2):
        Xn, Yn = _pairs(rng, B, n)
        Xn[rep + 5, n - 1] = Xn[rep + 5, n - 2]
        Qn = _queries(rng, Xn, nxi)
        xd.copy_(_t(Xn))
        yd.copy_(_t(Yn))
        qd.copy_(_t(Qn))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        got, gok = out.cpu().numpy(), ok.cpu().numpy()
        eager, eok = mi.interp_each(mi_ctx, xd.T, yd.T, qd.T, want_ok=True)
        want, wok = _oracle_each(Xn, Yn, Qn)
        assert _eq(got, eager.T.cpu().numpy()) and _eq(got, want)
        assert np.array_equal(gok, wok) and np.array_equal(eok.cpu().numpy(), wok) and not wok[rep + 5]


def test_workspace_flags_back_to_back_with_the_other_slot_3_calls(mi_ctx):
    """the direct form without col_ok keeps its flags in context scratch slot 3, as the paired-column, the shared-axis
    and the gridded calls keep theirs: interleaved on one context and stream without a synchronisation, each gives its
    own result"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(33)
    nx, ny = 70, 90
    xg, yg = np.cumsum(rng.uniform(0.2, 1.0, nx)), np.cumsum(rng.uniform(0.1, 2.0, ny)) - 3.0
    Z = rng.standard_normal((ny, nx))
    g2 = mi.Grid2.from_axes(mi_ctx, xg, yg, Z)
    gx = rng.uniform(xg[0] - 1, xg[-1] + 1, 3000)
    gy = rng.uniform(yg[0] - 1, yg[-1] + 1, 700)
    n, B, nxi = LDS_MAX_N + 904, 40, 3000
    Xb, Yb = _pairs(rng, B, n)
    Q = _queries(rng, Xb, nxi)
    Xb[3, 100] = Xb[3, 99]
    Xb[17, n - 1] = np.nan
    Xp = Xb[::-1].copy()                                     # the paired-column call sees other bad columns: 36 and 22
    X = Xb[0].copy()
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    xd, xpd, yd, gxd, gyd, qd, q0 = _t(Xb), _t(Xp), _t(Yb), _t(gx), _t(gy), _t(Q), _t(Q[0])
    torch.cuda.synchronize()
    e1 = mi.interp_each(mi_ctx, xd.T, yd.T, qd.T)
    p1 = mi.interp_pairs(mi_ctx, xpd.T, yd.T, q0)
    e2 = mi.interp_each(mi_ctx, xd.T, yd.T, qd.T)
    a1 = axis.interp_cols(yd.T, q0)
    e3 = mi.interp_each(mi_ctx, xd.T, yd.T, qd.T)
    z1 = g2.interp_grid(gxd, gyd)
    e4 = mi.interp_each(mi_ctx, xd.T, yd.T, qd.T)
    p2 = mi.interp_pairs(mi_ctx, xpd.T, yd.T, q0)
    torch.cuda.synchronize()
    want, wok = _oracle_each(Xb, Yb, Q)
    assert not wok[3] and not wok[17] and wok.sum() == B - 2
    for e in (e1, e2, e3, e4):
        assert _eq(e.T.cpu().numpy(), want)
    pref, pok = _oracle_each(Xp, Yb, Q[0])
    assert not pok[B - 4] and not pok[B - 18] and pok.sum() == B - 2
    assert _eq(p1.T.cpu().numpy(), pref) and _eq(p2.T.cpu().numpy(), pref)
    XX, YY = np.meshgrid(gx, gy)
    zref = oracle.interp2_bilinear(xg, yg, Z, XX.ravel("F"), YY.ravel("F"), np.nan, nthreads=8).reshape(gy.size, gx.size, order="F")
    assert _eq(z1.cpu().numpy(), zref)
    aref = np.stack([oracle.interp1_bracket(X, Yb[c], np.ascontiguousarray(Q[0])) for c in range(B)])
    assert _eq(a1.T.cpu().numpy(), aref)
    axis.close()
    g2.close()


def test_host_path_below_and_above_its_chunking_threshold(mi_ctx, monkeypatch):
    """one-shot and chunked (more than 2 x 8 M elements: pinned, pipelined column chunks, XI travelling with its
    columns) host calls equal the device call; nothing stays pinned afterwards, also after a failure forced in the middle
    of the chunk loop; MI_ERR_GRID for a bad column without col_ok, MI_OK with it, the outputs complete either way"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L = mi_ctx._L
    rng = np.random.default_rng(11)
    assert L.mi_debug_pinned_ranges() == 0
    # the thin shape, one-shot, per-column and shared queries
    Xb, Yb = _pairs(rng, 5000, 2)
    Q = _queries(rng, Xb, 1)
    for XI in (Q, np.ascontiguousarray(Q[7])):
        got = mi.interp_each_host(mi_ctx, Xb.T, Yb.T, XI.T if XI.ndim == 2 else XI, extrap=1.5)
        assert _eq(got.T, _oracle_each(Xb, Yb, XI, 1.5)[0]) and L.mi_debug_pinned_ranges() == 0
    n, nxi = 1024, 2048
    for B in (50, 9001):                                # 9001 x 2048 > 2 x 8 M: three chunks of 4096 columns
        Xb, Yb = _pairs(rng, B, n)
        lens = rng.integers(2, n + 1, B)
        lo, hi = Xb[:, :1], Xb[np.arange(B), lens - 1][:, None]
        Q = lo - 0.05 * (hi - lo) + rng.uniform(0.0, 1.1, (B, nxi)) * (hi - lo)
        Q[:, 3], Q[:, 4], Q[:, 5] = lo[:, 0], hi[:, 0], np.nan
        ld = torch.from_numpy(lens.astype(np.int32)).cuda()
        dev = mi.interp_each(mi_ctx, _t(Xb).T, _t(Yb).T, _t(Q).T, lens=ld, extrap=1.5).T.cpu().numpy()
        got = mi.interp_each_host(mi_ctx, Xb.T, Yb.T, Q.T, lens=lens, extrap=1.5)
        assert got.shape == (nxi, B) and got.flags["F_CONTIGUOUS"]
        assert _eq(got.T, dev) and L.mi_debug_pinned_ranges() == 0
        idx = np.arange(0, B, 97)
        assert _eq(dev[idx], _oracle_each(Xb[idx], Yb[idx], Q[idx], 1.5, lens[idx])[0])
        # a shared XI through the host form equals the paired-column host call
        sh = mi.interp_each_host(mi_ctx, Xb.T, Yb.T, Q[B // 2], lens=lens, extrap=1.5)
        assert _eq(sh, mi.interp_pairs_host(mi_ctx, Xb.T, Yb.T, Q[B // 2], lens=lens, extrap=1.5)) and L.mi_debug_pinned_ranges() == 0
        # padded leading dimensions on the host side
        ldx, ldy, ldxi, ldyi = n + 1, n + 3, nxi + 2, nxi + 5
        hx, hy, hq = np.full((B, ldx), np.nan), np.full((B, ldy), np.nan), np.full((B, ldxi), np.nan)
        hx[:, :n], hy[:, :n], hq[:, :nxi] = Xb, Yb, Q
        ho = np.full((B, ldyi), SENTINEL)
        hl = lens.astype(np.uint32)
        hok = np.full(B, 9, dtype=np.uint32)
        st = L.mi_interp1_each_f64_host(mi_ctx._h, C.c_void_p(hx.ctypes.data), ldx, C.c_void_p(hy.ctypes.data), ldy, n,
                                        C.c_void_p(hl.ctypes.data), B, C.c_void_p(hq.ctypes.data), ldxi, nxi,
                                        C.c_void_p(ho.ctypes.data), ldyi, 1.5, C.c_void_p(hok.ctypes.data))
        assert st == 0 and L.mi_debug_pinned_ranges() == 0 and np.all(hok == 1)
        assert _eq(ho[:, :nxi], dev) and np.all(ho[:, nxi:] == SENTINEL)
        # the status rule: a bad column in the first and one in the last chunk
        Xbad = Xb.copy()
        Xbad[3, 1] = Xbad[3, 0]
        Xbad[B - 2, lens[B - 2] - 1] = np.nan
        g2, ok2 = mi.interp_each_host(mi_ctx, Xbad.T, Yb.T, Q.T, lens=lens, extrap=1.5, want_ok=True)
        assert ok2.dtype == np.uint32 and sorted(np.nonzero(ok2 == 0)[0].tolist()) == [3, B - 2]
        assert np.isnan(g2[:, 3]).all() and np.isnan(g2[:, B - 2]).all()
        keep = np.ones(B, dtype=bool)
        keep[[3, B - 2]] = False
        assert _eq(g2.T[keep], dev[keep])
        hx[:, :n] = Xbad
        ho.fill(SENTINEL)
        st = L.mi_interp1_each_f64_host(mi_ctx._h, C.c_void_p(hx.ctypes.data), ldx, C.c_void_p(hy.ctypes.data), ldy, n,
                                        C.c_void_p(hl.ctypes.data), B, C.c_void_p(hq.ctypes.data), ldxi, nxi,
                                        C.c_void_p(ho.ctypes.data), ldyi, 1.5, None)
        assert st == 2 and b"column 3 " in L.mi_last_error(mi_ctx._h) and L.mi_debug_pinned_ranges() == 0
        assert _eq(ho[:, :nxi], g2.T), "the outputs are complete when the status is MI_ERR_GRID"
        with pytest.raises(mi.MiError) as e:
            mi.interp_each_host(mi_ctx, Xbad.T, Yb.T, Q.T, lens=lens)
        assert e.value.code == 2
    monkeypatch.setenv("MI_TEST_FAIL_EACH_CHUNK", "1")
    with pytest.raises(mi.MiError) as e:
        mi.interp_each_host(mi_ctx, Xb.T, Yb.T, Q.T, lens=lens)
    assert "MI_TEST_FAIL_EACH_CHUNK" in str(e.value) and L.mi_debug_pinned_ranges() == 0
    monkeypatch.delenv("MI_TEST_FAIL_EACH_CHUNK")
    assert _eq(mi.interp_each_host(mi_ctx, Xb.T, Yb.T, Q.T, lens=lens, extrap=1.5).T, dev) and L.mi_debug_pinned_ranges() == 0


def _group_devices():
    import torch
    return {"single": [0], "rehearsal": [0, 0, 0], "all_gpus": list(range(max(1, torch.cuda.device_count())))}


@pytest.mark.parametrize("which", ["single", "rehearsal", "all_gpus"])
def test_group_call_shards_the_columns(mi_ctx, which):
    """member r takes the columns mi_shard_bounds(B, r, P) and, with per-column queries, those columns of XI; a shared
    XI is replicated; B smaller than, equal to and not divisible by P, bad columns included; bit-equal to the
    single-device call in all three forms.  all_gpus is [0, 1, ..] over every device of the machine"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    devices = _group_devices()[which]
    P = len(devices)
    grp = mi.Group(devices)
    rng = np.random.default_rng(P)
    for n, nxi in FORMS.values():
        for B in sorted({1, max(P - 1, 1), P, 2 * P, 37, 8 * P + 3}):
            Xb, Yb = _pairs(rng, B, n)
            lens = rng.integers(2, n + 1, B)
            Q = _queries(rng, Xb, nxi, lens)
            if B >= 2:
                Xb[B - 1, 1] = Xb[B - 1, 0]
            if B >= 37:
                Xb[20, lens[20] - 1] = np.inf
            ld = torch.from_numpy(lens.astype(np.int32)).cuda()
            for XI in (Q, np.ascontiguousarray(Q[B // 2])):
                arg = _t(XI).T if XI.ndim == 2 else _t(XI)
                one, ok1 = mi.interp_each(mi_ctx, _t(Xb.copy()).T, _t(Yb.copy()).T, arg, lens=ld, extrap=-4.0, want_ok=True)
                one, ok1 = one.T.cpu().numpy(), ok1.cpu().numpy()
                got, ok = grp.interp_each_host(Xb.T, Yb.T, XI.T if XI.ndim == 2 else XI, lens=lens, extrap=-4.0, want_ok=True)
                assert got.shape == (nxi, B)
                want, wok = _oracle_each(Xb, Yb, XI, -4.0, lens)
                assert _eq(got.T, one) and _eq(one, want)
                assert np.array_equal(ok, wok) and np.array_equal(ok1, wok)
            if B >= 2:
                with pytest.raises(mi.MiError) as e:
                    grp.interp_each_host(Xb.T, Yb.T, Q.T, lens=lens)
                assert e.value.code == 2 and "column" in str(e.value)
    # above the size from which the group call page-locks the caller's arrays (2 x 8 M elements)
    n, nxi, B = 1024, 2048, 9001
    Xb, Yb = _pairs(rng, B, n)
    lo, hi = Xb[:, :1], Xb[:, -1:]
    Q = lo - 0.05 * (hi - lo) + rng.uniform(0.0, 1.1, (B, nxi)) * (hi - lo)
    Xb[B - 3, 5] = np.nan
    one = mi.interp_each(mi_ctx, _t(Xb).T, _t(Yb).T, _t(Q).T, extrap=-4.0).T.cpu().numpy()
    got, ok = grp.interp_each_host(Xb.T, Yb.T, Q.T, extrap=-4.0, want_ok=True)
    assert _eq(got.T, one) and sorted(np.nonzero(ok == 0)[0].tolist()) == [B - 3]
    idx = np.arange(0, B, 97)
    assert _eq(one[idx], _oracle_each(Xb[idx], Yb[idx], Q[idx], -4.0)[0])
    assert mi_ctx._L.mi_debug_pinned_ranges() == 0
    assert grp.interp_each_host(np.zeros((5, 0)), np.zeros((5, 0)), np.zeros((3, 0))).shape == (3, 0)
    grp.close()


def test_cpp_arma_interp1_each(tmp_path):
    """mi355::interp1_each and its DeviceGroup form from C++, on long columns (LDS form) and on two-node columns with one
    query each (thin form): YI is XI.n_rows x Y.n_cols and bit-equal to the oracle column by column, the ok vectors name
    the bad columns, a shape mismatch throws std::invalid_argument"""
    from armadillocudalinearinterpolation_amd import _build as b
    b.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST, "arma_interp1_each_test"])
    out = subprocess.run([os.path.join(HOST, "arma_interp1_each_test"), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    dims = {w[0]: (int(w[1]), int(w[2])) for w in lines if w and w[0] in ("YP", "YE", "YG", "YR", "YRG")}
    assert ["threw", "2"] in lines, "mismatched shapes of Y and of XI must throw std::invalid_argument"
    assert ["bad_status", "2"] in lines, "a bad column without an ok vector is MI_ERR_GRID"
    rd = lambda f, dt=np.float64: np.fromfile(os.path.join(tmp_path, "e_%s.bin" % f), dtype=dt)  # noqa: E731
    n = int(rd("N", np.uint32)[0])
    Xb, Yb = rd("X").reshape(-1, n), rd("Y").reshape(-1, n)          # column-major n x B on disk = (B, n) rows
    B = Xb.shape[0]
    Q = rd("XI").reshape(B, -1)
    nxi = Q.shape[1]
    assert all(dims[k] == (nxi, B) for k in ("YP", "YE", "YG"))
    ref, wok = _oracle_each(Xb, Yb, Q)
    assert 0 < wok.sum() < B and np.isnan(ref[wok == 1]).any() and not np.isnan(ref[wok == 1]).all()
    for k in ("YP", "YG"):
        assert _eq(rd(k).reshape(B, nxi), ref), k
    assert _eq(rd("YE").reshape(B, nxi), _oracle_each(Xb, Yb, Q, -7.5)[0])
    assert np.array_equal(rd("OK", np.uint32), wok) and np.array_equal(rd("OKG", np.uint32), wok)
    X2, Y2 = rd("X2").reshape(-1, 2), rd("Y2").reshape(-1, 2)
    B2 = X2.shape[0]
    Q2 = rd("Q2").reshape(B2, 1)
    assert dims["YR"] == (1, B2) and dims["YRG"] == (1, B2)
    ref2, wok2 = _oracle_each(X2, Y2, Q2, 99.0)
    assert wok2.sum() == B2 - 1 and (ref2 == 99.0).any() and np.isnan(ref2).any()
    assert _eq(rd("YR").reshape(B2, 1), ref2) and _eq(rd("YRG").reshape(B2, 1), ref2)
    assert np.array_equal(rd("OK2", np.uint32), wok2) and np.array_equal(rd("OK2G", np.uint32), wok2)
