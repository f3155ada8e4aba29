"""interp1 over paired rows (mi_interp1_rowpairs_f64_dev, mi_debug_rowpairs_launches, mi.interp_rowpairs): YI[r, :] is
interp1 of XI on the table (X[r, :n_r], Y[r, :n_r]), NaN for a bad row.  The reference is the CPU oracle row by row,
oracle.interp1_bracket on the first n_r nodes, for EVERY row, and -- where a test says so -- the shipped interp_pairs on
the transposed data and Axis1.interp_rows.  Every comparison is np.array_equal(..., equal_nan=True) on every output plus
the sign of zeros: no tolerance, no sampling.

Matrices are (m, n) numpy arrays here; on the device they are C-contiguous (n, ld) "time-major" buffers, row k of the
buffer being node k of every row (column k of the column-major matrix)."""
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
W = 64                      # lanes of a wave: a lane owns a row


def _constants():
    """kThinN as csrc/mi_rowpairs1.hip states it, and the rows of a unit of work (kBlock: a lane per row)"""
    text = open(os.path.join(CSRC, "mi_rowpairs1.hip")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(CSRC, "mi_interp2_eval.hpp")).read()).group(1))
    thin = int(re.search(r"^constexpr size_t kThinN = (\d+);", text, flags=re.M).group(1))
    return thin, block


T, B = _constants()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _eq(a, b):
    """every element equal (NaN == NaN), and zeros carry the same sign"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & (a == 0), np.signbit(b) & (b == 0))


def _rows(rng, m, n):
    """(m, n) nodes and values: jittered increments, a scale and an offset per row, so that a query in range in one
    row is out of range in the next and falls into different cells of different rows"""
    X = np.cumsum(rng.uniform(0.2, 1.0, (m, n)), axis=1)
    X = X * rng.uniform(0.8, 1.2, (m, 1)) + rng.uniform(-0.1, 0.1, (m, 1)) * n
    return X, rng.standard_normal((m, n))


def _queries(rng, X, nxi, lens=None):
    """unsorted queries over the union of the rows' ranges, with points below and above every row's range, NaN, both end
    nodes of some rows and interior nodes of several"""
    m, n = X.shape
    lo, hi = X[:, 0].min(), X.max()
    q = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), nxi)
    k = max(1, nxi // 4)
    rows = rng.integers(0, m, k)
    top = (np.asarray(lens)[rows] if lens is not None else np.full(k, n)).clip(2, n)
    nodes = (rng.uniform(0, 1, k) * top).astype(np.int64)
    where = rng.permutation(nxi)
    q[where[:k]] = X[rows, nodes]
    if nxi >= 16:
        mid_top = n if lens is None else int(np.clip(lens[m // 2], 2, n))
        q[where[k]], q[where[k + 1]] = X[0, 0], X[rows[-1], top[-1] - 1]
        q[where[k + 2]], q[where[k + 3]] = X[m // 2, 0], X[m // 2, mid_top - 1]
        q[where[k + 4]], q[where[k + 5]], q[where[k + 6]] = np.nan, lo - 1.0, hi + 1.0
    return q


def _is_bad(x):
    """mi_axis1_create's rule on the valid nodes of a row"""
    return x.size < 2 or not np.all(np.isfinite(x)) or not np.all(x[:-1] < x[1:])


def _oracle(X, Y, xi, extrap=np.nan, lens=None):
    """(m, nxi) expected outputs, every row, and the (m,) expected row_ok"""
    m, n = X.shape
    want = np.full((m, xi.size), np.nan)
    ok = np.zeros(m, dtype=np.int64)
    for r in range(m):
        nr = n if lens is None else int(lens[r])
        if nr < 2 or nr > n or _is_bad(X[r, :nr]):
            continue
        ok[r] = 1
        want[r] = oracle.interp1_bracket(X[r, :nr], Y[r, :nr], xi, extrap)
    return want, ok


def _forms(ctx):
    return [int(ctx._L.mi_debug_rowpairs_launches(f)) for f in range(2)]


def _lens_t(lens):
    import torch
    return None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.int32)).cuda()


def _run(ctx, X, Y, xi, extrap=np.nan, lens=None, ldx_pad=0, ldy_pad=0, ldyi_pad=0, misalign=False, want_ok=True, form=None):
    """the device call on column-major views with padded leading dimensions: NaN in the padding rows of x and y (must not
    leak), a sentinel in the padding rows of yi and around the buffer (must survive); misalign: x, y and yi 8-B but not
    16-B aligned.  form: the one counter of mi_debug_rowpairs_launches that must move, by one (default: by n).
    Returns ((m, nxi) outputs, (m,) row_ok or None)."""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    m, n = X.shape
    nxi = xi.size
    views = []
    for A, pad in ((X, ldx_pad), (Y, ldy_pad)):
        ld = m + pad
        flat = torch.full((n * ld + 2,), np.nan, dtype=torch.float64, device="cuda")
        off = 0 if (flat.data_ptr() % 16 == 0) != misalign else 1
        h = np.full((n, ld), np.nan)
        h[:, :m] = A.T
        buf = flat[off:off + n * ld].view(n, ld)
        buf.copy_(_t(h))
        assert (buf.data_ptr() % 16 != 0) == misalign
        views.append(buf[:, :m].T)
    ldyi = m + ldyi_pad
    flat = torch.full((nxi * ldyi + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    off = 0 if (flat.data_ptr() % 16 == 0) != misalign else 1
    ob = flat[off:off + nxi * ldyi].view(nxi, ldyi)
    assert (ob.data_ptr() % 16 != 0) == misalign
    before = _forms(ctx)
    got = mi.interp_rowpairs(ctx, views[0], views[1], _t(xi), lens=_lens_t(lens), out=ob[:, :m].T, extrap=extrap, want_ok=want_ok)
    ok = None
    if want_ok:
        got, ok = got
        ok = ok.cpu().numpy()
    assert tuple(got.shape) == (m, nxi)
    h = flat.cpu().numpy()
    after = _forms(ctx)
    if form is None:
        form = 0 if n <= T else 1
    assert [a - b for a, b in zip(after, before)] == [int(f == form) for f in range(2)], (before, after, form)
    body = h[off:off + nxi * ldyi].reshape(nxi, ldyi)
    assert np.all(body[:, m:] == SENTINEL), "padding rows of YI were written"
    assert np.all(h[:off] == SENTINEL) and np.all(h[off + nxi * ldyi:] == SENTINEL), "wrote outside YI"
    return body[:, :m].T.copy(), ok


def _pairs_on_transpose(ctx, X, Y, xi, extrap=np.nan, lens=None):
    """(m, nxi) through the shipped interp_pairs: the rows as the columns of an (n, m) matrix"""
    import armadillocudalinearinterpolation_amd as mi
    return mi.interp_pairs(ctx, _t(X).T, _t(Y).T, _t(xi), lens=_lens_t(lens), extrap=extrap).T.cpu().numpy()


LAYOUTS = [(0, 0, 0, False), (1, 2, 3, False), (3, 1, 5, True)]          # (ldx_pad, ldy_pad, ldyi_pad, misalign)


@pytest.mark.parametrize("n", [7, T + 1])
@pytest.mark.parametrize("m", [1, 2, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 3])
def test_row_counts(mi_ctx, m, n):
    """row counts around a wave and around a row block, short rows (form 0) and long rows (form 1), operands dense, padded
    and padded + misaligned; against the oracle and against interp_pairs on the transpose"""
    rng = np.random.default_rng(1000 + 10 * m + n)
    X, Y = _rows(rng, m, n)
    xi = _queries(rng, X, 37)
    want, wok = _oracle(X, Y, xi, -7.25)
    assert wok.all() and np.isnan(xi).any() and (xi < X.min()).any() and (xi > X.max()).any()
    for ldx_pad, ldy_pad, ldyi_pad, misalign in LAYOUTS:
        got, ok = _run(mi_ctx, X, Y, xi, -7.25, None, ldx_pad, ldy_pad, ldyi_pad, misalign, form=0 if n <= T else 1)
        assert _eq(got, want), (m, n, ldx_pad, ldy_pad, ldyi_pad, misalign)
        assert np.array_equal(ok, wok)
    assert _eq(_pairs_on_transpose(mi_ctx, X, Y, xi, -7.25), want)


@pytest.mark.parametrize("n", [2, 3, T - 1, T, T + 1, 100, 1025])
def test_node_counts_and_the_form_switch(mi_ctx, n):
    """the short-row form up to kThinN nodes, the long-row form beyond, with and without row_ok"""
    rng = np.random.default_rng(n)
    m = 70
    X, Y = _rows(rng, m, n)
    xi = _queries(rng, X, 211)
    want, wok = _oracle(X, Y, xi, 0.5)
    form = 0 if n <= T else 1
    got, ok = _run(mi_ctx, X, Y, xi, 0.5, form=form)
    assert _eq(got, want) and np.array_equal(ok, wok)
    blind, none = _run(mi_ctx, X, Y, xi, 0.5, ldx_pad=1, misalign=True, want_ok=False, form=form)
    assert none is None and _eq(blind, want)
    assert _eq(_pairs_on_transpose(mi_ctx, X, Y, xi, 0.5), want)


@pytest.mark.parametrize("n", [64, T])
def test_lanes_of_one_wave_at_different_brackets(mi_ctx, n):
    """the hazard of the per-lane march: neighbouring lanes hold brackets far apart and advance, re-locate forward and
    re-locate backward at different queries.  Even rows have all but four nodes inside the first 1 % of the common
    range, odd rows inside the last 1 %; one row is uniform, one lies above every query, one below"""
    rng = np.random.default_rng(64 + n)
    m, nxi = 130, 500
    lo, hi = 0.0, 1000.0
    c = n - 4
    X = np.empty((m, n))
    for r in range(m):
        cluster = np.sort(rng.uniform(0.0, 10.0, c))
        cluster += np.arange(c) * 1e-9                                           # strictly increasing
        if r % 2 == 0:
            X[r] = np.concatenate([[lo - 1.0], cluster + lo, [300.0 + r, 600.0 + r, hi + 1.0]])
        else:
            X[r] = np.concatenate([[lo - 1.0, 300.0 + r, 600.0 + r], cluster + (hi - 10.0), [hi + 1.0]])
    X[126] = np.linspace(lo - 1.0, hi + 1.0, n)
    X[127] = np.linspace(2000.0, 3000.0, n)
    X[128] = np.linspace(-3000.0, -2000.0, n)
    Y = rng.standard_normal((m, n))
    base = np.sort(rng.uniform(lo, hi, nxi))
    for name, xi in (("ascending", base), ("descending", base[::-1].copy()), ("permuted", rng.permutation(base))):
        want, wok = _oracle(X, Y, xi, 2.5)
        assert wok.all() and np.all(want[127] == 2.5) and np.all(want[128] == 2.5)
        got, ok = _run(mi_ctx, X, Y, xi, 2.5)
        assert _eq(got, want), name
        assert np.array_equal(ok, wok)


def _sequences(X):
    """hand-written query sequences on rows 0 and 1 of X"""
    n = X.shape[1]
    x0, x1 = X[0], X[1]
    mid = lambda k, f=0.3: x0[k] + f * (x0[k + 1] - x0[k])  # noqa: E731
    below, above, nan = X.min() - 1.0, X.max() + 1.0, np.nan
    return {
        "repeats inside a cell": [mid(0, .1), mid(0, .5), mid(0, .5), mid(1), mid(1, .7), mid(1, .9), mid(3), mid(4), mid(4, .8)],
        "every node of row 0 exactly, in order": list(x0),
        "the last node of row 1 three times, then the cell before it": [x1[-1], x1[-1], x1[-1], x1[-2] + 0.3 * (x1[-1] - x1[-2]),
                                                                        x1[-2] + 0.9 * (x1[-1] - x1[-2])],
        "alternating first and last cell": [mid(0), mid(n - 2), mid(0, .6), mid(n - 2, .2), mid(0), mid(n - 2)],
        "flagged between two queries of the same cell": [mid(2), nan, mid(2, .6), below, mid(2, .7), above, mid(2, .1)],
        "flagged between two queries of adjacent cells": [mid(1), nan, mid(2), below, mid(3), above, mid(4)],
        "all flagged": [nan, below, above, nan],
        "a single query": [mid(3)],
        "a single flagged query": [below],
    }


@pytest.mark.parametrize("n", [6, T + 2])
@pytest.mark.parametrize("which", range(9))
def test_query_sequences(mi_ctx, which, n):
    """hand-written query sequences through every step of the march -- keep, advance by one, re-locate in front and
    behind, the last node, flagged queries in between -- on rows that are shifted copies of one jittered axis, so that
    one query falls into different cells of different rows; a row block and a bit, and five rows"""
    rng = np.random.default_rng(77)
    m = B + 1
    axis = np.cumsum(rng.uniform(0.2, 1.0, n)) - 3.0
    X = axis[None, :] + 0.29 * (np.arange(m) % 7)[:, None]
    name, xi = list(_sequences(X).items())[which]
    xi = np.array(xi)
    Y = rng.standard_normal((m, n))
    want, wok = _oracle(X, Y, xi, 3.5)
    assert wok.all()
    got, _ = _run(mi_ctx, X, Y, xi, 3.5)
    assert _eq(got, want), name
    got, _ = _run(mi_ctx, X, Y, xi, 3.5, ldx_pad=1, ldy_pad=1, ldyi_pad=3 if xi.size > 1 else 0)
    assert _eq(got, want), name
    got, _ = _run(mi_ctx, X[:5], Y[:5], xi, 3.5)
    assert _eq(got, want[:5]), name


@pytest.mark.parametrize("n", [T, 90])
def test_ragged_rows(mi_ctx, n):
    """a fill count per row in [2, n], some rows with 2 and some with n; what lies beyond a row's count -- NaN, decreasing
    values and inf in x, NaN in y -- influences nothing; row_ok is all 1"""
    rng = np.random.default_rng(n)
    m = 2 * B + 9
    X, Y = _rows(rng, m, n)
    lens = rng.integers(2, n + 1, m)
    lens[[0, 5, W, m - 1]] = 2
    lens[[1, W - 1, B, m - 2]] = n
    xi = _queries(rng, X, 300, lens)
    xi[:4] = [X[3, lens[3] - 1], X[7, lens[7] - 1], X[B + 1, 0], X[m - 1, 1]]
    for r in range(m):
        nr = lens[r]
        tail = n - nr
        if tail:
            junk = np.concatenate([[np.nan, X[r, 0] - 5.0, np.inf], X[r, nr - 1] - np.arange(1, n + 1)])[:tail]
            X[r, nr:] = junk
            Y[r, nr:] = np.nan
    want, wok = _oracle(X, Y, xi, 1.5, lens)
    assert wok.all()
    for ldx_pad, ldy_pad, ldyi_pad, misalign in LAYOUTS[::2]:
        got, ok = _run(mi_ctx, X, Y, xi, 1.5, lens, ldx_pad, ldy_pad, ldyi_pad, misalign)
        assert _eq(got, want)
        assert np.array_equal(ok, wok)
    assert _eq(_pairs_on_transpose(mi_ctx, X, Y, xi, 1.5, lens), want)


DEFECTS = ["len 0", "len 1", "len n+1", "NaN node", "+inf last", "-inf first", "equal nodes", "-0.0, 0.0", "decreasing first pair",
           "decreasing last valid pair"]


def _spoil(X, lens, r, defect):
    n = X.shape[1]
    k = n // 2
    if defect == "len 0":
        lens[r] = 0
    elif defect == "len 1":
        lens[r] = 1
    elif defect == "len n+1":
        lens[r] = n + 1
    elif defect == "NaN node":
        X[r, k] = np.nan
    elif defect == "+inf last":
        X[r, n - 1] = np.inf
    elif defect == "-inf first":
        X[r, 0] = -np.inf
    elif defect == "equal nodes":
        X[r, k] = X[r, k - 1]
    elif defect == "-0.0, 0.0":
        X[r] = X[r] - X[r, k]
        X[r, k - 1], X[r, k] = -0.0, 0.0
        X[r, :k - 1] -= 1.0
    elif defect == "decreasing first pair":
        X[r, 0], X[r, 1] = X[r, 1], X[r, 0]
    else:
        lens[r] = n - 1                                     # the last valid pair is (n-3, n-2)
        X[r, n - 3], X[r, n - 2] = X[r, n - 2], X[r, n - 3]


@pytest.mark.parametrize("n", [8, T + 8])
def test_bad_rows(mi_ctx, n):
    """every defect of the rule, in rows 0, W-1, W and m-1 (the first and last lane of a wave, the first and last row): all
    outputs of a bad row are NaN whatever the query and extrap, row_ok tells, and every good row equals the run on a
    matrix that never held a defect; a decreasing pair beyond n_r is not a defect.  With and without row_ok."""
    rng = np.random.default_rng(n)
    m = 2 * W + 5
    clean, Y = _rows(rng, m, n)
    xi = _queries(rng, clean, 64)
    clean_lens = np.full(m, n)
    clean_lens[9] = n - 3
    clean[9, n - 2], clean[9, n - 1] = clean[9, n - 1], clean[9, n - 2]          # beyond n_r: not bad
    base, bok = _run(mi_ctx, clean, Y, xi, 2.5, clean_lens)
    assert bok.all()
    assert _eq(base, _oracle(clean, Y, xi, 2.5, clean_lens)[0])
    bad = [0, W - 1, W, m - 1]
    good = [r for r in range(m) if r not in bad]
    for defect in DEFECTS:
        X, lens = clean.copy(), clean_lens.copy()
        for r in bad:
            _spoil(X, lens, r, defect)
        want, wok = _oracle(X, Y, xi, 2.5, lens)
        assert sorted(np.nonzero(wok == 0)[0].tolist()) == bad, defect
        for ldx_pad, misalign in ((0, False), (3, True)):
            got, ok = _run(mi_ctx, X, Y, xi, 2.5, lens, ldx_pad=ldx_pad, misalign=misalign)
            assert np.array_equal(ok, wok), (defect, np.nonzero(ok != wok)[0][:8])
            assert np.isnan(got[bad]).all(), defect
            assert _eq(got, want), defect
            assert _eq(got[good], base[good]), defect
        blind, none = _run(mi_ctx, X, Y, xi, 2.5, lens, want_ok=False)
        assert none is None and _eq(blind, want), defect


def test_workspace_flags_back_to_back_with_the_other_slot_3_calls(mi_ctx):
    """the long-row form without row_ok keeps its flags in context scratch slot 3, as the shared-axis calls keep their
    records and the long-column paired call its flags: interleaved on one context and stream, in both orders, without a
    synchronisation, each gives its own result"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(34)
    m, n, nxi = 300, T + 18, 900
    X, Y = _rows(rng, m, n)
    X[3, 10] = X[3, 9]
    X[B + 1, n - 1] = np.nan
    xi = _queries(rng, X[[0, 1, 2]], nxi)
    shared = X[0].copy()
    axis = mi.Axis1.from_nodes(mi_ctx, shared)
    np_, Bp = 4096 + 904, 12                                             # a long-column interp_pairs: its direct form
    Xp = np.cumsum(rng.uniform(0.2, 1.0, (Bp, np_)), axis=1)
    Yp = rng.standard_normal((Bp, np_))
    Xp[5, 100] = Xp[5, 99]
    xip = rng.uniform(0.0, Xp.max(), 500)
    xd, yd, qd = _t(X.T), _t(Y.T), _t(xi)                                # (n, m) buffers: .T is the rows layout
    xpd, ypd, qpd, ycd = _t(Xp), _t(Yp), _t(xip), _t(Y)
    torch.cuda.synchronize()
    r1 = mi.interp_rowpairs(mi_ctx, xd.T, yd.T, qd)
    a1 = axis.interp_rows(yd.T, qd)
    r2 = mi.interp_rowpairs(mi_ctx, xd.T, yd.T, qd)
    p1 = mi.interp_pairs(mi_ctx, xpd.T, ypd.T, qpd)
    r3 = mi.interp_rowpairs(mi_ctx, xd.T, yd.T, qd)
    c1 = axis.interp_cols(ycd.T, qd)                                     # the same values as an (n, m) matrix of columns
    r4 = mi.interp_rowpairs(mi_ctx, xd.T, yd.T, qd)
    p2 = mi.interp_pairs(mi_ctx, xpd.T, ypd.T, qpd)
    a2 = axis.interp_rows(yd.T, qd)
    torch.cuda.synchronize()
    want, wok = _oracle(X, Y, xi)
    assert not wok[3] and not wok[B + 1] and wok.sum() == m - 2
    for r in (r1, r2, r3, r4):
        assert _eq(r.cpu().numpy(), want)
    aref = np.stack([oracle.interp1_bracket(shared, Y[r], xi) for r in range(m)])
    assert _eq(a1.cpu().numpy(), aref) and _eq(a2.cpu().numpy(), aref) and _eq(c1.T.cpu().numpy(), aref)
    pref = np.full((Bp, xip.size), np.nan)
    for c in range(Bp):
        if c != 5:
            pref[c] = oracle.interp1_bracket(Xp[c], Yp[c], xip)
    assert _eq(p1.T.cpu().numpy(), pref) and _eq(p2.T.cpu().numpy(), pref)
    axis.close()


@pytest.mark.parametrize("m", [W + 3, 3])
def test_non_finite_values_stay_inside_their_row(mi_ctx, m):
    """inf, -inf, NaN and -0.0 at the first, an interior and the last valid node of a few rows go through the two-term
    blend as interp1 passes them (the oracle row by row); every other row equals the run that never saw them"""
    rng = np.random.default_rng(m)
    for n in (9, T + 9):
        X, clean = _rows(rng, m, n)
        Y = clean.copy()
        k = n // 2
        rows = [0, m - 1] if m == 3 else [1, 2, m - 1, W - 1, W]
        specials = [np.inf, -np.inf, np.nan, -0.0]
        for j, r in enumerate(rows):
            Y[r, 0] = specials[j % 4]
            Y[r, k] = specials[(j + 1) % 4]
            Y[r, n - 1] = specials[(j + 2) % 4]
        Y[rows[0], k + 1] = -0.0
        Y[rows[0], k] = -0.0
        xi = _queries(rng, X, 200)
        at = []
        for r in rows:
            x = X[r]
            at += [x[k], x[k - 1], x[k + 1], 0.5 * (x[k] + x[k + 1]), 0.5 * (x[k - 1] + x[k]), x[0], x[n - 1], x[n - 2],
                   0.5 * (x[n - 2] + x[n - 1]), np.nextafter(x[k], np.inf), np.nextafter(x[k], -np.inf), 0.5 * (x[0] + x[1])]
        xi[:len(at)] = at
        got, ok = _run(mi_ctx, X, Y, xi, 1.25)
        want, wok = _oracle(X, Y, xi, 1.25)
        assert _eq(got, want) and ok.all() and wok.all()
        assert np.isinf(got[rows]).any() and np.isnan(got[rows][:, ~np.isnan(xi)]).any() and (np.signbit(got[rows]) & (got[rows] == 0)).any()
        base, _ = _run(mi_ctx, X, clean, xi, 1.25)
        others = [r for r in range(m) if r not in rows]
        assert _eq(got[others], base[others])


@pytest.mark.parametrize("extrap", [2.5, np.inf, None])
def test_extrapolation_values(mi_ctx, extrap):
    """a finite value, inf, and the default (NaN) outside a row's own range; NaN for a NaN query whatever extrap is"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(5)
    for m, n in ((B + 1, 12), (4, T + 3)):
        X, Y = _rows(rng, m, n)
        xi = _queries(rng, X, 90)
        oor = (xi[None, :] < X[:, :1]) | (xi[None, :] > X[:, -1:])
        assert oor.any() and np.isnan(xi).any()
        if extrap is None:
            got = mi.interp_rowpairs(mi_ctx, _t(X.T).T, _t(Y.T).T, _t(xi)).cpu().numpy()
            assert np.isnan(got[oor]).all()
            assert _eq(got, _oracle(X, Y, xi)[0])
        else:
            got, _ = _run(mi_ctx, X, Y, xi, extrap)
            assert np.all(got[oor] == extrap)
            assert _eq(got, _oracle(X, Y, xi, extrap)[0])
        assert np.isnan(got[:, np.isnan(xi)]).all()


@pytest.mark.parametrize("n,nxi,m,order", [(50, 20_000, 5, "sorted"), (50, 20_000, 5, "permuted"),
                                           (50, 20_000, B + 1, "sorted"), (50, 20_000, B + 1, "permuted"),
                                           (T, 20_000, B + 1, "sorted"), (T, 20_000, B + 1, "permuted")])
def test_run_boundaries(mi_ctx, n, nxi, m, order):
    """enough queries that the call cuts several runs: every run begins with nothing held and a search of its rows, and
    the results depend on neither the cut nor the order"""
    rng = np.random.default_rng(n + nxi + m)
    X, Y = _rows(rng, m, n)
    xi = np.sort(rng.uniform(X.min() - 0.5, X.max() + 0.5, nxi))
    xi[1], xi[-2] = X[0, 0], X[0, -1]
    xi.sort()
    if order == "permuted":
        xi = rng.permutation(xi)
    got, ok = _run(mi_ctx, X, Y, xi, -1.0)
    assert _eq(got, _oracle(X, Y, xi, -1.0)[0]) and ok.all()
    assert _eq(got, _pairs_on_transpose(mi_ctx, X, Y, xi, -1.0))


@pytest.mark.parametrize("n", [19, T + 19])
def test_identical_rows_equal_the_shared_axis_call(mi_ctx, n):
    """every row of X the same axis: bit-equal to Axis1.interp_rows with that axis"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(n)
    m = B + 70
    shared = np.cumsum(rng.uniform(0.2, 1.0, n)) - 3.0
    X = np.repeat(shared[None, :], m, axis=0)
    Y = rng.standard_normal((m, n))
    xi = _queries(rng, X, 400)
    got, ok = _run(mi_ctx, X, Y, xi, 0.75)
    axis = mi.Axis1.from_nodes(mi_ctx, shared)
    rows = axis.interp_rows(_t(Y.T).T, _t(xi), extrap=0.75).cpu().numpy()
    assert _eq(got, rows) and ok.all()
    axis.close()


def test_empty_and_refused_calls(mi_ctx):
    """m == 0 or nxi == 0 is MI_OK with nothing written; MI_ERR_INVALID_ARG through the raw binding for each NULL pointer,
    each pointer off by 4 bytes, ldx / ldy / ldyi < m, n < 2 and sizes whose byte counts overflow -- nothing launched,
    nothing written; the Python layer's own rules raise ValueError"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, ch = mi_ctx._L, mi_ctx._h
    n, m, nxi = 5, 300, 30
    x = (torch.arange(n, dtype=torch.float64, device="cuda")[:, None] + torch.zeros((n, m), dtype=torch.float64, device="cuda")).contiguous()
    x = torch.cat([x.reshape(-1), torch.zeros(1, dtype=torch.float64, device="cuda")])
    y = torch.zeros(m * n + 1, dtype=torch.float64, device="cuda")
    xi = torch.full((nxi + 1,), 0.5, dtype=torch.float64, device="cuda")
    yi = torch.full((m * nxi + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    lens = torch.full((m + 1,), n, dtype=torch.int32, device="cuda")
    okb = torch.full((m + 1,), 7, dtype=torch.int32, device="cuda")
    p = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)  # noqa: E731

    def call(ctx=ch, xp=p(x), ldx=m, yp=p(y), ldy=m, rows=m, nodes=n, lp=p(lens), qp=p(xi), q=nxi, op=p(yi), ldyi=m, kp=p(okb)):
        return L.mi_interp1_rowpairs_f64_dev(ctx, xp, ldx, yp, ldy, rows, nodes, lp, qp, q, op, ldyi, 0.0, kp)

    def err():
        return (L.mi_last_error(ch) or b"").decode()

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((yi[:m * nxi] == 0.0).all()) and float(yi[m * nxi]) == SENTINEL
    assert bool((okb[:m] == 1).all()) and int(okb[m]) == 7
    yi.fill_(SENTINEL)
    okb.fill_(7)
    before = _forms(mi_ctx)
    assert call(rows=0) == 0 and call(q=0) == 0
    assert call(rows=0, xp=None, yp=None, op=None, lp=None, kp=None) == 0 and call(q=0, qp=None, op=None) == 0
    INVALID = 1
    for kw, word in [(dict(xp=None), "NULL"), (dict(yp=None), "NULL"), (dict(qp=None), "NULL"), (dict(op=None), "NULL"),
                     (dict(xp=p(x, 4)), "8-byte aligned"), (dict(yp=p(y, 4)), "8-byte aligned"), (dict(qp=p(xi, 4)), "8-byte aligned"),
                     (dict(op=p(yi, 4)), "8-byte aligned"), (dict(lp=p(lens, 2)), "4-byte aligned"), (dict(kp=p(okb, 2)), "4-byte aligned"),
                     (dict(ldx=m - 1), "ldx"), (dict(ldy=m - 1), "ldy"), (dict(ldyi=m - 1), "ldyi"),
                     (dict(nodes=1), "at least two nodes"), (dict(nodes=2 ** 31), "2^31"),
                     (dict(rows=2 ** 62, ldx=2 ** 62, ldy=2 ** 62, ldyi=2 ** 62), "too large"),
                     (dict(ldx=2 ** 62), "too large"), (dict(ldy=2 ** 62), "too large"), (dict(ldyi=2 ** 62), "too large"),
                     (dict(q=2 ** 62), "too large")]:
        assert call(**kw) == INVALID, kw
        assert word in err() and "mi_interp1_rowpairs_f64_dev" in err(), (kw, err())
    assert call(ctx=None) == INVALID
    assert _forms(mi_ctx) == before, "an empty or refused call launched a kernel"
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()) and bool((okb == 7).all()), "an empty or refused call wrote something"
    # 8-B aligned pointers that are not 16-B aligned, and no len / row_ok, are fine
    assert call(xp=p(x, 8), yp=p(y, 8), qp=p(xi, 8), op=p(yi, 8), lp=None, kp=None) == 0
    torch.cuda.synchronize()
    X, Y, q = x[:m * n].view(n, m).T, y[:m * n].view(n, m).T, xi[:nxi]
    z = lambda *s, **k: torch.zeros(s, dtype=k.get("dtype", torch.float64), device="cuda")  # noqa: E731
    for kw in (dict(X=z(m, n)),                                          # C-ordered (m, n)
               dict(Y=z(n + 1, m).T),                                    # mismatched shapes
               dict(lens=z(m - 1, dtype=torch.int32)),                   # a count too few
               dict(lens=z(m, dtype=torch.int64)),                       # the wrong dtype
               dict(out=z(nxi, m + 1).T),                                # the wrong rows
               dict(xi=z(nxi, dtype=torch.float32))):
        args = dict(X=X, Y=Y, xi=q)
        args.update(kw)
        with pytest.raises(ValueError):
            mi.interp_rowpairs(mi_ctx, args.pop("X"), args.pop("Y"), args.pop("xi"), **args)
    assert _forms(mi_ctx)[0] == before[0] + 1


@pytest.mark.parametrize("n,with_ok", [(7, False), (T + 4, True), (T + 4, False)])
def test_hipgraph_capture(mi_ctx, n, with_ok):
    """the short-row form is one kernel and never allocates; the long-row form is two kernels and allocates nothing with
    row_ok, or once its flag workspace has grown (a warm call).  Captured on a side stream, replayed twice with new X and
    Y in the same buffers -- the second replay holds a bad row -- and equal to the oracle each time"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(8 + n)
    m, nxi = B + 2, 700
    X, Y = _rows(rng, m, n)
    xi = _queries(rng, X, nxi)
    xd, yd, qd = _t(X.T), _t(Y.T), _t(xi)
    out = torch.full((nxi, m), SENTINEL, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mi_ctx.use_torch_stream()
        mi.interp_rowpairs(mi_ctx, xd.T, yd.T, qd, out=out.T, want_ok=with_ok)          # warm call: grows the workspace
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mi_ctx.use_torch_stream()
            res = mi.interp_rowpairs(mi_ctx, xd.T, yd.T, qd, out=out.T, want_ok=with_ok)
    torch.cuda.current_stream().wait_stream(side)
    mi_ctx.use_torch_stream()
    for rep in range(2):
        X, Y = _rows(rng, m, n)
        if rep == 1:
            X[W, n - 2] = np.nan
        xd.copy_(_t(X.T))
        yd.copy_(_t(Y.T))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want, wok = _oracle(X, Y, xi)
        assert wok.sum() == m - rep
        assert _eq(out.cpu().numpy().T, want)
        if with_ok:
            assert np.array_equal(res[1].cpu().numpy(), wok)


def test_a_small_ensemble(mi_ctx):
    """5000 trajectories with 150 to 300 jittered event times each, resampled onto 700 sorted mesh points: every row
    against the oracle"""
    rng = np.random.default_rng(2024)
    m, n, nxi = 5000, 300, 700
    X = np.cumsum(rng.uniform(0.2, 1.0, (m, n)), axis=1)
    Y = rng.standard_normal((m, n))
    lens = rng.integers(150, n + 1, m)
    xi = np.sort(rng.uniform(0.0, 0.6 * n, nxi))
    got, ok = _run(mi_ctx, X, Y, xi, lens=lens, ldx_pad=3, ldyi_pad=1)
    want, wok = _oracle(X, Y, xi, lens=lens)
    assert wok.all() and np.array_equal(ok, wok)
    assert _eq(got, want)
    assert np.isfinite(got).any() and np.isnan(got).any()
