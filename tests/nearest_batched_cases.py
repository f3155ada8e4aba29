"""Inputs and references shared by tests/test_nearest_batched_cpu.py and tests/test_nearest_batched_gpu.py.

Plain numpy: no torch, no GPU.  Nodes are integer steps scaled by a power of two, so that every cell midpoint, and both
differences the nearest rule takes at a midpoint, are exact: a midpoint query is an exact tie.  The reference of every
value is nearest_cases.nearest_rule, per row or per column, on every output element."""
import numpy as np

import nearest_cases as nc


def nodes(rng, n, origin=-3.0):
    """n strictly increasing nodes on the grid of 1/8"""
    return np.cumsum(rng.integers(1, 9, n)) / 8.0 + origin


def _specials(X):
    span = X[-1] - X[0]
    return np.array([X[0], X[-1], np.nan, np.inf, -np.inf, X[0] - 1.0 - span, X[-1] + 1.0 + span])


def queries(rng, X, nxi):
    """nxi permuted queries over the axis X: exact midpoints (ties), their two ulp neighbours, nodes, both end nodes, NaN,
    +-inf, one point out of range on each side, and uniform fill over the range widened by 5 % each side.  From 37
    queries on every kind is there, with at least 9 exact ties."""
    mid = 0.5 * X[:-1] + 0.5 * X[1:]
    special = _specials(X)
    if nxi < 37:
        return rng.choice(np.concatenate([mid, X, special]), nxi)
    a, b, c = max(9, nxi // 4), max(4, nxi // 10), max(5, nxi // 8)
    span = X[-1] - X[0]
    fill = rng.uniform(X[0] - 0.05 * span, X[-1] + 0.05 * span, nxi - (a + 2 * b + c + special.size))
    q = np.concatenate([rng.choice(mid, a), np.nextafter(rng.choice(mid, b), -np.inf), np.nextafter(rng.choice(mid, b), np.inf),
                        rng.choice(X, c), special, fill])
    assert q.size == nxi
    return rng.permutation(q)


def select_counts(X, xi):
    """(exact ties, queries that take the left node of a proper cell, queries that take the right one), from the inputs
    alone: the picked node is nearest_cases.rule_index's"""
    X, xi = np.asarray(X, dtype=np.float64), np.asarray(xi, dtype=np.float64)
    inr = (xi >= X[0]) & (xi <= X[-1])
    q = xi[inr]
    l = np.searchsorted(X, q, side="right") - 1
    r = np.minimum(l + 1, X.size - 1)
    k = nc.rule_index(X, xi)[inr]
    cell = r > l
    ties = int(np.count_nonzero(cell & (q - X[l] == X[r] - q)))
    return ties, int(np.count_nonzero(cell & (k == l) & (q > X[l]))), int(np.count_nonzero(cell & (k == r)))


def assert_select(tables, xi):
    """the condition on the inputs of a test that claims to exercise the select: at least 8 exact ties, and both the left
    and the right node picked.  tables: one axis, or the valid nodes of several columns (counts are summed)."""
    tables = [tables] if isinstance(tables, np.ndarray) and tables.ndim == 1 else tables
    ties = left = right = 0
    for X in tables:
        t, a, b = select_counts(X, xi)
        ties, left, right = ties + t, left + a, right + b
    assert ties >= 8 and left > 0 and right > 0, (ties, left, right)


def ref_rows(X, Y, xi, extrap=np.nan):
    """(m, nxi): row r = nearest_rule on the table (X, Y[r, :]), every row (the picked nodes depend on X and xi only)"""
    k = nc.rule_index(X, xi)
    return np.stack([nc._gather(Y[r], k, extrap) for r in range(Y.shape[0])]) if Y.shape[0] else np.empty((0, np.size(xi)))


def sequences(X):
    """the ten held-column sequences of the tile body, on an axis of at least 6 nodes"""
    n = X.size
    mid = lambda k: 0.5 * X[k] + 0.5 * X[k + 1]  # noqa: E731
    at = lambda k, f: X[k] + f * (X[k + 1] - X[k])  # noqa: E731
    below, above, nan = X[0] - 1.0, X[-1] + 1.0, np.nan
    return {
        "ascending with repeats": [at(0, .125), at(0, .25), at(0, .25), at(0, .75), at(1, .75), at(1, .875), at(3, .25), mid(4), at(4, .75)],
        "right half of a cell then left half of the next (same node, no load)": [at(1, .75), at(2, .25), at(2, .75), at(3, .25), mid(3)],
        "every node in order": list(X),
        "every midpoint in order": [mid(k) for k in range(n - 1)],
        "the last node three times": [X[-1], X[-1], X[-1], at(n - 2, .25), at(n - 2, .875)],
        "strictly descending": [X[-1]] + [at(k, .25) for k in range(n - 2, -1, -1)] + [X[0]],
        "alternating first and last node": [X[0], X[-1], at(0, .25), at(n - 2, .875), X[0], X[-1]],
        "flagged between outputs of the same node and of different nodes": [at(2, .25), nan, at(2, .125), below, mid(2), above,
                                                                            at(2, .75), nan, at(4, .25), below, at(1, .125)],
        "all flagged": [nan, below, above, nan],
        "a single query and a single flagged query": None,           # two calls: see the test
    }


# ---- paired columns ---------------------------------------------------------------------------------------------------

def pairs(rng, B, n):
    """(B, n) nodes and values.  Every column on a grid of its own -- steps of 1/8 scaled by 1/2, 1 or 2, shifted by a
    multiple of 1/16 -- so that a query in range in one column may be out of range in the next; midpoints stay exact."""
    Xb = np.cumsum(rng.integers(1, 9, (B, n)), axis=1) / 8.0
    Xb = Xb * 2.0 ** rng.integers(-1, 2, (B, 1)) + rng.integers(-32, 33, (B, 1)) / 16.0
    return Xb, rng.standard_normal((B, n))


def col_len(lens, c, n):
    return n if lens is None else int(lens[c])


def pair_queries(rng, Xb, nxi, lens=None):
    """nxi permuted queries shared by every column: midpoints, their ulp neighbours and nodes of randomly chosen columns
    (inside their valid rows), end nodes, NaN, +-inf, points outside every column, uniform fill"""
    B, n = Xb.shape
    top = np.array([min(max(col_len(lens, c, n), 2), n) for c in range(B)])

    def pick(count):
        c = rng.integers(0, B, count)
        k = (rng.random(count) * (top[c] - 1)).astype(np.int64)           # 0 .. top-2
        return c, k
    lo, hi = Xb[:, 0].min(), max(Xb[c, top[c] - 1] for c in range(B))
    special = np.array([Xb[0, 0], Xb[B - 1, top[B - 1] - 1], Xb[B // 2, 0], np.nan, np.inf, -np.inf, lo - 1.0 - (hi - lo),
                        hi + 1.0 + (hi - lo)])
    if nxi < 40:
        c, k = pick(nxi)
        q = 0.5 * Xb[c, k] + 0.5 * Xb[c, k + 1]
        q[::3] = Xb[c, k][::3]
        if nxi >= 5:
            q[rng.integers(0, nxi)] = np.nan
        return q
    a, b, d = max(10, nxi // 4), max(4, nxi // 10), max(5, nxi // 8)
    c, k = pick(a)
    mid = 0.5 * Xb[c, k] + 0.5 * Xb[c, k + 1]
    c, k = pick(2 * b)
    m2 = 0.5 * Xb[c, k] + 0.5 * Xb[c, k + 1]
    c, k = pick(d)
    fill = rng.uniform(lo - 0.02 * (hi - lo), hi + 0.02 * (hi - lo), nxi - (a + 2 * b + d + special.size))
    q = np.concatenate([mid, np.nextafter(m2[:b], -np.inf), np.nextafter(m2[b:], np.inf), Xb[c, k], special, fill])
    assert q.size == nxi
    return rng.permutation(q)


def is_bad(x):
    """mi_axis1_create's rule on the valid rows of a column"""
    return x.size < 2 or not np.all(np.isfinite(x)) or not np.all(x[:-1] < x[1:])


def ref_pairs(Xb, Yb, xi, extrap=np.nan, lens=None):
    """(B, nxi) expected outputs -- nearest_rule column by column on the valid rows, NaN for a bad column -- and the (B,)
    expected col_ok"""
    B, n = Xb.shape
    want = np.full((B, np.size(xi)), np.nan)
    ok = np.zeros(B, dtype=np.int64)
    for c in range(B):
        m = col_len(lens, c, n)
        if m < 2 or m > n or is_bad(Xb[c, :m]):
            continue
        ok[c] = 1
        want[c] = nc.nearest_rule(Xb[c, :m], Yb[c, :m], xi, extrap)
    return want, ok


def valid_tables(Xb, lens=None, limit=8):
    """the valid nodes of the first `limit` good columns, for assert_select"""
    out = []
    for c in range(Xb.shape[0]):
        m = col_len(lens, c, Xb.shape[1])
        if 2 <= m <= Xb.shape[1] and not is_bad(Xb[c, :m]):
            out.append(Xb[c, :m])
        if len(out) == limit:
            break
    return out
