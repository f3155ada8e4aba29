"""References and shared query sets for arma::interp1's "nearest" method (include/mi355_interp.h, "nearest rule").

Plain numpy: no torch, no GPU, no oracle.

nearest_rule        the rule as the header states it, vectorised with searchsorted: the linear bracket l, r = min(l+1, n-1),
                    a = q - X[l], b = X[r] - q (one rounded subtraction each), k = r if b < a else l, out = Y[k] copied.
arma_nearest_scan   Armadillo's interp1_helper_nearest restated literally: the queries are sorted (stably), every query
                    scans the nodes from the previous query's optimum and stops at the first j whose error
                    |X[j] - q| is not smaller than the best so far (err >= best_err), and the results are put back
                    into the caller's order.  NaN queries (which the stable sort puts last) give NaN, as for every
                    entry point of this library; Armadillo does not define them.
tests/test_interp1_nearest_cpu.py holds the two to each other on every element; tests/test_interp1_nearest_gpu.py holds
every kernel to nearest_rule, bit for bit."""
import functools

import numpy as np

import sweep_cases as sc


def _eq_bits(a, b):
    """the same 64 bits wherever neither side is NaN (the sign of zero included), and NaN in the same positions"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def rule_index(X, xq):
    """int64[nq]: the node the rule picks; -1 out of range, -2 NaN"""
    X = np.asarray(X, dtype=np.float64)
    xq = np.asarray(xq, dtype=np.float64)
    n = X.size
    k = np.full(xq.shape, -1, dtype=np.int64)
    k[np.isnan(xq)] = -2
    inr = sc.in_range(xq, X)
    q = xq[inr]
    l = np.searchsorted(X, q, side="right") - 1          # largest l with X[l] <= q
    r = np.minimum(l + 1, n - 1)
    a = q - X[l]
    b = X[r] - q
    k[inr] = np.where(b < a, r, l)                       # a tie keeps the left node
    return k


def _gather(Y, k, extrap):
    Y = np.asarray(Y, dtype=np.float64)
    out = np.full(k.shape, float(extrap), dtype=np.float64)
    out[k == -2] = np.nan
    out[k >= 0] = Y[k[k >= 0]]                            # a copy: the stored bits
    return out


def nearest_rule(X, Y, xq, extrap=np.nan):
    return _gather(Y, rule_index(X, xq), extrap)


def scan_index(X, xq):
    """int64[nq]: the node Armadillo's scan stops at; -1 out of range, -2 NaN.  A plain Python loop (the scan carries
    its position from query to query), about a microsecond per query and node."""
    X = np.asarray(X, dtype=np.float64)
    xq = np.asarray(xq, dtype=np.float64)
    order = np.argsort(xq, kind="stable")                # NaN last
    xs = X.tolist()
    qs = xq[order].tolist()
    ng = len(xs)
    xmin, xmax = xs[0], xs[-1]
    inf = float("inf")
    res = [0] * len(qs)
    best_j = 0
    for i, q in enumerate(qs):
        if q != q:
            res[i] = -2
            continue
        if q < xmin or q > xmax:
            res[i] = -1
            continue
        best_err = inf
        j = best_j                                       # start from the last known optimum
        while j < ng:
            tmp = xs[j] - q
            err = tmp if tmp >= 0.0 else -tmp
            if err >= best_err:                          # the error is going up: the optimum is behind us
                break
            best_err = err
            best_j = j
            j += 1
        res[i] = best_j
    k = np.empty(xq.size, dtype=np.int64)
    k[order] = np.array(res, dtype=np.int64)
    return k.reshape(xq.shape)


def arma_nearest_scan(X, Y, xq, extrap=np.nan):
    return _gather(Y, scan_index(X, xq), extrap)


N_SWEEP_QUERIES = 33_007


@functools.lru_cache(maxsize=None)
def sweep_queries(name, n=sc.N_NODES):
    """the seeded query set over sweep_cases table `name`: 3000 random nodes and their ulp neighbours, the midpoints of
    the cells to their right and those midpoints' ulp neighbours, X[0], X[-1], NaN, +-inf, one point out of range on each
    side, and 15 000 uniform fill queries over the range widened by 1 % each side; permuted"""
    X = sc.table(name, n)["X"] if n == sc.N_NODES else sc.make_nodes(name, n)
    m = X.size
    rng = np.random.default_rng([0x4EA2, sc.TABLES.index(name), n])
    j = rng.integers(0, m, 3000)
    jr = np.minimum(j + 1, m - 1)
    nodes = X[j]
    mid = 0.5 * X[j] + 0.5 * X[jr]
    span = X[-1] - X[0]
    fill = (X[0] - 0.01 * span) + 1.02 * span * rng.random(15_000)
    xq = np.concatenate([nodes, np.nextafter(nodes, -np.inf), np.nextafter(nodes, np.inf),
                         mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf),
                         [X[0], X[-1], np.nan, np.inf, -np.inf, X[0] - 0.5 * span, X[-1] + 0.5 * span], fill])
    xq = rng.permutation(xq)
    assert xq.size == N_SWEEP_QUERIES
    xq.setflags(write=False)
    return xq
