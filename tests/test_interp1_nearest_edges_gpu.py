"""The whole-table-in-LDS form of mi_interp1_nearest_f64_dev (nearest1_lds_kernel) at the edges of its window and of its
query count -- what needs 2^20 queries and so cannot live in the seeded fuzz (tests/nearest_fuzz_cases.py, capped at 2^18).

The form is taken for unordered (or AUTO) queries, nq >= 2^20, and a table of n + 1 entries above the lower and up to the
upper limit: closed-form tables (8 B per entry, Y only) for 4096 <= n <= 16383, centred {x,y} tables (16 B) for
128 <= n <= 8191.  Every result is held to nearest_cases.nearest_rule on every element with nearest_cases._eq_bits,
between sentinels, with the form proved by mi_debug_nearest_launches: test_interp1_nearest_gpu._nearest, as it is.

Tables: sweep_cases.make_nodes(kind, n), Y = make_values with interp1_value_cases.special_values written over it (the last
node NaN or -0.0: the padding node behind the table copies it, and a pinned last abscissa comes from the closed form while
its Y comes from LDS).  cf_mul_pinned keeps its closed form only where the pinned span divided by n - 1 still rounds to
the step: 5464 and 13654 are the sizes nearest to the window's ends that do.
Queries: nearest_cases.sweep_queries (nodes, their ulp neighbours, cell midpoints and theirs, both ends, NaN, +-inf, out
of range) filled up with seeded uniform queries over the range widened by 1 % each side, and permuted."""
import functools

import numpy as np
import pytest

import interp1_value_cases as vc
import nearest_cases as nc
import sweep_cases as sc
from test_interp1_nearest_gpu import LDS, STREAM, _nearest

pytestmark = pytest.mark.gpu

NQ_MIN = 1 << 20                  # 8 * kLdsQueriesPerBlock: fewer queries stream
LDS_CHUNK = 1 << 17               # kLdsQueriesPerBlock: queries of one workgroup
UNIFORM = (-1.0, 2.0 ** -7)       # Grid1.uniform with cf_fma's origin and step
# (kind, n) inside the window; "uniform" is the implicit table over cf_fma's nodes
IN_WINDOW = [(kind, n) for kind in ("cf_fma", "cf_mul", "cf_fma_pinned", "cf_div", "uniform") for n in (4096, 16383)] + [
    ("cf_mul_pinned", 5464), ("cf_mul_pinned", 13654), ("jitter", 128), ("jitter", 8191)]
# (kind, n) one step outside it: the streaming form whatever the hint
OUTSIDE = [("cf_div", 4095), ("cf_div", 16384), ("jitter", 127), ("jitter", 8192)]
NQ_EDGE_TABLES = [("cf_div", 16383), ("jitter", 8191)]
PREFIXES = [(NQ_MIN - 1, STREAM), (NQ_MIN, LDS), (NQ_MIN + 1, LDS), (NQ_MIN + 2, LDS), (NQ_MIN + 3, LDS)]


def _family(kind):
    return "cf_fma" if kind == "uniform" else kind


def _table(ctx, kind, n, variant):
    """(grid, X, Y), the reported (mode, formula, pin_last) asserted against sweep_cases.TABLE_SPECS"""
    import armadillocudalinearinterpolation_amd as mi
    X = sc.make_nodes(_family(kind), n)
    Y = sc.make_values(X).copy()
    for k, v in vc.special_values(n, variant).items():
        Y[k] = v
    if kind == "uniform":
        assert np.array_equal(X, UNIFORM[0] + UNIFORM[1] * np.arange(n))
        grid = mi.Grid1.uniform(ctx, UNIFORM[0], UNIFORM[1], Y)
    else:
        grid = mi.Grid1.from_nodes(ctx, X, Y, sanitise=False)
    info = grid.info()
    want = tuple(-1 if v is None else v for v in sc.TABLE_SPECS[_family(kind)])
    assert (info["mode"], info["formula"], info["pin_last"]) == want, (kind, n, info)
    assert info["n_nodes"] == n
    return grid, X, Y


def _queries(kind, n, nq, seed):
    X = sc.make_nodes(_family(kind), n)
    head = nc.sweep_queries(_family(kind), n)
    rng = np.random.default_rng([0xED6E, seed, n])
    span = X[-1] - X[0]
    fill = (X[0] - 0.01 * span) + 1.02 * span * rng.random(nq - head.size)
    return rng.permutation(np.concatenate([head, fill]))


@pytest.mark.parametrize("kind,n", IN_WINDOW, ids=["%s-%d" % kn for kn in IN_WINDOW])
def test_in_window_tables_take_the_lds_form(mi_ctx, kind, n):
    """unordered hint: the LDS form, in every closed form, pinned or not, implicit, and {x,y}, at both ends of the window;
    ordered hint: the streaming form on the same queries, the same bits"""
    variant = vc.VARIANTS[(IN_WINDOW.index((kind, n))) % 2]
    grid, X, Y = _table(mi_ctx, kind, n, variant)
    xq = _queries(kind, n, NQ_MIN, IN_WINDOW.index((kind, n)))
    ref = nc.nearest_rule(X, Y, xq, -0.0)
    try:
        mi_ctx.set_query_order(1)
        lds = _nearest(mi_ctx, grid, xq, -0.0, LDS)
        mi_ctx.set_query_order(2)
        stream = _nearest(mi_ctx, grid, xq, -0.0, STREAM)
    finally:
        mi_ctx.set_query_order(0)
        grid.close()
    assert nc._eq_bits(lds, ref), (kind, n, "lds")
    assert nc._eq_bits(stream, ref), (kind, n, "stream")
    # the reference holds what the table was given: the specials, the last node's among them, and extrap's sign
    assert np.isinf(ref).any() and np.isnan(ref[~np.isnan(xq)]).any() and (np.signbit(ref) & (ref == 0)).any()
    assert nc._eq_bits(ref[xq == X[-1]], np.full(int((xq == X[-1]).sum()), Y[-1])) and (xq == X[-1]).any()


@pytest.mark.parametrize("kind,n", OUTSIDE, ids=["%s-%d" % kn for kn in OUTSIDE])
def test_one_step_outside_the_window_streams(mi_ctx, kind, n):
    """n + 1 entries of exactly the lower limit, and one entry beyond the upper limit, under the unordered hint"""
    grid, X, Y = _table(mi_ctx, kind, n, vc.VARIANTS[OUTSIDE.index((kind, n)) % 2])
    xq = _queries(kind, n, NQ_MIN, 100 + OUTSIDE.index((kind, n)))
    try:
        mi_ctx.set_query_order(1)
        got = _nearest(mi_ctx, grid, xq, np.inf, STREAM)
    finally:
        mi_ctx.set_query_order(0)
        grid.close()
    assert nc._eq_bits(got, nc.nearest_rule(X, Y, xq, np.inf)), (kind, n)


@functools.lru_cache(maxsize=None)
def _edge_vector(kind, n):
    """(2^20 + 3 queries, their reference, X, Y): the last 70 places cycle through the last node, the last cell's midpoint
    and its ulp neighbours, NaN and a point out of range on each side, so that every prefix ends in another of them"""
    X = sc.make_nodes(kind, n)
    Y = sc.make_values(X).copy()
    for k, v in vc.special_values(n, "negzero_last").items():
        Y[k] = v
    xq = _queries(kind, n, NQ_MIN + 3, 200 + n)
    mid = 0.5 * X[-2] + 0.5 * X[-1]
    span = X[-1] - X[0]
    ends = [X[-1], mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf), np.nan, X[-1] + 0.5 * span, X[0] - 0.5 * span]
    for p in range(xq.size - 70, xq.size):
        xq[p] = ends[p % len(ends)]
    ref = nc.nearest_rule(X, Y, xq, 2.5)
    xq.setflags(write=False)
    ref.setflags(write=False)
    return xq, ref, X, Y


@pytest.mark.parametrize("nq,form", PREFIXES, ids=["nq-2^20%+d" % (nq - NQ_MIN) for nq, _ in PREFIXES])
@pytest.mark.parametrize("kind,n", NQ_EDGE_TABLES, ids=["%s-%d" % kn for kn in NQ_EDGE_TABLES])
def test_query_counts_around_the_threshold(mi_ctx, kind, n, nq, form):
    """prefixes of one query vector under the unordered hint: 2^20 - 1 streams; 2^20 has eight full workgroups and no
    tail; 2^20 + 1, + 2, + 3 give the ninth workgroup one odd element, one vector, one vector and an odd element"""
    import armadillocudalinearinterpolation_amd as mi
    xq, ref, X, Y = _edge_vector(kind, n)
    assert xq.size == NQ_MIN + 3 and NQ_MIN % LDS_CHUNK == 0 and {nq - NQ_MIN for nq, _ in PREFIXES} == {-1, 0, 1, 2, 3}
    grid = mi.Grid1.from_nodes(mi_ctx, X, Y, sanitise=False)
    try:
        mi_ctx.set_query_order(1)
        got = _nearest(mi_ctx, grid, xq[:nq], 2.5, form)
    finally:
        mi_ctx.set_query_order(0)
        grid.close()
    assert nc._eq_bits(got, ref[:nq]), (kind, n, nq)
    tail = xq[nq - 7:nq]                                         # the last seven queries of this prefix: all of `ends`
    assert np.isnan(tail).any() and (tail == X[-1]).any() and (tail > X[-1]).any() and (tail < X[0]).any()
