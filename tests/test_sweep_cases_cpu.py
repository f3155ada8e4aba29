"""CPU checks of the cases tests/test_sweep_edges_gpu.py runs the region-sweep kernels on (tests/sweep_cases.py): the
reference those kernels are held to is itself held to two independent ones here, and the query vector is what its
description says.  No GPU.

Bound of test_oracle_is_within_the_derived_bound_of_the_exact_interpolant.  With u = 2^-53 and every operation of
    a = q - X[l];  b = X[r] - q;  w = a / (a + b);  out = (1 - w) * Y[l] + w * Y[r]
rounded once (oracle/Makefile: -ffp-contract=off), to first order in u:
    w^ = w (1 + d1 - (a d1 + b d2)/(a + b) - d3 + d4)        four roundings in the weight: |w^ - w| <= 4 u w
    c^ = (1 - w^)(1 + d5)                                     one in 1 - w:  |c^ - (1 - w)| <= 4 u w + u (1 - w)
    out^ = (c^ Y[l] (1 + d6) + w^ Y[r] (1 + d7)) (1 + d8)     three in the products and the sum
    |out^ - out| <= u [ |Y[l]| (4 w + 3 (1 - w)) + |Y[r]| 6 w ] <= u (4 |Y[l]| + 6 |Y[r]|) <= 6 u (|Y[l]| + |Y[r]|)
for 0 <= w <= 1.  The bound asserted is 8 u (|Y[l]| + |Y[r]|): the first-order figure with room for the second-order
terms (below 64 u^2) and nothing else.  Measured worst distance in those units, 3000 seeded in-range queries per table:
cf_fma 0.81, cf_mul 0.98, cf_mul_pinned 0.95, cf_fma_pinned 0.92, cf_div 1.06, jitter 0.93, walk 0.93, clustered 0.99."""
import numpy as np
import pytest

import oracle
import sweep_cases as sc

C = sc.CPU_C
STRETCH_HEAD = 40 * sc.TILE          # all 13 patterns lie in the first 40 tiles
STRETCH_TAIL = 20_000                # the last tile's end and the ragged tail


@pytest.fixture(scope="module", params=sc.TABLES)
def case(request):
    """one table, its full query vector for C = 256, and the reference on all of it"""
    tab = sc.table(request.param)
    xq = sc.query_vector(request.param, C)
    ref = oracle.interp1_bracket(tab["X"], tab["Y"], xq, nthreads=min(8, oracle.max_threads()))
    return tab, xq, ref


def test_vector_layout():
    sizes = sc.prefix_sizes(C)
    assert [s[:2] for s in sizes] == [(T, tail) for T in (1, 2, 257, 513, 770) for tail in (0, 4099)]
    assert sizes[-1][2] == 770 * sc.TILE + 4099 == sc.pattern_index(C).size
    # every pattern at both parities of a workgroup's local tile index (tile t: workgroup t % C, local index t // C)
    seen = {(sc.pattern_of_tile(t, C), (t // C) & 1) for t in range(sc.full_tiles(C))}
    assert seen == {(p, par) for p in range(sc.NPATTERNS) for par in (0, 1)}
    # consecutive tiles of one workgroup differ
    assert all(sc.pattern_of_tile(t, C) != sc.pattern_of_tile(t + C, C) for t in range(sc.full_tiles(C) - C))
    assert set(sc.pattern_index(C)[:STRETCH_HEAD].tolist()) == set(range(sc.NPATTERNS))


def test_tables_are_what_the_cases_assume():
    for name in sc.TABLES:
        X = sc.table(name)["X"]
        assert X.size == (49_997 if name == "clustered" else sc.N_NODES) and np.all(np.diff(X) > 0), name
        assert 16 * (X.size + 1) > 8 * (X.size + 1) > 128 * 1024              # beyond the LDS window in both layouts
    assert np.array_equal(sc.table("cf_mul_pinned")["X"][:-1], sc.table("cf_mul")["X"][:-1])
    assert sc.table("cf_mul_pinned")["X"][-1] == np.nextafter(sc.table("cf_mul")["X"][-1], np.inf)
    assert sc.table("cf_fma_pinned")["X"][-1] == np.nextafter(sc.table("cf_fma")["X"][-1], np.inf)
    assert float(np.min(np.diff(sc.table("clustered")["X"]))) == float(np.spacing(1e3))   # neighbours one ulp apart
    zero_in_range = [n for n in sc.TABLES if sc.table(n)["X"][0] <= 0.0 <= sc.table(n)["X"][-1]]
    assert "cf_fma" in zero_in_range and "jitter" in zero_in_range


def test_patterns_are_what_they_say(case):
    tab, xq, _ = case
    X = tab["X"]
    pat = sc.pattern_index(C)
    reg, inr, nan = sc.region(xq, X), sc.in_range(xq, X), np.isnan(xq)
    first = {p: next(t for t in range(sc.full_tiles(C)) if sc.pattern_of_tile(t, C) == p) for p in range(sc.NPATTERNS)}
    tile = lambda a, p: a[first[p] * sc.TILE:(first[p] + 1) * sc.TILE]       # noqa: E731
    assert np.unique(tile(xq, 1)).size == 1 and tile(inr, 1).all()
    assert np.unique(reg[pat == 1].reshape(-1, sc.TILE), axis=1).shape[1] == 1   # a whole tile in one region
    assert (reg[pat == 2] == 0).all() and inr[pat == 2].all()
    assert (reg[pat == 3] == sc.BINS - 1).all() and inr[pat == 3].all() and (tile(xq, 3)[::7] == X[-1]).all()
    assert nan[pat == 4].all()
    assert (xq[pat == 5] < X[0]).all() and (reg[pat == 5] == 0).all()
    assert {-np.inf, float(np.nextafter(X[0], -np.inf))} <= set(tile(xq, 5).tolist())
    assert (xq[pat == 6] > X[-1]).all() and (reg[pat == 6] == sc.BINS - 1).all()
    assert {np.inf, 1e300, float(np.nextafter(X[-1], np.inf))} <= set(tile(xq, 6).tolist())
    s = (first[7] * 4096) % (X.size - 4097)
    q7 = set(tile(xq, 7).tolist())
    assert all({float(X[i]), float(np.nextafter(X[i], -np.inf)), float(np.nextafter(X[i], np.inf)),
                float(0.5 * (X[i] + X[i + 1]))} <= q7 for i in (s, s + 1, s + 4095))
    # (a boundary and both its neighbours may round into the region below: most regions, not necessarily all 256)
    assert len(set(tile(reg, 8).tolist())) >= sc.BINS - 32 and X[-1] in tile(xq, 8) and X[0] in tile(xq, 8)
    r9 = tile(reg, 9).reshape(-1, 2)
    assert set(r9[0::2].ravel().tolist()) == {0} and set(r9[1::2].ravel().tolist()) == {sc.BINS - 1} and inr[pat == 9].all()
    assert (np.diff(tile(xq, 10)) <= 0).all() and (np.diff(tile(xq, 11)) >= 0).all()
    assert inr[pat == 10].all() and inr[pat == 11].all() and len(set(tile(reg, 10).tolist())) == sc.BINS
    t12 = tile(xq, 12)
    assert np.isnan(t12).sum() == sc.TILE // 4 and (~tile(inr, 12) & ~np.isnan(t12)).sum() >= sc.TILE // 4
    assert (t12 == X[0]).sum() >= 32 and (t12 == X[-1]).sum() >= 32
    if X[0] <= 0.0 <= X[-1]:
        assert (np.signbit(t12) & (t12 == 0.0)).sum() == 32 and (t12 == 5e-324).sum() == 32
    # the tail is pattern 7 of the tile that would follow
    assert inr[-sc.TAIL:].mean() > 0.99
    frac = inr.mean()
    print("%s: in range %.1f %%, NaN %.1f %%, out of range %.1f %%" % (tab["name"], 100 * frac, 100 * nan.mean(),
                                                                       100 * (1 - frac - nan.mean())))
    assert frac >= 0.70


def test_bracket_oracle_equals_the_literal_armadillo_scan(case):
    tab, xq, ref = case
    for sl in (slice(0, STRETCH_HEAD), slice(xq.size - STRETCH_TAIL, xq.size)):
        scan = oracle.interp1_arma(tab["X"], tab["Y"], xq[sl])
        assert sc.same_bits(ref[sl], scan), tab["name"]


def test_extrapolation_value_only_replaces_out_of_range_results(case):
    """sc.with_extrap (what the GPU file derives its references for the other extrapolation values with) is the oracle's
    own answer, bit for bit, the sign of -0.0 included"""
    tab, xq, ref = case
    sl = slice(0, STRETCH_HEAD)
    for e in (-3.25, -0.0, np.inf):
        want = oracle.interp1_bracket(tab["X"], tab["Y"], xq[sl], extrap=e)
        assert sc.same_bits(sc.with_extrap(ref[sl], xq[sl], tab["X"], e), want), (tab["name"], e)
        assert not sc.same_bits(ref[sl], want)


def test_oracle_is_within_the_derived_bound_of_the_exact_interpolant(case):
    """|oracle - exact rational interpolant| <= 8 * 2^-53 * (|Y[l]| + |Y[r]|) (module docstring) on 3000 seeded in-range
    queries of the vector, the ulp neighbours of nodes and region boundaries among them"""
    tab, xq, ref = case
    X, Y = tab["X"], tab["Y"]
    idx = np.flatnonzero(sc.in_range(xq, X))
    pick = np.random.default_rng([0xE8AC, sc.TABLES.index(tab["name"])]).choice(idx, 3000, replace=False)
    worst = max(sc.blend_error_units(X, Y, xq[k], ref[k]) for k in pick)
    print("%s: worst |oracle - exact| = %.3f x 2^-53 (|Y[l]| + |Y[r]|)" % (tab["name"], worst))
    assert worst <= sc.BLEND_BOUND_UNITS
