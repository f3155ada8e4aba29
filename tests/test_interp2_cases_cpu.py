"""CPU checks of the cases tests/test_interp2_edges_gpu.py and tests/test_interp1_values_gpu.py run the kernels on
(tests/interp2_cases.py, tests/interp1_value_cases.py): the references those kernels are held to are themselves held to
independent ones here, and the inputs are what their descriptions say.  No GPU.

Bound of test_oracle_is_within_the_derived_bound_of_the_exact_bilinear.  With u = 2^-53, every operation of
    wy = ay / (ay + by);  c0 = (1 - wy) * z00 + wy * z01;  c1 = (1 - wy) * z10 + wy * z11
    wx = ax / (ax + bx);  out = (1 - wx) * c0 + wx * c1
rounded once (oracle/Makefile: -ffp-contract=off), and S = |z00| + |z01| + |z10| + |z11|, to first order in u:
  stage one  two 1-D blends of exact inputs.  By the derivation in tests/test_sweep_cases_cpu.py (four roundings in the
             weight, one in 1 - w, three in the products and the sum)
                 |c0^ - c0| <= u (4 |z00| + 6 |z01|) <= 6 u (|z00| + |z01|),  |c1^ - c1| <= 6 u (|z10| + |z11|)
  stage two  one more blend, of the inexact c0^, c1^.  Its own roundings give, by the same derivation,
             6 u (|c0| + |c1|) <= 6 u S, since |c0| <= max(|z00|, |z01|) and |c1| <= max(|z10|, |z11|) for 0 <= wy <= 1.
             The errors it inherits are weighted by (1 - wx) and wx, which sum to 1:
                 (1 - wx) |c0^ - c0| + wx |c1^ - c1| <= 6 u max(|z00| + |z01|, |z10| + |z11|) <= 6 u S
    |out^ - out| <= 12 u S
The bound asserted is 16 u S: the first-order figure with the same room for second-order terms that the 1-D bound has
(8 for 6), and nothing else.  Underflow (weights down to 5e-324 on the span_overflow table, products of 1e-150-sized
values with small weights) adds a few 2^-1075 per operation, nothing against u S >= 1e-170 on these tables.
Measured worst distance in those units (3000 seeded in-range queries and every node pair per table):
t2x2 0.97, t2rows 1.36, t2cols 1.94, guess_bsearch 1.38, uniform 1.77, huge_tiny 1.96, span_overflow 1.95."""
from fractions import Fraction

import numpy as np
import pytest

import interp1_value_cases as vc
import interp2_cases as ic
import oracle
import sweep_cases as sc

EXTRAPS = (-3.25, -0.0, np.inf)


@pytest.fixture(scope="module", params=ic.TABLES)
def case(request):
    """one table, its full scattered vector, and the reference (extrap = NaN) on all of it"""
    t = ic.table(request.param)
    xq, yq = ic.scattered(request.param)
    return t, xq, yq, ic.reference(request.param, xq, yq)


def test_tables_are_what_the_cases_assume():
    shapes = {n: ic.table(n)["Z"].shape for n in ic.TABLES}
    assert shapes == {"t2x2": (2, 2), "t2rows": (2, 67), "t2cols": (131, 2), "guess_bsearch": (29, 37),
                      "uniform": (48, 64), "huge_tiny": (21, 33), "span_overflow": (4, 3)}
    g = ic.table("guess_bsearch")
    assert ic.axis_uses_guess(g["xg"]) and not ic.axis_uses_guess(g["yg"])           # guess + walk / binary search
    assert float(np.min(np.diff(g["yg"]))) == float(np.spacing(1e3))                 # neighbours one ulp apart
    cell = np.diff(g["xg"]).mean()
    assert np.max(np.abs(g["xg"] - np.linspace(g["xg"][0], g["xg"][-1], 37))) < cell / 3 and np.ptp(np.diff(g["xg"])) > 0.1 * cell
    s = ic.table("span_overflow")
    assert np.isinf(s["xg"][-1] - s["xg"][0]) and not ic.axis_uses_guess(s["xg"])    # scale 0: binary search
    assert np.signbit(s["yg"][0]) and s["yg"][1] == 5e-324
    u = ic.table("uniform")
    x0, dx, y0, dy = u["uniform"]
    # fma(i, dx, x0) is inexact at most nodes of both axes
    assert sum(Fraction(i) * Fraction(dx) + Fraction(x0) != Fraction(float(u["xg"][i])) for i in range(64)) > 32
    assert sum(Fraction(i) * Fraction(dy) + Fraction(y0) != Fraction(float(u["yg"][i])) for i in range(48)) > 24
    h = ic.table("huge_tiny")
    assert np.abs(h["xg"]).max() > 5e306 and np.abs(h["yg"]).max() < 1e-300
    for name in ic.TABLES:
        t = ic.table(name)
        Z, Zf = t["Z"], t["Zfinite"]
        assert np.all(np.isfinite(Zf)) and np.abs(Zf).max() < 1e152
        places = ic.special_places(*Z.shape)
        mask = np.zeros(Z.shape, dtype=bool)
        for (i, j), v in places.items():
            mask[i, j] = True
            assert sc.same_bits(Z[i, j:j + 1], np.array([v]))
        assert sc.same_bits(Z[~mask], Zf[~mask])
        if min(Z.shape) >= 5 and name != "span_overflow":
            ny, nx = Z.shape
            assert len(places) == 20 and {(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)} <= set(places)
            # a finite last-row element whose sign shows, and a non-finite first row of the next column
            assert any(i == ny - 1 and np.isfinite(v) and not np.isfinite(Z[0, j + 1]) for (i, j), v in places.items() if j + 1 < nx)
            assert np.signbit(Z[ny - 1, nx - 1]) and Z[ny - 1, nx - 1] == 0.0        # next to the compact padding element
        else:
            assert len(places) == (6 if name == "span_overflow" else 1)


def test_query_sets_are_what_they_say(case):
    t, xq, yq, ref = case
    xg, yg = t["xg"], t["yg"]
    assert xq.size % 2 == 1 and xq.size == yq.size
    for nodes, q in ((xg, xq), (yg, yq)):
        have = set(q[~np.isnan(q)].view(np.int64).tolist())
        want = np.concatenate([nodes, np.nextafter(nodes, -np.inf), np.nextafter(nodes, np.inf),
                               0.5 * nodes[:-1] + 0.5 * nodes[1:], [np.inf, -np.inf]])
        assert set(want.view(np.int64).tolist()) <= have
        assert np.isnan(q).any() and (q < nodes[0]).sum() >= 2 and (q > nodes[-1]).sum() >= 2
        if nodes[0] <= 0.0 <= nodes[-1]:
            assert set(np.array([-0.0, 0.0, 5e-324, -5e-324]).view(np.int64).tolist()) <= have
    with np.errstate(invalid="ignore"):
        # NaN in one coordinate, out of range in the other: NaN wins
        assert (np.isnan(xq) & ((yq < yg[0]) | (yq > yg[-1]))).any() and (np.isnan(yq) & ((xq < xg[0]) | (xq > xg[-1]))).any()
    inr = ic.in_range(xq, yq, xg, yg)
    print("%s: %d queries, %d in range, %d of them finite, %d negative zeros" % (
        t["name"], xq.size, inr.sum(), np.isfinite(ref[inr]).sum(), (np.signbit(ref[inr]) & (ref[inr] == 0.0)).sum()))
    assert inr.sum() >= 25 and np.isfinite(ref[inr]).sum() >= 9
    # the gridded inputs: runs inside one table column interrupted by flagged columns and by other columns
    xi = ic.grid_xi(xg)
    with np.errstate(invalid="ignore"):
        flagged = ~((xi >= xg[0]) & (xi <= xg[-1]))
    lx = np.where(flagged, -1, np.searchsorted(xg, np.where(flagged, xg[0], xi), side="right") - 1)
    after_flag = [(lx[j], lx[j + 2]) for j in range(xi.size - 2) if flagged[j + 1] and lx[j] >= 0]
    assert sum(a == b for a, b in after_flag) >= 4                       # the same column again after a flagged one
    assert any(lx[j] == lx[j + 1] >= 0 for j in range(xi.size - 1))      # ... and directly
    assert any(lx[j] >= 0 and lx[j + 1] >= 0 and lx[j] != lx[j + 1] and lx[j + 2] == lx[j] for j in range(xi.size - 2))
    assert np.isnan(xi).any() and (xi == xg[-1]).any() and np.isinf(xi).any()
    assert set(ic.axis_queries(xg).view(np.int64).tolist()) <= set(np.where(np.isnan(xi), np.nan, xi).view(np.int64).tolist())
    for nyi in (1, 2, 254, 515):
        yi = ic.grid_yi(yg, nyi)
        assert yi.size == nyi and (nyi < ic.axis_queries(yg).size or set(ic.axis_queries(yg)[1:3].tolist()) <= set(yi.tolist()))


def test_oracle_equals_the_literal_scan(case):
    t, xq, yq, ref = case
    assert sc.same_bits(ref, ic.literal_bilinear(t["xg"], t["yg"], t["Z"], xq, yq)), t["name"]
    if t["uniform"]:
        # the implicit-axes entry point above; the explicit one on the nodes fma(i, dx, x0) must agree with both
        assert sc.same_bits(oracle.interp2_bilinear(t["xg"], t["yg"], t["Z"], xq, yq), ref)


def test_extrapolation_value_only_replaces_out_of_range_results(case):
    """ic.with_extrap (what the GPU file derives its references for the other extrapolation values with) is the oracle's
    own answer, bit for bit: out of range and no NaN coordinate -> the value, nothing else changes"""
    t, xq, yq, ref = case
    out = ~ic.in_range(xq, yq, t["xg"], t["yg"]) & ~np.isnan(xq) & ~np.isnan(yq)
    assert np.isnan(ref[~ic.in_range(xq, yq, t["xg"], t["yg"])]).all() and out.any()
    for e in EXTRAPS:
        want = ic.reference(t["name"], xq, yq, e)
        assert sc.same_bits(ic.with_extrap(ref, xq, yq, t["xg"], t["yg"], e), want), (t["name"], e)
        assert sc.same_bits(want[~out], ref[~out]) and sc.same_bits(want[out], np.full(out.sum(), e))


def test_reach_of_non_finite_table_values(case):
    """an in-range output is non-finite only if one of its four bracket corners is: every output whose corners are all
    finite is checked.  (And if one is, the output cannot be finite: inf times a weight is inf or NaN.)"""
    t, xq, yq, ref = case
    inr = ic.in_range(xq, yq, t["xg"], t["yg"])
    fin = ic.corners_finite(t["xg"], t["yg"], t["Z"], xq[inr], yq[inr])
    assert np.all(np.isfinite(ref[inr][fin])), t["name"]
    assert not np.any(np.isfinite(ref[inr][~fin])), t["name"]
    assert fin.sum() >= 9 and ((~fin).sum() >= 9 or np.isfinite(t["Z"]).all())     # (t2x2's one special is a -0.0)


def test_oracle_is_within_the_derived_bound_of_the_exact_bilinear(case):
    """|oracle - exact rational result| <= 16 * 2^-53 * (sum of the four corner magnitudes) (module docstring), on the
    finite-only variant of the table: 3000 seeded in-range queries (half of them from the scattered vector: nodes, ulp
    neighbours, midpoints; half uniform over the range) and every pair of nodes"""
    t, xq, yq, _ = case
    xg, yg, Z = t["xg"], t["yg"], t["Zfinite"]
    rng = np.random.default_rng([0xB11, ic.TABLES.index(t["name"])])
    idx = np.flatnonzero(ic.in_range(xq, yq, xg, yg))
    pick = rng.choice(idx, min(1500, idx.size), replace=False)
    m = 3000 - pick.size
    ux, uy = rng.random(m), rng.random(m)
    qx = np.concatenate([xq[pick], np.clip(xg[0] * (1 - ux) + xg[-1] * ux, xg[0], xg[-1]), np.repeat(xg, yg.size)])
    qy = np.concatenate([yq[pick], np.clip(yg[0] * (1 - uy) + yg[-1] * uy, yg[0], yg[-1]), np.tile(yg, xg.size)])
    assert ic.in_range(qx, qy, xg, yg).all() and qx.size == 3000 + xg.size * yg.size
    got = ic.reference(t["name"], qx, qy, Z=Z)
    assert np.all(np.isfinite(got))
    worst = max(ic.bilinear_error_units(xg, yg, Z, a, b, g) for a, b, g in zip(qx, qy, got))
    print("%s: worst |oracle - exact| = %.3f x 2^-53 x (sum of the corner magnitudes)" % (t["name"], worst))
    assert worst <= ic.BILINEAR_BOUND_UNITS


# ---- the 1-D companion: the reference of tests/test_interp1_values_gpu.py --------------------------------------
@pytest.mark.parametrize("name", list(vc.SPECS))
def test_interp1_value_cases_reference(name):
    """on the tables with non-finite, signed-zero and denormal values: oracle.interp1_bracket has the bits of the literal
    Armadillo scan, and an in-range result is non-finite exactly when one of its two bracket values is"""
    X, xq = vc.nodes(name), vc.queries(name)
    assert xq.size == (vc.NQ_LDS if name in vc.LDS else vc.NQ_BIG) and np.isnan(xq).sum() >= vc.REPEAT
    n = X.size
    have = set(xq[~np.isnan(xq)].tolist())
    for k in vc.special_values(n, "nan_last"):
        for j in range(max(k - 2, 0), min(k + 2, n - 1) + 1):
            want = {float(X[j]), float(np.nextafter(X[j], -np.inf)), float(np.nextafter(X[j], np.inf))}
            if j + 1 < n:
                want.add(float(0.5 * X[j] + 0.5 * X[j + 1]))
            assert want <= have, (name, k, j)
    assert (xq < X[0]).sum() >= 3 * vc.REPEAT and (xq > X[-1]).sum() >= 3 * vc.REPEAT
    head = slice(0, vc.NQ_BIG)                                  # the scan is O(n) per unsorted call: a stretch of it
    for variant in vc.VARIANTS:
        Y = vc.values(name, variant)
        assert np.signbit(Y[n - 2]) and Y[0] == np.inf and (np.isnan(Y[-1]) if variant == "nan_last" else np.signbit(Y[-1]))
        ref = oracle.interp1_bracket(X, Y, xq, nthreads=min(4, oracle.max_threads()))
        assert sc.same_bits(ref[head], oracle.interp1_arma(X, Y, xq[head])), (name, variant)
        assert vc.reach_violations(X, Y, xq, ref).size == 0, (name, variant)
        inr = sc.in_range(xq, X)
        assert np.isnan(ref[~inr]).all()
        zeros = np.signbit(ref[inr]) & (ref[inr] == 0.0)
        print("%s %s: %d in range, %d non-finite, %d negative zeros" % (name, variant, inr.sum(), (~np.isfinite(ref[inr])).sum(), zeros.sum()))
        assert zeros.sum() >= vc.REPEAT and (~np.isfinite(ref[inr])).sum() >= 10 * vc.REPEAT
        for e in (-0.0, 2.5):
            assert sc.same_bits(sc.with_extrap(ref, xq, X, e), oracle.interp1_bracket(X, Y, xq, extrap=e)), (name, variant, e)
