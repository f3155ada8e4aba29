"""CPU proof that tests/test_wide_strides_gpu.py can fail: the cases of tests/wide_stride_cases.py are what they claim
(arithmetic on offsets, no 51 GB), true data and decoys give different results wherever a result reads them, and the one
checking function passes a stand-in kernel with exact addresses and fails it under each of four planted 32-bit
truncations, on every case.  The references are oracle.interp1_bracket and oracle.interp2_bilinear; every comparison
is bit for bit."""
import collections
import os
import re

import numpy as np
import pytest

import wide_stride_cases as W
from wide_stride_cases import CASES

IDS = [c.id for c in CASES]


def test_the_matrix_is_complete():
    """every form of every call, every strided operand of it wide; ids are unique; len is given in every paired call and
    with it a good, a short and (three tables) a bad one"""
    assert len(set(IDS)) == len(IDS)
    have = collections.Counter((c.call, c.form, c.wide) for c in CASES)
    forms = {"cols": ["lds16", "lds8", "direct"], "pairs": ["lds", "direct"], "each": ["thin", "lds", "direct"],
             "rows": ["tile16", "tile8", "flat"], "rowpairs": ["short", "long"],
             "slices2": ["lds-tile", "lds-flat", "direct-tile", "direct-flat"]}
    for call, fs in forms.items():
        for f in fs:
            for wide in W.OPERANDS[call]:
                if call == "cols" and f != "direct":          # the store width is a property of ldyi; ldy takes both too
                    assert have[(call, "lds16", wide)] and have[(call, "lds8", wide)]
                else:
                    assert have[(call, f, wide)] >= 1, (call, f, wide)
    for call in ("pairs", "each", "rowpairs"):
        with_len = [c for c in CASES if c.call == call and "lens" in c.arrays]
        assert with_len and any(c.bad for c in with_len)
        for c in with_len:
            ok = c.want()[1]
            assert ok is not None and ok[0] == 1 and ok[-1] == 1 and ok.sum() == ok.size - c.bad
    for call in W.COUNTERS:
        used = W.COUNTERS[call][1] - (call == "each")           # form 3 of interp1_each forwards to interp1_pairs
        assert {c.counter for c in CASES if c.call == call} == set(range(used))
    assert {c.parity for c in CASES} == {0, 1} and {c.align for c in CASES} == {0, 1}
    for role in ("in", "out"):                                 # dense and padded slices, read and written
        for padded in (True, False):
            assert any(c.how == "slice" and c.role == role and (c.inner > c.wshape[0]) == padded for c in CASES)


def test_limits_are_the_sources():
    """LIMITS, against which the form-selecting sizes are held, are the constants csrc/ states (cols and pairs have no
    form counter: there the limit alone says which kernel a case reaches)"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "armadillocudalinearinterpolation_amd", "csrc")

    def const(name, what):
        text = open(os.path.join(csrc, name)).read()
        m = re.search(r"^constexpr (?:size_t|int) %s = (\w+);" % what, text, flags=re.M)
        assert m, (name, what)
        return block if m.group(1) == "kBlock" else int(m.group(1))

    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(csrc, "mi_interp2_eval.hpp")).read()).group(1))
    assert W.LIMITS == {"cols_lds_n": const("mi_cols1.hip", "kLdsMaxN"), "pairs_lds_n": const("mi_pairs1.hip", "kLdsMaxN"),
                        "each_thin_n": const("mi_each1.hip", "kThinMaxN"), "each_thin_q": const("mi_each1.hip", "kThinMaxQ"),
                        "rows_thin_m": const("mi_rows1.hip", "kThinM"), "rowpairs_thin_n": const("mi_rowpairs1.hip", "kThinN"),
                        "slices_lds_elems": const("mi_slices2.hip", "kLdsMaxElems"),
                        "slices_thin_rows": const("mi_slices2.hip", "kThinRows")}
    assert const("mi_each1.hip", "kLdsMaxN") == W.LIMITS["pairs_lds_n"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_geometry(case):
    """the extent passes 2^32 elements, every block and every alias of it lies inside the pool, and everything planted is
    pairwise disjoint; the stride has the parity the case names"""
    assert case.extent() > 2**32
    assert case.stride % 2 == case.parity and case.base == W.BASE + case.align
    blocks = case.blocks()
    assert blocks[0].D == 0 and blocks[-1].D >= 2**32
    if len(blocks) > 2:
        assert all(2**31 <= b.D < 2**32 for b in blocks[len(blocks) // 2 + 1:-1]) and any(2**31 <= b.D < 2**32 for b in blocks)
    for b in blocks:
        for name, f in W.ADDRESS.items():
            a = case.base + f(b.D)
            assert 0 <= a and a + b.span <= W.POOL, (name, b.D)
        assert {a for _, a in W.aliases(b.D)} == {f(b.D) for f in W.ADDRESS.values()} - {b.D}
    spans = sorted((start, start + img.size, kind, k) for kind, k, _, start, img in case.windows())
    assert spans[0][0] >= 0 and spans[-1][1] <= W.POOL
    for lo, hi in zip(spans, spans[1:]):
        assert lo[1] <= hi[0], "windows overlap: %s and %s" % (lo, hi)
    if case.role == "out":                                     # guards hug their block
        kinds = collections.Counter(kind for kind, *_ in case.windows())
        assert kinds["guard"] == 2 * len(blocks) and kinds["true"] == len(blocks)
    # the far block is misread by every truncation (just beyond 2^32 the four may meet in one window), and the view
    # fits the pool
    assert all(f(blocks[-1].D) != blocks[-1].D for name, f in W.ADDRESS.items() if name != "exact")
    reach = sum((n - 1) * s for n, s in zip(case.wshape, case.view_strides()))
    assert case.base + reach < W.POOL and reach + 1 == case.extent()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_form_selecting_sizes(case):
    """the sizes are on the intended side of the documented limits, and only one operand is wide"""
    A, L = case.arrays, W.LIMITS
    call, form = case.call, case.form
    if call == "cols":
        n, nq = A["x"].size, A["xi"].size
        assert (n <= L["cols_lds_n"]) == form.startswith("lds")
        ldyi, aligned = (case.stride, case.align == 0) if case.wide == "ldyi" else (case.compact_ld("YI"), True)
        if form != "direct":                                   # 16-B stores: yi 16-B aligned and ldyi even
            assert (ldyi % 2 == 0 and aligned) == (form == "lds16")
    elif call in ("pairs", "each"):
        n = A["X"].shape[0]
        nq = A["XI"].shape[0] if call == "each" else A["xi"].size
        thin = call == "each" and n <= L["each_thin_n"] and nq <= L["each_thin_q"]
        assert thin == (form == "thin")
        if not thin:
            assert (n <= L["pairs_lds_n"]) == (form == "lds") and n in (257, L["pairs_lds_n"], L["pairs_lds_n"] + 1)
    elif call == "rows":
        m = A["Y"].shape[0]
        assert (m < L["rows_thin_m"]) == (form == "flat")
        if form != "flat":
            lds = [case.stride, case.compact_ld("YI" if case.role == "in" else "Y")]
            assert (all(v % 2 == 0 for v in lds) and case.align == 0) == (form == "tile16")
    elif call == "rowpairs":
        assert (A["X"].shape[1] <= L["rowpairs_thin_n"]) == (form == "short") and A["X"].shape[1] in (3, 32, 33)
    else:
        ny, nx, S = A["Z"].shape
        assert (nx * ny <= L["slices_lds_elems"]) == form.startswith("lds")
        assert (A["yi"].size < L["slices_thin_rows"]) == form.endswith("flat")
        assert S == (2 if case.how == "slice" else 1)
    assert list(W.OPERANDS[call]).count(case.wide) == 1
    rows, cols, S = case.wshape
    assert max(rows, cols) <= 8193 and S <= 2 and (case.how == "slice" or cols <= 33)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_queries_and_flagged_outputs(case):
    """the queries hit both end nodes, the first and the last cell, an interior node's ulp neighbours, NaN and both sides
    out of range; the flagged outputs are exactly the handful that was planted"""
    A = case.arrays
    axes = []
    if case.call in ("cols", "rows"):
        axes.append((A["x"], A["xi"]))
    elif case.call == "slices2":
        axes += [(A["ax"], A["xi"]), (A["ay"], A["yi"])]
    elif case.call == "each":
        axes.append((A["X"][:, -1], A["XI"][:, -1]))
    else:
        axes.append((A["X"][-1] if case.call == "rowpairs" else A["X"][:, -1], A["xi"]))
    for x, q in axes:
        n = x.size
        cell = np.searchsorted(x, q[np.isfinite(q) & (q >= x[0]) & (q <= x[-1])], side="right") - 1
        assert x[0] in q and x[-1] in q and np.isnan(q).sum() == 1 and (q < x[0]).sum() == 1 and (q > x[-1]).sum() == 1
        assert np.any((q > x[0]) & (q < x[1])) or case.form == "thin"
        assert np.any((q > x[-2]) & (q < x[-1])) and (n - 1) in cell and (n - 2) in cell
        assert any(np.nextafter(v, np.inf) in q for v in x[:-1]) and any(np.nextafter(v, -np.inf) in q for v in x[1:])
    flagged = case.flagged()
    assert int(flagged.sum()) == case.planted_flagged(), (int(flagged.sum()), case.planted_flagged())
    assert flagged.sum() < flagged.size / 2 or case.form == "thin"
    assert not np.any(case.want()[0] == W.SENT_FILL) and not np.any(case.want()[0] == W.SENT_GUARD)


@pytest.mark.parametrize("case", [c for c in CASES if c.role == "in"], ids=[c.id for c in CASES if c.role == "in"])
def test_every_decoy_changes_every_result_that_reads_it(case):
    """Detection condition.  An output READS block k when a gross change of the block (+2^20) changes it: a column-type
    block is read by every in-range, non-NaN query of its column or slice, a node column of a row-type call by the
    queries whose bracket holds it with a non-zero weight.  For every decoy of every block, every such output computed
    on the decoy differs bitwise from the one computed on the true data: 0 coincidences.  Flagged outputs (extrap, NaN)
    read nothing and are left out; test_queries_and_flagged_outputs counts them."""
    want = case.want()[0].reshape(case._shape3("YI"))
    flagged = case.flagged().reshape(want.shape)
    L = case._logical()
    compared = coincidences = 0
    for k, b in enumerate(case.blocks()):
        probe = W.expected(case.call, case.substituted(k, L[b.sel] + 2.0**20))[0].reshape(want.shape)
        reads = ~W._same(probe, want) & ~flagged
        table_bad = False
        if case.call in ("cols", "pairs", "each") or case.how == "slice":
            mine = np.zeros_like(reads)
            mine[(slice(None), slice(None), k) if case.how == "slice" else (slice(None), k)] = True
            table_bad = bool(flagged[mine].all())              # the bad column of a case with lens: nothing reads it
            assert np.array_equal(reads, mine & ~flagged), "block %d is not read by all its in-range queries" % k
        assert reads.any() or table_bad, "no output reads block %d" % k
        decoys = [w for w in case.windows() if w[0] == "decoy" and w[1] == k]
        assert len(decoys) == len(W.aliases(b.D))
        for rank in range(len(decoys)):
            d = case.decoy(k, rank)
            assert np.all(np.isfinite(d) | np.isnan(L[b.sel])) and not np.any(d == L[b.sel])
            got = W.expected(case.call, case.substituted(k, d))[0].reshape(want.shape)
            compared += int(reads.sum())
            coincidences += int((reads & W._same(got, want)).sum())
    assert compared > 0 and coincidences == 0, (compared, coincidences)


def _planted(case):
    pool = W.SparsePool()
    case.plant(pool.write)
    return pool


def _delta(case):
    return None if case.counter is None else [int(f == case.counter) for f in range(W.COUNTERS[case.call][1])]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_check_passes_exact_addresses(case):
    pool = _planted(case)
    out, ok = W.model_call(case, pool, W.ADDRESS["exact"])
    W.check(case, pool.read, out, ok, _delta(case))


@pytest.mark.parametrize("wrong", W.WRONG)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_check_fails_every_planted_truncation(case, wrong):
    """reads (a wide input) and writes (a wide output) through a 32-bit misreading of the offset: the stand-in kernel
    stays inside the planted windows (SparsePool raises otherwise) and check() refuses the result"""
    pool = _planted(case)
    out, ok = W.model_call(case, pool, W.ADDRESS[wrong])
    with pytest.raises(AssertionError):
        W.check(case, pool.read, out, ok, _delta(case))


def test_check_fails_the_other_faults():
    """an output block left unwritten, one written past its end, a wrong flag and a wrong form are refused too"""
    case = next(c for c in CASES if c.role == "out" and "lens" in c.arrays and c.counter is not None)
    b = case.blocks()[-1]
    for fault in ("unwritten", "overrun", "flag", "form"):
        pool = _planted(case)
        out, ok = W.model_call(case, pool, W.ADDRESS["exact"])
        delta = _delta(case)
        if fault == "unwritten":
            img = pool.read(case.base + b.D, b.span)
            img[b.idx.reshape(-1)[-1]] = W.SENT_FILL
            pool.write(case.base + b.D, img)
        elif fault == "overrun":
            pool.write(case.base + b.D + b.span, np.array([1.5]))
        elif fault == "flag":
            ok = 1 - ok
        else:
            delta = delta[::-1]
        with pytest.raises(AssertionError):
            W.check(case, pool.read, out, ok, delta)
