"""The generator of tests/nearest_fuzz_cases.py is what it claims, and batched_fuzz_cases.check() has teeth on its cases --
without a GPU.  Determinism; the census of both calls (forms, the sizes on both sides of every limit, axis kinds, query
styles, extrap values, base offsets); the restated limits against the constexpr values of csrc/mi_nearest1.hip; exact ties
and both sides of the select as conditions on the inputs; check() passes the exact numpy model on every case and refuses
every planted defect on every case it applies to.  Run with -s for the census and the defect table."""
import os
import re

import numpy as np
import pytest

import batched_fuzz_cases as F
import nearest_cases as nc
import nearest_fuzz_cases as NF
from armadillocudalinearinterpolation_amd import _build

MIN_FORM, MIN_TIE_CASES, MIN_DEFECT = 10, 6, 6


@pytest.fixture(scope="module")
def cases():
    return {call: NF.all_cases(call) for call in NF.CALLS}


def test_cases_are_determined_by_call_and_index(cases):
    for call in NF.CALLS:
        assert len(cases[call]) == NF.CASES_PER_CALL == 48
        assert [c.index for c in cases[call]] == list(range(48)) and all(c.call == call for c in cases[call])
    for call in reversed(NF.CALLS):                              # built again, in another order and alone: identical bytes
        for i in (47, 0, 13, 30):
            assert NF.case(call, i).key_bytes() == cases[call][i].key_bytes(), (call, i)
    assert NF.case("cols_nearest", 3, seed=NF.SEED + 1).key_bytes() != cases["cols_nearest"][3].key_bytes()
    assert NF.case("cols_nearest", 3, seed=NF.SEED).key_bytes() == cases["cols_nearest"][3].key_bytes()
    for call in NF.CALLS:                                        # the long runs' indices keep cycling the forms
        assert {NF.case(call, 48 + i).form for i in range(len(NF.FORMS[call]))} == set(NF.FORMS[call])
    assert not set(NF.CALL_INDEX.values()) & set(range(len(F.CALLS)))        # streams of their own


@pytest.mark.parametrize("call", NF.CALLS)
def test_census(cases, call):
    cen = NF.census(call, cases[call])
    print("\n%s: forms %s\n  kinds %s\n  styles %s\n  extrap %s\n  base offsets %s\n  n %s\n  nq %s" % (
        call, cen["forms"], cen["kinds"], cen["styles"], cen["extrap"], dict(sorted(cen["base"].items())), sorted(cen["n"]),
        sorted(cen["nq"])))
    print("  cases with an exact tie %d (%d ties), pad_node traps %d, special values %d, Y pads %s, largest table %d, largest "
          "output %d" % (cen["tie_cases"], cen["ties"], cen["trap"], cen["special"], dict(sorted(cen["y_pad"].items())),
                         cen["max_table"], cen["max_out"]))
    print("  in-range queries of the cases with nq >= 255: %d, the right node chosen for %d (%.1f %%)" % (
        cen["in_range"], cen["right"], 100.0 * cen["right"] / cen["in_range"]))
    assert set(cen["forms"]) == set(NF.FORMS[call]) and min(cen["forms"].values()) >= MIN_FORM
    if call == "cols_nearest":
        assert {NF.COLS_LDS_N, NF.COLS_LDS_N + 1} <= cen["n"]
        assert {2, 3} <= cen["n"] and set(cen["y_pad"]) > {0, 1}
        for c in cases[call]:
            assert c.meta["store"] == (16 if c.ops["YI"].base == 0 and c.ops["YI"].ld % 2 == 0 else 8)
            assert c.counter == (NF.COLS_LDS if dict(c.meta["sizes"])["n"] <= NF.COLS_LDS_N else NF.COLS_DIRECT)
    else:
        assert {NF.STREAM_BLOCK - 1, NF.STREAM_BLOCK, NF.STREAM_BLOCK + 1} <= cen["nq"]
        assert cen["nq"] == set(NF.TABLE_NQ) and cen["n"] >= set(NF.TABLE_N)
        for c in cases[call]:
            nq, bases = dict(c.meta["sizes"])["nq"], (c.ops["xq"].base, c.ops["yq"].base)
            assert (c.form, c.counter) == (("scalar", NF.SCALAR) if any(bases) else
                                           ("stream-full" if nq >= NF.STREAM_BLOCK + 1 else "stream-part", NF.STREAM)), c
            assert c.form != "stream-part" or nq < NF.STREAM_BLOCK
            assert (c.meta["kinds"][0] == "uniform") == c.meta["implicit"]
    assert set(cen["kinds"]) == set(NF.KINDS[call])
    assert set(cen["styles"]) == set(F.STYLES)
    assert set(cen["extrap"]) == set(range(len(F.EXTRAPS)))
    for name in sorted(set(name for c in cases[call] for name in c.ops)):
        assert cen["base"].get((name, 0), 0) >= 8 and cen["base"].get((name, 1), 0) >= 8, (name, cen["base"])
    assert cen["max_table"] <= F.CAP and cen["max_out"] <= F.CAP
    assert cen["trap"] == 16 and cen["special"] == 16


def _constexpr(name):
    text = re.sub(r"//.*", "", open(os.path.join(_build.CSRC, "mi_nearest1.hip")).read())
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, name
    return int(m.group(1))


def test_the_limits_are_the_sources():
    assert _constexpr("kLdsMaxN") == NF.COLS_LDS_N == F.LIMITS["cols_lds_n"]
    assert _constexpr("kBlock") * _constexpr("kVecVpl") * 2 == NF.STREAM_BLOCK
    text = open(os.path.join(_build.CSRC, "mi_nearest1.hip")).read()
    assert "0 streaming, 1 table in LDS, 2 scalar, 3 columns LDS form, 4 columns direct form" in text
    assert re.search(r"g_launches\[%d\]" % NF.NCOUNTERS, text)


@pytest.mark.parametrize("call", NF.CALLS)
def test_ties_and_both_sides_of_the_select(cases, call):
    """conditions on the inputs, not on the kernel: recounted here from the case's arrays with nearest_cases.rule_index"""
    tie_cases, inr_all, right_all = 0, 0, 0
    for c in cases[call]:
        x = c.axes["x"]["nodes"]
        q = c.arrays["xi" if call == "cols_nearest" else "xq"]
        k = nc.rule_index(x, q)
        inr = k >= 0
        l = np.searchsorted(x, q[inr], side="right") - 1
        r = np.minimum(l + 1, x.size - 1)
        ties = int(np.sum((r > l) & (q[inr] - x[l] == x[r] - q[inr])))
        assert (ties, int(inr.sum()), int(np.sum(k[inr] > l))) == (c.meta["ties"], c.meta["in_range"], c.meta["right"])
        assert np.all(k[inr][(r > l) & (q[inr] - x[l] == x[r] - q[inr])] == l[(r > l) & (q[inr] - x[l] == x[r] - q[inr])])
        tie_cases += ties > 0
        if q.size >= 255:
            inr_all += int(inr.sum())
            right_all += int(np.sum(k[inr] > l))
        if q.size >= 7 + NF.EXTRA:                               # the added points are there
            last = 0.5 * x[-2] + 0.5 * x[-1]
            for v in (last, np.nextafter(last, -np.inf), np.nextafter(last, np.inf), x[-1], x[0]):
                assert np.any(q == v), (c, v)
            assert np.isnan(q).any()
    assert tie_cases >= MIN_TIE_CASES, tie_cases
    assert 0.30 <= right_all / inr_all <= 0.70, (right_all, inr_all)


@pytest.mark.parametrize("call", NF.CALLS)
def test_check_passes_the_exact_model(cases, call):
    for c in cases[call]:
        F.check(c, *NF.model_call(c))


@pytest.mark.parametrize("call", NF.CALLS)
def test_check_refuses_every_planted_defect(cases, call):
    row = []
    for defect in NF.DEFECTS:
        hit = 0
        for c in cases[call]:
            if not NF.applies(c, defect):
                continue
            hit += 1
            with pytest.raises(AssertionError, match=r"\(%s, %d\)" % (call, c.index)):
                F.check(c, *NF.model_call(c, defect))
        row.append("%s %d / %d" % (defect, hit, hit))
        if call in NF.CAN_APPLY[defect]:
            assert hit >= MIN_DEFECT, (call, defect, hit)
        else:
            assert hit == 0, (call, defect, hit)
        if defect in ("stray_store", "wrong_form"):
            assert hit == len(cases[call])
    print("\n%-13s applies / refused: %s (cases of 48)" % (call, ", ".join(row)))


def test_the_model_is_not_the_reference(cases):
    """model_call computes its own bracket and select: it reads nothing of nearest_cases, and a wrong tie rule in it is
    refused on exactly the cases that hold an exact tie"""
    import inspect
    assert "nc." not in inspect.getsource(NF._np_nearest) + inspect.getsource(NF._model_out)
    for call in NF.CALLS:
        assert [c.index for c in cases[call] if NF.applies(c, "tie_right")] == [c.index for c in cases[call] if c.meta["ties"]]
