"""The generator of tests/batched_fuzz_cases.py is what it claims, and its check() has teeth -- without a GPU.
Determinism; the census of every call (forms, limits hit exactly and at +1, base offsets, leading-dimension parity, axis
kinds, query styles, extrap values, bad tables, lens, want_ok, the size caps); the limits against the constexpr values in
csrc/; check() passes the exact numpy model on every case and refuses every planted defect on every case it applies to.
Run with -s for the census and the defect matrix."""
import os
import re

import numpy as np
import pytest

import batched_fuzz_cases as F
from armadillocudalinearinterpolation_amd import _build

MIN_FORM, MIN_BASE, MIN_PARITY, MIN_DEFECT = 4, 8, 8, 4


@pytest.fixture(scope="module")
def cases():
    return {call: F.all_cases(call) for call in F.CALLS}


def test_cases_are_determined_by_call_and_index(cases):
    for call in F.CALLS:
        assert len(cases[call]) == F.CASES_PER_CALL == 48
        assert [c.index for c in cases[call]] == list(range(48)) and all(c.call == call for c in cases[call])
    # built again, in another order and alone: identical bytes
    for call in reversed(F.CALLS):
        for i in (47, 0, 13, 30):
            assert F.case(call, i).key_bytes() == cases[call][i].key_bytes(), (call, i)
    # another seed is another case; the fixed one is the default
    assert F.case("cols", 3, seed=F.SEED + 1).key_bytes() != cases["cols"][3].key_bytes()
    assert F.case("cols", 3, seed=F.SEED).key_bytes() == cases["cols"][3].key_bytes()
    # indices beyond the fixed block (the long runs) work too, and keep cycling the forms
    assert {F.case("each", 48 + i).form for i in range(4)} == set(F.FORMS["each"])


@pytest.mark.parametrize("call", F.CALLS)
def test_census(cases, call):
    cen = F.census(call, cases[call])
    print("\n%s: forms %s\n  kinds %s\n  styles %s\n  extrap %s\n  base offsets %s\n  output ld parity %s\n  sizes %s" % (
        call, cen["forms"], cen["kinds"], cen["styles"], cen["extrap"], dict(sorted(cen["base"].items())), cen["out_ld"],
        {k: sorted(v) for k, v in cen["sizes"].items()}))
    print("  pad_node traps %d, special values %d, largest table %d, largest output %d" % (
        cen["trap"], cen["special"], cen["max_table"], cen["max_out"]))
    if call in F.PAIRED:
        print("  lens %s, want_ok %s, bad tables %s, bad-table cases by want_ok %s, a bad table first in %d cases, last in %d" % (
            cen["lens"], cen["use_ok"], cen["bad"], cen["bad_use_ok"], cen["bad_first"], cen["bad_last"]))
    assert set(cen["forms"]) == set(F.FORMS[call]) and min(cen["forms"].values()) >= MIN_FORM
    for limit, size in F.LIMIT_SIZES[call]:
        seen = cen["sizes"][size]
        assert F.LIMITS[limit] in seen and F.LIMITS[limit] + 1 in seen, (limit, sorted(seen))
    for name in sorted(set(name for c in cases[call] for name in c.ops)):
        assert cen["base"].get((name, 0), 0) >= MIN_BASE and cen["base"].get((name, 1), 0) >= MIN_BASE, (name, cen["base"])
    assert cen["out_ld"]["odd"] >= MIN_PARITY and cen["out_ld"]["even"] >= MIN_PARITY
    kinds = set(F.AXIS_KINDS if call not in F.PAIRED else F.TABLE_KINDS)
    assert set(cen["kinds"]) >= kinds, kinds - set(cen["kinds"])
    assert set(cen["styles"]) == set(F.STYLES)
    assert set(cen["extrap"]) == set(range(len(F.EXTRAPS)))
    assert cen["max_table"] <= F.CAP and cen["max_out"] <= F.CAP
    assert cen["trap"] >= MIN_DEFECT and cen["special"] >= 12
    if call in F.PAIRED:
        assert set(cen["bad"]) == set(F.BAD_KINDS)
        assert cen["lens"][True] == 24 and cen["lens"][False] == 24
        assert min(cen["use_ok"].values()) >= 12 and min(cen["bad_use_ok"].values()) >= 2
        assert cen["bad_first"] >= 1 and cen["bad_last"] >= 1
        assert sum(1 for c in cases[call] if c.meta["bad"]) == 12


def test_each_reaches_the_thin_form_in_a_quarter_of_its_cases(cases):
    thin = [c for c in cases["each"] if c.form == "thin"]
    assert len(thin) == 12
    for c in thin:
        Z = dict(c.meta["sizes"])
        assert Z["n"] <= F.LIMITS["each_thin_n"] and Z["nq"] <= F.LIMITS["each_thin_q"]
    assert sum("xi" in c.ops for c in thin) == 6 and sum("XI" in c.ops for c in thin) == 6       # one shared XI / one per column


def test_layout_is_what_the_canvases_hold(cases):
    """inputs: the data where the Operand says, NaN everywhere else; outputs: SENT_FILL there, SENT_GUARD everywhere else"""
    for call in F.CALLS:
        for c in cases[call][::5]:
            cv = F.canvases(c)
            for name, op in c.ops.items():
                idx = op.index()
                assert cv[name].size == op.size and idx.min() == F.FRONT + op.base and idx.max() + F.TAIL + 1 == op.size
                assert np.unique(idx).size == idx.size
                rest = np.ones(op.size, dtype=bool)
                rest[idx.reshape(-1)] = False
                if name == "lens":
                    assert np.all(cv[name][rest] == -1)
                elif op.role == "out":
                    assert np.all(cv[name][rest] == F.SENT_GUARD) and np.all(cv[name][idx] == F.SENT_FILL)
                else:
                    assert np.all(np.isnan(cv[name][rest]))
                    assert F.same_bits(cv[name][idx], np.asarray(c.arrays[name], dtype=np.float64).reshape(op.shape))


def _constexpr(unit, name):
    text = re.sub(r"//.*", "", open(os.path.join(_build.CSRC, unit)).read())
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, (unit, name)
    expr = m.group(1).strip()
    if expr == "kBlock":
        b = re.search(r"constexpr\s+\w+\s+kBlock\s*=\s*(\d+)\s*;", text)
        if not b:
            for header in re.findall(r'#include\s+"(mi_[\w.]+)"', text):           # the unit's own headers
                b = b or re.search(r"constexpr\s+\w+\s+kBlock\s*=\s*(\d+)\s*;", open(os.path.join(_build.CSRC, header)).read())
        assert b, (unit, "kBlock")
        return int(b.group(1))
    assert re.fullmatch(r"\d+", expr), (unit, name, expr)
    return int(expr)


def test_the_limits_are_the_sources():
    L = F.LIMITS
    assert _constexpr("mi_cols1.hip", "kLdsMaxN") == L["cols_lds_n"]
    assert _constexpr("mi_pairs1.hip", "kLdsMaxN") == L["pairs_lds_n"]
    assert _constexpr("mi_each1.hip", "kLdsMaxN") == L["pairs_lds_n"]
    assert _constexpr("mi_each1.hip", "kThinMaxN") == L["each_thin_n"]
    assert _constexpr("mi_each1.hip", "kThinMaxQ") == L["each_thin_q"]
    assert _constexpr("mi_rows1.hip", "kThinM") == L["rows_thin_m"]
    assert _constexpr("mi_rowpairs1.hip", "kThinN") == L["rowpairs_thin_n"]
    assert _constexpr("mi_interp2_grid.hip", "kThinRows") == L["grid_thin_rows"]
    assert _constexpr("mi_slices2.hip", "kLdsMaxElems") == L["slices_lds_elems"]
    assert _constexpr("mi_slices2.hip", "kThinRows") == L["slices_thin_rows"]


@pytest.mark.parametrize("call", F.CALLS)
def test_check_passes_the_exact_model(cases, call):
    for c in cases[call]:
        F.check(c, *F.model_call(c))


# the calls a defect can apply to at all (batched_fuzz_cases.PRECONDITION)
CAN_APPLY = {
    "pad_node": F.CALLS, "stray_store": F.CALLS, "nan_is_extrap": F.CALLS, "ignores_len": F.PAIRED, "signed_zero_ok": F.PAIRED,
    "reads_padding": tuple(c for c in F.CALLS if c != "grid"), "wrong_form": tuple(F.COUNTER_CALL),
}


@pytest.mark.parametrize("call", F.CALLS)
def test_check_refuses_every_planted_defect(cases, call):
    row = []
    for defect in F.DEFECTS:
        hit = 0
        for c in cases[call]:
            if not F.applies(c, defect):
                continue
            hit += 1
            with pytest.raises(AssertionError, match=r"\(%s, %d\)" % (call, c.index)):
                F.check(c, *F.model_call(c, defect))
        row.append("%s %d" % (defect, hit))
        if call in CAN_APPLY[defect]:
            assert hit >= MIN_DEFECT, (call, defect, hit)
        else:
            assert hit == 0, (call, defect, hit)
    print("\n%-8s refused on: %s (cases of 48)" % (call, ", ".join(row)))


def test_check_names_the_first_bad_element():
    c = F.case("cols", 0)
    after, ok, before, cafter = F.model_call(c)
    op = c.ops["YI"]
    at = int(op.index()[0, op.cols - 1, 0])
    good = after["YI"][at]
    after["YI"][at] = 0.125 if good != 0.125 else 0.25
    with pytest.raises(AssertionError) as e:
        F.check(c, after, ok, before, cafter)
    assert "(cols, 0)" in str(e.value) and "(0, %d, 0)" % (op.cols - 1) in str(e.value) and repr(c.want[0, op.cols - 1, 0]) in str(e.value)
    after["YI"][at] = F.SENT_FILL
    with pytest.raises(AssertionError, match="not written"):
        F.check(c, after, ok, before, cafter)
    after2 = {k: v.copy() for k, v in F.model_call(c)[0].items()}
    after2["YI"][0] = 1.0                                        # the front guard
    with pytest.raises(AssertionError, match="stray store"):
        F.check(c, after2, ok, before, cafter)
    after3 = {k: v.copy() for k, v in F.model_call(c)[0].items()}
    after3["Y"][5] = 0.0                                         # an input's guard
    with pytest.raises(AssertionError, match="input canvas Y changed"):
        F.check(c, after3, ok, before, cafter)
