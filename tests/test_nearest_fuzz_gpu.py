"""The two "nearest" device calls on the seeded cases of tests/nearest_fuzz_cases.py: 48 cases per call (cols_nearest,
table_nearest), eight to a test id, four of each call alternating -- so the columns call's 4-B records in the context's
scratch slot 3 are regrown and shrunk between table calls, on one stream with no synchronisation in between.  Every
operand is a strided view into a guarded canvas; after the one synchronisation everything is read back and
batched_fuzz_cases.check() holds each case: results equal to nearest_cases.nearest_rule bit for bit, every logical output
element written, every other element of every canvas untouched, mi_debug_nearest_launches moved by one in the predicted
form.  tests/test_nearest_fuzz_cases_cpu.py proves the generator's census and that check() refuses the planted defects.
A failure names (call, index): nearest_fuzz_cases.case(call, index) is the case, anywhere."""
import importlib.util
import os

import pytest

import nearest_fuzz_cases as NF
import sweep_cases as sc

pytestmark = pytest.mark.gpu

PER_CALL = 4                                                     # cases of each call in one test id
CHUNKS = NF.CASES_PER_CALL // PER_CALL
SCRIPTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
REPORTED = {}                                                    # chunk -> [(mode, formula, pin_last, implicit)] of its tables


@pytest.fixture(scope="module")
def device_side():
    spec = importlib.util.spec_from_file_location("gpu_fuzz_nearest", os.path.join(SCRIPTS, "gpu_fuzz_nearest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _chunk(k):
    return [NF.case(call, k * PER_CALL + j) for j in range(PER_CALL) for call in NF.CALLS]


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_nearest_fuzz(mi_ctx, device_side, chunk):
    cases = _chunk(chunk)
    print("\nchunk %d: %s" % (chunk, " ".join("%s:%s" % (c.id, c.form) for c in cases)))
    REPORTED[chunk] = device_side.run_batch(mi_ctx, cases)
    print("  tables (mode, formula, pin_last, implicit): %s" % (REPORTED[chunk],))


def test_the_fixed_tables_reach_every_table_form(mi_ctx, device_side):
    """between them the 48 table_nearest cases report every (mode, formula, pin_last) of sweep_cases.TABLE_SPECS and an
    implicit (Grid1.uniform) table: the select has then run behind every bracket of nearest_batch_from"""
    for k in range(CHUNKS):
        if k not in REPORTED:                                    # (this test alone: run what has not run)
            REPORTED[k] = device_side.run_batch(mi_ctx, _chunk(k))
    seen = [t for k in range(CHUNKS) for t in REPORTED[k]]
    assert len(seen) == NF.CASES_PER_CALL
    print("\nreported: %s" % sorted(set(seen)))
    explicit = {t[:3] for t in seen if not t[3]}
    want = {tuple(-1 if v is None else v for v in spec) for spec in sc.TABLE_SPECS.values()}
    assert explicit >= want, want - explicit
    assert any(t[3] for t in seen) and all(t[:3] == (0, 0, 0) for t in seen if t[3]), seen


def test_nearest_fuzz_short(mi_ctx, device_side):
    res = device_side.run(8.0, 2024, ctx=mi_ctx)
    for call in NF.CALLS:
        assert set(res["forms"][call]) == set(NF.FORMS[call]), res["forms"]
