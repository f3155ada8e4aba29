"""The seven batched device calls on the seeded cases of tests/batched_fuzz_cases.py: 48 cases per call (cols, rows, stack,
pairs, each, rowpairs, grid, slices2), eight to a test id.  Every operand is a strided view into a guarded canvas; within
one id the canvases go up, the eight calls are enqueued in order on the context's stream with no synchronisation between
them (so the context's scratch slot 3 serves calls of growing and shrinking size in an order nobody chose), then one
synchronisation, everything is read back and batched_fuzz_cases.check() holds each case: results equal to the oracle
bit for bit, every logical output element written, every other element of every canvas untouched, flags right, the form
counter moved by one in the predicted form.  tests/test_batched_fuzz_cases_cpu.py proves the generator's census and
that check() refuses the planted defects.  A failure names (call, index): batched_fuzz_cases.case(call, index) is the
case, anywhere."""
import importlib.util
import os

import pytest

import batched_fuzz_cases as F

pytestmark = pytest.mark.gpu

CHUNK = 8
CHUNKS = F.CASES_PER_CALL // CHUNK
SCRIPTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")


@pytest.fixture(scope="module")
def device_side():
    spec = importlib.util.spec_from_file_location("gpu_fuzz_batched", os.path.join(SCRIPTS, "gpu_fuzz_batched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("call,chunk", [(call, k) for call in F.CALLS for k in range(CHUNKS)],
                         ids=["%s-%d" % (call, k) for call in F.CALLS for k in range(CHUNKS)])
def test_batched_fuzz(mi_ctx, device_side, call, chunk):
    cases = [F.case(call, chunk * CHUNK + j) for j in range(CHUNK)]
    print("\n%s chunk %d: forms %s" % (call, chunk, " ".join(c.form for c in cases)))
    device_side.run_batch(mi_ctx, cases)
