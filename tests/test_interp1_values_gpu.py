"""GPU checks of non-finite, signed-zero and denormal table VALUES through every interp1 kernel behind
mi_interp1_f64_dev, on the cases of tests/interp1_value_cases.py: +inf at the first node, NaN or -0.0 at the last (the
padding node behind the table copies it; cf_mul_pinned also pins its last abscissa), -0.0 at the last but one, +inf next
to -inf, an isolated NaN, two neighbouring -0.0, +-5e-324 and +-1e300 neighbours, with queries on each of those nodes,
their neighbours, ulp neighbours and midpoints.

Everything is compared with oracle.interp1_bracket (held to the literal Armadillo scan and to the reach property on
these inputs in tests/test_interp2_cases_cpu.py): NaN where the oracle has NaN, the same 64 bits everywhere else, the
sign of zero included.  Extrapolation values NaN and -0.0.

Forms: the streaming kernel (order hint 2), the scalar kernel (the vector from its second element), AUTO twice, the
whole-table-in-LDS kernel (hint 1 on the tables inside its 128 KiB window, at least 2^20 queries; the deferred-store
launch counter stays put) -- in this process; the three region-sweep forms each in a child process of its own, under the
hooks and the FORMS table of tests/test_sweep_edges_gpu.py (the hooks are read once per process).  The children are
started together, the launch counter proves the deferred-store kernel ran exactly when the hooks say so, and the sha256
digests they print must agree across the three forms."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import interp1_value_cases as vc
import oracle
import sweep_cases as sc
from test_sweep_edges_gpu import FORMS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAPS = (math.nan, -0.0)

CHILD = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import armadillocudalinearinterpolation_amd as mi
from armadillocudalinearinterpolation_amd import _lib
import oracle
import sweep_cases as sc
import interp1_value_cases as vc
EXPECT = %(expect)d                       # launches of the deferred-store kernel per call that takes the sweep
ctx = mi.Context(0)
L = _lib.load()
ctx.set_query_order(1)
for name, (kind, n, mode) in vc.BIG.items():
    X, xq_np = vc.nodes(name), vc.queries(name)
    xq = torch.from_numpy(xq_np).cuda()
    for variant in vc.VARIANTS:
        Y = vc.values(name, variant)
        grid = mi.Grid1.from_nodes(ctx, X, Y, sanitise=False)
        info = grid.info()
        assert info["mode"] == mode and info["table_bytes"] > 128 * 1024, (name, info)
        if name == "cf_mul_pinned":
            assert (info["formula"], info["pin_last"]) == sc.TABLE_SPECS[name][1:], (name, info)
        ref_nan = oracle.interp1_bracket(X, Y, xq_np)
        for extrap in (float("nan"), -0.0):
            ref = ref_nan if extrap != extrap else sc.with_extrap(ref_nan, xq_np, X, extrap)
            before = L.mi_debug_sweep_ds_launches()
            got = grid.interp(xq, extrap=extrap)
            launched = L.mi_debug_sweep_ds_launches() - before
            assert launched == EXPECT, (name, variant, launched, EXPECT)
            got = got.cpu().numpy()
            if not sc.same_bits(got, ref):
                bad = np.flatnonzero(~np.where(np.isnan(ref), np.isnan(got), got.view(np.int64) == ref.view(np.int64)))
                print("MISMATCH", name, variant, extrap, "count", bad.size, flush=True)
                for i in bad[:24]:
                    l = int(np.searchsorted(X, xq_np[i], side="right")) - 1
                    print("  index", i, "tile", i // sc.TILE, "query", float(xq_np[i]).hex(), "l", l, "Y[l]", Y[max(l, 0)],
                          "Y[r]", Y[min(max(l, 0) + 1, X.size - 1)], "got", float(got[i]).hex(), "want", float(ref[i]).hex(), flush=True)
                raise SystemExit(3)
            print("CASE", name, variant, "nan" if extrap != extrap else "negzero", hashlib.sha256(memoryview(got)).hexdigest(), flush=True)
        grid.close()
print("DONE", flush=True)
"""


def _start(extra, expect):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI_SWEEP_")}
    env.update(MI_SWEEP_MIN_BYTES="0", MI_SWEEP_MIN_TILES_PER_CU="0", **extra)
    prog = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "expect": expect}
    return subprocess.Popen([sys.executable, "-c", prog], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


@pytest.fixture(scope="module")
def runs():
    """(returncode, stdout, stderr) of the three children, started together, each with a time limit of its own"""
    procs = [_start(extra, expect) for _, extra, expect in FORMS]
    out = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        out.append((p.returncode, so, se))
    return out


def _cases(stdout):
    return {tuple(f[1:4]): f[4] for f in (ln.split() for ln in stdout.splitlines()) if f and f[0] == "CASE"}


@pytest.mark.parametrize("which", range(len(FORMS)), ids=[f[0] for f in FORMS])
def test_sweep_forms_equal_the_oracle_bit_for_bit(runs, which):
    """each child asserts, for the four tables beyond the LDS window, both variants and both extrapolation values: the
    mode as the cases state it, its sweep kernel equal to the oracle on every element, and the deferred-store kernel
    launched exactly when its hooks say so.  A mismatch is printed with its index, tile, query and bracket values."""
    rc, so, se = runs[which]
    assert rc == 0 and "DONE" in so, so[-3000:] + se[-3000:]
    assert set(_cases(so)) == {(n, v, e) for n in vc.BIG for v in vc.VARIANTS for e in ("nan", "negzero")}


def test_the_three_sweep_forms_print_the_same_digests(runs):
    d = [_cases(r[1]) for r in runs]
    assert len(d[0]) == 16 and d[0].keys() == d[1].keys() == d[2].keys()
    assert [k for k in d[0] if not (d[0][k] == d[1][k] == d[2][k])] == []


@pytest.fixture(scope="module")
def own_ctx():
    """a context of this module's own: the order hints set here must not reach other tests"""
    import armadillocudalinearinterpolation_amd as mi
    ctx = mi.Context(0)
    yield ctx
    ctx.close()


def _mismatch(tag, got, ref, X, Y, xq):
    bad = np.flatnonzero(~np.where(np.isnan(ref), np.isnan(got), got.view(np.int64) == ref.view(np.int64)))
    lines = ["%r: %d of %d differ" % (tag, bad.size, ref.size)]
    for i in bad[:12]:
        l = max(int(np.searchsorted(X, xq[i], side="right")) - 1, 0)
        lines.append("  index %d query %s l %d Y[l] %r Y[r] %r got %s want %s" % (
            i, float(xq[i]).hex(), l, Y[l], Y[min(l + 1, X.size - 1)], float(got[i]).hex(), float(ref[i]).hex()))
    return "\n".join(lines)


@pytest.mark.parametrize("variant", vc.VARIANTS)
@pytest.mark.parametrize("name", list(vc.SPECS))
def test_streaming_scalar_lds_and_auto_equal_the_oracle_bit_for_bit(own_ctx, name, variant):
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L = own_ctx._L
    kind, n, mode = vc.SPECS[name]
    X, Y, xq = vc.nodes(name), vc.values(name, variant), vc.queries(name)
    grid = mi.Grid1.from_nodes(own_ctx, X, Y, sanitise=False)
    try:
        info = grid.info()
        assert info["mode"] == mode and info["n_nodes"] == X.size, info
        assert (info["table_bytes"] <= 128 * 1024) == (name in vc.LDS), info
        if name == "cf_mul_pinned":
            assert (info["formula"], info["pin_last"]) == sc.TABLE_SPECS[name][1:], info
        ref_nan = oracle.interp1_bracket(X, Y, xq, nthreads=min(4, oracle.max_threads()))
        xd = torch.from_numpy(xq).cuda()
        out = torch.empty(xq.size + 1, dtype=torch.float64, device="cuda")
        assert xd.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        before = L.mi_debug_sweep_ds_launches()
        for extrap in EXTRAPS:
            ref = ref_nan if extrap != extrap else sc.with_extrap(ref_nan, xq, X, extrap)

            def run(tag, hint, lo):
                own_ctx.set_query_order(hint)
                out.fill_(-12345.678)
                grid.interp(xd[lo:], out=out[lo:xq.size], extrap=extrap)
                got = out[lo:xq.size].cpu().numpy()
                assert sc.same_bits(got, ref[lo:]), _mismatch((name, variant, extrap, tag), got, ref[lo:], X, Y, xq[lo:])
                assert float(out[xq.size]) == -12345.678 and (lo == 0 or float(out[0]) == -12345.678)

            run("streaming", 2, 0)
            run("scalar", 2, 1)                      # 8-byte aligned only
            run("scalar, unordered hint", 1, 1)
            if name in vc.LDS:
                run("table in LDS", 1, 0)            # unordered hint, inside the window, >= 2^20 queries
            run("auto, first call", 0, 0)
            run("auto, second call", 0, 0)
        assert L.mi_debug_sweep_ds_launches() == before          # no hooks in this process: never the region sweep
    finally:
        own_ctx.set_query_order(0)
        grid.close()
