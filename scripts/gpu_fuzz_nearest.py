"""Differential fuzz of the two "nearest" device calls (Axis1.interp_cols_nearest, Grid1.interp_nearest) against
nearest_cases.nearest_rule, with guarded canvases around every operand (run on the GPU box).  The generator and the
reference are tests/nearest_fuzz_cases.py, the check is batched_fuzz_cases.check(); this file holds the device side --
upload the canvases, make the strided views, create the axis / table, enqueue the calls, read everything back -- which
tests/test_nearest_fuzz_gpu.py uses for the fixed cases, and run(), the long run by hand with other seeds."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

import batched_fuzz_cases as F
import nearest_fuzz_cases as NF


class Staged:
    """one case on the device: dev the canvases, view the strided operand views, h the Axis1 / Grid1, made before any call
    of the batch is enqueued (creating a handle uploads and may synchronise; the calls themselves must not).  table: what
    the library reports for a table_nearest case's Grid1, (mode, formula, pin_last, implicit)."""

    def __init__(self, ctx, c):
        import armadillocudalinearinterpolation_amd as mi
        self.case, self.ctx = c, ctx
        self.dev = {name: torch.from_numpy(a).cuda() for name, a in F.canvases(c).items()}
        self.view = {}
        for name, op in c.ops.items():
            t = self.dev[name]
            assert t.data_ptr() % 256 == 0, "a canvas is not 256-B aligned"
            if op.cols == 1 and name in ("xi", "xq", "yq"):
                self.view[name] = t[op.start:op.start + op.rows]
            else:
                self.view[name] = torch.as_strided(t, (op.rows, op.cols), (1, op.ld), op.start)
            assert (self.view[name].data_ptr() % 16 != 0) == bool(op.base)
        ax = c.axes["x"]
        self.table = None
        if c.call == "cols_nearest":
            self.h = (mi.Axis1.uniform(ctx, ax["x0"], ax["dx"], ax["nodes"].size) if ax["kind"] == "uniform"
                      else mi.Axis1.from_nodes(ctx, ax["nodes"]))
        else:
            Y = np.ascontiguousarray(c.arrays["Y"], dtype=np.float64)
            self.h = (mi.Grid1.uniform(ctx, ax["x0"], ax["dx"], Y) if ax["kind"] == "uniform"
                      else mi.Grid1.from_nodes(ctx, ax["nodes"], Y, sanitise=False))
            info = self.h.info()                                 # formula and pin_last: mi_debug_grid1_formula
            assert info["n_nodes"] == ax["nodes"].size
            self.table = (info["mode"], info["formula"], info["pin_last"], ax["kind"] == "uniform")
        self.before = self.after = None

    def _counters(self):
        return [int(getattr(self.ctx._L, NF.COUNTER_NAME)(f)) for f in range(NF.NCOUNTERS)]

    def enqueue(self):
        """the call, asynchronous on the context's stream; the status is held by check() of api.py: anything but MI_OK raises"""
        c, v = self.case, self.view
        self.before = self._counters()
        if c.call == "cols_nearest":
            r = self.h.interp_cols_nearest(v["Y"], v["xi"], out=v["YI"], extrap=c.extrap)
        else:
            r = self.h.interp_nearest(v["xq"], out=v["yq"], extrap=c.extrap)
        self.after = self._counters()
        assert r.data_ptr() == v[c.out].data_ptr(), "%s: the call did not write into the given out" % c.id

    def finish(self):
        """after the synchronisation: close the handle, read every canvas back and check"""
        self.h.close()
        got = {name: t.cpu().numpy() for name, t in self.dev.items()}
        F.check(self.case, got, None, self.before, self.after)


def run_batch(ctx, cases):
    """stage the cases, enqueue their calls in order with no synchronisation between them, synchronise once, check each;
    returns what the library reported for every table_nearest case's table.  The context is left at query order 0."""
    ctx.set_query_order(0)
    staged = [Staged(ctx, c) for c in cases]
    try:
        for s in staged:
            s.enqueue()
    finally:
        ctx.synchronize()
        torch.cuda.synchronize()
        ctx.set_query_order(0)
    failure = None
    for s in staged:                                             # every handle is closed, whichever case fails first
        try:
            s.finish()
        except AssertionError as e:
            failure = failure or e
    if failure:
        raise failure
    return [s.table for s in staged if s.table is not None]


def run(budget, seed, ctx=None):
    """rounds of four cases per call, the two calls alternating (the 4-B record slot of the columns call is regrown and
    shrunk between table calls), until the budget, in seconds, is spent; seed: any but the suite's fixed one"""
    import armadillocudalinearinterpolation_amd as mi
    ctx = ctx or mi.Context(0)
    t0, cases, forms, tables = time.time(), 0, {call: {} for call in NF.CALLS}, {}
    beat, index = t0, 0
    while time.time() - t0 < budget:
        if time.time() - beat > 60.0:          # a sign of life every minute (a silent GPU command is taken to be hung)
            beat = time.time()
            print("  ... %d cases after %.0f s" % (cases, beat - t0), flush=True)
        batch = [NF.case(call, index + j, seed) for j in range(4) for call in NF.CALLS]
        try:
            seen = run_batch(ctx, batch)
        except AssertionError:
            print("MISMATCH in indices %d..%d of seed %d: nearest_fuzz_cases.case(call, index, %d) reproduces it" % (
                index, index + 3, seed, seed), flush=True)
            raise
        for c in batch:
            forms[c.call][c.form] = forms[c.call].get(c.form, 0) + 1
        for t in seen:
            tables[t] = tables.get(t, 0) + 1
        cases += len(batch)
        index += 4
    print("nearest fuzz ok: %d cases in %.0f s, forms %s, tables (mode, formula, pin_last, implicit) %s" % (
        cases, time.time() - t0, forms, tables), flush=True)
    return {"cases": cases, "forms": forms, "tables": tables}


def main():
    run(float(sys.argv[1]) if len(sys.argv) > 1 else 120.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1)


if __name__ == "__main__":
    main()
