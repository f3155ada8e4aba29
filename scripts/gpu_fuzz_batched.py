"""Differential fuzz of the seven batched device calls (interp_cols, interp_rows / interp_stack, interp_pairs, interp_each,
interp_rowpairs, Grid2.interp_grid, interp2_slices) against the CPU oracle, with guarded canvases around every operand
(run on the GPU box).  The generator, the reference and the check are tests/batched_fuzz_cases.py; this file holds the
device side -- upload the canvases, make the strided views, enqueue the calls, read everything back -- which
tests/test_batched_fuzz_gpu.py uses for the fixed cases, and run(), the long run by hand with other seeds."""
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


class Staged:
    """one case on the device: dev the canvases, view the strided operand views, handles the axes / grid, made before any
    call of the batch is enqueued (creating a handle uploads and may synchronise; the calls themselves must not)"""

    def __init__(self, ctx, c):
        import armadillocudalinearinterpolation_amd as mi
        self.case, self.ctx = c, ctx
        self.dev = {name: torch.from_numpy(a).cuda() for name, a in F.canvases(c).items()}
        self.view = {}
        for name, op in c.ops.items():
            t = self.dev[name]
            assert t.data_ptr() % 256 == 0, "a canvas is not 256-B aligned"
            if op.cols == 1 and op.S == 1 and name in ("xi", "yi", "lens"):
                self.view[name] = t[op.start:op.start + op.rows]
            elif c.call == "grid":                               # ZI: the dense (nxi, nyi) buffer interp_grid takes
                self.view[name] = t[op.start:op.start + op.rows * op.cols].view(op.cols, op.rows)
            elif name in ("Z", "ZI"):
                self.view[name] = torch.as_strided(t, (op.rows, op.cols, op.S), (1, op.ld, op.stride), op.start)
            else:
                self.view[name] = torch.as_strided(t, (op.rows, op.cols), (1, op.ld), op.start)
            if name != "lens":
                assert (self.view[name].data_ptr() % 16 != 0) == bool(op.base)
        self.h = {}
        if c.call == "grid":
            ax, ay = c.axes["ax"], c.axes["ay"]
            if ax["kind"] == "uniform":
                self.h["g"] = mi.Grid2.uniform(ctx, ax["x0"], ax["dx"], ax["nodes"].size, ay["x0"], ay["dx"], ay["nodes"].size,
                                               np.ascontiguousarray(c.arrays["Z"][:, :, 0]))
            else:
                self.h["g"] = mi.Grid2.from_axes(ctx, ax["nodes"], ay["nodes"], c.arrays["Z"][:, :, 0])
        else:
            for key, ax in c.axes.items():
                self.h[key] = (mi.Axis1.uniform(ctx, ax["x0"], ax["dx"], ax["nodes"].size) if ax["kind"] == "uniform"
                               else mi.Axis1.from_nodes(ctx, ax["nodes"]))
        self.flags = None
        self.before = self.after = None

    def _counters(self):
        c = self.case
        if c.counter is None:
            return None
        name, n = F.COUNTERS[F.COUNTER_CALL[c.call]]
        return [int(getattr(self.ctx._L, name)(f)) for f in range(n)]

    def enqueue(self):
        """the call, asynchronous on the context's stream; the status is held by check() of api.py: anything but MI_OK raises"""
        import armadillocudalinearinterpolation_amd as mi
        c, v, ctx, e = self.case, self.view, self.ctx, self.case.extrap
        self.before = self._counters()
        if c.call == "cols":
            r = self.h["x"].interp_cols(v["Y"], v["xi"], out=v["YI"], extrap=e)
        elif c.call == "rows":
            r = self.h["x"].interp_rows(v["Y"], v["xi"], out=v["YI"], extrap=e)
        elif c.call == "stack":
            r = self.h["x"].interp_stack(v["Z"], v["xi"], out=v["ZI"], extrap=e)
        elif c.call == "grid":
            r = self.h["g"].interp_grid(v["xi"], v["yi"], out=v["ZI"], extrap=e)
        elif c.call == "slices2":
            r = mi.interp2_slices(ctx, self.h["ax"], self.h["ay"], v["Z"], v["xi"], v["yi"], out=v["ZI"], extrap=e)
        else:
            lens = v.get("lens")
            if c.call == "pairs":
                r = mi.interp_pairs(ctx, v["X"], v["Y"], v["xi"], lens=lens, out=v["YI"], extrap=e, want_ok=c.use_ok)
            elif c.call == "rowpairs":
                r = mi.interp_rowpairs(ctx, v["X"], v["Y"], v["xi"], lens=lens, out=v["YI"], extrap=e, want_ok=c.use_ok)
            else:
                r = mi.interp_each(ctx, v["X"], v["Y"], v["XI"] if "XI" in v else v["xi"], lens=lens, out=v["YI"], extrap=e,
                                   want_ok=c.use_ok)
            if c.use_ok:
                r, self.flags = r
        self.after = self._counters()
        out = v[c.out]
        assert r.data_ptr() == out.data_ptr(), "%s: the call did not write into the given out" % c.id

    def finish(self):
        """after the synchronisation: read every canvas back and check"""
        got = {name: t.cpu().numpy() for name, t in self.dev.items()}
        F.check(self.case, got, None if self.flags is None else self.flags.cpu().numpy(), self.before, self.after)
        for h in self.h.values():
            h.close()


def run_batch(ctx, cases):
    """stage the cases, enqueue their calls in order with no synchronisation between them, synchronise once, check each"""
    staged = [Staged(ctx, c) for c in cases]
    for s in staged:
        s.enqueue()
    ctx.synchronize()
    torch.cuda.synchronize()
    for s in staged:
        s.finish()


def run(budget, seed, ctx=None):
    """rounds of one case per call (the eight calls enqueued back to back: the context's scratch slot serves calls of
    growing and shrinking size) until the budget, in seconds, is spent; seed: any but the suite's fixed one"""
    import armadillocudalinearinterpolation_amd as mi
    ctx = ctx or mi.Context(0)
    t0, cases, forms = time.time(), 0, {call: {} for call in F.CALLS}
    beat, index = t0, 0
    while time.time() - t0 < budget:
        if time.time() - beat > 60.0:          # a sign of life every minute (a silent GPU command is taken to be hung)
            beat = time.time()
            print("  ... %d cases after %.0f s" % (cases, beat - t0), flush=True)
        batch = [F.case(call, index, seed) for call in F.CALLS]
        try:
            run_batch(ctx, batch)
        except AssertionError:
            print("MISMATCH in round %d of seed %d: batched_fuzz_cases.case(call, %d, %d) reproduces it" % (index, seed, index, seed), flush=True)
            raise
        for c in batch:
            forms[c.call][c.form] = forms[c.call].get(c.form, 0) + 1
        cases += len(batch)
        index += 1
    print("fuzz ok: %d cases in %.0f s, forms %s" % (cases, time.time() - t0, forms), flush=True)
    return {"cases": cases, "forms": forms}


def main():
    run(float(sys.argv[1]) if len(sys.argv) > 1 else 120.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1)


if __name__ == "__main__":
    main()
