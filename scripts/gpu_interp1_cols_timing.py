"""Timing of interp1 over the columns of a matrix (Axis1.interp_cols = mi_interp1_cols_f64_dev) on one MI355X, against
the only route to the same outputs the library had before it: a compact mi_grid2 with Z = Y and the column number as the
x axis (Grid2, column pairs), evaluated by the gridded bilinear call at XI = 0, 1, .., B-1.  The table build of that route
is timed separately and not counted against it.  Every timed result is checked bit for bit: the new call against the
grid2 route on every output (finite data, so the two agree), and -- unless --no-cpu -- against the CPU oracle column by
column (oracle.interp1_bracket on every column).

Shapes:
  S1  n = 1024, B = 125 000, XI = 2048 sorted points spanning the axis (1.02 GB read, 2.05 GB written)   [LDS form]
  S2  S1 with XI permuted
  S3  n = 1e6, B = 64, XI = 1e6 sorted                                                                   [direct form]
  S4  B = 1, n = 1e6, nxi = 1e8 random: the degenerate case, beside Grid1.interp (mi_interp1_f64_dev) on the same table
Per shape: median (and min, max) of --reps launches after --warmup, each launch (locate pass + column kernel) between two
device events; algorithmic bytes = 8*n*B + 8*nxi*B + 8*nxi over that time as a fraction of 8 TB/s.  Kernel times: run
this under `rocprofv3 --kernel-trace --stats` with --no-cpu --no-yardstick (a separate run); counters in a run of their own.

  python3 scripts/gpu_interp1_cols_timing.py [--reps 20] [--warmup 3] [--no-cpu] [--no-yardstick] [--shapes S1,S2,S3,S4]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def _median_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def _bits_equal(a, b):
    import torch
    return bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


SHAPES = {
    # name: (n, B, nxi, queries)
    "S1": (1024, 125_000, 2048, "sorted"),
    "S2": (1024, 125_000, 2048, "permuted"),
    "S3": (1_000_000, 64, 1_000_000, "sorted"),
    "S4": (1_000_000, 1, 100_000_000, "random"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU oracle (and the bit check against it)")
    ap.add_argument("--no-yardstick", action="store_true", help="skip the grid2 route (and the bit check against it)")
    ap.add_argument("--shapes", default="S1,S2,S3,S4")
    args = ap.parse_args()
    import numpy as np
    import torch

    import armadillocudalinearinterpolation_amd as mi
    from armadillocudalinearinterpolation_amd.api import MI_GRID2_COMPACT, MI_GRID_DEVICE_PTRS, Grid2, check

    ctx = mi.Context(0)
    dev = torch.device("cuda:0")
    nthreads = min(16, os.cpu_count() or 1)
    print(json.dumps({"device": ctx.device_info(), "cpu_threads": nthreads, "reps": args.reps, "warmup": args.warmup}),
          flush=True)
    gen = torch.Generator(device=dev).manual_seed(1234)
    for name in args.shapes.split(","):
        n, B, nxi, order = SHAPES[name]
        X = np.linspace(0.0, 1.0, n)
        axis = mi.Axis1.from_nodes(ctx, X)
        Yb = torch.rand((B, n), generator=gen, dtype=torch.float64, device=dev) * 2.0 - 1.0   # column c = Yb[c]
        if order == "random":
            xi = torch.rand(nxi, generator=gen, dtype=torch.float64, device=dev) * 1.02 - 0.01
        else:
            xi = torch.linspace(-0.01, 1.01, nxi, dtype=torch.float64, device=dev)   # a few out of range on both ends
            if order == "permuted":
                xi = xi[torch.randperm(nxi, generator=gen, device=dev)].contiguous()
        outb = torch.empty((B, nxi), dtype=torch.float64, device=dev)
        ms, lo, hi = _median_ms(lambda: axis.interp_cols(Yb.T, xi, out=outb.T), args.reps, args.warmup)
        alg = 8.0 * n * B + 8.0 * nxi * B + 8.0 * nxi
        rec = {"shape": name, "n": n, "B": B, "nxi": nxi, "queries": order, "form": "lds" if n <= 8192 else "direct",
               "cols_ms_median": ms, "cols_ms_min": lo, "cols_ms_max": hi, "alg_bytes": alg,
               "alg_frac_8TBs": alg / (ms * 1e-3) / HBM_PEAK}
        if name == "S4":
            # the single-table call on the same table and queries
            g1 = mi.Grid1.from_nodes(ctx, X, Yb[0].cpu().numpy(), sanitise=False)
            o1 = torch.empty_like(xi)
            m1, l1, h1 = _median_ms(lambda: g1.interp(xi, out=o1), args.reps, args.warmup)
            rec.update({"interp1_ms_median": m1, "interp1_ms_min": l1, "interp1_ms_max": h1, "cols_over_interp1": ms / m1,
                        "bit_equal_interp1": _bits_equal(o1, outb[0])})
            g1.close()
            del o1
        if not args.no_yardstick:
            # the grid2 route: x axis = column number, y axis = X, Z(y_i, x_c) = Y[i, c]; device pointers throughout
            cx = torch.arange(B if B > 1 else 2, dtype=torch.float64, device=dev)
            Xd = torch.from_numpy(X).to(dev)
            Z = Yb if B > 1 else torch.cat([Yb, Yb])          # a grid2 needs two columns
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = C.c_void_p()
            check(ctx._L.mi_grid2_create(ctx._h, C.c_void_p(cx.data_ptr()), cx.numel(), C.c_void_p(Xd.data_ptr()), n,
                                         C.c_void_p(Z.data_ptr()), MI_GRID_DEVICE_PTRS | MI_GRID2_COMPACT, C.byref(h)), ctx._h)
            ctx.synchronize()
            rec["grid2_build_s"] = time.perf_counter() - t0
            g2 = Grid2(ctx, h)
            cq = cx[:B].contiguous()
            out2 = torch.empty((B, nxi), dtype=torch.float64, device=dev)
            m2, l2, h2 = _median_ms(lambda: g2.interp_grid(cq, xi, out=out2), args.reps, args.warmup)
            rec.update({"grid2_ms_median": m2, "grid2_ms_min": l2, "grid2_ms_max": h2, "cols_over_grid2": ms / m2,
                        "grid2_table_bytes": g2.info()["table_bytes"], "bit_equal_grid2": _bits_equal(outb, out2)})
            g2.close()
            del out2, Z
        if not args.no_cpu:
            import oracle
            Yh, got, xih = Yb.cpu().numpy(), outb.cpu().numpy(), xi.cpu().numpy()
            t0 = time.perf_counter()
            ok = True
            for c in range(B):
                ok = ok and np.array_equal(got[c], oracle.interp1_bracket(X, Yh[c], xih, np.nan, nthreads=nthreads if B < 256 else 1),
                                           equal_nan=True)
            rec["cpu_oracle_s"] = time.perf_counter() - t0
            rec["bit_equal_oracle"] = bool(ok)
            del Yh, got, xih
        print(json.dumps(rec), flush=True)
        axis.close()
        del Yb, outb, xi
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
