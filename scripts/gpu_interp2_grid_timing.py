"""Timing of the gridded bilinear call (Grid2.interp_grid = mi_interp2_grid_f64_dev) on one MI355X, against the same
outputs through the scattered call (pairs materialised on the device beforehand, untimed) and the CPU oracle on the
meshgrid pairs (OpenMP).  Every gridded result is checked bit for bit against the scattered one and the oracle.

Shapes:
  A   table 1024^2 (uniform axes, quad cells), XI = 16384, YI = 8192 sorted: 1.07 GB written
  B   the config-3 table (4096^2, synth.config3_table), quad cells and column pairs, XI = YI = 8192 sorted
  C   shape A with XI and YI randomly permuted
  D   thin outputs: nyi = 1, nxi = 1e8 and nxi = 1, nyi = 1e8
Per shape: median of --reps launches after --warmup, each launch between two device events (the locate pass and the grid
kernel); algorithmic bytes = 8*nxi*nyi + 8*(nxi+nyi) + 8*nx*ny (the table once, in input layout) over that time as a
fraction of 8 TB/s.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` with --no-cpu (a separate run).

  python3 scripts/gpu_interp2_grid_timing.py [--reps 20] [--warmup 3] [--no-cpu] [--shapes A,B,C,D]
"""
import argparse
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


def shapes(sel):
    out = []
    if "A" in sel:
        out.append(("A", 1024, False, 16384, 8192, False))
    if "B" in sel:
        out.append(("B_quad", 4096, False, 8192, 8192, False))
        out.append(("B_compact", 4096, True, 8192, 8192, False))
    if "C" in sel:
        out.append(("C", 1024, False, 16384, 8192, True))
    if "D" in sel:
        out.append(("D_row", 1024, False, 100_000_000, 1, False))
        out.append(("D_col", 1024, False, 1, 100_000_000, False))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU oracle (and the bit check against it)")
    ap.add_argument("--shapes", default="A,B,C,D")
    args = ap.parse_args()
    import numpy as np
    import torch

    import armadillocudalinearinterpolation_amd as mi
    from armadillocudalinearinterpolation_amd import synth

    ctx = mi.Context(0)
    dev = torch.device("cuda:0")
    nthreads = min(16, os.cpu_count() or 1)
    print(json.dumps({"device": ctx.device_info(), "cpu_threads": nthreads, "nproc": os.cpu_count(),
                      "reps": args.reps, "warmup": args.warmup}), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1234)
    for name, n, compact, nxi, nyi, permute in shapes(args.shapes.split(",")):
        z = synth.config3_table(n, dev)
        grid = mi.Grid2.uniform(ctx, 0.0, 1.0 / (n - 1), n, 0.0, 1.0 / (n - 1), n, z, compact=compact)
        # sorted queries over [-0.01, 1.01]: a few out of range on both ends
        xi = torch.linspace(-0.01, 1.01, nxi, dtype=torch.float64, device=dev)
        yi = torch.linspace(-0.01, 1.01, nyi, dtype=torch.float64, device=dev)
        if permute:
            xi = xi[torch.randperm(nxi, generator=gen, device=dev)].contiguous()
            yi = yi[torch.randperm(nyi, generator=gen, device=dev)].contiguous()
        out = torch.empty((nxi, nyi), dtype=torch.float64, device=dev)
        ms, lo, hi = _median_ms(lambda: grid.interp_grid(xi, yi, out=out), args.reps, args.warmup)
        alg = 8.0 * nxi * nyi + 8.0 * (nxi + nyi) + 8.0 * n * n
        rec = {"shape": name, "table": "%d^2 %s" % (n, "pairs" if compact else "quads"), "nxi": nxi, "nyi": nyi,
               "permuted": permute, "grid_ms_median": ms, "grid_ms_min": lo, "grid_ms_max": hi,
               "alg_bytes": alg, "alg_frac_8TBs": alg / (ms * 1e-3) / HBM_PEAK}
        grid_out = out.T.cpu().numpy()
        # the same outputs through the scattered call, the pairs materialised beforehand (untimed)
        px = xi.repeat_interleave(nyi)
        py = yi.repeat(nxi)
        zs = torch.empty_like(px)
        sms, _, _ = _median_ms(lambda: grid.interp(px, py, out=zs), args.reps, args.warmup)
        rec["scattered_ms_median"] = sms
        rec["speedup_vs_scattered"] = sms / ms
        sc = zs.cpu().numpy().reshape(nyi, nxi, order="F")
        rec["bit_equal_scattered"] = bool(np.array_equal(grid_out, sc, equal_nan=True))
        del px, py, zs
        if not args.no_cpu:
            import oracle
            zh = z.cpu().numpy().reshape(n, n).T          # (ny, nx)
            XX, YY = np.meshgrid(xi.cpu().numpy(), yi.cpu().numpy())
            pxh, pyh = XX.ravel("F"), YY.ravel("F")
            del XX, YY
            t0 = time.perf_counter()
            ref = oracle.interp2_bilinear_uniform(0.0, 1.0 / (n - 1), n, 0.0, 1.0 / (n - 1), n, zh, pxh, pyh,
                                                  nthreads=nthreads)
            rec["cpu_oracle_s"] = time.perf_counter() - t0
            rec["bit_equal_oracle"] = bool(np.array_equal(grid_out, ref.reshape(nyi, nxi, order="F"), equal_nan=True))
            del ref, pxh, pyh
        print(json.dumps(rec), flush=True)
        del out, grid_out, grid, z
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
