"""Timing of gridded interp2 over the slices of a cube (mi.interp2_slices = mi_interp2_slices_f64_dev) on one MI355X,
beside the routes that existed before it, measured in the same process on the same build.

For each shape (slices of ny x nx -> nyi x nxi):
  (a) slices    the new call: one locate launch, one slice kernel, Z read where it lies.
  (b) rebuild   per slice: mi_grid2_create(MI_GRID_DEVICE_PTRS) + mi_interp2_grid_f64_dev + mi_grid2_destroy -- the only
                route to a Z that changes on the device without the new call (an allocation, a repacking pass and a
                stream synchronisation per slice).
  (c) resident  for information: mi_interp2_grid_f64_dev alone per slice, on tables built beforehand (what (b) would cost
                if Z never changed).
Shapes: many64 = 4096 slices of 64^2 -> 128^2; big2048 = 8 slices of 2048^2 -> 4096^2; zoom64 = 1 slice of 64^2 -> 4096^2.
Queries: sorted uniform meshes spanning the table (regridding), one NaN and one out-of-range point per axis.
Method: median (and min, max) of --reps repetitions after --warmup, each between two device events on the context's
stream ((b) synchronises inside, so its events bracket host time too); the result of (a) is compared bit for bit with
(c) on the first and the last slice before anything is timed.  Algorithmic bytes = Z read once + ZI written once; the
share is that over 8 TB/s over the median.  The form (a) took is read from mi_debug_slices2_launches.

  python3 scripts/bench_interp2_slices.py [--reps 10] [--warmup 2] [--shapes many64,big2048,zoom64] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
FORMS = ["lds_tile", "lds_flat", "direct_tile", "direct_flat"]
SHAPES = {   # name: (ny, nx, nyi, nxi, slices)
    "many64": (64, 64, 128, 128, 4096),
    "big2048": (2048, 2048, 4096, 4096, 8),
    "zoom64": (64, 64, 4096, 4096, 1),
    "tiny": (16, 16, 32, 32, 8),          # rehearsal size
}


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


def run_shape(mi, ctx, name, reps, warmup):
    import numpy as np
    import torch
    from armadillocudalinearinterpolation_amd._lib import check
    ny, nx, nyi, nxi, S = SHAPES[name]
    L = ctx._L
    rng = np.random.default_rng(12)
    xg, yg = np.cumsum(rng.uniform(0.5, 1.0, nx)), np.cumsum(rng.uniform(0.5, 1.0, ny))
    xi, yi = np.linspace(xg[0], xg[-1], nxi), np.linspace(yg[0], yg[-1], nyi)
    xi[-1], yi[-1] = xg[-1], yg[-1]
    if nxi >= 8 and nyi >= 8:
        xi[1], xi[2], yi[1], yi[2] = np.nan, xg[-1] + 1.0, np.nan, yg[0] - 1.0
    gen = torch.Generator(device="cuda").manual_seed(5)
    Zbuf = torch.randn((S, nx, ny), dtype=torch.float64, device="cuda", generator=gen)      # slice by slice, column-major
    Z = Zbuf.permute(2, 1, 0)
    xd, yd, xgd, ygd = (torch.from_numpy(a).cuda() for a in (xi, yi, xg, yg))
    ax, ay = mi.Axis1.from_nodes(ctx, xg), mi.Axis1.from_nodes(ctx, yg)
    out = torch.empty((S, nxi, nyi), dtype=torch.float64, device="cuda")
    out_v = out.permute(2, 1, 0)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    DEVICE_PTRS = 0x2
    math_nan = float("nan")

    def slices():
        mi.interp2_slices(ctx, ax, ay, Z, xd, yd, out=out_v)

    out_b = torch.empty((S, nxi, nyi), dtype=torch.float64, device="cuda")

    def rebuild():
        for s in range(S):
            g = C.c_void_p()
            check(L.mi_grid2_create(ctx._h, p(xgd), nx, p(ygd), ny, p(Zbuf[s]), DEVICE_PTRS, C.byref(g)), ctx._h)
            check(L.mi_interp2_grid_f64_dev(ctx._h, g, p(xd), nxi, p(yd), nyi, p(out_b[s]), math_nan), ctx._h)
            L.mi_grid2_destroy(g)

    grids = []
    for s in range(S):
        g = C.c_void_p()
        check(L.mi_grid2_create(ctx._h, p(xgd), nx, p(ygd), ny, p(Zbuf[s]), DEVICE_PTRS, C.byref(g)), ctx._h)
        grids.append(g)
    out_c = torch.empty((S, nxi, nyi), dtype=torch.float64, device="cuda")

    def resident():
        for s in range(S):
            check(L.mi_interp2_grid_f64_dev(ctx._h, grids[s], p(xd), nxi, p(yd), nyi, p(out_c[s]), math_nan), ctx._h)

    before = [int(L.mi_debug_slices2_launches(f)) for f in range(4)]
    slices()
    form = FORMS[[int(L.mi_debug_slices2_launches(f)) - b for f, b in enumerate(before)].index(1)]
    resident()
    rebuild()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(torch.nan_to_num(out[s], nan=1e300), torch.nan_to_num(o[s], nan=1e300)))
               for s in (0, S - 1) for o in (out_c, out_b))
    frac_nan = float(torch.isnan(out[0]).double().mean())
    res = {"shape": name, "ny": ny, "nx": nx, "nyi": nyi, "nxi": nxi, "slices": S, "form": form, "bit_equal_to_grid_call": same,
           "nan_fraction": round(frac_nan, 4)}
    bytes_ = 8 * S * (ny * nx + nyi * nxi)
    res["algorithmic_bytes"] = bytes_
    for key, fn in (("slices", slices), ("rebuild", rebuild), ("resident", resident)):
        med, lo, hi = _median_ms(fn, reps, warmup)
        res[key + "_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        res[key + "_share_of_8TBps"] = round(bytes_ / HBM_PEAK / (med * 1e-3), 4)
    res["rebuild_over_slices"] = round(res["rebuild_ms"]["median"] / res["slices_ms"]["median"], 3)
    res["resident_over_slices"] = round(res["resident_ms"]["median"] / res["slices_ms"]["median"], 3)
    for g in grids:
        L.mi_grid2_destroy(g)
    ax.close()
    ay.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="many64,big2048,zoom64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import armadillocudalinearinterpolation_amd as mi
    if not torch.cuda.is_available():
        raise SystemExit("bench_interp2_slices.py needs a GPU (there is no CPU fallback)")
    ctx = mi.Context(0)
    info = ctx.device_info()
    results = []
    for name in args.shapes.split(","):
        r = run_shape(mi, ctx, name, args.reps, args.warmup)
        print(json.dumps(r), flush=True)
        results.append(r)
    doc = {"device": info, "reps": args.reps, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
