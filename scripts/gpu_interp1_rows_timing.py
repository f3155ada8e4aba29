"""Timing of interp1 along the rows of a matrix (Axis1.interp_rows / interp_stack = mi_interp1_rows_f64_dev) on one
MI355X, beside the two routes that existed before it, alternated in one process on the same build.

Y is column-major m x n (one table per row; on the device a C-contiguous (n, m) buffer), XI holds nxi queries, YI is m x nxi.
  (a) rows       the new call: one locate launch, one rows kernel.
  (b) transpose  torch transposes Y into a contiguous (m, n) buffer, Axis1.interp_cols runs on it, torch transposes the
                 (nxi x m) result back: timed in full, and the interp_cols call alone ("cols_only").
  (c) slices     mi.interp2_slices on ONE slice with a uniform axis over the row number and yi = 0..m-1: four corners per
                 output, 16-B records per row.  (Not bit-equal to interp1 once a row holds inf or NaN; the data here are
                 finite, and its equality with (a) is reported, not required.)
Shapes:
  R1  m = 125 000, n = 1024 onto 2048 sorted points (3.07 GB: the transposed S1 of DESIGN.md 4.8)
  R2  R1 with the same queries permuted
  R3  a cube of 512 x 512 fields at 64 levels onto 128 sorted times (m = 262 144; (a) goes through interp_stack)
  R4  downsampling: m = 125 000, n = 2048 onto 256 sorted points (most columns of Y are bracketed by no query)
  R5  thin: m = 8, n = 100 000 onto 1 000 000 sorted points (flat body)
Queries: a uniform sorted mesh over the axis ending on its last node, one NaN and one point below the range among them.
Method: --reps repetitions after --warmup, the routes alternated inside every repetition, each call between two device
events; median, min and max are reported.  Before anything is timed the result of (a) must equal that of (b) bit for bit
(NaN == NaN).  Algorithmic bytes = 8 * m * (columns of Y that a query brackets + nxi) -- for R2 that of the same queries
sorted; the share is that over 8 TB/s over the median.  The form (a) took is read from mi_debug_rows1_launches.

  python3 scripts/gpu_interp1_rows_timing.py [--reps 10] [--warmup 2] [--shapes R1,R2,R3,R4,R5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
FORMS = ["tile_16B", "tile_8B", "flat"]
SHAPES = {   # name: (m, n, nxi, permuted, cube (ny, nx) or None)
    "R1": (125_000, 1024, 2048, False, None),
    "R2": (125_000, 1024, 2048, True, None),
    "R3": (512 * 512, 64, 128, False, (512, 512)),
    "R4": (125_000, 2048, 256, False, None),
    "R5": (8, 100_000, 1_000_000, False, None),
    "tiny": (1300, 16, 40, False, None),          # rehearsal sizes
    "tiny_thin": (4, 50, 300, True, None),
    "tiny_cube": (6 * 50, 5, 9, False, (6, 50)),
}


def bracketed_columns(X, xi):
    """number of columns of Y that at least one in-range query brackets"""
    import numpy as np
    q = xi[(xi >= X[0]) & (xi <= X[-1])]
    left = np.searchsorted(X, q, side="right") - 1
    left = np.minimum(left, X.size - 1)
    right = np.minimum(left + 1, X.size - 1)
    return int(np.union1d(left, right).size)


def run_shape(mi, ctx, name, reps, warmup):
    import numpy as np
    import torch
    m, n, nxi, permuted, cube = SHAPES[name]
    L = ctx._L
    rng = np.random.default_rng(12)
    X = np.cumsum(rng.uniform(0.5, 1.0, n))
    xi = np.linspace(X[0], X[-1], nxi)
    xi[-1] = X[-1]
    if nxi >= 8:
        xi[1], xi[2] = np.nan, X[0] - 1.0
    ncols = bracketed_columns(X, xi)
    if permuted:
        xi = rng.permutation(xi)
    gen = torch.Generator(device="cuda").manual_seed(5)
    Ybuf = torch.randn((n, m), dtype=torch.float64, device="cuda", generator=gen)      # column k of Y = row k of the buffer
    Y = Ybuf.T
    xd = torch.from_numpy(xi).cuda()
    axis = mi.Axis1.from_nodes(ctx, X)
    rows_axis = mi.Axis1.uniform(ctx, 0.0, 1.0, m)
    rows_q = torch.arange(m, dtype=torch.float64, device="cuda")
    out_a = torch.empty((nxi, m), dtype=torch.float64, device="cuda")
    out_b = torch.empty((nxi, m), dtype=torch.float64, device="cuda")
    out_c = torch.empty((nxi, m), dtype=torch.float64, device="cuda")
    Yt = torch.empty((m, n), dtype=torch.float64, device="cuda")
    tmp = torch.empty((m, nxi), dtype=torch.float64, device="cuda")

    if cube:
        ny, nx = cube
        Z = Ybuf.view(n, nx, ny).permute(2, 1, 0)
        out_a3 = out_a.view(nxi, nx, ny).permute(2, 1, 0)

        def rows():
            axis.interp_stack(Z, xd, out=out_a3)
    else:
        def rows():
            axis.interp_rows(Y, xd, out=out_a.T)

    def cols_only():
        axis.interp_cols(Yt.T, xd, out=tmp.T)

    def transpose():
        Yt.copy_(Ybuf.T)
        cols_only()
        out_b.copy_(tmp.T)

    def slices():
        mi.interp2_slices(ctx, axis, rows_axis, Ybuf.view(1, n, m).permute(2, 1, 0), xd, rows_q,
                          out=out_c.view(1, nxi, m).permute(2, 1, 0))

    before = [int(L.mi_debug_rows1_launches(f)) for f in range(3)]
    rows()
    form = FORMS[[int(L.mi_debug_rows1_launches(f)) - b for f, b in enumerate(before)].index(1)]
    transpose()
    slices()
    torch.cuda.synchronize()
    same = lambda p, q: bool(torch.equal(torch.nan_to_num(p, nan=1e300), torch.nan_to_num(q, nan=1e300)))  # noqa: E731
    assert same(out_a, out_b), "%s: interp_rows differs from interp_cols on the transposed data" % name
    res = {"shape": name, "m": m, "n": n, "nxi": nxi, "permuted": permuted, "form": form, "bit_equal_to_cols_on_transpose": True,
           "equal_to_one_slice_interp2": same(out_a, out_c), "columns_bracketed": ncols,
           "nan_fraction": round(float(torch.isnan(out_a).double().mean()), 5)}
    bytes_ = 8 * m * (ncols + nxi)
    res["algorithmic_bytes"] = bytes_
    routes = (("rows", rows), ("transpose", transpose), ("cols_only", cols_only), ("slices", slices))
    times = {k: [] for k, _ in routes}
    for rep in range(warmup + reps):
        for key, fn in routes:                           # alternated: every repetition runs every route once
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[key].append(a.elapsed_time(b))
    for key, _ in routes:
        med = statistics.median(times[key])
        res[key + "_ms"] = {"median": round(med, 4), "min": round(min(times[key]), 4), "max": round(max(times[key]), 4)}
        res[key + "_share_of_8TBps"] = round(bytes_ / HBM_PEAK / (med * 1e-3), 4)
    for key in ("transpose", "cols_only", "slices"):
        res[key + "_over_rows"] = round(res[key + "_ms"]["median"] / res["rows_ms"]["median"], 3)
    axis.close()
    rows_axis.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="R1,R2,R3,R4,R5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import armadillocudalinearinterpolation_amd as mi
    if not torch.cuda.is_available():
        raise SystemExit("gpu_interp1_rows_timing.py needs a GPU (there is no CPU fallback)")
    ctx = mi.Context(0)
    info = ctx.device_info()
    print(json.dumps({"device": info, "reps": args.reps, "warmup": args.warmup}), flush=True)
    results = []
    for name in args.shapes.split(","):
        r = run_shape(mi, ctx, name, args.reps, args.warmup)
        print(json.dumps(r), flush=True)
        results.append(r)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": info, "reps": args.reps, "warmup": args.warmup, "results": results}, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
