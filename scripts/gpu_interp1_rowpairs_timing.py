"""Timing of interp1 over paired rows (mi.interp_rowpairs = mi_interp1_rowpairs_f64_dev) on one MI355X, beside the route
it replaces and the floor of the layout, alternated in one process on the same build.

X and Y are column-major m x n (one table per row, an X per row; on the device C-contiguous (n, m) buffers), XI holds nxi
queries shared by every row, YI is m x nxi.  X is each row's own cumulative jittered times.
  (a) rowpairs   the new call.
  (b) transpose  torch transposes X and Y into contiguous (m, n) buffers, mi.interp_pairs runs on them (mi.interp_each
                 with one shared XI on Q3, the way to the thin kernel), torch transposes the (nxi x m) result back: timed
                 in full, and the middle call alone ("pairs_only").
  (c) rows       Axis1.interp_rows on the same Y with ONE shared axis (row 0 of X).  It does not compute the same thing;
                 it is the floor this layout has reached.
Shapes:
  Q1  m = 125 000, n = 1024 onto 2048 sorted points
  Q2  Q1 with the same queries permuted
  Q3  m = 1 000 000, n = 2, nxi = 1: the Restrict shape
  Q4  downsampling: m = 125 000, n = 2048 onto 256 sorted points
  Q5  few long rows: m = 8, n = 100 000 onto 1 000 000 sorted points (a lane per row leaves the machine empty)
Queries: a uniform sorted mesh over the range every row covers, one NaN and one point below every range among them.
Method: --reps repetitions after --warmup, the routes alternated inside every repetition, each call between two device
events; median, min and max are reported.  Before anything is timed the result of (a) must equal that of (b) bit for bit
(NaN == NaN).  Algorithmic bytes = 8 * (2 * m * n_bracketed + m * nxi), n_bracketed the mean number of nodes of a row
that a query brackets (over 64 rows spread over the matrix; for Q2 that of the same queries sorted); the share is that
over 8 TB/s over the median.  The form (a) took is read from mi_debug_rowpairs_launches.
Every shape runs in a process of its own under its own time limit (--limit seconds); the first one that fails or runs
out of time ends the whole run, nothing is started after it.

  python3 scripts/gpu_interp1_rowpairs_timing.py [--reps 10] [--warmup 2] [--shapes Q1,Q2,Q3,Q4,Q5] [--limit 240] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
FORMS = ["short_rows", "long_rows"]
SHAPES = {   # name: (m, n, nxi, permuted)
    "Q1": (125_000, 1024, 2048, False),
    "Q2": (125_000, 1024, 2048, True),
    "Q3": (1_000_000, 2, 1, False),
    "Q4": (125_000, 2048, 256, False),
    "Q5": (8, 100_000, 1_000_000, False),
    "tiny": (1300, 40, 90, False),                # rehearsal sizes
    "tiny_permuted": (300, 16, 300, True),
    "tiny_restrict": (5000, 2, 1, False),
}


def bracketed_nodes(Xs, xi):
    """mean number of nodes of a row that at least one in-range query brackets; Xs: (rows, n) sample"""
    import numpy as np
    counts = []
    for X in Xs:
        q = xi[(xi >= X[0]) & (xi <= X[-1])]
        left = np.minimum(np.searchsorted(X, q, side="right") - 1, X.size - 1)
        right = np.minimum(left + 1, X.size - 1)
        counts.append(np.union1d(left, right).size)
    return float(np.mean(counts))


def run_shape(name, reps, warmup):
    import numpy as np
    import torch
    import armadillocudalinearinterpolation_amd as mi
    if not torch.cuda.is_available():
        raise SystemExit("gpu_interp1_rowpairs_timing.py needs a GPU (there is no CPU fallback)")
    ctx = mi.Context(0)
    m, n, nxi, permuted = SHAPES[name]
    L = ctx._L
    gen = torch.Generator(device="cuda").manual_seed(5)
    # node k of every row = row k of the buffer; increments in [0.5, 1): each row its own cumulative jittered times
    Xbuf = torch.cumsum(torch.rand((n, m), dtype=torch.float64, device="cuda", generator=gen) * 0.5 + 0.5, dim=0)
    Ybuf = torch.randn((n, m), dtype=torch.float64, device="cuda", generator=gen)
    lo, hi = float(Xbuf[0].max()), float(Xbuf[-1].min())
    assert lo < hi, "the rows have no common range"
    rng = np.random.default_rng(12)
    xi = np.linspace(lo, hi, nxi) if nxi > 1 else np.array([0.5 * (lo + hi)])
    if nxi >= 8:
        xi[1], xi[2] = np.nan, float(Xbuf[0].min()) - 1.0
    sample = Xbuf[:, torch.linspace(0, m - 1, min(m, 64), device="cuda").long()].T.cpu().numpy()
    nodes = bracketed_nodes(sample, xi)
    if permuted:
        xi = rng.permutation(xi)
    xd = torch.from_numpy(xi).cuda()
    axis = mi.Axis1.from_device_nodes(ctx, Xbuf[:, 0].contiguous())
    X, Y = Xbuf.T, Ybuf.T
    out_a = torch.empty((nxi, m), dtype=torch.float64, device="cuda")
    out_b = torch.empty((nxi, m), dtype=torch.float64, device="cuda")
    out_c = torch.empty((nxi, m), dtype=torch.float64, device="cuda")
    Xt = torch.empty((m, n), dtype=torch.float64, device="cuda")
    Yt = torch.empty((m, n), dtype=torch.float64, device="cuda")
    tmp = torch.empty((m, nxi), dtype=torch.float64, device="cuda")
    thin = n <= 32 and nxi <= 8                        # interp_each's thin kernel (kThinMaxN, kThinMaxQ in csrc/mi_each1.hip)

    def rowpairs():
        mi.interp_rowpairs(ctx, X, Y, xd, out=out_a.T)

    def pairs_only():
        if thin:
            mi.interp_each(ctx, Xt.T, Yt.T, xd, out=tmp.T)
        else:
            mi.interp_pairs(ctx, Xt.T, Yt.T, xd, out=tmp.T)

    def transpose():
        Xt.copy_(Xbuf.T)
        Yt.copy_(Ybuf.T)
        pairs_only()
        out_b.copy_(tmp.T)

    def rows():
        axis.interp_rows(Y, xd, out=out_c.T)

    before = [int(L.mi_debug_rowpairs_launches(f)) for f in range(2)]
    rowpairs()
    form = FORMS[[int(L.mi_debug_rowpairs_launches(f)) - b for f, b in enumerate(before)].index(1)]
    transpose()
    rows()
    torch.cuda.synchronize()
    same = lambda p, q: bool(torch.equal(torch.nan_to_num(p, nan=1e300), torch.nan_to_num(q, nan=1e300)))  # noqa: E731
    assert same(out_a, out_b), "%s: interp_rowpairs differs from the paired-column call on the transposed data" % name
    bytes_ = int(8 * (2 * m * nodes + m * nxi))
    res = {"shape": name, "m": m, "n": n, "nxi": nxi, "permuted": permuted, "form": form, "middle_call": "interp_each" if thin else "interp_pairs",
           "bit_equal_to_pairs_on_transpose": True, "nodes_bracketed_per_row": round(nodes, 2), "algorithmic_bytes": bytes_,
           "nan_fraction": round(float(torch.isnan(out_a).double().mean()), 5), "device": ctx.device_info()}
    routes = (("rowpairs", rowpairs), ("transpose", transpose), ("pairs_only", pairs_only), ("rows", rows))
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
    for key in ("transpose", "pairs_only", "rows"):
        res[key + "_over_rowpairs"] = round(res[key + "_ms"]["median"] / res["rowpairs_ms"]["median"], 3)
    axis.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="Q1,Q2,Q3,Q4,Q5")
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(run_shape(args.child, args.reps, args.warmup)), flush=True)
        return
    results = []
    for name in args.shapes.split(","):
        # a process and a time limit per shape; this process never opens the GPU itself
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", name,
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit("%s ended with status %d: nothing is run after it" % (name, done.returncode))
        r = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"reps": args.reps, "warmup": args.warmup, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
