"""Timing of interp1 over paired columns with a query vector per column (mi.interp_each = mi_interp1_each_f64_dev) on
one MI355X, beside the unchanged mi_interp1_pairs_f64_dev (mi.interp_pairs) measured in the same process on the same
build as the yardstick.

Shapes:
  P5, P5n8   the Restrict shape, n = 2 (and 8), B = 1e6, one query: the thin kernel with a shared XI (ldxi = 0) and with a
             query per column (ldxi > 0), against the existing call.  Condition on the thin form: at P5 with ldxi = 0 the
             new call's slowest repetition lies below the existing call's fastest ("thin_slowest_below_pairs_fastest").
  T<n>q<q>   sweep of n and nxi around the thin thresholds (kThinMaxN, kThinMaxQ in csrc/mi_each1.hip): the new call
             (thin wherever the dispatcher sends it there) against the existing call (its LDS form) on the same inputs
             with a shared XI, and the new call with per-column queries.  The crossover fixes the thresholds.
  P1e, P4e   P1 (n = 1024, B = 125 000, nxi = 2048, sorted per column) and P4 (n = 1e5, B = 640, nxi = 1e5) with
             per-column queries against the shared-XI call on the same X and Y: a floor, since that call moves
             8*nxi*B fewer bytes; reported as each / pairs beside the ratio of the bytes.
Method: per call, median (and min, max) of --reps launches after --warmup, each launch between two device events; every
timed result is checked bit for bit against the CPU oracle on --check-cols columns; the form that ran is read from
mi_debug_each_launches.  Algorithmic bytes = 16 n B + 8 nxi B (YI) + 8 nxi B (per-column XI) or 8 nxi (shared) + 4 B.

  python3 scripts/gpu_interp1_each_timing.py [--reps 20] [--warmup 3] [--shapes P5,P5n8,sweep,P1e,P4e]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
FORMS = ["thin", "lds", "direct", "forwarded"]


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


def _shapes(which, sweep_n, sweep_q):
    out = []
    for w in which.split(","):
        if w == "P5":
            out.append(("P5", 2, 1_000_000, 1, True))
        elif w == "P5n8":
            out.append(("P5n8", 8, 1_000_000, 1, True))
        elif w == "sweep":
            for n in sweep_n:
                for q in sweep_q:
                    out.append(("T%dq%d" % (n, q), n, min(1_000_000, (16 << 20) // max(n, q)), q, True))
        elif w == "P1e":
            out.append(("P1e", 1024, 125_000, 2048, True))
        elif w == "P4e":
            out.append(("P4e", 100_000, 640, 100_000, True))
        else:
            raise SystemExit("unknown shape %s" % w)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="P5,P5n8,sweep,P1e,P4e")
    ap.add_argument("--sweep-n", default="2,4,8,16,32,64")
    ap.add_argument("--sweep-q", default="1,2,4,8,16")
    ap.add_argument("--check-cols", type=int, default=8)
    args = ap.parse_args()
    import numpy as np
    import torch

    import armadillocudalinearinterpolation_amd as mi
    import oracle

    ctx = mi.Context(0)
    L = ctx._L
    dev = torch.device("cuda:0")
    print(json.dumps({"device": ctx.device_info(), "reps": args.reps, "warmup": args.warmup}), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1234)

    def form_of(fn):
        before = [int(L.mi_debug_each_launches(f)) for f in range(4)]
        fn()
        after = [int(L.mi_debug_each_launches(f)) for f in range(4)]
        hit = [FORMS[f] for f in range(4) if after[f] != before[f]]
        return hit[0] if len(hit) == 1 else str(hit)

    for name, n, B, nxi, _ in _shapes(args.shapes, [int(v) for v in args.sweep_n.split(",")], [int(v) for v in args.sweep_q.split(",")]):
        # nodes: jittered increments, every column with an offset of its own; column c = row c of the buffers
        Xb = torch.cumsum(torch.rand((B, n), generator=gen, dtype=torch.float64, device=dev) * 0.8 + 0.2, dim=1)
        Xb += torch.rand((B, 1), generator=gen, dtype=torch.float64, device=dev) * 4.0 - 2.0
        Yb = torch.rand((B, n), generator=gen, dtype=torch.float64, device=dev) * 2.0 - 1.0
        lo, hi = Xb[:, :1], Xb[:, n - 1:]
        # per-column queries: sorted along each column, 1 % of them on either side of the column's range
        Q = torch.sort(lo - 0.01 * (hi - lo) + torch.rand((B, nxi), generator=gen, dtype=torch.float64, device=dev) * 1.02 * (hi - lo), dim=1).values
        xi = Q[B // 2].clone()                                # the shared vector: in range for a part of the columns
        outb = torch.empty((B, nxi), dtype=torch.float64, device=dev)
        cols = sorted(set(np.linspace(0, B - 1, args.check_cols).astype(int).tolist()))
        xih = xi.cpu().numpy()

        def bit_equal(per_column):
            good = True
            for c in cols:
                q = Q[c].cpu().numpy() if per_column else xih
                want = oracle.interp1_bracket(Xb[c].cpu().numpy(), Yb[c].cpu().numpy(), np.ascontiguousarray(q), np.nan)
                good = good and np.array_equal(outb[c].cpu().numpy(), want, equal_nan=True)
            return bool(good)

        rec = {"shape": name, "n": n, "B": B, "nxi": nxi}
        calls = {"each_shared": lambda: mi.interp_each(ctx, Xb.T, Yb.T, xi, out=outb.T, want_ok=True),
                 "each_percol": lambda: mi.interp_each(ctx, Xb.T, Yb.T, Q.T, out=outb.T, want_ok=True),
                 "pairs": lambda: mi.interp_pairs(ctx, Xb.T, Yb.T, xi, out=outb.T, want_ok=True)}
        base = 16.0 * n * B + 8.0 * nxi * B + 4.0 * B
        alg = {"each_shared": base + 8.0 * nxi, "each_percol": base + 8.0 * nxi * B, "pairs": base + 8.0 * nxi}
        for key, fn in calls.items():
            if key == "each_shared" and name in ("P1e", "P4e"):
                continue                                      # forwarded to the pairs call: the same kernel
            if key != "pairs":
                rec[key + "_form"] = form_of(fn)
            ms, mn, mx = _median_ms(fn, args.reps, args.warmup)
            rec.update({key + "_ms_median": ms, key + "_ms_min": mn, key + "_ms_max": mx, key + "_alg_bytes": alg[key],
                        key + "_alg_frac_8TBs": alg[key] / (ms * 1e-3) / HBM_PEAK, key + "_bit_equal_oracle": bit_equal(key == "each_percol")})
        rec["bit_equal_oracle_cols"] = len(cols)
        if "each_shared_ms_median" in rec:
            rec["pairs_over_each_shared"] = rec["pairs_ms_median"] / rec["each_shared_ms_median"]
            rec["thin_slowest_below_pairs_fastest"] = bool(rec["each_shared_ms_max"] < rec["pairs_ms_min"])
        rec["each_percol_over_pairs"] = rec["each_percol_ms_median"] / rec["pairs_ms_median"]
        rec["bytes_ratio_percol_over_shared"] = alg["each_percol"] / alg["pairs"]
        print(json.dumps(rec), flush=True)
        del Xb, Yb, Q, xi, outb
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
