"""Timing of arma::interp1's "nearest" method (Grid1.interp_nearest = mi_interp1_nearest_f64_dev, Axis1.interp_cols_nearest
= mi_interp1_cols_nearest_f64_dev) on one MI355X, each shape against the LINEAR call on the same inputs in the same
process: nearest and linear alternate, --rounds times, --reps launches each after --warmup, every launch between two
device events, so that the spread between rounds is visible beside the spread inside a round.  Every timed nearest result
is checked bit for bit at the timed size against the nearest rule restated with torch on the device (searchsorted, the two
rounded subtractions, the select, a gather of the stored value), and the linear result of the table shapes against
mi_interp1_f64_dev's streaming kernel.

Table shapes (1e8 queries; algorithmic bytes 16 B per query):
  T1  1e6-node closed-form grid (linspace: mode 0), the sorted uniform set j/(NQ-1), ordered hint: streaming form both
  T2  the same queries on the jittered 1e6-node grid (mode 3), ordered hint: streaming form both
  T3  random queries on a 16 383-node closed-form table, unordered hint: table-in-LDS form both
  T4  random queries on the 1e6-node closed-form grid, unordered hint: nearest has NO region sweep and streams; the linear
      call takes its region sweep (Grid1.interp = mi_interp1_f64_dev_v2)
Columns shapes (algorithmic bytes 8*n*B + 8*nxi*B + 8*nxi):
  C1  n = 1024, B = 125 000, XI = 2048 sorted points (DESIGN.md 4.8's S1)      [LDS form]
  C2  C1 with XI permuted
  C3  n = 50 001, B = 2048, XI = 50 001 sorted points                         [direct form]
Also, once and untimed: the chunked host form (Grid1.interp_nearest_host, 2 x 8 M + 5 queries) against the device form.

  python3 scripts/gpu_interp1_nearest_timing.py [--reps 20] [--warmup 3] [--rounds 3] [--shapes T1,T2,T3,T4,C1,C2,C3,H]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
NQ = 100_000_000


def _times_ms(fn, reps, warmup):
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
    return ts


def _alternate(near, lin, reps, warmup, rounds):
    """{"nearest": .., "linear": ..}: per-round medians, and median / min / max over all launches"""
    ts = {"nearest": [], "linear": []}
    for _ in range(rounds):
        ts["nearest"].append(_times_ms(near, reps, warmup))
        ts["linear"].append(_times_ms(lin, reps, warmup))
    out = {}
    for k, rs in ts.items():
        flat = [t for r in rs for t in r]
        out[k] = {"round_medians_ms": [round(statistics.median(r), 4) for r in rs], "median_ms": statistics.median(flat),
                  "min_ms": min(flat), "max_ms": max(flat)}
    out["nearest_over_linear"] = out["nearest"]["median_ms"] / out["linear"]["median_ms"]
    return out


def _same_bits(a, b):
    """NaN in the same positions, the same 64 bits everywhere else"""
    import torch
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a.view(torch.int64)[~na], b.view(torch.int64)[~nb]))


def _rule_index(Xd, q):
    """the nearest rule on the device: int64 node index, -1 out of range, -2 NaN"""
    import torch
    n = Xd.numel()
    inr = (q >= Xd[0]) & (q <= Xd[-1])
    qs = torch.where(inr, q, Xd[0])
    l = torch.searchsorted(Xd, qs, right=True) - 1
    r = torch.clamp(l + 1, max=n - 1)
    a = qs - Xd[l]
    b = Xd[r] - qs
    k = torch.where(b < a, r, l)
    k = torch.where(inr, k, torch.full_like(k, -1))
    return torch.where(torch.isnan(q), torch.full_like(k, -2), k)


def _rule(Xd, Yd, q, extrap=float("nan")):
    import torch
    k = _rule_index(Xd, q)
    out = Yd[torch.clamp(k, min=0)]
    out = torch.where(k == -1, torch.full_like(out, extrap), out)
    return torch.where(k == -2, torch.full_like(out, float("nan")), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="T1,T2,T3,T4,C1,C2,C3,H")
    args = ap.parse_args()
    import numpy as np
    import torch

    import armadillocudalinearinterpolation_amd as mi

    ctx = mi.Context(0)
    L = ctx._L
    dev = torch.device("cuda:0")
    shapes = args.shapes.split(",")
    print(json.dumps({"device": ctx.device_info(), "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds}), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1234)
    forms = lambda: [L.mi_debug_nearest_launches(f) for f in range(5)]  # noqa: E731

    def table(kind):
        n = 16_383 if kind == "small" else 1_000_000
        if kind == "jitter":
            u = np.random.default_rng(7).random(n)
            X = -2.0 + 3.0 * (np.arange(n) + 0.5 * u) / n
        else:
            X = np.linspace(0.0, 1.0, n)
        Y = np.sin(5.0 * (X - X[0]) / (X[-1] - X[0])) + 0.25 * (X - X[0])
        return X, Y

    TABLE_SHAPES = {"T1": ("closed", "sorted", 2), "T2": ("jitter", "sorted", 2), "T3": ("small", "random", 1),
                    "T4": ("closed", "random", 1)}
    for name in [s for s in shapes if s in TABLE_SHAPES]:
        kind, order, hint = TABLE_SHAPES[name]
        X, Y = table(kind)
        grid = mi.Grid1.from_nodes(ctx, X, Y, sanitise=False)
        lo, hi = float(X[0]), float(X[-1])
        if order == "sorted":
            xq = torch.arange(NQ, dtype=torch.float64, device=dev) / float(NQ - 1) * (hi - lo) + lo   # j/(NQ-1) over the range
            xq.clamp_(lo, hi)
        else:
            xq = (torch.rand(NQ, generator=gen, dtype=torch.float64, device=dev) * 1.02 - 0.01) * (hi - lo) + lo
        on, ol = torch.empty_like(xq), torch.empty_like(xq)
        ctx.set_query_order(hint)
        f0, d0 = forms(), L.mi_debug_sweep_ds_launches()
        rec = {"shape": name, "table": kind, "n": int(X.size), "mode": grid.info()["mode"], "nq": NQ, "queries": order,
               "hint": {1: "unordered", 2: "ordered"}[hint]}
        rec.update(_alternate(lambda: grid.interp_nearest(xq, out=on), lambda: grid.interp(xq, out=ol), args.reps, args.warmup,
                              args.rounds))
        launches = [a - b for a, b in zip(forms(), f0)]
        rec["nearest_form"] = ["streaming", "lds", "scalar"][max(range(3), key=lambda i: launches[i])]
        rec["linear_region_sweep_launches"] = L.mi_debug_sweep_ds_launches() - d0
        rec["note"] = "no region-sweep form of nearest: it streams" if name == "T4" else ""
        alg = 16.0 * NQ
        for k in ("nearest", "linear"):
            rec[k]["alg_frac_8TBs"] = alg / (rec[k]["median_ms"] * 1e-3) / HBM_PEAK
        rec["alg_bytes"] = alg
        Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
        rec["nearest_bits_equal_rule"] = _same_bits(on, _rule(Xd, Yd, xq))
        ctx.set_query_order(2)
        ref = torch.empty_like(xq)
        check = ctx._L.mi_interp1_f64_dev(ctx._h, grid._h, xq.data_ptr(), ref.data_ptr(), NQ, float("nan"))
        rec["linear_bits_equal_streaming"] = check == 0 and _same_bits(ol, ref)
        ctx.set_query_order(0)
        print(json.dumps(rec), flush=True)
        grid.close()
        del xq, on, ol, ref, Xd, Yd
        torch.cuda.empty_cache()

    COLS_SHAPES = {"C1": (1024, 125_000, 2048, "sorted"), "C2": (1024, 125_000, 2048, "permuted"),
                   "C3": (50_001, 2048, 50_001, "sorted")}
    for name in [s for s in shapes if s in COLS_SHAPES]:
        n, B, nxi, order = COLS_SHAPES[name]
        X = np.linspace(0.0, 1.0, n)
        axis = mi.Axis1.from_nodes(ctx, X)
        Yb = torch.rand((B, n), generator=gen, dtype=torch.float64, device=dev) * 2.0 - 1.0   # column c = Yb[c]
        xi = torch.linspace(-0.01, 1.01, nxi, dtype=torch.float64, device=dev)                # a few out of range on both ends
        if order == "permuted":
            xi = xi[torch.randperm(nxi, generator=gen, device=dev)].contiguous()
        on = torch.empty((B, nxi), dtype=torch.float64, device=dev)
        ol = torch.empty((B, nxi), dtype=torch.float64, device=dev)
        f0 = forms()
        rec = {"shape": name, "n": n, "B": B, "nxi": nxi, "queries": order}
        rec.update(_alternate(lambda: axis.interp_cols_nearest(Yb.T, xi, out=on.T), lambda: axis.interp_cols(Yb.T, xi, out=ol.T),
                              args.reps, args.warmup, args.rounds))
        launches = [a - b for a, b in zip(forms(), f0)]
        rec["nearest_form"] = "lds" if launches[3] else "direct"
        alg = 8.0 * n * B + 8.0 * nxi * B + 8.0 * nxi
        for k in ("nearest", "linear"):
            rec[k]["alg_frac_8TBs"] = alg / (rec[k]["median_ms"] * 1e-3) / HBM_PEAK
        rec["alg_bytes"] = alg
        k = _rule_index(torch.from_numpy(X).to(dev), xi)
        ok = True
        for c0 in range(0, B, 8192):                       # the reference in slabs of columns
            ref = Yb[c0:c0 + 8192][:, torch.clamp(k, min=0)]
            ref[:, k < 0] = float("nan")
            ok = ok and _same_bits(on[c0:c0 + 8192], ref)
            del ref
        rec["nearest_bits_equal_rule"] = bool(ok)
        print(json.dumps(rec), flush=True)
        axis.close()
        del Yb, on, ol, xi
        torch.cuda.empty_cache()

    if "H" in shapes:
        X, Y = table("closed")
        grid = mi.Grid1.from_nodes(ctx, X, Y, sanitise=False)
        nq = 2 * (8 << 20) + 5                              # one query past the single-shot form: three chunks
        xq = np.random.default_rng(5).random(nq) * 1.02 - 0.01
        host = grid.interp_nearest_host(xq, extrap=-1.0)
        devr = grid.interp_nearest(torch.from_numpy(xq).to(dev), extrap=-1.0).cpu().numpy()
        same = np.array_equal(np.isnan(host), np.isnan(devr)) and np.array_equal(host.view(np.int64)[~np.isnan(host)],
                                                                                  devr.view(np.int64)[~np.isnan(devr)])
        print(json.dumps({"shape": "H", "nq": nq, "host_chunked_bits_equal_device": bool(same),
                          "pinned_ranges_after": int(L.mi_debug_pinned_ranges())}), flush=True)
        grid.close()
    ctx.close()


if __name__ == "__main__":
    main()
