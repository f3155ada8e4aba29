"""Timing of arma::interp1's "nearest" method along matrix rows and over paired columns (Axis1.interp_rows_nearest /
interp_stack_nearest = mi_interp1_rows_nearest_f64_dev, mi.interp_pairs_nearest = mi_interp1_pairs_nearest_f64_dev) on one
MI355X, each shape against its LINEAR twin on the same inputs in the same process: nearest and linear alternate, --rounds
times, --reps launches each after --warmup, every launch between two device events, so that the spread between rounds is
visible beside the spread inside a round.  Every timed nearest result is checked bit for bit at the timed size against the
nearest rule restated with torch on the device (searchsorted, the two rounded subtractions, the select, a gather of the
stored value).

Rows shapes (algorithmic bytes 8*m*(columns touched) + 8*m*nxi + 8*nxi):
  R1  m = 125 000, n = 1024 onto 2048 sorted points
  R2  R1 with the same queries permuted
  R3  a cube of 512 x 512 fields at 64 levels onto 128 sorted times (interp_stack_nearest)
  R4  downsampling: m = 125 000, n = 2048 onto 256 sorted points
  R5  thin: m = 8, n = 100 000 onto 1 000 000 sorted points (flat body)
Pairs shapes (algorithmic bytes 16*sum(n_c) + 8*nxi*B + 8*nxi + 4 B per column for each of len and col_ok):
  P1  n = 1024, B = 125 000, XI = 2048 sorted points                        [LDS form]
  P2  P1 with XI permuted
  P3  P1 ragged: len uniform in [512, 1024]
  P4  n = 1e5, B = 640, XI = 1e5 sorted                                     [direct form]
Acceptance (reported per shape as "within_spread"): nearest is not slower than linear by more than the spread between
that shape's three round medians (the larger of the two calls' spreads).

  python3 scripts/gpu_nearest_batched_timing.py [--reps 20] [--warmup 3] [--rounds 3] [--shapes R1,..,P4]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
FORMS = ["rows_tile_16B", "rows_tile_8B", "rows_flat", "pairs_lds", "pairs_direct"]
ROWS = {   # name: (m, n, nxi, permuted, cube (ny, nx) or None)
    "R1": (125_000, 1024, 2048, False, None),
    "R2": (125_000, 1024, 2048, True, None),
    "R3": (512 * 512, 64, 128, False, (512, 512)),
    "R4": (125_000, 2048, 256, False, None),
    "R5": (8, 100_000, 1_000_000, False, None),
    "tinyR": (1300, 16, 40, True, None),           # rehearsal sizes
}
PAIRS = {  # name: (n, B, nxi, queries, ragged)
    "P1": (1024, 125_000, 2048, "sorted", False),
    "P2": (1024, 125_000, 2048, "permuted", False),
    "P3": (1024, 125_000, 2048, "sorted", True),
    "P4": (100_000, 640, 100_000, "sorted", False),
    "tinyP": (300, 50, 700, "permuted", True),
}


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
    """{"nearest": .., "linear": ..}: per-round medians, and median / min / max over all launches; the acceptance rule"""
    ts = {"nearest": [], "linear": []}
    for _ in range(rounds):
        ts["nearest"].append(_times_ms(near, reps, warmup))
        ts["linear"].append(_times_ms(lin, reps, warmup))
    out = {}
    for k, rs in ts.items():
        flat = [t for r in rs for t in r]
        meds = [statistics.median(r) for r in rs]
        out[k] = {"round_medians_ms": [round(v, 4) for v in meds], "median_ms": statistics.median(flat), "min_ms": min(flat),
                  "max_ms": max(flat), "round_spread_ms": max(meds) - min(meds)}
    out["nearest_over_linear"] = out["nearest"]["median_ms"] / out["linear"]["median_ms"]
    spread = max(out["nearest"]["round_spread_ms"], out["linear"]["round_spread_ms"])
    out["within_spread"] = bool(out["nearest"]["median_ms"] <= out["linear"]["median_ms"] + spread)
    return out


def _same_bits(a, b):
    """NaN in the same positions, the same 64 bits everywhere else"""
    import torch
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a.view(torch.int64)[~na], b.view(torch.int64)[~nb]))


def _rule_index(Xd, q):
    """the nearest rule on the device, one axis: int64 node index, -1 out of range, -2 NaN"""
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


def _pairs_rule(Xs, Ys, q, lens):
    """the nearest rule on the device for a slab of paired columns (rows of Xs, Ys): (b, nxi), extrap = NaN"""
    import torch
    b, n = Xs.shape
    nc = lens.to(torch.int64) if lens is not None else torch.full((b,), n, dtype=torch.int64, device=Xs.device)
    Xm = Xs.clone()
    Xm[torch.arange(n, device=Xs.device)[None, :] >= nc[:, None]] = float("inf")     # rows behind n_c are never a bracket
    first, last = Xs[:, :1], Xs.gather(1, (nc - 1)[:, None])
    qq = q[None, :].expand(b, q.numel())
    inr = (qq >= first) & (qq <= last)
    qs = torch.where(inr, qq, first).contiguous()
    l = torch.searchsorted(Xm, qs, right=True) - 1
    r = torch.minimum(l + 1, (nc - 1)[:, None])
    a = qs - Xs.gather(1, l)
    bb = Xs.gather(1, r) - qs
    k = torch.where(bb < a, r, l)
    out = Ys.gather(1, k)
    return torch.where(inr, out, torch.full_like(out, float("nan")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="R1,R2,R3,R4,R5,P1,P2,P3,P4")
    args = ap.parse_args()
    import numpy as np
    import torch

    import armadillocudalinearinterpolation_amd as mi

    if not torch.cuda.is_available():
        raise SystemExit("gpu_nearest_batched_timing.py needs a GPU (there is no CPU fallback)")
    ctx = mi.Context(0)
    L = ctx._L
    dev = torch.device("cuda:0")
    print(json.dumps({"device": ctx.device_info(), "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds}), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1234)
    forms = lambda: [int(L.mi_debug_nearest_batched_launches(f)) for f in range(5)]  # noqa: E731
    shapes = args.shapes.split(",")

    for name in [s for s in shapes if s in ROWS]:
        m, n, nxi, permuted, cube = ROWS[name]
        rng = np.random.default_rng(12)
        X = np.cumsum(rng.uniform(0.5, 1.0, n))
        xi = np.linspace(X[0], X[-1], nxi)
        xi[-1] = X[-1]
        if nxi >= 8:
            xi[1], xi[2] = np.nan, X[0] - 1.0
        Xd = torch.from_numpy(X).to(dev)
        touched = int((torch.unique(_rule_index(Xd, torch.from_numpy(xi).to(dev))) >= 0).sum())   # columns some query is nearest to
        if permuted:
            xi = rng.permutation(xi)
        Ybuf = torch.randn((n, m), dtype=torch.float64, device=dev, generator=gen)        # column k of Y = row k of the buffer
        xd = torch.from_numpy(xi).to(dev)
        axis = mi.Axis1.from_nodes(ctx, X)
        on = torch.empty((nxi, m), dtype=torch.float64, device=dev)
        ol = torch.empty((nxi, m), dtype=torch.float64, device=dev)
        if cube:
            ny, nx = cube
            Z = Ybuf.view(n, nx, ny).permute(2, 1, 0)
            on3, ol3 = on.view(nxi, nx, ny).permute(2, 1, 0), ol.view(nxi, nx, ny).permute(2, 1, 0)
            near = lambda: axis.interp_stack_nearest(Z, xd, out=on3)  # noqa: E731
            lin = lambda: axis.interp_stack(Z, xd, out=ol3)  # noqa: E731
        else:
            near = lambda: axis.interp_rows_nearest(Ybuf.T, xd, out=on.T)  # noqa: E731
            lin = lambda: axis.interp_rows(Ybuf.T, xd, out=ol.T)  # noqa: E731
        f0 = forms()
        rec = {"shape": name, "m": m, "n": n, "nxi": nxi, "permuted": permuted, "cube": list(cube) if cube else None}
        rec.update(_alternate(near, lin, args.reps, args.warmup, args.rounds))
        launches = [a - b for a, b in zip(forms(), f0)]
        rec["nearest_form"] = FORMS[max(range(5), key=lambda i: launches[i])]
        alg = 8.0 * m * touched + 8.0 * m * nxi + 8.0 * nxi
        rec["columns_touched"], rec["alg_bytes"] = touched, alg
        rec["nearest"]["alg_frac_8TBs"] = alg / (rec["nearest"]["median_ms"] * 1e-3) / HBM_PEAK
        k = _rule_index(Xd, xd)
        ok = True
        step = max(1, (1 << 27) // m)                       # the reference in slabs of output columns
        for i0 in range(0, nxi, step):
            ks = k[i0:i0 + step]
            ref = Ybuf[torch.clamp(ks, min=0)]
            ref[ks < 0] = float("nan")
            ok = ok and _same_bits(on[i0:i0 + step], ref)
            del ref
        rec["nearest_bits_equal_rule"] = bool(ok)
        print(json.dumps(rec), flush=True)
        axis.close()
        del Ybuf, on, ol, xd
        torch.cuda.empty_cache()

    for name in [s for s in shapes if s in PAIRS]:
        n, B, nxi, order, ragged = PAIRS[name]
        # nodes: jittered increments, the same range [0, ~0.6 n] for every column; column c = row c of the buffers
        Xb = torch.cumsum(torch.rand((B, n), generator=gen, dtype=torch.float64, device=dev) * 0.8 + 0.2, dim=1)
        Xb -= Xb[:, :1].clone()
        Yb = torch.rand((B, n), generator=gen, dtype=torch.float64, device=dev) * 2.0 - 1.0
        lens = torch.randint(n // 2, n + 1, (B,), generator=gen, device=dev, dtype=torch.int32) if ragged else None
        top = float(Xb[:, (n // 2 if ragged else n) - 1].min())
        xi = torch.linspace(-0.01 * top, 1.01 * top, nxi, dtype=torch.float64, device=dev)
        if order == "permuted":
            xi = xi[torch.randperm(nxi, generator=gen, device=dev)].contiguous()
        on = torch.empty((B, nxi), dtype=torch.float64, device=dev)
        ol = torch.empty((B, nxi), dtype=torch.float64, device=dev)
        okn = [None]

        def near():
            okn[0] = mi.interp_pairs_nearest(ctx, Xb.T, Yb.T, xi, lens=lens, out=on.T, want_ok=True)[1]

        def lin():
            mi.interp_pairs(ctx, Xb.T, Yb.T, xi, lens=lens, out=ol.T, want_ok=True)

        f0 = forms()
        rec = {"shape": name, "n": n, "B": B, "nxi": nxi, "queries": order, "ragged": ragged}
        rec.update(_alternate(near, lin, args.reps, args.warmup, args.rounds))
        launches = [a - b for a, b in zip(forms(), f0)]
        rec["nearest_form"] = FORMS[max(range(5), key=lambda i: launches[i])]
        rows = float(lens.sum()) if ragged else float(n) * B
        alg = 16.0 * rows + 8.0 * nxi * B + 8.0 * nxi + 4.0 * B * (2 if ragged else 1)
        rec["alg_bytes"] = alg
        rec["nearest"]["alg_frac_8TBs"] = alg / (rec["nearest"]["median_ms"] * 1e-3) / HBM_PEAK
        rec["all_columns_ok"] = bool((okn[0] == 1).all())
        ok = True
        step = max(1, (1 << 24) // max(n, nxi))             # the reference in slabs of columns
        for c0 in range(0, B, step):
            ref = _pairs_rule(Xb[c0:c0 + step], Yb[c0:c0 + step], xi, None if lens is None else lens[c0:c0 + step])
            ok = ok and _same_bits(on[c0:c0 + step], ref)
            del ref
        rec["nearest_bits_equal_rule"] = bool(ok)
        print(json.dumps(rec), flush=True)
        del Xb, Yb, on, ol, xi
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
