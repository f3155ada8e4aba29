"""Timing of arma::interp2's "nearest" method (Grid2.interp_nearest / interp_grid_nearest = mi_interp2_nearest_f64_dev /
mi_interp2_grid_nearest_f64_dev, mi.interp2_slices_nearest = mi_interp2_slices_nearest_f64_dev) on one MI355X, each shape
against its LINEAR twin on the same inputs in the same process: nearest and linear alternate, --rounds times, --reps
launches each after --warmup, every launch between two device events, so that the spread between rounds is visible beside
the spread inside a round.  Every timed nearest result is checked bit for bit at the timed size against the 2-D nearest
rule restated with torch on the device (searchsorted, the two rounded subtractions and the select per axis, one gather).

Shapes (the ones README.md quotes for the linear calls):
  G1  gridded: 1024^2 table onto 16384 x 8192 outputs (nyi x nxi), sorted axes
  G2  gridded: 8192^2 table, same outputs, quad cells        G3  the same table as column pairs (compact)
  G4  G1 with xi permuted
  G5  thin: 1 x 1e8 outputs (flat body)
  S1  slices: 4096 slices of 64^2 onto 128^2                 (the linear call's LDS form; nearest has the direct form only)
  S2  slices: 8 slices of 2048^2 onto 4096^2
  S3  slices: one 64^2 slice onto 4096^2
  P1  scattered: 4096^2 table, 1e8 random pairs
Acceptance (reported per shape as "within_spread"): nearest is not slower than linear by more than the spread between
that shape's round medians (the larger of the two calls' spreads).

  python3 scripts/gpu_interp2_nearest_timing.py [--reps 20] [--warmup 3] [--rounds 3] [--shapes G1,..,P1]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
FORMS = ["scattered", "grid_tile_16B", "grid_tile_8B", "grid_flat_16B", "grid_flat_8B", "slices_tile_16B", "slices_tile_8B",
         "slices_flat"]
GRIDDED = {   # name: (table n (n x n), nyi, nxi, compact, xi permuted)
    "G1": (1024, 16384, 8192, False, False),
    "G2": (8192, 16384, 8192, False, False),
    "G3": (8192, 16384, 8192, True, False),
    "G4": (1024, 16384, 8192, False, True),
    "G5": (1024, 1, 100_000_000, False, False),
    "tinyG": (64, 300, 200, False, True),          # rehearsal sizes
}
SLICES = {    # name: (slices, table n (n x n), outputs n (n x n))
    "S1": (4096, 64, 128),
    "S2": (8, 2048, 4096),
    "S3": (1, 64, 4096),
    "tinyS": (5, 20, 300),
}
SCATTERED = {"P1": (4096, 100_000_000), "tinyP": (64, 5000)}


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


def _grid_ok(out, Zb, kx, ky):
    """out: (S, nxi, nyi) buffer; Zb: (S, nx, ny) buffer (row j of a slice = table column j); checked in slabs of slices
    and output columns of about 2^26 elements"""
    import torch
    nan = float("nan")
    S, nxi, nyi = out.shape
    kyc = torch.clamp(ky, min=0)[None, :]
    cols = max(1, min(nxi, (1 << 26) // nyi))
    per = max(1, (1 << 26) // (cols * nyi))
    ok = True
    for s0 in range(0, S, per):
        for j0 in range(0, nxi, cols):
            kj = kx[j0:j0 + cols]
            ref = Zb[s0:s0 + per][:, torch.clamp(kj, min=0)[:, None], kyc]     # (slices, columns, nyi): copies of the stored values
            ref[:, :, ky < 0] = nan                                            # extrap is NaN in every timed call
            ref[:, kj < 0, :] = nan
            ok = ok and _same_bits(out[s0:s0 + per, j0:j0 + cols], ref)
            del ref
    return bool(ok)


def _axis(rng, n):
    import numpy as np
    return np.cumsum(rng.uniform(0.5, 1.0, n))


def _queries(X, n, rng, permuted):
    import numpy as np
    q = np.linspace(X[0], X[-1], n) if n > 1 else np.array([0.5 * (X[0] + X[-1])])
    q[-1] = X[-1] if n > 1 else q[-1]
    if n >= 8:
        q[1], q[2] = np.nan, X[0] - 1.0
    return rng.permutation(q) if permuted else q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="G1,G2,G3,G4,G5,S1,S2,S3,P1")
    args = ap.parse_args()
    import numpy as np
    import torch

    import armadillocudalinearinterpolation_amd as mi

    if not torch.cuda.is_available():
        raise SystemExit("gpu_interp2_nearest_timing.py needs a GPU (there is no CPU fallback)")
    ctx = mi.Context(0)
    L = ctx._L
    dev = torch.device("cuda:0")
    print(json.dumps({"device": ctx.device_info(), "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds}), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1234)
    forms = lambda: [int(L.mi_debug_nearest2_launches(f)) for f in range(8)]  # noqa: E731
    shapes = args.shapes.split(",")

    def finish(rec, f0, alg_near, alg_lin):
        launches = [a - b for a, b in zip(forms(), f0)]
        rec["nearest_form"] = FORMS[max(range(8), key=lambda i: launches[i])]
        rec["alg_bytes_nearest"], rec["alg_bytes_linear"] = alg_near, alg_lin
        rec["nearest"]["alg_frac_8TBs"] = alg_near / (rec["nearest"]["median_ms"] * 1e-3) / HBM_PEAK
        rec["linear"]["alg_frac_8TBs"] = alg_lin / (rec["linear"]["median_ms"] * 1e-3) / HBM_PEAK
        print(json.dumps(rec), flush=True)

    for name in [s for s in shapes if s in GRIDDED]:
        n, nyi, nxi, compact, permuted = GRIDDED[name]
        rng = np.random.default_rng(12)
        X, Y = _axis(rng, n), _axis(rng, n)
        Zt = torch.randn((n, n), dtype=torch.float64, device=dev, generator=gen)          # row j = column j of Z (ny x nx)
        g = mi.Grid2.from_axes(ctx, X, Y, Zt.cpu().numpy().T, compact=compact)
        xi, yi = _queries(X, nxi, rng, permuted), _queries(Y, nyi, rng, False)
        xd, yd = torch.from_numpy(xi).to(dev), torch.from_numpy(yi).to(dev)
        on = torch.empty((nxi, nyi), dtype=torch.float64, device=dev)
        ol = torch.empty((nxi, nyi), dtype=torch.float64, device=dev)
        near = lambda: g.interp_grid_nearest(xd, yd, out=on)  # noqa: E731
        lin = lambda: g.interp_grid(xd, yd, out=ol)  # noqa: E731
        f0 = forms()
        rec = {"shape": name, "table": [n, n], "nyi": nyi, "nxi": nxi, "compact": compact, "xi_permuted": permuted}
        rec.update(_alternate(near, lin, args.reps, args.warmup, args.rounds))
        kx, ky = _rule_index(torch.from_numpy(X).to(dev), xd), _rule_index(torch.from_numpy(Y).to(dev), yd)
        rec["nearest_bits_equal_rule"] = _grid_ok(on[None], Zt[None], kx, ky)
        cells = int((torch.unique(kx) >= 0).sum()) * int((torch.unique(ky) >= 0).sum())   # nodes some output copies
        out_bytes = 8.0 * nxi * nyi + 8.0 * (nxi + nyi)
        finish(rec, f0, out_bytes + 8.0 * cells, out_bytes + 32.0 * cells)
        g.close()
        del Zt, on, ol, xd, yd
        torch.cuda.empty_cache()

    for name in [s for s in shapes if s in SLICES]:
        S, n, no = SLICES[name]
        rng = np.random.default_rng(13)
        X, Y = _axis(rng, n), _axis(rng, n)
        Zb = torch.randn((S, n, n), dtype=torch.float64, device=dev, generator=gen)       # [slice][column][row]
        Z = Zb.permute(2, 1, 0)
        ax, ay = mi.Axis1.from_nodes(ctx, X), mi.Axis1.from_nodes(ctx, Y)
        xi, yi = _queries(X, no, rng, False), _queries(Y, no, rng, False)
        xd, yd = torch.from_numpy(xi).to(dev), torch.from_numpy(yi).to(dev)
        on = torch.empty((S, no, no), dtype=torch.float64, device=dev)
        ol = torch.empty((S, no, no), dtype=torch.float64, device=dev)
        on3, ol3 = on.permute(2, 1, 0), ol.permute(2, 1, 0)
        near = lambda: mi.interp2_slices_nearest(ctx, ax, ay, Z, xd, yd, out=on3)  # noqa: E731
        lin = lambda: mi.interp2_slices(ctx, ax, ay, Z, xd, yd, out=ol3)  # noqa: E731
        f0 = forms()
        rec = {"shape": name, "slices": S, "table": [n, n], "outputs": [no, no]}
        rec.update(_alternate(near, lin, args.reps, args.warmup, args.rounds))
        kx, ky = _rule_index(torch.from_numpy(X).to(dev), xd), _rule_index(torch.from_numpy(Y).to(dev), yd)
        rec["nearest_bits_equal_rule"] = _grid_ok(on, Zb, kx, ky)
        out_bytes = 8.0 * S * no * no + 8.0 * 2 * no
        finish(rec, f0, out_bytes + 8.0 * S * min(n * n, no * no), out_bytes + 8.0 * S * n * n)
        ax.close()
        ay.close()
        del Zb, Z, on, ol, on3, ol3
        torch.cuda.empty_cache()

    for name in [s for s in shapes if s in SCATTERED]:
        n, nq = SCATTERED[name]
        rng = np.random.default_rng(14)
        X, Y = _axis(rng, n), _axis(rng, n)
        Zt = torch.randn((n, n), dtype=torch.float64, device=dev, generator=gen)
        g = mi.Grid2.from_axes(ctx, X, Y, Zt.cpu().numpy().T)
        span = lambda A: (A[0] - 0.01 * (A[-1] - A[0]), 1.02 * (A[-1] - A[0]))  # noqa: E731
        xq = torch.rand(nq, dtype=torch.float64, device=dev, generator=gen) * span(X)[1] + span(X)[0]
        yq = torch.rand(nq, dtype=torch.float64, device=dev, generator=gen) * span(Y)[1] + span(Y)[0]
        xq[1], yq[2] = float("nan"), float("nan")
        on, ol = torch.empty_like(xq), torch.empty_like(xq)
        near = lambda: g.interp_nearest(xq, yq, out=on)  # noqa: E731
        lin = lambda: g.interp(xq, yq, out=ol)  # noqa: E731
        f0 = forms()
        rec = {"shape": name, "table": [n, n], "nq": nq}
        rec.update(_alternate(near, lin, args.reps, args.warmup, args.rounds))
        Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
        ok = True
        step = 1 << 24
        for i0 in range(0, nq, step):
            kx, ky = _rule_index(Xd, xq[i0:i0 + step]), _rule_index(Yd, yq[i0:i0 + step])
            ref = Zt[torch.clamp(kx, min=0), torch.clamp(ky, min=0)]
            ref[(kx < 0) | (ky < 0)] = float("nan")
            ok = ok and _same_bits(on[i0:i0 + step], ref)
            del ref
        rec["nearest_bits_equal_rule"] = bool(ok)
        finish(rec, f0, 24.0 * nq + 8.0 * nq, 24.0 * nq + 32.0 * nq)
        g.close()
        del Zt, xq, yq, on, ol
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
