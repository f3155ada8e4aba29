"""Clock stamps of the phased region sweep (interp1_phased_sweep_kernel with its stamping flag on): do the offsets between
the phase classes hold over the run, and when does each class end?  Run on the GPU box.

    python scripts/gpu_sweep_phase_stamps.py [P:first_units ...]      e.g. 4:0 4:4123 4:4321 4:1234 2:42

1e8 random queries over the 1e6-node closed-form table (the headline), one workgroup per CU, through
mi_debug_interp1_phased_sweep_ex; first_units 0 is the clock form (run it first: it is the "before").  Per form, the
last of twelve launches is read.  Printed per class (blockIdx % P), medians over the class's workgroups, in microseconds:
the start of the gather step of tiles 1, 12 and the last tile every workgroup has, as an offset against class 0 modulo
the tile period (the median distance of consecutive gather starts, tiles 4..16 of class 0); and the exit of the class's
slowest workgroup, counted from the earliest entry of the launch."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    import armadillocudalinearinterpolation_amd as mi
    from armadillocudalinearinterpolation_amd import _lib, synth
    forms = [(int(a.split(":")[0]), int(a.split(":")[1])) for a in sys.argv[1:]] or [(4, 0), (4, 4123), (4, 4321), (4, 1234), (2, 42)]
    ctx = mi.Context(0)
    L = _lib.load()
    dev = torch.device("cuda", 0)
    cus = ctx.device_info()["compute_units"]
    khz = 100_000                                    # the constant-rate wall clock of gfx950 runs at 100 MHz
    ng, nq, cap = 1_000_000, 100_000_000, 32
    X = np.arange(ng) / (ng - 1)
    grid = mi.Grid1.from_nodes(ctx, X, np.sin(2 * np.pi * X) + 0.5 * X, sanitise=False)
    xq = synth.splitmix_uniform(0x5EED0003, nq, dev)
    out = torch.empty_like(xq)
    ctx.set_query_order(1)
    us = 1e3 / khz
    for phases, first_units in forms:
        stamps = torch.full((cus * cap,), -1, dtype=torch.int64, device=dev)
        for _ in range(12):                              # (the clocks of an idle device take a few launches to settle)
            stamps.fill_(-1)
            _lib.check(L.mi_debug_interp1_phased_sweep_ex(ctx._h, grid._h, ctypes.c_void_p(xq.data_ptr()), ctypes.c_void_p(out.data_ptr()), nq,
                                                          float("nan"), phases, cus, first_units, ctypes.c_void_p(stamps.data_ptr()), cap), ctx._h)
            ctx.synchronize()
        s = stamps.cpu().numpy().reshape(cus, cap).astype(np.float64)
        slots = (s >= 0).sum(axis=1)                     # entry + gather steps + exit
        tiles = slots - 2
        t0 = s[:, 0].min()
        cls = np.arange(cus) % phases
        ref = cls == 0
        period = float(np.median(np.diff(s[ref, 5:18], axis=1))) * us
        common = int(tiles.min())
        print("form P=%d first_units=%d: %d workgroups, tiles per workgroup %d..%d, tile period %.2f us (class 0, tiles 4..16)" % (
            phases, first_units, cus, tiles.min(), tiles.max(), period), flush=True)
        for c in range(phases):
            me = cls == c
            offs = []
            for i in (1, 12, common - 1):
                d = (np.median(s[me, 1 + i]) - np.median(s[ref, 1 + i])) * us
                offs.append(d % period if period > 0 else d)
            exits = s[me, slots[me] - 1]
            print("  class %d: gather start of tile 1 / 12 / %d against class 0, mod period: %6.2f %6.2f %6.2f us;  entry %.2f us,  slowest exit %.2f us" % (
                c, common - 1, offs[0], offs[1], offs[2], (s[me, 0].min() - t0) * us, (exits.max() - t0) * us), flush=True)
        print("  kernel span (earliest entry to latest exit): %.2f us" % ((s[np.arange(cus), slots - 1].max() - t0) * us), flush=True)


if __name__ == "__main__":
    main()
