"""GPU checks of mi_interp1_f64_dev_v2: the pipelined region sweep with part of each tile's result stores held back to the
owning group's next step (DEFER > 0, csrc/mi_interp1_sweep.hpp) must reproduce the streaming kernel bit for bit, for every parity of the
per-workgroup tile count, for workgroups with one tile or none, with and without a ragged tail, and must write nothing
past the end of the result vector.

The environment hooks are read once per process, so the cases run in child processes: one with the new kernel, one with
MI_SWEEP_DEFER=0 (every call forwarded to mi_interp1_f64_dev); both are started together and their digests compared."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAILS = (0, 1, 2, 16383)
KINDS = ("closed", "jitter", "clustered", "walk")      # table modes 0, 3, 2, 1: one kernel instance each

CHILD = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, %(root)r)
import armadillocudalinearinterpolation_amd as mi
from armadillocudalinearinterpolation_amd import synth, _lib
TILE, GUARD, SENT = 16384, 16384, -12345.678
ctx = mi.Context(0)
C = ctx.device_info()["compute_units"]
L = _lib.load()
dev = torch.device("cuda", 0)
tiles = [1, 2, 3, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 7, 4 * C + C // 2]
tails = %(tails)r
nmax = max(tiles) * TILE + max(tails)
print("CU", C, "NMAX", nmax)
xq_all = synth.splitmix_uniform(11, nmax, dev) * 1.02 - 0.01          # both sides out of range
xq_all[torch.tensor([0, 5, 16383, 16384, 40000, nmax - 1, nmax - 16384], device=dev)] = float("nan")
buf = torch.empty(nmax + GUARD, dtype=torch.float64, device=dev)
ref = torch.empty(nmax, dtype=torch.float64, device=dev)
same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
for kind in %(kinds)r:
    ng = 1_000_000
    X = np.arange(ng) / (ng - 1)
    u = synth.splitmix_uniform(7, ng, torch.device("cpu")).numpy()
    if kind == "jitter":
        X = (np.arange(ng) + 0.5 * u) / ng
    elif kind == "clustered":                   # bucket index + binary search
        X = np.unique(np.sort(u ** 3))
    elif kind == "walk":                        # more than a cell off the straight line: generic guess + bounded walk
        X = np.unique(np.sort((np.arange(ng) + 1.5 * u) / ng))
    Y = np.sin(2 * np.pi * X) + 0.5 * X
    grid = mi.Grid1.from_nodes(ctx, X, Y, sanitise=False)
    assert grid.info()["mode"] == {"closed": 0, "jitter": 3, "clustered": 2, "walk": 1}[kind], (kind, grid.info())
    ctx.set_query_order(2)                      # ordered: streaming kernel, the reference (a prefix of it serves every case)
    grid.interp(xq_all, out=ref)
    assert bool(torch.isnan(ref).any()) and bool((ref == ref).any())
    for T in tiles:
        for tail in tails:
            nq = T * TILE + tail
            xq, out = xq_all[:nq], buf[:nq]
            buf.fill_(SENT)
            ctx.set_query_order(1)              # unordered: region sweep
            before = L.mi_debug_sweep_ds_launches()
            for _ in range(3):                  # back to back into the same buffers, nothing waited for in between
                grid.interp(xq, out=out)
            launched = L.mi_debug_sweep_ds_launches() - before
            assert launched == (3 if %(expect_new)r else 0), (kind, T, tail, launched)
            assert same(out, ref[:nq]), (kind, T, tail)
            assert bool((buf[nq:] == SENT).all()), ("guard", kind, T, tail)
            print("CASE", kind, T, tail, hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest())
    # AUTO: the probe inside one call predicts the kernel of the next (the verdict lands in a host mailbox: the sequence
    # waits for each call so that the prediction is there).  Random, sorted, random query sets.
    nq = 2 * C * TILE + 2
    rnd = xq_all[:nq]
    srt = torch.sort(torch.nan_to_num(rnd, nan=0.5)).values
    ctx.set_query_order(2)
    want = {"random": grid.interp(rnd), "sorted": grid.interp(srt)}
    ctx.set_query_order(0)
    before = L.mi_debug_sweep_ds_launches()
    for name, q in (("random", rnd), ("random", rnd), ("random", rnd), ("sorted", srt), ("sorted", srt), ("random", rnd),
                    ("random", rnd), ("random", rnd)):
        got = grid.interp(q)
        ctx.synchronize()
        assert same(got, want[name]), ("auto", kind, name)
    launched = L.mi_debug_sweep_ds_launches() - before
    assert (launched >= 2) if %(expect_new)r else (launched == 0), ("auto", kind, launched)
    print("AUTO", kind, "ok", launched)
print("DONE")
"""


def _start(defer_off):
    env = dict(os.environ, MI_SWEEP_VARIANT="2", MI_SWEEP_MIN_TILES_PER_CU="0")
    env.pop("MI_SWEEP_DEFER", None)
    if defer_off:
        env["MI_SWEEP_DEFER"] = "0"
    prog = CHILD % {"root": ROOT, "tails": TAILS, "kinds": KINDS, "expect_new": not defer_off}
    return subprocess.Popen([sys.executable, "-c", prog], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


@pytest.fixture(scope="module")
def runs():
    """(returncode, stdout, stderr) of the child with the new kernel and of the child with MI_SWEEP_DEFER=0"""
    procs = [_start(False), _start(True)]
    out = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        out.append((p.returncode, so, se))
    return out


def _cases(stdout):
    return {tuple(ln.split()[1:4]): ln.split()[4] for ln in stdout.splitlines() if ln.startswith("CASE")}


@pytest.mark.parametrize("which", [0, 1], ids=["deferred_stores", "MI_SWEEP_DEFER=0"])
def test_every_case_reproduces_the_streaming_kernel_and_keeps_the_guard(runs, which):
    """each child asserts, case by case: three back-to-back calls equal the streaming path (NaN-normalised), the 16 384
    doubles behind the result vector still hold the sentinel, and the new kernel was launched exactly when expected"""
    rc, so, se = runs[which]
    assert rc == 0 and "DONE" in so, so[-1500:] + se[-2500:]
    assert len(_cases(so)) == len(KINDS) * 10 * len(TAILS)
    assert all(("AUTO %s ok" % k) in so for k in KINDS)


def test_digests_equal_those_of_the_forwarding_run(runs):
    """sha256 of every result vector: new kernel == MI_SWEEP_DEFER=0 (mi_interp1_f64_dev's own kernels)"""
    new, old = _cases(runs[0][1]), _cases(runs[1][1])
    assert new and new.keys() == old.keys()
    assert [k for k in new if new[k] != old[k]] == []


DEFAULTS = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
import armadillocudalinearinterpolation_amd as mi
from armadillocudalinearinterpolation_amd import synth, _lib
ctx = mi.Context(0)
C = ctx.device_info()["compute_units"]
L = _lib.load()
dev = torch.device("cuda", 0)
def launches(grid, xq, want):
    before = L.mi_debug_sweep_ds_launches()
    got = grid.interp(xq)
    n = L.mi_debug_sweep_ds_launches() - before
    ctx.set_query_order(2)
    ref = grid.interp(xq)
    ctx.set_query_order(1)
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(ref, nan=-7.0)), want
    return n
ng = 1_000_000
X = np.arange(ng) / (ng - 1)
big = mi.Grid1.from_nodes(ctx, X, np.sin(2 * np.pi * X) + 0.5 * X, sanitise=False)            # 8 MB: region sweep
Xs = np.arange(10_000) / 9_999.0
small = mi.Grid1.from_nodes(ctx, Xs, np.cos(3 * Xs), sanitise=False)                           # 80 KB: table-in-LDS kernel
Xm = np.arange(300_000) / 299_999.0
mid = mi.Grid1.from_nodes(ctx, Xm, np.cos(3 * Xm), sanitise=False)                             # 2.4 MB: below the sweep's window
xq = synth.splitmix_uniform(11, 16 * C * 16384 + 5, dev) * 1.02 - 0.01
ctx.set_query_order(1)
assert launches(big, xq, "16 tiles per CU") == 1
assert launches(big, xq[:15 * C * 16384 + 5], "15 tiles per CU: the one-phase-after-the-other form") == 0
assert launches(small, xq, "table in LDS") == 0
assert launches(mid, xq, "table below 5 MiB") == 0
ctx.set_query_order(2)
before = L.mi_debug_sweep_ds_launches()
big.interp(xq)
assert L.mi_debug_sweep_ds_launches() == before, "ordered hint: streaming kernel"
print("DONE")
"""


def test_default_dispatch_takes_the_new_kernel_only_where_the_pipelined_form_ran():
    """no environment overrides: from 16 tiles per CU over a table beyond 5 MiB the new kernel is launched; fewer tiles,
    a table that fits LDS, a table below the sweep's window and the ORDERED hint are forwarded (launch counter unchanged)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI_SWEEP_")}
    r = subprocess.run([sys.executable, "-c", DEFAULTS % {"root": ROOT}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-1500:] + r.stderr[-2500:]
