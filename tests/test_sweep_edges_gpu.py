"""GPU checks of the three region-sweep kernels of interp1 -- the one-phase form and the pipelined two-group form
and its deferred-store form (DEFER > 0), both csrc/mi_interp1_sweep.hpp -- on the cases of tests/sweep_cases.py:
eight tables (every table mode; closed forms 0, 1 and 3, with and without a pinned last node, asserted from the
library's own answer) and a query vector whose tiles have sharply different region histograms (a whole tile in one
region, only NaN, only out of range on one side, every node with its ulp neighbours, ...), so that the two tiles a
workgroup holds at one moment never look alike.

EVERY element is compared with oracle.interp1_bracket (held to the literal Armadillo scan and to the exact rational
interpolant in tests/test_sweep_cases_cpu.py): NaN where the oracle has NaN, the same 64 bits everywhere else, the sign of
zero included.  Every prefix size is also compared with the streaming kernel, three calls run back to back into a
buffer whose 16 384 doubles behind the result must keep their sentinel, and mi_debug_sweep_ds_launches proves which
kernel ran.  Extrapolation values NaN and -3.25 at every size, -0.0 and +inf at the largest.

The environment hooks are read once per process, so each kernel form runs in a child process of its own; the three are
started together and must print the same digests.

The same vector also goes to tables inside the window of the whole-table-in-LDS kernel (interp1_lds_kernel), which had
the same blind spot: closed form n = 16 383 and jitter n = 8191, the largest that fit 128 KiB with their padding node.
Nothing proves which kernel ran there beyond the launch counter staying put: the dispatch rule of launch_mode
(csrc/mi_interp1.hip: unordered hint, table within the window, at least 2^20 queries) is what selects it.  n = 16 384 and
n = 8192 run as well: their padding node puts them 8 and 16 bytes past the window, so under the hooks they take the
sweep (the counter says so)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTABLES, NSIZES, NPATTERNS = 8, 10, 13
LDS_CASES = (("lds_closed", "cf_div", 16383, 0, True), ("lds_jitter", "jitter", 8191, 3, True),
             ("lds_closed", "cf_div", 16384, 0, False), ("lds_jitter", "jitter", 8192, 3, False))

CHILD = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import armadillocudalinearinterpolation_amd as mi
from armadillocudalinearinterpolation_amd import _lib
import oracle
import sweep_cases as sc
TILE, GUARD, SENT = sc.TILE, 16384, -12345.678
EXPECT = %(expect)d                       # launches of the deferred-store kernel per call that takes the sweep
ctx = mi.Context(0)
C = ctx.device_info()["compute_units"]
L = _lib.load()
dev = torch.device("cuda", 0)
sizes = sc.prefix_sizes(C)
nmax = sizes[-1][2]
pat = sc.pattern_index(C)
threads = max(1, min(5, oracle.max_threads()))
print("CU", C, "NMAX", nmax, flush=True)
buf = torch.empty(nmax + GUARD, dtype=torch.float64, device=dev)
sbuf = torch.empty(nmax, dtype=torch.float64, device=dev)

class Ref:
    # the oracle's answer on the device: its bits and where it is NaN
    def __init__(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.bits = torch.from_numpy(a.view(np.int64)).to(dev)
        self.nan = torch.from_numpy(np.isnan(a)).to(dev)

def check(tag, got, ref, lo, ntiles):
    # NaN where the oracle has NaN, the same 64 bits everywhere else
    n = got.numel()
    ok = torch.where(ref.nan[lo:lo + n], torch.isnan(got), got.view(torch.int64) == ref.bits[lo:lo + n])
    if bool(ok.all()):
        return
    bad = torch.nonzero(~ok).flatten()
    print("MISMATCH", tag, "count", bad.numel(), flush=True)
    grid = max(1, min(ntiles, C))
    for i in bad[:24].tolist():
        t = (lo + i) // TILE
        where = ("tile %%d workgroup %%d local %%d group %%d" %% (t, t %% grid, t // grid, (t // grid) & 1)) if t < ntiles else "tail"
        print("  index", lo + i, "pattern", int(pat[lo + i]), where, "got", got[i].item().hex(), "want",
              np.int64(ref.bits[lo + i].item()).view(np.float64).item().hex(), flush=True)
    by_pat = np.bincount(pat[lo:lo + n][(~ok).cpu().numpy()], minlength=sc.NPATTERNS)
    print("  mismatches by pattern", by_pat.tolist(), flush=True)
    raise SystemExit(3)

def sweep_calls(grid, xq, out, extrap, want_launches, tag):
    # three calls back to back into the same buffer, nothing waited for in between
    buf.fill_(SENT)
    ctx.set_query_order(1)
    before = L.mi_debug_sweep_ds_launches()
    for _ in range(3):
        grid.interp(xq, out=out, extrap=extrap)
    launched = L.mi_debug_sweep_ds_launches() - before
    assert launched == want_launches, (tag, launched, want_launches)

def guard_ok(nq, tag):
    assert bool((buf[nq:] == SENT).all()), ("guard", tag)

def digest(t):
    return hashlib.sha256(memoryview(t.cpu().numpy())).hexdigest()

for name in sc.TABLES:
    tab = sc.table(name)
    X, Y = tab["X"], tab["Y"]
    grid = mi.Grid1.from_nodes(ctx, X, Y, sanitise=False)
    info = grid.info()
    assert info["mode"] == tab["mode"], (name, info)
    if tab["mode"] == 0:
        assert (info["formula"], info["pin_last"]) == (tab["formula"], tab["pin_last"]), (name, info)
    else:
        assert (info["formula"], info["pin_last"]) == (-1, -1), (name, info)
    print("TABLE", name, "mode", info["mode"], "formula", info["formula"], "pin_last", info["pin_last"], flush=True)
    xq_np = sc.query_vector(name, C)
    ref_np = oracle.interp1_bracket(X, Y, xq_np, nthreads=threads)          # on ALL of it
    xq = torch.from_numpy(xq_np).to(dev)
    for extrap in (float("nan"), -3.25, -0.0, float("inf")):
        first = extrap != extrap
        ref = Ref(ref_np if first else sc.with_extrap(ref_np, xq_np, X, extrap))
        for T, tail, nq in (sizes if (first or extrap == -3.25) else sizes[-1:]):
            tag = (name, T, tail, extrap)
            out = buf[:nq]
            sweep_calls(grid, xq[:nq], out, extrap, 3 * EXPECT, tag)
            check(tag, out, ref, 0, T)
            guard_ok(nq, tag)
            ctx.set_query_order(2)                                          # the streaming kernel on the same prefix
            grid.interp(xq[:nq], out=sbuf[:nq], extrap=extrap)
            check(tag + ("streaming",), sbuf[:nq], ref, 0, 0)
            assert torch.equal(out.view(torch.int64), sbuf[:nq].view(torch.int64)), tag
            if first:
                print("CASE", name, T, tail, digest(out), ",".join(str(c) for c in np.bincount(pat[:nq], minlength=sc.NPATTERNS)), flush=True)
        if first:
            # below one tile there is no sweep to take: the streaming kernel, whatever the hooks say
            lo = 7 * TILE                                                   # (pattern 7: nodes and their ulp neighbours)
            for nq in (1, 100, 16383):
                out = buf[:nq]
                sweep_calls(grid, xq[lo:lo + nq], out, extrap, 0, (name, "small", nq))
                check((name, "small", nq), out, ref, lo, 0)
                guard_ok(nq, (name, "small", nq))
            print("SMALL", name, "ok", flush=True)
            # AUTO: the probe's verdict on this vector is arbitrary, and the results must not depend on it
            ctx.set_query_order(0)
            for k in range(2):
                got = grid.interp(xq)
                ctx.synchronize()
                check((name, "auto", k), got, ref, 0, sizes[-1][0])
            print("AUTO", name, "ok", flush=True)
    grid.close()

for label, kind, n, mode, inside in %(lds)r:
    X = sc.make_nodes(kind, n)
    Y = sc.make_values(X)
    grid = mi.Grid1.from_nodes(ctx, X, Y, sanitise=False)
    info = grid.info()
    assert info["mode"] == mode and (info["table_bytes"] <= 128 * 1024) == inside, (label, n, info)
    xq_np = sc.query_vector(label, C, n, kind)
    assert xq_np.size >= 1 << 20
    ref = Ref(oracle.interp1_bracket(X, Y, xq_np, nthreads=threads))
    xq = torch.from_numpy(xq_np).to(dev)
    out = buf[:nmax]
    # inside the window the table-in-LDS kernel comes first in both dispatchers: the sweep's counter stays put
    sweep_calls(grid, xq, out, float("nan"), 0 if inside else 3 * EXPECT, (label, n))
    check((label, n), out, ref, 0, sizes[-1][0])
    guard_ok(nmax, (label, n))
    print("LDS", label, n, digest(out), flush=True)
    grid.close()
print("DONE", flush=True)
"""

FORMS = [("deferred_stores", {"MI_SWEEP_VARIANT": "2"}, 1),
         ("pipelined", {"MI_SWEEP_VARIANT": "2", "MI_SWEEP_DEFER": "0"}, 0),
         ("one_phase", {"MI_SWEEP_VARIANT": "1"}, 0)]


def _start(extra, expect):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI_SWEEP_")}
    env.update(MI_SWEEP_MIN_BYTES="0", MI_SWEEP_MIN_TILES_PER_CU="0", **extra)
    prog = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "expect": expect, "lds": LDS_CASES}
    return subprocess.Popen([sys.executable, "-c", prog], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


@pytest.fixture(scope="module")
def runs():
    """(returncode, stdout, stderr) of the three children, started together"""
    procs = [_start(extra, expect) for _, extra, expect in FORMS]
    out = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        out.append((p.returncode, so, se))
    return out


def _lines(stdout, key):
    return [ln.split()[1:] for ln in stdout.splitlines() if ln.startswith(key + " ")]


def _digests(stdout):
    d = {("CASE",) + tuple(f[:3]): f[3] for f in _lines(stdout, "CASE")}
    d.update({("LDS",) + tuple(f[:2]): f[2] for f in _lines(stdout, "LDS")})
    return d


@pytest.mark.parametrize("which", range(len(FORMS)), ids=[f[0] for f in FORMS])
def test_every_element_equals_the_oracle_bit_for_bit(runs, which):
    """each child asserts, table by table and size by size: mode, closed form and pinned last node as the cases state
    them; three back-to-back calls of its sweep kernel, the streaming kernel and (below one tile, under AUTO, inside the
    LDS window) whatever the dispatch picks equal the oracle on every element; the guard keeps its sentinel; the
    deferred-store kernel was launched exactly when this child's hooks say so.  A mismatch is printed with its pattern,
    tile, workgroup, local tile index and wave group."""
    import sweep_cases as sc
    rc, so, se = runs[which]
    assert rc == 0 and "DONE" in so, so[-3000:] + se[-3000:]
    cases = _lines(so, "CASE")
    assert len(cases) == NTABLES * NSIZES and len({tuple(c[:3]) for c in cases}) == NTABLES * NSIZES
    tables = {f[0]: (int(f[2]), int(f[4]), int(f[6])) for f in _lines(so, "TABLE")}
    assert tables == {n: (m, -1 if f is None else f, -1 if p is None else p) for n, (m, f, p) in sc.TABLE_SPECS.items()}
    # closed forms 0, 1 and 3, each pinned-last-node state of 0 and 1, and the {x,y} modes 1, 2 and 3 all ran
    assert {(f, p) for m, f, p in tables.values() if m == 0} == {(0, 0), (0, 1), (1, 0), (1, 1), (3, 0)}
    assert {m for m, _, _ in tables.values()} == {0, 1, 2, 3}
    for name in sc.TABLES:
        per_size = [[int(x) for x in c[4].split(",")] for c in cases if c[0] == name]
        assert len(per_size) == NSIZES and all(len(p) == NPATTERNS for p in per_size)
        assert all(sum(p) == int(c[1]) * sc.TILE + int(c[2]) for p, c in zip(per_size, [c for c in cases if c[0] == name]))
        assert min(per_size[-1]) >= 3 * sc.TILE          # the full vector: every pattern, in several tiles
        assert ("SMALL %s ok" % name) in so and ("AUTO %s ok" % name) in so
    assert len(_lines(so, "LDS")) == len(LDS_CASES)


def test_the_three_kernel_forms_print_the_same_digests(runs):
    """sha256 of every result vector: deferred-store form == pipelined form == one-phase form"""
    d = [_digests(r[1]) for r in runs]
    assert len(d[0]) == NTABLES * NSIZES + len(LDS_CASES)
    assert d[0].keys() == d[1].keys() == d[2].keys()
    assert [k for k in d[0] if not (d[0][k] == d[1][k] == d[2][k])] == []
