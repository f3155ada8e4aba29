"""GPU checks of the region sweep with the XCD groups out of phase (interp1_phased_sweep_kernel, csrc/mi_sweep_phase.hip).

mi_debug_interp1_phased_sweep launches the kernel on its own on at most 8 or 16 workgroups, so that every per-workgroup
tile count from 0 to 5 is reached with about 1.3e6 queries.  For phases 1, 2, 4, 8 the result must have the bytes of
mi_interp1_f64_dev on the same inputs (under the ORDERED hint that is the family's streaming kernel: another kernel over
the same eval_batch), must leave the 16 384 doubles behind the result alone, and on a 2^16 sample must have the bytes of
oracle.interp1_bracket.

Tables: the closed forms the table builder can produce at 4 099 nodes -- fma(i, dx, x0) (with and without a pinned
last node), x0 + i*dx and the division form, which the builder always stores as formula 3: the Markstein step is tried before the
IEEE division and is correctly rounded for every such denominator, so no table reaches formula 2 (tests/sweep_cases.py
has none either) -- and the 1e6-node table of the headline.

Tile counts T for W = 8, 16 workgroups (rank s owns tiles s, s + W, ...): fewer tiles than workgroups; k W (all equal);
k W + 1 (only the first workgroup of the earliest class has one more); k W + W/2 and k W + W - 1 (the late ranks one
fewer); up to 5 tiles per workgroup.  Tails 0, 1, 16 383, and calls below one tile (tail only).

The dispatch of mi_interp1_f64_dev_v2 and the launch counters are checked in two child processes (the switch is read
once per process) at the smallest shape the wrapper takes: 16 tiles per CU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import sweep_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, GUARD, SENT = 16384, 16384, -12345.678
PHASES = (1, 2, 4, 8)
WORKGROUPS = (8, 16)
TAILS = (0, 1, 16383)
NPAT = 5


def tile_counts(W):
    return [1, 3, W - 1, W, W + 1, W + W // 2, 2 * W - 1, 2 * W + 1, 3 * W + W // 2, 4 * W - 1, 4 * W + 1, 5 * W]


NMAX = 5 * max(WORKGROUPS) * TILE + max(TAILS)


def make_queries(X, seed):
    """NMAX queries, tile by tile: seeded uniform over the range widened by 1 %; all in one region; every query on a
    node; NaN, +-inf, -0.0 and values just outside both ends among uniform ones; uniform again"""
    rng = np.random.default_rng(seed)
    lo, hi = X[0], X[-1]
    span = hi - lo
    q = np.empty(NMAX, dtype=np.float64)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), lo, hi,
                        lo - span, hi + span, 1e300, -1e300, 5e-324, np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf)])
    for t in range(0, NMAX, TILE):
        n = min(TILE, NMAX - t)
        pat = (t // TILE) % NPAT
        if pat in (0, 4):
            v = lo - 0.01 * span + 1.02 * span * rng.random(n)
        elif pat == 1:                                   # one region of 256: every lane's histogram ticket from one counter
            r = int(rng.integers(0, 256))
            v = lo + span * (r + 0.02 + 0.96 * rng.random(n)) / 256.0
        elif pat == 2:
            v = X[rng.integers(0, X.size, n)]
        else:
            v = lo + span * rng.random(n)
            k = rng.integers(0, n, n // 3)
            v[k] = special[rng.integers(0, special.size, k.size)]
            v[:special.size] = special[:n]
        q[t:t + n] = v
    return q


class Case:
    pass


@pytest.fixture(scope="module")
def env():
    import torch
    import armadillocudalinearinterpolation_amd as mi
    from armadillocudalinearinterpolation_amd import _lib
    e = Case()
    e.torch, e.mi, e.L, e.check = torch, mi, _lib.load(), _lib.check
    e.ctx = mi.Context(0)
    e.dev = torch.device("cuda", 0)
    e.buf = torch.empty(NMAX + GUARD, dtype=torch.float64, device=e.dev)
    yield e
    e.ctx.close()


def _tables():
    out = [(name, sc.make_nodes(name, 4099), sc.TABLE_SPECS[name][1:]) for name in ("cf_fma_pinned", "cf_mul", "cf_fma", "cf_div")]
    ng = 1_000_000
    out.append(("headline_1e6", np.arange(ng) / (ng - 1), None))
    return out


@pytest.fixture(scope="module", params=range(5), ids=["cf_fma_pinned", "cf_mul", "cf_fma", "cf_div", "headline_1e6"])
def table(env, request):
    """the table, its queries on the device, and mi_interp1_f64_dev's answer on all of them for extrap NaN and -0.0 (computed once)"""
    torch = env.torch
    name, X, spec = _tables()[request.param]
    Y = sc.make_values(X)
    t = Case()
    t.name, t.X, t.Y = name, X, Y
    t.grid = env.mi.Grid1.from_nodes(env.ctx, X, Y, sanitise=False)
    info = t.grid.info()
    assert info["mode"] == 0, info
    if spec is not None:
        assert (info["formula"], info["pin_last"]) == spec, (name, info)
    t.q_np = make_queries(X, 1000 + request.param)
    t.q = torch.from_numpy(t.q_np).to(env.dev)
    t.ref = {}
    env.ctx.set_query_order(2)                       # ORDERED: the family's streaming kernel
    for key, extrap in (("nan", float("nan")), ("negzero", -0.0)):
        r = torch.empty(NMAX, dtype=torch.float64, device=env.dev)
        env.check(env.L.mi_interp1_f64_dev(env.ctx._h, t.grid._h, ctypes.c_void_p(t.q.data_ptr()), ctypes.c_void_p(r.data_ptr()),
                                           NMAX, extrap), env.ctx._h)
        t.ref[key] = r
    env.ctx.set_query_order(1)
    yield t
    t.grid.close()


def _phased(env, t, nq, extrap, phases, W):
    env.buf.fill_(SENT)
    env.check(env.L.mi_debug_interp1_phased_sweep(env.ctx._h, t.grid._h, ctypes.c_void_p(t.q.data_ptr()),
                                                  ctypes.c_void_p(env.buf.data_ptr()), nq, extrap, phases, W), env.ctx._h)
    return env.buf[:nq]


def _same_bytes(env, a, b):
    return env.torch.equal(a.view(env.torch.int64), b.view(env.torch.int64))


@pytest.mark.parametrize("W", WORKGROUPS)
@pytest.mark.parametrize("phases", PHASES)
def test_bytes_of_the_streaming_kernel_at_every_tile_count(env, table, phases, W):
    before = env.L.mi_debug_sweep_ds_launches()
    base_before = env.L.mi_debug_sweep_ds_launches_base()
    calls = 0
    for k, T in enumerate(tile_counts(W)):
        # every tail at the counts around one and two tiles per workgroup and at the largest, one tail (in turn) elsewhere
        tails = TAILS if T in (W - 1, W, W + 1, 2 * W + 1, 5 * W) else (TAILS[k % 3],)
        for tail in tails:
            nq = T * TILE + tail
            out = _phased(env, table, nq, float("nan"), phases, W)
            calls += 1
            assert _same_bytes(env, out, table.ref["nan"][:nq]), (table.name, phases, W, T, tail)
            assert bool((env.buf[nq:] == SENT).all()), ("guard", table.name, phases, W, T, tail)
    assert env.L.mi_debug_sweep_ds_launches() - before == calls
    assert env.L.mi_debug_sweep_ds_launches_base() == base_before


@pytest.mark.parametrize("phases", PHASES)
def test_below_one_tile_and_the_other_extrapolation_value(env, table, phases):
    for W in WORKGROUPS:
        for nq in (1, 2, 100, 4097, 16383):                                   # tail only: one workgroup, no tile
            off = 3 * TILE                                                    # (the tile with the special values)
            env.buf.fill_(SENT)
            q = table.q[off:off + nq]
            env.check(env.L.mi_debug_interp1_phased_sweep(env.ctx._h, table.grid._h, ctypes.c_void_p(q.data_ptr()),
                                                          ctypes.c_void_p(env.buf.data_ptr()), nq, float("nan"), phases, W), env.ctx._h)
            assert _same_bytes(env, env.buf[:nq], table.ref["nan"][off:off + nq]), (table.name, phases, W, nq)
            assert bool((env.buf[nq:] == SENT).all()), ("guard", table.name, phases, W, nq)
        for T, tail in ((2 * W + 1, 16383), (3 * W + W // 2, 1)):
            nq = T * TILE + tail
            out = _phased(env, table, nq, -0.0, phases, W)
            assert _same_bytes(env, out, table.ref["negzero"][:nq]), (table.name, phases, W, T, tail)


def test_bytes_of_the_oracle_on_a_sample(env, table):
    idx = np.unique(np.concatenate([np.random.default_rng(5).integers(0, NMAX, 1 << 16), np.arange(3 * TILE, 3 * TILE + 64)]))
    threads = max(1, min(4, oracle.max_threads()))
    want = oracle.interp1_bracket(table.X, table.Y, table.q_np[idx], nthreads=threads)
    for extrap, ref in ((float("nan"), want), (-0.0, sc.with_extrap(want, table.q_np[idx], table.X, -0.0))):
        for phases, W in ((2, 16), (8, 8)):
            out = _phased(env, table, NMAX, extrap, phases, W).cpu().numpy()
            assert sc.same_bits(out[idx], ref), (table.name, phases, W, extrap)


def test_probe_for_the_next_call_runs_under_the_auto_hint(env, table):
    """AUTO: the last-ranked workgroup's last wave probes the query order while the kernel runs; results as ever"""
    env.ctx.set_query_order(0)
    try:
        for phases in PHASES:
            nq = 21 * TILE + 1
            out = _phased(env, table, nq, float("nan"), phases, 8)
            env.ctx.synchronize()
            assert _same_bytes(env, out, table.ref["nan"][:nq]), (table.name, phases)
    finally:
        env.ctx.set_query_order(1)


def test_debug_entry_point_rejects_what_the_kernel_does_not_serve(env, table):
    torch, L = env.torch, env.L
    q, o = ctypes.c_void_p(table.q.data_ptr()), ctypes.c_void_p(env.buf.data_ptr())
    assert L.mi_debug_interp1_phased_sweep(env.ctx._h, table.grid._h, q, o, TILE, 0.0, 3, 8) == 1
    assert L.mi_debug_interp1_phased_sweep(env.ctx._h, table.grid._h, q, o, TILE, 0.0, 0, 8) == 1
    assert L.mi_debug_interp1_phased_sweep(env.ctx._h, table.grid._h, q, o, TILE, 0.0, 2, 0) == 1
    assert L.mi_debug_interp1_phased_sweep(env.ctx._h, table.grid._h, ctypes.c_void_p(table.q.data_ptr() + 8), o, TILE, 0.0, 2, 8) == 1
    assert L.mi_debug_interp1_phased_sweep(env.ctx._h, None, q, o, TILE, 0.0, 2, 8) == 1
    assert L.mi_debug_interp1_phased_sweep(env.ctx._h, table.grid._h, q, o, 0, 0.0, 2, 8) == 0      # nothing to do
    if table.name == "cf_fma":
        Xj = sc.make_nodes("jitter", 4099)
        g3 = env.mi.Grid1.from_nodes(env.ctx, Xj, sc.make_values(Xj), sanitise=False)
        assert g3.info()["mode"] == 3
        assert L.mi_debug_interp1_phased_sweep(env.ctx._h, g3._h, q, o, TILE, 0.0, 2, 8) == 1     # {x,y} tables: not this kernel
        g3.close()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the wrapper: dispatch and counters, one process per switch value
CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
import armadillocudalinearinterpolation_amd as mi
from armadillocudalinearinterpolation_amd import synth, _lib
ctx = mi.Context(0)
C = ctx.device_info()["compute_units"]
L = _lib.load()
dev = torch.device("cuda", 0)
free = torch.cuda.mem_get_info(0)[0]
nq = 16 * C * 16384 + 5
if free < 4 * nq * 8:
    print("SHORT OF MEMORY")
    raise SystemExit(0)
ng = 1_000_000
X = np.arange(ng) / (ng - 1)
big = mi.Grid1.from_nodes(ctx, X, np.sin(2 * np.pi * X) + 0.5 * X, sanitise=False)
Xm = np.arange(300_000) / 299_999.0
mid = mi.Grid1.from_nodes(ctx, Xm, np.cos(3 * Xm), sanitise=False)
xq = synth.splitmix_uniform(11, nq, dev) * 1.02 - 0.01
xq[torch.tensor([0, 5, 16384, nq - 1], device=dev)] = float("nan")
ctx.set_query_order(2)
ref = big.interp(xq)
ctx.set_query_order(1)
def counts():
    return L.mi_debug_sweep_ds_launches(), L.mi_debug_sweep_ds_launches_base()
def run(grid, q):
    t0, b0 = counts()
    out = grid.interp(q)
    t1, b1 = counts()
    return out, t1 - t0, b1 - b0
out, total, base = run(big, xq)
assert torch.equal(out.view(torch.int64), ref.view(torch.int64))
print("BIG", total, base, int(out.view(torch.int64).sum().item()))
_, total, base = run(big, xq[:15 * C * 16384 + 5])
print("FEWER_TILES", total, base)
_, total, base = run(mid, xq)
print("SMALL_TABLE", total, base)
_, total, base = run(big, xq[1:])
print("UNALIGNED", total, base)
ctx.set_query_order(2)
_, total, base = run(big, xq)
print("ORDERED", total, base)
print("DONE")
"""


@pytest.fixture(scope="module")
def children():
    """the child with two phase classes and the child with the switch at 0, started together"""
    procs = []
    for value in ("2", "0"):
        e = {k: v for k, v in os.environ.items() if not k.startswith("MI_SWEEP_")}
        e["MI_SWEEP_XCD_PHASES"] = value
        procs.append(subprocess.Popen([sys.executable, "-c", CHILD % {"root": ROOT}], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True, env=e))
    out = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        out.append((p.returncode, so, se))
    if any("SHORT OF MEMORY" in so for _, so, _ in out):
        pytest.skip("not enough free device memory for 16 tiles per CU")
    return out


def _lines(stdout):
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in stdout.splitlines() if ln and ln.split()[0].isupper() and ln != "DONE"}


def test_wrapper_launches_the_phased_kernel_exactly_where_the_deferred_store_sweep_ran(children):
    rc, so, se = children[0]
    assert rc == 0 and "DONE" in so, so[-1500:] + se[-2500:]
    got = _lines(so)
    assert got["BIG"][:2] == [1, 0]                       # one launch per Grid1.interp, and not the family's kernel
    # forwarded: the family's own choice (none of these is its deferred-store sweep either)
    assert got["FEWER_TILES"] == [0, 0] and got["SMALL_TABLE"] == [0, 0] and got["UNALIGNED"] == [0, 0] and got["ORDERED"] == [0, 0]


def test_switch_at_zero_forwards_to_the_base_with_equal_results(children):
    rc, so, se = children[1]
    assert rc == 0 and "DONE" in so, so[-1500:] + se[-2500:]
    got = _lines(so)
    assert got["BIG"][:2] == [1, 1]                       # the family's deferred-store kernel, counted in both
    assert got["FEWER_TILES"] == [0, 0] and got["SMALL_TABLE"] == [0, 0] and got["UNALIGNED"] == [0, 0] and got["ORDERED"] == [0, 0]
    # both children hold their result to the streaming kernel's bytes; the checksums of the two say the same
    assert got["BIG"][2] == _lines(children[0][1])["BIG"][2]
