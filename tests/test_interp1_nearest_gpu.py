"""arma::interp1's "nearest" method on the device: mi_interp1_nearest_f64_dev / _host / mi_interp1_nearest_f64
(Grid1.interp_nearest, .interp_nearest_host, interp1_nearest), mi_interp1_cols_nearest_f64_dev (Axis1.interp_cols_nearest)
and the C++ method strings (mi355::interp1(..., method), Interp1Table::nearest).

Every comparison is nearest_cases._eq_bits against nearest_cases.nearest_rule (held to the literal Armadillo scan in
tests/test_interp1_nearest_cpu.py): NaN in the same positions, the same 64 bits everywhere else, on every element -- no
tolerance, no sampling.  mi_debug_nearest_launches proves which form ran: 0 streaming, 1 table in LDS, 2 scalar,
3 columns LDS form, 4 columns direct form.  The largest input is interp1_value_cases.NQ_LDS = 2^20 + 4099 queries."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import interp1_value_cases as vc
import nearest_cases as nc
import oracle
import sweep_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "host")
STREAM, LDS, SCALAR, COLS_LDS, COLS_DIRECT = 0, 1, 2, 3, 4
LDS_MAX_N = 8192          # kLdsMaxN in csrc/mi_nearest1.hip: the columns' LDS form up to here, the direct form beyond
ROW_BLOCK = 2048          # kRowBlock: outputs of one column per unit of work
LAUNCH_SHAPE = 1024       # queries of one workgroup of the streaming kernel (256 lanes x 2 vectors x 2)
SENTINEL = -12345.678
GUARD = 16                # sentinel elements on both sides of a result


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()        # (a writable copy: the shared cases are read-only)


def _forms(L):
    return [L.mi_debug_nearest_launches(f) for f in range(5)]


def _delta(L, before):
    return [a - b for a, b in zip(_forms(L), before)]


def _only(form, count=1):
    d = [0] * 5
    d[form] = count
    return d


def _nearest(ctx, grid, xq_np, extrap, want_form, misalign=False):
    """one device call into a buffer with sentinels on both sides; misalign: xq and yq 8-B but not 16-B aligned.
    Asserts the form that ran and that nothing outside the result was written."""
    import torch
    L = ctx._L
    nq = xq_np.size
    off = GUARD + (1 if misalign else 0)
    xbuf = torch.empty(nq + 2, dtype=torch.float64, device="cuda")
    xq = xbuf[1:1 + nq] if misalign else xbuf[:nq]
    xq.copy_(torch.from_numpy(np.array(xq_np, dtype=np.float64)))        # (a writable copy: the shared cases are read-only)
    buf = torch.full((nq + 2 * GUARD + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    out = buf[off:off + nq]
    assert xbuf.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    assert nq == 0 or ((xq.data_ptr() % 16 != 0) == misalign and (out.data_ptr() % 16 != 0) == misalign)
    before = _forms(L)
    got = grid.interp_nearest(xq, out=out, extrap=extrap)
    assert _delta(L, before) == (_only(want_form) if nq else [0] * 5), (_delta(L, before), want_form)
    h = buf.cpu().numpy()
    assert np.all(h[:off] == SENTINEL) and np.all(h[off + nq:] == SENTINEL), "wrote outside the result"
    assert got.data_ptr() == out.data_ptr()
    return h[off:off + nq].copy()


# ---------------------------------------------------------------------------------------------------- table lookup
@pytest.mark.parametrize("name", sc.TABLES + ["uniform"])
def test_streaming_form_in_every_table_mode(mi_ctx, name):
    """n = 50 000 nodes, the CPU file's 33 007 queries: every table mode and closed form through the streaming kernel"""
    import armadillocudalinearinterpolation_amd as mi
    if name == "uniform":
        x0, dx = -1.0, 2.0 ** -7
        t = sc.table("cf_fma")
        X, Y, want = t["X"], t["Y"], (0, 0, 0)
        assert np.array_equal(X, x0 + dx * np.arange(X.size))
        grid = mi.Grid1.uniform(mi_ctx, x0, dx, Y)
        xq = nc.sweep_queries("cf_fma")
    else:
        t = sc.table(name)
        X, Y = t["X"], t["Y"]
        want = tuple(-1 if v is None else v for v in sc.TABLE_SPECS[name])
        grid = mi.Grid1.from_nodes(mi_ctx, X, Y, sanitise=False)
        xq = nc.sweep_queries(name)
    info = grid.info()
    formula, pin = C.c_int(0), C.c_int(0)
    assert mi_ctx._L.mi_debug_grid1_formula(grid._h, C.byref(formula), C.byref(pin)) == 0
    assert (info["mode"], info["formula"], info["pin_last"]) == want == (info["mode"], formula.value, pin.value)
    assert X.size == (49_997 if name == "clustered" else 50_000)    # clustered: made unique after its shift (sweep_cases)
    for extrap in (np.nan, -3.25):
        got = _nearest(mi_ctx, grid, xq, extrap, STREAM)
        assert nc._eq_bits(got, nc.nearest_rule(X, Y, xq, extrap)), (name, extrap)
    grid.close()


@functools.lru_cache(maxsize=None)
def _value_ref(name, variant):
    ref = nc.nearest_rule(vc.nodes(name), vc.values(name, variant), vc.queries(name), 7.5)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("variant", vc.VARIANTS)
@pytest.mark.parametrize("name", sorted(vc.SPECS))
def test_values_come_back_as_they_are_in_every_form(mi_ctx, name, variant):
    """inf, -0.0, denormals and NaN in Y, the last node among them: BIG tables through the streaming and the scalar
    form; the LDS-window tables through the LDS form (unordered hint), the streaming form (ordered hint) and the scalar
    form (xq and yq offset by 8 B) -- all equal to the rule and therefore to each other, bit for bit"""
    import armadillocudalinearinterpolation_amd as mi
    X, Y, xq = vc.nodes(name), vc.values(name, variant), vc.queries(name)
    ref = _value_ref(name, variant)
    grid = mi.Grid1.from_nodes(mi_ctx, X, Y, sanitise=False)
    assert grid.info()["mode"] == vc.SPECS[name][2]
    try:
        got = {}
        if name in vc.LDS:
            assert xq.size == vc.NQ_LDS
            mi_ctx.set_query_order(1)
            got["lds"] = _nearest(mi_ctx, grid, xq, 7.5, LDS)
            mi_ctx.set_query_order(2)
            got["stream"] = _nearest(mi_ctx, grid, xq, 7.5, STREAM)
            mi_ctx.set_query_order(0)
            got["auto"] = _nearest(mi_ctx, grid, xq, 7.5, LDS)        # AUTO: the window decides, no probe
            mi_ctx.set_query_order(1)
        else:
            got["stream"] = _nearest(mi_ctx, grid, xq, 7.5, STREAM)
        got["scalar"] = _nearest(mi_ctx, grid, xq, 7.5, SCALAR, misalign=True)
        for form, g in got.items():
            assert nc._eq_bits(g, ref), (name, variant, form)
        assert np.isnan(ref).any() and np.isinf(ref).any() and (np.signbit(ref) & (ref == 0)).any()
    finally:
        mi_ctx.set_query_order(0)
        grid.close()


@pytest.mark.parametrize("nq", [0, 1, 2, 3, LAUNCH_SHAPE - 1, LAUNCH_SHAPE, LAUNCH_SHAPE + 1, 4099])
def test_sizes_tails_and_sentinels(mi_ctx, nq):
    """tables of two and three nodes (closed form and {x,y}); nq of 0..3, one launch shape +- 1 and an odd tail, 16-B
    aligned and not; the sentinels on both sides of yq survive (checked in _nearest)"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(nq)
    for X in (np.array([0.0, 1.0]), np.array([-1.0, 0.25, 3.0]), np.array([2.0, 2.5, 3.0])):
        Y = np.array([-0.0, np.inf, 5e-324])[:X.size]
        grid = mi.Grid1.from_nodes(mi_ctx, X, Y, sanitise=False)
        span = X[-1] - X[0]
        xq = X[0] - 0.2 * span + 1.4 * span * rng.random(nq)
        edge = np.concatenate([X, 0.5 * X[:-1] + 0.5 * X[1:], [np.nan]])
        m = min(nq, edge.size)
        xq[:m] = rng.permutation(edge)[:m]
        ref = nc.nearest_rule(X, Y, xq, -1.0)
        assert nc._eq_bits(_nearest(mi_ctx, grid, xq, -1.0, STREAM), ref)
        assert nc._eq_bits(_nearest(mi_ctx, grid, xq, -1.0, SCALAR, misalign=True), ref)
        grid.close()


PROBE_CHILD = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import armadillocudalinearinterpolation_amd as mi
from armadillocudalinearinterpolation_amd import _lib
import interp1_value_cases as vc, nearest_cases as nc, sweep_cases as sc, oracle
L = _lib.load()
dev = torch.device("cuda", 0)
name, variant = "cf_mul_pinned", "nan_last"            # 50 000 nodes, mode 0, 400 KB: outside the LDS window
X, Y = vc.nodes(name), vc.values(name, variant)
NQ = vc.NQ_LDS                                         # 64 tiles and a tail
rng = np.random.default_rng(41)
span = X[-1] - X[0]
rnd = (X[0] - 0.01 * span) + 1.02 * span * rng.random(NQ)
srt = np.sort(X[0] + span * (0.25 + 0.5 * rng.random(NQ)))      # 4096 places on: half a region (of 256) further
sets = {"random": rnd, "sorted": srt}
lin_ref = {k: oracle.interp1_bracket(X, Y, q, np.nan, nthreads=8) for k, q in sets.items()}
near_ref = {k: nc.nearest_rule(X, Y, q) for k, q in sets.items()}
dsets = {k: torch.from_numpy(q.copy()).to(dev) for k, q in sets.items()}
SEQ = ["sorted", "sorted", "random", "random", "sorted", "sorted", "random", "random"]
other = {"sorted": "random", "random": "sorted"}

def run(with_nearest):
    ctx = mi.Context(0)                                # a fresh context: AUTO, no verdict yet
    grid = mi.Grid1.from_nodes(ctx, X, Y, sanitise=False)
    assert grid.info()["mode"] == 0
    deltas, forms0 = [], [L.mi_debug_nearest_launches(f) for f in range(5)]
    for k, key in enumerate(SEQ):
        if with_nearest:
            # the query set a probe would judge the other way than the linear call before it (the first: unordered)
            nk = other[SEQ[k - 1]] if k else "random"
            got = grid.interp_nearest(dsets[nk])
            ctx.synchronize()
            assert nc._eq_bits(got.cpu().numpy(), near_ref[nk]), ("nearest", k, nk)
        before = L.mi_debug_sweep_ds_launches()
        out = grid.interp(dsets[key])                  # mi_interp1_f64_dev_v2, AUTO
        deltas.append(L.mi_debug_sweep_ds_launches() - before)
        ctx.synchronize()                              # this call's verdict is in the mailbox before the next call reads it
        assert sc.same_bits(out.cpu().numpy(), lin_ref[key]), ("linear", k, key)
    forms = [L.mi_debug_nearest_launches(f) - a for f, a in enumerate(forms0)]
    assert forms == ([len(SEQ), 0, 0, 0, 0] if with_nearest else [0] * 5), forms      # the streaming form
    # the linear results on the shared value cases, after all that
    q = vc.queries(name)
    assert sc.same_bits(grid.interp(torch.from_numpy(q.copy()).to(dev)).cpu().numpy(), oracle.interp1_bracket(X, Y, q, np.nan))
    grid.close()
    ctx.close()
    return deltas

plain = run(False)
mixed = run(True)
print("PLAIN", plain)
print("MIXED", mixed)
print("DONE")
"""


def test_the_order_probe_is_left_alone():
    """AUTO on a table outside the LDS window, in a child process whose hooks make the region sweep eligible at this size
    (MI_SWEEP_MIN_BYTES=0, MI_SWEEP_MIN_TILES_PER_CU=0, MI_SWEEP_VARIANT=2), so that which kernel a linear call launches
    depends on the verdict the call before it left in the context's mailbox: no verdict -> probe and both kernels gated
    (no deferred-store launch), verdict unordered -> the deferred-store sweep (mi_debug_sweep_ds_launches + 1), verdict
    ordered -> the streaming kernel (+ 0).  Linear calls on sorted, sorted, random, random, sorted, sorted, random, random
    therefore count 0 0 0 1 1 0 0 1.  With a nearest call in front of every linear call -- on the query set a probe would
    judge the OTHER way -- the counts must be the same: a nearest kernel that wrote the mailbox, or a nearest dispatch
    that forgot the verdict, would change them."""
    env = dict(os.environ, MI_SWEEP_MIN_BYTES="0", MI_SWEEP_MIN_TILES_PER_CU="0", MI_SWEEP_VARIANT="2")
    env.pop("MI_SWEEP_DEFER", None)
    r = subprocess.run([sys.executable, "-c", PROBE_CHILD % {"root": ROOT}], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-1500:] + r.stderr[-2500:]
    seen = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in r.stdout.splitlines() if ln.startswith(("PLAIN", "MIXED"))}
    assert seen["PLAIN"] == seen["MIXED"] == str([0, 0, 0, 1, 1, 0, 0, 1]), seen


def test_host_form_and_one_shot(mi_ctx):
    """the host form and the sanitising one-shot equal the device form; nothing stays pinned; a permuted X gives the rule
    on the sorted table; an unsorted X without sanitising is MI_ERR_GRID"""
    import armadillocudalinearinterpolation_amd as mi
    L = mi_ctx._L
    name, variant = "jitter", "negzero_last"
    X, Y, xq = vc.nodes(name), vc.values(name, variant), vc.queries(name)
    ref = nc.nearest_rule(X, Y, xq, 0.5)
    grid = mi.Grid1.from_nodes(mi_ctx, X, Y, sanitise=False)
    dev = grid.interp_nearest(_t(xq), extrap=0.5).cpu().numpy()
    assert nc._eq_bits(dev, ref)
    before = _forms(L)
    host = grid.interp_nearest_host(xq, extrap=0.5)
    assert nc._eq_bits(host, dev) and L.mi_debug_pinned_ranges() == 0 and _delta(L, before) == _only(STREAM)
    out = np.full(xq.size, SENTINEL)
    assert grid.interp_nearest_host(xq, extrap=0.5, out=out) is out and nc._eq_bits(out, dev)
    assert grid.interp_nearest_host(np.empty(0)).size == 0
    grid.close()
    perm = np.random.default_rng(3).permutation(X.size)
    assert nc._eq_bits(mi.interp1_nearest(mi_ctx, X[perm], Y[perm], xq, extrap=0.5), ref)
    assert L.mi_debug_pinned_ranges() == 0
    with pytest.raises(mi.MiError) as e:
        mi.Grid1.from_nodes(mi_ctx, X[perm], Y[perm], sanitise=False)
    assert e.value.code == 2
    assert L.mi_interp1_nearest_f64_dev(mi_ctx._h, None, None, None, 4, 0.0) == 1          # NULL grid
    assert "mi_interp1_nearest_f64_dev" in L.mi_last_error(mi_ctx._h).decode()


def test_argument_checks_of_the_device_form(mi_ctx):
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, ch = mi_ctx._L, mi_ctx._h
    grid = mi.Grid1.from_nodes(mi_ctx, np.array([0.0, 1.0, 3.0]), np.array([1.0, 2.0, 3.0]), sanitise=False)
    x = torch.full((9,), 0.5, dtype=torch.float64, device="cuda")
    y = torch.full((9,), SENTINEL, dtype=torch.float64, device="cuda")
    p = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)  # noqa: E731
    err = lambda: (L.mi_last_error(ch) or b"").decode()  # noqa: E731
    before = _forms(L)
    assert L.mi_interp1_nearest_f64_dev(ch, grid._h, None, None, 0, 0.0) == 0          # nq == 0: nothing launched
    assert L.mi_interp1_nearest_f64_dev(ch, grid._h, None, p(y), 8, 0.0) == 1 and "NULL" in err()
    assert L.mi_interp1_nearest_f64_dev(ch, grid._h, p(x), None, 8, 0.0) == 1 and "mi_interp1_nearest_f64_dev" in err()
    assert L.mi_interp1_nearest_f64_dev(ch, grid._h, p(x, 4), p(y), 8, 0.0) == 1 and "aligned" in err()
    assert L.mi_interp1_nearest_f64_dev(ch, grid._h, p(x), p(y, 4), 8, 0.0) == 1 and "aligned" in err()
    assert L.mi_interp1_nearest_f64_host(ch, grid._h, None, None, 0, 0.0) == 0
    assert L.mi_interp1_nearest_f64_host(ch, grid._h, None, None, 3, 0.0) == 1 and "mi_interp1_nearest_f64_host" in err()
    assert _delta(L, before) == [0] * 5
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()), "a refused call wrote something"
    with pytest.raises(ValueError):
        grid.interp_nearest(x.float())
    with pytest.raises(ValueError):
        grid.interp_nearest(x, out=y[:4])
    grid.close()


def test_capture_and_replay(mi_ctx):
    """the device form allocates nothing and never synchronises: captured into a graph (one kernel) and replayed with
    fresh inputs in the same buffers, it equals the eager result"""
    import armadillocudalinearinterpolation_amd as mi
    import torch
    rng = np.random.default_rng(21)
    X = np.cumsum(rng.random(30000) + 0.01)
    Y = np.sin(X)
    grid = mi.Grid1.from_nodes(mi_ctx, X, Y, sanitise=False)
    q = rng.random(200001) * (X[-1] - X[0]) + X[0]
    xq = _t(q)
    eager = grid.interp_nearest(xq).cpu().numpy()
    assert nc._eq_bits(eager, nc.nearest_rule(X, Y, q))
    out = torch.zeros_like(xq)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(side):
            mi_ctx.use_torch_stream()
            grid.interp_nearest(xq, out=out)                                       # warm-up outside capture
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                mi_ctx.use_torch_stream()
                grid.interp_nearest(xq, out=out)
        torch.cuda.current_stream().wait_stream(side)
    finally:
        mi_ctx.use_torch_stream()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert nc._eq_bits(out.cpu().numpy(), eager)
    q2 = np.random.default_rng(1).random(q.size) * (X[-1] - X[0]) + X[0]
    xq.copy_(_t(q2))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert nc._eq_bits(out.cpu().numpy(), nc.nearest_rule(X, Y, q2))
    assert nc._eq_bits(grid.interp_nearest(xq).cpu().numpy(), out.cpu().numpy())
    grid.close()


# ---------------------------------------------------------------------------------------------------- matrix columns
# Matrices are kept as C-contiguous (B, ld) buffers: row c of the buffer is column c of the column-major matrix.
def _axis_queries(rng, nodes, n):
    """unsorted queries over the axis, with points out of range on both sides, NaN, both end nodes, interior nodes and
    cell midpoints (exact ties where the axis allows)"""
    lo, hi = nodes[0], nodes[-1]
    q = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n)
    if n >= 2:
        m = max(1, n // 5)
        q[rng.integers(0, n, m)] = nodes[rng.integers(0, nodes.size, m)]
        j = rng.integers(0, nodes.size - 1, m)
        q[rng.integers(0, n, m)] = 0.5 * nodes[j] + 0.5 * nodes[j + 1]
        q[rng.integers(0, n)] = hi
        q[rng.integers(0, n)] = lo
    if n >= 5:
        q[rng.integers(0, n)] = np.nan
    return q


def _jittered(rng, n):
    return np.cumsum(rng.uniform(0.2, 1.0, n)) - 3.0


def _rule_cols(X, Yb, xi, extrap=np.nan):
    """(B, nxi): row c = nearest_rule on column c (the picked node does not depend on the column)"""
    k = nc.rule_index(X, xi)
    return np.stack([nc._gather(Yb[c], k, extrap) for c in range(Yb.shape[0])]) if Yb.shape[0] else np.empty((0, xi.size))


def _grid1_cols(ctx, X, Yb, xi, extrap, uniform=None):
    """the same through a 1-D table per column on the device (Grid1.interp_nearest)"""
    import armadillocudalinearinterpolation_amd as mi
    xd = _t(xi)
    rows = []
    for c in range(Yb.shape[0]):
        g = mi.Grid1.uniform(ctx, uniform[0], uniform[1], Yb[c]) if uniform else mi.Grid1.from_nodes(ctx, X, Yb[c], sanitise=False)
        rows.append(g.interp_nearest(xd, extrap=extrap).cpu().numpy())
        g.close()
    return np.stack(rows)


def _run_cols(ctx, axis, Yb, xi, extrap=np.nan, ldy_pad=0, ldyi_pad=0, misalign=False, call=None):
    """the device call on column-major views with padded leading dimensions: NaN below each column of Y (must not leak),
    a sentinel below each column of YI (must survive); misalign: yi 8-B but not 16-B aligned.  Returns (B, nxi)."""
    import torch
    L = ctx._L
    B, n = Yb.shape
    nxi = xi.size
    buf = np.full((B, n + ldy_pad), np.nan)
    buf[:, :n] = Yb
    yd = _t(buf)
    ldyi = nxi + ldyi_pad
    flat = torch.full((B * ldyi + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    off = 0 if (flat.data_ptr() % 16 == 0) != misalign else 1
    ob = flat[off:off + B * ldyi].view(B, ldyi)
    assert (ob.data_ptr() % 16 != 0) == misalign
    before = _forms(L)
    got = (call or axis.interp_cols_nearest)(yd[:, :n].T, _t(xi), out=ob[:, :nxi].T, extrap=extrap)
    if call is None:
        assert _delta(L, before) == _only(COLS_LDS if n <= LDS_MAX_N else COLS_DIRECT)
    assert tuple(got.shape) == (nxi, B)
    h = flat.cpu().numpy()
    body = h[off:off + B * ldyi].reshape(B, ldyi)
    assert np.all(body[:, nxi:] == SENTINEL), "padding rows of YI were written"
    assert np.all(h[:off] == SENTINEL) and np.all(h[off + B * ldyi:] == SENTINEL), "wrote outside YI"
    return body[:, :nxi].copy()


def _check_cols(ctx, axis, X, Yb, xi, extrap=np.nan, uniform=None, **kw):
    got = _run_cols(ctx, axis, Yb, xi, extrap, **kw)
    assert nc._eq_bits(got, _rule_cols(X, Yb, xi, extrap))
    if Yb.shape[0] <= 8:
        assert nc._eq_bits(got, _grid1_cols(ctx, X, Yb, xi, extrap, uniform))
    return got


@pytest.mark.parametrize("n", [2, 3, 1024, LDS_MAX_N, LDS_MAX_N + 1, 50_001])
def test_cols_both_forms_and_the_switch_between_them(mi_ctx, n):
    """jittered explicit axes across the LDS-form limit, even and odd column lengths (both load alignments), a padded
    ldy, a misaligned yi; a uniform axis at n = 1024"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(100 + n)
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    for B, nxi, ldy_pad in [(5, 1500, 0), (4, 3001, 1)]:
        Yb = rng.standard_normal((B, n))
        _check_cols(mi_ctx, axis, X, Yb, _axis_queries(rng, X, nxi), ldy_pad=ldy_pad, misalign=bool(ldy_pad))
    axis.close()
    if n == 1024:
        x0, dx = -3.0, 2.0 ** -6
        Xu = x0 + dx * np.arange(n)
        axis = mi.Axis1.uniform(mi_ctx, x0, dx, n)
        for B, nxi, ldy_pad in [(5, 1500, 0), (4, 3001, 1)]:
            Yb = rng.standard_normal((B, n))
            _check_cols(mi_ctx, axis, Xu, Yb, _axis_queries(rng, Xu, nxi), extrap=4.25, uniform=(x0, dx), ldy_pad=ldy_pad)
        axis.close()


@pytest.mark.parametrize("B", [1, 2, 257])
@pytest.mark.parametrize("nxi", [ROW_BLOCK - 1, ROW_BLOCK, ROW_BLOCK + 1, 2 * ROW_BLOCK + 1])
def test_cols_unit_boundaries(mi_ctx, nxi, B):
    """nxi on both sides of a row block, one, two and 257 columns, in both forms and both store widths"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(nxi * 1000 + B)
    for n in (300, LDS_MAX_N + 9):
        X = _jittered(rng, n)
        axis = mi.Axis1.from_nodes(mi_ctx, X)
        Yb = rng.standard_normal((B, n))
        xi = _axis_queries(rng, X, nxi)
        _check_cols(mi_ctx, axis, X, Yb, xi, extrap=-1.5, ldyi_pad=nxi % 2)          # ldyi even: 16-B stores
        _check_cols(mi_ctx, axis, X, Yb, xi, extrap=-1.5, ldyi_pad=1 - nxi % 2)      # ldyi odd: 8-B stores
        axis.close()


def test_cols_runs_of_several_columns_and_empty_calls(mi_ctx):
    """more columns than the launch has units for single columns (2732 columns x 3 row blocks on a 256-CU device: runs of
    two columns, the last run cut short); ncols == 0 and nxi == 0 are MI_OK with nothing launched or written"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, ch = mi_ctx._L, mi_ctx._h
    rng = np.random.default_rng(8)
    n, B, nxi = 64, 2 * 1366 + 1, 2 * ROW_BLOCK + 10
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    Yb = rng.standard_normal((B, n))
    _check_cols(mi_ctx, axis, X, Yb, _axis_queries(rng, X, nxi), extrap=2.0)
    y = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
    xi = torch.full((30,), 0.5, dtype=torch.float64, device="cuda")
    yi = torch.full((4 * 30,), SENTINEL, dtype=torch.float64, device="cuda")
    p = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)  # noqa: E731
    err = lambda: (L.mi_last_error(ch) or b"").decode()  # noqa: E731

    def call(yp=p(y), ldy=n, ncols=4, xp=p(xi), m=30, op=p(yi), ldyi=30):
        return L.mi_interp1_cols_nearest_f64_dev(ch, axis._h, yp, ldy, ncols, xp, m, op, ldyi, 0.0)

    before = _forms(L)
    assert call(ncols=0) == 0 and call(m=0) == 0 and call(ncols=0, yp=None, op=None) == 0 and call(m=0, xp=None) == 0
    for kw, word in [(dict(ldy=n - 1), "ldy"), (dict(ldyi=29), "ldyi"), (dict(yp=p(y, 4)), "aligned"), (dict(xp=p(xi, 4)), "aligned"),
                     (dict(op=p(yi, 4)), "aligned"), (dict(yp=None), "NULL"), (dict(xp=None), "NULL"), (dict(op=None), "NULL")]:
        assert call(**kw) == 1, kw
        assert word in err() and "mi_interp1_cols_nearest_f64_dev" in err(), (kw, err())
    assert L.mi_interp1_cols_nearest_f64_dev(ch, None, p(y), n, 4, p(xi), 30, p(yi), 30, 0.0) == 1 and "NULL" in err()
    assert _delta(L, before) == [0] * 5
    torch.cuda.synchronize()
    assert bool((yi == SENTINEL).all()), "an empty or refused call wrote something"
    assert call(yp=p(y, 8), xp=p(xi, 8), op=p(yi, 8), ncols=3, m=29, ldyi=29) == 0    # 8-B aligned is fine
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        axis.interp_cols_nearest(torch.zeros((4, n), dtype=torch.float64, device="cuda"), xi)     # (B, n), not (n, B)
    axis.close()


@pytest.mark.parametrize("n", [500, LDS_MAX_N + 809])
def test_cols_non_finite_values_come_back_as_stored(mi_ctx, n):
    """NaN, +-inf and -0.0 nodes, the last node among them; queries on, beside and midway between those nodes; the clean
    columns between them equal a call that never saw the specials"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(n)
    X = _jittered(rng, n)
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    B = 8
    clean = rng.standard_normal((B, n))
    Yb = clean.copy()
    k = n // 3
    Yb[1, k], Yb[1, 0] = np.inf, -np.inf
    Yb[3, k], Yb[3, n - 1] = np.nan, np.nan
    Yb[5, k], Yb[5, k + 1], Yb[5, n - 1], Yb[5, 0] = -0.0, -0.0, -0.0, -0.0
    Yb[7, n - 1], Yb[7, n - 2] = np.inf, -0.0
    xi = _axis_queries(rng, X, 1200)
    pts = []
    for j in (0, 1, k - 1, k, k + 1, n - 2, n - 1):
        pts += [X[j], np.nextafter(X[j], -np.inf), np.nextafter(X[j], np.inf)]
        if j + 1 < n:
            mid = 0.5 * X[j] + 0.5 * X[j + 1]
            pts += [mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf)]
    xi[:len(pts)] = pts
    got = _check_cols(mi_ctx, axis, X, Yb, xi, extrap=np.inf)
    assert np.isinf(got[1]).any() and np.isnan(got[3]).any() and (np.signbit(got[5]) & (got[5] == 0)).any()
    nan_q = np.isnan(xi)
    assert np.array_equal(np.isnan(got[3]) & ~nan_q, np.isin(nc.rule_index(X, xi), (k, n - 1)))   # only its own half cells
    base = _run_cols(mi_ctx, axis, clean, xi, np.inf)
    for c in (0, 2, 4, 6):
        assert nc._eq_bits(got[c], base[c])
    axis.close()


def test_cols_linear_and_nearest_share_the_record_workspace(mi_ctx):
    """both calls keep their per-query records in the same workspace slot (16 B and 4 B per query): alternating on one
    context and stream, nothing waited for in between, growing and shrinking query counts, each equals its own reference"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(33)
    n, B = 1500, 12
    X = _jittered(rng, n)
    Yb = rng.standard_normal((B, n))
    axis = mi.Axis1.from_nodes(mi_ctx, X)
    yd = _t(Yb)
    xs = [_axis_queries(rng, X, m) for m in (100, 6000, 37, 20_000)]
    xd = [_t(x) for x in xs]
    torch.cuda.synchronize()
    outs = []
    for d in xd:
        outs.append(("near", axis.interp_cols_nearest(yd.T, d, extrap=1.0)))
        outs.append(("lin", axis.interp_cols(yd.T, d, extrap=1.0)))
        outs.append(("near", axis.interp_cols_nearest(yd.T, d, extrap=1.0)))
    torch.cuda.synchronize()
    for i, (kind, o) in enumerate(outs):
        x = xs[i // 3]
        if kind == "near":
            assert nc._eq_bits(o.T.cpu().numpy(), _rule_cols(X, Yb, x, 1.0)), i
        else:
            ref = np.stack([oracle.interp1_bracket(X, Yb[c], x, 1.0) for c in range(B)])
            assert sc.same_bits(o.T.cpu().numpy(), ref), i
    axis.close()


# ---------------------------------------------------------------------------------------------------- C++
def test_cpp_method_strings(tmp_path):
    """mi355::interp1(X, Y, XI, YI, method, extrap) with Armadillo's four strings, an unknown one, a double and an integer
    fifth argument (the linear overload), and Interp1Table::nearest"""
    from armadillocudalinearinterpolation_amd import _build as b
    b.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST, "arma_interp1_nearest_test"])
    out = subprocess.run([os.path.join(HOST, "arma_interp1_nearest_test"), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    for flag in ("threw_unknown", "threw_null", "threw_unsorted"):
        assert [flag, "1"] in lines, flag
    rd = lambda f: np.fromfile(os.path.join(tmp_path, "n_%s.bin" % f), dtype=np.float64)  # noqa: E731
    X, Y, XI = rd("X"), rd("Y"), rd("XI")
    lin = oracle.interp1_bracket(X, Y, XI, 2.5)
    for k in ("D", "L", "SL", "TL"):
        assert sc.same_bits(rd(k), lin), k
    assert sc.same_bits(rd("I0"), oracle.interp1_bracket(X, Y, XI, 0.0))
    near = nc.nearest_rule(X, Y, XI)
    assert np.isnan(near).any() and np.isinf(near).any() and (np.signbit(near) & (near == 0)).any()
    assert not nc._eq_bits(near, oracle.interp1_bracket(X, Y, XI))
    for k in ("N", "SN"):
        assert nc._eq_bits(rd(k), near), k
    for k in ("NE", "T"):
        assert nc._eq_bits(rd(k), nc.nearest_rule(X, Y, XI, -7.5)), k
