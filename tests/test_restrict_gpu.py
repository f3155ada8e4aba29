"""Edge sweep of armadillocudalinearinterpolation_amd/csrc/mi_restrict.hip -- mi_restrict_f32_dev / _host,
mi_masked_mean_f32_dev, mi_restrict_mean_f32_dev -- against the exact references of tests/restrict_cases.py and against oracle/ (held against those references case by case
in tests/test_restrict_reference_cpu.py).  Restrict: bit-equal.  Mean: bit-equal on quantised inputs; on generic inputs
the a-priori summation bound on the fp64 sums plus the one-rounding rule on the device's own block (restrict_cases'
docstring) -- no tuned tolerance anywhere, and the 1-ulp(fp32) acceptance of the older tests is not used here.
Seeded and deterministic: every listed shape runs on every run, every generated case is asserted.

The ABI is called through the binding's library handle with caller-owned buffers, so that NULL / non-NULL optional
outputs, misaligned views and sentinel elements after every output can be expressed."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


def _cases():
    if "restrict_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location(
            "restrict_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)), "restrict_cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["restrict_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["restrict_cases"]


rc = _cases()

SENT = -12345.0                     # sentinel of every float guard element
SENT_U16 = 0x5A5A
GUARD = 8
DEVICE = "cuda:0"


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEVICE)


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from armadillocudalinearinterpolation_amd import _lib as L
    return L.load(), L.check


def _placed(a, off, at_end=False):
    """`a` on the device inside a larger allocation: [GUARD sentinels | off sentinels | a | GUARD sentinels], or with
    at_end the array is the end of its tensor.  at_end varies placement and alignment only: the caching allocator
    rounds a request up and carves it out of a larger segment, so an access past the last element lands in mapped memory
    and is not seen (a write past `out` is seen through the trailing guard of the other placements).
    Returns (whole buffer, view of a)."""
    import torch
    a = np.ascontiguousarray(a)
    sent = SENT_U16 if a.dtype == np.uint16 else np.float32(SENT)
    host = np.full(GUARD + off + a.size + (0 if at_end else GUARD), sent, dtype=a.dtype)
    host[GUARD + off:GUARD + off + a.size] = a
    buf = _dev(host)
    assert buf.data_ptr() % 16 == 0                          # an aligned base: the offsets are what they say
    return buf, buf[GUARD + off:GUARD + off + a.size]


def _guards_intact(buf, off, n, at_end=False):
    h = _np(buf)
    sent = np.int16(SENT_U16) if h.dtype == np.int16 else np.float32(SENT)
    return bool(np.all(h[:GUARD + off] == sent) and (at_end or np.all(h[GUARD + off + n:] == sent)))


def _restrict_dev(ctx, c, offs=(0, 0, 0, 0, 0), in_place=False, at_end=False):
    """one mi_restrict_f32_dev call on placed arrays; checks every guard element; returns the output (host)"""
    L, check = _lib()
    n = c["n"]
    o_t0, o_t1, o_out, o_i0, o_i1 = offs
    bt0, t0 = _placed(c["t0"], o_t0, at_end)
    bt1, t1 = _placed(c["t1"], o_t1, at_end)
    bi0, i0 = _placed(c["i0"], o_i0, at_end)
    bi1, i1 = _placed(c["i1"], o_i1, at_end)
    if in_place:
        bout, out, o_out = bt0, t0, o_t0
    else:
        bout, out = _placed(np.full(n, SENT, dtype=np.float32), o_out, at_end)
    check(L.mi_restrict_f32_dev(ctx._h, _ptr(t0), _ptr(i0), _ptr(t1), _ptr(i1), c["T"], c["L"], c["ngrid"], _ptr(out), n), ctx._h)
    got = _np(out).copy()
    assert _guards_intact(bout, o_out, n, at_end), ("guard of out overwritten", n, offs)
    for name, b, o, src in (("t1", bt1, o_t1, c["t1"]), ("i0", bi0, o_i0, c["i0"]), ("i1", bi1, o_i1, c["i1"])):
        assert _guards_intact(b, o, n, at_end), (name, n, offs)
        assert np.array_equal(_np(b)[GUARD + o:GUARD + o + n].view(src.dtype), src, equal_nan=src.dtype == np.float32), (name, "input modified")
    if not in_place:
        assert _guards_intact(bt0, o_t0, n, at_end) and _eq(_np(t0), c["t0"])
    return got


def _restrict_expected(c):
    ref = rc.restrict_ref(c["t0"], c["i0"], c["t1"], c["i1"], c["T"], c["L"], c["ngrid"])
    assert _eq(ref, oracle.restrict_f32(c["t0"], c["i0"], c["t1"], c["i1"], c["T"], c["L"], c["ngrid"]))
    return ref


def _mismatches(a, b):
    return int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))


# ---------------------------------------------------------------------------------------------- mi_restrict_f32_dev
@pytest.mark.parametrize("n", rc.RESTRICT_SIZES)
def test_restrict_sizes(mi_ctx, n):
    """vector kernel, its tail at n = 4k + {1, 2, 3} with k = 0 and k > 0, the grid-stride loop past the grid cap; out of
    place and in place (out is t0)"""
    N, L, T = rc.restrict_params()[rc.RESTRICT_SIZES.index(n) % len(rc.restrict_params())]
    for c in (rc.restrict_case(n, seed=1), rc.restrict_case(n, N, L, T, seed=2)):
        ref = _restrict_expected(c)
        got = _restrict_dev(mi_ctx, c)
        assert got.shape == (n,) and _eq(got, ref), (n, c["ngrid"], c["L"], c["T"], _mismatches(got, ref))
        got = _restrict_dev(mi_ctx, c, in_place=True)
        assert _eq(got, ref), ("in place", n, _mismatches(got, ref))


@pytest.mark.parametrize("ngrid", rc.RESTRICT_NGRIDS)
def test_restrict_parameters(mi_ctx, ngrid):
    """ngrid x L x T of the CPU sweep, indices over the full uint16 range (read unsigned), i1 < i0, t1 == t0, NaN / inf"""
    seen = 0
    for N, L, T in rc.restrict_params():
        if N != ngrid:
            continue
        for n in (rc.RESTRICT_PARAM_N, 4096):
            c = rc.restrict_case(n, N, L, T, seed=3)
            assert np.any(c["i0"] >= 32768) and np.any(c["i1"] < c["i0"])
            ref = _restrict_expected(c)
            got = _restrict_dev(mi_ctx, c)
            assert _eq(got, ref), (N, L, T, n, _mismatches(got, ref))
            seen += 1
    assert seen == 2 * len(rc.RESTRICT_LS) * len(rc.RESTRICT_TS)


@pytest.mark.parametrize("n", rc.RESTRICT_OFFSET_SIZES)
def test_restrict_alignment(mi_ctx, n):
    """t0, t1, out offset by 0..3 floats and i0, i1 by 0..3 uint16 inside larger tensors: the vector kernel (everything
    16-B / 8-B aligned) and the scalar kernel (anything else) give the same bits; guards stay; a third of the placements
    put every array at the end of its tensor (no trailing guard)"""
    c = rc.align_case(n)
    ref = _restrict_expected(c)
    for k, offs in enumerate(rc.RESTRICT_OFFSETS):
        got = _restrict_dev(mi_ctx, c, offs, at_end=(k % 3 == 0))
        assert _eq(got, ref), (n, offs, _mismatches(got, ref))


@pytest.mark.parametrize("n", rc.RESTRICT_INPLACE_SIZES)
def test_restrict_in_place_scalar_and_vector(mi_ctx, n):
    """out is t0: on the vector path (aligned; n = 1027 and 6 have a tail) and on the scalar path (t0 / i1 / t1 offset)"""
    c = rc.inplace_case(n)
    ref = _restrict_expected(c)
    for offs in ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 0, 0, 0, 1), (0, 2, 0, 0, 0), (3, 1, 0, 1, 3)):
        for at_end in (False, True):
            got = _restrict_dev(mi_ctx, c, offs, in_place=True, at_end=at_end)
            assert _eq(got, ref), ("in place", n, offs, _mismatches(got, ref))


@pytest.mark.parametrize("n", rc.RESTRICT_HOST_SIZES)
def test_restrict_host_entry_point(mi_ctx, n):
    """mi_restrict_f32_host on numpy arrays: plain, out aliasing t0, and inputs that are odd-offset slices of larger host
    arrays; bit-equal to the device call and to the references"""
    L, check = _lib()
    c = rc.host_case(n)
    ref = _restrict_expected(c)
    dev = _restrict_dev(mi_ctx, c)
    assert _eq(dev, ref)

    def host(t0, i0, t1, i1, out):
        for a in (t0, i0, t1, i1, out):
            assert a.flags["C_CONTIGUOUS"]
        check(L.mi_restrict_f32_host(mi_ctx._h, C.c_void_p(t0.ctypes.data), C.c_void_p(i0.ctypes.data), C.c_void_p(t1.ctypes.data),
                                     C.c_void_p(i1.ctypes.data), c["T"], c["L"], c["ngrid"], C.c_void_p(out.ctypes.data), n), mi_ctx._h)

    out = np.full(n + 2, SENT, dtype=np.float32)
    host(c["t0"], c["i0"], c["t1"], c["i1"], out[1:1 + n])
    assert _eq(out[1:1 + n], dev) and out[0] == np.float32(SENT) and out[-1] == np.float32(SENT)
    t0c = c["t0"].copy()
    host(t0c, c["i0"], c["t1"], c["i1"], t0c)                                    # out aliases t0
    assert _eq(t0c, dev)

    def odd(a, k):
        big = np.full(a.size + 4, SENT_U16 if a.dtype == np.uint16 else SENT, dtype=a.dtype)
        big[k:k + a.size] = a
        return big, big[k:k + a.size]
    bt0, t0 = odd(c["t0"], 1)
    bi0, i0 = odd(c["i0"], 1)
    bt1, t1 = odd(c["t1"], 3)
    bi1, i1 = odd(c["i1"], 3)
    assert t0.ctypes.data % 8 == 4 and i0.ctypes.data % 4 == 2
    host(t0, i0, t1, i1, t0)                                                     # odd-offset slices, in place
    assert _eq(t0, dev)
    assert bt0[0] == np.float32(SENT) and np.all(bt0[1 + n:] == np.float32(SENT))
    assert np.array_equal(i0, c["i0"]) and np.array_equal(i1, c["i1"]) and _eq(t1, c["t1"])


# ---------------------------------------------------------------------------------------------- the masked mean
class _Events:
    """the four event arrays of a fused case on the device (uploaded once while the host arrays stay the same objects)"""

    def __init__(self):
        self.key, self.d = None, None

    def get(self, c):
        key = tuple(id(c[k]) for k in ("t0", "i0", "t1", "i1"))
        if key != self.key:
            self.key, self.d = key, [_dev(c[k]) for k in ("t0", "i0", "t1", "i1")]
            self.keep = [c[k] for k in ("t0", "i0", "t1", "i1")]                 # ids stay unique while referenced
        return self.d


def _mean_call(ctx, S, R, quirk, accept_d, events=None, x_d=None, par=None, want_restricted=True, want_count=True,
               want_sums=True):
    """mi_restrict_mean_f32_dev (events given) or mi_masked_mean_f32_dev (x_d given) with caller-owned buffers and
    sentinels after mean[S-1], sums[2S], restricted[S*R-1].  Returns dict of host arrays (None where not asked for)."""
    import torch
    L, check = _lib()
    mean = torch.full((S + 4,), SENT, dtype=torch.float32, device=DEVICE)
    cnt = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=DEVICE) if want_count else None
    sums = torch.full((2 * S + 1 + 4,), SENT, dtype=torch.float64, device=DEVICE) if want_sums else None
    restricted = None
    if events is not None:
        if want_restricted:
            restricted = torch.full((S * R + 4,), SENT, dtype=torch.float32, device=DEVICE)
        T, Lh, N = par
        check(L.mi_restrict_mean_f32_dev(ctx._h, _ptr(events[0]), _ptr(events[1]), _ptr(events[2]), _ptr(events[3]),
                                         _ptr(accept_d), T, Lh, N, R, S, int(quirk), _ptr(restricted), _ptr(mean), _ptr(cnt),
                                         _ptr(sums)), ctx._h)
    else:
        check(L.mi_masked_mean_f32_dev(ctx._h, _ptr(x_d), _ptr(accept_d), R, S, int(quirk), _ptr(mean), _ptr(cnt), _ptr(sums)),
              ctx._h)
    out = {"mean": None, "count": None, "block": None, "restricted": None, "restricted_dev": None}
    m = _np(mean)
    assert np.all(m[S:] == np.float32(SENT)), "wrote past mean[S-1]"
    out["mean"] = m[:S].copy()
    if want_count:
        cc = _np(cnt, np.uint32)
        assert np.all(cc[1:] == 0x5A5A5A5A), "wrote past count[0]"
        out["count"] = int(cc[0])
    if want_sums:
        b = _np(sums)
        assert np.all(b[2 * S + 1:] == SENT), "wrote past sums[2S]"
        out["block"] = b[:2 * S + 1].copy()
    if restricted is not None:
        tail = _np(restricted[S * R:])
        assert np.all(tail == np.float32(SENT)), "wrote past restricted[S*R-1]"
        out["restricted_dev"] = restricted[:S * R]
    return out


def _same_result(a, b):
    return (rc.same_f32(a["mean"], b["mean"]) and a["count"] == b["count"]
            and (a["block"] is None or b["block"] is None or _eq(a["block"], b["block"])))


def _check_against_oracle(tag, c, S, quirk, got):
    """the oracle's mean: bit-equal on quantised inputs (its index-order fp64 sum is exact there), count always"""
    om, oc = oracle.masked_mean_f32(c["x"], c["accept"], S, quirk=bool(quirk))
    assert got["count"] == oc, (tag, got["count"], oc)
    if c["family"] == "quantised":
        assert rc.same_f32(got["mean"], om), (tag, got["mean"], om)


def _mean_cases(mi_ctx, R, S, patterns, plants):
    ev = _Events()
    n = 0
    for family in rc.MEAN_FAMILIES:
        for pattern in patterns:
            for plant in plants:
                for quirk in (0, 1):
                    ce = rc.mean_event_case(S, R, family, pattern, plant, quirk)
                    cx = rc.mean_x_case(S, R, family, pattern, plant, quirk)
                    acc_d = _dev(ce["accept"])
                    tag = (R, S, family, pattern, plant, quirk)
                    # fused, everything asked for
                    ref = rc.mean_ref(ce["x"], ce["accept"], S, quirk)
                    fused = _mean_call(mi_ctx, S, R, quirk, acc_d, events=ev.get(ce), par=(ce["T"], ce["L"], ce["ngrid"]))
                    assert _eq(_np(fused["restricted_dev"]), ce["x"]), (tag, "restricted")
                    rc.check_mean_outputs(tag + ("fused",), family, ref, S, quirk, fused["mean"], fused["count"], fused["block"])
                    _check_against_oracle(tag + ("fused",), ce, S, quirk, fused)
                    # separate kernel on the fused kernel's own restricted values: the same bits, whatever the family
                    sep = _mean_call(mi_ctx, S, R, quirk, acc_d, x_d=fused["restricted_dev"])
                    assert _same_result(sep, fused), (tag, "separate != fused", sep, fused)
                    # separate kernel on directly given values (several magnitudes)
                    refx = rc.mean_ref(cx["x"], cx["accept"], S, quirk)
                    sepx = _mean_call(mi_ctx, S, R, quirk, acc_d, x_d=_dev(cx["x"]))
                    rc.check_mean_outputs(tag + ("separate",), family, refx, S, quirk, sepx["mean"], sepx["count"], sepx["block"])
                    _check_against_oracle(tag + ("separate",), cx, S, quirk, sepx)
                    if plant == "rejected" and ref["count"] > 0:
                        assert ce["planted"] and cx["planted"]
                        assert np.all(np.isfinite(fused["mean"])) and np.all(np.isfinite(sepx["mean"])), (tag, fused["mean"], sepx["mean"])
                    if pattern == "none":
                        assert fused["count"] == 0 and np.all(np.isnan(fused["mean"])) and np.all(np.isnan(sepx["mean"]))
                    n += 1
    return n


@pytest.mark.parametrize("R,S", rc.MEAN_SHAPES)
def test_mean_sweep(mi_ctx, R, S):
    """nspikes 1..8 x nreal (the largest four for nspikes in {1, 3, 8}: restrict_cases.MEAN_SHAPES) x quirk x family x
    acceptance pattern: fused == separate == references"""
    assert _mean_cases(mi_ctx, R, S, rc.MEAN_PATTERNS, [None]) == 2 * len(rc.MEAN_PATTERNS) * 2


@pytest.mark.parametrize("R,S", rc.PLANT_SHAPES)
def test_mean_nonfinite_values(mi_ctx, R, S):
    """+inf, -inf and NaN restricted values (fused: t1 == t0) in rejected realisations are selected away, not multiplied
    by 0 -- every mean stays finite and exact; in accepted ones they propagate as the reference says"""
    assert _mean_cases(mi_ctx, R, S, rc.PLANT_PATTERNS, rc.PLANTS) == 2 * len(rc.PLANT_PATTERNS) * 2 * 2


@pytest.mark.parametrize("R,S", [(65, 1), (65, 8), (4099, 3), (4099, 8)])
def test_mean_optional_outputs(mi_ctx, R, S):
    """every combination of restricted_dev, count_dev, sums_dev NULL / non-NULL gives the same mean bits (and the same
    values in whatever is asked for)"""
    for family in rc.MEAN_FAMILIES:
        for quirk in (0, 1):
            for pattern in ("p90", "one_mid"):
                c = rc.mean_event_case(S, R, family, pattern)
                ev, acc_d = [_dev(c[k]) for k in ("t0", "i0", "t1", "i1")], _dev(c["accept"])
                par = (c["T"], c["L"], c["ngrid"])
                full = _mean_call(mi_ctx, S, R, quirk, acc_d, events=ev, par=par)
                rc.check_mean_outputs((R, S, family, quirk, pattern), family, rc.mean_ref(c["x"], c["accept"], S, quirk), S, quirk,
                                      full["mean"], full["count"], full["block"])
                x_d = _dev(c["x"])
                for wr in (False, True):
                    for wc in (False, True):
                        for ws in (False, True):
                            g = _mean_call(mi_ctx, S, R, quirk, acc_d, events=ev, par=par, want_restricted=wr, want_count=wc, want_sums=ws)
                            tag = (R, S, family, quirk, pattern, wr, wc, ws)
                            assert rc.same_f32(g["mean"], full["mean"]), tag
                            assert (g["count"] == full["count"]) if wc else g["count"] is None, tag
                            assert _eq(g["block"], full["block"]) if ws else g["block"] is None, tag
                            assert _eq(_np(g["restricted_dev"]), c["x"]) if wr else g["restricted_dev"] is None, tag
                            if not wr:
                                s = _mean_call(mi_ctx, S, R, quirk, acc_d, x_d=x_d, want_count=wc, want_sums=ws)
                                assert rc.same_f32(s["mean"], full["mean"]), tag
                                assert (s["count"] == full["count"]) if wc else s["count"] is None, tag
                                assert _eq(s["block"], full["block"]) if ws else s["block"] is None, tag


def test_mean_workspace_reuse():
    """The Partials block lives in the context's reduction workspace and is reused by every call: a big call then a small
    one, a quirk call then a non-quirk call on the same inputs (x0 part zeros again), and interp1 AUTO-hint calls on the
    region-sweep path (its probe flags live in the same workspace) between mean calls -- each mean equal to the same call
    on a fresh context, each interpolation equal to the oracle."""
    import armadillocudalinearinterpolation_amd as mi
    S = 8
    big = rc.mean_event_case(S, (1 << 20) + 7, "generic", "all")
    small = rc.mean_event_case(S, 65, "generic", "all")

    def run(ctx, c, quirk):
        return _mean_call(ctx, S, c["R"], quirk, _dev(c["accept"]), events=[_dev(c[k]) for k in ("t0", "i0", "t1", "i1")],
                          par=(c["T"], c["L"], c["ngrid"]), want_restricted=False)

    def fresh(c, quirk):
        ctx = mi.Context(0)
        try:
            return run(ctx, c, quirk)
        finally:
            ctx.close()

    ctx = mi.Context(0)
    try:
        ref_small = {q: rc.mean_ref(small["x"], small["accept"], S, q) for q in (0, 1)}
        run(ctx, big, 1)
        a = run(ctx, small, 1)                                                   # big, then small
        assert _same_result(a, fresh(small, 1)), (a, "after a big call")
        rc.check_mean_outputs("small after big", "generic", ref_small[1], S, 1, a["mean"], a["count"], a["block"])
        b = run(ctx, small, 0)                                                   # quirk, then non-quirk
        assert _same_result(b, fresh(small, 0))
        assert np.array_equal(b["block"][S + 1:], np.zeros(S))
        rc.check_mean_outputs("non-quirk after quirk", "generic", ref_small[0], S, 0, b["mean"], b["count"], b["block"])
        # A table and a query count that really take interp1's region sweep (mi_interp1.hip launch_mode: table >= 5 MiB,
        # nq / 16384 tiles >= 2 per CU, unordered queries), the only path that touches the workspace: on this fresh
        # context the first AUTO call has no verdict yet, so the probe kernel writes flags[2] and both gated kernels read
        # it; the later calls know the queries are unordered and run the one-launch sweep, which reads the constant
        # flags[0].  Partials growing into the flags, or a probe writing into the partial block, shows in one of them.
        ng, nq = 1 << 19, (1 << 24) + 5
        X = np.cumsum(np.random.default_rng(3).random(ng) + 0.01)
        Y = np.sin(X * (40.0 / X[-1]))
        grid = mi.Grid1.from_nodes(ctx, X, Y)
        cus = ctx.device_info()["compute_units"]
        assert grid.info()["table_bytes"] >= (5 << 20) and nq // 16384 >= 2 * cus, (grid.info(), cus)
        q = np.random.default_rng(4).random(nq) * (X[-1] - X[0]) + X[0]
        want = oracle.interp1_bracket(X, Y, q, nthreads=min(16, oracle.max_threads()))
        q_d = _dev(q)
        assert _eq(_np(grid.interp(q_d)), want)                                  # probe + gated sweep / streaming kernels
        c2 = run(ctx, small, 1)
        assert _same_result(c2, a)
        assert _eq(_np(grid.interp(q_d)), want)                                  # one-launch sweep: the flags survived the mean
        c3 = run(ctx, small, 0)
        assert _same_result(c3, b)
        d = run(ctx, big, 0)
        assert _same_result(d, fresh(big, 0))
        assert _eq(_np(grid.interp(q_d)), want)                                  # and the big call's 2048 partial blocks
    finally:
        ctx.close()


def test_mean_run_to_run_identical(mi_ctx):
    """the same call three times: identical bits in mean and sums (fixed-order reduction, no float atomics)"""
    S, R = 3, (1 << 20) + 7
    c = rc.mean_event_case(S, R, "generic", "p90")
    ev, acc_d = [_dev(c[k]) for k in ("t0", "i0", "t1", "i1")], _dev(c["accept"])
    runs = [_mean_call(mi_ctx, S, R, 1, acc_d, events=ev, par=(c["T"], c["L"], c["ngrid"]), want_restricted=False) for _ in range(3)]
    x_d = _dev(c["x"])
    runs += [_mean_call(mi_ctx, S, R, 1, acc_d, x_d=x_d) for _ in range(3)]
    for r in runs[1:]:
        assert np.array_equal(r["mean"].view(np.uint32), runs[0]["mean"].view(np.uint32))
        assert np.array_equal(r["block"].view(np.uint64), runs[0]["block"].view(np.uint64)) and r["count"] == runs[0]["count"]


def _finish(S, quirk, T, Z, block):
    from armadillocudalinearinterpolation_amd import api
    L, check = _lib()
    p = api.default_edm_params(n_spikes=S, mean_quirk=int(quirk), time_horizon=T)
    f = np.empty(S)
    Z, block = np.ascontiguousarray(Z, dtype=np.float64), np.ascontiguousarray(block, dtype=np.float64)
    check(L.mi_edm_residual_from_sums(C.byref(p), C.c_void_p(Z.ctypes.data), C.c_void_p(block.ctypes.data), C.c_void_p(f.ctypes.data)))
    return f


@pytest.mark.parametrize("P", [2, 3, 8])
def test_mean_sharded_blocks(mi_ctx, P):
    """R split by mi_shard_bounds, the fused call per shard (quirk in shard 0 only), the blocks added on the host and
    finished by mi_edm_residual_from_sums: on quantised inputs bit-equal to the unsharded call -- count == 1 with the
    accepted realisation in the last shard and accept[0] == 0 included"""
    from armadillocudalinearinterpolation_amd import api
    for S in rc.DEV_SHARD_SPIKES:
        Z = 0.25 + 0.125 * np.arange(S)
        for R in rc.DEV_SHARD_REALS:
            for pattern in rc.DEV_SHARD_PATTERNS:
                for quirk in (0, 1):
                    c = rc.mean_event_case(S, R, "quantised", pattern, seed=rc.SHARD_SEED)
                    par = (c["T"], c["L"], c["ngrid"])
                    tag = (P, S, R, pattern, quirk)
                    whole = _mean_call(mi_ctx, S, R, quirk, _dev(c["accept"]), events=[_dev(c[k]) for k in ("t0", "i0", "t1", "i1")], par=par)
                    rc.check_mean_outputs(tag, "quantised", rc.mean_ref(c["x"], c["accept"], S, quirk), S, quirk,
                                          whole["mean"], whole["count"], whole["block"])
                    f_whole = _finish(S, quirk, c["T"], Z, whole["block"])
                    assert _eq(f_whole, rc.residual_ref(Z, whole["mean"], c["T"])), tag
                    total = np.zeros(2 * S + 1)
                    for r in range(P):
                        lo, hi = api.shard_bounds(R, r, P)
                        assert hi > lo
                        ev = [_dev(rc.shard_slices(c[k], S, R, lo, hi)) for k in ("t0", "i0", "t1", "i1")]
                        part = _mean_call(mi_ctx, S, hi - lo, quirk and lo == 0, _dev(c["accept"][lo:hi]), events=ev, par=par)
                        assert _eq(_np(part["restricted_dev"]), rc.shard_slices(c["x"], S, R, lo, hi)), tag
                        total += part["block"]
                    assert _eq(total, whole["block"]), (tag, total, whole["block"])
                    assert _eq(_finish(S, quirk, c["T"], Z, total), f_whole), tag


def test_restrict_mean_hipgraph_capture(mi_ctx):
    """mi_restrict_mean_f32_dev allocates nothing, copies nothing and never synchronises (mi355_interp.h conventions): it
    is captured into a HIP graph on a side stream (single stream, linear) and replayed twice with fresh inputs in the same
    buffers"""
    import torch
    L, check = _lib()
    (S, R), quirk = rc.GRAPH_SHAPE, 1
    c = rc.mean_event_case(S, R, "quantised", rc.GRAPH_CASES[0][1], seed=rc.GRAPH_CASES[0][0])
    ev, acc_d = [_dev(c[k]) for k in ("t0", "i0", "t1", "i1")], _dev(c["accept"])
    mean = torch.zeros(S, dtype=torch.float32, device=DEVICE)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEVICE)
    sums = torch.zeros(2 * S + 1, dtype=torch.float64, device=DEVICE)
    restricted = torch.zeros(S * R, dtype=torch.float32, device=DEVICE)

    def call():
        check(L.mi_restrict_mean_f32_dev(mi_ctx._h, _ptr(ev[0]), _ptr(ev[1]), _ptr(ev[2]), _ptr(ev[3]), _ptr(acc_d), c["T"], c["L"],
                                         c["ngrid"], R, S, quirk, _ptr(restricted), _ptr(mean), _ptr(cnt), _ptr(sums)), mi_ctx._h)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(side):
            mi_ctx.use_torch_stream()
            call()                                                               # warm-up outside capture
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                mi_ctx.use_torch_stream()
                call()
        torch.cuda.current_stream().wait_stream(side)
    finally:
        mi_ctx.use_torch_stream()
    for seed, pattern in rc.GRAPH_CASES[1:]:
        c2 = rc.mean_event_case(S, R, "quantised", pattern, seed=seed)
        for d, k in zip(ev, ("t0", "i0", "t1", "i1")):
            d.copy_(_dev(c2[k]))
        acc_d.copy_(_dev(c2["accept"]))
        for t in (mean, sums, restricted, cnt):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _eq(_np(restricted), c2["x"])
        rc.check_mean_outputs(("graph", seed), "quantised", rc.mean_ref(c2["x"], c2["accept"], S, quirk), S, quirk,
                              _np(mean), int(_np(cnt, np.uint32)[0]), _np(sums))
