"""EventDrivenMap under MI_EDM_MATH_FAST: every FAST-only kernel held to a reference, in every form.

FAST math is a product mode with instantiations of its own (csrc/mi_edm.hip): evolve_kernel<1, ..> -- whose firing-time
solves run one neuron per lane at slot popcount(store & ((1 << k) - 1)) of the live-slice layout, no compaction, no lane
pairs --, evolve_wg_kernel<1, ..>, lift_kernel<1>, beta_of<1> (erfinvf_<1>, the hardware log) and the tapped
evolve_kernel<1, .., TAPS>.  Cases and the reasoning behind each reference: tests/edm_fast_cases.py (verdicts shown on the
CPU by tests/test_edm_fast_cases_cpu.py).

1. Cross-form identity, BIT FOR BIT, no tolerance: the throughput form, the latency form (every slice in plain order: no
   mask, no slots), the automatic choice and the arrays the tapped kernel leaves behind evaluate the same expressions on
   the same operands through the same primitives, so every event array is the same -- under every lift mask of
   tests/edm_mask_cases.py, whole and partial last slices, ragged workgroups, the latency form's grid stride, other
   spike counts, degenerate parameters, ties, dedup_identical and real_offset shards with per-neuron beta.
2. The oracle within one grid cell (the project's FAST tolerance), at decision-insensitive inputs: a fault common to
   all FAST forms.
3. The FAST primitives (mi_edm_math_probe) against numpy in float64, within bounds derived from the 1-ulp accuracy of
   v_exp_f32 / v_log_f32 / v_rcp_f32 (AMD CDNA ISA guide; csrc/mi_edm_math.hpp) and the roundings around them.

One session context, no group and no host-array entry point."""
import ctypes as C

import numpy as np
import pytest

import edm_fast_cases as fc
import edm_mask_cases as mc

pytestmark = pytest.mark.gpu

FORMS = {"form1": 1, "form4": 4, "form0": 0}          # waves per realisation: throughput, latency, automatic
LAUNCH_BY_NAME = {c.name: c for c in fc.IDENTITY}


# ---- 1. cross-form identity -----------------------------------------------------------------------------------------

def _evaluate(mi_ctx, launch, form, tapped=False, **more):
    """One FAST ComputeF of `launch` in `form`: the taps of debug_read() plus f and the partial block; with tapped=True
    also (the tapped kernel's counters, the taps it leaves behind)."""
    import armadillocudalinearinterpolation_amd as mi
    params = dict(launch.params, **more)
    n_real = params.pop("n_real", launch.n_real)
    edm = mi.EventDrivenMap(mi_ctx, [launch.beta], n_real, math_mode=mi.MATH_FAST, **params)
    try:
        assert edm.params.math_mode == mi.MATH_FAST
        edm.set_kernel_choice(FORMS[form], True)
        f, partial = edm.ComputeF(launch.Z, want_partial=True)
        out = dict(edm.debug_read(), f=f, partial=partial)
        if not tapped:
            return out
        counters = edm.debug_counters()
        return out, counters, edm.debug_read()
    finally:
        edm.close()


def _every_form(mi_ctx, launch, **more):
    """{form1, form4, form0, tapped: taps}, the tapped kernel's counters"""
    runs = {}
    runs["form1"], counters, runs["tapped"] = _evaluate(mi_ctx, launch, "form1", tapped=True, **more)
    runs["form4"] = _evaluate(mi_ctx, launch, "form4", **more)
    runs["form0"] = _evaluate(mi_ctx, launch, "form0", **more)
    return runs, counters


def _assert_same(what, ref, got, keys, n_spikes):
    """bit for bit (NaN == NaN), no tolerance; says which realisations differ before it fails"""
    for k in keys:
        a, b = np.asarray(ref[k]), np.asarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        if np.array_equal(a, b, equal_nan=True):
            continue
        same = (a == b) | ((a != a) & (b != b))
        where = np.flatnonzero(~same)
        if a.size % n_spikes == 0 and k in ("t0", "i0", "t1", "i1", "restricted"):
            where = np.unique(where % (a.size // n_spikes))              # [spike][realisation]: the realisations
        print(what, k, "differs at", where[:10].tolist(), "of", a.size, ":", a.ravel()[~same.ravel()][:4], "against", b.ravel()[~same.ravel()][:4])
        raise AssertionError((what, k, where[:10].tolist()))


def _assert_forms_identical(name, runs, n_spikes):
    """form 4 carries every slice in plain order: it is the reference of the other three"""
    ref = runs["form4"]
    for other in ("form1", "form0"):
        _assert_same("%s: %s against form4" % (name, other), ref, runs[other], fc.TAPS + ("partial", "f"), n_spikes)
    _assert_same("%s: tapped against form4" % name, ref, runs["tapped"], fc.TAPS, n_spikes)


def _assert_counters(launch, run, counters, n_real=None):
    """the tapped FAST kernel's counters against what the form-4 arrays imply"""
    R = launch.n_real if n_real is None else n_real
    S = len(launch.Z)
    accepted = int(run["accept"].sum())
    assert set(np.unique(run["accept"]).tolist()) <= {0, 1}
    assert counters["accepted"] == accepted and run["partial"][S] == accepted, (counters, accepted)
    assert counters["events"] >= R and counters["max_events_one"] >= 1          # every realisation runs at least one event
    assert counters["max_events_one"] <= launch.params.get("max_events", 1 << 20)
    assert counters["event_cap_hits"] <= R - accepted                            # a realisation at the cap is not accepted
    if counters["max_events_one"] < launch.params.get("max_events", 1 << 20):
        assert counters["event_cap_hits"] == 0
    assert counters["no_firing_events"] <= counters["events"]
    if launch.params.get("beta_stddev", 0.0) == 0.0:                              # R copies of one computation
        assert counters["events"] == R * counters["max_events_one"]
        assert counters["event_cap_hits"] in (0, R) and counters["accepted"] in (0, R)
        assert counters["no_firing_events"] % R == 0


def _assert_copies(run, n_real, n_spikes):
    """sigma = 0: every realisation is realisation 0"""
    for k in ("t0", "i0", "t1", "i1", "restricted"):
        a = run[k].reshape(n_spikes, n_real)
        assert np.array_equal(a, np.repeat(a[:, :1], n_real, axis=1), equal_nan=True), k
    assert np.all(run["accept"] == run["accept"][0])


@pytest.mark.parametrize("name", [c.name for c in fc.IDENTITY])
def test_every_form_leaves_the_same_bits(mi_ctx, name):
    launch = LAUNCH_BY_NAME[name]
    S, N = len(launch.Z), launch.params.get("n_grid", 1024)
    runs, counters = _every_form(mi_ctx, launch)
    ref = runs["form4"]
    print(name, "events per realisation (longest)", counters["max_events_one"], "accepted", counters["accepted"], "of", launch.n_real,
          "no firing", counters["no_firing_events"], "ties", counters["argmin_ties"], "newton cap", counters["newton_cap_hits"])
    _assert_forms_identical(name, runs, S)
    if name.startswith("mask-"):
        case = mc.BY_NAME[name[len("mask-"):]]
        mask = mc.mask_string(ref["s"], N)                           # the mask of the device's own FAST lift profile
        print(name, "FAST mask", mask, "EXACT mask", case.mask, "same" if mask == case.mask else "DIFFERENT")
        assert len(mask) == (N + 63) // 64
        if name in fc.HEAD_DEAD:                                     # a live slice in a slot other than its own, still
            assert mc.slots_differ_from_slices(mask), (mask, case.mask)
            if case.family == "head_dead":                           # ... and evolved, not one event
                assert counters["max_events_one"] > 110
    _assert_counters(launch, ref, counters)
    if launch.params.get("beta_stddev", 0.0) == 0.0:
        _assert_copies(ref, launch.n_real, S)
    else:
        assert len({tuple(col) for col in ref["t0"].reshape(S, launch.n_real).T.tolist()}) >= 2      # really heterogeneous


def test_latency_form_past_its_grid(mi_ctx):
    """R = compute_units * wper_cu + 3 at N = 512: the last three realisations of the latency form come from a second trip
    round its grid-stride loop.  sigma = 0, so they must equal the first, and every form must leave the same bits."""
    launch = fc.make_launch("past-grid", fc.Z_DRIVER, 1, n_grid=512)
    cus = mi_ctx.device_info()["compute_units"]
    assert cus > 0
    R = fc.latency_grid_limit(cus, n_grid=512) + 3
    print("compute units", cus, "realisations", R)
    runs, counters = _every_form(mi_ctx, launch, n_real=R)
    _assert_forms_identical("past-grid", runs, 3)
    _assert_counters(launch, runs["form4"], counters, n_real=R)
    _assert_copies(runs["form4"], R, 3)
    one = _evaluate(mi_ctx, launch, "form4")                         # ... and are what one realisation alone gives
    for k in ("t0", "i0", "t1", "i1", "restricted"):
        assert np.array_equal(runs["form4"][k].reshape(3, R)[:, 0], one[k], equal_nan=True), k


@pytest.mark.parametrize("name", [c.name for c in fc.DEDUP])
def test_dedup_identical_is_the_full_evolution(mi_ctx, name):
    launch = {c.name: c for c in fc.DEDUP}[name]
    full, counters = _every_form(mi_ctx, launch)
    _assert_forms_identical(name, full, 3)
    _assert_copies(full["form4"], launch.n_real, 3)
    dedup, counters_dd = _every_form(mi_ctx, launch, dedup_identical=1)
    for form in ("form1", "form4", "form0"):
        _assert_same("%s: dedup %s against the full form4" % (name, form), full["form4"], dedup[form], fc.TAPS + ("partial", "f"), 3)
    _assert_same("%s: tapped after dedup" % name, full["form4"], dedup["tapped"], fc.TAPS, 3)
    assert counters_dd == counters and counters["events"] >= 110 * launch.n_real
    _assert_counters(launch, full["form4"], counters)


def test_per_neuron_beta_shards_equal_the_unsharded_columns(mi_ctx):
    """beta is drawn by the global realisation index (real_offset + r): the rows a shard [lo, hi) leaves are the columns
    lo..hi-1 of the whole launch, in every form -- through beta_of<1> in both evolve kernels."""
    launch = fc.SHARDED
    S, R = len(launch.Z), launch.n_real
    whole, counters = _every_form(mi_ctx, launch)
    _assert_forms_identical(launch.name, whole, S)
    _assert_counters(launch, whole["form4"], counters)
    ref = whole["form4"]
    assert len({tuple(col) for col in ref["t0"].reshape(S, R).T.tolist()}) >= 2
    count, sums = 0.0, np.zeros(S)
    for lo, hi in fc.SHARDS:
        shard, sc = _every_form(mi_ctx, launch, n_real=hi - lo, real_offset=lo)
        _assert_forms_identical("%s[%d,%d)" % (launch.name, lo, hi), shard, S)
        _assert_counters(launch, shard["form4"], sc, n_real=hi - lo)
        cols = {k: np.ascontiguousarray(ref[k].reshape(S, R)[:, lo:hi]).reshape(-1) for k in ("t0", "i0", "t1", "i1", "restricted")}
        cols.update(accept=ref["accept"][lo:hi], v=ref["v"], s=ref["s"], w=ref["w"], seed_ind=ref["seed_ind"])
        for form in ("form1", "form4", "form0", "tapped"):
            _assert_same("shard [%d,%d) %s against the whole launch" % (lo, hi, form), cols, shard[form], fc.TAPS, S)
        count += shard["form4"]["partial"][S]
        sums += shard["form4"]["partial"][:S]
    assert count == ref["partial"][S] == ref["accept"].sum()
    assert np.allclose(sums, ref["partial"][:S], rtol=1e-12, atol=0)


# ---- 2. against the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in fc.ORACLE_CANDIDATES if c.insensitive])
def test_fast_is_within_one_grid_cell_of_the_oracle(mi_ctx, name):
    """test_fast_mode_within_tolerance's rule (tests/test_edm_gpu.py), per N: accept equal, |i0|, |i1| within 1, restricted and f
    within one grid cell, in both evolve forms -- at inputs whose decisions the CPU test shows to be insensitive."""
    cand = fc.CANDIDATE_BY_NAME[name]
    launch = fc.make_launch(name, cand.Z, cand.n_real, **cand.params)
    fo, d, c = fc.oracle_run(name)
    cell = fc.grid_cell(cand.params["n_grid"])
    for form in ("form1", "form4"):
        run = _evaluate(mi_ctx, launch, form)
        di0 = np.abs(run["i0"].astype(int) - d["i0"].astype(int)).max()
        di1 = np.abs(run["i1"].astype(int) - d["i1"].astype(int)).max()
        dt = max(np.abs(run["t0"].astype(np.float64) - d["t0"]).max(), np.abs(run["t1"].astype(np.float64) - d["t1"]).max())
        dr = np.abs(run["restricted"].astype(np.float64) - d["restricted"]).max()
        df = np.abs(run["f"] - fo).max()
        print("%s %s: |di0| %d |di1| %d |dt| %.3g |drestricted| %.3g |df| %.3g (cell %.3g), accepted %d of %d"
              % (name, form, di0, di1, dt, dr, df, cell, run["accept"].sum(), cand.n_real))
        assert np.array_equal(run["accept"], d["accept"]) and np.all(run["accept"] == 1)
        assert di0 <= 1 and di1 <= 1
        assert dr < cell and df < cell


# ---- 3. FAST primitives ---------------------------------------------------------------------------------------------

U23, U24 = 2.0 ** -23, 2.0 ** -24             # one ulp relative to a float32 (at most), one rounding to nearest (at most)
FLT_MAX, FLT_MIN, DENORM = float(np.finfo(np.float32).max), 2.0 ** -126, 2.0 ** -149
OPS = {"exp": 0, "log": 1, "pow": 2, "erfinv": 3, "div": 4, "ieee_div": 5}
# The places where FAST may legitimately leave another CLASS (NaN / +inf / -inf / finite by sign) than the EXACT routine at
# special arguments: none.  (What differs is inside the class "finite": v_exp_f32 may flush a subnormal result to zero.)
CLASS_DIFFERENCES = {}


def _probe(ctx, mode, op, a, b=None):
    import torch
    from armadillocudalinearinterpolation_amd import _lib
    L = _lib.load()
    ta = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(a if b is None else b, np.float32)).cuda()
    out = torch.empty_like(ta)
    _lib.check(L.mi_edm_math_probe(ctx._h, mode, OPS[op], C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()),
                                   C.c_void_p(out.data_ptr()), ta.numel()), ctx._h)
    return out.cpu().numpy()


def _klass(a):
    """0 NaN, 1 +inf, 2 -inf, 3 finite with the sign bit clear, 4 finite with the sign bit set"""
    a = np.asarray(a, np.float32)
    neg = np.signbit(a)
    return np.where(np.isnan(a), 0, np.where(np.isinf(a), np.where(neg, 2, 1), np.where(neg, 4, 3)))


def _assert_same_class(op, args, fast, exact):
    kf, ke = _klass(fast), _klass(exact)
    for i in np.flatnonzero(kf != ke):
        key = (op, float(args[i]), int(ke[i]), int(kf[i]))
        assert key in CLASS_DIFFERENCES.get(op, ()), ("class differs", op, args[i], "exact", exact[i], "fast", fast[i])


def _assert_within(what, got, ref, rel, extra_abs=0.0, may_flush=False):
    """|got - ref| <= rel |ref| (+ one subnormal step where the result is subnormal); a result whose bound straddles the
    largest float may be +-inf; with may_flush a subnormal result may be a zero.  Prints the worst ratio first."""
    got = np.asarray(got, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        bound = rel * np.abs(ref) + extra_abs + np.where(np.abs(ref) * (1.0 - rel) < FLT_MIN, DENORM, 0.0)
        err = np.abs(got - ref)
        ok = np.isfinite(got) & (err <= bound)
        ok |= np.isinf(got) & (np.sign(got) == np.sign(ref)) & (np.abs(ref) + bound >= FLT_MAX)
        if may_flush:
            ok |= (got == 0.0) & (np.abs(ref) * (1.0 - rel) < FLT_MIN)
        flushed = (got == 0.0) & (np.abs(ref) * (1.0 - rel) < FLT_MIN) if may_flush else np.zeros(got.shape, bool)
        ratio = np.where(np.isfinite(got) & (bound > 0) & ~flushed, err / np.where(bound > 0, bound, 1.0), 0.0)
    print("%s: %d points, worst error / bound %.3f, flushed to zero %d, overflowed %d"
          % (what, got.size, float(ratio.max()), int(((got == 0.0) & (ref != 0.0)).sum()), int(np.isinf(got).sum())))
    assert ok.all(), (what, np.flatnonzero(~ok)[:5].tolist(), got[~ok][:5], ref[~ok][:5], bound[~ok][:5])


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38, -1.0, -2.5,
                    1.0, 1e30, -1e30, 3.4028235e38, -3.4028235e38], np.float32)


def test_fast_exp(mi_ctx):
    """__expf(x) = v_exp_f32(RN(x log2(e))).  The product's rounding moves the argument by at most |x log2 e| 2^-24, i.e. the
    result by |x| 2^-24 relatively (the rounded constant log2(e) adds less than that again); the instruction gives 1 ulp,
    2^-23.  Twice the first-order sum, for what the first order leaves out: 2 (|x| 2^-24 + 2^-23).  Results below 2^-126:
    v_exp_f32 may flush them to zero, otherwise one subnormal step more.  Over [-104, 89], the range of the EXACT routine's
    clamp -- what the evolve can produce."""
    rng = np.random.default_rng(41)
    x = np.concatenate([np.linspace(-104.0, 89.0, 300001), rng.uniform(-104.0, 89.0, 100000), rng.standard_normal(100000),
                        [88.72283, 88.72284, -87.33654, -87.33655, -103.97, 0.0]]).astype(np.float32)
    x64 = x.astype(np.float64)
    _assert_within("exp", _probe(mi_ctx, 1, "exp", x), np.exp(x64), 2.0 * (np.abs(x64) * U24 + U23), may_flush=True)
    _assert_same_class("exp", SPECIAL, _probe(mi_ctx, 1, "exp", SPECIAL), _probe(mi_ctx, 0, "exp", SPECIAL))


def test_fast_log(mi_ctx):
    """__logf(x) = v_log_f32(x) ln 2: the instruction gives log2(x) to 1 ulp (2^-23 relative), ln 2 as a float is off by at
    most 2^-24 relative, the product is rounded once (2^-24).  Twice the first-order sum: 2 (2^-23 + 2^-24 + 2^-24) = 2^-21,
    relative to |log x| -- so log(1) must be 0 exactly.  Over (0, 2^60] (kBigS bounds what the evolve divides), dense around
    1, where the relative bound is hardest, and every power of two."""
    rng = np.random.default_rng(42)
    one = np.float32(1.0).view(np.uint32)
    x = np.concatenate([np.exp(rng.uniform(np.log(FLT_MIN), np.log(2.0 ** 60), 400000)).astype(np.float32),
                        np.arange(int(one) - 20000, int(one) + 20000, dtype=np.uint32).view(np.float32),
                        (2.0 ** np.arange(-126, 61)).astype(np.float32), rng.uniform(0.5, 2.0, 100000).astype(np.float32)])
    assert x.min() >= FLT_MIN * 0.999 and x.max() <= 2.0 ** 60
    got = _probe(mi_ctx, 1, "log", x)
    _assert_within("log", got, np.log(x.astype(np.float64)), 2.0 * (U23 + U24 + U24))
    assert np.all(got[x == 1.0] == 0.0)
    _assert_same_class("log", SPECIAL, _probe(mi_ctx, 1, "log", SPECIAL), _probe(mi_ctx, 0, "log", SPECIAL))


def test_fast_pow(mi_ctx):
    """powf_(a, b) = exp(RN(b log a)), as will_fire takes ratio^(1 / beta).  With y = b log a: log a carries 2^-22 relative
    (the first-order sum of test_fast_log), the product one rounding more, so y is off by |y| (2^-22 + 2^-24); exp adds
    |y| 2^-24 + 2^-23 (test_fast_exp).  First-order sum |y| (2^-22 + 2^-23) + 2^-23, asserted twice that.  Ratios over 26
    decades, exponents from 1 / 50 to 2 (beta from 0.5 to 50) and the reference's 1 / 13.0589."""
    rng = np.random.default_rng(43)
    n = 300000
    a = np.exp(rng.uniform(-30.0, 30.0, n)).astype(np.float32)
    a[: n // 10] = rng.uniform(0.5, 2.0, n // 10).astype(np.float32)
    b = rng.uniform(0.02, 2.0, n).astype(np.float32)
    b[::3] = np.float32(1.0) / np.float32(13.0589)
    y = b.astype(np.float64) * np.log(a.astype(np.float64))
    _assert_within("pow", _probe(mi_ctx, 1, "pow", a, b), np.exp(y), 2.0 * (np.abs(y) * (2.0 ** -22 + U23) + U23))
    for bb in (np.float32(1.0) / np.float32(13.0589), np.float32(1.5), np.float32(0.0)):
        bs = np.full(SPECIAL.size, bb, np.float32)
        _assert_same_class("pow", SPECIAL, _probe(mi_ctx, 1, "pow", SPECIAL, bs), _probe(mi_ctx, 0, "pow", SPECIAL, bs))


def test_fast_uniform_division(mi_ctx):
    """div_by<1, ..>(a, c) = div_<1>(a, c) = RN(a v_rcp_f32(c)): the reciprocal to 1 ulp (2^-23), the product rounded once
    (2^-24).  Twice the first-order sum: 2 (2^-23 + 2^-24), relative to the quotient.  Divisors in [2^-20, 2^20] in magnitude
    (the reference's 1 - beta, beta - 1 and vth - I, awkward significands, both ends), numerators over the exponents the
    EXACT shortcut accepts, where neither form over- or underflows."""
    rng = np.random.default_rng(44)
    n = 1 << 19
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    expo = rng.integers(127 - 100, 127 + 100, n, dtype=np.uint32)
    a = ((rng.integers(0, 2, n, dtype=np.uint32) << 31) | (expo << 23) | mant).view(np.float32)
    beta = np.float32(13.0589)
    divisors = [np.float32(1.0) - beta, beta - np.float32(1.0), np.float32(1.0) - np.float32(0.9), np.float32(0.1), np.float32(3.0),
                np.float32(-7.0), np.float32(1.9999999), np.float32(1.0000001), np.float32(0.5), np.float32(2.0 ** -20), np.float32(-2.0 ** -20),
                np.float32(2.0 ** 20), np.float32(-2.0 ** 20)]
    divisors += list((rng.uniform(1.0, 2.0, 12) * 2.0 ** rng.integers(-20, 20, 12) * rng.choice([-1.0, 1.0], 12)).astype(np.float32))
    for c in divisors:
        assert 2.0 ** -20 <= abs(float(c)) <= 2.0 ** 20
        cb = np.concatenate([np.full(4, c, np.float32), a[4:]])                 # (the probe divides by b[0])
        _assert_within("div by %g" % c, _probe(mi_ctx, 1, "div", a, cb), a.astype(np.float64) / float(c), 2.0 * (U23 + U24))
        sb = np.full(SPECIAL.size, c, np.float32)
        _assert_same_class("div", SPECIAL, _probe(mi_ctx, 1, "div", SPECIAL, sb), _probe(mi_ctx, 0, "ieee_div", SPECIAL, sb))


def test_fast_erfinv(mi_ctx):
    """erfinvf_<1>(x) = p(t) x with w = -log((1 - x)(1 + x)), t = w - 2.5 (w < 5) or sqrt(w) - 3: the EXACT routine with the
    hardware log.  Reference: the same pair of polynomials in float64 (fc.erfinv_parts; shown on the CPU to invert erf).
    Error of the float32 evaluation, first order:
      the argument of the log carries three roundings, 3 * 2^-24 relative, i.e. 3 * 2^-24 absolute in w; the log 2^-22
      relative to |w| (test_fast_log):                                dw = 3 * 2^-24 + |w| 2^-22
      t: dw (central) or dw / (2 sqrt(w)) (tail), plus the roundings of w - 2.5, or of sqrt (below 8: 2^-22) and of - 3
      (2^-24):                                                        dt = dw [ / (2 sqrt w)] + 2^-21
      p by Horner's rule with nine fmaf: 9 * 2^-24 sum |c_i| |t|^i (Higham, Accuracy and Stability, section 5.1)
      the product p x: one rounding.
    Asserted: twice |x| (|p'(t)| dt + 9 * 2^-24 sum |c_i| |t|^i) + 2^-24 |p x|.  Where w is within dw of 5 the device may
    take the other branch, and is held to that branch's value.  Arguments: what beta_of forms from its 24-bit draw."""
    x = fc.beta_draw_arguments(300000, seed=45)
    ends = np.abs(x) >= 1.0                                    # the largest draw rounds to exactly 1: p(inf) * 1, class only
    assert ends.sum() >= 1 and np.all(x[ends] == 1.0)
    special = np.concatenate([x[ends][:1], np.array([1.0, -1.0, 0.0, -0.0, np.nan, 1.5, -1.5, np.inf, -np.inf, 1e-45, -1e-45], np.float32)])
    _assert_same_class("erfinv", special, _probe(mi_ctx, 1, "erfinv", special), _probe(mi_ctx, 0, "erfinv", special))
    x = x[~ends]
    got = _probe(mi_ctx, 1, "erfinv", x).astype(np.float64)
    parts = fc.erfinv_parts(x)
    w, ax = parts["w"], np.abs(parts["x"])
    dw = 3.0 * U24 + np.abs(w) * 2.0 ** -22
    ok, worst = {}, {}
    for key, scale in (("central", 1.0), ("tail", 1.0 / (2.0 * np.sqrt(np.maximum(w, 1.0))))):     # (the tail is only used from w = 5 - dw on)
        b = parts[key]
        dt = dw * scale + 2.0 ** -21
        ref = b["p"] * parts["x"]
        bound = 2.0 * (ax * (np.abs(b["dp"]) * dt + 9.0 * U24 * b["mag"]) + U24 * np.abs(ref))
        err = np.abs(got - ref)
        ok[key] = err <= bound
        worst[key] = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    central = w < 5.0
    near = np.abs(w - 5.0) <= dw
    good = np.where(central, ok["central"], ok["tail"]) | (near & (ok["central"] | ok["tail"]))
    ratio = np.where(central, worst["central"], worst["tail"])
    print("erfinv: %d points (%d in the tail, %d near the branch), worst error / bound %.3f central, %.3f tail"
          % (x.size, int((~central).sum()), int(near.sum()), float(ratio[central & ~near].max()), float(ratio[~central & ~near].max())))
    assert (~central).sum() > 1000 and good.all(), (x[~good][:5], got[~good][:5], w[~good][:5])
