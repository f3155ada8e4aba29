"""EventDrivenMap's evolve kernels under lift profiles other than the reference's, every stage tap BIT FOR BIT.

evolve_kernel (csrc/mi_edm.hip, one wave per realisation) sizes and addresses its LDS by the live-slice mask of the lift
profile: slice k of the grid lives in slot popcount(mask & ((1 << k) - 1)), per-neuron beta at B[slot * 64 + lane], the
dead slices stand in the arg-min through nan_key, and padding lanes (i >= N) run the state pass when their slice is live.
At the reference's parameters slot == slice and the partial slice is dead, always.  The cases of tests/edm_mask_cases.py
(shown to be what they claim by tests/test_edm_lift_masks_cpu.py) evolve full masks, masks with a dead head, live partial
slices, four and five bumps and per-neuron beta for hundreds to thousands of events, in every evolve form: the
throughput form with and without the exact quotient by uniform divisors, the latency form (which carries every slice
and must agree), and the automatic choice.  EXACT math here; under FAST math the same cases are held to the latency
form bit for bit, form against form and against the tapped kernel, by tests/test_edm_fast_gpu.py.

One session context, no group and no host-array entry point."""
import functools

import numpy as np
import pytest

import edm_mask_cases as mc
import oracle

pytestmark = pytest.mark.gpu

TAPS = ("t0", "i0", "t1", "i1")
COUNTERS = ("events", "max_events_one", "max_newton_iter", "newton_cap_hits", "event_cap_hits", "accepted", "no_firing_events")
# (waves per realisation, exact quotient by uniform divisors): 1 throughput, 4 latency, 0 automatic
FORMS = {"form1": (1, True), "form1_nodiv": (1, False), "form4": (4, True), "form0": (0, True)}


def _runs():
    for case in mc.CASES:
        for form in FORMS:
            if form == "form1_nodiv" and mc.is_hetero(case):       # per-neuron beta never takes the uniform-divisor quotient
                continue
            yield pytest.param(case.name, form, id="%s-%s" % (case.name, form))


def _launch(mi_ctx, case, form):
    import armadillocudalinearinterpolation_amd as mi
    edm = mi.EventDrivenMap(mi_ctx, [13.0589], mc.n_real_of(case), **mc.overrides_of(case))
    edm.set_kernel_choice(*FORMS[form])
    f, partial = edm.ComputeF(case.Z, want_partial=True)
    return edm, f, partial, edm.debug_read()


@functools.lru_cache(maxsize=None)
def _realisation_taps(name):
    """the oracle realisation by realisation (blocks of three), once per case for all the forms"""
    case = mc.BY_NAME[name]
    R = mc.n_real_of(case)
    return oracle.edm_realisation_taps(oracle.edm_default_params(n_real=R, **mc.overrides_of(case)), case.Z, np.arange(R),
                                       nthreads=max(1, min(16, oracle.max_threads())), block=3)


def _assert_taps(case, f, partial, dbg):
    R, N, S = mc.n_real_of(case), mc.n_grid_of(case), len(case.Z)
    fo, d, c = mc.oracle_run(case.name)
    assert np.array_equal(dbg["seed_ind"], d["seed_ind"])
    for k in ("w", "v", "s"):
        assert np.array_equal(dbg[k], d[k], equal_nan=True), k            # coupling table + lift profile
    assert mc.mask_string(dbg["s"], N) == case.mask                       # the mask of the device's own lift profile
    assert mc.unbounded(dbg["s"]) == bool(case.facts.get("big", False))
    if mc.is_hetero(case):
        o = _realisation_taps(case.name)
        ref = dict({k: o[k] for k in TAPS}, accept=o["accept"])
        for k in TAPS:                                                    # ... which is the whole launch's, too
            assert np.array_equal(ref[k], d[k].reshape(S, R), equal_nan=True), k
        assert len({tuple(col) for col in ref["t0"].T.tolist()}) >= 2     # really heterogeneous
    else:                                                                 # R copies of the oracle's one computation
        ref = dict({k: np.repeat(d[k].reshape(S, R)[:, :1], R, axis=1) for k in TAPS}, accept=np.repeat(d["accept"][:1], R))
    for k in TAPS:
        dev = dbg[k].reshape(S, R)
        bad = ~((dev == ref[k]) | ((dev != dev) & (ref[k] != ref[k]))).all(axis=0)
        print(case.name, k, "realisations that differ:", int(bad.sum()), "of", R)
        assert not bad.any(), (k, np.flatnonzero(bad)[:10].tolist())
    assert np.array_equal(dbg["accept"], ref["accept"]) and np.array_equal(dbg["accept"], d["accept"])
    assert np.array_equal(dbg["restricted"], d["restricted"], equal_nan=True)
    # the partial block [sums | count | x0] and the residual, as in test_compute_f_exact_mode_bit_parity (tests/test_edm_gpu.py)
    assert partial.shape == (2 * S + 1,) and partial[S] == d["accept"].sum() == c["accepted"]
    assert np.allclose(partial[:S], d["sums"][:S], rtol=1e-12, atol=0, equal_nan=True)
    assert np.array_equal(partial[S + 1:], d["sums"][S + 1:], equal_nan=True)
    assert np.array_equal(np.isnan(f), np.isnan(fo)) and np.allclose(f, fo, rtol=0, atol=2e-7, equal_nan=True)


@pytest.mark.parametrize("name,form", list(_runs()))
def test_every_tap_equals_the_oracle(mi_ctx, name, form):
    case = mc.BY_NAME[name]
    edm, f, partial, dbg = _launch(mi_ctx, case, form)
    try:
        _assert_taps(case, f, partial, dbg)
    finally:
        edm.close()


@pytest.mark.parametrize("name", [c.name for c in mc.CASES if c.counters])
def test_decision_counters_equal_the_oracles(mi_ctx, name):
    """The tapped instantiation of the throughput kernel on the same mask: it counts what the oracle counts -- so the
    device ran the events the table promises -- and leaves the very same events behind."""
    case = mc.BY_NAME[name]
    edm, f, partial, dbg = _launch(mi_ctx, case, "form1")
    try:
        dev = edm.debug_counters()
        again = edm.debug_read()
        o = mc.oracle_run(name)[2]
        print(name, "mask", mc.mask_string(dbg["s"], mc.n_grid_of(case)), "device counters", dev)
        for k in COUNTERS:
            assert dev[k] == o[k], (k, dev, o)
        assert (dev["argmin_ties"] > 0) == (o["argmin_ties"] > 0)
        assert dev["events"] >= case.min_events * mc.n_real_of(case)
        for k in TAPS + ("accept", "restricted", "v", "s", "w"):
            assert np.array_equal(again[k], dbg[k], equal_nan=True), k
        _assert_taps(case, f, partial, again)
    finally:
        edm.close()
