"""CPU suite for the EventDrivenMap oracle (oracle/edm_oracle.c): math routines against libm/scipy, stage
known-answers, and the physics sanity of the residual at the reference's own inputs (Driver.cu:16,24).
The reference holds no expected outputs for any of this ("parity unpinned", see the oracle header)."""
import numpy as np
import pytest
from scipy.special import erfinv

import oracle

Z_DRIVER = [0.3310, 0.6914, 1.3557]          # Driver.cu:24
BETA = 13.0589                               # Driver.cu:16


def test_math_routines_accuracy_and_special_values():
    x = np.linspace(-87, 88, 400001).astype(np.float32)
    e = oracle.edm_math_probe(0, x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    assert np.max(np.abs(e - ref) / ref) < 1.5e-7                       # ~1.2 ulp
    sp = oracle.edm_math_probe(0, np.array([0.0, -0.0, np.inf, -np.inf, 89.0, -104.0], np.float32))
    assert sp[0] == 1.0 and sp[1] == 1.0 and np.isinf(sp[2]) and sp[3] == 0.0 and np.isinf(sp[4]) and sp[5] == 0.0
    assert np.isnan(oracle.edm_math_probe(0, np.array([np.nan], np.float32))[0])
    xl = np.exp(np.linspace(-80, 80, 400001)).astype(np.float32)
    l = oracle.edm_math_probe(1, xl).astype(np.float64)
    refl = np.log(xl.astype(np.float64))
    assert np.max(np.abs(l - refl) / np.maximum(np.abs(refl), 1.0)) < 2e-7
    sl = oracle.edm_math_probe(1, np.array([0.0, -1.0, np.inf, 1.0], np.float32))
    assert np.isneginf(sl[0]) and np.isnan(sl[1]) and np.isposinf(sl[2]) and sl[3] == 0.0
    a = np.linspace(0.01, 300, 5000).astype(np.float32)
    b = np.full_like(a, 1.0 / BETA)
    pw = oracle.edm_math_probe(2, a, b).astype(np.float64)
    assert np.max(np.abs(pw - a.astype(np.float64) ** (1.0 / BETA)) / pw) < 1e-6
    assert np.isnan(oracle.edm_math_probe(2, np.array([-1.0], np.float32), np.array([0.3], np.float32))[0])
    u = np.linspace(-0.99999, 0.99999, 100001).astype(np.float32)
    ei = oracle.edm_math_probe(3, u).astype(np.float64)
    assert np.max(np.abs(ei - erfinv(u.astype(np.float64))) / np.maximum(np.abs(erfinv(u.astype(np.float64))), 1e-3)) < 2e-6


def test_coupling_table_and_seed_indices():
    p = oracle.edm_default_params()
    w = oracle.edm_coupling(p)
    N, L = 1024, 3.0
    x = -L + (2 * L / N) * np.arange(N)
    w0 = (11 * np.exp(-5 * np.abs(x)) - 7 * np.exp(-3.5 * np.abs(x))) * 2 * L / N
    assert np.allclose(w, np.roll(w0, -N // 2), rtol=3e-6, atol=1e-9)       # circshift by N/2, :826-841
    assert w[0] == np.float32(4.0 * 2 * 3 / 1024)                           # distance 0: (a1-a2)*2L/N, exact
    ind = oracle.edm_seed_indices(p, Z_DRIVER)
    assert ind[0] == 512
    for m in (1, 2):                                                         # first grid point left of -c*Z_m
        target = -Z_DRIVER[0] * Z_DRIVER[m]
        xi = -3 + (2 * ind[m] * 3.0) / 1024
        assert xi < target <= -3 + (2 * (ind[m] + 1) * 3.0) / 1024
    # [D5] no qualifying point: the previous entry is kept
    stale = oracle.edm_seed_indices(p, [0.3310, 50.0, 1.3557], prev=[7, 9, 11])
    assert stale[1] == 9


def test_lift_profile_shape():
    p = oracle.edm_default_params()
    U = np.array([Z_DRIVER[0], 0.0, Z_DRIVER[1], Z_DRIVER[2]], np.float32)
    v, s = oracle.edm_lift(p, U)
    ok = ~np.isnan(v)
    assert ok.sum() > 800 and np.all(v[ok] < 1.0) and np.all(v[ok] >= 0.0)   # sub-threshold, clamped (:538)
    # 0*inf poisoning of the unselected branch (boolean-multiply structure, :522-528): far ahead of the wave
    # (exp overflow at x < c*U_m - 88.7*c/beta): v is NaN from index 857 on, s from 820 on
    assert np.isnan(v[-1]) and np.all(np.isnan(v[857:])) and not np.isnan(v[856])
    assert np.all(np.isfinite(s[:820])) and np.all(np.isnan(s[820:]))


def test_residual_is_small_at_the_drivers_initial_guess():
    """The reference's Newton solve starts from Z_DRIVER (Driver.cu:24) because it is near a root: a faithful
    restatement of lift/evolve/restrict must give |F| << 1 there, and every realisation must be accepted."""
    p = oracle.edm_default_params(n_real=2, mean_quirk=0)       # the true mean: the physics check
    f, d = oracle.edm_compute_f(p, Z_DRIVER, nthreads=2)
    assert np.all(d["accept"] == 1)
    assert np.linalg.norm(f) < 2e-2
    # bumps sit near c*T - c*U_m after time T: 3 ordered positions, one grid cell apart for last/crossed
    assert np.all(d["i1"].astype(int) - d["i0"].astype(int) == 1)
    assert np.all(d["t0"] <= 5.0) and np.all(d["t1"] > 5.0)
    x = d["restricted"].reshape(3, 2)[:, 0]
    assert x[0] > x[1] > x[2] and abs(x[0] - Z_DRIVER[0] * 5.0) < 0.02
    # sigma = 0: realisations are identical
    assert np.all(d["restricted"].reshape(3, 2)[:, 0] == d["restricted"].reshape(3, 2)[:, 1])
    # f = -c*U - mean + c*T in fp64 (:239)
    mean = d["sums"][:3] / d["sums"][3]
    c = Z_DRIVER[0]
    fexp = -c * np.array([0.0, Z_DRIVER[1], Z_DRIVER[2]]) - mean.astype(np.float32).astype(np.float64) + c * 5.0
    assert np.allclose(f, fexp, rtol=0, atol=1e-7)
    assert np.all(d["sums"][4:] == 0.0)                          # no realisation-0 term without the reference rule


def test_reference_averaging_is_the_default_and_leaves_realisation_0_out():
    """EventDrivenMap.cu:800-802 overwrites accept[0] with the count, :817 then tests accept[index]==1 and :822 divides
    by accept[0]: with R accepted, identical realisations the reference returns x*(R-1)/R.  That is the default
    (mean_quirk = 1); the partial block carries realisation 0 separately so that shards can be added."""
    assert oracle.edm_default_params().mean_quirk == 1
    R = 4
    pq = oracle.edm_default_params(n_real=R)
    pt = oracle.edm_default_params(n_real=R, mean_quirk=0)
    fq, dq = oracle.edm_compute_f(pq, Z_DRIVER, nthreads=2)
    ft, dt = oracle.edm_compute_f(pt, Z_DRIVER, nthreads=2)
    x = dq["restricted"].reshape(3, R)
    assert np.array_equal(dq["restricted"], dt["restricted"]) and np.all(dq["accept"] == 1)
    assert dq["sums"][3] == R and np.array_equal(dq["sums"][4:], x[:, 0].astype(np.float64))
    assert np.array_equal(dq["sums"][:3], x[:, 1:].astype(np.float64).sum(axis=1))
    mean_q = (dq["sums"][:3] / R).astype(np.float32).astype(np.float64)
    c = Z_DRIVER[0]
    assert np.array_equal(fq, (-c * np.array([0.0, Z_DRIVER[1], Z_DRIVER[2]]) - mean_q) + c * 5.0)
    assert np.allclose(ft - fq, -x[:, 0] / R, rtol=0, atol=1e-6)      # the reference's mean is short by x_0 / R
    assert np.array_equal(oracle.edm_residual_from_sums(pq, Z_DRIVER, dq["sums"]), fq)
    # count == 1: realisation 0 is summed whatever its flag (accept[0] then holds 1)
    p1 = oracle.edm_default_params(n_real=1)
    f1, d1 = oracle.edm_compute_f(p1, Z_DRIVER)
    assert np.array_equal(f1, oracle.edm_compute_f(oracle.edm_default_params(n_real=1, mean_quirk=0), Z_DRIVER)[0])
    assert np.array_equal(oracle.edm_residual_from_sums(p1, Z_DRIVER, d1["sums"]), f1)
    # shards: blocks add; only the shard holding realisation 0 applies the rule
    ph = oracle.edm_default_params(n_real=5, beta_stddev=0.3, seed=99)
    fw, dw = oracle.edm_compute_f(ph, Z_DRIVER, nthreads=2)
    tot = np.zeros(7)
    for lo, hi in ((0, 2), (2, 5)):
        tot += oracle.edm_compute_f(oracle.edm_default_params(n_real=hi - lo, real_offset=lo, beta_stddev=0.3, seed=99), Z_DRIVER)[1]["sums"]
    assert np.allclose(tot, dw["sums"], rtol=1e-15, atol=0)
    assert np.allclose(oracle.edm_residual_from_sums(ph, Z_DRIVER, tot), fw, rtol=0, atol=1e-7)


def test_heterogeneous_beta_is_deterministic_and_centred():
    p = oracle.edm_default_params(beta_stddev=0.5, seed=123)
    b = np.array([oracle.edm_beta(p, r, i) for r in range(4) for i in range(0, 1024, 7)])
    assert abs(b.mean() - BETA) < 0.08 and 0.4 < b.std() < 0.6
    assert oracle.edm_beta(p, 3, 5) == oracle.edm_beta(p, 3, 5)
    p0 = oracle.edm_default_params()
    assert oracle.edm_beta(p0, 3, 5) == np.float32(BETA)


_TAPS = ("t0", "i0", "t1", "i1")


def _assert_block_equals_slice(p, full, lo, hi, Z=Z_DRIVER):
    """the oracle run on realisations [lo, hi) alone (n_real = hi - lo, real_offset moved by lo) equals that slice of `full`"""
    S, R = p.n_spikes, p.n_real
    q = oracle.edm_default_params(**{k: getattr(p, k) for k, _ in oracle.EdmParams._fields_})
    q.n_real, q.real_offset = hi - lo, p.real_offset + lo
    _, d = oracle.edm_compute_f(q, Z, nthreads=oracle.max_threads())
    for k in _TAPS:
        assert np.array_equal(d[k].reshape(S, hi - lo), full[k].reshape(S, R)[:, lo:hi], equal_nan=True), (k, lo, hi)
    assert np.array_equal(d["accept"], full["accept"][lo:hi]), (lo, hi)


def _assert_taps_helper_equals_slices(p, full, reals, Z=Z_DRIVER):
    S, R = p.n_spikes, p.n_real
    o = oracle.edm_realisation_taps(p, Z, reals, nthreads=oracle.max_threads(), block=7)
    assert np.array_equal(o["reals"], np.unique(reals))
    for k in _TAPS:
        assert np.array_equal(o[k], full[k].reshape(S, R)[:, o["reals"]], equal_nan=True), k
    assert np.array_equal(o["accept"], full["accept"][o["reals"]])


def test_blocks_of_heterogeneous_realisations_equal_the_slices_of_the_full_run():
    """The premise of the realisation-by-realisation GPU checks (tests/test_edm_hetero_gpu.py): the per-neuron beta draw is
    keyed by the global realisation index r + real_offset only, so the oracle evaluated on any block [lo, hi) of a launch
    (n_real = hi - lo, real_offset + lo) gives exactly that block's taps of the whole launch."""
    p = oracle.edm_default_params(n_grid=512, n_real=64, beta_stddev=0.3, seed=11)
    _, full = oracle.edm_compute_f(p, Z_DRIVER, nthreads=oracle.max_threads())
    cols = set(zip(*[full[k].reshape(3, 64)[m].tolist() for k in ("t0", "i0") for m in range(3)]))
    assert len(cols) >= 58                                                  # the realisations really differ
    for r in range(64):                                                     # every realisation on its own
        _assert_block_equals_slice(p, full, r, r + 1)
    for lo, hi in ((0, 2), (2, 5), (5, 12), (12, 29), (29, 63), (63, 64), (0, 64), (17, 48)):
        _assert_block_equals_slice(p, full, lo, hi)
    rng = np.random.default_rng(5)
    _assert_taps_helper_equals_slices(p, full, np.concatenate([[0, 1, 2, 63], rng.choice(64, 30, replace=False)]))


def test_realisation_counter_is_64_bit_across_2_to_the_32():
    """The draw's counter (r + real_offset) * n_grid + i passes 2^32 at r + real_offset = 2^23 for n_grid = 512 (inside
    realisation 508 of this launch).  Blocks on both sides, and across, still equal the full run, and the realisations past
    the boundary are new ones -- not the realisations 0, 1, .. that a counter wrapped to 32 bits would repeat."""
    off, R, N = 8_388_100, 1000, 512
    assert ((off + 507) * N + N - 1) < 2 ** 32 <= (off + 508) * N
    p = oracle.edm_default_params(n_grid=N, n_real=R, beta_stddev=0.3, seed=11, real_offset=off)
    _, full = oracle.edm_compute_f(p, Z_DRIVER, nthreads=oracle.max_threads())
    t0, i0 = full["t0"].reshape(3, R), full["i0"].reshape(3, R)
    cols = [tuple(t0[:, r].tolist() + i0[:, r].tolist()) for r in range(R)]
    assert len(set(cols[:508])) >= 0.9 * 508 and len(set(cols[508:])) >= 0.9 * (R - 508)
    assert len(set(cols)) >= 0.9 * R
    for lo, hi in ((500, 508), (508, 516), (504, 512), (0, 300), (300, 700), (700, 1000)):
        _assert_block_equals_slice(p, full, lo, hi)
    rng = np.random.default_rng(6)
    _assert_taps_helper_equals_slices(p, full, np.concatenate([np.arange(500, 516), rng.choice(R, 40, replace=False)]))
    # past the boundary the draw is not the one of the wrapped counter (r + off) * N + i - 2^32
    p0 = oracle.edm_default_params(n_grid=N, beta_stddev=0.3, seed=11)
    for r in (508, 509, 999):
        wrapped = r + off - 2 ** 23
        same = [oracle.edm_beta(p, r, i) == oracle.edm_beta(p0, wrapped, i) for i in range(0, N, 5)]
        assert sum(same) <= 3, r


# ---- what "parity unpinned" can be narrowed to (missing 1-2) ----------------------------------------------
# The restatement cannot follow the reference at five documented points: D0 counterMax undefined
# (EventDrivenMap.cu:564), D1 arg-min ties / NaN times (:843-881), D2 uninitialised per-bump slots (:580-583), D5 stale
# seed (:366-371), D8 event cap (:601).  The two tests below state (a) that NONE of them is reached on the inputs of
# BASELINE configs 4-5, over every residual evaluation of the whole Newton solve, and (b) how far the two arithmetic
# freedoms the reference's toolchain had (nvcc's FMA contraction, Makefile:3; libdevice exp/log/pow) can move the result.

Z0_F32 = [float(np.float32(z)) for z in Z_DRIVER]              # Driver.cu:24 stores the guess as float literals


def _residual(p, u, seed, n_real_mean, log=None, variant=None):
    """f(u) of R = n_real_mean IDENTICAL realisations (sigma = 0) from one oracle realisation; the reference's averaging
    (realisation 0 left out of the sum, R in the divisor, EventDrivenMap.cu:800-802,:817,:822) when n_real_mean > 1 and
    p.mean_quirk, else the true mean (same shortcut as tests/test_host_cpp.py::_oracle_f, checked there).
    log: a list that receives (counters of THIS evaluation, f) pairs."""
    c = oracle.EdmCounters() if log is not None else None
    _, d = oracle.edm_compute_f(p, u, seed_ind=seed, counters=c, variant=variant)
    S = p.n_spikes
    x = d["restricted"].reshape(S, p.n_real)[:, 0].astype(np.float64)
    if int(d["accept"][0]) != 1:
        mean = np.full(S, np.nan)                              # 0 / 0 on the device (:822), whatever the slots hold
    elif p.mean_quirk and n_real_mean > 1:
        mean = ((n_real_mean - 1) * x / n_real_mean).astype(np.float32).astype(np.float64)
    else:
        mean = x
    U0 = np.concatenate([[u[0], 0.0], np.asarray(u, dtype=np.float64)[1:]])
    f = (-U0[0] * U0[1:S + 1] - mean) + U0[0] * float(p.time_horizon)
    if log is not None:
        log.append((c.as_dict(), f))
    return f, d["seed_ind"]


def _newton(p, n_real_mean, log=None, variant=None, tol=1e-4, max_it=10, eps=1e-2):
    """NewtonSolver.cpp:40-197 with Driver.cu:28-37's settings on the oracle residual (a NaN residual does not stop the
    reference's loop, :110-113 compares with `>`; numpy's solve then propagates the NaN exactly as arma::solve would)."""
    u = np.array(Z0_F32)
    f, seed = _residual(p, u, None, n_real_mean, log, variant)
    hist, it = [float(np.linalg.norm(f))], 0
    while it < max_it and not hist[-1] <= tol:
        J = np.empty((3, 3))
        for i in range(3):
            du = u.copy()
            du[i] += eps
            df, seed = _residual(p, du, seed, n_real_mean, log, variant)
            J[:, i] = (df - f) * eps ** -1
        u = u + np.linalg.solve(J, -f)
        it += 1
        f, seed = _residual(p, u, seed, n_real_mean, log, variant)
        hist.append(float(np.linalg.norm(f)))
    return u, hist, it


_DECISION_COUNTERS = ("argmin_ties", "argmin_tree_mismatch", "nan_times", "unwritten_last_slots", "unwritten_last_slots_all",
                      "seed_scans_empty", "newton_cap_hits", "event_cap_hits")


@pytest.mark.parametrize("n_grid", [1024, 512])
@pytest.mark.parametrize("averaging", ["true", "reference_1e6", "reference_125k", "reference_1000"])
def test_documented_decisions_are_not_exercised_on_baseline_inputs(n_grid, averaging):
    """Over EVERY residual evaluation of the config-5 Newton solve (Driver.cu problem; N = 1024 as config 4 names it and
    N = 512 as Driver.cu:69 ships it; the true mean and the reference's averaging at 1e6 / 125 000 / 1000 realisations):

    * whenever the realisation is ACCEPTED -- the only case in which its numbers reach f -- there is no exact tie among
      real firing times and no NaN firing time (D1), the reference's own reduction emulated literally (32-wide shuffle
      trees + padded second stage, orc_edm_argmin_reference_tree) picks the same (time, index) as the oracle's rule at
      EVERY event (D1), every bump recorded a pre-T event (D2), every seed scan found its grid point (D5), no firing-time
      solve came near the iteration cap (D0: at most 12 of counterMax := 100) and the event cap was not reached (D8).
      Events at which NO neuron will fire (every thread returns exactly 100.0f, a 512- or 1024-way tie) occur in accepted
      evaluations only at N = 512 with the Driver's own 1000 realisations (evaluations 9 and 11 of that solve); there the
      literal tree returns the padding pair (100.0f, 0) of :867-868 -- index 0, the oracle's "lowest index" -- so the two
      agree; at N = 1024 (no padding lanes: the tree would return index 1023) such an event never occurs;
    * a decision is reached only in evaluations whose realisation is NOT accepted (the N = 512 iteration leaves the basin
      after its 8th step and ends in NaN iterates): there the reference's mean is 0 / 0 (:822) and f is NaN whatever the
      decision -- asserted -- and no evaluation anywhere hits the Newton or the event cap.

    So on these inputs no finite number the oracle produces depends on a decision it had to make.  At N = 1024 every
    evaluation is of the first kind and the solve converges."""
    n_mean = {"true": 1, "reference_1e6": 1_000_000, "reference_125k": 125_000, "reference_1000": 1000}[averaging]
    p = oracle.edm_default_params(n_grid=n_grid, n_real=1, mean_quirk=0 if averaging == "true" else 1)
    log = []
    try:
        u, hist, it = _newton(p, n_mean, log=log)
    except np.linalg.LinAlgError:                       # a singular FD Jacobian ends the solve; what ran still counts
        hist, it = [], -1
    assert len(log) >= 5
    n_acc = 0
    for k, f in log:
        assert k["realisations"] == 1
        assert k["newton_cap_hits"] == 0 and k["max_newton_iter"] <= 12 < p.newton_max_iter          # D0, always
        assert k["event_cap_hits"] == 0 and k["max_events_one"] < 2000 < p.max_events                # D8, always
        assert k["argmin_ties"] == 0 and k["nan_times"] == 0                                         # D1 (real times), always
        if k["accepted"] == 1:
            n_acc += 1
            assert all(k[name] == 0 for name in _DECISION_COUNTERS), k
            assert k["no_firing_events"] == 0 or (n_grid == 512 and averaging == "reference_1000"), k
            assert k["time_cap_exits"] == 0 and np.all(np.isfinite(f))
            assert k["wave64_rounds"] + k["no_firing_events"] == k["events"]   # (the HIP kernel's compacted rounds: one per event)
        else:
            assert np.all(np.isnan(f)), (k, f)           # nothing of this evaluation's event slots reaches a finite number
    if n_grid == 1024:
        assert n_acc == len(log) == 1 + 4 * it and hist[-1] <= 1e-4 and it <= 9
    else:
        assert n_acc >= 24 and not (hist and hist[-1] <= 1e-4)      # Driver.cu:69's grid: no convergence in 10 iterations
    tot = {name: sum(k[name] for k, _ in log) for name in ("events", "newton_solves")}
    print("N=%d %s: %d evaluations (%d accepted), %d events, %d solves, max %d Newton iterations"
          % (n_grid, averaging, len(log), n_acc, tot["events"], tot["newton_solves"], max(k["max_newton_iter"] for k, _ in log)))


def test_counters_do_register_the_decisions_when_they_are_reached():
    """The counters are not vacuous: inputs built to reach D5, D8 / the time exit and D0 make them tick."""
    c = oracle.EdmCounters()
    oracle.edm_compute_f(oracle.edm_default_params(n_real=1), [0.3310, 50.0, 1.3557], counters=c)
    assert c.seed_scans_empty >= 1                                               # -c*Z1 left of the whole grid: D5
    c = oracle.EdmCounters()
    oracle.edm_compute_f(oracle.edm_default_params(n_real=1, max_events=10), Z_DRIVER, counters=c)
    assert c.event_cap_hits == 1 and c.accepted == 0 and c.max_events_one == 10  # D8
    assert c.unwritten_last_slots_all >= 1 or c.unwritten_last_slots == 0
    c = oracle.EdmCounters()
    oracle.edm_compute_f(oracle.edm_default_params(n_real=1, newton_max_iter=2), Z_DRIVER, counters=c)
    assert c.newton_cap_hits > 0 and c.max_newton_iter == 2                      # D0


@pytest.mark.parametrize("n_grid", [1024, 512])
def test_contraction_and_libm_sensitivity_is_below_newton_tolerance(n_grid):
    """What the reference's toolchain was free to do and this repository cannot reproduce: nvcc contracts a*b+c into FMA
    (-fmad=true is its default, reference Makefile:3) and calls libdevice's expf/powf.  Two SENSITIVITY builds of the
    oracle sources (oracle/Makefile: -ffp-contract=fast -mfma; libm expf/logf/powf) bound the effect:

    * at EVERY point the oracle's own Newton solve evaluates (29 points at N = 1024, 41 at N = 512) f moves by less than
      1e-5 (measured: <= 3.5e-6 / 1.8e-6) and no event index changes -- against Driver.cu:37's tolerance of 1e-4;
    * the Newton ITERATION is less forgiving than f: the finite-difference Jacobian (eps 1e-2) spans event-index jumps
      and the oracle's 7th iterate stops at |F| = 0.97e-4, just under the tolerance, where both variants have 1.05e-4
      and take an 8th step.  So the iteration count moves by one and the returned roots differ by 3.7e-4 -- while each
      root satisfies the OTHER build's residual within the solver tolerance (asserted): they are the same solution as far
      as the reference's own stopping rule can tell.  (N = 1024 only; at N = 512 no build converges in 10 iterations.)"""
    if "fma" not in open("/proc/cpuinfo").read():
        pytest.skip("host CPU has no FMA: the contracted build cannot run")
    p = oracle.edm_default_params(n_grid=n_grid, n_real=1, mean_quirk=0)
    points = []                                          # the evaluation points of the oracle's solve, in order
    real_residual = _residual

    def recording(p_, u, seed, n, log_=None, variant=None):
        points.append(np.array(u, dtype=np.float64))
        return real_residual(p_, u, seed, n, log_, variant)

    globals()["_residual"] = recording
    try:
        try:
            u0, h0, it0 = _newton(p, 1)
        except np.linalg.LinAlgError:
            u0, h0, it0 = None, [], -1
    finally:
        globals()["_residual"] = real_residual
    assert len(points) >= 25
    worst = 0.0
    for u in points:
        if not np.all(np.isfinite(u)):
            continue
        f0, d0 = oracle.edm_compute_f(p, u)
        if not np.all(np.isfinite(f0)):
            continue
        for variant in ("contract", "libm"):
            fv, dv = oracle.edm_compute_f(p, u, variant=variant)
            assert np.array_equal(dv["i0"], d0["i0"]) and np.array_equal(dv["i1"], d0["i1"]) and np.array_equal(dv["accept"], d0["accept"])
            worst = max(worst, float(np.max(np.abs(fv - f0))))
    assert 0.0 < worst <= 1e-5, worst                    # it does move (the builds really differ), by < 1e-5
    if n_grid == 1024:
        assert h0[-1] <= 1e-4
        for variant in ("contract", "libm"):
            uv, hv, itv = _newton(p, 1, variant=variant)
            assert hv[-1] <= 1e-4 and abs(itv - it0) <= 1
            assert float(np.max(np.abs(uv - u0))) < 1e-3                               # measured 3.7e-4
            assert np.linalg.norm(oracle.edm_compute_f(p, uv)[0]) <= 1e-4              # the variant's root, in the oracle: 2.1e-5
            assert np.linalg.norm(oracle.edm_compute_f(p, u0, variant=variant)[0]) <= 1e-4   # and vice versa: 9.6e-5
    print("N=%d: max |delta f| over %d evaluation points, contracted and libm builds = %.3g" % (n_grid, len(points), worst))


def test_argmin_rule_equals_the_literal_reference_reduction():
    """D1, as far as it can be closed: on 32-wide warps the reference's blockReduceMin (EventDrivenMap.cu:843-881) is a
    deterministic function of the block's times, ties included.  orc_edm_argmin -- the rule the oracle's event loop and both
    HIP kernels use: minimal time, ties to the largest key rev5(i >> 5) * 32 + rev5(i & 31), and the padding pair
    (100.0f, 0) whenever fewer than 32 warps hold no time below 100.0f -- must return exactly what the literal emulation of
    the two shuffle trees returns, on blocks with few and many ties, all-"never" blocks, infinities, and every warp count."""
    rng = np.random.default_rng(20240)
    for trial in range(6000):
        n = int(rng.choice([32, 64, 96, 256, 512, 992, 1024]))
        kind = trial % 5
        if kind == 0:
            t = rng.random(n)
        elif kind == 1:
            t = rng.integers(0, 3, n)                                           # a few values: ties everywhere
        elif kind == 2:
            t = np.full(n, 100.0)                                               # nobody fires ...
            for _ in range(int(rng.integers(0, 4))):
                t[rng.integers(0, n)] = rng.choice([1.0, 100.0, 150.0])         # ... or almost nobody
        elif kind == 3:
            t = np.where(rng.random(n) < 0.9, 100.0, rng.integers(1, 4, n))
        else:
            t = np.where(rng.random(n) < 0.5, np.inf, rng.integers(100, 103, n))
        t = t.astype(np.float32)
        assert oracle.edm_argmin(t) == oracle.edm_argmin_reference_tree(t), (n, kind)
    # the two shapes the reference runs, nobody firing: 1024 threads -> the last lane of the last warp; 512 threads -> padding
    assert oracle.edm_argmin(np.full(1024, 100.0, np.float32)) == (100.0, 1023)
    assert oracle.edm_argmin(np.full(512, 100.0, np.float32)) == (100.0, 0)
    assert oracle.edm_argmin(np.array([3.0] * 8 + [2.0] + [5.0] * 23 + [2.0] * 32, np.float32)) == (2.0, 63)
    # not whole warps (a launch the reference cannot make): ties to the lowest index, NaN never wins
    assert oracle.edm_argmin(np.array([np.nan, 2.0, 2.0, 7.0], np.float32)) == (2.0, 1)


@pytest.mark.parametrize("n_grid", [1024, 512, 992])
def test_tie_laden_evolutions_agree_with_the_literal_reduction(n_grid):
    """newton_max_iter = 0 makes every firing neuron return the time 0: some 80 events with up to ten-way exact ties of REAL
    firing times, then one event at which nobody fires.  At every one of them the oracle's rule picks what the literal
    reference reduction picks (argmin_tree_mismatch stays 0)."""
    c = oracle.EdmCounters()
    _, d = oracle.edm_compute_f(oracle.edm_default_params(n_grid=n_grid, n_real=1, newton_max_iter=0, max_events=300), Z_DRIVER, counters=c)
    assert c.argmin_ties >= 20 and c.no_firing_events == 1 and c.argmin_tree_mismatch == 0
    assert int(d["i1"].max()) == (1023 if n_grid == 1024 else 0)       # who "fires" when nobody does: :867-868's padding or lane 1023
