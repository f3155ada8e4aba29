"""Shared cases for EventDrivenMap under MI_EDM_MATH_FAST (hardware exp / log / reciprocal).

FAST is a product mode with kernels of its own: evolve_kernel<1, ..> (every lane solves its own neuron at slot
popcount(store & ((1 << k) - 1)), no compaction, no lane pairs), evolve_wg_kernel<1, ..>, lift_kernel<1>, beta_of<1>
through erfinvf_<1>, and the tapped evolve_kernel<1, .., TAPS>.  Two references hold them (tests/test_edm_fast_gpu.py):

1. THE LATENCY FORM, bit for bit, at any input.  In FAST mode both evolve forms evaluate the same expressions on the same
   operands through the same primitives (the library is built with -ffp-contract=off and without fast-math; div_by<1, ..>
   and div_<1> are both a * rcp(b); will_fire<1, ..> ignores FILTER; GAP only adds an exit the host check makes
   equivalent), and the latency form carries every slice in plain order: no live-slice mask, no slots, no compaction.
   IDENTITY lists the launches compared across the forms and the tapped kernel.

2. THE ORACLE (EXACT arithmetic), within the project's FAST tolerances -- one grid cell -- at inputs whose decisions are
   insensitive to the arithmetic: ORACLE_CANDIDATES, each with the verdict of insensitivity() recorded in its row
   (tests/test_edm_fast_cases_cpu.py recomputes every verdict on the CPU and asserts that at least five rows qualify).

Plain numpy plus the CPU oracle: no torch, no GPU.
"""
import collections
import functools

import numpy as np

import edm_mask_cases as mc

Z_DRIVER = [0.3310, 0.6914, 1.3557]                     # Driver.cu:24
Z_TWO = [0.3310, 0.6914]                                # tests/test_edm_gpu.py::test_other_spike_counts
Z_FIVE = [0.3310, 0.35, 0.6914, 1.0, 1.3557]
Z_PERTURBED = [Z_DRIVER[0] + 1e-2, Z_DRIVER[1], Z_DRIVER[2]]      # test_setters_and_second_call: a finite-difference column

TAPS = ("t0", "i0", "t1", "i1", "accept", "restricted", "v", "s", "w", "seed_ind")

# ---- 1. cross-form identity ----------------------------------------------------------------------------------------
# name: the pytest id; Z: ComputeF's argument; n_real; params: overrides of the default parameters (math_mode is added by
# the test); beta: the mean of beta handed to EventDrivenMap
Launch = collections.namedtuple("Launch", "name Z n_real params beta")


def make_launch(name, Z, n_real, beta=13.0589, **params):
    assert params.get("n_grid", 1024) <= 1024
    return Launch(name, list(Z), int(n_real), dict(params), float(beta))


# Parameters that replace a mask case's own under FAST math.  The FAST lift profile need not have the mask the EXACT one
# has; a head_dead* row whose FAST mask lost "some live slice sits in a slot other than its own" would be moved here to a
# neighbouring input that has it.  None had to be: on the device every head_dead* row has, under FAST, the very mask of
# its EXACT row (DESIGN.md section 5 lists them).
FAST_OVERRIDES = {}


def mask_launch(case):
    """the launch of a row of tests/edm_mask_cases.py under FAST math"""
    params = dict(mc.overrides_of(case), **FAST_OVERRIDES.get(case.name, {}))
    return make_launch("mask-" + case.name, case.Z, mc.n_real_of(case), **params)


MASK = [mask_launch(c) for c in mc.CASES]
HEAD_DEAD = {"mask-" + c.name for c in mc.CASES if c.family.startswith("head_dead")}

# whole and partial last slices, the !TREE instantiation (N not a multiple of 32), one and two slices; five realisations:
# two workgroups of the throughput form, the second with one wave
GRIDS = [make_launch("N%d" % n, Z_DRIVER, 5, n_grid=n) for n in (1024, 512, 1000, 992, 130, 65, 64, 33)]

# the ragged last workgroup of four waves (R mod 4 = 1, 2, 3, 0), one to three workgroups
REALISATIONS = [make_launch("R%d" % r, Z_DRIVER, r, n_grid=512) for r in (1, 2, 3, 4, 5, 7, 9)]

SPIKES = [make_launch("spikes2", Z_TWO, 3, n_grid=512, n_spikes=2), make_launch("spikes5", Z_FIVE, 3, n_grid=512, n_spikes=5)]

# tests/test_edm_gpu.py::test_pathological_parameters_terminate_and_match, every set under an event cap of 3000 at most
_PATHOLOGICAL = [dict(vth=0.0), dict(vth=-1.0), dict(I=1.5), dict(beta_mean=1.0), dict(beta_mean=0.0), dict(time_horizon=1e-3),
                 dict(a1=0.0, a2=0.0), dict(newton_max_iter=0), dict(newton_tol=0.0), dict(time_horizon=40.0), dict(I=0.999),
                 dict(a1=50.0)]


def _pathological(kw):
    kw = dict(kw)
    beta = kw.pop("beta_mean", 13.0589)
    name = "path-" + "-".join("%s=%g" % kv for kv in sorted(kw.items())) if kw else "path-beta=%g" % beta
    return make_launch(name, Z_DRIVER, 2, beta=beta, n_grid=512, max_events=3000, **kw)


PATHOLOGICAL = [_pathological(kw) for kw in _PATHOLOGICAL]

# tests/test_edm_gpu.py::test_arg_min_ties_follow_the_reference_reduction: many-way ties of real firing times, and an
# event at which nobody fires, on whole warps with and without the reference's padding pairs and on N = 1000
TIES = [make_launch("ties-N%d" % n, Z_DRIVER, 5, n_grid=n, newton_max_iter=0, max_events=300) for n in (1024, 512, 992, 1000, 64)] + \
       [make_launch("quiet-N%d" % n, Z_DRIVER, 5, n_grid=n, I=0.5, max_events=3000) for n in (1024, 512, 992, 1000, 64)]

IDENTITY = MASK + GRIDS + REALISATIONS + SPIKES + PATHOLOGICAL + TIES
assert len({c.name for c in IDENTITY}) == len(IDENTITY)

# dedup_identical = 1 against the full evolution, per-neuron beta in shards: nine realisations
DEDUP = [make_launch("dedup-N%d" % n, Z_DRIVER, 9, n_grid=n) for n in (512, 1024)]
SHARDED = make_launch("shards-hetero", Z_DRIVER, 9, n_grid=512, beta_stddev=0.3, seed=5)
SHARDS = ((0, 4), (4, 9))


def latency_grid_limit(compute_units, n_grid=512, hetero=False, waves=4):
    """Workgroups of the latency form's launch as launch_evolve (csrc/mi_edm.hip) sizes it: compute_units * wper_cu, with
    wper_cu = min(8, 160 KiB / LDS bytes of one workgroup).  Realisations beyond that go round the grid-stride loop."""
    bt = 64 * waves
    wslots = (n_grid + bt - 1) // bt * bt
    wlds = (1024 + (3 if hetero else 2) * wslots) * 4 + 4 * waves * 4
    wper_cu = max(1, min(8, (160 * 1024) // wlds))
    return compute_units * wper_cu


# ---- 2. against the oracle -----------------------------------------------------------------------------------------
# insensitive: the verdict of insensitivity() below, recorded (tests/test_edm_fast_cases_cpu.py recomputes it); only rows
# with True are held to the oracle on the device.  A row with False stays in the table, with the reason.
Candidate = collections.namedtuple("Candidate", "name Z n_real params insensitive why_not")
ORACLE_R = 4                                            # as tests/test_edm_gpu.py::test_fast_mode_within_tolerance

ORACLE_CANDIDATES = [
    Candidate("ref-N1024", Z_DRIVER, ORACLE_R, dict(n_grid=1024), True, None),
    Candidate("ref-N512", Z_DRIVER, ORACLE_R, dict(n_grid=512), True, None),
    Candidate("ref-N1000", Z_DRIVER, ORACLE_R, dict(n_grid=1000), True, None),
    # LEFT OUT, both: with the Z of test_other_spike_counts no realisation is accepted (the activity dies: 187 and 4 events,
    # the last one an event at which nobody fires), so there are no positions to compare -- and with five bumps the
    # sensitivity builds already move `restricted` by 2e-4 and 1.8e-3.  Both stay in the cross-form identity (SPIKES).
    Candidate("spikes2-N512", Z_TWO, ORACLE_R, dict(n_grid=512, n_spikes=2), False, "no realisation is accepted"),
    Candidate("spikes5-N512", Z_FIVE, ORACLE_R, dict(n_grid=512, n_spikes=5), False,
              "no realisation is accepted; restricted moves by more than 1e-4 under both sensitivity builds"),
    Candidate("T4-N512", Z_DRIVER, ORACLE_R, dict(n_grid=512, time_horizon=4.0), True, None),
    Candidate("perturbed-N512", Z_PERTURBED, ORACLE_R, dict(n_grid=512), True, None),
    # the device draws beta through the hardware log (beta_of<1>): held to these tolerances only
    Candidate("hetero-N512", Z_DRIVER, ORACLE_R, dict(n_grid=512, beta_stddev=0.05), True, None),
]
CANDIDATE_BY_NAME = {c.name: c for c in ORACLE_CANDIDATES}
MIN_INSENSITIVE = 5
RESTRICTED_AGREEMENT = 1e-4


def oracle_params(cand, **more):
    import oracle
    return oracle.edm_default_params(n_real=cand.n_real, **dict(cand.params, **more))


@functools.lru_cache(maxsize=None)
def oracle_run(name, variant=None):
    """(f, taps, counters) of the oracle -- or of one of its sensitivity builds -- on a candidate, once per process"""
    import oracle
    cand = CANDIDATE_BY_NAME[name]
    c = oracle.EdmCounters()
    f, d = oracle.edm_compute_f(oracle_params(cand), cand.Z, nthreads=max(1, min(4, oracle.max_threads())), counters=c,
                                variant=variant)
    for a in list(d.values()) + [f]:
        a.setflags(write=False)
    return f, d, c.as_dict()


def insensitivity(name):
    """Why the candidate's decisions are NOT insensitive to the arithmetic -- an empty list when they are: every realisation
    accepted, no ties, no NaN times, neither cap hit, and i0, i1, accept bit-equal and `restricted` within 1e-4 between the
    oracle and its two sensitivity builds (FMA contraction; libm's expf / logf / powf)."""
    f, d, c = oracle_run(name)
    cand = CANDIDATE_BY_NAME[name]
    why = []
    if c["accepted"] != cand.n_real or not np.all(d["accept"] == 1):
        why.append("accepted %d of %d" % (c["accepted"], cand.n_real))
    for k in ("argmin_ties", "nan_times", "newton_cap_hits", "event_cap_hits"):
        if c[k] != 0:
            why.append("%s = %d" % (k, c[k]))
    for variant in ("contract", "libm"):
        fv, dv, cv = oracle_run(name, variant)
        for k in ("i0", "i1", "accept"):
            if not np.array_equal(d[k], dv[k]):
                why.append("%s differs under %s" % (k, variant))
        with np.errstate(invalid="ignore"):
            dev = np.abs(dv["restricted"].astype(np.float64) - d["restricted"].astype(np.float64))
        if not np.all(dev <= RESTRICTED_AGREEMENT):                   # (a NaN fails)
            why.append("restricted moves by %.3g under %s" % (float(np.nanmax(dev)), variant))
    return why


def grid_cell(n_grid, L=3.0):
    """One grid cell, 2 L / N: the project's FAST tolerance on positions and on f (5.9e-3 at N = 1024, scaling as 1 / N)"""
    return 2.0 * L / n_grid


# ---- 3. FAST primitives: references in float64 ---------------------------------------------------------------------
# erfinvf_ (csrc/mi_edm_math.hpp) IS this pair of polynomials in w = -log((1 - x)(1 + x)) (M. Giles, "Approximating the
# erfinv function", single-precision form); coefficients highest power first
ERFINV_CENTRAL = (2.81022636e-08, 3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087, -0.00125372503, -0.00417768164,
                  0.246640727, 1.50140941)                          # in w - 2.5, for w < 5
ERFINV_TAIL = (-0.000200214257, 0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773, -0.0076224613, 0.00943887047,
               1.00167406, 2.83297682)                              # in sqrt(w) - 3


def erfinv_parts(x):
    """The routine in float64 at float32 arguments x in (-1, 1): w, and for each branch (polynomial argument t, p(t),
    p'(t), sum |c_i| |t|^i).  Coefficients as the float32 constants the device holds."""
    x = np.asarray(x, np.float32).astype(np.float64)
    w = -np.log((1.0 - x) * (1.0 + x))
    out = {"x": x, "w": w}
    for key, coef, t in (("central", ERFINV_CENTRAL, w - 2.5), ("tail", ERFINV_TAIL, np.sqrt(w) - 3.0)):
        c = np.asarray(coef, np.float32).astype(np.float64)
        out[key] = dict(t=t, p=np.polyval(c, t), dp=np.polyval(np.polyder(c), t), mag=np.polyval(np.abs(c), np.abs(t)))
    return out


def beta_draw_arguments(n, seed=0):
    """Arguments erfinv gets from beta_of: fmaf(2, u, -1) with u = ((float)k + 0.5f) 2^-24, k a 24-bit integer -- random k,
    both ends of the range and the middle.  (From k = 2^23 on the sum k + 0.5 is rounded to an integer, ties to even, so
    the largest k gives u = 1 and the argument 1.0f exactly; the caller sets that one aside.)"""
    rng = np.random.default_rng(seed)
    k = np.concatenate([rng.integers(0, 1 << 24, n), np.arange(0, 64), (1 << 24) - 1 - np.arange(0, 64),
                        (1 << 23) + np.arange(-32, 32)]).astype(np.float32)
    u = (k + np.float32(0.5)) * np.float32(2.0 ** -24)
    return (2.0 * u.astype(np.float64) - 1.0).astype(np.float32)  # one rounding, as fmaf
