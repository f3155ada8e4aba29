"""Shared cases for EventDrivenMap's evolve kernels under lift profiles other than the reference's.

The wave-per-realisation kernel (evolve_kernel, csrc/mi_edm.hip) lays its LDS out by the LIVE-SLICE MASK that the lift
kernel reports: bit k is set when the 64-neuron slice k holds a synaptic value that is not NaN.  The mask sizes the LDS,
maps slice k to slot popcount(mask & ((1 << k) - 1)), addresses per-neuron beta, decides through nan_key / valid who wins
an event at which nobody fires, and decides which padding lanes (i >= N) meet the state pass.  At the reference's
parameters the mask is always `1111111111111000` (N = 1024 / 1000 / 992) or `11111110` (N = 512): slot == slice, the last,
partial slice dead.  The inputs below give every other kind of mask and evolve it for hundreds to thousands of events.

Plain numpy plus the CPU oracle: no torch, no GPU.  tests/test_edm_lift_masks_cpu.py shows with the oracle alone that
every case is what its row says (mask, events, facts); tests/test_edm_lift_masks_gpu.py holds the device to the oracle on
every tap.  Both take the oracle's result from oracle_run, which evaluates a case once per process.

Mask strings list slice 0 first and have (n_grid + 63) // 64 characters.
"""
import collections
import functools

import numpy as np

Z3 = [0.3310, 0.6914, 1.3557]                        # Driver.cu:24
Z3_WIDE = [3.0, 0.6914, 1.3557]                      # a slow wave on a long ring: the head of the profile is NaN
Z3_NEG = [-0.331, 0.6914, 1.3557]                    # negative speed: the lift profile holds +inf
Z4 = [0.566, 0.548, 2.254, 2.572]
Z5 = [0.545, 0.948, 0.993, 1.814, 2.455]

R_HOMOGENEOUS = 5                                    # two workgroups of the throughput form, the last one partial
R_HETEROGENEOUS = 9                                  # three, the last one partial
HETERO = dict(beta_stddev=0.3, seed=5)
BIG_S = 2.0 ** 60                                    # kBigS (csrc/mi_edm.hip): bit 31 of the lift word

# name:       unique, the pytest id
# family:     the mechanism the row isolates (FAMILIES)
# Z, params:  ComputeF's argument and the overrides of the default parameters (n_grid is 1024 unless given)
# mask:       the live-slice mask the lift profile must have
# min_events: events per realisation, at least (the count measured with the oracle)
# facts:      accepted (True: every realisation, False: none), no_firing / ties / newton_cap / event_cap (the oracle's
#             counter is > 0), nan_in_last_slice (NaN synaptic values in the last, live slice), big (some |s| >= 2^60 or
#             infinite: bit 31 of the lift word), max_events_one (the longest realisation has at least that many events)
# counters:   this case also compares mi_edm_debug_counters with the oracle's (at least one per family)
Case = collections.namedtuple("Case", "name family Z params mask min_events facts counters")

FAMILIES = ("full_whole", "full_partial", "partial_dead", "head_dead", "head_dead_unbounded", "bumps", "ties_caps")


def _case(name, family, Z, params, mask, min_events, counters=False, **facts):
    return Case(name, family, list(Z), dict(params), mask, min_events, dict(facts), counters)


def _ones(n_grid):
    return "1" * ((n_grid + 63) // 64)


HOMOGENEOUS = [
    # full mask, whole slices: the largest LDS footprint (16 slices: 36 KiB, 53 KiB with per-neuron beta)
    _case("L1.5", "full_whole", Z3, dict(L=1.5), _ones(1024), 1696, counters=True, accepted=True),
    _case("L1.0", "full_whole", Z3, dict(L=1.0), _ones(1024), 4622, accepted=True),
    _case("L1.5_N512", "full_whole", Z3, dict(L=1.5, n_grid=512), _ones(512), 847, accepted=True),
] + [
    # full mask with a live partial slice: padding lanes (i >= N) inside a live slice meet the state pass.  N = 1000, 1001,
    # 1023, 961 and the small odd ones are not whole warps (!TREE), 992 is (TREE, with the reference's padding pairs)
    _case("L1.5_N%d" % n, "full_partial", Z3, dict(L=1.5, n_grid=n), _ones(n), ev, counters=(n == 1000), accepted=True)
    for n, ev in ((1000, 1655), (992, 1641), (1001, 1713), (1023, 1750), (961, 1647), (500, 826), (130, 218), (65, 173), (33, 181))
] + [
    _case("L2.0_N1023", "full_partial", Z3, dict(L=2.0, n_grid=1023), _ones(1023), 1338, nan_in_last_slice=51),
    # the partial slice dead, but not with the reference's count of dead slices: only lanes 0..39 carry a nan_key
    _case("L2.0_N1000", "partial_dead", Z3, dict(L=2.0, n_grid=1000), "1111111111111110", 1244, counters=True),
    # the head of the profile dead: slot != slice for every live slice
    _case("head_L20", "head_dead", Z3_WIDE, dict(L=20.0, max_events=3000), "0111111111111100", 241, counters=True),
    _case("head_L20_T40", "head_dead", Z3_WIDE, dict(L=20.0, max_events=3000, time_horizon=40.0), "0111111111111100", 324,
          no_firing=True),
    _case("head_L24_T40", "head_dead", Z3_WIDE, dict(L=24.0, max_events=3000, time_horizon=40.0), "0011111111111000", 270,
          no_firing=True),
    _case("head_L28_T40", "head_dead", Z3_WIDE, dict(L=28.0, max_events=3000, time_horizon=40.0), "0001111111110000", 232,
          no_firing=True),
    _case("head_L20_N1000", "head_dead", Z3_WIDE, dict(L=20.0, max_events=3000, n_grid=1000), "0111111111111000", 235),
    # ... with an unbounded synaptic profile: one event, the guarded state pass with s_bounded false
    _case("head_unbounded", "head_dead_unbounded", Z3_NEG, dict(), "0001111111111111", 1, counters=True, big=True),
    # four and five bumps: the kMaxSpikes instantiation
    _case("bumps4_N1000", "bumps", Z4, dict(n_spikes=4, L=1.5, n_grid=1000, max_events=6000), _ones(1000), 3007,
          counters=True, accepted=True),
    _case("bumps4_N1024", "bumps", Z4, dict(n_spikes=4, L=1.5, n_grid=1024, max_events=6000), _ones(1024), 3079, accepted=True),
    _case("bumps5_N1000", "bumps", Z5, dict(n_spikes=5, L=1.5, n_grid=1000, max_events=6000), _ones(1000), 2080, accepted=True),
    # exact ties, events at which nobody fires and the two caps, at a full mask
    _case("ties_N1000", "ties_caps", Z3, dict(L=1.5, newton_max_iter=0, max_events=300, n_grid=1000), _ones(1000), 192,
          counters=True, ties=True, no_firing=True),
    _case("ties_N992", "ties_caps", Z3, dict(L=1.5, newton_max_iter=0, max_events=300, n_grid=992), _ones(992), 190,
          counters=True, ties=True, no_firing=True),
    # nobody ever fires: the winner's index comes from the quiet mask, not from nan_key
    _case("quiet_N1000", "ties_caps", Z3, dict(L=1.5, I=0.5, n_grid=1000), _ones(1000), 1, counters=True, no_firing=True),
    _case("newton_cap_N1000", "ties_caps", Z3, dict(L=1.5, n_grid=1000, newton_max_iter=2), _ones(1000), 1655,
          counters=True, newton_cap=True),
    _case("event_cap_N1000", "ties_caps", Z3, dict(L=1.5, n_grid=1000, max_events=10), _ones(1000), 10, counters=True,
          event_cap=True, accepted=False),
]


HETERO_SLACK = 10      # "to within a few events" of the homogeneous row


def _hetero(case, counters=False, **more):
    return Case(case.name + "_hetero", case.family, case.Z, dict(case.params, **HETERO), case.mask,
                case.min_events - HETERO_SLACK, dict(case.facts, **more), counters)


_BY_NAME = {c.name: c for c in HOMOGENEOUS}

# Per-neuron beta (beta_stddev = 0.3, seed = 5, nine realisations): slot != slice under B[sl * 64 + lane] and bidx(a), the
# 53 KiB footprint, the beta of padding lanes.  The lift profile uses beta_mean, so every row keeps its mask; the mean
# event count per realisation stays within a few events of the homogeneous row's (HETERO_SLACK), and where a count was
# measured for the heterogeneous launch itself, the longest realisation has at least that many (max_events_one).
HETEROGENEOUS = [
    _hetero(_BY_NAME["L1.5"], counters=True),
    _hetero(_BY_NAME["L1.5_N992"]),
    _hetero(_BY_NAME["L1.5_N33"]),
    _hetero(_BY_NAME["L2.0_N1000"], counters=True, accepted=True, max_events_one=1244),
    _hetero(_BY_NAME["head_L20"], counters=True),
    _hetero(_BY_NAME["head_L20_T40"]),
    _hetero(_BY_NAME["head_L24_T40"]),
    _hetero(_BY_NAME["head_L28_T40"]),
    _hetero(_BY_NAME["head_L20_N1000"]),
    _hetero(_BY_NAME["bumps4_N1000"], counters=True, max_events_one=3008),
    _hetero(_BY_NAME["bumps5_N1000"], max_events_one=2081),
    # A wide spread of beta, NaN synaptic values inside the live partial slice, events at which nobody fires.  Those sit
    # in realisations 19, 55, 57 and 62, so this one launch has 64 realisations, not nine.
    Case("L2.0_N1023_sigma3", "full_partial", list(Z3), dict(L=2.0, n_grid=1023, beta_stddev=3.0, seed=11, n_real=64),
         _ones(1023), 1300, dict(accepted=True, no_firing=True, nan_in_last_slice=51), True),
]

CASES = HOMOGENEOUS + HETEROGENEOUS
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def is_hetero(case):
    return case.params.get("beta_stddev", 0.0) != 0.0


def n_grid_of(case):
    return case.params.get("n_grid", 1024)


def n_real_of(case):
    return case.params.get("n_real", R_HETEROGENEOUS if is_hetero(case) else R_HOMOGENEOUS)


def overrides_of(case):
    """the case's parameters without the realisation count (EventDrivenMap takes that as an argument of its own)"""
    return {k: v for k, v in case.params.items() if k != "n_real"}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The CPU oracle on case `name`, once per process: (f, taps, counters as a dict).  taps is oracle.edm_compute_f's
    dictionary of every stage output for the whole launch of n_real_of(case) realisations; the arrays are read-only."""
    import oracle
    case = BY_NAME[name]
    p = oracle.edm_default_params(n_real=n_real_of(case), **overrides_of(case))
    counters = oracle.EdmCounters()
    f, taps = oracle.edm_compute_f(p, case.Z, nthreads=max(1, min(16, oracle.max_threads())), counters=counters)
    for a in list(taps.values()) + [f]:
        a.setflags(write=False)
    return f, taps, counters.as_dict()


def mask_string(s, n_grid=None):
    """The live-slice mask of a synaptic profile `s` (the lift kernel's word, bits 0..15), slice 0 first: '1' where the
    64-neuron slice holds a value that is not NaN."""
    s = np.asarray(s)
    n = s.size if n_grid is None else int(n_grid)
    assert s.ndim == 1 and s.size == n
    return "".join("1" if not np.isnan(s[k:k + 64]).all() else "0" for k in range(0, n, 64))


def unbounded(s):
    """Bit 31 of the lift word: some synaptic value that is not NaN is infinite or at least 2^60 in magnitude."""
    s = np.asarray(s, dtype=np.float64)
    return bool(np.any(~np.isnan(s) & ~(np.abs(s) < BIG_S)))


def slots_differ_from_slices(mask):
    """some live slice k sits in a slot popcount(mask & ((1 << k) - 1)) != k"""
    return any(c == "1" and mask[:k].count("1") != k for k, c in enumerate(mask))
