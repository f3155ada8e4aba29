"""The cases of tests/edm_mask_cases.py are what their rows say -- shown with the CPU oracle alone.

tests/test_edm_lift_masks_gpu.py holds the evolve kernels to the oracle under live-slice masks that the reference's
parameters never produce.  That is worth something only while each input still gives the mask, the number of events and
the decisions (ties, events at which nobody fires, a cap) its row promises: an input that quietly degenerated to one
event, or back to the reference's mask, would still pass on the device.  An input that stops satisfying its row is
replaced by a neighbouring one that does; the row is not loosened."""
import numpy as np
import pytest

import edm_mask_cases as mc
import oracle


@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_case_is_what_its_row_says(name):
    case = mc.BY_NAME[name]
    R, N = mc.n_real_of(case), mc.n_grid_of(case)
    f, d, c = mc.oracle_run(name)
    S = len(case.Z)
    assert c["realisations"] == R and d["s"].size == N and d["t0"].size == S * R
    assert mc.mask_string(d["s"], N) == case.mask
    assert len(case.mask) == (N + 63) // 64
    assert c["events"] >= case.min_events * R, (c["events"] / R, case.min_events)
    assert c["max_events_one"] >= case.facts.get("max_events_one", case.min_events)
    if not mc.is_hetero(case):                          # one computation R times over: every realisation has that many
        assert c["events"] == R * c["max_events_one"]
    accepted = case.facts.get("accepted")
    if accepted is not None:
        assert c["accepted"] == (R if accepted else 0)
    assert set(np.unique(d["accept"]).tolist()) <= {0, 1} and d["accept"].sum() == c["accepted"]
    for fact, counter in (("no_firing", "no_firing_events"), ("ties", "argmin_ties"), ("newton_cap", "newton_cap_hits"),
                          ("event_cap", "event_cap_hits")):
        if case.facts.get(fact):
            assert c[counter] > 0, (fact, c)
    assert c["argmin_tree_mismatch"] == 0
    assert mc.unbounded(d["s"]) == bool(case.facts.get("big", False))
    if "nan_in_last_slice" in case.facts:
        last = d["s"][(N - 1) // 64 * 64:]
        assert case.mask[-1] == "1" and int(np.isnan(last).sum()) == case.facts["nan_in_last_slice"]
    if mc.is_hetero(case):                              # the realisations really differ
        assert len({tuple(col) for col in d["t0"].reshape(S, R).T.tolist()}) >= 2


def test_heterogeneous_rows_keep_the_mask_of_their_homogeneous_row():
    for case in mc.HETEROGENEOUS:
        base = case.name[:-len("_hetero")]
        if case.name.endswith("_hetero"):
            assert mc.BY_NAME[base].mask == case.mask and mc.BY_NAME[base].Z == case.Z
            assert np.array_equal(mc.oracle_run(case.name)[1]["s"], mc.oracle_run(base)[1]["s"], equal_nan=True)


def test_sigma3_launch_holds_its_quiet_events_where_the_table_says():
    """the reason that row has 64 realisations: one event at which nobody fires in each of realisations 19, 55, 57, 62"""
    case = mc.BY_NAME["L2.0_N1023_sigma3"]
    assert mc.n_real_of(case) == 64 and mc.oracle_run(case.name)[2]["no_firing_events"] == 4
    for r in (19, 55, 57, 62):
        c = oracle.EdmCounters()
        oracle.edm_compute_f(oracle.edm_default_params(n_real=1, real_offset=r, **mc.overrides_of(case)), case.Z, counters=c)
        assert c.no_firing_events == 1 and c.accepted == 1, r


def test_the_families_cover_what_the_reference_mask_hides():
    cases = mc.CASES
    assert {c.family for c in cases} == set(mc.FAMILIES)
    for hetero in (False, True):
        mine = [c for c in cases if mc.is_hetero(c) == hetero]
        # a live slice in a slot other than its own
        assert any(mc.slots_differ_from_slices(c.mask) and c.min_events > 110 for c in mine)
        # the full 16-slice mask: the largest LDS footprint
        assert any(c.mask == "1" * 16 and c.min_events > 110 for c in mine)
        # a live partial slice (padding lanes inside a live slice), in whole warps and not
        live_partial = [mc.n_grid_of(c) for c in mine if mc.n_grid_of(c) % 64 != 0 and c.mask[-1] == "1" and c.min_events > 110]
        assert any(n % 32 == 0 for n in live_partial) and any(n % 32 != 0 for n in live_partial), live_partial
    # one case of every family compares the device's decision counters with the oracle's
    assert {c.family for c in mc.HOMOGENEOUS if c.counters} == set(mc.FAMILIES)
    assert all(not mc.slots_differ_from_slices(m) for m in ("1111111111111000", "11111110"))     # the reference's masks
    # the partial slice dead with lanes 0..39 only: not the reference's count of dead slices
    pd = mc.BY_NAME["L2.0_N1000"]
    assert pd.mask == "1" * 15 + "0" and mc.n_grid_of(pd) - 64 * 15 == 40
    # the kMaxSpikes instantiation (n_spikes > 3) with thousands of events, both beta models
    assert any(len(c.Z) == 4 and c.min_events > 2000 for c in cases) and any(len(c.Z) == 5 and c.min_events > 2000 for c in cases)
    assert any(len(c.Z) > 3 and mc.is_hetero(c) for c in cases)
    # a grid of whole warps with the reference's padding pairs (fewer than 32 warps), grids that are not whole warps
    grids = {mc.n_grid_of(c) for c in cases if c.family == "full_partial"}
    assert {1000, 992, 1001, 1023, 961, 500, 130, 65, 33} <= grids
    assert 992 % 32 == 0 and 992 // 32 < 32 and all(n % 32 for n in (1000, 1001, 1023, 961))


def test_mask_helper():
    s = np.full(130, np.nan, np.float32)
    assert mc.mask_string(s) == "000"
    s[129] = 0.0
    assert mc.mask_string(s) == "001"
    s[63] = np.inf
    assert mc.mask_string(s) == "101" and mc.unbounded(s)
    s[63] = -2.0 ** 60
    assert mc.unbounded(s)
    s[63] = np.nextafter(np.float32(2.0 ** 60), np.float32(0))
    assert not mc.unbounded(s)
    assert mc.slots_differ_from_slices("0111") and not mc.slots_differ_from_slices("1110") and mc.slots_differ_from_slices("1011")
