"""The cases of tests/edm_fast_cases.py are what the file says -- shown with the CPU oracle alone.

tests/test_edm_fast_gpu.py holds the FAST-math kernels to the oracle only at inputs whose decisions do not depend on the
arithmetic: a tolerance of one grid cell says nothing at an input where one rounding moves an event to another neuron or
rejects a realisation.  This file recomputes that verdict for every candidate from the oracle and its two sensitivity
builds, and asserts that the verdicts recorded in the table are those and that enough rows qualify."""
import math

import numpy as np
import pytest

import edm_fast_cases as fc
import edm_mask_cases as mc
import oracle


@pytest.mark.parametrize("name", [c.name for c in fc.ORACLE_CANDIDATES])
def test_recorded_verdict_is_the_oracles(name):
    cand = fc.CANDIDATE_BY_NAME[name]
    why = fc.insensitivity(name)
    f, d, c = fc.oracle_run(name)
    print(name, "events per realisation (longest)", c["max_events_one"], "ties", c["argmin_ties"], "no firing", c["no_firing_events"],
          "verdict:", why or "insensitive")
    for variant in ("contract", "libm"):
        dv = fc.oracle_run(name, variant)[1]
        with np.errstate(invalid="ignore"):
            moved = np.abs(dv["restricted"].astype(np.float64) - d["restricted"])
        print("   ", variant, "max |restricted - oracle's| = %.3g" % float(np.max(moved)),
              "events moved:", int((dv["i0"] != d["i0"]).sum() + (dv["i1"] != d["i1"]).sum()))
    assert cand.insensitive == (not why), why
    assert (cand.why_not is None) == cand.insensitive               # a row that is left out says why
    assert cand.n_real == fc.ORACLE_R and c["realisations"] == cand.n_real
    assert cand.params.get("n_grid", 1024) <= 1024
    if cand.insensitive:                                            # a comparison of positions needs positions
        assert np.all(np.isfinite(d["restricted"])) and np.all(np.isfinite(f)) and c["max_events_one"] > 100
    if cand.params.get("beta_stddev", 0.0) != 0.0:                  # the realisations really differ
        S = len(cand.Z)
        assert len({tuple(col) for col in d["t0"].reshape(S, cand.n_real).T.tolist()}) >= 2


def test_enough_candidates_are_decision_insensitive():
    qualifying = [c.name for c in fc.ORACLE_CANDIDATES if c.insensitive]
    print("decision-insensitive:", qualifying)
    assert len(qualifying) >= fc.MIN_INSENSITIVE == 5
    assert [c.name for c in fc.ORACLE_CANDIDATES if not fc.insensitivity(c.name)] == qualifying
    # the candidates the table has to offer: three grids at the reference's parameters, two other spike counts, a shorter
    # horizon, a finite-difference column and per-neuron beta
    by = fc.CANDIDATE_BY_NAME
    assert {by[n].params["n_grid"] for n in ("ref-N1024", "ref-N512", "ref-N1000")} == {1024, 512, 1000}
    assert by["spikes2-N512"].params["n_spikes"] == 2 and by["spikes5-N512"].params["n_spikes"] == 5
    assert by["T4-N512"].params["time_horizon"] == 4.0 and by["perturbed-N512"].Z[0] == fc.Z_DRIVER[0] + 1e-2
    assert by["hetero-N512"].params == dict(n_grid=512, beta_stddev=0.05)
    assert fc.grid_cell(1024) == 6.0 / 1024 and abs(fc.grid_cell(1024) - 5.9e-3) < 1e-4 and fc.grid_cell(512) == 2 * fc.grid_cell(1024)


def test_identity_launches_cover_what_the_issue_lists():
    names = {c.name for c in fc.IDENTITY}
    assert {"mask-" + c.name for c in mc.CASES} <= names and len(fc.MASK) == len(mc.CASES)
    assert {c.params["n_grid"] for c in fc.GRIDS} == {1024, 512, 1000, 992, 130, 65, 64, 33}
    assert [c.n_real for c in fc.REALISATIONS] == [1, 2, 3, 4, 5, 7, 9] and all(c.params == dict(n_grid=512) for c in fc.REALISATIONS)
    assert {c.params["n_spikes"]: c.Z for c in fc.SPIKES} == {2: fc.Z_TWO, 5: fc.Z_FIVE}
    assert len(fc.PATHOLOGICAL) == 12 and len(fc.TIES) == 10
    for c in fc.IDENTITY:
        assert c.params.get("n_grid", 1024) <= 1024
    for c in fc.PATHOLOGICAL + fc.TIES:                             # nothing can run to the default cap of 2^20 events
        assert c.params["max_events"] <= 3000
    for c in fc.MASK:                                               # an unchanged row keeps its parameters; a moved one stays a head_dead row
        case = mc.BY_NAME[c.name[len("mask-"):]]
        if case.name not in fc.FAST_OVERRIDES:
            assert c.params == mc.overrides_of(case) and c.Z == case.Z and c.n_real == mc.n_real_of(case)
        else:
            assert c.name in fc.HEAD_DEAD
    assert fc.HEAD_DEAD and all(mc.slots_differ_from_slices(mc.BY_NAME[n[len("mask-"):]].mask) for n in fc.HEAD_DEAD)
    assert all(c.n_real == 9 for c in fc.DEDUP) and fc.SHARDED.n_real == 9 and fc.SHARDS == ((0, 4), (4, 9))
    assert fc.SHARDED.params["beta_stddev"] > 0


def test_latency_grid_limit_is_launch_evolves_rule():
    # N = 512, homogeneous: (1024 + 2 * 512) * 4 + 16 = 8208 bytes of LDS, 19 workgroups in 160 KiB, capped at 8
    assert fc.latency_grid_limit(256) == 256 * 8 and fc.latency_grid_limit(1) == 8
    # N = 1024 with per-neuron beta: (1024 + 3 * 1024) * 4 + 16 = 16400 bytes, 9 -> 8; a workgroup of 40 KiB would get 4
    assert fc.latency_grid_limit(256, n_grid=1024, hetero=True) == 256 * 8


def test_erfinv_reference_inverts_erf():
    """The float64 restatement of erfinvf_ that the device is compared with is the inverse error function to the accuracy
    of Giles' single-precision polynomials (a few 1e-7 relative), on both branches and over the arguments beta_of forms."""
    x = fc.beta_draw_arguments(4000, seed=1)
    x = x[np.abs(x) < 1.0]
    parts = fc.erfinv_parts(x)
    central = parts["w"] < 5.0
    assert central.any() and (~central).any()
    y = np.where(central, parts["central"]["p"], parts["tail"]["p"]) * parts["x"]
    back = np.array([math.erf(v) for v in y])
    # d erf / dy = 2 / sqrt(pi) exp(-y^2): a relative error e of y moves erf(y) by |y| e times that
    slope = 2.0 / math.sqrt(math.pi) * np.exp(-y * y) * np.abs(y)
    assert np.all(np.abs(back - parts["x"]) <= 1e-6 * slope + 2.0 ** -52)
    # the largest 24-bit draw rounds to u = 1: the argument 1.0f exactly (set aside by the device test)
    assert fc.beta_draw_arguments(1).max() == 1.0 and fc.beta_draw_arguments(1).min() > -1.0
