"""oracle/ against the exact references of tests/restrict_cases.py, bit for bit, on every case that
tests/test_restrict_gpu.py runs (same parameter lists, imported) -- so that the GPU file may hold the device against
oracle and reference alike and a disagreement between those two shows on a machine without a GPU -- and the sharded
finish of the partial blocks [sums | count | x0] on the host (mi_edm_residual_from_sums, a host-only ABI call)."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

import oracle


def _cases():
    if "restrict_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location(
            "restrict_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)), "restrict_cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["restrict_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["restrict_cases"]


rc = _cases()


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _restrict_both(c):
    ref = rc.restrict_ref(c["t0"], c["i0"], c["t1"], c["i1"], c["T"], c["L"], c["ngrid"])
    orc = oracle.restrict_f32(c["t0"], c["i0"], c["t1"], c["i1"], c["T"], c["L"], c["ngrid"])
    return ref, orc


@pytest.mark.parametrize("n", rc.RESTRICT_SIZES)
def test_restrict_oracle_equals_reference_sizes(n):
    N, L, T = rc.restrict_params()[rc.RESTRICT_SIZES.index(n) % len(rc.restrict_params())]
    for c in (rc.restrict_case(n, seed=1), rc.restrict_case(n, N, L, T, seed=2)):
        ref, orc = _restrict_both(c)
        assert ref.shape == (n,) and _eq(ref, orc), (n, c["ngrid"], c["L"], c["T"], int(np.sum(~((ref == orc) | (np.isnan(ref) & np.isnan(orc))))))
        if n >= 8:                                           # the planted specials came out as specials
            assert np.isinf(ref[0]) and np.isinf(ref[-1]) and np.sign(ref[0]) == -np.sign(ref[-1])
            assert np.isnan(ref).sum() >= 3


@pytest.mark.parametrize("ngrid", rc.RESTRICT_NGRIDS)
def test_restrict_oracle_equals_reference_parameters(ngrid):
    seen = 0
    for N, L, T in rc.restrict_params():
        if N != ngrid:
            continue
        for n in (rc.RESTRICT_PARAM_N, 4096):
            ref, orc = _restrict_both(rc.restrict_case(n, N, L, T, seed=3))
            assert _eq(ref, orc), (N, L, T, n)
            seen += 1
    assert seen == 2 * len(rc.RESTRICT_LS) * len(rc.RESTRICT_TS)


def test_restrict_oracle_equals_reference_other_device_cases():
    """the cases of the device's alignment, in-place and host-entry tests"""
    cases = [rc.align_case(n) for n in rc.RESTRICT_OFFSET_SIZES] + [rc.inplace_case(n) for n in rc.RESTRICT_INPLACE_SIZES] + \
            [rc.host_case(n) for n in rc.RESTRICT_HOST_SIZES]
    assert len(cases) == len(rc.RESTRICT_OFFSET_SIZES) + len(rc.RESTRICT_INPLACE_SIZES) + len(rc.RESTRICT_HOST_SIZES)
    for c in cases:
        ref, orc = _restrict_both(c)
        assert ref.shape == (c["n"],) and _eq(ref, orc), (c["n"], c["ngrid"])


def test_restrict_known_answer_and_ngrid_range():
    """SURVEY 8c known answer, exact in fp32; the reference refuses an ngrid outside the range of its exactness argument"""
    out = rc.restrict_ref(np.float32([4]), np.uint16([512]), np.float32([6]), np.uint16([514]), 5.0, 3.0, 1024)
    assert out[0] == np.float32(0.005859375)
    for bad in (1, 65537):
        with pytest.raises(AssertionError):
            rc.restrict_ref(np.float32([4]), np.uint16([1]), np.float32([6]), np.uint16([2]), 5.0, 3.0, bad)


def _mean_both(tag, x, accept, S, quirk):
    ref = rc.mean_ref(x, accept, S, quirk)
    om, oc = oracle.masked_mean_f32(x, accept, S, quirk=quirk)
    assert oc == ref["count"], (tag, oc, ref["count"])
    assert rc.same_f32(om, ref["mean"]), (tag, om, ref["mean"])
    # the reference's own block obeys the one-rounding rule it is built from
    if np.all(ref["finite"]):
        assert rc.same_f32(rc.host_mean_from_block(ref["block"], S, quirk), ref["mean"]), tag
    return ref


@pytest.mark.parametrize("R,S", rc.MEAN_SHAPES)
def test_mean_oracle_equals_reference(R, S):
    n = 0
    for family in rc.MEAN_FAMILIES:
        for pattern in rc.MEAN_PATTERNS:
            ce = rc.mean_event_case(S, R, family, pattern)
            cx = rc.mean_x_case(S, R, family, pattern)
            orc_x = oracle.restrict_f32(ce["t0"], ce["i0"], ce["t1"], ce["i1"], ce["T"], ce["L"], ce["ngrid"])
            assert _eq(orc_x, ce["x"]), (R, S, family, pattern)
            for quirk in (0, 1):
                for kind, c in (("events", ce), ("x", cx)):
                    ref = _mean_both((R, S, family, pattern, quirk, kind), c["x"], c["accept"], S, quirk)
                    if pattern == "none":
                        assert ref["count"] == 0 and np.all(np.isnan(ref["mean"]))
                    if pattern == "flags2":
                        assert ref["count"] > int(np.sum(c["accept"] == 1))
                    n += 1
    assert n == 2 * len(rc.MEAN_PATTERNS) * 2 * 2


@pytest.mark.parametrize("R,S", rc.PLANT_SHAPES)
def test_mean_oracle_equals_reference_nonfinite(R, S):
    for family in rc.MEAN_FAMILIES:
        for pattern in rc.PLANT_PATTERNS:
            for plant in rc.PLANTS:
                for quirk in (0, 1):
                    ce = rc.mean_event_case(S, R, family, pattern, plant, quirk)
                    cx = rc.mean_x_case(S, R, family, pattern, plant, quirk)
                    orc_x = oracle.restrict_f32(ce["t0"], ce["i0"], ce["t1"], ce["i1"], ce["T"], ce["L"], ce["ngrid"])
                    assert _eq(orc_x, ce["x"])
                    for kind, c in (("events", ce), ("x", cx)):
                        tag = (R, S, family, pattern, plant, quirk, kind)
                        ref = _mean_both(tag, c["x"], c["accept"], S, quirk)
                        if plant == "rejected" and ref["count"] > 0:
                            # +inf, -inf and NaN in rejected realisations are selected away: every mean stays finite
                            assert c["planted"] and np.all(np.isfinite(ref["mean"])), (tag, ref["mean"])
                        if plant == "accepted" and c["planted"]:
                            assert not np.all(np.isfinite(ref["mean"])), (tag, ref["mean"])


def _event_case_both(tag, c, S, quirk):
    orc_x = oracle.restrict_f32(c["t0"], c["i0"], c["t1"], c["i1"], c["T"], c["L"], c["ngrid"])
    assert _eq(orc_x, c["x"]), tag
    return _mean_both(tag, c["x"], c["accept"], S, quirk)


def test_mean_oracle_equals_reference_graph_cases():
    """the cases of the device's HIP-graph test (warm-up and both replays)"""
    S, R = rc.GRAPH_SHAPE
    for seed, pattern in rc.GRAPH_CASES:
        for quirk in (0, 1):
            _event_case_both(("graph", seed, pattern, quirk), rc.mean_event_case(S, R, "quantised", pattern, seed=seed), S, quirk)


@pytest.mark.parametrize("S", rc.DEV_SHARD_SPIKES)
def test_mean_oracle_equals_reference_device_shard_cases(S):
    """the cases of the device's sharded test: the whole ensemble and every shard's slice (quirk in shard 0 only)"""
    from armadillocudalinearinterpolation_amd import api
    n = 0
    for R in rc.DEV_SHARD_REALS:
        for pattern in rc.DEV_SHARD_PATTERNS:
            c = rc.mean_event_case(S, R, "quantised", pattern, seed=rc.SHARD_SEED)
            for quirk in (0, 1):
                whole = _event_case_both((S, R, pattern, quirk), c, S, quirk)
                for P in (2, 3, 8):
                    total = np.zeros(2 * S + 1)
                    for r in range(P):
                        lo, hi = api.shard_bounds(R, r, P)
                        assert hi > lo
                        part = _mean_both((S, R, pattern, quirk, P, r), rc.shard_slices(c["x"], S, R, lo, hi), c["accept"][lo:hi],
                                          S, quirk and lo == 0)
                        total += part["block"]
                    assert _eq(total, whole["block"]), (S, R, pattern, quirk, P)
                n += 1
    assert n == len(rc.DEV_SHARD_REALS) * len(rc.DEV_SHARD_PATTERNS) * 2


# ---------------------------------------------------------------------------------------------- sharded finish
def _finish(S, quirk, T, Z, block):
    from armadillocudalinearinterpolation_amd import _lib, api
    L = _lib.load()
    p = api.default_edm_params(n_spikes=S, mean_quirk=int(quirk), time_horizon=T)
    f = np.empty(S)
    Z, block = np.ascontiguousarray(Z, dtype=np.float64), np.ascontiguousarray(block, dtype=np.float64)
    _lib.check(L.mi_edm_residual_from_sums(C.byref(p), C.c_void_p(Z.ctypes.data), C.c_void_p(block.ctypes.data),
                                           C.c_void_p(f.ctypes.data)))
    return f


def test_shard_bounds_agree():
    from armadillocudalinearinterpolation_amd import api
    for n in (0, 1, 7, 8, 65, 1000, 4099, (1 << 20) + 7):
        for world in rc.SHARD_WORLDS:
            for r in range(world):
                assert api.shard_bounds(n, r, world) == rc.shard_bounds(n, r, world)


@pytest.mark.parametrize("S", rc.MEAN_SPIKES)
@pytest.mark.parametrize("quirk", [0, 1])
def test_sharded_blocks_finish_like_the_whole(S, quirk):
    """Blocks of P shards built from the reference (quirk applied in shard 0 only, as mi_edm.hip does with
    real_offset == 0), added on the host and finished by mi_edm_residual_from_sums: on quantised inputs bit-equal to the
    unsharded block's f -- for count 0, 1 (accepted realisation in the LAST shard, accept[0] == 0), 1 (accept[0] == 1),
    2 and R."""
    from armadillocudalinearinterpolation_amd import api
    T = 5.0
    Z = 0.25 + 0.125 * np.arange(S)
    for R in rc.SHARD_REALS:
        for pattern in rc.SHARD_COUNTS:
            c = rc.mean_x_case(S, R, "quantised", pattern, seed=7)
            whole = rc.mean_ref(c["x"], c["accept"], S, quirk)
            assert whole["count"] == {"zero": 0, "one_last_shard": 1, "one_first": 1, "two": 2, "all": R}[pattern]
            f_whole = _finish(S, quirk, T, Z, whole["block"])
            assert _eq(f_whole, rc.residual_ref(Z, whole["mean"], T)), (R, pattern, f_whole)
            for P in rc.SHARD_WORLDS:
                total = np.zeros(2 * S + 1)
                for r in range(P):
                    lo, hi = api.shard_bounds(R, r, P)
                    if hi == lo:
                        continue
                    part = rc.mean_ref(rc.shard_slices(c["x"], S, R, lo, hi), c["accept"][lo:hi], S, quirk and lo == 0)
                    total += part["block"]
                if pattern == "one_last_shard" and P > 1:
                    lo, hi = api.shard_bounds(R, P - 1, P)
                    assert lo > 0 and c["accept"][R - 1] == 1 and c["accept"][0] == 0
                assert _eq(total, whole["block"]), (R, pattern, P, total, whole["block"])
                assert _eq(_finish(S, quirk, T, Z, total), f_whole), (R, pattern, P)
