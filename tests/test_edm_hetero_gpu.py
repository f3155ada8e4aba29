"""Heterogeneous beta (beta_stddev > 0) at device-filling realisation counts, realisation by realisation.

With beta_stddev = 0 every realisation is the same computation, so a kernel that mixed realisations up -- drew one
realisation's beta under another's index, wrote its events into another's slot, kept a stale beta in LDS across the
grid-stride passes of the latency form -- would still return R copies of the right answer.  Here every realisation is
its own computation, and each one checked is held BIT FOR BIT to the oracle (oracle.edm_realisation_taps evaluates
contiguous blocks of a launch; tests/test_edm_oracle_cpu.py pins that a block equals that slice of the whole launch).
The realisation counts are derived from the device's compute-unit count so that each launch has more workgroups than
are resident at once, several grid-stride passes, or a draw counter that passes 2^32.  EXACT math throughout."""
import math

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

Z3 = [0.3310, 0.6914, 1.3557]                        # Driver.cu:24
Z5 = [0.3310, 0.35, 0.6914, 1.0, 1.3557]
TAPS = ("t0", "i0", "t1", "i1")
LATENCY_WG_PER_CU = 8                                 # evolve_wg_kernel: min(8, 160 KiB / LDS) workgroups per CU at N <= 1024


def _threads():
    return max(1, min(16, oracle.max_threads()))


@pytest.fixture(scope="module")
def cus(mi_ctx):
    n = int(mi_ctx.device_info()["compute_units"])
    assert n > 0
    return n


def _launch(mi_ctx, form, R, Z, **kw):
    """One ComputeF with the evolve kernel form forced on the handle (0: the automatic choice)."""
    import armadillocudalinearinterpolation_amd as mi
    edm = mi.EventDrivenMap(mi_ctx, [13.0589], R, **kw)
    edm.set_kernel_choice(form)
    f, partial = edm.ComputeF(Z, want_partial=True)
    d = edm.debug_read()
    return edm, f, partial, d


def _oracle_params(R, **kw):
    return oracle.edm_default_params(n_real=R, **{k: v for k, v in kw.items() if k != "dedup_identical"})


def _sample(R, form, cus, seed):
    """The realisations of the first 16 and the last 3 workgroups of the form's launch, 8 on each side of every multiple
    of the latency form's grid, and 256 more at random."""
    G = LATENCY_WG_PER_CU * cus
    s = set()
    if form == 1:                                     # throughput: workgroup b holds realisations 4b .. 4b + 3
        nb = (R + 3) // 4
        for b in list(range(16)) + list(range(nb - 3, nb)):
            s.update(range(4 * b, min(4 * b + 4, R)))
    else:                                             # latency: workgroup b holds b, b + G, b + 2G, ..
        g = min(R, G)
        for b in list(range(16)) + list(range(g - 3, g)):
            s.update(range(b, R, g))
    for m in range(G, R, G):
        s.update(range(max(0, m - 8), min(R, m + 8)))
    s.update(np.random.default_rng(seed).choice(R, min(R, 256), replace=False).tolist())
    return np.array(sorted(s))


def assert_realisations_match_oracle(d, R, S, Z, reals, **kw):
    """device taps t0, i0, t1, i1 and accept of the realisations `reals` == the oracle's, bit for bit"""
    o = oracle.edm_realisation_taps(_oracle_params(R, **kw), Z, reals, nthreads=_threads())
    rs = o["reals"]
    bad = np.zeros(rs.size, bool)
    for k in TAPS:
        dev, ref = d[k].reshape(S, R)[:, rs], o[k]
        same = dev == ref
        if dev.dtype.kind == "f":
            same |= np.isnan(dev) & np.isnan(ref)
        bad |= ~same.all(axis=0)
    bad |= d["accept"][rs] != o["accept"]
    assert not bad.any(), "%d of %d realisations differ from the oracle, first: %s" % (bad.sum(), rs.size, rs[bad][:10].tolist())
    return o


def assert_whole_launch(edm, f, partial, d, R, S, Z, real_offset=0, mean_quirk=1):
    """every realisation: they differ, Restrict of the device's own events, the count, and the mean against exact sums"""
    t0, i0 = d["t0"].reshape(S, R), d["i0"].reshape(S, R)
    cols = np.unique(np.concatenate([t0.view(np.uint32).astype(np.uint64), i0.astype(np.uint64)]).T, axis=0)
    assert cols.shape[0] >= 0.9 * R, "only %d distinct event columns among %d realisations" % (cols.shape[0], R)
    p = edm.params
    rr = oracle.restrict_f32(d["t0"], d["i0"], d["t1"], d["i1"], p.time_horizon, p.L, p.n_grid)
    assert np.array_equal(d["restricted"], rr, equal_nan=True)
    acc = d["accept"]
    assert set(np.unique(acc).tolist()) <= {0, 1}
    assert partial[S] == acc.sum()
    # the partial block [sums | count | x0] from the device's taps, exactly (oracle/edm_oracle.c, compute_f_impl, dsums)
    x = d["restricted"].reshape(S, R).astype(np.float64)
    quirk = mean_quirk != 0 and real_offset == 0
    use = acc == 1
    if quirk:
        use[0] = False
    exact = np.empty(2 * S + 1)
    for m in range(S):
        exact[m] = math.fsum(x[m, use])
        exact[S + 1 + m] = x[m, 0] if quirk else 0.0
        bound = R * 2.0 ** -52 * math.fsum(np.abs(x[m, use]))
        assert abs(partial[m] - exact[m]) <= bound, (m, partial[m], exact[m], bound)
    exact[S] = acc.sum()
    assert np.array_equal(partial[S + 1:], exact[S + 1:])
    assert np.allclose(edm.residual_from_sums(Z, exact), f, rtol=0, atol=2e-7, equal_nan=True)


# case: (form, n_grid, n_spikes, sigma, R as a function of the CU count, seed, mean_quirk, real_offset, every realisation)
CASES = {
    # more throughput workgroups than are resident at once (about 3 per CU at N = 1024 with per-neuron beta in LDS),
    # a partial last workgroup
    "A_throughput_resident_rounds": (1, 1024, 3, 0.3, lambda c: 4 * 4 * c + 3, 21, 1, 0, False),
    # N not a multiple of 32 (the !TREE arg-min, padding lanes) with a mixed accept mask ...
    "B_throughput_N1000": (1, 1000, 3, 3.0, lambda c: 4 * 4 * c + 1, 11, 0, 0, False),
    # ... and with the kMaxSpikes instantiation (five bumps: at the default parameters no realisation is accepted)
    "B_throughput_N1000_S5": (1, 1000, 5, 3.0, lambda c: 4 * 4 * c + 1, 11, 0, 0, False),
    # at least three grid-stride passes of evolve_wg_kernel
    "C_latency_grid_stride": (4, 1024, 3, 0.3, lambda c: 2 * c * LATENCY_WG_PER_CU + 5, 31, 0, 0, False),
    # the same at Driver.cu's grid with rejected realisations, realisation 0 among them
    "D_latency_rejections": (4, 512, 3, 3.0, lambda c: 2 * c * LATENCY_WG_PER_CU + 5, 14, 1, 0, True),
    # the automatic choice (the latency form for 48 <= R <= CUs)
    "E_auto": (0, 1024, 3, 0.3, lambda c: 200, 41, 1, 0, True),
    # the draw counter (r + real_offset) * n_grid + i passes 2^32 at realisation 508
    "F_auto_counter_past_2_32": (0, 512, 3, 0.3, lambda c: 1000, 11, 1, 8_388_100, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_heterogeneous_launch_matches_the_oracle_realisation_by_realisation(mi_ctx, cus, case):
    form, N, S, sigma, Rof, seed, quirk, off, every = CASES[case]
    R, Z = Rof(cus), (Z3 if S == 3 else Z5)
    kw = dict(n_grid=N, n_spikes=S, beta_stddev=sigma, seed=seed, mean_quirk=quirk, real_offset=off)
    edm, f, partial, d = _launch(mi_ctx, form, R, Z, **kw)
    acc = d["accept"]
    if sigma == 3.0 and S == 3:                       # fixture facts: the case stays heterogeneous in its accept mask
        assert 0 < acc.sum() < R, acc.sum()
    if S == 5:
        assert acc.sum() == 0
    if case.startswith("D"):
        assert quirk == 1 and acc[0] == 0             # the reference's rule with realisation 0 rejected
    if case.startswith("F"):
        assert (off + 507) * N + N - 1 < 2 ** 32 <= (off + 508) * N
    reals = np.arange(R) if every else _sample(R, form, cus, seed)
    assert_realisations_match_oracle(d, R, S, Z, reals, **kw)
    assert_whole_launch(edm, f, partial, d, R, S, Z, real_offset=off, mean_quirk=quirk)
    edm.close()


def test_group_shards_equal_single_device_realisation_by_realisation(mi_ctx):
    """A rehearsal group of three shards on one GPU: each shard's taps, in shard order, are the single-device launch's
    taps, and every realisation is the oracle's (the draw is keyed by the global realisation index)."""
    import armadillocudalinearinterpolation_amd as mi
    R, S = 3001, 3
    kw = dict(n_grid=512, beta_stddev=3.0, seed=14)
    grp = mi.Group([0, 0, 0])
    ge = grp.edm([13.0589], R, **kw)
    fg, pg = ge.ComputeF(Z3, want_partial=True)
    edm, f1, p1, d1 = _launch(mi_ctx, 0, R, Z3, **kw)
    bounds = [ge.shard_bounds(r) for r in range(3)]
    assert bounds[0][0] == 0 and bounds[-1][1] == R and all(bounds[k][1] == bounds[k + 1][0] for k in range(2))
    shards = [ge.shard_debug_read(r) for r in range(3)]
    for (lo, hi), sd in zip(bounds, shards):
        assert sd["accept"].size == hi - lo
    for k in TAPS + ("restricted",):
        cat = np.concatenate([sd[k].reshape(S, -1) for sd in shards], axis=1)
        assert np.array_equal(cat, d1[k].reshape(S, R), equal_nan=True), k
    assert np.array_equal(np.concatenate([sd["accept"] for sd in shards]), d1["accept"])
    assert 0 < d1["accept"].sum() < R and pg[S] == p1[S] == d1["accept"].sum()
    assert_realisations_match_oracle(d1, R, S, Z3, np.arange(R), **kw)
    assert_whole_launch(edm, f1, p1, d1, R, S, Z3)
    assert np.allclose(fg, f1, rtol=0, atol=2e-7)
    edm.close()
    ge.close()
    grp.close()
