"""GPU checks of the region sweep with the phase classes set apart by work (fractional tiles of
interp1_phased_sweep_kernel, csrc/mi_sweep_phase.hip; ownership: csrc/mi_sweep_partition.hpp).

mi_debug_interp1_phased_sweep_ex launches the kernel on at most 8 or 16 workgroups with a first-tile table.  The tables
(lookup tables, queries, references) are those of tests/test_sweep_phase_gpu.py: its fixtures are imported, that file is
not touched.  Units are 4096 queries.  The unit counts U are chosen by the share w = U / W (some workgroups one more) so
that, with first tiles f = 1..4 by class, some workgroup has: no unit at all (U < W); fewer units than its first tile
wants (w = 1..3 under f = 4); exactly its first tile; f + 1, f + 3, f + 4, f + 5 (w = 2..9 for every f); and f + 4 k + r
up to five and six tiles (w = 12, 13, 16, 17, 19, 20).  Tails 0, 1, 4095.  The largest call is 20 * 16 units + 4095 =
1 314 815 queries.  Results must have the bytes of mi_interp1_f64_dev under the ORDERED hint (the family's streaming
kernel), must leave the 16 384 doubles behind the output alone, and on a 2^16 sample must have the bytes of
oracle.interp1_bracket.  One case runs the stamping instance: same bytes, and no workgroup's stamps decrease."""
import ctypes

import numpy as np
import pytest

import oracle
import sweep_cases as sc
from test_sweep_phase_gpu import GUARD, NMAX, SENT, TILE, _same_bytes, env, table  # noqa: F401  (env, table: fixtures)

pytestmark = pytest.mark.gpu

UNIT = 4096
FORMS = ((4, 4123), (4, 4321), (4, 1234), (2, 42), (1, 4))
WORKGROUPS = (8, 16)
TAILS = (0, 1, 4095)


def unit_counts(W):
    return [3, W - 1, W + 3, 2 * W + 5, 3 * W + 1, 4 * W + W // 2, 5 * W + 3, 6 * W + W - 1, 8 * W + 1, 9 * W + W // 2,
            12 * W + 3, 16 * W + 5, 19 * W + W - 1]


assert (max(unit_counts(16)) + 1) * UNIT <= NMAX and TILE == 4 * UNIT


def _work(env, t, nq, extrap, phases, W, first_units, stamps=None, cap=0, offset=0):
    env.buf.fill_(SENT)
    q = t.q[offset:offset + nq]
    env.check(env.L.mi_debug_interp1_phased_sweep_ex(env.ctx._h, t.grid._h, ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(env.buf.data_ptr()),
                                                     nq, extrap, phases, W, first_units,
                                                     ctypes.c_void_p(stamps.data_ptr()) if stamps is not None else None, cap), env.ctx._h)
    return env.buf[:nq]


@pytest.mark.parametrize("W", WORKGROUPS)
@pytest.mark.parametrize("phases,first_units", FORMS)
def test_bytes_of_the_streaming_kernel_at_every_share(env, table, phases, first_units, W):
    before = env.L.mi_debug_sweep_ds_launches()
    base_before = env.L.mi_debug_sweep_ds_launches_base()
    calls = 0
    for k, U in enumerate(unit_counts(W)):
        # every tail around one and two units per workgroup and at the largest count, one tail (in turn) elsewhere
        tails = TAILS if U in (W - 1, W + 3, 2 * W + 5, 19 * W + W - 1) else (TAILS[k % 3],)
        for tail in tails:
            nq = U * UNIT + tail
            out = _work(env, table, nq, float("nan"), phases, W, first_units)
            calls += 1
            assert _same_bytes(env, out, table.ref["nan"][:nq]), (table.name, phases, first_units, W, U, tail)
            assert bool((env.buf[nq:] == SENT).all()), ("guard", table.name, phases, first_units, W, U, tail)
    assert env.L.mi_debug_sweep_ds_launches() - before == calls
    assert env.L.mi_debug_sweep_ds_launches_base() == base_before


@pytest.mark.parametrize("phases,first_units", FORMS)
def test_below_one_unit_offsets_and_the_other_extrapolation_value(env, table, phases, first_units):
    for W in WORKGROUPS:
        off = 3 * TILE                                                        # (the tile with the special values)
        for nq in (1, 2, 100, 4095):                                          # tail only: no unit
            out = _work(env, table, nq, float("nan"), phases, W, first_units, offset=off)
            assert _same_bytes(env, out, table.ref["nan"][off:off + nq]), (table.name, phases, first_units, W, nq)
            assert bool((env.buf[nq:] == SENT).all()), ("guard", table.name, phases, first_units, W, nq)
        for U, tail in ((2 * W + 5, 4095), (6 * W + W - 1, 1)):
            nq = U * UNIT + tail
            out = _work(env, table, nq, -0.0, phases, W, first_units)
            assert _same_bytes(env, out, table.ref["negzero"][:nq]), (table.name, phases, first_units, W, U, tail)


def test_bytes_of_the_oracle_on_a_sample(env, table):
    idx = np.unique(np.concatenate([np.random.default_rng(5).integers(0, NMAX, 1 << 16), np.arange(3 * TILE, 3 * TILE + 64)]))
    threads = max(1, min(4, oracle.max_threads()))
    want = oracle.interp1_bracket(table.X, table.Y, table.q_np[idx], nthreads=threads)
    for extrap, ref in ((float("nan"), want), (-0.0, sc.with_extrap(want, table.q_np[idx], table.X, -0.0))):
        for phases, first_units, W in ((4, 4123, 16), (2, 42, 8)):
            out = _work(env, table, NMAX, extrap, phases, W, first_units).cpu().numpy()
            assert sc.same_bits(out[idx], ref), (table.name, phases, first_units, W, extrap)


def test_stamps_change_no_byte_and_do_not_decrease(env, table):
    torch = env.torch
    W, cap = 8, 10
    for phases, first_units in ((4, 4123), (4, 0)):                           # the work form and the clock form
        nq = (17 * W + 3) * UNIT + 1
        stamps = torch.full((W * cap,), -1, dtype=torch.int64, device=env.dev)
        out = _work(env, table, nq, float("nan"), phases, W, first_units, stamps=stamps, cap=cap)
        assert _same_bytes(env, out, table.ref["nan"][:nq]), (table.name, phases, first_units)
        assert bool((env.buf[nq:] == SENT).all())
        s = stamps.cpu().numpy().reshape(W, cap)
        for b in range(W):
            written = int((s[b] != -1).sum())
            assert written >= 4 and bool((s[b, :written] != -1).all()), (b, s[b])     # entry, gather steps, exit: a prefix of the slots
            assert bool((np.diff(s[b, :written]) >= 0).all()), (b, s[b])
        # with the capacity too small for the gather steps nothing is written past it
        small = torch.full((W * 2 + 4,), -1, dtype=torch.int64, device=env.dev)
        _work(env, table, nq, float("nan"), phases, W, first_units, stamps=small, cap=2)
        assert bool((small[W * 2:] == -1).all()) and bool((small[:W * 2] != -1).all())


def test_probe_for_the_next_call_runs_under_the_auto_hint(env, table):
    env.ctx.set_query_order(0)
    try:
        for phases, first_units in FORMS:
            nq = (21 * 4 + 3) * UNIT + 1
            out = _work(env, table, nq, float("nan"), phases, 8, first_units)
            env.ctx.synchronize()
            assert _same_bytes(env, out, table.ref["nan"][:nq]), (table.name, phases, first_units)
    finally:
        env.ctx.set_query_order(1)


def test_entry_point_rejects_what_the_kernel_does_not_serve(env, table):
    L = env.L
    q, o = ctypes.c_void_p(table.q.data_ptr()), ctypes.c_void_p(env.buf.data_ptr())
    h, g = env.ctx._h, table.grid._h
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, q, o, TILE, 0.0, 8, 8, 11111111, None, 0) == 1     # an eighth of a tile is no gather pass
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, q, o, TILE, 0.0, 4, 8, 412, None, 0) == 1
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, q, o, TILE, 0.0, 4, 8, 4125, None, 0) == 1
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, q, o, TILE, 0.0, 2, 8, 4123, None, 0) == 1
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, q, o, TILE, 0.0, 3, 8, 444, None, 0) == 1
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, q, o, TILE, 0.0, 4, 0, 4123, None, 0) == 1
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, q, o, TILE, 0.0, 4, 8, 4123, o, 1) == 1           # a stamp buffer needs two slots
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, ctypes.c_void_p(table.q.data_ptr() + 8), o, TILE, 0.0, 4, 8, 4123, None, 0) == 1
    assert L.mi_debug_interp1_phased_sweep_ex(h, None, q, o, TILE, 0.0, 4, 8, 4123, None, 0) == 1
    assert L.mi_debug_interp1_phased_sweep_ex(h, g, q, o, 0, 0.0, 4, 8, 4123, None, 0) == 0            # nothing to do
    env.torch.cuda.synchronize()
