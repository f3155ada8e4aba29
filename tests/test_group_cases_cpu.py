"""tests/group_cases.py holds what tests/test_group_edges_gpu.py runs: here, without a GPU, the (n_per_shard, K) pairs of the
chunked gather are shown to reach every branch of its chunk arithmetic (csrc/mi_group.hip, interp1_chunked_gather: fallback
below 2K, c = ceil(n / K) rounded up to even, ceil(n / c) chunks), the Python copy of that arithmetic is checked against
its own invariants, and the tables and query sets are shown to be what the GPU tests take them for."""
import numpy as np

import group_cases as gc
import oracle


def _plans():
    return {(n, K): gc.chunk_plan(n, K) for n, K in gc.CHUNK_PAIRS}


def test_chunk_plan_invariants():
    """for every n up to 300 and every K: unchunked exactly when K == 1 or n < 2K; else the chunks tile [0, n) in order,
    start at even offsets (16-byte aligned starts for the vector kernels), all but the last have the even length c, the
    last is 1 .. c long, and there are between 2 and K of them"""
    for K in range(1, gc.MAX_CHUNKS + 1):
        for n in list(range(0, 301)) + [4097, 4099, 1 << 20]:
            plan = gc.chunk_plan(n, K)
            if K == 1 or n < 2 * K:
                assert plan is None
                continue
            c = plan[0][1]
            assert c % 2 == 0 and c >= 2 and c in (-(-n // K), -(-n // K) + 1)
            assert plan[0][0] == 0 and sum(length for _, length in plan) == n
            assert all(plan[i][0] + plan[i][1] == plan[i + 1][0] for i in range(len(plan) - 1))
            assert all(off % 2 == 0 for off, _ in plan)
            assert all(length == c for _, length in plan[:-1]) and 1 <= plan[-1][1] <= c
            assert 2 <= len(plan) <= K and len(plan) == -(-n // c)


def test_the_issue_examples_by_hand():
    assert gc.chunk_plan(15, 7) == [(0, 4), (4, 4), (8, 4), (12, 3)]
    assert len(gc.chunk_plan(50, 7)) == 7 and gc.chunk_plan(50, 7)[-1] == (48, 2)
    assert gc.chunk_plan(5, 2) == [(0, 4), (4, 1)]
    assert gc.chunk_plan(13, 7) is None and gc.chunk_plan(14, 7) == [(2 * k, 2) for k in range(7)]


def test_pairs_reach_every_branch():
    plans = _plans()
    assert len(set(gc.CHUNK_PAIRS)) == len(gc.CHUNK_PAIRS)
    assert all(1 <= K <= gc.MAX_CHUNKS for _, K in gc.CHUNK_PAIRS)
    chunked = {p: v for p, v in plans.items() if v is not None}
    # the fallback at n = 2K - 1 with K > 1 (the last size that is not chunked), and the first chunked size n = 2K
    assert any(K > 1 and n == 2 * K - 1 and plans[(n, K)] is None for n, K in plans)
    assert any(n == 2 * K and plans[(n, K)] is not None for n, K in plans)
    # fewer chunks than K / exactly K chunks
    assert any(len(v) < K for (n, K), v in chunked.items())
    assert any(len(v) == K for (n, K), v in chunked.items())
    # a last chunk of length 1 / of full length / of a length in between
    assert any(v[-1][1] == 1 for v in chunked.values())
    assert any(v[-1][1] == v[0][1] and len(v) > 1 for v in chunked.values())
    assert any(1 < v[-1][1] < v[0][1] for v in chunked.values())
    # ceil(n / K) odd (rounded up to even) and already even
    assert any((-(-n // K)) % 2 == 1 for (n, K) in chunked)
    assert any((-(-n // K)) % 2 == 0 for (n, K) in chunked)
    # K = 64, the maximum: the fallback, the first chunked size and a many-chunk call
    assert plans[(127, 64)] is None and len(plans[(128, 64)]) == 64 and any(K == 64 and len(v) > 32 for (n, K), v in chunked.items() if n > 128)
    # an odd n that is chunked: with several members the slots s * n of the gathered vector start 8-byte aligned only
    assert any(n % 2 == 1 and n > 1000 for (n, K) in chunked)
    # the sizes every form is run at, chunked by request and not
    for n in (0, 1, 2, 3, 4097):
        assert any(m == n and K > 1 for m, K in plans), n
    assert {0, 1, 3, 4097} <= {n for n, K in plans if K == 1}
    # small enough for a test of a few seconds
    assert max(n for n, _ in plans) <= 5000


def test_chunk_sequence_grows_then_partly_uses_the_event_vectors():
    seq = gc.CHUNK_SEQUENCE
    assert seq == [1, 7, 2, 64, 3] and max(seq) == gc.MAX_CHUNKS
    n = 4097                                               # the size the GPU test runs the sequence at
    used = [len(gc.chunk_plan(n, K) or []) for K in seq]
    assert used[0] == 0 and used[1] > used[2] and used[3] > used[1] and used[4] < used[3]


def test_host_counts_leave_members_without_work():
    from armadillocudalinearinterpolation_amd import sharding
    for devices in gc.REHEARSAL_GROUPS:
        P = len(devices)
        counts = gc.host_counts(P)
        assert {0, 1, 2, P, P + 1, 2 * P + 1, 4099} <= set(counts) and (P == 1 or P - 1 in counts)
        for nq in counts:
            sizes = [hi - lo for lo, hi in (sharding.shard_bounds(nq, r, P) for r in range(P))]
            assert sum(sizes) == nq and max(sizes) - min(sizes) <= 1
        if P > 1:
            assert any(0 < nq < P for nq in counts)         # some members get an empty shard, others do not
    assert gc.REHEARSAL_GROUPS == [[0], [0, 0], [0, 0, 0], [0] * 5]


def test_tables_and_queries_are_what_the_gpu_tests_take_them_for():
    for kind in ("nonuniform", "uniform"):
        X, Y = gc.table1(kind)
        assert X.size == 1001 and X[0] == 0.0 and X[-1] == 1.0 and np.all(np.diff(X) > 0) and np.all(Y > 0.5)
    X, _ = gc.table1("nonuniform")
    assert np.ptp(np.diff(X)) > 0.2 * np.mean(np.diff(X))
    Xu, _ = gc.table1("uniform")
    assert np.array_equal(Xu, np.arange(1001) / 1000)
    x, y, z = gc.table2()
    assert z.shape == (29, 33) and x[0] == 0.0 and x[-1] == 1.0 and y[0] == 0.0 and y[-1] == 1.0 and np.all(np.diff(y) > 0)
    q = gc.queries(3, 4097)
    assert np.isnan(q[0]) and q[1] == np.inf and q[2] == -np.inf and q[3] == 0.0 and q[4] == 1.0 and q[5] < 0.0 and q[6] > 1.0
    assert np.sum(q[7:] < 0) > 50 and np.sum(q[7:] > 1) > 50
    assert gc.queries(3, 2).size == 2 and gc.queries(3, 0).size == 0
    # a read that ran too early sees zeros: the table's value there differs from every expected result
    X, Y = gc.table1("nonuniform")
    qi = gc.inside_queries(5, 4098)
    assert qi.min() > 0.05 and qi.max() < 0.95
    ref = oracle.interp1_arma(X, Y, qi)
    stale = oracle.interp1_arma(X, Y, np.zeros(4))
    assert np.all(stale == Y[0]) and not np.any(ref == Y[0])
    ref2 = oracle.interp2_bilinear(x, y, z, gc.inside_queries(6, 2049), gc.inside_queries(7, 2049))
    assert not np.any(ref2 == z[0, 0]) and oracle.interp2_bilinear(x, y, z, np.zeros(1), np.zeros(1))[0] == z[0, 0]
    assert gc.same_bits(np.array([np.nan, -0.0]), np.array([np.nan, -0.0])) and not gc.same_bits(np.array([0.0]), np.array([-0.0]))
