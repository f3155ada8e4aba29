"""Shared cases for the multi-GPU layer's original entry points (csrc/mi_group.hip: mi_group_interp1_f64_host / _dev,
mi_group_interp2_f64_host / _dev, the chunked gather of mi_group_set_gather_chunks, group EDM): the small tables, the
groups, the (n_per_shard, K) pairs of the chunked gather with a pure-Python copy of its chunk arithmetic, and the host
forms' query counts.

Plain numpy plus the CPU oracle: no torch, no GPU.  tests/test_group_cases_cpu.py proves that the pairs reach every branch
of the arithmetic; tests/test_group_edges_gpu.py and tests/test_group_order_gpu.py run the cases on the device and hold
every result to oracle.interp1_arma / oracle.interp2_bilinear bit for bit.
"""
import functools

import numpy as np

import oracle
from sweep_cases import same_bits  # noqa: F401  (re-exported: NaN where the reference has NaN, else the same 64 bits)

MAX_CHUNKS = 64                                   # mi_group_set_gather_chunks accepts [1, 64]
REHEARSAL_GROUPS = [[0], [0, 0], [0, 0, 0], [0] * 5]


def chunk_plan(n, K):
    """What mi_group_interp1_f64_dev does with a gathered call of n queries per shard under K gather chunks (the arithmetic
    of interp1_chunked_gather): None when it takes the unchunked path (K == 1 or n < 2K), else the list of (offset, length)
    of the chunks: c = ceil(n / K) rounded up to even, ceil(n / c) chunks, the last one possibly shorter."""
    assert 1 <= K <= MAX_CHUNKS and n >= 0
    if K == 1 or n < 2 * K:
        return None
    c = (n + K - 1) // K
    c += c & 1
    plan = []
    k = 0
    while k * c < n:
        plan.append((k * c, min(c, n - k * c)))
        k += 1
    return plan


# (n_per_shard, K): what each pair is for is asserted by tests/test_group_cases_cpu.py
CHUNK_PAIRS = [
    (0, 3), (1, 3), (2, 3), (3, 3), (4097, 3),    # the sizes every form is run at
    (0, 1), (1, 1), (3, 1), (4097, 1),            # the same, unchunked by choice
    (13, 7),                                      # n = 2K - 1: the fallback
    (14, 7),                                      # n = 2K: the first chunked size
    (3, 2), (4, 2),                               # the same threshold at the smallest K that chunks
    (15, 7),                                      # c = 4: 4 chunks, fewer than K, the last of length 3
    (50, 7),                                      # c = 8: exactly K chunks, the last of length 2
    (5, 2),                                       # c = 4: the last chunk has length 1
    (56, 7),                                      # c = 8: exactly K chunks, the last one full
    (127, 64), (128, 64), (4097, 64), (4100, 64),  # K = 64: fallback, first chunked size (c = 2), 63 and 60 chunks
    (4097, 7), (4099, 2),                         # odd n with several members: slots start 8-byte aligned only
]

CHUNK_SEQUENCE = [1, 7, 2, 64, 3]                 # K changed on one live group: the event vectors grow, then are partly used


def host_counts(P):
    """query counts of the host forms for a group of P members: some members get an empty shard below P"""
    return sorted({0, 1, 2, max(P - 1, 0), P, P + 1, 2 * P + 1, 4099})


HOST_LARGE = 200_003                              # large -> 1 -> large on one live group: scratch grown, kept, reused


@functools.lru_cache(maxsize=None)
def table1(kind="nonuniform"):
    """1 001 nodes: "nonuniform" (cumulated random steps) or "uniform" (k / 1000)"""
    n = 1001
    if kind == "uniform":
        X = np.arange(n) / (n - 1)
    else:
        X = np.cumsum(0.25 + oracle.splitmix_uniform(101, n))
        X = (X - X[0]) / (X[-1] - X[0])
    Y = np.sin(7.0 * X) + 0.5 * X + 2.0          # > 0 at X = 0 .. 1: a query read as 0 never gives the right value by luck
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def table2():
    """33 x 29 grid: x uniform, y non-uniform; Z is (ny, nx)"""
    nx, ny = 33, 29
    x = np.linspace(0.0, 1.0, nx)
    y = np.cumsum(0.5 + oracle.splitmix_uniform(103, ny))
    y = (y - y[0]) / (y[-1] - y[0])
    z = np.sin(3 * y)[:, None] * np.cos(2 * x)[None, :] + 0.1 * x[None, :] * y[:, None] + 3.0
    for a in (x, y, z):
        a.setflags(write=False)
    return x, y, z


def queries(seed, n, lo=-0.05, hi=1.05, specials=True):
    """n queries over [lo, hi) (the tables span [0, 1]: about a tenth are out of range); with specials the first elements
    are NaN, +inf, -inf, both ends of the table, one ulp outside either end -- as many of them as fit"""
    q = lo + oracle.splitmix_uniform(seed, n) * (hi - lo)
    if specials:
        sp = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, np.nextafter(0.0, -1.0), np.nextafter(1.0, 2.0)])
        m = min(n, sp.size)
        q[:m] = sp[:m]
    return q


def inside_queries(seed, n):
    """n queries strictly inside (0.05, 0.95): none of them is 0, whose table value a stale read would return"""
    return 0.05 + oracle.splitmix_uniform(seed, n) * 0.9
