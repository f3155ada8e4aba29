"""Shared cases for non-finite, signed-zero and denormal table VALUES through the interp1 kernels (streaming, scalar,
whole-table-in-LDS and the three region-sweep forms): include/mi355_interp.h says such values "go through the two-term
blend", and the padding node, the pinned last node, the LDS copy of the table and the sweep's trip through LDS are where
a kernel could treat them differently.

Plain numpy plus the CPU oracle: no torch, no GPU.  tests/test_interp2_cases_cpu.py holds oracle.interp1_bracket on these
inputs to the literal Armadillo scan and to the reach property; tests/test_interp1_values_gpu.py holds every kernel to
oracle.interp1_bracket, bit for bit.

Tables: sweep_cases.make_nodes(kind, n).  BIG (n = 50 000, beyond the LDS window): one per table mode.  LDS (the largest
that fit the 128 KiB window with their padding node): closed form n = 16 383, jitter n = 8191.
Y = sweep_cases.make_values(X) with the specials of special_values() written over it, in two variants: the last node NaN,
and the last node -0.0 (the padding node behind the table copies it).
"""
import functools

import numpy as np

import sweep_cases as sc

# name -> (kind, n, mode the library must report)
BIG = {"cf_mul_pinned": ("cf_mul_pinned", sc.N_NODES, 0), "jitter": ("jitter", sc.N_NODES, 3),
       "walk": ("walk", sc.N_NODES, 1), "clustered": ("clustered", sc.N_NODES, 2)}
LDS = {"lds_closed": ("cf_div", 16383, 0), "lds_jitter": ("jitter", 8191, 3)}
SPECS = {**BIG, **LDS}
VARIANTS = ("nan_last", "negzero_last")
NQ_BIG = 2 * sc.TILE + sc.TAIL               # two tiles of the sweep kernels and a ragged tail
NQ_LDS = (1 << 20) + sc.TAIL                 # the LDS kernel is only picked from 2^20 queries
REPEAT = 4                                   # copies of the edge queries in a vector


def special_values(n, variant):
    """{index: value} written over Y"""
    a, b, c, d, e = n // 5, n // 3, n // 2, (2 * n) // 3, (3 * n) // 4
    s = {0: np.inf, n - 1: np.nan if variant == "nan_last" else -0.0, n - 2: -0.0,
         a: np.inf, a + 1: -np.inf,              # +inf next to -inf
         b: np.nan,                              # an isolated NaN
         c: -0.0, c + 1: -0.0,
         d: 5e-324, d + 1: -5e-324,
         e: 1e300, e + 1: -1e300}
    assert len(s) == 12 and variant in VARIANTS
    return s


@functools.lru_cache(maxsize=None)
def nodes(name):
    kind, n, _ = SPECS[name]
    X = sc.make_nodes(kind, n)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def values(name, variant):
    X = nodes(name)
    Y = sc.make_values(X).copy()
    for k, v in special_values(X.size, variant).items():
        Y[k] = v
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def queries(name):
    """for every special index k and k +- 1, k +- 2: the node, its two ulp neighbours and the midpoints to both sides;
    X[0] and X[-1], NaN, +-inf, out of range on both sides; REPEAT copies of all that, filled up with seeded uniform
    queries over the range widened by 1 % each side, and permuted"""
    X = nodes(name)
    n = X.size
    idx = sorted({min(max(k + o, 0), n - 1) for k in special_values(n, VARIANTS[0]) for o in (-2, -1, 0, 1, 2)})
    j = np.array(idx)
    left, right = X[np.maximum(j - 1, 0)], X[np.minimum(j + 1, n - 1)]
    span = X[-1] - X[0]
    edge = np.concatenate([X[j], np.nextafter(X[j], -np.inf), np.nextafter(X[j], np.inf), 0.5 * left + 0.5 * X[j],
                           0.5 * X[j] + 0.5 * right,
                           [X[0], X[-1], np.nan, np.inf, -np.inf, X[0] - 0.5 * span, X[-1] + 0.5 * span, -1e300, 1e300]])
    nq = NQ_LDS if name in LDS else NQ_BIG
    rng = np.random.default_rng([0x1D, list(SPECS).index(name)])
    fill = (X[0] - 0.01 * span) + 1.02 * span * rng.random(nq - REPEAT * edge.size)
    xq = rng.permutation(np.concatenate([np.tile(edge, REPEAT), fill]))
    assert xq.size == nq
    xq.setflags(write=False)
    return xq


def reach_violations(X, Y, xq, out):
    """indices of in-range queries whose result is non-finite although both bracket values are finite, or finite
    although the blend of a non-finite bracket value cannot be (the two-term blend: 0 * inf is NaN)"""
    inr = np.flatnonzero(sc.in_range(xq, X))
    l = np.searchsorted(X, xq[inr], side="right") - 1
    r = np.minimum(l + 1, X.size - 1)
    both = np.isfinite(Y[l]) & np.isfinite(Y[r])
    return inr[np.isfinite(out[inr]) != both]
