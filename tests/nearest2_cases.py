"""Inputs and references shared by tests/test_interp2_nearest_cpu.py and tests/test_interp2_nearest_gpu.py.

Plain numpy: no torch, no GPU.  The 2-D nearest rule (include/mi355_interp.h) is the 1-D rule per axis, so every
reference here is nearest_cases.rule_index on the x axis and on the y axis and one copy Z[ky, kx]:
    either coordinate NaN -> NaN;  else either coordinate out of range -> extrap;  else Z[ky, kx], the stored bits.
Axes lie on a grid of 1/8 (nearest_batched_cases.nodes and the three kinds below), so that every cell midpoint is an
exact tie; queries per axis are nearest_batched_cases.queries.  Tables hold distinct values that encode (i, j, slice), so
that a wrong index is a visibly wrong value, with inf, -inf, NaN, -0.0 and a denormal at chosen nodes."""
import numpy as np

import nearest_batched_cases as bc
import nearest_cases as nc

POISON = -9.87654321e300          # fills every padding row and slice gap of z: must never appear in an output
SENTINEL = -12345.678             # fills zi before a call: padding rows, gaps and guards must keep it
DENORMAL = 5e-324
KINDS = ("near", "clustered", "uniform")
MAX_WALK = 4                      # kMaxWalk, csrc/mi_interp2_eval.hpp


def axis(kind, rng, n):
    """n strictly increasing nodes on the grid of 1/8.
    near       explicit, steps of 4/8 or 5/8: the index guess stays within kMaxWalk nodes -> guess-and-walk locate
    clustered  explicit, geometric steps 2^k / 8 (a power-of-two grid): the guess is far off -> binary search
    uniform    x0 + i * dx with dx = 1/4, created as an implicit axis (Grid2.uniform / Axis1.uniform)
    random     nearest_batched_cases.nodes"""
    if kind == "near":
        return np.cumsum(rng.integers(4, 6, n)) / 8.0 - 3.0
    if kind == "clustered":
        return np.cumsum(2.0 ** np.arange(n)) / 8.0 - 3.0
    if kind == "uniform":
        return UNIFORM_X0 + UNIFORM_DX * np.arange(n)
    return bc.nodes(rng, n)


UNIFORM_X0, UNIFORM_DX = -1.5, 0.25


def uses_guess(X):
    """the rule of make_explicit_axis (csrc/mi_interp2.hip, csrc/mi_cols1.hip): analytic guess + walk when the guess stays
    within kMaxWalk nodes of every node, else binary search"""
    n = X.size
    scale = (n - 1) / (X[-1] - X[0])
    gi = np.clip(((X - X[0]) * scale).astype(np.int64), 0, n - 1)
    e = gi - np.arange(n)
    return int(max(e.max(), 0) - min(e.min(), 0) + 1) <= MAX_WALK


def table(ny, nx, s=0, specials=True):
    """Z[i, j] = 1e6 * (s + 1) + 1000 * (j + 1) + (i + 1): distinct, exact, encodes (i, j, s); the special values at the
    nodes SPECIAL_NODES (inside any table of at least 6 x 6 nodes)"""
    i, j = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    Z = 1e6 * (s + 1) + 1000.0 * (j + 1) + (i + 1.0)
    if specials and ny >= 6 and nx >= 6:
        for (a, b), v in SPECIAL_NODES.items():
            Z[a, b] = v
    return Z


SPECIAL_NODES = {(1, 2): np.inf, (2, 2): -np.inf, (3, 4): np.nan, (0, 0): -0.0, (5, 5): DENORMAL, (4, 1): -0.0}


def cube(ny, nx, S):
    """(ny, nx, S): slice s is table(ny, nx, s), the special values in slice 0 only (they must not reach another slice)"""
    return np.stack([table(ny, nx, s, specials=(s == 0)) for s in range(S)], axis=2)


def _combine(kx, ky):
    """flags of a (row, column) mesh: -2 where either is NaN, else -1 where either is out of range, else 0"""
    f = np.zeros((ky.size, kx.size), dtype=np.int64)
    f[(ky[:, None] == -1) | (kx[None, :] == -1)] = -1
    f[(ky[:, None] == -2) | (kx[None, :] == -2)] = -2               # NaN wins over out-of-range
    return f


def ref_grid(X, Y, Z, xi, yi, extrap=np.nan):
    """(nyi, nxi): ZI[i, j] = Z[ky(yi[i]), kx(xi[j])]"""
    kx, ky = nc.rule_index(X, xi), nc.rule_index(Y, yi)
    f = _combine(kx, ky)
    out = np.asarray(Z, dtype=np.float64)[np.maximum(ky, 0)[:, None], np.maximum(kx, 0)[None, :]]     # a copy of the bits
    out[f == -1] = float(extrap)
    out[f == -2] = np.nan
    return out


def ref_pairs(X, Y, Z, xq, yq, extrap=np.nan):
    """(nq,): out[k] = Z[ky(yq[k]), kx(xq[k])]"""
    kx, ky = nc.rule_index(X, xq), nc.rule_index(Y, yq)
    out = np.asarray(Z, dtype=np.float64)[np.maximum(ky, 0), np.maximum(kx, 0)]
    oor = (kx == -1) | (ky == -1)
    nan = (kx == -2) | (ky == -2)
    out[oor] = float(extrap)
    out[nan] = np.nan
    return out


def ref_slices(X, Y, Zc, xi, yi, extrap=np.nan):
    """(nyi, nxi, S): slice s = ref_grid on Zc[:, :, s]"""
    return np.stack([ref_grid(X, Y, Zc[:, :, s], xi, yi, extrap) for s in range(Zc.shape[2])], axis=2)


def pair_queries(rng, X, Y, nq):
    """nq scattered pairs: bc.queries on each axis, independently permuted; from 4 pairs on, pair 0 is (NaN, NaN), pair 1
    (NaN, out of range) and pair 2 (out of range, NaN)"""
    xq, yq = bc.queries(rng, X, nq), bc.queries(rng, Y, nq)
    if nq >= 4:
        xq[0], yq[0] = np.nan, np.nan
        xq[1], yq[1] = np.nan, Y[-1] + 10.0
        xq[2], yq[2] = X[0] - 10.0, np.nan
    return xq, yq


def x_sequences(X):
    """held-value sequences along x for the tile body (the two-axis analogue of nearest_batched_cases.sequences): runs of
    equal kx, flagged columns inside a run, a run that starts flagged, every node in order, strictly descending xi, kx
    returning to an earlier column, all flagged"""
    n = X.size
    at = lambda k, f: X[k] + f * (X[k + 1] - X[k])  # noqa: E731
    mid = lambda k: 0.5 * X[k] + 0.5 * X[k + 1]  # noqa: E731
    below, above, nan = X[0] - 1.0, X[-1] + 1.0, np.nan
    return {
        "runs of equal kx": [at(0, .125), at(0, .25), at(0, .25), mid(0), at(0, .75), at(1, .25), at(1, .75), at(2, .125), at(2, .25)],
        "flagged columns inside a run": [at(2, .25), nan, at(2, .125), below, mid(2), above, at(1, .75), nan, at(2, .125)],
        "a run that starts flagged": [nan, below, above, at(3, .25), at(3, .125), nan, mid(3)],
        "every node in order": list(X),
        "strictly descending": [X[-1]] + [at(k, .25) for k in range(n - 2, -1, -1)] + [X[0]],
        "kx returning to an earlier column": [at(1, .25), at(4, .25), at(1, .125), at(4, .125), X[1], at(0, .875), X[4]],
        "all flagged": [nan, below, above, nan],
    }
