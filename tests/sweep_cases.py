"""Shared cases for the region-sweep kernels of interp1 (csrc/mi_interp1_sweep.hpp): eight tables
that between them reach every table mode and every closed form a test can reach, and one seeded query vector built
tile by tile so that neighbouring tiles of a workgroup have sharply different region histograms.

Plain numpy plus the CPU oracle for its SplitMix64 stream: no torch, no GPU.  tests/test_sweep_cases_cpu.py checks the
reference on these cases (oracle.interp1_bracket against the literal Armadillo scan and against the exact rational
interpolant); tests/test_sweep_edges_gpu.py holds the three sweep kernels, the streaming kernel and the table-in-LDS
kernel to oracle.interp1_bracket on every element, bit for bit.

Tables (TABLE_SPECS): n = 50 000 nodes -- 400 KB as Y only, 800 KB as {x,y} nodes, both beyond the 128 KiB window of the
whole-table-in-LDS kernel, so with MI_SWEEP_MIN_BYTES=0 the region sweep is taken.  Each entry states the mode, and for
mode 0 the closed form and the pinned last node, that the library must report for it (mi_grid1_info,
mi_debug_grid1_formula).  Closed form 2 (x0 + span * (i / den) with the IEEE quotient) is left out on purpose:
detect_closed_form tries form 3 (the same expression with the quotient from a Markstein step) first, and for
3 + 5 * (i / (n-1)) no n in 20 001 ... 69 999 makes the two differ at any node, so no grid of this family reaches it.
`clustered` is made unique AFTER its shift (1e3 + u^3 rounds neighbouring nodes together): 49 997 nodes, the closest
pairs one ulp apart.

Y = sin(5 (X - X0) / (Xl - X0)) + 0.25 (X - X0).

Query vector (query_vector): tiles of TILE = 16 384 queries, the kernels' tile.  With C workgroups (the CU count) tile
t belongs to workgroup t % C as its local tile t // C, and gets pattern (t + t // C) % 13: consecutive tiles of one
workgroup differ, and every pattern occurs at both parities of the local index (both wave groups of the pipelined
kernels).  The patterns are listed at PATTERNS.  The full vector is 3C + 2 tiles plus a tail of TAIL = 4099 queries of
pattern 7; the sizes under test (prefix_sizes) are its prefixes of T in {1, 2, C+1, 2C+1, 3C+2} tiles, each with 0 and
with 4099 queries more.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import oracle

TILE = 16384
TAIL = 4099
BINS = 256                 # regions of the sweep's counting sort (kSweepBins)
N_NODES = 50_000
NPATTERNS = 13
CPU_C = 256                # the CU count the CPU file builds the vector for (an MI355X has 256)

# name -> (mode, formula, pin_last) the library must report; formula / pin_last are None for the {x,y} modes
TABLE_SPECS = {
    "cf_fma": (0, 0, 0),
    "cf_mul": (0, 1, 0),
    "cf_mul_pinned": (0, 1, 1),
    "cf_fma_pinned": (0, 0, 1),
    "cf_div": (0, 3, 0),
    "jitter": (3, None, None),
    "walk": (1, None, None),
    "clustered": (2, None, None),
}
TABLES = list(TABLE_SPECS)

PATTERNS = [
    "uniform over the range widened by 1 % each side",
    "one cell midpoint 16 384 times",
    "all inside region 0",
    "all inside region 255, every seventh query exactly xmax",
    "all NaN",
    "all below the range, -inf and nextafter(xmin, -inf) among them",
    "all above the range, +inf, nextafter(xmax, +inf) and 1e300 among them",
    "4096 consecutive nodes, each with its two ulp neighbours and the midpoint to the next node, permuted",
    "the 257 region boundaries and their ulp neighbours, repeated and permuted",
    "lanes alternating between the lowest and the highest 1/300 of the range",
    "sorted descending over the whole range",
    "sorted ascending over the whole range",
    "a quarter NaN, a quarter far out of range, X[0] and X[-1] exactly, random values; -0.0 and 5e-324 where 0 is in range",
]
assert len(PATTERNS) == NPATTERNS


# ---------------------------------------------------------------------------------------------- tables
def make_nodes(kind, n=N_NODES):
    """abscissae of one table family at n nodes (the LDS-window tables of the GPU file reuse cf_div and jitter)"""
    i = np.arange(n, dtype=np.float64)
    u = oracle.splitmix_uniform(7, n)
    if kind in ("cf_fma", "cf_fma_pinned"):
        X = -1.0 + 2.0 ** -7 * i                       # every product and sum exact: fma(i, dx, x0) reproduces it
    elif kind in ("cf_mul", "cf_mul_pinned"):
        X = 0.1 + 0.3 * i                              # two roundings per node
    elif kind == "cf_div":
        X = 3.0 + 5.0 * (i / (n - 1))
    elif kind == "jitter":
        X = -2.0 + 3.0 * (i + 0.5 * u) / n
    elif kind == "walk":                               # more than a cell off the straight line: guess + bounded walk
        X = np.unique(np.sort((i + 1.5 * u) / n))
    elif kind == "clustered":                          # bucket index + binary search
        X = np.unique(1e3 + np.unique(np.sort(u ** 3)))
    else:
        raise ValueError(kind)
    if kind.endswith("_pinned"):
        X = X.copy()
        X[-1] = np.nextafter(X[-1], np.inf)
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert np.all(np.diff(X) > 0) and np.all(np.isfinite(X))
    return X


def make_values(X):
    return np.sin(5.0 * (X - X[0]) / (X[-1] - X[0])) + 0.25 * (X - X[0])


@functools.lru_cache(maxsize=None)
def table(name, n=N_NODES):
    """{"name", "X", "Y", "mode", "formula", "pin_last"} of one entry of TABLE_SPECS (arrays are shared: do not modify)"""
    X = make_nodes(name, n)
    mode, formula, pin = TABLE_SPECS[name]
    X.setflags(write=False)
    Y = make_values(X)
    Y.setflags(write=False)
    return {"name": name, "X": X, "Y": Y, "mode": mode, "formula": formula, "pin_last": pin}


# ---------------------------------------------------------------------------------------------- regions
def region(q, X):
    """the region sweep_bin (csrc/mi_interp1_eval.hpp) sorts a query into: clamp((int)((q - xmin) * bscale), 0, 255) with
    bscale = 256 / (xmax - xmin) and a saturating conversion (NaN -> 0)"""
    xmin, xmax = float(X[0]), float(X[-1])
    bscale = BINS / (xmax - xmin)
    with np.errstate(all="ignore"):
        t = (np.asarray(q, dtype=np.float64) - xmin) * bscale
    t = np.where(np.isnan(t), 0.0, np.clip(t, 0.0, BINS - 1.0))
    return t.astype(np.int64)                          # truncation of a value in [0, 255]


def in_range(q, X):
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (q >= X[0]) & (q <= X[-1])


# ---------------------------------------------------------------------------------------------- the query vector
def pattern_of_tile(t, C):
    return (t + t // C) % NPATTERNS


def full_tiles(C):
    return 3 * C + 2


def prefix_sizes(C):
    """[(tiles, tail, nq)] of the ten sizes under test"""
    return [(T, tail, T * TILE + tail) for T in (1, 2, C + 1, 2 * C + 1, 3 * C + 2) for tail in (0, TAIL)]


def _inside(X, u):
    """u in [0, 1) -> in-range values spread over [xmin, xmax]"""
    xmin, xmax = float(X[0]), float(X[-1])
    return np.minimum(xmin + (xmax - xmin) * u, xmax)


def make_tile(X, t, pattern, seed):
    """the TILE queries of tile t under `pattern` (0 .. 12) for the table with abscissae X"""
    n = X.size
    xmin, xmax = float(X[0]), float(X[-1])
    span = xmax - xmin
    rng = np.random.default_rng([0x5EE9, seed, t, pattern])
    if pattern == 0:
        return (xmin - 0.01 * span) + (1.02 * span) * rng.random(TILE)
    if pattern == 1:
        k = (t * 7919 + 13) % (n - 1)
        return np.full(TILE, 0.5 * (X[k] + X[k + 1]))
    if pattern == 2:
        return xmin + (span / BINS) * (0.999 * rng.random(TILE))
    if pattern == 3:
        q = np.minimum(xmin + span * ((BINS - 1 + 0.002 + 0.997 * rng.random(TILE)) / BINS), xmax)
        q[::7] = xmax
        return q
    if pattern == 4:
        return np.full(TILE, np.nan)
    if pattern in (5, 6):
        far = span * (1e-9 + 10.0 ** rng.uniform(-6.0, 6.0, TILE))
        if pattern == 5:
            q = xmin - far
            q[rng.choice(TILE, 96, replace=False)] = np.repeat([-np.inf, np.nextafter(xmin, -np.inf), -1e300], 32)
            assert np.all(q < xmin)
        else:
            q = xmax + far
            q[rng.choice(TILE, 96, replace=False)] = np.repeat([np.inf, np.nextafter(xmax, np.inf), 1e300], 32)
            assert np.all(q > xmax)
        return q
    if pattern == 7:
        s = (t * 4096) % (n - 4097)
        a, b = X[s:s + 4096], X[s + 1:s + 4097]
        q = np.concatenate([a, np.nextafter(a, -np.inf), np.nextafter(a, np.inf), 0.5 * (a + b)])
        return rng.permutation(q)
    if pattern == 8:
        b = xmin + np.arange(BINS + 1, dtype=np.float64) * (span / BINS)
        b[-1] = xmax
        q = np.concatenate([b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)])
        return rng.permutation(np.resize(q, TILE))
    if pattern == 9:                                   # a lane holds two neighbouring queries (one 16-byte vector)
        u = rng.random(TILE) * (span / 300.0)
        lane = (np.arange(TILE) // 2) & 1
        return np.where(lane == 0, np.minimum(xmin + u, xmax), np.maximum(xmax - u, xmin))
    if pattern in (10, 11):
        q = np.sort(_inside(X, rng.random(TILE)))
        return q[::-1].copy() if pattern == 10 else q
    if pattern == 12:
        q = _inside(X, rng.random(TILE))
        quarter = TILE // 4
        q[:quarter] = np.nan
        far = span * (1.0 + 100.0 * rng.random(quarter))
        q[quarter:2 * quarter] = np.where(np.arange(quarter) & 1, xmax + far, xmin - far)
        k = 2 * quarter
        edge = [X[0], X[-1], np.nextafter(X[0], -np.inf), np.nextafter(X[0], np.inf), np.nextafter(X[-1], -np.inf),
                np.nextafter(X[-1], np.inf), X[1], X[-2], np.nextafter(X[-2], -np.inf), np.nextafter(X[-2], np.inf)]
        if xmin <= 0.0 <= xmax:
            edge += [-0.0, 0.0, 5e-324, -5e-324]
        for v in edge:
            q[k:k + 32] = v
            k += 32
        return rng.permutation(q)
    raise ValueError(pattern)


def query_vector(name, C, n=N_NODES, kind=None):
    """the full query vector of table `name` for C workgroups: full_tiles(C) tiles and the pattern-7 tail"""
    X = make_nodes(kind, n) if kind else table(name, n)["X"]
    seed = (TABLES + ["lds_closed", "lds_jitter"]).index(name)
    T = full_tiles(C)
    xq = np.empty(T * TILE + TAIL, dtype=np.float64)
    for t in range(T):
        xq[t * TILE:(t + 1) * TILE] = make_tile(X, t, pattern_of_tile(t, C), seed)
    xq[T * TILE:] = make_tile(X, T, 7, seed)[:TAIL]
    return xq


def pattern_index(C):
    """int8[len(query_vector)]: the pattern every query of the full vector belongs to"""
    T = full_tiles(C)
    p = np.array([pattern_of_tile(t, C) for t in range(T)], dtype=np.int8)
    return np.concatenate([np.repeat(p, TILE), np.full(TAIL, 7, dtype=np.int8)])


# ---------------------------------------------------------------------------------------------- references
def with_extrap(ref_nan, xq, X, extrap):
    """the reference under another extrapolation value, from the one computed with extrap = NaN: queries that are
    neither NaN nor in range get `extrap` (what the header states; the CPU file holds the oracle to it)"""
    xq = np.asarray(xq, dtype=np.float64)
    out = np.array(ref_nan, dtype=np.float64, copy=True)
    out[~in_range(xq, X) & ~np.isnan(xq)] = extrap
    return out


def same_bits(got, ref):
    """NaN where the reference has NaN, the same 64 bits everywhere else (the sign of zero included)"""
    got = np.ascontiguousarray(got, dtype=np.float64)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    return got.shape == ref.shape and bool(np.all(np.where(nan, np.isnan(got), got.view(np.int64) == ref.view(np.int64))))


def exact_interp(X, Y, q):
    """the exact rational interpolant at one in-range query (fractions.Fraction), and the bracket (l, r)"""
    q = float(q)
    assert X[0] <= q <= X[-1]
    l = int(np.searchsorted(X, q, side="right")) - 1
    r = min(l + 1, X.size - 1)
    if r == l:
        return Fraction(float(Y[l])), l, r
    w = (Fraction(q) - Fraction(float(X[l]))) / (Fraction(float(X[r])) - Fraction(float(X[l])))
    return (1 - w) * Fraction(float(Y[l])) + w * Fraction(float(Y[r])), l, r


BLEND_BOUND_UNITS = 8      # |oracle - exact| <= 8 * 2^-53 * (|Y[l]| + |Y[r]|): derived in tests/test_sweep_cases_cpu.py


def blend_error_units(X, Y, q, got):
    """|got - exact| in units of 2^-53 * (|Y[l]| + |Y[r]|), as a float (exact arithmetic up to the final conversion)"""
    ex, l, r = exact_interp(X, Y, q)
    scale = Fraction(1, 2 ** 53) * (abs(Fraction(float(Y[l]))) + abs(Fraction(float(Y[r]))))
    err = abs(Fraction(float(got)) - ex)
    if scale == 0:
        return 0.0 if err == 0 else math.inf
    return float(err / scale)
