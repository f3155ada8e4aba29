"""Seeded differential fuzz of the batched device calls: the generator, the reference, the checker and a numpy model with
planted defects.  Plain numpy plus the CPU oracle: no torch, no GPU, no hypothesis.  tests/test_batched_fuzz_cases_cpu.py
proves that the generator covers what it claims and that check() refuses every planted defect;
tests/test_batched_fuzz_gpu.py and scripts/gpu_fuzz_batched.py run the cases on the device.

    call      C entry point                  Python                               forms
    cols      mi_interp1_cols_f64_dev        Axis1.interp_cols                    lds / direct (n <= 8192)
    rows      mi_interp1_rows_f64_dev        Axis1.interp_rows                    tile16 / tile8 / flat (m < 256)
    stack     mi_interp1_rows_f64_dev        Axis1.interp_stack                   the same, m = ny*nx
    pairs     mi_interp1_pairs_f64_dev       interp_pairs                         lds / direct (n <= 4096)
    each      mi_interp1_each_f64_dev        interp_each                          thin / lds / direct / forwarded
    rowpairs  mi_interp1_rowpairs_f64_dev    interp_rowpairs                      short (n <= 32) / long
    grid      mi_interp2_grid_f64_dev        Grid2.interp_grid                    tile / flat (nyi < 256)
    slices2   mi_interp2_slices_f64_dev      interp2_slices                       lds / direct (nx*ny <= 8192) x tile / flat

case(call, index) is one fully determined case: its random source is default_rng([seed, CALLS.index(call), index]) and
nothing else, so cases do not depend on each other or on the order they are built in.  What has to be covered evenly
(the form, the form-selecting size, the axis kind, the query style, extrap, lens, bad tables, want_ok) is not left to the
stream: it comes from a plan, one per (seed, call, block of CASES_PER_CALL indices) -- the form cycles with the index
(so any few consecutive indices meet every form), the other attributes are balanced shuffles drawn from
default_rng([seed, call, 10**6 + block]).  A draw that degenerates is drawn again from the same stream; no case is dropped.

A case holds the logical arrays (case.arrays), the layout of every operand (case.ops: an Operand says where element
(i, j, s) lies in its flat canvas) and the expected result (case.want, case.want_ok).  canvases(case) builds the flat
canvases: every operand is a strided view into a canvas of its own, FRONT guard elements, then a base offset of 0 or 1
element (the canvas is 256-B aligned on the device, so this picks 16-B or 8-B alignment), then the matrix with its
leading-dimension pad (and slice-stride pad), then TAIL guard elements.  Padding and guards of an input hold NaN; an
output canvas holds SENT_GUARD, its logical elements SENT_FILL.

Sizes straddle every limit of wide_stride_cases.LIMITS (and the grid call's, GRID_THIN_ROWS here) and the tile
boundaries; CAP bounds the table elements and the outputs of a case, and a draw beyond it shrinks the batch dimension,
never the one that selects the form.

Axes.  The shared-axis calls draw one kind per axis (AXIS_KINDS): "uniform" goes through Axis1.uniform / Grid2.uniform
and is held to oracle.interp1_uniform / interp2_bilinear_uniform (x0 and dx are dyadic with few bits, so i*dx is exact
and x0 + i*dx IS fma(i, dx, x0)); the others are explicit nodes.  The paired calls give every table its own kind, origin
and scale around the window [0, 1]: the shared queries are in range for some tables and out of range for others.

Bad tables (pairs, each, rowpairs; BAD_KINDS) give NaN in all their outputs and flag 0; nodes beyond a fill count
hold NaN.  The device forms return MI_OK whatever the tables hold (include/mi355_interp.h: bad tables are data, found
asynchronously; only the _host forms report MI_ERR_GRID), so the status is held by the call not raising, and the
flags by check().

check() is the single checking function.  model_call() is a numpy stand-in for the device call (its own bracket and
blend, not the oracle's: that check() passes it on every case also holds the two against each other) that reads its
inputs from the canvases and writes into copies of them; DEFECTS can be planted in it.  A defect APPLIES to a case when
its structural precondition holds (PRECONDITION, below) AND it changes at least one bit of what the call returns there
(model_call with the defect differs from model_call without): no checker can refuse a defect that returns the right
bits, and the generator plants what makes each one observable (pad_node: +inf in the last-but-one valid value of a good
table whose last node is queried).
"""
import functools

import numpy as np

import wide_stride_cases as W
from wide_stride_cases import COUNTERS, SENT_FILL, SENT_GUARD, _is_bad, _same, same_bits

SEED = 20261021
CALLS = ("cols", "rows", "stack", "pairs", "each", "rowpairs", "grid", "slices2")
CASES_PER_CALL = 48
CAP = 2**18                        # table elements of a case, and its outputs, at most
FRONT, TAIL = 32, 64               # guard elements before (256 B: the alignment is the base offset's) and behind an operand
GRID_THIN_ROWS = 256               # csrc/mi_interp2_grid.hip kThinRows (wide_stride_cases.LIMITS has no grid call)
LIMITS = dict(W.LIMITS, grid_thin_rows=GRID_THIN_ROWS)
PADS = (0, 1, 2, 3, 17)
EXTRAPS = (np.nan, 2.5, -0.0, np.inf)
SCALES = (1.0, 1e200, 1e-200)
SPECIALS = (np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324, -5e-324, 1e300, -1e300)
AXIS_KINDS = ("uniform", "linspace", "jitter", "clustered", "two", "ulp", "huge", "tiny")
TABLE_KINDS = AXIS_KINDS[1:]       # a paired table has explicit nodes
STYLES = ("sorted", "reversed", "permuted", "one_cell", "all_equal", "sawtooth", "on_nodes")
BAD_KINDS = ("equal", "decreasing", "signed_zero", "nan_node", "inf_last", "minf_first", "len0", "len1", "len_n1")
# the first bad table of the 12 bad-table cases of a block: every kind, signed_zero four times (signed_zero_ok needs it)
BAD_FIRST = ("signed_zero", "equal", "decreasing", "nan_node", "signed_zero", "inf_last", "minf_first", "len0", "signed_zero",
             "len1", "len_n1", "signed_zero")
PAIRED = ("pairs", "each", "rowpairs")
DEFECTS = ("pad_node", "ignores_len", "stray_store", "reads_padding", "signed_zero_ok", "nan_is_extrap", "wrong_form")
# the structural half of "applies" (the other half: the defect changes a bit of the result, see the module docstring)
PRECONDITION = {
    "pad_node": "every call; observable where a good table's last valid node is queried and the value before it is not finite",
    "ignores_len": "paired calls: lens is given and some len < n",
    "stray_store": "every call, every case",
    "reads_padding": "every call but grid (its Z is a dense host array): some 2-D input has a padded leading dimension (stack: slice stride)",
    "signed_zero_ok": "paired calls: some table is bad by the pair -0.0, 0.0 and by nothing else",
    "nan_is_extrap": "every call: extrap is not NaN and a NaN query reaches a good table",
    "wrong_form": "the calls with a form counter (wide_stride_cases.COUNTERS), every case",
}

FORMS = {
    "cols": ("lds", "direct"), "rows": ("tile16", "tile8", "flat"), "stack": ("tile16", "tile8", "flat"),
    "pairs": ("lds", "direct"), "each": ("thin", "lds", "direct", "forwarded"), "rowpairs": ("short", "long"),
    "grid": ("tile", "flat"), "slices2": ("lds-tile", "lds-flat", "direct-tile", "direct-flat"),
}
COUNTER_CALL = {"rows": "rows", "stack": "rows", "each": "each", "rowpairs": "rowpairs", "slices2": "slices2"}   # call -> COUNTERS key
COLS_SET = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 2051)
QUERY_SET = (1, 2, 7, 8, 9, 63, 65, 255, 257, 511, 513, 2047, 2049, 4100)
SMALL_NODES = (2, 3, 5, 31, 32, 33, 255, 257)


def _node_sets(limit):
    return (2, 3, 5, 31, 32, 33, 255, 257, limit - 1, limit), (limit + 1, limit + 2, 9001)


# ---- layout ---------------------------------------------------------------------------------------------------------------

class Operand:
    """where the (rows, cols, S) array of one operand lies in its flat canvas: element (i, j, s) at
    FRONT + base + i + j*ld + s*stride; a vector has cols == S == 1"""

    def __init__(self, name, role, rows, cols=1, S=1, base=0, ld=None, stride=None):
        self.name, self.role, self.rows, self.cols, self.S, self.base = name, role, int(rows), int(cols), int(S), int(base)
        self.ld = int(rows if ld is None else ld)
        self.stride = int(self.ld * cols if stride is None else stride)
        assert self.ld >= self.rows and self.stride >= self.ld * self.cols

    @property
    def shape(self):
        return (self.rows, self.cols, self.S)

    @property
    def start(self):
        return FRONT + self.base

    @property
    def extent(self):
        return (self.S - 1) * self.stride + (self.cols - 1) * self.ld + self.rows

    @property
    def size(self):
        return self.start + self.extent + TAIL

    def index(self):
        """canvas index of every logical element, an int64 array of shape (rows, cols, S)"""
        i = np.arange(self.rows, dtype=np.int64)[:, None, None]
        j = np.arange(self.cols, dtype=np.int64)[None, :, None]
        s = np.arange(self.S, dtype=np.int64)[None, None, :]
        return self.start + i + j * self.ld + s * self.stride

    def describe(self):
        return "%s[%dx%dx%d base %d ld %d stride %d]" % (self.name, self.rows, self.cols, self.S, self.base, self.ld, self.stride)


class Case:
    """One call.  arrays: the logical operands by name (2-D / 3-D arrays as the API sees them, "lens" int32); axis / axes:
    how the shared axes are made ({"kind", "nodes"} and, for "uniform", "x0", "dx"); ops: the Operand of every device operand;
    out: the output operand's name; form / counter: the predicted form and its index among COUNTERS (None: no counter);
    want: the expected output, shape ops[out].shape; want_ok: the expected flags, or None when the call is made without
    want_ok; meta: what the census counts."""

    def __init__(self, **k):
        self.__dict__.update(k)
        self.id = "%s-%d" % (self.call, self.index)

    def __repr__(self):
        return "%s(%s %s)" % (self.id, self.form, " ".join(o.describe() for o in self.ops.values()))

    def key_bytes(self):
        """every byte that defines the case: for the determinism check"""
        parts = [repr((self.call, self.index, self.form, self.counter, self.extrap, self.use_ok, sorted(self.meta.items()),
                       [o.describe() for o in self.ops.values()])).encode()]
        for name in sorted(self.arrays):
            parts.append(np.ascontiguousarray(self.arrays[name]).tobytes())
        for ax in self.axes.values():
            parts.append(repr((ax["kind"], ax.get("x0"), ax.get("dx"))).encode() + np.ascontiguousarray(ax["nodes"]).tobytes())
        parts.append(self.want.tobytes())
        parts.append(b"" if self.want_ok is None else self.want_ok.tobytes())
        return b"|".join(parts)


# ---- axes, values, queries ------------------------------------------------------------------------------------------------

def _unit_axis(rng, kind, n):
    """n strictly increasing finite nodes of the kind: about [0, 1] for the ordinary kinds"""
    i = np.arange(n, dtype=np.float64)
    while True:
        if kind == "linspace":
            x = np.linspace(0.0, 1.0, n)
        elif kind in ("jitter", "two"):
            x = (i + 0.4 * rng.random(n)) / n
        elif kind == "clustered":
            x = np.cumsum(rng.random(n) ** 6 + 1e-9)
            x = x / x[-1]
        elif kind == "ulp":
            first = np.array([rng.uniform(0.25, 0.75)])
            steps = np.concatenate(([0], np.cumsum(rng.integers(1, 4, n - 1))))
            x = (first.view(np.int64) + steps).view(np.float64)
        elif kind == "huge":
            x = 1e307 * (-1.0 + 2.0 * (i + 0.3 * rng.random(n)) / n)
        elif kind == "tiny":
            x = 1e-300 * (-1.0 + 2.0 * (i + 0.3 * rng.random(n)) / n)
        else:
            raise ValueError(kind)
        if x.size == n and np.all(np.isfinite(x)) and np.all(x[:-1] < x[1:]):
            return x


def _shared_axis(rng, kind, n):
    """an axis of a shared-axis call: {"kind", "nodes"} (+ "x0", "dx" for "uniform": nodes fma(i, dx, x0), exactly)"""
    if kind == "uniform":
        x0 = float(rng.integers(-64, 65)) / 16.0
        dx = float(rng.integers(1, 2**12)) / 1024.0
        nodes = x0 + np.arange(n, dtype=np.float64) * dx          # i*dx is exact (26 bits at most): one rounding, as fma
        return {"kind": kind, "nodes": nodes, "x0": x0, "dx": dx}
    x = _unit_axis(rng, kind, n)
    if kind in ("linspace", "jitter", "clustered", "two"):
        x = rng.uniform(-3.0, 3.0) + rng.uniform(0.1, 4.0) * x
        assert np.all(x[:-1] < x[1:])
    return {"kind": kind, "nodes": x}


def _values(rng, shape, special):
    y = rng.standard_normal(shape) * SCALES[rng.integers(len(SCALES))]
    if special:
        hit = rng.random(shape) < 0.01
        y[hit] = np.asarray(SPECIALS)[rng.integers(0, len(SPECIALS), int(hit.sum()))]
    return y


def _lerp(a, b, u):
    return np.clip(a * (1.0 - u) + b * u, a, b)


def _queries(rng, x, count, style):
    """count queries on the table x in the style, then the mandatory points over the first of them that fit, in order of
    rank: the last node, NaN, the first node, a point above, one below, +inf, -inf -- and the whole shuffled where the
    style is no order of its own"""
    n, a, b = x.size, x[0], x[-1]
    if style in ("sorted", "reversed", "permuted"):
        q = _lerp(a, b, rng.random(count))
        if style != "permuted":
            q = np.sort(q)
            if style == "reversed":
                q = q[::-1].copy()
    elif style == "one_cell":
        c = int(rng.integers(0, n - 1))
        q = _lerp(x[c], x[c + 1], rng.random(count))
    elif style == "all_equal":
        q = np.full(count, _lerp(a, b, rng.random()))
    elif style == "sawtooth":
        t = np.cumsum(rng.random(count) * (4.0 / max(count, 4)))
        back = rng.random(count) < 0.08
        t = t - np.cumsum(np.where(back, rng.random(count), 0.0))
        q = _lerp(a, b, np.abs(np.mod(t, 2.0) - 1.0) if rng.random() < 0.2 else np.mod(t, 1.0))
    elif style == "on_nodes":
        k = rng.integers(0, n, count)
        pick = x[k]
        how = rng.integers(0, 4, count)
        mid = 0.5 * x[k] + 0.5 * x[np.minimum(k + 1, n - 1)]
        q = np.where(how == 0, pick, np.where(how == 1, np.nextafter(pick, -np.inf), np.where(how == 2, np.nextafter(pick, np.inf), mid)))
    else:
        raise ValueError(style)
    must = [b, np.nan, a, np.nextafter(b, np.inf), np.nextafter(a, -np.inf), np.inf, -np.inf][:count]
    slots = rng.permutation(count)[:len(must)]
    q = np.array(q, dtype=np.float64)
    q[slots] = must
    return q


# ---- the plan -------------------------------------------------------------------------------------------------------------

def _balanced(rng, items, count):
    reps = -(-count // len(items))
    seq = [items[k % len(items)] for k in range(reps * len(items))][:count]
    return [seq[k] for k in rng.permutation(count)]


@functools.lru_cache(maxsize=None)
def _plan(seed, call, block):
    """the balanced attributes of the CASES_PER_CALL cases of one block: a dict of lists"""
    rng = np.random.default_rng([seed, CALLS.index(call), 10**6 + block])
    N = CASES_PER_CALL
    forms = FORMS[call]
    off = int(rng.integers(len(forms)))
    P = {"form": [forms[(k + off) % len(forms)] for k in range(N)],
         "kind": _balanced(rng, AXIS_KINDS, N), "kind2": _balanced(rng, AXIS_KINDS, N),
         "style": _balanced(rng, STYLES, N), "style2": _balanced(rng, STYLES, N),
         "extrap": _balanced(rng, range(len(EXTRAPS)), N), "special": _balanced(rng, (True, False, False), N),
         "trap": _balanced(rng, (True, False, False), N), "use_ok": _balanced(rng, (True, False), N)}
    # the k-th case of a form takes the k-th of that form's size candidates, shuffled: every candidate comes round
    P["pick"] = [0] * N
    for f in forms:
        mine = [k for k in range(N) if P["form"][k] == f]
        order = rng.permutation(len(mine))
        for r, k in zip(order, mine):
            P["pick"][k] = int(r)
    # lens in half of the cases, bad tables in half of those, each evenly over the forms
    lens, bad = [False] * N, [None] * N
    nbad = 0
    for f in forms:
        mine = [k for k in range(N) if P["form"][k] == f]
        mine = [mine[r] for r in rng.permutation(len(mine))]
        for r, k in enumerate(mine):
            lens[k] = r % 2 == 0
            if r % 4 == 0:
                bad[k] = nbad
                nbad += 1
    P["lens"], P["bad"] = lens, bad
    # operands that only some cases have: each (thin form) takes one shared XI in half of its cases, and the base offsets of
    # lens and of the two kinds of XI alternate over the cases that have them
    thin = [k for k in range(N) if P["form"][k] == "thin"]
    P["shared"] = [P["form"][k] == "forwarded" or (k in thin and thin.index(k) % 2 == 0) for k in range(N)]

    def alternate(subset):
        return {k: r % 2 for r, k in enumerate(subset[j] for j in rng.permutation(len(subset)))} if subset else {}

    P["base_lens"] = alternate([k for k in range(N) if lens[k]])
    P["base_q"] = alternate([k for k in range(N) if P["shared"][k]])
    P["base_q"].update(alternate([k for k in range(N) if not P["shared"][k]]))
    return P


def _pick(cands, r):
    return cands[r % len(cands)]


def _fit(cands, limit):
    """the candidates that are at most limit (the smallest one if none is)"""
    ok = [c for c in cands if c <= limit]
    return ok or [min(cands)]


def _sizes(call, form, r, rng):
    """the sizes of a case: the form-selecting ones from the r-th candidate of the form, the others from the stream, the batch
    dimension shrunk to CAP"""
    L = LIMITS
    if call in ("cols", "pairs"):
        lo, hi = _node_sets(L["cols_lds_n"] if call == "cols" else L["pairs_lds_n"])
        n = _pick(lo if form == "lds" else hi, r)
        nq = int(rng.choice(QUERY_SET))
        B = int(rng.choice(_fit(COLS_SET, min(CAP // n, CAP // nq))))
        return {"n": n, "nq": nq, "B": B}
    if call == "each":
        lo, hi = _node_sets(L["pairs_lds_n"])
        tn, tq = L["each_thin_n"], L["each_thin_q"]
        thin = [(n, q) for n in (2, 3, 5, tn - 1, tn) for q in (1, 2, 7, tq)]
        thin = [(tn, tq), (2, 1)] + thin
        mid = [(tn + 1, tq), (tn, tq + 1), (tn + 1, 1), (2, tq + 1)] + [(n, None) for n in lo if n > tn]
        if form == "thin":
            n, nq = _pick(thin, r)
        elif form == "lds":
            n, nq = _pick(mid, r)
        elif form == "direct":
            n, nq = _pick(hi, r), None
        else:
            n, nq = _pick(mid + [(h, None) for h in hi], r)
        if nq is None:
            nq = int(rng.choice(QUERY_SET))
        B = int(rng.choice(_fit(COLS_SET, min(CAP // n, CAP // nq))))
        return {"n": n, "nq": nq, "B": B}
    if call == "rowpairs":
        tn = L["rowpairs_thin_n"]
        n = _pick((2, 3, 5, tn - 1, tn) if form == "short" else (tn + 1, tn + 2, 255, 257, 9001), r)
        nq = int(rng.choice(QUERY_SET))
        m = int(rng.choice(_fit(COLS_SET, min(CAP // n, CAP // nq))))
        return {"n": n, "nq": nq, "m": m}
    if call == "rows":
        tm = L["rows_thin_m"]
        m = _pick((1, 2, 3, 63, 64, 65, tm - 1) if form == "flat" else (tm, tm + 1, 1023, 1025, 2051), r)
        n = int(rng.choice(_fit(SMALL_NODES, CAP // m)))
        nq = int(rng.choice(_fit(QUERY_SET[form != "flat":], CAP // m)))       # (one output column has no leading dimension to be even)
        return {"n": n, "nq": nq, "m": m}
    if call == "stack":
        tm = L["rows_thin_m"]
        flat = ((1, 1), (1, 2), (3, 1), (7, 9), (8, 8), (5, 13), (15, 17), (1, tm - 1))
        tile = ((16, tm // 16), (tm + 1, 1), (1, tm + 1), (33, 31), (25, 41), (7, 293))
        ny, nx = _pick(flat if form == "flat" else tile, r)
        m = ny * nx
        n = int(rng.choice(_fit(SMALL_NODES, CAP // m)))
        nq = int(rng.choice(_fit(QUERY_SET[form != "flat":], CAP // m)))
        return {"n": n, "nq": nq, "ny": ny, "nx": nx, "m": m}
    if call == "grid":
        t = L["grid_thin_rows"]
        nyi = _pick((1, 2, 7, 8, 9, 63, 65, t - 1) if form == "flat" else (t, t + 1, 511, 513, 2047, 2049, 4100), r)
        nxi = int(rng.choice(_fit(QUERY_SET, CAP // nyi)))
        nx = int(rng.choice(SMALL_NODES + (9001,)))
        ny = int(rng.choice(_fit(SMALL_NODES + (9001,), CAP // nx)))
        return {"nx": nx, "ny": ny, "nxi": nxi, "nyi": nyi}
    if call == "slices2":
        e, t = L["slices_lds_elems"], L["slices_thin_rows"]
        lds = ((2, 2), (3, 5), (31, 33), (32, e // 32), (2, e // 2), (e // 2, 2), (5, 257), (255, 32), (e - 1, 1), (3, 2730))
        lds = [(a, b) for a, b in lds if b >= 2]
        direct = ((3, 2731), (2, e // 2 + 1), (33, 257), (91, 91), (9001, 2), (2, 9001), (e // 2 + 1, 2))
        nx, ny = _pick(lds if form.startswith("lds") else direct, r)
        nyi = _pick((1, 2, 7, 8, 9, 63, 65, t - 1) if form.endswith("flat") else (t, t + 1, 511, 513, 2047), r // 2 + r)
        nxi = int(rng.choice(_fit(QUERY_SET, min(2049, CAP // nyi))))
        S = int(rng.choice(_fit((1, 2, 3, 5, 17), min(CAP // (nx * ny), CAP // (nyi * nxi)))))
        return {"nx": nx, "ny": ny, "nxi": nxi, "nyi": nyi, "S": S}
    raise ValueError(call)


# ---- paired tables --------------------------------------------------------------------------------------------------------

def _make_bad(rng, kind, X, lens, t, n):
    """make table t (a row of X, its fill count in lens) bad in the one way `kind` says"""
    L = int(lens[t])
    x = X[t]
    # the pair (k, k+1), or the node k: a third at the head, a third at the tail (where a staged column is checked by code of
    # its own: the element in front of the first 16-B vector, an odd element behind the last), a third anywhere
    where = int(rng.integers(3))
    k = 0 if where == 0 else L - 2 if where == 1 else int(rng.integers(0, L - 1))
    if kind == "equal":
        x[k + 1] = x[k]
    elif kind == "decreasing":
        x[k], x[k + 1] = x[k + 1], x[k]
    elif kind == "signed_zero":
        x[:L] = x[:L] - x[k]
        x[k], x[k + 1] = -0.0, 0.0
    elif kind == "nan_node":
        x[k + (where == 1)] = np.nan
    elif kind == "inf_last":
        x[L - 1] = np.inf
    elif kind == "minf_first":
        x[0] = -np.inf
    elif kind == "len0":
        lens[t] = 0
    elif kind == "len1":
        lens[t] = 1
    elif kind == "len_n1":
        lens[t] = n + 1
    else:
        raise ValueError(kind)


def _tables(rng, T, n, P, k, special, trap):
    """(X, Y) of T tables, one per ROW of the (T, n) arrays, lens or None, the bad tables {t: kind}, the anchor (a good
    table whose end nodes the shared queries contain), trap planted or not"""
    kinds = [TABLE_KINDS[int(v)] for v in rng.integers(0, len(TABLE_KINDS), T)]
    if n > 2:
        kinds = [("jitter" if kd == "two" else kd) for kd in kinds]
    X = np.empty((T, n))
    for t in range(T):
        x = _unit_axis(rng, kinds[t], n)
        if kinds[t] in ("linspace", "jitter", "clustered", "two"):
            x = rng.uniform(-0.3, 0.3) + rng.uniform(0.5, 1.3) * x
        X[t] = x
    Y = _values(rng, (T, n), special)
    lens = None
    if P["lens"][k]:
        lens = np.full(T, n, dtype=np.int64)
        how = rng.integers(0, 3, T)
        lens[how == 1] = 2
        rnd = how == 2
        lens[rnd] = rng.integers(2, n + 1, int(rnd.sum()))
    bad = {}
    if P["bad"][k] is not None:
        j = P["bad"][k]
        nb = max(1, min(T, -(-T // 10)))
        where = set(int(v) for v in rng.choice(T, nb, replace=False))
        if j % 3 == 0:
            where.add(0)
        if j % 3 == 1:
            where.add(T - 1)
        first = BAD_KINDS.index(BAD_FIRST[j % len(BAD_FIRST)])
        for r, t in enumerate(sorted(where)):
            kind = BAD_KINDS[(first + r) % len(BAD_KINDS)]
            bad[t] = kind
            _make_bad(rng, kind, X, lens, t, n)
    good = [t for t in range(T) if t not in bad]
    anchor = good[int(rng.integers(len(good)))] if good else 0
    planted = False
    if trap and good:
        L = n if lens is None else int(lens[anchor])
        Y[anchor, L - 2], Y[anchor, L - 1] = np.inf, 1.5
        planted = True
    if lens is not None:
        for t in range(T):
            if lens[t] < n:
                X[t, lens[t]:] = np.nan
                Y[t, lens[t]:] = np.nan
    return X, Y, lens, bad, anchor, planted, kinds


def _valid(X, lens, t):
    n = X.shape[1]
    L = n if lens is None else int(lens[t])
    return X[t, :min(max(L, 0), n)]


# ---- the reference --------------------------------------------------------------------------------------------------------

def _ref1_shared(ax, Ycols, q, extrap):
    """oracle on every column of Ycols (n, T) over one shared axis: (nq, T)"""
    import oracle
    if ax["kind"] == "uniform":
        return np.stack([oracle.interp1_uniform(ax["x0"], ax["dx"], Ycols[:, c], q, extrap) for c in range(Ycols.shape[1])], axis=1)
    return np.stack([oracle.interp1_bracket(ax["nodes"], Ycols[:, c], q, extrap) for c in range(Ycols.shape[1])], axis=1)


def _ref1_paired(X, Y, lens, queries, extrap):
    """oracle table by table on the first len nodes; X, Y (T, n), queries(t) the queries of table t: (T, nq) and flags"""
    import oracle
    T, n = X.shape
    nq = queries(0).size
    out = np.full((T, nq), np.nan)
    ok = np.zeros(T, dtype=np.int64)
    for t in range(T):
        L = n if lens is None else int(lens[t])
        if L < 2 or L > n or _is_bad(X[t, :L]):
            continue
        ok[t] = 1
        out[t] = oracle.interp1_bracket(X[t, :L], Y[t, :L], queries(t), extrap)
    return out, ok


def _ref2(ax, ay, Z, xi, yi, extrap):
    """oracle slice by slice: (nyi, nxi, S)"""
    import oracle
    xq, yq = np.repeat(xi, yi.size), np.tile(yi, xi.size)
    out = []
    for s in range(Z.shape[2]):
        if ax["kind"] == "uniform" and ay["kind"] == "uniform":
            z = oracle.interp2_bilinear_uniform(ax["x0"], ax["dx"], ax["nodes"].size, ay["x0"], ay["dx"], ay["nodes"].size,
                                                Z[:, :, s], xq, yq, extrap)
        else:
            z = oracle.interp2_bilinear(ax["nodes"], ay["nodes"], Z[:, :, s], xq, yq, extrap)
        out.append(z.reshape(xi.size, yi.size).T)
    return np.stack(out, axis=2)


# ---- the generator --------------------------------------------------------------------------------------------------------

def _layout2(rng, name, role, rows, cols, S=1, dense_ld=False, want_even=None, base=None):
    """an Operand with drawn base offset and pads; want_even True: base 0 and even ld and stride; False: no constraint"""
    base = int(rng.integers(0, 2)) if base is None else base
    pad = int(rng.choice(PADS))
    spad = int(rng.choice(PADS))
    if want_even:
        base = 0
        if dense_ld:
            spad = _even_pad(rng, rows * cols)
        else:
            pad = _even_pad(rng, rows)
            spad = _even_pad(rng, (rows + pad) * cols)
    if cols == 1 and not dense_ld:
        pad = 0                      # the stride of a single column is not read (api._leading_dim): such a matrix is dense
    if S == 1:
        spad = 0                     # nor that of a single slice
    ld = rows if dense_ld else rows + pad
    return Operand(name, role, rows, cols, S, base, ld, ld * cols + spad)


def _even_pad(rng, count):
    return int(rng.choice([p for p in PADS if (count + p) % 2 == 0]))


def _vec(rng, name, count, role="in", base=None):
    drawn = int(rng.integers(0, 2))
    return Operand(name, role, count, base=drawn if base is None else base)


def case(call, index, seed=SEED):
    """the index-th case of the call; see the module docstring"""
    ci = CALLS.index(call)
    rng = np.random.default_rng([seed, ci, index])
    P = _plan(seed, call, index // CASES_PER_CALL)
    k = index % CASES_PER_CALL
    form, style, special, trap = P["form"][k], P["style"][k], P["special"][k], P["trap"][k]
    extrap = float(EXTRAPS[P["extrap"][k]])
    Z = _sizes(call, form, P["pick"][k], rng)
    meta = {"style": style, "special": special, "sizes": tuple(sorted(Z.items())), "extrap": P["extrap"][k], "trap": False}
    A, axes, ops = {}, {}, {}
    want_ok, use_ok = None, False

    def kind_for(n, which="kind"):
        kd = P[which][k]
        return "two" if n == 2 else ("jitter" if kd == "two" else kd)            # "two" IS n == 2

    if P["kind"][k] == "two":                                    # where n selects no form the kind sets it
        if call in ("rows", "stack"):
            Z["n"] = 2
        elif call == "grid":
            Z["nx"] = 2
        meta["sizes"] = tuple(sorted(Z.items()))

    if call in ("cols", "rows", "stack"):
        n, nq = Z["n"], Z["nq"]
        T = Z["B"] if call == "cols" else Z["m"]
        ax = _shared_axis(rng, kind_for(n), n)
        axes["x"] = ax
        Yt = _values(rng, (n, T), special)                       # one table per column of Yt
        if trap:
            Yt[n - 2, int(rng.integers(T))] = np.inf
            meta["trap"] = True
        xi = _queries(rng, ax["nodes"], nq, style)
        want = _ref1_shared(ax, Yt, xi, extrap)                  # (nq, T)
        A["xi"] = xi
        ops["xi"] = _vec(rng, "xi", nq)
        if call == "cols":
            A["Y"] = Yt
            ops["Y"] = _layout2(rng, "Y", "in", n, T)
            ops["YI"] = _layout2(rng, "YI", "out", nq, T)
            want3, out = want.reshape(nq, T, 1), "YI"
        elif call == "rows":
            A["Y"] = np.ascontiguousarray(Yt.T)                  # (m, n)
            even = True if form == "tile16" else None
            while True:
                ops["Y"] = _layout2(rng, "Y", "in", T, n, want_even=even)
                ops["YI"] = _layout2(rng, "YI", "out", T, nq, want_even=even)
                got = "flat" if T < LIMITS["rows_thin_m"] else (
                    "tile16" if ops["Y"].base == 0 and ops["YI"].base == 0 and (ops["Y"].ld | ops["YI"].ld) % 2 == 0 else "tile8")
                if got == form:
                    break
            want3, out = np.ascontiguousarray(want.T).reshape(T, nq, 1), "YI"
        else:
            ny, nx = Z["ny"], Z["nx"]
            A["Z"] = np.ascontiguousarray(Yt.T).reshape(nx, ny, n).transpose(1, 0, 2).copy()      # row r = i + j*ny
            even = True if form == "tile16" else None
            while True:
                ops["Z"] = _layout2(rng, "Z", "in", ny, nx, n, dense_ld=True, want_even=even)
                ops["ZI"] = _layout2(rng, "ZI", "out", ny, nx, nq, dense_ld=True, want_even=even)
                got = "flat" if T < LIMITS["rows_thin_m"] else (
                    "tile16" if ops["Z"].base == 0 and ops["ZI"].base == 0 and (ops["Z"].stride | ops["ZI"].stride) % 2 == 0 else "tile8")
                if got == form:
                    break
            want3, out = np.ascontiguousarray(want.T).reshape(nx, ny, nq).transpose(1, 0, 2).copy(), "ZI"
        meta["kinds"] = (ax["kind"],)
    elif call in PAIRED:
        n, nq = Z["n"], Z["nq"]
        T = Z["m"] if call == "rowpairs" else Z["B"]
        X, Y, lens, bad, anchor, planted, kinds = _tables(rng, T, n, P, k, special, trap)
        meta.update(trap=planted, bad=tuple(sorted(bad.items())), lens=lens is not None, kinds=tuple(sorted(set(kinds))),
                    bad_first=0 in bad, bad_last=(T - 1) in bad)
        use_ok = bool(P["use_ok"][k])
        shared = call != "each" or P["shared"][k]
        if shared:
            xa = _valid(X, lens, anchor) if anchor not in bad else _unit_axis(rng, "jitter", n)
            xi = _queries(rng, xa, nq, style)
            out_t, ok = _ref1_paired(X, Y, lens, lambda t: xi, extrap)
        else:
            styles = [STYLES[int(v)] for v in rng.integers(0, len(STYLES), T)]
            styles[anchor] = style
            XIt = np.empty((T, nq))
            for t in range(T):
                xt = _valid(X, lens, t)
                if t in bad or xt.size < 2:
                    xt = _unit_axis(rng, "jitter", max(n, 2))
                XIt[t] = _queries(rng, xt, nq, styles[t])
            out_t, ok = _ref1_paired(X, Y, lens, lambda t: XIt[t], extrap)
        want_ok = ok if use_ok else None
        if lens is not None:
            A["lens"] = lens.astype(np.int32)
            ops["lens"] = _vec(rng, "lens", T, base=P["base_lens"][k])
        if call == "rowpairs":
            A["X"], A["Y"] = X, Y
            ops["X"] = _layout2(rng, "X", "in", T, n)
            ops["Y"] = _layout2(rng, "Y", "in", T, n)
            ops["YI"] = _layout2(rng, "YI", "out", T, nq)
            want3 = out_t.reshape(T, nq, 1)
        else:
            A["X"], A["Y"] = np.ascontiguousarray(X.T), np.ascontiguousarray(Y.T)
            ops["X"] = _layout2(rng, "X", "in", n, T)
            ops["Y"] = _layout2(rng, "Y", "in", n, T)
            ops["YI"] = _layout2(rng, "YI", "out", nq, T)
            want3 = np.ascontiguousarray(out_t.T).reshape(nq, T, 1)
        qbase = P["base_q"][k] if call == "each" else None       # (pairs, rowpairs: every case has xi, the stream draws it)
        if shared:
            A["xi"] = xi
            ops["xi"] = _vec(rng, "xi", nq, base=qbase)
        else:
            A["XI"] = np.ascontiguousarray(XIt.T)
            ops["XI"] = _layout2(rng, "XI", "in", nq, T, base=qbase)
        out = "YI"
    else:
        nx, ny, nxi, nyi = Z["nx"], Z["ny"], Z["nxi"], Z["nyi"]
        S = Z.get("S", 1)
        kx = kind_for(nx)
        if call == "grid":
            ky = "uniform" if kx == "uniform" else kind_for(ny, "kind2")
            if ky == "uniform" and kx != "uniform":
                ky = "clustered" if ny > 2 else "two"
        else:
            ky = kind_for(ny, "kind2")
        ax, ay = _shared_axis(rng, kx, nx), _shared_axis(rng, ky, ny)
        axes["ax"], axes["ay"] = ax, ay
        Zc = _values(rng, (ny, nx, S), special)
        if trap:
            s = int(rng.integers(S))
            Zc[:, nx - 2, s] = np.inf
            last = Zc[:, nx - 1, s]
            last[~np.isfinite(last)] = 1.5
            meta["trap"] = True
        xi = _queries(rng, ax["nodes"], nxi, style)
        yi = _queries(rng, ay["nodes"], nyi, P["style2"][k])
        A.update(Z=Zc, xi=xi, yi=yi)
        ops["xi"], ops["yi"] = _vec(rng, "xi", nxi), _vec(rng, "yi", nyi)
        want3 = _ref2(ax, ay, Zc, xi, yi, extrap)
        if call == "grid":
            ops["ZI"] = Operand("ZI", "out", nyi, nxi, 1, int(rng.integers(0, 2)))      # dense, Z itself is a host array
        else:
            ops["Z"] = _layout2(rng, "Z", "in", ny, nx, S)
            ops["ZI"] = _layout2(rng, "ZI", "out", nyi, nxi, S)
        out = "ZI"
        meta["kinds"] = (ax["kind"], ay["kind"])
        meta["style2"] = P["style2"][k]
    counter = None
    if call in COUNTER_CALL:
        counter = FORMS[call].index(form)
    c = Case(call=call, index=index, seed=seed, form=form, counter=counter, arrays=A, axes=axes, ops=ops, out=out, extrap=extrap,
             use_ok=use_ok, want=np.ascontiguousarray(want3, dtype=np.float64), want_ok=want_ok, meta=meta)
    assert c.want.shape == ops[out].shape and predicted_form(c) == form, (c, predicted_form(c))
    return c


def predicted_form(c):
    """the form the library's dispatch takes, from the limits and the layout alone"""
    L, Z = LIMITS, dict(c.meta["sizes"])
    if c.call == "cols":
        return "lds" if Z["n"] <= L["cols_lds_n"] else "direct"
    if c.call == "pairs":
        return "lds" if Z["n"] <= L["pairs_lds_n"] else "direct"
    if c.call == "each":
        if Z["n"] <= L["each_thin_n"] and Z["nq"] <= L["each_thin_q"]:
            return "thin"
        if "xi" in c.ops:
            return "forwarded"
        return "lds" if Z["n"] <= L["pairs_lds_n"] else "direct"
    if c.call == "rowpairs":
        return "short" if Z["n"] <= L["rowpairs_thin_n"] else "long"
    if c.call in ("rows", "stack"):
        if Z["m"] < L["rows_thin_m"]:
            return "flat"
        y, yi = (c.ops["Y"], c.ops["YI"]) if c.call == "rows" else (c.ops["Z"], c.ops["ZI"])
        ld = (y.ld | yi.ld) if c.call == "rows" else (y.stride | yi.stride)
        return "tile16" if y.base == 0 and yi.base == 0 and ld % 2 == 0 else "tile8"
    if c.call == "grid":
        return "flat" if Z["nyi"] < L["grid_thin_rows"] else "tile"
    return ("lds" if Z["nx"] * Z["ny"] <= L["slices_lds_elems"] else "direct") + ("-flat" if Z["nyi"] < L["slices_thin_rows"] else "-tile")


def all_cases(call, seed=SEED):
    return [case(call, i, seed) for i in range(CASES_PER_CALL)]


# ---- canvases -------------------------------------------------------------------------------------------------------------

def canvases(c):
    """{operand name: flat canvas} as the device gets them: float64, lens int32 (its guards hold -1)"""
    out = {}
    for name, op in c.ops.items():
        if name == "lens":
            cv = np.full(op.size, -1, dtype=np.int32)
            cv[op.index().reshape(-1)] = c.arrays["lens"]
        elif op.role == "out":
            cv = np.full(op.size, SENT_GUARD)
            cv[op.index().reshape(-1)] = SENT_FILL
        else:
            cv = np.full(op.size, np.nan)
            cv[op.index()] = np.asarray(c.arrays[name], dtype=np.float64).reshape(op.shape)
        out[name] = cv
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------

def _np_interp1(x, y, q, extrap, pad_node=False):
    """the bracket rule and the two-term blend on one table, in numpy; y may be (n,) or (n, T)"""
    n = x.size
    with np.errstate(all="ignore"):
        l = np.clip(np.searchsorted(x, q, side="right") - 1, 0, n - 1)
        l = np.where(np.isnan(q), 0, l)
        r = np.minimum(l + 1, n - 1)
        if pad_node:
            r = np.where(l == n - 1, n - 2, r)
        a, b = q - x[l], x[r] - q
        w = np.where(a > 0.0, a / (a + b), 0.0)
        if y.ndim == 2:
            w = w[:, None]
        res = (1.0 - w) * y[l] + w * y[r]
        oob = (q < x[0]) | (q > x[-1])
        res[oob] = extrap
        res[np.isnan(q)] = np.nan
    return res


def _np_interp2(xn, yn, Z, xi, yi, extrap, pad_node=False):
    """orc_interp2_bilinear on the (nyi, nxi) query grid of one slice Z (ny, nx), in numpy"""
    nx, ny = xn.size, yn.size
    with np.errstate(all="ignore"):
        lx = np.where(np.isnan(xi), 0, np.clip(np.searchsorted(xn, xi, side="right") - 1, 0, nx - 1))
        ly = np.where(np.isnan(yi), 0, np.clip(np.searchsorted(yn, yi, side="right") - 1, 0, ny - 1))
        rx, ry = np.minimum(lx + 1, nx - 1), np.minimum(ly + 1, ny - 1)
        if pad_node:
            rx = np.where(lx == nx - 1, nx - 2, rx)
        a, b = xi - xn[lx], xn[rx] - xi
        wx = np.where(a > 0.0, a / (a + b), 0.0)[None, :]
        a, b = yi - yn[ly], yn[ry] - yi
        wy = np.where(a > 0.0, a / (a + b), 0.0)[:, None]
        c0 = (1.0 - wy) * Z[np.ix_(ly, lx)] + wy * Z[np.ix_(ry, lx)]
        c1 = (1.0 - wy) * Z[np.ix_(ly, rx)] + wy * Z[np.ix_(ry, rx)]
        res = (1.0 - wx) * c0 + wx * c1
        ox = (xi < xn[0]) | (xi > xn[-1])
        oy = (yi < yn[0]) | (yi > yn[-1])
        res[oy[:, None] | ox[None, :]] = extrap
        res[np.isnan(yi)[:, None] | np.isnan(xi)[None, :]] = np.nan
    return res


def _gather(c, cv, name, shift_last_row=False):
    """operand `name` read out of its canvas; shift_last_row: row `rows` where row rows-1 belongs (a padded ld only)"""
    op = c.ops[name]
    idx = op.index()
    padded = (op.stride > op.rows * op.cols) if c.call == "stack" else (op.ld > op.rows)
    if shift_last_row and padded:
        idx = idx.copy()
        if c.call == "stack":
            idx[-1, -1, :] += 1                                  # row m = ny*nx of the (m, n) matrix whose ld is the slice stride
        else:
            idx[-1, :, :] += 1
    return cv[name][idx]


def _model_out(c, cv, defect):
    """(output of shape ops[out].shape, flags or None) computed from the canvases"""
    pad = defect == "pad_node"
    shift = defect == "reads_padding"
    call = c.call
    e = c.extrap
    if call in ("cols", "rows", "stack"):
        x = c.axes["x"]["nodes"]
        q = _gather(c, cv, "xi")[:, 0, 0]
        if call == "cols":
            Y = _gather(c, cv, "Y", shift)[:, :, 0]
            out = _np_interp1(x, Y, q, e, pad)[:, :, None]
        elif call == "rows":
            Y = _gather(c, cv, "Y", shift)[:, :, 0]
            out = _np_interp1(x, np.ascontiguousarray(Y.T), q, e, pad).T[:, :, None]
        else:
            Zc = _gather(c, cv, "Z", shift)                                  # (ny, nx, n)
            ny, nx, n = Zc.shape
            Yt = Zc.transpose(2, 1, 0).reshape(n, nx * ny)                  # table r = i + j*ny in column r
            out = _np_interp1(x, Yt, q, e, pad).reshape(q.size, nx, ny).transpose(2, 1, 0)
        if defect == "nan_is_extrap":
            out = np.array(out)
            nanq = np.isnan(q)
            if call == "cols":
                out[nanq, :, :] = e
            elif call == "rows":
                out[:, nanq, :] = e
            else:
                out[:, :, nanq] = e
        return np.ascontiguousarray(out), None
    if call in PAIRED:
        byrow = call == "rowpairs"
        X = _gather(c, cv, "X", shift)[:, :, 0]
        Y = _gather(c, cv, "Y", shift)[:, :, 0]
        if not byrow:
            X, Y = X.T, Y.T
        T, n = X.shape
        lens = None
        if "lens" in c.ops and defect != "ignores_len":
            lens = cv["lens"][c.ops["lens"].index()[:, 0, 0]].astype(np.int64)
        if "xi" in c.ops:
            xi = _gather(c, cv, "xi")[:, 0, 0]
            qs = lambda t: xi
            nq = xi.size
        else:
            XI = _gather(c, cv, "XI", shift)[:, :, 0]
            qs = lambda t: XI[:, t]
            nq = XI.shape[0]
        out = np.full((T, nq), np.nan)
        ok = np.zeros(T, dtype=np.int64)
        for t in range(T):
            L = n if lens is None else int(lens[t])
            if L < 2 or L > n:
                continue
            x = X[t, :L]
            if _is_bad(x):
                sz = defect == "signed_zero_ok" and np.all(np.isfinite(x)) and np.all(
                    (x[:-1] < x[1:]) | ((x[:-1] == 0.0) & (x[1:] == 0.0) & np.signbit(x[:-1]) & ~np.signbit(x[1:])))
                if not sz:
                    continue
            ok[t] = 1
            q = qs(t)
            out[t] = _np_interp1(x, Y[t, :L], q, e, pad and L >= 2)
            if defect == "nan_is_extrap":
                out[t, np.isnan(q)] = e
        out3 = (out if byrow else np.ascontiguousarray(out.T))[:, :, None]
        return np.ascontiguousarray(out3), (ok if c.use_ok else None)
    xn, yn = c.axes["ax"]["nodes"], c.axes["ay"]["nodes"]
    xi, yi = _gather(c, cv, "xi")[:, 0, 0], _gather(c, cv, "yi")[:, 0, 0]
    Zc = c.arrays["Z"] if call == "grid" else _gather(c, cv, "Z", shift)
    out = np.stack([_np_interp2(xn, yn, Zc[:, :, s], xi, yi, e, pad) for s in range(Zc.shape[2])], axis=2)
    if defect == "nan_is_extrap":
        out[np.isnan(yi)[:, None] | np.isnan(xi)[None, :], :] = e
    return out, None


def precondition(c, defect):
    """the structural half of "applies": PRECONDITION[defect]"""
    if defect in ("pad_node", "stray_store"):
        return True
    if defect == "ignores_len":
        return c.call in PAIRED and "lens" in c.arrays and bool(np.any(c.arrays["lens"] < dict(c.meta["sizes"])["n"]))
    if defect == "reads_padding":
        if c.call == "grid":
            return False
        ins = [o for o in c.ops.values() if o.role == "in" and o.name in ("X", "Y", "XI", "Z")]
        return any((o.stride > o.rows * o.cols) if c.call == "stack" else (o.ld > o.rows) for o in ins)
    if defect == "signed_zero_ok":
        return c.call in PAIRED and any(kind == "signed_zero" for _, kind in c.meta["bad"])
    if defect == "nan_is_extrap":
        return not np.isnan(c.extrap)
    if defect == "wrong_form":
        return c.counter is not None
    raise ValueError(defect)


def _counters(c, wrong=False):
    if c.counter is None:
        return None, None
    nforms = COUNTERS[COUNTER_CALL[c.call]][1]
    before = [7 + f for f in range(nforms)]
    after = list(before)
    after[(c.counter + 1) % nforms if wrong else c.counter] += 1
    return before, after


def model_call(c, defect=None):
    """a numpy stand-in for the device call, defect one of DEFECTS or None: (canvases after, flags, counters before, counters
    after), the arguments of check() after the case"""
    assert defect is None or defect in DEFECTS
    cv = canvases(c)
    out, ok = _model_out(c, cv, defect if defect in ("pad_node", "ignores_len", "reads_padding", "signed_zero_ok", "nan_is_extrap") else None)
    after = {name: a.copy() for name, a in cv.items()}
    op = c.ops[c.out]
    idx = op.index()
    after[c.out][idx] = out
    if defect == "stray_store":
        after[c.out][int(idx.max()) + 1] = out.reshape(-1)[-1] if np.isfinite(out.reshape(-1)[-1]) else 1.0
    before, cafter = _counters(c, wrong=defect == "wrong_form")
    return after, ok, before, cafter


def applies(c, defect):
    """precondition(c, defect) and the defect changes at least one bit of what the call returns on this case"""
    if not precondition(c, defect):
        return False
    if defect in ("stray_store", "wrong_form"):
        return True
    cv = canvases(c)
    a, oka = _model_out(c, cv, None)
    b, okb = _model_out(c, cv, defect)
    return not (bool(np.all(_same(a, b))) and (oka is None or np.array_equal(oka, okb)))


# ---- the check ------------------------------------------------------------------------------------------------------------

def _first_bad(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def check(c, canvases_after, flags, counters_before, counters_after):
    """The one check.  canvases_after: {operand name: flat canvas read back after the call}, the output's at least (an input's,
    if given, must be as it was uploaded); flags: col_ok / row_ok or None; counters_*: the values of the call's form
    counters before and after it (None for a call without them).  AssertionError names (call, index) and the first bad
    element with both values."""
    tag = "(%s, %d) [%s]" % (c.call, c.index, c.form)
    op = c.ops[c.out]
    got = np.asarray(canvases_after[c.out], dtype=np.float64)
    assert got.shape == (op.size,), "%s: the output canvas has %s elements, not %d" % (tag, got.shape, op.size)
    idx = op.index()
    vals = got[idx]
    unwritten = vals.view(np.uint64) == np.array(SENT_FILL).view(np.uint64)
    if unwritten.any():
        at = _first_bad(unwritten)
        raise AssertionError("%s: output element %s was not written (it still holds the pre-fill %r; %r expected)" % (tag, at, SENT_FILL, c.want[at]))
    if not same_bits(vals, c.want):                              # any NaN equals any NaN, signed zeros are distinct
        wrong = ~_same(vals, c.want)
        at = _first_bad(wrong)
        raise AssertionError("%s: output element %s is %r (%s), the oracle says %r (%s); %d of %d elements differ" % (
            tag, at, vals[at], vals[at].tobytes().hex(), c.want[at], c.want[at].tobytes().hex(), int(wrong.sum()), wrong.size))
    rest = np.ones(op.size, dtype=bool)
    rest[idx.reshape(-1)] = False
    hurt = rest & (got.view(np.uint64) != np.array(SENT_GUARD).view(np.uint64))
    if hurt.any():
        at = int(np.argmax(hurt))
        raise AssertionError("%s: element %d of the output canvas (%d behind the operand's first element, outside its logical "
                             "elements) holds %r, not the sentinel %r: a stray store; %d disturbed" % (
                                 tag, at, at - op.start, got[at], SENT_GUARD, int(hurt.sum())))
    first = canvases(c)
    for name, a in canvases_after.items():
        if name != c.out:
            same = np.array_equal(a, first[name]) if name == "lens" else bool(np.all(_same(np.asarray(a, dtype=np.float64), first[name])))
            assert same, "%s: the input canvas %s changed during the call" % (tag, name)
    if c.want_ok is None:
        assert flags is None, "%s: flags came back from a call made without want_ok" % tag
    else:
        assert flags is not None, "%s: no flags came back" % tag
        f = np.asarray(flags).astype(np.int64).reshape(-1)
        assert f.shape == c.want_ok.shape, "%s: %d flags for %d tables" % (tag, f.size, c.want_ok.size)
        if not np.array_equal(f, c.want_ok):
            at = int(np.argmax(f != c.want_ok))
            raise AssertionError("%s: flag of table %d is %d, %d expected" % (tag, at, f[at], c.want_ok[at]))
    if c.counter is not None:
        assert counters_before is not None and counters_after is not None, "%s: no form counters given" % tag
        delta = [int(a) - int(b) for a, b in zip(counters_after, counters_before)]
        expect = [int(f == c.counter) for f in range(len(delta))]
        assert delta == expect, "%s: the form counters moved by %s, %s expected (form %s)" % (tag, delta, expect, c.form)


# ---- the census -----------------------------------------------------------------------------------------------------------

def census(call, cases=None):
    """what the 48 cases of a call cover, as counts: the CPU test asserts on it and prints it"""
    cases = cases or all_cases(call)
    cen = {"forms": {}, "kinds": {}, "styles": {}, "extrap": {}, "base": {}, "out_ld": {"odd": 0, "even": 0}, "sizes": {},
           "bad": {}, "lens": {True: 0, False: 0}, "use_ok": {True: 0, False: 0}, "bad_use_ok": {True: 0, False: 0},
           "bad_first": 0, "bad_last": 0, "trap": 0, "special": 0, "max_table": 0, "max_out": 0}

    def bump(d, key):
        d[key] = d.get(key, 0) + 1

    for c in cases:
        bump(cen["forms"], c.form)
        for kd in c.meta["kinds"]:
            bump(cen["kinds"], kd)
        bump(cen["styles"], c.meta["style"])
        if "style2" in c.meta:
            bump(cen["styles"], c.meta["style2"])
        bump(cen["extrap"], c.meta["extrap"])
        for name, op in c.ops.items():
            bump(cen["base"], (name, op.base))
        o = c.ops[c.out]
        cen["out_ld"]["odd" if (o.stride if c.call == "stack" else o.ld) % 2 else "even"] += 1
        for name, v in c.meta["sizes"]:
            cen["sizes"].setdefault(name, set()).add(v)
        if c.call in ("grid", "slices2"):
            Z = dict(c.meta["sizes"])
            cen["sizes"].setdefault("nx*ny", set()).add(Z["nx"] * Z["ny"])
        cen["trap"] += bool(c.meta["trap"])
        cen["special"] += bool(c.meta["special"])
        if c.call in PAIRED:
            cen["lens"][c.meta["lens"]] += 1
            cen["use_ok"][c.use_ok] += 1
            for _, kind in c.meta["bad"]:
                bump(cen["bad"], kind)
            if c.meta["bad"]:
                cen["bad_use_ok"][c.use_ok] += 1
            cen["bad_first"] += c.meta["bad_first"]
            cen["bad_last"] += c.meta["bad_last"]
        tab = max(int(np.asarray(c.arrays[nm]).size) for nm in ("Y", "Z", "X") if nm in c.arrays)
        cen["max_table"] = max(cen["max_table"], tab)
        cen["max_out"] = max(cen["max_out"], int(c.want.size))
    return cen


# the limit each call's sizes have to hit exactly and at +1: {call: [(name in LIMITS, name in census()["sizes"])]}
LIMIT_SIZES = {
    "cols": [("cols_lds_n", "n")], "pairs": [("pairs_lds_n", "n")],
    "each": [("pairs_lds_n", "n"), ("each_thin_n", "n"), ("each_thin_q", "nq")],
    "rows": [("rows_thin_m", "m")], "stack": [("rows_thin_m", "m")], "rowpairs": [("rowpairs_thin_n", "n")],
    "grid": [("grid_thin_rows", "nyi")], "slices2": [("slices_lds_elems", "nx*ny"), ("slices_thin_rows", "nyi")],
}
