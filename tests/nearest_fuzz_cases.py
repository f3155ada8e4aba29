"""Seeded differential fuzz of the two "nearest" device calls: the generator, the reference and a numpy model with planted
defects.  Plain numpy, nearest_cases and (through batched_fuzz_cases) the CPU oracle: no torch, no GPU.  The layout
classes, the guarded canvases, the axis / value / query generators and the one checking function are batched_fuzz_cases'
(F below) and are used as they are; tests/test_nearest_fuzz_cases_cpu.py proves the census and that F.check() refuses every
planted defect; tests/test_nearest_fuzz_gpu.py and scripts/gpu_fuzz_nearest.py run the cases on the device.

    call           C entry point                     Python                      forms (counter of mi_debug_nearest_launches)
    cols_nearest   mi_interp1_cols_nearest_f64_dev   Axis1.interp_cols_nearest   lds-vec / lds-8 (3), direct-vec / direct-8 (4)
    table_nearest  mi_interp1_nearest_f64_dev        Grid1.interp_nearest        stream-full / stream-part (0), scalar (2)

case(call, index) is one fully determined case, by F.case's discipline: its random source is
default_rng([seed, CALL_INDEX[call], index]) and nothing else, the evenly covered attributes (form, form-selecting size,
axis kind, query style, extrap, special values, the pad_node trap) come from a plan per block of CASES_PER_CALL indices drawn
from default_rng([seed, CALL_INDEX[call], 10**6 + block]), a draw that degenerates is drawn again from the same stream,
and no case is dropped.

cols_nearest: the operands of F's "cols" -- Y strided (n, B), xi, YI strided (nq, B).  LDS form iff n <= COLS_LDS_N;
16-B stores ("vec") iff YI has base offset 0 and an even leading dimension, else 8-B stores.  A one-column YI has the
leading dimension nq (the stride of a single column is not read), so a vec case never draws B = 1 with an odd nq: sizes
and layouts are drawn together until the predicted form is the planned one.

table_nearest: one resident Grid1 (case.axes["x"], case.arrays["Y"]: no canvas, the handle owns a copy), xq and yq vectors.
stream-full: both base offsets 0 and nq >= STREAM_BLOCK + 1 (full blocks through the WIN = true path and a partial one);
stream-part: both 0 and nq < STREAM_BLOCK (partial blocks only, the lazy load of node G-1 in mode 3); scalar: either base
offset 1, every nq.  Table kinds: F.AXIS_KINDS ("uniform" through Grid1.uniform) and the sweep_cases families of FAMILY_N.
The library chooses the table mode from the abscissae; FAMILY_N holds, per family, the sizes at which
csrc/mi_interp1_tables.hip's detection gives the family's form of sweep_cases.TABLE_SPECS (cf_div is form 0 wherever n-1
is a power of two; cf_mul_pinned keeps form 1 only where the pinned span divided by n-1 still rounds to the step), and
the GPU test asserts what the library reports.

Queries: F._queries' (its mandatory points: both end nodes, NaN, a point on each side, +-inf) and, in every case with
room, EXTRA more: the midpoint of the last cell with its two ulp neighbours (the pinned last node and the padding node
behind the table are judged there) and one midpoint of an interior cell, an exact tie (q - X[l] == X[r] - q) where the
axis has one.  In a third of the cases Y[n-2] = +inf and Y[n-1] = 1.5 are planted, as F does for pad_node.

The reference is nearest_cases.rule_index / _gather (nearest_rule column by column); on a uniform axis the nodes are the
x0 + i*dx that F._shared_axis makes exact.  model_call() is a numpy stand-in that computes bracket and select itself
from the canvases; DEFECTS can be planted in it, and applies() is F's notion: the precondition holds and the defect
changes a bit of the result."""
import functools

import numpy as np

import batched_fuzz_cases as F
import nearest_cases as nc
import sweep_cases as sc
from batched_fuzz_cases import (AXIS_KINDS, EXTRAPS, SEED, SPECIALS, STYLES, Case, Operand, _balanced, _layout2, _queries,  # noqa: F401
                                _shared_axis, _unit_axis, _values, _vec, canvases, check)

CALLS = ("cols_nearest", "table_nearest")
CALL_INDEX = {call: len(F.CALLS) + k for k, call in enumerate(CALLS)}      # behind F's calls: streams of their own
CASES_PER_CALL = 48
COUNTER_NAME, NCOUNTERS = "mi_debug_nearest_launches", 5
STREAM, TABLE_LDS, SCALAR, COLS_LDS, COLS_DIRECT = range(5)
COLS_LDS_N = 8192                  # csrc/mi_nearest1.hip kLdsMaxN
STREAM_BLOCK = 1024                # queries of one workgroup of the streaming kernel: kBlock * kVecVpl * 2
FORMS = {"cols_nearest": ("lds-vec", "lds-8", "direct-vec", "direct-8"), "table_nearest": ("stream-full", "stream-part", "scalar")}
FORM_COUNTER = {"lds-vec": COLS_LDS, "lds-8": COLS_LDS, "direct-vec": COLS_DIRECT, "direct-8": COLS_DIRECT,
                "stream-full": STREAM, "stream-part": STREAM, "scalar": SCALAR}
TABLE_N = (2, 3, 5, 31, 33, 255, 257, 8191, 8192, 9001)
TABLE_NQ = (1, 2, 3, 7, 1023, 1024, 1025, 2047, 2049, 4100)
FAMILY_N = {
    "cf_fma": (3, 5, 31, 33, 255, 257, 8191, 8192, 9001),
    "cf_mul": (5, 31, 33, 255, 257, 8191, 8192, 9001),
    "cf_mul_pinned": (7, 25, 47, 213, 425, 3413),
    "cf_fma_pinned": (5, 31, 33, 255, 257, 8191, 8192, 9001),
    "cf_div": (31, 255, 8191, 8192, 9001),
    "walk": (5, 31, 33, 255, 257, 8191, 8192, 9001),
}
TABLE_KINDS = AXIS_KINDS + tuple(FAMILY_N)
KINDS = {"cols_nearest": AXIS_KINDS, "table_nearest": TABLE_KINDS}
EXTRA = 4                          # queries added to F._queries': see the module docstring
DEFECTS = ("tie_right", "left_always", "blends", "pad_node", "nan_is_extrap", "reads_padding", "stray_store", "wrong_form")
PRECONDITION = {
    "tie_right": "both calls; observable where a query is an exact tie between two different nodes (b <= a takes the right one)",
    "left_always": "both calls; observable where the right node is nearer",
    "blends": "both calls; observable wherever the two-term linear blend is not the nearest value",
    "pad_node": "both calls; observable where the last node is queried (l = n-1 takes Y[n-2])",
    "nan_is_extrap": "both calls: extrap is not NaN and a query is NaN",
    "reads_padding": "cols_nearest: Y has a padded leading dimension (the last row is read one element low)",
    "stray_store": "both calls, every case",
    "wrong_form": "both calls, every case",
}
CAN_APPLY = {d: (("cols_nearest",) if d == "reads_padding" else CALLS) for d in DEFECTS}


# ---- the plan -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _plan(seed, call, block):
    """the balanced attributes of the CASES_PER_CALL cases of one block: a dict of lists"""
    rng = np.random.default_rng([seed, CALL_INDEX[call], 10**6 + block])
    N = CASES_PER_CALL
    forms = FORMS[call]
    off = int(rng.integers(len(forms)))
    P = {"form": [forms[(k + off) % len(forms)] for k in range(N)],
         "kind": _balanced(rng, KINDS[call], N), "style": _balanced(rng, STYLES, N),
         "extrap": _balanced(rng, range(len(EXTRAPS)), N), "special": _balanced(rng, (True, False, False), N),
         "trap": _balanced(rng, (True, False, False), N)}
    # the k-th case of a form takes the k-th of that form's size candidates, shuffled: every candidate comes round
    P["pick"] = [0] * N
    for f in forms:
        mine = [k for k in range(N) if P["form"][k] == f]
        for r, k in zip(rng.permutation(len(mine)), mine):
            P["pick"][k] = int(r)
    return P


def _extra_queries(rng, x):
    """the EXTRA queries of the module docstring on the axis x"""
    n = x.size
    last = 0.5 * x[n - 2] + 0.5 * x[n - 1]
    m = 0.5 * x[:-2] + 0.5 * x[1:-1]                             # the interior cells 0 .. n-3 (none for n == 2)
    if m.size:
        tie = np.flatnonzero((m - x[:-2] == x[1:-1] - m) & (x[:-2] < m) & (m < x[1:-1]))
        pool = tie if tie.size else np.arange(m.size)
        inner = m[pool[int(rng.integers(pool.size))]]
    else:
        inner = last
    return np.array([last, np.nextafter(last, -np.inf), np.nextafter(last, np.inf), inner])


def _all_queries(rng, x, count, style):
    """F._queries on count - k queries and k of the extra ones put in between them, k = what is left of EXTRA behind the
    seven mandatory points"""
    k = min(EXTRA, max(count - 7, 0))
    q = _queries(rng, x, count - k, style)
    extra = _extra_queries(rng, x)[:k]
    return np.insert(q, np.sort(rng.integers(0, q.size + 1, k)), extra) if k else q


def predicted_form(c):
    """the form the library's dispatch takes, from the limits and the layout alone"""
    Z = dict(c.meta["sizes"])
    if c.call == "cols_nearest":
        yi = c.ops["YI"]
        return ("lds" if Z["n"] <= COLS_LDS_N else "direct") + ("-vec" if yi.base == 0 and yi.ld % 2 == 0 else "-8")
    if c.ops["xq"].base or c.ops["yq"].base:
        return "scalar"
    return "stream-full" if Z["nq"] > STREAM_BLOCK else ("stream-part" if Z["nq"] < STREAM_BLOCK else "stream-1024")


def case(call, index, seed=SEED):
    """the index-th case of the call; see the module docstring"""
    rng = np.random.default_rng([seed, CALL_INDEX[call], index])
    P = _plan(seed, call, index // CASES_PER_CALL)
    k = index % CASES_PER_CALL
    form, style, special, trap, r = P["form"][k], P["style"][k], P["special"][k], P["trap"][k], P["pick"][k]
    extrap = float(EXTRAPS[P["extrap"][k]])
    kind = P["kind"][k]
    A, ops = {}, {}
    if call == "cols_nearest":
        lo, hi = F._node_sets(COLS_LDS_N)
        n = F._pick(lo if form.startswith("lds") else hi, r)
        kind = "two" if n == 2 else ("jitter" if kind == "two" else kind)       # "two" IS n == 2
        ax = _shared_axis(rng, kind, n)
        while True:                                              # sizes and layouts together: see the module docstring
            nq = int(rng.choice(F.QUERY_SET))
            B = int(rng.choice(F._fit(F.COLS_SET, min(F.CAP // n, F.CAP // nq))))
            ops["Y"] = _layout2(rng, "Y", "in", n, B)
            ops["xi"] = _vec(rng, "xi", nq)
            ops["YI"] = _layout2(rng, "YI", "out", nq, B, want_even=True if form.endswith("vec") else None)
            if (ops["YI"].base == 0 and ops["YI"].ld % 2 == 0) == form.endswith("vec"):
                break
        Y = _values(rng, (n, B), special)
        if trap:
            col = int(rng.integers(B))
            Y[n - 2, col], Y[n - 1, col] = np.inf, 1.5
        q = _all_queries(rng, ax["nodes"], nq, style)
        A["Y"], A["xi"] = Y, q
        pick = nc.rule_index(ax["nodes"], q)
        want = np.stack([nc._gather(Y[:, c], pick, extrap) for c in range(B)], axis=1).reshape(nq, B, 1)
        sizes, out = {"n": n, "nq": nq, "B": B}, "YI"
        meta = {"store": 16 if form.endswith("vec") else 8}
    elif call == "table_nearest":
        nq = F._pick({"stream-full": (1025, 2047, 2049, 4100), "stream-part": (1, 2, 3, 7, 1023), "scalar": TABLE_NQ}[form], r)
        if kind in FAMILY_N:
            n = int(rng.choice(FAMILY_N[kind]))
            nodes = sc.make_nodes(kind, n)
            ax = {"kind": kind, "nodes": nodes}
        else:
            n = 2 if kind == "two" else int(rng.choice(TABLE_N))
            kind = "two" if n == 2 else kind
            ax = _shared_axis(rng, kind, n)
        base = (0, 0) if form != "scalar" else ((1, 0), (0, 1), (1, 1))[int(rng.integers(3))]
        ops["xq"] = _vec(rng, "xq", nq, base=base[0])
        ops["yq"] = _vec(rng, "yq", nq, role="out", base=base[1])
        Y = _values(rng, n, special)
        if trap:
            Y[n - 2], Y[n - 1] = np.inf, 1.5
        q = _all_queries(rng, ax["nodes"], nq, style)
        A["Y"], A["xq"] = Y, q
        pick = nc.rule_index(ax["nodes"], q)
        want = nc._gather(Y, pick, extrap).reshape(nq, 1, 1)
        sizes, out = {"n": n, "nq": nq}, "yq"
        meta = {"implicit": kind == "uniform"}
    else:
        raise ValueError(call)
    inr = pick >= 0
    l = np.searchsorted(ax["nodes"], q[inr], side="right") - 1
    rr = np.minimum(l + 1, n - 1)
    with np.errstate(all="ignore"):
        ties = int(np.sum((rr > l) & (q[inr] - ax["nodes"][l] == ax["nodes"][rr] - q[inr])))
    meta.update(style=style, special=special, trap=bool(trap), extrap=P["extrap"][k], sizes=tuple(sorted(sizes.items())),
                kinds=(ax["kind"],), ties=ties, in_range=int(inr.sum()), right=int(np.sum(pick[inr] > l)))
    c = Case(call=call, index=index, seed=seed, form=form, counter=FORM_COUNTER[form], arrays=A, axes={"x": ax}, ops=ops, out=out,
             extrap=extrap, use_ok=False, want=np.ascontiguousarray(want, dtype=np.float64), want_ok=None, meta=meta)
    assert c.want.shape == ops[out].shape and predicted_form(c) == form, (c, predicted_form(c))
    return c


def all_cases(call, seed=SEED):
    return [case(call, i, seed) for i in range(CASES_PER_CALL)]


# ---- the model ------------------------------------------------------------------------------------------------------------

def _np_nearest(x, y, q, extrap, defect):
    """bracket, select and copy on one axis, in numpy; y (n,) or (n, B)"""
    n = x.size
    with np.errstate(all="ignore"):
        l = np.clip(np.searchsorted(x, q, side="right") - 1, 0, n - 1)
        l = np.where(np.isnan(q), 0, l)
        r = np.minimum(l + 1, n - 1)
        a, b = q - x[l], x[r] - q
        k = np.where((b <= a) if defect == "tie_right" else (b < a), r, l)
        if defect == "left_always":
            k = l
        if defect == "pad_node":
            k = np.where(l == n - 1, n - 2, k)
        res = np.array(y[k])
        if defect == "blends":
            w = np.where(a > 0.0, a / (a + b), 0.0)
            if y.ndim == 2:
                w = w[:, None]
            res = (1.0 - w) * y[l] + w * y[r]
        res[(q < x[0]) | (q > x[-1])] = extrap
        res[np.isnan(q)] = extrap if defect == "nan_is_extrap" else np.nan
    return res


def _model_out(c, cv, defect):
    x = c.axes["x"]["nodes"]
    if c.call == "cols_nearest":
        op = c.ops["Y"]
        idx = op.index()
        if defect == "reads_padding" and op.ld > op.rows:
            idx = idx.copy()
            idx[-1, :, :] += 1
        q = cv["xi"][c.ops["xi"].index()[:, 0, 0]]
        return _np_nearest(x, cv["Y"][idx][:, :, 0], q, c.extrap, defect)[:, :, None]
    q = cv["xq"][c.ops["xq"].index()[:, 0, 0]]
    return _np_nearest(x, np.asarray(c.arrays["Y"], dtype=np.float64), q, c.extrap, defect)[:, None, None]


def precondition(c, defect):
    """the structural half of "applies": PRECONDITION[defect]"""
    if defect == "nan_is_extrap":
        return not np.isnan(c.extrap)
    if defect == "reads_padding":
        return c.call == "cols_nearest" and c.ops["Y"].ld > c.ops["Y"].rows
    if defect in DEFECTS:
        return True
    raise ValueError(defect)


def model_call(c, defect=None):
    """a numpy stand-in for the device call, defect one of DEFECTS or None: (canvases after, None, counters before, counters
    after), the arguments of F.check() after the case"""
    assert defect is None or defect in DEFECTS
    cv = canvases(c)
    out = _model_out(c, cv, None if defect in ("stray_store", "wrong_form") else defect)
    after = {name: a.copy() for name, a in cv.items()}
    idx = c.ops[c.out].index()
    after[c.out][idx] = out
    if defect == "stray_store":
        last = out.reshape(-1)[-1]
        after[c.out][int(idx.max()) + 1] = last if np.isfinite(last) else 1.0
    before = [11 + f for f in range(NCOUNTERS)]
    cafter = list(before)
    cafter[(c.counter + 1) % NCOUNTERS if defect == "wrong_form" else c.counter] += 1
    return after, None, before, cafter


def applies(c, defect):
    """precondition(c, defect) and the defect changes at least one bit of what the call returns on this case"""
    if not precondition(c, defect):
        return False
    if defect in ("stray_store", "wrong_form"):
        return True
    cv = canvases(c)
    return not bool(np.all(F._same(_model_out(c, cv, None), _model_out(c, cv, defect))))


# ---- the census -----------------------------------------------------------------------------------------------------------

def census(call, cases=None):
    """what the 48 cases of a call cover, as counts: the CPU test asserts on it and prints it"""
    cases = cases or all_cases(call)
    cen = {"forms": {}, "kinds": {}, "styles": {}, "extrap": {}, "base": {}, "n": set(), "nq": set(), "tie_cases": 0, "ties": 0,
           "trap": 0, "special": 0, "in_range": 0, "right": 0, "max_table": 0, "max_out": 0, "y_pad": {}}

    def bump(d, key):
        d[key] = d.get(key, 0) + 1

    for c in cases:
        Z = dict(c.meta["sizes"])
        bump(cen["forms"], c.form)
        bump(cen["kinds"], c.meta["kinds"][0])
        bump(cen["styles"], c.meta["style"])
        bump(cen["extrap"], c.meta["extrap"])
        for name, op in c.ops.items():
            bump(cen["base"], (name, op.base))
        if "Y" in c.ops:
            bump(cen["y_pad"], c.ops["Y"].ld - c.ops["Y"].rows)
        cen["n"].add(Z["n"])
        cen["nq"].add(Z["nq"])
        cen["tie_cases"] += c.meta["ties"] > 0
        cen["ties"] += c.meta["ties"]
        cen["trap"] += c.meta["trap"]
        cen["special"] += bool(c.meta["special"])
        if Z["nq"] >= 255:
            cen["in_range"] += c.meta["in_range"]
            cen["right"] += c.meta["right"]
        cen["max_table"] = max(cen["max_table"], int(np.asarray(c.arrays["Y"]).size))
        cen["max_out"] = max(cen["max_out"], int(c.want.size))
    return cen
