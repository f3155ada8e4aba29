"""Shared cases for the strided entry points at element offsets beyond 2^32: mi_interp1_cols_f64_dev,
mi_interp1_pairs_f64_dev, mi_interp1_each_f64_dev, mi_interp1_rows_f64_dev, mi_interp1_rowpairs_f64_dev and
mi_interp2_slices_f64_dev take leading dimensions and slice strides as size_t and promise 64-bit addressing; a case
makes ONE strided operand of one call "wide" -- its last column or slice lies more than 2^32 elements behind its first
-- while the work stays a few kilobytes.  Plain numpy plus the CPU oracle: no torch, no GPU.
tests/test_wide_stride_cases_cpu.py proves the construction, tests/test_wide_strides_gpu.py runs it on the device.

The pool.  The GPU test owns one allocation of POOL = 3*2^31 + 2^22 doubles and never fills it as a whole.  A wide
operand is a strided view whose first element sits BASE = 2^31 (+1 for the 8-B aligned variants) elements into it.  A
kernel that forms an element offset D from the operand's base in 32 bits reaches one of
    D mod 2^32                 u32        an unsigned element index
    int32(D)                   s32        a signed one, sign-extended: as far as -2^31
    (8 D mod 2^32) / 8         byte_u32   an unsigned byte offset
    int32(8 D) / 8             byte_s32   a signed one: as far as -2^28
instead of D, all of them in [-2^31, 2^32): with BASE = 2^31 every one of them, and D itself (< 2^32 + 2^22), is an
address inside the pool.  A truncation is a wrong value or a disturbed sentinel, never an access outside the allocation.

Blocks.  A wide leading dimension makes every column of the operand a block (rows contiguous elements at D = j*ld); a
wide slice stride makes every slice a block (its whole matrix, padding rows included, at D = s*stride).  The stride is
2^32/(count-1), rounded up, plus a pad larger than two blocks and their guards, so that the last block lies just beyond
2^32 and no alias of one block touches another block.  (A pad of 2, i.e. ld = 2^32 + 2, would lay the u32 alias of column
1 over column 0: nothing could then be planted there.)  With more than two blocks the middle ones fall in [2^31, 2^32).

What is planted (plant): in an INPUT operand every block holds its true data and every alias of it (the four misreadings
above, minus D itself) a decoy: the true data + 3 + the alias's rank, finite, plausible, different; padding rows of a
padded slice hold NaN.  In an OUTPUT operand every alias window and GUARD elements before and after every true block hold
SENT_GUARD, as do the padding rows, and the true elements are pre-filled with SENT_FILL, so "written" is proven too.

check() is the one checking function of both tests: results equal the oracle bit for bit (NaN == NaN, signed zeros
distinct), every planted window but the true output elements is as it was planted, the true output elements are all
overwritten, col_ok / row_ok are right and the form counter moved by one in the expected form.  model_call() is a numpy
stand-in for the device call that forms its addresses through one of ADDRESS: the CPU test holds check() to pass the
exact one and to fail each of the other four on every case.

Data.  Axes run from exactly 1.0 to exactly 2.0 (every column / row of a paired call too, so that the shared queries are
in range for all of them) with jittered interior nodes; values are seeded normals.  Queries (queries()): both end nodes,
the midpoints of the first and of the last cell, an interior node, its ulp neighbours, NaN, one point below and one
above the range, then seeded uniform points; the last cell and the last node are the brackets that read the far columns of
the row-type calls.  The thin form of interp1_each takes 8 queries per column at most: its first column leaves the node and
its -1 ulp neighbour out, its far column the node and the first cell's midpoint.  Where a case gives `len`, column / row 0 is
one node short (its own axis still ends at 2.0; the node left out holds NaN) and, with three or more of them, number 1
is bad (its first two nodes are equal): all its outputs are NaN and its flag is 0.
"""
import functools

import numpy as np

POOL = 3 * 2**31 + 2**22          # elements of the GPU test's one allocation
BASE = 2**31                      # element index of a wide operand's first element (+1: 8-B aligned only)
GUARD = 64                        # sentinel elements before and after every true output block
SENT_GUARD = -12345.678           # alias windows, guards and padding rows of an output
SENT_FILL = 98765.4321            # pre-filled into the true elements of an output
EXTRAP = -7.25
FLAGGED_PER_TABLE = 3             # planted per output column / row / slice column: NaN, below, above

_W32 = 2**32


def _sext32(v):
    v &= _W32 - 1
    return v - _W32 if v >= 2**31 else v


ADDRESS = {
    "exact": lambda D: D,
    "u32": lambda D: D % _W32,
    "s32": _sext32,
    "byte_u32": lambda D: ((8 * D) % _W32) // 8,
    "byte_s32": lambda D: _sext32(8 * D) // 8,
}
WRONG = [k for k in ADDRESS if k != "exact"]


def aliases(D):
    """the misreadings of offset D that differ from it, in ADDRESS's order: [(name, offset)], equal offsets once"""
    out, seen = [], {D}
    for name in WRONG:
        a = ADDRESS[name](D)
        if a not in seen:
            seen.add(a)
            out.append((name, a))
    return out


def same_bits(a, b):
    """the same 64 bits in every element, any NaN equal to any NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(_same(a, b)))


def _same(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# call -> {wide stride: (operand, "in" / "out")}
OPERANDS = {
    "cols": {"ldy": ("Y", "in"), "ldyi": ("YI", "out")},
    "pairs": {"ldx": ("X", "in"), "ldy": ("Y", "in"), "ldyi": ("YI", "out")},
    "each": {"ldx": ("X", "in"), "ldy": ("Y", "in"), "ldxi": ("XI", "in"), "ldyi": ("YI", "out")},
    "rows": {"ldy": ("Y", "in"), "ldyi": ("YI", "out")},
    "rowpairs": {"ldx": ("X", "in"), "ldy": ("Y", "in"), "ldyi": ("YI", "out")},
    "slices2": {"ldz": ("Z", "in"), "z_slice_stride": ("Z", "in"), "ldzi": ("ZI", "out"), "zi_slice_stride": ("ZI", "out")},
}
# call -> (mi_debug_*_launches, number of forms)
COUNTERS = {"each": ("mi_debug_each_launches", 4), "rows": ("mi_debug_rows1_launches", 3),
            "rowpairs": ("mi_debug_rowpairs_launches", 2), "slices2": ("mi_debug_slices2_launches", 4)}
# the documented limits the form-selecting sizes are held against (csrc/mi_*.hip)
LIMITS = {"cols_lds_n": 8192, "pairs_lds_n": 4096, "each_thin_n": 32, "each_thin_q": 8, "rows_thin_m": 256,
          "rowpairs_thin_n": 32, "slices_lds_elems": 8192, "slices_thin_rows": 256}


class Block:
    """one contiguous piece of the wide operand: D its offset from the operand's base, span its elements, idx the position
    inside it of every logical element of sel, an index into the operand's (rows, cols, slices) array"""

    def __init__(self, D, span, idx, sel):
        self.D, self.span, self.idx, self.sel = D, span, idx, sel


def wide_stride(count, parity, span):
    """the stride that puts the last of `count` blocks of `span` elements just beyond 2^32"""
    pad = -(-2 * (span + 2 * GUARD) // 1024) * 1024
    ld = -(-_W32 // (count - 1)) + pad
    return ld + ((ld & 1) != parity)


class Case:
    """One call with one wide operand.  arrays: the logical operands by name (axes "x" / "ax", "ay", matrices "X", "Y",
    "XI", cube "Z", queries "xi", "yi", counts "lens"); form: the kernel form's name, counter: its index for
    COUNTERS[call] or None; wide: the stride made wide; parity: of that stride; align: 0 / 1 element added to BASE;
    inner: a cube's leading dimension when its slice stride is wide; even: compact operands get even leading dimensions
    (the 16-B forms); bad: tables of a paired call that are bad on purpose."""

    def __init__(self, call, form, counter, wide, parity, align, arrays, inner=None, even=False, bad=0):
        self.call, self.form, self.counter, self.wide, self.parity, self.align = call, form, counter, wide, parity, align
        self.arrays, self.even, self.bad = arrays, even, bad
        self.operand, self.role = OPERANDS[call][wide]
        self.how = "slice" if "slice" in wide else "ld"
        self.base = BASE + align
        self.wshape = self._shape3(self.operand)
        rows, cols, S = self.wshape
        if self.how == "ld":
            assert S == 1
            self.inner = None
            self.stride = wide_stride(cols, parity, rows)
        else:
            self.inner = inner or rows
            self.stride = wide_stride(S, parity, (cols - 1) * self.inner + rows)
        self.id = "%s-%s-%s-%s%s" % (call, form, wide, "odd" if parity else "even", "+8B" if align else "")

    def __repr__(self):
        return self.id

    # ---- shapes ----------------------------------------------------------------------------------------------------
    def out_shape(self):
        A = self.arrays
        if self.call in ("cols", "pairs", "each"):
            nxi = A["XI"].shape[0] if self.call == "each" else A["xi"].size
            return (nxi, A["Y"].shape[1])
        if self.call in ("rows", "rowpairs"):
            return (A["Y"].shape[0], A["xi"].size)
        return (A["yi"].size, A["xi"].size, A["Z"].shape[2])

    def _shape3(self, name):
        s = tuple(self.out_shape() if name in ("YI", "ZI") else self.arrays[name].shape)
        return s + (1,) * (3 - len(s))

    def compact_ld(self, name):
        """leading dimension of an operand that is not the wide one"""
        rows = self._shape3(name)[0]
        return rows + (rows & 1) if self.even else rows

    def view_strides(self):
        """element strides of the wide operand's (rows, cols, slices) view"""
        rows, cols, S = self.wshape
        return (1, self.stride, self.stride * cols) if self.how == "ld" else (1, self.inner, self.stride)

    def extent(self):
        """elements from the operand's first to behind its last"""
        return self.blocks()[-1].D + self.blocks()[-1].span

    @functools.lru_cache(maxsize=None)
    def blocks(self):
        rows, cols, S = self.wshape
        if self.how == "ld":
            return [Block(j * self.stride, rows, np.arange(rows), (slice(None), j, 0)) for j in range(cols)]
        idx = np.arange(rows)[:, None] + np.arange(cols)[None, :] * self.inner
        return [Block(s * self.stride, (cols - 1) * self.inner + rows, idx, (slice(None), slice(None), s)) for s in range(S)]

    # ---- the reference ---------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def want(self):
        """(expected output in out_shape(), expected col_ok / row_ok or None)"""
        return expected(self.call, self.arrays)

    @functools.lru_cache(maxsize=None)
    def flagged(self):
        """outputs that are no interpolated value: extrap, NaN of a NaN query, NaN of a bad column / row"""
        other, _ = expected(self.call, self.arrays, extrap=EXTRAP + 1.0)
        w = self.want()[0]
        return np.isnan(w) | ~_same(w, other)

    def planted_flagged(self):
        """what the construction plants: FLAGGED_PER_TABLE per good table, every output of a bad one"""
        shape = self.out_shape()
        if self.call == "slices2":
            nyi, nxi, S = shape
            return S * (FLAGGED_PER_TABLE * nyi + FLAGGED_PER_TABLE * nxi - FLAGGED_PER_TABLE**2)
        tables, nq = (shape[1], shape[0]) if self.call in ("cols", "pairs", "each") else shape
        return FLAGGED_PER_TABLE * (tables - self.bad) + nq * self.bad

    # ---- the pool --------------------------------------------------------------------------------------------------
    def _logical(self, arrays=None):
        """the wide operand as a (rows, cols, slices) array: an input's data, an output's expected values"""
        a = (arrays or self.arrays)[self.operand] if self.role == "in" else self.want()[0]
        return np.asarray(a, dtype=np.float64).reshape(self.wshape)

    def _image(self, b, values, pad):
        img = np.full(b.span, pad)
        img[b.idx] = values
        return img

    @functools.lru_cache(maxsize=None)
    def windows(self):
        """everything plant() writes: [(kind, block number, alias name or None, absolute start, image)], kind one of
        "true" (an input's data / an output's pre-fill), "decoy", "alias" (an output's sentinel window), "guard" """
        out = []
        L = self._logical()
        for k, b in enumerate(self.blocks()):
            start = self.base + b.D
            if self.role == "in":
                out.append(("true", k, None, start, self._image(b, L[b.sel], np.nan)))
                for rank, (name, a) in enumerate(aliases(b.D)):
                    out.append(("decoy", k, name, self.base + a, self._image(b, self.decoy(k, rank), np.nan)))
            else:
                out.append(("true", k, None, start, self._image(b, SENT_FILL, SENT_GUARD)))
                out.append(("guard", k, "before", start - GUARD, np.full(GUARD, SENT_GUARD)))
                out.append(("guard", k, "after", start + b.span, np.full(GUARD, SENT_GUARD)))
                for name, a in aliases(b.D):
                    out.append(("alias", k, name, self.base + a, np.full(b.span, SENT_GUARD)))
        return out

    def decoy(self, k, rank):
        """the logical elements of block k's decoy number rank"""
        return self._logical()[self.blocks()[k].sel] + (3.0 + rank)

    def substituted(self, k, values):
        """the case's arrays with block k of the (input) wide operand replaced"""
        A = dict(self.arrays)
        w = np.array(self._logical(), copy=True)
        w[self.blocks()[k].sel] = values
        A[self.operand] = w.reshape(self.arrays[self.operand].shape)
        return A

    def plant(self, write):
        """write(start, image) for every window"""
        for _, _, _, start, img in self.windows():
            write(start, img)

    def expected_image(self, k):
        """block k of an output operand after a right call"""
        b = self.blocks()[k]
        return self._image(b, self._logical()[b.sel], SENT_GUARD)


def _is_bad(x):
    """mi_axis1_create's rule on the valid nodes of a column / row"""
    return x.size < 2 or not np.all(np.isfinite(x)) or not np.all(x[:-1] < x[1:])


def expected(call, A, extrap=EXTRAP):
    """(output, ok or None) of one call on the logical arrays A, from oracle.interp1_bracket / oracle.interp2_bilinear"""
    import oracle
    if call == "cols":
        return np.stack([oracle.interp1_bracket(A["x"], A["Y"][:, c], A["xi"], extrap) for c in range(A["Y"].shape[1])], axis=1), None
    if call == "rows":
        return np.stack([oracle.interp1_bracket(A["x"], A["Y"][r], A["xi"], extrap) for r in range(A["Y"].shape[0])], axis=0), None
    if call == "slices2":
        xi, yi, Z = A["xi"], A["yi"], A["Z"]
        xq, yq = np.repeat(xi, yi.size), np.tile(yi, xi.size)
        return np.stack([oracle.interp2_bilinear(A["ax"], A["ay"], Z[:, :, s], xq, yq, extrap).reshape(xi.size, yi.size).T
                         for s in range(Z.shape[2])], axis=2), None
    # the paired calls: tables along axis 0 (columns) or along axis 1 (rows)
    byrow = call == "rowpairs"
    X, Y = (A["X"], A["Y"]) if byrow else (A["X"].T, A["Y"].T)
    T, n = X.shape
    lens = A.get("lens")
    nq = A["XI"].shape[0] if call == "each" else A["xi"].size
    out = np.full((T, nq), np.nan)
    ok = np.zeros(T, dtype=np.int64)
    for t in range(T):
        nt = n if lens is None else int(lens[t])
        if nt < 2 or nt > n or _is_bad(X[t, :nt]):
            continue
        ok[t] = 1
        out[t] = oracle.interp1_bracket(X[t, :nt], Y[t, :nt], A["XI"][:, t] if call == "each" else A["xi"], extrap)
    return (out if byrow else out.T), (ok if lens is not None else None)


# ---- the pool as the CPU test models it, and the stand-in for the device call -------------------------------------------

class SparsePool:
    """the pool as a dict of the planted windows; a read or a write that is not inside one of them raises KeyError:
    every misreading of every offset has to land in a planted window"""

    def __init__(self):
        self.w = {}

    def _find(self, start, n):
        if start in self.w and n <= self.w[start].size:
            return self.w[start], 0
        for s, a in self.w.items():
            if s <= start and start + n <= s + a.size:
                return a, start - s
        raise KeyError("elements [%d, %d) are in no planted window" % (start, start + n))

    def write(self, start, img):
        assert 0 <= start and start + img.size <= POOL
        try:
            a, o = self._find(start, img.size)
            a[o:o + img.size] = img
        except KeyError:
            self.w[start] = np.array(img, dtype=np.float64, copy=True)

    def read(self, start, n):
        a, o = self._find(start, n)
        return a[o:o + n].copy()


def model_call(case, pool, address):
    """a numpy stand-in for the device call whose offsets into the wide operand go through address(D): gathers a wide
    input from the pool and evaluates the oracle on it, or scatters the oracle's result into a wide output (only the
    logical elements are written, as the kernels do).  Returns (output or None, ok or None)."""
    if case.role == "in":
        w = np.empty(case.wshape)
        for b in case.blocks():
            w[b.sel] = pool.read(case.base + address(b.D), b.span)[b.idx]
        A = dict(case.arrays)
        A[case.operand] = w.reshape(case.arrays[case.operand].shape)
        return expected(case.call, A)
    out, ok = case.want()
    L = out.reshape(case.wshape)
    for b in case.blocks():
        start = case.base + address(b.D)
        img = pool.read(start, b.span)
        img[b.idx] = L[b.sel]
        pool.write(start, img)
    return None, ok


def check(case, read, out=None, ok=None, forms_delta=None):
    """The check of both tests; AssertionError names what is wrong.  read(start, n): n elements of the pool; out: the
    call's result when the wide operand is an input (a wide output is read from the pool); ok: col_ok / row_ok when the
    case gives lens; forms_delta: how far each counter of COUNTERS[case.call] moved during the call."""
    want, want_ok = case.want()
    if case.role == "in":
        assert out is not None and same_bits(np.asarray(out).reshape(want.shape), want), "%s: results differ from the oracle" % case.id
    for kind, k, name, start, img in case.windows():
        got = read(start, img.size)
        if kind == "true" and case.role == "out":
            b = case.blocks()[k]
            assert not np.any(got[b.idx] == SENT_FILL), "%s: block %d of the output was not fully written" % (case.id, k)
            exp = case.expected_image(k)
            assert same_bits(got, exp), "%s: block %d of the output differs from the oracle%s" % (
                case.id, k, "" if same_bits(got[b.idx], exp[b.idx]) else " (its values, not only its padding)")
        else:
            assert same_bits(got, img), "%s: the %s window (%s) of block %d was disturbed" % (case.id, kind, name, k)
    if want_ok is not None:
        assert ok is not None and np.array_equal(np.asarray(ok, dtype=np.int64), want_ok), "%s: col_ok / row_ok" % case.id
    if case.counter is not None and forms_delta is not None:
        nforms = COUNTERS[case.call][1]
        assert list(forms_delta) == [int(f == case.counter) for f in range(nforms)], "%s: form counters moved by %s, form %d expected" % (
            case.id, list(forms_delta), case.counter)


# ---- data -------------------------------------------------------------------------------------------------------------------

def axis(rng, n):
    """n strictly increasing nodes, the first exactly 1.0, the last exactly 2.0, the interior jittered"""
    g = rng.uniform(0.5, 1.5, n - 1)
    x = 1.0 + np.concatenate(([0.0], np.cumsum(g) / g.sum()))
    x[-1] = 2.0
    assert np.all(x[:-1] < x[1:])
    return x


def queries(rng, x, count, skip=()):
    """count queries on axis x in a seeded order: the kinds of the module docstring but those named in skip, then seeded
    uniform points in range"""
    n = x.size
    km, kp = max(1, n // 2), min(n - 2, n // 2)
    kinds = [("first_node", x[0]), ("last_node", x[-1]), ("first_cell", 0.5 * (x[0] + x[1])), ("last_cell", 0.5 * (x[-2] + x[-1])),
             ("node", x[n // 2]), ("node_minus", np.nextafter(x[km], -np.inf)), ("node_plus", np.nextafter(x[kp], np.inf)),
             ("nan", np.nan), ("below", 0.5), ("above", 2.5)]
    q = [v for k, v in kinds if k not in skip]
    assert len(q) <= count
    q = np.concatenate((q, rng.uniform(1.0, 2.0, count - len(q))))
    return q[rng.permutation(count)]


def _tables(rng, T, n, lens):
    """(T, n) nodes and values of a paired call, one table per row of the arrays, and (lens or None, bad tables)"""
    X = np.stack([axis(rng, n) for _ in range(T)])
    Y = rng.standard_normal((T, n))
    if not lens:
        return X, Y, None, 0
    L = np.full(T, n, dtype=np.int32)
    L[0] = n - 1
    X[0, :n - 1] = axis(rng, n - 1)
    X[0, n - 1] = Y[0, n - 1] = np.nan
    bad = 0
    if T >= 3:
        X[1, 1] = X[1, 0]
        bad = 1
    return X, Y, L, bad


def _case(call, form, counter, wide, parity, align=None, lens=False, even=False, n=None, nq=None, T=None, m=None, nx=None, ny=None,
          nyi=None, S=None, inner_pad=0, seed=0):
    rng = np.random.default_rng(seed)
    align = parity if align is None else align
    if call in ("cols", "rows"):
        x = axis(rng, n)
        A = {"x": x, "xi": queries(rng, x, nq)}
        A["Y"] = rng.standard_normal((n, T)) if call == "cols" else rng.standard_normal((m, n))
        return Case(call, form, counter, wide, parity, align, A, even=even)
    if call in ("pairs", "rowpairs", "each"):
        tables = m if call == "rowpairs" else T
        X, Y, L, bad = _tables(rng, tables, n, lens)
        far = X[-1]                                              # the table whose column is the far one
        A = {"X": X if call == "rowpairs" else X.T.copy(), "Y": Y if call == "rowpairs" else Y.T.copy()}
        if L is not None:
            A["lens"] = L
        if call == "each":
            thin = nq <= LIMITS["each_thin_q"]
            cols = []
            for t in range(tables):
                xt = X[t, :(n if L is None else int(L[t]))]
                skip = () if not thin else ("node_minus", "node") if t < tables - 1 else ("first_cell", "node")
                cols.append(queries(rng, xt, nq, skip))
            A["XI"] = np.stack(cols, axis=1)
        else:
            A["xi"] = queries(rng, far, nq)
        return Case(call, form, counter, wide, parity, align, A, even=even, bad=bad)
    ax, ay = axis(rng, nx), axis(rng, ny)
    A = {"ax": ax, "ay": ay, "Z": rng.standard_normal((ny, nx, S)), "xi": queries(rng, ax, nq), "yi": queries(rng, ay, nyi)}
    rows = nyi if OPERANDS[call][wide][1] == "out" else ny
    return Case(call, form, counter, wide, parity, align, A, inner=rows + inner_pad, even=even)


def build_cases():
    """the matrix: for every form of every call, every strided operand wide in turn"""
    C = []
    seed = [1000]

    def add(*a, **k):
        seed[0] += 1
        C.append(_case(*a, seed=seed[0], **k))

    # cols: LDS form (n <= 8192) with 16-B and with 8-B stores, direct form (n = 8193); no counter: the form follows from n
    add("cols", "lds16", None, "ldy", 0, even=True, n=257, T=2, nq=257)
    add("cols", "lds8", None, "ldy", 1, n=257, T=2, nq=255)
    add("cols", "lds16", None, "ldyi", 0, even=True, n=255, T=2, nq=257)
    add("cols", "lds8", None, "ldyi", 1, n=8192, T=2, nq=1025)
    add("cols", "direct", None, "ldy", 1, n=8193, T=2, nq=257)
    add("cols", "direct", None, "ldy", 0, even=True, n=8193, T=3, nq=255)
    add("cols", "direct", None, "ldyi", 0, even=True, n=8193, T=2, nq=257)
    add("cols", "direct", None, "ldyi", 1, n=8193, T=3, nq=255)
    # pairs: LDS form (n <= 4096), direct form (n = 4097: the validation pass first); no counter
    for form, n in (("lds", 257), ("direct", 4097)):
        add("pairs", form, None, "ldx", 0, lens=True, n=n, T=3, nq=257)
        add("pairs", form, None, "ldx", 1, n=n, T=2, nq=255)
        add("pairs", form, None, "ldy", 1, lens=True, n=n, T=2, nq=257)
        add("pairs", form, None, "ldy", 0, even=True, n=n, T=3, nq=255)
        add("pairs", form, None, "ldyi", 0, even=True, lens=True, n=n, T=3, nq=257)
        add("pairs", form, None, "ldyi", 1, n=n, T=2, nq=255)
    # each: thin (n <= 32 and nxi <= 8), LDS form, direct form
    for form, counter, n, nq in (("thin", 0, 32, 8), ("lds", 1, 4096, 257), ("direct", 2, 4097, 255)):
        for i, wide in enumerate(("ldx", "ldy", "ldxi", "ldyi")):
            add("each", form, counter, wide, i & 1, lens=wide in ("ldx", "ldyi"), even=not i & 1, n=n, T=3 if wide == "ldx" else 2, nq=nq)
    # rows: tile body 16-B (m >= 256, everything even and 16-B aligned), tile body 8-B (an odd ld), flat body (m < 256)
    for form, counter, m, parity in (("tile16", 0, 1025, 0), ("tile8", 1, 257, 1), ("flat", 2, 255, 0), ("flat", 2, 2, 1)):
        add("rows", form, counter, "ldy", parity, even=form == "tile16", n=2 if m == 257 else 3, m=m, nq=13)
        add("rows", form, counter, "ldyi", parity, even=form == "tile16", n=7, m=m, nq=13)
    add("rows", "tile8", 1, "ldy", 0, align=1, even=True, n=3, m=256, nq=13)             # even everywhere, 8-B aligned only
    # rowpairs: short rows (n <= 32), long rows (n = 33)
    for form, counter, n in (("short", 0, 3), ("short", 0, 32), ("long", 1, 33)):
        for i, wide in enumerate(("ldx", "ldy", "ldyi")):
            add("rowpairs", form, counter, wide, (i + n) & 1, lens=wide != "ldy", n=n, m=65 if n > 3 else 257,
                nq=13 if wide == "ldyi" else 257)               # enough queries to read every node column of x and y
    # slices2: forms 0-3 = LDS / direct x tile / flat; dense and padded slices
    for lds, (nx, ny) in ((True, (5, 37)), (False, (3, 4097))):
        for thin, nyi in ((False, 257), (True, 11)):
            form = "%s-%s" % ("lds" if lds else "direct", "flat" if thin else "tile")
            counter = (0 if lds else 2) + int(thin)
            for i, wide in enumerate(("ldz", "z_slice_stride", "ldzi", "zi_slice_stride")):
                S = 2 if "slice" in wide else 1
                parity = (i + int(thin)) & 1
                add("slices2", form, counter, wide, parity, even=not parity, nx=nx, ny=ny, nq=11, nyi=nyi, S=S,
                    inner_pad=(0 if parity else 4) if "slice" in wide else 0)
            add("slices2", form, counter, "z_slice_stride", int(thin), nx=nx, ny=ny, nq=11, nyi=nyi, S=2,
                inner_pad=0 if thin else 3)                     # the other of dense / padded slices of Z
    return C


CASES = build_cases()
