"""CPU checks of arma::interp1's "nearest" method along matrix rows and over paired columns
(mi_interp1_rows_nearest_f64_dev, mi_interp1_pairs_nearest_f64_dev, mi_debug_nearest_batched_launches;
Axis1.interp_rows_nearest, Axis1.interp_stack_nearest, interp_pairs_nearest): the names are declared, bound with their
linear twins' argument types and exported; the header still compiles as C99; a NULL context is refused by name before
any device call; the Python entry points hand the C ABI what their twins hand it and refuse what their twins refuse;
csrc/mi_nearest_batched.hip is built, lies outside the stamped kernel families, and what it restates of the rows, the
paired-column and the first nearest unit equals the originals; its nine kernels are in the gfx950 code object with a zero
private segment, and the kernel counts the older tests pin are unchanged."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_api_calls_cpu as tac
from test_interp1_cols_cpu import FAMILY_HASH

from armadillocudalinearinterpolation_amd import _build, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
ROWS, PAIRS, HOOK = "mi_interp1_rows_nearest_f64_dev", "mi_interp1_pairs_nearest_f64_dev", "mi_debug_nearest_batched_launches"
UNIT = "mi_nearest_batched.hip"
FAMILIES = ("interp1", "interp2", "edm")


def _rd(name):
    return open(os.path.join(_build.CSRC, name)).read()


def _header():
    whole = open(os.path.join(INCLUDE, "mi355_interp.h")).read()
    return whole, re.sub(r"/\*.*?\*/", "", whole, flags=re.S)


def test_names_declared_bound_and_exported():
    whole, text = _header()
    lib = ctypes.CDLL(_build.build_lib())
    for name in (ROWS, PAIRS):
        assert re.search(r"^mi_status\s+%s\s*\(" % name, text, flags=re.M), name
    assert re.search(r"^size_t\s+%s\s*\(\s*int\s+form\s*\)\s*;" % HOOK, text, flags=re.M)
    S = _lib.SIGNATURES
    for name in (ROWS, PAIRS, HOOK):
        assert name in S and hasattr(lib, name), name
    assert S[ROWS] == S["mi_interp1_rows_f64_dev"] and S[PAIRS] == S["mi_interp1_pairs_f64_dev"]
    assert S[HOOK] == (ctypes.c_size_t, [ctypes.c_int])
    assert lib.mi_abi_version() == 4 and "#define MI355_INTERP_ABI_VERSION 4" in text      # additive: the version stays
    additive = whole[whole.index("additive in 4"):whole.index("#define MI355_INTERP_ABI_VERSION")]
    assert all(name in additive for name in (ROWS, PAIRS, HOOK))
    L = _lib.load()
    assert L.mi_debug_nearest_batched_launches(-1) == 0 and L.mi_debug_nearest_batched_launches(5) == 0     # no such form
    assert all(L.mi_debug_nearest_batched_launches(f) >= 0 for f in range(5))
    assert L.mi_debug_nearest_launches(5) == 0                       # the first nearest hook keeps its five forms
    import armadillocudalinearinterpolation_amd as mi
    assert mi.interp_pairs_nearest is api.interp_pairs_nearest
    assert callable(mi.Axis1.interp_rows_nearest) and callable(mi.Axis1.interp_stack_nearest)


def test_header_says_which_call_when():
    whole, _ = _header()
    rows = whole[whole.index("interp1 along the rows of a matrix"):whole.index("mi_status mi_interp1_rows_f64_dev")]
    assert ROWS in rows[rows.rindex("Which call when"):]
    pairs = whole[whole.index("---- interp1 over paired columns (an X per column"):whole.index("mi_status mi_interp1_pairs_f64_dev")]
    tail = pairs[pairs.rindex("Which call when"):]
    assert PAIRS in tail and "no thin form" in tail and "n = 2" in tail
    near = whole[whole.index('arma::interp1\'s "nearest" method ---'):whole.index("mi_status mi_interp1_nearest_f64_dev")]
    tail = near[near.rindex("Which call when"):]
    assert ROWS in tail and PAIRS in tail
    for name in (ROWS, PAIRS):
        block = whole[:whole.index("mi_status " + name)]
        block = block[block.rindex("/*"):]
        assert "no host-pointer" in block and "bit for bit" in block, name


def test_header_compiles_as_c99_with_typedefs_of_the_new_calls(tmp_path):
    src = tmp_path / "nb.c"
    src.write_text('#include "mi355_interp.h"\n'
                   "typedef mi_status (*rows_fn)(mi_ctx*, const mi_axis1*, const double*, size_t, size_t, const double*, size_t,\n"
                   "                             double*, size_t, double);\n"
                   "typedef mi_status (*pairs_fn)(mi_ctx*, const double*, size_t, const double*, size_t, size_t, const uint32_t*,\n"
                   "                              size_t, const double*, size_t, double*, size_t, double, uint32_t*);\n"
                   "typedef size_t (*count_fn)(int);\n"
                   "int main(void) { rows_fn a = mi_interp1_rows_nearest_f64_dev; pairs_fn b = mi_interp1_pairs_nearest_f64_dev;\n"
                   "  count_fn d = mi_debug_nearest_batched_launches; rows_fn a0 = mi_interp1_rows_f64_dev;\n"
                   "  pairs_fn b0 = mi_interp1_pairs_f64_dev; return (a && b && d && a0 && b0) ? 0 : 1; }\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    out = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o",
                          str(tmp_path / "nb.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_a_null_context_is_refused_by_name_before_any_device_call():
    L = _lib.load()
    buf = (ctypes.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        ROWS: lambda: L.mi_interp1_rows_nearest_f64_dev(None, p, p, 4, 1, p, 4, p, 4, 0.0),
        PAIRS: lambda: L.mi_interp1_pairs_nearest_f64_dev(None, p, 4, p, 4, 4, None, 1, p, 4, p, 4, 0.0, None),
    }
    for name, call in calls.items():
        assert L.mi_group_wait_stream(None, 0, None) == 1          # another refusal in between: the text must be this call's
        assert call() == 1, name
        msg = L.mi_last_error(None).decode()
        assert msg.startswith(name + ":") and "NULL" in msg, (name, msg)


# ---- the Python entry points, without a device: what reaches the C ABI, and what is refused ---------------------------

T, cm, cube, vec = tac.T, tac.cm, tac.cube, tac.vec

ACCEPTED = {
    "rows_dense": (lambda e: e.axis(7).interp_rows_nearest(e.t("Y", cm(5, 7)), e.t("xi", vec(4)), out=e.t("out", cm(5, 4))),
                   (ROWS, ("ctx", "ax", "Y", 5, 5, "xi", 4, "out", 5, "nan"), [((5, 4), (1, 5))])),
    "rows_padded": (lambda e: e.axis(7).interp_rows_nearest(e.t("Y", cm(5, 7, ld=9)), e.t("xi", vec(4)),
                                                            out=e.t("out", cm(5, 4, ld=6)), extrap=0.25),
                    (ROWS, ("ctx", "ax", "Y", 9, 5, "xi", 4, "out", 6, 0.25), [((5, 4), (1, 6))])),
    "rows_default_out": (lambda e: e.axis(7).interp_rows_nearest(e.t("Y", cm(5, 7, ld=9)), e.t("xi", vec(4))),
                         (ROWS, ("ctx", "ax", "Y", 9, 5, "xi", 4, "out", 5, "nan"), [((5, 4), (1, 5))])),
    "stack_padded_slices": (lambda e: e.axis(4).interp_stack_nearest(e.t("Z", cube(5, 7, 4, stride=40)), e.t("ti", vec(2)),
                                                                     out=e.t("out", cube(5, 7, 2, stride=48)), extrap=0.25),
                            (ROWS, ("ctx", "ax", "Z", 40, 35, "ti", 2, "out", 48, 0.25), [((5, 7, 2), (1, 5, 48))])),
    "stack_default_out": (lambda e: e.axis(4).interp_stack_nearest(e.t("Z", cube(5, 7, 4, stride=40)), e.t("ti", vec(2))),
                          (ROWS, ("ctx", "ax", "Z", 40, 35, "ti", 2, "out", 35, "nan"), [((5, 7, 2), (1, 5, 35))])),
    "pairs_padded_x": (lambda e: api.interp_pairs_nearest(e.ctx, e.t("X", cm(5, 3, ld=9)), e.t("Y", cm(5, 3)),
                                                          e.t("xi", vec(4)), out=e.t("out", cm(4, 3))),
                       (PAIRS, ("ctx", "X", 9, "Y", 5, 5, None, 3, "xi", 4, "out", 4, "nan", None), [((4, 3), (1, 4))])),
    "pairs_lens_ok": (lambda e: api.interp_pairs_nearest(e.ctx, e.t("X", cm(5, 3)), e.t("Y", cm(5, 3, ld=6)), e.t("xi", vec(4)),
                                                         lens=e.t("lens", vec(3, np.int32)), out=e.t("out", cm(4, 3, ld=7)),
                                                         extrap=0.25, want_ok=True),
                      (PAIRS, ("ctx", "X", 5, "Y", 6, 5, "lens", 3, "xi", 4, "out", 7, 0.25, "second"),
                       [((4, 3), (1, 7)), ((3,), (1,))])),
    "pairs_default_out_ok": (lambda e: api.interp_pairs_nearest(e.ctx, e.t("X", cm(5, 3)), e.t("Y", cm(5, 3)),
                                                                e.t("xi", vec(4)), want_ok=True),
                             (PAIRS, ("ctx", "X", 5, "Y", 5, 5, None, 3, "xi", 4, "out", 4, "nan", "second"),
                              [((4, 3), (1, 4)), ((3,), (1,))])),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_accepted_call_reaches_the_library_as_its_twin_does(case):
    build, (function, args, layouts) = ACCEPTED[case]
    assert tac.record(build) == ([(function, args)], layouts)
    twin = {"rows": "rows", "stac": "stack", "pair": "pairs"}[case[:4]] + case[case.index("_"):]
    tfunction, targs, tlayouts = tac.EXPECTED[twin]                   # the linear twin: the same arguments, another function
    assert (targs, tlayouts) == (args, layouts) and tfunction == function.replace("_nearest", "")


def _pairs(e, **kw):
    a = dict(X=e.t("X", cm(5, 3)), Y=e.t("Y", cm(5, 3)), xi=e.t("xi", vec(4)))
    a.update(kw)
    return api.interp_pairs_nearest(e.ctx, a.pop("X"), a.pop("Y"), a.pop("xi"), **a)


REJECTED = {
    "rows_y_c_ordered": (lambda e: e.axis(7).interp_rows_nearest(e.t("Y", np.zeros((5, 7))), e.t("xi", vec(4, np.float32))),
                         tac.ROWMAJOR % ("Y", 7)),
    "rows_xi": (lambda e: e.axis(7).interp_rows_nearest(e.t("Y", cm(5, 7)), e.t("xi", vec(4, np.float32))), tac.XI),
    "rows_out_rows": (lambda e: e.axis(7).interp_rows_nearest(e.t("Y", cm(5, 7)), e.t("xi", vec(4)), out=e.t("out", cm(6, 4))),
                      "out must have as many rows as Y"),
    "stack_z_slices": (lambda e: e.axis(4).interp_stack_nearest(e.t("Z", cube(5, 7, 3)), e.t("ti", vec(2, np.float32))),
                       "Z must hold one slice per node of the axis (4), not 3"),
    "stack_z_padded_rows": (lambda e: e.axis(4).interp_stack_nearest(e.t("Z", cube(5, 7, 4, ld=8)), e.t("ti", vec(2))),
                            "Z: the slices must be dense (ldz == ny); this view has ldz = 8 > ny = 5"),
    "stack_out_shape": (lambda e: e.axis(4).interp_stack_nearest(e.t("Z", cube(5, 7, 4)), e.t("ti", vec(2)),
                                                                 out=e.t("out", cube(5, 7, 3))), "out must have shape (5, 7, 2)"),
    "pairs_xi_before_x": (lambda e: _pairs(e, X=e.t("X", cm(5, 3, dtype=np.float32)), xi=e.t("xi", vec(8)[::2])), tac.XI),
    "pairs_shapes_differ": (lambda e: _pairs(e, Y=e.t("Y", cm(5, 4))), tac.XY_SHAPE),
    "pairs_lens_before_out": (lambda e: _pairs(e, lens=e.t("lens", vec(2, np.int32)), out=e.t("out", cm(4, 3), cuda=False)),
                              tac.LENS),
    "pairs_out_columns": (lambda e: _pairs(e, out=e.t("out", cm(4, 2))), tac.OUT_COLS),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejected_call_names_the_rule_and_reaches_nothing(case):
    build, message = REJECTED[case]
    e = tac.Env()
    with pytest.raises(ValueError) as err:
        build(e)
    assert str(err.value) == message and e.L.calls == []


# ---- the new unit -----------------------------------------------------------------------------------------------------

def _const(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, name
    return re.sub(r"\s+", "", m.group(1))


def _body(text, signature):
    """the braces' content of the function whose text starts with `signature`, whitespace removed"""
    i = text.index(signature)
    a = text.index("{", i)
    depth, j = 0, a
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            break
        j += 1
    return re.sub(r"\s+", "", text[a:j + 1])


def test_the_unit_is_built_outside_the_stamped_families_and_they_are_untouched():
    assert os.path.join(_build.CSRC, UNIT) in _build.sources()
    assert sorted(FAMILY_HASH) == sorted(FAMILIES)
    assert {f: _build.source_hash(f) for f in FAMILIES} == FAMILY_HASH       # the pinned digests of the parent commit
    assert not any(UNIT.startswith("mi_" + f) for f in FAMILIES)
    import hashlib
    for f in FAMILIES:                                               # the unit, present or not, takes no part in a family's hash
        h = hashlib.sha256()
        for p in sorted(_build._deps()):
            b = os.path.basename(p)
            if b == UNIT or not (b.startswith("mi_" + f) or b in ("mi_common.hpp", "mi_ctx.hip")):
                continue
            h.update(b.encode())
            h.update(open(p, "rb").read())
        assert h.hexdigest() == _build.source_hash(f), f
    # and no file of a family, nor any older unit, differs from the committed parent (where git can tell)
    out = subprocess.run(["git", "diff", "--name-only", "HEAD", "--", "armadillocudalinearinterpolation_amd/csrc"], cwd=ROOT,
                         capture_output=True, text=True)
    if out.returncode == 0:
        assert [p for p in out.stdout.split() if not p.endswith(UNIT)] == []
    text = _rd(UNIT)
    code = re.sub(r"//.*", "", text)
    assert "getenv" not in code and "atomicAdd" not in code and "__atomic" not in code and "__hip_atomic" not in code
    assert "namespace mi_nearest_batched" in code
    assert not any(w in "mi_nearest_batched" for w in ("mi_rows1", "mi_pairs1", "mi_nearest1"))
    for inc in ("mi_axis1.hpp", "mi_interp2_eval.hpp", "mi_paired_cols.hpp"):
        assert '#include "%s"' % inc in text, inc
    for used in ("axis_locate", "axis_node", "col_issue", "col_commit", "col_len", "search(", "LdsX", "x_stride", "lds_bytes_for",
                 "ensure_scratch(ctx, 3"):
        assert used in code, used
    assert "struct ColLoad" not in code and "struct AxisDev" not in code        # used as they are, not restated


def test_restated_constants_and_helpers_equal_the_originals():
    new, rows, pairs, near = _rd(UNIT), _rd("mi_rows1.hip"), _rd("mi_pairs1.hip"), _rd("mi_nearest1.hip")
    for name in ("kLaneRows", "kRowBlock", "kThinM", "kMinRun", "kFlatStep", "kMaxFlatRun", "kMinFlatUnit"):
        assert _const(new, name) == _const(rows, name), name
    assert _const(new, "kPairRowBlock") == _const(pairs, "kRowBlock")
    assert _const(new, "kLdsMaxN") == _const(pairs, "kLdsMaxN")
    sig = "bool take_right(double xl, double xr, double q)"
    assert _body(new, sig) == _body(near, sig)
    for sig in ("void col_load(", "void col_store("):
        assert _body(new, sig) == _body(rows, sig), sig
    # the validation pass of long paired columns and the locate pass, but for their names
    assert _body(new, "void nb_pairs_validate_kernel(") == _body(pairs, "void pairs1_validate_kernel(")
    assert _body(new, "void nb_rows_locate_kernel(") == _body(near, "void nearest_cols_locate_kernel(")
    # check_args: the device form's rules, in the same order with the same texts
    strings = lambda t: re.findall(r'"(%s:[^"]*)"', t)  # noqa: E731
    assert strings(_body(new, "mi_status check_args(")) == strings(_body(pairs, "mi_status check_args("))
    # the unit arithmetic of both host sides
    unit_lines = lambda t, f: [re.sub(r"\s+", "", ln) for ln in t[t.index("mi_status " + f + "("):].split("\n")  # noqa: E731
                               if re.match(r"\s*(const (size_t|bool|unsigned) (thin|resident|target|nrb|min_run|run|nruns|nunits|grid|want_runs)"
                                           r"|size_t want_runs|if \(thin\) want_runs)", ln)]
    a, b = unit_lines(new, ROWS), unit_lines(rows, "mi_interp1_rows_f64_dev")
    assert len(b) == 11 and a[:11] == b, (a, b)
    a = [ln.replace("kPairRowBlock", "kRowBlock") for ln in unit_lines(new, PAIRS)]
    b = unit_lines(pairs, "mi_interp1_pairs_f64_dev")
    assert len(b) >= 6 and a[:6] == b[:6], (a, b)


def _kernels(work, pattern):
    llvm = "/opt/rocm/lib/llvm/bin"
    found = []
    for b in glob.glob(str(work / "lib.so.*gfx950")):
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", b], capture_output=True, text=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count", notes):
            name = re.search(r"\.name:\s*(\S*%s\S*)" % pattern, block)
            if name:
                found.append((name.group(1), int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)),
                              int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)),
                              int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1))))
    return found


def test_kernels_are_in_the_code_object_and_use_no_scratch(tmp_path):
    """one rows locate, two tile, one flat, one pairs validate and four pairs kernels under the new namespace, all with a
    zero private segment, the rows kernels without LDS; the kernel counts that older tests pin are what they were"""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf not found")
    _build.build_lib()
    work = tmp_path / "co"
    work.mkdir()
    shutil.copy(_build.LIB_PATH, work / "lib.so")                       # (--offloading writes the bundles next to its input)
    out = subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=work, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    mine = _kernels(work, "mi_nearest_batched")
    names = [n for n, _, _, _ in mine]
    for part, count in (("nb_rows_locate_kernel", 1), ("nb_rows_tile_kernel", 2), ("nb_rows_flat_kernel", 1),
                        ("nb_pairs_validate_kernel", 1), ("nb_pairs_kernel", 4)):
        assert sum(part in n for n in names) == count, (part, names)
    assert len(names) == 9, names
    assert all(private == 0 for _, private, _, _ in mine), mine
    assert all(lds == 0 for n, _, lds, _ in mine if "nb_rows_" in n), mine
    # one column held and one on its way: both tile kernels fit eight waves per SIMD (at most 64 registers per lane)
    assert all(v <= 64 for n, _, _, v in mine if "nb_rows_tile_kernel" in n), mine
    assert len(_kernels(work, "mi_rows1")) == 4 and len(_kernels(work, "mi_pairs1")) == 5
    assert len(_kernels(work, "mi_nearest1")) == len(set(n for n, _, _, _ in _kernels(work, "mi_nearest1")))
    near = [n for n, _, _, _ in _kernels(work, "mi_nearest1")]
    assert sum("nearest_cols_locate_kernel" in n for n in near) == 1 and sum("nearest_cols_kernel" in n for n in near) == 4


# ---- the inputs of tests/test_nearest_batched_gpu.py, before they go to the GPU ----------------------------------------

def test_generators_hold_ties_and_pick_both_sides():
    """the seeded inputs of the GPU tests, regenerated here with their seeds and draws: every set that a test claims the
    select with holds at least 8 exact ties and picks both the left and the right node; a midpoint query is an exact tie;
    the references agree with a literal per-element application of the rule"""
    import nearest_batched_cases as bc
    import nearest_cases as nc
    T, RB, PRB, LDS = 256, 1024, 2048, 4096
    for m in [1, 2, 3, T - 1, T, T + 1, RB - 1, RB, RB + 1, 2 * RB + 3]:              # test_rows_row_counts_and_forms
        rng = np.random.default_rng(1000 + m)
        X = bc.nodes(rng, 7)
        rng.standard_normal((m, 7))
        xi = bc.queries(rng, X, 37)
        assert xi.size == 37 and np.isnan(xi).any() and np.isinf(xi).sum() == 2
        bc.assert_select(X, xi)
    rng = np.random.default_rng(50 + 20_000 + RB + 1)                                 # test_rows_run_boundaries
    X = bc.nodes(rng, 50)
    mid = 0.5 * X[:-1] + 0.5 * X[1:]
    assert np.array_equal(mid - X[:-1], X[1:] - mid)                                  # exact ties
    assert bc.select_counts(X, mid) == (49, 49, 0)                                    # and a tie keeps the left node
    t, a, b = bc.select_counts(X, np.nextafter(mid, np.inf))                          # one ulp on: the right node, unless
    assert a == t and t + b == 49 and b >= 40                                         # both rounded differences still agree
    rng.standard_normal((RB + 1, 50))
    bc.assert_select(X, bc.queries(rng, X, 20_000))
    seqs = bc.sequences(bc.nodes(np.random.default_rng(77), 6))                       # test_rows_held_column_sequences
    assert len(seqs) == 10 and list(seqs.values())[-1] is None
    X = bc.nodes(np.random.default_rng(77), 6)
    k = nc.rule_index(X, np.array(seqs["right half of a cell then left half of the next (same node, no load)"]))
    assert list(k) == [2, 2, 3, 3, 3]
    assert list(nc.rule_index(X, np.array(seqs["alternating first and last node"]))) == [0, 5, 0, 5, 0, 5]
    assert all(v < 0 for v in nc.rule_index(X, np.array(seqs["all flagged"])))
    for n in [2, 3, 1024, LDS - 1, LDS, LDS + 1]:                                     # test_pairs_column_lengths_and_forms
        rng = np.random.default_rng(100 + n)
        Xb, Yb = bc.pairs(rng, 5, n)
        assert all(not bc.is_bad(x) for x in Xb)
        xi = bc.pair_queries(rng, Xb, 1500)
        assert xi.size == 1500
        bc.assert_select(bc.valid_tables(Xb), xi)
    for n in (1500, LDS + 500):                                                       # test_pairs_ragged_columns
        rng = np.random.default_rng(n + 1)
        Xb, Yb = bc.pairs(rng, 41, n)
        lens = rng.integers(2, n + 1, 41)
        lens[:6] = [2, 3, n, n - 1, 2, n]
        xi = bc.pair_queries(rng, Xb, 3000, lens)
        bc.assert_select(bc.valid_tables(Xb, lens), xi)
        want, ok = bc.ref_pairs(Xb, Yb, xi, 7.0, lens)
        assert ok.all()
        c, i = 7, 11
        assert nc._eq_bits(want[c, i:i + 1], nc.nearest_rule(Xb[c, :lens[c]], Yb[c, :lens[c]], xi[i:i + 1], 7.0))
    X = bc.nodes(np.random.default_rng(1), 9)                                         # ref_rows is the rule, row by row
    Y = np.random.default_rng(2).standard_normal((4, 9))
    xi = bc.queries(np.random.default_rng(3), X, 60)
    assert all(nc._eq_bits(bc.ref_rows(X, Y, xi, -0.0)[r], nc.nearest_rule(X, Y[r], xi, -0.0)) for r in range(4))
