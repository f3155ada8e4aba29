"""CPU checks of arma::interp2's "nearest" method (mi_interp2_nearest_f64_dev, mi_interp2_grid_nearest_f64_dev / _host,
mi_interp2_slices_nearest_f64_dev, mi_debug_nearest2_launches; Grid2.interp_nearest, .interp_grid_nearest,
.interp_grid_nearest_host, interp2_slices_nearest; mi355::interp2(..., method)): the 2-D reference of the GPU tests equals
Armadillo's two-pass scan; the names are declared, bound with their linear twins' argument types and exported; a NULL
context is refused by name; the Python entry points hand the C ABI what their twins hand it and refuse what their twins
refuse; csrc/mi_nearest2.hip is built, lies outside the stamped kernel families, and what it restates equals the
originals; its kernels are in the gfx950 code object with a zero private segment; the C++ overloads resolve."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import nearest2_cases as n2
import nearest_batched_cases as bc
import nearest_cases as nc
import test_api_calls_cpu as tac
import test_nearest_batched_cpu as tnb

from armadillocudalinearinterpolation_amd import _build, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
UNIT = "mi_nearest2.hip"
FAMILIES = ("interp1", "interp2", "edm")
PAIRS, GRID, GRID_H = "mi_interp2_nearest_f64_dev", "mi_interp2_grid_nearest_f64_dev", "mi_interp2_grid_nearest_f64_host"
SLICES, HOOK = "mi_interp2_slices_nearest_f64_dev", "mi_debug_nearest2_launches"
TWIN = {PAIRS: "mi_interp2_f64_dev", GRID: "mi_interp2_grid_f64_dev", GRID_H: "mi_interp2_grid_f64_host",
        SLICES: "mi_interp2_slices_f64_dev"}
NFORMS = 8


# ---- the reference ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_x,kind_y", [("near", "clustered"), ("clustered", "uniform"), ("uniform", "near"), ("random", "random")])
def test_reference_equals_armadillos_two_pass_scan(kind_x, kind_y):
    """arma::interp2's "nearest" runs interp2_helper_nearest along one axis, then along the other.  Restated with
    nearest_cases.scan_index (the literal scan) on sorted queries -- first the columns of Z picked along x, then the rows
    of that picked along y -- it equals ref_grid on EVERY element, for every pairing of the three axis kinds.  The 1-D
    rule's one documented deviation from the scan (include/mi355_interp.h: nodes [0, 2^-60, 1, 2], q = 1, where two nodes
    in front of the nearest one have equal rounded distances and the scan stops early) would show here as whole columns
    (x axis) or rows (y axis) of ZI taken from node 0 instead of node 2; the axes of these tests lie on a grid of 1/8,
    where every distance is exact, so it cannot occur."""
    rng = np.random.default_rng([2, n2.KINDS.index(kind_x) if kind_x in n2.KINDS else 9])
    X, Y = n2.axis(kind_x, rng, 11), n2.axis(kind_y, rng, 9)
    Z = n2.table(9, 11)
    xi, yi = np.sort(bc.queries(rng, X, 70)), np.sort(bc.queries(rng, Y, 37))          # ascending, NaN last
    bc.assert_select(X, xi)
    bc.assert_select(Y, yi)
    sx, sy = nc.scan_index(X, xi), nc.scan_index(Y, yi)
    assert np.array_equal(sx, nc.rule_index(X, xi)) and np.array_equal(sy, nc.rule_index(Y, yi))
    for extrap in (np.nan, -7.5):
        pass1 = np.stack([nc._gather(Z[i, :], sx, extrap) for i in range(9)])          # (ny, nxi): along x
        # along y; a flagged column of pass 1 stays what it is whatever row is picked, and NaN wins over out-of-range
        want = np.empty((yi.size, xi.size))
        for j in range(xi.size):
            want[:, j] = nc._gather(pass1[:, j], sy, extrap)
            if sx[j] == -2:
                want[:, j] = np.nan
            elif sx[j] == -1:
                want[sy != -2, j] = extrap
        assert nc._eq_bits(want, n2.ref_grid(X, Y, Z, xi, yi, extrap)), (kind_x, kind_y, extrap)


def test_references_agree_and_cases_hold_what_they_claim():
    rng = np.random.default_rng(5)
    for kind in n2.KINDS:
        X = n2.axis(kind, rng, 11)
        assert np.all(np.diff(X) > 0) and np.array_equal(X * 8, np.round(X * 8))          # on the grid of 1/8
        mid = 0.5 * X[:-1] + 0.5 * X[1:]
        assert np.array_equal(mid - X[:-1], X[1:] - mid)                                  # exact ties
    assert n2.uses_guess(n2.axis("near", rng, 11)) and n2.uses_guess(n2.axis("near", rng, 9))
    assert not n2.uses_guess(n2.axis("clustered", rng, 11)) and not n2.uses_guess(n2.axis("clustered", rng, 9))
    for n, nq in [(2, 37), (3, 40), (9, 37), (9, 70), (11, 257)]:                          # the condition the issue states
        for seed in range(200):
            r = np.random.default_rng(seed)
            Xs = bc.nodes(r, n)
            bc.assert_select(Xs, bc.queries(r, Xs, nq))
    X, Y = bc.nodes(rng, 11), bc.nodes(rng, 9)
    Z = n2.table(9, 11)
    assert np.unique(Z[np.isfinite(Z) & (Z != 0) & (np.abs(Z) > 1)]).size == Z.size - len(n2.SPECIAL_NODES)
    xi, yi = bc.queries(rng, X, 70), bc.queries(rng, Y, 37)
    G = n2.ref_grid(X, Y, Z, xi, yi, -7.5)
    xx, yy = np.meshgrid(xi, yi)                                                          # (nyi, nxi)
    assert nc._eq_bits(n2.ref_pairs(X, Y, Z, xx.ravel(), yy.ravel(), -7.5).reshape(G.shape), G)
    Zc = n2.cube(9, 11, 3)
    S = n2.ref_slices(X, Y, Zc, xi, yi, -7.5)
    assert S.shape == (37, 70, 3) and nc._eq_bits(S[:, :, 0], G)
    assert np.isfinite(Zc[:, :, 1:]).all() and not np.isfinite(Zc[:, :, 0]).all()
    # NaN wins over out-of-range; every special value appears, with its bits
    xq, yq = n2.pair_queries(rng, X, Y, 40)
    P = n2.ref_pairs(X, Y, Z, xq, yq, -7.5)
    assert np.isnan(P[:3]).all()
    assert np.isposinf(G).any() and np.isneginf(G).any() and np.isnan(G).any() and (G == n2.DENORMAL).any()
    assert (np.signbit(G) & (G == 0)).any() and n2.POISON not in G
    seqs = n2.x_sequences(X)
    assert list(nc.rule_index(X, np.array(seqs["kx returning to an earlier column"]))) == [1, 4, 1, 4, 1, 1, 4]
    assert list(nc.rule_index(X, np.array(seqs["runs of equal kx"]))) == [0, 0, 0, 0, 1, 1, 2, 2, 2]
    assert list(nc.rule_index(X, np.array(seqs["every node in order"]))) == list(range(11))
    assert all(k < 0 for k in nc.rule_index(X, np.array(seqs["all flagged"])))
    assert nc.rule_index(X, np.array(seqs["a run that starts flagged"]))[0] == -2


# ---- the ABI ----------------------------------------------------------------------------------------------------------

def _header():
    whole = open(os.path.join(INCLUDE, "mi355_interp.h")).read()
    return whole, re.sub(r"/\*.*?\*/", "", whole, flags=re.S)


def test_names_declared_bound_and_exported():
    whole, text = _header()
    lib = ctypes.CDLL(_build.build_lib())
    S = _lib.SIGNATURES
    for name, twin in TWIN.items():
        assert re.search(r"^mi_status\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in S and hasattr(lib, name), name
        assert S[name] == S[twin], name
        decl = lambda f: re.sub(r"\s+", " ", re.search(r"^mi_status\s+%s\s*\(([^;]*)\)\s*;" % f, text, flags=re.M).group(1))  # noqa: E731
        assert decl(name) == decl(twin), name                                 # the twin's parameter list, word for word
    assert re.search(r"^size_t\s+%s\s*\(\s*int\s+form\s*\)\s*;" % HOOK, text, flags=re.M)
    assert S[HOOK] == (ctypes.c_size_t, [ctypes.c_int]) and hasattr(lib, HOOK)
    assert lib.mi_abi_version() == 4 and "#define MI355_INTERP_ABI_VERSION 4" in text      # additive: the version stays
    additive = whole[whole.index("additive in 4"):whole.index("#define MI355_INTERP_ABI_VERSION")]
    assert all(name in additive for name in list(TWIN) + [HOOK])
    L = _lib.load()
    assert L.mi_debug_nearest2_launches(-1) == 0 and L.mi_debug_nearest2_launches(NFORMS) == 0   # no such form
    assert all(L.mi_debug_nearest2_launches(f) >= 0 for f in range(NFORMS))
    import armadillocudalinearinterpolation_amd as mi
    assert mi.interp2_slices_nearest is api.interp2_slices_nearest
    for m in ("interp_nearest", "interp_grid_nearest", "interp_grid_nearest_host"):
        assert callable(getattr(mi.Grid2, m)), m


def test_header_states_the_rule_and_says_which_call_when():
    whole, _ = _header()
    top = whole[:whole.index("#ifndef MI355_INTERP_H")]
    for words in ("2-D nearest rule", "either coordinate NaN", "NaN wins over out-of-range", "Z(ky, kx), the stored 64 bits",
                  "may be in any order"):
        assert words in top, words
    assert top.index("nearest rule shared by every") < top.index("2-D nearest rule")        # next to the 1-D rule
    i2 = whole[whole.index("2-D tables and scattered bilinear interpolation"):whole.index("mi_status " + PAIRS)]
    tail = i2[i2.index("Which call when"):]
    assert "nearest twins" in tail
    sl = whole[whole.index("gridded interp2 over the slices of a cube"):whole.index("mi_status mi_interp2_slices_f64_dev")]
    assert SLICES in sl[sl.rindex("Which call when"):]
    assert "There is no nearest form of the each and rowpairs calls." in whole
    assert "no nearest form of the each, rowpairs and slices" not in whole
    block = whole[:whole.index("mi_status " + SLICES)]
    block = block[block.rindex("/*"):]
    assert "word for word" in block and "never" in block and "bit-identical" in block


def test_header_compiles_as_c99_with_typedefs_of_the_new_calls(tmp_path):
    src = tmp_path / "n2.c"
    src.write_text('#include "mi355_interp.h"\n'
                   "typedef mi_status (*pairs_fn)(mi_ctx*, const mi_grid2*, const double*, const double*, double*, size_t, double);\n"
                   "typedef mi_status (*grid_fn)(mi_ctx*, const mi_grid2*, const double*, size_t, const double*, size_t, double*, double);\n"
                   "typedef mi_status (*slices_fn)(mi_ctx*, const mi_axis1*, const mi_axis1*, const double*, size_t, size_t, size_t,\n"
                   "                               const double*, size_t, const double*, size_t, double*, size_t, size_t, double);\n"
                   "typedef size_t (*count_fn)(int);\n"
                   "int main(void) { pairs_fn a = mi_interp2_nearest_f64_dev, a0 = mi_interp2_f64_dev;\n"
                   "  grid_fn b = mi_interp2_grid_nearest_f64_dev, b0 = mi_interp2_grid_f64_dev, c = mi_interp2_grid_nearest_f64_host;\n"
                   "  slices_fn d = mi_interp2_slices_nearest_f64_dev, d0 = mi_interp2_slices_f64_dev; count_fn e = mi_debug_nearest2_launches;\n"
                   "  return (a && a0 && b && b0 && c && d && d0 && e) ? 0 : 1; }\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    out = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o",
                          str(tmp_path / "n2.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_a_null_context_is_refused_by_name_before_any_device_call():
    L = _lib.load()
    buf = (ctypes.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        PAIRS: lambda: L.mi_interp2_nearest_f64_dev(None, p, p, p, p, 4, 0.0),
        GRID: lambda: L.mi_interp2_grid_nearest_f64_dev(None, p, p, 2, p, 2, p, 0.0),
        GRID_H: lambda: L.mi_interp2_grid_nearest_f64_host(None, p, p, 2, p, 2, p, 0.0),
        SLICES: lambda: L.mi_interp2_slices_nearest_f64_dev(None, p, p, p, 2, 4, 1, p, 2, p, 2, p, 2, 4, 0.0),
    }
    before = [L.mi_debug_nearest2_launches(f) for f in range(NFORMS)]
    for name, call in calls.items():
        assert L.mi_group_wait_stream(None, 0, None) == 1          # another refusal in between: the text must be this call's
        assert call() == 1, name
        msg = L.mi_last_error(None).decode()
        assert msg.startswith(name + ":") and "NULL" in msg, (name, msg)
    assert [L.mi_debug_nearest2_launches(f) for f in range(NFORMS)] == before


# ---- the Python entry points, without a device: what reaches the C ABI, and what is refused ---------------------------

cm, cube, vec = tac.cm, tac.cube, tac.vec


def _slices(e, Z, xi=None, yi=None, out=None, **kw):
    return api.interp2_slices_nearest(e.ctx, e.axis(3, "ax"), e.axis(2, "ay"), Z, xi if xi is not None else e.t("xi", vec(5)),
                                      yi if yi is not None else e.t("yi", vec(6)), out=out, **kw)


ACCEPTED = {
    "grid2_interp": lambda e: e.grid2().interp_nearest(e.t("xq", vec(4)), e.t("yq", vec(4)), out=e.t("out", vec(4)), extrap=2.0),
    "grid2_interp_grid": lambda e: e.grid2().interp_grid_nearest(e.t("xi", vec(3)), e.t("yi", vec(2)), out=e.t("out", np.zeros((3, 2)))),
    "grid2_interp_grid_default_out": lambda e: e.grid2().interp_grid_nearest(e.t("xi", vec(3)), e.t("yi", vec(2)), extrap=1.5),
    "slices_dense": lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", cube(6, 5, 4))),
    "slices_padded": lambda e: _slices(e, e.t("Z", cube(2, 3, 4, ld=8, stride=30)), out=e.t("out", cube(6, 5, 4, ld=7, stride=40)),
                                       extrap=0.25),
    "slices_one_slice": lambda e: _slices(e, e.t("Z", cube(2, 3, 1)), xi=e.t("xi", vec(1)), yi=e.t("yi", vec(1)),
                                          out=e.t("out", cube(1, 1, 1))),
    "slices_default_out": lambda e: _slices(e, e.t("Z", cube(2, 3, 4, ld=8, stride=30))),
}
NEW_NAME = {"mi_interp2_f64_dev": PAIRS, "mi_interp2_grid_f64_dev": GRID, "mi_interp2_slices_f64_dev": SLICES}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_accepted_call_reaches_the_library_as_its_twin_does(case):
    """the same arguments and the same layout of the result as the linear twin (tests/test_api_calls_cpu.py), another
    function; and the twin itself still reaches its own function with them"""
    tfunction, targs, tlayouts = tac.EXPECTED[case]
    assert tac.record(ACCEPTED[case]) == ([(NEW_NAME[tfunction], targs)], tlayouts)
    assert tac.record(tac.ACCEPTED[case]) == ([(tfunction, targs)], tlayouts)


def test_host_form_reaches_the_library_as_its_twin_does():
    near = tac.record(lambda e: e.grid2().interp_grid_nearest_host(e.a("xi", vec(3)), e.a("yi", vec(2)), extrap=1.5))
    twin = tac.record(lambda e: e.grid2().interp_grid_host(e.a("xi", vec(3)), e.a("yi", vec(2)), extrap=1.5))
    assert near == ([(GRID_H, ("ctx", "grid", "xi", 3, "yi", 2, "out", 1.5))], [((2, 3), (1, 2))])
    assert twin == ([("mi_interp2_grid_f64_host", near[0][0][1])], near[1])
    near = tac.record(lambda e: e.grid2().interp_grid_nearest_host([0.0, 1.0, 2.0], (0.5, 1.5)))          # lists are converted
    assert near == ([(GRID_H, ("ctx", "grid", "copy", 3, "copy", 2, "out", "nan"))], [((2, 3), (1, 2))])


REJECTED = {
    "grid2_interp_queries": (lambda e: e.grid2().interp_nearest(e.t("xq", vec(4)), e.t("yq", vec(8)[::2])),
                             "queries must be contiguous float64 CUDA tensors"),
    "grid2_interp_queries_before_sizes": (lambda e: e.grid2().interp_nearest(e.t("xq", vec(4, np.float32)), e.t("yq", vec(3))),
                                          "queries must be contiguous float64 CUDA tensors"),
    "grid2_interp_sizes": (lambda e: e.grid2().interp_nearest(e.t("xq", vec(4)), e.t("yq", vec(3))),
                           "xq and yq must have the same number of elements"),
    "grid2_interp_out_small": (lambda e: e.grid2().interp_nearest(e.t("xq", vec(4)), e.t("yq", vec(4)), out=e.t("out", vec(1))),
                               tac.SAME_SIZE),
    "grid2_interp_grid_axes": (lambda e: e.grid2().interp_grid_nearest(e.t("xi", vec(3)), e.t("yi", vec(2), cuda=False)), tac.AXES),
    "grid2_interp_grid_out": (lambda e: e.grid2().interp_grid_nearest(e.t("xi", vec(3)), e.t("yi", vec(2)),
                                                                      out=e.t("out", np.zeros((2, 3)))),
                              "out must be a contiguous float64 CUDA tensor of shape (len(xi), len(yi))"),
    "slices_axes": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), yi=e.t("yi", vec(6, np.float32))), tac.AXES),
    "slices_axes_before_z": (lambda e: _slices(e, e.t("Z", cm(2, 3)), xi=e.t("xi", vec(10)[::2])), tac.AXES),
    "slices_z_float32": (lambda e: _slices(e, e.t("Z", np.zeros((4, 3, 2), np.float32).transpose(2, 1, 0))),
                         "Z must be a float64 CUDA tensor"),
    "slices_z_shape": (lambda e: _slices(e, e.t("Z", cube(3, 2, 4))), "Z must have shape (2, 3, S)"),
    "slices_z_two_dims": (lambda e: _slices(e, e.t("Z", cm(2, 3))), "Z must have shape (2, 3, S)"),
    "slices_z_c_ordered": (lambda e: _slices(e, e.t("Z", np.zeros((2, 3, 4)))), tac.CUBE % ("Z", 3, 2)),
    "slices_z_overlapping": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4, ld=4, stride=11))), tac.CUBE % ("Z", 3, 2)),
    "slices_out_host": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", cube(6, 5, 4), cuda=False)), tac.OUT_CUDA),
    "slices_out_shape": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", cube(5, 6, 4))),
                         "out must have shape (6, 5, S)"),
    "slices_out_c_ordered": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", np.zeros((6, 5, 4)))),
                             tac.CUBE % ("out", 5, 6)),
    "slices_out_slices": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", cube(6, 5, 3))),
                          "out must have as many slices as Z"),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejected_call_names_its_twins_rule_and_reaches_nothing(case):
    build, message = REJECTED[case]
    assert tac.REJECTED[case][1] == message                          # the twin's message for the same input
    e = tac.Env()
    with pytest.raises(ValueError) as err:
        build(e)
    assert str(err.value) == message and e.L.calls == []


def test_every_rejection_of_the_twins_is_covered():
    twins = [k for k in tac.REJECTED if k.startswith(("grid2_interp", "slices_"))]
    assert sorted(twins) == sorted(REJECTED)


# ---- the new unit -----------------------------------------------------------------------------------------------------

_rd, _const, _body = tnb._rd, tnb._const, tnb._body


def test_the_unit_is_built_outside_the_stamped_families():
    assert os.path.join(_build.CSRC, UNIT) in _build.sources()
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
    text = _rd(UNIT)
    code = re.sub(r"//.*", "", text)
    assert "getenv" not in code and "atomicAdd" not in code and "__atomic" not in code and "__hip_atomic" not in code
    assert "namespace mi_nearest2" in code
    for inc in ("mi_axis1.hpp", "mi_interp2_eval.hpp"):
        assert '#include "%s"' % inc in text, inc
    for used in ("axis_locate", "axis_node", "kBlock", "AxisDev", "G2Dev", "mi_grid2", "mi_axis1", "ensure_scratch(ctx, 3"):
        assert used in code, used
    assert "struct AxisDev" not in code and "struct G2Dev" not in code          # used as they are, not restated
    # no pinning, no second stream, no LDS anywhere in the unit
    for absent in ("pin_host", "aux_stream", "ensure_aux_stream", "__shared__", "hipHostRegister", "hipStreamCreate"):
        assert absent not in code, absent
    # the value is never touched by arithmetic: the only fp64 subtractions are take_right's two
    assert len(re.findall(r"const double [ab] = ", code)) == 2


def test_restated_constants_and_helpers_equal_the_originals():
    new, grid, slices, nb = _rd(UNIT), _rd("mi_interp2_grid.hip"), _rd("mi_slices2.hip"), _rd("mi_nearest_batched.hip")
    for name in ("kTileRows", "kThinRows", "kMaxGrid"):
        assert _const(new, name) == _const(grid, name), name
    for name in ("kTileRows", "kThinRows", "kMaxFlatStrip"):
        assert _const(new, name) == _const(slices, name), name
    sig = "bool take_right(double xl, double xr, double q)"
    assert _body(new, sig) == _body(nb, sig)
    assert _body(new, "inline size_t mul_sat(") == _body(slices, "inline size_t mul_sat(")
    # check_args: the slices call's rules, in the same order with the same texts -- the whole body, where the twin's
    # record size stands as a constant
    assert _const(new, "kTwinRecBytes") == "16"
    assert _body(new, "mi_status check_args(").replace("kTwinRecBytes", "sizeof(AxRec)") == _body(slices, "mi_status check_args(")
    # the flat bodies' index arithmetic and the locate pass's loop
    assert _body(new, "void nearest2_grid_flat_kernel(").replace("T,cols", "g,cols") == _body(grid, "void interp2_grid_flat_kernel(")
    # the unit arithmetic of both host sides
    def lines(t, f, pattern):
        return [re.sub(r"\s+", "", ln) for ln in t[t.index("mi_status " + f + "("):].split("\n") if re.match(pattern, ln)]
    pat = (r"\s*(const size_t (total|nwork|nrb|target|want_strips|strip) =|const unsigned grid =|if \(nyi < kThinRows\)"
           r"|if \(\(reinterpret_cast<uintptr_t>\(zi\) & 15u\) == 0)")
    a, b = lines(new, GRID, pat), lines(grid, "mi_interp2_grid_f64_dev", pat)
    strip = lambda ls: [ln.rstrip("{") for ln in ls]  # noqa: E731
    assert len(b) >= 12 and strip(a[:12]) == strip(b[:12]), (a, b)       # (the host forms follow in both files)
    pat = (r"\s*(const size_t (cus|target|blocks) =|const bool (thin|vec) =|size_t want_strips =|if \(thin\) want_strips"
           r"|S\.(ldz|zstride|nslices|nxi|nyi|ldzi|zistride|nrb|strip|nstrips|nunits) =|const unsigned grid =)")
    a, b = lines(new, SLICES, pat), lines(slices, "mi_interp2_slices_f64_dev", pat)
    assert len(b) == 19 and a[:19] == b, (a, b)
    # the messages of the entry points: the twins' with the entry point's own name
    msgs = lambda t, f: [m.replace(f, "F") for m in re.findall(r'"(%s:[^"]*)"' % f, t)]  # noqa: E731
    scattered = _rd("mi_interp2.hip")
    assert msgs(new, PAIRS) == msgs(scattered, "mi_interp2_f64_dev") and len(msgs(new, PAIRS)) == 4
    assert msgs(new, GRID) == msgs(grid, "mi_interp2_grid_f64_dev") and len(msgs(new, GRID)) == 4
    assert msgs(new, SLICES) == msgs(slices, "mi_interp2_slices_f64_dev") and len(msgs(new, SLICES)) == 3
    host = msgs(grid, "mi_interp2_grid_f64_host")
    assert msgs(new, GRID_H)[:3] == host[:3]


def test_kernels_are_in_the_code_object_and_use_no_scratch(tmp_path):
    """two scattered kernels, one locate, two gridded tile, two gridded flat and three slices kernels under the new
    namespace, all with a zero private segment and no LDS; the kernel counts of the linear twins are what they were"""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf not found")
    _build.build_lib()
    work = tmp_path / "co"
    work.mkdir()
    shutil.copy(_build.LIB_PATH, work / "lib.so")                       # (--offloading writes the bundles next to its input)
    out = subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=work, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    mine = tnb._kernels(work, "mi_nearest2")
    names = [n for n, _, _, _ in mine]
    for part, count in (("nearest2_kernel", 2), ("nearest2_locate_kernel", 1), ("nearest2_grid_tile_kernel", 2),
                        ("nearest2_grid_flat_kernel", 2), ("nearest2_slices_kernel", 3)):
        assert sum(part in n for n in names) == count, (part, names)
    assert len(names) == 10, names
    print({n: v for n, _, _, v in mine})                               # VGPR counts
    assert all(private == 0 and lds == 0 for _, private, lds, _ in mine), mine
    assert all(v <= 64 for _, _, _, v in mine), mine                    # eight waves per SIMD everywhere
    assert len(tnb._kernels(work, "mi_slices2")) == 7 and len(tnb._kernels(work, "mi_nearest_batched")) == 9


# ---- C++ ----------------------------------------------------------------------------------------------------------------

def test_cpp_overloads_resolve_with_the_compat_shim(tmp_path):
    """compile only: interp2(..., ZI, "nearest"), (..., ZI, 0), (..., ZI, 0.0), (..., ZI) and the same on an arma::vec ZI
    each name exactly one overload -- a literal 0 is an extrapolation value, not a null method"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "ov.cpp"
    src.write_text('#include "mi355_arma.hpp"\n'
                   "void f(const arma::vec& X, const arma::vec& Y, const arma::mat& Z, const arma::vec& XI, const arma::vec& YI,\n"
                   "       arma::mat& ZI, arma::vec& ZV, mi355::Device& dev) {\n"
                   '  mi355::interp2(X, Y, Z, XI, YI, ZI, "nearest");\n'
                   '  mi355::interp2(X, Y, Z, XI, YI, ZI, "nearest", -7.5);\n'
                   '  mi355::interp2(X, Y, Z, XI, YI, ZI, "linear", 0.0, dev);\n'
                   "  mi355::interp2(X, Y, Z, XI, YI, ZI, 0);\n"
                   "  mi355::interp2(X, Y, Z, XI, YI, ZI, 0L, dev);\n"
                   "  mi355::interp2(X, Y, Z, XI, YI, ZI, 0.0);\n"
                   "  mi355::interp2(X, Y, Z, XI, YI, ZI);\n"
                   "  mi355::interp2(X, Y, Z, XI, YI, ZV, 0);\n"
                   "  mi355::interp2(X, Y, Z, XI, YI, ZV, 0.0);\n"
                   "  mi355::interp2(X, Y, Z, XI, YI, ZV);\n"
                   "  arma::vec V; mi355::interp1(X, Y, XI, V, 0); mi355::interp1(X, Y, XI, V, \"nearest\");\n"
                   "}\n")
    host = os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "host")
    out = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", host, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    text = open(os.path.join(INCLUDE, "mi355_arma.hpp")).read()
    assert 'throw std::invalid_argument("interp2(): unsupported interpolation type")' in text
    assert "mi_interp2_grid_nearest_f64_host" in text and text.index("mi355::interp2(X, Y, Z, XI, YI, ZI, method)") < text.index("#pragma once")
    mk = open(os.path.join(host, "Makefile")).read()
    assert re.search(r"^arma_interp2_nearest_test:", mk, flags=re.M) and "arma_interp2_nearest_test" in mk[mk.index("all:"):mk.index("driver:")]
    assert "host/arma_interp2_nearest_test\n" in open(os.path.join(ROOT, ".gitignore")).read()
