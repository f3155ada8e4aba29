"""CPU checks of interp1 over paired rows (mi_interp1_rowpairs_f64_dev, mi_debug_rowpairs_launches, mi.interp_rowpairs):
the entry points are declared, bound with the documented argument types and exported by the built library; the header
compiles in C; the new translation unit is built, lies outside the stamped kernel families and shares their weight code;
the kernels are in the gfx950 code object and use no scratch memory; the Python wrapper hands the library what it should
and refuses what it should, without a device."""
import ctypes
import glob
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from armadillocudalinearinterpolation_amd import _build, _lib, api
from test_api_calls_cpu import Env, _norm, cm, record, vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CALL = "mi_interp1_rowpairs_f64_dev"
COUNT = "mi_debug_rowpairs_launches"
SOURCE = "mi_rowpairs1.hip"
FAMILIES = ("interp1", "interp2", "edm")
# (x, ldx, y, ldy, m, n, len, xi, nxi, yi, ldyi, extrap, row_ok)
C_TAIL = ("const double*, size_t, const double*, size_t, size_t, size_t, const uint32_t*, const double*, size_t, double*, size_t, "
          "double, uint32_t*")


def _source():
    return open(os.path.join(_build.CSRC, SOURCE)).read()


def _header():
    whole = open(os.path.join(INCLUDE, "mi355_interp.h")).read()
    return whole, re.sub(r"/\*.*?\*/", "", whole, flags=re.S)


def test_entry_points_declared_bound_and_exported():
    _, text = _header()
    lib = ctypes.CDLL(_build.build_lib())
    vp, sz, dbl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
    assert re.search(r"^mi_status\s+%s\s*\(" % CALL, text, flags=re.M)
    assert re.search(r"^size_t\s+%s\s*\(\s*int\s+form\s*\)\s*;" % COUNT, text, flags=re.M)
    # (ctx, x, ldx, y, ldy, m, n, len, xi, nxi, yi, ldyi, extrap, row_ok)
    assert _lib.SIGNATURES[CALL] == (ctypes.c_int, [vp, vp, sz, vp, sz, sz, sz, vp, vp, sz, vp, sz, dbl, vp])
    assert _lib.SIGNATURES[COUNT] == (sz, [ctypes.c_int])
    assert hasattr(lib, CALL) and hasattr(lib, COUNT)


def test_debug_hook_counts_nothing_for_unknown_forms():
    lib = ctypes.CDLL(_build.build_lib())
    fn = getattr(lib, COUNT)
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int]
    assert all(fn(f) == 0 for f in (-1, 2, 3, 100)) and all(fn(f) >= 0 for f in (0, 1))


def test_abi_version_stays_and_the_names_are_listed_as_additive():
    whole, text = _header()
    assert ctypes.CDLL(_build.build_lib()).mi_abi_version() == 4
    assert "#define MI355_INTERP_ABI_VERSION 4" in text
    additive = whole[whole.index("additive in 4"):whole.index("#define MI355_INTERP_ABI_VERSION")]
    assert CALL in additive and COUNT in additive


def test_header_block_states_the_scope():
    whole, _ = _header()
    block = whole[whole.index("---- interp1 over paired rows"):whole.index("mi_status " + CALL)]
    assert "Device form only" in block and "no host-pointer" in block
    assert "query vector per row" in block and "fp32" in block
    assert "Which call when" in block
    for other in ("mi_status mi_interp1_pairs_f64_dev", "mi_status mi_interp1_rows_f64_dev"):      # and the way here from there
        before = whole[:whole.index(other)]
        assert CALL in before[before.rindex("Which call when"):]


def test_header_compiles_in_c(tmp_path):
    src = tmp_path / "rowpairs.c"
    src.write_text('#include "mi355_interp.h"\n'
                   "typedef mi_status (*rowpairs_fn)(mi_ctx*, %s);\n"
                   "typedef size_t (*count_fn)(int);\n"
                   "int main(void) { rowpairs_fn a = mi_interp1_rowpairs_f64_dev; count_fn d = mi_debug_rowpairs_launches;\n"
                   "  return (a && d) ? 0 : 1; }\n" % C_TAIL)
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    out = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o",
                          str(tmp_path / "rowpairs.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_new_translation_unit_is_built_and_outside_the_stamped_families():
    names = [os.path.basename(p) for p in _build.sources()]
    assert SOURCE in names
    assert not any(SOURCE.startswith("mi_" + f) for f in FAMILIES)
    stamped = {f: _build.source_hash(f) for f in FAMILIES}
    # a family's hash is that of its own sources: the new file, present or not, takes no part in it
    for f in FAMILIES:
        h = hashlib.sha256()
        for p in sorted(_build._deps()):
            b = os.path.basename(p)
            if b == SOURCE or not (b.startswith("mi_" + f) or b in ("mi_common.hpp", "mi_ctx.hip")):
                continue
            h.update(b.encode())
            h.update(open(p, "rb").read())
        assert h.hexdigest() == stamped[f], f
    # the names the other files' tests count kernels by do not occur in this file's name, namespace or kernel names
    text = _source()
    code = re.sub(r"//.*", "", text)
    assert "namespace mi_rowpairs1" in code
    for other in ("mi_rows1", "mi_pairs1", "mi_each1", "mi_cols1", "mi_slices2"):
        assert other not in SOURCE and other not in code, other
    assert set(re.findall(r"\b(\w+_kernel)\b", code)) == {"rowpairs1_validate_kernel", "rowpairs1_march_kernel"}


def test_source_shares_the_weight_and_rounds_every_operation():
    text = _source()
    code = re.sub(r"//.*", "", text)
    assert '#include "mi_interp2_eval.hpp"' in text
    assert "mi_interp2::weight(" in code and "double weight(" not in code          # used as it is, not copied
    assert "fma(" not in code and "__fma" not in code
    assert "-ffp-contract=off" in _build.HIPCC_FLAGS and SOURCE not in _build.PER_SOURCE_FLAGS


def test_the_form_limit_is_readable():
    thin = re.search(r"^constexpr size_t kThinN = (\d+);", _source(), flags=re.M)
    assert thin and int(thin.group(1)) >= 2


def test_kernels_are_in_the_code_object_and_use_no_scratch(tmp_path):
    """one validation kernel and two march kernels (short rows, long rows) are in the library's gfx950 code object, all
    with a zero private segment, no LDS and few enough registers for eight waves per SIMD"""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf not found")
    _build.build_lib()
    work = tmp_path / "co"
    work.mkdir()
    shutil.copy(_build.LIB_PATH, work / "lib.so")                       # (--offloading writes the bundles next to its input)
    out = subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=work, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    mine = []
    for b in glob.glob(str(work / "lib.so.*gfx950")):
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", b], capture_output=True, text=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count", notes):
            name = re.search(r"\.name:\s*(\S*mi_rowpairs1\S*)", block)
            if name:
                mine.append((name.group(1), int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)),
                             int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)),
                             int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1))))
    names = [n for n, _, _, _ in mine]
    assert sum("rowpairs1_validate_kernel" in n for n in names) == 1, names
    assert sum("rowpairs1_march_kernelILb1E" in n for n in names) == 1, names       # THIN = true: short rows
    assert sum("rowpairs1_march_kernelILb0E" in n for n in names) == 1, names       # long rows
    assert len(names) == 3, names
    assert all(private == 0 for _, private, _, _ in mine), mine
    assert all(lds == 0 for _, _, lds, _ in mine), mine
    assert all(v <= 64 for _, _, _, v in mine), mine


def test_python_function_is_exported():
    import armadillocudalinearinterpolation_amd as mi
    assert callable(mi.interp_rowpairs) and mi.interp_rowpairs is api.interp_rowpairs
    assert CALL in mi.interp_rowpairs.__doc__


# ---- what the wrapper hands to the library, and what it refuses (the stand-ins of test_api_calls_cpu.py) --------------

ACCEPTED = {
    "dense": (lambda e: api.interp_rowpairs(e.ctx, e.t("X", cm(5, 7)), e.t("Y", cm(5, 7)), e.t("xi", vec(4)), out=e.t("out", cm(5, 4))),
              ("ctx", "X", 5, "Y", 5, 5, 7, None, "xi", 4, "out", 5, "nan", None), [((5, 4), (1, 5))]),
    "padded_lens_ok": (lambda e: api.interp_rowpairs(e.ctx, e.t("X", cm(5, 7, ld=9)), e.t("Y", cm(5, 7, ld=6)), e.t("xi", vec(4)),
                                                     lens=e.t("lens", vec(5, np.int32)), out=e.t("out", cm(5, 4, ld=8)),
                                                     extrap=0.25, want_ok=True),
                       ("ctx", "X", 9, "Y", 6, 5, 7, "lens", "xi", 4, "out", 8, 0.25, "second"), [((5, 4), (1, 8)), ((5,), (1,))]),
    "default_out": (lambda e: api.interp_rowpairs(e.ctx, e.t("X", cm(5, 7, ld=9)), e.t("Y", cm(5, 7)), e.t("xi", vec(4))),
                    ("ctx", "X", 9, "Y", 5, 5, 7, None, "xi", 4, "out", 5, "nan", None), [((5, 4), (1, 5))]),
    "single_row_one_query": (lambda e: api.interp_rowpairs(e.ctx, e.t("X", cm(1, 7)), e.t("Y", cm(1, 7)), e.t("xi", vec(1)),
                                                           out=e.t("out", cm(1, 1))),
                             ("ctx", "X", 1, "Y", 1, 1, 7, None, "xi", 1, "out", 1, "nan", None), [((1, 1), (1, 1))]),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_accepted_call_reaches_the_library_unchanged(case):
    build, args, layouts = ACCEPTED[case]
    assert record(build) == ([(CALL, args)], layouts)


def _rp(e, X=None, Y=None, xi=None, **kw):
    return api.interp_rowpairs(e.ctx, X if X is not None else e.t("X", cm(5, 7)), Y if Y is not None else e.t("Y", cm(5, 7)),
                               xi if xi is not None else e.t("xi", vec(4)), **kw)


ROWMAJOR = "%s must be column-major (the .T view of a contiguous (%d, m) buffer)"
REJECTED = {
    "xi_float32": (lambda e: _rp(e, xi=e.t("xi", vec(4, np.float32))), "xi must be a contiguous float64 CUDA tensor"),
    "xi_before_x": (lambda e: _rp(e, X=e.t("X", cm(5, 7, dtype=np.float32)), xi=e.t("xi", vec(8)[::2])),
                    "xi must be a contiguous float64 CUDA tensor"),
    "x_float32": (lambda e: _rp(e, X=e.t("X", cm(5, 7, dtype=np.float32))), "X and Y must be float64 CUDA tensors"),
    "y_host": (lambda e: _rp(e, Y=e.t("Y", cm(5, 7), cuda=False)), "X and Y must be float64 CUDA tensors"),
    "shapes_differ": (lambda e: _rp(e, Y=e.t("Y", cm(5, 8))), "X and Y must both have shape (m, n)"),
    "one_dim": (lambda e: _rp(e, X=e.t("X", vec(7)), Y=e.t("Y", vec(7))), "X and Y must both have shape (m, n)"),
    "x_c_ordered": (lambda e: _rp(e, X=e.t("X", np.zeros((5, 7)))), ROWMAJOR % ("X", 7)),
    "y_c_ordered": (lambda e: _rp(e, Y=e.t("Y", np.zeros((5, 7)))), ROWMAJOR % ("Y", 7)),
    "lens_float": (lambda e: _rp(e, lens=e.t("lens", vec(5))), "lens must be a contiguous int32 CUDA tensor of shape (m,)"),
    "lens_count": (lambda e: _rp(e, lens=e.t("lens", vec(7, np.int32))), "lens must be a contiguous int32 CUDA tensor of shape (m,)"),
    "lens_before_out": (lambda e: _rp(e, lens=e.t("lens", vec(4, np.int32)), out=e.t("out", cm(5, 4), cuda=False)),
                        "lens must be a contiguous int32 CUDA tensor of shape (m,)"),
    "out_float32": (lambda e: _rp(e, out=e.t("out", cm(5, 4, dtype=np.float32))), "out must be a float64 CUDA tensor"),
    "out_columns": (lambda e: _rp(e, out=e.t("out", cm(5, 3))), "out must have shape (m, 4)"),
    "out_c_ordered": (lambda e: _rp(e, out=e.t("out", np.zeros((5, 4)))), ROWMAJOR % ("out", 4)),
    "out_rows": (lambda e: _rp(e, out=e.t("out", cm(6, 4))), "out must have as many rows as Y"),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejected_call_names_the_rule_and_reaches_nothing(case):
    build, message = REJECTED[case]
    e = Env()
    with pytest.raises(ValueError) as err:
        build(e)
    assert str(err.value) == message
    assert [(name, tuple(_norm(a, e.names) for a in args)) for name, args in e.L.calls] == []
