"""CPU checks of interp1 along the rows of a matrix (mi_interp1_rows_f64_dev, mi_debug_rows1_launches, Axis1.interp_rows,
Axis1.interp_stack): the entry points are declared, bound with the documented argument types and exported by the built
library; the header compiles in C; the new translation unit is built, lies outside the stamped kernel families and shares
their locate code; the kernels are in the gfx950 code object and use no scratch memory; the Python wrappers' layout rules
need no device."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from armadillocudalinearinterpolation_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
ROWS = "mi_interp1_rows_f64_dev"
COUNT = "mi_debug_rows1_launches"
FAMILIES = ("interp1", "interp2", "edm")
# (y, ldy, m, xi, nxi, yi, ldyi, extrap)
C_TAIL = "const double*, size_t, size_t, const double*, size_t, double*, size_t, double"


def _source():
    return open(os.path.join(_build.CSRC, "mi_rows1.hip")).read()


def test_entry_points_declared_bound_and_exported():
    whole = open(os.path.join(INCLUDE, "mi355_interp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    lib = ctypes.CDLL(_build.build_lib())
    vp, sz, dbl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
    assert re.search(r"^mi_status\s+%s\s*\(" % ROWS, text, flags=re.M)
    assert _lib.SIGNATURES[ROWS] == (ctypes.c_int, [vp, vp, vp, sz, sz, vp, sz, vp, sz, dbl])      # (ctx, axis, ...)
    assert _lib.SIGNATURES[ROWS] == _lib.SIGNATURES["mi_interp1_cols_f64_dev"]                     # the same argument list
    assert hasattr(lib, ROWS)
    assert re.search(r"^size_t\s+%s\s*\(\s*int\s+form\s*\)\s*;" % COUNT, text, flags=re.M)
    assert _lib.SIGNATURES[COUNT] == (sz, [ctypes.c_int])
    fn = getattr(lib, COUNT)
    fn.restype, fn.argtypes = sz, [ctypes.c_int]
    assert fn(-1) == 0 and fn(3) == 0 and all(fn(f) >= 0 for f in range(3))      # unknown forms count nothing
    assert lib.mi_abi_version() == 4                                 # additive: the version stays
    assert "#define MI355_INTERP_ABI_VERSION 4" in text
    additive = whole[whole.index("additive in 4"):whole.index("#define MI355_INTERP_ABI_VERSION")]
    assert ROWS in additive and COUNT in additive
    assert "Which call when: one table per ROW, or interpolation across the slices of a cube -> this call" in whole
    block = whole[whole.index("interp1 along the rows of a matrix"):whole.index("mi_status " + ROWS)]
    assert "Device form only" in block and "no host-pointer" in block


def test_header_compiles_in_c(tmp_path):
    src = tmp_path / "rows.c"
    src.write_text('#include "mi355_interp.h"\n'
                   "typedef mi_status (*rows_fn)(mi_ctx*, const mi_axis1*, %s);\n"
                   "typedef size_t (*count_fn)(int);\n"
                   "int main(void) { rows_fn a = mi_interp1_rows_f64_dev; count_fn d = mi_debug_rows1_launches;\n"
                   "  return (a && d) ? 0 : 1; }\n" % C_TAIL)
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    out = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o",
                          str(tmp_path / "rows.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_new_translation_unit_is_built_and_outside_the_stamped_families():
    names = [os.path.basename(p) for p in _build.sources()]
    assert "mi_rows1.hip" in names
    assert not any("mi_rows1.hip".startswith("mi_" + f) for f in FAMILIES)
    stamped = {f: _build.source_hash(f) for f in FAMILIES}
    # a family's hash is that of its own sources: the new file, present or not, takes no part in it
    import hashlib
    for f in FAMILIES:
        h = hashlib.sha256()
        for p in sorted(_build._deps()):
            b = os.path.basename(p)
            if b == "mi_rows1.hip" or not (b.startswith("mi_" + f) or b in ("mi_common.hpp", "mi_ctx.hip")):
                continue
            h.update(b.encode())
            h.update(open(p, "rb").read())
        assert h.hexdigest() == stamped[f], f
    text = _source()
    assert '#include "mi_interp2_eval.hpp"' in text and '#include "mi_axis1.hpp"' in text
    code = re.sub(r"//.*", "", text)
    for shared in ("axis_record", "AxRec", "AxisDev"):               # the shared code, as it is
        assert shared in code, shared
    assert "fma(" not in code and "__fma" not in code                # the blend rounds every operation
    assert "namespace mi_rows1" in text
    assert "struct mi_axis1 {" not in text and "struct AxRec" not in text
    # the limits are written so that tests can read them
    rb = int(re.search(r"^constexpr size_t kRowBlock = (\d+);", text, flags=re.M).group(1))
    assert re.search(r"^constexpr size_t kThinM = kBlock;", text, flags=re.M)
    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(_build.CSRC, "mi_interp2_eval.hpp")).read()).group(1))
    assert block == 256 and rb == 4 * block                          # four rows per lane: 8 KiB of a column per workgroup
    assert stamped == {f: _build.source_hash(f) for f in FAMILIES}


def test_rows_kernels_are_in_the_code_object_and_use_no_scratch(tmp_path):
    """one locate kernel and three rows kernels (tile body with 16-B accesses, tile body with 8-B accesses, flat body) are
    in the library's gfx950 code object, all with a zero private segment and no LDS"""
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
            name = re.search(r"\.name:\s*(\S*mi_rows1\S*)", block)
            if name:
                mine.append((name.group(1), int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)),
                             int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)),
                             int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1))))
    names = [n for n, _, _, _ in mine]
    assert sum("rows1_locate_kernel" in n for n in names) == 1, names
    assert sum("rows1_tile_kernel" in n for n in names) == 2, names
    assert sum("rows1_flat_kernel" in n for n in names) == 1, names
    assert len(names) == 4, names
    assert all(private == 0 for _, private, _, _ in mine), mine
    assert all(lds == 0 for _, _, lds, _ in mine), mine
    # the 16-B tile kernel (ILb1E: VEC = true) fits eight workgroups per CU: at most 64 registers per lane
    assert all(v <= 64 for n, _, _, v in mine if "rows1_tile_kernelILb1E" in n), mine


def test_python_methods_exist():
    import armadillocudalinearinterpolation_amd as mi
    assert callable(mi.Axis1.interp_rows) and callable(mi.Axis1.interp_stack)
    assert "interp_rows" in mi.Axis1.__doc__ and "interp_stack" in mi.Axis1.__doc__


def test_rows_layout_rule_needs_no_device():
    """Y is (m, n), stored column-major with one table per row: the .T view of a C-contiguous (n, m) buffer"""
    from armadillocudalinearinterpolation_amd.api import Axis1
    view = Axis1._rows_view
    assert view(np.zeros((7, 5)).T, 7, "Y") == (5, 5)               # m = 5 rows, n = 7 columns, ld = m
    assert view(np.zeros((7, 9))[:, :5].T, 7, "Y") == (9, 5)        # a padded view: ld = 9
    assert view(np.zeros((7, 1)).T, 7, "Y") == (1, 1)               # a single row
    assert view(np.zeros((1, 5)).T, 1, "out") == (5, 5)             # a single column (nxi = 1)
    for bad, cols in ((np.zeros((5, 7)), 7),                         # C-ordered (m, n)
                      (np.zeros((7, 5)).T, 6),                       # wrong n
                      (np.zeros(7), 7),                              # 1-D
                      (np.zeros((7, 5, 2)), 5),
                      (np.zeros((7, 10))[:, ::2].T, 7)):             # rows two elements apart
        with pytest.raises(ValueError):
            view(bad, cols, "Y")

    class _Refuses:                                                  # the rule comes before any device call
        n = 7
        _rows_view = staticmethod(view)

        def __getattr__(self, name):
            raise AssertionError("touched %s before the layout was checked" % name)
    with pytest.raises(ValueError):
        Axis1.interp_rows(_Refuses(), np.zeros((5, 7)), None)


def test_stack_layout_rule_needs_no_device():
    """Z is (ny, nx, S) laid out like an arma::cube with dense slices; the slice stride may exceed ny*nx"""
    from armadillocudalinearinterpolation_amd.api import Axis1
    view = Axis1._stack_view
    assert view(np.zeros((4, 7, 5)).transpose(2, 1, 0), "Z") == (5, 7, 35, 4)            # ny = 5, nx = 7, 4 slices
    gap = np.lib.stride_tricks.as_strided(np.zeros(4 * 40), shape=(5, 7, 4), strides=(8, 5 * 8, 40 * 8))
    assert view(gap, "Z") == (5, 7, 40, 4)                                               # a padded slice stride
    padded_rows = np.zeros((4, 7, 8)).transpose(2, 1, 0)[:5]                             # ldz = 8 > ny = 5
    with pytest.raises(ValueError, match="ldz"):
        view(padded_rows, "Z")
    for bad in (np.zeros((5, 7, 4)), np.zeros((5, 7)), np.zeros(5)):                     # C order; not a cube
        with pytest.raises(ValueError):
            view(bad, "Z")
