"""CPU checks of gridded interp2 over the slices of a cube (mi_interp2_slices_f64_dev, mi_debug_slices2_launches): the
entry points are declared, bound with the documented argument types and exported by the built library; the header
compiles in C; the new translation unit is built, lies outside the stamped kernel families and shares their locate /
blend code; the Python wrapper's layout rule needs no device; the kernels use no scratch memory and their LDS fits."""
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
SLICES = ["mi_interp2_slices_f64_dev"]
FAMILIES = ("interp1", "interp2", "edm")
# (z, ldz, z_slice_stride, nslices, xi, nxi, yi, nyi, zi, ldzi, zi_slice_stride, extrap)
C_TAIL = "const double*, size_t, size_t, size_t, const double*, size_t, const double*, size_t, double*, size_t, size_t, double"


def _source():
    return open(os.path.join(_build.CSRC, "mi_slices2.hip")).read()


def test_entry_points_declared_bound_and_exported():
    whole = open(os.path.join(INCLUDE, "mi355_interp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    lib = ctypes.CDLL(_build.build_lib())
    vp, sz, dbl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
    tail = [vp, sz, sz, sz, vp, sz, vp, sz, vp, sz, sz, dbl]
    for name in SLICES:
        assert re.search(r"^mi_status\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in SLICES:                                              # (ctx, ax, ay, ...)
        assert _lib.SIGNATURES[name] == (ctypes.c_int, [vp, vp, vp] + tail), name
    assert re.search(r"^size_t\s+mi_debug_slices2_launches\s*\(\s*int\s+form\s*\)\s*;", text, flags=re.M)
    assert _lib.SIGNATURES["mi_debug_slices2_launches"] == (sz, [ctypes.c_int])
    fn = lib.mi_debug_slices2_launches
    fn.restype, fn.argtypes = sz, [ctypes.c_int]
    assert fn(-1) == 0 and fn(4) == 0 and all(fn(f) >= 0 for f in range(4))      # unknown forms count nothing
    assert lib.mi_abi_version() == 4                                 # additive: the version stays
    assert "#define MI355_INTERP_ABI_VERSION 4" in text
    additive = whole[whole.index("additive in 4"):whole.index("#define MI355_INTERP_ABI_VERSION")]
    assert all(name in additive for name in SLICES + ["mi_debug_slices2_launches"])
    assert "Which call when: one table that answers many calls -> mi_grid2" in whole


def test_python_names_are_exported():
    import armadillocudalinearinterpolation_amd as mi
    assert callable(mi.interp2_slices)


def test_wrapper_refuses_mismatched_shapes_before_any_device_call():
    """the layout rules need no device: Z is (ny, nx, S), stored slice by slice and column-major inside a slice"""
    from armadillocudalinearinterpolation_amd import api
    Z = np.zeros((5, 4, 3)).transpose(2, 1, 0)                       # (3, 4, 5): ny = 3, nx = 4, 5 slices
    assert api._cube_view(Z, 3, 4, "Z") == (3, 12, 5)
    padded = np.zeros((5, 6, 8)).transpose(2, 1, 0)[:3, :4]          # ldz = 8, slice stride 48
    assert api._cube_view(padded, 3, 4, "Z") == (8, 48, 5)
    assert api._cube_view(np.zeros((1, 4, 3)).transpose(2, 1, 0), 3, 4, "Z") == (3, 12, 1)
    for bad, rows, cols in ((Z, 4, 4), (Z, 3, 5), (np.zeros((3, 4)), 3, 4), (np.zeros((3, 4, 5)), 3, 4),
                            (np.zeros((5, 3, 4)).transpose(2, 0, 1), 4, 3)):          # C order; rows and columns swapped
        with pytest.raises(ValueError):
            api._cube_view(bad, rows, cols, "Z")


def test_header_compiles_in_c(tmp_path):
    src = tmp_path / "slices.c"
    src.write_text('#include "mi355_interp.h"\n'
                   "typedef mi_status (*slices_fn)(mi_ctx*, const mi_axis1*, const mi_axis1*, %s);\n"
                   "typedef size_t (*count_fn)(int);\n"
                   "int main(void) { slices_fn a = mi_interp2_slices_f64_dev; count_fn d = mi_debug_slices2_launches;\n"
                   "  return (a && d) ? 0 : 1; }\n" % C_TAIL)
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    out = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o",
                          str(tmp_path / "slices.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_new_translation_unit_is_built_and_outside_the_stamped_families():
    names = [os.path.basename(p) for p in _build.sources()]
    assert "mi_slices2.hip" in names
    for new in ("mi_slices2.hip", "mi_axis1.hpp"):
        assert not any(new.startswith("mi_" + f) for f in FAMILIES)
    stamped = {f: _build.source_hash(f) for f in FAMILIES}
    text = _source()
    assert '#include "mi_interp2_eval.hpp"' in text and '#include "mi_axis1.hpp"' in text
    code = re.sub(r"//.*", "", text)
    for shared in ("axis_record", "AxRec", "flagged_result", "blend_records", "AxisDev"):     # the shared code, as it is
        assert shared in code, shared
    assert "fma(" not in code and "__fma" not in code                # the blend is the header's, nothing is fused here
    assert "namespace mi_slices2" in text
    # the axis handle has one definition, shared with the columns call
    cols = open(os.path.join(_build.CSRC, "mi_cols1.hip")).read()
    assert "struct mi_axis1 {" not in cols and '#include "mi_axis1.hpp"' in cols
    assert "struct mi_axis1 {" in open(os.path.join(_build.CSRC, "mi_axis1.hpp")).read()
    # the limits are written so that tests can read them
    assert int(re.search(r"kLdsMaxElems = (\d+);", text).group(1)) == 8192
    assert re.search(r"kThinRows = kBlock;", text)
    assert stamped == {f: _build.source_hash(f) for f in FAMILIES}


def test_slices_kernels_use_no_scratch_and_fit_the_lds(tmp_path):
    """the locate kernel and the six slice kernels (LDS / direct x tile with 16-B stores, tile with 8-B stores, flat) are
    in the library's gfx950 code object with a zero private segment and no static LDS; the largest dynamic-LDS request
    of the LDS form fits the CU's 160 KiB"""
    text = _source()
    max_elems = int(re.search(r"kLdsMaxElems = (\d+);", text).group(1))
    assert 2 * max_elems * 8 <= 160 * 1024 - 16 * 1024               # two slice images, and room for the runtime's own
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
            name = re.search(r"\.name:\s*(\S*mi_slices2\S*)", block)
            if name:
                mine.append((name.group(1), int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)),
                             int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1))))
    names = [n for n, _, _ in mine]
    assert sum("slices2_locate_kernel" in n for n in names) == 1, names
    assert sum("slices2_kernel" in n for n in names) == 6, names
    assert not any("mi_cols1" in n for n in names), names
    assert all(private == 0 for _, private, _ in mine), mine
    assert all(static_lds == 0 for _, _, static_lds in mine), mine
