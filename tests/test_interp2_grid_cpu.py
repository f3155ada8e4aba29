"""CPU checks of the gridded bilinear call (arma::interp2's XI x YI -> ZI form): the three entry points are declared,
bound and exported; the headers compile in C and in C++ (with the Armadillo stand-in) with the gridded overloads; and
moving the shared arithmetic into mi_interp2_eval.hpp left the scattered kernel's gfx950 code exactly as it was."""
import ctypes
import glob
import hashlib
import os
import re
import shutil
import subprocess

import pytest

from armadillocudalinearinterpolation_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ["mi_interp2_grid_f64_dev", "mi_interp2_grid_f64_host", "mi_group_interp2_grid_f64_host"]

# sha256 of the instruction text of interp2_kernel<true> / <false> (addresses and encodings dropped) as compiled from the
# parent commit's mi_interp2.hip with the library's flags
SCATTERED_ISA = {
    "_ZN10mi_interp214interp2_kernelILb1EEEv5G2DevPKdS3_Pdmd":
        "bcb853410f28105a5580af7f0e988d36e1a813d07b3543a306e0ed022ac21709",
    "_ZN10mi_interp214interp2_kernelILb0EEEv5G2DevPKdS3_Pdmd":
        "01f6551476767b4bd504659ea12aa2f4fddfede67560b8d1dbf16737a48f5fd3",
}


def test_entry_points_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "mi355_interp.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_build.build_lib())
    for name in NEW:
        assert re.search(r"^mi_status\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][1][3] is ctypes.c_size_t and _lib.SIGNATURES[name][1][5] is ctypes.c_size_t
    assert lib.mi_abi_version() == 4          # additive: the version stays


def test_header_compiles_in_c(tmp_path):
    src = tmp_path / "grid.c"
    src.write_text('#include "mi355_interp.h"\n'
                   "typedef mi_status (*grid_fn)(mi_ctx*, const mi_grid2*, const double*, size_t, const double*, size_t,\n"
                   "                             double*, double);\n"
                   "typedef mi_status (*group_fn)(mi_group*, const mi_group_grid2*, const double*, size_t, const double*,\n"
                   "                              size_t, double*, double);\n"
                   "int main(void) { grid_fn a = mi_interp2_grid_f64_dev, b = mi_interp2_grid_f64_host;\n"
                   "  group_fn c = mi_group_interp2_grid_f64_host; return (a && b && c) ? 0 : 1; }\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    out = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o",
                          str(tmp_path / "grid.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_arma_header_overloads_compile_with_the_stand_in(tmp_path):
    """with the stand-in arma::vec and arma::mat are unrelated types: each ZI type picks its overload"""
    src = tmp_path / "ovl.cpp"
    src.write_text('#include "mi355_arma.hpp"\n'
                   "#include <type_traits>\n"
                   "void (*grid)(const arma::vec&, const arma::vec&, const arma::mat&, const arma::vec&, const arma::vec&,\n"
                   "             arma::mat&, double, mi355::Device&) = mi355::interp2;\n"
                   "void (*scattered)(const arma::vec&, const arma::vec&, const arma::mat&, const arma::vec&,\n"
                   "                  const arma::vec&, arma::vec&, double, mi355::Device&) = mi355::interp2;\n"
                   "void (mi355::GroupInterp2Table::*gop)(const arma::vec&, const arma::vec&, arma::mat&, double) const =\n"
                   "    &mi355::GroupInterp2Table::operator();\n"
                   "int main() { return (grid && scattered && gop) ? 0 : 1; }\n")
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-DMI355_FORCE_ARMA_SHIM", "-I", INCLUDE,
                          "-c", str(src), "-o", str(tmp_path / "ovl.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def _isa(src, work):
    flags = [f for f in _build.HIPCC_FLAGS if f != "-shared"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc] + flags + ["-I", INCLUDE, "-I", _build.CSRC, "-c", src, "-o", str(work / "x.o")])
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", "x.o"], cwd=work, stdout=subprocess.DEVNULL)
    co = glob.glob(str(work / "x.o.*gfx950"))
    assert co, "no gfx950 code object"
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co[0]],
                         capture_output=True, text=True, check=True).stdout
    funcs, cur = {}, None
    for ln in txt.splitlines():
        m = re.match(r"^<(\S+)>:$", ln)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        ins = " ".join(ln.split("//")[0].split())
        if cur is not None and ins:
            cur.append(ins)
    return {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in funcs.items()}


def test_scattered_kernel_code_is_unchanged(tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("ROCm's llvm-objdump not found")
    got = _isa(os.path.join(_build.CSRC, "mi_interp2.hip"), tmp_path)
    for name, digest in SCATTERED_ISA.items():
        assert got.get(name) == digest, name
