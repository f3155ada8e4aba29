"""CPU checks of the deferred-store region sweep (interp1_sweep_pipe_kernel<MODE, FORMULA, DEFER>, csrc/mi_interp1_sweep.hpp;
dispatch in csrc/mi_interp1.hip): its entry point is declared, bound and exported under the unchanged ABI version, the
pipelined kernel exists once, and no committed traffic figure is stamped with the sources it lives in."""
import ctypes
import glob
import json
import os
import re

from armadillocudalinearinterpolation_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355_interp.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_build.build_lib())
    assert re.search(r"^mi_status\s+mi_interp1_f64_dev_v2\s*\(", text, flags=re.M)
    assert re.search(r"^size_t\s+mi_debug_sweep_ds_launches\s*\(\s*void\s*\)", text, flags=re.M)
    assert hasattr(lib, "mi_interp1_f64_dev_v2") and hasattr(lib, "mi_debug_sweep_ds_launches")
    # the same contract as mi_interp1_f64_dev: (ctx, grid, xq, yq, nq, extrap)
    assert _lib.SIGNATURES["mi_interp1_f64_dev_v2"] == _lib.SIGNATURES["mi_interp1_f64_dev"]
    assert _lib.SIGNATURES["mi_debug_sweep_ds_launches"] == (ctypes.c_size_t, [])
    assert lib.mi_abi_version() == 4          # additive: the version stays
    lib.mi_debug_sweep_ds_launches.restype = ctypes.c_size_t
    assert lib.mi_debug_sweep_ds_launches() == 0


def test_one_pipelined_kernel_and_no_orphaned_interp1_profile():
    assert not os.path.exists(os.path.join(_build.CSRC, "mi_sweep_ds.hip"))
    text = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(_build.CSRC, "*.h*"))))
    kernels = re.findall(r"__global__(?:(?!__global__)[^;{])*?\bvoid\s+(\w+)\s*\(", text)
    assert len(kernels) > 10                                     # (the pattern sees the library's kernels)
    assert [k for k in kernels if "sweep_pipe_kernel" in k] == ["interp1_sweep_pipe_kernel"]
    assert not [k for k in kernels if "sweep_ds_kernel" in k]
    # the kernel lives in the stamped interp1 sources, so their digest moves with it: no quoted figure may depend on it
    # (an entry without "family" is an interp1 entry: scripts/parse_rocprof.py)
    entries = json.load(open(os.path.join(ROOT, "profiles", "traffic_latest.json")))
    assert entries and all(e.get("family", "interp1") != "interp1" for e in entries.values())


def test_python_hot_path_calls_the_new_entry_point():
    api = open(os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "api.py")).read()
    assert "mi_interp1_f64_dev_v2(" in api and "mi_interp1_f64_dev(" not in api
