"""CPU checks of the deferred-store region sweep (csrc/mi_sweep_ds.hip): its entry point is declared, bound and exported
under the unchanged ABI version, the new translation unit is built, and it lies outside the kernel families whose
sources the committed traffic profiles are stamped with."""
import ctypes
import os
import re

from armadillocudalinearinterpolation_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAMPED = ("mi_interp1", "mi_interp2", "mi_edm")


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


def test_new_translation_unit_is_built_and_outside_the_stamped_families():
    names = [os.path.basename(p) for p in _build.sources()]
    assert "mi_sweep_ds.hip" in names
    assert not "mi_sweep_ds.hip".startswith(STAMPED)
    before = _build.source_hash("interp1")
    text = open(os.path.join(_build.CSRC, "mi_sweep_ds.hip")).read()
    assert '#include "mi_interp1_sweep.hpp"' in text and "eval_batch" not in text.split("interp1_sweep_ds_kernel", 1)[0]
    assert "pipe_gather_rounds<MODE, FORMULA>" in text          # the gather rounds are the pipelined form's own
    assert _build.source_hash("interp1") == before


def test_python_hot_path_calls_the_new_entry_point():
    api = open(os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "api.py")).read()
    assert "mi_interp1_f64_dev_v2(" in api and "mi_interp1_f64_dev(" not in api
