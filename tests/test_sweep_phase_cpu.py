"""CPU checks of the seam that lets the region sweep's headline kernel be restated outside the pinned interp1 sources
(csrc/mi_sweep_phase.hip): mi_interp1.hip is compiled with its two exported names renamed (_build.PER_SOURCE_FLAGS) and
the new unit defines the names themselves.  The pinned files stay what they were; the new unit adds arithmetic of its
own nowhere, reads the environment only for its one switch and the family's four hooks, and never waits for another
workgroup."""
import ctypes
import os
import re

from armadillocudalinearinterpolation_amd import _build, _lib
import test_interp1_cols_cpu as pinned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "mi_sweep_phase.hip"
BASE = ["mi_interp1_f64_dev_v2_base", "mi_debug_sweep_ds_launches_base"]
NEW = BASE + ["mi_debug_interp1_phased_sweep"]


def _header():
    return open(os.path.join(ROOT, "include", "mi355_interp.h")).read()


def _unit():
    return open(os.path.join(_build.CSRC, UNIT)).read()


def _code(text):
    """the unit without its comments"""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_base_names_exported_declared_additive_and_bound():
    raw = _header()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_build.build_lib())
    additive = raw[raw.index("additive in 4"):raw.index("#define MI355_INTERP_ABI_VERSION")]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in additive, name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"^mi_status\s+mi_interp1_f64_dev_v2_base\s*\(", text, flags=re.M)
    assert re.search(r"^size_t\s+mi_debug_sweep_ds_launches_base\s*\(\s*void\s*\)\s*;", text, flags=re.M)
    assert re.search(r"^mi_status\s+mi_debug_interp1_phased_sweep\s*\(", text, flags=re.M)
    S = _lib.SIGNATURES
    assert S["mi_interp1_f64_dev_v2_base"] == S["mi_interp1_f64_dev_v2"] == S["mi_interp1_f64_dev"]
    assert S["mi_debug_sweep_ds_launches_base"] == S["mi_debug_sweep_ds_launches"] == (ctypes.c_size_t, [])
    assert S["mi_debug_interp1_phased_sweep"] == (ctypes.c_int, S["mi_interp1_f64_dev"][1] + [ctypes.c_int, ctypes.c_int])
    # the exported names are still there, and both counters start at 0
    assert hasattr(lib, "mi_interp1_f64_dev_v2") and hasattr(lib, "mi_debug_sweep_ds_launches")
    for name in ("mi_debug_sweep_ds_launches", "mi_debug_sweep_ds_launches_base"):
        getattr(lib, name).restype = ctypes.c_size_t
        assert getattr(lib, name)() == 0


def test_abi_version_stays_4():
    assert "#define MI355_INTERP_ABI_VERSION 4" in _header()
    assert ctypes.CDLL(_build.build_lib()).mi_abi_version() == 4


def test_new_unit_is_built_outside_the_stamped_families_which_are_what_they_were():
    assert UNIT in [os.path.basename(p) for p in _build.sources()]
    assert not any(UNIT.startswith("mi_" + f) for f in pinned.FAMILY_HASH)
    for family, digest in pinned.FAMILY_HASH.items():
        assert _build.source_hash(family) == digest, family


def test_interp1_unit_is_compiled_with_the_two_renames():
    flags = _build.PER_SOURCE_FLAGS["mi_interp1.hip"]
    assert "-Dmi_interp1_f64_dev_v2=mi_interp1_f64_dev_v2_base" in flags
    assert "-Dmi_debug_sweep_ds_launches=mi_debug_sweep_ds_launches_base" in flags
    assert _build.PER_SOURCE_FLAGS["mi_edm.hip"] == ["-fno-slp-vectorize"]           # (what was there stays)


def test_null_arguments_reach_the_family_with_its_message_texts():
    """the wrapper forwards what it does not take: the errors are mi_interp1.hip's, before any device call"""
    L = _lib.load()
    assert L.mi_interp1_f64_dev_v2(None, None, None, None, 5, 0.0) == 1
    assert "mi_interp1_f64_dev: NULL context or grid" in L.mi_last_error(None).decode()
    assert L.mi_interp1_f64_dev_v2_base(None, None, None, None, 5, 0.0) == 1
    assert L.mi_debug_interp1_phased_sweep(None, None, None, None, 5, 0.0, 2, 8) == 1
    assert "mi_debug_interp1_phased_sweep" in L.mi_last_error(None).decode()


def test_new_unit_adds_no_arithmetic_no_other_switch_and_no_wait_between_workgroups():
    code = _code(_unit())
    assert '#include "mi_interp1_sweep.hpp"' in code
    assert "eval_batch" not in code                                              # the blend comes in through the header's helpers only
    assert "pipe_gather_rounds<0, FORMULA>" in code and "pipe_tail<0, FORMULA>" in code
    assert not re.search(r"\bfma[fl]?\s*\(", code) and "__fma" not in code
    # the environment: the one switch, and the presence of the family's four hooks
    assert sorted(re.findall(r'getenv\("(\w+)"\)', code)) == sorted(
        ["MI_SWEEP_XCD_PHASES", "MI_SWEEP_MIN_BYTES", "MI_SWEEP_MIN_TILES_PER_CU", "MI_SWEEP_VARIANT", "MI_SWEEP_DEFER"])
    assert len(re.findall(r"\bgetenv\b", code)) == 5
    # atomics: the two LDS counters of the parent kernel (histogram tickets, the group's arrival counter) and nothing on
    # global memory -- no flag, ticket or counter that one workgroup could wait on
    targets = re.findall(r"\batomic\w*\s*\(\s*&?\s*(\w+)", code)
    assert sorted(set(targets)) == ["gbar", "myhist"], targets
    assert re.search(r"__shared__\s+unsigned\s+hist\[2\]\[kSweepBins\]", code) and re.search(r"__shared__\s+unsigned\s+gbar\[2\]", code)
    assert "myhist = hist[grp]" in code
    assert "__hip_atomic" not in code and "__atomic" not in code and "__threadfence" not in code and "cooperative" not in code
    # the waits: the group's LDS counter, and the clock wait, which is bounded by a poll count
    loops = [ln.strip() for ln in code.splitlines() if re.search(r"\b(while|do)\b", ln)]
    assert loops == ["while (*(lds_vu32*)&gbar[grp] < gb_target) __builtin_amdgcn_s_sleep(2);"], loops
    assert re.search(r"for\s*\(int poll = 0; poll < kPhaseWaitPolls && wall_clock64\(\) - t0 < want; \+\+poll\)", code)
    kernels = re.findall(r"__global__(?:(?!__global__)[^;{])*?\bvoid\s+(\w+)\s*\(", code)
    assert kernels == ["interp1_phased_sweep_kernel"]
