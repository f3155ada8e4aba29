"""CPU checks of csrc/mi_paired_cols.hpp, the one copy of the device helpers mi_pairs1.hip and mi_each1.hip share: both
units include it and define none of the shared pieces themselves, the header defines each of them once and no kernel,
and it lies outside the stamped kernel families (whose digests are what test_interp1_cols_cpu.py pins).  The blend, the
validation pass and the host side (check_args, copy_cols, the unit cut, the chunked host call) are still one copy per
unit; each host entry point names its own error-path hook."""
import os
import re

from armadillocudalinearinterpolation_amd import _build
from test_interp1_cols_cpu import FAMILY_HASH

HEADER = "mi_paired_cols.hpp"
UNITS = ("mi_pairs1.hip", "mi_each1.hip")
# name -> what its definition looks like (a use of skew( or search( is not one)
RET = r"\b(?:void|bool|int|size_t|double)\s+"
SHARED = {
    "struct ColLoad": r"\bstruct\s+ColLoad\b",
    "struct LdsX": r"\bstruct\s+LdsX\b",
    "col_issue": RET + r"col_issue\s*\(",
    "col_commit": RET + r"col_commit\s*\(",
    "vec_bad": RET + r"vec_bad\s*\(",
    "col_len": RET + r"col_len\s*\(",
    "search(": RET + r"search\s*\(",
    "skew(": RET + r"skew\s*\(",
    "x_stride(": RET + r"x_stride\s*\(",
    "lds_bytes_for(": RET + r"lds_bytes_for\s*\(",
    "kQIter": r"\bconstexpr\s+\w+\s+kQIter\b",
    "kPrefetch": r"\bconstexpr\s+\w+\s+kPrefetch\b",
}


def _code(name):
    return re.sub(r"//.*", "", open(os.path.join(_build.CSRC, name)).read())


def test_both_units_include_the_header():
    assert os.path.exists(os.path.join(_build.CSRC, HEADER))
    for unit in UNITS:
        assert '#include "%s"' % HEADER in _code(unit), unit


def test_the_shared_pieces_are_defined_once_in_the_header():
    header = _code(HEADER)
    for what, pattern in SHARED.items():
        assert len(re.findall(pattern, header)) == 1, what
        for unit in UNITS:
            assert not re.search(pattern, _code(unit)), (unit, what)
    assert "__global__" not in header                                 # the kernels, and their names, stay in the units
    assert "namespace mi_paired" in header
    assert "atomic" not in open(os.path.join(_build.CSRC, HEADER)).read().lower()   # as mi_pairs1.hip: flags are plain stores
    assert "double weight(" not in header                             # the units blend with mi_interp2::weight, as it is


def test_the_header_is_outside_the_stamped_families():
    assert not any(HEADER.startswith("mi_" + f) for f in FAMILY_HASH)
    assert HEADER not in ("mi_common.hpp", "mi_ctx.hip")
    assert os.path.join(_build.CSRC, HEADER) in _build._deps()        # a change to it rebuilds the library
    assert {f: _build.source_hash(f) for f in FAMILY_HASH} == FAMILY_HASH


def test_each_host_entry_point_names_its_own_hook():
    assert 'getenv("MI_TEST_FAIL_PAIRS_CHUNK")' in _code("mi_pairs1.hip")
    assert 'getenv("MI_TEST_FAIL_EACH_CHUNK")' in _code("mi_each1.hip")
