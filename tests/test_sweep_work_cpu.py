"""CPU checks of the ownership function of the region sweep's shift by work (csrc/mi_sweep_partition.hpp, walked through
mi_debug_sweep_partition: the function the kernel itself calls, no device involved).

Units are 4096 queries.  For nwg workgroups, P phase classes and a first-tile table, and for U = nq / 4096 whole units:
  1. the tiles of all workgroups cover [0, U) exactly once (so with the nq % 4096 queries of the tail, [0, nq));
  2. the work w_s of rank s is U / nwg, one more below rank U % nwg (ranks are (class, blockIdx), class = blockIdx % P);
  3. the first tile of a class-c workgroup has min(table[c], w_s) units, every tile between first and last 4, the last
     1..4, and no workgroup has more than ceil(w_s / 4) + 1 tiles;
  4. workgroups with equal blockIdx % 8 (one XCD) have the same unit count at every tile index but their last;
  5. the tiles of one step (tile index) lie in one span of the arrays that holds no tile of another step, in rank order;
     a step in which every workgroup has a full tile that is not its last puts rank s at (start of the span) + 4 s.
Sizes: nwg 1, 7, 8, 16 with every U from 0 to 6 nwg, nwg 256 with U = 0, 5, 10, ... (5 is prime to 256: every residue of
U % nwg); every residue of nq % 4096 (the tail does not move a tile); the headline's 1e8 on 256.
The unit's text keeps what tests/test_sweep_phase_cpu.py pins: one kernel, five environment names, LDS atomics only."""
import ctypes
import os
import re

import numpy as np
import pytest

from armadillocudalinearinterpolation_amd import _build, _lib

UNIT_Q = 4096
TABLES = [(4, 4123), (4, 4321), (4, 1234), (2, 42), (2, 24), (1, 4), (1, 2)]
WORKGROUPS = (1, 7, 8, 16, 256)


@pytest.fixture(scope="module")
def fn():
    lib = ctypes.CDLL(_build.build_lib())
    f = lib.mi_debug_sweep_partition
    f.restype = ctypes.c_int
    # the out pointers as plain addresses into numpy arrays (the binding table has them typed: _lib.SIGNATURES)
    f.argtypes = [ctypes.c_size_t, ctypes.c_uint, ctypes.c_int, ctypes.c_uint, ctypes.c_uint] + [ctypes.c_void_p] * 9
    return f


def digits(table):
    return [int(c) for c in str(table)]


def ranks(nwg, P):
    """rank -> (class, blockIdx): ranks are ordered by (class, blockIdx)"""
    order = sorted(range(nwg), key=lambda b: (b % P, b))
    return np.array([b % P for b in order]), np.array(order)


def walk(fn, nq, nwg, P, table):
    u32 = np.zeros((3, nwg), dtype=np.uint32)
    u64 = np.zeros((6, nwg), dtype=np.uint64)
    a32, a64 = u32.ctypes.data, u64.ctypes.data
    for r in range(nwg):
        rc = fn(nq, nwg, P, table, r, a32 + 4 * r, a32 + 4 * (nwg + r), a32 + 4 * (2 * nwg + r), a64 + 8 * r, a64 + 8 * (nwg + r),
                a64 + 8 * (2 * nwg + r), a64 + 8 * (3 * nwg + r), a64 + 8 * (4 * nwg + r), a64 + 8 * (5 * nwg + r))
        assert rc == 0
    return u32.astype(np.int64), u64.astype(np.int64)


def check(fn, nq, nwg, P, table):
    what = (nq, nwg, P, table)
    (nt, fu, lu), (work, fs, mo, ms, ps, ls) = walk(fn, nq, nwg, P, table)
    U = nq // UNIT_Q
    cls, block = ranks(nwg, P)
    rank = np.arange(nwg)
    first_want = np.array(digits(table))[cls]
    # 2: shares
    assert np.array_equal(work, U // nwg + (rank < U % nwg)), what
    # 3: the cut of a share
    assert np.array_equal(fu, np.minimum(first_want, work)), what
    assert np.array_equal(nt == 0, work == 0), what
    has = nt > 0
    assert np.all((lu[has] >= 1) & (lu[has] <= 4)), what
    assert np.all(nt <= (work + 3) // 4 + 1), what
    one = nt == 1
    assert np.array_equal(lu[one], fu[one]) and np.array_equal(fu[one], work[one]) and np.array_equal(ls[one], fs[one]), what
    more = nt >= 2
    assert np.array_equal(fu[more] + 4 * (nt[more] - 2) + lu[more], work[more]), what
    # every tile of every workgroup: (rank, tile index, start, units), by the rule the header states
    T = int(nt.sum())
    owner = np.repeat(rank, nt)
    idx = np.arange(T) - np.repeat(np.cumsum(nt) - nt, nt)
    n_of = nt[owner]
    start = np.where(idx == 0, fs[owner], np.where(idx == n_of - 1, ls[owner], np.where(idx == n_of - 2, ps[owner], mo[owner] + (idx - 1) * ms[owner])))
    units = np.where(idx == 0, fu[owner], np.where(idx == n_of - 1, lu[owner], 4))
    # 1: exact cover, on unit boundaries by construction (starts are counted in units)
    by = np.argsort(start, kind="stable")
    s_sorted, u_sorted = start[by], units[by]
    if T:
        assert s_sorted[0] == 0 and np.array_equal(s_sorted[1:], s_sorted[:-1] + u_sorted[:-1]) and s_sorted[-1] + u_sorted[-1] == U, what
    else:
        assert U == 0, what
    # 4: one XCD, one unit count per tile index (last tiles apart)
    not_last = idx < n_of - 1
    for x in range(min(8, nwg)):
        sel = not_last & (block[owner] % 8 == x)
        for i in np.unique(idx[sel]):
            assert np.unique(units[sel & (idx == i)]).size == 1, (what, x, i)
    # 5: a step's tiles in one span of their own, in rank order; a step of full inner tiles of everybody is a regular row
    step_sorted = idx[by]
    for i in np.unique(idx):
        pos = np.nonzero(step_sorted == i)[0]
        assert pos[-1] - pos[0] + 1 == pos.size, (what, i)                   # nothing of another step in between
        assert np.all(np.diff(owner[by][pos]) > 0), (what, i)                # rank order
        here = idx == i
        if i >= 1 and here.sum() == nwg and np.all(units[here] == 4) and np.all(not_last[here]):
            assert np.array_equal(start[here], start[here][0] + 4 * owner[here]), (what, i)
    return nt, units


@pytest.mark.parametrize("P,table", TABLES)
@pytest.mark.parametrize("nwg", WORKGROUPS)
def test_properties_over_every_share_residue(fn, nwg, P, table):
    tails = (0, 1, 4095, 2048)
    for k, U in enumerate(range(0, 6 * nwg + 1, 5 if nwg == 256 else 1)):
        check(fn, U * UNIT_Q + tails[k % 4], nwg, P, table)


@pytest.mark.parametrize("P,table", TABLES)
def test_the_tail_moves_no_tile(fn, P, table):
    """every residue of nq % 4096: what a rank owns is what it owns without the tail"""
    out = np.zeros((2, 12), dtype=np.uint64)
    args = [[out.ctypes.data + 96 * j + 8 * k for k in range(9)] for j in range(2)]
    for nwg in WORKGROUPS:
        for r in range(UNIT_Q):
            U = r % (6 * nwg + 1)
            rank = r % nwg
            out[:] = 0
            assert fn(U * UNIT_Q + r, nwg, P, table, rank, *args[0]) == 0
            assert fn(U * UNIT_Q, nwg, P, table, rank, *args[1]) == 0
            assert np.array_equal(out[0], out[1]), (nwg, P, table, r)


@pytest.mark.parametrize("P,table", TABLES)
def test_headline_shape(fn, P, table):
    """1e8 queries on 256 workgroups: 24414 units, 95 or 96 per workgroup; the tail of 256 queries is the last rank's"""
    nt, units = check(fn, 100_000_000, 256, P, table)
    assert nt.max() <= 25 and nt.min() >= 24
    assert units.sum() == 24414 and 100_000_000 - 24414 * UNIT_Q == 256


def test_bad_arguments_are_refused(fn):
    out = np.zeros(12, dtype=np.uint64)
    ptrs = [out.ctypes.data + 8 * k for k in range(9)]
    for nq, nwg, P, table, rank in ((1 << 20, 8, 8, 11111111, 0), (1 << 20, 8, 3, 444, 0), (1 << 20, 8, 4, 412, 0), (1 << 20, 8, 4, 41234, 0),
                                    (1 << 20, 8, 4, 4025, 0), (1 << 20, 8, 4, 4123, 8), (1 << 20, 0, 4, 4123, 0), (1 << 20, 8, 2, 45, 0)):
        assert fn(nq, nwg, P, table, rank, *ptrs) == 1, (nq, nwg, P, table, rank)
    assert fn(1 << 20, 8, 4, 4123, 7, *([None] * 9)) == 0                     # any out pointer may be NULL


def test_entry_points_are_declared_additive_and_bound():
    raw = open(os.path.join(_build.REPO_ROOT, "include", "mi355_interp.h")).read()
    additive = raw[raw.index("additive in 4"):raw.index("#define MI355_INTERP_ABI_VERSION")]
    lib = ctypes.CDLL(_build.build_lib())
    for name in ("mi_debug_sweep_partition", "mi_debug_interp1_phased_sweep_ex"):
        assert name in additive and name in _lib.SIGNATURES and hasattr(lib, name), name
    S = _lib.SIGNATURES
    assert S["mi_debug_interp1_phased_sweep_ex"] == (ctypes.c_int, S["mi_debug_interp1_phased_sweep"][1] + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32])
    assert "#define MI355_INTERP_ABI_VERSION 4" in raw and lib.mi_abi_version() == 4
    L = _lib.load()
    assert L.mi_debug_interp1_phased_sweep_ex(None, None, None, None, 5, 0.0, 4, 8, 4123, None, 0) == 1
    assert "mi_debug_interp1_phased_sweep_ex" in L.mi_last_error(None).decode()


def test_unit_text_one_kernel_five_environment_names_lds_atomics_only():
    text = open(os.path.join(_build.CSRC, "mi_sweep_phase.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    kernels = re.findall(r"__global__(?:(?!__global__)[^;{])*?\bvoid\s+(\w+)\s*\(", code)
    assert kernels == ["interp1_phased_sweep_kernel"]
    assert sorted(re.findall(r'getenv\("(\w+)"\)', code)) == sorted(
        ["MI_SWEEP_XCD_PHASES", "MI_SWEEP_MIN_BYTES", "MI_SWEEP_MIN_TILES_PER_CU", "MI_SWEEP_VARIANT", "MI_SWEEP_DEFER"])
    assert len(re.findall(r"\bgetenv\b", code)) == 5
    targets = re.findall(r"\batomic\w*\s*\(\s*&?\s*(\w+)", code)
    assert sorted(set(targets)) == ["gbar", "myhist"], targets
    assert "__hip_atomic" not in code and "__atomic" not in code and "__threadfence" not in code
    # the ownership is the header's one function, called by the kernel and by the export, and the header has no device call
    assert code.count("mi_sweep::sweep_partition<") == 2
    header = open(os.path.join(_build.CSRC, "mi_sweep_partition.hpp")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", header).lower() and "__host__ __device__" in header
    assert "pipe_gather_rounds<0, FORMULA>" in code and "pipe_tail<0, FORMULA>" in code and "eval_batch" not in code
