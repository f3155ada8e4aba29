"""CPU checks of arma::interp1's "nearest" method: the numpy restatement of the nearest rule (nearest_cases.nearest_rule,
the reference of tests/test_interp1_nearest_gpu.py) against a literal restatement of Armadillo's scan on every element of
every shared case; the one documented deviation; ties, the last node and a NaN node; the five new symbols declared,
exported and bound; NULL contexts refused before any device call; the launch shapes mi_nearest1.hip restates against
the files it restates them from."""
import ctypes
import os
import re

import numpy as np
import pytest

import interp1_value_cases as vc
import nearest_cases as nc
import oracle
import sweep_cases as sc

from armadillocudalinearinterpolation_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi_interp1_nearest_f64_dev", "mi_interp1_nearest_f64_host", "mi_interp1_nearest_f64",
       "mi_interp1_cols_nearest_f64_dev", "mi_debug_nearest_launches"]


@pytest.mark.parametrize("name", sorted(vc.SPECS))
def test_rule_equals_the_literal_scan_on_the_value_cases(name):
    """every (name, variant) of interp1_value_cases, every element: the picked node (which does not depend on Y) and,
    per variant, the values bit for bit"""
    X, xq = vc.nodes(name), vc.queries(name)
    k_rule, k_scan = nc.rule_index(X, xq), nc.scan_index(X, xq)
    assert np.array_equal(k_rule, k_scan)
    inr = k_rule >= 0
    l = np.searchsorted(X, xq[inr], side="right") - 1
    r = np.minimum(l + 1, X.size - 1)
    ties = np.count_nonzero((xq[inr] - X[l] == X[r] - xq[inr]) & (r > l))
    right = np.count_nonzero(k_rule[inr] == r)
    assert ties >= 100 and 0.3 < right / inr.sum() < 0.7          # the cases do exercise ties and both sides
    for variant in vc.VARIANTS:
        Y = vc.values(name, variant)
        ref = nc.nearest_rule(X, Y, xq, 4.5)
        assert nc._eq_bits(ref, nc.arma_nearest_scan(X, Y, xq, 4.5))
        assert nc._eq_bits(ref, nc._gather(Y, k_rule, 4.5))
        assert np.isnan(ref).any() and np.isinf(ref).any() and (np.signbit(ref) & (ref == 0)).any()


@pytest.mark.parametrize("name", sc.TABLES)
def test_rule_equals_the_literal_scan_on_the_sweep_tables(name):
    t = sc.table(name)
    xq = nc.sweep_queries(name)
    assert xq.size == nc.N_SWEEP_QUERIES == 33_007
    assert np.array_equal(nc.rule_index(t["X"], xq), nc.scan_index(t["X"], xq))
    assert nc._eq_bits(nc.nearest_rule(t["X"], t["Y"], xq, -2.0), nc.arma_nearest_scan(t["X"], t["Y"], xq, -2.0))


def test_the_plateau_is_the_one_deviation_from_the_scan():
    """X = [0, 2^-60, 1, 2], q = 1: 1 - 0 and 1 - 2^-60 round to the same double, so the scan stops at node 0; the rule
    returns the true nearest node"""
    X = np.array([0.0, 2.0 ** -60, 1.0, 2.0])
    Y = np.array([10.0, 11.0, 12.0, 13.0])
    q = np.array([1.0])
    assert (1.0 - X[0]) == (1.0 - X[1])
    assert nc.rule_index(X, q)[0] == 2 and nc.nearest_rule(X, Y, q)[0] == 12.0
    assert nc.scan_index(X, q)[0] == 0 and nc.arma_nearest_scan(X, Y, q)[0] == 10.0


def test_a_tie_keeps_the_left_node_and_the_last_node_is_itself():
    X = np.array([0.0, 1.0, 3.0, 4.0])
    Y = np.array([5.0, 6.0, 7.0, -0.0])
    q = np.array([0.5, 2.0, 3.5, 4.0, np.nextafter(0.5, 1.0), np.nextafter(2.0, 3.0), 0.0, np.nan, -1.0, 4.5])
    ref = np.array([5.0, 6.0, 7.0, -0.0, 6.0, 7.0, 5.0, np.nan, 9.0, 9.0])
    for fn in (nc.nearest_rule, nc.arma_nearest_scan):
        assert nc._eq_bits(fn(X, Y, q, 9.0), ref), fn.__name__
    assert not nc._eq_bits(np.array([0.0]), np.array([-0.0])) and nc._eq_bits(np.array([np.nan, 1.0]), np.array([np.nan, 1.0]))
    assert not nc._eq_bits(np.array([np.nan, 1.0]), np.array([1.0, np.nan]))


def test_a_nan_node_reaches_its_own_half_cells_only():
    """a NaN node at k makes NaN exactly the queries in (mid(k-1, k), mid(k, k+1)]; the linear blend
    (oracle.interp1_bracket) loses both whole cells -- nearest is not linear"""
    X = np.arange(10.0)
    Y = 1.0 + X
    k = 4
    Y[k] = np.nan
    q = np.arange(0.0, 9.0 + 1e-9, 0.125)                        # exact in binary, midpoints among them
    near = nc.nearest_rule(X, Y, q)
    assert np.array_equal(np.isnan(near), (q > 3.5) & (q <= 4.5))
    assert nc._eq_bits(near, nc.arma_nearest_scan(X, Y, q))
    lin = oracle.interp1_bracket(X, Y, q, np.nan)
    assert np.all(np.isnan(lin[(q > 3.0) & (q < 5.0)])) and not np.isnan(lin[(q < 3.0) | (q >= 5.0)]).any()
    assert np.count_nonzero(np.isnan(lin)) > np.count_nonzero(np.isnan(near))
    finite = ~np.isnan(near)
    assert np.all(np.isin(near[finite], Y[np.isfinite(Y)]))      # stored values only


def test_new_entry_points_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355_interp.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_build.build_lib())
    for name in NEW:
        assert re.search(r"^(?:mi_status|size_t)\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    S = _lib.SIGNATURES
    assert S["mi_interp1_nearest_f64_dev"] == S["mi_interp1_f64_dev"] and S["mi_interp1_nearest_f64_host"] == S["mi_interp1_f64_host"]
    assert S["mi_interp1_nearest_f64"] == S["mi_interp1_f64"]
    assert S["mi_interp1_cols_nearest_f64_dev"] == S["mi_interp1_cols_f64_dev"]
    assert S["mi_debug_nearest_launches"] == (ctypes.c_size_t, [ctypes.c_int])
    assert lib.mi_abi_version() == 4                               # additive: the version stays
    L = _lib.load()
    assert L.mi_debug_nearest_launches(-1) == 0 and L.mi_debug_nearest_launches(5) == 0    # no such form
    assert all(L.mi_debug_nearest_launches(f) >= 0 for f in range(5))


def test_a_null_context_is_refused_by_name_before_any_device_call():
    L = _lib.load()
    buf = (ctypes.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "mi_interp1_nearest_f64_dev": lambda: L.mi_interp1_nearest_f64_dev(None, p, p, p, 4, 0.0),
        "mi_interp1_nearest_f64_host": lambda: L.mi_interp1_nearest_f64_host(None, p, p, p, 4, 0.0),
        "mi_interp1_nearest_f64": lambda: L.mi_interp1_nearest_f64(None, p, p, 4, p, p, 4, 0.0),
        "mi_interp1_cols_nearest_f64_dev": lambda: L.mi_interp1_cols_nearest_f64_dev(None, p, p, 4, 1, p, 4, p, 4, 0.0),
    }
    for name, call in calls.items():
        assert L.mi_group_wait_stream(None, 0, None) == 1          # another refusal in between: the text must be this call's
        assert call() == 1, name
        msg = L.mi_last_error(None).decode()
        assert msg.startswith(name + ":") and "NULL" in msg, (name, msg)


def _const(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, name
    return re.sub(r"\s+", "", m.group(1))


def test_restated_launch_shapes_equal_the_linear_ones():
    """mi_nearest1.hip cannot include mi_interp1_stream.hpp (it defines a kernel that is no template) or mi_cols1.hip, so
    it restates their launch shapes and the LDS window; they must stay the same expressions.  It adds no environment
    hook, never touches the order probe's state, and lies outside the digest-stamped kernel families."""
    rd = lambda f: open(os.path.join(_build.CSRC, f)).read()  # noqa: E731
    near, stream, cols = rd("mi_nearest1.hip"), rd("mi_interp1_stream.hpp"), rd("mi_cols1.hip")
    for name in ("kBlock", "kVecVpl", "kLdsBlock", "kLdsMaxTableBytes", "kLdsMinTableBytes0", "kLdsMinTableBytes3",
                 "kLdsQueriesPerBlock"):
        assert _const(near, name) == _const(stream, name), name
    for name in ("kRecIter", "kRowBlock", "kLdsMaxN"):
        assert _const(near, name) == _const(cols, name), name
    code = re.sub(r"//.*", "", near)
    assert "getenv" not in code and "probe_host" not in code and "reduce_ws" not in code and "kFlagOffset" not in code
    assert os.path.join(_build.CSRC, "mi_nearest1.hip") in _build.sources()
    assert not any("mi_nearest1.hip".startswith("mi_" + f) for f in ("interp1", "interp2", "edm"))
