"""What api.py hands to the C ABI, and what it refuses, checked without a device and without the library.

A stand-in tensor (numpy memory behind the attributes api.py reads from a torch tensor), a stub in place of the loaded
library that records every call and returns 0, and handles made with __new__ are enough to run every argument rule of
the Python layer.  ACCEPTED pins, per entry point and layout case, the C function called and every argument that
reaches it (addresses by the name of the stand-in they belong to) together with the shape and the strides of what is
returned.  REJECTED pins every ValueError the file can raise: the smallest input that triggers it, the exact message,
the check that fires first when two rules are broken, and that nothing reached the library.

The expected values are literals recorded by running these tables on the commit before the helpers of api.py were
shared; one entry, marked below, differs from that commit on purpose."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from armadillocudalinearinterpolation_amd import api
from armadillocudalinearinterpolation_amd._lib import EdmParams

TORCH_DTYPE = {np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64,
               np.uint32: getattr(torch, "uint32", torch.int32)}


class T:
    """stand-in for a CUDA tensor over numpy memory; allocations made 'on its device' are real CPU tensors"""

    def __init__(self, a, cuda=True):
        self._a, self.is_cuda = a, cuda
        self.dtype, self.shape, self.device = TORCH_DTYPE[a.dtype.type], tuple(a.shape), torch.device("cpu")

    def stride(self):
        return tuple(s // self._a.itemsize for s in self._a.strides)

    def dim(self):
        return self._a.ndim

    def numel(self):
        return self._a.size

    def is_contiguous(self):
        return bool(self._a.flags["C_CONTIGUOUS"])

    def data_ptr(self):
        return self._a.ctypes.data

    @property
    def T(self):
        return T(self._a.T, self.is_cuda)


class Stub:
    """in place of the loaded library: every attribute is a function that records its call and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class Env:
    """one stub, one bare context, and the names of every address handed out"""

    def __init__(self):
        self.L, self.names, self._next, self.kept = Stub(), {}, 0xA0, []      # kept: no __del__ during a case
        self.ctx = types.SimpleNamespace(_L=self.L, _h=self.handle("ctx"))

    def handle(self, name):
        self._next += 1
        self.names[self._next] = name
        return C.c_void_p(self._next)

    def t(self, name, a, cuda=True):
        self.names[a.ctypes.data] = name
        return T(a, cuda)

    def a(self, name, a):
        self.names[a.ctypes.data] = name
        return a

    def made(self, cls, name, **attrs):
        obj = cls.__new__(cls)
        obj._L, obj._h = self.L, self.handle(name)
        for k, v in attrs.items():
            setattr(obj, k, v)
        self.kept.append(obj)
        return obj

    def axis(self, n, name="ax"):
        return self.made(api.Axis1, name, _ctx=self.ctx, n=n)

    def grid1(self):
        return self.made(api.Grid1, "grid", _ctx=self.ctx)

    def grid2(self):
        return self.made(api.Grid2, "grid", _ctx=self.ctx)

    def group(self):
        return self.made(api.Group, "group")

    def edm(self, cls=api.EventDrivenMap):
        return self.made(cls, "edm", _ctx=self.ctx, params=EdmParams(n_spikes=3, n_real=4, n_grid=8))


def vec(n, dtype=np.float64):
    return np.zeros(n, dtype)


def cm(rows, B, ld=None, dtype=np.float64):
    """(rows, B) stored column-major with leading dimension ld: buffer[:, :rows].T of a C-contiguous (B, ld) buffer"""
    return np.zeros((B, ld or rows), dtype)[:, :rows].T


def cube(rows, cols, S, ld=None, stride=None, dtype=np.float64):
    """(rows, cols, S) laid out like an arma::cube: element (i, j, s) at i + j*ld + s*stride"""
    ld = ld or rows
    stride = stride or ld * cols
    it = np.dtype(dtype).itemsize
    return np.lib.stride_tricks.as_strided(np.zeros(max(S, 1) * stride, dtype), shape=(rows, cols, S),
                                           strides=(it, ld * it, stride * it))


def _norm(arg, names):
    if isinstance(arg, C.c_void_p):
        return names.get(arg.value, "copy") if arg.value else None
    if isinstance(arg, float):
        return "nan" if arg != arg else arg
    if isinstance(arg, (int, str)) or arg is None:
        return arg
    return type(arg).__name__


def _layout(r):
    """(shape, strides in elements); the strides of an array without elements mean nothing"""
    if 0 in tuple(r.shape):
        return tuple(r.shape), ()
    if isinstance(r, np.ndarray):
        return tuple(r.shape), tuple(s // r.itemsize for s in r.strides)
    return tuple(r.shape), tuple(r.stride())


def record(build):
    """run one accepted call: [(C function, normalised arguments), ...] and (shape, strides) of each returned array"""
    e = Env()
    got = build(e)
    results = got if isinstance(got, tuple) else tuple(got.values()) if isinstance(got, dict) else (got,)
    results = [r for r in results if r is not None]
    for name, r in zip(("out", "second", "third", "fourth"), results):
        e.names.setdefault(r._a.ctypes.data if isinstance(r, T) else r.ctypes.data if isinstance(r, np.ndarray)
                           else r.data_ptr(), name)
    calls = [(name, tuple(_norm(a, e.names) for a in args)) for name, args in e.L.calls]
    return calls, [_layout(r) for r in results]


# ---- accepted calls: id -> call -------------------------------------------------------------------------------------

ACCEPTED = {
    # scattered queries on resident tables
    "grid1_interp": lambda e: e.grid1().interp(e.t("xq", vec(4)), out=e.t("out", vec(4))),
    "grid1_interp_extrap": lambda e: e.grid1().interp(e.t("xq", vec(4)), out=e.t("out", vec(4)), extrap=-7.5),
    "grid1_interp_empty": lambda e: e.grid1().interp(e.t("xq", vec(0)), out=e.t("out", vec(0))),
    "grid2_interp": lambda e: e.grid2().interp(e.t("xq", vec(4)), e.t("yq", vec(4)), out=e.t("out", vec(4)), extrap=2.0),
    "grid2_interp_grid": lambda e: e.grid2().interp_grid(e.t("xi", vec(3)), e.t("yi", vec(2)),
                                                         out=e.t("out", np.zeros((3, 2)))),
    "grid2_interp_grid_default_out": lambda e: e.grid2().interp_grid(e.t("xi", vec(3)), e.t("yi", vec(2)), extrap=1.5),
    # Axis1.interp_cols: Y (n, B) column-major
    "cols_dense": lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3)), e.t("xi", vec(4)), out=e.t("out", cm(4, 3))),
    "cols_padded": lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3, ld=9)), e.t("xi", vec(4)),
                                                   out=e.t("out", cm(4, 3, ld=6)), extrap=0.25),
    "cols_single_column": lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 1, ld=7)), e.t("xi", vec(4)),
                                                          out=e.t("out", cm(4, 1, ld=9))),
    "cols_single_row": lambda e: e.axis(1).interp_cols(e.t("Y", cm(1, 3)), e.t("xi", vec(4)), out=e.t("out", cm(4, 3))),
    "cols_one_query": lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3)), e.t("xi", vec(1)), out=e.t("out", cm(1, 3))),
    "cols_default_out": lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3, ld=9)), e.t("xi", vec(4))),
    # Axis1.interp_rows: Y (m, n) column-major, one table per row
    "rows_dense": lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7)), e.t("xi", vec(4)), out=e.t("out", cm(5, 4))),
    "rows_padded": lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7, ld=9)), e.t("xi", vec(4)),
                                                   out=e.t("out", cm(5, 4, ld=6)), extrap=0.25),
    "rows_single_row": lambda e: e.axis(7).interp_rows(e.t("Y", cm(1, 7)), e.t("xi", vec(4)), out=e.t("out", cm(1, 4))),
    "rows_single_column": lambda e: e.axis(1).interp_rows(e.t("Y", cm(5, 1, ld=8)), e.t("xi", vec(4)),
                                                          out=e.t("out", cm(5, 4))),
    "rows_one_query": lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7)), e.t("xi", vec(1)),
                                                      out=e.t("out", cm(5, 1, ld=8))),
    "rows_default_out": lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7, ld=9)), e.t("xi", vec(4))),
    # Axis1.interp_stack: Z (ny, nx, S) with dense slices
    "stack_dense": lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4)), e.t("ti", vec(2)),
                                                    out=e.t("out", cube(5, 7, 2))),
    "stack_padded_slices": lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4, stride=40)), e.t("ti", vec(2)),
                                                            out=e.t("out", cube(5, 7, 2, stride=48)), extrap=0.25),
    "stack_one_slice_one_time": lambda e: e.axis(1).interp_stack(e.t("Z", cube(5, 7, 1)), e.t("ti", vec(1)),
                                                                 out=e.t("out", cube(5, 7, 1))),
    "stack_default_out": lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4, stride=40)), e.t("ti", vec(2))),
    # interp_pairs
    "pairs_padded_x": lambda e: api.interp_pairs(e.ctx, e.t("X", cm(5, 3, ld=9)), e.t("Y", cm(5, 3)), e.t("xi", vec(4)),
                                                 out=e.t("out", cm(4, 3))),
    "pairs_lens_ok": lambda e: api.interp_pairs(e.ctx, e.t("X", cm(5, 3)), e.t("Y", cm(5, 3, ld=6)), e.t("xi", vec(4)),
                                                lens=e.t("lens", vec(3, np.int32)), out=e.t("out", cm(4, 3, ld=7)),
                                                extrap=0.25, want_ok=True),
    "pairs_single_column": lambda e: api.interp_pairs(e.ctx, e.t("X", cm(5, 1, ld=7)), e.t("Y", cm(5, 1)),
                                                      e.t("xi", vec(4)), out=e.t("out", cm(4, 1))),
    "pairs_single_row": lambda e: api.interp_pairs(e.ctx, e.t("X", cm(1, 3)), e.t("Y", cm(1, 3)), e.t("xi", vec(4)),
                                                   out=e.t("out", cm(4, 3))),
    "pairs_one_query": lambda e: api.interp_pairs(e.ctx, e.t("X", cm(5, 3)), e.t("Y", cm(5, 3)), e.t("xi", vec(1)),
                                                  out=e.t("out", cm(1, 3))),
    "pairs_default_out_ok": lambda e: api.interp_pairs(e.ctx, e.t("X", cm(5, 3)), e.t("Y", cm(5, 3)), e.t("xi", vec(4)),
                                                       want_ok=True),
    # interp_each: XI shared (1-D) or per column (2-D)
    "each_shared": lambda e: api.interp_each(e.ctx, e.t("X", cm(5, 3, ld=9)), e.t("Y", cm(5, 3)), e.t("XI", vec(4)),
                                             out=e.t("out", cm(4, 3))),
    "each_per_column": lambda e: api.interp_each(e.ctx, e.t("X", cm(5, 3)), e.t("Y", cm(5, 3)), e.t("XI", cm(4, 3)),
                                                 out=e.t("out", cm(4, 3))),
    "each_padded_lens_ok": lambda e: api.interp_each(e.ctx, e.t("X", cm(5, 3, ld=9)), e.t("Y", cm(5, 3, ld=6)),
                                                     e.t("XI", cm(4, 3, ld=8)), lens=e.t("lens", vec(3, np.int32)),
                                                     out=e.t("out", cm(4, 3, ld=7)), extrap=0.25, want_ok=True),
    "each_single_column": lambda e: api.interp_each(e.ctx, e.t("X", cm(5, 1, ld=7)), e.t("Y", cm(5, 1)),
                                                    e.t("XI", cm(4, 1, ld=6)), out=e.t("out", cm(4, 1))),
    "each_one_query": lambda e: api.interp_each(e.ctx, e.t("X", cm(5, 3)), e.t("Y", cm(5, 3)), e.t("XI", cm(1, 3)),
                                                out=e.t("out", cm(1, 3))),
    "each_default_out": lambda e: api.interp_each(e.ctx, e.t("X", cm(5, 3)), e.t("Y", cm(5, 3)), e.t("XI", cm(4, 3, ld=8))),
    # interp2_slices: Z (ny, nx, S)
    "slices_dense": lambda e: api.interp2_slices(e.ctx, e.axis(3, "ax"), e.axis(2, "ay"), e.t("Z", cube(2, 3, 4)),
                                                 e.t("xi", vec(5)), e.t("yi", vec(6)), out=e.t("out", cube(6, 5, 4))),
    "slices_padded": lambda e: api.interp2_slices(e.ctx, e.axis(3, "ax"), e.axis(2, "ay"),
                                                  e.t("Z", cube(2, 3, 4, ld=8, stride=30)), e.t("xi", vec(5)),
                                                  e.t("yi", vec(6)), out=e.t("out", cube(6, 5, 4, ld=7, stride=40)),
                                                  extrap=0.25),
    "slices_one_slice": lambda e: api.interp2_slices(e.ctx, e.axis(3, "ax"), e.axis(2, "ay"), e.t("Z", cube(2, 3, 1)),
                                                     e.t("xi", vec(1)), e.t("yi", vec(1)), out=e.t("out", cube(1, 1, 1))),
    "slices_default_out": lambda e: api.interp2_slices(e.ctx, e.axis(3, "ax"), e.axis(2, "ay"),
                                                       e.t("Z", cube(2, 3, 4, ld=8, stride=30)), e.t("xi", vec(5)),
                                                       e.t("yi", vec(6))),
    # host forms, on a context and on a group: an (n, B) Fortran-ordered input is used in place, a C-ordered one copied
    "cols_host_in_place": lambda e: e.axis(5).interp_cols_host(e.a("Y", np.zeros((5, 3), order="F")), e.a("xi", vec(4))),
    "cols_host_converted": lambda e: e.axis(5).interp_cols_host(e.a("Y", np.zeros((5, 3))), e.a("xi", vec(4)), extrap=0.25),
    "group_cols_host_in_place": lambda e: e.group().interp_cols_host(e.a("X", vec(5)), e.a("Y", np.zeros((5, 3), order="F")),
                                                                     e.a("xi", vec(4))),
    "group_cols_host_converted": lambda e: e.group().interp_cols_host(e.a("X", vec(5)), e.a("Y", np.zeros((5, 3))),
                                                                      e.a("xi", vec(4)), extrap=0.25),
    "pairs_host_in_place": lambda e: api.interp_pairs_host(e.ctx, e.a("X", np.zeros((5, 3), order="F")),
                                                           e.a("Y", np.zeros((5, 3), order="F")), e.a("xi", vec(4))),
    "pairs_host_converted_lens_ok": lambda e: api.interp_pairs_host(e.ctx, e.a("X", np.zeros((5, 3))),
                                                                    e.a("Y", np.zeros((5, 3), order="F")), e.a("xi", vec(4)),
                                                                    lens=[5, 4, 2], extrap=0.25, want_ok=True),
    "pairs_host_no_queries": lambda e: api.interp_pairs_host(e.ctx, e.a("X", np.zeros((5, 3), order="F")),
                                                             e.a("Y", np.zeros((5, 3), order="F")), e.a("xi", vec(0))),
    "group_pairs_host_in_place": lambda e: e.group().interp_pairs_host(e.a("X", np.zeros((5, 3), order="F")),
                                                                       e.a("Y", np.zeros((5, 3), order="F")),
                                                                       e.a("xi", vec(4))),
    "group_pairs_host_converted_lens_ok": lambda e: e.group().interp_pairs_host(
        e.a("X", np.zeros((5, 3), order="F")), e.a("Y", np.zeros((5, 3))), e.a("xi", vec(4)), lens=[5, 4, 2], extrap=0.25,
        want_ok=True),
    "each_host_shared": lambda e: api.interp_each_host(e.ctx, e.a("X", np.zeros((5, 3), order="F")),
                                                       e.a("Y", np.zeros((5, 3), order="F")), e.a("XI", vec(4))),
    "each_host_per_column_in_place": lambda e: api.interp_each_host(e.ctx, e.a("X", np.zeros((5, 3), order="F")),
                                                                    e.a("Y", np.zeros((5, 3), order="F")),
                                                                    e.a("XI", np.zeros((4, 3), order="F"))),
    "each_host_converted_lens_ok": lambda e: api.interp_each_host(e.ctx, e.a("X", np.zeros((5, 3))),
                                                                  e.a("Y", np.zeros((5, 3), order="F")),
                                                                  e.a("XI", np.zeros((4, 3))), lens=[5, 4, 2], extrap=0.25,
                                                                  want_ok=True),
    "group_each_host_shared": lambda e: e.group().interp_each_host(e.a("X", np.zeros((5, 3), order="F")),
                                                                   e.a("Y", np.zeros((5, 3), order="F")), e.a("XI", vec(4))),
    "group_each_host_per_column_in_place": lambda e: e.group().interp_each_host(
        e.a("X", np.zeros((5, 3), order="F")), e.a("Y", np.zeros((5, 3), order="F")), e.a("XI", np.zeros((4, 3), order="F"))),
    "group_each_host_converted_lens_ok": lambda e: e.group().interp_each_host(
        e.a("X", np.zeros((5, 3))), e.a("Y", np.zeros((5, 3), order="F")), e.a("XI", np.zeros((4, 3))), lens=[5, 4, 2],
        extrap=0.25, want_ok=True),
    # result buffers of the reference's own step and of ComputeF
    "masked_mean": lambda e: api.masked_mean(e.ctx, e.t("x", vec(6, np.float32)), e.t("accept", vec(2, np.int32)), 3),
    "masked_mean_sums": lambda e: api.masked_mean(e.ctx, e.t("x", vec(6, np.float32)), e.t("accept", vec(2, np.int32)), 3,
                                                  quirk=True, want_sums=True),
    "restrict_mean": lambda e: api.restrict_mean(e.ctx, e.t("t0", vec(6, np.float32)), e.t("i0", vec(6, np.int32)),
                                                 e.t("t1", vec(6, np.float32)), e.t("i1", vec(6, np.int32)),
                                                 e.t("accept", vec(2, np.int32)), 5.0, 3.0, 8, 3),
    "restrict_mean_sums": lambda e: api.restrict_mean(e.ctx, e.t("t0", vec(6, np.float32)), e.t("i0", vec(6, np.int32)),
                                                      e.t("t1", vec(6, np.float32)), e.t("i1", vec(6, np.int32)),
                                                      e.t("accept", vec(2, np.int32)), 5.0, 3.0, 8, 3, quirk=True,
                                                      want_sums=True),
    "edm_compute_f": lambda e: e.edm().ComputeF(e.a("Z", vec(3))),
    "edm_compute_f_partial": lambda e: e.edm().ComputeF(e.a("Z", vec(3)), want_partial=True),
    "edm_end": lambda e: e.edm().end(),
    "edm_end_partial": lambda e: e.edm().end(want_partial=True),
    "group_edm_compute_f": lambda e: e.edm(api.GroupEventDrivenMap).ComputeF(e.a("Z", vec(3))),
    "group_edm_compute_f_partial": lambda e: e.edm(api.GroupEventDrivenMap).ComputeF(e.a("Z", vec(3)), want_partial=True),
}

# id -> (the one C function called, its arguments, [(shape, strides in elements) of each array returned]).  Addresses
# carry the name of the stand-in they belong to; "out", "second", "third" are the arrays returned, in order; "copy" is
# memory made inside the call; "nan" stands for the default extrap.
COLS, ROWS, PAIRS, EACH = "mi_interp1_cols_f64_dev", "mi_interp1_rows_f64_dev", "mi_interp1_pairs_f64_dev", "mi_interp1_each_f64_dev"
SLICES, PAIRS_H, EACH_H = "mi_interp2_slices_f64_dev", "mi_interp1_pairs_f64_host", "mi_interp1_each_f64_host"
G_PAIRS_H, G_EACH_H = "mi_group_interp1_pairs_f64_host", "mi_group_interp1_each_f64_host"
RESTRICT_MEAN_ARGS = ("ctx", "t0", "i0", "t1", "i1", "accept", 5.0, 3.0, 8, 2, 3)
EXPECTED = {
    "grid1_interp": ("mi_interp1_f64_dev_v2", ("ctx", "grid", "xq", "out", 4, "nan"), [((4,), (1,))]),
    "grid1_interp_extrap": ("mi_interp1_f64_dev_v2", ("ctx", "grid", "xq", "out", 4, -7.5), [((4,), (1,))]),
    "grid1_interp_empty": ("mi_interp1_f64_dev_v2", ("ctx", "grid", "xq", "out", 0, "nan"), [((0,), ())]),
    "grid2_interp": ("mi_interp2_f64_dev", ("ctx", "grid", "xq", "yq", "out", 4, 2.0), [((4,), (1,))]),
    "grid2_interp_grid": ("mi_interp2_grid_f64_dev", ("ctx", "grid", "xi", 3, "yi", 2, "out", "nan"), [((2, 3), (1, 2))]),
    "grid2_interp_grid_default_out": ("mi_interp2_grid_f64_dev", ("ctx", "grid", "xi", 3, "yi", 2, "out", 1.5),
                                      [((2, 3), (1, 2))]),
    "cols_dense": (COLS, ("ctx", "ax", "Y", 5, 3, "xi", 4, "out", 4, "nan"), [((4, 3), (1, 4))]),
    "cols_padded": (COLS, ("ctx", "ax", "Y", 9, 3, "xi", 4, "out", 6, 0.25), [((4, 3), (1, 6))]),
    "cols_single_column": (COLS, ("ctx", "ax", "Y", 5, 1, "xi", 4, "out", 4, "nan"), [((4, 1), (1, 9))]),
    "cols_single_row": (COLS, ("ctx", "ax", "Y", 1, 3, "xi", 4, "out", 4, "nan"), [((4, 3), (1, 4))]),
    "cols_one_query": (COLS, ("ctx", "ax", "Y", 5, 3, "xi", 1, "out", 1, "nan"), [((1, 3), (1, 1))]),
    "cols_default_out": (COLS, ("ctx", "ax", "Y", 9, 3, "xi", 4, "out", 4, "nan"), [((4, 3), (1, 4))]),
    "rows_dense": (ROWS, ("ctx", "ax", "Y", 5, 5, "xi", 4, "out", 5, "nan"), [((5, 4), (1, 5))]),
    "rows_padded": (ROWS, ("ctx", "ax", "Y", 9, 5, "xi", 4, "out", 6, 0.25), [((5, 4), (1, 6))]),
    "rows_single_row": (ROWS, ("ctx", "ax", "Y", 1, 1, "xi", 4, "out", 1, "nan"), [((1, 4), (1, 1))]),
    "rows_single_column": (ROWS, ("ctx", "ax", "Y", 5, 5, "xi", 4, "out", 5, "nan"), [((5, 4), (1, 5))]),
    "rows_one_query": (ROWS, ("ctx", "ax", "Y", 5, 5, "xi", 1, "out", 5, "nan"), [((5, 1), (1, 8))]),
    "rows_default_out": (ROWS, ("ctx", "ax", "Y", 9, 5, "xi", 4, "out", 5, "nan"), [((5, 4), (1, 5))]),
    "stack_dense": (ROWS, ("ctx", "ax", "Z", 35, 35, "ti", 2, "out", 35, "nan"), [((5, 7, 2), (1, 5, 35))]),
    "stack_padded_slices": (ROWS, ("ctx", "ax", "Z", 40, 35, "ti", 2, "out", 48, 0.25), [((5, 7, 2), (1, 5, 48))]),
    "stack_one_slice_one_time": (ROWS, ("ctx", "ax", "Z", 35, 35, "ti", 1, "out", 35, "nan"), [((5, 7, 1), (1, 5, 35))]),
    "stack_default_out": (ROWS, ("ctx", "ax", "Z", 40, 35, "ti", 2, "out", 35, "nan"), [((5, 7, 2), (1, 5, 35))]),
    "pairs_padded_x": (PAIRS, ("ctx", "X", 9, "Y", 5, 5, None, 3, "xi", 4, "out", 4, "nan", None), [((4, 3), (1, 4))]),
    "pairs_lens_ok": (PAIRS, ("ctx", "X", 5, "Y", 6, 5, "lens", 3, "xi", 4, "out", 7, 0.25, "second"),
                      [((4, 3), (1, 7)), ((3,), (1,))]),
    "pairs_single_column": (PAIRS, ("ctx", "X", 5, "Y", 5, 5, None, 1, "xi", 4, "out", 4, "nan", None), [((4, 1), (1, 4))]),
    "pairs_single_row": (PAIRS, ("ctx", "X", 1, "Y", 1, 1, None, 3, "xi", 4, "out", 4, "nan", None), [((4, 3), (1, 4))]),
    "pairs_one_query": (PAIRS, ("ctx", "X", 5, "Y", 5, 5, None, 3, "xi", 1, "out", 1, "nan", None), [((1, 3), (1, 1))]),
    "pairs_default_out_ok": (PAIRS, ("ctx", "X", 5, "Y", 5, 5, None, 3, "xi", 4, "out", 4, "nan", "second"),
                             [((4, 3), (1, 4)), ((3,), (1,))]),
    "each_shared": (EACH, ("ctx", "X", 9, "Y", 5, 5, None, 3, "XI", 0, 4, "out", 4, "nan", None), [((4, 3), (1, 4))]),
    "each_per_column": (EACH, ("ctx", "X", 5, "Y", 5, 5, None, 3, "XI", 4, 4, "out", 4, "nan", None), [((4, 3), (1, 4))]),
    "each_padded_lens_ok": (EACH, ("ctx", "X", 9, "Y", 6, 5, "lens", 3, "XI", 8, 4, "out", 7, 0.25, "second"),
                            [((4, 3), (1, 7)), ((3,), (1,))]),
    "each_single_column": (EACH, ("ctx", "X", 5, "Y", 5, 5, None, 1, "XI", 4, 4, "out", 4, "nan", None), [((4, 1), (1, 4))]),
    "each_one_query": (EACH, ("ctx", "X", 5, "Y", 5, 5, None, 3, "XI", 1, 1, "out", 1, "nan", None), [((1, 3), (1, 1))]),
    "each_default_out": (EACH, ("ctx", "X", 5, "Y", 5, 5, None, 3, "XI", 8, 4, "out", 4, "nan", None), [((4, 3), (1, 4))]),
    "slices_dense": (SLICES, ("ctx", "ax", "ay", "Z", 2, 6, 4, "xi", 5, "yi", 6, "out", 6, 30, "nan"),
                     [((6, 5, 4), (1, 6, 30))]),
    "slices_padded": (SLICES, ("ctx", "ax", "ay", "Z", 8, 30, 4, "xi", 5, "yi", 6, "out", 7, 40, 0.25),
                      [((6, 5, 4), (1, 7, 40))]),
    "slices_one_slice": (SLICES, ("ctx", "ax", "ay", "Z", 2, 6, 1, "xi", 1, "yi", 1, "out", 1, 1, "nan"),
                         [((1, 1, 1), (1, 1, 1))]),
    "slices_default_out": (SLICES, ("ctx", "ax", "ay", "Z", 8, 30, 4, "xi", 5, "yi", 6, "out", 6, 30, "nan"),
                           [((6, 5, 4), (1, 6, 30))]),
    "cols_host_in_place": ("mi_interp1_cols_f64_host", ("ctx", "ax", "Y", 5, 3, "xi", 4, "out", 4, "nan"), [((4, 3), (1, 4))]),
    "cols_host_converted": ("mi_interp1_cols_f64_host", ("ctx", "ax", "copy", 5, 3, "xi", 4, "out", 4, 0.25),
                            [((4, 3), (1, 4))]),
    "group_cols_host_in_place": ("mi_group_interp1_cols_f64_host", ("group", "X", 5, "Y", 5, 3, "xi", 4, "out", 4, "nan"),
                                 [((4, 3), (1, 4))]),
    "group_cols_host_converted": ("mi_group_interp1_cols_f64_host", ("group", "X", 5, "copy", 5, 3, "xi", 4, "out", 4, 0.25),
                                  [((4, 3), (1, 4))]),
    "pairs_host_in_place": (PAIRS_H, ("ctx", "X", 5, "Y", 5, 5, None, 3, "xi", 4, "out", 4, "nan", None), [((4, 3), (1, 4))]),
    "pairs_host_converted_lens_ok": (PAIRS_H, ("ctx", "copy", 5, "Y", 5, 5, "copy", 3, "xi", 4, "out", 4, 0.25, "second"),
                                     [((4, 3), (1, 4)), ((3,), (1,))]),
    "pairs_host_no_queries": (PAIRS_H, ("ctx", "X", 5, "Y", 5, 5, None, 3, "xi", 0, "out", 1, "nan", None), [((0, 3), ())]),
    "group_pairs_host_in_place": (G_PAIRS_H, ("group", "X", 5, "Y", 5, 5, None, 3, "xi", 4, "out", 4, "nan", None),
                                  [((4, 3), (1, 4))]),
    "group_pairs_host_converted_lens_ok": (G_PAIRS_H, ("group", "X", 5, "copy", 5, 5, "copy", 3, "xi", 4, "out", 4, 0.25,
                                                       "second"), [((4, 3), (1, 4)), ((3,), (1,))]),
    "each_host_shared": (EACH_H, ("ctx", "X", 5, "Y", 5, 5, None, 3, "XI", 0, 4, "out", 4, "nan", None), [((4, 3), (1, 4))]),
    "each_host_per_column_in_place": (EACH_H, ("ctx", "X", 5, "Y", 5, 5, None, 3, "XI", 4, 4, "out", 4, "nan", None),
                                      [((4, 3), (1, 4))]),
    "each_host_converted_lens_ok": (EACH_H, ("ctx", "copy", 5, "Y", 5, 5, "copy", 3, "copy", 4, 4, "out", 4, 0.25, "second"),
                                    [((4, 3), (1, 4)), ((3,), (1,))]),
    "group_each_host_shared": (G_EACH_H, ("group", "X", 5, "Y", 5, 5, None, 3, "XI", 0, 4, "out", 4, "nan", None),
                               [((4, 3), (1, 4))]),
    "group_each_host_per_column_in_place": (G_EACH_H, ("group", "X", 5, "Y", 5, 5, None, 3, "XI", 4, 4, "out", 4, "nan", None),
                                            [((4, 3), (1, 4))]),
    "group_each_host_converted_lens_ok": (G_EACH_H, ("group", "copy", 5, "Y", 5, 5, "copy", 3, "copy", 4, 4, "out", 4, 0.25,
                                                     "second"), [((4, 3), (1, 4)), ((3,), (1,))]),
    "masked_mean": ("mi_masked_mean_f32_dev", ("ctx", "x", "accept", 2, 3, 0, "out", "second", None),
                    [((3,), (1,)), ((1,), (1,))]),
    "masked_mean_sums": ("mi_masked_mean_f32_dev", ("ctx", "x", "accept", 2, 3, 1, "out", "second", "third"),
                         [((3,), (1,)), ((1,), (1,)), ((7,), (1,))]),
    "restrict_mean": ("mi_restrict_mean_f32_dev", RESTRICT_MEAN_ARGS + (0, None, "out", "second", None),
                      [((3,), (1,)), ((1,), (1,))]),
    "restrict_mean_sums": ("mi_restrict_mean_f32_dev", RESTRICT_MEAN_ARGS + (1, None, "out", "second", "third"),
                           [((3,), (1,)), ((1,), (1,)), ((7,), (1,))]),
    "edm_compute_f": ("mi_edm_compute_f", ("edm", "Z", "out", None), [((3,), (1,))]),
    "edm_compute_f_partial": ("mi_edm_compute_f", ("edm", "Z", "out", "second"), [((3,), (1,)), ((7,), (1,))]),
    "edm_end": ("mi_edm_compute_f_end", ("edm", "out", None), [((3,), (1,))]),
    "edm_end_partial": ("mi_edm_compute_f_end", ("edm", "out", "second"), [((3,), (1,)), ((7,), (1,))]),
    "group_edm_compute_f": ("mi_group_edm_compute_f", ("edm", "Z", "out", "copy"), [((3,), (1,))]),
    "group_edm_compute_f_partial": ("mi_group_edm_compute_f", ("edm", "Z", "out", "second"), [((3,), (1,)), ((7,), (1,))]),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_accepted_call_reaches_the_library_unchanged(case):
    function, args, layouts = EXPECTED[case]
    assert record(ACCEPTED[case]) == ([(function, args)], layouts)


def test_issue_example_pairs_padded():
    """the worked example: a padded (5, 3) X with ld = 9 gives ldx = 9, ldy = 5, n = 5, B = 3, nxi = 4, ldyi = 4"""
    (name, args), = record(ACCEPTED["pairs_padded_x"])[0]
    assert name == "mi_interp1_pairs_f64_dev"
    assert args == ("ctx", "X", 9, "Y", 5, 5, None, 3, "xi", 4, "out", 4, "nan", None)


# ---- rejected calls: id -> (call, message[, the calls that may precede the refusal]) --------------------------------

COLMAJOR = "%s must be column-major (the .T view of a contiguous (B, %d) buffer)"
ROWMAJOR = "%s must be column-major (the .T view of a contiguous (%d, m) buffer)"
CUBE = ("%s must be stored slice by slice, column-major inside a slice (the .permute(2, 1, 0) view of a contiguous "
        "(S, %d, %d) buffer)")
SAME_SIZE = "out must be a contiguous float64 CUDA tensor of the same size"
NODES = "X and Y must have the same number of elements"
XI = "xi must be a contiguous float64 CUDA tensor"
XY_CUDA = "X and Y must be float64 CUDA tensors"
XY_SHAPE = "X and Y must both have shape (n, B)"
OUT_CUDA = "out must be a float64 CUDA tensor"
OUT_COLS = "out must have as many columns as Y"
LENS = "lens must be a contiguous int32 CUDA tensor of shape (B,)"
LENS_HOST = "lens must hold one count per column"
AXES = "query axes must be contiguous float64 CUDA tensors"


def _slices(e, Z, xi=None, yi=None, out=None):
    return api.interp2_slices(e.ctx, e.axis(3, "ax"), e.axis(2, "ay"), Z, xi if xi is not None else e.t("xi", vec(5)),
                              yi if yi is not None else e.t("yi", vec(6)), out=out)


def _pairs(e, X=None, Y=None, xi=None, **kw):
    return api.interp_pairs(e.ctx, X if X is not None else e.t("X", cm(5, 3)), Y if Y is not None else e.t("Y", cm(5, 3)),
                            xi if xi is not None else e.t("xi", vec(4)), **kw)


def _each(e, X=None, Y=None, XI=None, **kw):
    return api.interp_each(e.ctx, X if X is not None else e.t("X", cm(5, 3)), Y if Y is not None else e.t("Y", cm(5, 3)),
                           XI if XI is not None else e.t("XI", cm(4, 3)), **kw)


REJECTED = {
    # Grid1 and interp1
    "grid1_from_nodes_sizes": (lambda e: api.Grid1.from_nodes(e.ctx, [0.0, 1.0, 2.0], [0.0, 1.0]), NODES),
    "grid1_from_device_nodes_sizes": (lambda e: api.Grid1.from_device_nodes(e.ctx, e.t("x", vec(3)), e.t("y", vec(2))), NODES),
    "interp1_sizes": (lambda e: api.interp1(e.ctx, [0.0, 1.0, 2.0], [0.0, 1.0], [0.5]), NODES),
    "grid1_interp_xq_float32": (lambda e: e.grid1().interp(e.t("xq", vec(4, np.float32))),
                                "xq must be a contiguous float64 CUDA tensor"),
    "grid1_interp_xq_strided": (lambda e: e.grid1().interp(e.t("xq", vec(8)[::2])),
                                "xq must be a contiguous float64 CUDA tensor"),
    "grid1_interp_xq_host": (lambda e: e.grid1().interp(e.t("xq", vec(4), cuda=False)),
                             "xq must be a contiguous float64 CUDA tensor"),
    "grid1_interp_out_small": (lambda e: e.grid1().interp(e.t("xq", vec(4)), out=e.t("out", vec(1))), SAME_SIZE),
    "grid1_interp_out_float32": (lambda e: e.grid1().interp(e.t("xq", vec(4)), out=e.t("out", vec(4, np.float32))), SAME_SIZE),
    "grid1_interp_host_out": (lambda e: e.grid1().interp_host(vec(4), out=vec(3)),
                              "out must be a contiguous float64 array of the query size"),
    # Grid2
    "grid2_from_axes_z_shape": (lambda e: api.Grid2.from_axes(e.ctx, vec(3), vec(2), np.zeros((3, 2))),
                                "Z must have shape (len(y), len(x))"),
    "grid2_uniform_device_z_size": (lambda e: api.Grid2.uniform(e.ctx, 0.0, 1.0, 3, 0.0, 1.0, 2, e.t("z", vec(5))),
                                    "Z must have nx*ny elements"),
    "grid2_interp_queries": (lambda e: e.grid2().interp(e.t("xq", vec(4)), e.t("yq", vec(8)[::2])),
                             "queries must be contiguous float64 CUDA tensors"),
    "grid2_interp_queries_before_sizes": (lambda e: e.grid2().interp(e.t("xq", vec(4, np.float32)), e.t("yq", vec(3))),
                                          "queries must be contiguous float64 CUDA tensors"),
    "grid2_interp_sizes": (lambda e: e.grid2().interp(e.t("xq", vec(4)), e.t("yq", vec(3))),
                           "xq and yq must have the same number of elements"),
    # the one entry that differs from the commit these tables were recorded on: there Grid2.interp checked nothing
    # about out and handed this one-element buffer for four queries to mi_interp2_f64_dev
    "grid2_interp_out_small": (lambda e: e.grid2().interp(e.t("xq", vec(4)), e.t("yq", vec(4)), out=e.t("out", vec(1))),
                               SAME_SIZE),
    "grid2_interp_grid_axes": (lambda e: e.grid2().interp_grid(e.t("xi", vec(3)), e.t("yi", vec(2), cuda=False)), AXES),
    "grid2_interp_grid_out": (lambda e: e.grid2().interp_grid(e.t("xi", vec(3)), e.t("yi", vec(2)),
                                                              out=e.t("out", np.zeros((2, 3)))),
                              "out must be a contiguous float64 CUDA tensor of shape (len(xi), len(yi))"),
    # Axis1.interp_cols
    "cols_xi": (lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3)), e.t("xi", vec(8)[::2])), XI),
    "cols_xi_before_y": (lambda e: e.axis(5).interp_cols(e.t("Y", np.zeros((4, 3), np.float32)), e.t("xi", vec(4), cuda=False)), XI),
    "cols_y_float32": (lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3, dtype=np.float32)), e.t("xi", vec(4))),
                       "Y must be a float64 CUDA tensor"),
    "cols_y_rows": (lambda e: e.axis(5).interp_cols(e.t("Y", cm(4, 3)), e.t("xi", vec(4))), "Y must have shape (5, B)"),
    "cols_y_one_dim": (lambda e: e.axis(5).interp_cols(e.t("Y", vec(5)), e.t("xi", vec(4))), "Y must have shape (5, B)"),
    "cols_y_c_ordered": (lambda e: e.axis(5).interp_cols(e.t("Y", np.zeros((5, 3))), e.t("xi", vec(4))), COLMAJOR % ("Y", 5)),
    "cols_y_overlapping": (lambda e: e.axis(5).interp_cols(
        e.t("Y", np.lib.stride_tricks.as_strided(vec(16), shape=(5, 3), strides=(8, 24))), e.t("xi", vec(4))),
        COLMAJOR % ("Y", 5)),
    "cols_out_float32": (lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3)), e.t("xi", vec(4)),
                                                         out=e.t("out", cm(4, 3, dtype=np.float32))), OUT_CUDA),
    "cols_out_rows": (lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3)), e.t("xi", vec(4)), out=e.t("out", cm(5, 3))),
                      "out must have shape (4, B)"),
    "cols_out_c_ordered": (lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3)), e.t("xi", vec(4)),
                                                           out=e.t("out", np.zeros((4, 3)))), COLMAJOR % ("out", 4)),
    "cols_out_columns": (lambda e: e.axis(5).interp_cols(e.t("Y", cm(5, 3)), e.t("xi", vec(4)), out=e.t("out", cm(4, 2))),
                         OUT_COLS),
    "cols_host_y_rows": (lambda e: e.axis(5).interp_cols_host(np.zeros((4, 3)), vec(4)), "Y must have shape (5, B)"),
    # Axis1.interp_rows: the layout of Y is checked first
    "rows_y_columns": (lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 6)), e.t("xi", vec(4))), "Y must have shape (m, 7)"),
    "rows_y_c_ordered": (lambda e: e.axis(7).interp_rows(e.t("Y", np.zeros((5, 7))), e.t("xi", vec(4))), ROWMAJOR % ("Y", 7)),
    "rows_y_layout_before_xi": (lambda e: e.axis(7).interp_rows(e.t("Y", np.zeros((5, 7))), e.t("xi", vec(4, np.float32))),
                                ROWMAJOR % ("Y", 7)),
    "rows_xi": (lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7)), e.t("xi", vec(4, np.float32))), XI),
    "rows_y_float32": (lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7, dtype=np.float32)), e.t("xi", vec(4))),
                       "Y must be a float64 CUDA tensor"),
    "rows_out_host": (lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7)), e.t("xi", vec(4)),
                                                      out=e.t("out", cm(5, 4), cuda=False)), OUT_CUDA),
    "rows_out_columns": (lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7)), e.t("xi", vec(4)), out=e.t("out", cm(5, 3))),
                         "out must have shape (m, 4)"),
    "rows_out_c_ordered": (lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7)), e.t("xi", vec(4)),
                                                           out=e.t("out", np.zeros((5, 4)))), ROWMAJOR % ("out", 4)),
    "rows_out_rows": (lambda e: e.axis(7).interp_rows(e.t("Y", cm(5, 7)), e.t("xi", vec(4)), out=e.t("out", cm(6, 4))),
                      "out must have as many rows as Y"),
    # Axis1.interp_stack
    "stack_z_two_dims": (lambda e: e.axis(4).interp_stack(e.t("Z", cm(5, 7)), e.t("ti", vec(2))),
                         "Z must have shape (ny, nx, S)"),
    "stack_z_c_ordered": (lambda e: e.axis(4).interp_stack(e.t("Z", np.zeros((5, 7, 4))), e.t("ti", vec(2))),
                          CUBE % ("Z", 7, 5)),
    "stack_z_padded_rows": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4, ld=8)), e.t("ti", vec(2))),
                            "Z: the slices must be dense (ldz == ny); this view has ldz = 8 > ny = 5"),
    "stack_z_slices": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 3)), e.t("ti", vec(2))),
                       "Z must hold one slice per node of the axis (4), not 3"),
    "stack_slices_before_ti": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 3)), e.t("ti", vec(2, np.float32))),
                               "Z must hold one slice per node of the axis (4), not 3"),
    "stack_ti": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4)), e.t("ti", vec(4)[::2])),
                 "ti must be a contiguous float64 CUDA tensor"),
    "stack_z_float32": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4, dtype=np.float32)), e.t("ti", vec(2))),
                        "Z must be a float64 CUDA tensor"),
    "stack_out_host": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4)), e.t("ti", vec(2)),
                                                        out=e.t("out", cube(5, 7, 2), cuda=False)), OUT_CUDA),
    "stack_out_two_dims": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4)), e.t("ti", vec(2)),
                                                            out=e.t("out", cm(5, 7))), "out must have shape (ny, nx, S)"),
    "stack_out_padded_rows": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4)), e.t("ti", vec(2)),
                                                               out=e.t("out", cube(5, 7, 2, ld=6))),
                              "out: the slices must be dense (ldz == ny); this view has ldz = 6 > ny = 5"),
    "stack_out_shape": (lambda e: e.axis(4).interp_stack(e.t("Z", cube(5, 7, 4)), e.t("ti", vec(2)),
                                                         out=e.t("out", cube(5, 7, 3))), "out must have shape (5, 7, 2)"),
    # interp_pairs
    "pairs_xi": (lambda e: _pairs(e, xi=e.t("xi", vec(4, np.float32))), XI),
    "pairs_xi_before_x": (lambda e: _pairs(e, X=e.t("X", cm(5, 3, dtype=np.float32)), xi=e.t("xi", vec(8)[::2])), XI),
    "pairs_x_float32": (lambda e: _pairs(e, X=e.t("X", cm(5, 3, dtype=np.float32))), XY_CUDA),
    "pairs_y_host": (lambda e: _pairs(e, Y=e.t("Y", cm(5, 3), cuda=False)), XY_CUDA),
    "pairs_shapes_differ": (lambda e: _pairs(e, Y=e.t("Y", cm(5, 4))), XY_SHAPE),
    "pairs_one_dim": (lambda e: _pairs(e, X=e.t("X", vec(5)), Y=e.t("Y", vec(5))), XY_SHAPE),
    "pairs_x_c_ordered": (lambda e: _pairs(e, X=e.t("X", np.zeros((5, 3)))), COLMAJOR % ("X", 5)),
    "pairs_y_c_ordered": (lambda e: _pairs(e, Y=e.t("Y", np.zeros((5, 3)))), COLMAJOR % ("Y", 5)),
    "pairs_lens_float": (lambda e: _pairs(e, lens=e.t("lens", vec(3))), LENS),
    "pairs_lens_count": (lambda e: _pairs(e, lens=e.t("lens", vec(2, np.int32))), LENS),
    "pairs_lens_before_out": (lambda e: _pairs(e, lens=e.t("lens", vec(2, np.int32)), out=e.t("out", cm(4, 3), cuda=False)), LENS),
    "pairs_out_float32": (lambda e: _pairs(e, out=e.t("out", cm(4, 3, dtype=np.float32))), OUT_CUDA),
    "pairs_out_rows": (lambda e: _pairs(e, out=e.t("out", cm(5, 3))), "out must have shape (4, B)"),
    "pairs_out_c_ordered": (lambda e: _pairs(e, out=e.t("out", np.zeros((4, 3)))), COLMAJOR % ("out", 4)),
    "pairs_out_columns": (lambda e: _pairs(e, out=e.t("out", cm(4, 2))), OUT_COLS),
    "pairs_host_shapes": (lambda e: api.interp_pairs_host(e.ctx, np.zeros((5, 3)), np.zeros((5, 4)), vec(2)), XY_SHAPE),
    "pairs_host_lens": (lambda e: api.interp_pairs_host(e.ctx, np.zeros((5, 3)), np.zeros((5, 3)), vec(2), lens=[5, 5]), LENS_HOST),
    "group_pairs_host_shapes": (lambda e: e.group().interp_pairs_host(vec(5), vec(5), vec(2)), XY_SHAPE),
    "group_pairs_host_lens": (lambda e: e.group().interp_pairs_host(np.zeros((5, 3)), np.zeros((5, 3)), vec(2), lens=[5]), LENS_HOST),
    # interp_each
    "each_xi_float32": (lambda e: _each(e, XI=e.t("XI", cm(4, 3, dtype=np.float32))), "XI must be a float64 CUDA tensor"),
    "each_xi_before_x": (lambda e: _each(e, X=e.t("X", cm(5, 3), cuda=False), XI=e.t("XI", vec(4), cuda=False)),
                         "XI must be a float64 CUDA tensor"),
    "each_x_float32": (lambda e: _each(e, X=e.t("X", cm(5, 3, dtype=np.float32))), XY_CUDA),
    "each_shapes_differ": (lambda e: _each(e, Y=e.t("Y", cm(4, 3))), XY_SHAPE),
    "each_x_c_ordered": (lambda e: _each(e, X=e.t("X", np.zeros((5, 3)))), COLMAJOR % ("X", 5)),
    "each_y_c_ordered": (lambda e: _each(e, Y=e.t("Y", np.zeros((5, 3)))), COLMAJOR % ("Y", 5)),
    "each_y_before_shared_xi": (lambda e: _each(e, Y=e.t("Y", np.zeros((5, 3))), XI=e.t("XI", vec(8)[::2])), COLMAJOR % ("Y", 5)),
    "each_shared_xi_strided": (lambda e: _each(e, XI=e.t("XI", vec(8)[::2])), "a shared XI must be a contiguous 1-D tensor"),
    "each_xi_three_dims": (lambda e: _each(e, XI=e.t("XI", np.zeros((4, 3, 1)))),
                           "XI must be a column-major (nxi, B) view or a contiguous 1-D tensor"),
    "each_xi_c_ordered": (lambda e: _each(e, XI=e.t("XI", np.zeros((4, 3)))), COLMAJOR % ("XI", 4)),
    "each_xi_columns": (lambda e: _each(e, XI=e.t("XI", cm(4, 2))), "XI must have as many columns as X"),
    "each_lens_int64": (lambda e: _each(e, lens=e.t("lens", vec(3, np.int64))), LENS),
    "each_lens_strided": (lambda e: _each(e, lens=e.t("lens", vec(6, np.int32)[::2])), LENS),
    "each_out_host": (lambda e: _each(e, out=e.t("out", cm(4, 3), cuda=False)), OUT_CUDA),
    "each_out_rows": (lambda e: _each(e, out=e.t("out", cm(5, 3))), "out must have shape (4, B)"),
    "each_out_c_ordered": (lambda e: _each(e, out=e.t("out", np.zeros((4, 3)))), COLMAJOR % ("out", 4)),
    "each_out_columns": (lambda e: _each(e, out=e.t("out", cm(4, 4))), OUT_COLS),
    "each_host_shapes": (lambda e: api.interp_each_host(e.ctx, np.zeros((5, 3)), np.zeros((5, 4)), np.zeros((2, 3))), XY_SHAPE),
    "each_host_lens": (lambda e: api.interp_each_host(e.ctx, np.zeros((5, 3)), np.zeros((5, 3)), vec(2), lens=[5, 5]), LENS_HOST),
    "each_host_xi_columns": (lambda e: api.interp_each_host(e.ctx, np.zeros((5, 3)), np.zeros((5, 3)), np.zeros((2, 4))),
                             "XI must have shape (nxi, B), one column of queries per column of X, or be 1-D"),
    "group_each_host_xi_three_dims": (lambda e: e.group().interp_each_host(np.zeros((5, 3)), np.zeros((5, 3)), np.zeros((2, 3, 1))),
                                      "XI must have shape (nxi, B), one column of queries per column of X, or be 1-D"),
    "group_each_host_lens_before_xi": (lambda e: e.group().interp_each_host(np.zeros((5, 3)), np.zeros((5, 3)), np.zeros((2, 4)),
                                                                            lens=[5, 5]), LENS_HOST),
    # interp2_slices
    "slices_axes": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), yi=e.t("yi", vec(6, np.float32))), AXES),
    "slices_axes_before_z": (lambda e: _slices(e, e.t("Z", cm(2, 3)), xi=e.t("xi", vec(10)[::2])), AXES),
    "slices_z_float32": (lambda e: _slices(e, e.t("Z", np.zeros((4, 3, 2), np.float32).transpose(2, 1, 0))),
                         "Z must be a float64 CUDA tensor"),
    "slices_z_shape": (lambda e: _slices(e, e.t("Z", cube(3, 2, 4))), "Z must have shape (2, 3, S)"),
    "slices_z_two_dims": (lambda e: _slices(e, e.t("Z", cm(2, 3))), "Z must have shape (2, 3, S)"),
    "slices_z_c_ordered": (lambda e: _slices(e, e.t("Z", np.zeros((2, 3, 4)))), CUBE % ("Z", 3, 2)),
    "slices_z_overlapping": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4, ld=4, stride=11))), CUBE % ("Z", 3, 2)),
    "slices_out_host": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", cube(6, 5, 4), cuda=False)), OUT_CUDA),
    "slices_out_shape": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", cube(5, 6, 4))),
                         "out must have shape (6, 5, S)"),
    "slices_out_c_ordered": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", np.zeros((6, 5, 4)))),
                             CUBE % ("out", 5, 6)),
    "slices_out_slices": (lambda e: _slices(e, e.t("Z", cube(2, 3, 4)), out=e.t("out", cube(6, 5, 3))),
                          "out must have as many slices as Z"),
    # EventDrivenMap and the group forms
    "edm_compute_f_size": (lambda e: e.edm().ComputeF(vec(2)), "Z must have n_spikes=3 elements"),
    "edm_begin_size": (lambda e: e.edm().begin(vec(4)), "Z must have n_spikes=3 elements"),
    "group_cols_host_y_rows": (lambda e: e.group().interp_cols_host(vec(5), np.zeros((4, 3)), vec(4)),
                               "Y must have shape (len(X), B)"),
    "group_grid2_host_sizes": (lambda e: e.made(api.GroupGrid2, "grid", _g=e.group()).interp_host(vec(4), vec(3)),
                               "xq and yq must have the same number of elements"),
    # the library is asked for the shard first; the stub's 0 is its answer for a rank the group does not have
    "group_edm_no_shard": (lambda e: e.edm(api.GroupEventDrivenMap).shard_debug_read(5), "no shard 5 in this group",
                           [("mi_group_edm_shard", ("edm", 5))]),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejected_call_names_the_rule_and_reaches_nothing(case):
    build, message, before = (REJECTED[case] + ([],))[:3]
    e = Env()
    with pytest.raises(ValueError) as err:
        build(e)
    assert str(err.value) == message
    assert [(name, tuple(_norm(a, e.names) for a in args)) for name, args in e.L.calls] == before


# ---- handles: closed once, by the right function, owners first ------------------------------------------------------

DESTROY = {"Context": "mi_ctx_destroy", "Timer": "mi_timer_destroy", "Grid1": "mi_grid1_destroy",
           "Grid2": "mi_grid2_destroy", "Axis1": "mi_axis1_destroy", "EventDrivenMap": "mi_edm_destroy",
           "Group": "mi_group_destroy", "GroupGrid1": "mi_group_grid1_destroy", "GroupGrid2": "mi_group_grid2_destroy",
           "GroupEventDrivenMap": "mi_group_edm_destroy"}


@pytest.mark.parametrize("cls", sorted(DESTROY))
def test_close_destroys_the_handle_once(cls):
    e = Env()
    obj = e.made(getattr(api, cls), "h")
    obj.close()
    obj.close()
    obj.__del__()
    assert [(n, tuple(_norm(a, e.names) for a in args)) for n, args in e.L.calls] == [(DESTROY[cls], ("h",))]
    bare = getattr(api, cls).__new__(getattr(api, cls))            # never initialised: nothing to close
    bare.close()
    assert len(e.L.calls) == 1


def test_context_closes_its_children_first_and_edm_its_replicas():
    e = Env()
    ctx = e.made(api.Context, "ctx", _children=set())
    grid = api.Grid1(ctx, e.handle("grid"))                         # the constructors register with the context
    assert set(ctx._children) == {grid}
    ctx.close()
    assert [n for n, _ in e.L.calls] == ["mi_grid1_destroy", "mi_ctx_destroy"]
    borrowed = types.SimpleNamespace(_L=e.L, _h=e.handle("member"))  # a group member's context keeps no children
    api.Axis1(borrowed, e.handle("axis"), 3).close()
    edm = e.edm()
    edm._replicas = [e.made(api.EventDrivenMap, "replica")]         # as ComputeFBatch makes them: __new__, no __init__
    edm.close()
    assert [(n, tuple(_norm(a, e.names) for a in args)) for n, args in e.L.calls[2:]] == [
        ("mi_axis1_destroy", ("axis",)), ("mi_edm_destroy", ("replica",)), ("mi_edm_destroy", ("edm",))]
    assert edm._replicas == []
