"""Python host side over the C ABI (include/mi355_interp.h).

PyTorch is plumbing only: device memory (torch.Tensor on cuda:N), streams and,
in bench.py, torch.distributed.  Every computation runs in libmi355interp.so;
nothing here has a CPU or eager-torch fallback.

Names follow the reference's domain: grids / nodes / queries for the tables,
realisations / spikes for EventDrivenMap (EventDrivenMap.hpp:11-121).
"""
import ctypes as C
import os
import math
import weakref

import numpy as np

from . import _lib
from ._lib import EdmParams, MiError, check  # noqa: F401

MI_GRID_SANITISE = 0x1
MI_GRID_DEVICE_PTRS = 0x2
MI_GRID2_COMPACT = 0x4
MATH_EXACT = 0
MATH_FAST = 1


def _torch():
    import torch
    return torch


def _ptr(t):
    """Device/host address of a torch tensor or numpy array (must be contiguous)."""
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return C.c_void_p(t.ctypes.data)
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def _np64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))


class _Handle:
    """Owner of one handle of the C ABI: _L the library, _h the handle, _destroy the name of the function that frees it.
    Context, Grid1 and Grid2 do not derive from it yet and keep the same lines of their own (DESIGN.md section 1 says why)."""
    _destroy = None

    def _own(self, L, h, ctx=None):
        """take handle h; one created on a Context is also closed when that context is, before it (its device state
        belongs to the context).  A group member's context (_GroupCtx) keeps no such list: the group owns it."""
        self._L, self._h = L, h
        if hasattr(ctx, "_children"):
            ctx._children.add(self)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _need_f64_cuda(t, what, contiguous, message=None):
    """ValueError unless t is a float64 CUDA tensor (and contiguous, if asked); message: a call site's own wording"""
    if not (t.is_cuda and t.dtype == _torch().float64 and (not contiguous or t.is_contiguous())):
        raise ValueError(message or "%s must be a %sfloat64 CUDA tensor" % (what, "contiguous " if contiguous else ""))


def _strides(a):
    """strides of a tensor or numpy array, in elements"""
    return a.stride() if hasattr(a, "stride") else tuple(s // a.itemsize for s in a.strides)


def _leading_dim(a, rows, cols):
    """Leading dimension of the column-major (rows, cols) matrix in the first two dimensions of a -- element (i, j) at
    i + j*ld -- or None if a is not laid out so: rows not adjacent, or columns that overlap.  The stride of a single
    column is not read (it means nothing): such a matrix is dense."""
    st = _strides(a)
    ld = st[1] if cols > 1 else max(rows, 1)
    return None if (rows > 1 and st[0] != 1) or ld < rows else ld


def _cube_view(a, rows, cols, what):
    """(leading dimension, slice stride, slices) of a 3-D (rows, cols, S) array or tensor stored like an arma::cube:
    element (i, j, s) at i + j*ld + s*stride, i.e. the .permute(2, 1, 0) view of a contiguous (S, cols, rows) buffer, or
    a padded view of one; strides in elements"""
    shape = tuple(a.shape)
    if len(shape) != 3 or shape[0] != rows or shape[1] != cols:
        raise ValueError("%s must have shape (%d, %d, S)" % (what, rows, cols))
    S = shape[2]
    ld = _leading_dim(a, rows, cols)
    stride = _strides(a)[2] if S > 1 else (ld or 0) * cols           # the stride of a single slice is not read either
    if ld is None or stride < ld * cols:
        raise ValueError("%s must be stored slice by slice, column-major inside a slice (the .permute(2, 1, 0) view of a "
                         "contiguous (S, %d, %d) buffer)" % (what, cols, rows))
    return ld, stride, S


# Result buffers: the one the call allocates by default, or the caller's `out` once it passed the same rules.

def _out_colmajor(out, rows, B, Y):
    """(out, leading dimension) of a column-major (rows, B) result beside Y's B columns; default: the .T view of a new
    contiguous (B, rows) buffer"""
    if out is None:
        out = _torch().empty((B, rows), dtype=_torch().float64, device=Y.device).T
    else:
        _need_f64_cuda(out, "out", False)
    ld, Bo = Axis1._colmajor_view(out, rows, "out")
    if Bo != B:
        raise ValueError("out must have as many columns as Y")
    return out, ld


def _out_rows(out, m, cols, Y):
    """(out, leading dimension) of a column-major (m, cols) result beside Y's m row tables; default: the .T view of a
    new contiguous (cols, m) buffer"""
    if out is None:
        out = _torch().empty((cols, m), dtype=_torch().float64, device=Y.device).T
    else:
        _need_f64_cuda(out, "out", False)
    ld, mo = Axis1._rows_view(out, cols, "out")
    if mo != m:
        raise ValueError("out must have as many rows as Y")
    return out, ld


def _out_cube(out, rows, cols, S, Z):
    """a (rows, cols, S) result laid out like an arma::cube beside Z; default: the .permute(2, 1, 0) view of a new
    contiguous (S, cols, rows) buffer.  The caller checks the layout: interp_stack wants dense slices, interp2_slices
    takes padded ones."""
    if out is None:
        return _torch().empty((S, cols, rows), dtype=_torch().float64, device=Z.device).permute(2, 1, 0)
    _need_f64_cuda(out, "out", False)
    return out


class Context:
    """mi_ctx: one device + one stream.  By default it follows torch's current stream."""

    def __init__(self, device=0, stream="torch"):
        self._L = _lib.load()
        h = C.c_void_p()
        check(self._L.mi_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._children = weakref.WeakSet()     # grids / problems created on this context: closed before it is
        if stream == "torch":
            self.use_torch_stream()
        elif stream is not None:
            self.set_stream(stream)

    def use_torch_stream(self):
        torch = _torch()
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def set_stream(self, raw_stream):
        check(self._L.mi_ctx_set_stream(self._h, C.c_void_p(raw_stream)), self._h)

    def own_stream(self):
        """Give this context a non-blocking stream of its own (work of several contexts can then overlap)."""
        check(self._L.mi_ctx_own_stream(self._h), self._h)

    def synchronize(self):
        check(self._L.mi_ctx_synchronize(self._h), self._h)

    def set_query_order(self, order):
        """0 auto (device-side probe), 1 queries are unordered, 2 queries are ordered/clustered."""
        check(self._L.mi_ctx_set_query_order(self._h, int(order)), self._h)

    def device_info(self):
        name = C.create_string_buffer(128)
        cus, hbm = C.c_int(0), C.c_size_t(0)
        check(self._L.mi_ctx_device_info(self._h, name, 128, C.byref(cus), C.byref(hbm)), self._h)
        return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}

    def timer(self):
        return Timer(self)

    def close(self):
        """Closes the handles created on this context first (their device state belongs to it), then the context."""
        for child in list(getattr(self, "_children", ()) or ()):
            try:
                child.close()
            except Exception:
                pass
        if getattr(self, "_h", None):
            self._L.mi_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Timer(_Handle):
    """HIP events recorded on the context's stream."""
    _destroy = "mi_timer_destroy"

    def __init__(self, ctx):
        self._ctx = ctx
        h = C.c_void_p()
        check(ctx._L.mi_timer_create(ctx._h, C.byref(h)), ctx._h)
        self._own(ctx._L, h)

    def start(self):
        check(self._L.mi_timer_start(self._h), self._ctx._h)

    def stop(self):
        check(self._L.mi_timer_stop(self._h), self._ctx._h)

    def elapsed_ms(self):
        ms = C.c_float(0)
        check(self._L.mi_timer_elapsed_ms(self._h, C.byref(ms)), self._ctx._h)
        return float(ms.value)


class Grid1:
    """HBM-resident 1-D table (mi_grid1)."""

    def __init__(self, ctx, handle):
        self._ctx, self._h, self._L = ctx, handle, ctx._L
        if hasattr(ctx, "_children"):
            ctx._children.add(self)

    @classmethod
    def from_nodes(cls, ctx, x, y, sanitise=True):
        """Explicit abscissae -- the arma::interp1(X, Y, ...) table."""
        x, y = _np64(x), _np64(y)
        if x.size != y.size:
            raise ValueError("X and Y must have the same number of elements")
        h = C.c_void_p()
        check(ctx._L.mi_grid1_create(ctx._h, _ptr(x), _ptr(y), x.size,
                                     MI_GRID_SANITISE if sanitise else 0, C.byref(h)), ctx._h)
        return cls(ctx, h)

    @classmethod
    def from_device_nodes(cls, ctx, x, y):
        """Explicit, strictly increasing abscissae already resident on the device (float64 CUDA tensors)."""
        if x.numel() != y.numel():
            raise ValueError("X and Y must have the same number of elements")
        h = C.c_void_p()
        check(ctx._L.mi_grid1_create(ctx._h, _ptr(x), _ptr(y), x.numel(), MI_GRID_DEVICE_PTRS, C.byref(h)), ctx._h)
        return cls(ctx, h)

    @classmethod
    def uniform(cls, ctx, x0, dx, y):
        """Implicit grid X_i = fma(i, dx, x0)."""
        y = _np64(y)
        h = C.c_void_p()
        check(ctx._L.mi_grid1_create_uniform(ctx._h, float(x0), float(dx), _ptr(y), y.size, 0, C.byref(h)), ctx._h)
        return cls(ctx, h)

    def info(self):
        n, mode, tb = C.c_size_t(0), C.c_int(0), C.c_size_t(0)
        check(self._L.mi_grid1_info(self._h, C.byref(n), C.byref(mode), C.byref(tb)), self._ctx._h)
        formula, pin = C.c_int(0), C.c_int(0)
        check(self._L.mi_debug_grid1_formula(self._h, C.byref(formula), C.byref(pin)), self._ctx._h)
        return {"n_nodes": n.value, "mode": mode.value, "table_bytes": tb.value,
                "formula": formula.value, "pin_last": pin.value}     # closed form of a mode-0 table (-1 otherwise)

    def interp(self, xq, out=None, extrap=math.nan):
        """xq: float64 cuda tensor -> float64 cuda tensor (asynchronous on the ctx stream)."""
        torch = _torch()
        if not (xq.is_cuda and xq.dtype == torch.float64 and xq.is_contiguous()):
            raise ValueError("xq must be a contiguous float64 CUDA tensor")
        if out is None:
            out = torch.empty_like(xq)
        elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == xq.numel()):
            raise ValueError("out must be a contiguous float64 CUDA tensor of the same size")
        check(self._L.mi_interp1_f64_dev_v2(self._ctx._h, self._h, _ptr(xq), _ptr(out), xq.numel(), float(extrap)),
              self._ctx._h)
        return out

    def interp_host(self, xq, extrap=math.nan, out=None):
        xq = _np64(xq)
        if out is None:
            out = np.empty_like(xq)
        elif out.dtype != np.float64 or out.size != xq.size or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous float64 array of the query size")
        check(self._L.mi_interp1_f64_host(self._ctx._h, self._h, _ptr(xq), _ptr(out), xq.size, float(extrap)),
              self._ctx._h)
        return out

    def interp_nearest(self, xq, out=None, extrap=math.nan):
        """arma::interp1's "nearest" method on this table: out[i] = Y[k], k the node nearest to xq[i] (a tie keeps the
        left node; the stored value comes back as it is).  xq: contiguous float64 CUDA tensor; asynchronous on the
        context's stream."""
        _need_f64_cuda(xq, "xq", True)
        if out is None:
            out = _torch().empty_like(xq)
        else:
            _need_f64_cuda(out, "out", True, "out must be a contiguous float64 CUDA tensor of the same size")
            if out.numel() != xq.numel():
                raise ValueError("out must be a contiguous float64 CUDA tensor of the same size")
        check(self._L.mi_interp1_nearest_f64_dev(self._ctx._h, self._h, _ptr(xq), _ptr(out), xq.numel(), float(extrap)),
              self._ctx._h)
        return out

    def interp_nearest_host(self, xq, extrap=math.nan, out=None):
        """interp_nearest on host arrays (synchronous)"""
        xq = _np64(xq)
        if out is None:
            out = np.empty_like(xq)
        elif out.dtype != np.float64 or out.size != xq.size or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous float64 array of the query size")
        check(self._L.mi_interp1_nearest_f64_host(self._ctx._h, self._h, _ptr(xq), _ptr(out), xq.size, float(extrap)),
              self._ctx._h)
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.mi_grid1_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def interp1(ctx, X, Y, XI, extrap=math.nan):
    """arma::interp1(X, Y, XI, YI, "linear", extrap) on host arrays, computed on the GPU."""
    X, Y, XI = _np64(X), _np64(Y), _np64(XI)
    if X.size != Y.size:
        raise ValueError("X and Y must have the same number of elements")
    YI = np.empty_like(XI)
    check(ctx._L.mi_interp1_f64(ctx._h, _ptr(X), _ptr(Y), X.size, _ptr(XI), _ptr(YI), XI.size, float(extrap)), ctx._h)
    return YI


def interp1_nearest(ctx, X, Y, XI, extrap=math.nan):
    """arma::interp1(X, Y, XI, YI, "nearest", extrap) on host arrays (X sorted and de-duplicated first), on the GPU."""
    X, Y, XI = _np64(X), _np64(Y), _np64(XI)
    if X.size != Y.size:
        raise ValueError("X and Y must have the same number of elements")
    YI = np.empty_like(XI)
    check(ctx._L.mi_interp1_nearest_f64(ctx._h, _ptr(X), _ptr(Y), X.size, _ptr(XI), _ptr(YI), XI.size, float(extrap)),
          ctx._h)
    return YI


class Grid2:
    """HBM-resident 2-D table (mi_grid2); z is (ny, nx), stored column-major like arma::mat."""

    def __init__(self, ctx, handle):
        self._ctx, self._h, self._L = ctx, handle, ctx._L
        if hasattr(ctx, "_children"):
            ctx._children.add(self)

    @staticmethod
    def _colmajor(z, ny, nx):
        z = np.asarray(z, dtype=np.float64)
        if z.shape != (ny, nx):
            raise ValueError("Z must have shape (len(y), len(x))")
        return np.ascontiguousarray(z.T).reshape(-1)

    @classmethod
    def from_axes(cls, ctx, x, y, z, compact=False):
        x, y = _np64(x), _np64(y)
        zc = cls._colmajor(z, y.size, x.size)
        h = C.c_void_p()
        check(ctx._L.mi_grid2_create(ctx._h, _ptr(x), x.size, _ptr(y), y.size, _ptr(zc),
                                     MI_GRID2_COMPACT if compact else 0, C.byref(h)), ctx._h)
        return cls(ctx, h)

    @classmethod
    def uniform(cls, ctx, x0, dx, nx, y0, dy, ny, z, compact=False):
        """z: (ny, nx) numpy array, or a column-major float64 CUDA tensor of ny*nx elements."""
        h = C.c_void_p()
        if isinstance(z, np.ndarray) or not hasattr(z, "is_cuda"):
            zc = cls._colmajor(z, ny, nx)
            flags = 0
        else:
            if z.numel() != nx * ny:
                raise ValueError("Z must have nx*ny elements")
            zc, flags = z, MI_GRID_DEVICE_PTRS
        if compact:
            flags |= MI_GRID2_COMPACT
        check(ctx._L.mi_grid2_create_uniform(ctx._h, float(x0), float(dx), nx, float(y0), float(dy), ny,
                                             _ptr(zc), flags, C.byref(h)), ctx._h)
        return cls(ctx, h)

    def info(self):
        tb = C.c_size_t(0)
        check(self._L.mi_grid2_info(self._h, C.byref(tb)))
        return {"table_bytes": tb.value}

    def interp(self, xq, yq, out=None, extrap=math.nan):
        return self._scattered_call("mi_interp2_f64_dev", xq, yq, out, extrap)

    def interp_nearest(self, xq, yq, out=None, extrap=math.nan):
        """arma::interp2's "nearest" method on scattered pairs (mi_interp2_nearest_f64_dev): interp's arguments and
        layouts; out[i] = Z(ky, kx), the stored value of the node the nearest rule picks on each axis (a tie keeps the
        left node), inf / NaN / -0.0 as they are."""
        return self._scattered_call("mi_interp2_nearest_f64_dev", xq, yq, out, extrap)

    def _scattered_call(self, fn, xq, yq, out, extrap):
        torch = _torch()
        for t in (xq, yq):
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
                raise ValueError("queries must be contiguous float64 CUDA tensors")
        if xq.numel() != yq.numel():
            raise ValueError("xq and yq must have the same number of elements")
        if out is None:
            out = torch.empty_like(xq)
        elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == xq.numel()):
            raise ValueError("out must be a contiguous float64 CUDA tensor of the same size")     # Grid1.interp's rule
        check(getattr(self._L, fn)(self._ctx._h, self._h, _ptr(xq), _ptr(yq), _ptr(out), xq.numel(),
                                   float(extrap)), self._ctx._h)
        return out

    def interp_host(self, xq, yq, extrap=math.nan):
        xq, yq = _np64(xq), _np64(yq)
        out = np.empty_like(xq)
        check(self._L.mi_interp2_f64_host(self._ctx._h, self._h, _ptr(xq), _ptr(yq), _ptr(out), xq.size,
                                          float(extrap)), self._ctx._h)
        return out

    def interp_grid(self, xi, yi, out=None, extrap=math.nan):
        """arma::interp2's gridded output: ZI[i, j] = Z at (xi[j], yi[i]), a (nyi, nxi) tensor stored column-major (the
        .T view of a contiguous (nxi, nyi) buffer).  xi, yi: contiguous float64 CUDA tensors (any order); out: that
        contiguous (nxi, nyi) float64 buffer.  Asynchronous on the context's stream."""
        return self._grid_call("mi_interp2_grid_f64_dev", xi, yi, out, extrap)

    def interp_grid_nearest(self, xi, yi, out=None, extrap=math.nan):
        """arma::interp2's "nearest" method, gridded output (mi_interp2_grid_nearest_f64_dev): interp_grid's arguments
        and layouts; ZI[i, j] = Z(ky(yi[i]), kx(xi[j])), bit-identical to interp_nearest on that pair."""
        return self._grid_call("mi_interp2_grid_nearest_f64_dev", xi, yi, out, extrap)

    def _grid_call(self, fn, xi, yi, out, extrap):
        torch = _torch()
        for t in (xi, yi):
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
                raise ValueError("query axes must be contiguous float64 CUDA tensors")
        nxi, nyi = xi.numel(), yi.numel()
        if out is None:
            out = torch.empty((nxi, nyi), dtype=torch.float64, device=xi.device)
        elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (nxi, nyi)):
            raise ValueError("out must be a contiguous float64 CUDA tensor of shape (len(xi), len(yi))")
        check(getattr(self._L, fn)(self._ctx._h, self._h, _ptr(xi), nxi, _ptr(yi), nyi, _ptr(out),
                                   float(extrap)), self._ctx._h)
        return out.T

    def interp_grid_host(self, xi, yi, extrap=math.nan):
        """host form of interp_grid: numpy axes in, a Fortran-ordered (nyi, nxi) array out (synchronous)"""
        return self._grid_host_call("mi_interp2_grid_f64_host", xi, yi, extrap)

    def interp_grid_nearest_host(self, xi, yi, extrap=math.nan):
        """host form of interp_grid_nearest: numpy axes in, a Fortran-ordered (nyi, nxi) array out (synchronous)"""
        return self._grid_host_call("mi_interp2_grid_nearest_f64_host", xi, yi, extrap)

    def _grid_host_call(self, fn, xi, yi, extrap):
        xi, yi = _np64(xi), _np64(yi)
        out = np.empty((xi.size, yi.size))
        check(getattr(self._L, fn)(self._ctx._h, self._h, _ptr(xi), xi.size, _ptr(yi), yi.size, _ptr(out),
                                   float(extrap)), self._ctx._h)
        return out.T

    def close(self):
        if getattr(self, "_h", None):
            self._L.mi_grid2_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Axis1(_Handle):
    """Validated, device-resident 1-D axis (mi_axis1) for interp1 over the columns of a matrix: one X, many Y.

    Layout, as arma::mat: Y is (n, B) with one profile per COLUMN, stored column-major -- element (i, c) at
    i + c*ld -- and so is the (nxi, B) result.  In torch / numpy terms that is the .T view of a C-contiguous (B, n)
    buffer (a realisation per row of the buffer); a view with a row stride ld > n (buffer[:, :n].T) is taken as it is.
    X is used as given ("*linear" contract): strictly increasing and finite, else MiError (MI_ERR_GRID).

    Data stored the other way round -- one table per ROW of a column-major (m, n) matrix, i.e. a C-contiguous (n, m)
    "time-major" buffer viewed .T, every time level a contiguous block -- goes through interp_rows, and a cube of fields
    at n time levels through interp_stack (interpolation along the slice index); both are one call of
    mi_interp1_rows_f64_dev and bit-identical to interp_cols on the transposed data.  Device tensors only.
    interp_cols_nearest, interp_rows_nearest and interp_stack_nearest are the same calls with arma::interp1's "nearest"
    method: the stored value of the nearest node, copied."""

    _destroy = "mi_axis1_destroy"

    def __init__(self, ctx, handle, n):
        self._ctx, self.n = ctx, int(n)
        self._own(ctx._L, handle, ctx)

    @classmethod
    def from_nodes(cls, ctx, x):
        x = _np64(x)
        h = C.c_void_p()
        check(ctx._L.mi_axis1_create(ctx._h, _ptr(x), x.size, 0, C.byref(h)), ctx._h)
        return cls(ctx, h, x.size)

    @classmethod
    def from_device_nodes(cls, ctx, x):
        """nodes already resident on the device (a contiguous float64 CUDA tensor)"""
        h = C.c_void_p()
        check(ctx._L.mi_axis1_create(ctx._h, _ptr(x), x.numel(), MI_GRID_DEVICE_PTRS, C.byref(h)), ctx._h)
        return cls(ctx, h, x.numel())

    @classmethod
    def uniform(cls, ctx, x0, dx, n):
        """implicit nodes X_i = fma(i, dx, x0)"""
        h = C.c_void_p()
        check(ctx._L.mi_axis1_create_uniform(ctx._h, float(x0), float(dx), int(n), C.byref(h)), ctx._h)
        return cls(ctx, h, n)

    @staticmethod
    def _colmajor_view(a, rows, what):
        """(leading dimension, columns) of a 2-D (rows, B) array or tensor stored column-major; strides in elements"""
        shape = tuple(a.shape)
        if len(shape) != 2 or shape[0] != rows:
            raise ValueError("%s must have shape (%d, B)" % (what, rows))
        ld = _leading_dim(a, rows, shape[1])
        if ld is None:
            raise ValueError("%s must be column-major (the .T view of a contiguous (B, %d) buffer)" % (what, rows))
        return ld, shape[1]

    def interp_cols(self, Y, xi, out=None, extrap=math.nan):
        """Y: (n, B) float64 CUDA tensor, column-major (see the class docstring); xi: contiguous float64 CUDA tensor of
        nxi queries in any order; out: column-major (nxi, B) tensor (default: the .T view of a new contiguous (B, nxi)
        buffer).  Returns the (nxi, B) result; asynchronous on the context's stream."""
        _need_f64_cuda(xi, "xi", True)
        _need_f64_cuda(Y, "Y", False)
        ldy, B = self._colmajor_view(Y, self.n, "Y")
        nxi = xi.numel()
        out, ldyi = _out_colmajor(out, nxi, B, Y)
        check(self._L.mi_interp1_cols_f64_dev(self._ctx._h, self._h, C.c_void_p(Y.data_ptr()), ldy, B, _ptr(xi), nxi,
                                              C.c_void_p(out.data_ptr()), ldyi, float(extrap)), self._ctx._h)
        return out

    def interp_cols_nearest(self, Y, xi, out=None, extrap=math.nan):
        """interp_cols with arma::interp1's "nearest" method: out[i, c] = Y[k, c], k the node nearest to xi[i] (a tie
        keeps the left node; the stored value comes back as it is).  Arguments and layouts as interp_cols."""
        _need_f64_cuda(xi, "xi", True)
        _need_f64_cuda(Y, "Y", False)
        ldy, B = self._colmajor_view(Y, self.n, "Y")
        nxi = xi.numel()
        out, ldyi = _out_colmajor(out, nxi, B, Y)
        check(self._L.mi_interp1_cols_nearest_f64_dev(self._ctx._h, self._h, C.c_void_p(Y.data_ptr()), ldy, B, _ptr(xi), nxi,
                                                      C.c_void_p(out.data_ptr()), ldyi, float(extrap)), self._ctx._h)
        return out

    @staticmethod
    def _rows_view(a, cols, what):
        """(leading dimension, rows) of a 2-D (m, cols) array or tensor stored column-major, one table per row: element
        (r, k) at r + k*ld, the .T view of a C-contiguous (cols, m) buffer or a padded view of one (buffer[:, :m].T);
        strides in elements"""
        shape = tuple(a.shape)
        if len(shape) != 2 or shape[1] != cols:
            raise ValueError("%s must have shape (m, %d)" % (what, cols))
        ld = _leading_dim(a, shape[0], cols)
        if ld is None:
            raise ValueError("%s must be column-major (the .T view of a contiguous (%d, m) buffer)" % (what, cols))
        return ld, shape[0]

    @staticmethod
    def _stack_view(a, what):
        """(ny, nx, slice stride, slices) of a 3-D (ny, nx, S) array or tensor laid out like an arma::cube (_cube_view)
        whose slices are dense, ldz == ny: the ny*nx elements of a slice are then one column of a (ny*nx, S) matrix
        with the slice stride as its leading dimension"""
        shape = tuple(a.shape)
        if len(shape) != 3:
            raise ValueError("%s must have shape (ny, nx, S)" % what)
        ny, nx = shape[0], shape[1]
        ld, stride, S = _cube_view(a, ny, nx, what)
        if ld != ny:
            raise ValueError("%s: the slices must be dense (ldz == ny); this view has ldz = %d > ny = %d" % (what, ld, ny))
        return ny, nx, stride, S

    def interp_rows(self, Y, xi, out=None, extrap=math.nan):
        """mi_interp1_rows_f64_dev: one table per ROW.  Y: (m, n) float64 CUDA tensor stored column-major (the .T view of
        a C-contiguous (n, m) buffer, or a padded view of one); xi: contiguous float64 CUDA tensor of nxi queries in any
        order; out: (m, nxi) tensor in the same layout (default: the .T view of a new contiguous (nxi, m) buffer).
        Returns out with out[r, i] = interp1 of xi[i] on (X, Y[r, :]), bit-identical to interp_cols on the transposed
        data; asynchronous on the context's stream."""
        return Axis1._rows_call(self, "mi_interp1_rows_f64_dev", Y, xi, out, extrap)

    def interp_rows_nearest(self, Y, xi, out=None, extrap=math.nan):
        """interp_rows with arma::interp1's "nearest" method (mi_interp1_rows_nearest_f64_dev): out[r, i] = Y[r, k], k the
        node nearest to xi[i] (a tie keeps the left node; the stored value comes back as it is), bit-identical to
        interp_cols_nearest on the transposed data.  Arguments and layouts as interp_rows."""
        return Axis1._rows_call(self, "mi_interp1_rows_nearest_f64_dev", Y, xi, out, extrap)

    def _rows_call(self, fn, Y, xi, out, extrap):
        """the argument rules of interp_rows, written once for both methods; fn names the C function"""
        ldy, m = self._rows_view(Y, self.n, "Y")
        _need_f64_cuda(xi, "xi", True)
        _need_f64_cuda(Y, "Y", False)
        nxi = xi.numel()
        out, ldyi = _out_rows(out, m, nxi, Y)
        check(getattr(self._L, fn)(self._ctx._h, self._h, C.c_void_p(Y.data_ptr()), ldy, m, _ptr(xi), nxi,
                                   C.c_void_p(out.data_ptr()), ldyi, float(extrap)), self._ctx._h)
        return out

    def interp_stack(self, Z, ti, out=None, extrap=math.nan):
        """interp1 across the slices of a cube: Z is a (ny, nx, S) float64 CUDA tensor laid out like an arma::cube
        (_cube_view) with S == n fields, one per node of this axis, and dense slices (ldz == ny, else ValueError; the slice
        stride may exceed ny*nx); ti: contiguous float64 CUDA tensor of nti times in any order; out: (ny, nx, nti) tensor
        of the same layout (default: the .permute(2, 1, 0) view of a new contiguous (nti, nx, ny) buffer).  Returns out
        with out[i, j, k] = interp1 of ti[k] on (X, Z[i, j, :]): one call of mi_interp1_rows_f64_dev with m = ny*nx."""
        return Axis1._stack_call(self, "mi_interp1_rows_f64_dev", Z, ti, out, extrap)

    def interp_stack_nearest(self, Z, ti, out=None, extrap=math.nan):
        """interp_stack with the "nearest" method: out[i, j, k] = Z[i, j, s], s the slice whose node is nearest to ti[k]
        -- the snapshot closest in time, a zero-order hold across the slices (a tie keeps the earlier slice).  One call of
        mi_interp1_rows_nearest_f64_dev with m = ny*nx; arguments and layouts as interp_stack."""
        return Axis1._stack_call(self, "mi_interp1_rows_nearest_f64_dev", Z, ti, out, extrap)

    def _stack_call(self, fn, Z, ti, out, extrap):
        """the argument rules of interp_stack, written once for both methods; fn names the C function"""
        ny, nx, zstride, S = self._stack_view(Z, "Z")
        if S != self.n:
            raise ValueError("Z must hold one slice per node of the axis (%d), not %d" % (self.n, S))
        _need_f64_cuda(ti, "ti", True)
        _need_f64_cuda(Z, "Z", False)
        nti = ti.numel()
        out = _out_cube(out, ny, nx, nti, Z)
        oy, ox, ostride, So = self._stack_view(out, "out")
        if (oy, ox, So) != (ny, nx, nti):
            raise ValueError("out must have shape (%d, %d, %d)" % (ny, nx, nti))
        check(getattr(self._L, fn)(self._ctx._h, self._h, C.c_void_p(Z.data_ptr()), zstride, ny * nx, _ptr(ti), nti,
                                   C.c_void_p(out.data_ptr()), ostride, float(extrap)), self._ctx._h)
        return out

    def interp_cols_host(self, Y, xi, extrap=math.nan):
        """host form: Y a (n, B) numpy array (any layout; a column-major one is used in place), xi numpy queries;
        returns a Fortran-ordered (nxi, B) array (synchronous)"""
        return _cols_host(self._L, "mi_interp1_cols_f64_host", (self._ctx._h, self._h), self.n, "%d" % self.n, Y, xi, extrap,
                          self._ctx._h)


def _cols_host(L, fn, table, n, n_words, Y, xi, extrap, ctx_h=None):
    """The host form of interp1 over the columns of Y, for a context and for a group: fn names the C function of library
    L (looked up once the arguments have passed: the rules need no library), table holds its leading arguments, (ctx,
    axis) or (group, X, n); n_words says n in the shape message; ctx_h is the context a failure is reported on."""
    xi = _np64(xi)
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[0] != n:
        raise ValueError("Y must have shape (%s, B)" % n_words)
    if not Y.flags["F_CONTIGUOUS"]:
        Y = np.asfortranarray(Y)
    B = Y.shape[1]
    out = np.empty((B, xi.size)).T
    check(getattr(L, fn)(*table, C.c_void_p(Y.ctypes.data), n, B, _ptr(xi), xi.size, C.c_void_p(out.ctypes.data), xi.size,
             float(extrap)), ctx_h)
    return out


# ---- interp1 over paired columns, and interp2 over the slices of a cube -------------------------------------------

def _need_lens(lens, count, letter):
    """ValueError unless lens is None or a contiguous (count,) int32 / uint32 CUDA tensor; letter names count in the message"""
    torch = _torch()
    if lens is not None and not (lens.is_cuda and lens.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))
                                 and lens.is_contiguous() and tuple(lens.shape) == (count,)):
        raise ValueError("lens must be a contiguous int32 CUDA tensor of shape (%s,)" % letter)


def _paired_args(X, Y, queries, lens, out, want_ok):
    """What interp_pairs and interp_each share, checked in the order both keep: X and Y, then the queries -- the one
    step that differs: queries(B) returns (nxi, ldxi) -- then lens, out and ok.
    Returns (n, B, ldx, ldy, nxi, ldxi, out, ldyi, ok)."""
    torch = _torch()
    for t in (X, Y):
        _need_f64_cuda(t, "X and Y", False, "X and Y must be float64 CUDA tensors")
    if X.dim() != 2 or tuple(X.shape) != tuple(Y.shape):
        raise ValueError("X and Y must both have shape (n, B)")
    n = int(X.shape[0])
    ldx, B = Axis1._colmajor_view(X, n, "X")
    ldy, _ = Axis1._colmajor_view(Y, n, "Y")
    nxi, ldxi = queries(B)
    _need_lens(lens, B, "B")
    out, ldyi = _out_colmajor(out, nxi, B, Y)
    ok = torch.empty((B,), dtype=torch.int32, device=Y.device) if want_ok else None
    return n, B, ldx, ldy, nxi, ldxi, out, ldyi, ok


def interp_pairs(ctx, X, Y, xi, lens=None, out=None, extrap=math.nan, want_ok=False):
    """interp1 over paired columns (mi_interp1_pairs_f64_dev): column c of Y is sampled at the nodes in column c of X.

    X, Y: (n, B) float64 CUDA tensors given as column-major views (Axis1's layout rules: the .T view of a contiguous
    (B, ld) buffer; X and Y may have different leading dimensions); xi: contiguous float64 CUDA tensor of nxi queries in
    any order, shared by every column; lens: optional contiguous (B,) int32 / uint32 CUDA tensor, the number of valid
    leading rows of each column; out: column-major (nxi, B) tensor (default: the .T view of a new contiguous (B, nxi)
    buffer).  X is validated on the device at every call: a column whose length is outside [2, n] or whose nodes are not
    finite and strictly increasing gives NaN in all its outputs.  Returns the (nxi, B) result, or (result, ok) with
    want_ok=True, ok a (B,) int32 CUDA tensor (1 good, 0 bad).  Asynchronous on the context's stream."""
    return _pairs_call("mi_interp1_pairs_f64_dev", ctx, X, Y, xi, lens, out, extrap, want_ok)


def interp_pairs_nearest(ctx, X, Y, xi, lens=None, out=None, extrap=math.nan, want_ok=False):
    """interp_pairs with arma::interp1's "nearest" method (mi_interp1_pairs_nearest_f64_dev): out[i, c] = Y[k, c], k the
    node of column c of X nearest to xi[i] (a tie keeps the left node; the stored value comes back as it is) -- the state
    at the event closest to each mesh time.  Arguments, layouts, the bad-column rule and the return value as
    interp_pairs."""
    return _pairs_call("mi_interp1_pairs_nearest_f64_dev", ctx, X, Y, xi, lens, out, extrap, want_ok)


def _pairs_call(fn, ctx, X, Y, xi, lens, out, extrap, want_ok):
    """the argument rules of interp_pairs, written once for both methods; fn names the C function"""
    _need_f64_cuda(xi, "xi", True)
    n, B, ldx, ldy, nxi, _, out, ldyi, ok = _paired_args(X, Y, lambda B: (xi.numel(), 0), lens, out, want_ok)
    check(getattr(ctx._L, fn)(ctx._h, C.c_void_p(X.data_ptr()), ldx, C.c_void_p(Y.data_ptr()), ldy, n,
                              C.c_void_p(lens.data_ptr()) if lens is not None else None, B, _ptr(xi), nxi,
                              C.c_void_p(out.data_ptr()), ldyi, float(extrap),
                              C.c_void_p(ok.data_ptr()) if want_ok else None), ctx._h)
    return (out, ok) if want_ok else out


def interp_rowpairs(ctx, X, Y, xi, lens=None, out=None, extrap=math.nan, want_ok=False):
    """interp1 over paired rows (mi_interp1_rowpairs_f64_dev): row r of Y is sampled at the nodes in row r of X --
    interp_pairs for data stored the other way round, realisation-fastest, without a transpose.

    X, Y: (m, n) float64 CUDA tensors in the rows layout (Axis1._rows_view's rule: the .T view of a contiguous (n, ld)
    buffer, or a padded view of one; X and Y may have different leading dimensions); xi: contiguous float64 CUDA tensor of
    nxi queries in any order, shared by every row; lens: optional contiguous (m,) int32 / uint32 CUDA tensor, the number
    of valid leading nodes of each row; out: (m, nxi) tensor in the same layout (default: the .T view of a new contiguous
    (nxi, m) buffer).  X is validated on the device at every call: a row whose length is outside [2, n] or whose nodes are
    not finite and strictly increasing gives NaN in all its outputs.  Returns the (m, nxi) result, or (result, ok) with
    want_ok=True, ok an (m,) int32 CUDA tensor (1 good, 0 bad).  Asynchronous on the context's stream."""
    torch = _torch()
    _need_f64_cuda(xi, "xi", True)
    for t in (X, Y):
        _need_f64_cuda(t, "X and Y", False, "X and Y must be float64 CUDA tensors")
    if X.dim() != 2 or tuple(X.shape) != tuple(Y.shape):
        raise ValueError("X and Y must both have shape (m, n)")
    n = int(X.shape[1])
    ldx, m = Axis1._rows_view(X, n, "X")
    ldy, _ = Axis1._rows_view(Y, n, "Y")
    _need_lens(lens, m, "m")
    nxi = xi.numel()
    out, ldyi = _out_rows(out, m, nxi, Y)
    ok = torch.empty((m,), dtype=torch.int32, device=Y.device) if want_ok else None
    check(ctx._L.mi_interp1_rowpairs_f64_dev(ctx._h, C.c_void_p(X.data_ptr()), ldx, C.c_void_p(Y.data_ptr()), ldy, m, n,
                                             C.c_void_p(lens.data_ptr()) if lens is not None else None, _ptr(xi), nxi,
                                             C.c_void_p(out.data_ptr()), ldyi, float(extrap),
                                             C.c_void_p(ok.data_ptr()) if want_ok else None), ctx._h)
    return (out, ok) if want_ok else out


def _pairs_host_args(X, Y, xi, lens):
    xi = _np64(xi)
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    if X.ndim != 2 or X.shape != Y.shape:
        raise ValueError("X and Y must both have shape (n, B)")
    X = X if X.flags["F_CONTIGUOUS"] else np.asfortranarray(X)
    Y = Y if Y.flags["F_CONTIGUOUS"] else np.asfortranarray(Y)
    n, B = X.shape
    if lens is not None:
        lens = np.ascontiguousarray(np.asarray(lens).reshape(-1).astype(np.uint32, casting="unsafe"))
        if lens.size != B:
            raise ValueError("lens must hold one count per column")
    return X, Y, xi, lens, n, B


def _pairs_host(L, fn, h, X, Y, xi, lens, extrap, want_ok, ctx_h=None):
    """interp_pairs_host for a context and for a group: fn names the C function of library L (looked up once the
    arguments have passed), h is its context or group handle, ctx_h the context a failure is reported on"""
    X, Y, xi, lens, n, B = _pairs_host_args(X, Y, xi, lens)
    out = np.empty((B, xi.size)).T
    ok = np.ones(B, dtype=np.uint32) if want_ok else None
    check(getattr(L, fn)(h, C.c_void_p(X.ctypes.data), max(n, 1), C.c_void_p(Y.ctypes.data), max(n, 1), n,
             _ptr(lens) if lens is not None else None, B, _ptr(xi), xi.size, C.c_void_p(out.ctypes.data), max(xi.size, 1),
             float(extrap), _ptr(ok) if want_ok else None), ctx_h)
    return (out, ok) if want_ok else out


def interp_pairs_host(ctx, X, Y, xi, lens=None, extrap=math.nan, want_ok=False):
    """host form of interp_pairs (mi_interp1_pairs_f64_host): (n, B) numpy arrays (any layout; column-major ones are
    used in place), numpy queries and counts; returns a Fortran-ordered (nxi, B) array, or (array, ok) with want_ok=True
    (ok: (B,) uint32).  Synchronous.  Without want_ok a bad column raises MiError (code 2, MI_ERR_GRID)."""
    return _pairs_host(ctx._L, "mi_interp1_pairs_f64_host", ctx._h, X, Y, xi, lens, extrap, want_ok, ctx._h)


def interp_each(ctx, X, Y, XI, lens=None, out=None, extrap=math.nan, want_ok=False):
    """interp1 over paired columns with a query vector per column (mi_interp1_each_f64_dev): column c of Y, sampled at
    the nodes in column c of X, is evaluated at the queries in column c of XI.

    X, Y, lens, out, the validation of X and the return value are interp_pairs'.  XI is either a column-major (nxi, B)
    float64 CUDA view (Axis1's layout rules; its own leading dimension): the queries of each column -- or a contiguous
    1-D float64 CUDA tensor of nxi queries shared by every column (ldxi = 0): bit-identical to interp_pairs, and served by
    the thin one-lane-per-column kernel when the columns are very short.  Asynchronous on the context's stream."""
    def queries(B):
        if XI.dim() == 1:
            if not XI.is_contiguous():
                raise ValueError("a shared XI must be a contiguous 1-D tensor")
            return XI.numel(), 0
        if XI.dim() != 2:
            raise ValueError("XI must be a column-major (nxi, B) view or a contiguous 1-D tensor")
        nxi = int(XI.shape[0])
        ldxi, Bq = Axis1._colmajor_view(XI, nxi, "XI")
        if Bq != B:
            raise ValueError("XI must have as many columns as X")
        return nxi, ldxi

    _need_f64_cuda(XI, "XI", False)
    n, B, ldx, ldy, nxi, ldxi, out, ldyi, ok = _paired_args(X, Y, queries, lens, out, want_ok)
    check(ctx._L.mi_interp1_each_f64_dev(ctx._h, C.c_void_p(X.data_ptr()), ldx, C.c_void_p(Y.data_ptr()), ldy, n,
                                         C.c_void_p(lens.data_ptr()) if lens is not None else None, B,
                                         C.c_void_p(XI.data_ptr()), ldxi, nxi, C.c_void_p(out.data_ptr()), ldyi, float(extrap),
                                         C.c_void_p(ok.data_ptr()) if want_ok else None), ctx._h)
    return (out, ok) if want_ok else out


def _each_host_args(X, Y, XI, lens):
    """the host forms' arguments: (X, Y, XI, lens, n, B, nxi, ldxi); a 2-D XI must be (nxi, B), a 1-D one is shared"""
    XI = np.asarray(XI, dtype=np.float64)
    if XI.ndim == 1:
        X, Y, xi, lens, n, B = _pairs_host_args(X, Y, XI, lens)
        return X, Y, xi, lens, n, B, xi.size, 0
    X, Y, _, lens, n, B = _pairs_host_args(X, Y, np.zeros(0), lens)
    if XI.ndim != 2 or XI.shape[1] != B:
        raise ValueError("XI must have shape (nxi, B), one column of queries per column of X, or be 1-D")
    XI = XI if XI.flags["F_CONTIGUOUS"] else np.asfortranarray(XI)
    return X, Y, XI, lens, n, B, XI.shape[0], max(XI.shape[0], 1)


def _each_host(L, fn, h, X, Y, XI, lens, extrap, want_ok, ctx_h=None):
    """interp_each_host for a context and for a group; the arguments of _pairs_host"""
    X, Y, XI, lens, n, B, nxi, ldxi = _each_host_args(X, Y, XI, lens)
    out = np.empty((B, nxi)).T
    ok = np.ones(B, dtype=np.uint32) if want_ok else None
    check(getattr(L, fn)(h, C.c_void_p(X.ctypes.data), max(n, 1), C.c_void_p(Y.ctypes.data), max(n, 1), n,
             _ptr(lens) if lens is not None else None, B, C.c_void_p(XI.ctypes.data), ldxi, nxi,
             C.c_void_p(out.ctypes.data), max(nxi, 1), float(extrap), _ptr(ok) if want_ok else None), ctx_h)
    return (out, ok) if want_ok else out


def interp_each_host(ctx, X, Y, XI, lens=None, extrap=math.nan, want_ok=False):
    """host form of interp_each (mi_interp1_each_f64_host): (n, B) numpy arrays, XI an (nxi, B) array (any layout;
    column-major ones are used in place) or a 1-D array shared by every column; returns a Fortran-ordered (nxi, B) array,
    or (array, ok) with want_ok=True.  Synchronous.  Without want_ok a bad column raises MiError (code 2, MI_ERR_GRID)."""
    return _each_host(ctx._L, "mi_interp1_each_f64_host", ctx._h, X, Y, XI, lens, extrap, want_ok, ctx._h)


def interp2_slices(ctx, ax, ay, Z, xi, yi, out=None, extrap=math.nan):
    """mi_interp2_slices_f64_dev: arma::interp2's gridded output for every slice of a cube, Z read where it lies.
    ax, ay: Axis1 (nx and ny nodes; the same object is allowed); Z: (ny, nx, S) float64 CUDA tensor laid out like an
    arma::cube (see _cube_view; a padded view is taken as it is); xi, yi: contiguous float64 CUDA tensors in any order;
    out: (nyi, nxi, S) tensor of the same layout (default: the .permute(2, 1, 0) view of a new contiguous (S, nxi, nyi)
    buffer).  Returns out with out[i, j, s] = Z[:, :, s] at (xi[j], yi[i]), bit-identical to Grid2.interp_grid on that
    slice; asynchronous on the context's stream."""
    return _slices_call("mi_interp2_slices_f64_dev", ctx, ax, ay, Z, xi, yi, out, extrap)


def interp2_slices_nearest(ctx, ax, ay, Z, xi, yi, out=None, extrap=math.nan):
    """mi_interp2_slices_nearest_f64_dev: arma::interp2's "nearest" method for every slice of a cube, Z read where it
    lies.  interp2_slices' arguments, layouts and default output; out[i, j, s] = Z[ky(yi[i]), kx(xi[j]), s], the stored
    value (inf / NaN / -0.0 as they are), bit-identical to Grid2.interp_grid_nearest on that slice; asynchronous on the
    context's stream."""
    return _slices_call("mi_interp2_slices_nearest_f64_dev", ctx, ax, ay, Z, xi, yi, out, extrap)


def _slices_call(fn, ctx, ax, ay, Z, xi, yi, out, extrap):
    for t in (xi, yi):
        _need_f64_cuda(t, "query axes", True, "query axes must be contiguous float64 CUDA tensors")
    _need_f64_cuda(Z, "Z", False)
    ldz, zstride, S = _cube_view(Z, ay.n, ax.n, "Z")
    nxi, nyi = xi.numel(), yi.numel()
    out = _out_cube(out, nyi, nxi, S, Z)
    ldzi, zistride, So = _cube_view(out, nyi, nxi, "out")
    if So != S:
        raise ValueError("out must have as many slices as Z")
    check(getattr(ctx._L, fn)(ctx._h, ax._h, ay._h, C.c_void_p(Z.data_ptr()), ldz, zstride, S, _ptr(xi), nxi,
                              _ptr(yi), nyi, C.c_void_p(out.data_ptr()), ldzi, zistride, float(extrap)), ctx._h)
    return out


# ---- the reference's own step: Restrict + masked mean (EventDrivenMap.cu:769-824) ----

def restrict(ctx, t0, i0, t1, i1, final_time, half_length, ngrid, out=None):
    """RestrictKernel: CUDA tensors t0,t1 float32 and i0,i1 uint16 (or int16 views), [spike][realisation]."""
    torch = _torch()
    if out is None:
        out = torch.empty_like(t0)
    check(ctx._L.mi_restrict_f32_dev(ctx._h, _ptr(t0), _ptr(i0), _ptr(t1), _ptr(i1), float(final_time),
                                     float(half_length), int(ngrid), _ptr(out), t0.numel()), ctx._h)
    return out


def masked_mean(ctx, x, accept, nspikes, quirk=False, want_sums=False):
    torch = _torch()
    nreal = accept.numel()
    assert x.numel() == nspikes * nreal
    mean = torch.empty(nspikes, dtype=torch.float32, device=x.device)
    count = torch.empty(1, dtype=torch.int32, device=x.device)
    sums = torch.empty(2 * nspikes + 1, dtype=torch.float64, device=x.device) if want_sums else None   # [sums | count | x0]
    check(ctx._L.mi_masked_mean_f32_dev(ctx._h, _ptr(x), _ptr(accept), nreal, nspikes, int(bool(quirk)),
                                        _ptr(mean), _ptr(count), _ptr(sums) if want_sums else None), ctx._h)
    return (mean, count, sums) if want_sums else (mean, count)


def restrict_mean(ctx, t0, i0, t1, i1, accept, final_time, half_length, ngrid, nspikes, quirk=False,
                  want_restricted=False, want_sums=False):
    torch = _torch()
    nreal = accept.numel()
    assert t0.numel() == nspikes * nreal
    mean = torch.empty(nspikes, dtype=torch.float32, device=t0.device)
    count = torch.empty(1, dtype=torch.int32, device=t0.device)
    sums = torch.empty(2 * nspikes + 1, dtype=torch.float64, device=t0.device) if want_sums else None   # [sums | count | x0]
    restricted = torch.empty_like(t0) if want_restricted else None
    check(ctx._L.mi_restrict_mean_f32_dev(ctx._h, _ptr(t0), _ptr(i0), _ptr(t1), _ptr(i1), _ptr(accept),
                                          float(final_time), float(half_length), int(ngrid), nreal, nspikes,
                                          int(bool(quirk)), _ptr(restricted) if want_restricted else None,
                                          _ptr(mean), _ptr(count), _ptr(sums) if want_sums else None), ctx._h)
    return {"mean": mean, "count": count, "sums": sums, "restricted": restricted}


# ---- EventDrivenMap (EventDrivenMap.hpp:11-121) ---------------------------------------

def default_edm_params(**overrides):
    p = EdmParams()
    _lib.load().mi_edm_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError("mi_edm_params has no field %r" % k)
        setattr(p, k, v)
    return p


def _f_buffers(S, want_partial):
    """(f, partial) host buffers of one evaluation; partial has MI_EDM_PARTIAL_LEN(S) = 2 S + 1 elements, or is None"""
    return np.empty(S, dtype=np.float64), np.empty(2 * S + 1, dtype=np.float64) if want_partial else None


class EventDrivenMap(_Handle):
    """Mirror of the reference class: ComputeF(Z) -> f through lift/evolve/restrict/average."""
    _destroy = "mi_edm_destroy"

    def __init__(self, ctx, parameters, noReal, **overrides):
        self._ctx = ctx
        par = np.atleast_1d(np.asarray(parameters, dtype=np.float64))
        self.params = default_edm_params(beta_mean=float(np.float32(par[0])), n_real=int(noReal), **overrides)
        h = C.c_void_p()
        check(ctx._L.mi_edm_create(ctx._h, C.byref(self.params), C.byref(h)), ctx._h)
        self._own(ctx._L, h, ctx)
        # test / tuning hooks of the Python layer (the library itself reads no environment for this): force an evolve
        # kernel form, switch the exact quotient by launch-uniform divisors off.  Results are bit-identical either way.
        wpr = os.environ.get("MI_EDM_WAVES_PER_REALISATION", "")
        if wpr in ("1", "4") or "MI_EDM_NO_UNIFORM_DIV" in os.environ:
            self.set_kernel_choice(int(wpr) if wpr in ("1", "4") else 0, "MI_EDM_NO_UNIFORM_DIV" not in os.environ)

    def _push(self):
        check(self._L.mi_edm_set_params(self._h, C.byref(self.params)), self._ctx._h)

    def set_kernel_choice(self, waves_per_realisation=0, uniform_division=True):
        """mi_edm_set_kernel_choice: 0 / 1 / 4 waves per realisation, exact quotient by uniform divisors on / off."""
        check(self._L.mi_edm_set_kernel_choice(self._h, int(waves_per_realisation), int(bool(uniform_division))), self._ctx._h)

    # setters of EventDrivenMap.hpp:27-51
    def SetTimeHorizon(self, T):
        assert T > 0
        self.params.time_horizon = float(T)
        self._push()

    def SetNoRealisations(self, noReal):
        assert noReal > 0
        self.params.n_real = int(noReal)
        self._push()

    def SetNoThreads(self, noThreads):
        assert 0 < noThreads <= 1024
        self.params.n_grid = int(noThreads)
        self._push()

    def SetParameterStdDev(self, sigma):
        assert sigma >= 0
        self.params.beta_stddev = float(sigma)
        self._push()

    def SetParameters(self, parId, parVal):
        assert parId == 0
        self.params.beta_mean = float(parVal)
        self._push()

    def SetSeed(self, seed):
        self.params.seed = int(seed)
        self._push()

    def PostProcess(self):
        """EventDrivenMap.cu:343-346 draws a new seed; here: advance it deterministically."""
        self.params.seed = (int(self.params.seed) * 6364136223846793005 + 1442695040888963407) & (2**64 - 1)
        self._push()

    def ComputeF(self, Z, want_partial=False):
        Z = _np64(Z)
        S = int(self.params.n_spikes)
        if Z.size != S:
            raise ValueError("Z must have n_spikes=%d elements" % S)
        f, partial = _f_buffers(S, want_partial)
        check(self._L.mi_edm_compute_f(self._h, _ptr(Z), _ptr(f), _ptr(partial) if want_partial else None),
              self._ctx._h)
        return (f, partial) if want_partial else f

    def begin(self, Z):
        """Enqueue one evaluation and return at once (mi_edm_compute_f_begin); collect it with end()."""
        Z = _np64(Z)
        if Z.size != int(self.params.n_spikes):
            raise ValueError("Z must have n_spikes=%d elements" % int(self.params.n_spikes))
        check(self._L.mi_edm_compute_f_begin(self._h, _ptr(Z)), self._ctx._h)

    def end(self, want_partial=False):
        f, partial = _f_buffers(int(self.params.n_spikes), want_partial)
        check(self._L.mi_edm_compute_f_end(self._h, _ptr(f), _ptr(partial) if want_partial else None), self._ctx._h)
        return (f, partial) if want_partial else f

    def ComputeFBatch(self, Zs, want_partial=False):
        """Several independent evaluations at once (the columns of a finite-difference Jacobian): every
        evaluation runs on a replica of this problem with a context and stream of its own, all are enqueued before
        any is waited for, so they overlap on the device.  Returns F[b] (and partial[b]) in the order of Zs; each
        equals what ComputeF(Zs[b]) returns."""
        Zs = [np.asarray(z, dtype=np.float64) for z in Zs]
        reps = getattr(self, "_replicas", None)
        if reps is None:
            reps = self._replicas = []
        while len(reps) < len(Zs):
            ctx = Context(self._ctx.device, stream=None)
            ctx.own_stream()
            h = C.c_void_p()
            par = EdmParams()
            C.memmove(C.byref(par), C.byref(self.params), C.sizeof(EdmParams))
            check(self._L.mi_edm_create(ctx._h, C.byref(par), C.byref(h)), ctx._h)
            rep = EventDrivenMap.__new__(EventDrivenMap)
            rep._ctx, rep._L, rep.params, rep._h = ctx, self._L, par, h
            reps.append(rep)
        mine = bytes(self.params)
        for rep in reps[:len(Zs)]:
            if bytes(rep.params) != mine:                      # a setter ran on the parent since the last batch
                C.memmove(C.byref(rep.params), C.byref(self.params), C.sizeof(EdmParams))
                rep._push()
        begun = []
        try:
            for rep, z in zip(reps, Zs):
                rep.begin(z)
                begun.append(rep)
            out = [rep.end(want_partial) for rep in reps[:len(Zs)]]
            begun = []
        finally:
            for rep in begun:                                  # a begin() or end() raised: nothing may stay pending
                try:
                    rep._push()                                # mi_edm_set_params drains the stream and abandons the evaluation
                except Exception:
                    pass
        if want_partial:
            return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        return np.stack(out)

    def residual_from_sums(self, Z, sums_and_count):
        Z, sc = _np64(Z), _np64(sums_and_count)
        f = np.empty(int(self.params.n_spikes), dtype=np.float64)
        check(self._L.mi_edm_residual_from_sums(C.byref(self.params), _ptr(Z), _ptr(sc), _ptr(f)), self._ctx._h)
        return f

    def debug_read(self):
        """Stage outputs of the last ComputeF (the reference's Save* taps, EventDrivenMap.cu:406-503)."""
        return _edm_debug_read(self._L, self._h, self.params, self._ctx._h)

    def debug_counters(self):
        """Decision-coverage taps of the last ComputeF (mi_edm_debug_counters: one more, tapped, evolve)."""
        c = (C.c_uint64 * 8)()
        check(self._L.mi_edm_debug_counters(self._h, C.byref(c)), self._ctx._h)
        names = ("events", "max_events_one", "max_newton_iter", "newton_cap_hits", "event_cap_hits", "accepted",
                 "no_firing_events", "argmin_ties")
        return {n: int(c[i]) for i, n in enumerate(names)}

    def last_timings(self):
        ms = (C.c_float * 4)()
        check(self._L.mi_edm_last_timings(self._h, C.byref(ms)), self._ctx._h)
        return {"lift_ms": ms[0], "evolve_ms": ms[1], "restrict_mean_ms": ms[2], "total_ms": ms[3]}

    def close(self):
        for rep in getattr(self, "_replicas", None) or []:
            rep.close()
        self._replicas = []
        super().close()


def _edm_debug_read(L, h, params, ctx_h=None):
    """mi_edm_debug_read of handle h, whose current parameters are params (n_spikes, n_real and n_grid size the taps)."""
    S, R, N = int(params.n_spikes), int(params.n_real), int(params.n_grid)
    out = {
        "v": np.empty(N, np.float32), "s": np.empty(N, np.float32), "w": np.empty(N, np.float32),
        "t0": np.empty(S * R, np.float32), "i0": np.empty(S * R, np.uint16),
        "t1": np.empty(S * R, np.float32), "i1": np.empty(S * R, np.uint16),
        "accept": np.empty(R, np.uint32), "restricted": np.empty(S * R, np.float32),
        "seed_ind": np.empty(S, np.uint16),
    }
    order = ["v", "s", "w", "t0", "i0", "t1", "i1", "accept", "restricted", "seed_ind"]
    check(L.mi_edm_debug_read(h, *[_ptr(out[k]) for k in order]), ctx_h)
    return out


# ---- several GPUs of one node, one host process (mi_group_*) ---------------------------------------------------

def shard_bounds(n, rank, world):
    """mi_shard_bounds: contiguous balanced split (host arithmetic of the C ABI; equals sharding.shard_bounds)."""
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    _lib.load().mi_shard_bounds(int(n), int(rank), int(world), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class _GroupCtx:
    """borrowed view of a group member's context (owned by the group)"""

    def __init__(self, L, h, device):
        self._L, self._h, self.device = L, h, device

    def timer(self):
        """HIP events on this member's stream (the stream its shard's kernels are launched on)"""
        return Timer(self)

    def device_info(self):
        return Context.device_info(self)


class Group(_Handle):
    """One process driving several GPUs: devices = [0, 1, ..] (a repeated ordinal rehearses the sharding on one GPU)."""
    REDUCE_HOST, REDUCE_RCCL = 0, 1
    _destroy = "mi_group_destroy"

    def __init__(self, devices):
        L = _lib.load()
        devices = list(range(devices)) if isinstance(devices, int) else [int(d) for d in devices]
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        check(L.mi_group_create(len(devices), arr, C.byref(h)))
        self._own(L, h)
        self.devices = devices

    def __len__(self):
        return int(self._L.mi_group_size(self._h))

    def ctx(self, rank):
        return _GroupCtx(self._L, C.c_void_p(self._L.mi_group_ctx(self._h, int(rank))), self.devices[rank])

    def set_reduce(self, mode):
        check(self._L.mi_group_set_reduce(self._h, int(mode)))

    def set_gather_chunks(self, chunks):
        """mi_group_set_gather_chunks: >= 2 hides the gather of interp_dev(gather=True) behind the kernels, chunk by chunk"""
        check(self._L.mi_group_set_gather_chunks(self._h, int(chunks)))

    def rccl_ranks(self):
        """ranks of the group's RCCL communicator as RCCL reports it (ncclCommCount); 0: no communicator possible"""
        return int(self._L.mi_group_rccl_ranks(self._h))

    def synchronize(self):
        check(self._L.mi_group_synchronize(self._h))

    def wait_stream(self, rank, raw_stream):
        """mi_group_wait_stream: member `rank`'s stream waits (on the device) for what `raw_stream` holds now"""
        check(self._L.mi_group_wait_stream(self._h, int(rank), C.c_void_p(raw_stream)))

    def _follow_torch(self):
        """every member's stream behind torch's current stream of its device: tensors handed to the next call may still be
        produced, or last written, there.  Stream-ordered (an event and a device-side wait per member), no host wait."""
        torch = _torch()
        for r, d in enumerate(self.devices):
            self.wait_stream(r, torch.cuda.current_stream(d).cuda_stream)

    def grid1(self, X, Y, sanitise=True):
        X, Y = _np64(X), _np64(Y)
        t = C.c_void_p()
        check(self._L.mi_group_grid1_create(self._h, _ptr(X), _ptr(Y), X.size, 1 if sanitise else 0, C.byref(t)))
        return GroupGrid1(self, t)

    def grid2(self, x, y, z, compact=False):
        """2-D table replicated on every device; z is (len(y), len(x))"""
        x, y = _np64(x), _np64(y)
        zc = Grid2._colmajor(z, y.size, x.size)
        t = C.c_void_p()
        check(self._L.mi_group_grid2_create(self._h, _ptr(x), x.size, _ptr(y), y.size, _ptr(zc),
                                            MI_GRID2_COMPACT if compact else 0, C.byref(t)))
        return GroupGrid2(self, t)

    def interp_cols_host(self, X, Y, xi, extrap=math.nan):
        """interp1 over the columns of Y (Axis1.interp_cols_host) with the columns sharded over the group's devices;
        X (n nodes, used as given) and xi are replicated.  Y: (n, B) numpy array; returns a Fortran-ordered (nxi, B) array."""
        X = _np64(X)
        return _cols_host(self._L, "mi_group_interp1_cols_f64_host", (self._h, _ptr(X), X.size), X.size, "len(X)", Y, xi, extrap)

    def interp_pairs_host(self, X, Y, xi, lens=None, extrap=math.nan, want_ok=False):
        """interp1 over paired columns (interp_pairs_host) with the columns sharded over the group's devices; xi is
        replicated.  Returns a Fortran-ordered (nxi, B) array, or (array, ok) with want_ok=True."""
        return _pairs_host(self._L, "mi_group_interp1_pairs_f64_host", self._h, X, Y, xi, lens, extrap, want_ok)

    def interp_each_host(self, X, Y, XI, lens=None, extrap=math.nan, want_ok=False):
        """interp1 over paired columns with a query vector per column (interp_each_host) with the columns sharded over
        the group's devices; a 2-D XI is sharded with its columns, a 1-D one is replicated."""
        return _each_host(self._L, "mi_group_interp1_each_f64_host", self._h, X, Y, XI, lens, extrap, want_ok)

    def edm(self, parameters, noReal, **overrides):
        return GroupEventDrivenMap(self, parameters, noReal, **overrides)


class GroupGrid1(_Handle):
    _destroy = "mi_group_grid1_destroy"

    def __init__(self, group, h):
        self._g = group
        self._own(group._L, h)

    def interp_host(self, xq, extrap=math.nan):
        """host arrays in, host array out; the queries are sharded over the group's devices"""
        xq = _np64(xq)
        out = np.empty_like(xq)
        check(self._L.mi_group_interp1_f64_host(self._g._h, self._h, _ptr(xq), _ptr(out), xq.size, float(extrap)))
        return out

    def interp_dev(self, xq_shards, extrap=math.nan, gather=False, out=None, gathered=None, sync=True):
        """device-resident shards (one float64 tensor per group member, equal sizes); returns the per-shard results and,
        with gather=True, one buffer per member holding every shard (RCCL all-gather, or device copies in a rehearsal group).
        out / gathered: caller-owned result tensors (no allocation in the call); sync=False: return with the shards'
        kernels enqueued on the members' streams (Group.synchronize waits) -- the shape bench.py --backend group times.
        Ordering: the members' streams are put behind torch's current stream of their device first, so the work that
        produces xq_shards, or that last wrote out / gathered, may still be pending there when this is called.  With
        sync=True the results are complete on return; with sync=False after Group.synchronize()."""
        torch = _torch()
        P, n = len(self._g), int(xq_shards[0].numel())
        assert len(xq_shards) == P and all(int(t.numel()) == n for t in xq_shards)
        outs = out if out is not None else [torch.empty_like(t) for t in xq_shards]
        assert len(outs) == P and all(int(t.numel()) == n and t.dtype == torch.float64 and t.is_contiguous() for t in outs)
        full = gathered
        if gather and full is None:
            full = [torch.empty(P * n, dtype=torch.float64, device=t.device) for t in xq_shards]
        if gather:
            assert len(full) == P and all(int(t.numel()) == P * n for t in full)
        arr = lambda ts: (C.c_void_p * P)(*[t.data_ptr() for t in ts])  # noqa: E731
        self._g._follow_torch()
        check(self._L.mi_group_interp1_f64_dev(self._g._h, self._h, arr(xq_shards), arr(outs), n, float(extrap),
                                               arr(full) if gather else None))
        if sync:
            self._g.synchronize()
        return (outs, full) if gather else outs


class GroupGrid2(_Handle):
    _destroy = "mi_group_grid2_destroy"

    def __init__(self, group, h):
        self._g = group
        self._own(group._L, h)

    def interp_host(self, xq, yq, extrap=math.nan):
        """host arrays in, host array out; the scattered queries are sharded over the group's devices"""
        xq, yq = _np64(xq), _np64(yq)
        if xq.size != yq.size:
            raise ValueError("xq and yq must have the same number of elements")
        out = np.empty_like(xq)
        check(self._L.mi_group_interp2_f64_host(self._g._h, self._h, _ptr(xq), _ptr(yq), _ptr(out), xq.size, float(extrap)))
        return out

    def interp_grid_host(self, xi, yi, extrap=math.nan):
        """gridded form (Grid2.interp_grid_host): the columns are sharded over the group's devices, yi replicated"""
        xi, yi = _np64(xi), _np64(yi)
        out = np.empty((xi.size, yi.size))
        check(self._L.mi_group_interp2_grid_f64_host(self._g._h, self._h, _ptr(xi), xi.size, _ptr(yi), yi.size, _ptr(out),
                                                     float(extrap)))
        return out.T

    def interp_dev(self, xq_shards, yq_shards, extrap=math.nan, gather=False):
        """device-resident shards (one pair of float64 tensors per group member, equal sizes).  The members' streams are put
        behind torch's current stream of their device first (the shards' producers may still be pending there); the
        results are complete on return."""
        torch = _torch()
        P, n = len(self._g), int(xq_shards[0].numel())
        assert len(xq_shards) == P and len(yq_shards) == P
        assert all(int(t.numel()) == n for t in xq_shards) and all(int(t.numel()) == n for t in yq_shards)
        outs = [torch.empty_like(t) for t in xq_shards]
        full = [torch.empty(P * n, dtype=torch.float64, device=t.device) for t in xq_shards] if gather else None
        arr = lambda ts: (C.c_void_p * P)(*[t.data_ptr() for t in ts])  # noqa: E731
        self._g._follow_torch()
        check(self._L.mi_group_interp2_f64_dev(self._g._h, self._h, arr(xq_shards), arr(yq_shards), arr(outs), n,
                                               float(extrap), arr(full) if gather else None))
        self._g.synchronize()
        return (outs, full) if gather else outs


class GroupEventDrivenMap(_Handle):
    """EventDrivenMap with the realisations sharded over a Group; noReal is the total."""
    _destroy = "mi_group_edm_destroy"

    def __init__(self, group, parameters, noReal, **overrides):
        self._g = group
        par = np.atleast_1d(np.asarray(parameters, dtype=np.float64))
        self.params = default_edm_params(beta_mean=float(np.float32(par[0])), n_real=int(noReal), **overrides)
        h = C.c_void_p()
        check(group._L.mi_group_edm_create(group._h, C.byref(self.params), C.byref(h)))
        self._own(group._L, h)

    def _push(self):
        check(self._L.mi_group_edm_set_params(self._h, C.byref(self.params)))

    def ComputeF(self, Z, want_partial=False):
        Z = _np64(Z)
        f, partial = _f_buffers(int(self.params.n_spikes), True)       # partial is always asked for, returned only if wanted
        check(self._L.mi_group_edm_compute_f(self._h, _ptr(Z), _ptr(f), _ptr(partial)))
        return (f, partial) if want_partial else f

    def shard_bounds(self, rank):
        lo, hi = C.c_size_t(0), C.c_size_t(0)
        check(self._L.mi_group_edm_shard_bounds(self._h, int(rank), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def shard_debug_read(self, rank):
        """Stage taps of the last ComputeF on shard `rank` (mi_group_edm_shard + mi_edm_debug_read): its realisations
        [lo, hi) of shard_bounds(rank), laid out [spike][realisation of the shard]."""
        h = self._L.mi_group_edm_shard(self._h, int(rank))
        if not h:
            raise ValueError("no shard %r in this group" % (rank,))
        lo, hi = self.shard_bounds(rank)
        par = EdmParams()
        C.memmove(C.byref(par), C.byref(self.params), C.sizeof(EdmParams))
        par.n_real = hi - lo
        return _edm_debug_read(self._L, C.c_void_p(h), par)
