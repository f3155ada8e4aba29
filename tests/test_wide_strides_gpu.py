"""The strided entry points at element offsets beyond 2^32 (mi_interp1_cols_f64_dev, mi_interp1_pairs_f64_dev,
mi_interp1_each_f64_dev, mi_interp1_rows_f64_dev, mi_interp1_rowpairs_f64_dev, mi_interp2_slices_f64_dev), through the
public Python API.  tests/wide_stride_cases.py holds the cases, the construction and the checking function, and says why
no 32-bit misreading of an offset can leave the pool; tests/test_wide_stride_cases_cpu.py proves that the checking
function refuses each such misreading.

One module-scoped pool of 3*2^31 + 2^22 doubles (about 51.6 GB) is allocated with torch.empty, never filled as a
whole and given back to the device in the fixture's teardown, which asserts that it was; every wide operand is a torch.as_strided view of it, every other operand a small tensor of its own, so that yi
never overlaps an input.  Per case: plant the true data, the decoys and the sentinels, make the call, read the windows
back, check() -- results equal to oracle.interp1_bracket / oracle.interp2_bilinear bit for bit, sentinels and guards
intact, true output elements all written, flags right, the form counter moved by one in the expected form -- and the same
call once more with the wide operand replaced by a compact copy: identical bits."""
import gc

import numpy as np
import pytest

import wide_stride_cases as W
from wide_stride_cases import CASES

pytestmark = pytest.mark.gpu

MIN_HBM = 96 * 2**30              # the module skips on a device with less memory (never an MI355X)


@pytest.fixture(scope="module")
def pool(mi_ctx):
    """[the pool tensor]: a holder, not the tensor.  pytest keeps what a fixture yields (the fixture's cached result, the
    last test's arguments) until after the fixture's teardown has run, so a tensor yielded itself would still be referenced
    when the teardown empties torch's cache and would stay reserved by torch: the library, whose hipMalloc does not go
    through torch, would never see the 51.6 GB again.  The teardown empties the holder, which drops the only reference, and
    asserts that torch's reserved memory is back to within 1 GiB of what it was before the allocation."""
    import torch
    hbm = mi_ctx.device_info()["hbm_bytes"]
    if hbm < MIN_HBM:
        pytest.skip("the %.1f GB pool needs a device with 96 GiB; this one has %.1f GiB" % (W.POOL * 8 / 1e9, hbm / 2**30))
    torch.cuda.empty_cache()
    before = torch.cuda.memory_reserved(0)
    holder = [torch.empty(W.POOL, dtype=torch.float64, device="cuda:0")]     # a failed allocation is an error, not a skip
    assert holder[0].data_ptr() % 16 == 0 and torch.cuda.memory_reserved(0) >= before + W.POOL * 8
    yield holder
    holder.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    after = torch.cuda.memory_reserved(0)
    assert after < before + 2**30, "the pool was not given back: torch reserves %d bytes, %d before the module" % (after, before)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _compact(case, name, values=None):
    """a small tensor of its own for operand `name`, laid out column-major (slice by slice) with the case's compact leading
    dimension: the (rows, cols) or (rows, cols, S) view the API takes; values None: an output, pre-filled"""
    rows, cols, S = case._shape3(name)
    ld = case.compact_ld(name)
    h = np.full((S, cols, ld), W.SENT_GUARD if values is None else np.nan)
    if values is not None:
        h[:, :, :rows] = np.asarray(values, dtype=np.float64).reshape(rows, cols, S).transpose(2, 1, 0)
    buf = _t(h)
    assert buf.data_ptr() % 16 == 0
    v = buf[:, :, :rows].permute(2, 1, 0)
    return v if name in ("Z", "ZI") else v[:, :, 0]


def _wide(case, pool):
    """the wide operand: a view of the pool"""
    import torch
    rows, cols, S = case.wshape
    s = case.view_strides()
    if case.operand in ("Z", "ZI"):
        return torch.as_strided(pool, (rows, cols, S), s, case.base)
    return torch.as_strided(pool, (rows, cols), s[:2], case.base)


def _forms(ctx, case):
    if case.call not in W.COUNTERS:
        return None
    name, n = W.COUNTERS[case.call]
    return [int(getattr(ctx._L, name)(f)) for f in range(n)]


def _call(ctx, case, ops, out):
    """the public call of the case on the operand tensors ops; returns (result tensor, ok tensor or None)"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    A = case.arrays
    lens = torch.from_numpy(A["lens"]).cuda() if "lens" in A else None
    want_ok = lens is not None
    if case.call in ("cols", "rows"):
        ax = mi.Axis1.from_nodes(ctx, A["x"])
        fn = ax.interp_cols if case.call == "cols" else ax.interp_rows
        return fn(ops["Y"], _t(A["xi"]), out=out, extrap=W.EXTRAP), None
    if case.call == "slices2":
        ax, ay = mi.Axis1.from_nodes(ctx, A["ax"]), mi.Axis1.from_nodes(ctx, A["ay"])
        return mi.interp2_slices(ctx, ax, ay, ops["Z"], _t(A["xi"]), _t(A["yi"]), out=out, extrap=W.EXTRAP), None
    if case.call == "each":
        r = mi.interp_each(ctx, ops["X"], ops["Y"], ops["XI"], lens=lens, out=out, extrap=W.EXTRAP, want_ok=want_ok)
    else:
        fn = mi.interp_pairs if case.call == "pairs" else mi.interp_rowpairs
        r = fn(ctx, ops["X"], ops["Y"], _t(A["xi"]), lens=lens, out=out, extrap=W.EXTRAP, want_ok=want_ok)
    return r if want_ok else (r, None)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_wide_operand(mi_ctx, pool, case):
    import torch
    pool = pool[0]                                             # (the fixture yields a holder: see there)

    def write(start, img):
        pool[start:start + img.size].copy_(torch.from_numpy(img))

    def read(start, n):
        return pool[start:start + n].cpu().numpy()

    case.plant(write)
    inputs = [name for name in ("X", "Y", "XI", "Z") if name in case.arrays]
    outname = "ZI" if case.call == "slices2" else "YI"
    wide = _wide(case, pool)
    assert wide.stride()[2 if case.how == "slice" else 1] == case.stride and (wide.data_ptr() % 16 != 0) == bool(case.align)
    ops = {name: wide if name == case.operand else _compact(case, name, case.arrays[name]) for name in inputs}
    out = wide if case.role == "out" else _compact(case, outname)
    before = _forms(mi_ctx, case)
    got, ok = _call(mi_ctx, case, ops, out)
    torch.cuda.synchronize()
    after = _forms(mi_ctx, case)
    delta = None if before is None else [a - b for a, b in zip(after, before)]
    ok = None if ok is None else ok.cpu().numpy()
    if case.role == "in":
        got = got.cpu().numpy()
    else:                                                      # block by block: no torch kernel walks the wide view
        assert got.data_ptr() == wide.data_ptr()
        got = np.empty(case.wshape)
        for b in case.blocks():
            got[b.sel] = read(case.base + b.D, b.span)[b.idx]
        got = got.reshape(case.out_shape())
    W.check(case, read, None if case.role == "out" else got, ok, delta)
    # the same call with the wide operand replaced by a compact copy: identical bits
    if case.role == "in":
        ops[case.operand] = _compact(case, case.operand, case.arrays[case.operand])
    again, ok2 = _call(mi_ctx, case, ops, _compact(case, outname))
    assert W.same_bits(again.cpu().numpy(), got), "%s: the compact copy gives other bits" % case.id
    assert ok is None or np.array_equal(ok2.cpu().numpy(), ok)
