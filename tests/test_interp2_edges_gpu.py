"""GPU checks of the bilinear kernels -- scattered (csrc/mi_interp2.hip) and gridded (csrc/mi_interp2_grid.hip: locate,
flat and tile kernels, each with 16-B and 8-B stores) -- on the cases of tests/interp2_cases.py: tables whose Z holds
inf, NaN, -0.0 and denormals where a kernel has to select a table element away (the compact layout's next-column element
behind the last row, its zero padding element, the quad layout's duplicated last row and column, the (xmin, ymin)
evaluation of an out-of-range query, the cells the tile kernel keeps in registers across columns), and a query on every
node, ulp neighbour and midpoint of both axes.

EVERY element is compared with oracle.interp2_bilinear (interp2_bilinear_uniform for the implicit table), itself held to
a literal scan, to the exact rational result and to the reach property in tests/test_interp2_cases_cpu.py: NaN where the
oracle has NaN, the same 64 bits everywhere else, the sign of zero included.  Every case runs on both resident layouts.

Nothing reports which gridded kernel ran: the dispatch rule of mi_interp2_grid_f64_dev (flat below 256 rows, tile from
256; 16-B stores when the result is 16-B aligned and, in the tile form, nyi is even) is what selects it, and GRID_FORMS
lists the smallest shape of each.  The tile kernel cuts the columns into strips of ceil(nxi / (32 CUs / row blocks))
columns and starts every strip with empty registers, so with a few hundred columns a strip is ONE column and the
`X.l != lx` cache is never used: test_tile_kernel_keeps_cells_across_the_columns_of_a_strip repeats the cache-exercising
columns until a strip is 17 columns long (the pattern's period is 90, so the strips start at every phase of it), and
compares on the device with the oracle's answer on one period."""
import ctypes as C
import math

import numpy as np
import pytest

import interp2_cases as ic

pytestmark = pytest.mark.gpu

SENT = -12345.678
GUARD = 512
PREFIXES = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1025)      # a workgroup is 256 lanes of two queries
ALL_EXTRAPS_TABLE = "guess_bsearch"                           # NaN and -3.25 everywhere, -0.0 and +inf here
# nyi -> the form mi_interp2_grid_f64_dev picks for a 16-B aligned result
GRID_FORMS = {1: "flat", 2: "flat", 254: "flat, 16-B stores", 255: "flat, 8-B stores", 256: "tile, one row block, 16-B",
              257: "tile, 8-B stores, second row in i0 + 256", 514: "tile, two row blocks, 16-B", 515: "tile, two row blocks, 8-B"}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _extraps(name):
    return (math.nan, -3.25, -0.0, math.inf) if name == ALL_EXTRAPS_TABLE else (math.nan, -3.25)


def _make(mi_ctx, name, compact):
    import armadillocudalinearinterpolation_amd as mi
    t = ic.table(name)
    if t["uniform"]:
        x0, dx, y0, dy = t["uniform"]
        return mi.Grid2.uniform(mi_ctx, x0, dx, t["xg"].size, y0, dy, t["yg"].size, t["Z"], compact=compact)
    return mi.Grid2.from_axes(mi_ctx, t["xg"], t["yg"], t["Z"], compact=compact)


@pytest.fixture(scope="module")
def grids(mi_ctx):
    """(table name, compact) -> Grid2, built on first use"""
    made = {}

    def get(name, compact):
        if (name, compact) not in made:
            made[name, compact] = _make(mi_ctx, name, compact)
        return made[name, compact]
    yield get
    for g in made.values():
        g.close()


_REFS = {}


def _scattered_ref(name):
    """the oracle on the full scattered vector, computed once"""
    if name not in _REFS:
        xq, yq = ic.scattered(name)
        _REFS[name] = ic.reference(name, xq, yq)
        _REFS[name].setflags(write=False)
    return _REFS[name]


def _report(tag, got, ref, xq, yq, t):
    """the first mismatches: index, query, bracket and the four table elements"""
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    bad = np.flatnonzero(~np.where(np.isnan(ref), np.isnan(got), got.view(np.int64) == ref.view(np.int64)))
    lines = ["%r: %d of %d differ" % (tag, bad.size, ref.size)]
    xg, yg, Z = t["xg"], t["yg"], t["Z"]
    for k in bad[:12]:
        where = "out of range / NaN"
        if ic.in_range(xq[k:k + 1], yq[k:k + 1], xg, yg)[0]:
            (lx,), (rx,) = ic.brackets(xg, xq[k:k + 1])
            (ly,), (ry,) = ic.brackets(yg, yq[k:k + 1])
            where = "lx %d ly %d corners %r %r %r %r" % (lx, ly, Z[ly, lx], Z[ry, lx], Z[ly, rx], Z[ry, rx])
        lines.append("  index %d query (%r, %r) got %s want %s %s" % (k, xq[k], yq[k], float(got[k]).hex(), float(ref[k]).hex(), where))
    return "\n".join(lines)


def _check(tag, got, ref, xq, yq, t):
    assert ic.same_bits(got, ref), _report(tag, got, ref, xq, yq, t)


@pytest.mark.parametrize("name", ic.TABLES)
def test_scattered_every_element_bit_for_bit(mi_ctx, grids, name):
    """Grid2.interp on the full vector (odd length: the tail element goes to the first lane past the vectors), on its
    prefixes around the workgroup size, and from its second element (8-byte aligned only: the scalar kernel); the 512
    doubles behind every result keep their sentinel"""
    import torch
    t = ic.table(name)
    xq, yq = ic.scattered(name)
    ref_nan = _scattered_ref(name)
    nq = xq.size
    xd, yd = _t(xq), _t(yq)
    buf = torch.empty(nq + GUARD, dtype=torch.float64, device="cuda")
    assert xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    for compact in (False, True):
        grid = grids(name, compact)
        assert grid.info()["table_bytes"] == t["xg"].size * t["yg"].size * (16 if compact else 32)
        for extrap in _extraps(name):
            ref = ref_nan if extrap != extrap else ic.with_extrap(ref_nan, xq, yq, t["xg"], t["yg"], extrap)
            for m in (nq,) + tuple(p for p in PREFIXES if p < nq):
                buf.fill_(SENT)
                grid.interp(xd[:m], yd[:m], out=buf[:m], extrap=extrap)
                b = buf.cpu().numpy()
                _check((name, compact, extrap, m), b[:m], ref[:m], xq, yq, t)
                assert np.all(b[m:] == SENT), ("guard", name, compact, extrap, m)
            buf.fill_(SENT)
            grid.interp(xd[1:], yd[1:], out=buf[1:nq], extrap=extrap)            # the scalar kernel
            b = buf.cpu().numpy()
            _check((name, compact, extrap, "from the second element"), b[1:nq], ref[1:], xq[1:], yq[1:], t)
            assert b[0] == SENT and np.all(b[nq:] == SENT), ("guard", name, compact, extrap, "scalar")


def _gridded_case(mi_ctx, grids, name, nyi, offset):
    """one table through interp_grid at nyi rows: against the oracle on the meshgrid pairs and against Grid2.interp on
    the same pairs, both layouts, its extrapolation values; offset: the result starts 8 bytes into a 16-B aligned buffer"""
    import torch
    from armadillocudalinearinterpolation_amd._lib import check
    t = ic.table(name)
    xi, yi = ic.grid_xi(t["xg"]), ic.grid_yi(t["yg"], nyi, seed=nyi)
    nxi = xi.size
    px, py = ic.mesh_pairs(xi, yi)
    ref_nan = ic.reference(name, px, py)
    xd, yd, pxd, pyd = _t(xi), _t(yi), _t(px), _t(py)
    buf = torch.empty(nxi * nyi + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0
    for compact in (False, True):
        grid = grids(name, compact)
        for extrap in _extraps(name):
            ref = ref_nan if extrap != extrap else ic.with_extrap(ref_nan, px, py, t["xg"], t["yg"], extrap)
            buf.fill_(SENT)
            if offset:
                check(grid._L.mi_interp2_grid_f64_dev(mi_ctx._h, grid._h, C.c_void_p(xd.data_ptr()), nxi, C.c_void_p(yd.data_ptr()),
                                                      nyi, C.c_void_p(buf.data_ptr() + 8), float(extrap)), mi_ctx._h)
                lo = 1
            else:
                zi = grid.interp_grid(xd, yd, out=buf[:nxi * nyi].view(nxi, nyi), extrap=extrap)
                assert tuple(zi.shape) == (nyi, nxi)
                lo = 0
            b = buf.cpu().numpy()
            _check((name, nyi, compact, extrap, offset), b[lo:lo + nxi * nyi], ref, px, py, t)
            assert np.all(b[:lo] == SENT) and np.all(b[lo + nxi * nyi:] == SENT), ("guard", name, nyi, compact, extrap)
            scattered = grid.interp(pxd, pyd, extrap=extrap).cpu().numpy()
            _check((name, nyi, compact, extrap, "Grid2.interp on the pairs"), scattered, ref, px, py, t)


@pytest.mark.parametrize("nyi", list(GRID_FORMS), ids=["nyi%d" % n for n in GRID_FORMS])
def test_gridded_every_form_bit_for_bit(mi_ctx, grids, nyi):
    """every table at the smallest shape of each form (GRID_FORMS), XI the cache-exercising columns of interp2_cases"""
    for name in ic.TABLES:
        _gridded_case(mi_ctx, grids, name, nyi, offset=False)


@pytest.mark.parametrize("nyi", [256, 514])
def test_gridded_output_offset_by_8_bytes(mi_ctx, grids, nyi):
    """a result pointer that is 8-B but not 16-B aligned forces the 8-B store form on an even nyi"""
    for name in ic.TABLES:
        _gridded_case(mi_ctx, grids, name, nyi, offset=True)


@pytest.mark.parametrize("nyi", [256, 257, 514, 515])
def test_tile_kernel_keeps_cells_across_the_columns_of_a_strip(mi_ctx, grids, nyi):
    """strips of 17 columns (module docstring): runs inside one table column interrupted by flagged columns, by a
    column of the next cell and by xmax, starting at every phase of the pattern.  The columns repeat with the pattern's
    period, so the oracle's answer on one period is the answer on all of it; compared on the device."""
    import torch
    name = "guess_bsearch"
    t = ic.table(name)
    period = ic.cache_xi(t["xg"])
    P = period.size
    nrb = (nyi + 511) // 512                                           # row blocks of 512 rows
    strips = mi_ctx.device_info()["compute_units"] * 32 // nrb         # the most strips the launch makes
    nxi = 16 * strips + 1
    assert P == 90 and -(-nxi // min(nxi, strips)) == 17
    xi = np.resize(period, nxi)
    yi = ic.grid_yi(t["yg"], nyi, seed=nyi)
    px, py = ic.mesh_pairs(period, yi)
    extrap = -3.25
    ref = ic.with_extrap(ic.reference(name, px, py), px, py, t["xg"], t["yg"], extrap).reshape(P, nyi)
    assert np.isfinite(ref).sum() > ref.size // 4 and np.isnan(ref).any() and (ref == extrap).any()
    col = torch.arange(nxi, device="cuda") % P
    ref_bits = torch.from_numpy(ref.view(np.int64)).cuda()[col]
    ref_nan = torch.from_numpy(np.isnan(ref)).cuda()[col]
    xd, yd = _t(xi), _t(yi)
    out = torch.empty((nxi, nyi), dtype=torch.float64, device="cuda")
    for compact in (False, True):
        out.fill_(SENT)
        grids(name, compact).interp_grid(xd, yd, out=out, extrap=extrap)
        ok = torch.where(ref_nan, torch.isnan(out), out.view(torch.int64) == ref_bits)
        if not bool(ok.all()):
            bad = torch.nonzero(~ok)[:12].cpu().numpy()
            msg = ["column %d (pattern position %d, strip position %d) row %d got %s want %s" % (
                j, j % P, j % 17, i, float(out[j, i]).hex(), float(ref[j % P, i]).hex()) for j, i in bad]
            raise AssertionError("%s compact=%s: %d differ\n%s" % (name, compact, int((~ok).sum()), "\n".join(msg)))


def test_host_and_group_paths(mi_ctx, grids):
    """interp_host, interp_grid_host and a three-member group on one device, once each per layout"""
    import armadillocudalinearinterpolation_amd as mi
    name = "guess_bsearch"
    t = ic.table(name)
    xq, yq = ic.scattered(name)
    ref = ic.with_extrap(_scattered_ref(name), xq, yq, t["xg"], t["yg"], -3.25)
    xi, yi = ic.grid_xi(t["xg"]), ic.grid_yi(t["yg"], 257, seed=257)
    px, py = ic.mesh_pairs(xi, yi)
    gref = ic.reference(name, px, py)
    grp = mi.Group([0, 0, 0])
    try:
        for compact in (False, True):
            grid = grids(name, compact)
            _check((name, compact, "interp_host"), grid.interp_host(xq, yq, extrap=-3.25), ref, xq, yq, t)
            zi = grid.interp_grid_host(xi, yi)
            assert zi.shape == (yi.size, xi.size)
            _check((name, compact, "interp_grid_host"), zi.ravel("F"), gref, px, py, t)
            gt = grp.grid2(t["xg"], t["yg"], t["Z"], compact=compact)
            try:
                _check((name, compact, "group interp_host"), gt.interp_host(xq, yq, extrap=-3.25), ref, xq, yq, t)
            finally:
                gt.close()
    finally:
        grp.close()


def test_explicit_axes_on_the_fma_nodes_equal_the_implicit_table(mi_ctx, grids):
    """the uniform table built from explicit axes fma(i, dx, x0): the same bits as the implicit form, scattered and
    gridded, both layouts"""
    import armadillocudalinearinterpolation_amd as mi
    t = ic.table("uniform")
    xq, yq = ic.scattered("uniform")
    xi, yi = ic.grid_xi(t["xg"]), ic.grid_yi(t["yg"], 257, seed=3)
    px, py = ic.mesh_pairs(xi, yi)
    gref = ic.reference("uniform", px, py)
    for compact in (False, True):
        explicit = mi.Grid2.from_axes(mi_ctx, t["xg"], t["yg"], t["Z"], compact=compact)
        try:
            implicit = grids("uniform", compact)
            assert explicit.info() == implicit.info() == {"table_bytes": 64 * 48 * (16 if compact else 32)}
            for g in (explicit, implicit):
                _check((compact, g is explicit, "scattered"), g.interp(_t(xq), _t(yq)).cpu().numpy(), _scattered_ref("uniform"), xq, yq, t)
                zi = g.interp_grid(_t(xi), _t(yi)).cpu().numpy()
                _check((compact, g is explicit, "gridded"), zi.ravel("F"), gref, px, py, t)
        finally:
            explicit.close()


def _capture(mi_ctx, call):
    """warm up outside the capture (a first gridded call grows its workspace), then capture `call` once on a side
    stream as a single linear stream"""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mi_ctx.use_torch_stream()
        call()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mi_ctx.use_torch_stream()
            call()
    torch.cuda.current_stream().wait_stream(side)
    mi_ctx.use_torch_stream()
    return graph


@pytest.mark.parametrize("compact", [False, True])
def test_hipgraph_replay_scattered(mi_ctx, grids, compact):
    """the scattered call captured once and replayed twice with fresh queries in the same buffers"""
    import torch
    name = "guess_bsearch"
    t = ic.table(name)
    xq, yq = ic.scattered(name)
    ref = _scattered_ref(name)
    grid = grids(name, compact)
    xd, yd = _t(xq), _t(yq)
    out = torch.zeros_like(xd)
    graph = _capture(mi_ctx, lambda: grid.interp(xd, yd, out=out))
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(xq.size)
        xd.copy_(_t(xq[perm]))
        yd.copy_(_t(yq[perm]))
        out.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        _check((name, compact, "replay", seed), out.cpu().numpy(), ref[perm], xq[perm], yq[perm], t)


@pytest.mark.parametrize("compact", [False, True])
def test_hipgraph_replay_gridded(mi_ctx, grids, compact):
    """the gridded call (locate + tile kernel, 8-B stores) captured once and replayed twice with fresh axes"""
    import torch
    name = "guess_bsearch"
    t = ic.table(name)
    xi, nyi = ic.grid_xi(t["xg"]), 257
    grid = grids(name, compact)
    xd, yd = _t(xi), _t(ic.grid_yi(t["yg"], nyi, seed=0))
    out = torch.zeros((xi.size, nyi), dtype=torch.float64, device="cuda")
    graph = _capture(mi_ctx, lambda: grid.interp_grid(xd, yd, out=out))
    for seed in (1, 2):
        xi2 = xi[np.random.default_rng(seed).permutation(xi.size)]
        yi2 = ic.grid_yi(t["yg"], nyi, seed=seed)
        xd.copy_(_t(xi2))
        yd.copy_(_t(yi2))
        out.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        px, py = ic.mesh_pairs(xi2, yi2)
        _check((name, compact, "replay", seed), out.cpu().numpy().reshape(-1), ic.reference(name, px, py), px, py, t)
