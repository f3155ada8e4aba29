"""arma::interp2's "nearest" method on the device: mi_interp2_nearest_f64_dev (Grid2.interp_nearest),
mi_interp2_grid_nearest_f64_dev / _host (Grid2.interp_grid_nearest, .interp_grid_nearest_host),
mi_interp2_slices_nearest_f64_dev (interp2_slices_nearest), mi_debug_nearest2_launches and the C++ method strings
(mi355::interp2(..., method)).

The reference of every value is tests/nearest2_cases.py -- nearest_cases.rule_index per axis and one copy Z[ky, kx] --
applied to EVERY output element and compared with nearest_cases._eq_bits: the same 64 bits, NaN in the same places, no
tolerance, no sampling.  tests/test_interp2_nearest_cpu.py holds that reference to Armadillo's two-pass scan.

Axes lie on a grid of 1/8, so that midpoint queries are exact ties; a test that claims to exercise the select asserts from
its own inputs, on EACH axis, that they hold at least 8 exact ties and pick both the left and the right node
(nearest_batched_cases.assert_select; only where an axis has at least 37 queries).  Tables are 9 x 11 nodes unless noted
and both resident layouts (quads, compact) run for every mi_grid2 test.  mi_debug_nearest2_launches proves which body
ran: 0 scattered; gridded 1 tile 16-B, 2 tile 8-B, 3 flat 16-B, 4 flat 8-B; slices 5 tile 16-B, 6 tile 8-B, 7 flat.

The tile bodies hold a table column across the output columns of a strip, and the host side cuts strips of ONE column
until there are more than 32 workgroups of work per CU (gridded) or 4 units per resident workgroup (slices): the
held-value tests therefore run 4 x that many columns, which makes them the largest device tests here (about 8.4 M
outputs each); the host form's chunk branch (16.81 M outputs, 134 MB through PCIe) is the one slow id."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nearest2_cases as n2
import nearest_batched_cases as bc
import nearest_cases as nc
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "armadillocudalinearinterpolation_amd", "host")
SCATTERED, G_TILE16, G_TILE8, G_FLAT16, G_FLAT8, S_TILE16, S_TILE8, S_FLAT = range(8)
NFORMS = 8
THIN = 256                # kThinRows: nyi below takes the flat body
GUARD = 16                # sentinel elements on both sides of a result
INVALID = 1
NY, NX = 9, 11


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _forms(ctx):
    return [int(ctx._L.mi_debug_nearest2_launches(f)) for f in range(NFORMS)]


def _moved(before, after, form, count=1):
    assert [a - b for a, b in zip(after, before)] == [count * int(f == form) for f in range(NFORMS)], (before, after, form)


def _axes(rng, kind_x="random", kind_y="random", nx=NX, ny=NY):
    return n2.axis(kind_x, rng, nx), n2.axis(kind_y, rng, ny)


def _grid2(ctx, X, Y, Z, compact, uniform=False):
    import armadillocudalinearinterpolation_amd as mi
    if uniform:
        return mi.Grid2.uniform(ctx, n2.UNIFORM_X0, n2.UNIFORM_DX, X.size, n2.UNIFORM_X0, n2.UNIFORM_DX, Y.size, Z, compact=compact)
    return mi.Grid2.from_axes(ctx, X, Y, Z, compact=compact)


def _select(X, Y, xi, yi):
    if xi.size >= 37:
        bc.assert_select(X, xi)
    if yi.size >= 37:
        bc.assert_select(Y, yi)


def _buffer(n, misalign):
    """a result of n elements inside a sentinel-filled buffer: (buffer, offset); misalign: 8-B but not 16-B aligned"""
    import torch
    buf = torch.full((n + 2 * GUARD + 2,), n2.SENTINEL, dtype=torch.float64, device="cuda")
    off = GUARD + (1 if misalign else 0)
    assert buf.data_ptr() % 16 == 0
    return buf, off


def _guards_intact(buf, off, n):
    h = buf.cpu().numpy()
    assert np.all(h[:off] == n2.SENTINEL) and np.all(h[off + n:] == n2.SENTINEL), "wrote outside the result"
    return h[off:off + n].copy()


def _scattered(ctx, g, xq, yq, extrap, misalign=False):
    """one scattered call; misalign: xq, yq and zq offset by one element.  Returns (nq,)."""
    import torch
    nq = xq.size
    o = 1 if misalign else 0
    xb, yb = (torch.zeros(nq + 2, dtype=torch.float64, device="cuda") for _ in range(2))
    xd, yd = xb[o:o + nq], yb[o:o + nq]
    xd.copy_(_t(xq))
    yd.copy_(_t(yq))
    buf, off = _buffer(nq, misalign)
    out = buf[off:off + nq]
    assert nq == 0 or all((t.data_ptr() % 16 != 0) == misalign for t in (xd, yd, out))
    before = _forms(ctx)
    got = g.interp_nearest(xd, yd, out=out, extrap=extrap)
    _moved(before, _forms(ctx), SCATTERED, 1 if nq else 0)
    assert got.data_ptr() == out.data_ptr()
    return _guards_intact(buf, off, nq)


def _grid_form(nyi, misalign):
    if nyi < THIN:
        return G_FLAT8 if misalign else G_FLAT16
    return G_TILE16 if (not misalign and nyi % 2 == 0) else G_TILE8


def _gridded(ctx, g, xi, yi, extrap, misalign=False):
    """one gridded call into a sentinel-guarded buffer; asserts the body that ran.  Returns (nyi, nxi)."""
    nxi, nyi = xi.size, yi.size
    buf, off = _buffer(nxi * nyi, misalign)
    out = buf[off:off + nxi * nyi].view(nxi, nyi)
    before = _forms(ctx)
    got = g.interp_grid_nearest(_t(xi), _t(yi), out=out, extrap=extrap)
    _moved(before, _forms(ctx), _grid_form(nyi, misalign))
    assert tuple(got.shape) == (nyi, nxi)
    return _guards_intact(buf, off, nxi * nyi).reshape(nxi, nyi).T


def _cube_dev(Zc, ldz_pad=0, zgap=0):
    """(ny, nx, S) -> a CUDA view with that layout over a buffer whose padding rows and slice gaps hold POISON"""
    import torch
    ny, nx, S = Zc.shape
    ldz = ny + ldz_pad
    zstride = ldz * nx + zgap
    zbuf = torch.full((S * zstride,), n2.POISON, dtype=torch.float64, device="cuda")
    Zd = torch.as_strided(zbuf, (ny, nx, S), (1, ldz, zstride))
    Zd.copy_(_t(Zc))
    return Zd, ldz, zstride


def _slices(ctx, ax, ay, Zc, xi, yi, extrap, ldz_pad=0, zgap=0, ldzi_pad=0, zigap=0, misalign=False, garbage_strides=False):
    """one slices call: POISON in the padding rows and gaps of z, a sentinel in those of zi and around it; asserts the body
    that ran, that nothing but the outputs was written and that no POISON came out.  garbage_strides (one slice): the raw
    C call with slice strides that mean nothing.  Returns (nyi, nxi, S)."""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    ny, nx, S = Zc.shape
    nxi, nyi = xi.size, yi.size
    Zd, ldz, zstride = _cube_dev(Zc, ldz_pad, zgap)
    ldzi = nyi + ldzi_pad
    zistride = ldzi * nxi + zigap
    obuf, off = _buffer(S * zistride, misalign)
    out = torch.as_strided(obuf, (nyi, nxi, S), (1, ldzi, zistride), off)
    vec = not misalign and ldzi % 2 == 0 and (S == 1 or zistride % 2 == 0)
    form = S_FLAT if nyi < THIN else (S_TILE16 if vec else S_TILE8)
    before = _forms(ctx)
    if garbage_strides:
        assert S == 1
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        xd, yd = _t(xi), _t(yi)
        st = ctx._L.mi_interp2_slices_nearest_f64_dev(ctx._h, ax._h, ay._h, p(Zd), ldz, 3, 1, p(xd), nxi, p(yd), nyi, p(out), ldzi, 1,
                                                      float(extrap))
        assert st == 0, ctx._L.mi_last_error(ctx._h)
    else:
        ret = mi.interp2_slices_nearest(ctx, ax, ay, Zd, _t(xi), _t(yi), out=out, extrap=extrap)
        assert ret.data_ptr() == out.data_ptr()
    _moved(before, _forms(ctx), form)
    written = torch.zeros_like(obuf, dtype=torch.bool)
    torch.as_strided(written, (nyi, nxi, S), (1, ldzi, zistride), off).fill_(True)
    untouched = obuf[~written].cpu().numpy()
    assert untouched.size == obuf.numel() - nyi * nxi * S and np.all(untouched == n2.SENTINEL), "padding, gap or guard written"
    got = out.cpu().numpy()
    assert not np.any(got == n2.POISON), "a padding row or a slice gap of z was read"
    return got


def _axis1(ctx, X, uniform=False):
    import armadillocudalinearinterpolation_amd as mi
    return mi.Axis1.uniform(ctx, n2.UNIFORM_X0, n2.UNIFORM_DX, X.size) if uniform else mi.Axis1.from_nodes(ctx, X)


# ---- scattered --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("compact", [False, True], ids=["quads", "compact"])
@pytest.mark.parametrize("nq", [1, 255, 256, 257, 1000])
def test_scattered_sizes_and_alignment(mi_ctx, nq, compact):
    """sizes around one workgroup of 256 lanes; 16-B aligned streams (two queries per lane) and streams offset by one
    element (8-B aligned only: one query per lane); pair 0 is (NaN, NaN), pairs 1 and 2 NaN with out-of-range"""
    rng = np.random.default_rng(3000 + nq)
    X, Y = _axes(rng)
    Z = n2.table(NY, NX)
    g = _grid2(mi_ctx, X, Y, Z, compact)
    xq, yq = n2.pair_queries(rng, X, Y, nq)
    _select(X, Y, xq, yq)
    for extrap in (-7.5, np.nan):
        want = n2.ref_pairs(X, Y, Z, xq, yq, extrap)
        for misalign in (False, True):
            assert nc._eq_bits(_scattered(mi_ctx, g, xq, yq, extrap, misalign), want), (nq, extrap, misalign)
    if nq >= 4:
        assert np.isnan(want[:3]).all()
    g.close()


@pytest.mark.parametrize("compact", [False, True], ids=["quads", "compact"])
@pytest.mark.parametrize("kinds", [("near", "clustered"), ("clustered", "near"), ("uniform", "uniform"), ("uniform", "clustered")],
                         ids="-".join)
def test_axis_kinds_scattered_and_gridded(mi_ctx, kinds, compact):
    """guess-and-walk, binary search and implicit uniform axes on x and on y (uniform-uniform as an implicit table; a
    uniform axis beside an explicit one as explicit nodes), through the scattered kernel, the flat and the tile body"""
    rng = np.random.default_rng([31, n2.KINDS.index(kinds[0]), n2.KINDS.index(kinds[1])])
    X, Y = _axes(rng, *kinds)
    assert n2.uses_guess(X) == (kinds[0] != "clustered") and n2.uses_guess(Y) == (kinds[1] != "clustered")
    Z = n2.table(NY, NX)
    g = _grid2(mi_ctx, X, Y, Z, compact, uniform=kinds == ("uniform", "uniform"))
    xq, yq = n2.pair_queries(rng, X, Y, 257)
    _select(X, Y, xq, yq)
    assert nc._eq_bits(_scattered(mi_ctx, g, xq, yq, -7.5), n2.ref_pairs(X, Y, Z, xq, yq, -7.5))
    for nyi in (70, 257):
        xi, yi = bc.queries(rng, X, 70), bc.queries(rng, Y, nyi)
        _select(X, Y, xi, yi)
        assert nc._eq_bits(_gridded(mi_ctx, g, xi, yi, -7.5), n2.ref_grid(X, Y, Z, xi, yi, -7.5)), nyi
    g.close()


# ---- gridded ----------------------------------------------------------------------------------------------------------

FLAT_SHAPES = [(nyi, nxi) for nyi in (1, 2, 3, 255) for nxi in (1, 37, 70)] + [(1, 513), (3, 171), (2, 256), (2, 512), (255, 257)]
TILE_SHAPES = [(nyi, nxi) for nyi in (256, 257, 512, 513, 700) for nxi in (1, 37, 70)]


@pytest.mark.parametrize("compact", [False, True], ids=["quads", "compact"])
@pytest.mark.parametrize("shape", FLAT_SHAPES + TILE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_gridded_shapes_and_alignment(mi_ctx, shape, compact):
    """flat body (nyi < 256): totals that are odd, a multiple of 512 (2 x 256, 2 x 512) and 512 k + 1 (1 x 513, 3 x 171,
    255 x 257); tile body: one and two row blocks, a one-row remainder (513), odd nyi (the 8-B body); zi 16-B aligned and
    offset by 8 B -- the hook moves by one in exactly the expected body"""
    nyi, nxi = shape
    rng = np.random.default_rng([41, nyi, nxi])
    X, Y = _axes(rng)
    Z = n2.table(NY, NX)
    g = _grid2(mi_ctx, X, Y, Z, compact)
    xi, yi = bc.queries(rng, X, nxi), bc.queries(rng, Y, nyi)
    _select(X, Y, xi, yi)
    want = n2.ref_grid(X, Y, Z, xi, yi, -7.5)
    for misalign in (False, True):
        assert nc._eq_bits(_gridded(mi_ctx, g, xi, yi, -7.5, misalign), want), (shape, misalign)
    g.close()


def _strip_columns(ctx, per_cu):
    """output columns that make the host side cut strips of 5 columns for one row block (and one slice): 4 x the number
    of strips it wants, and 5 more"""
    cus = ctx.device_info()["compute_units"]
    return cus * per_cu * 4 + 5


def _sequence_axis(X, nxi):
    """all held-value sequences one after another, repeated to nxi columns: strips of 5 columns start at every position
    of every sequence"""
    seq = np.concatenate([np.asarray(v, dtype=np.float64) for v in n2.x_sequences(X).values()])
    assert seq.size % 5 != 0
    return np.resize(seq, nxi)


@pytest.mark.parametrize("compact", [False, True], ids=["quads", "compact"])
@pytest.mark.parametrize("misalign", [False, True], ids=["16B", "8B"])
def test_gridded_tile_body_holds_values_across_a_strip(mi_ctx, misalign, compact):
    """enough output columns that a strip is 5 columns long, filled with the held-value sequences: runs of equal kx,
    flagged columns inside a run (the held values must survive them), a run that starts flagged, every node in order,
    strictly descending xi, kx returning to an earlier column, all flagged -- every element against the reference"""
    rng = np.random.default_rng(51)
    X, Y = _axes(rng)
    Z = n2.table(NY, NX)
    g = _grid2(mi_ctx, X, Y, Z, compact)
    nxi = _strip_columns(mi_ctx, 32)
    xi, yi = _sequence_axis(X, nxi), bc.queries(rng, Y, 256)
    bc.assert_select(Y, yi)
    got = _gridded(mi_ctx, g, xi, yi, -7.5, misalign)
    assert nc._eq_bits(got, n2.ref_grid(X, Y, Z, xi, yi, -7.5))
    g.close()


@pytest.mark.parametrize("compact", [False, True], ids=["quads", "compact"])
@pytest.mark.parametrize("nyi", [37, 257])
def test_gridded_equals_scattered_slices_and_the_two_1d_passes(mi_ctx, nyi, compact):
    """the gridded result equals the scattered call on the full pair mesh, the slices call slice by slice, and --
    separability -- Axis1.interp_cols_nearest along y followed by Axis1.interp_rows_nearest along x on the same data
    (everywhere but where a NaN row meets an out-of-range column: the second 1-D pass cannot know the first one's NaN
    was a flag, and writes extrap there)"""
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(60 + nyi)
    X, Y = _axes(rng)
    Zc = n2.cube(NY, NX, 3)
    xi, yi = bc.queries(rng, X, 70), bc.queries(rng, Y, nyi)
    _select(X, Y, xi, yi)
    ax, ay = _axis1(mi_ctx, X), _axis1(mi_ctx, Y)
    sl = _slices(mi_ctx, ax, ay, Zc, xi, yi, -7.5)
    xx, yy = np.meshgrid(xi, yi)
    for s in range(3):
        g = _grid2(mi_ctx, X, Y, Zc[:, :, s], compact)
        got = _gridded(mi_ctx, g, xi, yi, -7.5)
        assert nc._eq_bits(got, n2.ref_grid(X, Y, Zc[:, :, s], xi, yi, -7.5))
        assert nc._eq_bits(_scattered(mi_ctx, g, xx.ravel(), yy.ravel(), -7.5).reshape(nyi, 70), got)
        assert nc._eq_bits(sl[:, :, s], got)
        g.close()
        along_y = ay.interp_cols_nearest(_t(Zc[:, :, s].T).T, _t(yi), extrap=-7.5)            # (nyi, nx), column-major
        both = ax.interp_rows_nearest(along_y, _t(xi), extrap=-7.5).cpu().numpy()             # (nyi, nxi)
        clash = (nc.rule_index(Y, yi) == -2)[:, None] & (nc.rule_index(X, xi) == -1)[None, :]
        assert clash.any() and nc._eq_bits(np.where(clash, 0.0, both), np.where(clash, 0.0, got))
    ax.close()
    ay.close()


@pytest.mark.parametrize("compact", [False, True], ids=["quads", "compact"])
def test_special_values_come_back_at_their_node_and_nowhere_else(mi_ctx, compact):
    """inf, -inf, NaN, -0.0 and the denormal: each with its bits at exactly the outputs whose (ky, kx) is its node.  (The
    bilinear call on the same inputs spreads them: the NaN at node (3, 4) makes every output of its four neighbouring
    cells NaN, and inf - inf across rows 1 and 2 of column 2 makes more; here 1 node is 1 node.)"""
    rng = np.random.default_rng(71)
    X, Y = _axes(rng)
    Z = n2.table(NY, NX)
    g = _grid2(mi_ctx, X, Y, Z, compact)
    for nyi in (70, 300):
        xi, yi = np.concatenate([bc.queries(rng, X, 70 - NX), X]), np.concatenate([bc.queries(rng, Y, nyi - NY), Y])   # every node is hit
        _select(X, Y, xi, yi)
        got = _gridded(mi_ctx, g, xi, yi, -7.5)
        kx, ky = nc.rule_index(X, xi), nc.rule_index(Y, yi)
        inside = (ky[:, None] >= 0) & (kx[None, :] >= 0)
        bits = got.view(np.uint64)
        for (i, j), v in n2.SPECIAL_NODES.items():
            here = (ky[:, None] == i) & (kx[None, :] == j)
            assert here.any(), (i, j)
            same = np.isnan(got) if v != v else bits == np.float64(v).view(np.uint64)
            if v == 0:                                             # two nodes hold -0.0
                here = np.zeros_like(here)
                for (a, b), w in n2.SPECIAL_NODES.items():
                    if w == 0:
                        here |= (ky[:, None] == a) & (kx[None, :] == b)
            assert np.array_equal(same & inside, here), (i, j, v)
    g.close()


@pytest.mark.parametrize("extrap", [np.nan, -7.5, np.inf], ids=["nan", "-7.5", "inf"])
def test_extrapolation_value_and_nan_wins_over_out_of_range(mi_ctx, extrap):
    rng = np.random.default_rng(81)
    X, Y = _axes(rng)
    Z = n2.table(NY, NX, specials=False)
    xi, yi = bc.queries(rng, X, 70), bc.queries(rng, Y, 257)
    kx, ky = nc.rule_index(X, xi), nc.rule_index(Y, yi)
    assert ((ky[:, None] == -2) & (kx[None, :] == -1)).any() and ((ky[:, None] == -1) & (kx[None, :] == -2)).any()
    want = n2.ref_grid(X, Y, Z, xi, yi, extrap)
    nan_flag = (ky[:, None] == -2) | (kx[None, :] == -2)
    assert np.isnan(want[nan_flag]).all()
    ax, ay = _axis1(mi_ctx, X), _axis1(mi_ctx, Y)
    for compact in (False, True):
        g = _grid2(mi_ctx, X, Y, Z, compact)
        assert nc._eq_bits(_gridded(mi_ctx, g, xi, yi, extrap), want)
        assert nc._eq_bits(_gridded(mi_ctx, g, xi, yi[:70], extrap, True), want[:70])
        xx, yy = np.meshgrid(xi, yi[:40])
        assert nc._eq_bits(_scattered(mi_ctx, g, xx.ravel(), yy.ravel(), extrap), want[:40].ravel())
        g.close()
    assert nc._eq_bits(_slices(mi_ctx, ax, ay, Z[:, :, None], xi, yi, extrap)[:, :, 0], want)
    assert nc._eq_bits(_slices(mi_ctx, ax, ay, Z[:, :, None], xi, yi[:70], extrap)[:, :, 0], want[:70])
    ax.close()
    ay.close()


# ---- slices -----------------------------------------------------------------------------------------------------------

SLICE_LAYOUTS = {                       # ldz_pad, zgap, ldzi_pad (made even / odd below), zigap parity, misalign
    "dense": (0, 0, 0, None, False),
    "padded_16B": (3, 7, "even", 0, False),
    "odd_ldzi": (1, 2, "odd", 0, False),
    "odd_slice_stride": (2, 5, "even", 1, False),
    "zi_offset_8B": (3, 7, "even", 0, True),
}


@pytest.mark.parametrize("layout", sorted(SLICE_LAYOUTS))
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("nyi", [3, 255, 256, 513])
def test_slices_layouts_and_bodies(mi_ctx, nyi, S, layout):
    """flat and tile bodies; ldz > ny, ldzi > nyi and slice strides with gaps: POISON in z's padding never comes out, the
    sentinel in every padding row and gap of zi survives; 16-B stores when zi, ldzi and the slice stride allow, 8-B stores
    for an odd ldzi, an odd slice stride (3 slices) or a zi offset by 8 B; one slice: garbage slice strides are ignored"""
    ldz_pad, zgap, pad, gap_parity, misalign = SLICE_LAYOUTS[layout]
    rng = np.random.default_rng([91, nyi, S])
    X, Y = _axes(rng)
    Zc = n2.cube(NY, NX, S)
    nxi = 37
    xi, yi = bc.queries(rng, X, nxi), bc.queries(rng, Y, nyi)
    _select(X, Y, xi, yi)
    ldzi_pad = zigap = 0
    if gap_parity is not None:                               # one or two padding rows, a gap of two or three elements
        ld_parity = 0 if pad == "even" else 1
        ldzi_pad = 1 + int((nyi + 1) % 2 != ld_parity)
        zigap = 2 + int(((nyi + ldzi_pad) * nxi + 2) % 2 != gap_parity)
        assert ((nyi + ldzi_pad) * nxi + zigap) % 2 == gap_parity and (nyi + ldzi_pad) % 2 == ld_parity
    ax, ay = _axis1(mi_ctx, X), _axis1(mi_ctx, Y)
    got = _slices(mi_ctx, ax, ay, Zc, xi, yi, -7.5, ldz_pad, zgap, ldzi_pad, zigap, misalign, garbage_strides=(S == 1))
    assert nc._eq_bits(got, n2.ref_slices(X, Y, Zc, xi, yi, -7.5))
    if S > 1:                                                # the special values of slice 0 reach no other slice
        kx, ky = nc.rule_index(X, xi), nc.rule_index(Y, yi)
        inside = (ky[:, None] >= 0) & (kx[None, :] >= 0)
        assert np.isfinite(got[:, :, 1:][inside]).all() and not np.isfinite(got[:, :, 0][inside]).all()
        assert np.all(got[:, :, 1][inside] - got[:, :, 2][inside] == -1e6)      # and every slice holds its own values
    ax.close()
    ay.close()


@pytest.mark.parametrize("misalign", [False, True], ids=["16B", "8B"])
def test_slices_tile_body_holds_values_across_a_strip(mi_ctx, misalign):
    """as the gridded held-value test: two slices, strips of 5 columns filled with the held-value sequences"""
    rng = np.random.default_rng(95)
    X, Y = _axes(rng)
    Zc = n2.cube(NY, NX, 2)
    nxi = _strip_columns(mi_ctx, 16)                          # 8 resident workgroups per CU x 4 units, over 2 slices
    xi, yi = _sequence_axis(X, nxi), bc.queries(rng, Y, 256)
    bc.assert_select(Y, yi)
    ax, ay = _axis1(mi_ctx, X), _axis1(mi_ctx, Y)
    got = _slices(mi_ctx, ax, ay, Zc, xi, yi, -7.5, ldz_pad=1, misalign=misalign)
    assert nc._eq_bits(got, n2.ref_slices(X, Y, Zc, xi, yi, -7.5))
    ax.close()
    ay.close()


def test_slices_one_axis_object_for_both_axes_and_uniform_axes(mi_ctx):
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(97)
    X = n2.axis("random", rng, 11)
    Zc = n2.cube(11, 11, 2)
    ax = _axis1(mi_ctx, X)
    for nyi in (40, 280):
        xi, yi = bc.queries(rng, X, 45), bc.queries(rng, X, nyi)
        _select(X, X, xi, yi)
        assert nc._eq_bits(_slices(mi_ctx, ax, ax, Zc, xi, yi, np.nan), n2.ref_slices(X, X, Zc, xi, yi))
    ax.close()
    U, K = n2.axis("uniform", rng, 11), n2.axis("clustered", rng, 11)
    au, ak = _axis1(mi_ctx, U, uniform=True), _axis1(mi_ctx, K)
    xi, yi = bc.queries(rng, U, 45), bc.queries(rng, K, 280)
    _select(U, K, xi, yi)
    assert nc._eq_bits(_slices(mi_ctx, au, ak, Zc, xi, yi, 2.0), n2.ref_slices(U, K, Zc, xi, yi, 2.0))
    # the default output: the .permute(2, 1, 0) view of a new contiguous (S, nxi, nyi) buffer
    out = mi.interp2_slices_nearest(mi_ctx, au, ak, _cube_dev(Zc)[0], _t(xi), _t(yi), extrap=2.0)
    assert tuple(out.shape) == (280, 45, 2) and out.permute(2, 1, 0).is_contiguous()
    assert nc._eq_bits(out.cpu().numpy(), n2.ref_slices(U, K, Zc, xi, yi, 2.0))
    au.close()
    ak.close()


# ---- the record workspace, empty calls, refused calls -----------------------------------------------------------------

def test_linear_and_nearest_calls_back_to_back_share_the_record_workspace(mi_ctx):
    """linear grid call, nearest grid call, linear slices call, nearest slices call on one stream with no synchronisation
    in between, each with another nxi + nyi (the workspace grows and shrinks, 16-B and 4-B records in turn): all four
    results are bit-equal to their references"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    rng = np.random.default_rng(101)
    X, Y = _axes(rng)
    Zc = np.stack([n2.table(NY, NX, s, specials=False) for s in range(2)], axis=2)
    g = _grid2(mi_ctx, X, Y, Zc[:, :, 0], False)
    ax, ay = _axis1(mi_ctx, X), _axis1(mi_ctx, Y)
    Zd = _cube_dev(Zc)[0]
    rounds = []
    for sizes in (((40, 300), (900, 20), (37, 257), (300, 40)), ((7, 7), (64, 257), (1000, 3), (70, 513))):
        q = [(bc.queries(rng, X, a), bc.queries(rng, Y, b)) for a, b in sizes]
        d = [(_t(x), _t(y)) for x, y in q]
        torch.cuda.synchronize()
        before = _forms(mi_ctx)
        r = (g.interp_grid(*d[0], extrap=1.5), g.interp_grid_nearest(*d[1], extrap=1.5),
             mi.interp2_slices(mi_ctx, ax, ay, Zd, *d[2], extrap=1.5), mi.interp2_slices_nearest(mi_ctx, ax, ay, Zd, *d[3], extrap=1.5))
        assert sum(_forms(mi_ctx)) - sum(before) == 2
        rounds.append((q, r))
    torch.cuda.synchronize()

    def lin(Z2, xi, yi):
        XX, YY = np.meshgrid(xi, yi)
        return oracle.interp2_bilinear(X, Y, Z2, XX.ravel("F"), YY.ravel("F"), 1.5, nthreads=8).reshape(yi.size, xi.size, order="F")
    for q, r in rounds:
        assert np.array_equal(r[0].cpu().numpy(), lin(Zc[:, :, 0], *q[0]), equal_nan=True)
        assert nc._eq_bits(r[1].cpu().numpy(), n2.ref_grid(X, Y, Zc[:, :, 0], *q[1], 1.5))
        assert np.array_equal(r[2].cpu().numpy(), np.stack([lin(Zc[:, :, s], *q[2]) for s in range(2)], axis=2), equal_nan=True)
        assert nc._eq_bits(r[3].cpu().numpy(), n2.ref_slices(X, Y, Zc, *q[3], 1.5))
    g.close()
    ax.close()
    ay.close()


def test_empty_calls_launch_nothing_and_touch_nothing(mi_ctx):
    import torch
    import armadillocudalinearinterpolation_amd as mi
    L, h = mi_ctx._L, mi_ctx._h
    rng = np.random.default_rng(103)
    X, Y = _axes(rng)
    Zc = n2.cube(NY, NX, 2)
    g = _grid2(mi_ctx, X, Y, Zc[:, :, 0], False)
    ax, ay = _axis1(mi_ctx, X), _axis1(mi_ctx, Y)
    Zd, xd, yd = _cube_dev(Zc)[0], _t(bc.queries(rng, X, 9)), _t(bc.queries(rng, Y, 9))
    zi = torch.full((9 * 9 * 2,), n2.SENTINEL, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    before = _forms(mi_ctx)
    assert L.mi_interp2_nearest_f64_dev(h, g._h, p(xd), p(yd), p(zi), 0, 0.0) == 0
    assert L.mi_interp2_nearest_f64_dev(h, g._h, None, None, None, 0, 0.0) == 0
    for f in (L.mi_interp2_grid_nearest_f64_dev, L.mi_interp2_grid_nearest_f64_host):
        assert f(h, g._h, p(xd), 0, p(yd), 9, p(zi), 0.0) == 0
        assert f(h, g._h, p(xd), 9, p(yd), 0, p(zi), 0.0) == 0
        assert f(h, g._h, None, 0, None, 0, None, 0.0) == 0
    sl = L.mi_interp2_slices_nearest_f64_dev
    assert sl(h, ax._h, ay._h, p(Zd), NY, NY * NX, 0, p(xd), 9, p(yd), 9, p(zi), 9, 81, 0.0) == 0
    assert sl(h, ax._h, ay._h, p(Zd), NY, NY * NX, 2, p(xd), 0, p(yd), 9, p(zi), 9, 81, 0.0) == 0
    assert sl(h, ax._h, ay._h, p(Zd), NY, NY * NX, 2, p(xd), 9, p(yd), 0, p(zi), 9, 81, 0.0) == 0
    assert sl(h, ax._h, ay._h, None, 0, 0, 0, None, 0, None, 0, None, 0, 0, 0.0) == 0
    torch.cuda.synchronize()
    assert _forms(mi_ctx) == before and bool((zi == n2.SENTINEL).all())
    empty = torch.empty(0, dtype=torch.float64, device="cuda")
    assert tuple(g.interp_nearest(empty, empty).shape) == (0,)
    assert tuple(g.interp_grid_nearest(empty, yd).shape) == (9, 0) and tuple(g.interp_grid_nearest(xd, empty).shape) == (0, 9)
    assert tuple(g.interp_grid_nearest_host(np.empty(0), np.ones(3)).shape) == (3, 0)
    assert tuple(mi.interp2_slices_nearest(mi_ctx, ax, ay, Zd, empty, yd).shape) == (9, 0, 2)
    assert tuple(mi.interp2_slices_nearest(mi_ctx, ax, ay, Zd[:, :, :0], xd, yd).shape) == (9, 9, 0)
    assert _forms(mi_ctx) == before
    g.close()
    ax.close()
    ay.close()


def test_refused_calls_name_themselves_and_launch_nothing(mi_ctx):
    import torch
    L, h = mi_ctx._L, mi_ctx._h
    rng = np.random.default_rng(107)
    X, Y = _axes(rng)
    Zc = n2.cube(NY, NX, 2)
    g = _grid2(mi_ctx, X, Y, Zc[:, :, 0], False)
    ax, ay = _axis1(mi_ctx, X), _axis1(mi_ctx, Y)
    G, a, b = g._h, ax._h, ay._h
    z, x, y = _cube_dev(Zc)[0], _t(bc.queries(rng, X, 9)), _t(bc.queries(rng, Y, 8))
    zi = torch.full((8 * 9 * 2 + 2,), n2.SENTINEL, dtype=torch.float64, device="cuda")
    host = np.full(72, n2.SENTINEL)
    hp = C.c_void_p(host.ctypes.data)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    sc, gd, gh, sl = (L.mi_interp2_nearest_f64_dev, L.mi_interp2_grid_nearest_f64_dev, L.mi_interp2_grid_nearest_f64_host,
                      L.mi_interp2_slices_nearest_f64_dev)
    big = 2 ** 62
    zs = NY * NX
    cases = [
        ("mi_interp2_nearest_f64_dev", lambda: sc(h, None, p(x), p(x), p(zi), 8, 0.0)),
        ("mi_interp2_nearest_f64_dev", lambda: sc(h, G, None, p(x), p(zi), 8, 0.0)),
        ("mi_interp2_nearest_f64_dev", lambda: sc(h, G, p(x), None, p(zi), 8, 0.0)),
        ("mi_interp2_nearest_f64_dev", lambda: sc(h, G, p(x), p(x), None, 8, 0.0)),
        ("mi_interp2_nearest_f64_dev", lambda: sc(h, G, p(x, 4), p(x), p(zi), 8, 0.0)),
        ("mi_interp2_nearest_f64_dev", lambda: sc(h, G, p(x), p(x, 4), p(zi), 8, 0.0)),
        ("mi_interp2_nearest_f64_dev", lambda: sc(h, G, p(x), p(x), p(zi, 4), 8, 0.0)),
        ("mi_interp2_grid_nearest_f64_dev", lambda: gd(h, None, p(x), 9, p(y), 8, p(zi), 0.0)),
        ("mi_interp2_grid_nearest_f64_dev", lambda: gd(h, G, None, 9, p(y), 8, p(zi), 0.0)),
        ("mi_interp2_grid_nearest_f64_dev", lambda: gd(h, G, p(x), 9, None, 8, p(zi), 0.0)),
        ("mi_interp2_grid_nearest_f64_dev", lambda: gd(h, G, p(x), 9, p(y), 8, None, 0.0)),
        ("mi_interp2_grid_nearest_f64_dev", lambda: gd(h, G, p(x, 4), 9, p(y), 8, p(zi), 0.0)),
        ("mi_interp2_grid_nearest_f64_dev", lambda: gd(h, G, p(x), 9, p(y, 4), 8, p(zi), 0.0)),
        ("mi_interp2_grid_nearest_f64_dev", lambda: gd(h, G, p(x), 9, p(y), 8, p(zi, 4), 0.0)),
        ("mi_interp2_grid_nearest_f64_dev", lambda: gd(h, G, p(x), big, p(y), big, p(zi), 0.0)),
        ("mi_interp2_grid_nearest_f64_host", lambda: gh(h, None, hp, 9, hp, 8, hp, 0.0)),
        ("mi_interp2_grid_nearest_f64_host", lambda: gh(h, G, None, 9, hp, 8, hp, 0.0)),
        ("mi_interp2_grid_nearest_f64_host", lambda: gh(h, G, hp, 9, None, 8, hp, 0.0)),
        ("mi_interp2_grid_nearest_f64_host", lambda: gh(h, G, hp, 9, hp, 8, None, 0.0)),
        ("mi_interp2_grid_nearest_f64_host", lambda: gh(h, G, hp, big, hp, big, hp, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, None, b, p(z), NY, zs, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, None, p(z), NY, zs, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, None, NY, zs, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, None, 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, p(x), 9, None, 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, p(x), 9, p(y), 8, None, 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z, 4), NY, zs, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, p(x, 4), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, p(x), 9, p(y, 4), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, p(x), 9, p(y), 8, p(zi, 4), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY - 1, zs, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),   # ldz < ny
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, p(x), 9, p(y), 8, p(zi), 7, 72, 0.0)),       # ldzi < nyi
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs - 1, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),   # z stride
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, p(x), 9, p(y), 8, p(zi), 8, 71, 0.0)),       # zi stride
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, 2, p(x), big, p(y), big, p(zi), big, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), big, zs, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, zs, big, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0)),
        ("mi_interp2_slices_nearest_f64_dev", lambda: sl(h, a, b, p(z), NY, big, 2, p(x), 9, p(y), 8, p(zi), 8, big, 0.0)),
    ]
    before = _forms(mi_ctx)
    for k, (name, call) in enumerate(cases):
        assert call() == INVALID, (k, name)
        assert L.mi_last_error(h).decode().startswith(name + ":"), (k, name, L.mi_last_error(h))
    torch.cuda.synchronize()
    assert _forms(mi_ctx) == before
    assert bool((zi == n2.SENTINEL).all()) and np.all(host == n2.SENTINEL)          # nothing was written by a refused call
    if torch.cuda.device_count() > 1:                       # an axis of another context's device, where there is one
        import armadillocudalinearinterpolation_amd as mi
        other = mi.Context(1)
        far = mi.Axis1.from_nodes(other, X)
        assert sl(h, far._h, b, p(z), NY, zs, 2, p(x), 9, p(y), 8, p(zi), 8, 72, 0.0) == INVALID
        assert L.mi_last_error(h).decode().startswith("mi_interp2_slices_nearest_f64_dev:")
        far.close()
        other.close()
        torch.cuda.set_device(0)
    g.close()
    ax.close()
    ay.close()


# ---- host form --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("compact", [False, True], ids=["quads", "compact"])
def test_host_form_small_branch(mi_ctx, compact):
    rng = np.random.default_rng(111)
    X, Y = _axes(rng)
    Z = n2.table(NY, NX)
    g = _grid2(mi_ctx, X, Y, Z, compact)
    xi, yi = bc.queries(rng, X, 257), bc.queries(rng, Y, 70)
    _select(X, Y, xi, yi)
    before = _forms(mi_ctx)
    got = g.interp_grid_nearest_host(xi, yi, extrap=-7.5)
    _moved(before, _forms(mi_ctx), G_FLAT16)
    assert got.shape == (70, 257) and got.flags["F_CONTIGUOUS"]
    assert nc._eq_bits(got, n2.ref_grid(X, Y, Z, xi, yi, -7.5))
    g.close()


def test_host_form_chunk_branch(mi_ctx):
    """nxi = nyi = 4100: 16.81 M outputs, just above the 2 x 8 Mi threshold, so three chunks of 2046, 2046 and 8 columns
    (three tile-body launches), every element checked.  134 MB through PCIe once: the one slow id of this file."""
    rng = np.random.default_rng(113)
    X, Y = _axes(rng)
    Z = n2.table(NY, NX)
    g = _grid2(mi_ctx, X, Y, Z, False)
    n = 4100
    assert n * n > 2 * (8 << 20) and (8 << 20) // n == 2046 and n - 2 * 2046 == 8
    xi, yi = bc.queries(rng, X, n), bc.queries(rng, Y, n)
    _select(X, Y, xi, yi)
    before = _forms(mi_ctx)
    got = g.interp_grid_nearest_host(xi, yi, extrap=-7.5)
    _moved(before, _forms(mi_ctx), G_TILE16, 3)
    assert nc._eq_bits(got, n2.ref_grid(X, Y, Z, xi, yi, -7.5))
    g.close()


# ---- C++ ----------------------------------------------------------------------------------------------------------------

def test_cpp_method_strings(tmp_path):
    """mi355::interp2(X, Y, Z, XI, YI, ZI, method, extrap): "nearest" equals ref_grid; "linear" equals the existing
    overload's bits (with no, a double and an integer seventh argument); a bad, a starred and a null method throw"""
    from armadillocudalinearinterpolation_amd import _build as b
    b.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST, "arma_interp2_nearest_test"])
    out = subprocess.run([os.path.join(HOST, "arma_interp2_nearest_test"), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    for flag in ("threw_unknown", "threw_starred", "threw_null"):
        assert [flag, "1"] in lines, flag
    rd = lambda f: np.fromfile(os.path.join(tmp_path, "n2_%s.bin" % f), dtype=np.float64)  # noqa: E731
    X, Y, XI, YI = rd("X"), rd("Y"), rd("XI"), rd("YI")
    assert ["shape", str(YI.size), str(XI.size)] in lines
    Z = rd("Z").reshape(Y.size, X.size, order="F")
    mat = lambda f: rd(f).reshape(YI.size, XI.size, order="F")  # noqa: E731
    bc.assert_select(X, XI)
    bc.assert_select(Y, YI)
    near = n2.ref_grid(X, Y, Z, XI, YI)
    assert np.isinf(near).any() and (near == n2.DENORMAL).any() and (np.signbit(near) & (near == 0)).any()
    assert nc._eq_bits(mat("N"), near)
    assert nc._eq_bits(mat("NE"), n2.ref_grid(X, Y, Z, XI, YI, -7.5))
    XX, YY = np.meshgrid(XI, YI)
    lin = lambda e: oracle.interp2_bilinear(X, Y, Z, XX.ravel("F"), YY.ravel("F"), e, nthreads=8).reshape(YI.size, XI.size, order="F")  # noqa: E731
    assert np.array_equal(mat("L"), mat("D"), equal_nan=True) and np.array_equal(mat("D"), lin(2.5), equal_nan=True)
    assert np.array_equal(mat("LD"), lin(np.nan), equal_nan=True) and np.array_equal(mat("I0"), lin(0.0), equal_nan=True)
    assert not nc._eq_bits(mat("N"), mat("LD"))
