"""Edge sweep of the multi-GPU layer's original entry points (csrc/mi_group.hip): mi_group_interp1_f64_dev with and without
the (chunked) gather at every (n_per_shard, K) of tests/group_cases.py, mi_group_interp2_f64_dev's gather in place and out
of place, the host forms at query counts that leave members without work, two calls back to back without a
synchronisation in between, every documented error, the six sharded host forms under a failure injected at the second
member (MI_TEST_FAIL_GROUP_SHARD), and group EDM at the smallest shard sizes.

Groups: GPU 0 named one, two, three and five times (a rehearsal group: device-to-device copies instead of RCCL), and every
device of the machine ([0] on a single-GPU one: the RCCL binding with one rank).  One group is alive at a time.  Every
interpolation result is held to oracle.interp1_arma / oracle.interp2_bilinear bit for bit, and to the single-context call."""
import ctypes as C

import numpy as np
import pytest

import group_cases as gc
import oracle

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
Z3 = [0.3310, 0.6914, 1.3557]
GROUPS = {"1": [0], "2": [0, 0], "3": [0, 0, 0], "5": [0] * 5, "all_gpus": None}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _padded(a, pad=1):
    """a's values as a view at an odd element offset of a larger tensor: 8-byte but not 16-byte aligned"""
    import torch
    big = torch.full((a.size + 2 * pad + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    big[pad:pad + a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return big, big[pad:pad + a.size]


def _ptrs(addresses):
    return (C.c_void_p * len(addresses))(*addresses)


@pytest.fixture(scope="module")
def rig(request, mi_ctx):
    """the live group (named by the test's indirect parameter; a new one is made only after the last one is closed) with the
    three tables on it, and the same tables on the single context"""
    import torch
    import armadillocudalinearinterpolation_amd as mi
    devices = GROUPS[request.param] or list(range(max(1, torch.cuda.device_count())))
    grp = mi.Group(devices)
    assert len(grp) == len(devices)
    X, Y = gc.table1("nonuniform")
    Xu, Yu = gc.table1("uniform")
    x, y, z = gc.table2()
    r = {"grp": grp, "P": len(devices), "L": grp._L,
         "nonuniform": grp.grid1(X, Y), "uniform": grp.grid1(Xu, Yu), "grid2": grp.grid2(x, y, z),
         "one_nonuniform": mi.Grid1.from_nodes(mi_ctx, X, Y), "one_uniform": mi.Grid1.from_nodes(mi_ctx, Xu, Yu),
         "one_grid2": mi.Grid2.from_axes(mi_ctx, x, y, z)}
    yield r
    for k in ("nonuniform", "uniform", "grid2", "one_nonuniform", "one_uniform", "one_grid2"):
        r[k].close()
    grp.close()


every_group = pytest.mark.parametrize("rig", list(GROUPS), indirect=True)


def _ref1(kind, q, extrap):
    X, Y = gc.table1(kind)
    return oracle.interp1_arma(X, Y, q, extrap=extrap)


# ---- interp1, device form --------------------------------------------------------------------------------------------

def _run_interp1(rig, kind, n, K, extrap, seed):
    """one (n, K): without gather, gather out of place, gather in place; results against the oracle and the single context"""
    import torch
    grp, P, tab = rig["grp"], rig["P"], rig[kind]
    q = gc.queries(seed, P * n)
    ref = _ref1(kind, q, extrap)
    if P * n:
        single = rig["one_" + kind].interp(_t(q), extrap=extrap).cpu().numpy()
        assert gc.same_bits(single, ref)
    grp.set_gather_chunks(K)
    shards = [_t(q[r * n:(r + 1) * n]) for r in range(P)]
    outs = tab.interp_dev(shards, extrap=extrap)
    for r in range(P):
        assert gc.same_bits(outs[r].cpu().numpy(), ref[r * n:(r + 1) * n]), ("plain", n, K, r)
    outs = [torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(P)]
    fulls = [torch.full((P * n,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(P)]
    tab.interp_dev(shards, extrap=extrap, out=outs, gather=True, gathered=fulls)
    for r in range(P):
        assert gc.same_bits(outs[r].cpu().numpy(), ref[r * n:(r + 1) * n]), ("gather", n, K, r)
        assert gc.same_bits(fulls[r].cpu().numpy(), ref), ("gathered", n, K, r)
    fulls = [torch.full((P * n,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(P)]
    inplace = [fulls[r][r * n:(r + 1) * n] for r in range(P)]
    tab.interp_dev(shards, extrap=extrap, out=inplace, gather=True, gathered=fulls)
    for r in range(P):
        assert gc.same_bits(fulls[r].cpu().numpy(), ref), ("in place", n, K, r)


@every_group
@pytest.mark.parametrize("kind,extrap", [("nonuniform", np.nan), ("nonuniform", -2.5), ("uniform", np.nan)])
def test_interp1_dev_every_chunk_pair(rig, kind, extrap):
    """every (n_per_shard, K) of group_cases.CHUNK_PAIRS -- the fallback below 2K, the first chunked size, fewer than K and
    exactly K chunks, a last chunk of one element, K = 64, odd n -- with queries that hold NaN, +-inf, both table ends and
    out-of-range values; extrap NaN and finite"""
    for i, (n, K) in enumerate(gc.CHUNK_PAIRS):
        _run_interp1(rig, kind, n, K, extrap, 1000 + i)
    rig["grp"].set_gather_chunks(1)


@every_group
def test_interp1_dev_chunk_count_changed_on_a_live_group(rig):
    """K = 1 -> 7 -> 2 -> 64 -> 3 on one group: the per-chunk event vectors grow and are then only partly used"""
    for i, K in enumerate(gc.CHUNK_SEQUENCE):
        _run_interp1(rig, "nonuniform", 4097, K, np.nan, 2000 + i)
        _run_interp1(rig, "nonuniform", 50, K, -2.5, 2100 + i)
    rig["grp"].set_gather_chunks(1)


@every_group
@pytest.mark.parametrize("K", [1, 3, 64])
def test_interp1_dev_views_at_an_odd_element_offset(rig, K):
    """xq, out and gathered handed over as views that start one element into a larger tensor (8-byte aligned only); the
    elements around the views keep their sentinel"""
    import torch
    grp, P, tab = rig["grp"], rig["P"], rig["nonuniform"]
    grp.set_gather_chunks(K)
    for n in (4097, 4100, 5):
        q = gc.queries(3000 + n + K, P * n)
        ref = _ref1("nonuniform", q, np.nan)
        xs = [_padded(q[r * n:(r + 1) * n]) for r in range(P)]
        os_ = [_padded(np.full(n, SENTINEL)) for _ in range(P)]
        fs = [_padded(np.full(P * n, SENTINEL)) for _ in range(P)]
        tab.interp_dev([v for _, v in xs], out=[v for _, v in os_], gather=True, gathered=[v for _, v in fs])
        for r in range(P):
            big, view = os_[r]
            assert view.data_ptr() % 16 == 8
            assert gc.same_bits(view.cpu().numpy(), ref[r * n:(r + 1) * n])
            assert big[0].item() == SENTINEL and torch.all(big[1 + n:] == SENTINEL).item()
            big, view = fs[r]
            assert gc.same_bits(view.cpu().numpy(), ref)
            assert big[0].item() == SENTINEL and torch.all(big[1 + P * n:] == SENTINEL).item()
        # in place inside the padded gathered vector
        fs = [_padded(np.full(P * n, SENTINEL)) for _ in range(P)]
        inplace = [fs[r][1][r * n:(r + 1) * n] for r in range(P)]
        tab.interp_dev([v for _, v in xs], out=inplace, gather=True, gathered=[v for _, v in fs])
        for r in range(P):
            big, view = fs[r]
            assert gc.same_bits(view.cpu().numpy(), ref)
            assert big[0].item() == SENTINEL and torch.all(big[1 + P * n:] == SENTINEL).item()
    grp.set_gather_chunks(1)


@every_group
@pytest.mark.parametrize("K", [1, 3])
def test_interp1_dev_no_queries_with_gather_leaves_the_buffers_alone(rig, K):
    """n = 0 with gather: MI_OK, and buffers the pointers refer to keep their sentinel"""
    import torch
    grp, P, L = rig["grp"], rig["P"], rig["L"]
    grp.set_gather_chunks(K)
    bufs = [torch.full((64,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3 * P)]
    torch.cuda.synchronize()
    xq, out, full = bufs[:P], bufs[P:2 * P], bufs[2 * P:]
    st = L.mi_group_interp1_f64_dev(grp._h, rig["nonuniform"]._h, _ptrs([t.data_ptr() for t in xq]),
                                    _ptrs([t.data_ptr() for t in out]), 0, float("nan"), _ptrs([t.data_ptr() for t in full]))
    assert st == 0
    grp.synchronize()
    assert all(torch.all(t == SENTINEL).item() for t in bufs)
    empty = [torch.empty(0, dtype=torch.float64, device="cuda") for _ in range(P)]
    outs, fulls = rig["nonuniform"].interp_dev(empty, gather=True)
    assert all(o.numel() == 0 for o in outs) and all(f.numel() == 0 for f in fulls)
    grp.set_gather_chunks(1)


# ---- interp2, device form ----------------------------------------------------------------------------------------------

@every_group
@pytest.mark.parametrize("n", [0, 1, 2, 4097])
def test_interp2_dev_gather_in_place_and_out_of_place(rig, n):
    """GroupGrid2.interp_dev allocates its results, so the in-place gather goes through the loaded library"""
    import torch
    grp, P, L, tab = rig["grp"], rig["P"], rig["L"], rig["grid2"]
    x, y, z = gc.table2()
    for extrap in (np.nan, 7.0):
        xq, yq = gc.queries(4000 + n, P * n), gc.queries(4100 + n, P * n)[::-1].copy()
        ref = oracle.interp2_bilinear(x, y, z, xq, yq, extrap=extrap)
        if P * n:
            assert gc.same_bits(rig["one_grid2"].interp(_t(xq), _t(yq), extrap=extrap).cpu().numpy(), ref)
        xs = [_t(xq[r * n:(r + 1) * n]) for r in range(P)]
        ys = [_t(yq[r * n:(r + 1) * n]) for r in range(P)]
        outs = tab.interp_dev(xs, ys, extrap=extrap)
        for r in range(P):
            assert gc.same_bits(outs[r].cpu().numpy(), ref[r * n:(r + 1) * n])
        outs, fulls = tab.interp_dev(xs, ys, extrap=extrap, gather=True)
        for r in range(P):
            assert gc.same_bits(outs[r].cpu().numpy(), ref[r * n:(r + 1) * n])
            assert gc.same_bits(fulls[r].cpu().numpy(), ref)
        # in place: member r's results already live in its gathered vector (which is one element longer than needed)
        fulls = [torch.full((P * n + 1,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(P)]
        torch.cuda.synchronize()                           # a C caller orders its own producers
        addr = lambda ts: _ptrs([t.data_ptr() if t.numel() else fulls[0].data_ptr() for t in ts])  # noqa: E731
        st = L.mi_group_interp2_f64_dev(grp._h, tab._h, addr(xs), addr(ys), _ptrs([fulls[r].data_ptr() + 8 * r * n for r in range(P)]),
                                        n, float(extrap), _ptrs([f.data_ptr() for f in fulls]))
        assert st == 0, L.mi_last_error(None)
        grp.synchronize()
        for r in range(P):
            got = fulls[r].cpu().numpy()
            assert gc.same_bits(got[:P * n], ref) and got[P * n] == SENTINEL


# ---- two calls back to back, no synchronisation in between -------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("rig", ["3"], indirect=True)
def test_back_to_back_calls_without_a_synchronisation(rig, K):
    """a gather call with queries A (sync=False), at once a plain call with queries B into the same out tensors
    (sync=False), then Group.synchronize(): every gathered vector is the oracle of A, every out the oracle of B.  In a
    rehearsal group member r's stream copies out of member s's out tensor: the second call's kernel on member s's stream
    has to wait for those reads."""
    import torch
    grp, P, tab = rig["grp"], rig["P"], rig["nonuniform"]
    n = 1 << 20
    X, Y = gc.table1("nonuniform")
    qa, qb = gc.inside_queries(5000 + K, P * n), gc.inside_queries(5100 + K, P * n)
    ra, rb = oracle.interp1_arma(X, Y, qa), oracle.interp1_arma(X, Y, qb)
    A = [_t(qa[r * n:(r + 1) * n]) for r in range(P)]
    B = [_t(qb[r * n:(r + 1) * n]) for r in range(P)]
    outs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(P)]
    fulls = [torch.zeros(P * n, dtype=torch.float64, device="cuda") for _ in range(P)]
    grp.set_gather_chunks(K)
    torch.cuda.synchronize()
    tab.interp_dev(A, out=outs, gather=True, gathered=fulls, sync=False)
    tab.interp_dev(B, out=outs, sync=False)
    grp.synchronize()
    grp.set_gather_chunks(1)
    bad = [(r, int(np.sum(fulls[r].cpu().numpy() != ra))) for r in range(P)]
    print("back to back, K=%d: elements of the gathered vectors that differ from the oracle of A: %s" % (K, bad))
    for r in range(P):
        assert gc.same_bits(fulls[r].cpu().numpy(), ra), "gathered vector of member %d" % r
        assert gc.same_bits(outs[r].cpu().numpy(), rb[r * n:(r + 1) * n]), "out of member %d" % r


# ---- host forms ----------------------------------------------------------------------------------------------------

@every_group
def test_host_forms_at_counts_that_leave_members_without_work(rig):
    P, L = rig["P"], rig["L"]
    x, y, z = gc.table2()
    for nq in gc.host_counts(P):
        q = gc.queries(6000 + nq, nq)
        for kind, extrap in (("nonuniform", np.nan), ("uniform", -2.5)):
            got = rig[kind].interp_host(q, extrap=extrap)
            assert L.mi_debug_pinned_ranges() == 0
            assert gc.same_bits(got, _ref1(kind, q, extrap)), (kind, nq)
        yq = gc.queries(6100 + nq, nq)[::-1].copy()
        got = rig["grid2"].interp_host(q, yq, extrap=7.0)
        assert L.mi_debug_pinned_ranges() == 0
        assert gc.same_bits(got, oracle.interp2_bilinear(x, y, z, q, yq, extrap=7.0)), nq


@every_group
def test_host_forms_large_then_one_then_large(rig):
    """200 003 -> 1 -> 200 003 queries on one live group: the members' scratch is grown, kept and reused"""
    L = rig["L"]
    x, y, z = gc.table2()
    big_x, big_y = gc.queries(6200, gc.HOST_LARGE), gc.queries(6201, gc.HOST_LARGE)[::-1].copy()
    ref1, ref2 = _ref1("nonuniform", big_x, np.nan), oracle.interp2_bilinear(x, y, z, big_x, big_y)
    for nq in (gc.HOST_LARGE, 1, gc.HOST_LARGE):
        sl = slice(0, nq) if nq > 1 else slice(7, 8)           # the single query is an ordinary in-range one
        assert gc.same_bits(rig["nonuniform"].interp_host(big_x[sl]), ref1[sl])
        assert L.mi_debug_pinned_ranges() == 0
        assert gc.same_bits(rig["grid2"].interp_host(big_x[sl], big_y[sl]), ref2[sl])
        assert L.mi_debug_pinned_ranges() == 0


# ---- errors ----------------------------------------------------------------------------------------------------------

def _still_works(rig):
    q = gc.queries(7000, rig["P"] * 5)
    assert gc.same_bits(rig["nonuniform"].interp_host(q), _ref1("nonuniform", q, np.nan))
    shards = [_t(q[r * 5:(r + 1) * 5]) for r in range(rig["P"])]
    _, fulls = rig["nonuniform"].interp_dev(shards, gather=True)
    assert all(gc.same_bits(f.cpu().numpy(), _ref1("nonuniform", q, np.nan)) for f in fulls)


@every_group
def test_errors_name_their_function_and_leave_the_group_usable(rig):
    import torch
    import armadillocudalinearinterpolation_amd as mi
    grp, P, L = rig["grp"], rig["P"], rig["L"]
    X, Y = gc.table1("nonuniform")
    x, y, z = gc.table2()
    last = lambda: L.mi_last_error(None).decode()              # noqa: E731
    # a table of another group, device and host calls, 1-D and 2-D
    other = mi.Group([0])
    try:
        o1, o2 = other.grid1(X, Y), other.grid2(x, y, z)
        bufs = [torch.zeros(4, dtype=torch.float64, device="cuda") for _ in range(P)]
        torch.cuda.synchronize()
        p = _ptrs([t.data_ptr() for t in bufs])
        host = np.zeros(4)
        hp = C.c_void_p(host.ctypes.data)
        assert L.mi_group_interp1_f64_dev(grp._h, o1._h, p, p, 4, 0.0, None) == 1 and "mi_group_interp1_f64_dev" in last()
        assert L.mi_group_interp1_f64_host(grp._h, o1._h, hp, hp, 4, 0.0) == 1 and "mi_group_interp1_f64_host" in last()
        assert L.mi_group_interp2_f64_dev(grp._h, o2._h, p, p, p, 4, 0.0, None) == 1 and "mi_group_interp2_f64_dev" in last()
        assert L.mi_group_interp2_f64_host(grp._h, o2._h, hp, hp, hp, 4, 0.0) == 1 and "mi_group_interp2_f64_host" in last()
        assert "another group" in last()
        grp.synchronize()
        assert all(torch.all(t == 0).item() for t in bufs) and not host.any()
        o1.close()
        o2.close()
    finally:
        other.close()
    _still_works(rig)
    for bad in (0, 65):
        with pytest.raises(mi.MiError) as e:
            grp.set_gather_chunks(bad)
        assert e.value.code == 1 and "mi_group_set_gather_chunks" in str(e.value)
        _still_works(rig)
    for devices in ([], [0] * 65):
        with pytest.raises(mi.MiError) as e:
            mi.Group(devices)
        assert e.value.code == 1 and "mi_group_create" in str(e.value)
    # the second member's context cannot be created: the first one is given back, and a new group works
    with pytest.raises(mi.MiError) as e:
        mi.Group([0, 99])
    assert e.value.code == 1 and "mi_ctx_create" in str(e.value) and "99" in str(e.value)
    g0 = mi.Group([0])
    try:
        t0 = g0.grid1(X, Y)
        q = gc.queries(7100, 9)
        assert gc.same_bits(t0.interp_host(q), _ref1("nonuniform", q, np.nan))
        t0.close()
    finally:
        g0.close()
    with pytest.raises(mi.MiError) as e:                       # fewer realisations than members
        grp.edm([13.0589], P - 1, n_grid=512)
    assert e.value.code == 1 and "mi_group_edm" in str(e.value)
    _still_works(rig)
    assert L.mi_debug_pinned_ranges() == 0


def _host_form_calls(rig, mi_ctx):
    """(entry point, call, expected) for the six sharded host forms at the smallest shapes that give two members work: 4097
    queries for interp1 / interp2, 2P + 1 columns for the others (n = 5, nxi = 9; nyi = 5).  Expected: the oracle for
    interp1 / interp2, the single-context device call for the column forms"""
    import armadillocudalinearinterpolation_amd as mi
    grp, P = rig["grp"], rig["P"]
    x, y, z = gc.table2()
    q, q2 = gc.queries(7200, 4097), gc.queries(7201, 4097)[::-1].copy()
    B, n, nxi = 2 * P + 1, 5, 9
    gx, gy = gc.queries(7202, B), gc.queries(7203, 5)
    Xb = np.cumsum(0.25 + oracle.splitmix_uniform(7204, B * n).reshape(B, n), axis=1)      # a strictly increasing X per column
    Yb = oracle.splitmix_uniform(7205, B * n).reshape(B, n) + 2.0
    xi = Xb[0, 0] + gc.queries(7206, nxi) * (Xb[0, -1] - Xb[0, 0])
    Q = Xb[:, :1] + gc.queries(7207, B * nxi).reshape(B, nxi) * (Xb[:, -1:] - Xb[:, :1])
    axis = mi.Axis1.from_nodes(mi_ctx, Xb[0])
    host = lambda t: t.cpu().numpy()                           # noqa: E731
    calls = [
        ("mi_group_interp1_f64_host", lambda: rig["nonuniform"].interp_host(q, extrap=-2.5), _ref1("nonuniform", q, -2.5)),
        ("mi_group_interp2_f64_host", lambda: rig["grid2"].interp_host(q, q2, extrap=7.0),
         oracle.interp2_bilinear(x, y, z, q, q2, extrap=7.0)),
        ("mi_group_interp2_grid_f64_host", lambda: rig["grid2"].interp_grid_host(gx, gy, extrap=7.0),
         host(rig["one_grid2"].interp_grid(_t(gx), _t(gy), extrap=7.0))),
        ("mi_group_interp1_cols_f64_host", lambda: grp.interp_cols_host(Xb[0], Yb.T, xi, extrap=-4.0),
         host(axis.interp_cols(_t(Yb).T, _t(xi), extrap=-4.0))),
        ("mi_group_interp1_pairs_f64_host", lambda: grp.interp_pairs_host(Xb.T, Yb.T, xi, extrap=-4.0),
         host(mi.interp_pairs(mi_ctx, _t(Xb).T, _t(Yb).T, _t(xi), extrap=-4.0))),
        ("mi_group_interp1_each_f64_host", lambda: grp.interp_each_host(Xb.T, Yb.T, Q.T, extrap=-4.0),
         host(mi.interp_each(mi_ctx, _t(Xb).T, _t(Yb).T, _t(Q).T, extrap=-4.0))),
        ("mi_group_interp1_each_f64_host", lambda: grp.interp_each_host(Xb.T, Yb.T, xi, extrap=-4.0),
         host(mi.interp_each(mi_ctx, _t(Xb).T, _t(Yb).T, _t(xi), extrap=-4.0))),
    ]
    axis.close()
    return calls


@every_group
def test_host_forms_failing_at_the_second_member_release_their_pins(rig, mi_ctx, monkeypatch):
    """MI_TEST_FAIL_GROUP_SHARD makes the shard loop fail in place of the second member that has work, with the first one's
    copies and kernel enqueued: every host form reports MI_ERR_HIP naming itself and the hook, and no range stays
    page-locked (the streams were drained and the pins given back).  A group of one member never trips the hook.  With the
    variable gone the same calls on the same group give the expected bits."""
    import armadillocudalinearinterpolation_amd as mi
    P, L = rig["P"], rig["L"]
    calls = _host_form_calls(rig, mi_ctx)
    assert L.mi_debug_pinned_ranges() == 0
    monkeypatch.setenv("MI_TEST_FAIL_GROUP_SHARD", "1")
    for who, call, want in calls:
        if P == 1:
            assert gc.same_bits(call(), want), who
        else:
            with pytest.raises(mi.MiError) as e:
                call()
            assert e.value.code == 3 and who + ":" in str(e.value) and "MI_TEST_FAIL_GROUP_SHARD" in str(e.value), who
        assert L.mi_debug_pinned_ranges() == 0, who
    monkeypatch.delenv("MI_TEST_FAIL_GROUP_SHARD")
    for who, call, want in calls:
        assert gc.same_bits(call(), want), who
        assert L.mi_debug_pinned_ranges() == 0, who
    _still_works(rig)


# ---- group EDM at the smallest shard sizes ---------------------------------------------------------------------------

@pytest.mark.parametrize("rig", ["3", "5"], indirect=True)
def test_group_edm_smallest_shards(rig, mi_ctx):
    """n_grid = 512, sigma = 0: with P, P + 1 and 2P - 1 realisations (every member one, one member two, all but one two) the
    residual and the partial block equal the single-context EventDrivenMap bit for bit; then n_real moves through those
    values on the live objects"""
    import armadillocudalinearinterpolation_amd as mi
    grp, P = rig["grp"], rig["P"]
    sizes = [P, P + 1, 2 * P - 1]
    expect = {}
    for R in sizes:
        one = mi.EventDrivenMap(mi_ctx, [13.0589], R, n_grid=512)
        expect[R] = one.ComputeF(Z3, want_partial=True)
        one.close()
        ge = grp.edm([13.0589], R, n_grid=512)
        f, p = ge.ComputeF(Z3, want_partial=True)
        assert np.array_equal(f, expect[R][0]) and np.array_equal(p, expect[R][1]), R
        assert [ge.shard_bounds(r) for r in range(P)] == [mi.shard_bounds(R, r, P) for r in range(P)]
        ge.close()
    ge = grp.edm([13.0589], sizes[0], n_grid=512)
    for R in (sizes[2], sizes[0], sizes[1], sizes[2], sizes[1], sizes[0]):
        ge.params.n_real = R
        ge._push()
        f, p = ge.ComputeF(Z3, want_partial=True)
        assert np.array_equal(f, expect[R][0]) and np.array_equal(p, expect[R][1]), R
        assert [ge.shard_bounds(r) for r in range(P)] == [mi.shard_bounds(R, r, P) for r in range(P)]
    ge.close()
