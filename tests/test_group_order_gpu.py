"""Group device calls behind pending work on the caller's stream.

Every group member runs on a non-blocking stream of its own, and GroupGrid1.interp_dev / GroupGrid2.interp_dev take torch
tensors: the contract is that the work which produces those tensors, or which last wrote the result buffers, may still be
pending on torch's current stream of the member's device when the call is made (the call puts the members' streams behind
that stream, on the device, with mi_group_wait_stream).  Here the race is made deterministic: a delay of some tens of
milliseconds is put on torch's stream, then the operation under test, then the library is called at once -- enqueueing a
group call takes tens of microseconds of host time, so without the ordering the library's kernels run long before the
operation does.  Every buffer that could then be read stale holds zeros beforehand: a read that ran too early returns the
table's value at 0 (which no expected result equals, tests/test_group_cases_cpu.py), never uninitialised memory.

Expected results: oracle.interp1_arma / oracle.interp2_bilinear, bit for bit."""
import contextlib

import numpy as np
import pytest

import group_cases as gc
import oracle

pytestmark = pytest.mark.gpu

N1, N2 = 4098, 2049                    # queries per shard: interp1, interp2
DELAY_MIN_MS, DELAY_TARGET_MS, DELAY_CAP_MS = 5.0, 20.0, 50.0


@pytest.fixture(scope="module")
def delay():
    """delay(): enqueue DELAY_TARGET_MS or so of work on torch's current stream.  torch.cuda._sleep(cycles) where this build
    has it (one spinning thread: the device stays free for whatever is wrongly not ordered behind it), sized by one
    calibration run; else a fixed number of fills of one 1 GiB buffer.  Timed once, with torch events on an otherwise idle
    stream: at least DELAY_MIN_MS, or the tests below would have lost their teeth."""
    import torch

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    if hasattr(torch.cuda, "_sleep"):
        probe = 2_000_000
        torch.cuda._sleep(probe)                               # (first launch: loads the code object)
        ms = max(timed(lambda: torch.cuda._sleep(probe)), 1e-3)
        cycles = int(min(max(probe * DELAY_TARGET_MS / ms, 1.0), 2**31 - 1))
        fn = lambda: torch.cuda._sleep(cycles)                 # noqa: E731
    else:
        big = torch.empty(1 << 27, dtype=torch.float64, device="cuda")
        fn = lambda: [big.fill_(float(k)) for k in range(64)]  # noqa: E731
        fn()
    ms = timed(fn)
    print("delay on torch's stream: %.2f ms" % ms)
    assert ms >= DELAY_MIN_MS, "the delay is %.3f ms: too short to order anything" % ms
    assert ms <= 4 * DELAY_CAP_MS, "the delay is %.1f ms: the tests would no longer be quick" % ms
    return fn


@pytest.fixture(scope="module", params=[[0], [0, 0, 0]], ids=lambda d: "x".join(map(str, d)))
def rig(request):
    """one live group at a time, with the 1 001-node non-uniform table and the 33 x 29 grid on it"""
    import armadillocudalinearinterpolation_amd as mi
    grp = mi.Group(request.param)
    X, Y = gc.table1("nonuniform")
    x, y, z = gc.table2()
    t1, t2 = grp.grid1(X, Y), grp.grid2(x, y, z)
    # the first gathered call of a group binds RCCL and the first chunked one creates the exchange streams: host work of
    # milliseconds, behind which a delay on the device would have run out.  Done here, every call below only enqueues.
    for K in (3, 1):
        grp.set_gather_chunks(K)
        t1.interp_dev(_zeros(len(grp), N1), gather=True)
    t2.interp_dev(_zeros(len(grp), N2), _zeros(len(grp), N2), gather=True)
    yield grp, t1, t2
    grp.set_gather_chunks(1)
    t1.close()
    t2.close()
    grp.close()


N_SIDE = 8


@pytest.fixture(scope="module")
def side_streams():
    import torch
    return [torch.cuda.Stream() for _ in range(N_SIDE)]


def _callers(which, side_streams):
    """torch's current stream for the call: the default stream, or each of N_SIDE side streams in turn.  Why several:
    HIP maps streams onto a few hardware queues (4 by default), and a member's stream that shares its hardware queue with
    the caller's stream runs behind the delay whether the library orders it or not -- such a pair proves nothing.  A
    member's stream shares a queue with at most some of eight streams that are alive together, so an unordered call is
    caught on the others; every one of them must give the right result."""
    import torch
    return [contextlib.nullcontext()] if which == "default" else [torch.cuda.stream(s) for s in side_streams]


@pytest.fixture(scope="module")
def ref1():
    X, Y = gc.table1("nonuniform")
    q = gc.inside_queries(41, 3 * N1)
    ref = oracle.interp1_arma(X, Y, q)
    q.setflags(write=False)
    ref.setflags(write=False)
    return q, ref


@pytest.fixture(scope="module")
def ref2():
    x, y, z = gc.table2()
    xq, yq = gc.inside_queries(42, 3 * N2), gc.inside_queries(43, 3 * N2)
    ref = oracle.interp2_bilinear(x, y, z, xq, yq)
    for a in (xq, yq, ref):
        a.setflags(write=False)
    return xq, yq, ref


def _dev(a, P, n):
    import torch
    return [torch.from_numpy(a[r * n:(r + 1) * n].copy()).cuda() for r in range(P)]


def _zeros(P, n):
    import torch
    return [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(P)]


def _check1(P, outs, fulls, ref):
    for r in range(P):
        assert gc.same_bits(outs[r].cpu().numpy(), ref[r * N1:(r + 1) * N1]), "shard %d" % r
        if fulls is not None:
            assert gc.same_bits(fulls[r].cpu().numpy(), ref[:P * N1]), "gathered vector of member %d" % r


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "nosync"])
@pytest.mark.parametrize("stream", ["default", "side"])
@pytest.mark.parametrize("chunks", [1, 3])
def test_late_inputs_interp1(rig, delay, side_streams, ref1, chunks, stream, sync):
    """the copy that fills the query shards is still behind the delay when interp_dev is called"""
    import torch
    grp, t1, _ = rig
    P = len(grp)
    q, ref = ref1
    grp.set_gather_chunks(chunks)
    real = _dev(q, P, N1)
    for caller in _callers(stream, side_streams):
        xq, outs, fulls = _zeros(P, N1), _zeros(P, N1), _zeros(P, P * N1)
        torch.cuda.synchronize()
        with caller:
            delay()
            for r in range(P):
                xq[r].copy_(real[r])
            t1.interp_dev(xq, out=outs, gather=True, gathered=fulls, sync=sync)
            if not sync:
                grp.synchronize()
        _check1(P, outs, fulls, ref)


@pytest.mark.parametrize("stream", ["default", "side"])
def test_late_inputs_interp1_without_gather(rig, delay, side_streams, ref1, stream):
    import torch
    grp, t1, _ = rig
    P = len(grp)
    q, ref = ref1
    real = _dev(q, P, N1)
    for caller in _callers(stream, side_streams):
        xq, outs = _zeros(P, N1), _zeros(P, N1)
        torch.cuda.synchronize()
        with caller:
            delay()
            for r in range(P):
                xq[r].copy_(real[r])
            t1.interp_dev(xq, out=outs)
        _check1(P, outs, None, ref)


@pytest.mark.parametrize("stream", ["default", "side"])
@pytest.mark.parametrize("chunks", [1, 3])
def test_late_output_fill(rig, delay, side_streams, ref1, chunks, stream):
    """the fill of the gathered buffers (the -7 of tests/test_group_gpu.py's in-place section) is still behind the delay
    when the in-place gather call is made: it must run BEFORE the library's kernels and copies, not over their results"""
    import torch
    grp, t1, _ = rig
    P = len(grp)
    q, ref = ref1
    grp.set_gather_chunks(chunks)
    shards = _dev(q, P, N1)
    for caller in _callers(stream, side_streams):
        fulls = _zeros(P, P * N1)
        torch.cuda.synchronize()
        with caller:
            delay()
            for r in range(P):
                fulls[r].fill_(-7.0)
            inplace = [fulls[r][r * N1:(r + 1) * N1] for r in range(P)]
            t1.interp_dev(shards, out=inplace, gather=True, gathered=fulls)
        # the results are complete now -- and must still be there once the caller's stream has drained: read at once from
        # the default stream, they could be seen before a fill that was wrongly left behind them has landed
        torch.cuda.synchronize()
        for r in range(P):
            got = fulls[r].cpu().numpy()
            assert not np.any(got == -7.0), "member %d: %d elements still hold the fill" % (r, int(np.sum(got == -7.0)))
            assert gc.same_bits(got, ref[:P * N1])


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gather"])
@pytest.mark.parametrize("stream", ["default", "side"])
def test_late_inputs_interp2(rig, delay, side_streams, ref2, stream, gather):
    import torch
    grp, _, t2 = rig
    P = len(grp)
    xq, yq, ref = ref2
    rx, ry = _dev(xq, P, N2), _dev(yq, P, N2)
    for caller in _callers(stream, side_streams):
        xs, ys = _zeros(P, N2), _zeros(P, N2)
        torch.cuda.synchronize()
        with caller:
            delay()
            for r in range(P):
                xs[r].copy_(rx[r])
                ys[r].copy_(ry[r])
            res = t2.interp_dev(xs, ys, gather=gather)
        outs, fulls = res if gather else (res, None)
        for r in range(P):
            assert gc.same_bits(outs[r].cpu().numpy(), ref[r * N2:(r + 1) * N2]), "shard %d" % r
            if gather:
                assert gc.same_bits(fulls[r].cpu().numpy(), ref[:P * N2]), "gathered vector of member %d" % r
