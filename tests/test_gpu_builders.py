"""GPU tests of the operator builders, whole: the persistent DT builder and its Jacobi SVD (csrc/qil_build_persist.hip), the
persistent complex chain builder (qil_build_chain.hip), the launch-per-step Builder (qil_build.hip) and the zT verb
(qil_build_zt.hip), on every route, against the oracle's operator of the SAME algorithm.

For every case of tests/builder_cases.py (validated on the CPU by tests/test_builder_cases_oracle.py) the device operator is
downloaded with to_host() and judged on the host -- no other device verb stands between the builder and the verdict:
  1. bond_dims equal the oracle's (every case has a decision margin >= 1e-3, so both must keep the same columns).  The one
     exception: the launch-per-step route pads the values of a batch to a common bond profile; there every bond is >= the
     oracle's, and diff_norm is blind to the padding;
  2. diff_norm(device, oracle) <= 32 max(y, L^2 2^-53): y = diff_norm(host restatement, oracle) is computed at run time from
     the two host implementations, never from the device; the floor is one rounding per site and layer; 32 is the allowance
     for Jacobi against LAPACK and another summation order.
The route a DT case takes is read from the line the persistent builder prints under QIL_DT_PROFILE (how many values went over
its in-LDS capacity) in a second build, which on the persistent route must repeat the first bit for bit; the chain builders'
persistent route is the entry itself, which reports a fallback.  The measured values are printed by the last test and recorded
in MEASUREMENTS.md."""
import gc
import re

import numpy as np
import pytest

import builder_cases as B

pytestmark = pytest.mark.gpu

MEASURED = {}            # case name -> (bond dimensions, y, device value, bound)


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    gc.collect()
    assert qil.default_context().unowned_bytes() == 0


def _ids(cases):
    return [c.name for c in cases]


def _judge(c, devs):
    """Assertions 1 and 2 for the device operators `devs` (site-tensor lists, one per damping value) of case c."""
    ref = B.reference(c)
    assert len(devs) == len(ref.oracle)
    padded = c.builder == "dt" and c.route != "persistent" and len(c.wrs) > 1
    worst = (0.0, 0.0, 0.0)
    for W, ora, y in zip(devs, ref.oracle, ref.y):
        got, want = B.bonds_of(W), B.bonds_of(ora)
        if padded:
            assert len(got) == len(want) and all(g >= w for g, w in zip(got, want)), (got, want)
        else:
            assert got == want, (got, want)
        d, bound = B.diff_norm(W, ora), B.bound(c, y)
        print(f"{c.name}: bonds max {max(got, default=1)}, y {y:.2e}, device {d:.2e}, bound {bound:.2e}")
        worst = max(worst, (d / bound, d, y))
        assert d <= bound, (c.name, d, y, bound)
    MEASURED[c.name] = ([max(B.bonds_of(o), default=1) for o in ref.oracle], worst[2], worst[1], B.bound(c, worst[2]))


# ---------------------------------------------------------------- DT
DT_ENV = {"persistent": {}, "overflow": {}, "launches": {"QIL_DT_BUILDER": "launches"}, "dcap8": {"QIL_DT_DCAP": "8"}}
OVER = re.compile(r"\[qil dt persistent\] kernel [0-9.]+ ms, (\d+) of (\d+) values over capacity")


def _build_dt(qil, c):
    return [W.to_host() for W in qil.build_dt_mpo_batch(c.n, list(c.wrs), cutoff=c.cutoff, maxdim=c.maxdim)]


@pytest.mark.parametrize("c", B.DT_CASES, ids=_ids(B.DT_CASES))
def test_dt_builder(qil, c, monkeypatch, capfd):
    for k, v in DT_ENV[c.route].items():
        monkeypatch.setenv(k, v)
    devs = _build_dt(qil, c)
    # the route: the same build again with the persistent builder's profile line on stderr
    monkeypatch.setenv("QIL_DT_PROFILE", "1")
    capfd.readouterr()
    again = _build_dt(qil, c)
    lines = OVER.findall(capfd.readouterr().err)
    if c.route == "launches":
        assert lines == []                                                   # the persistent kernel never ran
    else:
        assert len(lines) == 1 and int(lines[0][1]) == len(c.wrs), lines
        over = int(lines[0][0])
        if c.route == "persistent":
            assert over == 0
            assert all(np.array_equal(a, b) for W, V in zip(devs, again) for a, b in zip(W, V))
        else:                                                                # one value over capacity takes the whole batch
            assert over >= 1
    assert [B.bonds_of(W) for W in again] == [B.bonds_of(W) for W in devs]
    _judge(c, devs)


def test_dt_batches_equal_the_single_builds_bit_for_bit(qil, monkeypatch, capfd):
    """Persistent route: every value is its own workgroup and workspace slice, so batches of 1, 2, 5 and 70 mixed values give
    the operators of the single builds, bit for bit (and none of the 70 leaves the persistent route)."""
    n = B.BATCH_N
    single = {w: qil.build_dt_mpo_batch(n, [w])[0].to_host() for w in B.MIXED70}
    for size in B.BATCH_SIZES:
        wrs = list(B.MIXED70[-size:]) if size < 70 else list(B.MIXED70)
        monkeypatch.setenv("QIL_DT_PROFILE", "1")
        capfd.readouterr()
        Ws = qil.build_dt_mpo_batch(n, wrs)
        monkeypatch.delenv("QIL_DT_PROFILE")
        lines = OVER.findall(capfd.readouterr().err)
        assert lines == [("0", str(size))], lines
        assert len(Ws) == size
        for W, w in zip(Ws, wrs):
            got = W.to_host()
            assert len(got) == 2 * n and all(np.array_equal(a, b) for a, b in zip(got, single[w])), (size, w)


# ---------------------------------------------------------------- QFT and the paired QFT chain
def _chain(qil, c):
    import importlib
    Bd = importlib.import_module("qilaplace_jl_amd.builders")
    L = importlib.import_module("qilaplace_jl_amd._lib")
    ctx = qil.default_context()
    fn, cls, generic = ((L.lib.qil_build_qft_mpo, qil.SingleSiteMPO, qil.qft_mpo_device) if c.builder == "qft" else
                        (L.lib.qil_build_zt_qft_chain, qil.PairedSiteMPO, qil.zt_qft_chain_device))
    if c.route == "persistent":                  # the entry itself: it reports a fallback instead of taking it
        W = Bd._persistent_chain(fn, cls, c.n, list(range(1, c.sites + 1)), c.cutoff, c.maxdim, ctx)
        assert W is not None, "the persistent chain builder fell back"
        return W
    return generic(c.n, None, c.cutoff, c.maxdim, ctx, persistent=False)


@pytest.mark.parametrize("c", B.QFT_CASES + B.ZTQ_CASES, ids=_ids(B.QFT_CASES + B.ZTQ_CASES))
def test_qft_chain_builders(qil, c):
    W = _chain(qil, c)
    assert len(W) == c.n and W.dtype == np.complex128
    assert W.bond_dims == B.bonds_of(B.reference(c).oracle[0])
    _judge(c, [W.to_host()])
    if c.route == "persistent":                  # the front-end's default is this route
        front = (qil.qft_mpo_device if c.builder == "qft" else qil.zt_qft_chain_device)(c.n, None, c.cutoff, c.maxdim)
        assert all(np.array_equal(a, b) for a, b in zip(front.to_host(), W.to_host()))


# ---------------------------------------------------------------- zT
ZT_ROUTE = {"verb": "device", "parts": "parts", "host": "host"}


@pytest.mark.parametrize("c", B.ZT_CASES, ids=_ids(B.ZT_CASES))
def test_zt_builder(qil, c):
    Ws = qil.build_zt_mpo_batch(c.n, list(c.wrs), cutoff=c.cutoff, maxdim=c.maxdim, qft=ZT_ROUTE[c.route])
    assert all(W.ntensors == 2 * c.n and W.paired and W.dtype == np.complex128 for W in Ws)
    _judge(c, [W.to_host() for W in Ws])


# ---------------------------------------------------------------- refused damping values
@pytest.mark.parametrize("n,wrs,index,what", [
    (8, [0.5, float("nan")], 1, "not finite"), (8, [float("inf")], 0, "not finite"), (3, [1.0, 2.0, float("-inf")], 2, "not finite"),
    (24, [0.25, 1.0, -0.5], 2, "overflows"), (12, [-1.0], 0, "overflows")])
def test_bad_damping_values_are_refused_before_any_allocation(qil, n, wrs, index, what):
    ctx = qil.default_context()
    before = ctx.mem_info()
    ctx.fail_alloc_after(0)                      # an allocation in front of the check would fail with the pool's message
    try:
        for build in (qil.build_dt_mpo_batch, qil.build_zt_mpo_batch,
                      lambda n_, w_: qil.build_zt_mpo_batch(n_, w_, qft="parts")):
            with pytest.raises(ValueError, match=rf"damping value {index} .*{what}"):
                build(n, wrs)
    finally:
        ctx.fail_alloc_after(None)
    after = ctx.mem_info()
    assert (after["pool_in_use"], after["pool_cached"]) == (before["pool_in_use"], before["pool_cached"])
    # the same values one step inside the domain build (a negative damping is legal while its gates are finite)
    assert len(qil.build_dt_mpo_batch(3, [-0.5, 0.0])) == 2


# ---------------------------------------------------------------- failed hand-out of the launch-per-step route
def test_launch_route_failures_leave_no_handle_behind(qil, monkeypatch):
    """Whichever allocation of the launch-per-step build fails -- the hand-out of the finished operators at its end included,
    where the handles already made own their blocks and `unowned_bytes` cannot see them -- the pool's in-use bytes return to
    what they were, and the build succeeds afterwards."""
    monkeypatch.setenv("QIL_DT_BUILDER", "launches")
    ctx = qil.default_context()
    n, wrs = 2, [0.5, 1.5, 3.0]
    gc.collect()
    base = ctx.mem_info()["pool_in_use"]

    def attempt(k):
        ctx.fail_alloc_after(k)
        try:
            out = qil.build_dt_mpo_batch(n, wrs)
        except MemoryError:
            return False
        finally:
            ctx.fail_alloc_after(None)
        del out
        gc.collect()
        return True

    lo, hi = 0, 1                                # the call makes `hi` allocations: the smallest k at which it succeeds
    while not attempt(hi):
        assert ctx.mem_info()["pool_in_use"] == base and ctx.unowned_bytes() == 0, hi
        lo, hi = hi, 2 * hi
        assert hi < (1 << 20)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if attempt(mid):
            hi = mid
        else:
            assert ctx.mem_info()["pool_in_use"] == base and ctx.unowned_bytes() == 0, mid
            lo = mid
    assert ctx.mem_info()["pool_in_use"] == base
    tail = len(wrs) * (2 * n + 2) + 4            # covers every allocation of the hand-out: per value a handle's sites
    assert hi > tail
    for k in list(range(0, 6)) + list(range(hi - tail, hi)):
        assert not attempt(k), k
        assert ctx.unowned_bytes() == 0, k
        assert ctx.mem_info()["pool_in_use"] == base, (k, hi, ctx.mem_info()["pool_in_use"], base)
    Ws = qil.build_dt_mpo_batch(n, wrs)
    assert len(Ws) == len(wrs) and ctx.mem_info()["pool_in_use"] > base
    del Ws
    gc.collect()
    assert ctx.mem_info()["pool_in_use"] == base


# ---------------------------------------------------------------- the record
def test_print_measured_values():
    print("\ncase | max bond | y | device | bound")
    for name, (bonds, y, d, bound) in MEASURED.items():
        c = B.BY_NAME[name]
        print(f"{name} | {c.builder} {c.route} | {bonds} | {y:.2e} | {d:.2e} | {bound:.2e}")
