"""GPU tests of qil.environment (qil_environment): every case of tests/environment_cases.py on both routes, both sides, every
count and every dtype mix against the longdouble model (pinned against dense vectors by tests/test_esprit_model.py).

The bound is componentwise: |got - ref| <= 4 L eps E_abs, with E_abs the same contraction of the |tensors| and L the sum over the
walked sites of the inner lengths of the three products (s + 2 D + 2 p; s + 2 p without an operator) -- the standard gamma bound
of a chain of inner products, the factor 4 rounding up the 2 sqrt 2 of complex multiplication, eps = 2^-52.  It is derived, not
fitted, and it catches an index error in a small entry that a norm-wise bound would hide.  Where a walk does not fit the
one-workgroup route a forced "chain" falls back to the GEMMs, as documented; the route hook says which one ran."""
import ctypes as C
import gc
import importlib

import numpy as np
import pytest

import environment_cases as EV
from environment_cases import CASES, SIDES, EPS

pytestmark = pytest.mark.gpu

ROUTES = pytest.mark.parametrize("route", ["chain", "gemm"])
CASE = pytest.mark.parametrize("case", sorted(CASES))


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    assert q.ops.ENV_CHAIN_MAX_OP_BOND == EV.CAP
    return q


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("qilaplace_jl_amd._lib")


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    gc.collect()                     # handles held by a caught exception's traceback go now, not inside a later test
    assert qil.default_context().unowned_bytes() == 0


_DEV = {}


def _operand(qil, case, which, complex_):
    """the device handle of one operand of a case, amplitude 1.75 / 0.5 on the states (never applied): made once"""
    key = (case, which, bool(complex_))
    if key not in _DEV:
        paired = CASES[case][3]
        data = EV.case_data(case, which, complex_)
        ids = [int(v) for v in np.random.default_rng(77).permutation(500)[:len(data)]]
        if which == "W":
            _DEV[key] = (qil.PairedSiteMPO if paired else qil.SingleSiteMPO)(data, sites=ids)
        else:
            _DEV[key] = (qil.ZTMPS if paired else qil.SignalMPS)(data, sites=ids, amplitude=1.75 if which == "phi" else 0.5)
    return _DEV[key]


def _operands(qil, case, mix, with_op):
    if with_op:
        pc, wc, sc = mix
        return _operand(qil, case, "phi", pc), _operand(qil, case, "W", wc), _operand(qil, case, "psi", sc)
    pc, sc = mix
    return _operand(qil, case, "phi", pc), None, _operand(qil, case, "psi", sc)


def _mixes(with_op):
    return EV.OP_MIXES if with_op else EV.STATE_MIXES


def _check(got, ref, what):
    E, Eabs, Lsum = ref
    want = np.asarray(E, dtype=np.complex128)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = 4 * max(Lsum, 1) * EPS * np.asarray(Eabs, dtype=np.float64)
    excess = np.abs(got.astype(np.clongdouble) - E) - bound
    assert np.all(excess <= 0), (what, float(excess.max()), float(bound.min()))


@CASE
@ROUTES
@pytest.mark.parametrize("with_op", [False, True], ids=["states", "operator"])
def test_every_count_side_and_dtype_mix_against_the_model(qil, monkeypatch, case, route, with_op):
    monkeypatch.setenv("QIL_ENV_ROUTE", route)
    pd, sd, od = EV.bond_dims(case)
    for mix in _mixes(with_op):
        phi, W, psi = _operands(qil, case, mix, with_op)
        for side in SIDES:
            ref = EV.reference(case, mix, with_op, side)
            for count in EV.counts(case):
                took = qil.ops.environment_route(side, count, pd, sd, od if with_op else None)
                assert took == ("CHAIN" if route == "chain" and EV.chain_eligible(case, with_op, side, count) else "GEMM")
                got = qil.environment(phi, psi, W=W, side=side, count=count)
                assert got.dtype == np.complex128 and got.ndim == (3 if with_op else 2)
                _check(got if with_op else got[:, None, :], ref[count], (case, route, mix, side, count))


@pytest.mark.parametrize("case", ["small", "cap", "over_state", "paired"])
def test_left_and_right_environments_meet_in_the_overlap(qil, case):
    """sum L_k[p, a, s] R_(n - k)[p, a, s] = inner / amplitudes at every bond k, both dtypes, with and without an operator: the leg
    order of the two sides against each other.  1e-12 of scale, the project's read-out tolerance."""
    n = EV.ntensors(case)
    for cplx in (False, True):
        for with_op in (False, True):
            mix = (cplx,) * (3 if with_op else 2)
            phi, W, psi = _operands(qil, case, mix, with_op)
            want = (qil.inner(phi, W, psi) if with_op else qil.inner(phi, psi)) / (phi.amplitude * psi.amplitude)
            scale = float(EV.reference(case, mix, with_op, "left")[n][1][0, 0, 0])
            for k in range(n + 1):
                Lk = qil.environment(phi, psi, W=W, side="left", count=k)
                Rk = qil.environment(phi, psi, W=W, side="right", count=n - k)
                assert Lk.shape == Rk.shape
                assert abs(np.sum(Lk * Rk) - want) <= 1e-12 * scale, (case, cplx, with_op, k)
            full = qil.environment(phi, psi, W=W)                          # count=None: the whole chain, right side
            assert full.shape == ((1, 1, 1) if with_op else (1, 1)) and abs(full.reshape(-1)[0] - want) <= 1e-12 * scale
            one = qil.environment(phi, psi, W=W, side="left", count=0)
            assert np.array_equal(one.reshape(-1), [1.0 + 0.0j])


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["f64", "c64"])
def test_the_right_environment_of_a_right_canonical_state_is_the_identity(qil, dt):
    from helpers import random_mps_data
    rng = np.random.default_rng(512)
    psi = qil.SignalMPS(random_mps_data([2, 4, 7, 12, 16, 8, 3, 2], rng, dtype=dt))
    qil.canonicalize(psi, "left")                                          # every tensor but the first a right isometry
    bonds = psi.bond_dims
    for count in range(1, len(psi)):
        E = qil.environment(psi, psi, side="right", count=count)
        chi = bonds[len(psi) - 1 - count]
        assert E.shape == (chi, chi)
        assert np.abs(E - np.eye(chi)).max() <= 1e-13, count


@pytest.mark.parametrize("case", ["small", "cap", "paired"])
def test_the_routes_agree(qil, monkeypatch, case):
    n = EV.ntensors(case)
    for with_op in (False, True):
        mix = (True, False, True) if with_op else (False, True)
        phi, W, psi = _operands(qil, case, mix, with_op)
        for side in SIDES:
            ref = EV.reference(case, mix, with_op, side)
            for count in (1, n - 1, n):
                got = {}
                for route in ("chain", "gemm"):
                    monkeypatch.setenv("QIL_ENV_ROUTE", route)
                    got[route] = qil.environment(phi, psi, W=W, side=side, count=count)
                bound = 8 * max(ref[count][2], 1) * EPS * np.asarray(ref[count][1], dtype=np.float64).reshape(got["gemm"].shape)
                assert np.all(np.abs(got["chain"] - got["gemm"]) <= bound), (case, with_op, side, count)


def test_the_size_query_and_the_raw_entry(qil, L):
    phi, W, psi = _operands(qil, "small", (False, True, False), True)
    pd, sd, od = EV.bond_dims("small")
    for side, code in (("left", 0), ("right", 1)):
        for count in range(6):
            dims = (C.c_int64 * 3)(-1, -1, -1)
            L.check(L.lib.qil_environment(phi.handle, W.handle, psi.handle, code, count, None, dims))
            b = count if side == "left" else 5 - count
            assert list(dims) == [pd[b], od[b], sd[b]]
            L.check(L.lib.qil_environment(phi.handle, None, psi.handle, code, count, None, dims))
            assert list(dims) == [pd[b], 1, sd[b]]
    assert qil.default_context().unowned_bytes() == 0
    # the raw entry fills exactly p a s complex doubles
    dims = (C.c_int64 * 3)()
    buf = np.full(2 * 3 * 2 * 2 + 2, np.nan)
    L.check(L.lib.qil_environment(phi.handle, W.handle, psi.handle, 0, 2, buf.ctypes.data_as(L._pdbl), dims))
    assert list(dims) == [3, 2, 2] and np.isfinite(buf[:-2]).all() and np.isnan(buf[-2:]).all()


def test_operand_mismatches_raise_as_inner_does(qil):
    from helpers import random_mps_data, random_mpo_data
    rng = np.random.default_rng(3)
    a5 = qil.SignalMPS(random_mps_data([2, 2, 2, 2], rng))
    a6 = qil.SignalMPS(random_mps_data([2, 2, 2, 2, 2], rng))
    other_ids = qil.SignalMPS(random_mps_data([2, 2, 2, 2], rng), sites=[9, 8, 7, 6, 5])
    zt = qil.ZTMPS(random_mps_data([2, 2, 2], rng))
    W6 = qil.SingleSiteMPO(random_mpo_data([2, 2, 2, 2, 2], rng))
    for args, kwargs in (((a5, a6), {}), ((a5, other_ids), {}), ((a5, zt), {}), ((a5, a5), {"W": W6}), ((a6, a5), {"count": 2})):
        with pytest.raises(ValueError) as env_err:
            qil.environment(*args, **kwargs)
        with pytest.raises(ValueError) as inner_err:
            qil.inner(args[0], kwargs["W"], args[1]) if "W" in kwargs else qil.inner(*args)
        assert str(env_err.value) == str(inner_err.value)
    other = qil.Context(0)
    try:
        b5 = qil.SignalMPS(random_mps_data([2, 2, 2, 2], rng), ctx=other)
        with pytest.raises(ValueError, match="inner: MPS belong to different contexts"):
            qil.environment(a5, b5)
        del b5
    finally:
        other.close()


@ROUTES
def test_a_failed_allocation_leaves_nothing_behind(qil, monkeypatch, route):
    monkeypatch.setenv("QIL_ENV_ROUTE", route)
    ctx = qil.default_context()
    phi, W, psi = _operands(qil, "cap", (False, True, True), True)
    want = qil.environment(phi, psi, W=W, side="right", count=4)
    before = ctx.unowned_bytes()
    failures = 0
    for k in range(12):
        ctx.fail_alloc_after(k)
        try:
            got = qil.environment(phi, psi, W=W, side="right", count=4)
        except MemoryError:
            failures += 1
            assert ctx.unowned_bytes() == before
            continue
        finally:
            ctx.fail_alloc_after(-1)
        assert np.array_equal(got, want)                                    # the call after the last failing one: the same numbers
        break
    assert failures >= 1
    assert np.array_equal(qil.environment(phi, psi, W=W, side="right", count=4), want)
