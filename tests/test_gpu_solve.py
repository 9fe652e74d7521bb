"""GPU tests of qil.solve (qil_mps_solve) and its front-ends: every case of tests/solve_model.py on auto and on each forced route,
against numpy's dense solve under the derived bound
    |x - x_ref| / |x_ref| <= kappa * tol + sqrt((n - 1) * cutoff) + 64 * kappa * eps
(tests/solve_model.py has the derivation; tests/test_solve_model.py shows on the CPU that the inputs are solvable within the cap).
The route counters of `info` say which local solve ran; the decision is read through qil.solve_local_fits, so the byte formula may
change without touching this file.  After every test no pool memory is left outside a handle."""
import gc
import importlib

import numpy as np
import pytest

import solve_model as SM

pytestmark = pytest.mark.gpu

ROUTES = pytest.mark.parametrize("route", ["auto", "local", "gemm"])


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("qilaplace_jl_amd._lib")


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    gc.collect()
    assert qil.default_context().unowned_bytes() == 0


def _set_route(monkeypatch, route):
    if route == "auto":
        monkeypatch.delenv("QIL_SOLVE_ROUTE", raising=False)
    else:
        monkeypatch.setenv("QIL_SOLVE_ROUTE", route)


_DEV = {}


def _operands(qil, name):
    """(A, c, x0) of a case on the device, made once; amplitudes on the states as the case says"""
    if name not in _DEV:
        d = SM.case(name)
        ids = [int(v) for v in np.random.default_rng(91).permutation(500)[:d["n"]]]
        mpo, mps = (qil.PairedSiteMPO, qil.ZTMPS) if d["paired"] else (qil.SingleSiteMPO, qil.SignalMPS)
        x0 = None if d["x0"] is None else mps(d["x0"], sites=ids, amplitude=d["x0_amp"])
        _DEV[name] = (mpo(d["A"], sites=ids), mps(d["c"], sites=ids, amplitude=d["c_amp"]), x0, ids)
    return _DEV[name]


def _solve(qil, monkeypatch, name, route):
    A, c, x0, ids = _operands(qil, name)
    _set_route(monkeypatch, route)
    x, info = qil.solve(A, c, x0=x0, return_info=True, **SM.case(name)["kwargs"])
    return x, info


def _dense(x):
    return SM.dense_mps(x.to_host()) * x.amplitude


def _bonds(x):
    return [1] + list(x.bond_dims) + [1]


def _expected_local(qil, name, x):
    """local solves per half-sweep when x keeps the bonds it ends with, read through the host decision"""
    d = SM.case(name)
    cx = np.complex128 if any(np.iscomplexobj(t) for t in d["A"] + d["c"] + (d["x0"] or [])) else np.float64
    xb = _bonds(x)
    ab = [1] + [t.shape[3] for t in d["A"][:-1]] + [1]
    cb = [1] + [t.shape[2] for t in d["c"][:-1]] + [1]
    return sum(qil.solve_local_fits(xb[k], xb[k + 2], ab[k], ab[k + 1], ab[k + 2], cb[k], cb[k + 1], cb[k + 2], dtype=cx)
               for k in range(d["n"] - 1))


def _always_fits(qil, name):
    """whether every local problem the sweep can meet fits the one-launch route (the decision is monotone)"""
    d = SM.case(name)
    cx = np.complex128 if any(np.iscomplexobj(t) for t in d["A"] + d["c"] + (d["x0"] or [])) else np.float64
    X = min(d["kwargs"]["maxdim"], 2 ** (d["n"] // 2))
    D = max(t.shape[3] for t in d["A"])
    Cb = max(t.shape[2] for t in d["c"])
    return qil.solve_local_fits(X, X, D, D, D, Cb, Cb, Cb, dtype=cx)


def _check_common(qil, name, route, x, info):
    d = SM.case(name)
    kw = d["kwargs"]
    A, c, x0, ids = _operands(qil, name)
    assert type(x) is type(c) and x.site_ids == ids and x.paired == c.paired
    assert x.amplitude == c.amplitude
    assert max(x.bond_dims) <= kw["maxdim"] and info["max_bond"] == max(x.bond_dims)
    assert all(np.isfinite(t).all() for t in x.to_host())
    # the stopping rule
    assert 1 <= info["sweeps"] <= kw["max_sweeps"]
    assert info["converged"] == (info["residual"] <= kw["tol"])
    if not info["converged"]:
        assert info["sweeps"] == kw["max_sweeps"]
    # the routes
    steps = 2 * (d["n"] - 1) * info["sweeps"]
    assert info["local_solves"] + info["gemm_solves"] == steps
    assert info["matvecs"] >= steps
    if route == "gemm":
        assert info["local_solves"] == 0
    elif _always_fits(qil, name):
        assert info["gemm_solves"] == 0
    print(f"{name} [{route}]: {info}")


@ROUTES
@pytest.mark.parametrize("name", [k for k in SM.DENSE_CASES if SM.case(k)["kind"] != "conditions"])
def test_dense_cases_meet_the_derived_bound_on_every_route(qil, monkeypatch, name, route):
    x, info = _solve(qil, monkeypatch, name, route)
    _check_common(qil, name, route, x, info)
    ref, kappa = SM.reference(name)
    want = ref * SM.case(name)["c_amp"]
    err = float(np.linalg.norm(_dense(x) - want) / np.linalg.norm(want))
    bound = SM.bound(name, kappa)
    print(f"{name} [{route}]: error {err:.3e} bound {bound:.3e} kappa {kappa:.4g}")
    assert err <= bound, (name, route, err, bound)


@ROUTES
def test_helm8_with_the_identity_as_a_shift_gives_the_same_answer(qil, monkeypatch, route):
    x, _ = _solve(qil, monkeypatch, "helm8_f64", route)
    xs, _ = _solve(qil, monkeypatch, "helm8_shift", route)
    ref, kappa = SM.reference("helm8_f64")
    assert np.linalg.norm(_dense(x) - _dense(xs)) <= 2 * SM.bound("helm8_f64", kappa) * np.linalg.norm(ref)


@ROUTES
@pytest.mark.parametrize("name", ["straddle8_f64", "straddle8_c64"])
def test_bonds_on_both_sides_of_the_fit_take_their_routes(qil, monkeypatch, name, route):
    """The right-hand side has full bonds 2, 4, 8, 16, 8, 4, 2 and so has x throughout: the host decision, asked for each bond,
    splits them into both routes, and the counters of `info` show that each ran -- and that a forced local fell back to the GEMMs
    where the bond does not fit."""
    x, info = _solve(qil, monkeypatch, name, route)
    assert _bonds(x) == [1, 2, 4, 8, 16, 8, 4, 2, 1]
    per_half = _expected_local(qil, name, x)                             # under this route's QIL_SOLVE_ROUTE
    if route == "gemm":
        assert per_half == 0 and info["local_solves"] == 0 and info["gemm_solves"] == 14 * info["sweeps"]
    else:
        assert 0 < per_half < 7                                          # the case straddles the decision
        assert info["local_solves"] == 2 * per_half * info["sweeps"]
        assert info["gemm_solves"] == 2 * (7 - per_half) * info["sweeps"]


@ROUTES
def test_grow12_grows_the_rank_from_a_product_state(qil, monkeypatch, route):
    x, info = _solve(qil, monkeypatch, "grow12", route)
    assert max(_operands(qil, "grow12")[2].bond_dims) == 1
    assert info["max_bond"] == 13 and info["sweeps"] == 3                        # as the model


@ROUTES
def test_capped10_conditions(qil, monkeypatch, route):
    x, info = _solve(qil, monkeypatch, "capped10", route)
    _check_common(qil, "capped10", route, x, info)
    d = SM.case("capped10")
    assert max(x.bond_dims) <= 4
    start = SM._truncate_to(d["c"], 4)
    ref, _ = SM.reference("capped10")
    err = np.linalg.norm(_dense(x) - ref) / np.linalg.norm(ref)
    assert np.isfinite(err) and err < SM.rel_error(SM.dense_mps(start), "capped10")


@ROUTES
def test_exp40_matches_the_closed_form_row_by_row(qil, monkeypatch, route):
    A, c, _, _ = _operands(qil, "exp40")
    x, info = _solve(qil, monkeypatch, "exp40", route)
    _check_common(qil, "exp40", route, x, info)
    bits = SM.exp40_rows()
    got = qil.coefficient_batch(x, bits)
    want = qil.coefficient_batch(c, bits) / SM.exp40_lambda()
    kw = SM.case("exp40")["kwargs"]
    bound = SM.EXP40_KAPPA * kw["tol"] + np.sqrt((SM.EXP40_N - 1) * kw["cutoff"]) + 64 * SM.EXP40_KAPPA * SM.EPS
    rel = np.abs(got - want) / np.abs(want)
    print(f"exp40 [{route}]: worst row {rel.max():.3e} bound {bound:.3e}")
    assert rel.max() <= bound


# ---------------------------------------------------------------- errors
def _small(qil, n=3, seed=3):
    rng = np.random.default_rng(seed)
    return qil.SingleSiteMPO.identity(n), qil.SignalMPS(SM.random_state(SM.capped(n, 2), rng, False))


def test_argument_errors_raise_with_their_codes(qil, L):
    A, c = _small(qil)
    h = L.C.c_void_p()

    def code(**kw):
        a = dict(shift=0.0, maxdim=8, cutoff=1e-20, tol=1e-10, max_sweeps=2, cg_iters=10)
        a.update(kw)
        return L.lib.qil_mps_solve(A.handle, a["shift"], c.handle, None, a["maxdim"], a["cutoff"], a["tol"], a["max_sweeps"],
                                   a["cg_iters"], L.C.byref(h), None)

    for kw in (dict(maxdim=0), dict(max_sweeps=0), dict(cg_iters=0), dict(shift=np.nan), dict(cutoff=np.inf), dict(tol=np.nan),
               dict(cutoff=-1.0), dict(tol=0.0)):
        assert code(**kw) == L.QIL_EINVAL_ARG, kw
        with pytest.raises(ValueError, match="solve: "):
            qil.solve(A, c, **kw)
    assert L.lib.qil_mps_solve(None, 0.0, c.handle, None, 8, 0.0, 1e-10, 1, 1, L.C.byref(h), None) == L.QIL_EINVAL_ARG
    assert L.lib.qil_mps_solve(A.handle, 0.0, c.handle, None, 8, 0.0, 1e-10, 1, 1, None, None) == L.QIL_EINVAL_ARG
    assert h.value is None


def test_operand_errors_are_those_of_apply_and_inner(qil):
    A, c = _small(qil)
    with pytest.raises(ValueError, match="needs a bond"):
        qil.solve(qil.SingleSiteMPO.identity(1), qil.SignalMPS([np.ones((1, 2, 1))]))
    with pytest.raises(ValueError, match="apply: MPO and MPS must have the same number of sites"):
        qil.solve(qil.SingleSiteMPO.identity(4), c)
    with pytest.raises(ValueError, match="apply: MPO and MPS must have the same site indices"):
        qil.solve(qil.SingleSiteMPO.identity(3, sites=[7, 8, 9]), c)
    with pytest.raises(ValueError, match="inner: MPS must have the same number of sites"):
        qil.solve(A, c, x0=qil.SignalMPS(SM.random_state([2, 2, 2], np.random.default_rng(1), False)))
    with pytest.raises(ValueError, match="inner: MPS must have the same site indices"):
        qil.solve(A, c, x0=qil.SignalMPS(SM.random_state([2, 2], np.random.default_rng(1), False), sites=[4, 5, 6]))


@pytest.mark.parametrize("route", ["local", "gemm"])
def test_minus_identity_is_a_domain_error_not_a_fault(qil, monkeypatch, route):
    """A = -I is negative definite: the first p^H H p is negative, the loop exits on the flag and the verb returns QIL_EDOMAIN."""
    _set_route(monkeypatch, route)
    _, c = _small(qil, 4)
    minus = qil.mpo_scale(qil.SingleSiteMPO.identity(4), -1.0)
    x0 = qil.SignalMPS(SM.random_state([2, 2, 2], np.random.default_rng(8), False))
    with pytest.raises(qil.QilDomainError, match=r"solve: operator not positive definite on the local space \(bond 1\)"):
        qil.solve(minus, c, x0=x0)
    x = qil.solve(minus, c, x0=x0, shift=3.0)                               # -I + 3 I = 2 I
    assert np.linalg.norm(_dense(x) - _dense(c) / 2) <= (1e-10 + 64 * SM.EPS) * np.linalg.norm(_dense(c) / 2)     # kappa = 1, tol = 1e-10


def test_a_failed_allocation_leaves_nothing_behind(qil):
    A, c, _, _ = _operands(qil, "helm_n3")
    ctx = qil.default_context()
    ctx.trim()
    failures = 0
    for after in (0, 3, 11, 40):
        ctx.fail_alloc_after(after)
        try:
            qil.solve(A, c, **SM.case("helm_n3")["kwargs"])
        except MemoryError:
            failures += 1
        finally:
            ctx.fail_alloc_after(-1)
        gc.collect()
        assert ctx.unowned_bytes() == 0
    assert failures >= 3


# ---------------------------------------------------------------- front-ends
def test_build_laplacian_mpo_is_the_exact_second_difference(qil):
    lap = qil.build_laplacian_mpo(5)
    host = lap.to_host()
    assert lap.bond_dims == [5, 5, 5, 5] and all(np.array_equal(t, np.round(t.real)) for t in host)
    S = np.roll(np.eye(32), 1, axis=0)
    assert np.array_equal(SM.dense_op(host), 2 * np.eye(32) - S - S.T)
    assert np.array_equal(SM.dense_op(host), SM.dense_op(qil.laplacian_mpo_tensors(5)))


def test_least_squares_on_a_non_symmetric_fir_operator(qil, monkeypatch):
    monkeypatch.delenv("QIL_SOLVE_ROUTE", raising=False)
    n, reg, tol, cutoff = 8, 1e-3, 1e-12, 1e-24
    W = qil.fir_mpo((1.0, 0.5, 0.25), n)
    Wd = SM.dense_op(W.to_host())
    assert np.abs(Wd - Wd.T).max() > 0.1                                   # not symmetric
    b_data = SM.random_state(SM.capped(n, 3), np.random.default_rng(17), False)
    b = qil.SignalMPS(b_data, amplitude=1.5)
    x, info = qil.least_squares(W, b, reg=reg, tol=tol, cutoff=cutoff, return_info=True)
    N = Wd.conj().T @ Wd + reg * np.eye(2 ** n)
    ref = np.linalg.solve(N, Wd.conj().T @ (1.5 * SM.dense_mps(b_data)))
    kappa = np.linalg.cond(N)
    err = np.linalg.norm(_dense(x) - ref) / np.linalg.norm(ref)
    bound = kappa * tol + np.sqrt((n - 1) * cutoff) + 64 * kappa * SM.EPS
    print(f"least_squares: error {err:.3e} bound {bound:.3e} kappa {kappa:.4g} {info}")
    assert err <= bound and info["converged"]


def test_smooth_fills_a_masked_quarter(qil, monkeypatch):
    monkeypatch.delenv("QIL_SOLVE_ROUTE", raising=False)
    n, alpha, tol, cutoff = 8, 4.0, 1e-12, 1e-24
    N = 2 ** n
    rng = np.random.default_rng(23)
    t = np.arange(N) / N
    yv = np.sin(2 * np.pi * 3 * t) + 0.5 * np.cos(2 * np.pi * 7 * t) + 0.05 * rng.standard_normal(N)
    mv = np.ones(N)
    mv[(np.arange(N) % 16) >= 12] = 0.0                                    # a quarter of the samples, in runs of four
    assert mv.sum() == 3 * N // 4
    y = qil.SignalMPS(SM.tt_svd(yv, n, 0.0))
    mask = qil.SignalMPS(SM.tt_svd(mv, n, 1e-28))
    x, info = qil.smooth(y, alpha, mask=mask, tol=tol, cutoff=cutoff, return_info=True)
    S = np.roll(np.eye(N), 1, axis=0)
    M = np.diag(mv) + alpha * (2 * np.eye(N) - S - S.T)
    ref = np.linalg.solve(M, mv * yv)
    kappa = np.linalg.cond(M)
    err = np.linalg.norm(_dense(x) - ref) / np.linalg.norm(ref)
    bound = kappa * tol + np.sqrt((n - 1) * cutoff) + 64 * kappa * SM.EPS
    print(f"smooth (mask): error {err:.3e} bound {bound:.3e} kappa {kappa:.4g} {info}")
    assert err <= bound
    # without a mask: (I + alpha L) x = y, the identity as a shift
    x1 = qil.smooth(y, alpha, tol=tol, cutoff=cutoff)
    M1 = np.eye(N) + alpha * (2 * np.eye(N) - S - S.T)
    ref1 = np.linalg.solve(M1, yv)
    assert np.linalg.norm(_dense(x1) - ref1) / np.linalg.norm(ref1) <= np.linalg.cond(M1) * (tol + 64 * SM.EPS) + np.sqrt(7 * cutoff)
    # order 2: the operator is mpo_compress(L L)
    x2 = qil.smooth(y, 0.5, order=2, tol=tol, cutoff=cutoff)
    Lp = 2 * np.eye(N) - S - S.T
    M2 = np.eye(N) + 0.5 * Lp @ Lp
    ref2 = np.linalg.solve(M2, yv)
    assert np.linalg.norm(_dense(x2) - ref2) / np.linalg.norm(ref2) <= np.linalg.cond(M2) * (tol + 64 * SM.EPS) + np.sqrt(7 * cutoff) + 1e-12


def test_solve_residual_against_the_dense_residual_down_to_its_floor(qil, monkeypatch):
    monkeypatch.delenv("QIL_SOLVE_ROUTE", raising=False)
    for name in ("helm8_f64", "helm8_shift", "gram6_cc"):
        d = SM.case(name)
        A, c, _, _ = _operands(qil, name)
        shift = d["kwargs"]["shift"]
        M = SM.dense_op(d["A"]) + shift * np.eye(2 ** d["n"])
        cv = _dense(c)

        def dense_res(x):
            return float(np.linalg.norm(M @ _dense(x) - cv) / np.linalg.norm(cv))

        far = c                                                            # x = c: a residual of order one
        assert abs(qil.solve_residual(A, far, c, shift=shift) - dense_res(far)) <= 1e-9 * dense_res(far)
        kw = dict(d["kwargs"], tol=1e-3, max_sweeps=1)
        loose = qil.solve(A, c, **kw)
        assert dense_res(loose) > 1e-7
        assert abs(qil.solve_residual(A, loose, c, shift=shift) - dense_res(loose)) <= 1e-7
        tight = qil.solve(A, c, **d["kwargs"])
        assert dense_res(tight) < 1e-9 and qil.solve_residual(A, tight, c, shift=shift) <= 1e-6     # the floor, or 0
