"""GPU tests of qil.eigs (qil_mps_eigs) and its front-ends: every case of tests/eigs_model.py on auto and on each forced route,
against numpy's dense eigenpairs under the derived bounds
    B = tol + sqrt((n - 1) * cutoff) + 64 * n * eps
    |A v - theta v| / |A| <= B,   |theta - lambda_ref| / |A| <= B,   |v - z <z|v>| <= 2 * B * |A| / gap
(tests/eigs_model.py has the derivation; tests/test_eigs_model.py shows on the CPU that the restatement meets them).  The route
counters of `info` say which local solve ran; the decision is read through qil.eigs_local_fits, so the byte formula may change
without touching this file.  After every test no pool memory is left outside a handle.

Worst figures on one MI355X over the three route settings, against their bounds: residual 9.94e-11 of 1.03e-10 (`krylov2`, second
pair: by construction it ends just below tol, the local solves stop at |r| <= tol * scale), value 3.0e-15 of 1.0e-10, vector
2.3e-10 of 6.9e-10."""
import gc
import importlib

import numpy as np
import pytest

import eigs_model as EM

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
        monkeypatch.delenv("QIL_EIGS_ROUTE", raising=False)
    else:
        monkeypatch.setenv("QIL_EIGS_ROUTE", route)


_DEV = {}


def _operands(qil, name):
    """(A, x0) of a case on the device, made once"""
    if name not in _DEV:
        d = EM.case(name)
        ids = [int(v) for v in np.random.default_rng(92).permutation(500)[:d["n"]]]
        mpo, mps = (qil.PairedSiteMPO, qil.ZTMPS) if d["paired"] else (qil.SingleSiteMPO, qil.SignalMPS)
        x0 = None if d["x0"] is None else mps(d["x0"], sites=ids, amplitude=d["x0_amp"])
        _DEV[name] = (mpo(d["A"], sites=ids), x0, ids)
    return _DEV[name]


def _eigs(qil, monkeypatch, name, route, **over):
    d = EM.case(name)
    A, x0, ids = _operands(qil, name)
    _set_route(monkeypatch, route)
    kw = dict(d["kwargs"], **over)
    return qil.eigs(A, d["k"], d["which"], x0=x0, seed=d["seed"], return_info=True, **kw)


def _dense(x):
    return EM.dense_mps(x.to_host()) * x.amplitude


def _bonds(x):
    return [1] + list(x.bond_dims) + [1]


def _fits_per_half(qil, name, x, n_ortho):
    d = EM.case(name)
    cx = np.complex128 if EM.is_complex(name) else np.float64
    xb = _bonds(x)
    ab = [1] + [t.shape[3] for t in d["A"][:-1]] + [1]
    return sum(qil.eigs_local_fits(xb[k], xb[k + 2], ab[k], ab[k + 1], ab[k + 2], krylov=d["kwargs"]["krylov"], n_ortho=n_ortho,
                                   dtype=cx) for k in range(d["n"] - 1))


def _always_fits(qil, name, n_ortho):
    d = EM.case(name)
    cx = np.complex128 if EM.is_complex(name) else np.float64
    X = min(d["kwargs"]["maxdim"], 2 ** (d["n"] // 2))
    D = max(t.shape[3] for t in d["A"])
    return qil.eigs_local_fits(X, X, D, D, D, krylov=d["kwargs"]["krylov"], n_ortho=n_ortho, dtype=cx)


def _check_common(qil, name, route, j, x, info):
    d = EM.case(name)
    kw = d["kwargs"]
    A, x0, ids = _operands(qil, name)
    assert isinstance(x, qil.ZTMPS if d["paired"] else qil.SignalMPS) and x.site_ids == ids and x.amplitude == 1.0
    assert max(x.bond_dims) <= kw["maxdim"] and info["max_bond"] == max(x.bond_dims)
    assert all(np.isfinite(t).all() for t in x.to_host())
    assert abs(qil.norm(x) - 1.0) <= 64 * d["n"] * EM.EPS
    assert 1 <= info["sweeps"] <= kw["max_sweeps"]
    assert info["converged"] == (info["residual"] <= kw["tol"])
    if not info["converged"]:
        assert info["sweeps"] == kw["max_sweeps"]
    steps = 2 * (d["n"] - 1) * info["sweeps"]
    assert info["local_solves"] + info["gemm_solves"] == steps
    assert steps <= info["matvecs"] <= steps * kw["krylov"] * kw["restarts"]
    assert info["scale"] > 0
    if d["kind"] != "field40":                                             # a lower bound of |A|
        assert info["scale"] <= EM.reference(name)[2] * (1 + 1e-12)
    if route == "gemm":
        assert info["local_solves"] == 0
    elif _always_fits(qil, name, j):
        assert info["gemm_solves"] == 0
    print(f"{name}[{j}] [{route}]: {info}")


@ROUTES
@pytest.mark.parametrize("name", EM.IDENTITY_CASES)
def test_identity_passes_the_stopping_test_after_one_matvec_per_bond(qil, monkeypatch, name, route):
    d = EM.case(name)
    values, states, infos = _eigs(qil, monkeypatch, name, route)
    assert abs(values[0] - 1.0) <= 1e-14
    assert infos[0]["sweeps"] == 1 and infos[0]["converged"] and infos[0]["matvecs"] == 2 * (d["n"] - 1)
    want = EM.dense_mps(d["x0"])
    want = want / np.linalg.norm(want)
    got = _dense(states[0])
    assert np.linalg.norm(got * np.sign(np.vdot(want, got).real) - want) <= 1e-13


@ROUTES
@pytest.mark.parametrize("name", EM.DENSE_CASES)
def test_dense_cases_meet_the_derived_bounds_on_every_route(qil, monkeypatch, name, route):
    d = EM.case(name)
    values, states, infos = _eigs(qil, monkeypatch, name, route)
    vecs = [_dense(x) for x in states]
    B, nrmA = EM.bound(name), EM.reference(name)[2]
    for j in range(d["k"]):
        _check_common(qil, name, route, j, states[j], infos[j])
        for label, got, bnd in EM.dense_checks(name, j, values[j], vecs[j]):
            print(f"{name}[{j}] [{route}] {label}: {got:.3e} bound {bnd:.3e}")
            assert got <= bnd, (name, route, j, label, got, bnd)
        for i in range(j):                                                  # deflated results are mutually orthogonal
            gap = min(EM.wanted(name, i)[2], EM.wanted(name, j)[2])
            assert abs(np.vdot(vecs[i], vecs[j])) <= 2 * B * nrmA / gap


@ROUTES
@pytest.mark.parametrize("name", ["gram6_f64", "neg_gram6_c64"])
def test_ortho_without_a_weight_deflates_the_first_call(qil, monkeypatch, name, route):
    """eigs(A, k, ortho=[x1]) is the obvious way to ask for the next pairs after an earlier call: every call is deflated, the
    first one too, with the weight taken from an undeflated probe sweep.  Pairs 2 and 3 under the bounds of the dense cases."""
    d = EM.case(name)
    A, _, ids = _operands(qil, name)
    _set_route(monkeypatch, route)
    _, (x1,) = qil.eigs(A, 1, d["which"], seed=d["seed"], **d["kwargs"])
    values, states, infos = qil.eigs(A, 2, d["which"], ortho=[x1], seed=d["seed"] + 1, return_info=True, **d["kwargs"])
    vecs = [_dense(x1)] + [_dense(x) for x in states]
    B, nrmA = EM.bound(name), EM.reference(name)[2]
    for j in (1, 2):
        assert infos[j - 1]["converged"]
        for label, got, bnd in EM.dense_checks(name, j, values[j - 1], vecs[j]):
            print(f"{name} ortho [{route}] pair {j} {label}: {got:.3e} bound {bnd:.3e}")
            assert got <= bnd, (name, route, j, label, got, bnd)
        for i in range(j):
            assert abs(np.vdot(vecs[i], vecs[j])) <= 2 * B * nrmA / min(EM.wanted(name, i)[2], EM.wanted(name, j)[2])


@ROUTES
def test_a_space_smaller_than_krylov_ends_the_restart_through_the_breakdown_branch(qil, monkeypatch, route):
    """gram2: one bond, a local space of 4 < krylov = 8.  First solve: 4 vectors span the space (beta_3 <= 1e-14 scale: the
    breakdown branch), the Ritz pair is exact, one more matvec passes the stopping test; the three later solves of the two sweeps
    take one matvec each.  8 matvecs per pair, as the restatement."""
    values, states, infos = _eigs(qil, monkeypatch, "gram2", route)
    for info, model in zip(infos, EM.model("gram2")[2]):
        assert info["matvecs"] == model["matvecs"] == 8 and info["sweeps"] == 2 and info["converged"]


@ROUTES
@pytest.mark.parametrize("name", ["straddle8_f64", "straddle8_c64"])
def test_route_counts_follow_the_host_decision_on_settled_bonds(qil, monkeypatch, name, route):
    """x reaches the full bonds 2, 4, 8, 16, 8, 4, 2.  A sweep that starts from such a state meets the same bond dimensions at every
    step, so the counters of `info` are exactly the host decision, asked bond by bond: the bonds next to the ends take the
    one-launch route, the middle ones the GEMMs -- also under a forced local, which applies only where the bond fits."""
    d = EM.case(name)
    A, _, ids = _operands(qil, name)
    _set_route(monkeypatch, route)
    _, (x,) = qil.eigs(A, 1, "largest", seed=d["seed"], **d["kwargs"])
    assert _bonds(x) == [1, 2, 4, 8, 16, 8, 4, 2, 1]
    _, _, (info,) = qil.eigs(A, 1, "largest", x0=x, return_info=True, **dict(d["kwargs"], max_sweeps=1))
    per_half = _fits_per_half(qil, name, x, 0)
    assert info["local_solves"] == 2 * per_half and info["gemm_solves"] == 2 * (7 - per_half)
    assert (per_half == 0) if route == "gemm" else (0 < per_half < 7)
    assert info["converged"] and info["matvecs"] == 14                       # an eigenvector is a fixed point: one matvec per bond


@ROUTES
@pytest.mark.parametrize("name", EM.FIELD40_CASES)
def test_field40_matches_the_closed_form_without_a_dense_object(qil, monkeypatch, name, route):
    d = EM.case(name)
    values, states, infos = _eigs(qil, monkeypatch, name, route)
    _check_common(qil, name, route, 0, states[0], infos[0])
    lam, gap, vecs = EM.field_closed_form(40, EM.WHICH[d["which"]])
    assert infos[0]["converged"]
    assert abs(values[0] - lam) <= 64 * 40 * EM.EPS * abs(lam)
    assert states[0].bond_dims == [1] * 39
    bits = EM.field_rows(40)
    got = qil.coefficient_batch(states[0], bits)
    want = np.array([np.prod([vecs[j, b] for j, b in enumerate(row)]) for row in bits])
    got = got * np.sign((got[0] / want[0]).real)
    rel = np.abs(got - want) / np.abs(want)
    print(f"{name} [{route}]: theta error {abs(values[0] - lam) / abs(lam):.3e} worst row {rel.max():.3e} {infos[0]}")
    assert rel.max() <= 1e-12


@ROUTES
def test_capped8_conditions(qil, monkeypatch, route):
    d = EM.case("capped8")
    values, states, infos = _eigs(qil, monkeypatch, "capped8", route)
    x = states[0]
    _check_common(qil, "capped8", route, 0, x, infos[0])
    assert max(x.bond_dims) <= 6
    ev, _, nrmA = EM.reference("capped8")
    v = _dense(x)
    assert abs(np.linalg.norm(v) - 1.0) <= 64 * d["n"] * EM.EPS
    assert values[0] <= ev[-1] + EM.bound("capped8") * nrmA
    assert abs(values[0] - np.vdot(v, EM.dense_op(d["A"]) @ v).real) <= 64 * d["n"] * EM.EPS * nrmA


# ---------------------------------------------------------------- errors
def _small(qil, n=3, seed=3):
    rng = np.random.default_rng(seed)
    return qil.SingleSiteMPO.identity(n), qil.SignalMPS(EM.random_state(EM.capped(n, 2), rng, False))


def test_argument_errors_raise_with_their_codes_and_leave_the_outputs_untouched(qil, L):
    A, x0 = _small(qil)
    h = L.C.c_void_p(12345)
    theta = L.C.c_double(-7.0)
    ok = dict(which=0, n_ortho=0, weight=0.0, maxdim=8, cutoff=1e-20, tol=1e-10, max_sweeps=2, krylov=4, restarts=2)

    def code(A=A, x0=x0, ortho=None, **kw):
        a = dict(ok, **kw)
        return L.lib.qil_mps_eigs(A.handle, a["which"], x0.handle, ortho, a["n_ortho"], a["weight"], a["maxdim"], a["cutoff"], a["tol"],
                                  a["max_sweeps"], a["krylov"], a["restarts"], L.C.byref(h), L.C.byref(theta), None)

    for kw in (dict(which=2), dict(which=-1), dict(n_ortho=-1), dict(n_ortho=9), dict(n_ortho=1), dict(krylov=1), dict(krylov=17),
               dict(restarts=0), dict(maxdim=0), dict(max_sweeps=0), dict(weight=np.nan), dict(cutoff=np.inf), dict(tol=np.nan),
               dict(weight=-1.0), dict(cutoff=-1.0), dict(tol=0.0)):
        assert code(**kw) == L.QIL_EINVAL_ARG, kw
        assert L.last_error().startswith("eigs: ")
    for kw in (dict(which="middle"), dict(krylov=1), dict(tol=0.0)):
        with pytest.raises(ValueError, match="eigs: "):
            qil.eigs(A, x0=x0, **kw)
    # a mismatched deflation state: the operand errors of inner
    other = qil.SignalMPS(EM.random_state([2, 2, 2], np.random.default_rng(1), False))
    arr = (L.C.c_void_p * 1)(other.handle)
    assert code(ortho=arr, n_ortho=1) != L.QIL_OK and "inner: MPS must have the same number of sites" in L.last_error()
    with pytest.raises(ValueError, match="inner: MPS must have the same site indices"):
        qil.eigs(A, x0=x0, ortho=[qil.SignalMPS(EM.random_state([2, 2], np.random.default_rng(1), False), sites=[4, 5, 6])])
    with pytest.raises(ValueError, match="apply: MPO and MPS must have the same number of sites"):
        qil.eigs(qil.SingleSiteMPO.identity(4), x0=x0)
    with pytest.raises(ValueError, match="needs a bond"):
        qil.eigs(qil.SingleSiteMPO.identity(1), x0=qil.SignalMPS([np.ones((1, 2, 1))]))
    assert h.value == 12345 and theta.value == -7.0


@pytest.mark.parametrize("route", ["local", "gemm"])
def test_a_zero_start_and_a_non_finite_operator_are_domain_errors_not_faults(qil, monkeypatch, route):
    _set_route(monkeypatch, route)
    A, x0 = _small(qil, 4)
    zero = qil.SignalMPS([np.zeros((1, 2, 2)), np.zeros((2, 2, 2)), np.zeros((2, 2, 2)), np.zeros((2, 2, 1))])
    with pytest.raises(qil.QilDomainError, match="eigs: "):
        qil.eigs(A, x0=zero)
    bad = [np.eye(2).reshape(1, 2, 2, 1).copy() for _ in range(4)]
    bad[1][0, 0, 0, 0] = np.nan
    with pytest.raises(qil.QilDomainError, match=r"eigs: a Ritz value at bond \d is not finite"):
        qil.eigs(qil.SingleSiteMPO(bad), x0=x0)


def test_pool_live_bytes_are_equal_before_and_after_a_call(qil, monkeypatch):
    monkeypatch.delenv("QIL_EIGS_ROUTE", raising=False)
    A, _, _ = _operands(qil, "gram6_f64")
    ctx = qil.default_context()
    qil.eigs(A, 2, "largest", **EM.case("gram6_f64")["kwargs"])           # warm: the pool and the staging buffers have their size
    gc.collect()
    before = ctx.mem_info()
    values, states = qil.eigs(A, 2, "largest", **EM.case("gram6_f64")["kwargs"])
    held = sum(t.nbytes for x in states for t in x.to_host())
    del states
    gc.collect()
    after = ctx.mem_info()
    assert after["pool_in_use"] == before["pool_in_use"] and held > 0, (before, after, held)


def test_a_failed_allocation_leaves_nothing_behind(qil):
    A, _, _ = _operands(qil, "gram3_c64")
    ctx = qil.default_context()
    ctx.trim()
    failures = 0
    for after in (0, 3, 11, 40):
        ctx.fail_alloc_after(after)
        try:
            qil.eigs(A, 2, "largest", **EM.case("gram3_c64")["kwargs"])
        except MemoryError:
            failures += 1
        finally:
            ctx.fail_alloc_after(-1)
        gc.collect()
        assert ctx.unowned_bytes() == 0
    assert failures >= 3


# ---------------------------------------------------------------- front-ends
def test_eig_residual_against_the_dense_residual_down_to_its_floor(qil, monkeypatch):
    monkeypatch.delenv("QIL_EIGS_ROUTE", raising=False)
    name = "gram6_c64"
    d = EM.case(name)
    A, _, ids = _operands(qil, name)
    M = EM.dense_op(d["A"])
    nrmA = EM.reference(name)[2]

    def dense_res(x, theta):
        v = _dense(x)
        return float(np.linalg.norm(M @ v - theta * v) / np.linalg.norm(v))

    far = qil.SignalMPS(EM.random_state([2] * 5, np.random.default_rng(5), True), sites=ids, amplitude=1.5)
    for theta in (0.0, 0.3 * nrmA):
        assert abs(qil.eig_residual(A, far, theta) - dense_res(far, theta)) <= 1e-9 * dense_res(far, theta)
    (t1,), (loose,) = qil.eigs(A, 1, "largest", **dict(d["kwargs"], tol=1e-2, max_sweeps=1, krylov=2, restarts=1))
    assert dense_res(loose, t1) > 1e-6 * nrmA
    assert abs(qil.eig_residual(A, loose, t1) - dense_res(loose, t1)) <= 1e-7 * nrmA
    (t2,), (tight,) = qil.eigs(A, 1, "largest", **d["kwargs"])
    assert dense_res(tight, t2) < 1e-9 * nrmA and qil.eig_residual(A, tight, t2) <= 1e-6 * nrmA     # the floor, or 0


def test_operator_norm_of_a_random_operator(qil, monkeypatch):
    monkeypatch.delenv("QIL_EIGS_ROUTE", raising=False)
    n, kw = 6, dict(EM.EIGS_DEFAULTS)
    data = EM.random_operator([2] * (n - 1), np.random.default_rng(61), True)
    W = qil.SingleSiteMPO(data)
    want = float(np.linalg.norm(EM.dense_op(data), 2))
    got = qil.operator_norm(W, **kw)
    B = kw["tol"] + np.sqrt((n - 1) * kw["cutoff"]) + 64 * n * EM.EPS
    print(f"operator_norm: {got:.15g} numpy {want:.15g}")
    # sqrt of an eigenvalue of W^dagger W within B |W|^2, plus the 1e-14 cutoff of mpo_compress on the operator
    assert got <= want * (1 + 64 * n * EM.EPS) and want - got <= (B + 1e-13) * want


def test_condition_number_is_a_lower_bound_and_close(qil, monkeypatch):
    monkeypatch.delenv("QIL_EIGS_ROUTE", raising=False)
    d = EM.case("gram6_f64")
    n = d["n"]
    A, _, ids = _operands(qil, "gram6_f64")
    P = qil.mpo_linear_combination([A, qil.SingleSiteMPO.identity(n, sites=ids)], [1.0, 0.5])
    ev = EM.reference("gram6_f64")[0] + 0.5
    kappa = float(ev[-1] / ev[0])
    got = qil.condition_number(P, **d["kwargs"])
    print(f"condition_number: {got:.12g} numpy {kappa:.12g}")
    assert got <= kappa * (1 + EM.bound("gram6_f64")) and got >= 0.99 * kappa
