"""CPU: the numpy restatement of qil.eigs (tests/eigs_model.py) meets every bound of its case table, so the GPU tests ask for
nothing the algorithm cannot deliver.  A case that misses here is changed, not its bound."""
import numpy as np
import pytest

import eigs_model as EM


@pytest.mark.parametrize("name", EM.IDENTITY_CASES)
def test_identity_passes_the_stopping_test_after_one_matvec_per_bond(name):
    d = EM.case(name)
    values, states, infos = EM.model(name)
    assert abs(values[0] - 1.0) <= 1e-14
    assert infos[0]["sweeps"] == 1 and infos[0]["converged"] and infos[0]["matvecs"] == 2 * (d["n"] - 1)
    want = EM.dense_mps(d["x0"])
    want = want / np.linalg.norm(want)
    assert np.linalg.norm(EM.dense_mps(states[0]) - want) <= 1e-13


@pytest.mark.parametrize("name", EM.DENSE_CASES)
def test_dense_cases_meet_the_derived_bounds(name):
    d = EM.case(name)
    values, states, infos = EM.model(name)
    for j in range(d["k"]):
        assert infos[j]["converged"] and infos[j]["sweeps"] <= d["kwargs"]["max_sweeps"], (name, j, infos[j])
        for label, got, bnd in EM.dense_checks(name, j, values[j], EM.dense_mps(states[j])):
            print(f"{name}[{j}] {label}: {got:.3e} bound {bnd:.3e} {infos[j]}")
            assert got <= bnd, (name, j, label, got, bnd)
    lam, _, gap = EM.wanted(name, d["k"] - 1)
    B, nrmA = EM.bound(name), EM.reference(name)[2]
    for i in range(d["k"]):
        for j in range(i):
            assert abs(np.vdot(EM.dense_mps(states[i]), EM.dense_mps(states[j]))) <= 2 * B * nrmA / min(
                EM.wanted(name, i)[2], EM.wanted(name, j)[2])


@pytest.mark.parametrize("name", EM.FIELD40_CASES)
def test_field40_matches_the_closed_form_without_a_dense_object(name):
    d = EM.case(name)
    values, states, infos = EM.model(name)
    lam, gap, vecs = EM.field_closed_form(40, EM.WHICH[d["which"]])
    assert infos[0]["converged"]
    assert abs(values[0] - lam) <= 64 * 40 * EM.EPS * abs(lam)
    assert all(t.shape[2] == 1 for t in states[0])
    bits = EM.field_rows(40)
    got = EM.coefficient_rows(states[0], bits)
    want = np.array([np.prod([vecs[j, b] for j, b in enumerate(row)]) for row in bits])
    got = got * np.sign((got[0] / want[0]).real)
    assert np.abs(got.imag).max() == 0.0
    assert np.max(np.abs(got.real - want) / np.abs(want)) <= 1e-12


@pytest.mark.parametrize("name", ["gram6_f64", "neg_gram6_c64"])
def test_ortho_without_a_weight_deflates_the_first_call(name):
    """eigs(A, ortho=[x1]) is the obvious way to ask for the next pair: the first call is deflated, with the weight from a probe"""
    d = EM.case(name)
    _, (x1, *_), _ = EM.model(name)
    values, states, infos = EM.model_eigs_k(d["A"], 2, EM.WHICH[d["which"]], seed=d["seed"] + 1, ortho=[x1], **d["kwargs"])
    for j in (1, 2):
        assert infos[j - 1]["converged"]
        for label, got, bnd in EM.dense_checks(name, j, values[j - 1], EM.dense_mps(states[j - 1])):
            assert got <= bnd, (name, j, label, got, bnd)


def test_a_space_smaller_than_krylov_ends_the_restart_through_the_breakdown_branch():
    """gram2: one bond, a local space of 4 < krylov = 8.  First solve: 4 vectors span the space (beta_3 <= 1e-14 scale), the Ritz
    pair is exact, one more matvec passes the stopping test; the three later solves of the two sweeps take one matvec each."""
    for info in EM.model("gram2")[2]:
        assert info["matvecs"] == 8 and info["sweeps"] == 2
    rng = np.random.default_rng(4)
    Q = np.linalg.qr(rng.standard_normal((12, 12)))[0]
    M = Q @ np.diag(np.arange(1.0, 13.0)) @ Q.T
    y0 = Q[:, [0, 4, 9]] @ np.array([0.5, -0.7, 0.4])                      # an invariant subspace of dimension 3
    y, theta, res0, scale, mv = EM.lanczos_local(lambda v: M @ v, y0, 1, 1e-10, 0.0, 8, 4, False)
    assert mv == 4 and abs(theta - 10.0) <= 1e-13 * 12 and abs(abs(y @ Q[:, 9]) - 1.0) <= 1e-13


def test_capped8_conditions():
    d = EM.case("capped8")
    values, states, infos = EM.model("capped8")
    x = states[0]
    assert max(t.shape[2] for t in x) <= 6
    v = EM.dense_mps(x)
    assert abs(np.linalg.norm(v) - 1.0) <= 64 * d["n"] * EM.EPS
    ev, _, nrmA = EM.reference("capped8")
    M = EM.dense_op(d["A"])
    assert values[0] <= ev[-1] + EM.bound("capped8") * nrmA
    assert abs(values[0] - np.vdot(v, M @ v).real) <= 64 * d["n"] * EM.EPS * nrmA


def test_the_local_solver_handles_its_edge_paths():
    rng = np.random.default_rng(3)
    M = rng.standard_normal((12, 12))
    M = M + M.T
    ev = np.linalg.eigvalsh(M)
    y0 = rng.standard_normal(12)
    for which in (0, 1):
        y, theta, res0, scale, mv = EM.lanczos_local(lambda v: M @ v, y0, which, 1e-12, 0.0, 8, 40, False)
        assert abs(theta - ev[-1 if which else 0]) <= 1e-10 * np.abs(ev).max() and mv <= 8 * 40
        assert scale <= np.abs(ev).max() * (1 + 1e-12)
    # an eigenvector as the start: one matvec, the stopping test
    z = np.linalg.eigh(M)[1][:, 0]
    y, theta, res0, scale, mv = EM.lanczos_local(lambda v: M @ v, z, 0, 1e-10, 0.0, 8, 4, False)
    assert mv == 1 and abs(theta - ev[0]) <= 1e-12 * np.abs(ev).max()
    with pytest.raises(ArithmeticError):
        EM.lanczos_local(lambda v: M @ v, np.zeros(12), 0, 1e-10, 0.0, 8, 4, False)
