"""CPU checks of what the GPU tests of qil.solve rely on (tests/solve_model.py): the numpy restatement of the algorithm meets the
bound of every case within the case's max_sweeps -- so the inputs are known to be solvable within the cap before the device is
asked -- and the host tensors of the Laplacian are exactly 2 I - S - S^T."""
import numpy as np
import pytest

import solve_model as SM


@pytest.fixture(scope="module")
def solved():
    out = {}

    def get(name):
        if name not in out:
            d = SM.case(name)
            out[name] = SM.model_solve(d["A"], d["c"], d["x0"], **d["kwargs"])
        return out[name]
    return get


@pytest.mark.parametrize("name", [k for k in SM.DENSE_CASES if SM.case(k)["kind"] != "conditions"])
def test_the_model_meets_the_bound_of_every_dense_case(solved, name):
    x, info = solved(name)
    ref, kappa = SM.reference(name)
    err, bound = SM.rel_error(SM.dense_mps(x), name), SM.bound(name, kappa)
    print(f"{name}: error {err:.3e} bound {bound:.3e} kappa {kappa:.4g} {info}")
    assert info["sweeps"] <= SM.case(name)["kwargs"]["max_sweeps"]
    assert err <= bound, (name, err, bound)
    assert info["converged"] == (info["residual"] <= SM.case(name)["kwargs"]["tol"])


def test_grow12_grows_the_rank_from_a_product_state(solved):
    x, info = solved("grow12")
    assert all(t.shape == (1, 2, 1) for t in SM.case("grow12")["x0"])
    assert info["max_bond"] == 13 and info["sweeps"] == 3 and not info["converged"]     # the cutoff is coarser than tol


def test_capped10_conditions(solved):
    d = SM.case("capped10")
    x, info = solved("capped10")
    assert max(t.shape[2] for t in x) <= 4 and all(np.isfinite(t).all() for t in x)
    start = SM._truncate_to(d["c"], 4)
    assert SM.rel_error(SM.dense_mps(x), "capped10") < SM.rel_error(SM.dense_mps(start), "capped10")
    assert not info["converged"] and info["sweeps"] == d["kwargs"]["max_sweeps"]


def test_exp40_model_matches_the_closed_form(solved):
    x, info = solved("exp40")
    d = SM.case("exp40")
    bits = SM.exp40_rows()
    lam = SM.exp40_lambda()
    assert abs(lam - 2001.0000000114292) < 1e-9
    got, want = SM.coefficient_rows(x, bits), SM.coefficient_rows(d["c"], bits) / lam
    kw = d["kwargs"]
    bound = SM.EXP40_KAPPA * kw["tol"] + np.sqrt((SM.EXP40_N - 1) * kw["cutoff"]) + 64 * SM.EXP40_KAPPA * SM.EPS
    assert np.max(np.abs(got - want) / np.abs(want)) <= bound
    assert info["max_bond"] == 1 and info["converged"]


def test_the_laplacian_host_tensors_are_exact_at_n5():
    from qilaplace_jl_amd.builders import laplacian_mpo_tensors
    n, N = 5, 32
    data = laplacian_mpo_tensors(n)
    assert [t.shape for t in data] == [(1, 2, 2, 5)] + [(5, 2, 2, 5)] * 3 + [(5, 2, 2, 1)]
    assert all(np.array_equal(t, np.round(t)) for t in data)
    S = np.roll(np.eye(N), 1, axis=0)                               # (S v)_x = v_{x - 1}
    assert np.array_equal(SM.dense_op(data), 2 * np.eye(N) - S - S.T)
    with pytest.raises(ValueError, match="n must be >= 2"):
        laplacian_mpo_tensors(1)


def test_the_helmholtz_and_gram_operators_of_the_cases_are_hermitian_positive_definite():
    for name in ("helm8_f64", "helm8_shift", "gram6_cc", "gram6_rc", "paired3", "straddle8_c64"):
        d = SM.case(name)
        M = SM.dense_op(d["A"]) + d["kwargs"]["shift"] * np.eye(2 ** d["n"])
        assert np.abs(M - M.conj().T).max() <= 1e-13 * np.abs(M).max()
        assert np.linalg.eigvalsh(M).min() > 0
    M = SM.dense_op(SM.case("helm8_shift")["A"]) + np.eye(256)
    assert np.allclose(M, SM.dense_op(SM.case("helm8_f64")["A"]), atol=1e-13)
