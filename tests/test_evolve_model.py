"""The numpy restatement of qil.evolve (tests/evolve_model.py) against numpy's dense exponential, on the CPU: it meets the derived
bound B on every case that is exact in exact arithmetic, shows the first-order transient of a start narrower than the bonds it grows
to, shows that a binding maxdim leaves the projection error whatever the step, pins THE STIFF LIMIT and the matvec counts of the
identity and gram2 cases.  The GPU tests hold qil.evolve to the same table (tests/test_gpu_evolve.py)."""
import numpy as np
import pytest

import evolve_model as EV


@pytest.mark.parametrize("name", EV.IDENTITY_CASES + EV.EXACT_CASES)
def test_the_restatement_meets_the_derived_bound_on_every_exact_case(name):
    d = EV.case(name)
    v, info = EV.model(name)
    err, B = EV.rel_error(v, name), EV.bound(name)
    ev = EV.reference(name)[1]
    print(f"{name}: error {err:.3e} bound {B:.3e} {info}")
    assert abs(complex(d["t"]).real) * (ev[-1] - ev[0]) <= 3.0            # the cases stay where G is modest
    assert info["converged"] and info["local"] == d["n_local"]
    assert err <= B


def test_identity_and_gram2_matvec_counts():
    for name in EV.IDENTITY_CASES:
        d = EV.case(name)
        v, info = EV.model(name)
        assert info["matvecs"] == d["n_local"] == d["kwargs"]["steps"] * (4 * d["n"] - 6)   # A = I: beta_1 = 0, one matvec each
        want = EV.dense_mps(d["x0"]) * np.exp(d["t"])
        assert np.linalg.norm(v - want) <= 1e-13 * np.linalg.norm(want)
    v, info = EV.model("gram2")
    # one bond, a local space of 4 < krylov = 8: every exponential ends through the invariant-space branch after 4 vectors
    assert info["matvecs"] == 4 * EV.case("gram2")["n_local"] == 16 and info["estimate"] == 0.0
    assert EV.rel_error(v, "gram2") <= 1e-14


def test_sat6_imag_takes_the_halving_branch_and_still_converges():
    v, info = EV.model("sat6_imag")
    assert info["halved"] and info["substeps"] > 0 and info["converged"]
    # with one pass only the same case cannot meet tol and says so
    _, one = EV.model("sat6_imag", substeps=1)
    assert not one["converged"] and one["substeps"] == 0


def test_the_lanczos_exponential_agrees_with_the_dense_local_exponential():
    for name in ("sat6_f64", "sat6_c64_c"):
        v, _ = EV.model(name)
        w, _ = EV.model(name, dense_local=True)
        assert np.linalg.norm(v - w) <= EV.case(name)["n_local"] * 1e-10 * np.linalg.norm(w)


def _narrow_case():
    rng = np.random.default_rng(66)
    A = EV._normalised(EV.gram_tensors(EV.random_operator([2] * 5, rng, True)))
    x0 = EV.random_state([2] * 5, rng, True)
    M = EV.dense_op(A)
    ev, Z = np.linalg.eigh(M)
    return A, x0, lambda t: Z @ (np.exp(t * ev) * (Z.conj().T @ EV.dense_mps(x0)))


def test_a_start_narrower_than_the_bonds_it_grows_to_costs_first_order_in_tau():
    A, x0, exact = _narrow_case()
    t = 2.0j
    ref = exact(t)
    errs = []
    for steps in (1, 2, 4, 8):
        x, lg, info = EV.model_evolve(A, x0, t / steps, steps=steps, maxdim=8, cutoff=1e-24)
        errs.append(float(np.linalg.norm(EV.dense_mps(x) * np.exp(lg) - ref) / np.linalg.norm(ref)))
        assert info["max_bond"] == 8
    print("narrow start:", errs)
    assert errs[0] > 1e-4                                                   # far above the exact cases' 1e-11
    for a, b in zip(errs, errs[1:]):
        assert b <= 0.6 * a, errs


@pytest.mark.parametrize("name", EV.CAPPED_CASES)
def test_a_binding_maxdim_leaves_the_projection_error_whatever_the_step(name):
    d = EV.case(name)
    base = EV.rel_error(EV.model(name)[0], name)
    finer = EV.rel_error(EV.model(name, steps=4 * d["kwargs"]["steps"])[0], name)
    full = EV.rel_error(EV.model(name, maxdim=16)[0], name)
    print(f"{name}: maxdim 6 error {base:.3e}, 4 x the steps {finer:.3e}, maxdim 16 {full:.3e}")
    assert EV.model(name)[1]["max_bond"] <= 6
    assert base > 1e-5 and finer > 0.25 * base                              # does not fall with the step
    assert full <= EV.bound(name)                                           # and is the projection's alone: full bonds are exact


def test_the_stiff_limit_on_the_restatement():
    """tau = -20 in one step on the n = 8 Laplacian: the backward step exp(+10 H1) amplifies rounding by e^40; tau = -2.5 is fine."""
    n = 8
    A = EV.laplacian_tensors(n)
    rng = np.random.default_rng(88)
    x0 = EV.random_state(EV.capped(n, 16), rng, False)
    M = EV.dense_op(A)
    ev, Z = np.linalg.eigh(M)
    v0 = EV.dense_mps(x0)
    out = {}
    for tau in (-20.0, -2.5):
        ref = Z @ (np.exp(tau * ev) * (Z.T @ v0))
        x, lg, info = EV.model_evolve(A, x0, tau, steps=1, maxdim=16, cutoff=0.0, tol=1e-12, krylov=16, substeps=8)
        out[tau] = (float(np.linalg.norm(EV.dense_mps(x) * np.exp(lg) - ref) / np.linalg.norm(ref)), info["backward_growth"])
    print("stiff limit:", out)
    assert out[-20.0][0] > 1.0 and out[-20.0][1] > 30.0
    assert out[-2.5][0] <= 1e-9 and out[-2.5][1] <= 5.0
