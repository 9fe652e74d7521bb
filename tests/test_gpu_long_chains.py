"""GPU tests of the grouped launches on chains whose site table is larger than one 64 KiB descriptor slot: apply, hadamard,
diagonal_mpo, adjoint, inner (chain route) and coefficient_batch (chain route) upload their table through the one device-table
helper, which takes a pool block for such a table instead of a slot of the descriptor ring.

The state is a product state, so every reference is a closed form: all bonds are 1, site i is the unit vector
(cos t_i, e^{i phi_i} sin t_i) with t_i <= 0.03, hence |psi| = 1 and the all-zero coefficient has modulus
prod cos t_i >= cos(0.03)^2100 = 0.38 -- nothing under- or overflows over 2 100 sites.

Tolerances.  apply: W is real with entries in (-1, 1) and |A| <= 1, so each component of an output element is a two-term sum
below 2 in modulus, rounded twice by the kernel's FMA chain and at most three times by numpy: the two differ by at most
5 x 2^-53 = 5.6e-16 per component, 7.9e-16 in modulus, inside the 1e-15 asked.  inner and the coefficients: about three
roundings of 2^-53 per site and side over 2 100 sites is 7e-13 at worst, inside 1e-12."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# table entries: the apply's and the product's ProductSite 72 B (overflows a 65 536 B slot from n = 911), MoveSite of
# diagonal_mpo / adjoint 40 B (from 1 639), InnerSite and the read-out's ChainSite 32 B (from 2 049)
N = 2100


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    assert qil.default_context().unowned_bytes() == 0


def _product_state(rng):
    t = rng.uniform(0.01, 0.03, N)
    ph = rng.uniform(0.0, 2 * np.pi, N)
    v = np.stack([np.cos(t).astype(np.complex128), np.exp(1j * ph) * np.sin(t)], axis=1)      # (N, 2)
    return v, [v[i].reshape(1, 2, 1) for i in range(N)]


@pytest.fixture(scope="module")
def host():
    """The operands on the host, made once and left unchanged."""
    rng = np.random.default_rng(2100)
    v, a = _product_state(rng)
    _, p = _product_state(rng)
    dims = [1] + [2] * (N - 1) + [1]
    w = [rng.uniform(-1.0, 1.0, (dims[i], 2, 2, dims[i + 1])) for i in range(N)]
    return {"v": v, "a": a, "p": p, "w": w}


@pytest.fixture(scope="module")
def dev(qil, host):
    return {"psi": qil.SignalMPS(host["a"]), "phi": qil.SignalMPS(host["p"]), "W": qil.SingleSiteMPO(host["w"])}


def _sites(chain):
    """every site tensor of a chain (chain.to_host() asks the library for the bond dimensions once per site)"""
    L = importlib.import_module("qilaplace_jl_amd._lib")
    d =[1] + chain.bond_dims + [1]
    mid = (2,) * chain._rank
    out = []
    for i in range(len(d) - 1):
        t = np.empty((d[i],) + mid + (d[i + 1],), dtype=chain.dtype, order="F")
        L.check(chain._fn("download_site")(chain.handle, i, t.ctypes.data_as(C.c_void_p)))
        out.append(t)
    return out


def test_apply_matches_the_per_site_contraction(qil, host, dev):
    out = qil.apply(dev["W"], dev["psi"])
    assert out.bond_dims == [2] * (N - 1) and out.dtype == np.complex128
    got = _sites(out)
    worst = 0.0
    for i in range(N):
        w, a = host["w"][i], host["a"][i]
        ref = np.einsum("atsb,xty->axsby", w, a).reshape(w.shape[0] * a.shape[0], 2, w.shape[3] * a.shape[2])
        assert got[i].shape == ref.shape, i
        worst = max(worst, np.abs(got[i] - ref).max())
    print(f"apply, n = {N}: largest site deviation {worst:.3e}")
    assert worst <= 1e-15, worst


def test_hadamard_equals_apply_of_the_diagonal_operator(qil, dev):
    D = qil.diagonal_mpo(dev["phi"])
    assert D.bond_dims == [1] * (N - 1)
    a, b = _sites(qil.hadamard(dev["phi"], dev["psi"])), _sites(qil.apply(D, dev["psi"]))
    assert len(a) == len(b) == N
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_adjoint_twice_is_the_operator(qil, host, dev):
    back = _sites(qil.adjoint(qil.adjoint(dev["W"])))
    assert len(back) == N
    assert all(np.array_equal(x, y) for x, y in zip(back, host["w"]))


def test_inner_on_the_chain_route(qil, dev, monkeypatch):
    monkeypatch.setenv("QIL_INNER_ROUTE", "chain")
    got = qil.inner(dev["psi"], dev["psi"])
    print(f"inner, n = {N}: |<psi|psi> - 1| = {abs(got - 1.0):.3e}")
    assert abs(got - 1.0) <= 1e-12, got


def test_coefficients_match_the_closed_form(qil, host, dev):
    v = host["v"]
    bits = np.zeros((5, N), dtype=np.uint8)
    for r, k in enumerate((0, 911, 1639, N - 1), start=1):        # one bit set: first and last site, and mid-chain
        bits[r, k] = 1
    want = np.array([np.prod(v[np.arange(N), row]) for row in bits])
    assert abs(want[0]) >= 0.38
    got = qil.coefficient_batch(dev["psi"], bits)
    rel = np.abs(got - want) / np.abs(want)
    print(f"coefficient_batch, n = {N}: relative deviations {rel}")
    assert np.all(rel <= 1e-12), rel
