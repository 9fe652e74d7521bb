"""GPU tests of qil.esprit / shift_pencil on the cases of tests/esprit_cases.py.  The yardstick is model_err, the pole error a
numpy model of shift_pencil (site loops on host tensors, then the same esprit_from_pencil) reaches against the planted poles --
recorded in the case table and re-derived by tests/test_esprit_model.py.  The device may be 100x worse: another summation order
passing through a non-normal eigenproblem."""
import gc

import numpy as np
import pytest

import esprit_cases as EC
from esprit_cases import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    yield
    gc.collect()                     # handles held by a caught exception's traceback go now, not inside a later test
    assert qil.default_context().unowned_bytes() == 0


def _match(found, planted):
    return [int(np.argmin(np.abs(np.asarray(found) - z))) for z in planted]


@pytest.mark.parametrize("case", EC.SUM_N10)
def test_planted_modes_of_an_exact_exponential_sum(qil, case):
    c = CASES[case]
    psi = qil.exponential_sum(c["amps"], c["poles"], c["n"], maxdim=None, tol=None)
    poles, amps, model, dist = qil.esprit(psi, return_model=True)
    assert len(poles) == len(c["poles"]) == len(amps)
    assert np.all(np.diff(np.abs(amps)) <= 0)                              # sorted by |amplitude|, descending
    err = EC.pole_error(poles, c["poles"])
    at = _match(poles, c["poles"])
    aerr = max(abs(amps[j] - a) / abs(a) for j, a in zip(at, c["amps"]))
    print(f"{case}: pole error {err:.3e} (model {c['model_err']:.3e}), amplitude error {aerr:.3e}, model distance {dist:.3e}")
    assert sorted(at) == list(range(len(at)))                             # every planted pole has its own estimate
    assert err <= max(100 * c["model_err"], 1e-13)
    assert aerr <= 1e-9
    assert dist <= 1e-10
    assert isinstance(model, qil.SignalMPS) and max(model.bond_dims) == len(poles)
    plain = qil.esprit(psi)
    assert len(plain) == 2 and np.array_equal(plain[0], poles) and np.array_equal(plain[1], amps)


def test_the_pencil_is_the_dense_register(qil):
    """shift_pencil against the dense low-register matrix R of the same state: G = R R^H, P = R[:, 1:] R[:, :-1]^H, r = R[:, -1]"""
    c = CASES["k4_damped"]
    psi = qil.exponential_sum(c["amps"], c["poles"], c["n"], maxdim=None, tol=None)
    data = psi.to_host()
    for count in (1, 3, 6):
        T = data[len(data) - count]
        for A in data[len(data) - count + 1:]:
            T = np.tensordot(T, A, axes=([-1], [0]))
        R = T.reshape(T.shape[0], -1)
        G, P, r = qil.shift_pencil(psi, count)
        scale = np.abs(R @ R.conj().T).max()
        assert np.abs(G - R @ R.conj().T).max() <= 1e-13 * scale
        assert np.abs(P - R[:, 1:] @ R[:, :-1].conj().T).max() <= 1e-13 * scale
        assert np.abs(r - R[:, -1]).max() <= 1e-13 * np.abs(R).max()


def test_two_tones_3e_10_apart_at_n_40(qil):
    c = CASES["two_tones_n40"]
    psi = qil.exponential_sum(c["amps"], c["poles"], c["n"], maxdim=None, tol=None)
    sep = abs(c["poles"][0] - c["poles"][2])                               # 1.9e-9 in z
    poles, _ = qil.esprit(psi)
    errs = [float(np.min(np.abs(poles - z))) for z in c["poles"]]
    short, _ = qil.esprit(psi, count=4)
    short_err = EC.pole_error(short, c["poles"])
    print(f"two tones: separation {sep:.3e}, errors {max(errs):.3e} (model {c['model_err']:.3e}), with count=4 {short_err:.3e}")
    assert max(errs) <= 1e-3 * sep                                         # both tones (and their conjugates) resolved
    assert short_err > 0.1 * sep                                           # four tensors do not separate them: the environment does


def test_a_noisy_dense_signal_through_the_encoder(qil):
    c = CASES["noisy_n14"]
    psi = qil.signal_mps(EC.dense_signal("noisy_n14"))
    poles, amps = qil.esprit(psi, maxdim=c["maxdim"])
    err = EC.pole_error(poles, c["poles"])
    short_err = EC.pole_error(qil.esprit(psi, maxdim=c["maxdim"], count=3)[0], c["poles"])
    at = _match(poles, c["poles"])
    aerr = max(abs(amps[j] - a) / abs(a) for j, a in zip(at, c["amps"]))
    print(f"noisy: pole error {err:.3e} (model {c['model_err']:.3e}), with count=3 {short_err:.3e}, amplitude error {aerr:.3e}")
    assert len(poles) == c["maxdim"]
    assert err <= 100 * c["model_err"]
    assert err < short_err
    assert max(psi.bond_dims) > c["maxdim"]                                # esprit compressed a copy, not the caller's state


def test_documented_errors(qil):
    c = CASES["k4_damped"]
    psi = qil.exponential_sum(c["amps"], c["poles"], c["n"], maxdim=None, tol=None)
    zt = qil.signal_ztmps(np.cos(0.3 * np.arange(64)))
    for fn, args in ((qil.esprit, ()), (qil.shift_pencil, (3,))):
        with pytest.raises(TypeError, match="a ZTMPS has no single sample register"):
            fn(zt, *args)
    for count in (0, c["n"], -1, 99):
        with pytest.raises(ValueError, match=r"outside \[1, 9\]"):
            qil.esprit(psi, count=count)
    for count in (1, 2):                                                   # 1 and 3 shifted columns for a bond of 4
        with pytest.raises(ValueError, match="fewer than the bond 4 at its cut"):
            qil.esprit(psi, count=count)
    assert len(qil.esprit(psi, count=3)[0]) == 4                           # 7 columns: enough
