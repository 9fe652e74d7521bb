"""CPU checks of the two reference models the GPU tests lean on.

tests/environment_cases.reference_environments is pinned against dense vectors: the full walk is the overlap of the dense states,
and a left and a right environment that meet at a bond contract to the same number -- which fixes the leg order of the two sides
against each other.  tests/esprit_cases.model_pencil (site loops on host tensors) is pinned against the dense low-register matrix
R and then fed into the real esprit_from_pencil on every ESPRIT case: the pole error it reaches against the planted poles is
model_err, and the value recorded in the case table must be within 10x of what this run computes (both ways; values at the
rounding floor are compared from eps upwards, where a factor means nothing)."""
import numpy as np
import pytest

import environment_cases as EV
import esprit_cases as EC
from helpers import dense_mpo, dense_mps

EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize("case", ["small", "over_op", "paired"])
def test_the_environment_model_against_dense_vectors(case):
    n = EV.ntensors(case)
    for mix in EV.OP_MIXES:
        pc, wc, sc = mix
        phi, W, psi = EV.case_data(case, "phi", pc), EV.case_data(case, "W", wc), EV.case_data(case, "psi", sc)
        vphi, vpsi = dense_mps(phi).reshape(-1), dense_mps(psi).reshape(-1)
        for with_op, want in ((False, np.vdot(vphi, vpsi)), (True, np.vdot(vphi, dense_mpo(W).T @ vpsi))):
            if not with_op and wc:
                continue
            key = mix if with_op else (pc, sc)
            left, right = EV.reference(case, key, with_op, "left"), EV.reference(case, key, with_op, "right")
            scale = abs(left[n][1][0, 0, 0])
            for full in (left[n], right[n]):
                assert full[0].shape == (1, 1, 1) and abs(complex(full[0][0, 0, 0]) - want) <= 1e-13 * scale
            for k in range(n + 1):                                        # L_k . R_(n - k): the same number at every bond
                Lk, Rk = left[k][0], right[n - k][0]
                assert Lk.shape == Rk.shape
                assert abs(complex(np.sum(Lk * Rk)) - want) <= 1e-13 * scale, (k, mix, with_op)
                assert np.all(np.abs(Lk) <= left[k][1] * (1 + 1e-15))     # E_abs bounds E entry by entry
            assert left[0][2] == 0 and left[1][2] == (1 + 2 + 2 if with_op else 1 + 2)


def test_the_inner_length_of_a_walk():
    """L of the componentwise bound: s + 2 D + 2 p of the bonds a walk enters each site by"""
    pd, sd, od = EV.bond_dims("small")
    ref = EV.reference("small", (False, False, False), True, "left")
    assert [r[2] for r in ref] == list(np.cumsum([0] + [sd[i] + 2 * od[i] + 2 * pd[i] for i in range(5)]))
    ref = EV.reference("small", (False, False), False, "right")
    assert [r[2] for r in ref] == list(np.cumsum([0] + [sd[i] + 2 * pd[i] for i in range(5, 0, -1)]))
    assert EV.chain_eligible("over_state", False, "left", 1) and not EV.chain_eligible("over_state", False, "left", 2)
    assert EV.chain_eligible("over_op", False, "right", 5) and not EV.chain_eligible("over_op", True, "right", 3)
    assert EV.chain_eligible("over_op", True, "right", 2)


def test_the_pencil_model_against_the_dense_register():
    import qilaplace_jl_amd as qil
    data = EC.model_tensors("k4_damped", qil.exponential_tensors)
    n = len(data)
    for count in (1, 3, 6):
        T = data[n - count]
        for A in data[n - count + 1:]:
            T = np.tensordot(T, A, axes=([-1], [0]))
        R = T.reshape(T.shape[0], -1)
        G, P, r = EC.model_pencil(data, count)
        scale = np.abs(R @ R.conj().T).max()
        assert np.abs(G - R @ R.conj().T).max() <= 1e-13 * scale
        assert np.abs(P - R[:, 1:] @ R[:, :-1].conj().T).max() <= 1e-13 * scale
        assert np.abs(r - R[:, -1]).max() <= 1e-13 * np.abs(R).max()
    # the model's shift tensors are the package's
    for a, b in zip(qil.shift_mpo_tensors(4, 1), [EC.shift_tensor(int(i == 3), 1 if i == 0 else 2, 1 if i == 3 else 2) for i in range(4)]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", sorted(EC.CASES))
def test_model_err_is_what_the_table_records(case):
    import qilaplace_jl_amd as qil
    c = EC.CASES[case]
    data = EC.model_tensors(case, qil.exponential_tensors)
    count = EC.default_count(data)
    poles = qil.esprit_from_pencil(*EC.model_pencil(data, count))
    model_err = EC.pole_error(poles, c["poles"])
    print(f"{case}: count {count}, model_err {model_err:.3e}, recorded {c['model_err']:.3e}")
    assert max(model_err, EPS) <= 10 * max(c["model_err"], EPS) and max(c["model_err"], EPS) <= 10 * max(model_err, EPS)
    if case == "two_tones_n40":
        sep = abs(c["poles"][0] - c["poles"][2])
        assert abs(sep - 2 * np.pi * EC.DF40) < 1e-3 * sep                # 1.9e-9 in z
        assert 1000 * model_err < 1e-3 * sep                              # the model leaves the GPU test's condition a 1000x margin
        short = EC.pole_error(qil.esprit_from_pencil(*EC.model_pencil(data, 4)), c["poles"])
        assert short > 0.1 * sep                                          # four tensors do not separate the tones
    if case == "noisy_n14":
        short = EC.pole_error(qil.esprit_from_pencil(*EC.model_pencil(data, 3)), c["poles"])
        assert 100 * model_err < short                                    # the long register is what buys the accuracy
