"""CPU: the numpy model of tests/mpo_algebra_cases.py in the device's place, against helpers.dense_mpo, on every case of at most
10 tensors and with the bounds the GPU test asserts (1e-14, 1e-12, 1e-13: the project's own numbers) -- the chosen inputs keep
the reference itself inside them.  And the shift operators of the host builder: dense-equal to the np.roll permutation,
orthogonal with exact integer overlaps, and the dyadic three-tap filter with its exact norm."""
import numpy as np
import pytest

import mpo_algebra_cases as cases
from helpers import dense_mpo


@pytest.mark.parametrize("name", [c.name for c in cases.SUMS])
def test_model_sum_against_dense(name):
    ref = cases.sum_reference(name)
    datas, handles, coeffs, ids = cases.sum_operands(name)
    assert len(ids) == len(ref) and (not cases.sum_case(name).paired or len(ref) % 2 == 0)
    bonds = [t.shape[3] for t in ref[:-1]]
    cases.check_sum_sites(name, ref, bonds)
    assert len(ref) <= 10
    cases.check_sum_dense(name, ref)


@pytest.mark.parametrize("name", [c.name for c in cases.INNERS])
def test_model_overlap_against_dense(name):
    v, w = cases.inner_operands(name)
    assert not cases.inner_case(name).paired or len(v) % 2 == 0
    got = cases.frobenius(v, w)
    cases.check_inner(name, got)
    cases.check_inner_agree(name, got, np.conj(cases.frobenius(w, v)))
    want, scale = cases.inner_reference(name)
    if len(v) >= 4:
        assert abs(want) <= 0.5 * scale                  # a random overlap is small against the norms: the scale must be theirs


def _shifts(n):
    return (0, 1, 2 ** n - 1, 2 ** (n - 1), 37 % 2 ** n, -3)


@pytest.mark.parametrize("n", range(1, 9))
def test_shift_tensors_are_the_roll_permutation(n):
    import qilaplace_jl_amd as qil
    for s in _shifts(n):
        data = qil.shift_mpo_tensors(n, s)
        assert np.array_equal(dense_mpo(data), cases.shift_dense(n, s)), (n, s)
        x = np.arange(2 ** n, dtype=np.float64)
        assert np.array_equal(dense_mpo(data).T @ x, np.roll(x, s)), (n, s)          # (S psi)_x = psi_{(x - s) mod 2^n}


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_shifts_are_orthogonal_with_exact_integer_overlaps(n):
    import qilaplace_jl_amd as qil
    shifts = sorted({s % 2 ** n for s in _shifts(n)})
    ops = {s: qil.shift_mpo_tensors(n, s) for s in shifts}
    for a in shifts:
        for b in shifts:
            assert cases.frobenius(ops[a], ops[b]) == (2 ** n if a == b else 0), (n, a, b)


@pytest.mark.parametrize("n", [2, 6, 8])
def test_dyadic_three_tap_filter_has_its_exact_norm(n):
    """0.5 S^0 + 0.25 S^1 - 0.125 S^3: dyadic weights and 0/1 entries keep every partial sum an integer multiple of 2^-6 far below
    2^53, so the norm is exact."""
    import qilaplace_jl_amd as qil
    taps = cases.SHIFT_TAPS
    terms = [qil.shift_mpo_tensors(n, k) for k in taps]
    total = cases.direct_sum(terms, list(taps.values()))
    assert cases.frobenius(total, total) == 2 ** n * cases.SHIFT_TAPS_NORM2_PER_SAMPLE
    want = sum(h * cases.shift_dense(n, k) for k, h in taps.items())
    assert np.array_equal(dense_mpo(total), want)
