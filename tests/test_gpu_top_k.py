"""GPU tests of the top-k coefficient search (qil_top_k / qil.top_k): the k configurations with the largest |psi_x| and a bound
on what the beam search may have dropped.

The oracle is numpy's top-k of |dense vector| (helpers.dense_mps; flat index = the bit row read big-endian over the tensors).
Rows whose |value| lies within 1e-12 relative of the k-th value are exempt from set identity (rounding decides ties); values
match coefficient_batch to 1e-12 relative on the small cases and to 1e-10 at full size."""
import numpy as np
import pytest

from helpers import random_mps_data, saturated_profile, dense_mps, basis_mps

pytestmark = pytest.mark.gpu

TIE = 1e-12


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


def _mps(qil, data, paired, amp=1.0):
    return (qil.ZTMPS if paired else qil.SignalMPS)(data, amplitude=amp)


def _flat(rows):
    n = rows.shape[1]
    return rows.astype(np.int64) @ (np.int64(1) << np.arange(n - 1, -1, -1, dtype=np.int64))


def _check_rows(qil, psi, rows, vals, bound, rtol):
    """what holds whether or not the result is certified"""
    k = rows.shape[0]
    assert len(np.unique(_flat(rows))) == k, "repeated configuration"
    ref = qil.coefficient_batch(psi, rows)
    assert np.all(np.abs(vals - ref) <= rtol * np.abs(ref) + 1e-300), np.abs(vals - ref).max()
    mag = np.abs(vals)
    assert np.all(mag[1:] <= mag[:-1] * (1 + TIE)), "not sorted"
    assert bound >= 0.0


def _check_exact(dense, rows, vals, amp, k):
    """the result is the exact top-k of |amp * dense| (ties at the k-th value exempt)"""
    mag = np.abs(amp * dense.reshape(-1))
    top = np.sort(mag)[::-1][:k]
    np.testing.assert_allclose(np.abs(vals), top, rtol=TIE, atol=0)
    kth = top[-1]
    idx = _flat(rows)
    assert np.all(mag[idx] >= kth * (1 - TIE))
    must = np.nonzero(mag > kth * (1 + TIE))[0]
    assert set(must.tolist()) <= set(idx.tolist())


# ---------------------------------------------------------------- 1. dense oracle, nothing dropped
CASES = {
    "n1": [],
    "bond1": [1] * 7,
    "odd": [2, 3, 5, 7, 5, 3, 2],
    "sat8": saturated_profile(12, 8),
    "sat64": saturated_profile(14, 64),
}
KINDS = [(c, p) for c in sorted(CASES) for p in (False, True) if not (p and c == "n1")]


@pytest.mark.parametrize("dt", [np.float64, np.complex128])
@pytest.mark.parametrize("case,paired", KINDS)
def test_full_beam_is_certified_and_exact(qil, case, paired, dt):
    rng = np.random.default_rng(sorted(CASES).index(case) * 4 + 2 * paired + (dt == np.complex128))
    data = random_mps_data(CASES[case], rng, dt)
    n = len(data)
    psi = _mps(qil, data, paired, amp=-0.37)
    dense = dense_mps(data)
    for k in sorted({1, min(5, 2 ** n), min(37, 2 ** n), 2 ** n if case == "bond1" else 1}):
        rows, vals, bound, cert = qil.top_k(psi, k, beam=2 ** n, bits=True)
        assert rows.shape == (k, n) and rows.dtype == np.uint8 and vals.shape == (k,)
        assert vals.dtype == (np.complex128 if dt == np.complex128 else np.float64)
        assert bound == 0.0 and cert
        _check_rows(qil, psi, rows, vals, bound, 1e-12)
        _check_exact(dense, rows, vals, -0.37, k)


def test_index_and_pair_decoding(qil):
    rng = np.random.default_rng(5)
    data = random_mps_data(saturated_profile(10, 8), rng)
    rows, v, _, _ = qil.top_k(qil.SignalMPS(data), 6, beam=64, bits=True)
    idx, v2, _, _ = qil.top_k(qil.SignalMPS(data), 6, beam=64)
    assert np.array_equal(idx, _flat(rows)) and np.array_equal(v, v2)
    vec = dense_mps(data).reshape(-1)
    assert np.allclose(v, vec[idx], rtol=1e-12, atol=0)
    (kk, ll), vz, _, _ = qil.top_k(qil.ZTMPS(data), 6, beam=64)
    assert np.array_equal(kk, rows[:, 0::2].astype(np.int64) @ (1 << np.arange(5)))
    assert np.array_equal(ll, rows[:, 1::2].astype(np.int64) @ (1 << np.arange(5)))
    assert np.array_equal(vz, v)


# ---------------------------------------------------------------- 2. bound soundness
def test_bound_soundness_fuzz(qil):
    rng = np.random.default_rng(2024)
    certified = 0
    for trial in range(40):
        n = int(rng.integers(6, 13))
        cap = int(rng.choice([2, 4, 8, 16]))
        bonds = [int(rng.integers(1, cap + 1)) for _ in range(n - 1)]
        dt = np.complex128 if trial % 2 else np.float64
        data = random_mps_data(bonds, rng, dt)
        if trial % 3 == 0:                               # a peaked state: one heavy configuration on top of the noise
            for A in data:
                A[:, 0, :] *= 3.0
        psi = qil.SignalMPS(data, amplitude=1.7)
        k = int(rng.integers(1, 9))
        beam = int(rng.integers(k, 65))
        rows, vals, bound, cert = qil.top_k(psi, k, beam=beam, bits=True)
        _check_rows(qil, psi, rows, vals, bound, 1e-12)
        dense = 1.7 * dense_mps(data).reshape(-1)
        assert np.abs(vals[0]) <= np.abs(dense).max() * (1 + TIE)
        if cert:
            certified += 1
            _check_exact(dense, rows, vals, 1.0, k)
            assert np.all(np.abs(vals) >= bound)
    assert certified >= 5, certified


# ---------------------------------------------------------------- 3. structure
def test_qft_tones_are_found_and_certified(qil):
    n = 20
    N = 2 ** n
    t = np.arange(N)
    tones = [(3, 1.0), (1000, 0.6), (77777, 0.3)]
    x = sum(a * np.exp(2j * np.pi * k * t / N) for k, a in tones)
    psi = qil.signal_mps(x, cutoff=1e-15)
    out = qil.build_qft_mpo(psi) * psi
    vec = qil.mps_to_vector(out)
    want = np.argsort(np.abs(vec))[::-1][:3]
    idx, vals, bound, cert = qil.top_k(out, 3, beam=64)
    assert cert, (bound, vals)
    assert list(idx) == list(want)
    np.testing.assert_allclose(vals, vec[want], rtol=1e-9, atol=0)


@pytest.mark.parametrize("j", [0, 1, 2 ** 10 - 1, 357])
def test_basis_state_returns_itself_with_bound_zero(qil, j):
    psi = qil.SignalMPS(basis_mps(j, 10).data, amplitude=2.0)
    idx, vals, bound, cert = qil.top_k(psi, 1, beam=4)
    assert idx.tolist() == [j] and vals.tolist() == [2.0] and bound == 0.0 and cert


def test_bonds_past_128_match_the_dense_oracle(qil):
    rng = np.random.default_rng(129)
    for bonds in ([2, 4, 8, 16, 129, 16, 8, 4, 2], [2, 4, 8, 200, 8, 4, 2]):
        data = random_mps_data(bonds, rng, np.complex128)
        psi = qil.SignalMPS(data)
        n = len(data)
        rows, vals, bound, cert = qil.top_k(psi, 20, beam=2 ** n, bits=True)
        assert cert and bound == 0.0
        _check_rows(qil, psi, rows, vals, bound, 1e-12)
        _check_exact(dense_mps(data), rows, vals, 1.0, 20)


# ---------------------------------------------------------------- 4. full size
def test_full_size_matches_coefficients_and_is_deterministic(qil):
    psi = qil.ZTMPS.alloc(saturated_profile(48, 64), dtype=np.complex128, amplitude=2.5).fill_random(20241016)
    r1 = qil.top_k(psi, 16, beam=2 ** 16, bits=True)
    rows, vals, bound, _ = r1
    _check_rows(qil, psi, rows, vals, bound, 1e-10)
    r2 = qil.top_k(psi, 16, beam=2 ** 16, bits=True)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and r1[2] == r2[2] and r1[3] == r2[3]


def test_large_amplitude_neither_overflows_nor_underflows(qil):
    amp = float(np.exp(157.0))
    psi = qil.ZTMPS.alloc(saturated_profile(48, 16), dtype=np.complex128, amplitude=amp).fill_random(7)
    rows, vals, bound, _ = qil.top_k(psi, 8, beam=256, bits=True)
    assert np.all(np.isfinite(vals)) and np.all(np.abs(vals) > 0) and np.isfinite(bound)
    _check_rows(qil, psi, rows, vals, bound, 1e-10)
    small = qil.ZTMPS.alloc(saturated_profile(48, 16), dtype=np.complex128, amplitude=1.0 / amp).fill_random(7)
    rs, vs, bs, _ = qil.top_k(small, 8, beam=256, bits=True)
    assert np.array_equal(rs, rows)
    np.testing.assert_allclose(vs * amp * amp, vals, rtol=1e-12)
    assert bs * amp * amp == pytest.approx(bound, rel=1e-12)


# ---------------------------------------------------------------- 5. errors, allocation failures
def test_errors(qil):
    rng = np.random.default_rng(3)
    data = random_mps_data(saturated_profile(8, 8), rng)
    psi = qil.SignalMPS(data)
    idx, vals, bound, cert = qil.top_k(psi, 0, beam=0)
    assert idx.shape == (0,) and vals.shape == (0,) and bound == 0.0 and cert
    rows, _, _, _ = qil.top_k(psi, 0, bits=True)
    assert rows.shape == (0, 8)
    zero = [a.copy() for a in data]
    zero[4][:] = 0
    with pytest.raises(qil.QilDomainError, match="zero norm"):
        qil.top_k(qil.SignalMPS(zero), 3)
    with pytest.raises(ValueError, match="cap"):
        qil.top_k(psi, 1, beam=2 ** 40)
    with pytest.raises(ValueError, match="configurations"):
        qil.top_k(psi, 257, beam=512)


def test_failed_top_k_calls_leave_no_device_memory_behind(qil):
    ctx = qil.default_context()
    rng = np.random.default_rng(21)
    data = random_mps_data(saturated_profile(10, 16), rng, np.complex128)
    psi = qil.SignalMPS(data)
    ref = qil.top_k(psi, 5, beam=32, bits=True)
    failures = 0
    for j in range(0, 64):
        ctx.fail_alloc_after(j)
        try:
            got = qil.top_k(psi, 5, beam=32, bits=True)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, j
        if not failed:
            break
        failures += 1
    assert failures >= 10, failures
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    assert all(np.array_equal(psi.site(i), data[i]) for i in range(10))
