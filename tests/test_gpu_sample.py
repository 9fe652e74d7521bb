"""GPU tests of perfect sampling (qil_sample / qil.sample): configurations x with probability |psi_x|^2 / |psi|^2.

The oracle is a numpy sequential sampler on the dense vector (helpers.dense_mps): its conditional probabilities come from
exact marginals of |psi|^2 and it applies the documented threshold rule s = 0 iff u (q_0 + q_1) < q_0.  A sample whose
oracle margin min_i |u (q_0 + q_1) - q_0| / (q_0 + q_1) is at most 1e-10 sits on a threshold where rounding may decide
either way: such rows are exempt from bit identity.  Probabilities agree to 1e-12 relative (the same products in a different
order); the full-size check against coefficient_batch to 1e-10."""
import numpy as np
import pytest

from helpers import random_mps_data, saturated_profile, dense_mps

pytestmark = pytest.mark.gpu

MARGIN = 1e-10


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


# ---------------------------------------------------------------- numpy restatements
def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def seeded_uniforms(seed, nb, n):
    """u[r, i] = (splitmix64(seed ^ splitmix64(r n + i)) >> 11) 2^-53 (include/qilaplace_hip.h, qil_sample)"""
    idx = (np.arange(nb, dtype=np.uint64)[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :])
    h = splitmix64(np.uint64(seed) ^ splitmix64(idx))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def oracle_sample(data, U):
    """(bits, probs, margin) of the sequential sampler on the dense |psi|^2 with the uniforms U (nb x n)"""
    p = np.abs(dense_mps(data)) ** 2
    n = p.ndim
    marg = [p.sum(axis=tuple(range(i + 1, n))).reshape(-1, 2) for i in range(n)]   # [prefix (MSB first), s]
    nb = U.shape[0]
    bits = np.zeros((nb, n), dtype=np.uint8)
    probs = np.ones(nb)
    margin = np.full(nb, np.inf)
    prefix = np.zeros(nb, dtype=np.int64)
    for i in range(n):
        q = marg[i][prefix]
        q0, q1 = q[:, 0], q[:, 1]
        tot = q0 + q1
        u = U[:, i]
        margin = np.minimum(margin, np.abs(u * tot - q0) / tot)
        s = np.where(u * tot < q0, 0, 1)
        probs *= np.where(s == 0, q0, q1) / tot
        bits[:, i] = s
        prefix = 2 * prefix + s
    return bits, probs, margin


def _mps(qil, data, paired, amp=1.0):
    return (qil.ZTMPS if paired else qil.SignalMPS)(data, amplitude=amp)


def _rank_deficient(rng, dtype):
    """saturated bonds with a site whose slice 1 is zero and a site of rank 1"""
    d = random_mps_data(saturated_profile(10, 16), rng, dtype, normalize=False)
    d[3][:, 1, :] = 0
    a, b = rng.standard_normal(d[5].shape[0]), rng.standard_normal(d[5].shape[2])
    d[5] = (a[:, None, None] * np.array([1.0, -0.5])[None, :, None] * b[None, None, :]).astype(dtype)
    return d


CASES = {
    "n1": lambda rng, dt: random_mps_data([], rng, dt),
    "pair1": lambda rng, dt: random_mps_data([1], rng, dt),
    "bond1": lambda rng, dt: random_mps_data([1] * 7, rng, dt),
    "odd": lambda rng, dt: random_mps_data([2, 3, 5, 7, 5, 3, 2], rng, dt),
    "sat16": lambda rng, dt: random_mps_data(saturated_profile(12, 16), rng, dt),
    "bond128": lambda rng, dt: random_mps_data([2, 4, 8, 16, 128, 16, 8, 4, 2], rng, dt),
    "bond129": lambda rng, dt: random_mps_data([2, 4, 8, 16, 129, 16, 8, 4, 2], rng, dt),
    "rankdef": _rank_deficient,
}


def _check_against_oracle(got_bits, got_probs, data, U):
    ob, op, margin = oracle_sample(data, U)
    ok = margin > MARGIN
    assert ok.mean() > 0.9, ok.mean()
    np.testing.assert_array_equal(got_bits[ok], ob[ok])
    rel = np.abs(got_probs[ok] - op[ok]) / op[ok]
    assert rel.max() < 1e-12, rel.max()


# ---------------------------------------------------------------- 1. oracle parity with given uniforms
CASE_KINDS = [(c, p) for c in sorted(CASES) for p in (False, True) if not (p and c == "n1")]   # a pair needs two tensors


@pytest.mark.parametrize("route", ["fused", "gemm"])
@pytest.mark.parametrize("dt", [np.float64, np.complex128])
@pytest.mark.parametrize("case,paired", CASE_KINDS)
def test_oracle_parity_with_given_uniforms(qil, case, paired, dt, route, monkeypatch):
    rng = np.random.default_rng(sorted(CASES).index(case) * 8 + 2 * paired + (dt == np.complex128))
    data = CASES[case](rng, dt)
    monkeypatch.setenv("QIL_SAMPLE_ROUTE", route)
    psi = _mps(qil, data, paired, amp=0.37)
    n = len(data)
    U = rng.random((700, n))
    b, p = qil.sample(psi, 700, uniforms=U, bits=True)
    assert b.shape == (700, n) and b.dtype == np.uint8 and p.shape == (700,)
    _check_against_oracle(b, p, data, U)


def test_index_decoding(qil):
    rng = np.random.default_rng(5)
    data = random_mps_data(saturated_profile(10, 8), rng)
    U = rng.random((256, 10))
    idx, p = qil.sample(qil.SignalMPS(data), 256, uniforms=U)
    b, p2 = qil.sample(qil.SignalMPS(data), 256, uniforms=U, bits=True)
    assert np.array_equal(idx, b.astype(np.int64) @ (1 << np.arange(9, -1, -1))) and np.array_equal(p, p2)
    vec = dense_mps(data).reshape(-1)
    psi = qil.SignalMPS(data)
    for j in idx[:5]:
        assert abs(qil.coefficient(psi, int(j)) - vec[j]) < 1e-12
    (k, l), pz = qil.sample(qil.ZTMPS(data), 256, uniforms=U)
    assert np.array_equal(k, b[:, 0::2].astype(np.int64) @ (1 << np.arange(5)))
    assert np.array_equal(l, b[:, 1::2].astype(np.int64) @ (1 << np.arange(5)))
    assert np.array_equal(pz, p)


# ---------------------------------------------------------------- 2. seeded path
@pytest.mark.parametrize("route", ["fused", "gemm"])
def test_seeded_path_is_the_documented_formula(qil, route, monkeypatch):
    monkeypatch.setenv("QIL_SAMPLE_ROUTE", route)
    rng = np.random.default_rng(8)
    data = random_mps_data(saturated_profile(12, 32), rng, np.complex128)
    psi = qil.SignalMPS(data)
    for seed in (0, 1234, 2 ** 64 - 1):
        U = seeded_uniforms(seed, 1000, 12)
        assert U.min() >= 0 and U.max() < 1
        b1, p1 = qil.sample(psi, 1000, seed=seed, bits=True)
        b2, p2 = qil.sample(psi, 1000, uniforms=U, bits=True)
        assert np.array_equal(b1, b2) and np.array_equal(p1, p2)
    _check_against_oracle(b1, p1, data, U)


# ---------------------------------------------------------------- 3. invariance
def test_prefix_route_and_amplitude_invariance(qil, monkeypatch):
    rng = np.random.default_rng(9)
    data = random_mps_data(saturated_profile(12, 32), rng, np.complex128)
    U = seeded_uniforms(77, 4096, 12)
    ok = oracle_sample(data, U)[2] > MARGIN
    got = {}
    for route in ("fused", "gemm"):
        monkeypatch.setenv("QIL_SAMPLE_ROUTE", route)
        b10, p10 = qil.sample(qil.SignalMPS(data), 10, seed=77, bits=True)
        b, p = qil.sample(qil.SignalMPS(data), 4096, seed=77, bits=True)
        assert np.array_equal(b10[ok[:10]], b[:10][ok[:10]])
        assert np.allclose(p10[ok[:10]], p[:10][ok[:10]], rtol=1e-13, atol=0)
        ba, pa = qil.sample(qil.SignalMPS(data, amplitude=-3.5e7), 4096, seed=77, bits=True)
        assert np.array_equal(ba, b) and np.array_equal(pa, p)
        got[route] = (b, p)
    assert np.array_equal(got["fused"][0][ok], got["gemm"][0][ok])
    assert np.allclose(got["fused"][1][ok], got["gemm"][1][ok], rtol=1e-12, atol=0)


# ---------------------------------------------------------------- 4. structure: the tones of a Fourier transform
def test_samples_land_on_the_tones_of_a_qft(qil):
    n = 20
    N = 2 ** n
    t = np.arange(N)
    tones = [(3, 1.0), (1000, 0.6), (77777, 0.3)]
    x = sum(a * np.cos(2 * np.pi * k * t / N) for k, a in tones)
    psi = qil.signal_mps(x, cutoff=1e-15)
    out = qil.build_qft_mpo(psi) * psi
    idx, p = qil.sample(out, 2 ** 14, seed=4)
    # coefficient(out, lsb bits of k) = fft(x)[k] / sqrt(N): a big-endian sample index is k bit-reversed
    rev = lambda k: int(format(k, f"0{n}b")[::-1], 2)
    X2 = np.abs(np.fft.fft(x)) ** 2
    bins = {rev(k): X2[k] / X2.sum() for k0, _ in tones for k in (k0, N - k0)}
    assert len(bins) == 6
    assert set(np.unique(idx).tolist()) <= set(bins)
    ns = len(idx)
    for b, share in bins.items():
        cnt = int((idx == b).sum())
        assert abs(cnt - ns * share) <= 6 * np.sqrt(ns * share * (1 - share)) + 1, (b, cnt, ns * share)
    # the returned probabilities are the bins' shares
    for b, share in bins.items():
        if (idx == b).any():
            assert abs(p[idx == b][0] - share) < 1e-6 * share


# ---------------------------------------------------------------- 5. statistics
def test_site_and_pair_frequencies_at_n12(qil):
    n = 12
    rng = np.random.default_rng(12)
    data = random_mps_data(saturated_profile(n, 8), rng, np.complex128)
    psi = qil.SignalMPS(data)
    b, _ = qil.sample(psi, 2 ** 18, seed=2024, bits=True)
    P = np.abs(dense_mps(data)) ** 2
    P /= P.sum()
    ns = b.shape[0]
    for i in range(n):
        p1 = P.sum(axis=tuple(j for j in range(n) if j != i))[1]
        f = b[:, i].mean()
        assert abs(f - p1) <= 6 * np.sqrt(p1 * (1 - p1) / ns) + 1e-12, (i, f, p1)
    for i in range(n - 1):
        pp = P.sum(axis=tuple(j for j in range(n) if j not in (i, i + 1)))
        for s in range(2):
            for t in range(2):
                f = ((b[:, i] == s) & (b[:, i + 1] == t)).mean()
                assert abs(f - pp[s, t]) <= 6 * np.sqrt(pp[s, t] * (1 - pp[s, t]) / ns) + 1e-12, (i, s, t, f, pp[s, t])


# ---------------------------------------------------------------- 6. full size
def test_full_size_probabilities_match_coefficients(qil):
    L = 48
    psi = qil.ZTMPS.alloc(saturated_profile(L, 64), dtype=np.complex128, amplitude=2.5).fill_random(20241016)
    b, p = qil.sample(psi, 4096, seed=11, bits=True)
    c = qil.coefficient_batch(psi, b)
    ref = np.abs(c) ** 2 / (psi.amplitude ** 2 * qil.norm(psi) ** 2)
    assert np.all(ref > 0)
    rel = np.abs(p - ref) / ref
    assert rel.max() < 1e-10, rel.max()


# ---------------------------------------------------------------- 7. errors, allocation failures
def test_errors(qil):
    rng = np.random.default_rng(3)
    data = random_mps_data(saturated_profile(8, 8), rng)
    zero = [a.copy() for a in data]
    zero[4][:] = 0
    with pytest.raises(qil.QilDomainError, match="zero norm"):
        qil.sample(qil.SignalMPS(zero), 16, seed=1)
    psi = qil.SignalMPS(data)
    U = rng.random((16, 8))
    for bad in (1.0, -1e-300, np.nan, np.inf):
        V = U.copy()
        V[7, 3] = bad
        with pytest.raises(ValueError, match="outside"):
            qil.sample(psi, 16, uniforms=V)
    with pytest.raises(ValueError, match="shape"):
        qil.sample(psi, 16, uniforms=U[:, :7])
    b, p = qil.sample(psi, 0, bits=True)
    assert b.shape == (0, 8) and p.shape == (0,)


@pytest.mark.parametrize("route", ["fused", "gemm"])
def test_failed_sample_calls_leave_no_device_memory_behind(qil, route, monkeypatch):
    monkeypatch.setenv("QIL_SAMPLE_ROUTE", route)
    ctx = qil.default_context()
    rng = np.random.default_rng(21)
    data = random_mps_data(saturated_profile(10, 16), rng, np.complex128)
    psi = qil.SignalMPS(data)
    U = rng.random((100, 10))
    ref = qil.sample(psi, 100, uniforms=U, bits=True)
    failures = 0
    for k in range(0, 64):
        ctx.fail_alloc_after(k)
        try:
            got = qil.sample(psi, 100, uniforms=U, bits=True)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        if not failed:
            break
        failures += 1
        assert ctx.unowned_bytes() == 0, k
    assert failures >= 5, failures
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert all(np.array_equal(psi.site(i), data[i]) for i in range(10))
