"""GPU tests of lazy perfect sampling of W psi (qil.apply_sample, qil_apply_sample), which never forms W psi.

The reference is numpy on the dense vector: P = abs(helpers.apply_dense(w, a))**2 reshaped to (2,)*n, and the sequential
sampler of test_gpu_sample.py on it (exact marginals, s = 0 iff u (q0 + q1) < q0), restated here.  A row whose oracle margin
min_i |u tot - q0| / tot is <= 1e-10 is exempt from bit identity, and at most 1 % of the rows may be.  Probabilities: 1e-10
relative to the dense ones, the project's mid-size read-out tolerance (test_gpu_sample.py, the full-size test); each parity
case prints the largest deviation it saw.

Shapes (chi bonds of psi / D bonds of W): the five profiles of test_gpu_apply_weight.py; `two`, the shortest chain with a bond;
`tile65`, whose widest bond chi D = 65 is one past the scoring kernel's 64-column panel and no multiple of its K step of 4.  700
rows, no multiple of the 32-row tile.  All have an even number of tensors, so each also runs paired.  Both routes
(QIL_APPLY_SAMPLE_ROUTE) run everywhere."""
import ctypes as C
import functools
import importlib
import importlib.util
import os

import numpy as np
import pytest

from helpers import random_mps_data, random_mpo_data, saturated_profile, apply_dense

pytestmark = pytest.mark.gpu

MARGIN = 1e-10
ROUTE = "QIL_APPLY_SAMPLE_ROUTE"
RENV = "QIL_APPLY_SAMPLE_RENV_BYTES"
ROUTES = ["fused", "gemm"]
NB = 700
F, Z = np.float64, np.complex128
DT_PAIRS = [(F, F), (F, Z), (Z, F), (Z, Z)]                                  # (psi, W)
DT_IDS = ["f64-f64", "f64-c64", "c64-f64", "c64-c64"]
PROFILES = {
    "bond1": ([1] * 7, [1] * 7),
    "odd": ([2, 3, 5, 7, 5, 3, 2], [3, 5, 2, 7, 3, 2, 5]),
    "sat": (saturated_profile(10, 8), saturated_profile(10, 6, 4)),
    "wideD": (saturated_profile(10, 4), saturated_profile(10, 16, 4)),
    "widechi": (saturated_profile(10, 24), saturated_profile(10, 4, 4)),
    "two": ([2], [3]),
    "tile65": ([2, 4, 5, 5, 5, 4, 2], [4, 13, 13, 13, 13, 13, 4]),
}
CASES = list(PROFILES)


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
    """u[r, i] = (splitmix64(seed ^ splitmix64(r n + i)) >> 11) 2^-53 (include/qilaplace_hip.h, qil_apply_sample)"""
    idx = (np.arange(nb, dtype=np.uint64)[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :])
    h = splitmix64(np.uint64(seed) ^ splitmix64(idx))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def oracle_sample(P, U):
    """(bits, probs, margin) of the sequential sampler on the dense weights P ((2,)*n) with the uniforms U (nb x n)"""
    n = P.ndim
    marg = [P.sum(axis=tuple(range(i + 1, n))).reshape(-1, 2) for i in range(n)]   # [prefix (MSB first), s]
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


def _amp(dt):
    return -1.3 if dt == Z else 1.7                                           # a parent amplitude != 1


@functools.lru_cache(maxsize=None)
def _case(case, dta, dtw):
    """host tensors, the dense weights, 700 uniform rows and the oracle's samples on them: computed once, shared, left unchanged"""
    rng = np.random.default_rng(17000 + 4 * CASES.index(case) + 2 * (dta == Z) + (dtw == Z))
    chi, D = PROFILES[case]
    a = random_mps_data(chi, rng, dta)
    w = random_mpo_data(D, rng, dtw)
    n = len(a)
    P = np.abs(apply_dense(w, a)).reshape((2,) * n) ** 2
    U = rng.random((NB, n))
    ob, op, margin = oracle_sample(P, U)
    for x in (P, U, ob, op, margin):
        x.setflags(write=False)
    return a, w, P, U, ob, op, margin


def _operands(qil, a, w, paired, amp):
    if paired:
        return qil.PairedSiteMPO(w), qil.ZTMPS(a, amplitude=amp)
    return qil.SingleSiteMPO(w), qil.SignalMPS(a, amplitude=amp)


def _check(bits, probs, ob, op, margin, tol=1e-10):
    ok = margin > MARGIN
    assert ok.mean() >= 0.99, ok.mean()
    np.testing.assert_array_equal(bits[ok], ob[ok])
    rel = np.abs(probs[ok] - op[ok]) / op[ok]
    assert rel.max() <= tol, rel.max()
    return rel.max()


def _chunk(chi, D, nb, itemsize):
    """the documented chunk size, restated"""
    c, d = [1] + list(chi) + [1], [1] + list(D) + [1]
    m = x = 1
    for i in range(len(c) - 1):
        m = max(m, c[i] * d[i], c[i + 1] * d[i + 1])
        x = max(x, 2 * c[i] * d[i + 1])
    return max(1, min(nb, 32768, (64 << 20) // ((5 * m + x) * itemsize + 16 * ((m + 63) // 64))))


# ---------------------------------------------------------------- 1. oracle parity with given uniforms
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
@pytest.mark.parametrize("case", CASES)
def test_oracle_parity_with_given_uniforms(qil, case, paired, dts, route, monkeypatch):
    a, w, P, U, ob, op, margin = _case(case, *dts)
    monkeypatch.setenv(ROUTE, route)
    W, psi = _operands(qil, a, w, paired, _amp(dts[0]))
    n = len(a)
    b, p = qil.apply_sample(W, psi, NB, uniforms=U, bits=True)
    assert b.shape == (NB, n) and b.dtype == np.uint8 and p.shape == (NB,) and p.dtype == np.float64
    worst = _check(b, p, ob, op, margin)
    print(f"apply_sample {case} paired={paired} {DT_IDS[DT_PAIRS.index(dts)]} {route}: worst relative probability error {worst:.2e}, "
          f"{int((margin <= MARGIN).sum())} rows exempt, smallest margin {margin.min():.1e}")
    for nb in (1, 33):
        b, p = qil.apply_sample(W, psi, nb, uniforms=U[:nb], bits=True)
        good = margin[:nb] > MARGIN
        np.testing.assert_array_equal(b[good], ob[:nb][good])
        assert b.shape == (nb, n) and np.all(np.abs(p - op[:nb])[good] <= 1e-10 * op[:nb][good])


def test_index_decoding(qil):
    a, w, P, U, ob, op, margin = _case("sat", F, Z)
    n = len(a)
    W, psi = _operands(qil, a, w, False, 1.0)
    idx, p = qil.apply_sample(W, psi, 256, uniforms=U[:256])
    b, p2 = qil.apply_sample(W, psi, 256, uniforms=U[:256], bits=True)
    assert np.array_equal(idx, b.astype(np.int64) @ (1 << np.arange(n - 1, -1, -1))) and np.array_equal(p, p2)
    Wp, zt = _operands(qil, a, w, True, 1.0)
    (k, l), pz = qil.apply_sample(Wp, zt, 256, uniforms=U[:256])
    assert np.array_equal(k, b[:, 0::2].astype(np.int64) @ (1 << np.arange(n // 2)))
    assert np.array_equal(l, b[:, 1::2].astype(np.int64) @ (1 << np.arange(n // 2)))
    assert np.array_equal(pz, p)


# ---------------------------------------------------------------- 2. seeded path
@pytest.mark.parametrize("route", ROUTES)
def test_seeded_path_is_the_documented_formula(qil, route, monkeypatch):
    monkeypatch.setenv(ROUTE, route)
    a, w, P, _, _, _, _ = _case("sat", Z, Z)
    n = len(a)
    W, psi = _operands(qil, a, w, False, _amp(Z))
    for seed in (0, 1234, 2 ** 64 - 1):
        U = seeded_uniforms(seed, 1000, n)
        assert U.min() >= 0 and U.max() < 1
        b1, p1 = qil.apply_sample(W, psi, 1000, seed=seed, bits=True)
        b2, p2 = qil.apply_sample(W, psi, 1000, uniforms=U, bits=True)
        assert np.array_equal(b1, b2) and np.array_equal(p1, p2)
    _check(b1, p1, *oracle_sample(P, U))


# ---------------------------------------------------------------- 3. invariance
def test_prefix_amplitude_and_route_invariance(qil, monkeypatch):
    a, w, P, _, _, _, _ = _case("sat", Z, Z)
    n = len(a)
    U = seeded_uniforms(77, 4096, n)
    ok = oracle_sample(P, U)[2] > MARGIN
    assert ok.mean() >= 0.99
    got = {}
    for route in ROUTES:
        monkeypatch.setenv(ROUTE, route)
        W, psi = _operands(qil, a, w, False, _amp(Z))
        b10, p10 = qil.apply_sample(W, psi, 10, seed=77, bits=True)
        b, p = qil.apply_sample(W, psi, 4096, seed=77, bits=True)
        assert np.array_equal(b10[ok[:10]], b[:10][ok[:10]])
        assert np.allclose(p10[ok[:10]], p[:10][ok[:10]], rtol=1e-12, atol=0)
        Wa, psia = _operands(qil, a, w, False, -3.5e7)
        ba, pa = qil.apply_sample(Wa, psia, 4096, seed=77, bits=True)
        assert np.array_equal(ba, b) and np.array_equal(pa, p)
        got[route] = (b, p)
    assert np.array_equal(got["fused"][0][ok], got["gemm"][0][ok])
    assert np.allclose(got["fused"][1][ok], got["gemm"][1][ok], rtol=1e-12, atol=0)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", ["odd", "bond1"])
def test_rows_across_chunk_boundaries(qil, case, route, monkeypatch):
    """nb = 32768 + 700 is past the row cap of a chunk: `bond1` runs in chunks of 32768 rows, `odd` (c64) in smaller ones that the
    64 MiB budget sets; either way rows 0 .. 699 are the rows of a 700-row call."""
    monkeypatch.setenv(ROUTE, route)
    a, w, P, _, _, _, _ = _case(case, Z, Z)
    n = len(a)
    nb = 32768 + NB
    chunk = _chunk(*PROFILES[case], nb, 16)
    assert chunk < nb and (case != "bond1" or chunk == 32768)
    ok = oracle_sample(P, seeded_uniforms(5, NB, n))[2] > MARGIN
    assert ok.mean() >= 0.99
    W, psi = _operands(qil, a, w, False, _amp(Z))
    b, p = qil.apply_sample(W, psi, nb, seed=5, bits=True)
    bs, ps = qil.apply_sample(W, psi, NB, seed=5, bits=True)
    assert np.array_equal(b[:NB][ok], bs[ok])
    assert np.allclose(p[:NB][ok], ps[ok], rtol=1e-12, atol=0)
    # the rows of the later chunks are the seeded rows of their own index
    tail = slice(nb - 64, nb)
    ob, op, margin = oracle_sample(P, seeded_uniforms(5, nb, n)[tail])
    good = margin > MARGIN
    assert np.array_equal(b[tail][good], ob[good]) and np.all(np.abs(p[tail] - op)[good] <= 1e-10 * op[good])


# ---------------------------------------------------------------- 4. against the materialised route
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
@pytest.mark.parametrize("case", ["sat", "tile65"])
def test_lazy_samples_are_the_samples_of_the_formed_product(qil, case, dts, route, monkeypatch):
    monkeypatch.setenv(ROUTE, route)
    a, w, P, U, ob, op, margin = _case(case, *dts)
    ok = margin > MARGIN
    W, psi = _operands(qil, a, w, False, _amp(dts[0]))
    b, p = qil.apply_sample(W, psi, NB, uniforms=U, bits=True)
    prod = qil.apply(W, psi)
    bf, pf = qil.sample(prod, NB, uniforms=U, bits=True)
    del prod
    assert np.array_equal(b[ok], bf[ok])
    assert np.all(np.abs(p - pf)[ok] <= 1e-10 * pf[ok])


# ---------------------------------------------------------------- 5. structure: the tones of a Fourier transform
def test_samples_land_on_the_tones_of_a_qft(qil):
    n = 16
    N = 2 ** n
    t = np.arange(N)
    tones = [(3, 1.0), (1000, 0.6), (7777, 0.3)]
    x = sum(amp * np.cos(2 * np.pi * k * t / N) for k, amp in tones)
    psi = qil.signal_mps(x, cutoff=1e-15)
    W = qil.build_qft_mpo(psi)
    idx, p = qil.apply_sample(W, psi, 2 ** 13, seed=4)
    # coefficient(W psi, lsb bits of k) = fft(x)[k] / sqrt(N): a big-endian sample index is k bit-reversed
    rev = lambda k: int(format(k, f"0{n}b")[::-1], 2)
    X2 = np.abs(np.fft.fft(x)) ** 2
    bins = {rev(k): X2[k] / X2.sum() for k0, _ in tones for k in (k0, N - k0)}
    assert len(bins) == 6
    assert set(np.unique(idx).tolist()) <= set(bins)
    ns = len(idx)
    for b, share in bins.items():
        cnt = int((idx == b).sum())
        assert abs(cnt - ns * share) <= 6 * np.sqrt(ns * share * (1 - share)) + 1, (b, cnt, ns * share)
    for b, share in bins.items():
        if (idx == b).any():
            assert abs(p[idx == b][0] - share) < 1e-6 * share


# ---------------------------------------------------------------- 6. statistics
def test_site_and_pair_frequencies(qil):
    a, w, P, _, _, _, _ = _case("sat", Z, Z)
    n = len(a)
    W, psi = _operands(qil, a, w, False, _amp(Z))
    b, _ = qil.apply_sample(W, psi, 2 ** 16, seed=2024, bits=True)
    Pn = P / P.sum()
    ns = b.shape[0]
    for i in range(n):
        p1 = Pn.sum(axis=tuple(j for j in range(n) if j != i))[1]
        f = b[:, i].mean()
        assert abs(f - p1) <= 6 * np.sqrt(p1 * (1 - p1) / ns), (i, f, p1)
    for i in range(n - 1):
        pp = Pn.sum(axis=tuple(j for j in range(n) if j not in (i, i + 1)))
        for s in range(2):
            for t in range(2):
                f = ((b[:, i] == s) & (b[:, i + 1] == t)).mean()
                assert abs(f - pp[s, t]) <= 6 * np.sqrt(pp[s, t] * (1 - pp[s, t]) / ns), (i, s, t, f, pp[s, t])


# ---------------------------------------------------------------- 7. mid size, no dense vector
@pytest.mark.parametrize("route", ROUTES)
def test_mid_size_probabilities_match_the_lazy_coefficients(qil, route, monkeypatch):
    """24 paired tensors, chi <= 16, D <= 16: a product bond of 256, 24 MiB of environments."""
    monkeypatch.setenv(ROUTE, route)
    psi = qil.ZTMPS.alloc(saturated_profile(24, 16), dtype=Z, amplitude=2.5).fill_random(20241020)
    W = qil.PairedSiteMPO.alloc(saturated_profile(24, 16, 4), dtype=Z).fill_random(20241021)
    b, p = qil.apply_sample(W, psi, 4096, seed=11, bits=True)
    c = qil.apply_coefficient_batch(W, psi, b)
    ref = np.abs(c) ** 2 / (psi.amplitude ** 2 * qil.apply_norm(W, psi) ** 2)
    assert np.all(ref > 0)
    rel = np.abs(p - ref) / ref
    print(f"mid-size apply_sample {route}: worst relative probability error {rel.max():.2e}")
    assert rel.max() <= 1e-10, rel.max()


# ---------------------------------------------------------------- 8. errors
def test_errors_and_edge_cases(qil, monkeypatch):
    L = importlib.import_module("qilaplace_jl_amd._lib")
    a, w, P, U, _, _, _ = _case("sat", F, Z)
    n = len(a)
    ctx = qil.default_context()
    for k in (0, 4, n - 1):
        zero = [t.copy() for t in w]
        zero[k][:] = 0
        with pytest.raises(qil.QilDomainError, match="zero norm"):
            qil.apply_sample(qil.SingleSiteMPO(zero), qil.SignalMPS(a), 16, seed=1)
    W, psi = qil.SingleSiteMPO(w), qil.SignalMPS(a)
    chi, D = PROFILES["sat"]
    need = 16 * sum((c * d) ** 2 for c, d in zip(chi, D))
    monkeypatch.setenv(RENV, "1024")
    ctx.fail_alloc_after(0)                              # an allocation in front of the cap would fail with the pool's message
    try:
        with pytest.raises(MemoryError, match=str(need)):
            qil.apply_sample(W, psi, 16, seed=1)
    finally:
        ctx.fail_alloc_after(None)
    assert ctx.unowned_bytes() == 0
    monkeypatch.setenv(RENV, str(need))                  # exactly what is needed passes
    assert qil.apply_sample(W, psi, 16, seed=1, bits=True)[0].shape == (16, n)
    monkeypatch.delenv(RENV)
    for bad in (1.0, -1e-300, np.nan, np.inf):
        V = U[:16].copy()
        V[7, 3] = bad
        with pytest.raises(ValueError, match="outside"):
            qil.apply_sample(W, psi, 16, uniforms=V)
        # the library's own check, behind the front-end's
        out = np.full((16, n), 9, dtype=np.uint8)
        assert L.lib.qil_apply_sample(W.handle, psi.handle, 16, 0, V.ctypes.data_as(C.POINTER(C.c_double)),
                                      out.ctypes.data_as(C.POINTER(C.c_uint8)), None) == L.QIL_EINVAL_CONFIG
        assert "outside [0, 1)" in L.last_error() and np.all(out == 9)
    with pytest.raises(ValueError, match="shape"):
        qil.apply_sample(W, psi, 16, uniforms=U[:16, :n - 1])
    with pytest.raises(ValueError, match="shape"):
        qil.apply_sample(W, psi, 15, uniforms=U[:16])
    with pytest.raises(ValueError, match="non-negative"):
        qil.apply_sample(W, psi, -1)
    assert L.lib.qil_apply_sample(W.handle, psi.handle, -1, 0, None, None, None) == L.QIL_EINVAL_ARG
    assert L.lib.qil_apply_sample(W.handle, psi.handle, 0, 0, None, None, None) == L.QIL_OK
    b, p = qil.apply_sample(W, psi, 0, bits=True)
    assert b.shape == (0, n) and b.dtype == np.uint8 and p.shape == (0,)
    idx, p = qil.apply_sample(W, psi, 0)
    assert idx.shape == (0,) and p.shape == (0,)
    # the operand errors of apply
    rng = np.random.default_rng(71)
    a8, a7 = random_mps_data([2] * 7, rng), random_mps_data([2] * 6, rng)
    w8 = random_mpo_data([2] * 7, rng)
    with pytest.raises(ValueError, match="same number of sites"):
        qil.apply_sample(qil.SingleSiteMPO(w8), qil.SignalMPS(a7), 4)
    with pytest.raises(ValueError, match="same site indices"):
        qil.apply_sample(qil.SingleSiteMPO(w8, sites=list(range(11, 19))), qil.SignalMPS(a8), 4)
    with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
        qil.apply_sample(qil.PairedSiteMPO(w8), qil.SignalMPS(a8), 4)


def test_single_site_chain(qil):
    A = np.array([0.25, -1.5]).reshape(1, 2, 1)
    M = np.array([[0.5, -2.0], [1.0, 0.25]])                                  # M[s_in, s_out]
    W, psi = qil.SingleSiteMPO([M.reshape(1, 2, 2, 1)]), qil.SignalMPS([A], amplitude=3.0)
    y = np.array([0.25 * 0.5 - 1.5 * 1.0, 0.25 * -2.0 - 1.5 * 0.25]) ** 2     # |(W psi)[s_out]|^2 by hand
    u = np.array([[0.1], [0.9], [y[0] / y.sum() - 1e-6], [y[0] / y.sum() + 1e-6]])
    b, p = qil.apply_sample(W, psi, 4, uniforms=u, bits=True)
    want = (u[:, 0] * y.sum() >= y[0]).astype(np.uint8)
    assert np.array_equal(b[:, 0], want) and np.allclose(p, y[want] / y.sum(), rtol=1e-14, atol=0)


# ---------------------------------------------------------------- 9. allocation failures
@pytest.mark.parametrize("route", ROUTES)
def test_failed_calls_leave_no_device_memory_behind(qil, route, monkeypatch):
    monkeypatch.setenv(ROUTE, route)
    a, w, P, U, _, _, _ = _case("odd", F, Z)
    ctx = qil.default_context()
    W, psi = _operands(qil, a, w, False, _amp(F))
    ref = qil.apply_sample(W, psi, 100, uniforms=U[:100], bits=True)
    failures, got = 0, None
    for k in range(0, 400):
        ctx.fail_alloc_after(k)
        try:
            got = qil.apply_sample(W, psi, 100, uniforms=U[:100], bits=True)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, k
        if not failed:
            break
        failures += 1
    assert got is not None and failures >= 5, failures
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert all(np.array_equal(psi.site(i), a[i]) for i in range(len(a)))
    assert all(np.array_equal(W.site(i), w[i]) for i in range(len(w)))


# ---------------------------------------------------------------- 10. the example
def test_lazy_sample_example_checks_itself(qil, capsys):
    """examples/lazy_sample.py asserts what it prints against the materialised product; run in this process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lazy_sample", os.path.join(root, "examples", "lazy_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tones, cells = mod.main()
    assert tones == [250, 1250, 3000] and len(cells) == 4
    assert "distinct bins hit" in capsys.readouterr().out
