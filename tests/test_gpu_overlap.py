"""GPU tests of the overlaps: inner(phi, psi), inner(phi, W, psi) = <phi|W psi>, apply_norm(W, psi) = norm(W psi) and the
distances built on them, against dense references (helpers.dense_mps / apply_dense, np.vdot) and against the same numbers
computed on the materialised product W * psi.

Tolerances (fp64): dense parity and identities 1e-12 relative (exact contractions, different summation order); the two
routes of inner 1e-13; distances through the expansion |phi|^2 + |psi|^2 - 2 Re<phi|psi>, whose squared value carries an
absolute error of a few eps * (|phi|^2 + |psi|^2) (the floor the docstring of `distance` states)."""
import numpy as np
import pytest

import oracle as O
from helpers import random_mps_data, random_mpo_data, saturated_profile, dense_mps, apply_dense

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


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


def rel(a, b):
    return abs(a - b) / max(1e-300, abs(b))


def near(a, b, scale, tol):
    """|a - b| <= tol * max(|b|, scale): an inner product is conditioned by the norms of its operands (scale), not by its
    own size -- two random states of many sites are nearly orthogonal"""
    return abs(a - b) <= tol * max(abs(b), scale)


def _mps(qil, data, amp, paired):
    return (qil.ZTMPS if paired else qil.SignalMPS)(data, amplitude=amp)


def _mpo(qil, data, paired):
    return (qil.PairedSiteMPO if paired else qil.SingleSiteMPO)(data)


def _vec(data, amp=1.0):
    return amp * dense_mps(data).reshape(-1)


def _floor(*norms2):
    """absolute error of a squared distance from the expansion: a few eps times the squared norms involved"""
    return 64 * EPS * sum(norms2)


# ---------------------------------------------------------------- 1. dense parity
DTYPES = [(p, w, s) for p in (np.float64, np.complex128) for w in (np.float64, np.complex128) for s in (np.float64, np.complex128)]


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("pdt,wdt,sdt", DTYPES)
def test_dense_parity_all_dtypes(qil, pdt, wdt, sdt, paired, monkeypatch):
    rng = np.random.default_rng(7 + 3 * paired + 11 * DTYPES.index((pdt, wdt, sdt)))
    L = 8
    p = random_mps_data([2, 4, 8, 16, 33, 37, 4], rng, pdt)
    s = random_mps_data(saturated_profile(L, 16), rng, sdt)
    w = random_mpo_data([3, 5, 12, 7, 9, 4, 2], rng, wdt)
    phi, psi, W = _mps(qil, p, 1.7, paired), _mps(qil, s, -0.6, paired), _mpo(qil, w, paired)
    vphi, vpsi, vw = _vec(p, 1.7), _vec(s, -0.6), apply_dense(w, s)
    all_real = all(d == np.float64 for d in (pdt, wdt, sdt))
    for route in ("chain", "gemm"):
        monkeypatch.setenv("QIL_INNER_ROUTE", route)
        got = qil.inner(phi, psi)
        ref = np.vdot(vphi, vpsi)
        assert near(got, ref, np.linalg.norm(vphi) * np.linalg.norm(vpsi), 1e-12), (route, got, ref)
        assert isinstance(got, float if (pdt == np.float64 and sdt == np.float64) else complex)
    got = qil.inner(phi, W, psi)
    ref = np.vdot(vphi, -0.6 * vw)
    assert near(got, ref, np.linalg.norm(vphi) * np.linalg.norm(0.6 * vw), 1e-12), (got, ref)
    assert isinstance(got, float if all_real else complex)
    nrm = qil.apply_norm(W, psi)
    assert isinstance(nrm, float) and rel(nrm, np.linalg.norm(vw)) < 1e-12


def test_dense_parity_longer_odd_chain(qil):
    rng = np.random.default_rng(10)
    L = 10
    p = random_mps_data([2, 3, 5, 9, 17, 31, 13, 7, 2], rng, np.complex128)
    s = random_mps_data([2, 4, 8, 16, 32, 16, 8, 4, 2], rng, np.float64)
    w = random_mpo_data([4, 7, 5, 11, 6, 9, 3, 5, 2], rng, np.complex128)
    phi, psi, W = qil.SignalMPS(p, amplitude=0.3), qil.SignalMPS(s, amplitude=2.0), qil.SingleSiteMPO(w)
    vw = apply_dense(w, s)
    vp, vs = _vec(p, 0.3), _vec(s, 2.0)
    assert near(qil.inner(phi, psi), np.vdot(vp, vs), np.linalg.norm(vp) * np.linalg.norm(vs), 1e-12)
    assert near(qil.inner(phi, W, psi), np.vdot(vp, 2.0 * vw), np.linalg.norm(vp) * np.linalg.norm(2.0 * vw), 1e-12)
    assert rel(qil.apply_norm(W, psi), np.linalg.norm(vw)) < 1e-12


# ---------------------------------------------------------------- 2. identities
PROFILES = {
    "63": [2, 4, 8, 16, 32, 63, 63, 32, 16, 8, 4, 2],
    "64": [2, 4, 8, 16, 32, 64, 64, 32, 16, 8, 4, 2],
    "65": [2, 4, 8, 16, 32, 64, 65, 32, 16, 8, 4, 2],
    "129": [2, 4, 8, 16, 32, 64, 129, 64, 32, 16, 8, 4],
}


@pytest.mark.parametrize("key", sorted(PROFILES))
@pytest.mark.parametrize("D", [33, 40])
def test_identities_across_the_crossover_and_tile_edges(qil, key, D):
    rng = np.random.default_rng(int(key) * 100 + D)
    bonds = PROFILES[key]
    L = len(bonds) + 1
    psi = qil.SignalMPS(random_mps_data(bonds, rng, np.complex128), amplitude=1.3)
    phi = qil.SignalMPS(random_mps_data(list(reversed(bonds)), rng, np.float64), amplitude=0.8)
    W = qil.SingleSiteMPO(random_mpo_data([min(D, 4 ** (i + 1), 4 ** (L - 1 - i)) for i in range(L - 1)], rng))
    a = psi.amplitude * qil.norm(psi)
    assert rel(qil.inner(psi, psi).real, a * a) < 1e-13 and abs(qil.inner(psi, psi).imag) < 1e-13 * a * a
    b = phi.amplitude * qil.norm(phi)
    x, y = qil.inner(phi, psi), qil.inner(psi, phi)
    assert near(x, np.conj(y), a * b, 1e-13)
    prod = W * psi
    nw = qil.apply_norm(W, psi)
    assert rel(nw, qil.norm(prod)) < 1e-12
    assert near(qil.inner(phi, W, psi), qil.inner(phi, prod), b * psi.amplitude * nw, 1e-12)
    del prod


# ---------------------------------------------------------------- 3. route agreement
@pytest.mark.parametrize("chi", [1, 7, 32, 63, 64])
@pytest.mark.parametrize("dts", [(np.float64, np.float64), (np.complex128, np.float64), (np.float64, np.complex128),
                                 (np.complex128, np.complex128)])
def test_chain_and_gemm_routes_agree(qil, chi, dts, monkeypatch):
    rng = np.random.default_rng(chi)
    L = 40
    phi = qil.SignalMPS(random_mps_data(saturated_profile(L, chi), rng, dts[0]), amplitude=1.1)
    psi = qil.SignalMPS(random_mps_data(saturated_profile(L, max(1, chi - 3)), rng, dts[1]), amplitude=0.9)
    vals = {}
    for route in ("chain", "gemm"):
        monkeypatch.setenv("QIL_INNER_ROUTE", route)
        vals[route] = qil.inner(phi, psi)
    assert abs(vals["chain"] - vals["gemm"]) <= 1e-13 * max(abs(vals["gemm"]), 1.1 * 0.9), vals


# ---------------------------------------------------------------- 4. errors
def test_operand_mismatches_raise_like_apply(qil):
    rng = np.random.default_rng(4)
    a8 = random_mps_data(saturated_profile(8, 8), rng)
    a7 = random_mps_data(saturated_profile(7, 8), rng)
    w8 = random_mpo_data(saturated_profile(8, 4), rng)
    psi, W = qil.SignalMPS(a8), qil.SingleSiteMPO(w8)
    with pytest.raises(ValueError, match="same number of sites"):
        qil.inner(qil.SignalMPS(a7), psi)
    with pytest.raises(ValueError, match="same number of sites"):
        qil.inner(qil.SignalMPS(a7), W, psi)
    with pytest.raises(ValueError, match="same number of sites"):
        qil.inner(psi, W, qil.SignalMPS(a7))
    with pytest.raises(ValueError, match="same number of sites"):
        qil.apply_norm(W, qil.SignalMPS(a7))
    other = qil.SignalMPS(a8, sites=list(range(11, 19)))
    with pytest.raises(ValueError, match="same site indices"):
        qil.inner(other, psi)
    with pytest.raises(ValueError, match="same site indices"):
        qil.inner(other, W, psi)
    with pytest.raises(ValueError, match="same site indices"):
        qil.apply_norm(qil.SingleSiteMPO(w8, sites=list(range(11, 19))), psi)
    zt = qil.ZTMPS(a8)                                      # 8 tensors, paired flag set
    with pytest.raises(ValueError, match="cannot mix paired"):
        qil.inner(zt, psi)
    with pytest.raises(ValueError, match="cannot mix paired"):
        qil.inner(zt, W, psi)
    ctx2 = qil.Context(0)
    try:
        far = qil.SignalMPS(a8, ctx=ctx2)
        with pytest.raises(ValueError, match="different contexts"):
            qil.inner(far, psi)
        with pytest.raises(ValueError, match="different contexts"):
            qil.inner(far, W, psi)
        with pytest.raises(ValueError, match="different contexts"):
            qil.apply_norm(W, far)
        del far
    finally:
        ctx2.close()


def test_failed_overlap_calls_leave_no_device_memory_behind(qil, monkeypatch):
    ctx = qil.default_context()
    rng = np.random.default_rng(12)
    L = 8
    a = random_mps_data(saturated_profile(L, 16), rng)
    p = random_mps_data(saturated_profile(L, 12), rng, np.complex128)
    w = random_mpo_data(saturated_profile(L, 12, base=4), rng, np.float64)
    psi, phi, W = qil.SignalMPS(a), qil.SignalMPS(p, amplitude=0.5), qil.SingleSiteMPO(w)
    ref = {"apply_inner": qil.inner(phi, W, psi), "apply_norm": qil.apply_norm(W, psi)}
    monkeypatch.setenv("QIL_INNER_ROUTE", "gemm")
    ref["inner (GEMM route)"] = qil.inner(phi, psi)
    calls = {"apply_inner": lambda: qil.inner(phi, W, psi), "apply_norm": lambda: qil.apply_norm(W, psi),
             "inner (GEMM route)": lambda: qil.inner(phi, psi)}
    before = [x.site(i).copy() for x in (psi, phi, W) for i in range(L)]
    for name, fn in calls.items():
        failures = 0
        for k in list(range(0, 12)) + [20, 40]:
            ctx.fail_alloc_after(k)
            try:
                fn()
                failed = False
            except MemoryError:
                failed = True
            finally:
                ctx.fail_alloc_after(None)
            if not failed:
                break
            failures += 1
            assert ctx.unowned_bytes() == 0, (name, k)
        assert failures >= 1, name
        assert fn() == ref[name], name
        assert ctx.unowned_bytes() == 0, name
    after = [x.site(i) for x in (psi, phi, W) for i in range(L)]
    assert all(np.array_equal(u, v) for u, v in zip(before, after))


# ---------------------------------------------------------------- 5. truncation error, end to end
def test_apply_distance_of_a_truncated_product(qil):
    n = 8
    t = np.arange(2 ** n) / 2 ** n
    x = np.sin(2 * np.pi * 5 * t) * np.exp(-3 * t) + 0.5 * np.cos(2 * np.pi * 11 * t) + 0.2 * t * t
    psi = qil.signal_ztmps(x, cutoff=1e-14)
    W = qil.build_zt_mpo(n, 2 * np.pi)
    exact = helpers_apply(W, psi)
    nw2 = float(np.vdot(exact, exact).real)
    checked = []
    for m in range(1, 33):
        phi = qil.apply_compress(W, psi, maxdim=m, tol=1e-16)
        vphi = _vec(phi.to_host(), phi.amplitude)
        d_ref = np.linalg.norm(vphi - exact)
        r = d_ref / np.sqrt(nw2)
        if r < 1e-5:
            break
        if r > 0.1:
            continue
        got = qil.apply_distance(phi, W, psi)
        nphi2 = float(np.vdot(vphi, vphi).real)
        tol = 1e-7 * d_ref + _floor(nphi2, nw2) / d_ref
        assert abs(got - d_ref) <= tol, (m, r, got, d_ref)
        if 1e-4 <= r <= 1e-2:
            assert rel(got, d_ref) < 1e-7, (m, r, got, d_ref)
        checked.append(r)
    assert any(1e-4 <= r <= 1e-2 for r in checked), checked


def helpers_apply(W, psi):
    """dense vec(W psi) from the downloaded sites: the oracle's site-wise apply, then helpers.dense_mps"""
    out = O.apply(O.SingleSiteMPO(W.to_host()), O.SignalMPS(psi.to_host(), amplitude=psi.amplitude))
    return _vec(out.data, out.amplitude)


def test_distance_between_two_encodings(qil):
    n = 12
    rng = np.random.default_rng(12)
    t = np.arange(2 ** n) / 2 ** n
    x = np.exp(-4 * t) * np.sin(2 * np.pi * 9 * t) + 0.05 * rng.standard_normal(2 ** n)
    a = qil.signal_mps(x, method="svd", cutoff=1e-15)
    b = qil.signal_mps(x, method="rsvd", k=6, p=4, q=1, maxdim=6)
    va, vb = _vec(a.to_host(), a.amplitude), _vec(b.to_host(), b.amplitude)
    d_ref = np.linalg.norm(va - vb)
    got = qil.distance(a, b)
    na2, nb2 = float(np.vdot(va, va).real), float(np.vdot(vb, vb).real)
    assert d_ref > 1e-4 * np.sqrt(na2)
    assert abs(got - d_ref) <= 1e-7 * d_ref + _floor(na2, nb2) / d_ref, (got, d_ref)
    assert qil.distance(a, a) <= np.sqrt(_floor(na2, na2))


# ---------------------------------------------------------------- 6. full size, Parseval
def test_config2_parseval_through_apply_norm(qil):
    n = 20
    rng = np.random.default_rng(20240032)
    psi = qil.SignalMPS(random_mps_data(saturated_profile(n, 32), rng))
    W = qil.build_qft_mpo(n)
    got = qil.apply_norm(W, psi)
    assert rel(got, qil.norm(psi)) < 1e-6
    prod = W * psi
    assert rel(got, qil.norm(prod)) < 1e-12
    del prod


# ---------------------------------------------------------------- 7. full size, cfg3 shapes
def test_config3_lazy_overlaps_at_full_size(qil):
    """n = 24 paired (48 tensors), chi_s = 64, D = 128: <phi|W psi> lazily against the 80 GB materialised product, pool use
    of both lazy calls, and the consistency of norm(W psi) with <phi|W psi> for an SVD-truncated phi."""
    ctx = qil.default_context()
    L = 48
    cb, db = saturated_profile(L, 64), saturated_profile(L, 128, base=4)
    psi = qil.ZTMPS.alloc(cb, dtype=np.float64, amplitude=1.5).fill_random(20240064)
    W = qil.PairedSiteMPO.alloc(db, dtype=np.complex128).fill_random(777)
    phi = qil.apply_compress(W, psi, maxdim=64)
    assert max(phi.bond_dims) <= 64

    def pool():
        m = ctx.mem_info()
        return m["pool_in_use"] + m["pool_cached"]

    ctx.synchronize()
    ctx.trim()
    base = pool()
    lazy = qil.inner(phi, W, psi)
    inner_bytes = pool() - base
    ctx.trim()
    base = pool()
    nw = qil.apply_norm(W, psi)
    norm_bytes = pool() - base
    ctx.trim()
    assert inner_bytes < 256 << 20, inner_bytes
    assert norm_bytes < 8 << 30, norm_bytes

    prod = W * psi
    mat = qil.inner(phi, prod)
    del prod
    ctx.trim()
    assert rel(lazy, mat) < 1e-10, (lazy, mat)

    nwpsi = psi.amplitude * nw
    nphi = phi.amplitude * qil.norm(phi)
    assert abs(lazy) <= nphi * nwpsi * (1 + 1e-12)
    d = qil.apply_distance(phi, W, psi)
    # phi = P(W psi) up to the truncation's own error: Re<phi|W psi> = |phi|^2, so d^2 = |W psi|^2 - |phi|^2
    floor = _floor(nphi ** 2, nwpsi ** 2)
    assert abs(lazy.real - nphi ** 2) <= 1e-2 * d * d + floor, (lazy, nphi ** 2, d)
    assert abs(d * d - (nwpsi ** 2 - nphi ** 2)) <= 2e-2 * d * d + 2 * floor, (d * d, nwpsi ** 2 - nphi ** 2)
