"""GPU tests of the element-wise products and adjoints (qil.hadamard, diagonal_mpo, adjoint, hadamard_compress) and of
convolve / correlate / power_spectrum on top of them.

Tolerances: 1e-14 of a tensor's largest entry for site tensors (what test_gpu_parity.py holds `apply` to), 1e-12 of the
largest entry for dense read-outs (the project's read-out tolerance), 1e-10 relative at full size (as the top-k tests).  The
inverse-QFT checks measure their tolerance: the QFT MPO at cutoff 1e-14 is unitary only to 3e-9 ... 3e-7, so the round trip is
compared with the SAME pipeline in numpy on the SAME tensors (1e-12), and against np.fft with that pipeline's own deviation."""
import numpy as np
import pytest

import oracle as O
from helpers import random_mps_data, random_mpo_data, saturated_profile, dense_mps, dense_mpo

pytestmark = pytest.mark.gpu


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


def _site_product(p, a):
    """C[(a, alpha), s, (b, beta)] = p[a, s, b] a[alpha, s, beta]"""
    Dl, _, Dr = p.shape
    cl, _, cr = a.shape
    return np.einsum("asb,xsy->axsby", p, a).reshape(Dl * cl, 2, Dr * cr)


def _scale(t):
    return max(np.abs(t).max(), 1e-300)


# ---------------------------------------------------------------- 1. product against numpy
CASES = {
    "n1": [],
    "bond1": [1] * 7,
    "odd": [2, 3, 5, 7, 5, 3, 2],
    "sat8": saturated_profile(12, 8),
    "sat64": saturated_profile(14, 64),
}
KINDS = [(c, p) for c in sorted(CASES) for p in (False, True) if not (p and c == "n1")]
DTYPES = [(np.float64, np.float64), (np.float64, np.complex128), (np.complex128, np.float64), (np.complex128, np.complex128)]


def _check_product(qil, pd, ad, paired, conj, amp_phi, amp_psi):
    phi, psi = _mps(qil, pd, paired, amp_phi), _mps(qil, ad, paired, amp_psi)
    out = qil.hadamard(phi, psi, conj=conj)
    assert type(out) is type(psi) and out.site_ids == psi.site_ids and out.paired == psi.paired
    want_dt = np.complex128 if np.complex128 in (pd[0].dtype, ad[0].dtype) else np.float64
    assert out.dtype == want_dt
    assert out.amplitude == amp_phi * amp_psi
    assert out.bond_dims == [p * a for p, a in zip(phi.bond_dims, psi.bond_dims)]
    worst = 0.0
    for i in range(len(pd)):
        ref = _site_product(pd[i].conj() if conj else pd[i], ad[i])
        got = out.site(i)
        assert got.shape == ref.shape
        worst = max(worst, np.abs(got - ref).max() / _scale(ref))
    assert worst <= 1e-14, worst
    if len(pd) <= 14:
        dv = (amp_phi * dense_mps(pd).reshape(-1)) * (amp_psi * dense_mps(ad).reshape(-1))
        if conj:
            dv = (amp_phi * dense_mps(pd).reshape(-1)).conj() * (amp_psi * dense_mps(ad).reshape(-1))
        got = qil.mps_to_vector(out)
        assert np.abs(got - dv).max() <= 1e-12 * _scale(dv), np.abs(got - dv).max() / _scale(dv)
    return out


@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("pdt,adt", DTYPES)
@pytest.mark.parametrize("case,paired", KINDS)
def test_product_matches_numpy(qil, case, paired, pdt, adt, conj):
    rng = np.random.default_rng(sorted(CASES).index(case) * 16 + 8 * paired + 4 * conj + 2 * (pdt == np.complex128)
                                + (adt == np.complex128))
    pb = CASES[case]
    ab = saturated_profile(len(pb) + 1, 7) if pb else []
    pd, ad = random_mps_data(pb, rng, pdt), random_mps_data(ab, rng, adt)
    amp_phi, amp_psi = (-0.37, 1.9) if conj else (2.5, -0.8)
    _check_product(qil, pd, ad, paired, conj, amp_phi, amp_psi)


@pytest.mark.parametrize("pb,ab", [([2, 4, 8, 200, 8, 4, 2], [1] * 7),                       # phi's slab does not fit the LDS tile
                                   (saturated_profile(10, 40), saturated_profile(10, 32)),   # several row tiles per site
                                   ([1] * 9, saturated_profile(10, 32)),
                                   ([3, 9, 27, 9, 3], [3, 5, 15, 5, 3])])                     # odd row counts everywhere
@pytest.mark.parametrize("pdt,adt", [(np.float64, np.float64), (np.complex128, np.complex128)])
def test_product_tiling_edges(qil, pb, ab, pdt, adt):
    rng = np.random.default_rng(len(pb) * 100 + pb[2] + (pdt == np.complex128))
    pd, ad = random_mps_data(pb, rng, pdt), random_mps_data(ab, rng, adt)
    _check_product(qil, pd, ad, False, pdt == np.complex128, 1.0, -1.5)


# ---------------------------------------------------------------- 2. the two routes agree
@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("pdt,adt", DTYPES)
def test_hadamard_equals_apply_of_the_diagonal_operator(qil, pdt, adt, conj):
    """hadamard(phi, psi) against apply(diagonal_mpo(phi), psi): the kernel drops the structural zeros of diag(phi) from the
    apply's 2-term FMA chain, fma(0, x, w a) = w a, so the tensors are EQUAL for every dtype pair when amp_phi = 1 (the
    diagonal operator folds phi's amplitude into its first tensor; with amp_phi != 1 the first tensors differ by that factor
    and its rounding: 1e-14 of scale)."""
    rng = np.random.default_rng(40 + 2 * (pdt == np.complex128) + (adt == np.complex128) + 4 * conj)
    pd = random_mps_data(saturated_profile(10, 12), rng, pdt)
    ad = random_mps_data([2, 3, 5, 7, 9, 7, 5, 3, 2], rng, adt)
    for amp in (1.0, -0.6):
        phi, psi = qil.SignalMPS(pd, amplitude=amp), qil.SignalMPS(ad, amplitude=1.3)
        D = qil.diagonal_mpo(phi, conj=conj)
        assert type(D) is qil.SingleSiteMPO and D.bond_dims == phi.bond_dims and D.site_ids == phi.site_ids
        assert D.dtype == phi.dtype
        a, b = qil.hadamard(phi, psi, conj=conj), qil.apply(D, psi)
        assert a.bond_dims == b.bond_dims and a.dtype == b.dtype
        assert a.amplitude == amp * 1.3 and b.amplitude == 1.3
        for i in range(10):
            ta, tb = a.site(i), b.site(i)
            if amp == 1.0 or i > 0:
                assert np.array_equal(ta, tb), i
            else:
                assert np.abs(amp * ta - tb).max() <= 1e-14 * _scale(tb)
        # diag(phi) as a dense operator: diag(amp dense(phi)), exact zeros elsewhere
        M = dense_mpo(D.to_host())
        dv = amp * dense_mps(pd).reshape(-1)
        dv = dv.conj() if conj else dv
        assert np.count_nonzero(M - np.diag(np.diag(M))) == 0
        assert np.abs(np.diag(M) - dv).max() <= 1e-12 * _scale(dv)        # two numpy contraction orders: read-out tolerance
    Z = qil.diagonal_mpo(qil.ZTMPS(pd, amplitude=2.0))
    assert type(Z) is qil.PairedSiteMPO and Z.paired


# ---------------------------------------------------------------- 3. adjoint
@pytest.mark.parametrize("dt", [np.float64, np.complex128])
@pytest.mark.parametrize("paired", [False, True])
def test_adjoint_is_exact(qil, paired, dt):
    rng = np.random.default_rng(300 + 2 * paired + (dt == np.complex128))
    w = random_mpo_data(saturated_profile(8, 9, base=4), rng, dt)
    W = (qil.PairedSiteMPO if paired else qil.SingleSiteMPO)(w)
    Wd = qil.adjoint(W)
    assert type(Wd) is type(W) and Wd.bond_dims == W.bond_dims and Wd.site_ids == W.site_ids and Wd.dtype == W.dtype
    assert np.array_equal(dense_mpo(Wd.to_host()), dense_mpo(w).conj().T)
    Wdd = qil.adjoint(Wd)
    back = Wdd.to_host()
    assert all(np.array_equal(back[i], w[i]) for i in range(8))
    pd, ad = random_mps_data(saturated_profile(8, 5), rng, dt), random_mps_data(saturated_profile(8, 6), rng, np.complex128)
    cls = qil.ZTMPS if paired else qil.SignalMPS
    phi, psi = cls(pd, amplitude=0.7), cls(ad, amplitude=-1.2)
    lhs, rhs = qil.inner(phi, Wd, psi), np.conj(qil.inner(psi, W, phi))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(rhs), 1e-300)


# ---------------------------------------------------------------- 4. fused route
def _same_state(qil, a, b):
    return (a.bond_dims == b.bond_dims and a.amplitude == b.amplitude and a.dtype == b.dtype
            and all(np.array_equal(x, y) for x, y in zip(a.to_host(), b.to_host())))


@pytest.mark.parametrize("case", range(8))
def test_hadamard_compress_against_both_routes(qil, case):
    """Bit-identical to apply_compress(diagonal_mpo(phi), psi); against the exact route (hadamard, then compress) the contract
    qil_apply_compress documents, on the construction of test_apply_compress_random_products_against_oracle (random
    flat-spectrum operands): identical bonds and a state error of at most 2x the truncation's own."""
    rng = np.random.default_rng(7100 + case)
    L = int(rng.integers(8, 13))
    chi = int(rng.choice([8, 12, 16, 24, 32]))
    D = int(rng.choice([6, 8, 12, 16]))
    adt = np.complex128 if rng.random() < 0.4 else np.float64
    pdt = np.complex128 if rng.random() < 0.6 else np.float64
    conj = bool(case % 2)
    ad = random_mps_data(saturated_profile(L, chi), rng, dtype=adt)
    pd = random_mps_data(saturated_profile(L, D), rng, dtype=pdt)
    maxdim = int(rng.choice([8, 16, 32, 64]))
    tol = float(rng.choice([1e-6, 1e-8, 1e-10]))
    phi, psi = qil.SignalMPS(pd, amplitude=1.7), qil.SignalMPS(ad, amplitude=-0.9)
    fused = qil.hadamard_compress(phi, psi, conj=conj, maxdim=maxdim, tol=tol)
    via = qil.apply_compress(qil.diagonal_mpo(phi, conj=conj), psi, maxdim=maxdim, tol=tol)
    assert _same_state(qil, fused, via)
    product = qil.hadamard(phi, psi, conj=conj)
    exact = qil.compress(qil.hadamard(phi, psi, conj=conj), maxdim=maxdim, tol=tol)
    nrm = abs(product.amplitude) * qil.norm(product)
    e_trunc = qil.distance(exact, product) / nrm
    e_fused = qil.distance(fused, product) / nrm
    print(f"case {case}: L={L} chi={chi} D={D} maxdim={maxdim} tol={tol:g} e_trunc={e_trunc:.3e} e_fused={e_fused:.3e}")
    assert fused.bond_dims == exact.bond_dims, (fused.bond_dims, exact.bond_dims)
    assert e_fused <= 2 * e_trunc + 1e-9, (e_fused, e_trunc)


def test_power_spectrum_band_energies(qil):
    rng = np.random.default_rng(77)
    data = random_mps_data(saturated_profile(10, 6), rng, np.complex128)
    psi = qil.SignalMPS(data, amplitude=1.4)
    ps = qil.power_spectrum(psi)
    v = np.abs(1.4 * dense_mps(data).reshape(-1)) ** 2
    got = qil.mps_to_vector(ps)
    assert np.abs(got - v).max() <= 1e-10 * v.max()
    bits = np.full((4, 10), 2, dtype=np.uint8)
    bits[:, 0], bits[:, 1] = [0, 0, 1, 1], [0, 1, 0, 1]
    bands = qil.marginal_batch(ps, bits)
    assert np.abs(bands - v.reshape(4, -1).sum(axis=1)).max() <= 1e-10 * v.sum()


def test_failed_calls_leave_no_device_memory_behind(qil):
    ctx = qil.default_context()
    rng = np.random.default_rng(21)
    pd = random_mps_data(saturated_profile(10, 8), rng, np.complex128)
    ad = random_mps_data(saturated_profile(10, 16), rng)
    phi, psi = qil.SignalMPS(pd), qil.SignalMPS(ad)
    w = random_mpo_data(saturated_profile(10, 4, base=4), rng)
    W = qil.SingleSiteMPO(w)
    calls = {
        "hadamard": lambda: qil.hadamard(phi, psi),
        "diagonal_mpo": lambda: qil.diagonal_mpo(phi),
        "adjoint": lambda: qil.adjoint(W),
        "hadamard_compress": lambda: qil.hadamard_compress(phi, psi, conj=True, maxdim=12, tol=1e-8),
    }
    for name, call in calls.items():
        ref = call()
        failures = 0
        got = None
        for j in range(0, 2000):
            ctx.fail_alloc_after(j)
            try:
                got = call()
                failed = False
            except MemoryError:
                failed = True
            finally:
                ctx.fail_alloc_after(None)
            assert ctx.unowned_bytes() == 0, (name, j)
            if not failed:
                break
            failures += 1
        assert got is not None and failures >= (10 if name != "hadamard_compress" else 20), (name, failures)
        assert _same_state_or_operator(qil, got, ref), name
        del got, ref
    assert all(np.array_equal(phi.site(i), pd[i]) for i in range(10))


def _same_state_or_operator(qil, a, b):
    ha, hb = a.to_host(), b.to_host()
    return a.bond_dims == b.bond_dims and all(np.array_equal(x, y) for x, y in zip(ha, hb))


# ---------------------------------------------------------------- 5. errors
def test_operand_mismatches_raise_what_inner_raises(qil):
    rng = np.random.default_rng(3)
    d8 = random_mps_data(saturated_profile(8, 4), rng)
    d6 = random_mps_data(saturated_profile(6, 4), rng)
    psi = qil.SignalMPS(d8)
    other = qil.Context()
    pairs = {
        "length": (qil.SignalMPS(d6), psi),
        "sites": (qil.SignalMPS(d8, sites=list(range(11, 19))), psi),
        "paired": (qil.ZTMPS(d8), psi),
        "context": (qil.SignalMPS(d8, ctx=other), psi),
    }
    for what, (a, b) in pairs.items():
        with pytest.raises(Exception) as want:
            qil.inner(a, b)
        for fn in (qil.hadamard, lambda x, y: qil.hadamard_compress(x, y, maxdim=4)):
            with pytest.raises(type(want.value)) as got:
                fn(a, b)
            assert type(got.value) is type(want.value) is ValueError, what
            tail = lambda e: str(e.value).split(": ", 1)[1]
            assert tail(got) == tail(want), what                               # the same message under the verb's name
    del a, b, pairs
    other.close()


# ---------------------------------------------------------------- 6. inverse QFT and convolution
def _signals(n):
    N = 2 ** n
    t = np.arange(N) / N
    x = np.cos(2 * np.pi * 5 * t) * np.exp(-3 * t) + 0.3 * np.sin(2 * np.pi * 17 * t)
    h = np.exp(-40 * t) + 0.5 * np.exp(-8 * t) * np.cos(2 * np.pi * 3 * t)
    return x, h


def _np_adjoint(Fh):
    return [w.transpose(0, 2, 1, 3).conj() for w in Fh]


def _np_diag(psi, conj):
    out = []
    for i, A in enumerate(psi.data):
        A = A.conj() if conj else A
        W = np.zeros((A.shape[0], 2, 2, A.shape[2]), dtype=np.result_type(A.dtype, np.float64))
        W[:, 0, 0, :], W[:, 1, 1, :] = A[:, 0, :], A[:, 1, :]
        out.append(W * psi.amplitude if i == 0 else W)
    return O.SingleSiteMPO(out)


def _fft_reference(x, h, conj):
    fx = np.fft.fft(x)
    return np.fft.ifft((fx.conj() if conj else fx) * np.fft.fft(h))


@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("n", [6, 8, 10])
def test_untruncated_pipeline_against_numpy_on_the_same_tensors(qil, n, conj):
    """(a) device vs the numpy pipeline on the SAME tensors: 1e-12 of max|y|.  (b) device vs np.fft: at most twice the numpy
    pipeline's own deviation e_ref (the truncation of the QFT MPO at its build cutoff, common to both) + 1e-12 max|y|."""
    N = 2 ** n
    x, h = _signals(n)
    px, ph = qil.signal_mps(x), qil.signal_mps(h)
    F = qil.build_qft_mpo(n)
    Fh = F.to_host()
    # device
    X, H = qil.apply(F, px), qil.apply(F, ph)
    y_dev = np.sqrt(N) * qil.mps_to_vector(qil.apply(qil.adjoint(F), qil.hadamard(X, H, conj=conj)))
    # numpy, same tensors
    Xn = O.mps_to_vector(O.apply(O.SingleSiteMPO(Fh), O.SignalMPS(px.to_host(), amplitude=px.amplitude)))
    Hn = O.mps_to_vector(O.apply(O.SingleSiteMPO(Fh), O.SignalMPS(ph.to_host(), amplitude=ph.amplitude)))
    y_np = np.sqrt(N) * (dense_mpo(_np_adjoint(Fh)).T @ ((Xn.conj() if conj else Xn) * Hn))
    y_fft = _fft_reference(x, h, conj)
    top = np.abs(y_fft).max()
    e_same = np.abs(y_dev - y_np).max() / top
    e_ref = np.abs(y_np - y_fft).max() / top
    e_dev = np.abs(y_dev - y_fft).max() / top
    print(f"n={n} conj={conj}: device-vs-numpy {e_same:.3e}  e_ref {e_ref:.3e}  device-vs-fft {e_dev:.3e}")
    assert e_same <= 1e-12, e_same
    assert e_dev <= 2 * e_ref + 1e-12, (e_dev, e_ref)


@pytest.mark.parametrize("conj", [False, True])
def test_truncating_convolve_n12(qil, conj):
    """qil.convolve / qil.correlate at tol = 1e-10: bonds never above the untruncated pipeline's; deviation from np.fft at most
    2 e_ref(12) (the numpy pipeline's own, on the device-built QFT tensors) plus sqrt(N) times the sum of the four stages' own
    truncation errors, each measured as qil.distance(truncated stage, untruncated stage on the same inputs)."""
    n, tol = 12, 1e-10
    N = 2 ** n
    x, h = _signals(n)
    px, ph = qil.signal_mps(x), qil.signal_mps(h)
    F = qil.build_qft_mpo(n)
    Fd = qil.adjoint(F)
    y = (qil.correlate if conj else qil.convolve)(px, ph, F=F, tol=tol)
    assert type(y) is qil.SignalMPS and y.site_ids == px.site_ids
    # untruncated on the device
    Xu, Hu = qil.apply(F, px), qil.apply(F, ph)
    Pu = qil.hadamard(Xu, Hu, conj=conj)
    Yu = qil.apply(Fd, Pu)
    assert all(b <= u for b, u in zip(y.bond_dims, Yu.bond_dims)), (y.bond_dims, Yu.bond_dims)
    # the four truncated stages and their own errors
    Xt, Ht = qil.apply_compress(F, px, tol=tol), qil.apply_compress(F, ph, tol=tol)
    Pt = qil.hadamard_compress(Xt, Ht, conj=conj, tol=tol)
    Yt = qil.apply_compress(Fd, Pt, tol=tol)
    assert all(b <= u for b, u in zip(Pt.bond_dims, Pu.bond_dims))
    stages = [qil.distance(Xt, Xu), qil.distance(Ht, Hu), qil.distance(Pt, qil.hadamard(Xt, Ht, conj=conj)),
              qil.distance(Yt, qil.apply(Fd, Pt))]
    # e_ref(12): the numpy pipeline in MPS form on the same tensors (a dense 4096 x 4096 operator is not needed)
    Fo = O.SingleSiteMPO(F.to_host())
    Xn = O.apply(Fo, O.SignalMPS(px.to_host(), amplitude=px.amplitude))
    Hn = O.apply(Fo, O.SignalMPS(ph.to_host(), amplitude=ph.amplitude))
    yn = np.sqrt(N) * O.mps_to_vector(O.apply(O.SingleSiteMPO(_np_adjoint(Fo.data)), O.apply(_np_diag(Xn, conj), Hn)))
    y_fft = _fft_reference(x, h, conj)
    top = np.abs(y_fft).max()
    e_ref = np.abs(yn - y_fft).max() / top
    dev = np.abs(qil.mps_to_vector(y) - y_fft).max() / top
    bound = 2 * e_ref + np.sqrt(N) * sum(stages) / top
    print(f"n=12 conj={conj}: deviation {dev:.3e}  e_ref {e_ref:.3e}  stage distances {stages}  bound {bound:.3e}  "
          f"bonds {max(y.bond_dims)} (untruncated {max(Yu.bond_dims)})")
    assert dev <= bound, (dev, bound)


def test_convolve_n20_sampled(qil):
    """A cap against a wrong formula, three orders above the n = 12 figure: finite and below 1e-3 of max|y| on 4096 samples."""
    n = 20
    x, h = _signals(n)
    y = qil.convolve(qil.signal_mps(x), qil.signal_mps(h), tol=1e-10)
    y_fft = _fft_reference(x, h, False)
    idx = np.random.default_rng(20).integers(0, 2 ** n, size=4096)
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    got = qil.coefficient_batch(y, bits)
    dev = np.abs(got - y_fft[idx]).max() / np.abs(y_fft).max()
    print(f"n=20 convolve: deviation {dev:.3e} of max|y| on 4096 samples, bonds {max(y.bond_dims)}")
    assert np.all(np.isfinite(got)) and dev < 1e-3, dev


# ---------------------------------------------------------------- 7. full size
def test_full_size_product_on_sampled_coefficients(qil):
    phi = qil.ZTMPS.alloc(saturated_profile(48, 64), dtype=np.complex128, amplitude=-1.5).fill_random(20241016)
    psi = qil.ZTMPS.alloc(saturated_profile(48, 16), dtype=np.complex128, amplitude=0.5).fill_random(7)
    out = qil.hadamard(phi, psi, conj=True)
    assert max(out.bond_dims) == 1024 and out.amplitude == -0.75
    bits = np.random.default_rng(48).integers(0, 2, size=(4096, 48)).astype(np.uint8)
    want = qil.coefficient_batch(phi, bits).conj() * qil.coefficient_batch(psi, bits)
    got = qil.coefficient_batch(out, bits)
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want) + 1e-300), (np.abs(got - want) / np.abs(want)).max()
