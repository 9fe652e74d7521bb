"""GPU tests of the linear combinations (qil.linear_combination, linear_combination_compress, add / sub / scale, `+` / `-`) and
of exponential_mps / exponential_sum on top of them.

Tolerances: interior and last tensors of the materialised sum are EQUAL to the numpy direct sum (copies and exact zeros); the
first tensor, which carries the one multiply by the weight, is within 1e-14 of its largest entry (what test_gpu_parity.py holds
`apply` to); dense read-outs 1e-12 of scale (the project's read-out tolerance); the fused route against the exact one: identical
bonds and a state error <= 2x the exact route's + 1e-9 (the contract of qil_apply_compress and the floor of qil_compress);
1e-10 relative at full size (as the top-k tests).  The reference restatement of the sum is `_direct_sum` below."""
import numpy as np
import pytest

import oracle as O
from helpers import random_mps_data, saturated_profile, dense_mps

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


def _scale(t):
    return max(np.abs(t).max(), 1e-300)


def _direct_sum(terms, w):
    """The numpy direct sum of host chains with the weights w (coefficient * amplitude) in the first tensor."""
    N = len(terms[0])
    dt = np.result_type(*[t[0].dtype for t in terms], np.complex128 if np.iscomplexobj(w) and np.any(np.imag(w) != 0) else np.float64)
    w = np.asarray(w).astype(dt)
    if N == 1:
        return [sum(c * t[0] for c, t in zip(w, terms)).astype(dt)]
    out = [np.concatenate([c * t[0].astype(dt) for c, t in zip(w, terms)], axis=2)]
    for i in range(1, N - 1):
        A = np.zeros((sum(t[i].shape[0] for t in terms), 2, sum(t[i].shape[2] for t in terms)), dt)
        lo = ro = 0
        for t in terms:
            A[lo:lo + t[i].shape[0], :, ro:ro + t[i].shape[2]] = t[i]
            lo, ro = lo + t[i].shape[0], ro + t[i].shape[2]
        out.append(A)
    out.append(np.concatenate([t[N - 1].astype(dt) for t in terms], axis=0))
    return out


# ---------------------------------------------------------------- 1. site tensors against the numpy direct sum
CASES = {
    "n1": [],
    "bond1": [1] * 7,
    "odd": [2, 3, 5, 7, 5, 3, 2],
    "sat8": saturated_profile(12, 8),
    "sat64": saturated_profile(14, 64),
}
KINDS = [(c, p) for c in sorted(CASES) for p in (False, True) if not (p and c == "n1")]
# (dtype of the even terms, dtype of the odd terms)
DTYPES = [(np.float64, np.float64), (np.float64, np.complex128), (np.complex128, np.float64), (np.complex128, np.complex128)]


def _term_bonds(base, j):
    """mixed bonds per term: term j has the profile capped at a term-dependent value (never above the saturated one)"""
    cap = (3, 64, 5, 2, 7, 1, 4)[j % 7]
    n = len(base) + 1
    return [min(b, cap, 2 ** (i + 1), 2 ** (n - 1 - i)) for i, b in enumerate(base)]


def _check_sum(qil, datas, amps, coeffs, paired, handles=None):
    """datas[j]: host tensors of term j; handles: term j -> index of the state to use (repeated handles)"""
    handles = list(range(len(datas))) if handles is None else handles
    states = {h: _mps(qil, datas[h], paired, amps[h]) for h in set(handles)}
    terms = [states[h] for h in handles]
    out = qil.linear_combination(terms, coeffs)
    tdata, tamps = [datas[h] for h in handles], [amps[h] for h in handles]
    c = np.ones(len(terms)) if coeffs is None else np.asarray(coeffs)
    w = c * np.asarray(tamps)
    ref = _direct_sum(tdata, w)
    assert type(out) is type(terms[0]) and out.site_ids == terms[0].site_ids and out.paired == terms[0].paired
    assert out.dtype == ref[0].dtype
    assert out.amplitude == 1.0
    assert out.bond_dims == [sum(b) for b in zip(*[t.bond_dims for t in terms])] if len(tdata[0]) > 1 else out.bond_dims == []
    n = len(ref)
    for i in range(n):
        got = out.site(i)
        assert got.shape == ref[i].shape and got.dtype == ref[i].dtype, i
        if i == 0:
            assert np.abs(got - ref[i]).max() <= 1e-14 * _scale(ref[i]), (i, np.abs(got - ref[i]).max() / _scale(ref[i]))
        else:
            assert np.array_equal(got, ref[i]), i                     # copies and exact zeros, off-block entries included
            assert not np.any(np.signbit(got.real[ref[i] == 0])), i   # +0.0
    if n <= 14:
        dv = sum(wj * dense_mps(d).reshape(-1) for wj, d in zip(w, tdata))
        got = qil.mps_to_vector(out)
        top = max(_scale(dv), max(abs(wj) * _scale(dense_mps(d)) for wj, d in zip(w, tdata)))
        assert np.abs(got - dv).max() <= 1e-12 * top, np.abs(got - dv).max() / top
    return out


@pytest.mark.parametrize("cplx_coeff", [False, True])
@pytest.mark.parametrize("dt0,dt1", DTYPES)
@pytest.mark.parametrize("nterms", [1, 2, 3, 7])
@pytest.mark.parametrize("case,paired", KINDS)
def test_sum_matches_the_numpy_direct_sum(qil, case, paired, nterms, dt0, dt1, cplx_coeff):
    rng = np.random.default_rng(sorted(CASES).index(case) * 1000 + 100 * paired + 10 * nterms + 4 * cplx_coeff
                                + 2 * (dt0 == np.complex128) + (dt1 == np.complex128))
    base = CASES[case]
    datas = [random_mps_data(_term_bonds(base, j) if base else [], rng, dt1 if j % 2 else dt0) for j in range(nterms)]
    amps = [float(a) for a in rng.uniform(0.5, 2.0, nterms) * rng.choice([-1.0, 1.0], nterms)]
    coeffs = rng.standard_normal(nterms) + (1j * rng.standard_normal(nterms) if cplx_coeff else 0)
    handles = list(range(nterms))
    if nterms >= 3:
        coeffs[1] = 0                       # a zero-weight term keeps its block
        handles[2] = 0                      # a repeated handle
    _check_sum(qil, datas, amps, coeffs, paired, handles)


def test_null_coefficients_are_ones_and_operators_compose(qil):
    rng = np.random.default_rng(5)
    d1, d2 = random_mps_data(saturated_profile(9, 6), rng), random_mps_data(saturated_profile(9, 4), rng, np.complex128)
    _check_sum(qil, [d1, d2], [1.5, -0.5], None, False)
    a, b = qil.SignalMPS(d1, amplitude=1.5), qil.SignalMPS(d2, amplitude=-0.5)
    va, vb = qil.mps_to_vector(a), qil.mps_to_vector(b)
    for got, want in ((a + b, va + vb), (a - b, va - vb), (-a, -va), (qil.scale(b, 2.5), 2.5 * vb), (qil.scale(a, 1j), 1j * va),
                      (qil.add(a, a), 2 * va), (qil.sub(b, a), vb - va)):
        assert type(got) is qil.SignalMPS
        assert np.abs(qil.mps_to_vector(got) - want).max() <= 1e-12 * _scale(want)
    assert (-a).amplitude == -1.5 and (-a).bond_dims == a.bond_dims and qil.scale(a, 2).dtype == np.float64
    z1 = qil.ZTMPS(random_mps_data(saturated_profile(8, 4), rng))
    z2 = qil.ZTMPS(random_mps_data(saturated_profile(8, 3), rng))
    assert type(z1 + z2) is qil.ZTMPS and (z1 - z2).paired


# ---------------------------------------------------------------- 2. tiling edges
def test_one_wide_term_next_to_bond_one_terms(qil):
    """one term whose bond exceeds a row tile (600 > 512 rows of a real tile), next to bond-1 terms"""
    rng = np.random.default_rng(11)
    wide = [2, 4, 600, 4, 2]
    for dt in (np.float64, np.complex128):
        datas = [random_mps_data([1] * 5, rng, dt), random_mps_data(wide, rng, dt), random_mps_data([1] * 5, rng, dt)]
        _check_sum(qil, datas, [1.0, -2.0, 0.5], [1.0, 0.25, -3.0], False)


def test_33_terms_of_bond_3(qil):
    """odd row counts and unaligned offsets: 99 rows, every block starts at a multiple of 3"""
    rng = np.random.default_rng(12)
    for dt in (np.float64, np.complex128):
        datas = [random_mps_data([2, 3, 3, 3, 3, 2], rng, dt) for _ in range(33)]
        _check_sum(qil, datas, [1.0] * 33, rng.standard_normal(33), False)


def test_real_result_with_odd_rows_takes_the_unpacked_store(qil):
    rng = np.random.default_rng(13)
    datas = [random_mps_data([2, 4, 5, 4, 2], rng), random_mps_data([2, 3, 4, 3, 1], rng), random_mps_data([1, 2, 2, 2, 2], rng)]
    out = _check_sum(qil, datas, [1.0, 1.0, 1.0], [1.0, -1.0, 2.0], False)
    assert out.dtype == np.float64 and [b % 2 for b in out.bond_dims] == [1, 1, 1, 1, 1]


# ---------------------------------------------------------------- 3. algebra
def test_psi_minus_psi_is_zero(qil):
    """norm <= 1e-13 |psi|, read out densely: qil.norm is the square root of a quadratic form whose four block contributions
    cancel, so IT resolves a zero state only to sqrt(eps) |psi|."""
    rng = np.random.default_rng(31)
    for dt in (np.float64, np.complex128):
        d = random_mps_data(saturated_profile(12, 16), rng, dt)
        psi = qil.SignalMPS(d, amplitude=3.0)
        z = psi + (-psi)
        assert z.bond_dims == [2 * b for b in psi.bond_dims]
        assert np.linalg.norm(qil.mps_to_vector(z)) <= 1e-13 * 3.0 * qil.norm(psi)


def test_inner_is_linear_in_the_sum(qil):
    rng = np.random.default_rng(32)
    phi = qil.SignalMPS(random_mps_data(saturated_profile(16, 12), rng, np.complex128), amplitude=0.8)
    psi = qil.SignalMPS(random_mps_data(saturated_profile(16, 9), rng, np.complex128), amplitude=-1.1)
    chi = qil.SignalMPS(random_mps_data(saturated_profile(16, 20), rng), amplitude=2.0)
    a, b = 0.7 - 0.2j, -1.3 + 0.9j
    lhs = qil.inner(phi, qil.linear_combination([psi, chi], [a, b]))
    t1, t2 = a * qil.inner(phi, psi), b * qil.inner(phi, chi)
    assert abs(lhs - (t1 + t2)) <= 1e-12 * (abs(t1) + abs(t2))


def test_apply_is_linear_and_addition_commutes(qil):
    """W(a phi + b psi) against a W phi + b W psi through apply then distance, and add(phi, psi) against add(psi, phi):
    <= 1e-12 of the norm.  `distance` resolves no relative distance below ~1e-7 from its expansion (see its docstring), so
    both differences are read out densely, as a vector norm."""
    rng = np.random.default_rng(33)
    n = 12
    phi = qil.SignalMPS(random_mps_data(saturated_profile(n, 8), rng, np.complex128), amplitude=1.2)
    psi = qil.SignalMPS(random_mps_data(saturated_profile(n, 5), rng), amplitude=-0.6)
    W = qil.build_qft_mpo(n)
    a, b = 0.4 + 1.1j, -2.0
    lhs = qil.apply(W, qil.linear_combination([phi, psi], [a, b]))
    rhs = qil.linear_combination([qil.apply(W, phi), qil.apply(W, psi)], [a, b])
    nrm = np.linalg.norm(qil.mps_to_vector(rhs))
    assert np.linalg.norm(qil.mps_to_vector(lhs) - qil.mps_to_vector(rhs)) <= 1e-12 * nrm
    assert qil.distance(lhs, rhs) <= 1e-6 * nrm                      # the floor of the expansion
    s1, s2 = qil.add(phi, psi), qil.add(psi, phi)
    nrm = np.linalg.norm(qil.mps_to_vector(s1))
    assert np.linalg.norm(qil.mps_to_vector(s1) - qil.mps_to_vector(s2)) <= 1e-12 * nrm
    assert qil.distance(s1, s2) <= 1e-6 * nrm


# ---------------------------------------------------------------- 4. fused against exact
def _fused_case(rng, trial):
    n = int(rng.integers(8, 13))
    nb = int(rng.integers(2, 6))
    chi = int(rng.choice([4, 8, 16]))
    cplx = trial % 2
    terms = [random_mps_data(saturated_profile(n, chi), rng, np.complex128 if cplx else np.float64) for _ in range(nb)]
    coef = rng.standard_normal(nb) + (1j * rng.standard_normal(nb) if cplx else 0)
    maxdim = int(rng.choice([4, 8, 12, 1000]))
    return terms, coef, (None if maxdim == 1000 else maxdim)


def _damped_terms(qil, k, rng):
    n = 12
    t = np.arange(2 ** n) / 2 ** n
    xs = [np.exp(-rng.uniform(1, 6) * t) * np.cos(2 * np.pi * rng.integers(3, 40) * t + rng.uniform(0, 6)) for _ in range(k)]
    states = [qil.signal_mps(x) for x in xs]
    return states, [s.to_host() for s in states], [s.amplitude for s in states]


def _route(states, maxdim):
    """Which way qil_mps_sum_compress takes: "stacked" when every concatenated bond fits under the intermediate cap (the exact
    route's gauge pass on the row-stacked operands, no zip-up), "zip-up" otherwise (sites whose bond fits still take the stacked
    step).  Restated from the documented rule: cap = max(maxdim + 16, maxdim + ceil(maxdim / 8)), none without maxdim."""
    if maxdim is None:
        return "stacked"
    cap = max(maxdim + 16, maxdim + (maxdim + 7) // 8)
    widest = max(sum(b) for b in zip(*[s.bond_dims for s in states]))
    return "stacked" if widest <= cap else f"zip-up (sum chi {widest} > cap {cap})"


def _check_fused(qil, states, datas, amps, coef, maxdim, tol, label):
    w = np.asarray(coef) * np.asarray(amps)
    ref = O.SignalMPS(_direct_sum(datas, w))
    dense = O.mps_to_vector(ref)
    O.compress(ref, maxdim=maxdim, tol=tol)
    v_or = O.mps_to_vector(ref)
    b_or = [a.shape[2] for a in ref.data[:-1]]
    fused = qil.linear_combination_compress(states, coef, maxdim=maxdim, tol=tol)
    exact = qil.compress(qil.linear_combination(states, coef), maxdim=maxdim, tol=tol)
    sc = np.linalg.norm(dense)
    e_or = np.linalg.norm(v_or - dense) / sc
    e_fu = np.linalg.norm(qil.mps_to_vector(fused) - dense) / sc
    e_ex = np.linalg.norm(qil.mps_to_vector(exact) - v_or) / sc
    print(f"{label}: route {_route(states, maxdim)} nb={len(states)} maxdim={maxdim} bonds oracle {max(b_or)} fused {max(fused.bond_dims)} "
          f"e_oracle={e_or:.3e} e_fused={e_fu:.3e} ratio={e_fu / max(e_or, 1e-300):.3f} exact-vs-oracle={e_ex:.3e}")
    assert abs(qil.norm(fused) - 1) <= 1e-10                                   # compress!: unit-norm tensors, norm in amplitude
    assert fused.bond_dims == b_or, (fused.bond_dims, b_or)
    assert e_fu <= 2 * e_or + 1e-9, (e_fu, e_or)
    assert exact.bond_dims == b_or, (exact.bond_dims, b_or)
    assert e_ex <= 1e-9, e_ex


def test_fused_route_against_the_oracle_on_random_sums(qil):
    """The 24 seeded cases of the prototype's distribution (n 8..12, 2..5 terms, chi 4..16, f64 / c64, maxdim 4 / 8 / 12 /
    none, tol 1e-8): reference = oracle.compress on the numpy direct sum."""
    rng = np.random.default_rng(0)
    for trial in range(24):
        datas, coef, maxdim = _fused_case(rng, trial)
        amps = [1.0 + 0.25 * j for j in range(len(datas))]
        states = [qil.SignalMPS(d, amplitude=a) for d, a in zip(datas, amps)]
        _check_fused(qil, states, datas, amps, coef, maxdim, 1e-8, f"random {trial}")


@pytest.mark.parametrize("case", range(5))
def test_fused_route_on_sums_of_damped_sinusoids(qil, case):
    rng = np.random.default_rng(900 + case)
    k = 2 + case % 3
    states, datas, amps = _damped_terms(qil, k, rng)
    coef = rng.standard_normal(k)
    _check_fused(qil, states, datas, amps, coef, (None, 6, 4, 8, 3)[case], 1e-8, f"damped {case}")


def test_fused_route_above_the_grouped_threshold(qil):
    """terms of bond 96 > 64 take the GEMM per term instead of the grouped launch: same contract"""
    rng = np.random.default_rng(77)
    datas = [random_mps_data(saturated_profile(14, 96), rng, np.float64) for _ in range(3)]
    states = [qil.SignalMPS(d) for d in datas]
    fused = qil.linear_combination_compress(states, [1.0, -0.5, 2.0], maxdim=32, tol=1e-8)
    full = qil.linear_combination(states, [1.0, -0.5, 2.0])
    exact = qil.compress(qil.linear_combination(states, [1.0, -0.5, 2.0]), maxdim=32, tol=1e-8)
    dense = qil.mps_to_vector(full)
    e_ex = np.linalg.norm(qil.mps_to_vector(exact) - dense)
    e_fu = np.linalg.norm(qil.mps_to_vector(fused) - dense)
    print(f"above threshold: e_exact={e_ex:.3e} e_fused={e_fu:.3e}")
    assert fused.bond_dims == exact.bond_dims and e_fu <= 2 * e_ex + 1e-9 * np.linalg.norm(dense)


# ---------------------------------------------------------------- 5. exponential_sum at n = 40
def _fixed_point_powers(z, idx, n, frac=200):
    """z^j for a double-complex z (|z| <= 1) and integers j < 2^n in 200-bit fixed point, as long doubles: the reference needs
    more than long double arithmetic, whose j * eps = 2^40 * 5e-20 = 6e-8 is above the gate"""
    from fractions import Fraction
    one = 1 << frac
    sq = [(int(Fraction(z.real) * one), int(Fraction(z.imag) * one))]
    for _ in range(n - 1):
        zr, zi = sq[-1]
        sq.append(((zr * zr - zi * zi) >> frac, (2 * zr * zi) >> frac))
    out = np.zeros(len(idx), dtype=np.clongdouble)
    for t, j in enumerate(idx):
        rr, ri, k = one, 0, 0
        j = int(j)
        while j:
            if j & 1:
                zr, zi = sq[k]
                rr, ri = (rr * zr - ri * zi) >> frac, (rr * zi + ri * zr) >> frac
            j >>= 1
            k += 1
        # 64 leading bits of the 200 are what a long double holds
        out[t] = np.longdouble(rr >> (frac - 70)) / np.longdouble(1 << 70) + 1j * (np.longdouble(ri >> (frac - 70)) / np.longdouble(1 << 70))
    return out


def test_exponential_sum_n40_against_the_closed_form(qil):
    """6 modes, 2^40 samples: 4096 seeded coefficients against sum_k a_k z_k^j with the powers from 200-bit fixed point and the
    sum in long double; 1e-10 relative, sample by sample; bond after compression <= 6.  Every mode lives over the whole record
    (damping <= 3e-12 per sample): compress! opens with a gauge pass at cutoff 1e-12 of the squared norm, so a mode that dies
    within a few samples of 2^40 carries 1e-12 of the weight and is, rightly, truncated away."""
    n = 40
    rng = np.random.default_rng(40)
    zs = [complex(np.exp(-g + 1j * th)) for g, th in zip(rng.uniform(0, 3e-12, 6), rng.uniform(0.1, 3.0, 6))]
    zs[0] = complex(abs(zs[0]))                                        # a purely damped mode: real z = exp(-g)
    amps = rng.standard_normal(6) + 1j * rng.standard_normal(6)
    x = qil.exponential_sum(amps, zs, n, tol=1e-12)
    assert type(x) is qil.SignalMPS and len(x) == n and max(x.bond_dims) <= 6, x.bond_dims
    idx = rng.integers(0, 2 ** n, size=4096)
    idx[:4] = [0, 1, 2 ** n - 1, 2 ** 39]
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    got = qil.coefficient_batch(x, bits)
    want = np.zeros(4096, dtype=np.clongdouble)
    for a, z in zip(amps, zs):
        want += np.clongdouble(a) * _fixed_point_powers(z, idx, n)
    err = (np.abs(got - want) / np.abs(want)).max()
    print(f"exponential_sum n=40: bonds {max(x.bond_dims)}, worst relative deviation {float(err):.3e}")
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 1e-10 * np.abs(want)), float(err)
    raw = qil.exponential_sum(amps, zs, n, tol=None)
    assert raw.bond_dims == [6] * (n - 1) and raw.amplitude == 1.0
    got = qil.coefficient_batch(raw, bits)
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want))


# ---------------------------------------------------------------- 6. failure paths
def _same_state(a, b):
    return a.bond_dims == b.bond_dims and a.amplitude == b.amplitude and all(
        np.array_equal(x, y) for x, y in zip(a.to_host(), b.to_host()))


def test_failed_calls_leave_no_device_memory_behind(qil):
    ctx = qil.default_context()
    rng = np.random.default_rng(21)
    d1 = random_mps_data(saturated_profile(10, 8), rng, np.complex128)
    d2 = random_mps_data(saturated_profile(10, 16), rng)
    a, b = qil.SignalMPS(d1, amplitude=0.5), qil.SignalMPS(d2)
    calls = {
        "linear_combination": lambda: qil.linear_combination([a, b, a], [1.0, 2.0, -0.5j]),
        "linear_combination_compress": lambda: qil.linear_combination_compress([a, b, a], [1.0, 2.0, -0.5j], maxdim=12, tol=1e-8),
    }
    for name, call in calls.items():
        ref = call()
        failures = 0
        got = None
        for j in range(0, 3000):
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
        assert got is not None and failures >= (10 if name == "linear_combination" else 40), (name, failures)
        assert _same_state(got, ref), name
        del got, ref
    assert all(np.array_equal(a.site(i), d1[i]) for i in range(10)) and a.amplitude == 0.5


def test_operand_mismatches_raise_what_inner_raises(qil):
    L = __import__("importlib").import_module("qilaplace_jl_amd._lib")
    rng = np.random.default_rng(3)
    d8 = random_mps_data(saturated_profile(8, 4), rng)
    d6 = random_mps_data(saturated_profile(6, 4), rng)
    psi = qil.SignalMPS(d8)
    other = qil.Context()
    pairs = {
        "length": (qil.SignalMPS(d6), L.QIL_EINVAL_LENGTH),
        "sites": (qil.SignalMPS(d8, sites=list(range(11, 19))), L.QIL_EINVAL_SITES),
        "context": (qil.SignalMPS(d8, ctx=other), L.QIL_EINVAL_ARG),
    }
    import ctypes as C
    for what, (bad, code) in pairs.items():
        with pytest.raises(ValueError) as want:
            qil.inner(psi, bad)
        for fn in (qil.linear_combination, lambda t: qil.linear_combination_compress(t, maxdim=4)):
            with pytest.raises(ValueError) as got:
                fn([psi, psi, bad])
            tail = lambda e: str(e.value).split(": ", 1)[1]
            assert tail(got) == tail(want), what                               # the same message under the verb's name
        arr = (C.c_void_p * 2)(psi.handle.value, bad.handle.value)
        h = C.c_void_p()
        assert L.lib.qil_mps_sum(arr, 2, None, C.byref(h)) == code and h.value is None
        assert L.lib.qil_mps_sum_compress(arr, 2, None, 4, 1e-8, 1, 0, C.byref(h)) == code and h.value is None
    # mixed register kinds: refused by the front-end (TypeError) and by the library (QIL_EINVAL_ARG)
    zt = qil.ZTMPS(random_mps_data(saturated_profile(8, 4), rng))
    arr = (C.c_void_p * 2)(psi.handle.value, zt.handle.value)
    h = C.c_void_p()
    assert L.lib.qil_mps_sum(arr, 2, None, C.byref(h)) == L.QIL_EINVAL_ARG and "paired" in L.last_error()
    one = qil.SignalMPS(random_mps_data([], rng))
    with pytest.raises(qil.QilDomainError):
        qil.linear_combination_compress([one, one], maxdim=4)
    with pytest.raises(ValueError, match="sweeps"):
        qil.linear_combination_compress([psi, psi], sweeps=0)
    with pytest.raises(ValueError, match="not finite"):
        qil.linear_combination([psi, psi], [1.0, np.nan])
    del bad, pairs
    other.close()


# ---------------------------------------------------------------- 7. full size
def _sum_error_from_inner(qil, out, terms, c):
    """|out - sum_j c_j psi_j|^2 = |out|^2 - 2 Re sum_j c_j <out|psi_j> + sum_jk conj(c_j) c_k <psi_j|psi_k>, from inner alone"""
    nb = len(terms)
    n_out = (out.amplitude * qil.norm(out)) ** 2
    cross = sum(c[j] * qil.inner(out, terms[j]) for j in range(nb))
    G = np.zeros((nb, nb), dtype=np.complex128)
    for j in range(nb):
        for k in range(j, nb):
            G[j, k] = qil.inner(terms[j], terms[k])
            G[k, j] = np.conj(G[j, k])
    n_sum = np.real(np.conj(c) @ G @ c)
    return float(np.sqrt(max(0.0, n_out - 2 * np.real(cross) + n_sum))), float(np.sqrt(n_sum))


def test_full_size_sum_of_64_states(qil):
    """64 terms of n = 24, chi = 64, c64: the fused entry completes with bonds <= 64.  Random terms are nearly orthogonal, so
    the truncation error is large; accuracy is gated at 8 terms, where the exact route fits (fused error <= 2x the exact
    route's, identical bonds); the 64-term case has to be finite and no worse than returning zero."""
    rng = np.random.default_rng(64)
    prof = saturated_profile(24, 64)
    terms = [qil.SignalMPS.alloc(prof, dtype=np.complex128, amplitude=1.0 + 0.01 * j).fill_random(1000 + j) for j in range(64)]
    c = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    small, cs = terms[:8], c[:8]
    fused8 = qil.linear_combination_compress(small, cs, maxdim=64, tol=1e-8)
    exact8 = qil.compress(qil.linear_combination(small, cs), maxdim=64, tol=1e-8)
    e_fu, nrm = _sum_error_from_inner(qil, fused8, small, cs)
    e_ex, _ = _sum_error_from_inner(qil, exact8, small, cs)
    print(f"8 x chi 64: |sum| {nrm:.4e}  exact-route error {e_ex:.4e}  fused error {e_fu:.4e}  ratio {e_fu / e_ex:.3f}")
    assert fused8.bond_dims == exact8.bond_dims, (fused8.bond_dims, exact8.bond_dims)
    assert e_fu <= 2 * e_ex, (e_fu, e_ex)
    out = qil.linear_combination_compress(terms, c, maxdim=64, tol=1e-8)
    assert max(out.bond_dims) <= 64 and np.isfinite(out.amplitude)
    err, nrm = _sum_error_from_inner(qil, out, terms, c)
    print(f"64 x chi 64: |sum| {nrm:.4e}  error {err:.4e}")
    bits = rng.integers(0, 2, size=(256, 24)).astype(np.uint8)
    assert np.all(np.isfinite(qil.coefficient_batch(out, bits)))
    assert np.isfinite(err) and err <= nrm, (err, nrm)
