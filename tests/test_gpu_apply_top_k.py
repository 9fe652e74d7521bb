"""GPU tests of the lazy top-k search of W psi (qil.apply_top_k, qil_apply_top_k), which never forms W psi.

The oracle is a numpy beam search on dense marginals.  v = helpers.apply_dense(w, a) (or the dense vector of the site-wise product
MPS where the 2^n x 2^n operator does not fit); at level i the key of a prefix is the sum of |v|^2 over the trailing sites divided
by |v|^2, which is what key = p q_s / (q_0 + q_1) is in exact arithmetic; the cut rule of the header with a stable sort: keep the
min(2 f, beam) largest (k at the last level), ties to the lower candidate 2 row + s, the next frontier in candidate order, the
largest key dropped before the last level recorded.  It returns the kept set in descending |value|, the values, the bound
sqrt(largest dropped key sum |v|^2) |amp| and the smallest relative gap (key_M - key_{M+1}) / key_M over all cuts, next to the
smallest relative gap between consecutive returned magnitudes.  The gaps are conditions, not tolerances: every comparison of rows
asserts gap > 1e-9 for its case, so that rounding (1e-15 per tensor) cannot decide a cut; the inputs are chosen so that the
oracle alone meets it.

Shapes (chi bonds of psi / D bonds of W): the seven profiles of test_gpu_apply_sample.py.  All have an even number of tensors, so
each also runs paired.  (k, beam) in (1, 1), (3, 5), (7, 37), (16, 64), k clipped to the 2^n configurations of the two-tensor
chain (a larger k is an error by contract).  Both routes (QIL_APPLY_SAMPLE_ROUTE) run everywhere."""
import ctypes as C
import functools
import importlib
import importlib.util
import os

import numpy as np
import pytest

from helpers import random_mps_data, random_mpo_data, saturated_profile, apply_dense, dense_mps, basis_mps

pytestmark = pytest.mark.gpu

GAP = 1e-9
SLACK = 1e-10                                                                # certified: bound < |value_k| (1 - 1e-10)
ROUTE = "QIL_APPLY_SAMPLE_ROUTE"
RENV = "QIL_APPLY_SAMPLE_RENV_BYTES"
ROUTES = ["fused", "gemm"]
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
K_BEAM = [(1, 1), (3, 5), (7, 37), (16, 64)]


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
def oracle_top_k(v, k, beam, amp=1.0):
    """(indices (site 1 = MSB) in descending |value|, values, bound, cut gap, order gap) of the beam search on the dense vector v"""
    v = np.asarray(v).reshape(-1)
    n = int(np.log2(v.size))
    P = np.abs(v) ** 2
    tot = P.sum()
    frontier = np.zeros(1, dtype=np.int64)
    dropped, gap = 0.0, np.inf
    for i in range(n):
        marg = P.reshape(2 ** (i + 1), -1).sum(axis=1) / tot                    # [prefix, site 1 = MSB]
        cand = (2 * frontier[:, None] + np.arange(2)[None, :]).reshape(-1)      # candidate 2 row + s
        keys = marg[cand]
        M = min(cand.size, k if i == n - 1 else beam)
        if M < cand.size:
            order = np.argsort(-keys, kind="stable")
            a, b = keys[order[M - 1]], keys[order[M]]
            gap = min(gap, (a - b) / a if a > 0 else 0.0)
            if i < n - 1:
                dropped = max(dropped, b)
            cand = cand[np.sort(order[:M])]
        frontier = cand
    vals = amp * v[frontier]
    order = np.argsort(-np.abs(vals), kind="stable")
    mag = np.abs(vals[order])
    ogap = np.min((mag[:-1] - mag[1:]) / mag[:-1]) if mag.size > 1 else np.inf
    return frontier[order], vals[order], float(np.sqrt(dropped * tot) * abs(amp)), gap, ogap


def product_dense(w, a):
    """the dense vector of the site-wise product MPS B[(alpha, a), s_out, (beta, b)] = sum_s' A[alpha, s', beta] W[a, s', s_out, b]"""
    sites = [np.einsum("xsy,asub->xauyb", A, T).reshape(A.shape[0] * T.shape[0], 2, A.shape[2] * T.shape[3]) for A, T in zip(a, w)]
    return dense_mps(sites).reshape(-1)


def _index(rows):
    return rows.astype(np.int64) @ (np.int64(1) << np.arange(rows.shape[1] - 1, -1, -1, dtype=np.int64))


def _amp(dt):
    return -1.3 if dt == Z else 1.7                                           # a parent amplitude != 1


def _beam_cap(chi, D, itemsize):
    """the documented cap, restated: beam <= min(2^29, 2^30 / (3 maxM e + 4 n + 64)), maxM = max(chi_l D_l, chi_r D_r)"""
    c, d = [1] + list(chi) + [1], [1] + list(D) + [1]
    n = len(c) - 1
    m = max(max(c[i] * d[i], c[i + 1] * d[i + 1]) for i in range(n))
    return min(2 ** 29, 2 ** 30 // (3 * m * itemsize + 4 * n + 64))


def _chunk(chi, D, fcap, itemsize):
    """the documented chunk size, restated: max(1, min(largest frontier, 32768, 64 MiB / ((2 maxM + maxX) e + 16 ceil(maxM / 64))))"""
    c, d = [1] + list(chi) + [1], [1] + list(D) + [1]
    m = x = 1
    for i in range(len(c) - 1):
        m = max(m, c[i] * d[i], c[i + 1] * d[i + 1])
        x = max(x, 2 * c[i] * d[i + 1])
    return max(1, min(fcap, 32768, (64 << 20) // ((2 * m + x) * itemsize + 16 * ((m + 63) // 64))))


@functools.lru_cache(maxsize=None)
def _case(case, dta, dtw):
    """host tensors and the dense vector (without the amplitude): computed once, shared, left unchanged"""
    rng = np.random.default_rng(31000 + 4 * CASES.index(case) + 2 * (dta == Z) + (dtw == Z))
    chi, D = PROFILES[case]
    a = random_mps_data(chi, rng, dta)
    w = random_mpo_data(D, rng, dtw)
    v = apply_dense(w, a)
    v.setflags(write=False)
    return a, w, v


@functools.lru_cache(maxsize=None)
def _oracle(case, dta, dtw, k, beam):
    a, w, v = _case(case, dta, dtw)
    return oracle_top_k(v, k, beam, _amp(dta))


def _clip(case, k, beam):
    k = min(k, 2 ** (len(PROFILES[case][0]) + 1))
    return k, max(beam, k)


def _operands(qil, a, w, paired, amp):
    if paired:
        return qil.PairedSiteMPO(w), qil.ZTMPS(a, amplitude=amp)
    return qil.SingleSiteMPO(w), qil.SignalMPS(a, amplitude=amp)


def _check_against_oracle(got, want, scale):
    rows, vals, bound, cert = got
    idx, ovals, obound, gap, ogap = want
    assert gap > GAP and ogap > GAP, (gap, ogap)
    assert np.array_equal(_index(rows), idx)
    err = np.abs(vals - ovals).max() / scale
    assert err <= 1e-10, err
    assert (bound == 0.0 and obound == 0.0) or abs(bound - obound) <= 1e-9 * obound, (bound, obound)
    assert cert == bool(obound < np.abs(ovals[-1]) * (1.0 - SLACK))
    return err


# ---------------------------------------------------------------- 1. oracle parity
def test_the_oracle_meets_its_gap_condition_on_every_case():
    """The condition the row comparisons below rest on, for all cases at once; needs no device.  The cut gaps of the recorded
    draw order: the smallest is 5.9e-5."""
    gaps, kinds = [], set()
    for case in CASES:
        for dts in DT_PAIRS:
            for kb in K_BEAM:
                idx, vals, bound, gap, ogap = _oracle(case, *dts, *_clip(case, *kb))
                gaps.append(min(gap, ogap))
                kinds.add((bound == 0.0, bool(bound < np.abs(vals[-1]) * (1.0 - SLACK))))
    print(f"smallest gap over {len(gaps)} oracle runs: {min(gaps):.2e}")
    assert min(gaps) > GAP
    assert kinds == {(True, True), (False, True), (False, False)}               # exact, certified with drops, uncertified


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
@pytest.mark.parametrize("case", CASES)
def test_oracle_parity(qil, case, paired, dts, route, monkeypatch):
    a, w, v = _case(case, *dts)
    monkeypatch.setenv(ROUTE, route)
    amp = _amp(dts[0])
    W, psi = _operands(qil, a, w, paired, amp)
    n = len(a)
    worst = 0.0
    for kb in K_BEAM:
        k, beam = _clip(case, *kb)
        got = qil.apply_top_k(W, psi, k, beam=beam, bits=True)
        assert got[0].shape == (k, n) and got[0].dtype == np.uint8 and got[1].shape == (k,)
        assert got[1].dtype == (Z if Z in dts else F)
        worst = max(worst, _check_against_oracle(got, _oracle(case, *dts, k, beam), np.abs(amp * v).max()))
    print(f"apply_top_k {case} paired={paired} {DT_IDS[DT_PAIRS.index(dts)]} {route}: worst value error {worst:.2e} of max |v|")


def test_index_decoding(qil):
    a, w, v = _case("sat", F, Z)
    n = len(a)
    W, psi = _operands(qil, a, w, False, 1.0)
    rows, vals, bound, cert = qil.apply_top_k(W, psi, 7, beam=37, bits=True)
    idx, v2, b2, c2 = qil.apply_top_k(W, psi, 7, beam=37)
    assert np.array_equal(idx, _index(rows)) and np.array_equal(vals, v2) and bound == b2 and cert == c2
    Wp, zt = _operands(qil, a, w, True, 1.0)
    (kk, ll), vz, bz, cz = qil.apply_top_k(Wp, zt, 7, beam=37)
    assert np.array_equal(kk, rows[:, 0::2].astype(np.int64) @ (1 << np.arange(n // 2)))
    assert np.array_equal(ll, rows[:, 1::2].astype(np.int64) @ (1 << np.arange(n // 2)))
    assert np.array_equal(vz, vals) and bz == bound and cz == cert


# ---------------------------------------------------------------- 2. full beam
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dts", [(F, F), (Z, Z)], ids=["f64-f64", "c64-c64"])
@pytest.mark.parametrize("case", ["odd", "sat", "two"])
def test_full_beam_is_exact_and_certified(qil, case, dts, route, monkeypatch):
    monkeypatch.setenv(ROUTE, route)
    a, w, v = _case(case, *dts)
    n = len(a)
    amp = _amp(dts[0])
    W, psi = _operands(qil, a, w, False, amp)
    for k in (1, min(16, 2 ** n), min(100, 2 ** n)):
        rows, vals, bound, cert = qil.apply_top_k(W, psi, k, beam=2 ** n, bits=True)
        order = np.argsort(-np.abs(v), kind="stable")
        mag = np.abs(v[order[:k + 1]])
        assert np.all(mag[:-1] - mag[1:] > GAP * mag[:-1])                     # the dense order is decided
        assert bound == 0.0 and cert
        assert np.array_equal(_index(rows), order[:k])
        assert np.abs(vals - amp * v[order[:k]]).max() <= 1e-10 * np.abs(amp * v).max()


# ---------------------------------------------------------------- 3. soundness
@pytest.mark.parametrize("route", ROUTES)
def test_bound_soundness_fuzz(qil, route, monkeypatch):
    monkeypatch.setenv(ROUTE, route)
    rng = np.random.default_rng(2025)
    n, certified = 8, 0
    for trial in range(40):
        cap = int(rng.choice([2, 3, 4, 6]))
        chi = [int(rng.integers(1, cap + 1)) for _ in range(n - 1)]
        D = [int(rng.integers(1, cap + 1)) for _ in range(n - 1)]
        dta, dtw = DT_PAIRS[trial % 4]
        a, w = random_mps_data(chi, rng, dta), random_mpo_data(D, rng, dtw)
        if trial % 3 == 0:                               # a peaked state: one heavy configuration on top of the noise
            for A in a:
                A[:, 0, :] *= 3.0
        v = 1.7 * apply_dense(w, a)
        k = int(rng.integers(1, 9))
        beam = int(rng.integers(k, 65)) if trial % 2 else k + int(rng.integers(0, 4))    # wide beams certify, tight ones rarely
        W, psi = _operands(qil, a, w, False, 1.7)
        rows, vals, bound, cert = qil.apply_top_k(W, psi, k, beam=beam, bits=True)
        idx = _index(rows)
        assert len(set(idx.tolist())) == k
        assert np.abs(vals - v[idx]).max() <= 1e-10 * np.abs(v).max()
        assert np.all(np.diff(np.abs(vals)) <= 0) and bound >= 0.0
        rest = np.delete(np.abs(v), idx)
        assert rest.size == 0 or rest.max() <= max(bound, np.abs(vals[-1])) * (1 + 1e-9), trial
        assert cert == bool(bound < np.abs(vals[-1]) * (1.0 - SLACK))
        if cert:
            certified += 1
            assert rest.size == 0 or rest.max() <= np.abs(vals[-1]) * (1 + 1e-9), trial       # the set is the exact top-k
    assert 10 <= certified <= 30, certified                                      # both outcomes occur (the oracle: 25 of 40)


# ---------------------------------------------------------------- 4. against the materialised route
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
@pytest.mark.parametrize("case", ["sat", "tile65"])
def test_lazy_search_is_the_search_on_the_formed_product(qil, case, dts, route, monkeypatch):
    monkeypatch.setenv(ROUTE, route)
    a, w, v = _case(case, *dts)
    W, psi = _operands(qil, a, w, False, _amp(dts[0]))
    prod = qil.apply(W, psi)
    for k, beam in K_BEAM:
        idx, vals, bound, gap, ogap = _oracle(case, *dts, k, beam)
        assert gap > GAP and ogap > GAP
        rows, lv, lb, lc = qil.apply_top_k(W, psi, k, beam=beam, bits=True)
        frows, fv, fb, fc = qil.top_k(prod, k, beam=beam, bits=True)
        assert np.array_equal(rows, frows) and lc == fc
        assert np.all(np.abs(lv - fv) <= 1e-10 * np.abs(fv))
        assert (lb == 0.0 and fb == 0.0) or abs(lb - fb) <= 1e-9 * fb
    del prod


# ---------------------------------------------------------------- 5. a frontier across the row-step chunk
@functools.lru_cache(maxsize=None)
def _wide_case(seed):
    rng = np.random.default_rng(seed)
    chi, D = [2] + [3] * 14 + [2], [2] * 16
    a = random_mps_data(chi, rng, F)
    w = random_mpo_data(D, rng, Z)
    v = product_dense(w, a)
    return chi, D, a, w, oracle_top_k(v, 16, 40000, 1.7), np.abs(1.7 * v).max()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("seed", [41017, 41018])
def test_frontier_across_the_row_step_chunk(qil, seed, route, monkeypatch):
    """17 tensors, beam 40000: the frontier grows to 32768 rows, then 40000 = 32768 + 7232 (two chunks of the row step), with
    real cuts at the last two levels (65536 -> 40000 and 80000 -> 16)."""
    monkeypatch.setenv(ROUTE, route)
    chi, D, a, w, want, scale = _wide_case(seed)
    assert _chunk(chi, D, 40000, 16) == 32768 and 40000 <= _beam_cap(chi, D, 16)
    print(f"seed {seed}: cut gap {want[3]:.1e}, order gap {want[4]:.1e}, bound {want[2]:.3e}, |value_k| {abs(want[1][-1]):.3e}")
    got = qil.apply_top_k(qil.SingleSiteMPO(w), qil.SignalMPS(a, amplitude=1.7), 16, beam=40000, bits=True)
    _check_against_oracle(got, want, scale)
    assert got[3]                                                               # certified: the kept set is the exact top 16


# ---------------------------------------------------------------- 6. mid size, no dense vector
@pytest.mark.parametrize("route", ROUTES)
def test_mid_size_values_are_the_lazy_coefficients(qil, route, monkeypatch):
    """24 paired tensors, chi <= 8, D <= 6, beam 4096."""
    monkeypatch.setenv(ROUTE, route)
    psi = qil.ZTMPS.alloc(saturated_profile(24, 8), dtype=Z, amplitude=2.5).fill_random(20241120)
    W = qil.PairedSiteMPO.alloc(saturated_profile(24, 6, 4), dtype=Z).fill_random(20241121)
    r1 = qil.apply_top_k(W, psi, 16, beam=4096, bits=True)
    rows, vals, bound, cert = r1
    c = qil.apply_coefficient_batch(W, psi, rows)
    rel = np.abs(vals - c) / np.abs(c)
    print(f"mid-size apply_top_k {route}: worst relative value error {rel.max():.2e}, bound {bound:.3e}, certified {cert}")
    assert rel.max() <= 1e-10, rel.max()
    assert np.all(np.diff(np.abs(vals)) <= 0) and len({tuple(r) for r in rows.tolist()}) == 16
    r2 = qil.apply_top_k(W, psi, 16, beam=4096, bits=True)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and r1[2] == r2[2] and r1[3] == r2[3]


# ---------------------------------------------------------------- 7. structure
def test_qft_tones_are_found_and_certified(qil):
    n = 14
    N = 2 ** n
    tones = [(3, 1.0), (1000, 0.6), (7777, 0.3)]
    psi = qil.exponential_sum([amp for _, amp in tones], [np.exp(2j * np.pi * f / N) for f, _ in tones], n)
    W = qil.build_qft_mpo(psi)
    idx, vals, bound, cert = qil.apply_top_k(W, psi, 3, beam=64)
    vec = qil.mps_to_vector(W * psi)
    want = np.argsort(-np.abs(vec), kind="stable")[:3]
    assert cert, (bound, vals)
    assert list(idx) == list(want)
    np.testing.assert_allclose(vals, vec[want], rtol=1e-9, atol=0)
    # the QFT output holds the bin lsb first: a big-endian index is the tone bit-reversed
    assert sorted(int(format(int(i), f"0{n}b")[::-1], 2) for i in idx) == [3, 1000, 7777]


@pytest.mark.parametrize("j", [0, 1, 2 ** 10 - 1, 357])
def test_basis_state_through_the_identity_returns_itself(qil, j):
    eye = [np.eye(2).reshape(1, 2, 2, 1) for _ in range(10)]
    psi = qil.SignalMPS(basis_mps(j, 10).data, amplitude=2.0)
    idx, vals, bound, cert = qil.apply_top_k(qil.SingleSiteMPO(eye), psi, 1, beam=4)
    assert idx.tolist() == [j] and vals[0] == pytest.approx(2.0, rel=1e-14) and bound == 0.0 and cert


# ---------------------------------------------------------------- 8. scale
def test_large_amplitude_neither_overflows_nor_underflows(qil):
    amp = float(np.exp(157.0))
    psi = qil.ZTMPS.alloc(saturated_profile(48, 8), dtype=Z, amplitude=amp).fill_random(7)
    W = qil.PairedSiteMPO.alloc(saturated_profile(48, 4, 4), dtype=Z).fill_random(8)
    rows, vals, bound, cert = qil.apply_top_k(W, psi, 8, beam=256, bits=True)
    assert np.all(np.isfinite(vals)) and np.all(np.abs(vals) > 0) and np.isfinite(bound) and bound > 0
    prod = qil.apply(W, psi)
    frows, fv, fb, fc = qil.top_k(prod, 8, beam=256, bits=True)
    del prod
    assert np.array_equal(rows, frows)
    assert np.all(np.abs(vals - fv) <= 1e-10 * np.abs(fv))
    assert abs(bound - fb) <= 1e-9 * fb and cert == fc


# ---------------------------------------------------------------- 9. errors and edges
def test_errors_and_edge_cases(qil, monkeypatch):
    L = importlib.import_module("qilaplace_jl_amd._lib")
    a, w, v = _case("sat", F, Z)
    n = len(a)
    chi, D = PROFILES["sat"]
    ctx = qil.default_context()
    W, psi = qil.SingleSiteMPO(w), qil.SignalMPS(a)
    # k = 0 leaves the outputs untouched
    bits = np.full((2, n), 9, dtype=np.uint8)
    vals = np.full(4, -7.0)
    bound = C.c_double(-3.0)
    out = (bits.ctypes.data_as(C.POINTER(C.c_uint8)), vals.ctypes.data_as(C.POINTER(C.c_double)), C.byref(bound))
    assert L.lib.qil_apply_top_k(W.handle, psi.handle, 0, 0, *out) == L.QIL_OK
    assert L.lib.qil_apply_top_k(W.handle, psi.handle, 0, 5, None, None, None) == L.QIL_OK
    assert np.all(bits == 9) and np.all(vals == -7.0) and bound.value == -3.0
    idx, vs, b, cert = qil.apply_top_k(W, psi, 0, beam=0)
    assert idx.shape == (0,) and vs.shape == (0,) and b == 0.0 and cert
    assert qil.apply_top_k(W, psi, 0, bits=True)[0].shape == (0, n)
    # the library's own checks, behind the front-end's
    assert L.lib.qil_apply_top_k(W.handle, psi.handle, 5, 4, *out) == L.QIL_EINVAL_ARG and "beam 4 below k 5" in L.last_error()
    assert L.lib.qil_apply_top_k(W.handle, psi.handle, 2 ** n + 1, 2 ** n + 1, *out) == L.QIL_EINVAL_ARG
    assert "configurations" in L.last_error()
    assert L.lib.qil_apply_top_k(W.handle, psi.handle, 1, 4, None, *out[1:]) == L.QIL_EINVAL_ARG
    assert "apply_top_k: null argument" in L.last_error()
    with pytest.raises(ValueError, match="at least k"):
        qil.apply_top_k(W, psi, 5, beam=4)
    with pytest.raises(ValueError, match="configurations"):
        qil.apply_top_k(W, psi, 2 ** n + 1, beam=2 ** n + 1)
    cap = _beam_cap(chi, D, 16)
    assert cap == 2 ** 30 // (3 * 48 * 16 + 4 * 10 + 64)
    with pytest.raises(ValueError, match=f"above the cap {cap}"):
        qil.apply_top_k(W, psi, 1, beam=cap + 1)
    assert np.all(bits == 9) and np.all(vals == -7.0) and bound.value == -3.0
    # the environment budget is apply_sample's
    need = 16 * sum((c * d) ** 2 for c, d in zip(chi, D))
    monkeypatch.setenv(RENV, str(need - 1))
    ctx.fail_alloc_after(0)                              # an allocation in front of the check would fail with the pool's message
    try:
        with pytest.raises(MemoryError, match=f"apply_top_k: the right environments need {need} bytes"):
            qil.apply_top_k(W, psi, 3, beam=16)
    finally:
        ctx.fail_alloc_after(None)
    assert ctx.unowned_bytes() == 0
    monkeypatch.setenv(RENV, str(need))                  # exactly what is needed passes
    assert qil.apply_top_k(W, psi, 3, beam=16, bits=True)[0].shape == (3, n)
    monkeypatch.delenv(RENV)
    # a zero state
    for t in (0, 4, n - 1):
        zero = [x.copy() for x in w]
        zero[t][:] = 0
        with pytest.raises(qil.QilDomainError, match="apply_top_k: the transformed state has zero norm"):
            qil.apply_top_k(qil.SingleSiteMPO(zero), qil.SignalMPS(a), 3, beam=16)
    # the operand errors of apply
    rng = np.random.default_rng(71)
    a8, a7 = random_mps_data([2] * 7, rng), random_mps_data([2] * 6, rng)
    w8 = random_mpo_data([2] * 7, rng)
    with pytest.raises(ValueError, match="same number of sites"):
        qil.apply_top_k(qil.SingleSiteMPO(w8), qil.SignalMPS(a7), 4)
    with pytest.raises(ValueError, match="same site indices"):
        qil.apply_top_k(qil.SingleSiteMPO(w8, sites=list(range(11, 19))), qil.SignalMPS(a8), 4)
    with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
        qil.apply_top_k(qil.PairedSiteMPO(w8), qil.SignalMPS(a8), 4)


@pytest.mark.parametrize("route", ROUTES)
def test_single_tensor_chain(qil, route, monkeypatch):
    monkeypatch.setenv(ROUTE, route)
    A = np.array([0.25, -1.5]).reshape(1, 2, 1)
    M = np.array([[0.5, -2.0], [1.0, 0.25]])                                  # M[s_in, s_out]
    W, psi = qil.SingleSiteMPO([M.reshape(1, 2, 2, 1)]), qil.SignalMPS([A], amplitude=3.0)
    y = 3.0 * np.array([0.25 * 0.5 - 1.5 * 1.0, 0.25 * -2.0 - 1.5 * 0.25])      # amp (W psi)[s_out] by hand: -4.125, -2.625
    idx, vals, bound, cert = qil.apply_top_k(W, psi, 2, beam=2)
    assert idx.tolist() == [0, 1] and np.allclose(vals, y, rtol=1e-14, atol=0) and bound == 0.0 and cert
    idx, vals, bound, cert = qil.apply_top_k(W, psi, 1, beam=1)
    assert idx.tolist() == [0] and np.allclose(vals, y[:1], rtol=1e-14, atol=0) and bound == 0.0 and cert


# ---------------------------------------------------------------- 10. allocation failures
@pytest.mark.parametrize("route", ROUTES)
def test_failed_calls_leave_no_device_memory_behind(qil, route, monkeypatch):
    monkeypatch.setenv(ROUTE, route)
    a, w, v = _case("odd", F, Z)
    ctx = qil.default_context()
    W, psi = _operands(qil, a, w, False, _amp(F))
    ref = qil.apply_top_k(W, psi, 7, beam=37, bits=True)
    failures, got = 0, None
    for j in range(0, 400):
        ctx.fail_alloc_after(j)
        try:
            got = qil.apply_top_k(W, psi, 7, beam=37, bits=True)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, j
        if not failed:
            break
        failures += 1
    assert got is not None and failures >= 20, failures
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2] and got[3] == ref[3]
    _check_against_oracle(got, _oracle("odd", F, Z, 7, 37), np.abs(_amp(F) * v).max())
    assert all(np.array_equal(psi.site(i), a[i]) for i in range(len(a)))
    assert all(np.array_equal(W.site(i), w[i]) for i in range(len(w)))


# ---------------------------------------------------------------- 11. the example
def test_lazy_top_k_example_checks_itself(qil, capsys):
    """examples/lazy_top_k.py asserts what it prints against the materialised product; run in this process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lazy_top_k", os.path.join(root, "examples", "lazy_top_k.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tones, certified = mod.main()
    assert tones == [250, 1250, 3000] and certified
    assert "certified" in capsys.readouterr().out
