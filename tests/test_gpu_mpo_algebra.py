"""GPU tests of the operator algebra: mpo_linear_combination (qil_mpo_sum) with `+`, `-`, unary `-` and `c *`, mpo_inner
(qil_mpo_inner) on both routes, mpo_norm / mpo_distance / mpo_trace, and build_shift_mpo / fir_mpo on top of them -- on the
table of tests/mpo_algebra_cases.py, with the assertions tests/test_mpo_algebra_model.py makes of the numpy model on the CPU.

Tolerances (the project's): interior and last tensors of a sum EQUAL to the numpy direct sum with +0.0 off the blocks, the first
tensor within 1e-14 of its largest entry; dense read-outs 1e-12 of scale; an overlap within 1e-12 of |V|_F |W|_F, two routes
within 1e-13 of it; overlaps of 0/1 operators with dyadic weights are exact integers; a distance within 1e-7 d + floor / d of
the dense one, floor = 64 eps (|V|^2 + |W|^2) (the floor `mpo_distance` states)."""
import ctypes as C

import numpy as np
import pytest

import mpo_algebra_cases as cases
from helpers import random_mps_data, random_mpo_data, saturated_profile, dense_mpo

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
F, Z = np.float64, np.complex128


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


def _mpo(qil, data, paired, sites=None, ctx=None):
    return (qil.PairedSiteMPO if paired else qil.SingleSiteMPO)([np.array(t) for t in data], sites=sites, ctx=ctx)


def _floor(*norms2):
    """absolute error of a squared distance from the expansion: a few eps times the squared norms involved"""
    return 64 * EPS * sum(norms2)


def _same_sites(a, b):
    return a.bond_dims == b.bond_dims and a.dtype == b.dtype and all(np.array_equal(x, y) for x, y in zip(a.to_host(), b.to_host()))


def _route(monkeypatch, route):
    if route == "auto":
        monkeypatch.delenv("QIL_MPO_INNER_ROUTE", raising=False)
    else:
        monkeypatch.setenv("QIL_MPO_INNER_ROUTE", route)


# ---------------------------------------------------------------- 1. sum sites against the model
@pytest.mark.parametrize("name", [c.name for c in cases.SUMS])
def test_sum_sites_match_the_model(qil, name):
    c = cases.sum_case(name)
    datas, handles, coeffs, ids = cases.sum_operands(name)
    ops = {h: _mpo(qil, datas[h], c.paired, ids) for h in set(handles)}
    terms = [ops[h] for h in handles]
    out = qil.mpo_linear_combination(terms, coeffs)
    assert type(out) is type(terms[0]) and out.site_ids == ids and out.paired == c.paired
    got = out.to_host()
    assert out.dtype == cases.sum_reference(name)[0].dtype
    cases.check_sum_sites(name, got, out.bond_dims)
    err = cases.check_sum_dense(name, got)
    print(f"sum {name}: bonds {out.bond_dims}, dense error {err:.2e} of scale")
    for h in ops:                                                            # the operands are read-only
        assert all(np.array_equal(x, y) for x, y in zip(ops[h].to_host(), datas[h])), (name, h)


def test_null_coefficients_are_ones_and_operators_spell_the_sums(qil):
    rng = np.random.default_rng(51)
    for paired in (False, True):
        v = random_mpo_data([3, 9, 17, 6, 4], rng, Z)
        w = random_mpo_data([2, 5, 13, 7, 3], rng, F)
        V, W = _mpo(qil, v, paired), _mpo(qil, w, paired)
        lc = qil.mpo_linear_combination
        assert _same_sites(lc([V, W]), lc([V, W], [1.0, 1.0]))
        for got, want in ((V + W, lc([V, W], [1, 1])), (V - W, lc([V, W], [1, -1])), (-W, lc([W], [-1.0])), (2j * W, lc([W], [2j])),
                          (qil.mpo_add(W, W), lc([W, W], [1, 1])), (qil.mpo_sub(W, V), lc([W, V], [1, -1])),
                          (qil.mpo_scale(V, 0.5), lc([V], [0.5])), (3 * W, lc([W], [3.0]))):
            assert type(got) is type(V) and _same_sites(got, want)
        assert (-W).dtype == F and (2j * W).dtype == Z and (V + W).dtype == Z
        assert (V + W).bond_dims == [a + b for a, b in zip(V.bond_dims, W.bond_dims)] and (-W).bond_dims == W.bond_dims
        assert np.abs(dense_mpo((V - W).to_host()) - (dense_mpo(v) - dense_mpo(w))).max() <= 1e-12 * cases.scale_of(dense_mpo(v))
        with pytest.raises(TypeError, match="apply: unsupported operand types"):
            W * 2.0
    with pytest.raises(TypeError):
        _mpo(qil, v, False) + _mpo(qil, w, True)


# ---------------------------------------------------------------- 2. the sum acts as a sum
@pytest.mark.parametrize("paired", [False, True])
def test_sum_acts_as_a_sum(qil, paired):
    rng = np.random.default_rng(52 + paired)
    V = _mpo(qil, random_mpo_data([3, 9, 17, 6, 4], rng, Z), paired)
    W = _mpo(qil, random_mpo_data([2, 5, 13, 7, 3], rng, F), paired)
    psi = (qil.ZTMPS if paired else qil.SignalMPS)(random_mps_data([2, 4, 7, 4, 2], rng, Z), amplitude=1.5)
    got = qil.mps_to_vector(qil.apply(V + W, psi))
    v1, v2 = qil.mps_to_vector(qil.apply(V, psi)), qil.mps_to_vector(qil.apply(W, psi))
    top = max(cases.scale_of(v1), cases.scale_of(v2))
    assert np.abs(got - (v1 + v2)).max() <= 1e-12 * top, np.abs(got - (v1 + v2)).max() / top


# ---------------------------------------------------------------- 3. overlap against dense
@pytest.mark.parametrize("name", [c.name for c in cases.INNERS])
def test_overlap_against_dense_on_every_route(qil, monkeypatch, name):
    c = cases.inner_case(name)
    v, w = cases.inner_operands(name)
    V, W = _mpo(qil, v, c.paired), _mpo(qil, w, c.paired)
    got = {}
    for route in cases.ROUTES:                       # bond65 with "chain" forced does not fit the cap: the GEMM route, same value
        _route(monkeypatch, route)
        got[route] = qil.mpo_inner(V, W)
        err = cases.check_inner(name, got[route])
        print(f"overlap {name} [{route}]: {got[route]:.6e}, error {err:.2e} of |V||W|")
        cases.check_inner_agree(name, got[route], np.conj(qil.mpo_inner(W, V)))
    cases.check_inner_agree(name, got["chain"], got["gemm"])
    cases.check_inner_agree(name, got["auto"], got["gemm"])
    want_complex = c.dtypes[0] == Z or c.dtypes[1] == Z
    assert isinstance(got["auto"], complex) == want_complex
    assert all(np.array_equal(x, y) for x, y in zip(V.to_host(), v)) and all(np.array_equal(x, y) for x, y in zip(W.to_host(), w))


# ---------------------------------------------------------------- 4. against verbs that exist, past dense sizes
@pytest.mark.parametrize("paired", [False, True])
def test_norm_matches_the_bond_spectra_norm(qil, paired):
    rng = np.random.default_rng(54 + paired)
    for dt in (F, Z):
        W = _mpo(qil, random_mpo_data(saturated_profile(30, 12, base=4), rng, dt), paired)
        assert len(W) == (15 if paired else 30)
        _, nrm = qil.mpo_bond_spectra(W, return_norm=True)
        got = qil.mpo_norm(W)
        assert abs(got - nrm) <= 1e-12 * nrm, (got, nrm)


@pytest.mark.parametrize("paired", [False, True])
def test_overlap_of_diagonal_operators_is_the_overlap_of_the_states(qil, monkeypatch, paired):
    rng = np.random.default_rng(56 + paired)
    cls = qil.ZTMPS if paired else qil.SignalMPS
    phi = cls(random_mps_data(saturated_profile(30, 12), rng, Z), amplitude=0.8)
    psi = cls(random_mps_data(saturated_profile(30, 9), rng, F), amplitude=-1.7)
    want = qil.inner(phi, psi)
    scale = abs(phi.amplitude * psi.amplitude) * qil.norm(phi) * qil.norm(psi)
    Dphi, Dpsi = qil.diagonal_mpo(phi), qil.diagonal_mpo(psi)                   # the diagonal operator folds the amplitude
    for route in cases.ROUTES:
        _route(monkeypatch, route)
        got = qil.mpo_inner(Dphi, Dpsi)
        assert cases.near(got, want, scale, 1e-12), (route, got, want)


def test_trace_of_the_product_with_the_adjoint_is_the_overlap(qil):
    rng = np.random.default_rng(58)
    for paired in (False, True):
        V = _mpo(qil, random_mpo_data([3, 6, 9, 12, 9, 6, 3], rng, Z), paired)
        W = _mpo(qil, random_mpo_data([2, 5, 8, 11, 8, 5, 2], rng, F), paired)
        want = qil.mpo_inner(V, W)
        got = qil.mpo_trace(qil.apply(qil.adjoint(V), W))
        assert cases.near(got, want, qil.mpo_norm(V) * qil.mpo_norm(W), 1e-12), (got, want)
        eye = type(V).identity(len(V))
        assert qil.mpo_trace(eye) == 2.0 ** 8 and qil.mpo_norm(eye) == 16.0


# ---------------------------------------------------------------- 5. exact integers
@pytest.mark.parametrize("route", ["chain", "gemm"])
def test_shift_overlaps_are_exact_integers_at_n40(qil, monkeypatch, route):
    n = 40
    _route(monkeypatch, route)
    shifts = (0, 1, 5, 2 ** 39)
    S = {s: qil.build_shift_mpo(n, s) for s in shifts}
    assert all(S[s].bond_dims == [2] * (n - 1) and S[s].dtype == F for s in shifts)
    for a in shifts:
        for b in shifts:
            assert qil.mpo_inner(S[a], S[b]) == (2.0 ** n if a == b else 0.0), (route, a, b)
    taps = cases.SHIFT_TAPS
    T = qil.mpo_linear_combination([qil.build_shift_mpo(n, k) for k in taps], list(taps.values()))
    assert T.bond_dims == [6] * (n - 1)
    assert qil.mpo_inner(T, T) == 2.0 ** n * cases.SHIFT_TAPS_NORM2_PER_SAMPLE
    assert qil.mpo_norm(T) == np.sqrt(2.0 ** n * cases.SHIFT_TAPS_NORM2_PER_SAMPLE)


# ---------------------------------------------------------------- 6. distance
def test_distance_to_a_truncated_operator_against_dense(qil):
    rng = np.random.default_rng(60)
    w = random_mpo_data([4, 16, 40, 40, 40, 16, 4], rng, Z)
    W = _mpo(qil, w, False)
    dw = dense_mpo(w)
    n2 = np.linalg.norm(dw) ** 2
    for m in (4, 12, 24):
        Wc = qil.mpo_compress(_mpo(qil, w, False), maxdim=m)                     # in place, on a copy
        assert max(Wc.bond_dims) <= m
        dc = dense_mpo(Wc.to_host())
        d_ref = np.linalg.norm(dw - dc)
        got = qil.mpo_distance(W, Wc)
        bound = 1e-7 * d_ref + _floor(n2, np.linalg.norm(dc) ** 2) / d_ref
        print(f"distance maxdim {m}: {got:.6e} against dense {d_ref:.6e} (|W| = {np.sqrt(n2):.3e}), bound {bound:.2e}")
        assert abs(got - d_ref) <= bound, (m, got, d_ref)
        assert abs(qil.mpo_distance(Wc, W) - d_ref) <= bound
    assert qil.mpo_distance(W, W) <= np.sqrt(_floor(n2, n2))
    assert qil.mpo_distance(W, _mpo(qil, w, False)) <= np.sqrt(_floor(n2, n2))


# ---------------------------------------------------------------- 7. FIR
def test_fir_filter_is_the_circular_convolution(qil):
    n = 8
    rng = np.random.default_rng(61)
    taps = cases.SHIFT_TAPS
    Wf = qil.fir_mpo(taps, n)
    assert type(Wf) is qil.SingleSiteMPO and len(Wf) == n and max(Wf.bond_dims) <= 6, Wf.bond_dims
    x = rng.standard_normal(2 ** n)
    psi = qil.signal_mps(x)
    got = qil.mps_to_vector(qil.apply(Wf, psi))
    want = sum(h * np.roll(x, k) for k, h in taps.items())
    assert np.abs(got - want).max() <= 1e-12 * cases.scale_of(want), np.abs(got - want).max() / cases.scale_of(want)
    # a sequence of taps starts at offset 0; a state supplies n, the sites and the context
    Ws = qil.fir_mpo([0.5, 0.25, 0.0, -0.125], psi)
    assert Ws.site_ids == psi.site_ids
    assert qil.mpo_distance(Wf, Ws) <= 1e-6 * qil.mpo_norm(Wf)
    for s in (1, -3, 37):
        got = qil.mps_to_vector(qil.apply(qil.build_shift_mpo(psi, s), psi))
        assert np.abs(got - np.roll(x, s)).max() <= 1e-12 * cases.scale_of(x)


# ---------------------------------------------------------------- 8. errors and failure paths
def test_operand_mismatches_raise_what_inner_and_linear_combination_raise(qil):
    L = __import__("importlib").import_module("qilaplace_jl_amd._lib")
    rng = np.random.default_rng(62)
    w6 = random_mpo_data([2, 4, 4, 4, 2], rng)
    w4 = random_mpo_data([2, 4, 2], rng)
    W = qil.SingleSiteMPO(w6)
    other = qil.Context()
    pairs = {
        "length": (qil.SingleSiteMPO(w4), L.QIL_EINVAL_LENGTH),
        "sites": (qil.SingleSiteMPO(w6, sites=list(range(11, 17))), L.QIL_EINVAL_SITES),
        "paired": (qil.PairedSiteMPO(w6), L.QIL_EINVAL_ARG),
        "context": (qil.SingleSiteMPO(w6, ctx=other), L.QIL_EINVAL_ARG),
    }
    for what, (bad, code) in pairs.items():
        with pytest.raises(ValueError) as want:                                  # inner raises ValueError for all four
            qil.mpo_inner(W, bad)
        v = (C.c_double * 2)()
        assert L.lib.qil_mpo_inner(W.handle, bad.handle, v) == code, what
        assert L.last_error().startswith("mpo_inner: ")
        # linear_combination: ValueError from the library, TypeError from the front-end for mixed register kinds
        with pytest.raises(TypeError if what == "paired" else ValueError) as got:
            qil.mpo_linear_combination([W, W, bad])
        if what != "paired":
            tail = lambda e: str(e.value).split(": ", 1)[1]
            assert tail(got) == tail(want), what                                 # the same message under the verb's name
            with pytest.raises(ValueError):
                qil.mpo_distance(W, bad)
        arr = (C.c_void_p * 2)(W.handle.value, bad.handle.value)
        h = C.c_void_p()
        assert L.lib.qil_mpo_sum(arr, 2, None, C.byref(h)) == code and h.value is None, what
        assert L.last_error().startswith("mpo_sum: ")
    with pytest.raises(ValueError, match="not finite"):
        qil.mpo_linear_combination([W, W], [1.0, np.nan])
    del bad, pairs
    other.close()


def test_failed_calls_leave_no_device_memory_behind(qil, monkeypatch):
    ctx = qil.default_context()
    rng = np.random.default_rng(63)
    v, w = random_mpo_data([4, 16, 20, 16, 4], rng, Z), random_mpo_data([4, 9, 9, 9, 4], rng, F)
    V, W = qil.SingleSiteMPO(v), qil.SingleSiteMPO(w)
    calls = {"sum": lambda: qil.mpo_linear_combination([V, W, V], [1.0, 2.0, -0.5j]).to_host()}
    for route in ("chain", "gemm"):
        calls[f"inner-{route}"] = lambda: [np.asarray(qil.mpo_inner(V, W))]
    for name, call in calls.items():
        _route(monkeypatch, name.split("-")[1] if "-" in name else "auto")
        ref = call()
        failures, got = 0, None
        for j in range(0, 400):
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
        assert got is not None and failures >= 1, (name, failures)
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), name
    assert all(np.array_equal(x, y) for x, y in zip(V.to_host(), v))
