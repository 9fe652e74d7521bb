"""GPU tests of the operator read-outs: qil.mpo_entry_batch / mpo_slice and the front-ends on top of them (mpo_entries,
mpo_to_matrix, mpo_column, mpo_row, mpo_diagonal_state).

The reference is tests/mpo_slice_cases.reference_slice: numpy on the dense 2n-leg tensor in longdouble (pinned against
helpers.dense_mpo by tests/test_mpo_slice_cases_model.py).  Tolerances: read-outs 1e-12 of the reference's largest entry -- for
numbers the largest among the rows of the same kind (pure entries, rows with sums, rows with traces), so that a large summed row
cannot hide an error in a small entry; 1e-12 is the project's read-out tolerance (test_gpu_restrict.py, test_gpu_parity.py), a
double-precision chain over these profiles stays within 1.4e-15 of longdouble.  Kept tensors that absorb nothing are EQUAL to
the numpy gather; integer-valued operands give the exact integer.  The bond profiles cover bond 1, bonds that are no multiple of
4 or 16, the LDS limits of the run kernel (64 for c64, 96 for f64), a profile on both sides of both (one call mixes the routes)
and, for the entries, one bond above the cap of the one-launch route."""
import ctypes as C
import importlib

import numpy as np
import pytest

from helpers import dense_mpo, random_mpo_data, random_mps_data, saturated_profile
import mpo_slice_cases as MC
from mpo_slice_cases import FIX0, FIX1, SUM, FREE, TIE, DIAG, reference_slice

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["f64", "c64"])
PAIRED = pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    assert (q.ops.FIX0, q.ops.FIX1, q.ops.SUM, q.ops.FREE, q.ops.TIE, q.ops.DIAG) == (FIX0, FIX1, SUM, FREE, TIE, DIAG)
    return q


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("qilaplace_jl_amd._lib")


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    assert qil.default_context().unowned_bytes() == 0


def _mpo(qil, data, paired, sites=None):
    return (qil.PairedSiteMPO if paired else qil.SingleSiteMPO)(data, sites=sites)


def _ids(case, n):
    return [int(v) for v in np.random.default_rng(len(case)).permutation(1000)[:n]]      # non-default site ids


def _scale(t):
    return max(np.abs(t).max(), 1e-300)


_ENTRY_REF = {}


def _entry_reference(case, dt):
    """(specs, kinds, reference) of a profile: computed once, shared by the routes and the pairings, never modified"""
    key = (case, dt == np.complex128)
    if key not in _ENTRY_REF:
        data, dense = MC.case_data(*key)
        rng = np.random.default_rng(2750 + sorted(MC.ENTRY_PROFILES).index(case))
        specs, kinds = MC.entry_rows(len(data), rng)
        _ENTRY_REF[key] = (specs, kinds, MC.reference_entries(data, dense, specs))
    return _ENTRY_REF[key]


def _raw_entries(L, W, specs):
    sp = np.ascontiguousarray(specs, dtype=np.uint8)
    out = np.full(len(sp), np.nan + 1j * np.nan)
    L.check(L.lib.qil_mpo_entry_batch(W.handle, len(sp), sp.ctypes.data_as(L._pu8), out.ctypes.data_as(L._pdbl)))
    return out


# ---------------------------------------------------------------- 1. entries
ENTRY_CASES = [(c, r) for c in sorted(MC.PROFILES) for r in ("chain", "gemm")] + [(c, "auto") for c in sorted(MC.ENTRY_ONLY_PROFILES)]


@DTYPES
@PAIRED
@pytest.mark.parametrize("case,route", ENTRY_CASES, ids=[f"{c}-{r}" for c, r in ENTRY_CASES])
def test_entries_match_the_reference(qil, L, monkeypatch, case, route, paired, dt):
    data, _ = MC.case_data(case, dt == np.complex128)
    specs, kinds, ref = _entry_reference(case, dt)
    W = _mpo(qil, data, paired, _ids(case, len(data)))
    if route == "auto":
        monkeypatch.delenv("QIL_MPO_ENTRY_ROUTE", raising=False)
    else:
        monkeypatch.setenv("QIL_MPO_ENTRY_ROUTE", route)
    got = qil.mpo_entry_batch(W, specs)
    assert got.shape == (len(specs),) and got.dtype == dt
    for kind, name in ((MC.ENTRY, "entries"), (MC.SUMS, "sums"), (MC.TRACES, "traces")):
        sel = kinds == kind
        err = np.abs(got[sel] - ref[sel]).max() / _scale(ref[sel])
        print(f"mpo_entry_batch {case} {route} paired={paired} {np.dtype(dt).name} {name}: worst deviation {err:.2e} of scale")
        assert err <= 1e-12, (case, route, name, err)
    if dt == np.float64:                                             # a real operator: the imaginary part is the constant 0
        raw = _raw_entries(L, W, specs)
        assert np.all(raw.imag == 0.0) and not np.any(np.signbit(raw.imag)) and np.array_equal(raw.real, got)


@DTYPES
@pytest.mark.parametrize("case", MC.SMALLEST)
def test_the_whole_matrix_matches_the_dense_operator(qil, case, dt):
    data, _ = MC.case_data(case, dt == np.complex128)
    M = dense_mpo(data)
    got = qil.mpo_to_matrix(qil.SingleSiteMPO(data))
    assert got.shape == M.shape and got.dtype == M.dtype
    assert np.abs(got - M).max() <= 1e-12 * _scale(M)
    W = qil.SingleSiteMPO(data)
    n = len(data)
    # the front-ends for one entry and for a few: other batch sizes, possibly the other route
    assert abs(qil.mpo_entry(W, 5, "1" * n) - M[5, 2 ** n - 1]) <= 1e-12 * _scale(M)
    assert np.abs(qil.mpo_entries(W, [3, 9], np.array([0, 7, 11])) - M[[3, 9]][:, [0, 7, 11]]).max() <= 1e-12 * _scale(M)


def test_no_rows_is_a_no_op(qil):
    W = qil.SingleSiteMPO(MC.case_data("bond1", False)[0])
    out = qil.mpo_entry_batch(W, np.zeros((0, 6, 2), dtype=np.uint8))
    assert out.shape == (0,) and out.dtype == np.float64


# ---------------------------------------------------------------- 2. entry exactness
def _integer_chain(rng, n, complex_):
    dims = [1] + [int(v) for v in rng.integers(2, 5, n - 1)] + [1]
    re = [rng.integers(-1, 2, (dims[i], 2, 2, dims[i + 1])) for i in range(n)]
    im = [rng.integers(-1, 2, r.shape) if complex_ else np.zeros_like(r) for r in re]
    return re, im


def _int64_entry(re, im, spec):
    """prod_i S_i in Gaussian integers (int64 parts), the slices of a factor added as the spec says"""
    vr, vi = np.ones((1, 1), dtype=np.int64), np.zeros((1, 1), dtype=np.int64)
    for i, (a, b) in enumerate(spec):
        terms = [(0, 0), (1, 1)] if a == TIE else [(x, y) for y in ([b] if b < 2 else [0, 1]) for x in ([a] if a < 2 else [0, 1])]
        sr = sum(re[i][:, x, y, :] for x, y in terms)
        si = sum(im[i][:, x, y, :] for x, y in terms)
        vr, vi = vr @ sr - vi @ si, vr @ si + vi @ sr
    return int(vr[0, 0]), int(vi[0, 0])


@DTYPES
def test_integer_operands_give_the_exact_integer_on_both_routes(qil, L, monkeypatch, dt):
    cx = dt == np.complex128
    rng = np.random.default_rng(2760 + cx)
    re, im = _integer_chain(rng, 10, cx)
    W = qil.SingleSiteMPO([(r + 1j * i).astype(dt) if cx else r.astype(dt) for r, i in zip(re, im)])
    specs, _ = MC.entry_rows(10, rng)
    want = np.array([complex(*_int64_entry(re, im, [(int(a), int(b)) for a, b in s])) for s in specs])
    assert np.abs(want).max() < 2.0 ** 40 and np.count_nonzero(want) > len(want) // 2      # far below 2^53, and not a table of zeros
    for route in ("chain", "gemm"):
        monkeypatch.setenv("QIL_MPO_ENTRY_ROUTE", route)
        assert np.array_equal(_raw_entries(L, W, specs), want), route


@DTYPES
def test_a_chain_row_does_not_depend_on_its_batch(qil, L, monkeypatch, dt):
    data, _ = MC.case_data("sat96", dt == np.complex128)
    specs, _, _ = _entry_reference("sat96", dt)
    W = qil.SingleSiteMPO(data)
    monkeypatch.setenv("QIL_MPO_ENTRY_ROUTE", "chain")
    batch = _raw_entries(L, W, specs)
    again = _raw_entries(L, W, specs)
    assert len(specs) == 300 and np.array_equal(batch.view(np.float64), again.view(np.float64))
    for r in (0, 57, 100, 199, 200, 299):
        alone = _raw_entries(L, W, specs[r:r + 1])
        assert np.array_equal(alone.view(np.float64), batch[r:r + 1].view(np.float64)), r
    perm = np.random.default_rng(5).permutation(300)
    assert np.array_equal(_raw_entries(L, W, specs[perm]).view(np.float64), batch[perm].view(np.float64))


# ---------------------------------------------------------------- 3. slices
def _check_metadata(qil, W, out, spec, paired, dt):
    kept = MC.kept_positions(spec)
    want = qil.ZTMPS if paired and MC.whole_pairs(spec) else qil.SignalMPS
    assert type(out) is want and out.paired == (want is qil.ZTMPS)
    assert out.site_ids == [W.site_ids[i] for i in kept]
    assert out.bond_dims == [W.bond_dims[i] for i in kept[:-1]]            # the parent's right bonds of the kept sites
    assert out.dtype == dt and out.amplitude == 1.0


@DTYPES
@PAIRED
@pytest.mark.parametrize("case", sorted(MC.PROFILES))
def test_slices_match_the_reference(qil, case, paired, dt):
    data, dense = MC.case_data(case, dt == np.complex128)
    n = len(data)
    rng = np.random.default_rng(2770 + sorted(MC.PROFILES).index(case) * 4 + 2 * paired + (dt == np.complex128))
    W = _mpo(qil, data, paired, _ids(case, n))
    worst, forms = 0.0, set()
    for name, spec in MC.slice_specs(n, rng).items():
        out = qil.mpo_slice(W, spec)
        _check_metadata(qil, W, out, spec, paired, dt)
        ref = reference_slice(data, spec, dense)
        got = qil.mps_to_vector(out)
        assert got.shape == ref.shape and got.dtype == dt, name
        err = np.abs(got - ref).max() / _scale(ref)
        worst = max(worst, float(err))
        assert err <= 1e-12, (case, name, err)
        forms |= {tuple(int(v) for v in row) for row in spec}
    assert set(MC.REMOVED_FORMS) <= forms and set(MC.KEPT_FORMS) <= forms
    print(f"mpo_slice {case} paired={paired} {np.dtype(dt).name}: worst deviation {worst:.2e} of scale")


def test_result_type_follows_the_pairing_rule(qil):
    data, _ = MC.case_data("odd", False)
    ids = [11, 12, 21, 22, 31, 32, 41, 42]
    K, R = (1, FREE), (SUM, 0)
    cases = [([K, K, R, R, K, K, R, R], True),          # pairs 0 and 2 kept whole
             ([R, R, K, K, K, K, R, R], True),
             ([K, R, K, R, K, R, K, R], False),         # main sites only
             ([R, K, K, R, R, R, K, K], False),         # sites 1, 2 are no (main, copy) pair
             ([K, K, K, R, R, R, R, R], False),         # an odd number
             ([K] * 8, True)]
    zt, plain = qil.PairedSiteMPO(data, sites=ids), qil.SingleSiteMPO(data, sites=ids)
    for spec, pairs in cases:
        spec = np.array(spec, dtype=np.uint8)
        out = qil.mpo_slice(zt, spec)
        assert type(out) is (qil.ZTMPS if pairs else qil.SignalMPS), spec
        _check_metadata(qil, zt, out, spec, True, np.float64)
        out = qil.mpo_slice(plain, spec)
        assert type(out) is qil.SignalMPS
        _check_metadata(qil, plain, out, spec, False, np.float64)


# ---------------------------------------------------------------- 4. slice exactness
def _numpy_gather(w, form):
    a, b = form
    if a == DIAG:
        return np.stack([w[:, 0, 0, :], w[:, 1, 1, :]], axis=1)
    if a == FREE:
        return w[:, :, b, :] if b < 2 else w[:, :, 0, :] + w[:, :, 1, :]
    return w[:, a, :, :] if a < 2 else w[:, 0, :, :] + w[:, 1, :, :]


@DTYPES
@pytest.mark.parametrize("case", ["odd", "straddle"])
def test_a_tensor_that_absorbs_nothing_is_the_gather_of_the_slices(qil, case, dt):
    data, _ = MC.case_data(case, dt == np.complex128)
    n = len(data)
    W = qil.SingleSiteMPO(data)
    for shift in range(len(MC.KEPT_FORMS)):                           # every tensor meets every kept form
        spec = np.array([MC.KEPT_FORMS[(i + shift) % len(MC.KEPT_FORMS)] for i in range(n)], dtype=np.uint8)
        out = qil.mpo_slice(W, spec)
        assert len(out) == n and out.bond_dims == W.bond_dims
        for i in range(n):
            assert np.array_equal(out.site(i), _numpy_gather(data[i], tuple(spec[i]))), (shift, i)
    # one interior run: only the tensor on its right changes
    spec = np.array([MC.KEPT_FORMS[i % len(MC.KEPT_FORMS)] for i in range(n)], dtype=np.uint8)
    spec[2], spec[3] = (SUM, 1), (TIE, TIE)
    out = qil.mpo_slice(W, spec)
    for j, i in enumerate(k for k in range(n) if k not in (2, 3)):
        if i != 4:
            assert np.array_equal(out.site(j), _numpy_gather(data[i], tuple(spec[i]))), i


@DTYPES
@PAIRED
def test_the_diagonal_of_a_diagonal_operator_is_the_state(qil, paired, dt):
    rng = np.random.default_rng(2780 + 2 * paired + (dt == np.complex128))
    data = random_mps_data([2, 3, 5, 7, 5, 3, 2], rng, dt)
    psi = (qil.ZTMPS if paired else qil.SignalMPS)(data, sites=list(range(40, 48)))
    back = qil.mpo_diagonal_state(qil.diagonal_mpo(psi))
    assert type(back) is type(psi) and back.site_ids == psi.site_ids and back.bond_dims == psi.bond_dims
    assert back.amplitude == 1.0 and back.dtype == dt
    for i in range(8):
        assert np.array_equal(back.site(i), data[i]), i


@DTYPES
def test_two_calls_give_identical_tensors(qil, dt):
    """on the profile that mixes the routes: in-place runs, LDS runs and GEMM runs in one call"""
    data, _ = MC.case_data("straddle", dt == np.complex128)
    W = qil.SingleSiteMPO(data)
    specs = MC.slice_specs(len(data), np.random.default_rng(2790))
    for name in ("several", "both", "random", "only_middle", "trailing"):
        a, b = qil.mpo_slice(W, specs[name]), qil.mpo_slice(W, specs[name])
        assert a.bond_dims == b.bond_dims
        for i in range(len(a)):
            assert np.array_equal(a.site(i), b.site(i)), (name, i)


# ---------------------------------------------------------------- 5. against the project's own verbs
def _basis(qil, bits, sites=None, paired=False):
    data = []
    for b in bits:
        A = np.zeros((1, 2, 1))
        A[0, int(b), 0] = 1.0
        data.append(A)
    return (qil.ZTMPS if paired else qil.SignalMPS)(data, sites=sites)


def test_qft_entries_and_columns_at_24_sites(qil):
    """no dense operator, no mps_to_vector: the 64 (in, out) pairs -- and all 64 x 64 combinations of them -- against the lazy
    read-out of W on a basis state, through mpo_entries in both forms of its arguments, mpo_entry_batch and mpo_column"""
    n = 24
    W = qil.build_qft_mpo(n)
    rng = np.random.default_rng(2800)
    ins, outs = rng.integers(0, 2, (64, n)).astype(np.uint8), rng.integers(0, 2, (64, n)).astype(np.uint8)
    ref = np.stack([qil.apply_coefficient_batch(W, _basis(qil, b, W.site_ids), outs) for b in ins])     # ref[r, c]: in r, out c
    pairs = np.diagonal(ref)
    tol = 1e-12 * 2.0 ** -12
    table = qil.mpo_entries(W, ins, outs)
    assert table.shape == (64, 64) and table.dtype == np.complex128
    assert np.abs(np.diagonal(table) - pairs).max() <= tol and np.abs(table - ref).max() <= tol
    one_by_one = np.array([qil.mpo_entries(W, ins[r:r + 1], outs[r:r + 1])[0, 0] for r in range(64)])
    assert np.abs(one_by_one - pairs).max() <= tol
    weights = 2 ** np.arange(n - 1, -1, -1, dtype=np.int64)                 # the same configurations as integers, site 1 first
    assert np.abs(qil.mpo_entries(W, ins.astype(np.int64) @ weights, outs.astype(np.int64) @ weights) - ref).max() <= tol
    assert np.abs(qil.mpo_entry_batch(W, np.stack([ins, outs], axis=2)) - pairs).max() <= tol
    for r in range(64):
        col = qil.mpo_column(W, ins[r])
        assert type(col) is qil.SignalMPS and len(col) == n and col.site_ids == W.site_ids and col.bond_dims == W.bond_dims
        assert np.abs(qil.coefficient_batch(col, outs) - ref[r]).max() <= tol, r


def test_a_row_is_the_functional_of_one_output(qil):
    n = 12
    W = qil.build_qft_mpo(n)
    rng = np.random.default_rng(2810)
    psi = qil.SignalMPS(random_mps_data(saturated_profile(n, 8), rng, np.complex128), sites=W.site_ids, amplitude=1.5)
    x = qil.mps_to_vector(psi)                                       # the amplitude included
    for k in (0, 1, 1365, 4095):
        bits = qil.ops._msb_bits([k], n)
        row = qil.mpo_row(W, int(k))
        assert type(row) is qil.SignalMPS and row.amplitude == 1.0 and row.site_ids == W.site_ids
        r = qil.mps_to_vector(row)
        want = qil.apply_coefficient_batch(W, psi, bits)[0]
        assert abs(np.dot(r, x) - want) <= 1e-12 * np.linalg.norm(r) * np.linalg.norm(x), k


def test_shift_entries_are_exact_at_40_sites(qil, L):
    n, s = 40, 12345678901
    N = 2 ** n
    W = qil.build_shift_mpo(n, s)
    rng = np.random.default_rng(2820)
    x = rng.integers(0, N, 64)
    msb = qil.ops._msb_bits
    on = np.stack([msb(x, n), msb((x + s) % N, n)], axis=2)                      # M[x, (x + s) mod N] = 1
    off = np.stack([msb(x, n), msb((x + s + 1 + rng.integers(0, N - 1, 64)) % N, n)], axis=2)
    trace = np.full((1, n, 2), TIE, dtype=np.uint8)
    raw = _raw_entries(L, W, np.concatenate([on, off, trace]))
    assert np.all(raw[:64] == 1.0) and np.all(raw[64:] == 0.0)
    assert np.all(qil.mpo_entry_batch(W, on) == 1.0)


@DTYPES
def test_the_traced_row_is_the_trace(qil, dt):
    data, _ = MC.case_data("sat48", dt == np.complex128)
    W = qil.SingleSiteMPO(data)
    n = len(data)
    got = qil.mpo_entry_batch(W, np.full((1, n, 2), TIE, dtype=np.uint8))[0]
    assert abs(got - qil.mpo_trace(W)) <= 1e-12 * qil.mpo_norm(W) * 2.0 ** (n / 2)        # |tr W| <= |I|_F |W|_F


def test_a_column_of_a_paired_operator_is_a_paired_state(qil):
    n = 6
    rng = np.random.default_rng(2830)
    x = rng.standard_normal(2 ** n) * np.exp(-0.05 * np.arange(2 ** n))
    psi = qil.signal_ztmps(x)
    W = qil.build_zt_mpo(psi, 0.7)
    for _ in range(3):
        bits = rng.integers(0, 2, 2 * n)
        col = qil.mpo_column(W, bits)
        assert type(col) is qil.ZTMPS and len(col) == n and col.site_ids == W.site_ids and col.amplitude == 1.0
        ref = qil.apply(W, _basis(qil, bits, W.site_ids, paired=True))
        want = qil.mps_to_vector(ref)
        assert np.abs(qil.mps_to_vector(col) - want).max() <= 1e-12 * _scale(want)


# ---------------------------------------------------------------- 6. failures
def test_native_errors_carry_their_status_and_message(qil, L):
    W = qil.SingleSiteMPO(MC.case_data("bond1", False)[0])
    n = 6
    h = C.c_void_p()
    col = np.stack([np.zeros(n), np.full(n, FREE)], axis=1).astype(np.uint8)

    def slice_(spec):
        sp = np.ascontiguousarray(spec, dtype=np.uint8)
        return L.lib.qil_mpo_slice(W.handle, sp.ctypes.data_as(L._pu8), C.byref(h))

    for edit, msg in ((((2, 1), 6), "spec value 6 of tensor 2 outside [0,5]"), (((3, 0), 4), "tie both legs"),
                      (((3, 1), 5), "tie both legs"), (((1, 0), 3), "tensor 1 keeps both legs: sub-operators are not built")):
        s = col.copy()
        s[edit[0]] = edit[1]
        assert slice_(s) == L.QIL_EINVAL_CONFIG
        assert msg in L.last_error() and h.value is None
    for none_kept in (np.zeros((n, 2)), np.full((n, 2), TIE), np.full((n, 2), SUM)):
        assert slice_(none_kept) == L.QIL_EINVAL_CONFIG
        assert "that number is what mpo_entry_batch returns" in L.last_error() and h.value is None
    assert L.lib.qil_mpo_slice(W.handle, None, C.byref(h)) == L.QIL_EINVAL_ARG and "mpo_slice: null argument" in L.last_error()
    out = np.zeros(3, dtype=np.complex128)

    def entries(spec, nb=3):
        sp = np.ascontiguousarray(spec, dtype=np.uint8)
        return L.lib.qil_mpo_entry_batch(W.handle, nb, sp.ctypes.data_as(L._pu8), out.ctypes.data_as(L._pdbl))

    for value in ((3, 0), (0, 3), (5, 5), (6, 0), (4, 0), (2, 4), (4, 5)):
        s = np.zeros((3, n, 2), dtype=np.uint8)
        s[2, 4] = value
        assert entries(s) == L.QIL_EINVAL_CONFIG
        assert "row 2, tensor 4" in L.last_error()
    assert entries(np.zeros((3, n, 2)), nb=-1) == L.QIL_EINVAL_ARG and "nb must be non-negative" in L.last_error()
    assert L.lib.qil_mpo_entry_batch(W.handle, 3, None, out.ctypes.data_as(L._pdbl)) == L.QIL_EINVAL_ARG
    assert "mpo_entry_batch: null argument" in L.last_error()
    assert np.all(out == 0)
    with pytest.raises(ValueError):
        L.check(L.QIL_EINVAL_CONFIG)


def _until_it_succeeds(ctx, call):
    failures, got = 0, None
    for j in range(200):
        ctx.fail_alloc_after(j)
        try:
            got = call()
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, j
        if not failed:
            break
        failures += 1
    return failures, got


def test_allocation_failure_leaves_nothing_behind(qil, monkeypatch):
    """Fault injection (a host-side refusal by the pool) at every allocation of a GEMM-route entry call and of a slice call that
    takes all three routes: the call raises, nothing is stranded, the operand is intact, the call then succeeds with the same
    result."""
    ctx = qil.default_context()
    data, _ = MC.case_data("straddle", True)
    W = qil.SingleSiteMPO(data)
    specs, _, _ = _entry_reference("straddle", np.complex128)
    monkeypatch.setenv("QIL_MPO_ENTRY_ROUTE", "gemm")
    ref = qil.mpo_entry_batch(W, specs)
    failures, got = _until_it_succeeds(ctx, lambda: qil.mpo_entry_batch(W, specs))
    assert failures >= 5 and np.array_equal(got, ref), failures          # out, the spec, the carry twice, the products
    spec = np.array([MC.KEPT_FORMS[i % len(MC.KEPT_FORMS)] for i in range(len(data))], dtype=np.uint8)
    for j, i in enumerate((0, 1, 3, 5, 6)):       # a leading run in LDS, a run of length 1 in place, a wide run through the GEMM
        spec[i] = MC.REMOVED_FORMS[(3 * j + 4) % len(MC.REMOVED_FORMS)]
    ref = qil.mpo_slice(W, spec)
    failures, got = _until_it_succeeds(ctx, lambda: qil.mpo_slice(W, spec))
    assert failures >= len(ref) + 3, failures                            # the result's tensors and the runs' temporaries
    assert got.bond_dims == ref.bond_dims
    assert all(np.array_equal(got.site(i), ref.site(i)) for i in range(len(ref)))
    assert all(np.array_equal(W.site(i), data[i]) for i in range(len(data)))
