"""GPU tests of the MPS-valued restriction (qil.restrict, zt_row, zt_column, copy_marginal).

The reference is numpy on `helpers.dense_mps(data)`: index the axes of the fixed sites, `sum` the summed ones, keep the rest
(`_dense_slice`).  Tolerances: dense read-outs 1e-12 of the reference's largest entry (the project's read-out tolerance, as in
test_gpu_sum.py and test_gpu_parity.py); tensors that absorb nothing are EQUAL to the parent's; 1e-10 relative at full size (as
the top-k tests).  The bond profiles cover bond 1, bonds that are no multiple of 4 or 16, the LDS limit of the run kernel for
c64 (64), bonds above it (96: the GEMM route for c64, the limit itself for f64) and a profile that straddles the limit for both
dtypes (128 in the middle, small bonds at the ends), so that one call mixes the routes."""
import importlib

import numpy as np
import pytest

from helpers import random_mps_data, saturated_profile, dense_mps

pytestmark = pytest.mark.gpu

FIX0, FIX1, SUM, FREE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    assert (q.ops.FIX0, q.ops.FIX1, q.ops.SUM, q.ops.FREE) == (FIX0, FIX1, SUM, FREE)
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    assert qil.default_context().unowned_bytes() == 0


def _mps(qil, data, paired, amp=1.0, sites=None):
    return (qil.ZTMPS if paired else qil.SignalMPS)(data, sites=sites, amplitude=amp)


def _scale(t):
    return max(np.abs(t).max(), 1e-300)


def _dense_slice(dense, spec):
    """numpy restatement: fixed axes indexed, summed axes summed, the rest kept in order"""
    T = dense
    for i in range(len(spec) - 1, -1, -1):
        if spec[i] == SUM:
            T = T.sum(axis=i)
        elif spec[i] != FREE:
            T = np.take(T, int(spec[i]), axis=i)
    return T


def _whole_pairs(spec):
    kept = [i for i, s in enumerate(spec) if s == FREE]
    return len(kept) % 2 == 0 and all(kept[j] % 2 == 0 and kept[j + 1] == kept[j] + 1 for j in range(0, len(kept), 2))


def _check_metadata(qil, psi, out, spec, paired):
    kept = [i for i, s in enumerate(spec) if s == FREE]
    want = qil.ZTMPS if paired and _whole_pairs(spec) else qil.SignalMPS
    assert type(out) is want and out.paired == (want is qil.ZTMPS)
    assert out.site_ids == [psi.site_ids[i] for i in kept]
    assert out.bond_dims == [psi.bond_dims[i] for i in kept[:-1]]          # the parent's right bonds of the kept sites
    assert out.dtype == psi.dtype and out.amplitude == psi.amplitude


# ---------------------------------------------------------------- 1. dense parity
PROFILES = {
    "bond1": [1] * 7,
    "odd": [2, 3, 5, 7, 5, 3, 2],
    "sat8": saturated_profile(12, 8),
    "sat64": saturated_profile(14, 64),
    "sat96": saturated_profile(16, 96),
    "straddle": saturated_profile(16, 128),
}


def _specs(n, rng):
    """name -> spec for an n-tensor chain (n >= 8)"""
    def keep_all():
        return np.full(n, FREE, dtype=np.uint8)
    out = {}
    s = keep_all(); s[:3] = [FIX1, SUM, FIX0]; out["leading"] = s
    s = keep_all(); s[-3:] = [SUM, FIX1, FIX0]; out["trailing"] = s
    s = keep_all(); s[:2] = [FIX0, FIX1]; s[-2:] = [FIX1, SUM]; out["both"] = s
    s = keep_all(); s[3] = FIX1; out["run1"] = s
    s = keep_all(); s[3:5] = [FIX1, FIX0]; out["run2"] = s
    s = keep_all(); s[1:6] = [FIX0, FIX1, FIX1, SUM, FIX0]; out["run5"] = s
    if n >= 12:
        s = keep_all(); s[1] = SUM; s[3:5] = [FIX0, SUM]; s[6:11] = [FIX1, FIX0, SUM, FIX1, FIX1]; out["runs125"] = s
        s = keep_all(); s[1:3] = [FIX1, FIX0]; s[n // 2 - 1:n // 2 + 1] = [FIX0, FIX1]; s[-2:] = [FIX1, FIX1]; out["far_runs"] = s
    s = keep_all(); s[1::2] = rng.integers(0, 2, n // 2); out["copy_fixed"] = s
    s = keep_all(); s[1::2] = SUM; out["copy_summed"] = s
    s = keep_all(); s[0::2] = rng.integers(0, 2, n // 2); out["main_fixed"] = s
    for name, k in (("only_first", 0), ("only_middle", n // 2), ("only_last", n - 1)):
        s = rng.integers(0, 3, n).astype(np.uint8); s[k] = FREE; out[name] = s
    s = keep_all(); s[2:6] = [FIX0, SUM, FIX1, SUM]; out["alternating"] = s
    s = rng.integers(0, 4, n).astype(np.uint8); s[int(rng.integers(0, n))] = FREE; out["random"] = s
    return out


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["f64", "c64"])
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
@pytest.mark.parametrize("case", sorted(PROFILES))
def test_slices_match_the_numpy_slice(qil, case, paired, dt):
    rng = np.random.default_rng(sorted(PROFILES).index(case) * 4 + 2 * paired + (dt == np.complex128))
    data = random_mps_data(PROFILES[case], rng, dt)
    n = len(data)
    amp = -1.3 if dt == np.complex128 else 1.7                         # a parent amplitude != 1
    ids = [int(v) for v in rng.permutation(1000)[:n]]                  # non-default site ids
    psi = _mps(qil, data, paired, amp, sites=ids)
    dense = dense_mps(data)
    worst = 0.0
    for name, spec in _specs(n, rng).items():
        out = qil.restrict(psi, spec)
        _check_metadata(qil, psi, out, spec, paired)
        ref = amp * _dense_slice(dense, spec).reshape(-1)
        got = qil.mps_to_vector(out) * 1
        assert got.shape == ref.shape and got.dtype == ref.dtype, name
        err = np.abs(got - ref).max() / _scale(ref)
        worst = max(worst, err)
        assert err <= 1e-12, (case, name, err)
    print(f"restrict {case} paired={paired} {np.dtype(dt).name}: worst deviation {worst:.2e} of scale")


# ---------------------------------------------------------------- 2. exactness
@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["f64", "c64"])
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
def test_keeping_every_site_clones_bit_for_bit(qil, paired, dt):
    rng = np.random.default_rng(101 + 2 * paired + (dt == np.complex128))
    data = random_mps_data([2, 3, 5, 7, 5, 3, 2], rng, dt)
    psi = _mps(qil, data, paired, 0.75, sites=list(range(40, 48)))
    out = qil.restrict(psi, [FREE] * 8)
    assert type(out) is type(psi) and out.site_ids == psi.site_ids and out.bond_dims == psi.bond_dims and out.amplitude == 0.75
    for i in range(8):
        assert np.array_equal(out.site(i), data[i]), i


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["f64", "c64"])
def test_only_the_absorbing_tensor_changes(qil, dt):
    """one interior run (sites 4 .. 6 of 12): kept tensor 7 absorbs it, every other kept tensor is a copy"""
    rng = np.random.default_rng(111 + (dt == np.complex128))
    data = random_mps_data(saturated_profile(12, 8), rng, dt)
    psi = qil.SignalMPS(data)
    spec = np.full(12, FREE, dtype=np.uint8)
    spec[4:7] = [FIX1, SUM, FIX0]
    out = qil.restrict(psi, spec)
    kept = [i for i in range(12) if spec[i] == FREE]
    for j, i in enumerate(kept):
        if i == 7:
            M = data[4][:, 1, :] @ (data[5][:, 0, :] + data[5][:, 1, :]) @ data[6][:, 0, :]
            ref = np.tensordot(M, data[7], axes=([1], [0]))
            assert np.abs(out.site(j) - ref).max() <= 1e-14 * 8 * _scale(ref)
        else:
            assert np.array_equal(out.site(j), data[i]), i


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["f64", "c64"])
def test_two_calls_give_identical_tensors(qil, dt):
    """on the profile that mixes the routes: in-place runs, LDS runs and GEMM runs in one call"""
    rng = np.random.default_rng(121 + (dt == np.complex128))
    data = random_mps_data(PROFILES["straddle"], rng, dt)
    psi = qil.SignalMPS(data, amplitude=2.0)
    specs = _specs(16, rng)
    for name in ("far_runs", "runs125", "random", "both"):
        a, b = qil.restrict(psi, specs[name]), qil.restrict(psi, specs[name])
        assert a.bond_dims == b.bond_dims
        for i in range(len(a)):
            assert np.array_equal(a.site(i), b.site(i)), (name, i)


# ---------------------------------------------------------------- 3. metadata
def test_result_type_follows_the_pairing_rule(qil):
    rng = np.random.default_rng(131)
    data = random_mps_data(saturated_profile(8, 4), rng)
    ids = [11, 12, 21, 22, 31, 32, 41, 42]
    zt, plain = qil.ZTMPS(data, sites=ids), qil.SignalMPS(data, sites=ids)
    cases = [([3, 3, 0, 2, 3, 3, 1, 1], True),         # pairs 0 and 2 kept whole
             ([0, 1, 3, 3, 3, 3, 2, 2], True),
             ([3, 0, 3, 1, 3, 2, 3, 0], False),        # main sites only
             ([0, 3, 3, 1, 2, 2, 3, 3], False),        # sites 1, 2 are no (main, copy) pair
             ([3, 3, 3, 0, 1, 2, 0, 0], False),        # an odd number
             ([3, 3, 3, 3, 3, 3, 3, 3], True)]
    for spec, pairs in cases:
        out = qil.restrict(zt, spec)
        assert type(out) is (qil.ZTMPS if pairs else qil.SignalMPS), spec
        _check_metadata(qil, zt, out, spec, True)
        out = qil.restrict(plain, spec)
        assert type(out) is qil.SignalMPS, spec
        _check_metadata(qil, plain, out, spec, False)


# ---------------------------------------------------------------- 4. composition
@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["f64", "c64"])
def test_restrictions_compose(qil, dt):
    rng = np.random.default_rng(141 + (dt == np.complex128))
    n = 14
    data = random_mps_data(saturated_profile(n, 64), rng, dt)
    psi = qil.ZTMPS(data, amplitude=0.6)
    s1 = np.full(n, FREE, dtype=np.uint8)
    s1[[1, 2, 6, 11, 13]] = [FIX1, SUM, FIX0, SUM, FIX1]
    kept1 = np.nonzero(s1 == FREE)[0]
    s2 = np.full(len(kept1), FREE, dtype=np.uint8)
    s2[[0, 3, 4, 8]] = [SUM, FIX1, FIX0, FIX1]
    merged = s1.copy()
    merged[kept1] = s2
    two = qil.restrict(qil.restrict(psi, s1), s2)
    one = qil.restrict(psi, merged)
    assert two.site_ids == one.site_ids and two.bond_dims == one.bond_dims and type(two) is type(one)
    v2, v1 = qil.mps_to_vector(two), qil.mps_to_vector(one)
    assert np.abs(v2 - v1).max() <= 1e-12 * _scale(v1)
    # ... and reading a slice out is a marginal of the parent on the merged bits
    nk = int((merged == FREE).sum())
    b = rng.integers(0, 2, size=(64, nk)).astype(np.uint8)
    bits = np.tile(merged, (64, 1))
    bits[:, merged == FREE] = b
    got = qil.coefficient_batch(one, b)
    ref = qil.marginal_batch(psi, bits)
    assert np.abs(got - ref).max() <= 1e-12 * _scale(ref)


# ---------------------------------------------------------------- 5. conveniences
@pytest.mark.parametrize("n", [4, 5])
def test_conveniences_hold_their_defining_identities(qil, n):
    rng = np.random.default_rng(150 + n)
    N = 2 ** n
    x = rng.standard_normal(N) * np.exp(-0.05 * np.arange(N))
    psi = qil.signal_ztmps(x)
    phi = qil.build_zt_mpo(psi, 0.7) * psi
    lsb = qil.ops._lsb_bits
    ks = np.arange(N)
    grid = qil.coefficient_grid(phi, ks, ks)
    top = _scale(grid)
    for l in range(N):
        row = qil.zt_row(phi, l)
        assert type(row) is qil.SignalMPS and len(row) == n and row.site_ids == phi.site_ids[0::2]
        got = qil.coefficient_batch(row, lsb(ks, n))
        assert np.abs(got - grid[:, l]).max() <= 1e-12 * top, l
        k = (5 * l + 3) % N                                        # ... and the property as stated, point by point
        assert abs(got[k] - qil.coefficient_grid(phi, [k], [l])[0, 0]) <= 1e-12 * top, (k, l)
    for k in range(N):
        col = qil.zt_column(phi, k)
        assert type(col) is qil.SignalMPS and len(col) == n and col.site_ids == phi.site_ids[1::2]
        got = qil.coefficient_batch(col, lsb(ks, n))
        assert np.abs(got - grid[k, :]).max() <= 1e-12 * top, k
        l = (3 * k + 1) % N
        assert abs(got[l] - qil.coefficient_grid(phi, [k], [l])[0, 0]) <= 1e-12 * top, (k, l)
    cm = qil.copy_marginal(phi)
    assert type(cm) is qil.SignalMPS and len(cm) == n and cm.site_ids == phi.site_ids[0::2]
    dt = 0.01
    for sel in (ks, np.array([0, 3, 5, 9])):                     # the dense-block and the marginal route of laplace_values
        ref = qil.laplace_values(phi, sel, dt)
        got = dt * np.sqrt(2.0 ** n) * qil.coefficient_batch(cm, lsb(sel, n))
        assert np.abs(got - ref).max() <= 1e-12 * _scale(ref)


# ---------------------------------------------------------------- 6. errors
def test_bad_specs_raise_value_errors(qil):
    import ctypes as C
    L = importlib.import_module("qilaplace_jl_amd._lib")
    rng = np.random.default_rng(161)
    psi = qil.SignalMPS(random_mps_data([2, 4, 2], rng))
    with pytest.raises(ValueError, match=r"outside \[0,3\]"):
        qil.restrict(psi, [3, 4, 3, 3])
    for none_kept in ([0, 1, 2, 0], [2, 2, 2, 2]):
        with pytest.raises(ValueError, match="coefficient"):
            qil.restrict(psi, none_kept)
    # the library's own checks, behind the front-end's
    h = C.c_void_p()
    for raw, msg in (([3, 4, 3, 3], "spec value 4 outside"), ([0, 1, 2, 0], "keeps no site")):
        sp = (C.c_uint8 * 4)(*raw)
        assert L.lib.qil_mps_restrict(psi.handle, sp, C.byref(h)) == L.QIL_EINVAL_CONFIG
        assert msg in L.last_error() and h.value is None
    with pytest.raises(ValueError):
        L.check(L.QIL_EINVAL_CONFIG)


def test_single_site_chain(qil):
    A = np.array([0.25, -1.5]).reshape(1, 2, 1)
    psi = qil.SignalMPS([A], sites=[77], amplitude=3.0)
    out = qil.restrict(psi, [FREE])
    assert type(out) is qil.SignalMPS and len(out) == 1 and out.site_ids == [77] and out.amplitude == 3.0
    assert np.array_equal(out.site(0), A)


# ---------------------------------------------------------------- 7. allocation failure
def test_allocation_failure_leaves_nothing_behind(qil):
    """Fault injection (a host-side refusal by the pool) at every allocation of a call that takes all three routes: the call
    raises, nothing is stranded, the operand is intact, and the call then succeeds with the same tensors."""
    ctx = qil.default_context()
    rng = np.random.default_rng(171)
    data = random_mps_data(PROFILES["straddle"], rng, np.complex128)
    psi = qil.SignalMPS(data, amplitude=0.5)
    spec = _specs(16, rng)["far_runs"]
    ref = qil.restrict(psi, spec)
    failures, got = 0, None
    for j in range(200):
        ctx.fail_alloc_after(j)
        try:
            got = qil.restrict(psi, spec)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, j
        if not failed:
            break
        failures += 1
    assert got is not None and failures >= len(ref) + 3, failures       # the result's tensors and the runs' temporaries
    assert got.bond_dims == ref.bond_dims
    assert all(np.array_equal(got.site(i), ref.site(i)) for i in range(len(ref)))
    assert all(np.array_equal(psi.site(i), data[i]) for i in range(16)) and psi.amplitude == 0.5


# ---------------------------------------------------------------- 8. full size
def test_full_size_row_against_the_parent(qil):
    """n = 24 paired, chi = 64, c64: 256 seeded coefficients of zt_row against coefficient_batch of the parent on the merged
    bits, 1e-10 relative."""
    n = 24
    psi = qil.ZTMPS.alloc(saturated_profile(2 * n, 64), dtype=np.complex128, amplitude=2.5).fill_random(20241017)
    rng = np.random.default_rng(181)
    l = int(rng.integers(0, 2 ** n))
    row = qil.zt_row(psi, l)
    assert type(row) is qil.SignalMPS and len(row) == n and row.amplitude == 2.5
    assert row.bond_dims == psi.bond_dims[0::2][:-1] and row.site_ids == psi.site_ids[0::2]
    kb = rng.integers(0, 2, size=(256, n)).astype(np.uint8)
    bits = np.empty((256, 2 * n), dtype=np.uint8)
    bits[:, 0::2] = kb
    bits[:, 1::2] = qil.ops._lsb_bits([l], n)[0]
    got = qil.coefficient_batch(row, kb)
    ref = qil.coefficient_batch(psi, bits)
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print(f"full-size zt_row: worst relative deviation {rel.max():.2e}")
    assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref) + 1e-300), rel.max()
