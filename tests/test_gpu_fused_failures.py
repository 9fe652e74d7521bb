"""GPU tests of the failure paths of the fused truncations (apply_compress, hadamard_compress, linear_combination_compress) and
of signal_ztmps: every pool allocation of a call is made to fail in turn.

After each failed call nothing of it may be left on the device: no unowned block (`unowned_bytes`), and no block owned by a
handle that died with the call either -- `pool_in_use` is back at its value before the call, which a leaked intermediate
handle (the gauged copy of a state, the temporary operator of hadamard_compress) would raise without `unowned_bytes` seeing it.
The operands are untouched, and the first call that is allowed all its allocations returns bit for bit what the undisturbed
call returns.  No tolerances: every comparison is equality.

Every case has 6 sites and bonds <= 8.  The number of failing calls, printed per case, is the number of pool allocations the
call makes before its last one; it is at least the number of sites (the gauged copy alone takes one block per site, and the
encoder behind signal_ztmps more than one per site)."""
import numpy as np
import pytest

from helpers import random_mps_data, random_mpo_data, saturated_profile

pytestmark = pytest.mark.gpu

SITES = 6


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


def _same_state(a, b):
    return a.bond_dims == b.bond_dims and a.amplitude == b.amplitude and all(
        np.array_equal(x, y) for x, y in zip(a.to_host(), b.to_host()))


def _untouched(handle, data, amplitude=None):
    return (all(np.array_equal(handle.site(i), data[i]) for i in range(len(data)))
            and (amplitude is None or handle.amplitude == amplitude))


def _fail_every_allocation(qil, name, call, operands_untouched):
    ctx = qil.default_context()
    base = ctx.mem_info()["pool_in_use"]                 # the operands are alive, no result is
    ref = call()
    ref_state = (ref.bond_dims, ref.amplitude, ref.to_host())
    del ref
    assert ctx.mem_info()["pool_in_use"] == base, name
    failures, got = 0, None
    for j in range(3000):
        ctx.fail_alloc_after(j)
        try:
            got = call()
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        if not failed:
            break
        failures += 1
        assert ctx.unowned_bytes() == 0, (name, j)
        assert ctx.mem_info()["pool_in_use"] == base, (name, j, ctx.mem_info()["pool_in_use"], base)
        assert operands_untouched(), (name, j)
    print(f"{name}: {failures} pool allocations before the last one")
    assert got is not None, name
    assert got.bond_dims == ref_state[0] and got.amplitude == ref_state[1], name
    assert all(np.array_equal(x, y) for x, y in zip(got.to_host(), ref_state[2])), name
    assert failures >= SITES, (name, failures)
    del got
    assert ctx.mem_info()["pool_in_use"] == base and operands_untouched(), name


def _apply_operands(qil, seed, wdtype, adtype):
    rng = np.random.default_rng(seed)
    w = random_mpo_data([3] * (SITES - 1), rng, wdtype)
    a = random_mps_data(saturated_profile(SITES, 8), rng, adtype)
    return w, a, qil.SingleSiteMPO(w), qil.SignalMPS(a, amplitude=1.25)


@pytest.mark.parametrize("case,wdtype,zip_maxdim", [
    ("capped", np.complex128, 6),        # sketched basis from the third site on, SVD before; W as it is, psi widened
    ("default-cap", np.complex128, None),  # no bond capped: the SVD branch at every site
    ("all-real", np.float64, 6),         # nothing is widened
])
def test_apply_compress_fails_cleanly_at_every_allocation(qil, case, wdtype, zip_maxdim):
    w, a, W, psi = _apply_operands(qil, 101, wdtype, np.float64)
    _fail_every_allocation(qil, f"apply_compress {case}",
                           lambda: qil.apply_compress(W, psi, maxdim=4, tol=1e-8, zip_maxdim=zip_maxdim),
                           lambda: _untouched(W, w) and _untouched(psi, a, 1.25))


def test_apply_compress_widens_a_real_operator_too(qil):
    """the other widening path: a real W under a complex psi"""
    w, a, W, psi = _apply_operands(qil, 102, np.float64, np.complex128)
    _fail_every_allocation(qil, "apply_compress real W, complex psi",
                           lambda: qil.apply_compress(W, psi, maxdim=4, tol=1e-8, zip_maxdim=6),
                           lambda: _untouched(W, w) and _untouched(psi, a, 1.25))


def test_hadamard_compress_fails_cleanly_at_every_allocation(qil):
    rng = np.random.default_rng(103)
    d1 = random_mps_data(saturated_profile(SITES, 4), rng)
    d2 = random_mps_data(saturated_profile(SITES, 4), rng, np.complex128)
    phi, psi = qil.SignalMPS(d1, amplitude=0.5), qil.SignalMPS(d2, amplitude=-2.0)
    _fail_every_allocation(qil, "hadamard_compress",
                           lambda: qil.hadamard_compress(phi, psi, maxdim=4, tol=1e-8),
                           lambda: _untouched(phi, d1, 0.5) and _untouched(psi, d2, -2.0))


def test_linear_combination_compress_zip_route_fails_cleanly_at_every_allocation(qil):
    """[a, b, a]: the repeated handle is copied once, the real term widened; concatenated bond 24 > zip_maxdim 6"""
    rng = np.random.default_rng(104)
    d1 = random_mps_data(saturated_profile(SITES, 8), rng, np.complex128)
    d2 = random_mps_data(saturated_profile(SITES, 8), rng)
    a, b = qil.SignalMPS(d1, amplitude=0.5), qil.SignalMPS(d2)
    _fail_every_allocation(qil, "linear_combination_compress zip-up",
                           lambda: qil.linear_combination_compress([a, b, a], [1.0, 2.0, -0.5j], maxdim=4, tol=1e-8, zip_maxdim=6),
                           lambda: _untouched(a, d1, 0.5) and _untouched(b, d2, 1.0))


def test_linear_combination_compress_literal_route_fails_cleanly_at_every_allocation(qil):
    """two real terms of bond 2 under the default cap (maxdim + 16): the operands are read as they are"""
    rng = np.random.default_rng(105)
    d1 = random_mps_data([2] * (SITES - 1), rng)
    d2 = random_mps_data([2] * (SITES - 1), rng)
    a, b = qil.SignalMPS(d1, amplitude=0.5), qil.SignalMPS(d2, amplitude=3.0)
    _fail_every_allocation(qil, "linear_combination_compress literal",
                           lambda: qil.linear_combination_compress([a, b], [1.0, -2.0], maxdim=4, tol=1e-8),
                           lambda: _untouched(a, d1, 0.5) and _untouched(b, d2, 3.0))


def test_signal_ztmps_fails_cleanly_at_every_allocation(qil):
    rng = np.random.default_rng(106)
    t = np.arange(2 ** SITES) / 2 ** SITES
    x = np.exp(-2.0 * t) * np.cos(2 * np.pi * 5 * t) + 0.05 * rng.standard_normal(2 ** SITES)
    x0 = x.copy()
    _fail_every_allocation(qil, "signal_ztmps",
                           lambda: qil.signal_ztmps(x, cutoff=1e-10, maxdim=8),
                           lambda: np.array_equal(x, x0))
