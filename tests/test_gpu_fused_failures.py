"""GPU tests of the failure paths of the fused truncations (apply_compress, hadamard_compress, linear_combination_compress), of
signal_ztmps, and of the verbs whose temporaries belong to a qil_scratch since: the gauge sweeps (canonicalize, compress,
mpo_compress and the routes of their truncated SVD), the signal encoders (signal_mps by svd and rsvd, rsvd and svd_trunc on
host operands) and the launch-per-step DT builder.  Every pool allocation of a call is made to fail in turn
(`fail_alloc_after`: the library's host-side injected QIL_ENOMEM; nothing faults on the device).

After each failed call nothing of it may be left on the device: no unowned block (`unowned_bytes`), and no block owned by a
handle that died with the call either -- `pool_in_use`, which sums the pools of the batch workers too, is back at its value
before the call, which a leaked intermediate handle (the gauged copy of a state, the temporary operator of hadamard_compress)
or a block stranded on a worker context would raise without `unowned_bytes` seeing it.  The operands are untouched, and the
first call that is allowed all its allocations returns bit for bit what the undisturbed call returns.  No tolerances on
results: every comparison is equality.

A call that works IN PLACE gets a fresh operand per failing allocation.  A failed call leaves the chain as its last finished
gauge step left it, and once the chain is released the pool is back at its value before: where the call loses nothing the pool
held exactly the chain's sites and the dense state (or operator) is unchanged to 1e-12 |v| (the figure of test_gpu_gauge.py::test_allocation_failures_leave_the_state_of_a_sorted_
operand), where it truncates the chain is whole (consistent bond dimensions, finite norm).

The small cases have 6 sites and bonds <= 8.  The number of failing calls, printed per case, is the number of pool
allocations the call makes before its last one (the number tried, where the later ones are sampled); it is at least the number
of sites (the gauged copy alone takes one block per site, and the encoder behind signal_ztmps more than one per site), and at
least 20 where sampled."""
import itertools

import numpy as np
import pytest

import gauge_cases as G
from helpers import dense_mpo, dense_mps, random_mps_data, random_mpo_data, saturated_profile

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


def _chain_state(h):
    return (h.bond_dims, getattr(h, "amplitude", 1.0), h.to_host())        # (an operator carries no amplitude)


def _same(a, b):
    """Equality of nested tuples / lists of numbers and arrays."""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def _attempts(sampled):
    """j = 0, 1, 2, ... ; sampled: every j up to 63, then every 8th"""
    return itertools.chain(range(64), range(64, 30000, 8)) if sampled else range(3000)


def _fail_every_allocation(qil, name, call, operands_untouched, state=_chain_state, sampled=False, floor=SITES):
    ctx = qil.default_context()
    base = ctx.mem_info()["pool_in_use"]                 # the operands are alive, no result is
    ref = call()
    ref_state = state(ref)
    del ref
    assert ctx.mem_info()["pool_in_use"] == base, name
    failures, got = 0, None
    for j in _attempts(sampled):
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
    print(f"{name}: {failures} " + ("failing calls tried" if sampled else "pool allocations before the last one"))
    assert got is not None, name
    assert _same(state(got), ref_state), name
    assert failures >= (20 if sampled else floor), (name, failures)
    del got
    assert ctx.mem_info()["pool_in_use"] == base and operands_untouched(), name


def _pool_bytes(sites):
    """What the pool holds for a chain with these site tensors: one block per site, in units of 256 bytes."""
    return sum((t.nbytes + 255) // 256 * 256 for t in sites)


def _fail_every_allocation_in_place(qil, name, make, call, dense, lossless, sampled=False):
    """make() -> (handle, its site tensors); call(handle) works in place.  dense(sites) -> the vector the chain stands for."""
    ctx = qil.default_context()
    base = ctx.mem_info()["pool_in_use"]
    ref, up = make()
    up = [t.copy() for t in up]                                    # what the caller's arrays held before any call
    call(ref)
    ref_state = _chain_state(ref)
    del ref
    assert ctx.mem_info()["pool_in_use"] == base, name
    v = dense(up)
    failures, done = 0, False
    for j in _attempts(sampled):
        h, up_j = make()
        ctx.fail_alloc_after(j)
        try:
            call(h)
            done = True
        except MemoryError:
            failures += 1
        finally:
            ctx.fail_alloc_after(None)
        if done:
            break
        assert ctx.unowned_bytes() == 0, (name, j)
        sites = h.to_host()
        if lossless:                                               # (a truncated factor keeps the block of its full size)
            assert ctx.mem_info()["pool_in_use"] == base + _pool_bytes(sites), (name, j)
        assert _same(up_j, up), (name, j)                          # caller memory
        dims = [1] + list(h.bond_dims) + [1]
        assert all(t.shape[0] == dims[i] and t.shape[-1] == dims[i + 1] for i, t in enumerate(sites)), (name, j, dims)
        w = dense(sites)
        if lossless:
            assert np.linalg.norm(w - v) <= 1e-12 * np.linalg.norm(v), (name, j, np.linalg.norm(w - v))
        else:
            assert np.isfinite(np.linalg.norm(w)) and np.isfinite(getattr(h, "amplitude", 1.0)), (name, j)
        del h
        assert ctx.mem_info()["pool_in_use"] == base, (name, j)
    print(f"{name}: {failures} " + ("failing calls tried" if sampled else "pool allocations before the last one"))
    assert done and _same(_chain_state(h), ref_state), name
    assert failures >= (20 if sampled else SITES), (name, failures)
    del h
    assert ctx.mem_info()["pool_in_use"] == base, name


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


# ---------------------------------------------------------------- gauge sweeps (in place)
def _flat(sites):
    return (dense_mps if sites[0].ndim == 3 else dense_mpo)(sites).reshape(-1)


@pytest.mark.parametrize("direction", ["right", "left"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
def test_canonicalize_fails_cleanly_at_every_allocation(qil, dtype, direction):
    """the truncating SVD steps at canonicalize!'s cutoff 1e-12: saturated bonds have full rank, nothing is lost"""
    a = random_mps_data(saturated_profile(SITES, 8), np.random.default_rng(107), dtype)
    _fail_every_allocation_in_place(qil, f"canonicalize {direction} {np.dtype(dtype).name}",
                                    lambda: (qil.SignalMPS(a, amplitude=1.25), a),
                                    lambda psi: qil.canonicalize(psi, direction), _flat, lossless=True)


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
def test_compress_fails_cleanly_at_every_allocation(qil, dtype):
    a = random_mps_data(saturated_profile(SITES, 8), np.random.default_rng(108), dtype)
    _fail_every_allocation_in_place(qil, f"compress {np.dtype(dtype).name}",
                                    lambda: (qil.SignalMPS(a, amplitude=1.25), a),
                                    lambda psi: qil.compress(psi, maxdim=4, tol=1e-8), _flat, lossless=False)


@pytest.mark.parametrize("direction", ["down", "up"])
def test_mpo_compress_fails_cleanly_at_every_allocation(qil, direction):
    """the gauge pass takes the thin-QR steps, the return pass the SVD steps; bonds 3 of a random operator have full rank"""
    w = random_mpo_data([3] * (SITES - 1), np.random.default_rng(109))
    _fail_every_allocation_in_place(qil, f"mpo_compress {direction}",
                                    lambda: (qil.SingleSiteMPO(w), w),
                                    lambda W: qil.mpo_compress(W, direction), _flat, lossless=True)


@pytest.mark.parametrize("case,label,direction", [
    ("flat-1024x640-f64", "cert-640", "right"),          # absorb = 2: the certificate's QR factors and the copies out of them
    ("cut-1024x640-f64", "cert-declined", "left"),       # absorb = 1: declined, then the three transposition temporaries
    ("deficient-512x384-f64", "lowrank", "right"),       # absorb = 2: the sketch's per-attempt scratch
    ("deficient-512x384-f64", "lowrank", "left"),        # absorb = 1 below the sketch
])
def test_the_routes_of_the_truncated_svd_fail_cleanly(qil, case, label, direction, monkeypatch):
    """One chain of tests/gauge_cases.py per route of svd_trunc_dev that allocates beyond the common path; the head of the chain
    takes the first allocations, the operand's step the last, sampled ones."""
    c = G.BY_NAME[case]
    assert label in G.predicted(c.name)[0] and c.cert
    monkeypatch.setenv("QIL_SVD_CERT", "1")
    up = G.chain(c, direction)
    _fail_every_allocation_in_place(qil, f"{label} {direction} ({case})",
                                    lambda: (qil.SignalMPS(up, amplitude=G.AMPLITUDE), up),
                                    lambda psi: qil.canonicalize(psi, direction, center=G.center(c, direction), cutoff=c.cutoff,
                                                                 maxdim=c.maxdim),
                                    G.dense, lossless=c.kind == "flat", sampled=True)


# ---------------------------------------------------------------- encoders
def _signal(n, seed):
    t = np.arange(2 ** n) / 2 ** n
    return np.exp(-2.0 * t) * np.cos(2 * np.pi * 5 * t) + 0.05 * np.random.default_rng(seed).standard_normal(2 ** n)


@pytest.mark.parametrize("method", ["svd", "rsvd"])
def test_signal_mps_fails_cleanly_at_every_allocation(qil, method):
    """2^6 samples: below the level-parallel bisection, rsvd takes the sequential recursion"""
    x = _signal(SITES, 110)
    x0 = x.copy()
    _fail_every_allocation(qil, f"signal_mps {method}",
                           lambda: qil.signal_mps(x, method=method, cutoff=1e-10, maxdim=8),
                           lambda: np.array_equal(x, x0))


def test_signal_mps_level_parallel_bisection_fails_cleanly(qil):
    """2^16 samples, the smallest signal compress_tt_root splits over the worker contexts.  `fail_alloc_after` counts the
    allocations of the HOME context only (the root's own nodes and every first task of a level); `pool_in_use` includes the
    workers' pools, so a block that a failed level left on a worker would show."""
    x = _signal(16, 111)
    x0 = x.copy()
    _fail_every_allocation(qil, "signal_mps rsvd 2^16",
                           lambda: qil.signal_mps(x, method="rsvd", cutoff=1e-10, k=12, p=4, q=1),
                           lambda: np.array_equal(x, x0), sampled=True)


@pytest.mark.parametrize("verb", ["rsvd", "svd_trunc"])
def test_factorisations_of_host_operands_fail_cleanly_at_every_allocation(qil, verb):
    A = np.random.default_rng(112).standard_normal((64, 48))
    A0 = A.copy()
    call = (lambda: qil.rsvd(A, k=12, p=4, q=1)) if verb == "rsvd" else (lambda: qil.svd_trunc(A, cutoff=1e-12))
    _fail_every_allocation(qil, f"{verb} 64 x 48", call, lambda: np.array_equal(A, A0), state=tuple, floor=3)


# ---------------------------------------------------------------- launch-per-step DT builder
def test_build_dt_mpo_batch_launches_route_fails_cleanly_at_every_allocation(qil, monkeypatch):
    """n = 3, two damping values: a failing call returns no handle and leaves nothing in the pool"""
    monkeypatch.setenv("QIL_DT_BUILDER", "launches")                 # read per call
    wrs = [0.5, 2.0]
    _fail_every_allocation(qil, "build_dt_mpo_batch launches",
                           lambda: qil.build_dt_mpo_batch(3, wrs),
                           lambda: wrs == [0.5, 2.0],
                           state=lambda Ws: [(W.bond_dims, W.to_host()) for W in Ws])
