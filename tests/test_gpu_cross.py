"""GPU tests of the cross-interpolation encoder (qil.signal_mps_cross, the qil_cross_* session) and of qil.ztmps_from_mps.

The yardstick is the signal itself: dense at n = 12 / 14 (mps_to_vector, which carries the amplitude), 2 000 seeded random
samples through coefficient_batch at n = 40.  Bound: max |interpolant - x| <= n tol max|x| -- each of the n - 1 bonds is allowed
tol fmax by the stop rule; tests/test_cross_model.py holds the numpy model of the same algorithm to a ninth of that bound on the
same inputs.  Every case runs under QIL_CROSS_ROUTE=lds and =global: the same code on another pointer, so nothing else changes
(a block whose bound does not fit the LDS takes the global route under either).

Shapes: n = 12 is the smallest register on which the four signals reach their ranks (16 for the chirp) with room on both
sides; the full-rank cases saturate every bond, c64 at n = 14 / maxdim 128 with blocks of 128 x 128 and 256 x 64 (256 KiB: the
global route unforced), f64 at n = 12 / maxdim 64 with blocks of 64 x 64 and 128 x 32 (32 KiB: LDS)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cross_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["lds", "global"]
DTYPES = {"f64": np.float64, "c64": np.complex128}
QIL_EINVAL_ARG = 7


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary or session outlives a call)."""
    yield
    assert qil.default_context().unowned_bytes() == 0


@functools.lru_cache(maxsize=None)
def _signal(name, n):
    sig = M.SIGNALS.get(name) or getattr(M, name)
    return sig(np.arange(2 ** n, dtype=np.float64), float(2 ** n))


@functools.lru_cache(maxsize=None)
def _random_signal(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(2 ** n) + 1j * rng.standard_normal(2 ** n)


def _on_device(torch, x, dtype):
    assert dtype == np.complex128 or not np.iscomplexobj(x), "a complex signal has no f64 twin"
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _check_gauge(qil, psi, x, n, tol):
    """unit-norm chain, amplitude = the norm of the represented signal (within the max-norm bound in the 2-norm)"""
    assert abs(qil.norm(psi) - 1.0) <= 64 * n * 2.0 ** -52
    assert abs(psi.amplitude - np.linalg.norm(x)) <= np.sqrt(x.size) * n * tol * np.abs(x).max() + 64 * n * 2.0 ** -52 * np.linalg.norm(x)


CASES_DENSE = [(name, dt) for name in sorted(M.SIGNALS) for dt in ("f64", "c64") if not (name == "three_modes" and dt == "f64")]


# ---------------------------------------------------------------- 1. dense check
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tol", [1e-9, 1e-6])
@pytest.mark.parametrize("name, dt", CASES_DENSE)
def test_dense_signal_within_the_bound(qil, torch, monkeypatch, name, dt, tol, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n = 12
    x = _signal(name, n)
    psi, info = qil.signal_mps_cross(_on_device(torch, x, DTYPES[dt]), maxdim=64, tol=tol, return_info=True)
    y = qil.mps_to_vector(psi)
    err, bound = np.abs(y - x).max(), n * tol * np.abs(x).max()
    print(f"{name} {dt} tol {tol:g} {route}: bonds max {max(psi.bond_dims)}, sweeps {info['sweeps']}, nevals {info['nevals']}, "
          f"est {info['est']:.2e}, err / bound {err / bound:.3g}")
    assert psi.dtype == DTYPES[dt] and len(psi) == n
    assert info["converged"] == 1 and info["est"] <= tol and 0 < info["nevals"] < 8 * 2 ** n
    assert err <= bound, (err, bound)
    _check_gauge(qil, psi, x, n, tol)


# ---------------------------------------------------------------- 2. full-rank block sizes
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dt, n, maxdim", [("c64", 14, 128), ("f64", 12, 64)])
def test_full_rank_blocks_are_exact(qil, torch, monkeypatch, dt, n, maxdim, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    x = _random_signal(n, 20 + n)
    x = x if dt == "c64" else np.ascontiguousarray(x.real)
    tol = 1e-9
    psi, info = qil.signal_mps_cross(_on_device(torch, x, DTYPES[dt]), maxdim=maxdim, tol=tol, return_info=True)
    assert psi.bond_dims == [min(2 ** l, 2 ** (n - l), maxdim) for l in range(1, n)]
    err, bound = np.abs(qil.mps_to_vector(psi) - x).max(), n * tol * np.abs(x).max()
    print(f"full rank {dt} n {n} maxdim {maxdim} {route}: sweeps {info['sweeps']}, nevals {info['nevals']}, est {info['est']:.2e}, "
          f"err / max|x| {err / np.abs(x).max():.2e}")
    assert info["converged"] == 1 and info["est"] == 0.0
    assert err <= bound, (err, bound)
    _check_gauge(qil, psi, x, n, tol)


# ---------------------------------------------------------------- 3. rank cap
@functools.lru_cache(maxsize=None)
def _model_cap_error():
    n = 12
    R = M.cross(M.sampler(M.chirp, n), n, 1e-9, 8, M.default_seeds(n))
    return np.abs(M.dense(R["sites"]) - _signal("chirp", n)).max(), R["est"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_rank_cap_reports_what_is_left(qil, torch, monkeypatch, dt, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, tol = 12, 1e-9
    x = _signal("chirp", n)
    psi, info = qil.signal_mps_cross(_on_device(torch, x, DTYPES[dt]), maxdim=8, tol=tol, return_info=True)
    err = np.abs(qil.mps_to_vector(psi) - x).max()
    model_err, model_est = _model_cap_error()
    print(f"rank cap {dt} {route}: bonds {psi.bond_dims}, est {info['est']:.4f}, err {err:.4f}, err / est {err / info['est']:.3f}, "
          f"model err {model_err:.4f} est {model_est:.4f}, err / model err {err / model_err:.3f}")
    assert max(psi.bond_dims) <= 8
    assert info["converged"] == 0 and info["sweeps"] == 8 and info["est"] > tol
    assert err <= 4 * model_err, (err, model_err)


# ---------------------------------------------------------------- 4. callable route, n = 40
def _torch_signal(torch, name, n, complex_out):
    """The signals in t = k / N: k < 2^53 is exact in a double, and so is the division by a power of two."""
    scale = 1.0 / float(2 ** n)

    def f(idx):
        t = idx.to(torch.float64) * scale
        if name == "gauss":
            v = torch.exp(-0.5 * ((t - 0.37) / 0.04) ** 2)
        else:
            v = torch.cos(2 * np.pi * (5 * t + 20 * t * t))
        return v.to(torch.complex128) if complex_out else v
    return f


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dt", ["f64", "c64"])
@pytest.mark.parametrize("name", ["gauss", "chirp"])
def test_callable_route_at_two_to_the_forty(qil, torch, monkeypatch, name, dt, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, tol = 40, 1e-9
    psi, info = qil.signal_mps_cross(_torch_signal(torch, name, n, dt == "c64"), n=n, maxdim=64, tol=tol, return_info=True)
    idx = np.random.default_rng(77).integers(0, 2 ** n, size=2000, dtype=np.int64)
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    got = qil.coefficient_batch(psi, bits)
    want = M.SIGNALS[name](idx.astype(np.float64), float(2 ** n))
    err = np.abs(got - want).max()
    print(f"callable {name} {dt} {route}: bonds max {max(psi.bond_dims)}, sweeps {info['sweeps']}, nevals {info['nevals']}, "
          f"est {info['est']:.2e}, err / bound {err / (n * tol):.3g}")
    assert psi.dtype == DTYPES[dt] and len(psi) == n
    assert info["converged"] == 1 and info["nevals"] < 2 ** 20
    assert err <= n * tol * 1.0, err                              # max|x| = 1 for both signals
    assert abs(qil.norm(psi) - 1.0) <= 64 * n * 2.0 ** -52


def test_callable_needs_n_and_device_values(qil, torch):
    with pytest.raises(ValueError, match="needs n"):
        qil.signal_mps_cross(lambda idx: idx.to(torch.float64))
    with pytest.raises(ValueError, match="float64 or complex128"):
        qil.signal_mps_cross(lambda idx: idx.to(torch.float32), n=8)
    with pytest.raises(ValueError, match="seeds must be indices"):
        qil.signal_mps_cross(lambda idx: idx.to(torch.float64), n=8, seeds=[0, 256])


# ---------------------------------------------------------------- 5. session equals one-shot
def _drive_session(qil, torch, x_dev, n, code, maxdim, tol, max_sweeps, seeds):
    import importlib
    L = importlib.import_module("qilaplace_jl_amd._lib")
    ctx = qil.default_context()
    s = C.c_void_p()
    sd = (C.c_int64 * len(seeds))(*[int(v) for v in seeds])
    L.check(L.lib.qil_cross_begin(ctx.handle, n, code, maxdim, tol, max_sweeps, sd, len(seeds), C.byref(s)))
    h = C.c_void_p()
    try:
        # finish with samples pending is an argument error, and leaves the session usable
        assert L.lib.qil_cross_finish(s, C.byref(h), None, None, None, None) == QIL_EINVAL_ARG
        assert "samples are still pending" in L.last_error() and not h.value
        count, requests = C.c_int64(), 0
        while True:
            L.check(L.lib.qil_cross_pending(s, C.byref(count)))
            if count.value == 0:
                break
            idx = torch.empty(count.value, dtype=torch.int64, device=x_dev.device)
            L.check(L.lib.qil_cross_indices(s, C.c_void_p(idx.data_ptr())))
            assert int(idx.min()) >= 0 and int(idx.max()) < 2 ** n
            vals = x_dev[idx].contiguous()
            torch.cuda.current_stream(x_dev.device).synchronize()
            L.check(L.lib.qil_cross_supply(s, C.c_void_p(vals.data_ptr())))
            requests += 1
        # nothing pending: indices and supply are argument errors
        assert L.lib.qil_cross_indices(s, C.c_void_p(x_dev.data_ptr())) == QIL_EINVAL_ARG
        assert "cross_indices: nothing is pending" in L.last_error()
        assert L.lib.qil_cross_supply(s, C.c_void_p(x_dev.data_ptr())) == QIL_EINVAL_ARG
        assert "cross_supply: nothing is pending" in L.last_error()
        est, nevals, sweeps, converged = C.c_double(), C.c_int64(), C.c_int(), C.c_int()
        L.check(L.lib.qil_cross_finish(s, C.byref(h), C.byref(est), C.byref(nevals), C.byref(sweeps), C.byref(converged)))
        extra = C.c_void_p()
        assert L.lib.qil_cross_finish(s, C.byref(extra), None, None, None, None) == QIL_EINVAL_ARG and not extra.value
    finally:
        L.lib.qil_cross_destroy(s)
    info = {"est": est.value, "nevals": nevals.value, "sweeps": sweeps.value, "converged": converged.value}
    return qil.SignalMPS(ctx=ctx, _handle=h), info, requests


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name, dt", [("cospoly", "f64"), ("three_modes", "c64"), ("chirp", "c64")])
def test_session_equals_one_shot(qil, torch, monkeypatch, name, dt, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, tol = 12, 1e-9
    x_dev = _on_device(torch, _signal(name, n), DTYPES[dt])
    seeds = M.default_seeds(n)
    one, info1 = qil.signal_mps_cross(x_dev, maxdim=64, tol=tol, seeds=seeds, return_info=True)
    two, info2, requests = _drive_session(qil, torch, x_dev, n, 1 if dt == "c64" else 0, 64, tol, 8, seeds)
    assert info1 == info2
    assert requests == 1 + (2 * info1["sweeps"] + 1) * (n - 1)        # the seeds, two half-sweeps per sweep, the final one
    assert one.bond_dims == two.bond_dims and one.amplitude == two.amplitude
    for i in range(n):
        assert np.array_equal(one.site(i), two.site(i)), i


# ---------------------------------------------------------------- 6. seeds: the documented blind spot
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_seeds_decide_whether_an_isolated_spike_is_seen(qil, torch, monkeypatch, dt, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, tol = 12, 1e-9
    x = _signal("spike", n)
    x_dev = _on_device(torch, x, DTYPES[dt])
    seen, info = qil.signal_mps_cross(x_dev, maxdim=64, tol=tol, seeds=[0, 1234], return_info=True)
    assert info["converged"] == 1
    assert np.abs(qil.mps_to_vector(seen) - x).max() <= n * tol * np.abs(x).max()
    blind, info = qil.signal_mps_cross(x_dev, maxdim=64, tol=tol, seeds=[0], return_info=True)
    y = qil.mps_to_vector(blind)
    # the limitation, pinned: converged, the estimate small, the spike missing -- and everything else right
    assert info["converged"] == 1 and info["est"] <= tol
    assert abs(y[1234] - x[1234]) > 0.5
    assert np.abs(np.delete(y - x, 1234)).max() <= n * tol * np.abs(x).max()


# ---------------------------------------------------------------- 7. agreement with the existing encoder
@pytest.mark.parametrize("route", ROUTES)
def test_agrees_with_signal_mps(qil, torch, monkeypatch, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, tol = 12, 1e-9
    x = _signal("three_modes", n)
    x_dev = _on_device(torch, x, np.complex128)
    a = qil.signal_mps_cross(x_dev, maxdim=64, tol=tol)
    b = qil.signal_mps(x_dev)
    rel = qil.distance(a, b) / np.linalg.norm(x)
    print(f"distance to signal_mps / norm {route}: {rel:.2e} (bound {np.sqrt(2 ** n) * n * tol:.2e})")
    assert rel <= np.sqrt(2 ** n) * n * tol


# ---------------------------------------------------------------- 8. ztmps_from_mps
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_ztmps_from_mps_is_signal_ztmps_bit_for_bit(qil, dt):
    n, c = 6, 1e-10
    rng = np.random.default_rng(5)
    x = rng.standard_normal(2 ** n) + (1j * rng.standard_normal(2 ** n) if dt == "c64" else 0.0)
    want = qil.signal_ztmps(x, cutoff=c)
    psi = qil.signal_mps(x, cutoff=c)
    before = [psi.site(i).copy() for i in range(n)]
    got = qil.ztmps_from_mps(psi, cutoff=c)
    assert isinstance(got, qil.ZTMPS) and got.paired and got.ntensors == 2 * n
    assert got.bond_dims == want.bond_dims and got.amplitude == want.amplitude and got.dtype == want.dtype
    for a, b in zip(got.to_host(), want.to_host()):
        assert np.array_equal(a, b)
    for i in range(n):
        assert np.array_equal(psi.site(i), before[i])             # the operand is left intact
    with pytest.raises(ValueError, match="paired state already"):
        qil.ztmps_from_mps(got)
    import importlib
    L = importlib.import_module("qilaplace_jl_amd._lib")
    h = C.c_void_p()
    assert L.lib.qil_ztmps_from_mps(got.handle, c, 0, C.byref(h)) == QIL_EINVAL_ARG and not h.value
    # a cross-encoded state enters the same way
    z = qil.ztmps_from_mps(qil.signal_mps_cross(x, maxdim=16, tol=1e-12), cutoff=c)
    assert z.ntensors == 2 * n and z.paired


# ---------------------------------------------------------------- 9. edges
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dt", ["f64", "c64"])
@pytest.mark.parametrize("n", [1, 2])
def test_shortest_chains(qil, torch, monkeypatch, n, dt, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    x = np.array([0.3, -1.5, 2.0, 0.25])[:2 ** n] * (1.0 if dt == "f64" else (1.0 + 0.5j))
    for operand in (_on_device(torch, x, DTYPES[dt]), x):            # a device tensor and a host array
        psi, info = qil.signal_mps_cross(operand, maxdim=4, tol=1e-12, return_info=True)
        assert len(psi) == n and info["converged"] == 1
        assert np.abs(qil.mps_to_vector(psi) - x).max() <= 16 * 2.0 ** -52 * np.abs(x).max()
        _check_gauge(qil, psi, x, n, 0.0)


@pytest.mark.parametrize("route", ROUTES)
def test_length_that_is_no_power_of_two_zero_fills_and_warns(qil, torch, monkeypatch, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, tol, length = 12, 1e-9, 3072
    full = _signal("cospoly", n).copy()
    full[length:] = 0.0
    with pytest.warns(UserWarning, match="not a power of 2; zero-filling to 4096"):
        psi, info = qil.signal_mps_cross(_on_device(torch, full[:length], np.float64), maxdim=64, tol=tol, return_info=True)
    assert len(psi) == n and info["converged"] == 1
    assert np.abs(qil.mps_to_vector(psi) - full).max() <= n * tol * np.abs(full).max()
    with pytest.raises(ValueError, match="power of 2"):
        import importlib
        L = importlib.import_module("qilaplace_jl_amd._lib")
        h, sd = C.c_void_p(), (C.c_int64 * 1)(0)
        L.check(L.lib.qil_signal_mps_cross(qil.default_context().handle, full.ctypes.data_as(C.c_void_p), 2500, 0, 8, tol, 2, sd, 1,
                                           C.byref(h), None, None, None, None))                     # round(log2 2500) = 11, 2500 > 2048


@pytest.mark.parametrize("route", ROUTES)
def test_all_zero_signal_and_failed_calls_leave_the_pool_as_it_was(qil, torch, monkeypatch, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    ctx = qil.default_context()
    x_dev = _on_device(torch, _signal("gauss", 10), np.float64)
    qil.signal_mps_cross(x_dev, maxdim=16, tol=1e-9)                       # warm the pool, so that only live blocks are compared
    before = ctx.mem_info()["pool_in_use"]
    with pytest.raises(ArithmeticError, match="every sampled value is 0"):
        qil.signal_mps_cross(torch.zeros(1024, dtype=torch.float64, device="cuda"), maxdim=16, tol=1e-9)
    assert ctx.mem_info()["pool_in_use"] == before and ctx.unowned_bytes() == 0
    with pytest.raises(ArithmeticError):
        qil.signal_mps_cross(lambda idx: torch.zeros(idx.shape, dtype=torch.complex128, device=idx.device), n=30)
    assert ctx.mem_info()["pool_in_use"] == before and ctx.unowned_bytes() == 0
    for k in (0, 3, 7, 8, 12):                                             # in begin, and in the gauge / norm of finish
        ctx.fail_alloc_after(k)
        try:
            with pytest.raises(MemoryError):
                qil.signal_mps_cross(x_dev, maxdim=16, tol=1e-9)
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.mem_info()["pool_in_use"] == before and ctx.unowned_bytes() == 0, k
    for bad in (dict(maxdim=0), dict(maxdim=257), dict(tol=-1.0), dict(seeds=[0, 1024]), dict(seeds=[]), dict(max_sweeps=0)):
        with pytest.raises(ValueError):
            qil.signal_mps_cross(x_dev, **{**dict(maxdim=16, tol=1e-9), **bad})
        assert ctx.mem_info()["pool_in_use"] == before
    qil.signal_mps_cross(x_dev, maxdim=16, tol=1e-9)                       # and the encoder still works
    assert ctx.mem_info()["pool_in_use"] == before


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_maxdim_one_gives_a_product_state(qil, torch, monkeypatch, dt, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n = 10
    # a product signal is exact at maxdim 1; anything else is cut to a product state
    k = np.arange(2 ** n, dtype=np.float64)
    x = np.exp(-3e-3 * k) * (1.0 if dt == "f64" else np.exp(0.4j))
    psi, info = qil.signal_mps_cross(_on_device(torch, x, DTYPES[dt]), maxdim=1, tol=1e-9, return_info=True)
    assert psi.bond_dims == [1] * (n - 1) and info["converged"] == 1
    assert np.abs(qil.mps_to_vector(psi) - x).max() <= n * 1e-9 * np.abs(x).max()
    psi, info = qil.signal_mps_cross(_on_device(torch, _signal("chirp", n), DTYPES[dt]), maxdim=1, tol=1e-9, return_info=True)
    assert psi.bond_dims == [1] * (n - 1) and info["converged"] == 0 and info["est"] > 1e-9
    assert abs(qil.norm(psi) - 1.0) <= 64 * n * 2.0 ** -52


def test_example_runs():
    env = dict(os.environ)
    env.pop("QIL_CROSS_ROUTE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cross_encode.py")], capture_output=True, text=True,
                       cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "samples read" in r.stdout
