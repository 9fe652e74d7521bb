"""GPU tests of the element-wise maps: qil.map_states (qil_mps_map), cross_map, and the front-ends magnitude, log_power,
shrink, divide, deconvolve.  Every case runs under QIL_CROSS_ROUTE=lds and =global (tests/test_gpu_cross.py).

Dense cases (tests/map_cases.py, n = 12): g is computed in numpy from mps_to_vector of the operands, the budget is map_cases'
    n tol max|g| + perturbation(delta) + 16 * 2^-53 max|g|,
delta = the sum over the operands of the largest chain bound (the sampler) + block bound (mps_to_vector) of readout_cases.
tests/test_map_cases_oracle.py holds the numpy model of the interpolation to a ninth of n tol max|g| on the same cases.

n = 40: operands exponential_mps(z), which is z^j for the DOUBLE z exactly (|z| differs from 1 by an ulp, which 2^40 powers
turn into 1e-4), so the closed forms are taken from the same doubles: (z1 / z2)^j and |z1^j + z2^j|^2 from the dyadic powers of
exponential_tensors, in longdouble; for |z| = 1 they are e^{i (t1 - t2) j} and 2 + 2 cos((t1 - t2) j)."""
import ctypes as C
import gc
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import map_cases as P
import readout_cases as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["lds", "global"]
CLD = np.clongdouble


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
    gc.collect()
    assert qil.default_context().unowned_bytes() == 0


def _check_gauge(qil, psi, x, n, tol):
    """unit-norm chain, amplitude = the norm of the represented signal (within the max-norm bound in the 2-norm)"""
    assert abs(qil.norm(psi) - 1.0) <= 64 * n * 2.0 ** -52
    assert abs(psi.amplitude - np.linalg.norm(x)) <= np.sqrt(x.size) * n * tol * np.abs(x).max() + 64 * n * 2.0 ** -52 * np.linalg.norm(x)


def _readout_delta(psi):
    """The largest distance between a sample the map reads from psi and the entry of mps_to_vector(psi) the test uses: the sum
    of the two read-outs' rounding bounds."""
    data = psi.to_host()
    dims = [1] + list(psi.bond_dims) + [1]
    mag = R.dense_tensor(data, R.modulus).reshape(-1)
    return float((R.bound(mag, R.chain_qs(dims), psi.amplitude) + R.bound(mag, R.block_qs(dims), psi.amplitude)).max())


def _operands(qil, c):
    return tuple(qil.signal_mps(x) for x in P.dense_operands(c))


def _map(qil, c, states, tol, **kw):
    return qil.map_states(c.op, *states, params=() if c.param is None else (c.param,), maxdim=P.MAXDIM, tol=tol,
                          max_sweeps=P.MAX_SWEEPS, return_info=True, **kw)


def _budget(qil, c, states, tol):
    xs = [qil.mps_to_vector(s) for s in states]
    g = P.evaluate(c, *xs)
    return g, P.budget(c, tol, g, sum(_readout_delta(s) for s in states), *xs)


# ---------------------------------------------------------------- 1. dense cases
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tol", P.TOLS)
@pytest.mark.parametrize("c", P.CASES, ids=[c.name for c in P.CASES])
def test_dense_case_within_the_budget(qil, monkeypatch, c, tol, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n = P.N_SITES
    states = _operands(qil, c)
    out, info = _map(qil, c, states, tol)
    g, budget = _budget(qil, c, states, tol)
    err = np.abs(qil.mps_to_vector(out) - g).max()
    print(f"{c.name} tol {tol:g} {route}: bonds max {max(out.bond_dims)}, sweeps {info['sweeps']}, nevals {info['nevals']}, "
          f"est {info['est']:.2e}, err {err:.3e}, budget {budget:.3e}, err / budget {err / budget:.3g}")
    assert out.dtype == (np.complex128 if c.result_complex else np.float64) and len(out) == n
    assert out.site_ids == states[0].site_ids
    assert info["converged"] == 1 and info["est"] <= tol
    assert err <= budget, (err, budget)
    _check_gauge(qil, out, g, n, tol)


def test_front_ends_are_the_verb(qil):
    c = P.BY_NAME
    a, b = qil.signal_mps(P.signal("chirp")), qil.signal_mps(P.signal("b"))
    same = lambda x, y: all(np.array_equal(s, t) for s, t in zip(x.to_host(), y.to_host())) and x.amplitude == y.amplitude
    assert same(qil.magnitude(a), qil.map_states("abs", a))
    assert same(qil.shrink(a, c["shrink_chirp"].param), qil.map_states("shrink", a, params=(c["shrink_chirp"].param,)))
    assert same(qil.divide(a, b, 0.1, tol=1e-6), qil.map_states("divide", a, b, params=(0.1,), tol=1e-6))
    gs = qil.signal_mps(P.signal("gauss"))
    assert same(qil.log_power(gs, 1e-12), qil.map_states("log", gs, params=(1e-12,)))
    assert qil.magnitude(a).dtype == np.float64


# ---------------------------------------------------------------- 2. n = 40 on exact operands
def _exact_exponential(qil, z, n, idx):
    """z^j for the double z at the indices idx, in longdouble, from the dyadic powers the state is built from."""
    pw = [t[0, 1, 0] for t in qil.exponential_tensors(z, n)]           # site i + 1: z^(2^(n - 1 - i))
    v = np.ones(len(idx), dtype=CLD)
    for i in range(n):
        v = np.where((idx >> (n - 1 - i)) & 1, v * CLD(pw[i]), v)
    return v


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("what", ["divide", "power"])
def test_exact_operands_at_two_to_the_forty(qil, monkeypatch, what, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, tol = 40, 1e-9
    z1, z2 = complex(np.exp(0.31j)), complex(np.exp(-1.1j))
    p1, p2 = qil.exponential_mps(z1, n), qil.exponential_mps(z2, n)
    idx = np.random.default_rng(77).integers(0, 2 ** n, size=2000, dtype=np.int64)
    x1, x2 = _exact_exponential(qil, z1, n, idx), _exact_exponential(qil, z2, n, idx)
    if what == "divide":
        out, info = qil.map_states("divide", p1, p2, params=(0.0,), maxdim=64, tol=tol, return_info=True)
        want, gmax = x1 / x2, float(np.abs(x1 / x2).max())
    else:
        out, info = qil.map_states("power", qil.add(p1, p2), params=(2.0,), maxdim=64, tol=tol, return_info=True)
        want, gmax = np.abs(x1 + x2) ** 2, 4.0 * (1 + 1e-3)          # |z|^(2^40) = 1 +- 1e-4 at most
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    got = qil.coefficient_batch(out, bits)
    err = float(np.abs(got.astype(CLD) - want).max())
    print(f"{what} n = 40 {route}: bonds max {max(out.bond_dims)}, sweeps {info['sweeps']}, nevals {info['nevals']}, "
          f"est {info['est']:.2e}, err / bound {err / (n * tol * gmax):.3g}")
    assert len(out) == n and out.dtype == (np.complex128 if what == "divide" else np.float64)
    assert info["converged"] == 1 and info["nevals"] < 2 ** 20
    assert err <= n * tol * gmax, err
    assert abs(qil.norm(out) - 1.0) <= 64 * n * 2.0 ** -52


# ---------------------------------------------------------------- 3. cross_map
def _torch_op(torch, c):
    if c.op == "divide":
        return lambda a, b: a * torch.conj(b) / (torch.abs(b) ** 2 + c.param) if a.is_complex() or b.is_complex() else a * b / (b * b + c.param)
    if c.op == "shrink":
        def f(a):
            m = torch.abs(a)
            return a * torch.where(m > 0, torch.clamp(1.0 - c.param / torch.where(m > 0, m, torch.ones_like(m)), min=0.0), torch.zeros_like(m))
        return f
    if c.op == "abs":
        return lambda a: torch.abs(a)
    raise KeyError(c.op)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["divide_three_modes_b", "shrink_chirp", "abs_chirp"])
def test_cross_map_agrees_with_map_states(qil, torch, monkeypatch, name, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    c, tol = P.BY_NAME[name], 1e-9
    states = _operands(qil, c)
    native, _ = _map(qil, c, states, tol)
    general, info = qil.cross_map(_torch_op(torch, c), *states, maxdim=P.MAXDIM, tol=tol, max_sweeps=P.MAX_SWEEPS, return_info=True)
    _, budget = _budget(qil, c, states, tol)
    diff = np.abs(qil.mps_to_vector(general) - qil.mps_to_vector(native)).max()
    print(f"cross_map vs map_states {name} {route}: diff / (2 budget) {diff / (2 * budget):.3g}, nevals {info['nevals']}")
    assert info["converged"] == 1 and general.dtype == native.dtype
    assert diff <= 2 * budget, (diff, budget)


@pytest.mark.parametrize("route", ROUTES)
def test_cross_map_of_an_arbitrary_function(qil, torch, monkeypatch, route):
    """tanh(Re a) on cospoly: no built-in op; both tanh and Re are non-expansive, so L_f = 1."""
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, tol = P.N_SITES, 1e-9
    psi = qil.signal_mps(P.signal("cospoly"))
    out, info = qil.cross_map(lambda a: torch.tanh(a.real if a.is_complex() else a), psi, maxdim=P.MAXDIM, tol=tol, return_info=True)
    g = np.tanh(qil.mps_to_vector(psi).real)
    budget = n * tol * np.abs(g).max() + _readout_delta(psi) + 16 * 2.0 ** -53 * np.abs(g).max()
    err = np.abs(qil.mps_to_vector(out) - g).max()
    print(f"cross_map tanh {route}: bonds max {max(out.bond_dims)}, nevals {info['nevals']}, err / budget {err / budget:.3g}")
    assert info["converged"] == 1 and out.dtype == np.float64
    assert err <= budget, (err, budget)
    with pytest.raises(ValueError, match="does not match"):
        qil.cross_map(torch.abs, psi, n=n + 1)
    with pytest.raises(ValueError, match="float64 or complex128"):
        qil.cross_map(lambda a: a.to(torch.float32), psi)


# ---------------------------------------------------------------- 4. deconvolve
@pytest.mark.parametrize("route", ROUTES)
def test_deconvolve_follows_its_dense_model(qil, monkeypatch, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    n, map_tol = 10, 1e-10
    N = 2 ** n
    x = P.signal("three_modes", n)
    h = np.zeros(N)
    h[:3] = [1.0, 0.5, 0.25]
    y = np.fft.ifft(np.fft.fft(x) * np.fft.fft(h))
    py, ph = qil.signal_mps(y), qil.signal_mps(h)
    F = qil.build_qft_mpo(py)
    got = qil.mps_to_vector(qil.deconvolve(py, ph, F=F, map_tol=map_tol))
    Fm = qil.mpo_to_matrix(F).T                              # M[in, out]: (F v)[out] = sum_in M[in, out] v[in]
    Y, H = Fm @ y, Fm @ h.astype(np.complex128)
    Q = Y * np.conj(H) / np.abs(H) ** 2
    model = Fm.conj().T @ Q / np.sqrt(N)
    dist = np.linalg.norm(got - model)
    bound = 1.01 * np.sqrt(N) * n * map_tol * np.abs(Q).max() + 1e-10 * np.linalg.norm(model)
    print(f"deconvolve {route}: |dev - model| {dist:.3e}, bound {bound:.3e}, ratio {dist / bound:.3g}; distance to the true x "
          f"{np.abs(got - x).max():.3e} of max|x| {np.abs(x).max():.3g} (the QFT operator's unitarity defect over min|Fh| = {np.abs(H).min():.3g})")
    assert dist <= bound, (dist, bound)
    with pytest.raises(TypeError, match="deconvolve: unsupported operand types"):
        qil.deconvolve(py, h)
    with pytest.raises(ValueError, match="same number of sites"):
        qil.deconvolve(py, qil.signal_mps(h[:N // 2]))


# ---------------------------------------------------------------- 5. errors
@pytest.mark.parametrize("route", ROUTES)
def test_failed_calls_leave_the_pool_as_it_was(qil, monkeypatch, route):
    monkeypatch.setenv("QIL_CROSS_ROUTE", route)
    L = importlib.import_module("qilaplace_jl_amd._lib")
    ctx = qil.default_context()
    n = 10
    a, b = qil.signal_mps(P.signal("chirp", n)), qil.signal_mps(P.signal("b", n))
    # b vanishes exactly on the first half of the register (index 0 is a seed): a / b is not finite there
    zero = qil.SignalMPS([np.array([0.0, 1.0]).reshape(1, 2, 1)] + [np.ones((1, 2, 1))] * (n - 1))
    paired = qil.signal_ztmps(P.signal("gauss", 5))
    short = qil.signal_mps(P.signal("b", n - 1))
    other = qil.SignalMPS(b.to_host(), sites=list(range(101, 101 + n)), amplitude=b.amplitude)
    qil.divide(a, b, maxdim=16, tol=1e-9)                                   # warm the pool, so that only live blocks are compared
    gc.collect()
    before = ctx.mem_info()["pool_in_use"]

    def unchanged():
        gc.collect()
        return ctx.mem_info()["pool_in_use"] == before and ctx.unowned_bytes() == 0

    with pytest.raises(L.QilDomainError, match="not finite"):
        qil.divide(a, zero, maxdim=16, tol=1e-9)
    assert unchanged()
    v = qil.mps_to_vector(qil.divide(a, zero, reg=0.5, maxdim=16, tol=1e-9))    # regularised: finite, and 0 where b is
    assert np.abs(v[:2 ** (n - 1)]).max() <= n * 1e-9 * np.abs(v).max()
    assert unchanged()
    with pytest.raises(ValueError, match="paired states are not supported; map the SignalMPS and call ztmps_from_mps"):
        qil.magnitude(paired)
    h, seeds, par = C.c_void_p(), (C.c_int64 * 1)(0), (C.c_double * 1)(0.0)
    tail = (C.byref(h), None, None, None, None)
    assert L.lib.qil_mps_map((C.c_void_p * 1)(paired.handle), 1, L.QIL_MAP_ABS, None, 16, 1e-9, 4, seeds, 1, *tail) == 7
    assert "paired states are not supported" in L.last_error() and not h.value
    with pytest.raises(ValueError, match="same number of sites"):
        qil.divide(a, short)
    assert L.lib.qil_mps_map((C.c_void_p * 2)(a.handle, short.handle), 2, L.QIL_MAP_DIVIDE, par, 16, 1e-9, 4, seeds, 1, *tail) == 1   # QIL_EINVAL_LENGTH
    with pytest.raises(ValueError, match="same site indices"):
        qil.divide(a, other, maxdim=16, tol=1e-9)
    assert L.lib.qil_mps_map((C.c_void_p * 2)(a.handle, other.handle), 2, L.QIL_MAP_DIVIDE, par, 16, 1e-9, 4, seeds, 1, *tail) == 2   # QIL_EINVAL_SITES
    far = (C.c_int64 * 1)(2 ** n)
    assert L.lib.qil_mps_map((C.c_void_p * 1)(a.handle), 1, L.QIL_MAP_ABS, None, 16, 1e-9, 4, far, 1, *tail) == 7
    assert f"seed {2 ** n} outside" in L.last_error()
    assert unchanged()
    for k in (0, 2, 5, 9):                                                  # an allocation failure inside the call
        ctx.fail_alloc_after(k)
        try:
            with pytest.raises(MemoryError):
                qil.map_states("divide", a, b, maxdim=16, tol=1e-9, params=(0.0,), seed_peaks=0)
        finally:
            ctx.fail_alloc_after(None)
        assert unchanged(), k
    out = qil.divide(a, b, maxdim=16, tol=1e-9)                             # and the verb still works
    assert len(out) == n
    del out
    gc.collect()
    assert unchanged()


def test_example_runs():
    env = dict(os.environ)
    env.pop("QIL_CROSS_ROUTE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "deconvolve.py")], capture_output=True, text=True,
                       cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "deconvolved signal against the input" in r.stdout
