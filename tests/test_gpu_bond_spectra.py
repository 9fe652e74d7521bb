"""GPU tests of the Schmidt spectra (qil.bond_spectra, qil.mpo_bond_spectra) and of the helpers on top of them.

The yardstick is numpy's dense SVD of the state vector (of the dense operator for MPOs) reshaped at every cut and normalised;
N <= 14 tensors, so the vector has at most 2^14 entries -- but for the two f64 cap cases, which need 16 tensors (below).

Tolerance: every comparison of spectra is ABSOLUTE, at 64 N chi_max eps (eps = 2^-52, N tensors, chi_max the operand's largest
bond).  By Weyl's inequality a singular value moves by at most the 2-norm of the backward error; the 2 N QR steps and the Jacobi
iteration are each backward stable to a modest multiple of chi eps on a unit-norm state.  A numpy restatement of the two sweeps
stayed below 2e-15 against the dense SVD on every shape used here, so the yardstick alone sits far inside the bound.  Relative
accuracy of tiny values is not promised and not tested: the QR sweeps do not preserve it.

The LDS cap K of the one-launch kernel is 138 (f64) / 97 (c64).  Two kinds of case meet it:
  * "cap" / "cap+1": random chains of FULL rank whose middle bond is K (K + 1), so that the kernel really stages a K x K carry
    (150 544 B of LDS for c64, 153 456 B for f64, and for f64 the wave-per-pair sweep that columns longer than 128 take); at K + 1
    that bond takes the SVD route while its neighbours stay in the launch.  A carry of K rows needs a Schmidt rank of K on both
    sides of the cut, i.e. ceil(log2 K) tensors on each side: 14 tensors for c64 (bonds min(2^i, 2^(14 - i), K)), but 16 for f64
    (138 > 2^7), whose dense vector has 2^16 entries and whose largest dense SVD is 256 x 256.  `_carry_rows` restates the shapes
    of the two sweeps and the test asserts from it that the carry at the cap bond is K x K.
  * "padcap" / "padcap+1": bonds forced to K (K + 1) by zero-padding a small random chain and mixing each padded bond with a
    seeded orthogonal (unitary) gauge.  The exact gauge sweep shrinks these bonds to what the cuts can carry (<= 64), so the
    carries stay small: these cases check the routing by the operand's bond and the zeros of a rank-deficient bond, not the
    kernel at its cap."""
import functools

import numpy as np
import pytest

from helpers import random_mps_data, random_mpo_data, saturated_profile

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CAP = {np.float64: 138, np.complex128: 97}
CAP_TENSORS = {np.float64: 16, np.complex128: 14}             # 2 ceil(log2 K): the shortest chain whose middle cut carries rank K
DTYPES = {"f64": np.float64, "c64": np.complex128}


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


def _tol(n_tensors, chi_max):
    return 64.0 * n_tensors * chi_max * EPS


# ---------------------------------------------------------------- the yardstick
def _dense_chain(data):
    """The chain contracted to one tensor with the physical legs in site order (2 per MPS site, 2 x 2 per MPO site)."""
    T = data[0][0]
    for A in data[1:]:
        T = np.tensordot(T, A, axes=([-1], [0]))
    return T[..., 0]


def _reference(data):
    """(spectra, norm): the singular values of the dense tensor at every cut, normalised and padded with zeros to the bond."""
    T = _dense_chain(data)
    pd = int(np.prod(data[0].shape[1:-1]))
    n = len(data)
    nrm = np.linalg.norm(T.reshape(-1))
    out = []
    for k in range(1, n):
        s = np.linalg.svd(T.reshape(pd ** k, -1), compute_uv=False) / nrm
        bond = data[k].shape[0]
        full = np.zeros(bond)
        m = min(bond, s.size)
        full[:m] = s[:m]
        assert s[m:].size == 0 or s[m:].max() <= 1e-14     # the bond can carry the state
        out.append(full)
    return out, nrm


def _decaying(data):
    """Every site scaled by 0.7^j along its right bond index."""
    out = []
    for A in data:
        w = 0.7 ** np.arange(A.shape[-1])
        out.append(A * w.reshape((1,) * (A.ndim - 1) + (-1,)))
    return out


def _unitary(k, rng, dtype):
    M = rng.standard_normal((k, k))
    if np.issubdtype(dtype, np.complexfloating):
        M = M + 1j * rng.standard_normal((k, k))
    Q, _ = np.linalg.qr(M)
    return Q.astype(dtype)


def _forced_bonds(data, which, K, rng, dtype):
    """Bonds `which` (0-based) of the chain zero-padded to K and mixed with a seeded unitary gauge: the same state."""
    data = [A.copy() for A in data]
    for b in which:
        A, B = data[b], data[b + 1]
        chi = A.shape[-1]
        G = _unitary(K, rng, dtype)
        Ap = np.zeros(A.shape[:-1] + (K,), dtype=dtype)
        Ap[..., :chi] = A
        Bp = np.zeros((K,) + B.shape[1:], dtype=dtype)
        Bp[:chi] = B
        data[b] = np.tensordot(Ap, G, axes=([-1], [0]))
        data[b + 1] = np.tensordot(G.conj().T, Bp, axes=([1], [0]))
    return data


def _mps_case(name):
    kind, dt = name.rsplit("-", 1)
    dtype = DTYPES[dt]
    rng = np.random.default_rng(sum(ord(c) for c in name))     # one seed per case
    if kind == "n2chi2":
        return random_mps_data(saturated_profile(2, 2), rng, dtype)
    if kind == "n10chi16":
        return random_mps_data(saturated_profile(10, 16), rng, dtype)
    if kind == "n12chi17":
        return random_mps_data(saturated_profile(12, 17), rng, dtype)
    if kind == "n14chi64":
        return random_mps_data(saturated_profile(14, 64), rng, dtype)
    if kind == "n14chi65":
        return random_mps_data(saturated_profile(14, 65), rng, dtype)
    if kind == "n12decay":
        return _decaying(random_mps_data(saturated_profile(12, 32), rng, dtype, normalize=False))
    if kind in ("cap", "cap+1"):
        K = CAP[dtype] + (1 if kind == "cap+1" else 0)
        return random_mps_data(saturated_profile(CAP_TENSORS[dtype], K), rng, dtype)
    if kind in ("padcap", "padcap+1"):
        K = CAP[dtype] + (1 if kind == "padcap+1" else 0)
        base = random_mps_data(saturated_profile(14, 8), rng, dtype)
        return _forced_bonds(base, (5, 6, 7), K, rng, dtype)
    if kind == "nonminimal":
        return random_mps_data([4, 4, 2], rng, dtype)
    if kind == "product3":
        n = 6
        dims = [1] + [3] * (n - 1) + [1]
        data = []
        for i in range(n):
            A = np.zeros((dims[i], 2, dims[i + 1]), dtype=dtype)
            v = rng.standard_normal(2) + (1j * rng.standard_normal(2) if dt == "c64" else 0)
            A[0, :, 0] = v
            data.append(A)
        return data
    raise KeyError(name)


MPS_KINDS = ["n2chi2", "n10chi16", "n12chi17", "n14chi64", "n14chi65", "n12decay", "cap", "cap+1", "padcap", "padcap+1",
             "nonminimal", "product3"]
MPS_CASES = [f"{k}-{d}" for k in MPS_KINDS for d in DTYPES]
MPO_CASES = ["qft6", "dt3", "random5D6-f64", "random5D6-c64"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(data, reference spectra, reference norm) of a case, made once and left unchanged."""
    data = _mps_case(name)
    for A in data:
        A.setflags(write=False)
    spectra, nrm = _reference(data)
    return data, spectra, nrm


def _carry_rows(bonds, pd=2):
    """Rows k_b of the carry C_b (k_b x c_b) of every bond, and its columns c_b: the shapes of the two sweeps restated.  The exact
    right gauge shrinks a bond to what its right neighbour can carry (c_b = min(bond_b, pd c_{b+1})), the left-to-right sweep
    gives k_b = min(pd k_{b-1}, c_b)."""
    cols = list(bonds)
    nxt = 1
    for b in range(len(bonds) - 1, -1, -1):
        cols[b] = min(bonds[b], pd * nxt)
        nxt = cols[b]
    rows, k = [], 1
    for c in cols:
        k = min(pd * k, c)
        rows.append(k)
    return rows, cols


def _check_blocks(got, want, bonds, tol):
    assert len(got) == len(want) == len(bonds)
    worst = 0.0
    for k, (g, w, b) in enumerate(zip(got, want, bonds)):
        assert g.dtype == np.float64 and g.shape == (b,), k
        assert np.all(g >= 0.0) and np.all(np.diff(g) <= 0.0), (k, g)
        assert abs(np.sum(g * g) - 1.0) <= tol, (k, np.sum(g * g) - 1.0)
        worst = max(worst, np.abs(g - w).max())
        assert np.abs(g - w).max() <= tol, (k, np.abs(g - w).max(), tol)
    return worst


def _snapshot(x, mps=True):
    bonds = list(x.bond_dims)
    return [x.site(i) for i in range(len(bonds) + 1)], bonds, (x.amplitude if mps else None)


def _same(a, b):
    return a[1] == b[1] and a[2] == b[2] and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))


# ---------------------------------------------------------------- spectra against the dense SVD
@pytest.mark.parametrize("name", MPS_CASES)
def test_mps_spectra_match_the_dense_svd(qil, name):
    data, want, _ = _case(name)
    psi = qil.SignalMPS([np.array(A) for A in data], amplitude=1.75)
    before = _snapshot(psi)
    got = qil.bond_spectra(psi)
    assert _same(before, _snapshot(psi))                       # sites, bonds and amplitude bit-identical
    bonds = [A.shape[-1] for A in data[:-1]]
    worst = _check_blocks(got, want, bonds, _tol(len(data), max(bonds)))
    print(f"{name}: worst |s - s_ref| {worst:.2e} (bound {_tol(len(data), max(bonds)):.2e})")
    kind, dt = name.rsplit("-", 1)
    rows, cols = _carry_rows(bonds)
    K = CAP[DTYPES[dt]]
    if kind in ("cap", "cap+1"):                # the carry of the middle bond is really K x K (K + 1 x K + 1: the SVD route)
        mid = len(bonds) // 2
        want_side = K + (kind == "cap+1")
        assert bonds[mid] == max(bonds) == want_side and (rows[mid], cols[mid]) == (want_side, want_side)
        assert max(c for c in cols if c <= K) == (K if kind == "cap" else 2 ** int(np.log2(K)))     # the largest staged carry
    if kind in ("padcap", "padcap+1"):          # padded bonds shrink in the gauge sweep: routing and zeros only
        assert max(bonds) == K + (kind == "padcap+1") and max(cols) <= 64
    if name.startswith("nonminimal"):
        assert np.all(got[0][:2] > 0.0) and np.all(got[0][2:] == 0.0)       # the cut carries two values: exact zeros behind
    if name.startswith("product3"):
        for g in got:
            assert abs(g[0] - 1.0) <= _tol(len(data), 3) and np.all(g[1:] <= _tol(len(data), 3))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_paired_chain_from_signal_ztmps(qil, dt):
    rng = np.random.default_rng(77)
    t = np.arange(32) / 32.0
    x = np.exp(-1.5 * t) * np.cos(2 * np.pi * 3.2 * t) + 0.05 * rng.standard_normal(32)
    if dt == "c64":
        x = x + 1j * np.exp(-0.7 * t) * np.sin(2 * np.pi * 5.1 * t)
    psi = qil.signal_ztmps(x.astype(DTYPES[dt]))
    assert isinstance(psi, qil.ZTMPS) and psi.ntensors == 10
    before = _snapshot(psi)
    data = before[0]
    want, nrm = _reference(data)
    got, gn = qil.bond_spectra(psi, return_norm=True)
    assert _same(before, _snapshot(psi))
    bonds = psi.bond_dims
    assert len(got) == 9
    _check_blocks(got, want, bonds, _tol(10, max(bonds)))
    assert abs(gn - nrm) <= 1e-12 * nrm


def _mpo_case(qil, name):
    if name == "qft6":
        return qil.build_qft_mpo(6)
    if name == "dt3":
        return qil.build_dt_mpo(3, 2 * np.pi)
    dtype = DTYPES[name.rsplit("-", 1)[1]]
    rng = np.random.default_rng(31 if dtype is np.float64 else 32)
    return qil.SingleSiteMPO(random_mpo_data([6, 6, 6, 6], rng, dtype))


@pytest.mark.parametrize("name", MPO_CASES)
def test_mpo_spectra_match_the_dense_operator(qil, name):
    W = _mpo_case(qil, name)
    before = _snapshot(W, mps=False)
    data = before[0]
    want, nrm = _reference(data)
    got, gn = qil.mpo_bond_spectra(W, return_norm=True)
    assert _same(before, _snapshot(W, mps=False))
    bonds = W.bond_dims
    worst = _check_blocks(got, want, bonds, _tol(len(data), max(bonds)))
    print(f"{name}: bonds {bonds}, worst |s - s_ref| {worst:.2e}")
    assert abs(gn - nrm) <= 1e-12 * nrm                        # the Frobenius norm of the dense operator


def test_norm_out_is_the_number_norm_returns(qil):
    data, _, nrm = _case("n12chi17-c64")
    psi = qil.SignalMPS([np.array(A) for A in data], amplitude=0.5)
    _, got = qil.bond_spectra(psi, return_norm=True)
    want = qil.norm(psi)
    assert abs(got - want) <= 1e-12 * want
    assert abs(got - nrm) <= 1e-12 * nrm


@pytest.mark.parametrize("name", ["n12chi17-f64", "cap-c64", "cap-f64", "cap+1-f64"])
def test_the_svd_route_agrees_with_the_default(qil, name, monkeypatch):
    data, want, _ = _case(name)
    psi = qil.SignalMPS([np.array(A) for A in data])
    bonds = [A.shape[-1] for A in data[:-1]]
    tol = _tol(len(data), max(bonds))
    monkeypatch.delenv("QIL_SPECTRA_ROUTE", raising=False)
    default = qil.bond_spectra(psi)
    monkeypatch.setenv("QIL_SPECTRA_ROUTE", "svd")              # monkeypatch restores the environment afterwards
    by_svd = qil.bond_spectra(psi)
    monkeypatch.delenv("QIL_SPECTRA_ROUTE")
    _check_blocks(by_svd, want, bonds, tol)
    for a, b in zip(default, by_svd):
        assert np.abs(a - b).max() <= tol


@pytest.mark.parametrize("sign", [+1, -1])
def test_a_norm_whose_square_leaves_the_double_range(qil, sign):
    """Every site times 2^(+-50): the norm is 2^(+-600) times the original, its square is not a double."""
    data, want, nrm = _case("n12chi17-f64")
    scaled = [np.ldexp(np.array(A), sign * 50) for A in data]
    psi = qil.SignalMPS(scaled)
    got, gn = qil.bond_spectra(psi, return_norm=True)
    bonds = [A.shape[-1] for A in data[:-1]]
    _check_blocks(got, want, bonds, _tol(12, 17))
    expect = float(np.ldexp(nrm, sign * 600))
    assert np.isfinite(expect) and expect > 0.0
    assert abs(gn - expect) <= 1e-12 * expect


# ---------------------------------------------------------------- the helpers against compress
@pytest.mark.parametrize("maxdim", [4, 8])
def test_truncation_sandwich(qil, maxdim):
    """lower - s <= distance(psi, compress(psi, maxdim, tol = 0)) / |psi| <= upper + s with s = 2 sqrt((N - 1) 1e-12):
    compress's two gauge passes each run at canonicalize!'s fixed relative cut-off 1e-12 per bond.  A numpy TT-SVD of a chain of
    this kind gave 0.082 <= 0.102 <= 0.108 at maxdim 4 and 1.39e-3 <= 2.33e-3 <= 2.35e-3 at maxdim 8."""
    data, _, nrm = _case("n12decay-f64")
    psi = qil.SignalMPS([np.array(A) for A in data])
    lower, upper = qil.truncation_error_bounds(psi, maxdim)
    trunc = psi.copy()
    qil.compress(trunc, maxdim=maxdim, tol=0.0)
    assert max(trunc.bond_dims) <= maxdim
    d = qil.distance(psi, trunc) / (psi.amplitude * qil.norm(psi))
    s = 2.0 * np.sqrt(11 * 1e-12)
    print(f"maxdim {maxdim}: {lower:.4e} <= {d:.4e} <= {upper:.4e}")
    assert 0.0 < lower <= upper
    assert lower - s <= d <= upper + s
    if maxdim == 8:
        assert qil.required_maxdim(psi, upper) <= 8


# ---------------------------------------------------------------- errors
def test_a_zero_state_is_a_domain_error(qil):
    data = [np.array(A) for A in _case("n10chi16-f64")[0]]
    data[4] = np.zeros_like(data[4])
    psi = qil.SignalMPS(data)
    with pytest.raises(qil.QilDomainError, match="bond_spectra: zero or non-finite state"):
        qil.bond_spectra(psi)
    W = qil.SingleSiteMPO([np.zeros((1, 2, 2, 2)), np.ones((2, 2, 2, 1))])
    with pytest.raises(qil.QilDomainError, match="bond_spectra: zero or non-finite state"):
        qil.mpo_bond_spectra(W)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_state_that_cancels_to_zero(qil, dt):
    """v w u - v w u with no zero site.  The header promises QIL_EDOMAIN when the carry comes out exactly zero and otherwise the
    spectrum of the rounding residue, with a norm at rounding level: either way nothing hangs, faults or returns NaN."""
    dtype = DTYPES[dt]
    v, w, u = (np.array(x, dtype=dtype) for x in ([3.0, -1.0], [0.5, 2.0], [1.0, 4.0]))
    A0 = np.zeros((1, 2, 2), dtype=dtype)
    A0[0, :, 0] = A0[0, :, 1] = v
    A1 = np.zeros((2, 2, 2), dtype=dtype)
    A1[0, :, 0] = A1[1, :, 1] = w
    A2 = np.zeros((2, 2, 1), dtype=dtype)
    A2[0, :, 0], A2[1, :, 0] = u, -u
    psi = qil.SignalMPS([A0, A1, A2])
    before = _snapshot(psi)
    try:
        spectra, nrm = qil.bond_spectra(psi, return_norm=True)
    except qil.QilDomainError as e:
        assert "bond_spectra: zero or non-finite state" in str(e)
    else:
        scale = np.linalg.norm(v) * np.linalg.norm(w) * np.linalg.norm(u)
        assert np.isfinite(nrm) and nrm <= 1e-14 * scale
        assert all(np.all(np.isfinite(s)) and np.all(s >= 0.0) for s in spectra)
    assert _same(before, _snapshot(psi))


def test_a_single_site_has_no_bonds(qil):
    psi = qil.SignalMPS([np.array([3.0, -4.0]).reshape(1, 2, 1)], amplitude=2.0)
    spectra, nrm = qil.bond_spectra(psi, return_norm=True)
    assert spectra == [] and abs(nrm - 5.0) <= 1e-14 * 5.0


def test_failed_calls_leave_no_device_memory_behind(qil):
    ctx = qil.default_context()
    data, want, _ = _case("n10chi16-c64")
    psi = qil.SignalMPS([np.array(A) for A in data], amplitude=0.25)
    before = _snapshot(psi)
    ref = qil.bond_spectra(psi)
    in_use = ctx.mem_info()["pool_in_use"]
    failures, got = 0, None
    for j in range(0, 4000):
        ctx.fail_alloc_after(j)
        try:
            got = qil.bond_spectra(psi)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, j
        assert ctx.mem_info()["pool_in_use"] == in_use, j
        if not failed:
            break
        failures += 1
    assert got is not None and failures >= 20, failures
    assert _same(before, _snapshot(psi))
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_example_runs(qil):
    """examples/bond_spectrum.py asserts what it prints (unit blocks, the sandwich around compress's distance); run in this
    process."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bond_spectrum", os.path.join(root, "examples", "bond_spectrum.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main()
    assert res["needs"][1e-4] >= res["needs"][1e-1] >= 1 and res["distance"] <= 1e-3 + 1e-5
