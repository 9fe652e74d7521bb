"""GPU tests of the signal encoders (signal_mps_impl, svd_sweep, compress_tt(_root), rsvd_rowmajor, ztmps_from_sites and the
kernels sumsq_partial, scale_inplace, scale_copy, site_from_vh, site_from_chunk, fuse_delta of csrc/qil_truncate.hip), one
branch at a time.  tests/encode_cases.py holds the table, the planted signals and the references; tests/
test_encode_cases_oracle.py checks them on the CPU.

Every tolerance here is one of
  * 1e-12 max|x| (states that discard nothing above rounding) and 1e-14 (entries that must vanish): the project's own;
  * the tensor-train bound sqrt(sum of the reference's discarded weights) |x|, times 1.01, for truncated SVD encodes;
  * E.sumsq_bound, derived there from the summation order of sumsq_partial;
  * 10 x the oracle's own error (8 seeds, floor 1e-12) where the sketch does not cover the rank: MEASUREMENTS.md.
The routes (exact / sketch, l0, deflated width of every bisection node) are read from the QIL_RSVD_DEBUG lines of ONE fresh
child process that runs every RSVD case (this file, run as a script)."""
import gc
import hashlib
import importlib
import json
import os
import subprocess
import sys
import tempfile
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import encode_cases as E

pytestmark = pytest.mark.gpu

SVD_IDS = [c.name for c in E.SVD_CASES]
RSVD_IDS = [c.name for c in E.RSVD_CASES]


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    gc.collect()
    assert qil.default_context().unowned_bytes() == 0


def _left_isometry(t):
    q = t.reshape(-1, t.shape[2])
    return float(np.abs(q.conj().T @ q - np.eye(q.shape[1])).max())


def _norm2(v):
    v = np.asarray(v)
    return float(np.sqrt((np.abs(v.astype(E.CLD if np.iscomplexobj(v) else E.LD)) ** 2).sum()))


def _check_amplitude(psi, x):
    """psi.amplitude against the longdouble 2-norm of the samples handed over, within E.sumsq_bound."""
    _, amp, n = E.prepare(x)
    count = 2 ** n * (2 if np.iscomplexobj(x) else 1)
    rel = abs(float((E.LD(psi.amplitude) - amp) / amp))
    assert rel <= E.sumsq_bound(count), (rel, E.sumsq_bound(count))
    return rel


def _digest(sites):
    h = hashlib.sha256()
    for t in sites:
        h.update(np.asfortranarray(t).tobytes(order="F"))
    return h.hexdigest()


def _same_sites(a, b):
    a, b = a.to_host(), b.to_host()
    return len(a) == len(b) and all(s.shape == t.shape and np.array_equal(s, t) for s, t in zip(a, b))


# ---------------------------------------------------------------- the SVD sweep
@pytest.mark.parametrize("c", E.SVD_CASES, ids=SVD_IDS)
def test_svd_case(qil, c):
    x, xl, ref = E.samples(c), E.signal(c), E.reference(c)
    psi = qil.signal_mps(x, **c.kwargs)
    n, sites = ref.n, psi.to_host()
    big, nrm = float(np.abs(xl).max()), _norm2(xl)
    # 1. bond dimensions (inside a cluster the kept subspace, and with it the later ranks, is a choice)
    if c.cluster:
        assert len(psi.bond_dims) == n - 1 and max(psi.bond_dims) <= c.maxdim
    else:
        assert psi.bond_dims == ref.bond_dims, (psi.bond_dims, ref.bond_dims)
    # 2. reconstruction against the longdouble signal
    v = qil.mps_to_vector(psi)
    if c.exact:
        err, tol = float(np.abs(v - xl).max()), 1e-12 * big
    else:
        if c.cluster:       # subspace-independent: the values of the ORIGINAL unfoldings beyond maxdim (interlacing)
            disc = sum(float((s[c.maxdim:] ** 2).sum()) for s in E.unfolding_spectra(ref.xhat, n))
        else:
            disc = ref.discarded
        err, tol = _norm2(v - xl), 1.01 * np.sqrt(disc) * nrm + 1e-12 * big
        assert err > 1e-9 * nrm                                    # (the case does truncate)
    assert err <= tol, (err, tol)
    # 3. gauge: left isometries, the last site carries the norm
    iso = max(_left_isometry(t) for t in sites[:-1]) if n > 1 else 0.0
    assert iso <= 1e-12, iso
    last = float(np.linalg.norm(sites[-1]))
    if c.cluster:
        assert last <= 1 + 1e-12
    else:
        assert abs(last - float(np.linalg.norm(ref.sites[-1]))) <= 1e-12 and (not c.exact or abs(last - 1) <= 1e-12), last
    # 4. Schmidt values of the state that was kept
    dsig = 0.0
    if not c.cluster and n > 1:
        want = E.unfolding_spectra(E.dense(ref.sites), n)
        got = qil.bond_spectra(psi)
        for b in range(n - 1):                                        # 1e-12 relative to the largest value of the bond
            r = ref.bond_dims[b]
            dsig = max(dsig, float(np.abs(got[b] - want[b][:r]).max() / want[b][0]))
        assert dsig <= 1e-12, dsig
    # 6. amplitude
    damp = _check_amplitude(psi, x)
    print(f"{c.name}: bonds {psi.bond_dims} err {err:.2e} (tol {tol:.2e}) isometry {iso:.2e} sigma {dsig:.2e} amplitude {damp:.2e}")


# ---------------------------------------------------------------- the bisection
@pytest.mark.parametrize("c", E.RSVD_CASES, ids=RSVD_IDS)
def test_rsvd_case(qil, c):
    x, xl, ref = E.samples(c), E.signal(c), E.reference(c)
    psi = qil.signal_mps(x, **c.kwargs)
    sites = psi.to_host()
    big = float(np.abs(xl).max())
    err = float(np.abs(qil.mps_to_vector(psi) - xl).max())
    if c.refill:
        # the refilled columns are orthonormalised rounding noise: what ranks the children find in them is not determined
        root = E.mid_of(0, ref.n - 1)
        assert psi.bond_dims[root] == ref.bond_dims[root] == c.mindim, psi.bond_dims
        tol = 1e-12 * big
    elif ref.covered:
        assert psi.bond_dims == ref.bond_dims, (psi.bond_dims, ref.bond_dims)
        assert c.exact
        tol = 1e-12 * big
    else:
        # measured on the oracle, never on the library: its error on this case at equal (k, p, q), worst of 8 seeds, times 10
        # (the device draws another Omega)
        tol = max(E.UNCOVERED_MARGIN * E.oracle_rsvd_error(c), E.UNCOVERED_FLOOR) * big
    assert err <= tol, (err, tol)
    # the left children of the bisection are U factors: isometries.  Where mindim keeps more columns than the operand has rank
    # (refill), the left vectors of singular values at rounding level are not orthonormal -- measured 0.14 / 0.85 -- and carry no
    # weight; what must hold there is the isometry on the directions that do carry weight (_weighted_isometry).
    iso = max([_left_isometry(sites[i]) for i in ref.left_leaves] + [0.0])
    wiso = max([_weighted_isometry(sites, i) for i in ref.left_leaves] + [0.0])
    assert ref.left_leaves and (c.refill or iso <= 1e-12), iso
    assert wiso <= 1e-12, wiso
    damp = _check_amplitude(psi, x)
    print(f"{c.name}: bonds {psi.bond_dims} err {err:.2e} (tol {tol:.2e}) isometry {iso:.2e} weighted {wiso:.2e} amplitude {damp:.2e}")


def _weighted_isometry(sites, i):
    """The isometry defect of site i on the directions of its right bond that carry weight: with Q the site as a matrix,
    D = Q^H Q - 1 and R the chain to the right of it (bond x samples), max |W^1/2 D W^1/2| / |W|_2 for W = R R^H -- the
    non-zero part of R^H D R, what a lost isometry would change in the state's norm.  A bond direction that R gives no weight
    drops out; a defect between two weighted directions does not."""
    Q = sites[i].reshape(-1, sites[i].shape[2])
    R = sites[i + 1].reshape(sites[i + 1].shape[0], -1)
    for A in sites[i + 2:]:
        R = (R.reshape(-1, A.shape[0]) @ A.reshape(A.shape[0], -1)).reshape(Q.shape[1], -1)
    w, V = np.linalg.eigh(R @ R.conj().T)
    half = (V * np.sqrt(np.clip(w, 0, None))) @ V.conj().T
    D = Q.conj().T @ Q - np.eye(Q.shape[1])
    return float(np.abs(half @ D @ half).max() / w.max())


def _route_runs():
    """This file as a script in a fresh process: {case name: {depth: {"err": stderr text, "sites": digest}}, "plain": text}."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "routes.json")
        env = {k: v for k, v in os.environ.items() if k not in ("QIL_RSVD_DEBUG", "QIL_ENCODE_PAR_DEPTH")}
        done = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, timeout=300, capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
        with open(out) as f:
            return json.load(f)


@pytest.fixture(scope="module")
def routes():
    return _route_runs()


@pytest.mark.parametrize("c", E.RSVD_CASES, ids=RSVD_IDS)
def test_rsvd_routes(qil, routes, c):
    """One line per rsvd_rowmajor call: branch, l0 and the deflated width are the predicted ones, in the order of the
    sequential recursion under QIL_ENCODE_PAR_DEPTH=0 and as a set otherwise; concurrent and sequential sites are the same bits."""
    want = [nd.key for nd in E.reference(c).nodes]
    assert want and c.route
    runs = routes[c.name]
    for depth in c.par_depths:
        got = [tuple(t) for t in E.parse_routes(runs[str(depth)]["err"])]
        if c.refill:
            assert got[0] == want[0] and len(got) == len(want), (got, want)         # (below the root: ranks of rounding noise)
        elif depth == "0":
            assert got == want, (got, want)
        else:
            assert sorted(got, key=repr) == sorted(want, key=repr), (got, want)
    assert len({runs[str(d)]["sites"] for d in c.par_depths}) == 1
    # the same bits without the variable, in this process
    psi = qil.signal_mps(E.samples(c), **c.kwargs)
    assert _digest(psi.to_host()) == runs["0"]["sites"]


def test_no_route_line_without_the_variable(routes):
    assert "[rsvd]" not in routes["plain"] and routes["plain_sites"] == routes["rsvd-deflated-r7-n12-f64"]["0"]["sites"]


# ---------------------------------------------------------------- the paired chain
def _paired_bits(n, main, copy):
    bits = np.empty((len(main), 2 * n), dtype=np.uint8)
    for i in range(n):
        bits[:, 2 * i] = (main >> (n - 1 - i)) & 1
        bits[:, 2 * i + 1] = (copy >> (n - 1 - i)) & 1
    return bits


def _check_paired(qil, zt, xl, n, diag_tol):
    """Off-diagonal coefficients (main != copy at any site) vanish to 1e-14, the diagonal is the signal."""
    if n <= 4:
        main, copy = [a.reshape(-1) for a in np.meshgrid(np.arange(2 ** n), np.arange(2 ** n), indexing="ij")]
    else:
        rng = np.random.default_rng(n)
        main = np.concatenate([np.arange(2 ** n), rng.integers(0, 2 ** n, 256)])
        copy = np.concatenate([np.arange(2 ** n), np.zeros(256, dtype=np.int64)])
        copy[2 ** n:] = main[2 ** n:] ^ (1 << rng.integers(0, n, 256)) ^ (rng.integers(0, 2 ** n, 256) & rng.integers(0, 2 ** n, 256))
        copy[2 ** n:] = np.where(copy[2 ** n:] == main[2 ** n:], main[2 ** n:] ^ 1, copy[2 ** n:])
    co = qil.coefficient_batch(zt, _paired_bits(n, main, copy))
    off = main != copy
    assert off.sum() >= min(256, 4 ** n - 2 ** n)
    offmax = float(np.abs(co[off]).max())
    assert offmax <= 1e-14, offmax
    d = np.argsort(main[~off])
    derr = float(np.abs(co[~off][d] - xl).max()) if diag_tol[0] == "max" else _norm2(co[~off][d] - xl)
    assert derr <= diag_tol[1], (derr, diag_tol)
    return offmax, derr


@pytest.mark.parametrize("name,cutoff,maxdim", E.PAIRED, ids=[f"{nm}-maxdim{md}" for nm, _, md in E.PAIRED])
def test_paired_case(qil, name, cutoff, maxdim):
    c = E.BY_NAME[name]
    x, xl = E.samples(c), E.signal(c)
    kw = dict(c.kwargs, cutoff=cutoff, maxdim=maxdim)
    ref = E.reference_encode(x, **dict(c.ref_kwargs, cutoff=cutoff, maxdim=maxdim))
    data, copy_bonds = E.reference_paired(ref, cutoff, maxdim)
    zt = qil.signal_ztmps(x, **kw)
    assert zt.bonds_main == ref.bond_dims and zt.bonds_copy == [b.rank for b in copy_bonds], (zt.bond_dims, ref.bond_dims)
    sites = zt.to_host()
    iso = max(_left_isometry(t) for t in sites[0::2])                     # every core_main
    assert iso <= 1e-12, iso
    big, nrm = float(np.abs(xl).max()), _norm2(xl)
    if maxdim is None:
        tol = ("max", 1e-12 * big)
    else:
        # sites 1 .. i-1 are left isometries and the part right of site i has 2-norm <= 1 (the state has norm <= 1), so cutting
        # the fused site i by dT moves the state by at most |dT|_F = sqrt(discarded_i) |A_i|_F; the sweep before it obeys the
        # tensor-train bound; the errors add
        moved = np.sqrt(ref.discarded) + sum(np.sqrt(b.discarded) * np.linalg.norm(A) for b, A in zip(copy_bonds, ref.sites))
        tol = ("2", 1.01 * moved * nrm + 1e-12 * big)
    offmax, derr = _check_paired(qil, zt, xl, ref.n, tol)
    # ztmps_from_mps of the same encode is the same chain, bit for bit
    again = qil.ztmps_from_mps(qil.signal_mps(x, **kw), cutoff=cutoff, maxdim=maxdim)
    assert again.bond_dims == zt.bond_dims and _same_sites(again, zt) and again.amplitude == zt.amplitude
    print(f"{name} maxdim {maxdim}: bonds {zt.bond_dims} off-diagonal {offmax:.2e} diagonal {derr:.2e} (tol {tol[1]:.2e}) isometry {iso:.2e}")


@pytest.mark.parametrize("dtype", ["f64", "c64"])
def test_paired_two_sites(qil, dtype):
    """n = 1: one signal site, two tensors, all four coefficients."""
    xl = E.norm_signal(1, dtype, 1.0)
    x = xl.astype(np.complex128 if dtype == "c64" else np.float64)
    zt = qil.signal_ztmps(x)
    assert zt.ntensors == 2 and zt.bonds_copy == [2]
    _check_paired(qil, zt, xl, 1, ("max", 1e-12 * float(np.abs(xl).max())))
    assert _left_isometry(zt.to_host()[0]) <= 1e-12
    assert _same_sites(qil.ztmps_from_mps(qil.signal_mps(x, cutoff=1e-10)), zt)


# ---------------------------------------------------------------- device-resident samples
class _Owner:
    """Device memory for the tests without any framework: `buffer` is parked in the first site of a two-site chain (HBM owned
    by the library); view(offset, length) exposes a part of it through __cuda_array_interface__."""

    class _View:
        pass

    def __init__(self, qil, buffer):
        buffer = np.ascontiguousarray(buffer)
        assert buffer.size % 2 == 0
        h = buffer.size // 2
        site0 = np.ascontiguousarray(buffer.reshape(h, 2).T[None, :, :])       # memory order (s fastest) = buffer
        self._chain = qil.SignalMPS([site0, np.zeros((h, 2, 1), dtype=buffer.dtype)])
        self._dtype = buffer.dtype

    def view(self, offset, length):
        v = self._View()
        v.__cuda_array_interface__ = {"data": (self._chain.site_device_ptr(0) + offset * self._dtype.itemsize, False),
                                      "shape": (length,), "typestr": self._dtype.str, "version": 2}
        v.keep = self
        return v

    def download(self):
        return self._chain.site(0).reshape(-1, order="F")


def _host_samples(length, dtype):
    return E.length_signal(length, dtype).astype(np.complex128 if dtype == "c64" else np.float64)


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("length", [1024, 1000], ids=["in-place", "copy"])
@pytest.mark.parametrize("dtype", ["f64", "c64"])
def test_device_resident_signals(qil, dtype, length, offset):
    """len == 2^n is read in place (scale_copy), len < 2^n is copied (scale_inplace): the same kernels see the same values as on
    the host route, so the sites are the same bits; and the owner's buffer is untouched, before, inside and behind the view."""
    x = _host_samples(length, dtype)
    buffer = _host_samples(length + 8, dtype) * 3.0
    buffer[offset:offset + length] = x
    owner = _Owner(qil, buffer)
    for kw in (dict(method="svd", cutoff=1e-12), dict(method="rsvd", k=12, p=4, q=1, cutoff=1e-12)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            host = qil.signal_mps(x, **kw)
            dev = qil.signal_mps(owner.view(offset, length), **kw)
            hz, dz = qil.signal_ztmps(x, **kw), qil.signal_ztmps(owner.view(offset, length), **kw)
        assert dev.bond_dims == host.bond_dims and dev.amplitude == host.amplitude and _same_sites(dev, host)
        assert dz.bond_dims == hz.bond_dims and _same_sites(dz, hz)
        assert np.array_equal(owner.download(), buffer)


# ---------------------------------------------------------------- the length rule
# (device-resident where len >= 2: a single sample has no owner to sit in)
LENGTH_RUNS = [(k, dt, w) for k in E.LENGTHS for dt in ("f64", "c64") for w in ("host", "device") if w == "host" or k >= 2]


@pytest.mark.parametrize("length,dtype,where", LENGTH_RUNS, ids=[f"len{k}-{dt}-{w}" for k, dt, w in LENGTH_RUNS])
def test_length_rule(qil, length, dtype, where):
    n = E.LENGTHS[length]
    x = _host_samples(length, dtype)
    if where == "device":
        owner = _Owner(qil, np.concatenate([x, x[:length % 2]]))
        operand = owner.view(0, length)
    else:
        operand = x
    if n is None:
        with pytest.raises(ValueError):
            qil.signal_mps(operand)
    else:
        if length < 2 ** n:
            with pytest.warns(UserWarning, match="zero-filling"):
                psi = qil.signal_mps(operand)
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                psi = qil.signal_mps(operand)
        assert len(psi) == n
        v = qil.mps_to_vector(psi)
        big = float(np.abs(x).max())
        assert big <= 1.0                                             # (length_signal: the 1e-14 below is absolute)
        assert np.abs(v[:length] - x).max() <= 1e-12 * big
        tail = float(np.abs(v[length:]).max()) if length < 2 ** n else 0.0
        print(f"len {length} {dtype} {where}: n {n}, zero tail {tail:.2e}")
        assert v.size == 2 ** n and tail <= 1e-14, tail
        _check_amplitude(psi, x)
    good = _host_samples(16, dtype)                                  # the same context encodes a good signal afterwards
    assert np.abs(qil.mps_to_vector(qil.signal_mps(good)) - good).max() <= 1e-12 * np.abs(good).max()


# ---------------------------------------------------------------- the norm
@pytest.mark.parametrize("name,n,dtype,scale", E.NORMS, ids=[f"{nm}-n{n}-{dt}" for nm, n, dt, _ in E.NORMS])
def test_norm(qil, name, n, dtype, scale):
    """sumsq_partial with fewer elements than threads, with exactly one grid stride and with two; samples whose squares leave
    the range of a double encode like any other (the reference's norm scales: SignalConverters.jl:36)."""
    xl = E.norm_signal(n, dtype, scale)
    x = xl.astype(np.complex128 if dtype == "c64" else np.float64)
    psi = qil.signal_mps(x, cutoff=1e-20)
    assert len(psi) == n
    rel = _check_amplitude(psi, x)
    err = float(np.abs(qil.mps_to_vector(psi) - x).max() / np.abs(x).max())
    assert err <= 1e-12, err
    print(f"{name} n={n} {dtype}: amplitude rel err {rel:.2e} (bound {E.sumsq_bound(x.size * (2 if dtype == 'c64' else 1)):.2e}), state {err:.2e}")


@pytest.mark.parametrize("dtype", ["f64", "c64"])
@pytest.mark.parametrize("bad", ["zero", "nan", "inf", "inf-and-nan"])
def test_signals_without_a_norm_are_refused(qil, bad, dtype):
    ctx = qil.default_context()
    x = _host_samples(64, dtype)
    if bad == "zero":
        x[:] = 0
    if "nan" in bad:
        x[17] = np.nan
    if "inf" in bad:
        x[40] = np.inf
    before = ctx.mem_info()["pool_in_use"]
    for encode in (qil.signal_mps, qil.signal_ztmps):
        with pytest.raises(ValueError, match="zero or non-finite norm"):
            encode(x)
        assert ctx.mem_info()["pool_in_use"] == before and ctx.unowned_bytes() == 0
    good = _host_samples(64, dtype)
    assert np.abs(qil.mps_to_vector(qil.signal_mps(good)) - good).max() <= 1e-12 * np.abs(good).max()


# ---------------------------------------------------------------- failures in the concurrent bisection
def test_allocation_failures_in_the_concurrent_bisection(qil):
    """n = 16 runs compress_tt_root's level passes and concurrent sub-trees (qil_run_batch_on, blocks moved between contexts by
    qil_ctx_transfer).  With the k-th allocation failing the call raises MemoryError or succeeds, strands nothing, and reports
    the failure itself -- not qil_ctx_free's "unknown block" from releasing an operand twice."""
    L = importlib.import_module("qilaplace_jl_amd._lib")
    c = E.BY_NAME["rsvd-concurrent-n16-f64"]
    x, ref = E.samples(c), E.reference(c)
    ctx = qil.default_context()
    outcome = {}
    # (measured: the default context makes 60 .. 66 allocations in this call -- the root node, then item 0 of each level pass; the
    # sub-trees of the last pass allocate from the worker contexts, which the injection does not reach.  k = 67 succeeds.)
    for k in list(range(0, 40, 3)) + [40, 49, 58, 67]:
        ctx.fail_alloc_after(k)
        try:
            psi = qil.signal_mps(x, **c.kwargs)
            assert psi.bond_dims == ref.bond_dims
            outcome[k] = True
            del psi
        except MemoryError as e:
            outcome[k] = False
            assert "unknown block" not in str(e), (k, str(e))
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, k
        assert "unknown block" not in L.last_error(), (k, L.last_error())
    # every k below the first success failed (an injection that stops reaching the encode would show as an early success), the
    # issue's whole range among them, and from the first success on every call succeeds
    first = min(k for k, ok in outcome.items() if ok)
    assert first > 39 and all(ok == (k >= first) for k, ok in outcome.items()), outcome
    psi = qil.signal_mps(x, **c.kwargs)                             # and the same call succeeds afterwards
    assert psi.bond_dims == ref.bond_dims
    assert np.abs(qil.mps_to_vector(psi) - E.signal(c)).max() <= 1e-12 * np.abs(x).max()


# ---------------------------------------------------------------- the child process of test_rsvd_routes
def _child(out_path):
    import qilaplace_jl_amd as q

    def captured(fn):
        """fn() with file descriptor 2 pointed at a file: what the library wrote to stderr."""
        sys.stderr.flush()
        with tempfile.TemporaryFile() as f:
            saved = os.dup(2)
            os.dup2(f.fileno(), 2)
            try:
                res = fn()
                q.default_context().synchronize()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            f.seek(0)
            return res, f.read().decode()

    out = {}
    probe = E.BY_NAME["rsvd-deflated-r7-n12-f64"]
    psi, text = captured(lambda: q.signal_mps(E.samples(probe), **probe.kwargs))
    out["plain"], out["plain_sites"] = text, _digest(psi.to_host())
    os.environ["QIL_RSVD_DEBUG"] = "1"
    for c in E.RSVD_CASES:
        out[c.name] = {}
        for depth in c.par_depths:
            if depth is None:
                os.environ.pop("QIL_ENCODE_PAR_DEPTH", None)
            else:
                os.environ["QIL_ENCODE_PAR_DEPTH"] = depth
            psi, text = captured(lambda: q.signal_mps(E.samples(c), **c.kwargs))
            out[c.name][str(depth)] = {"err": text, "sites": _digest(psi.to_host())}
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    _child(sys.argv[1])
