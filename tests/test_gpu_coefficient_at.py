"""The read-out by index on the device (qil.coefficient_at) against longdouble references, case by case
(tests/index_readout_cases.py): every case under QIL_COEFFICIENT_AT_ROUTE unset and under `wave` and `bits` wherever the forced
route fits, every valid row within its own rounding bound, every row out of range NaN.  The bit order is pinned to an existing
verb: for n <= 12 the values are mps_to_vector's at the same indices.  Each test prints its worst err / bound (pytest -s)."""
import gc

import numpy as np
import pytest

import index_readout_cases as X

pytestmark = pytest.mark.gpu

FORCED = [None, "wave", "bits"]


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
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    gc.collect()
    assert qil.default_context().unowned_bytes() == 0


def _psi(qil, c):
    data, idx = X.operands(c)
    return (qil.ZTMPS if c.p["paired"] else qil.SignalMPS)(data, amplitude=X.AMPLITUDE), idx


def _set_route(monkeypatch, forced):
    if forced is None:
        monkeypatch.delenv("QIL_COEFFICIENT_AT_ROUTE", raising=False)
    else:
        monkeypatch.setenv("QIL_COEFFICIENT_AT_ROUTE", forced)


@pytest.mark.parametrize("forced", FORCED, ids=["auto", "wave", "bits"])
@pytest.mark.parametrize("c", X.CASES, ids=[c.name for c in X.CASES])
def test_device_within_bound(qil, torch, monkeypatch, c, forced):
    dims = X.dims_of(c.p["bonds"])
    assert qil.coefficient_at_route(dims) == c.route
    _set_route(monkeypatch, forced)
    psi, idx = _psi(qil, c)
    dev = torch.from_numpy(idx).cuda()
    out = qil.coefficient_at(psi, dev)
    assert out.is_cuda and out.shape == (len(idx),)
    assert out.dtype == (torch.float64 if c.dtype == "f64" else torch.complex128)
    again = qil.coefficient_at(psi, dev)
    got, ok = out.cpu().numpy(), X.valid(c)
    assert got.tobytes() == again.cpu().numpy().tobytes(), "a repeated call returned other bits"
    worst = X.check(got[ok], X.reference(c), c.name)
    print(f"{c.name} [{forced or 'auto'} -> {qil.coefficient_at_route(dims, forced)}]: worst err / bound {worst:.3g}")
    bad = got[~ok]
    assert np.isnan(bad.real).all() and (c.dtype == "f64" or np.isnan(bad.imag).all())
    if c.p["paired"]:                                      # the same numbers as the (k, l) table of the dense tensor
        grid = X.grid_reference(c)
        X.check(got.reshape(np.asarray(grid.value).shape), grid, c.name + " grid")
    dup = np.flatnonzero(idx == idx[-1])
    assert (got[dup] == got[dup[0]]).all() or not ok[dup[0]], "equal indices returned different values"


@pytest.mark.parametrize("forced", FORCED, ids=["auto", "wave", "bits"])
@pytest.mark.parametrize("name", ["one_site", "two_sites", "threshold_bond%d_count300" % X.CAP, "threshold_bond%d_count300" % (X.CAP + 1), "paired_grid"])
@pytest.mark.parametrize("dt", sorted(X.DTYPES))
def test_bit_order_is_mps_to_vectors(qil, torch, monkeypatch, name, dt, forced):
    """coefficient_at(psi, idx)[j] == mps_to_vector(psi)[idx[j]] within the sum of both bounds (the table's cases of n <= 12
    tensors).  The dense read-out's bound is the block bound of readout_cases."""
    import readout_cases as R
    c = X.BY_NAME[f"{name}-{dt}-random"]
    _set_route(monkeypatch, forced)
    psi, idx = _psi(qil, c)
    data, _ = X.operands(c)
    vec = qil.mps_to_vector(psi)
    got = qil.coefficient_at(psi, torch.from_numpy(idx).cuda()).cpu().numpy()
    dense_bound = R.bound(R.dense_tensor(data, R.modulus).reshape(-1)[idx], R.block_qs(X.dims_of(c.p["bonds"])))
    err = np.abs(got - vec[idx])
    assert (err <= np.asarray(X.reference(c).bound) + np.asarray(dense_bound)).all(), float(err.max())


def test_count_zero_is_a_no_op_and_host_indices_raise(qil, torch):
    c = X.BY_NAME["two_sites-c64-random"]
    psi, idx = _psi(qil, c)
    out = qil.coefficient_at(psi, torch.empty(0, dtype=torch.int64, device="cuda"))
    assert out.is_cuda and out.shape == (0,) and out.dtype == torch.complex128
    for host in (idx, torch.from_numpy(idx), list(idx)):
        with pytest.raises(TypeError, match="coefficient_batch"):
            qil.coefficient_at(psi, host)
    with pytest.raises(ValueError, match="1-D int64"):
        qil.coefficient_at(psi, torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="1-D int64"):
        qil.coefficient_at(psi, torch.zeros((2, 2), dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError, match="unsupported operand types"):
        qil.coefficient_at(None, torch.zeros(4, dtype=torch.int64, device="cuda"))


def test_the_c_entry_refuses_what_the_header_says(qil, torch):
    import ctypes as C
    import importlib
    L = importlib.import_module("qilaplace_jl_amd._lib")
    psi, _ = _psi(qil, X.BY_NAME["two_sites-f64-random"])
    buf = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    assert L.lib.qil_coefficient_at(psi.handle, 0, None, None) == 0
    assert L.lib.qil_coefficient_at(psi.handle, -1, C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr())) == 7
    assert "count = -1" in L.last_error()
    assert L.lib.qil_coefficient_at(psi.handle, 4, None, C.c_void_p(out.data_ptr())) == 7 and "null argument" in L.last_error()
    long = qil.SignalMPS([np.ones((1, 2, 1))] * 63)
    assert L.lib.qil_coefficient_at(long.handle, 4, C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr())) == 7
    assert "63 tensors outside 1 .. 62" in L.last_error()
