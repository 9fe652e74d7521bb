"""CPU-side checks of the product-vector read-out (qil_product_batch): declared, exported, bound; argument errors come back
before any device is touched; the Python front-ends check types and shapes before any native call; the host-only parts --
laplace_weights and the golden-section helper -- are checked against exact values.

The non-finite weight cannot be sent through the C entry here: the scan needs the tensor count of a live handle, and a handle
needs a device.  Its place before the activation is asserted in the source; tests/test_gpu_product.py sends it on the device."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7
U = 2.0 ** -53


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def test_product_batch_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    assert re.search(r"QIL_API\s+int\s+qil_product_batch\s*\(\s*const qil_mps\* psi,\s*int64_t nb,\s*const double\* v,\s*"
                     r"double\* out\s*\)\s*;", decl)
    assert hasattr(ctypes.CDLL(qil.LIB_PATH), "qil_product_batch")
    assert len(L.PROTOTYPES["qil_product_batch"]) == 4
    for name in ("product_batch", "laplace_weights", "laplace_sum", "power_sum", "dft_eval", "dt_eval", "zt_eval",
                 "refine_frequencies"):
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    assert "qil_product.hip" in open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "Makefile")).read()
    header = open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()
    assert "src/mps.jl:669-678" in header[header.find("Product-vector read-out"):header.find("qil_product_batch(")]


def test_argument_errors_precede_the_context_activation():
    """QIL_EINVAL_ARG for a null handle and for null weights with nb > 0, returned before the context is activated (this runs
    on a machine without a GPU: an activation would fail with QIL_EHIP instead)."""
    L = _lib()
    v = (ctypes.c_double * 8)(*([1.0, 0.0] * 4))
    out = (ctypes.c_double * 4)()
    assert L.lib.qil_product_batch(None, 2, v, out) == QIL_EINVAL_ARG
    assert "product_batch: null argument" in L.last_error()
    assert L.lib.qil_product_batch(None, 0, None, None) == QIL_EINVAL_ARG
    assert "product_batch: null argument" in L.last_error()


def test_checks_precede_the_activation_in_the_source():
    src = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_product.hip")).read()
    m = re.search(r'extern "C" int qil_product_batch\(.*?\n}\n', src, flags=re.S)
    assert m
    body = m.group(0)
    act = body.find("qil_ctx_activate")
    assert act > 0
    for needle in ("null argument", "nb <= 0 || (v && out)", "nb >= 0", "if (nb == 0) return QIL_OK;", "std::isfinite",
                   "are not finite", "row %lld, tensor %lld"):
        assert 0 <= body.find(needle) < act, needle
    assert body.count("QIL_REQUIRE") == 3 and body.rfind("QIL_REQUIRE") < act          # no check is left for after it
    assert body[:act].count("QIL_EINVAL_ARG") == 3
    assert act < body.find("qil_call_scope") < body.find("qil_scratch tmp")             # the temporaries' owners, in this order
    # the route: the marginal's decision, a per-call environment override, the cap last
    assert act < body.find("qil_readout_route(QIL_READOUT_MARGINAL") < body.find('getenv("QIL_PRODUCT_ROUTE")') \
        < body.find("wb <= kChainMaxBond")
    assert body.count("qil_stream_sync") == 1 and body.count("hipMemcpyAsync") == 1     # one download, one synchronisation


def test_the_read_out_has_kernels_of_its_own_and_leaves_the_verb_range_alone():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_product.hip")).read())
    assert re.search(r"__global__[^;{]*\bproduct_chain\b", code) and "struct combine_slices_k" in code
    assert "extern __shared__" in code and "hipFuncSetAttribute" not in code and "qil_lds_grant" not in code
    assert "qil_dev_finish_coeff(ctx, QIL_C64" in code and "qil_dev_gemm_skinny" in code
    readout = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_readout.hip")).read()
    assert "verb >= QIL_READOUT_PLAIN && verb <= QIL_READOUT_LAZY" in readout
    testing = open(os.path.join(ROOT, "include", "qilaplace_hip_testing.h")).read()
    assert "enum { QIL_READOUT_PLAIN = 0, QIL_READOUT_MARGINAL = 1, QIL_READOUT_SWEEP = 2, QIL_READOUT_LAZY = 3 };" in testing


class _Boom:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        raise AssertionError("native call made before the argument checks")


def _fake(cls):
    """a container object that never touched the device: enough for the front-end's checks"""
    x = object.__new__(cls)
    x.handle = None
    x.ctx = None
    return x


def test_python_checks_precede_native_calls(monkeypatch):
    import qilaplace_jl_amd as qil
    from qilaplace_jl_amd import ops
    L = _lib()
    boom = _Boom()
    monkeypatch.setattr(L.lib, "qil_product_batch", boom)
    good = np.ones((2, 3, 2))
    for cls in (qil.SingleSiteMPO, qil.PairedSiteMPO):
        for fn, args in ((qil.product_batch, (good,)), (qil.laplace_sum, (0.0, 0.1)), (qil.power_sum, (0.5,)),
                         (qil.dft_eval, (1.5,)), (qil.dt_eval, (1.0, 2.0)), (qil.zt_eval, (1.0, 2.0, 3.0)),
                         (qil.refine_frequencies, (3.0,))):
            with pytest.raises(TypeError, match="unsupported operand types"):
                fn(_fake(cls), *args)
    for x in (None, np.zeros((4, 2, 4)), [np.zeros((1, 2, 1))]):
        with pytest.raises(TypeError, match="product_batch: unsupported operand types"):
            qil.product_batch(x, good)
    psi = _fake(qil.SignalMPS)
    monkeypatch.setattr(ops, "_ntensors", lambda p: 3)
    for bad in (np.array([["a", "b"]] * 3)[None], np.ones((2, 3, 2), dtype=bool), np.array([[[None, 1.0]] * 3])):
        with pytest.raises(TypeError, match="product_batch: the weights must be real or complex numbers"):
            qil.product_batch(psi, bad)
    for bad in (np.ones((3, 2)), np.ones((2, 4, 2)), np.ones((2, 3, 3)), np.ones((2, 3, 2, 1)), np.ones(6)):
        with pytest.raises(ValueError, match=r"product_batch: expected weights of shape \(nb, 3, 2\)"):
            qil.product_batch(psi, bad)
    assert boom.calls == 0


def _exact_weight(sigma, c, m):
    """w^(2^m) of w = exp(-(sigma + 2 pi i c)) from exact arguments: the phase from Fraction(c) 2^m mod 1, the modulus from a
    longdouble exp of the exactly scaled sigma."""
    LD = np.longdouble
    frac = (Fraction(c) * 2 ** m) % 1                      # exact: c is a double
    if frac > Fraction(1, 2):
        frac -= 1
    ang = -2 * (4 * np.arctan(LD(1))) * (LD(frac.numerator) / LD(frac.denominator))
    mod = np.exp(-LD(sigma) * LD(2) ** m)
    return mod * np.cos(ang), mod * np.sin(ang)


@pytest.mark.parametrize("c", [0.3, 1.0 / 3.0], ids=["c0.3", "c1over3"])
@pytest.mark.parametrize("sigma", [0.0, 1e-7])
def test_laplace_weights_are_exact_to_4u(sigma, c):
    import qilaplace_jl_amd as qil
    n = 40
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended longdouble"
    w = qil.laplace_weights(sigma, c, n)
    assert w.shape == (1, n, 2) and w.dtype == np.complex128
    assert np.array_equal(w[0, :, 0], np.ones(n))
    worst = 0.0
    for i in range(n):
        m = n - 1 - i                                      # tensor 1 is the most significant bit
        re, im = _exact_weight(sigma, c, m)
        size = np.hypot(re, im)
        err = np.hypot(np.longdouble(w[0, i, 1].real) - re, np.longdouble(w[0, i, 1].imag) - im)
        if size < np.finfo(np.float64).tiny:               # below double's normal range: underflow (to zero) is the value
            assert err <= 2.0 ** -1074, (i, m, w[0, i, 1])
            continue
        worst = max(worst, float(err / size) / U)
        assert err <= 4 * U * size, (i, m, w[0, i, 1], float(err / size) / U)
    print(f"sigma {sigma} c {c}: worst relative error {worst:.2f} u")


def test_laplace_weights_broadcast_and_underflow():
    import qilaplace_jl_amd as qil
    w = qil.laplace_weights(np.array([0.0, 0.5, 2.0])[:, None], np.array([0.25, -0.125])[None, :], 12)
    assert w.shape == (6, 12, 2)
    assert w[0, 11, 1] == pytest.approx(np.exp(-2j * np.pi * 0.25), abs=1e-16)
    assert w[0, 9, 1] == 1.0                                # 0.25 * 4 = 1: the phase is exactly 1
    assert w[5, 0, 1] == 0.0                                # exp(-2 * 2048) underflows: the value
    # the lowest bit carries w itself
    z = np.clongdouble(qil.laplace_weights(1e-9, 0.3, 40)[0, 39, 1])
    assert abs(complex(z) - np.exp(-(1e-9 + 2j * np.pi * 0.3))) < 4e-16


def test_laplace_weights_raise_on_overflow():
    import qilaplace_jl_amd as qil
    with pytest.raises(ValueError, match=r"laplace_weights: .*overflows at bit m = 11"):
        qil.laplace_weights(-1.0, 0.0, 12)                  # exp(2^10) is finite, exp(2^11) is not
    assert np.isfinite(qil.laplace_weights(-1.0, 0.0, 10)).all()
    with pytest.raises(ValueError, match="finite"):
        qil.laplace_weights(np.nan, 0.0, 4)
    with pytest.raises(ValueError, match="n must be >= 1"):
        qil.laplace_weights(0.0, 0.0, 0)


def test_golden_section_helper_finds_an_off_grid_tone():
    """The search of refine_frequencies on a numpy evaluator: one tone at a non-integer frequency, several starting bins at
    once, every iteration one call."""
    from qilaplace_jl_amd import ops
    n, f_true = 10, 37.3137
    N = 2 ** n
    j = np.arange(N)
    x = np.exp(2j * np.pi * f_true * j / N)
    calls = []

    def evaluate(f):
        calls.append(len(f))
        return np.abs(np.exp(-2j * np.pi * np.outer(f, j) / N) @ x)

    f = ops._golden_maximise(evaluate, np.array([36.5, 36.9]), np.array([37.5, 37.9]), 1e-6)
    assert f.shape == (2,) and np.abs(f - f_true).max() < 2e-6, f
    assert calls[0] == 4 and set(calls[1:]) == {2}          # two probes per interval to start, then one new point each
    assert len(calls) <= 1 + 32                             # 0.618^k < 1e-6 at k = 29
    # a window that does not hold the maximum runs to its nearer edge
    g = ops._golden_maximise(evaluate, np.array([37.5]), np.array([38.0]), 1e-6)
    assert abs(g[0] - 37.5) < 2e-6


def test_julia_shim_binds_product_batch():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function product_batch\(psi::DeviceMPS, v::AbstractArray\{<:Number,3\}\)", src)
    assert "(:qil_product_batch, LIB)" in src
    assert re.search(r"export .*\bproduct_batch\b", src, flags=re.S)
    assert "`qil_product_batch`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
