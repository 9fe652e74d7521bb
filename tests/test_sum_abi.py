"""CPU-side checks of the linear combinations (qil_mps_sum, qil_mps_sum_compress): declared with their signatures, exported and
bound; null arguments, nb < 1 and non-finite coefficients come back before any device is touched; every operand check sits
ahead of the context activation, in the order of check_pair; the Python front-ends reject wrong operand types before any native
call; the state classes still do not overload `*`; the Julia shim binds both and INTEGRATION.md names them; the host tensors of
exponential_mps contract to z^j."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

SIGNATURES = {
    "qil_mps_sum": r"const qil_mps\* const\* terms,\s*int64_t nb,\s*const double\* coeffs,\s*qil_mps\*\* out",
    "qil_mps_sum_compress": r"const qil_mps\* const\* terms,\s*int64_t nb,\s*const double\* coeffs,\s*int64_t maxdim,\s*"
                            r"double tol,\s*int sweeps,\s*int64_t zip_maxdim,\s*qil_mps\*\* out",
}
ARITY = {"qil_mps_sum": 4, "qil_mps_sum_compress": 8}
VERBS = {"qil_mps_sum": "mps_sum", "qil_mps_sum_compress": "mps_sum_compress"}
FRONT_ENDS = ("linear_combination", "linear_combination_compress", "add", "sub", "scale", "exponential_mps", "exponential_sum")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _source():
    return open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_sum.hip")).read()


def test_entries_are_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    for name, args in SIGNATURES.items():
        assert re.search(r"QIL_API\s+int\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", decl), name
        assert hasattr(so, name), name
        assert len(L.PROTOTYPES[name]) == ARITY[name], name
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    assert "qil_sum.hip" in open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "Makefile")).read()


def _call(L, name, terms, nb, coeffs, out):
    if name == "qil_mps_sum":
        return L.lib.qil_mps_sum(terms, nb, coeffs, out)
    return L.lib.qil_mps_sum_compress(terms, nb, coeffs, 8, 1e-10, 1, 0, out)


def test_argument_errors_precede_the_context_activation():
    """QIL_EINVAL_ARG for null terms / out / entries, nb < 1 and non-finite coefficients, returned before the context is
    activated (this runs on a machine without a GPU: an activation would fail with QIL_EHIP instead; a non-null entry would be
    dereferenced, so the checks that need one are made on the source order below)."""
    L = _lib()
    out = ctypes.c_void_p()
    one_null = (ctypes.c_void_p * 1)(None)
    for name, verb in VERBS.items():
        assert _call(L, name, None, 1, None, ctypes.byref(out)) == QIL_EINVAL_ARG
        assert f"{verb}: null argument" in L.last_error()
        assert _call(L, name, one_null, 1, None, None) == QIL_EINVAL_ARG
        assert f"{verb}: null argument" in L.last_error()
        assert _call(L, name, one_null, 1, None, ctypes.byref(out)) == QIL_EINVAL_ARG          # a null entry
        assert f"{verb}: null argument" in L.last_error()
        for nb in (0, -3):
            assert _call(L, name, one_null, nb, None, ctypes.byref(out)) == QIL_EINVAL_ARG
            assert verb in L.last_error() and "null argument" not in L.last_error()
    assert out.value is None


def _body(src, name):
    m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", src, flags=re.S)
    assert m, name
    return m.group(0)


def test_checks_precede_the_activation_in_the_source():
    src = _source()
    for name, verb in VERBS.items():
        body = _body(src, name)
        act = body.find("qil_ctx_activate")
        assert 0 <= body.find(f'check_terms("{verb}", terms, nb, coeffs, out)') < act, name
    fused = _body(src, "qil_mps_sum_compress")
    assert 0 <= fused.find("QIL_EDOMAIN") < fused.find("qil_ctx_activate")
    assert 0 <= fused.find("sweeps >= 1") < fused.find("qil_ctx_activate")
    chk = re.search(r"int check_terms\(.*?\n}\n", src, flags=re.S).group(0)
    order = [chk.find(s) for s in ("terms && out, QIL_EINVAL_ARG", "nb >= 1, QIL_EINVAL_ARG", "terms[j], QIL_EINVAL_ARG",
                                   "std::isfinite(coeffs[j]), QIL_EINVAL_ARG", "qil_check_pair(verb, terms[0], terms[j])")]
    assert all(o >= 0 for o in order) and order == sorted(order), order
    assert '"%s: null argument"' in chk and "qil_ctx_activate" not in chk
    # the pair checks are the ones of the element-wise product, in their order, unchanged
    had = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_hadamard.hip")).read()
    assert re.search(r"int qil_check_pair\([^)]*\) \{ return check_pair\(verb, phi, psi\); \}", had)
    pair = re.search(r"int check_pair\(.*?\n}\n", had, flags=re.S).group(0)
    order = [pair.find(s) for s in ("phi->ctx == psi->ctx, QIL_EINVAL_ARG", "phi->paired == psi->paired, QIL_EINVAL_ARG",
                                    "phi->n() == psi->n(), QIL_EINVAL_LENGTH", "phi->site_ids == psi->site_ids, QIL_EINVAL_SITES")]
    assert all(o >= 0 for o in order) and order == sorted(order), order


def test_non_finite_coefficients_are_refused_before_a_handle_is_read():
    """The coefficient check runs after the null-entry check and before anything reads a handle's fields: the one entry here
    points at a zeroed buffer, not at a handle."""
    L = _lib()
    out = ctypes.c_void_p()
    dummy = ctypes.create_string_buffer(4096)
    one = (ctypes.c_void_p * 1)(ctypes.addressof(dummy))
    for name, verb in VERBS.items():
        for bad in ((np.nan, 0.0), (1.0, np.inf), (-np.inf, np.nan)):
            c = (ctypes.c_double * 2)(*bad)
            assert _call(L, name, one, 1, c, ctypes.byref(out)) == QIL_EINVAL_ARG, (name, bad)
            assert f"{verb}: coefficient 0 is not finite" in L.last_error()
    assert out.value is None
    chk = re.search(r"int check_terms\(.*?\n}\n", _source(), flags=re.S).group(0)
    assert "2 * nb" in chk                                              # (re, im) pairs: both components


def test_the_sum_has_kernels_of_its_own():
    src = _source()
    code = re.sub(r"//[^\n]*", "", src)
    assert re.search(r"__global__ __launch_bounds__\(kRows\) void site_sum_grouped\(", code)
    assert re.search(r"__global__ __launch_bounds__\(64\) void gemm_grouped_small\(", code)
    assert "mfma_step(" in code                                         # the f64 MFMA tile step: one definition, in the shared header
    utils = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_device_utils.h")).read()
    assert utils.count("void mfma_step(") == 1 and utils.count("__builtin_amdgcn_mfma_f64_16x16x4f64(") == 4
    assert "hipMemset" not in code and "qil_dev_zero" not in code      # zeros are stored by the one kernel, not by a memset
    assert code.count("site_sum_grouped<TA, TO, MIXED>") == 1           # one launch site: all sites in one grid
    assert "asm" not in code
    fused = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_truncate.hip")).read()
    assert re.search(r"\nint qil_sum_compress_impl\(", fused) and "qil_dev_gemm_grouped(" in fused
    assert re.search(r"constexpr int64_t kSumGroupedMaxBond = \d+;", fused)


class _Boom:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        raise AssertionError("native call made before the argument checks")


def _fake(cls):
    """a container object that never touched the device: enough for the front-ends' checks"""
    x = object.__new__(cls)
    x.handle = None
    x.ctx = None
    return x


def test_python_checks_precede_native_calls(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()
    for name in list(SIGNATURES) + ["qil_mps_clone", "qil_mps_nsites", "qil_mps_amplitude", "qil_mps_set_amplitude",
                                    "qil_mps_is_paired"]:
        monkeypatch.setattr(L.lib, name, boom)
    psi, zt = _fake(qil.SignalMPS), _fake(qil.ZTMPS)
    W = _fake(qil.SingleSiteMPO)
    msg = "linear_combination: unsupported operand types"
    for bad in (None, psi, np.zeros((4, 2, 4)), [], [psi, None], [psi, W], [np.zeros((1, 2, 1))], [psi, zt], [zt, psi]):
        for fn in (qil.linear_combination, qil.linear_combination_compress):
            with pytest.raises(TypeError, match=msg):
                fn(bad)
    for x in (None, W, np.zeros(3), 2.0):
        for fn in (qil.add, qil.sub):
            with pytest.raises(TypeError, match=msg):
                fn(psi, x)
            with pytest.raises(TypeError, match=msg):
                fn(x, psi)
        with pytest.raises(TypeError, match=msg):
            qil.scale(x, 2.0)
        if not isinstance(x, np.ndarray):               # numpy's reflected operators would probe the state as a sequence
            with pytest.raises(TypeError):
                psi + x
            with pytest.raises(TypeError):
                psi - x
    for fn in (qil.add, qil.sub):
        with pytest.raises(TypeError, match=msg):
            fn(psi, zt)
    with pytest.raises(TypeError):
        psi + zt
    with pytest.raises(TypeError):
        zt - psi
    with pytest.raises(TypeError, match=msg):
        qil.scale(psi, "2")
    with pytest.raises(TypeError, match=msg):
        qil.scale(psi, None)
    with pytest.raises(TypeError, match=msg):
        qil.linear_combination([psi, psi], ["a", "b"])
    with pytest.raises(ValueError, match="3 coefficients for 2 terms"):
        qil.linear_combination([psi, psi], [1, 2, 3])
    with pytest.raises(ValueError, match="1 coefficients for 2 terms"):
        qil.linear_combination_compress([psi, psi], [1j])
    assert boom.calls == 0


def test_states_overload_addition_but_not_multiplication():
    """`+`, `-` and unary `-` are the vector-space operations; `*` stays the operator application W * psi."""
    import qilaplace_jl_amd as qil
    for name in ("__add__", "__sub__", "__neg__"):
        assert name in qil.SignalMPS.__dict__, name
    assert "__mul__" not in qil.SignalMPS.__dict__ and "__mul__" not in qil.ZTMPS.__dict__
    assert "__rmul__" not in qil.SignalMPS.__dict__ and "__rmul__" not in qil.ZTMPS.__dict__


def test_julia_shim_binds_both():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function linear_combination\(terms::Vector\{<:DeviceMPS\}, coeffs=nothing\)", src)
    assert re.search(r"function linear_combination_compress\(terms::Vector\{<:DeviceMPS\}, coeffs=nothing;", src)
    assert re.search(r"Base\.:\+\(phi::DeviceMPS, psi::DeviceMPS\)", src)
    assert re.search(r"Base\.:-\(phi::DeviceMPS, psi::DeviceMPS\)", src)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SIGNATURES:
        assert f"(:{name}, LIB)" in src, name
        assert f"`{name}`" in doc, name
    for name in ("linear_combination", "linear_combination_compress"):
        assert re.search(r"export .*\b" + name + r"\b", src, flags=re.S), name


def test_documents_name_the_feature():
    import qilaplace_jl_amd as qil
    doc = " ".join(qil.exponential_sum.__doc__.split())
    assert "|z| > 1" in doc and "overflows" in doc and "underflows" in doc
    assert "TWO conjugate modes" in doc
    assert "linear_combination" in open(os.path.join(ROOT, "README.md")).read()
    assert "site_sum_grouped" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "superpose.py"))


@pytest.mark.parametrize("z", [0.998, -1.0003, np.exp(0.7312j), np.exp(-3e-3 + 2.1j), 0.5j],
                         ids=["real", "real-negative", "unit-modulus", "damped", "imaginary"])
def test_exponential_tensors_contract_to_the_powers(z):
    """x_j = z^j for j < 2^10 from the host tensors, contracted in numpy: 1e-12 of the largest entry."""
    import qilaplace_jl_amd as qil
    n = 10
    data = qil.exponential_tensors(z, n)
    assert len(data) == n and all(t.shape == (1, 2, 1) for t in data)
    want_dt = np.float64 if np.imag(z) == 0 else np.complex128
    assert all(t.dtype == want_dt for t in data)
    for i, t in enumerate(data):
        assert t[0, 0, 0] == 1
        want = np.clongdouble(z) ** (2 ** (n - 1 - i))
        assert abs(t[0, 1, 0] - want) <= 1e-14 * abs(want) + 1e-300, i
    v = data[0][0]
    for A in data[1:]:
        v = np.tensordot(v, A, axes=([-1], [0]))
    v = v[..., 0].reshape(-1)
    ref = np.asarray(z, dtype=np.clongdouble) ** np.arange(2 ** n)
    assert np.abs(v - ref).max() <= 1e-12 * np.abs(ref).max()


def test_exponential_powers_stay_accurate_and_saturate():
    """Squaring in double loses a bit per site (2^39 eps = 6e-5 at n = 40); the high-precision squaring does not: for
    z = exp(2 pi i / 2^20) the upper sites are exactly 1 to rounding.  |z| > 1 overflows to inf, |z| < 1 underflows to 0."""
    import qilaplace_jl_amd as qil
    z = complex(np.cos(2 * np.pi / 2 ** 20), np.sin(2 * np.pi / 2 ** 20))
    data = qil.exponential_tensors(z, 40)
    # z is the double nearest to the 2^20-th root of unity: z^(2^39) is within 2^39 * eps of 1 -- but its TENSOR is the
    # correctly rounded power of that double, which mpmath-free exact integer arithmetic reproduces here
    from fractions import Fraction
    re, im = Fraction(z.real), Fraction(z.imag)
    for k in range(6):                                  # exact rational squaring stays small for a few steps
        got = data[39 - k][0, 1, 0]
        assert abs(got.real - float(re)) <= 2e-16 and abs(got.imag - float(im)) <= 2e-16, k
        re, im = re * re - im * im, 2 * re * im
    assert np.isfinite(data[0][0, 1, 0]) and abs(abs(data[0][0, 1, 0]) - 1) < 1e-3
    big = qil.exponential_tensors(1.5, 12)
    assert big[0][0, 1, 0] == np.inf and big[-1][0, 1, 0] == 1.5 and big[-2][0, 1, 0] == 2.25
    small = qil.exponential_tensors(0.5 + 0.1j, 14)
    assert small[0][0, 1, 0] == 0 and small[-1][0, 1, 0] == 0.5 + 0.1j
