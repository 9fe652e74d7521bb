"""CPU-side checks of the operator algebra (qil_mpo_sum, qil_mpo_inner): declared with their signatures, exported and bound;
null arguments, nb < 1 and non-finite coefficients come back under the verb's name before any device is touched; the operand
checks sit ahead of the context activation; the Python front-ends reject wrong operand types before any native call; `W * 2.0`
still raises; the Julia shim binds both and INTEGRATION.md names them; the shift tensors are real, of bond 2, with 0/1 entries."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

SIGNATURES = {
    "qil_mpo_sum": r"const qil_mpo\* const\* terms,\s*int64_t nb,\s*const double\* coeffs,\s*qil_mpo\*\* out",
    "qil_mpo_inner": r"const qil_mpo\* V,\s*const qil_mpo\* W,\s*double\* out",
}
ARITY = {"qil_mpo_sum": 4, "qil_mpo_inner": 3}
FRONT_ENDS = ("mpo_linear_combination", "mpo_linear_combination_compress", "mpo_add", "mpo_sub", "mpo_scale", "mpo_inner",
              "mpo_norm", "mpo_distance", "mpo_trace", "shift_mpo_tensors", "build_shift_mpo", "fir_mpo")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _csrc(name):
    return open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", name)).read()


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


def test_sum_argument_errors_precede_the_context_activation():
    """As tests/test_sum_abi.py: QIL_EINVAL_ARG under the name "mpo_sum" on a machine without a GPU (an activation would fail
    with QIL_EHIP instead).  A zeroed buffer stands in for a handle only where no field is read (nb = 1: no pair check)."""
    L = _lib()
    out = ctypes.c_void_p()
    one_null = (ctypes.c_void_p * 1)(None)
    f = L.lib.qil_mpo_sum
    assert f(None, 1, None, ctypes.byref(out)) == QIL_EINVAL_ARG and "mpo_sum: null argument" in L.last_error()
    assert f(one_null, 1, None, None) == QIL_EINVAL_ARG and "mpo_sum: null argument" in L.last_error()
    assert f(one_null, 1, None, ctypes.byref(out)) == QIL_EINVAL_ARG and "mpo_sum: null argument" in L.last_error()
    for nb in (0, -3):
        assert f(one_null, nb, None, ctypes.byref(out)) == QIL_EINVAL_ARG
        assert "mpo_sum" in L.last_error() and "null argument" not in L.last_error()
    dummy = ctypes.create_string_buffer(4096)
    one = (ctypes.c_void_p * 1)(ctypes.addressof(dummy))
    for bad in ((np.nan, 0.0), (1.0, np.inf), (-np.inf, np.nan)):
        c = (ctypes.c_double * 2)(*bad)
        assert f(one, 1, c, ctypes.byref(out)) == QIL_EINVAL_ARG, bad
        assert "mpo_sum: coefficient 0 is not finite" in L.last_error()
    assert out.value is None


def test_inner_null_arguments_fail_without_a_device():
    L = _lib()
    v = (ctypes.c_double * 2)()
    fake = ctypes.c_void_p(0)
    dummy = ctypes.create_string_buffer(4096)
    for args in ((None, None, v), (fake, fake, None), (ctypes.addressof(dummy), None, v), (None, ctypes.addressof(dummy), v),
                 (ctypes.addressof(dummy), ctypes.addressof(dummy), None)):
        assert L.lib.qil_mpo_inner(*args) == QIL_EINVAL_ARG
        assert "mpo_inner: null argument" in L.last_error()


def _body(src, name):
    m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", src, flags=re.S)
    assert m, name
    return m.group(0)


def test_checks_precede_the_activation_in_the_source():
    """Both entries check everything before qil_ctx_activate, in qil_mps_sum's / qil_inner's order and with their codes."""
    sum_src, inner_src = _csrc("qil_sum.hip"), _csrc("qil_inner.hip")
    body = _body(sum_src, "qil_mpo_sum")
    assert 0 <= body.find('check_terms("mpo_sum", terms, nb, coeffs, out)') < body.find("qil_ctx_activate")
    # the checks themselves are the ones of qil_mps_sum (tests/test_sum_abi.py pins their order): one template over the handle type
    assert re.search(r"template <class H>\nint check_terms\(const char\* verb, const H\* const\* terms,", sum_src)
    assert sum_src.count("int check_terms(") == 1
    body = _body(inner_src, "qil_mpo_inner")
    act = body.find("qil_ctx_activate")
    assert 0 <= body.find("mpo_inner: null argument") < body.find('qil_check_pair("mpo_inner", V, W)') < act
    assert 'getenv("QIL_MPO_INNER_ROUTE")' in body                       # read per call
    pair = re.search(r"int qil_check_pair\(const char\* verb, const qil_mpo\* V, const qil_mpo\* W\) \{.*?\n}\n", inner_src, flags=re.S).group(0)
    order = [pair.find(s) for s in ("V->ctx == W->ctx, QIL_EINVAL_ARG", "V->paired == W->paired, QIL_EINVAL_ARG",
                                    "V->n() == W->n(), QIL_EINVAL_LENGTH", "V->site_ids == W->site_ids, QIL_EINVAL_SITES")]
    assert all(o >= 0 for o in order) and order == sorted(order), order
    assert "qil_ctx_activate" not in pair


def test_the_operator_sum_has_no_store_kernel_of_its_own():
    """qil_mpo_sum goes through site_sum_grouped: one kernel, one launch site, the slice count of the last / only site from the
    site table."""
    code = re.sub(r"//[^\n]*", "", _csrc("qil_sum.hip"))
    assert code.count("__global__") == 2                                  # site_sum_grouped and gemm_grouped_small
    assert code.count("site_sum_grouped<TA, TO, MIXED>") == 1
    assert "S.nphys" in code and "hipMemset" not in code and "qil_dev_zero" not in code
    assert re.search(r"constexpr long long kMpoChainAutoMax = \d+;", _csrc("qil_inner.hip"))


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
    for name in list(SIGNATURES) + ["qil_mpo_compress", "qil_mpo_nsites", "qil_mpo_is_paired", "qil_mpo_dtype", "qil_mpo_create",
                                    "qil_mpo_site_ids", "qil_mps_nsites"]:
        monkeypatch.setattr(L.lib, name, boom)
    W, Wp = _fake(qil.SingleSiteMPO), _fake(qil.PairedSiteMPO)
    psi = _fake(qil.SignalMPS)
    msg = "mpo_linear_combination: unsupported operand types"
    for bad in (None, W, np.zeros((1, 2, 2, 1)), [], [W, None], [W, psi], [np.zeros((1, 2, 2, 1))], [W, Wp], [Wp, W]):
        for fn in (qil.mpo_linear_combination, qil.mpo_linear_combination_compress):
            with pytest.raises(TypeError, match=msg):
                fn(bad)
    for x in (None, psi, np.zeros(3), 2.0):
        for fn in (qil.mpo_add, qil.mpo_sub):
            with pytest.raises(TypeError, match=msg):
                fn(W, x)
            with pytest.raises(TypeError, match=msg):
                fn(x, W)
        with pytest.raises(TypeError, match=msg):
            qil.mpo_scale(x, 2.0)
        for fn in (qil.mpo_inner, qil.mpo_distance):
            with pytest.raises(TypeError, match="mpo_inner: unsupported operand types"):
                fn(W, x)
            with pytest.raises(TypeError, match="mpo_inner: unsupported operand types"):
                fn(x, W)
        with pytest.raises(TypeError, match="mpo_inner: unsupported operand types"):
            qil.mpo_norm(x)
        with pytest.raises(TypeError, match="mpo_trace: unsupported operand types"):
            qil.mpo_trace(x)
        if not isinstance(x, np.ndarray):               # numpy's reflected operators would probe the operator as a sequence
            with pytest.raises(TypeError):
                W + x
            with pytest.raises(TypeError):
                W - x
    # the two classes do not mix
    for fn in (qil.mpo_add, qil.mpo_sub):
        with pytest.raises(TypeError, match=msg):
            fn(W, Wp)
    assert qil.SingleSiteMPO.__add__(W, Wp) is NotImplemented and qil.SingleSiteMPO.__sub__(Wp, W) is NotImplemented
    with pytest.raises(TypeError):
        W + Wp
    with pytest.raises(TypeError):
        Wp - W
    for c in ("2", None, [1.0], True):
        with pytest.raises(TypeError, match=msg):
            qil.mpo_scale(W, c)
    assert qil.SingleSiteMPO.__rmul__(W, "2") is NotImplemented and qil.SingleSiteMPO.__rmul__(W, psi) is NotImplemented
    with pytest.raises(TypeError, match=msg):
        qil.mpo_linear_combination([W, W], ["a", "b"])
    with pytest.raises(ValueError, match="3 coefficients for 2 terms"):
        qil.mpo_linear_combination([W, W], [1, 2, 3])
    with pytest.raises(ValueError, match="1 coefficients for 2 terms"):
        qil.mpo_linear_combination_compress([W, W], [1j])
    assert boom.calls == 0


def test_multiplication_from_the_right_keeps_its_meaning():
    """`W * x` is the application (W * psi, W1 * W2): a number on the right still raises the TypeError of `apply`; only
    `c * W` scales."""
    import qilaplace_jl_amd as qil
    W = _fake(qil.SingleSiteMPO)
    for c in (2.0, 2, 1j):
        with pytest.raises(TypeError, match="apply: unsupported operand types"):
            W * c
    for name in ("__add__", "__sub__", "__neg__", "__rmul__", "__mul__"):
        assert name in qil.SingleSiteMPO.__dict__, name
    assert "__rmul__" not in qil.SignalMPS.__dict__


def test_julia_shim_and_documents_name_both():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function mpo_linear_combination\(terms::Vector\{<:DeviceMPO\}, coeffs=nothing\)", src)
    assert re.search(r"Base\.:\+\(V::DeviceMPO, W::DeviceMPO\)", src)
    assert re.search(r"Base\.:-\(V::DeviceMPO, W::DeviceMPO\)", src)
    assert re.search(r"function mpo_inner\(V::DeviceMPO, W::DeviceMPO\)", src)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SIGNATURES:
        assert f"(:{name}, LIB)" in src, name
        assert f"`{name}`" in doc, name
    for name in ("mpo_linear_combination", "mpo_inner"):
        assert re.search(r"export .*\b" + name + r"\b", src, flags=re.S), name
    assert "mpo_linear_combination" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "qil_mpo_sum" in design and "qil_mpo_inner" in design
    assert os.path.exists(os.path.join(ROOT, "examples", "fir_filter.py"))
    import qilaplace_jl_amd as qil
    assert "1e-7" in qil.mpo_distance.__doc__ and "plain composition" in " ".join(qil.mpo_linear_combination_compress.__doc__.split())


@pytest.mark.parametrize("n,s", [(1, 1), (2, 3), (6, 37), (9, -3), (40, 2 ** 39), (40, 5)])
def test_shift_tensors_are_real_of_bond_2_with_unit_entries(n, s):
    import qilaplace_jl_amd as qil
    data = qil.shift_mpo_tensors(n, s)
    assert len(data) == n
    dims = [1] + [2] * (n - 1) + [1]
    for i, t in enumerate(data):
        assert t.dtype == np.float64 and t.shape == (dims[i], 2, 2, dims[i + 1]), i
        assert set(np.unique(t)) <= {0.0, 1.0}
        # one output bit per (input bit, carry in); the first site drops its carry out
        assert np.array_equal(t.sum(axis=(0, 2)), np.ones((2, dims[i + 1]))), i
    with pytest.raises(ValueError):
        qil.shift_mpo_tensors(0, 1)
