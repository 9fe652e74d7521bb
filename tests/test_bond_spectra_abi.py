"""CPU-side checks of the Schmidt spectra (qil_bond_spectra, qil_mpo_bond_spectra): declared with their signatures, exported,
prototyped and bound; null arguments come back with the documented message before any device is touched; the front-ends reject
wrong operands before any native entry is called; the numpy helpers on top (entanglement_entropy, truncation_error_bounds,
required_maxdim) reproduce hand-computed numbers."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")
QIL_EINVAL_ARG = 7

ENTRIES = {
    "qil_bond_spectra": r"const qil_mps\* psi,\s*double\* S_out,\s*double\* norm_out",
    "qil_mpo_bond_spectra": r"const qil_mpo\* W,\s*double\* S_out,\s*double\* norm_out",
}


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def test_entries_are_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    for name, signature in ENTRIES.items():
        assert re.search(r"QIL_API\s+int\s+" + name + r"\s*\(\s*" + signature + r"\s*\)\s*;", decl), name
        assert decl.index("QIL_API int qil_apply_norm") < decl.index("QIL_API int " + name)
        assert hasattr(so, name)
        assert len(L.PROTOTYPES[name]) == 3
    testing = open(os.path.join(ROOT, "include", "qilaplace_hip_testing.h")).read()
    assert "bond_spectra" not in testing
    for py in ("bond_spectra", "mpo_bond_spectra", "entanglement_entropy", "truncation_error_bounds", "required_maxdim"):
        assert py in qil.__all__ and callable(getattr(qil, py)), py
    assert "qil_spectra.hip" in open(os.path.join(CSRC, "Makefile")).read()
    shim = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert "(:qil_bond_spectra, LIB)" in shim and "(:qil_mpo_bond_spectra, LIB)" in shim
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`qil_bond_spectra`" in table and "`qil_mpo_bond_spectra`" in table


def test_null_arguments_precede_the_context_activation():
    """QIL_EINVAL_ARG with the documented message.  This runs on a machine without a GPU: an activation would fail with
    QIL_EHIP instead.  A null handle is refused before its length is read."""
    L = _lib()
    vals = (ctypes.c_double * 4)(*([-7.0] * 4))
    nrm = ctypes.c_double(-3.0)
    for entry in (L.lib.qil_bond_spectra, L.lib.qil_mpo_bond_spectra):
        for args in ((None, vals, ctypes.byref(nrm)), (None, None, None), (None, vals, None)):
            assert entry(*args) == QIL_EINVAL_ARG
            assert "bond_spectra: null argument" in L.last_error()
    assert list(vals) == [-7.0] * 4 and nrm.value == -3.0


def test_every_check_precedes_the_activation_in_the_source():
    src = open(os.path.join(CSRC, "qil_spectra.hip")).read()
    for name in ENTRIES:
        m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", src, flags=re.S)
        assert m, name
        body = m.group(0)
        assert body[body.index("{") + 1:].lstrip().startswith("QIL_REQUIRE(")
        assert '"bond_spectra: null argument"' in body and "qil_ctx_activate" not in body
        assert body.index("QIL_REQUIRE") < body.index("bond_spectra_impl(")
    assert 'QIL_EDOMAIN, "bond_spectra: zero or non-finite state"' in src
    assert src.index("qil_ctx_activate") < src.index("qil_call_scope call_scope") < src.index("qil_chain_alloc")


def test_front_ends_reject_wrong_operands_before_any_native_call(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()

    class _Refuse:
        def __getattr__(self, name):
            raise AssertionError(f"native entry {name} was reached")

    monkeypatch.setattr(L, "lib", _Refuse())
    for bad in (None, 3, "psi", np.ones(4), [np.ones(2)]):
        with pytest.raises(TypeError, match="bond_spectra: unsupported operand types"):
            qil.bond_spectra(bad)
        with pytest.raises(TypeError, match="mpo_bond_spectra: unsupported operand types"):
            qil.mpo_bond_spectra(bad)
    for fn, args in ((qil.entanglement_entropy, ()), (qil.truncation_error_bounds, (2,)), (qil.required_maxdim, (0.1,))):
        with pytest.raises(TypeError, match="expected an MPS, an MPO or a list of spectra"):
            fn(3.5, *args)
    with pytest.raises(ValueError):
        qil.truncation_error_bounds([[1.0]], 0)
    with pytest.raises(ValueError):
        qil.required_maxdim([[1.0]], -1.0)
    with pytest.raises(ValueError):
        qil.entanglement_entropy([[1.0]], alpha=0.0)


@pytest.mark.parametrize("alpha", [0.5, 1.0, 2.0])
def test_entropy_of_equal_values_is_the_logarithm_of_their_count(alpha):
    import qilaplace_jl_amd as qil
    counts = [1, 2, 3, 8, 17]
    spectra = [np.full(k, 1.0 / np.sqrt(k)) for k in counts]
    got = qil.entanglement_entropy(spectra, alpha=alpha)
    assert got.shape == (len(counts),)
    assert np.allclose(got, np.log2(counts), rtol=0, atol=1e-13)
    # another base, and a spectrum that is not normalised: the probabilities are s^2 / sum s^2
    nats = qil.entanglement_entropy([3.0 * s for s in spectra], alpha=alpha, base=np.e)
    assert np.allclose(nats, np.log(counts), rtol=0, atol=1e-13)


def test_entropy_of_a_product_state_is_zero_and_zeros_contribute_nothing():
    import qilaplace_jl_amd as qil
    product = [np.array([1.0]), np.array([1.0, 0.0, 0.0]), np.array([1.0, 0.0])]
    for alpha in (0.5, 1.0, 2.0):
        got = qil.entanglement_entropy(product, alpha=alpha)
        assert np.all(np.isfinite(got)) and np.all(got == 0.0), (alpha, got)
        padded = qil.entanglement_entropy([np.array([np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0])], alpha=alpha)
        assert np.isfinite(padded[0]) and abs(padded[0] - 1.0) <= 1e-14
    # a hand-computed unequal spectrum: p = (3/4, 1/4)
    s = [np.array([np.sqrt(0.75), 0.5])]
    assert abs(qil.entanglement_entropy(s)[0] - (2.0 - 0.75 * np.log2(3.0))) <= 1e-14
    assert abs(qil.entanglement_entropy(s, alpha=2.0)[0] - (-np.log2(0.625))) <= 1e-14
    assert qil.entanglement_entropy([]).shape == (0,)


THREE_BONDS = [np.array([0.8, 0.6]), np.array([np.sqrt(0.5), 0.5, 0.5, 0.0]), np.array([0.9, np.sqrt(0.19)])]


def test_truncation_bounds_and_required_maxdim_on_a_three_bond_example():
    """Tails t_k beyond maxdim 1: (0.36, 0.5, 0.19); beyond 2: (0, 0.25, 0); beyond 3: all 0."""
    import qilaplace_jl_amd as qil
    lo, up = qil.truncation_error_bounds(THREE_BONDS, 1)
    assert abs(lo - np.sqrt(0.5)) <= 1e-15 and abs(up - np.sqrt(1.05)) <= 1e-15
    lo, up = qil.truncation_error_bounds(THREE_BONDS, 2)
    assert abs(lo - 0.5) <= 1e-15 and abs(up - 0.5) <= 1e-15
    for maxdim in (3, 4, 100):
        assert qil.truncation_error_bounds(THREE_BONDS, maxdim) == (0.0, 0.0)
    assert qil.truncation_error_bounds([], 1) == (0.0, 0.0)
    assert qil.required_maxdim(THREE_BONDS, 2.0) == 1
    assert qil.required_maxdim(THREE_BONDS, 1.03) == 1          # sqrt(1.05) = 1.0247
    assert qil.required_maxdim(THREE_BONDS, 1.02) == 2
    assert qil.required_maxdim(THREE_BONDS, 0.6) == 2
    assert qil.required_maxdim(THREE_BONDS, 0.49) == 3
    assert qil.required_maxdim(THREE_BONDS, 0.0) == 3           # the exact zero of bond 2 is never needed
    # the order inside a block does not matter, nor does its scale
    shuffled = [2.0 * s[::-1] for s in THREE_BONDS]
    assert qil.truncation_error_bounds(shuffled, 1) == pytest.approx((np.sqrt(0.5), np.sqrt(1.05)), abs=1e-15)


def test_required_maxdim_is_monotone_in_tol():
    import qilaplace_jl_amd as qil
    rng = np.random.default_rng(5)
    spectra = []
    for width in (2, 4, 8, 16, 16, 8, 4, 2):
        s = np.sort(rng.random(width) * 0.5 ** np.arange(width))[::-1]
        spectra.append(s / np.linalg.norm(s))
    tols = np.logspace(-8, 0.5, 40)
    need = [qil.required_maxdim(spectra, t) for t in tols]
    assert all(a >= b for a, b in zip(need, need[1:])), need
    assert need[0] > need[-1] and need[-1] == 1
    for t, m in zip(tols, need):
        assert qil.truncation_error_bounds(spectra, m)[1] <= t
        assert m == 1 or qil.truncation_error_bounds(spectra, m - 1)[1] > t
