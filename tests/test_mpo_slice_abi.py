"""CPU-side checks of the operator read-outs (qil_mpo_entry_batch, qil_mpo_slice): declared with their signatures, exported and
bound; null arguments and nb < 0 come back before any device is touched, and those checks sit ahead of the context activation in
the source; the file has kernels of its own and shares the MFMA tile step; the Python front-ends are exported and reject a bad
spec, index or operand before a native entry is called; the Julia shim binds the entries and the documents name them."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

ENTRIES = {
    "qil_mpo_entry_batch": (r"const qil_mpo\* W,\s*int64_t nb,\s*const uint8_t\* spec,\s*double\* out", 4),
    "qil_mpo_slice": (r"const qil_mpo\* W,\s*const uint8_t\* spec,\s*qil_mps\*\* out", 3),
}
FRONT_ENDS = ("mpo_entry_batch", "mpo_slice", "mpo_entries", "mpo_entry", "mpo_to_matrix", "mpo_column", "mpo_row",
              "mpo_diagonal_state", "mpo_column_sums", "mpo_row_sums")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _source():
    return open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_mpo_slice.hip")).read()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_entries_are_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", _read("include", "qilaplace_hip.h"), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    for name, (signature, nargs) in ENTRIES.items():
        assert re.search(r"QIL_API\s+int\s+" + name + r"\s*\(\s*" + signature + r"\s*\)\s*;", decl), name
        assert hasattr(so, name)
        assert len(L.PROTOTYPES[name]) == nargs
    assert re.search(r"#define QIL_MPO_ENTRY_CHAIN_MAX_BOND 1024\b", decl)
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    assert (qil.ops.FIX0, qil.ops.FIX1, qil.ops.SUM, qil.ops.FREE, qil.ops.TIE, qil.ops.DIAG) == (0, 1, 2, 3, 4, 5)
    assert qil.ops.TRACE == 2                                           # the Born weights keep their word
    assert "qil_mpo_slice.hip" in _read("qilaplace.jl_amd", "csrc", "Makefile")


def test_null_arguments_and_a_negative_count_precede_the_context_activation():
    """QIL_EINVAL_ARG with the documented messages.  This runs on a machine without a GPU: an activation would fail with QIL_EHIP
    instead.  The non-null stand-ins are never dereferenced: a null (or the count) comes first in every call."""
    L = _lib()
    out = ctypes.c_void_p()
    dummy = ctypes.create_string_buffer(4096)
    spec = (ctypes.c_uint8 * 8)(*([3, 0] * 4))
    vals = (ctypes.c_double * 8)()
    handle = ctypes.c_void_p(ctypes.addressof(dummy))
    for args in ((None, spec, ctypes.byref(out)), (handle, None, ctypes.byref(out)), (handle, spec, None), (None, None, None)):
        assert L.lib.qil_mpo_slice(*args) == QIL_EINVAL_ARG
        assert "mpo_slice: null argument" in L.last_error()
    assert out.value is None
    for args in ((None, 1, spec, vals), (handle, 1, None, vals), (handle, 1, spec, None), (None, 0, None, None),
                 (None, -1, spec, vals)):
        assert L.lib.qil_mpo_entry_batch(*args) == QIL_EINVAL_ARG
        assert "mpo_entry_batch: null argument" in L.last_error()
    for nb in (-1, -(2 ** 40)):
        assert L.lib.qil_mpo_entry_batch(handle, nb, spec, vals) == QIL_EINVAL_ARG
        assert "nb must be non-negative" in L.last_error()
        assert L.lib.qil_mpo_entry_batch(handle, nb, None, None) == QIL_EINVAL_ARG
    assert L.lib.qil_mpo_entry_batch(handle, 0, None, None) == 0        # nb = 0 is a no-op
    assert all(v == 0.0 for v in vals)


def test_the_null_checks_sit_first_in_the_bodies():
    src = _source()
    firsts = {
        "qil_mpo_entry_batch": 'QIL_REQUIRE(W && (nb <= 0 || (spec && out)), QIL_EINVAL_ARG, "mpo_entry_batch: null argument");',
        "qil_mpo_slice": 'QIL_REQUIRE(W && spec && out, QIL_EINVAL_ARG, "mpo_slice: null argument");',
    }
    for name, first in firsts.items():
        m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", src, flags=re.S)
        assert m, name
        body = m.group(0)
        assert body[body.index("{") + 1:].lstrip().startswith(first), name
        act = body.find("qil_ctx_activate")
        assert 0 <= body.find("QIL_EINVAL_ARG") < act
        # every refusal of a spec comes before the activation too
        assert body.rfind("QIL_EINVAL_CONFIG") < act
        assert "qil_call_scope" in body[act:] and body.count("qil_ctx_activate") == 1
    body = re.search(r'extern "C" int qil_mpo_slice\(.*?\n}\n', src, flags=re.S).group(0)
    assert "keeps both legs: sub-operators are not built" in body
    assert "that number is what mpo_entry_batch returns" in body
    assert "qil_result_guard<qil_mps>" in body


def test_the_read_outs_have_kernels_of_their_own():
    code = re.sub(r"//[^\n]*", "", _source())
    for kernel in ("mpo_entry_chain", "mpo_slice_grouped", "mpo_slice_runs_lds"):
        assert re.search(r"__global__ __launch_bounds__\(kThreads\) void " + kernel + r"\(", code), kernel
    assert re.search(r"__global__ void mpo_entry_combine\(", code)
    assert "mfma_step(" in code and "void mfma_step(" not in code         # the f64 MFMA tile step: one definition, in the shared header
    utils = _read("qilaplace.jl_amd", "csrc", "qil_device_utils.h")
    assert utils.count("void mfma_step(") == 1 and utils.count("__builtin_amdgcn_mfma_f64_16x16x4f64(") == 4
    assert code.count("hipLaunchKernelGGL(mpo_slice_grouped<") == 2       # one launch site per dtype: all kept tensors in one grid
    assert code.count("hipLaunchKernelGGL(mpo_entry_chain<") == 2
    for shared in ("qil_dev_table", "last_entry_le<", "qil_call_scope", "qil_lds_grant", "qil_dev_gemm("):
        assert shared in code, shared
    assert "asm" not in code
    # the restriction's own file is as it was: no kernel moved out of it
    restrict = _read("qilaplace.jl_amd", "csrc", "qil_restrict.hip")
    assert restrict.count("hipLaunchKernelGGL(restrict_absorb_grouped<") == 2 and "restrict_runs_lds" in restrict


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


def test_python_checks_precede_the_native_entries(monkeypatch):
    """The chain length is the one thing the checks need from the handle; it is served here by a stand-in, and every other
    native entry the front-ends could reach raises."""
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()
    ntensors = [6]

    def nsites(handle, ref):
        ref._obj.value = ntensors[0]
        return 0

    monkeypatch.setattr(L.lib, "qil_mpo_nsites", nsites)
    for name in ("qil_mpo_entry_batch", "qil_mpo_slice", "qil_mps_is_paired", "qil_mpo_dtype", "qil_apply", "qil_mpo_inner"):
        monkeypatch.setattr(L.lib, name, boom)
    single, paired = _fake(qil.SingleSiteMPO), _fake(qil.PairedSiteMPO)          # 6 tensors each: 6 and 3 sites
    col = np.stack([np.zeros(6), np.full(6, 3)], axis=1).astype(np.uint8)
    for W in (single, paired):
        for bad in (col[:5], np.zeros((7, 2)), col.T, col.reshape(-1), np.zeros((6, 3), dtype=np.uint8), []):
            with pytest.raises(ValueError, match="expected 6 x 2 entries"):
                qil.mpo_slice(W, bad)
        for bad in (col[None, :5], col, np.zeros((2, 6, 3), dtype=np.uint8), np.zeros((2, 12), dtype=np.uint8)):
            with pytest.raises(ValueError, match="expected 6 x 2 entries"):
                qil.mpo_entry_batch(W, bad)
        for v in (6, 200, -1):
            s = col.astype(np.int64)
            s[2, 1] = v
            with pytest.raises(ValueError, match=r"outside \[0,5\]"):
                qil.mpo_slice(W, s)
            s3 = np.zeros((2, 6, 2), dtype=np.int64)
            s3[1, 2, 1] = v
            with pytest.raises(ValueError, match=r"outside \[0,5\]"):
                qil.mpo_entry_batch(W, s3)
        for half in ((4, 0), (0, 4), (5, 3), (2, 5), (4, 5), (5, 4)):
            s = col.copy()
            s[3] = half
            with pytest.raises(ValueError, match="both bytes of a site"):
                qil.mpo_slice(W, s)
        for half in ((4, 0), (1, 4), (4, 2)):
            s = np.zeros((3, 6, 2), dtype=np.uint8)
            s[1, 4] = half
            with pytest.raises(ValueError, match="both bytes of a site"):
                qil.mpo_entry_batch(W, s)
        s = col.copy()
        s[1] = (3, 3)
        with pytest.raises(ValueError, match="keeps both legs: sub-operators are not built"):
            qil.mpo_slice(W, s)
        for none_kept in (np.zeros((6, 2)), np.full((6, 2), 4), np.full((6, 2), 2)):
            with pytest.raises(ValueError, match="that number is what mpo_entry_batch returns"):
                qil.mpo_slice(W, none_kept.astype(np.uint8))
        for kept in ((3, 0), (1, 3), (5, 5)):
            s = np.zeros((2, 6, 2), dtype=np.uint8)
            s[1, 5] = kept
            with pytest.raises(ValueError, match="makes no number"):
                qil.mpo_entry_batch(W, s)
        with pytest.raises(TypeError, match="must hold integers"):
            qil.mpo_slice(W, col.astype(np.float64))
        # indices and configurations
        for fn in (qil.mpo_column, qil.mpo_row):
            for bad in (-1, 64, 1 << 40, "1012", "10101", [0, 1, 0], [0, 1, 2, 0, 1, 0]):
                with pytest.raises(ValueError):
                    fn(W, bad)
        for bad in ((64, 0), (0, 64), (-1, 0), (0, "0000000"), ([1] * 5, 0)):
            with pytest.raises(ValueError):
                qil.mpo_entry(W, *bad)
        for bad in ((np.array([0, 64]), np.array([0])), (np.array([0]), np.array([-1])), ([0, 1], [64]),
                    (np.zeros((2, 5), dtype=np.int64), [0]), (np.full((2, 6), 2), [0])):
            with pytest.raises(ValueError):
                qil.mpo_entries(W, *bad)
    for fn in FRONT_ENDS:
        args = {"mpo_entry_batch": (col[None],), "mpo_slice": (col,), "mpo_entries": ([0], [0]), "mpo_entry": (0, 0),
                "mpo_column": (0,), "mpo_row": (0,)}.get(fn, ())
        for bad in (None, np.zeros((1, 2, 2, 1)), _fake(qil.SignalMPS), _fake(qil.ZTMPS)):
            with pytest.raises(TypeError, match=fn + ": unsupported operand types"):
                getattr(qil, fn)(bad, *args)
    ntensors[0] = 13
    with pytest.raises(ValueError, match="stops at 12 tensors"):
        qil.mpo_to_matrix(single)
    ntensors[0] = 14
    with pytest.raises(ValueError, match="stops at 12 tensors"):
        qil.mpo_to_matrix(paired)
    assert boom.calls == 0


def test_julia_shim_and_documents_name_the_entries():
    src = _read("julia", "QILaplaceHIP.jl")
    assert re.search(r"function mpo_entry_batch\(W::DeviceMPO, specs::AbstractArray\{<:Integer,3\}\)", src)
    assert re.search(r"function mpo_slice\(W::DeviceMPO, spec::AbstractMatrix\{<:Integer\}\)", src)
    integration, readme = _read("INTEGRATION.md"), _read("README.md")
    for name in ENTRIES:
        assert f"(:{name}, LIB)" in src
        assert re.search(r"export .*\b" + name[4:] + r"\b", src, flags=re.S)
        assert f"`{name}`" in integration
    for name in ("mpo_entry_batch", "mpo_slice", "mpo_column", "mpo_row", "mpo_diagonal_state", "mpo_to_matrix"):
        assert f"`{name}`" in readme, name
    example = _read("examples", "operator_rows.py")
    for name in ("mpo_column", "mpo_row", "top_k", "fir_mpo"):
        assert name in example, name
    assert "QIL_MPO_ENTRY_ROUTE" in _read("tools", "README.md")
    header = _read("include", "qilaplace_hip.h")
    for phrase in ("sub-operators", "lazy form", "device-resident out"):      # what is deliberately left out is said
        assert phrase in header[header.index("operator read-outs"):], phrase
    flat = re.sub(r"\s*\n \* +", " ", header[header.index("operator read-outs"):])     # comment lines joined
    assert "chunks under 64 MiB" in flat and "rounding differs from the chain's" in flat
