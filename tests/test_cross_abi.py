"""CPU-side checks of the cross-interpolation encoder (qil_cross_*, qil_signal_mps_cross) and of qil_ztmps_from_mps: declared
with their signatures, exported, prototyped and bound; the header has no function-pointer parameter (a host evaluator is a
pull-style session, not a callback); every argument error comes back as QIL_EINVAL_ARG with its message before any device is
touched.  The errors that need a live session (indices / supply with nothing pending, finish with samples pending) are in
tests/test_gpu_cross.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")
QIL_EINVAL_LENGTH, QIL_EINVAL_ARG = 1, 7

ENTRIES = {
    "qil_cross_begin": (r"qil_context\* ctx,\s*int64_t n,\s*int dtype,\s*int64_t maxdim,\s*double tol,\s*int max_sweeps,\s*"
                        r"const int64_t\* seeds,\s*int64_t nseeds,\s*qil_cross\*\* out", 9),
    "qil_cross_pending": (r"qil_cross\* s,\s*int64_t\* count", 2),
    "qil_cross_indices": (r"qil_cross\* s,\s*int64_t\* idx_dev", 2),
    "qil_cross_supply": (r"qil_cross\* s,\s*const void\* values_dev", 2),
    "qil_cross_finish": (r"qil_cross\* s,\s*qil_mps\*\* out,\s*double\* est,\s*int64_t\* nevals,\s*int\* sweeps,\s*int\* converged", 6),
    "qil_cross_destroy": (r"qil_cross\* s", 1),
    "qil_signal_mps_cross": (r"qil_context\* ctx,\s*const void\* x,\s*int64_t len,\s*int dtype,\s*int64_t maxdim,\s*double tol,\s*"
                             r"int max_sweeps,\s*const int64_t\* seeds,\s*int64_t nseeds,\s*qil_mps\*\* out,\s*double\* est,\s*"
                             r"int64_t\* nevals,\s*int\* sweeps,\s*int\* converged", 14),
    "qil_ztmps_from_mps": (r"const qil_mps\* psi,\s*double cutoff,\s*int64_t maxdim,\s*qil_mps\*\* out", 4),
}


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)


def test_entries_are_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = _header()
    so = ctypes.CDLL(qil.LIB_PATH)
    assert re.search(r"typedef\s+struct\s+qil_cross\s+qil_cross\s*;", decl)
    for name, (signature, arity) in ENTRIES.items():
        assert re.search(r"QIL_API\s+int\s+" + name + r"\s*\(\s*" + signature + r"\s*\)\s*;", decl), name
        assert hasattr(so, name)
        assert len(L.PROTOTYPES[name]) == arity
    testing = open(os.path.join(ROOT, "include", "qilaplace_hip_testing.h")).read()
    assert "cross" not in testing and "ztmps_from_mps" not in testing
    for py in ("signal_mps_cross", "ztmps_from_mps"):
        assert py in qil.__all__ and callable(getattr(qil, py)), py
    assert "qil_cross.hip" in open(os.path.join(CSRC, "Makefile")).read()
    shim = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert f"(:{name}, LIB)" in shim, name
        assert f"`{name}`" in table, name


def test_header_has_no_function_pointer_parameter():
    """tests/test_julia_shim_signatures.py parses every prototype with a table of scalars: a callback would not fit it."""
    for header in ("qilaplace_hip.h", "qilaplace_hip_testing.h"):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        assert not re.search(r"\(\s*\*\s*\w*\s*\)\s*\(", src), header          # (*name)( ... )
        for args in re.findall(r"\bqil_[a-z0-9_]+\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            assert "(" not in args, args


def _ctx_stub():
    """A non-null context that must never be read: every check below fails before the context is activated."""
    return ctypes.create_string_buffer(64)


def test_null_arguments_precede_the_context_activation():
    L = _lib()
    lib = L.lib
    out, cnt = ctypes.c_void_p(), ctypes.c_int64(-5)
    seeds = (ctypes.c_int64 * 2)(0, 1)
    stub = _ctx_stub()
    assert lib.qil_cross_begin(None, 4, 0, 8, 1e-9, 4, seeds, 2, ctypes.byref(out)) == QIL_EINVAL_ARG
    assert "cross_begin: null argument" in L.last_error()
    assert lib.qil_cross_begin(stub, 4, 0, 8, 1e-9, 4, seeds, 2, None) == QIL_EINVAL_ARG
    assert lib.qil_cross_pending(None, ctypes.byref(cnt)) == QIL_EINVAL_ARG and "cross_pending: null argument" in L.last_error()
    assert lib.qil_cross_indices(None, None) == QIL_EINVAL_ARG and "cross_indices: null argument" in L.last_error()
    assert lib.qil_cross_supply(None, None) == QIL_EINVAL_ARG and "cross_supply: null argument" in L.last_error()
    assert lib.qil_cross_finish(None, ctypes.byref(out), None, None, None, None) == QIL_EINVAL_ARG
    assert "cross_finish: null argument" in L.last_error()
    assert lib.qil_cross_destroy(None) == 0
    x = np.ones(16)
    assert lib.qil_signal_mps_cross(None, x.ctypes.data_as(ctypes.c_void_p), 16, 0, 8, 1e-9, 4, seeds, 2, ctypes.byref(out),
                                    None, None, None, None) == QIL_EINVAL_ARG
    assert "signal_mps_cross: null argument" in L.last_error()
    assert lib.qil_signal_mps_cross(stub, None, 16, 0, 8, 1e-9, 4, seeds, 2, ctypes.byref(out), None, None, None, None) == QIL_EINVAL_ARG
    assert lib.qil_ztmps_from_mps(None, 1e-10, 0, ctypes.byref(out)) == QIL_EINVAL_ARG
    assert "ztmps_from_mps: null argument" in L.last_error()
    assert out.value is None and cnt.value == -5


BAD_BEGIN = [
    # (n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, message)
    (0, 0, 8, 1e-9, 4, [0], 1, "outside 1 .. 62"),
    (63, 0, 8, 1e-9, 4, [0], 1, "outside 1 .. 62"),
    (-3, 0, 8, 1e-9, 4, [0], 1, "outside 1 .. 62"),
    (10, 0, 0, 1e-9, 4, [0], 1, "maxdim must be finite, 1 .. 256"),
    (10, 0, 257, 1e-9, 4, [0], 1, "maxdim must be finite, 1 .. 256"),
    (10, 0, 2 ** 63 - 1, 1e-9, 4, [0], 1, "maxdim must be finite, 1 .. 256"),          # QIL_MAXDIM_NONE
    (10, 0, -1, 1e-9, 4, [0], 1, "maxdim must be finite, 1 .. 256"),
    (10, 0, 8, -1e-9, 4, [0], 1, "tol must be >= 0"),
    (10, 0, 8, float("nan"), 4, [0], 1, "tol must be >= 0"),
    (10, 0, 8, 1e-9, 0, [0], 1, "max_sweeps must be >= 1"),
    (10, 0, 8, 1e-9, 4, [0], 0, "seeds"),
    (10, 0, 8, 1e-9, 4, [0], -2, "seeds"),
    (10, 0, 8, 1e-9, 4, None, 1, "seeds"),
    (10, 0, 8, 1e-9, 4, [0, 1024], 2, "seed 1024 outside"),
    (10, 0, 8, 1e-9, 4, [5, -1], 2, "seed -1 outside"),
    (62, 1, 8, 1e-9, 4, [2 ** 62], 1, "outside"),
    (10, 7, 8, 1e-9, 4, [0], 1, "unknown dtype 7"),
]


@pytest.mark.parametrize("n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, message", BAD_BEGIN)
def test_begin_refuses_bad_arguments_before_the_context_is_touched(n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, message):
    L = _lib()
    out = ctypes.c_void_p()
    arr = (ctypes.c_int64 * len(seeds))(*seeds) if seeds is not None else None
    st = L.lib.qil_cross_begin(_ctx_stub(), n, dtype, maxdim, tol, max_sweeps, arr, nseeds, ctypes.byref(out))
    assert st == QIL_EINVAL_ARG and message in L.last_error(), L.last_error()
    assert out.value is None


def test_one_shot_refuses_bad_arguments_before_the_context_is_touched():
    L = _lib()
    out = ctypes.c_void_p()
    x = np.ones(16)
    xp = x.ctypes.data_as(ctypes.c_void_p)
    seeds = (ctypes.c_int64 * 2)(0, 15)
    tail = (ctypes.byref(out), None, None, None, None)
    call = L.lib.qil_signal_mps_cross
    assert call(_ctx_stub(), xp, 0, 0, 8, 1e-9, 4, seeds, 2, *tail) == QIL_EINVAL_LENGTH
    assert call(_ctx_stub(), xp, 20, 0, 8, 1e-9, 4, seeds, 2, *tail) == QIL_EINVAL_LENGTH          # round(log2 20) = 4 and 20 > 16
    assert "power of 2" in L.last_error()
    assert call(_ctx_stub(), xp, 16, 0, 2 ** 63 - 1, 1e-9, 4, seeds, 2, *tail) == QIL_EINVAL_ARG and "maxdim" in L.last_error()
    assert call(_ctx_stub(), xp, 16, 0, 8, -1.0, 4, seeds, 2, *tail) == QIL_EINVAL_ARG and "tol" in L.last_error()
    assert call(_ctx_stub(), xp, 16, 0, 8, 1e-9, 4, seeds, 0, *tail) == QIL_EINVAL_ARG and "seeds" in L.last_error()
    far = (ctypes.c_int64 * 1)(16)
    assert call(_ctx_stub(), xp, 16, 0, 8, 1e-9, 4, far, 1, *tail) == QIL_EINVAL_ARG and "seed 16 outside" in L.last_error()
    assert out.value is None


def test_every_check_precedes_the_activation_in_the_source():
    src = open(os.path.join(CSRC, "qil_cross.hip")).read()
    for name in ("qil_cross_begin", "qil_cross_indices", "qil_cross_supply", "qil_cross_finish", "qil_signal_mps_cross"):
        m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", src, flags=re.S)
        assert m, name
        body = m.group(0)
        act = body.index("qil_ctx_activate")
        first = min(body.index(w) for w in ("QIL_REQUIRE", "cross_check_args(") if w in body)
        assert first < act < body.index("qil_call_scope call_scope"), name
        assert "QIL_REQUIRE" not in body[act:] and "cross_check_args(" not in body[act:], name
    assert 'QIL_EDOMAIN, "signal_mps_cross: every sampled value is 0"' in src
    assert '"cross_indices: nothing is pending"' in src and '"cross_supply: nothing is pending"' in src
    assert "samples are still pending" in src
    # the lifted loop: one static function behind both entries of qil_truncate.hip
    tr = open(os.path.join(CSRC, "qil_truncate.hip")).read()
    assert tr.count("ztmps_from_sites(ctx,") == 2 and tr.count("fuse_delta_k<c64>") == 1


def test_front_ends_reject_wrong_operands_before_any_native_call(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()

    class _Refuse:
        def __getattr__(self, name):
            raise AssertionError(f"native entry {name} was reached")

    class _Ctx:
        handle, device = None, 0

    monkeypatch.setattr(L, "lib", _Refuse())
    for bad in (None, 3, np.ones(4), [np.ones(2)]):
        with pytest.raises(TypeError, match="ztmps_from_mps: unsupported operand types"):
            qil.ztmps_from_mps(bad)
    with pytest.raises(ValueError, match="maxdim must be an integer"):
        qil.signal_mps_cross(np.ones(8), maxdim=None, ctx=_Ctx())
    with pytest.raises(ValueError, match="n = 4 does not match"):
        qil.signal_mps_cross(np.ones(8), n=4, ctx=_Ctx())
    with pytest.raises(ValueError, match="float64 or complex128"):
        class _Dev:
            __cuda_array_interface__ = {"shape": (8,), "typestr": "<f4", "data": (256, False), "strides": None}
        qil.signal_mps_cross(_Dev(), ctx=_Ctx())
    doc = qil.signal_mps_cross.__doc__
    assert "blind spot" in doc and "spike" in doc and "seeds" in doc


def test_default_seeds_are_the_two_ends_and_62_drawn_indices():
    import importlib
    ops = importlib.import_module("qilaplace_jl_amd.ops")
    import cross_model as M
    for n in (1, 12, 40, 62):
        s, _ = ops._cross_seeds(n, None, 1234)
        assert s.dtype == np.int64 and len(s) == 64 and s[0] == 0 and s[1] == 2 ** n - 1
        assert s.min() >= 0 and s.max() < 2 ** n
        assert np.array_equal(s, M.default_seeds(n, 1234))
    assert not np.array_equal(ops._cross_seeds(40, None, 1)[0], ops._cross_seeds(40, None, 2)[0])
    given, _ = ops._cross_seeds(12, [5, 9], 1234)
    assert list(given) == [5, 9]
