"""CPU-side checks of qil_environment: declared with its signature, exported and bound; the defines are present and the Makefile
lists the file; null arguments, a bad side and a count out of range come back before any device is touched, and those checks sit
ahead of the context activation in the source; the route hook sends a state bond of 16 to the chain and 17 to the GEMMs; the
Python front-ends are exported and refuse bad operands before a native entry is called; the Julia shim binds the entry and the
documents name it."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

SIGNATURE = (r"const qil_mps\* phi,\s*const qil_mpo\* W,\s*const qil_mps\* psi,\s*int side,\s*int64_t count,\s*double\* out,\s*"
             r"int64_t\* dims")
FRONT_ENDS = ("environment", "shift_pencil", "esprit_from_pencil", "esprit")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _source():
    return _read("qilaplace.jl_amd", "csrc", "qil_environment.hip")


def test_the_entry_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    header = _read("include", "qilaplace_hip.h")
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"QIL_API\s+int\s+qil_environment\s*\(\s*" + SIGNATURE + r"\s*\)\s*;", decl)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert hasattr(so, "qil_environment") and hasattr(so, "qil_environment_route")
    assert len(L.PROTOTYPES["qil_environment"]) == 7 and len(L.PROTOTYPES["qil_environment_route"]) == 7
    assert re.search(r"#define QIL_ENV_LEFT\s+0\b", decl) and re.search(r"#define QIL_ENV_RIGHT\s+1\b", decl)
    cap = int(re.search(r"#define QIL_ENV_CHAIN_MAX_OP_BOND (\d+)\b", decl).group(1))
    assert cap >= 4 and cap == qil.ops.ENV_CHAIN_MAX_OP_BOND
    assert qil.ops.ENV_SIDES == {"left": 0, "right": 1}
    assert re.search(r"QIL_API\s+int\s+qil_environment_route\s*\(", decl)
    assert "qil_environment.hip" in _read("qilaplace.jl_amd", "csrc", "Makefile")
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    flat = re.sub(r"\s*\n \* +", " ", header[header.index("environments (no reference counterpart)"):])
    for phrase in ("amplitudes are NOT applied", "the size query", "QIL_ENV_ROUTE=chain / gemm"):
        assert phrase in flat, phrase


def test_null_arguments_a_bad_side_and_a_bad_count_precede_the_context_activation():
    """QIL_EINVAL_ARG with messages that start `environment:`.  This runs on a machine without a GPU: an activation would fail with
    QIL_EHIP instead.  The stand-in handle is zeroed memory -- a chain of no sites -- and is only asked for its length."""
    L = _lib()
    dummy = ctypes.create_string_buffer(4096)
    handle = ctypes.c_void_p(ctypes.addressof(dummy))
    dims = (ctypes.c_int64 * 3)(7, 7, 7)
    out = (ctypes.c_double * 2)(5.0, 5.0)
    for args in ((None, None, handle, 0, 0, out, dims), (handle, None, None, 0, 0, out, dims), (handle, None, handle, 0, 0, out, None),
                 (None, None, None, 5, -1, None, None)):
        assert L.lib.qil_environment(*args) == QIL_EINVAL_ARG
        assert L.last_error().startswith("environment: null argument")
    for side in (-1, 2, 77):
        assert L.lib.qil_environment(handle, None, handle, side, 0, out, dims) == QIL_EINVAL_ARG
        assert L.last_error().startswith("environment: side must be 0 (left) or 1 (right)")
    for count in (-1, 1, 2 ** 40):
        assert L.lib.qil_environment(handle, None, handle, 1, count, out, dims) == QIL_EINVAL_ARG
        assert L.last_error().startswith(f"environment: count {count} outside [0, 0]")
    assert list(dims) == [7, 7, 7] and list(out) == [5.0, 5.0]


def test_the_argument_checks_sit_first_in_the_body():
    src = _source()
    m = re.search(r'extern "C" int qil_environment\(.*?\n}\n', src, flags=re.S)
    assert m
    body = m.group(0)
    assert body[body.index("{") + 1:].lstrip().startswith('QIL_REQUIRE(phi && psi && dims, QIL_EINVAL_ARG, "environment: null argument");')
    act = body.find("qil_ctx_activate")
    order = [body.find(s) for s in ("environment: null argument", "environment: side must be", "environment: count %lld outside",
                                    "qil_check_apply_operands(W, psi)", "qil_check_overlap_pair(phi, psi)", "if (!out) return QIL_OK;")]
    assert all(o >= 0 for o in order) and order == sorted(order) and order[-1] < act, order
    assert body.count("qil_ctx_activate") == 1 and "qil_call_scope" in body[act:] and "qil_scratch tmp(ctx)" in body[act:]
    assert "qil_download(" in body[act:]
    # the operand checks are the overlap verbs' own, not restated
    inner = _read("qilaplace.jl_amd", "csrc", "qil_inner.hip")
    assert inner.count("int qil_check_overlap_pair(") == 1 and inner.count("QIL_TRY(qil_check_overlap_pair(phi, psi));") == 2


def test_the_chain_route_is_one_kernel_and_the_gemm_route_shares_the_overlap_steps():
    code = re.sub(r"//[^\n]*", "", _source())
    assert len(re.findall(r"__global__ __launch_bounds__\(kThreads\) void env_chain\(", code)) == 1
    assert code.count("__global__") == 1
    assert code.count("hipLaunchKernelGGL((env_chain<") == 1 and "dim3(1), dim3(kThreads)" in code      # one launch, one workgroup
    assert 'getenv("QIL_ENV_ROUTE")' in code and code.count("static int env_route(") == 1
    assert code.count("env_route(side, count, n,") == 2                   # the hook and the entry call it: one decision
    for shared in ("qil_overlap_env_step(", "qil_apply_overlap_env_step(", "QIL_SITE_REVERSED", "qil_dev_finish_coeff(", "qil_dev_table",
                   "qil_lds_grant"):
        assert shared in code, shared
    assert "qil_dev_gemm" not in code and "asm" not in code and "atomic" not in code
    # no barrier inside a branch on thread data: every __syncthreads() sits at the site loop's level or inside `if constexpr`
    kernel = code[code.index("void env_chain("):code.index("static void walked_span")]
    for m in re.finditer(r"__syncthreads\(\);", kernel):
        indent = kernel[kernel.rfind("\n", 0, m.start()) + 1:m.start()]
        assert indent in ("    ", "        ", "            "), repr(indent)
    # the steps live once, in qil_contract.hip, and the overlap verbs use them
    contract, inner = _read("qilaplace.jl_amd", "csrc", "qil_contract.hip"), _read("qilaplace.jl_amd", "csrc", "qil_inner.hip")
    for name in ("qil_overlap_env_step", "qil_apply_overlap_env_step"):
        assert contract.count("\nint " + name + "(") == 1 and ("QIL_TRY(" + name + "(") in inner, name


def test_the_route_hook_sends_16_to_the_chain_and_17_to_the_gemms(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.delenv("QIL_ENV_ROUTE", raising=False)
    route = qil.ops.environment_route
    cap = qil.ops.ENV_CHAIN_MAX_OP_BOND
    flat = [1, 2, 2, 2, 2, 1]
    for side in ("left", "right"):
        for count in (1, 3, 5):
            assert route(side, count, [1, 16, 16, 16, 16, 1], flat) == "CHAIN"
            assert route(side, count, flat, [1, 16, 16, 16, 16, 1]) == "CHAIN"
            assert route(side, count, [1, 17, 17, 17, 17, 1], flat) == "GEMM"
            assert route(side, count, flat, [1, 17, 17, 17, 17, 1]) == "GEMM"
            assert route(side, count, flat, flat, [1] + [cap] * 4 + [1]) == "CHAIN"
            assert route(side, count, flat, flat, [1] + [cap + 1] * 4 + [1]) == "GEMM"
    # only the walked tensors count: the 17 sits at bond 2
    dims = [1, 2, 17, 2, 2, 1]
    assert [route("left", c, dims, flat) for c in range(6)] == ["CHAIN", "CHAIN", "GEMM", "GEMM", "GEMM", "GEMM"]
    assert [route("right", c, dims, flat) for c in range(6)] == ["CHAIN", "CHAIN", "CHAIN", "GEMM", "GEMM", "GEMM"]
    monkeypatch.setenv("QIL_ENV_ROUTE", "gemm")
    assert route("left", 3, flat, flat) == "GEMM"
    monkeypatch.setenv("QIL_ENV_ROUTE", "chain")                          # a forced chain applies only where the bonds fit
    assert route("left", 3, flat, flat) == "CHAIN" and route("left", 3, dims, flat) == "GEMM"
    monkeypatch.delenv("QIL_ENV_ROUTE")
    for bad in ((2, 1), (0, 6), (0, -1)):
        with pytest.raises(ValueError, match="environment_route: "):
            L = _lib()
            r = ctypes.c_int()
            d = (ctypes.c_int64 * 6)(*flat)
            L.check(L.lib.qil_environment_route(bad[0], bad[1], 5, d, d, None, ctypes.byref(r)))


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
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()

    def nsites(handle, ref):
        ref._obj.value = 6
        return 0

    monkeypatch.setattr(L.lib, "qil_mps_nsites", nsites)
    for name in ("qil_environment", "qil_mps_clone", "qil_compress", "qil_mps_bond_dims", "qil_mps_create", "qil_mpo_create",
                 "qil_product_batch", "qil_inner", "qil_apply_inner"):
        monkeypatch.setattr(L.lib, name, boom)
    psi, zt = _fake(qil.SignalMPS), _fake(qil.ZTMPS)                      # 6 tensors each: 6 and 3 sites
    W, Wp = _fake(qil.SingleSiteMPO), _fake(qil.PairedSiteMPO)
    for bad in (None, np.zeros((1, 2, 1)), W):
        with pytest.raises(TypeError, match="environment: unsupported operand types"):
            qil.environment(bad, psi)
        with pytest.raises(TypeError, match="environment: unsupported operand types"):
            qil.environment(psi, bad)
    for bad in (psi, np.zeros((1, 2, 2, 1))):
        with pytest.raises(TypeError, match="apply: unsupported operand types"):
            qil.environment(psi, psi, W=bad)
    for op, state in ((Wp, psi), (W, zt)):
        with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
            qil.environment(state, state, W=op)
    for side in ("up", 0, None):
        with pytest.raises(ValueError, match="side must be 'left' or 'right'"):
            qil.environment(psi, psi, side=side)
    for count in (-1, 7, 1 << 40):
        with pytest.raises(ValueError, match=r"outside \[0, 6\]"):
            qil.environment(psi, psi, count=count)
        with pytest.raises(ValueError, match=r"outside \[0, 6\]"):
            qil.environment(zt, zt, count=count)                          # tensors of the 2n chain
    for count in (1.5, "2", True):
        with pytest.raises(TypeError, match="count must be an integer"):
            qil.environment(psi, psi, count=count)
    for fn, args in ((qil.shift_pencil, (3,)), (qil.esprit, ())):
        for bad in (None, W, np.zeros(8)):
            with pytest.raises(TypeError, match=fn.__name__ + ": unsupported operand types"):
                fn(bad, *args)
        with pytest.raises(TypeError, match="a ZTMPS has no single sample register"):
            fn(zt, *args)
    for count in (0, 6, -2, 99):
        with pytest.raises(ValueError, match=r"outside \[1, 5\]"):
            qil.shift_pencil(psi, count)
        with pytest.raises(ValueError, match=r"outside \[1, 5\]"):
            qil.esprit(psi, count=count)
    with pytest.raises(TypeError, match="count must be an integer"):
        qil.esprit(psi, count=2.0)
    assert boom.calls == 0


def test_esprit_from_pencil_needs_no_device():
    import qilaplace_jl_amd as qil
    z = np.array([0.9 * np.exp(0.7j), np.exp(-2.1j)])
    c = np.array([1.0, 0.5 - 0.2j])
    T = np.array([[1.0, 0.3], [-0.4j, 1.0]])
    R = T @ (c[:, None] * z[:, None] ** np.arange(64)[None, :])
    got = qil.esprit_from_pencil(R @ R.conj().T, R[:, 1:] @ R[:, :-1].conj().T, R[:, -1])
    assert max(np.abs(got - p).min() for p in z) < 1e-13
    for bad in ((np.eye(2), np.eye(3), np.ones(2)), (np.eye(2), np.eye(2), np.ones(3))):
        with pytest.raises(ValueError, match="expected G and P of shape"):
            qil.esprit_from_pencil(*bad)
    with pytest.raises(ValueError, match="not finite"):
        qil.esprit_from_pencil(np.full((1, 1), np.nan), np.eye(1), np.ones(1))


def test_julia_shim_and_documents_name_the_entry():
    src = _read("julia", "QILaplaceHIP.jl")
    assert "(:qil_environment, LIB)" in src
    assert re.search(r"function environment\(phi::DeviceMPS, psi::DeviceMPS", src)
    assert re.search(r"export .*\benvironment\b", src, flags=re.S)
    assert "`qil_environment`" in _read("INTEGRATION.md")
    readme = _read("README.md")
    for name in ("environment", "shift_pencil", "esprit_from_pencil", "esprit"):
        assert f"`{name}`" in readme, name
    assert "zt_eval" in readme[readme.index("`esprit`"):]                  # where it stands against a placed window is said
    design = _read("DESIGN.md")
    for phrase in ("qil_environment", "ESPRIT", "leftmost bond"):
        assert phrase in design, phrase
    example = _read("examples", "esprit_poles.py")
    for name in ("esprit", "exponential_sum", "signal_mps"):
        assert name in example, name
    tools = _read("tools", "README.md")
    assert "_environment_time.py" in tools and "QIL_ENV_ROUTE" in tools
    assert "qil_environment" in _read("MEASUREMENTS.md")
