"""CPU-side checks of qil_mps_solve and qil_mps_solve_local_fits: declared, exported and prototyped; the fit decision is callable
without a GPU, rejects null and non-positive dimensions, is monotone (growing a dimension never turns 0 into 1) and answers 0
under QIL_SOLVE_ROUTE=gemm; the argument errors of the verb come back before any device is touched; the Python front-ends are
exported and refuse bad operands before a native entry is called; the Julia shim and the documents name the entries."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_LENGTH, QIL_EINVAL_ARG = 1, 7
FRONT_ENDS = ("solve", "solve_local_fits", "solve_residual", "least_squares", "smooth", "build_laplacian_mpo", "laplacian_mpo_tensors")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_both_entries_are_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", _read("include", "qilaplace_hip.h"), flags=re.S)
    assert re.search(r"QIL_API\s+int\s+qil_mps_solve\s*\(\s*const qil_mpo\* A,\s*double shift,\s*const qil_mps\* c,\s*const qil_mps\* x0\s*,"
                     r"\s*int64_t maxdim,\s*double cutoff,\s*double tol,\s*int max_sweeps,\s*int cg_iters,\s*qil_mps\*\* out,\s*"
                     r"double\* info\s*\)\s*;", decl)
    assert re.search(r"QIL_API\s+int\s+qil_mps_solve_local_fits\s*\(\s*int complex_,\s*int64_t xl,\s*int64_t xr,\s*int64_t dl,\s*int64_t dm,"
                     r"\s*int64_t dr,\s*int64_t cl,\s*int64_t cm,\s*int64_t cr,\s*int\* fits\s*\)\s*;", decl)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert hasattr(so, "qil_mps_solve") and hasattr(so, "qil_mps_solve_local_fits")
    assert len(L.PROTOTYPES["qil_mps_solve"]) == 11 and len(L.PROTOTYPES["qil_mps_solve_local_fits"]) == 10
    make = _read("qilaplace.jl_amd", "csrc", "Makefile")
    assert "qil_solve.hip" in make and "qil_twosite.hip" in make
    assert re.search(r"qil_twosite\.o[^\n]*qil_solve\.o[^\n]*: qil_twosite\.h", make)
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    header = _read("include", "qilaplace_hip.h")
    flat = re.sub(r"\s*\n \* +", " ", header[header.index("linear solver (no reference counterpart)"):])
    for phrase in ("HERMITICITY IS THE CALLER'S PROMISE", "QIL_SOLVE_ROUTE=local / gemm", "12 xl xr + 2 blk", "within 160 KiB", "200000 multiply-adds"):
        assert phrase in flat, phrase


def test_local_fits_needs_no_gpu_and_rejects_null_and_non_positive_dimensions(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.delenv("QIL_SOLVE_ROUTE", raising=False)
    L = _lib()
    assert qil.solve_local_fits(1, 1, 1, 1, 1, 1, 1, 1) is True
    assert qil.solve_local_fits(1, 1, 1, 1, 1, 1, 1, 1, dtype=np.complex128) is True
    assert qil.solve_local_fits(4096, 4096, 8, 8, 8, 1, 1, 1) is False
    assert qil.solve_local_fits(2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40) is False
    assert L.lib.qil_mps_solve_local_fits(0, 1, 1, 1, 1, 1, 1, 1, 1, None) == QIL_EINVAL_ARG
    assert L.last_error().startswith("solve_local_fits: null argument")
    f = ctypes.c_int(5)
    for pos in range(8):
        for bad in (0, -1, -2 ** 40):
            dims = [2] * 8
            dims[pos] = bad
            assert L.lib.qil_mps_solve_local_fits(0, *dims, ctypes.byref(f)) == QIL_EINVAL_ARG
            assert L.last_error().startswith("solve_local_fits: dimensions must be positive")
    assert f.value == 5


def test_local_fits_is_monotone_and_complex_never_fits_where_real_does_not(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.delenv("QIL_SOLVE_ROUTE", raising=False)
    grid = (1, 2, 5, 16, 17, 40)
    rng = np.random.default_rng(5)
    points = [tuple(int(v) for v in rng.choice(grid, size=8)) for _ in range(300)]
    points += [(16, 16, d, d, d, 16, 16, 16) for d in range(1, 10)] + [(x, x, 2, 2, 2, x, x, x) for x in range(1, 40, 3)]
    seen = set()
    for p in points:
        for cx in (np.float64, np.complex128):
            fits = qil.solve_local_fits(*p, dtype=cx)
            seen.add(fits)
            if not fits:
                for pos in range(8):
                    for grow in (1, 7):
                        q = list(p)
                        q[pos] += grow
                        assert not qil.solve_local_fits(*q, dtype=cx), (p, q)
        assert qil.solve_local_fits(*p) or not qil.solve_local_fits(*p, dtype=np.complex128)
    assert seen == {True, False}


def test_route_gemm_makes_the_decision_zero(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.setenv("QIL_SOLVE_ROUTE", "gemm")
    assert qil.solve_local_fits(1, 1, 1, 1, 1, 1, 1, 1) is False
    monkeypatch.setenv("QIL_SOLVE_ROUTE", "local")                      # a forced local applies only where the bond fits
    assert qil.solve_local_fits(2, 2, 2, 2, 2, 2, 2, 2) is True and qil.solve_local_fits(64, 64, 8, 8, 8, 1, 1, 1) is False
    assert qil.solve_local_fits(16, 16, 5, 5, 5, 4, 4, 4) is True       # ... wherever it fits the LDS,
    monkeypatch.delenv("QIL_SOLVE_ROUTE")
    assert qil.solve_local_fits(16, 16, 5, 5, 5, 4, 4, 4) is False      # while auto keeps to where it was measured to win
    assert qil.solve_local_fits(16, 16, 3, 3, 3, 4, 4, 4) is True and qil.solve_local_fits(2, 2, 2, 2, 2, 2, 2, 2) is True


def test_argument_errors_precede_the_context_activation():
    """This runs on a machine without a GPU: an activation would fail with QIL_EHIP instead.  The stand-in handle is zeroed memory
    -- a chain of no tensors -- and is only asked for its length and labels."""
    L = _lib()
    dummy = ctypes.create_string_buffer(4096)
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    out = ctypes.c_void_p(12345)
    ok = dict(A=h, shift=0.0, c=h, x0=None, maxdim=8, cutoff=1e-20, tol=1e-10, max_sweeps=2, cg_iters=10)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lib.qil_mps_solve(a["A"], a["shift"], a["c"], a["x0"], a["maxdim"], a["cutoff"], a["tol"], a["max_sweeps"], a["cg_iters"],
                                   kw.get("out", ctypes.byref(out)), None)

    for kw in (dict(A=None), dict(c=None), dict(out=None)):
        assert call(**kw) == QIL_EINVAL_ARG and L.last_error().startswith("solve: null argument")
    for kw in (dict(maxdim=0), dict(maxdim=-3), dict(max_sweeps=0), dict(cg_iters=0), dict(cg_iters=-1)):
        assert call(**kw) == QIL_EINVAL_ARG and "must be >= 1" in L.last_error()
    for kw in (dict(shift=np.inf), dict(shift=np.nan), dict(cutoff=np.nan), dict(tol=np.inf), dict(tol=np.nan)):
        assert call(**kw) == QIL_EINVAL_ARG and "must be finite" in L.last_error()
    for kw in (dict(cutoff=-1e-30), dict(tol=0.0), dict(tol=-1.0)):
        assert call(**kw) == QIL_EINVAL_ARG and "cutoff must be >= 0 and tol > 0" in L.last_error()
    assert call() == QIL_EINVAL_LENGTH and "needs a bond" in L.last_error()       # a chain of no tensors has no bond either
    assert out.value == 12345
    src = _read("qilaplace.jl_amd", "csrc", "qil_solve.hip")
    body = re.search(r'extern "C" int qil_mps_solve\(.*?\n}\n', src, flags=re.S).group(0)
    act = body.find("qil_ctx_activate")
    order = [body.find(s) for s in ("solve: null argument", "must be >= 1", "must be finite", "cutoff must be >= 0", "needs a bond",
                                    "qil_check_apply_operands(A, c)", "qil_check_overlap_pair(x0, c)")]
    assert all(o >= 0 for o in order) and order == sorted(order) and order[-1] < act, order
    assert body.count("qil_ctx_activate") == 1 and "qil_call_scope" in body[act:] and "qil_scratch tmp(ctx)" in body[act:]


def test_the_local_route_is_one_launch_of_one_workgroup_without_spins_or_atomics():
    code = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_solve.hip"))
    assert len(re.findall(r"__global__ __launch_bounds__\(kThreads\) void solve_local\(", code)) == 1
    shared = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_twosite.h"))
    steps = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_twosite.hip"))
    launcher = shared[shared.index("int launch_local("):shared.index("struct Work {")]
    for once in ("qil_lds_grant", "hipLaunchKernelGGL(Kernel, dim3(1), dim3(kThreads), lds", "qil_read_back_post(", "qil_read_back_wait("):
        assert launcher.count(once) == 1 and shared.count(once) == 1, once          # the one launcher of the local kernels
    assert code.count("launch_local<solve_local<") == 1 and code.count("launch_local<") == 1 and code.count("solve_local<") == 1
    assert "hipLaunchKernelGGL" not in code and "dim3(" not in code             # no launch of its own
    kernel = code[code.index("void solve_local("):code.index("void cg_start(")]
    assert "it < g.cg_iters" in kernel and "atomic" not in code and "asm" not in code
    for step in ("qil_gauge_exact(", "qil_dev_svd(", "qil_truncation_rank(", "qil_apply_overlap_env_step(", "qil_overlap_env_step(",
                 "QIL_SITE_REVERSED", "qil_dev_gemm_batched("):
        assert step in steps and step not in code, step                            # the host steps live in qil_twosite.hip
    assert 'getenv("QIL_SOLVE_ROUTE")' in code
    assert code.count("qil_mps_solve_local_fits(dt == QIL_C64") == 1          # the verb switches on the exported decision


class _Boom:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        raise AssertionError("native call made before the argument checks")


def _fake(cls):
    x = object.__new__(cls)
    x.handle = None
    x.ctx = None
    return x


def test_python_checks_precede_the_native_entries(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()
    for name in ("qil_mps_solve", "qil_mpo_adjoint", "qil_apply_mpo_mpo", "qil_apply", "qil_mpo_create", "qil_mpo_sum", "qil_apply_norm",
                 "qil_norm", "qil_inner", "qil_apply_inner", "qil_hadamard", "qil_mpo_diagonal"):
        monkeypatch.setattr(L.lib, name, boom)
    psi, zt = _fake(qil.SignalMPS), _fake(qil.ZTMPS)
    W, Wp = _fake(qil.SingleSiteMPO), _fake(qil.PairedSiteMPO)
    for fn in (qil.solve, qil.least_squares):
        for bad in ((psi, psi), (W, W), (None, psi), (W, np.zeros(4))):
            with pytest.raises(TypeError, match="apply: unsupported operand types"):
                fn(*bad)
        for op, state in ((Wp, psi), (W, zt)):
            with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
                fn(op, state)
    with pytest.raises(TypeError, match="solve: unsupported operand types"):
        qil.solve(W, psi, x0=W)
    with pytest.raises(TypeError, match="maxdim must be an integer"):
        qil.solve(W, psi, maxdim=2.5)
    with pytest.raises(TypeError, match="apply: unsupported operand types"):
        qil.solve_residual(psi, psi, psi)
    with pytest.raises(TypeError, match="solve_residual: unsupported operand types"):
        qil.solve_residual(W, psi, W)
    for bad in (None, W, np.zeros(8)):
        with pytest.raises(TypeError, match="smooth: unsupported operand types"):
            qil.smooth(bad, 1.0)
    with pytest.raises(TypeError, match="smooth: unsupported operand types"):
        qil.smooth(zt, 1.0)
    for order in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="order must be a positive integer"):
            qil.smooth(psi, 1.0, order=order)
    for alpha in (-1.0, np.nan):
        with pytest.raises(ValueError, match="alpha must be >= 0"):
            qil.smooth(psi, alpha)
    assert boom.calls == 0


def test_julia_shim_and_documents_name_the_entries():
    src = _read("julia", "QILaplaceHIP.jl")
    assert "(:qil_mps_solve, LIB)" in src and "(:qil_mps_solve_local_fits, LIB)" in src
    assert re.search(r"function solve\(A::DeviceMPO, c::DeviceMPS", src)
    assert re.search(r"export .*\bsolve\b", src, flags=re.S)
    integ = _read("INTEGRATION.md")
    assert "`qil_mps_solve`" in integ and "`qil_mps_solve_local_fits`" in integ
    readme = _read("README.md")
    for name in ("solve", "least_squares", "smooth", "solve_residual", "build_laplacian_mpo"):
        assert f"`{name}`" in readme, name
    design = _read("DESIGN.md")
    for phrase in ("qil_mps_solve", "conjugate", "solve_local", "QIL_SOLVE_ROUTE"):
        assert phrase in design, phrase
    example = _read("examples", "smooth_fill.py")
    for name in ("smooth", "exponential_sum", "mask"):
        assert name in example, name
    tools = _read("tools", "README.md")
    assert "_solve_time.py" in tools and "QIL_SOLVE_ROUTE" in tools
    assert "qil_mps_solve" in _read("MEASUREMENTS.md")
