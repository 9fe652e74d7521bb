"""CPU-side checks of qil_mps_eigs and qil_mps_eigs_local_fits: declared, exported and prototyped; the front-ends are exported; the
Makefile names the new file and the header carries the three limits; the fit decision is callable without a GPU, rejects null and
non-positive arguments, is monotone (growing an argument never turns 0 into 1) and answers 0 under QIL_EIGS_ROUTE=gemm; every
argument error of the verb comes back before any device is touched; the Python front-ends refuse bad operands before a native
entry is called; the sweep's shared steps have one home; the Julia shim and the documents name the entries."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_LENGTH, QIL_EINVAL_ARG = 1, 7
FRONT_ENDS = ("eigs", "eigs_local_fits", "eig_residual", "operator_norm", "condition_number")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_both_entries_are_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    header = _read("include", "qilaplace_hip.h")
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"QIL_API\s+int\s+qil_mps_eigs\s*\(\s*const qil_mpo\* A,\s*int which\s*,\s*const qil_mps\* x0,\s*"
                     r"const qil_mps\* const\* ortho\s*,\s*int n_ortho,\s*double weight,\s*int64_t maxdim,\s*double cutoff,\s*double tol,"
                     r"\s*int max_sweeps,\s*int krylov,\s*int restarts,\s*qil_mps\*\* out,\s*double\* theta,\s*double\* info\s*\)\s*;", decl)
    assert re.search(r"QIL_API\s+int\s+qil_mps_eigs_local_fits\s*\(\s*int complex_,\s*int64_t xl,\s*int64_t xr,\s*int64_t dl,\s*int64_t dm,"
                     r"\s*int64_t dr,\s*int krylov,\s*int n_ortho,\s*int\* fits\s*\)\s*;", decl)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert hasattr(so, "qil_mps_eigs") and hasattr(so, "qil_mps_eigs_local_fits")
    assert len(L.PROTOTYPES["qil_mps_eigs"]) == 15 and len(L.PROTOTYPES["qil_mps_eigs_local_fits"]) == 9
    make = _read("qilaplace.jl_amd", "csrc", "Makefile")
    assert "qil_eigs.hip" in make and "qil_twosite.hip" in make
    assert re.search(r"qil_twosite\.o[^\n]*qil_eigs\.o[^\n]*: qil_twosite\.h", make)
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    flat = re.sub(r"\s*\n \* +", " ", header[header.index("extremal eigenpairs (no reference counterpart)"):])
    for phrase in ("HERMITICITY IS THE CALLER'S PROMISE", "NOT PROVABLY THE EXTREMAL ONE", "an eigenvector of small bond is a fixed point",
                   "every Fourier mode is one", "stopped 9 % of |A| from lambda_min", "top_k of the transfer function's magnitude",
                   "CLUSTERED ENDS CONVERGE SLOWLY", "relative gaps of 1e-8", "QIL_EIGS_ROUTE=local / gemm",
                   "(krylov + 1 + n_ortho) * 4 xl xr + 2 * 4 xl xr max(dl, dm, dr)", "within 160 KiB", "200000 multiply-adds",
                   "Growing any argument never turns 0 into 1"):
        assert phrase in flat, phrase
    doc = " ".join(qil.eigs_local_fits.__doc__.split())
    assert "200 000 multiply-adds" in doc and "160 KiB" in doc
    doc = " ".join(qil.condition_number.__doc__.split())
    assert "LOWER bound" in doc and "small end is the slow one" in doc
    assert "GUESS THE CALLER MAY OVERRIDE" in " ".join(qil.eigs.__doc__.split())


def test_local_fits_needs_no_gpu_and_rejects_null_and_non_positive_arguments(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.delenv("QIL_EIGS_ROUTE", raising=False)
    L = _lib()
    assert qil.eigs_local_fits(1, 1, 1, 1, 1) is True
    assert qil.eigs_local_fits(1, 1, 1, 1, 1, krylov=16, n_ortho=8, dtype=np.complex128) is True
    assert qil.eigs_local_fits(4096, 4096, 8, 8, 8) is False
    assert qil.eigs_local_fits(2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40) is False
    for big in (2 ** 14 + 1, 2 ** 20, 2 ** 21, 2 ** 62):                 # every term stays far below 2^63 for any arguments
        assert qil.eigs_local_fits(big, big, big, big, big, krylov=16, n_ortho=8, dtype=np.complex128) is False
    assert qil.eigs_local_fits(1, 1, 1, 1, 1, krylov=17) is False and qil.eigs_local_fits(1, 1, 1, 1, 1, n_ortho=9) is False
    assert L.lib.qil_mps_eigs_local_fits(0, 1, 1, 1, 1, 1, 8, 0, None) == QIL_EINVAL_ARG
    assert L.last_error().startswith("eigs_local_fits: null argument")
    f = ctypes.c_int(5)
    for pos in range(5):
        for bad in (0, -1, -2 ** 40):
            dims = [2] * 5
            dims[pos] = bad
            assert L.lib.qil_mps_eigs_local_fits(0, *dims, 8, 0, ctypes.byref(f)) == QIL_EINVAL_ARG
            assert L.last_error().startswith("eigs_local_fits: dimensions must be positive")
    for krylov, n_ortho in ((0, 0), (-1, 0), (8, -1)):
        assert L.lib.qil_mps_eigs_local_fits(0, 2, 2, 2, 2, 2, krylov, n_ortho, ctypes.byref(f)) == QIL_EINVAL_ARG
        assert L.last_error().startswith("eigs_local_fits: krylov must be >= 1 and n_ortho >= 0")
    assert f.value == 5


def test_local_fits_is_monotone_in_every_argument_and_complex_never_fits_where_real_does_not(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.delenv("QIL_EIGS_ROUTE", raising=False)
    grid = (1, 2, 5, 16, 17, 40)
    rng = np.random.default_rng(5)
    points = [tuple(int(v) for v in rng.choice(grid, size=5)) + (int(rng.integers(2, 17)), int(rng.integers(0, 9))) for _ in range(300)]
    points += [(16, 16, d, d, d, 8, 0) for d in range(1, 10)] + [(x, x, 2, 2, 2, 8, 2) for x in range(1, 40, 3)]
    points += [(12, 12, 3, 3, 3, k, o) for k in (2, 8, 16) for o in (0, 4, 8)]
    seen = set()
    for p in points:
        for cx in (np.float64, np.complex128):
            fits = qil.eigs_local_fits(*p[:5], krylov=p[5], n_ortho=p[6], dtype=cx)
            seen.add(fits)
            if not fits:
                for pos in range(7):
                    for grow in (1, 7):
                        q = list(p)
                        q[pos] += grow
                        assert not qil.eigs_local_fits(*q[:5], krylov=q[5], n_ortho=q[6], dtype=cx), (p, q)
        assert qil.eigs_local_fits(*p[:5], krylov=p[5], n_ortho=p[6]) or not qil.eigs_local_fits(*p[:5], krylov=p[5], n_ortho=p[6],
                                                                                                 dtype=np.complex128)
    assert seen == {True, False}


def test_route_gemm_makes_the_decision_zero(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.setenv("QIL_EIGS_ROUTE", "gemm")
    assert qil.eigs_local_fits(1, 1, 1, 1, 1) is False
    monkeypatch.setenv("QIL_EIGS_ROUTE", "local")                       # a forced local applies only where the bond fits
    assert qil.eigs_local_fits(2, 2, 2, 2, 2) is True and qil.eigs_local_fits(64, 64, 8, 8, 8) is False
    assert qil.eigs_local_fits(16, 16, 5, 5, 5, krylov=4) is True       # ... wherever it fits the LDS (266 k multiply-adds),
    monkeypatch.delenv("QIL_EIGS_ROUTE")
    assert qil.eigs_local_fits(16, 16, 5, 5, 5, krylov=4) is False      # while auto keeps to where it was measured to win
    assert qil.eigs_local_fits(16, 16, 3, 3, 3) is True and qil.eigs_local_fits(2, 2, 2, 2, 2) is True


def test_every_argument_error_precedes_the_context_activation():
    """This runs on a machine without a GPU: an activation would fail with QIL_EHIP instead.  The stand-in handle is zeroed memory
    -- a chain of no tensors -- and is only asked for its length and labels."""
    L = _lib()
    dummy = ctypes.create_string_buffer(4096)
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    out, theta = ctypes.c_void_p(12345), ctypes.c_double(-7.0)
    one = (ctypes.c_void_p * 1)(h)
    null_entry = (ctypes.c_void_p * 1)(None)
    ok = dict(A=h, which=0, x0=h, ortho=None, n_ortho=0, weight=0.0, maxdim=8, cutoff=1e-20, tol=1e-10, max_sweeps=2, krylov=8, restarts=4)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lib.qil_mps_eigs(a["A"], a["which"], a["x0"], a["ortho"], a["n_ortho"], a["weight"], a["maxdim"], a["cutoff"], a["tol"],
                                  a["max_sweeps"], a["krylov"], a["restarts"], kw.get("out", ctypes.byref(out)),
                                  kw.get("theta", ctypes.byref(theta)), None)

    for kw in (dict(A=None), dict(x0=None), dict(out=None), dict(theta=None)):
        assert call(**kw) == QIL_EINVAL_ARG and L.last_error().startswith("eigs: null argument"), kw
    for kw in (dict(which=2), dict(which=-1)):
        assert call(**kw) == QIL_EINVAL_ARG and "which must be 0 (smallest) or 1 (largest)" in L.last_error()
    for kw in (dict(n_ortho=-1), dict(n_ortho=9, ortho=one)):
        assert call(**kw) == QIL_EINVAL_ARG and "n_ortho must be in 0 .. 8" in L.last_error()
    assert call(n_ortho=1) == QIL_EINVAL_ARG and "null ortho" in L.last_error()
    assert call(n_ortho=1, ortho=null_entry) == QIL_EINVAL_ARG and "ortho[0] is null" in L.last_error()
    for kw in (dict(krylov=1), dict(krylov=17), dict(krylov=-2)):
        assert call(**kw) == QIL_EINVAL_ARG and "krylov must be in 2 .. 16" in L.last_error()
    for kw in (dict(restarts=0), dict(restarts=-1), dict(maxdim=0), dict(maxdim=-3), dict(max_sweeps=0)):
        assert call(**kw) == QIL_EINVAL_ARG and "must be >= 1" in L.last_error()
    for kw in (dict(weight=np.inf), dict(weight=np.nan), dict(cutoff=np.nan), dict(tol=np.inf), dict(tol=np.nan)):
        assert call(**kw) == QIL_EINVAL_ARG and "must be finite" in L.last_error()
    for kw in (dict(weight=-1e-30), dict(cutoff=-1e-30), dict(tol=0.0), dict(tol=-1.0)):
        assert call(**kw) == QIL_EINVAL_ARG and "weight and cutoff must be >= 0 and tol > 0" in L.last_error()
    assert call() == QIL_EINVAL_LENGTH and "needs a bond" in L.last_error()       # a chain of no tensors has no bond either
    assert call(n_ortho=1, ortho=one) == QIL_EINVAL_LENGTH
    assert out.value == 12345 and theta.value == -7.0
    src = _read("qilaplace.jl_amd", "csrc", "qil_eigs.hip")
    body = re.search(r'extern "C" int qil_mps_eigs\(.*?\n}\n', src, flags=re.S).group(0)
    act = body.find("qil_ctx_activate")
    order = [body.find(s) for s in ("eigs: null argument", "which must be", "n_ortho must be", "krylov must be", "restarts must be",
                                    "must be finite", "must be >= 0 and tol > 0", "qil_check_apply_operands(A, x0)",
                                    "qil_check_overlap_pair(ortho[i], x0)")]
    assert all(o >= 0 for o in order) and order == sorted(order) and order[-1] < act, order
    assert body.count("qil_ctx_activate") == 1 and "qil_call_scope" in body[act:] and "qil_scratch tmp(ctx)" in body[act:]
    assert body.index("*theta = ") > body.index("sv.sweep()") and body.index("*out = ") > body.index("sv.sweep()")


def test_the_local_route_is_one_launch_of_one_workgroup_and_the_sweep_has_one_home():
    code = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_eigs.hip"))
    solve = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_solve.hip"))
    shared = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_twosite.h"))
    steps = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_twosite.hip"))
    evolve = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_evolve.hip"))
    assert len(re.findall(r"__global__ __launch_bounds__\(kThreads\) void eigs_local\(", code)) == 1
    launcher = shared[shared.index("int launch_local("):shared.index("struct Work {")]
    for once in ("qil_lds_grant", "hipLaunchKernelGGL(Kernel, dim3(1), dim3(kThreads), lds", "qil_read_back_post(", "qil_read_back_wait("):
        assert launcher.count(once) == 1 and shared.count(once) == 1, once          # the one launcher of the local kernels
    assert code.count("launch_local<eigs_local<") == 1 and code.count("launch_local<") == 1 and code.count("eigs_local<") == 1
    assert "hipLaunchKernelGGL" not in code and "dim3(" not in code             # no launch of its own
    kernel = code[code.index("void eigs_local("):code.index("void eigs_begin(")]
    assert "rs < g.restarts" in kernel and "j < g.krylov" in kernel and "atomic" not in code and "asm" not in code
    assert "while" not in kernel                                            # bounded loops only
    assert code.count("qil_mps_eigs_local_fits(dt == QIL_C64") == 1          # the verb switches on the exported decision
    assert 'getenv("QIL_EIGS_ROUTE")' in code
    # one home: both files include the header, the matvec and the environment steps are defined once
    for src in (code, solve):
        assert '#include "qil_twosite.h"' in src and "local_matvec<TE>(g, Ls, Rs, W0, W1," in src
    assert shared.count("void local_matvec(") == 1 and "void local_matvec(" not in code + solve
    for step in ("Sweep::extend(", "Sweep::gemm_matvec(", "Sweep::overlap_local(", "Sweep::split(", "Sweep::init_envs("):
        assert steps.count("int " + step) == 1 and step not in code + solve + evolve, step
    for call in ("qil_dev_gemm_batched(", "qil_apply_overlap_env_step(", "qil_overlap_env_step(", "qil_dev_svd(", "qil_truncation_rank("):
        assert call not in code, call
    for use in ("gemm_matvec(k, A0, A1,", "overlap_local(", "split(k, to_right, y, true)", "init_envs()"):
        assert use in code, use


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
    for name in ("qil_mps_eigs", "qil_mpo_adjoint", "qil_apply_mpo_mpo", "qil_apply", "qil_mps_create", "qil_apply_norm", "qil_norm",
                 "qil_inner", "qil_apply_inner", "qil_mpo_compress"):
        monkeypatch.setattr(L.lib, name, boom)
    psi, zt = _fake(qil.SignalMPS), _fake(qil.ZTMPS)
    W, Wp = _fake(qil.SingleSiteMPO), _fake(qil.PairedSiteMPO)
    for bad in (psi, None, np.zeros((4, 4))):
        with pytest.raises(TypeError, match="eigs: unsupported operand types"):
            qil.eigs(bad)
        with pytest.raises(TypeError, match="operator_norm: unsupported operand types"):
            qil.operator_norm(bad)
        with pytest.raises(TypeError, match="eigs: unsupported operand types"):
            qil.condition_number(bad)
    with pytest.raises(ValueError, match="which must be 'smallest' or 'largest'"):
        qil.eigs(W, which="middle")
    for k in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="k must be a positive integer"):
            qil.eigs(W, k=k)
    with pytest.raises(TypeError, match="maxdim must be an integer"):
        qil.eigs(W, maxdim=2.5)
    with pytest.raises(TypeError, match="eigs: unsupported operand types"):
        qil.eigs(W, ortho=[W])
    with pytest.raises(ValueError, match="at most 8 deflation states"):
        qil.eigs(W, k=10)
    with pytest.raises(ValueError, match="at most 8 deflation states"):
        qil.eigs(W, k=2, ortho=[psi] * 8)
    with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
        qil.eigs(W, x0=zt)
    with pytest.raises(TypeError, match="apply: unsupported operand types"):
        qil.eigs(W, x0=W)
    with pytest.raises(TypeError, match="apply: unsupported operand types"):
        qil.eig_residual(psi, psi, 1.0)
    with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
        qil.eig_residual(Wp, psi, 1.0)
    assert boom.calls == 0


def test_least_squares_and_operator_norm_share_the_normal_operator():
    src = _read("qilaplace.jl_amd", "ops.py")
    assert src.count("def _normal_operator(W):") == 1 and src.count("_normal_operator(W)") == 3
    assert src.count("mpo_compress(A)") == 1 and src.count("apply(W, Wd)") == 1


def test_julia_shim_and_documents_name_the_entries():
    src = _read("julia", "QILaplaceHIP.jl")
    assert "(:qil_mps_eigs, LIB)" in src and "(:qil_mps_eigs_local_fits, LIB)" in src
    assert re.search(r"function eigs\(A::DeviceMPO, x0::DeviceMPS", src)
    assert re.search(r"export .*\beigs\b", src, flags=re.S)
    integ = _read("INTEGRATION.md")
    assert "`qil_mps_eigs`" in integ and "`qil_mps_eigs_local_fits`" in integ
    readme = _read("README.md")
    for name in ("eigs", "eig_residual", "operator_norm", "condition_number"):
        assert f"`{name}`" in readme, name
    for phrase in ("NOT PROVABLY THE EXTREMAL ONE", "every Fourier mode is one", "clustered ends converge slowly", "LOWER bound"):
        assert phrase in readme, phrase
    design = _read("DESIGN.md")
    for phrase in ("qil_mps_eigs", "eigs_local", "LDS layout", "Barrier structure", "qil_twosite.h"):
        assert phrase in design, phrase
    example = _read("examples", "operator_norm.py")
    for name in ("operator_norm", "build_dt_mpo", "eig_residual", "smooth_fill"):
        assert name in example, name
    tools = _read("tools", "README.md")
    assert "_eigs_time.py" in tools and "QIL_EIGS_ROUTE" in tools
    assert "qil_mps_eigs" in _read("MEASUREMENTS.md") and os.path.exists(os.path.join(ROOT, "profiles", "r31_eigs_time.jsonl"))
