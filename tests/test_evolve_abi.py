"""CPU-side checks of qil_mps_evolve and qil_mps_evolve_local_fits: declared, exported and prototyped; the front-ends are exported;
the Makefile names the new file and the header carries the limits; the fit decision is callable without a GPU, rejects null,
non-positive and out-of-range arguments, is monotone (growing an argument never turns 0 into 1), never fits complex where real
does not, fits one site wherever two sites fit (dm >= min(dl, dr)) and answers 0 under QIL_EVOLVE_ROUTE=gemm; every argument error
of the verb comes back before any device is touched; the Python front-ends refuse bad operands before a native entry is called;
the one-site matvec has one home; the Julia shim and the documents name the entries."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_LENGTH, QIL_EINVAL_ARG = 1, 7
FRONT_ENDS = ("evolve", "propagate", "diffuse", "evolve_local_fits")


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
    assert re.search(r"QIL_API\s+int\s+qil_mps_evolve\s*\(\s*const qil_mpo\* A,\s*const qil_mps\* x0,\s*double tau_re,\s*double tau_im,"
                     r"\s*int steps,\s*int64_t maxdim,\s*double cutoff,\s*double tol,\s*int krylov,\s*int substeps,\s*qil_mps\*\* out,"
                     r"\s*double\* info\s*\)\s*;", decl)
    assert re.search(r"QIL_API\s+int\s+qil_mps_evolve_local_fits\s*\(\s*int complex_,\s*int sites\s*,\s*int64_t xl,\s*int64_t xr,"
                     r"\s*int64_t dl,\s*int64_t dm\s*,\s*int64_t dr,\s*int krylov,\s*int\* fits\s*\)\s*;", decl)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert hasattr(so, "qil_mps_evolve") and hasattr(so, "qil_mps_evolve_local_fits")
    assert len(L.PROTOTYPES["qil_mps_evolve"]) == 12 and len(L.PROTOTYPES["qil_mps_evolve_local_fits"]) == 9
    make = _read("qilaplace.jl_amd", "csrc", "Makefile")
    assert "qil_evolve.hip" in make and re.search(r"qil_evolve\.o[^\n]*: qil_twosite\.h", make)
    assert "qil_twosite.hip" in make and re.search(r"qil_twosite\.o[^\n]*: qil_twosite\.h", make)
    assert "global: qil_*;" in _read("qilaplace.jl_amd", "csrc", "libqilhip.map")
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    flat = re.sub(r"\s*\n \* +", " ", header[header.index("time evolution (no reference counterpart)"):])
    for phrase in ("THE STIFF LIMIT", "exp(|Re tau| / 2 * spread(A))", "returned garbage (error 1e12) at tau = -20 in one step",
                   "|Re tau| * spread(A) of order one per step and for any imaginary tau",
                   "The error with a binding maxdim is the projection error and does not fall with the step",
                   "A start narrower than the bonds it grows to costs first order in tau once",
                   "QIL_EVOLVE_ROUTE=local / gemm", "(krylov + 1) * 4 xl xr + 2 * 4 xl xr max(dl, dm, dr)",
                   "(krylov + 1) * 2 xl xr + 2 * 2 xl xr max(dl, dr)", "within 160 KiB", "200000 multiply-adds",
                   "2 xl^2 xr dl + 4 xl xr dl dr + 2 xl xr^2 dr", "Growing any argument never turns 0 into 1",
                   "Hermitian operator A in MPS form (the caller's promise, not checked"):
        assert phrase in flat, phrase
    doc = " ".join(qil.evolve_local_fits.__doc__.split())
    assert "200 000 multiply-adds" in doc and "160 KiB" in doc
    doc = " ".join(qil.evolve.__doc__.split())
    for phrase in ("THE STIFF LIMIT", "strong smoothing stays with `smooth`", "Fourier route", "does not fall with the step",
                   "first order in tau once"):
        assert phrase in doc, phrase
    assert "smooth" in " ".join(qil.diffuse.__doc__.split()) and "evolve(H, x, -1j * t)" in " ".join(qil.propagate.__doc__.split())


def test_local_fits_needs_no_gpu_and_rejects_bad_arguments(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.delenv("QIL_EVOLVE_ROUTE", raising=False)
    L = _lib()
    assert qil.evolve_local_fits(1, 1, 1, 1, 1) is True and qil.evolve_local_fits(1, 1, 1, 1, 1, sites=1) is True
    assert qil.evolve_local_fits(1, 1, 1, 1, 1, krylov=16, dtype=np.complex128) is True
    assert qil.evolve_local_fits(4096, 4096, 8, 8, 8) is False and qil.evolve_local_fits(4096, 4096, 8, 8, 8, sites=1) is False
    for big in (2 ** 14 + 1, 2 ** 20, 2 ** 40, 2 ** 62):                 # every term stays far below 2^63 for any arguments
        for sites in (1, 2):
            assert qil.evolve_local_fits(big, big, big, big, big, sites=sites, krylov=16, dtype=np.complex128) is False
    assert qil.evolve_local_fits(1, 1, 1, 1, 1, krylov=17) is False
    assert qil.evolve_local_fits(2, 2, 2, -5, 2, sites=1) is True          # dm is ignored for one site
    assert L.lib.qil_mps_evolve_local_fits(0, 2, 1, 1, 1, 1, 1, 8, None) == QIL_EINVAL_ARG
    assert L.last_error().startswith("evolve_local_fits: null argument")
    f = ctypes.c_int(5)
    for sites in (0, 3, -1):
        assert L.lib.qil_mps_evolve_local_fits(0, sites, 2, 2, 2, 2, 2, 8, ctypes.byref(f)) == QIL_EINVAL_ARG
        assert L.last_error().startswith("evolve_local_fits: sites must be 1 or 2")
    for pos in range(5):
        for bad in (0, -1, -2 ** 40):
            dims = [2] * 5
            dims[pos] = bad
            assert L.lib.qil_mps_evolve_local_fits(0, 2, *dims, 8, ctypes.byref(f)) == QIL_EINVAL_ARG
            assert L.last_error().startswith("evolve_local_fits: dimensions must be positive")
            if pos != 3:
                assert L.lib.qil_mps_evolve_local_fits(0, 1, *dims, 8, ctypes.byref(f)) == QIL_EINVAL_ARG
    for krylov in (0, -1):
        assert L.lib.qil_mps_evolve_local_fits(0, 2, 2, 2, 2, 2, 2, krylov, ctypes.byref(f)) == QIL_EINVAL_ARG
        assert L.last_error().startswith("evolve_local_fits: krylov must be >= 1")
    assert f.value == 5


def test_local_fits_is_monotone_and_ordered_between_types_and_sites(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.delenv("QIL_EVOLVE_ROUTE", raising=False)
    grid = (1, 2, 5, 16, 17, 40)
    rng = np.random.default_rng(5)
    points = [tuple(int(v) for v in rng.choice(grid, size=5)) + (int(rng.integers(2, 17)),) for _ in range(300)]
    points += [(16, 16, d, d, d, 8) for d in range(1, 10)] + [(x, x, 2, 2, 2, 8) for x in range(1, 48, 3)]
    points += [(12, 12, 3, 3, 3, k) for k in (2, 8, 16)] + [(x, x, 5, 5, 5, 8) for x in range(8, 40, 2)]
    seen = set()
    for p in points:
        for sites in (1, 2):
            for cx in (np.float64, np.complex128):
                fits = qil.evolve_local_fits(*p[:5], sites=sites, krylov=p[5], dtype=cx)
                seen.add((sites, fits))
                if not fits:
                    for pos in range(6):
                        for grow in (1, 7):
                            q = list(p)
                            q[pos] += grow
                            assert not qil.evolve_local_fits(*q[:5], sites=sites, krylov=q[5], dtype=cx), (sites, p, q)
            assert qil.evolve_local_fits(*p[:5], sites=sites, krylov=p[5]) or \
                not qil.evolve_local_fits(*p[:5], sites=sites, krylov=p[5], dtype=np.complex128)
        if p[3] >= min(p[2], p[4]):                                         # where every term of the one-site formulas is no larger
            for cx in (np.float64, np.complex128):
                assert qil.evolve_local_fits(*p[:5], sites=1, krylov=p[5], dtype=cx) or \
                    not qil.evolve_local_fits(*p[:5], sites=2, krylov=p[5], dtype=cx), p
    assert seen == {(1, True), (1, False), (2, True), (2, False)}


def test_route_gemm_makes_the_decision_zero(monkeypatch):
    import qilaplace_jl_amd as qil
    monkeypatch.setenv("QIL_EVOLVE_ROUTE", "gemm")
    assert qil.evolve_local_fits(1, 1, 1, 1, 1) is False and qil.evolve_local_fits(1, 1, 1, 1, 1, sites=1) is False
    monkeypatch.setenv("QIL_EVOLVE_ROUTE", "local")                     # a forced local applies only where the tensors fit
    assert qil.evolve_local_fits(2, 2, 2, 2, 2) is True and qil.evolve_local_fits(64, 64, 8, 8, 8) is False
    assert qil.evolve_local_fits(16, 16, 5, 5, 5, krylov=4) is True       # ... wherever it fits the LDS (266 k multiply-adds),
    monkeypatch.delenv("QIL_EVOLVE_ROUTE")
    assert qil.evolve_local_fits(16, 16, 5, 5, 5, krylov=4) is False      # while auto keeps the size rule
    assert qil.evolve_local_fits(16, 16, 5, 5, 5, krylov=4, sites=1) is True   # 133 k multiply-adds for the one-site matvec
    assert qil.evolve_local_fits(16, 16, 3, 3, 3) is True and qil.evolve_local_fits(2, 2, 2, 2, 2) is True


def test_every_argument_error_precedes_the_context_activation():
    """This runs on a machine without a GPU: an activation would fail with QIL_EHIP instead.  The stand-in handle is zeroed memory
    -- a chain of no tensors -- and is only asked for its length and labels."""
    L = _lib()
    dummy = ctypes.create_string_buffer(4096)
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    out = ctypes.c_void_p(12345)
    ok = dict(A=h, x0=h, tau_re=-0.5, tau_im=0.25, steps=2, maxdim=8, cutoff=1e-20, tol=1e-10, krylov=8, substeps=4)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lib.qil_mps_evolve(a["A"], a["x0"], a["tau_re"], a["tau_im"], a["steps"], a["maxdim"], a["cutoff"], a["tol"],
                                    a["krylov"], a["substeps"], kw.get("out", ctypes.byref(out)), None)

    for kw in (dict(A=None), dict(x0=None), dict(out=None)):
        assert call(**kw) == QIL_EINVAL_ARG and L.last_error().startswith("evolve: null argument"), kw
    for kw in (dict(steps=0), dict(steps=-1), dict(maxdim=0), dict(maxdim=-3), dict(substeps=0)):
        assert call(**kw) == QIL_EINVAL_ARG and "steps, maxdim and substeps must be >= 1" in L.last_error()
    for kw in (dict(krylov=1), dict(krylov=17), dict(krylov=-2)):
        assert call(**kw) == QIL_EINVAL_ARG and "krylov must be in 2 .. 16" in L.last_error()
    for kw in (dict(tau_re=np.inf), dict(tau_im=np.nan), dict(cutoff=np.nan), dict(tol=np.inf), dict(tol=np.nan)):
        assert call(**kw) == QIL_EINVAL_ARG and "must be finite" in L.last_error()
    for kw in (dict(cutoff=-1e-30), dict(tol=0.0), dict(tol=-1.0)):
        assert call(**kw) == QIL_EINVAL_ARG and "cutoff must be >= 0 and tol > 0" in L.last_error()
    assert call(tau_re=0.0, tau_im=0.0) == QIL_EINVAL_ARG and "tau must not be zero" in L.last_error()
    assert call(steps=0, krylov=1, tol=0.0) == QIL_EINVAL_ARG and "steps, maxdim" in L.last_error()      # the first in the order wins
    assert call() == QIL_EINVAL_LENGTH and "needs a bond" in L.last_error()       # a chain of no tensors has no bond either
    assert out.value == 12345
    src = _read("qilaplace.jl_amd", "csrc", "qil_evolve.hip")
    body = re.search(r'extern "C" int qil_mps_evolve\(.*?\n}\n', src, flags=re.S).group(0)
    act = body.find("qil_ctx_activate")
    order = [body.find(s) for s in ("evolve: null argument", "substeps must be >= 1", "krylov must be in", "must be finite",
                                    "cutoff must be >= 0 and tol > 0", "tau must not be zero", "qil_check_apply_operands(A, x0)",
                                    "QIL_EINVAL_LENGTH")]
    assert all(o >= 0 for o in order) and order == sorted(order) and order[-1] < act, order
    assert body.count("qil_ctx_activate") == 1 and "qil_call_scope" in body[act:] and "qil_scratch tmp(ctx)" in body[act:]
    assert body.index("*out = ") > body.index("ev.step()") and "QIL_EDOMAIN" in body[act:]


def test_the_local_route_is_one_launch_of_one_workgroup_and_the_shared_steps_have_one_home():
    code = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_evolve.hip"))
    solve = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_solve.hip"))
    eigs = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_eigs.hip"))
    shared = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_twosite.h"))
    steps = re.sub(r"//[^\n]*", "", _read("qilaplace.jl_amd", "csrc", "qil_twosite.hip"))
    assert len(re.findall(r"__global__ __launch_bounds__\(kThreads\) void evolve_local\(", code)) == 1
    launcher = shared[shared.index("int launch_local("):shared.index("struct Work {")]
    for once in ("qil_lds_grant", "hipLaunchKernelGGL(Kernel, dim3(1), dim3(kThreads), lds", "qil_read_back_post(", "qil_read_back_wait("):
        assert launcher.count(once) == 1 and shared.count(once) == 1, once          # the one launcher of the local kernels
    assert code.count("launch_local<evolve_local<") == 1 and code.count("launch_local<") == 1 and code.count("evolve_local<") == 1
    assert "hipLaunchKernelGGL" not in code and "dim3(" not in code             # no launch of its own
    kernel = code[code.index("void evolve_local("):code.index("void evolve_begin(")]
    assert "pass < g.substeps" in kernel and "j < g.krylov" in kernel and "atomic" not in code and "asm" not in code
    assert "while" not in kernel and "while" not in code[code.index("krylov_exp("):code.index("void evolve_local(")]
    assert "h < kMaxHalvings" in code                                       # the halving is a bounded loop
    assert code.count("qil_mps_evolve_local_fits(dt == QIL_C64") == 1        # the verb switches on the exported decision
    assert 'getenv("QIL_EVOLVE_ROUTE")' in code
    # one home: the one-site matvecs, the Lanczos step and the small eigen-solver live in the shared header / in qil_twosite.hip
    assert '#include "qil_twosite.h"' in code
    assert shared.count("void local_matvec1(") == 1 and shared.count("void local_matvec(") == 1
    assert shared.count("void lanczos_step(") == 1 and shared.count("void tridiagonal_eig(") == 1
    for name in ("void local_matvec1(", "void local_matvec(", "void lanczos_step(", "void tridiagonal_eig("):
        assert name not in code + solve + eigs, name
    assert steps.count("int Sweep::gemm_matvec1(") == 1 and "Sweep::gemm_matvec1(" not in code + eigs + solve
    for step in ("Sweep::extend(", "Sweep::gemm_matvec(", "Sweep::split(", "Sweep::init_envs(", "Sweep::two_site("):
        assert steps.count("int " + step) == 1 and step not in code + eigs + solve, step
    for call in ("qil_dev_gemm_batched(", "qil_apply_overlap_env_step(", "qil_dev_svd(", "qil_truncation_rank("):
        assert call not in code, call
    for use in ("local_matvec<TE>(g, Ls, Rs, W0, W1,", "local_matvec1<TE>(g, Ls, Rs, W0,", "gemm_matvec(j, A0, A1,", "gemm_matvec1(j, A0,",
                "lanczos_step<TE>(j, nv, V,", "tridiagonal_eig(m,", "split(k, to_right, y, true)", "init_envs()", "start_chain(",
                "start_gauge("):
        assert use in code, use
    assert "lanczos_step<TE>(j, nv, V," in eigs and "tridiagonal_eig(m," in eigs      # the eigen-solver runs the same functions


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
    for name in ("qil_mps_evolve", "qil_apply_mpo_mpo", "qil_apply", "qil_mps_create", "qil_mpo_compress", "qil_norm"):
        monkeypatch.setattr(L.lib, name, boom)
    psi, zt = _fake(qil.SignalMPS), _fake(qil.ZTMPS)
    W, Wp = _fake(qil.SingleSiteMPO), _fake(qil.PairedSiteMPO)
    for bad in (psi, None, np.zeros((4, 4))):
        with pytest.raises(TypeError, match="^evolve: unsupported operand types"):
            qil.evolve(bad, psi, 1.0)
        with pytest.raises(TypeError, match="^evolve: unsupported operand types"):
            qil.propagate(bad, psi, 1.0)
    with pytest.raises(TypeError, match="^evolve: unsupported operand types"):
        qil.evolve(W, W, 1.0)
    with pytest.raises(TypeError, match="^evolve: PairedSiteMPO acts on ZTMPS"):
        qil.evolve(W, zt, 1.0)
    with pytest.raises(TypeError, match="^evolve: PairedSiteMPO acts on ZTMPS"):
        qil.evolve(Wp, psi, 1.0)
    for t in ("1", None, True, [1.0]):
        with pytest.raises(TypeError, match="^evolve: t must be a real or complex number"):
            qil.evolve(W, psi, t)
    for t in (0, 0.0, 0j, np.inf, complex(np.nan, 1.0)):
        with pytest.raises(ValueError, match="^evolve: t must be finite and not zero"):
            qil.evolve(W, psi, t)
    for kw in (dict(steps=0), dict(steps=1.5), dict(steps=True), dict(krylov=0), dict(substeps=-2)):
        with pytest.raises(ValueError, match="^evolve: .* must be a positive integer"):
            qil.evolve(W, psi, 1.0, **kw)
    with pytest.raises(TypeError, match="^evolve: maxdim must be an integer"):
        qil.evolve(W, psi, 1.0, maxdim=2.5)
    with pytest.raises(TypeError, match="^evolve: propagate needs a real time"):
        qil.propagate(W, psi, 1j)
    for bad in (zt, W, None):
        with pytest.raises(TypeError, match="^evolve: diffuse: unsupported operand types"):
            qil.diffuse(bad, 1.0)
    for kw in (dict(order=0), dict(order=1.5), dict(order=True)):
        with pytest.raises(ValueError, match="^evolve: diffuse: order must be a positive integer"):
            qil.diffuse(psi, 1.0, **kw)
    for t in (0.0, -1.0, np.inf, np.nan, 1j, "1"):
        with pytest.raises(ValueError, match="^evolve: diffuse: t must be a positive real number"):
            qil.diffuse(psi, t)
    with pytest.raises(ValueError, match=r"^evolve: diffuse: .* needs 4097 explicit steps .* call smooth"):
        qil.diffuse(psi, 8194.0)
    with pytest.raises(ValueError, match=r"call smooth"):
        qil.diffuse(psi, 2100.0, order=2)                                   # 4^2 * 2100 / 8 = 4200 steps
    assert boom.calls == 0


def test_julia_shim_and_documents_name_the_entries():
    src = _read("julia", "QILaplaceHIP.jl")
    assert "(:qil_mps_evolve, LIB)" in src and "(:qil_mps_evolve_local_fits, LIB)" in src
    assert re.search(r"function evolve\(A::DeviceMPO, x0::DeviceMPS", src)
    assert re.search(r"export .*\bevolve\b", src, flags=re.S) and re.search(r"export .*\bevolve_local_fits\b", src, flags=re.S)
    integ = _read("INTEGRATION.md")
    assert "`qil_mps_evolve`" in integ and "`qil_mps_evolve_local_fits`" in integ
    readme = " ".join(_read("README.md").split())
    for name in ("evolve", "propagate", "diffuse", "smooth"):
        assert f"`{name}`" in readme, name
    for phrase in ("THE STIFF LIMIT", "the error with a binding maxdim is the projection error and does not fall with the step",
                   "a start narrower than the bonds it grows to costs first order in τ once", "Fourier route"):
        assert phrase in readme, phrase
    design = _read("DESIGN.md")
    for phrase in ("3.26", "qil_mps_evolve", "evolve_local", "LDS layout", "Barrier structure", "sub-step rule", "Why the one-site step",
                   "qil_twosite.h"):
        assert phrase in design, phrase
    example = _read("examples", "propagate.py")
    for name in ("propagate", "diagonal_mpo", "build_laplacian_mpo", "inner", "closed form", "THE STIFF LIMIT"):
        assert name in example, name
    tools = _read("tools", "README.md")
    assert "_evolve_time.py" in tools and "QIL_EVOLVE_ROUTE" in tools
    meas = _read("MEASUREMENTS.md")
    assert "qil_mps_evolve" in meas and "capped8_imag" in meas and os.path.exists(os.path.join(ROOT, "profiles", "r32_evolve_time.jsonl"))
