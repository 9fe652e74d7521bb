"""A numpy restatement of qil.eigs (qil_mps_eigs) and the case table of its tests.  Not imported by the package.

The model is the algorithm of DESIGN.md ("Extremal eigenpairs"), written for clarity, on the helpers of tests/solve_model.py:
right-orthonormal unit start, environments L_A / R_A of <x|A|x> and Lp / Rp of <x|phi_i> for the deflation states, per bond the
local operator
    H v = L_A A_k A_{k+1} R_A v + s weight sum_i g_i (g_i^H v),   g_i = Lp_i phi_i,k phi_i,k+1 Rp_i,   s = +1 smallest / -1 largest,
restarted Lanczos with full reorthogonalisation (two modified Gram-Schmidt passes, at most `krylov` vectors, at most `restarts`
restarts) from the current two-site tensor, the stopping test |H y - theta y| <= tol * scale with scale the largest |Ritz value|
seen (with deflation states: at the wanted end only), the breakdown test beta <= 1e-14 * scale, the SVD split under the project's
truncation rule with the kept values rescaled to norm 1, a full sweep = left to right then right to left, and the stopping rule
on the largest pre-solve |r| / scale.

The bounds of every dense case (maxdim >= the full bond, so the middle local space is the whole space), with |A| and the gap
from numpy's eigvalsh and v the normalised dense result (derived, not fitted):
    B = tol + sqrt((n - 1) * cutoff) + 64 * n * eps                        (solve's form with kappa = 1)
    rho = |A v - theta v| / |A| <= B
    |theta - lambda_ref| / |A| <= B                                        (lambda_ref the j-th value from the wanted end: extremality)
    |v - z <z|v>| <= 2 * B * |A| / gap                                     (Davis-Kahan, factor 2 for rounding-level residuals)
tol: the local solves stop on the residual relative to scale <= |A|; sqrt((n - 1) * cutoff): the n - 1 truncations of the last
half-sweep; 64 * n * eps: the rounding floor of n tensor updates in double precision."""
import numpy as np

import solve_model as SM
from solve_model import EPS, dense_mps, dense_op, truncation_rank, gram_tensors, random_operator, random_state, capped, scaled, \
    identity_tensors, coefficient_rows, _right_orthonormal, _truncate_to

BREAKDOWN = 1e-14


def _ext_left(E, x, A):
    return np.einsum("pak,kxb,axyc,pyq->qcb", E, x, A, x.conj(), optimize=True)


def _ext_right(E, x, A):
    return np.einsum("qcb,kxb,axyc,pyq->pak", E, x, A, x.conj(), optimize=True)


def _ov_left(E, x, c):
    return np.einsum("pk,kxb,pxq->qb", E, c, x.conj(), optimize=True)


def _ov_right(E, x, c):
    return np.einsum("qb,kxb,pxq->pk", E, c, x.conj(), optimize=True)


def lanczos_local(H, y, which, tol, scale, krylov, restarts, wanted_only):
    """The local solver.  Returns (y, theta, res0, scale, matvecs)."""
    shape = y.shape
    v0 = y.reshape(-1)
    nrm = np.linalg.norm(v0)
    if not (nrm > 0 and np.isfinite(nrm)):
        raise ArithmeticError("eigs: the start vector is zero or not finite")
    v0 = v0 / nrm
    theta, res0, matvecs = 0.0, 0.0, 0
    for rs in range(restarts):
        V, al, be, done = [v0], [], [], False
        for j in range(krylov):
            w = H(V[j].reshape(shape)).reshape(-1)
            matvecs += 1
            a = 0.0
            for _ in range(2):
                for i in range(j + 1):
                    c = np.vdot(V[i], w)
                    w = w - c * V[i]
                    if i == j:
                        a += c.real
            b = float(np.linalg.norm(w))
            if not (np.isfinite(a) and np.isfinite(b)):
                raise ArithmeticError("eigs: a Ritz value is not finite")
            al.append(a)
            be.append(b)
            if j == 0:
                theta = a
                scale = max(scale, abs(a))
                if rs == 0:
                    res0 = b
                if b <= tol * scale:
                    done = True
                    break
            if b <= BREAKDOWN * scale:
                break
            if j + 1 < krylov:
                V.append(w / b)
        if done:
            break
        m = len(al)
        T = np.diag(al) + np.diag(be[:m - 1], 1) + np.diag(be[:m - 1], -1)
        ev, Z = np.linalg.eigh(T)
        pick = m - 1 if which else 0
        theta = float(ev[pick])
        scale = max(scale, abs(theta) if wanted_only else float(np.abs(ev).max()))
        w = sum(Z[i, pick] * V[i] for i in range(m))
        v0 = w / np.linalg.norm(w)
    return v0.reshape(shape), theta, res0, scale, matvecs


def model_eigs(A, which, x0, ortho=(), weight=0.0, maxdim=64, cutoff=1e-20, tol=1e-10, max_sweeps=10, krylov=8, restarts=4):
    """One call of the verb.  which: 0 smallest, 1 largest.  Returns (x tensors, theta, info dict)."""
    n = len(x0)
    assert n >= 2
    cx = any(np.iscomplexobj(t) for t in list(A) + list(x0) + [t for p in ortho for t in p])
    dt = np.complex128 if cx else np.float64
    A = [np.asarray(t, dtype=dt) for t in A]
    phis = [[np.asarray(t, dtype=dt) for t in p] for p in ortho]
    x = [np.asarray(t, dtype=dt) for t in x0]
    x = _truncate_to(x, maxdim) if max(t.shape[2] for t in x) > maxdim else _right_orthonormal(x)
    one3, one2 = np.ones((1, 1, 1), dtype=dt), np.ones((1, 1), dtype=dt)
    LA, RA = [None] * (n + 1), [None] * (n + 1)
    Lp = [[None] * (n + 1) for _ in phis]
    Rp = [[None] * (n + 1) for _ in phis]
    LA[0], RA[n] = one3, one3
    for i in range(len(phis)):
        Lp[i][0], Rp[i][n] = one2, one2
    for j in range(n - 1, 1, -1):
        RA[j] = _ext_right(RA[j + 1], x[j], A[j])
        for i, p in enumerate(phis):
            Rp[i][j] = _ov_right(Rp[i][j + 1], x[j], p[j])
    sw = (1.0 if which == 0 else -1.0) * weight
    state = {"scale": 0.0, "theta": 0.0, "matvecs": 0}

    def step(k, to_right):
        L, R = LA[k], RA[k + 2]
        gs = [np.einsum("pk,kxm,mzl,ql->pxzq", Lp[i][k], p[k], p[k + 1], Rp[i][k + 2], optimize=True) for i, p in enumerate(phis)]

        def H(v):
            T = np.tensordot(L, v, axes=([2], [0]))                        # p a x z l
            T = np.tensordot(T, A[k], axes=([1, 2], [0, 1]))               # p z l y m
            T = np.tensordot(T, A[k + 1], axes=([4, 1], [0, 1]))           # p l y w b
            out = np.tensordot(T, R, axes=([4, 1], [1, 2]))                # p y w q
            for g in gs:
                out = out + sw * np.vdot(g, v) * g
            return out

        y = np.einsum("kxm,mzl->kxzl", x[k], x[k + 1])
        y, theta, res0, scale, mv = lanczos_local(H, y, which, tol, state["scale"], krylov, restarts, bool(phis))
        state.update(scale=scale, theta=theta, matvecs=state["matvecs"] + mv)
        xl, xr = y.shape[0], y.shape[3]
        U, S, Vh = np.linalg.svd(y.reshape(2 * xl, 2 * xr), full_matrices=False)
        kk = truncation_rank(S, cutoff, maxdim)
        S = S[:kk] / np.linalg.norm(S[:kk])
        if to_right:
            x[k], x[k + 1] = U[:, :kk].reshape(xl, 2, kk), (S[:, None] * Vh[:kk]).reshape(kk, 2, xr)
        else:
            x[k], x[k + 1] = (U[:, :kk] * S).reshape(xl, 2, kk), Vh[:kk].reshape(kk, 2, xr)
        return res0 / scale if scale > 0 else (np.inf if res0 > 0 else 0.0)

    info = {"sweeps": 0, "converged": False, "residual": np.inf}
    for sweep in range(max_sweeps):
        worst = 0.0
        for k in range(n - 1):
            worst = max(worst, step(k, True))
            if k + 2 < n:
                LA[k + 1] = _ext_left(LA[k], x[k], A[k])
                for i, p in enumerate(phis):
                    Lp[i][k + 1] = _ov_left(Lp[i][k], x[k], p[k])
        for k in range(n - 2, -1, -1):
            worst = max(worst, step(k, False))
            if k >= 1:
                RA[k + 1] = _ext_right(RA[k + 2], x[k + 1], A[k + 1])
                for i, p in enumerate(phis):
                    Rp[i][k + 1] = _ov_right(Rp[i][k + 2], x[k + 1], p[k + 1])
        info.update(sweeps=sweep + 1, residual=worst)
        if worst <= tol:
            info["converged"] = True
            break
    info.update(matvecs=state["matvecs"], max_bond=max(t.shape[2] for t in x), scale=state["scale"])
    return x, state["theta"], info


def random_start(A, rng):
    """The draw of qil.eigs for x0=None: a bond-2 state, complex when A is."""
    n = len(A)
    cx = any(np.iscomplexobj(t) for t in A)
    dims = [1] + [2] * (n - 1) + [1]
    out = []
    for i in range(n):
        shp = (dims[i], 2, dims[i + 1])
        t = rng.standard_normal(shp)
        if cx:
            t = t + 1j * rng.standard_normal(shp)
        out.append(t / np.sqrt(2.0 * dims[i]))
    return out


def model_eigs_k(A, k, which, x0=None, seed=0, weight=None, ortho=(), **kw):
    """The k calls of qil.eigs: (values, list of tensor lists, infos).  With deflation states and no weight, scale comes from one
    undeflated probe sweep of one restart per bond before the first call, as in qil.eigs."""
    rng = np.random.default_rng(seed)
    found, states, values, infos = list(ortho), [], [], []
    w = weight
    for j in range(k):
        start = x0 if (j == 0 and x0 is not None) else random_start(A, rng)
        if w is None and found:
            w = 2.0 * model_eigs(A, which, start, **dict(kw, max_sweeps=1, restarts=1))[2]["scale"]
        x, theta, info = model_eigs(A, which, start, ortho=found, weight=0.0 if w is None else w, **kw)
        if w is None:
            w = 2.0 * info["scale"]
        found.append(x)
        states.append(x)
        values.append(theta)
        infos.append(info)
    return np.array(values), states, infos


# ---------------------------------------------------------------- the cases
EIGS_DEFAULTS = dict(maxdim=64, cutoff=1e-24, tol=1e-10, max_sweeps=10, krylov=8, restarts=4)

FIELD_SEED = 5150


def field_coefficients(n):
    rng = np.random.default_rng(FIELD_SEED + n)
    return rng.uniform(0.3, 1.0, n), rng.uniform(-1.0, 1.0, n)


def field_tensors(n):
    """A = sum_j (a_j sigma_x + b_j sigma_z) as a bond-2 operator."""
    a, b = field_coefficients(n)
    I2 = np.eye(2)
    out = []
    for j in range(n):
        h = np.array([[b[j], a[j]], [a[j], -b[j]]])
        if j == 0:
            W = np.zeros((1, 2, 2, 2))
            W[0, :, :, 0], W[0, :, :, 1] = h, I2
        elif j == n - 1:
            W = np.zeros((2, 2, 2, 1))
            W[0, :, :, 0], W[1, :, :, 0] = I2, h
        else:
            W = np.zeros((2, 2, 2, 2))
            W[0, :, :, 0], W[1, :, :, 0], W[1, :, :, 1] = I2, h, I2
        out.append(W)
    return out


def field_closed_form(n, which):
    """(lambda, gap, the n site vectors of the product eigenvector) at the wanted end"""
    a, b = field_coefficients(n)
    r = np.hypot(a, b)
    sgn = 1.0 if which else -1.0
    vecs = np.stack([a, sgn * r - b], axis=1)
    vecs = vecs / np.linalg.norm(vecs, axis=1, keepdims=True)
    return sgn * float(r.sum()), 2.0 * float(r.min()), vecs


def field_rows(n, count=200, seed=4141):
    return np.random.default_rng(seed).integers(0, 2, size=(count, n)).astype(np.uint8)


def _identity_case(n):
    rng = np.random.default_rng(100 + n)
    return dict(A=identity_tensors(n), x0=random_state(capped(n, 2), rng, False), x0_amp=0.5, which="smallest", k=1, kind="identity")


def _gram(bonds, a_complex, seed, which="largest", k=3, negate=False, x0_complex=None, paired=False, **kw):
    rng = np.random.default_rng(seed)
    A = gram_tensors(random_operator(list(bonds), rng, a_complex))
    if negate:
        A = scaled(A, -1.0)
    d = dict(A=A, which=which, k=k, kind="dense", paired=paired, kwargs=kw)
    if x0_complex is not None:
        d["x0"] = random_state([2] * len(bonds), rng, x0_complex)
    return d


def _straddle(complex_, **kw):
    """G of bond 5 (operator bond 25) at n = 8: x reaches the full bonds 2, 4, 8, 16, 8, 4, 2, the bonds next to the ends fit the
    one-launch route, the middle ones do not (tests read the decision through eigs_local_fits)."""
    rng = np.random.default_rng(811 + int(complex_))
    return dict(A=gram_tensors(random_operator([5] * 7, rng, complex_)), which="largest", k=2, kind="dense", kwargs=kw)


def _capped8():
    d = _straddle(False, maxdim=6)
    d.update(k=1, kind="conditions")
    return d


def _field(n, which):
    return dict(A=field_tensors(n), which=which, k=1, kind="dense" if n <= 10 else "field40")


CASE_BUILDERS = {
    "identity2": lambda: _identity_case(2),
    "identity3": lambda: _identity_case(3),
    "identity5": lambda: _identity_case(5),
    "gram2": lambda: _gram([3], False, 302, k=2),
    "gram3_c64": lambda: _gram([2, 2], True, 303, k=2),
    "gram6_f64": lambda: _gram([2] * 5, False, 307),
    "gram6_c64": lambda: _gram([2] * 5, True, 306),
    "neg_gram6_f64": lambda: _gram([2] * 5, False, 307, which="smallest", negate=True),
    "neg_gram6_c64": lambda: _gram([2] * 5, True, 306, which="smallest", negate=True),
    "gram6_rc": lambda: _gram([2] * 5, False, 307, k=1, x0_complex=True),
    "paired3": lambda: _gram([2] * 5, True, 309, k=2, paired=True),
    "straddle8_f64": lambda: _straddle(False),
    "straddle8_c64": lambda: _straddle(True),
    "krylov2": lambda: _straddle(True, krylov=2, restarts=16),
    "field10_min": lambda: _field(10, "smallest"),
    "field10_max": lambda: _field(10, "largest"),
    "field40_min": lambda: _field(40, "smallest"),
    "field40_max": lambda: _field(40, "largest"),
    "capped8": _capped8,
}
DENSE_CASES = [k for k in CASE_BUILDERS if not k.startswith(("field40", "capped", "identity"))]
IDENTITY_CASES = ["identity2", "identity3", "identity5"]
FIELD40_CASES = ["field40_min", "field40_max"]
WHICH = {"smallest": 0, "largest": 1}

_BUILT, _REF, _MODEL = {}, {}, {}


def case(name):
    if name not in _BUILT:
        d = CASE_BUILDERS[name]()
        d.setdefault("x0", None)
        d.setdefault("x0_amp", 1.0)
        d.setdefault("paired", False)
        d.setdefault("seed", 7)
        kw = dict(EIGS_DEFAULTS)
        kw.update(d.get("kwargs", {}))
        d["kwargs"] = kw
        d["n"] = len(d["A"])
        _BUILT[name] = d
    return _BUILT[name]


def is_complex(name):
    d = case(name)
    return any(np.iscomplexobj(t) for t in d["A"] + (d["x0"] or []))


def reference(name):
    """(eigenvalues ascending, eigenvectors, |A|) of the dense operator, computed once"""
    if name not in _REF:
        M = dense_op(case(name)["A"])
        assert np.allclose(M, M.conj().T, atol=1e-12 * np.abs(M).max())
        ev, Z = np.linalg.eigh(M)
        _REF[name] = (ev, Z, float(np.abs(ev).max()))
    return _REF[name]


def wanted(name, j):
    """(lambda_ref, eigenvector, gap to its nearest neighbour) of the j-th value from the wanted end"""
    ev, Z, _ = reference(name)
    idx = j if case(name)["which"] == "smallest" else len(ev) - 1 - j
    gap = min(abs(ev[idx] - ev[i]) for i in (idx - 1, idx + 1) if 0 <= i < len(ev))
    return float(ev[idx]), Z[:, idx], float(gap)


def bound(name):
    d = case(name)
    kw = d["kwargs"]
    return kw["tol"] + np.sqrt((d["n"] - 1) * kw["cutoff"]) + 64 * d["n"] * EPS


def dense_checks(name, j, theta, v):
    """The three figures of a dense case for the j-th result (v: the dense vector) against their bounds: a list of
    (label, value, bound)."""
    M = dense_op(case(name)["A"])
    _, _, nrmA = reference(name)
    lam, z, gap = wanted(name, j)
    v = v / np.linalg.norm(v)
    B = bound(name)
    rho = float(np.linalg.norm(M @ v - theta * v) / nrmA)
    angle = float(np.linalg.norm(v - z * np.vdot(z, v)))
    return [("residual", rho, B), ("value", abs(theta - lam) / nrmA, B), ("vector", angle, 2 * B * nrmA / gap)]


def model(name):
    """The restatement's (values, states, infos) of a case, computed once"""
    if name not in _MODEL:
        d = case(name)
        _MODEL[name] = model_eigs_k(d["A"], d["k"], WHICH[d["which"]], x0=d["x0"], seed=d["seed"], **d["kwargs"])
    return _MODEL[name]
