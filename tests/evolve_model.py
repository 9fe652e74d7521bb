"""A numpy restatement of qil.evolve (qil_mps_evolve) and the case table of its tests.  Not imported by the package.

The model is the algorithm of DESIGN.md ("Time evolution"), written for clarity: two-site TDVP.  Right-orthonormal start (cut to
maxdim where it is wider), the environments of <x|A|x> as in solve_model / eigs_model; one step is a sweep left to right and one
right to left; at bond k the two-site tensor goes through exp(+tau/2 H2) and is split under the project's truncation rule; unless
the bond is the last of its half sweep the centre tensor that moves on goes through exp(-tau/2 H1).  Every local exponential is
`lanczos_exp`: full reorthogonalisation, c = exp(delta T_m) e_1 after every vector from the second on, est = beta_m |c_m| / |c|,
the pass ends at est <= tol, at beta_m <= 1e-14 scale or at m = krylov; there delta is halved (at most 30 times) until est <= tol,
the vector advances by that part and the next pass takes the rest; the last permitted pass takes all that remains.  Norms: every
exponential starts from the unit vector and returns log(|v| g); every split rescales what it kept to norm 1 and returns its log.

The bound of the cases that are exact in exact arithmetic (derived, not fitted), relative to the dense exponential's norm:
    B = G * (N_loc * tol + sqrt(N_loc * cutoff) + 64 * N_loc * eps),   N_loc = steps * (4 n - 6),
    G = exp(|Re t| * (lambda_max - lambda_min))
N_loc local exponentials each wrong by at most tol of a unit vector, N_loc splits (a ceiling: there are steps * (2 n - 2)) each
dropping at most `cutoff` of the squared norm, the rounding floor of N_loc small contractions; G bounds how much any later factor
exp(s A) / |exp(t A) x|, 0 <= s <= t, can amplify an earlier error relative to the result (loose by construction)."""
import numpy as np

import solve_model as SM
import eigs_model as EM
from solve_model import EPS, dense_mps, dense_op, truncation_rank, gram_tensors, random_operator, random_state, capped, scaled, \
    identity_tensors, coefficient_rows, mpo_sum, laplacian_tensors, tt_svd, _right_orthonormal, _truncate_to
from eigs_model import _ext_left, _ext_right, field_tensors, field_coefficients, BREAKDOWN

MAX_HALVINGS = 30


def lanczos_exp(H, y, delta, tol, krylov, substeps):
    """y -> (the unit vector along exp(delta H) y, log(|y| g), stats).  H acts on arrays of y's shape."""
    shape = y.shape
    v0 = y.reshape(-1)
    nrm = np.linalg.norm(v0)
    if not (nrm > 0 and np.isfinite(nrm)):
        raise ArithmeticError("evolve: the start is zero or not finite")
    v0 = v0 / nrm
    rem = complex(delta)
    real = rem.imag == 0.0 and not np.iscomplexobj(v0)
    st = dict(matvecs=0, passes=0, est=0.0, conv=True, spread=0.0, log=float(np.log(nrm)), halved=False)
    scale, fin = 0.0, False
    for p in range(substeps):
        st["passes"] += 1
        V, al, be = [v0], [], []
        for j in range(krylov):
            w = H(V[j].reshape(shape)).reshape(-1)
            st["matvecs"] += 1
            a = 0.0
            for _ in range(2):
                for i in range(j + 1):
                    c = np.vdot(V[i], w)
                    w = w - c * V[i]
                    if i == j:
                        a += c.real
            b = float(np.linalg.norm(w))
            if not (np.isfinite(a) and np.isfinite(b)):
                raise ArithmeticError("evolve: a Lanczos coefficient is not finite")
            al.append(a)
            be.append(b)
            scale = max(scale, abs(a), b)
            m = j + 1
            invariant = b <= BREAKDOWN * scale
            if m == 1 and not invariant:
                V.append(w / b)
                continue
            T = np.diag(al) + np.diag(be[:m - 1], 1) + np.diag(be[:m - 1], -1)
            ev, Z = np.linalg.eigh(T)

            def coef(d):
                c = Z @ (np.exp((d.real if real else d) * ev) * Z[0])
                return c, b * abs(c[-1]) / np.linalg.norm(c)

            c, est = coef(rem)
            if invariant:
                est = 0.0
            part, everything, conv = rem, True, True
            if est > tol:
                if m < krylov:
                    V.append(w / b)
                    continue
                if p + 1 == substeps:
                    conv = False
                else:
                    f = 1.0
                    for _ in range(MAX_HALVINGS):
                        if est <= tol:
                            break
                        f *= 0.5
                        c, est = coef(rem * f)
                    part, everything, conv = rem * f, False, est <= tol
                    st["halved"] = True
            w = sum(c[i] * V[i] for i in range(m))
            g = float(np.linalg.norm(w))
            v0 = w / g
            st["log"] += float(np.log(g))
            st["est"] = max(st["est"], float(est))
            st["spread"] = max(st["spread"], float(ev[-1] - ev[0]))
            st["conv"] = st["conv"] and conv
            if everything:
                fin = True
            else:
                rem = rem - part
            break
        if fin:
            break
    return v0.reshape(shape), st["log"], st


def model_evolve(A, x0, tau, steps=1, maxdim=64, cutoff=1e-20, tol=1e-10, krylov=8, substeps=4, dense_local=False):
    """One call of the verb.  Returns (x tensors of norm 1, log of the norm factor, info dict).  dense_local=True takes every local
    exponential by a dense eigh of the local operator instead of Lanczos (the check of the check)."""
    n = len(x0)
    assert n >= 2
    tau = complex(tau)
    cx = tau.imag != 0.0 or any(np.iscomplexobj(t) for t in list(A) + list(x0))
    dt = np.complex128 if cx else np.float64
    A = [np.asarray(t, dtype=dt) for t in A]
    x = [np.asarray(t, dtype=dt) for t in x0]
    x = _truncate_to(x, maxdim) if max(t.shape[2] for t in x) > maxdim else _right_orthonormal(x)
    one3 = np.ones((1, 1, 1), dtype=dt)
    LA, RA = [None] * (n + 1), [None] * (n + 1)
    LA[0], RA[n] = one3, one3
    for j in range(n - 1, 1, -1):
        RA[j] = _ext_right(RA[j + 1], x[j], A[j])
    info = dict(matvecs=0, converged=True, estimate=0.0, substeps=0, backward_growth=0.0, local=0, halved=False)
    log_sum = 0.0

    def local(H, y, delta, one_site):
        nonlocal log_sum
        if dense_local:
            nv = y.size
            M = np.stack([H(e.reshape(y.shape)).reshape(-1) for e in np.eye(nv, dtype=dt)], axis=1)
            ev, Z = np.linalg.eigh(0.5 * (M + M.conj().T))
            w = Z @ (np.exp((delta.real if not cx else delta) * ev) * (Z.conj().T @ y.reshape(-1)))
            nr = np.linalg.norm(w)
            log_sum += float(np.log(nr))
            info["local"] += 1
            return (w / nr).reshape(y.shape)
        v, lg, st = lanczos_exp(H, y, delta, tol, krylov, substeps)
        log_sum += lg
        info["matvecs"] += st["matvecs"]
        info["converged"] = info["converged"] and st["conv"]
        info["estimate"] = max(info["estimate"], st["est"])
        info["substeps"] += st["passes"] - 1
        info["halved"] = info["halved"] or st["halved"]
        info["local"] += 1
        if one_site:
            info["backward_growth"] = max(info["backward_growth"], 0.5 * abs(tau.real) * st["spread"])
        return v

    def bond(k, to_right):
        nonlocal log_sum
        L, R = LA[k], RA[k + 2]

        def H2(v):
            T = np.tensordot(L, v, axes=([2], [0]))                        # p a x z l
            T = np.tensordot(T, A[k], axes=([1, 2], [0, 1]))               # p z l y m
            T = np.tensordot(T, A[k + 1], axes=([4, 1], [0, 1]))           # p l y w b
            return np.tensordot(T, R, axes=([4, 1], [1, 2]))               # p y w q

        y = local(H2, np.einsum("kxm,mzl->kxzl", x[k], x[k + 1]), 0.5 * tau, False)
        xl, xr = y.shape[0], y.shape[3]
        U, S, Vh = np.linalg.svd(y.reshape(2 * xl, 2 * xr), full_matrices=False)
        kk = truncation_rank(S, cutoff, maxdim)
        kept = float(np.sqrt(np.sum(S[:kk] ** 2)))
        log_sum += float(np.log(kept))
        S = S[:kk] / kept
        if to_right:
            x[k], x[k + 1] = U[:, :kk].reshape(xl, 2, kk), (S[:, None] * Vh[:kk]).reshape(kk, 2, xr)
        else:
            x[k], x[k + 1] = (U[:, :kk] * S).reshape(xl, 2, kk), Vh[:kk].reshape(kk, 2, xr)

    def site(j):
        L, R = LA[j], RA[j + 1]

        def H1(v):
            T = np.tensordot(L, v, axes=([2], [0]))                        # p a x l
            T = np.tensordot(T, A[j], axes=([1, 2], [0, 1]))               # p l y b
            return np.tensordot(T, R, axes=([3, 1], [1, 2]))               # p y q

        x[j] = local(H1, x[j], -0.5 * tau, True)

    for _ in range(steps):
        for k in range(n - 1):
            bond(k, True)
            if k + 2 < n:
                LA[k + 1] = _ext_left(LA[k], x[k], A[k])
                site(k + 1)
        for k in range(n - 2, -1, -1):
            bond(k, False)
            if k >= 1:
                RA[k + 1] = _ext_right(RA[k + 2], x[k + 1], A[k + 1])
                site(k)
    info["max_bond"] = max(t.shape[2] for t in x)
    info["log_norm"] = log_sum
    return x, log_sum, info


# ---------------------------------------------------------------- the cases
EVOLVE_DEFAULTS = dict(steps=1, maxdim=64, cutoff=1e-24, tol=1e-10, krylov=8, substeps=4)


def n_local(n, steps):
    return steps * (4 * n - 6)


def diag_tensors(v):
    """diag(v) for a state v: W[a, i, o, b] = delta_io v[a, i, b]"""
    out = []
    for t in v:
        W = np.zeros((t.shape[0], 2, 2, t.shape[2]), dtype=t.dtype)
        W[:, 0, 0, :], W[:, 1, 1, :] = t[:, 0, :], t[:, 1, :]
        out.append(W)
    return out


def _normalised(A):
    return scaled(A, 1.0 / float(np.linalg.norm(dense_op(A), 2)))


def _identity_case(n, t):
    rng = np.random.default_rng(100 + n)
    return dict(A=identity_tensors(n), x0=random_state(capped(n, 2), rng, False), x0_amp=0.5, t=t, kind="identity", kwargs=dict(steps=2))


def _sat6(a_complex, tau, seed=606, paired=False, **kw):
    """a normalised Gram operator (bond 4) on a start at the full bonds 2, 4, 8, 4, 2: every projector is the identity"""
    rng = np.random.default_rng(seed)
    A = _normalised(gram_tensors(random_operator([2] * 5, rng, a_complex)))
    return dict(A=A, x0=random_state(capped(6, 8), rng, a_complex), x0_amp=1.25, t=2 * tau, kind="exact", paired=paired,
                kwargs=dict(steps=2, maxdim=8, **kw))


def _gram2():
    rng = np.random.default_rng(302)
    A = _normalised(gram_tensors(random_operator([3], rng, False)))
    return dict(A=A, x0=random_state([2], rng, False), t=-2.0, kind="exact", kwargs=dict(steps=2))


def _straddle(complex_):
    """G of bond 5 (operator bond 25) at n = 8 on a start at the full bonds 2, 4, 8, 16, 8, 4, 2: the steps next to the ends fit the
    one-launch route, the middle ones do not (tests read the decision through evolve_local_fits)."""
    rng = np.random.default_rng(811 + int(complex_))
    A = _normalised(gram_tensors(random_operator([5] * 7, rng, complex_)))
    return dict(A=A, x0=random_state(capped(8, 16), rng, complex_), t=(-0.5 + 2j) if complex_ else -1.0, kind="exact",
                kwargs=dict(steps=1, maxdim=16))


FIELD_N = 40


def _field40(t):
    rng = np.random.default_rng(4040)
    cx = complex(t).imag != 0.0
    return dict(A=field_tensors(FIELD_N), x0=random_state([1] * (FIELD_N - 1), rng, cx), t=t, kind="field40", kwargs=dict(steps=2))


def field40_closed_form(name):
    """(the n evolved site vectors exp(t h_j) x_j, log of the product of their norms)"""
    d = case(name)
    a, b = field_coefficients(FIELD_N)
    out, lg = [], 0.0
    for j in range(FIELD_N):
        h = np.array([[b[j], a[j]], [a[j], -b[j]]])
        ev, Z = np.linalg.eigh(h)
        v = Z @ (np.exp(d["t"] * ev) * (Z.T @ d["x0"][j][0, :, 0]))
        out.append(v)
        lg += float(np.log(np.linalg.norm(v)))
    return out, lg


MODE_N, MODE_F = 40, int(round(0.3 * 2 ** 40))


def mode40_lambda():
    """lambda = 2 - 2 cos(2 pi f / N) of the periodic Laplacian at the mode f"""
    return 2.0 - 2.0 * np.cos(2.0 * np.pi * (MODE_F / 2.0 ** MODE_N))


def _mode40(t):
    from qilaplace_jl_amd.ops import exponential_tensors
    z = np.exp(2j * np.pi * (MODE_F / 2.0 ** MODE_N))
    return dict(A=laplacian_tensors(MODE_N), x0=exponential_tensors(z, MODE_N), t=t, kind="mode40", kwargs=dict(steps=2))


def capped8_operator():
    n = 8
    s = (np.arange(2 ** n) + 0.5) / 2 ** n
    V = tt_svd(0.5 * np.cos(2 * np.pi * s) + 0.25 * np.cos(6 * np.pi * s), n, 1e-28)
    return mpo_sum(laplacian_tensors(n), diag_tensors(V))


def _capped8(t, steps, cx):
    n = 8
    s = (np.arange(2 ** n) + 0.5) / 2 ** n
    carrier = np.exp(2j * np.pi * 12 * s) if cx else np.cos(2 * np.pi * 12 * s)
    pulses = np.exp(-((s - 0.3) / 0.05) ** 2) * carrier + 0.7 * np.exp(-((s - 0.72) / 0.03) ** 2)
    return dict(A=capped8_operator(), x0=tt_svd(pulses, n, 1e-28), t=t, kind="capped", kwargs=dict(steps=steps, maxdim=6))


CASE_BUILDERS = {
    "identity2": lambda: _identity_case(2, -0.7),
    "identity3": lambda: _identity_case(3, 0.5 + 1.1j),
    "identity5": lambda: _identity_case(5, 1.2j),
    "sat6_f64": lambda: _sat6(False, -1.5),
    "sat6_c64_a": lambda: _sat6(True, -1.5),
    "sat6_c64_b": lambda: _sat6(True, 1.0),
    "sat6_c64_c": lambda: _sat6(True, -0.5 + 2j),
    "sat6_imag": lambda: _sat6(True, 3j, krylov=8, substeps=4),
    "sat3_paired": lambda: _sat6(True, -0.5 + 2j, seed=609, paired=True),
    "gram2": _gram2,
    "straddle8_f64": lambda: _straddle(False),
    "straddle8_c64": lambda: _straddle(True),
    "field40_real": lambda: _field40(-0.4),
    "field40_imag": lambda: _field40(1.5j),
    "mode40_real": lambda: _mode40(-0.8),
    "mode40_imag": lambda: _mode40(2.5j),
    "capped8_imag": lambda: _capped8(6j, 3, True),
    "capped8_real": lambda: _capped8(-4.0, 4, False),
}
IDENTITY_CASES = ["identity2", "identity3", "identity5"]
EXACT_CASES = [k for k in CASE_BUILDERS if k.startswith(("sat", "gram2", "straddle"))]
STRADDLE_CASES = ["straddle8_f64", "straddle8_c64"]
FIELD40_CASES = ["field40_real", "field40_imag"]
MODE40_CASES = ["mode40_real", "mode40_imag"]
CAPPED_CASES = ["capped8_imag", "capped8_real"]
DENSE_CASES = IDENTITY_CASES + EXACT_CASES + CAPPED_CASES

_BUILT, _REF, _MODEL = {}, {}, {}


def case(name):
    if name not in _BUILT:
        d = CASE_BUILDERS[name]()
        d.setdefault("x0_amp", 1.0)
        d.setdefault("paired", False)
        kw = dict(EVOLVE_DEFAULTS)
        kw.update(d.get("kwargs", {}))
        d["kwargs"] = kw
        d["n"] = len(d["A"])
        d["n_local"] = n_local(d["n"], kw["steps"])
        _BUILT[name] = d
    return _BUILT[name]


def is_complex(name):
    d = case(name)
    return complex(d["t"]).imag != 0.0 or any(np.iscomplexobj(t) for t in d["A"] + d["x0"])


def reference(name):
    """(exp(t A) x0 dense, for x0's TENSORS; the eigenvalues of A) from numpy's eigh; computed once"""
    if name not in _REF:
        d = case(name)
        M = dense_op(d["A"])
        assert np.allclose(M, M.conj().T, atol=1e-12 * np.abs(M).max())
        ev, Z = np.linalg.eigh(M)
        _REF[name] = (Z @ (np.exp(d["t"] * ev) * (Z.conj().T @ dense_mps(d["x0"]))), ev)
    return _REF[name]


def bound(name):
    d = case(name)
    kw, N = d["kwargs"], d["n_local"]
    ev = reference(name)[1]
    G = float(np.exp(abs(complex(d["t"]).real) * (ev[-1] - ev[0])))
    return G * (N * kw["tol"] + np.sqrt(N * kw["cutoff"]) + 64 * N * EPS)


def rel_error(v, name):
    ref = reference(name)[0]
    return float(np.linalg.norm(v - ref) / np.linalg.norm(ref))


def model(name, **over):
    """(dense result with the norm factor, info) of the restatement; the plain call is computed once"""
    if over:
        d = case(name)
        kw = dict(d["kwargs"], **over)
        x, lg, info = model_evolve(d["A"], d["x0"], complex(d["t"]) / kw["steps"], **kw)
        return dense_mps(x) * np.exp(lg), info
    if name not in _MODEL:
        d = case(name)
        kw = d["kwargs"]
        x, lg, info = model_evolve(d["A"], d["x0"], complex(d["t"]) / kw["steps"], **kw)
        _MODEL[name] = (dense_mps(x) * np.exp(lg), info)
    return _MODEL[name]


def rows40(count=200, seed=4242):
    return np.random.default_rng(seed).integers(0, 2, size=(count, 40)).astype(np.uint8)
