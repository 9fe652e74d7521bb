"""numpy model of the cross-interpolation encoder (qil_signal_mps_cross): the yardstick of tests/test_cross_model.py and
tests/test_gpu_cross.py.

Sample j < 2^n has the bits b_1 .. b_n, site 1 the most significant.  For every bond l there is a list I_l of prefixes and a
list J_l of suffixes; I_0 = J_n = {empty}, J_l starts as the unique suffixes of the seeds.  A step at bond l evaluates the block
x(I_{l-1} x {0,1} x {0,1} x J_{l+1}) and factors it by LU with full pivoting (ties: the lowest column-major position).  Pivots
stop at rank maxdim and, after the first one, when the largest remaining |entry| <= tol fmax, fmax the largest |x| sampled so
far; an all-zero block still takes one pivot.  Sweeps run l = 1 .. n-1 and back until every estimate of a whole
back-and-forth sweep is <= tol fmax; a final forward sweep writes site l = L L11^-1 and site n = the pivot rows of the last block."""
import numpy as np


def lu_full(P, tol_abs, maxdim):
    """A (L below the diagonal, U on and above, in pivoted order), row order, column order, rank, largest remaining |entry|."""
    A = np.array(P, copy=True)
    m, k = A.shape
    rows, cols = list(range(m)), list(range(k))
    r, err = 0, 0.0
    while r < min(m, k):
        sub = np.abs(A[r:, r:])
        j, i = divmod(int(np.argmax(sub.T)), sub.shape[0])           # column-major: the lowest position wins a tie
        v = float(sub[i, j])
        if r >= maxdim or (r > 0 and (v <= tol_abs or v == 0.0)):
            err = v
            break
        i += r
        j += r
        A[[r, i], :] = A[[i, r], :]
        rows[r], rows[i] = rows[i], rows[r]
        A[:, [r, j]] = A[:, [j, r]]
        cols[r], cols[j] = cols[j], cols[r]
        if v > 0.0:
            A[r + 1:, r] /= A[r, r]
        A[r + 1:, r + 1:] -= np.outer(A[r + 1:, r], A[r, r + 1:])
        r += 1
    return A, rows, cols, r, err


def default_seeds(n, random_seed=1234):
    """0, 2^n - 1 and 62 indices drawn from random_seed: the default of signal_mps_cross."""
    drawn = np.random.default_rng(random_seed).integers(0, 2 ** n, size=62, dtype=np.int64)
    return np.concatenate([np.array([0, 2 ** n - 1], dtype=np.int64), drawn])


def cross(f, n, tol, maxdim, seeds, max_sweeps=8):
    """f(idx: int64 array) -> values.  Returns a dict: sites (A[alpha, s, beta] arrays), ranks, sweeps, nevals, est (relative
    to fmax), converged, fmax."""
    seeds = [int(s) for s in seeds]
    I = {0: [0]}
    J = {n: [0]}
    for l in range(1, n):
        J[l] = sorted({s & ((1 << (n - l)) - 1) for s in seeds})
    state = {"fmax": float(np.max(np.abs(f(np.array(seeds, dtype=np.int64))))), "nev": 0}

    def block(l):
        rows = np.array([(i << 1) | s for i in I[l - 1] for s in (0, 1)], dtype=np.int64)
        cols = np.array([(s << (n - l - 1)) | j for s in (0, 1) for j in J[l + 1]], dtype=np.int64)
        P = f(((rows[:, None] << (n - l)) | cols[None, :]).reshape(-1)).reshape(len(rows), len(cols))
        state["nev"] += P.size
        state["fmax"] = max(state["fmax"], float(np.abs(P).max()))
        return rows, cols, P

    def step(l):
        rows, cols, P = block(l)
        A, rp, cp, r, e = lu_full(P, tol * state["fmax"], maxdim)
        I[l] = [int(rows[x]) for x in rp[:r]]
        J[l] = [int(cols[x]) for x in cp[:r]]
        return P, A, rp, r, e

    if n == 1:
        x = f(np.array([0, 1], dtype=np.int64))
        return {"sites": [np.asarray(x).reshape(1, 2, 1)], "ranks": [], "sweeps": 1, "nevals": 2, "est": 0.0, "converged": 1,
                "fmax": max(state["fmax"], float(np.abs(x).max()))}
    sweeps, converged, emax = 0, 0, 0.0
    for _ in range(max_sweeps):
        errs = [step(l)[4] for l in range(1, n)]
        errs += [step(l)[4] for l in range(n - 1, 0, -1)]
        sweeps += 1
        emax = max(errs)
        converged = int(emax <= tol * state["fmax"])
        if converged:
            break
    sites = []
    for l in range(1, n):
        cl = len(I[l - 1])
        P, A, rp, r, _ = step(l)
        Lf = np.tril(A[:, :r], -1)
        Lf[np.arange(r), np.arange(r)] = 1
        X = np.linalg.solve(Lf[:r, :r].T, Lf.T).T                    # L L11^-1
        site = np.empty_like(X)
        site[rp, :] = X                                              # undo the row permutation
        sites.append(site.reshape(cl, 2, r))
        if l == n - 1:
            sites.append(P[rp[:r], :].reshape(r, 2, 1))
    return {"sites": sites, "ranks": [len(I[l]) for l in range(1, n)], "sweeps": sweeps, "nevals": state["nev"],
            "est": emax / state["fmax"], "converged": converged, "fmax": state["fmax"]}


def dense(sites):
    v = sites[0].reshape(2, -1)
    for t in sites[1:]:
        v = (v @ t.reshape(t.shape[0], -1)).reshape(-1, t.shape[2])
    return v.reshape(-1)


# ---- the signals of the tests: f(k, N) with k a float64 array of sample positions, evaluated in t = k / N where a raw index
# would cost digits ---------------------------------------------------------------------------------------------------------
MODES = [(1.0, np.exp(-2e-4 + 0.31j)), (0.5 - 0.2j, np.exp(-1e-3 - 1.1j)), (0.25j, np.exp(-5e-4 + 2.3j))]


def three_modes(k, N):
    return sum(a * z ** k for a, z in MODES)


def cospoly(k, N):
    return np.cos(0.05 * k) * (1 + (k / N) ** 2) + 0.3 * np.sin(0.7 * k + 1)


def gauss(k, N):
    return np.exp(-0.5 * ((k / N - 0.37) / 0.04) ** 2)


def chirp(k, N):
    t = k / N
    return np.cos(2 * np.pi * (5 * t + 20 * t * t))


def spike(k, N):
    return (k == 1234) * 1.0 + 1e-3 * np.cos(0.01 * k)


SIGNALS = {"three_modes": three_modes, "cospoly": cospoly, "gauss": gauss, "chirp": chirp}


def sampler(sig, n):
    """The evaluator cross() wants for one of the signals above."""
    N = float(2 ** n)
    return lambda idx: sig(np.asarray(idx, dtype=np.float64), N)
