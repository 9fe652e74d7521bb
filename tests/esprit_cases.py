"""The ESPRIT cases and a numpy model of `shift_pencil`: site loops on host tensors, fed into the real `esprit_from_pencil`.

model_err of a case is the pole error (largest distance of a planted pole from the nearest returned one) this model reaches
against the planted poles, recorded here from a run of tests/test_esprit_model.py, which asserts that the recorded value is within
10x of what it computes.  The GPU tests bound their error by 100 x model_err: a different summation order passing through a
non-normal eigenproblem."""
import numpy as np


def _modes(freqs, damps):
    return [complex(np.exp(-g + 2j * np.pi * f)) for f, g in zip(freqs, damps)]


_F = (0.1234, -0.31, 0.05, 0.42)                      # cycles per sample; the second one on the negative-frequency side
_G = (0.002, 0.004, 0.001, 0.003)
_A = (1.0, 0.6 - 0.3j, -0.45 + 0.2j, 0.25j)
_GN = (2e-5, 5e-5, 1e-5)                              # the dense case: slow enough that all of the 2^14 samples carry every mode

F40, DF40 = 0.1734, 3e-10                             # the two tones of the n = 40 case: 3e-10 of the sample rate apart


def _two_tones():
    f = (F40, F40 + DF40)
    return [complex(np.cos(2 * np.pi * s * x), np.sin(2 * np.pi * s * x)) for x in f for s in (1, -1)], [0.5, 0.5, 0.4, 0.4]


# name -> kind ("sum": exponential_sum untruncated; "dense": dense samples + noise, signal_mps, esprit(maxdim)), n, poles, amps,
# and what the model reached
CASES = {
    "k1_undamped": dict(kind="sum", n=10, poles=_modes(_F[:1], (0.0,)), amps=list(_A[:1]), model_err=1.6e-16),
    "k1_damped": dict(kind="sum", n=10, poles=_modes(_F[:1], _G[:1]), amps=list(_A[:1]), model_err=1.6e-16),
    "k2_undamped": dict(kind="sum", n=10, poles=_modes(_F[:2], (0.0, 0.0)), amps=list(_A[:2]), model_err=2.2e-16),
    "k2_damped": dict(kind="sum", n=10, poles=_modes(_F[:2], _G[:2]), amps=list(_A[:2]), model_err=2.5e-16),
    "k4_undamped": dict(kind="sum", n=10, poles=_modes(_F, (0.0,) * 4), amps=list(_A), model_err=4.0e-16),
    "k4_damped": dict(kind="sum", n=10, poles=_modes(_F, _G), amps=list(_A), model_err=1.1e-15),
    "two_tones_n40": dict(kind="sum", n=40, poles=_two_tones()[0], amps=_two_tones()[1], model_err=1.2e-15),
    "noisy_n14": dict(kind="dense", n=14, poles=_modes(_F[:3], _GN), amps=list(_A[:3]), noise=1e-6, seed=4711, maxdim=3,
                      model_err=4.6e-11),
}
SUM_N10 = [c for c in CASES if CASES[c]["kind"] == "sum" and CASES[c]["n"] == 10]


def exponential_sum_tensors(amps, poles, n, exponential_tensors):
    """Host tensors of the untruncated direct sum linear_combination builds: the weights in the first tensor, block-diagonal
    sites of bond K.  exponential_tensors: the package's host function (the dyadic powers come correctly rounded from it)."""
    K = len(poles)
    per = [exponential_tensors(z, n) for z in poles]
    data = []
    for i in range(n):
        l, r = (1 if i == 0 else K), (1 if i == n - 1 else K)
        A = np.zeros((l, 2, r), dtype=np.complex128)
        for k in range(K):
            A[0 if l == 1 else k, :, 0 if r == 1 else k] = per[k][i][0, :, 0] * (amps[k] if i == 0 else 1.0)
        data.append(A)
    return data


def dense_signal(case):
    c = CASES[case]
    j = np.arange(2 ** c["n"])
    x = sum(a * z ** j for a, z in zip(c["amps"], c["poles"]))
    rng = np.random.default_rng(c["seed"])
    return x + c["noise"] * (rng.standard_normal(j.size) + 1j * rng.standard_normal(j.size)) / np.sqrt(2.0)


def tt_svd(x, maxdim):
    """The plain left-to-right TT-SVD of 2^n samples (site 1 = the most significant bit), every bond cut at maxdim."""
    n = int(round(np.log2(x.size)))
    C, r, data = np.asarray(x).reshape(1, -1), 1, []
    for _ in range(n - 1):
        U, S, Vh = np.linalg.svd(C.reshape(2 * r, -1), full_matrices=False)
        k = min(maxdim, S.size)
        data.append(U[:, :k].reshape(r, 2, k))
        C, r = S[:k, None] * Vh[:k], k
    data.append(C.reshape(r, 2, 1))
    return data


def shift_tensor(bit, Dl, Dr):
    """one site of the ripple-carry shift operator, W[carry out, s_in, s_out, carry in] (builders.shift_mpo_tensors)"""
    W = np.zeros((Dl, 2, 2, Dr))
    for cin in range(Dr):
        for x in range(2):
            t = x + bit + cin
            W[(t >> 1) if Dl == 2 else 0, x, t & 1, cin] = 1.0
    return W


def model_pencil(data, count):
    """(G, P, r_last) of the last `count` host tensors by site loops: G = R R^H, P = R[:, 1:] R[:, :-1]^H, r_last = R[:, -1]"""
    n = len(data)
    G = np.ones((1, 1), dtype=np.complex128)
    E = np.ones((1, 1, 1), dtype=np.complex128)           # the right environment of <psi|S|psi>, E[p, carry, s]
    r = np.ones(1, dtype=np.complex128)
    for i in range(n - 1, n - 1 - count, -1):
        A = np.asarray(data[i], dtype=np.complex128)
        G = np.einsum("pxq,qt,sxt->ps", A, G, A.conj())
        W = shift_tensor(1 if i == n - 1 else 0, 1 if i == 0 else 2, 1 if i == n - 1 else 2)
        E = np.einsum("qbt,pyq,axyb,sxt->pas", E, A.conj(), W, A)
        r = A[:, 1, :] @ r
    return G, E[:, 0, :].conj(), r


def default_count(data):
    bonds = [A.shape[2] for A in data[:-1]]
    return len(data) - 1 - bonds.index(max(bonds))


def pole_error(found, planted):
    found = np.asarray(found)
    return max(float(np.min(np.abs(found - z))) for z in planted)


def model_tensors(case, exponential_tensors):
    c = CASES[case]
    if c["kind"] == "sum":
        return exponential_sum_tensors(c["amps"], c["poles"], c["n"], exponential_tensors)
    return tt_svd(dense_signal(case), c["maxdim"])
