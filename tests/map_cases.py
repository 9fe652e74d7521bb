"""The case table of the element-wise maps (qil_mps_map, map_states): operands, functions, seeds and the error budget.

tests/test_map_cases_oracle.py (CPU) runs the numpy model of the cross interpolation (tests/cross_model.py) on g = op(dense
operands) and holds it to a ninth of the interpolation bound, as tests/test_cross_model.py does for the encoder;
tests/test_gpu_map.py runs the same cases on the device.  Nothing here needs a GPU or the library.

Operands: the cross_model signals at n = 12 and b_j = 2 + cos(2 pi 3 j / N), which stays in [1, 3].  At n = 12 a rank of 64 is
full, so even the kinked shrinkage is representable at maxdim = 64.

Budget of a device result against g computed in numpy from the operands' dense read-out:
    n tol max|g|  +  perturbation(delta)  +  16 * 2^-53 max|g|
  * n tol max|g|: the stop rule allows tol fmax at each of the n - 1 bonds (tests/test_cross_model.py);
  * delta: how far a sample the map reads can lie from the dense read-out the test computes g from -- both contract the same
    tensors in another order, so the distance is at most the sum of their rounding bounds (readout_cases: the chain bound for the
    sampler, the block bound for mps_to_vector), summed over the operands;
  * perturbation(delta) = L_f delta for an op with the Lipschitz constant L_f on the operands' range:
        abs, shrink   1 (both are non-expansive, for complex values too)
        log           max |d/da log(a^2 + eps)| = 1 / sqrt(eps), at a = sqrt(eps)
        divide        max(1 / min|b|, max|a| / min|b|^2): the partial derivatives of a conj(b) / (|b|^2 + lambda) in a and in b
                      are largest at lambda = 0
    and delta^p for power with p <= 1, which has NO Lipschitz constant on a range that reaches 0 (the Gaussian's tail does):
    | |x|^p - |y|^p | <= |x - y|^p is its Hoelder bound;
  * 16 * 2^-53 max|g|: the roundings of evaluating the function itself (hypot, pow, log, the division), on both sides."""
import functools
from collections import namedtuple

import numpy as np

import cross_model as M

N_SITES = 12
MAXDIM = 64
MAX_SWEEPS = 8
TOLS = (1e-9, 1e-6)
SEED_PEAKS = 8
ROOM = 9.0

Case = namedtuple("Case", "name op operands param result_complex")


def _b(k, N):
    return 2.0 + np.cos(2 * np.pi * 3 * k / N)


SIGNALS = dict(M.SIGNALS, b=_b)


@functools.lru_cache(maxsize=None)
def signal(name, n=N_SITES):
    x = SIGNALS[name](np.arange(2 ** n, dtype=np.float64), float(2 ** n))
    x.setflags(write=False)
    return x


def _tau(name):
    return 0.3 * float(np.abs(signal(name)).max())


CASES = [
    Case("abs_chirp", "abs", ("chirp",), None, False),
    Case("power_gauss", "power", ("gauss",), 0.5, False),
    Case("log_gauss", "log", ("gauss",), 1e-12, False),
    Case("divide_three_modes_b", "divide", ("three_modes", "b"), 0.0, True),
    Case("divide_chirp_b_reg", "divide", ("chirp", "b"), 0.1, False),
    Case("shrink_gauss", "shrink", ("gauss",), _tau("gauss"), False),
    Case("shrink_chirp", "shrink", ("chirp",), _tau("chirp"), False),
]
BY_NAME = {c.name: c for c in CASES}


def evaluate(c, *xs):
    """The function of the case on dense operands, in numpy."""
    a = np.asarray(xs[0])
    if c.op == "abs":
        return np.abs(a)
    if c.op == "power":
        return np.abs(a) ** c.param
    if c.op == "log":
        return np.log(np.abs(a) ** 2 + c.param)
    if c.op == "divide":
        b = np.asarray(xs[1])
        return a * np.conj(b) / (np.abs(b) ** 2 + c.param)
    m = np.abs(a)                                          # shrink
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(m > 0, np.maximum(0.0, 1.0 - c.param / np.where(m > 0, m, 1.0)), 0.0)
    return a * f


def lipschitz(c, *xs):
    """L_f of the case on the range of its operands; None for power with p <= 1 (see perturbation)."""
    if c.op in ("abs", "shrink"):
        return 1.0
    if c.op == "log":
        return 1.0 / np.sqrt(c.param)
    if c.op == "divide":
        amax, bmin = float(np.abs(xs[0]).max()), float(np.abs(xs[1]).min())
        return max(1.0 / bmin, amax / bmin ** 2)
    return None if c.param <= 1 else c.param * float(np.abs(xs[0]).max()) ** (c.param - 1)


def perturbation(c, delta, *xs):
    """How far the function's value can move when every operand moves by at most delta."""
    L = lipschitz(c, *xs)
    return float(delta) ** c.param if L is None else L * float(delta)


def budget(c, tol, g, delta, *xs):
    gmax = float(np.abs(g).max())
    return N_SITES * tol * gmax + perturbation(c, delta, *xs) + 16 * 2.0 ** -53 * gmax


def seeds(*xs, n=N_SITES, random_seed=1234):
    """signal_mps_cross' default seeds, then the SEED_PEAKS largest entries of every operand: what map_states starts from."""
    parts = [M.default_seeds(n, random_seed)]
    for x in xs:
        parts.append(np.argsort(-np.abs(np.asarray(x)), kind="stable")[:SEED_PEAKS].astype(np.int64))
    return np.concatenate(parts)


def dense_operands(c):
    return tuple(signal(name) for name in c.operands)
