"""The case table of the product-vector read-out (product_batch): operands, weights, longdouble references and the per-value
rounding bound, in the manner of tests/readout_cases.py, whose bound model and operand families it imports.

tests/test_product_cases_model.py (CPU) asserts that a plain float64 numpy evaluation passes every bound, that every case reaches
the route written beside it and that the cone cases are conditioned as claimed; tests/test_gpu_product.py RUNS the table on the
device.  Nothing here needs a GPU or the library.

  value_r = amplitude * prod_i ( v[r,i,0] A_i[:,0,:] + v[r,i,1] A_i[:,1,:] )

Families (seeded by the case's name):
  random   Gaussian sites (readout_cases.mps_data) and Gaussian weights: the sums cancel;
  cone     no cancellation: the sites of readout_cases' cone family with HALF its phase budget (share = 2) and weights of
           modulus in [0.5, 1.5] with phases uniform in [0, pi / (16 n_tensors)], so a site entry times its weight stays
           inside pi / (8 n_tensors) and every partial sum inside a cone of half-angle pi / 8.  Real weights are positive.

References are np.clongdouble chains; the magnitude of a value is the same contraction on |re| + |im| of the sites and of the
weights, which bounds every partial sum of either route.

Bound of one value:   |amplitude| * mag_r * (prod_i (1 + gamma(q_i)) * (1 + 2u) - 1),   q_i = q_of(chi_l) + 8.
Derivation.  q_of(chi_l) = chi_l + 8 + 1 + chi_l is readout_cases' count for one entry of a site step, chain or GEMM: a dot
product of length chi_l in any order, the GEMM suite's 8 for tile edges and the complex product, one slice addition, and a
split-K product's at most chi_l partial sums.  What this verb adds per tensor is c0 x0 + c1 x1 with complex c and x: a complex
product is two real products and one addition per component (3 roundings without FMA), two of them are 6, their sum is 1 more:
7 <= 8.  The chain route forms it BEFORE the dot product (x = the site entries A[alpha, s, beta], each dot-product term then
carries the 7 once); the GEMM route forms it AFTER the product (x = the two slices of Tm, each carrying q_of(chi_l)).  Either
way an entry of the new carry is the exact expression times at most (1 + u)^(q_of(chi_l) + 8) on every term, and the terms are
bounded in sum by the magnitude contraction.  The last factor (1 + 2u) is the multiplication by the amplitude.

Cone cases: sum_i q_i <= 2500, and |value| >= cos(pi / 8) * (sum of moduli) >= cos(pi / 8) / sqrt(2) * mag, so
bound <= 1.53 * 2500 * u * |value| <= 5e-13 |value|: a condition on the inputs, asserted on the CPU."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from readout_cases import (AMPLITUDE, CLD, DTYPES, LD, U, Ref, bound, check, cone_tensors, dims_of, exact, gamma, growth,  # noqa: F401
                           mps_data, modulus, plain, q_of)

C64 = np.complex128
FAMILIES = ("random", "cone")
WEIGHT_KINDS = ("real", "complex")
CHAIN_CAP = 1024                          # QIL_PRODUCT_CHAIN_MAX_BOND: the bond the chain route's LDS carry holds
MANY_ROWS_CHAIN_WORK = 1 << 21            # the verb's own constant: bonds < 128 stay on the chain below this rows * bond^2
CONE_Q_SUM = 2500
CONE_RATIO = 5e-13

Case = namedtuple("Case", "name route bonds nb paired dtype wkind family")

#        name            route    internal bonds           nb    paired
SHAPES = (
    ("one_tensor", "chain", (), 1, False),
    ("two_tensors", "chain", (2,), 3, False),
    ("odd_small", "chain", (3, 5, 3), 7, False),
    ("wide_left", "chain", (33, 65, 2), 5, False),          # a chi_l above 64 lanes, a chi_r that is no multiple of the outputs per pass
    ("paired6", "chain", (2, 4, 8, 4, 2), 9, True),         # a 6-tensor paired state (n = 3)
    ("gemm_wide", "gemm", (130, 7), 5, False),              # the nb >= 4, chi >= 128 arm, odd rows
    # the marginal's nb >= 1024, chi >= 16 arm, rows no multiple of any tile: GEMM_SELECT for the marginal, but under this
    # verb's own many-rows constant (measured: the LDS chain is ahead while rows * bond^2 < 2^21), so it is a chain case, run
    # forced to gemm as every chain case is
    ("gemm_many", "chain", (17, 17, 17, 17), 1027, False),
    ("gemm_many48", "gemm", (48, 48, 48, 48), 1027, False),  # ... and the same arm above this verb's constant: 1027 * 48^2 > 2^21
    ("gemm_skinny", "gemm", (2, 128, 2), 4, False),         # skinny-GEMM rows
    ("above_cap", "gemm", (CHAIN_CAP + 1,), 4, False),      # two wide tensors, one above the LDS cap: GEMM whatever is forced
)

CASES = [Case(f"{name}-{dt}-{wk}-{fam}", route, bonds, nb, paired, dt, wk, fam)
         for name, route, bonds, nb, paired in SHAPES for dt in DTYPES for wk in WEIGHT_KINDS for fam in FAMILIES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def dims(c):
    return dims_of(c.bonds)


def route_of(c, marginal_route, forced=None):
    """The route qil_product_batch takes: the marginal read-out's decision for (nb, bonds) -- `marginal_route` is what
    qil_readout_route answers for the marginal verb -- with the verb's own many-rows constant, unless QIL_PRODUCT_ROUTE forces
    one; the chain only up to the cap."""
    chain = marginal_route == "CHAIN" or (max(dims(c)) < 128 and c.nb * max(dims(c)) ** 2 < MANY_ROWS_CHAIN_WORK)
    if forced is not None:
        chain = forced == "chain"
    return "chain" if chain and max(dims(c)) <= CHAIN_CAP else "gemm"


@functools.lru_cache(maxsize=None)
def weights(name):
    """(nb, n_tensors, 2) float64 / complex128."""
    c = BY_NAME[name]
    n, rng = len(c.bonds) + 1, _rng("weights", name)
    shp = (c.nb, n, 2)
    if c.family == "cone":
        w = rng.uniform(0.5, 1.5, shp)
        if c.wkind == "complex":
            w = w * np.exp(1j * rng.uniform(0.0, np.pi / (16 * n), shp))
    else:
        w = rng.standard_normal(shp)
        if c.wkind == "complex":
            w = w + 1j * rng.standard_normal(shp)
    w.setflags(write=False)
    return w


def operands(c):
    """(site tensors, weights)."""
    return mps_data(c.family, c.dtype, c.bonds, "product", 2), weights(c.name)


def product_values(data, w, work):
    """prod_i (w[:, i, 0] A_i[:, 0, :] + w[:, i, 1] A_i[:, 1, :]) per row, amplitude NOT applied; work = exact / modulus / plain."""
    sites, w = [work(t) for t in data], work(w)
    v = np.ones((w.shape[0], 1), dtype=np.result_type(w.dtype, *[s.dtype for s in sites]))
    for i, A in enumerate(sites):
        v = w[:, i, 0, None] * (v @ A[:, 0, :]) + w[:, i, 1, None] * (v @ A[:, 1, :])
    return v[:, 0]


def product_qs(dm):
    return [q_of(dm[i]) + 8 for i in range(len(dm) - 1)]


def reference_of(data, w, amplitude=AMPLITUDE):
    """The Ref (value, bound) of any operands: the front-end tests evaluate the case bound for an encoded state with it."""
    dm = [data[0].shape[0]] + [t.shape[2] for t in data]
    return Ref(amplitude * product_values(data, w, exact), bound(product_values(data, w, modulus), product_qs(dm), amplitude))


@functools.lru_cache(maxsize=None)
def _reference(name):
    return reference_of(*operands(BY_NAME[name]))


def reference(c):
    """Ref over the rows.  Computed once per case and shared; do not modify."""
    return _reference(c.name)


def oracle_result(c):
    """What a correct float64 implementation returns."""
    data, w = operands(c)
    return AMPLITUDE * product_values(data, w, plain)
