"""The case table of the read-out by index (qil_coefficient_at): operands, int64 indices, longdouble references and the
per-coefficient rounding bound of tests/readout_cases.py, which this module imports unmodified.

tests/test_index_readout_cases_oracle.py (CPU) asserts that a plain float64 numpy evaluation passes every bound and that every
case reaches the route written beside it; tests/test_gpu_coefficient_at.py RUNS the table on the device.  Nothing here needs a GPU
or the library.

An index j has the bits b_1 .. b_n of the chain's n tensors, tensor 1 the most significant: b_i = (j >> (n - i)) & 1.  For a
paired chain the tensors are main_1, copy_1, main_2, ..: the point (k, l) of coefficient_grid is the index with b_{2i+1} = bit i
of k and b_{2i+2} = bit i of l (readout_cases.grid_of's interleaving).

Bound of one coefficient: readout_cases.bound with the chain's q(k) = 2 k + 9 per tensor, k = chi_l -- both routes are dot
products of length chi_l per tensor (the wave route in any lane order, the bits route the chain and the selecting GEMM of the
table in readout_cases).  A row whose index lies outside [0, 2^n) must come back as NaN, in both parts for c64."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

import readout_cases as R
from readout_cases import (AMPLITUDE, CHAIN15, CONE_RATIO, DTYPES, FAMILIES, GRID_BONDS, GRID_N, Ref, bound, chain_qs, chain_values,  # noqa: F401
                           check, dims_of, exact, modulus, mps_data, plain)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the auto decision's cap, from the header: both sides of it are cases
CAP = int(re.search(r"#define\s+QIL_COEFFICIENT_AT_WAVE_MAX_BOND\s+(\d+)", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()).group(1))
WAVE_FIT = 1024                            # what QIL_COEFFICIENT_AT_ROUTE=wave can still take: the carry in LDS
INT64_MIN = -2 ** 63
LONG_BONDS = tuple((2, 3, 1, 4)[i % 4] for i in range(61))          # 62 tensors

Case = namedtuple("Case", "name route dtype family p")


def route_of(dims, forced=None):
    """The table's own statement of the decision (the C code and ops.coefficient_at_route must agree with it)."""
    top = max(dims)
    if forced == "bits":
        return "bits"
    if forced == "wave":
        return "wave" if top <= WAVE_FIT else "bits"
    return "wave" if top <= CAP else "bits"


def _random_indices(key, n, count):
    return R._rng("index", key, n, count).integers(0, 2 ** n, size=count, dtype=np.int64)


def _chain15_indices(count):
    n = len(CHAIN15) + 1
    idx = _random_indices("chain15", n, count)
    if count >= 3:
        idx[0], idx[1], idx[2] = 0, 2 ** n - 1, idx[-1]              # both ends and a duplicate
    return idx


def grid_points():
    """(ks, ls) of the paired case and their indices, row-major in (k, l)."""
    rng = R._rng("index grid")
    ks, ls = rng.permutation(2 ** GRID_N)[:7], rng.permutation(2 ** GRID_N)[:6]
    idx = np.zeros((len(ks), len(ls)), dtype=np.int64)
    for x, k in enumerate(ks):
        for y, l in enumerate(ls):
            j = 0
            for i in range(GRID_N):
                j = (j << 2) | (((int(k) >> i) & 1) << 1) | ((int(l) >> i) & 1)
            idx[x, y] = j
    return ks, ls, idx.reshape(-1)


def _rows():
    rows = []                                              # (name, bonds, idx, paired)
    for count in (1, 3, 300):
        rows.append((f"chain15_count{count}", CHAIN15, _chain15_indices(count), False))
    rows.append(("one_site", (), np.arange(2, dtype=np.int64), False))
    rows.append(("two_sites", (3,), np.arange(4, dtype=np.int64), False))
    special = np.array([0, 2 ** 61, 2 ** 62 - 1, 2 ** 32 - 1, 2 ** 32], dtype=np.int64)
    rows.append(("long62", LONG_BONDS, np.concatenate([special, _random_indices("long62", 62, 40)]), False))
    for top in (CAP, CAP + 1):
        for count in (5, 300):
            rows.append((f"threshold_bond{top}_count{count}", (2, 4, 8, top, 8, 4, 2), _random_indices("threshold", 8, count), False))
    rows.append(("paired_grid", GRID_BONDS, grid_points()[2], True))
    mixed = _chain15_indices(50)
    mixed[[4, 17, 33]] = [-1, 2 ** (len(CHAIN15) + 1), INT64_MIN]
    rows.append(("out_of_range", CHAIN15, mixed, False))
    return rows


CASES = [Case(f"{name}-{dt}-{fam}", route_of(dims_of(bonds)), dt, fam, dict(bonds=bonds, idx=idx, paired=paired, key=name))
         for name, bonds, idx, paired in _rows() for dt in DTYPES for fam in FAMILIES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def ntensors(c):
    return len(c.p["bonds"]) + 1


def valid(c):
    """The rows whose index lies in [0, 2^n); the others must read NaN."""
    idx = c.p["idx"]
    return (idx >= 0) & (idx < 2 ** ntensors(c))


def bits_of(idx, n):
    """(count, n) uint8, tensor 1 first: Python integers, so that no shift is taken in 32 or 64 bits."""
    return np.array([[(int(j) >> (n - 1 - i)) & 1 for i in range(n)] for j in idx], dtype=np.uint8).reshape(len(idx), n)


def operands(c):
    """(site tensors, indices)."""
    return mps_data(c.family, c.dtype, c.p["bonds"], "index-" + c.p["key"].split("_count")[0]), c.p["idx"]


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = BY_NAME[name]
    data, idx = operands(c)
    bits = bits_of(idx[valid(c)], ntensors(c))
    return Ref(AMPLITUDE * chain_values(data, bits, exact), bound(chain_values(data, bits, modulus), chain_qs(dims_of(c.p["bonds"]))))


def reference(c):
    """Ref over the VALID rows of the case, in order.  Computed once per case and shared; do not modify."""
    return _reference(c.name)


def grid_reference(c):
    """The paired case once more, from the dense tensor through readout_cases.grid_of: (value, bound) as (7, 6) arrays."""
    data, _ = operands(c)
    ks, ls, _ = grid_points()
    value = AMPLITUDE * R.grid_of(R.dense_tensor(data, exact), ks, ls)
    return Ref(value, bound(R.grid_of(R.dense_tensor(data, modulus), ks, ls), chain_qs(dims_of(c.p["bonds"]))))


def oracle_result(c):
    """What a correct float64 implementation returns on the valid rows."""
    data, idx = operands(c)
    return AMPLITUDE * chain_values(data, bits_of(idx[valid(c)], ntensors(c)), plain)
