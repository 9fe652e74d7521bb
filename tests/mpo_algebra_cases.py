"""The table of operator-sum and Frobenius-overlap cases shared by tests/test_mpo_algebra_model.py (CPU: the numpy model in the
device's place -- do the inputs keep the reference itself inside every bound?) and tests/test_gpu_mpo_algebra.py (GPU: the same
assertions on qil_mpo_sum / qil_mpo_inner).  No fixtures, no GPU, no library import.

The numpy model: `direct_sum` (the weights in the first tensor), `frobenius` (the overlap by environment contraction in
clongdouble) and `shift_dense` (the cyclic shift through np.roll).  The checks take the RESULT of a backend (site tensors, a
number), not the backend.

Tolerances are the project's: the first tensor of a sum within 1e-14 of its largest entry (one multiply), interior and last
tensors EQUAL with +0.0 off the blocks, dense read-outs 1e-12 of scale, an overlap within 1e-12 of |V|_F |W|_F (`near` of
tests/test_gpu_overlap.py: an overlap is conditioned by the norms of its operands, not by its own size), two routes or the two
argument orders within 1e-13 of that scale."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from helpers import random_mpo_data, dense_mpo

F, Z = np.float64, np.complex128
# (dtype of the even terms, dtype of the odd terms), as tests/test_gpu_sum.py
DTYPES = [(F, F), (F, Z), (Z, F), (Z, Z)]


# ================================================================ the model
def direct_sum(terms, w):
    """The direct sum of host MPO chains (lists of W[a, s_in, s_out, b]) with the weights w in the first tensor."""
    N = len(terms[0])
    w = np.asarray(w)
    dt = np.result_type(*[t[0].dtype for t in terms], Z if np.iscomplexobj(w) and np.any(np.imag(w) != 0) else F)
    w = w.astype(dt)
    if N == 1:
        return [sum(c * t[0] for c, t in zip(w, terms)).astype(dt)]
    out = [np.concatenate([c * t[0].astype(dt) for c, t in zip(w, terms)], axis=3)]
    for i in range(1, N - 1):
        A = np.zeros((sum(t[i].shape[0] for t in terms), 2, 2, sum(t[i].shape[3] for t in terms)), dt)
        lo = ro = 0
        for t in terms:
            A[lo:lo + t[i].shape[0], :, :, ro:ro + t[i].shape[3]] = t[i]
            lo, ro = lo + t[i].shape[0], ro + t[i].shape[3]
        out.append(A)
    out.append(np.concatenate([t[N - 1].astype(dt) for t in terms], axis=0))
    return out


def frobenius(v, w):
    """<V, W>_F = tr(V^dagger W) = sum_{x,y} conj(V[x,y]) W[x,y] by environment contraction, in clongdouble."""
    E = np.ones((1, 1), dtype=np.clongdouble)
    for a, b in zip(v, w):
        T = np.tensordot(E, b.astype(np.clongdouble), axes=([1], [0]))                    # [p, i, o, b]
        E = np.tensordot(np.conj(a.astype(np.clongdouble)), T, axes=([0, 1, 2], [0, 1, 2]))   # [q, b]
    return complex(E[0, 0])


def shift_dense(n, s):
    """helpers.dense_mpo's M[in, out] of (S psi)_x = psi_{(x - s) mod 2^n}: M[x, (x + s) mod 2^n] = 1."""
    return np.roll(np.eye(2 ** n), s, axis=1)


def scale_of(t):
    return max(np.abs(t).max(), 1e-300)


def near(a, b, scale, tol):
    """|a - b| <= tol * max(|b|, scale), as tests/test_gpu_overlap.py"""
    return abs(a - b) <= tol * max(abs(b), scale)


# ================================================================ sums
# bonds: the base profile; term j gets term_bonds(bonds, j).  dtypes: (even terms, odd terms).  handles: term -> operand index
# (None: each its own).  coeffs: "real", "complex", or a tuple.
SumCase = namedtuple("SumCase", "name paired bonds nterms dtypes coeffs handles seed", defaults=("real", None, 0))


def term_bonds(base, j, capped):
    """mixed bonds per term (the caps of tests/test_gpu_sum.py's _term_bonds), never above what the site count allows"""
    if not capped:
        return list(base)
    cap = (3, 64, 5, 2, 7, 1, 4)[j % 7]
    n = len(base) + 1
    return [min(b, cap, 4 ** (i + 1), 4 ** (n - 1 - i)) for i, b in enumerate(base)]


_SHAPES = {
    # name: (bonds, nterms, single, paired, per-term caps)
    "n1": ([], 3, True, False, False),                       # no bonds: the accumulate path, four entries
    "n2": ([3], 3, True, True, True),                        # first and last site only
    "bond1": ([1] * 5, 3, True, True, False),
    "odd": ([2, 3, 5, 7, 5, 3, 2], 3, True, True, True),     # odd row counts: the unpacked f64 store
    "tall": ([64, 64], 9, True, False, False),               # 576 rows: more than one f64 row tile of 512
    "many": ([1] * 3, 20, True, True, False),                # the term walk crosses column chunks
}


def _sum_cases():
    cases, seed = [], 300
    for name, (bonds, nterms, single, paired, _) in _SHAPES.items():
        for p in ([False] if single else []) + ([True] if paired else []):
            for d0, d1 in DTYPES:
                seed += 1
                cases.append(SumCase(f"{name}-{'paired' if p else 'single'}-{np.dtype(d0).kind}{np.dtype(d1).kind}", p, name,
                                     nterms, (d0, d1), "real", None, seed))
    cases.append(SumCase("repeat-single-ff", False, "odd", 2, (F, F), (1.0, 1.0), (0, 0), 390))          # W + W
    cases.append(SumCase("repeat-paired-cc", True, "bond1", 3, (Z, Z), "complex", (0, 1, 0), 391))
    cases.append(SumCase("complex-coeffs-real-operands", False, "odd", 3, (F, F), "complex", None, 392))
    cases.append(SumCase("complex-coeffs-n1", False, "n1", 2, (F, F), "complex", None, 393))
    cases.append(SumCase("zero-coeff-keeps-its-block", False, "odd", 3, (F, Z), (0.75, 0.0, -1.5), None, 394))
    cases.append(SumCase("one-term-scale", True, "n2", 1, (F, F), (2j,), None, 395))
    return cases


SUMS = _sum_cases()


def sum_case(name):
    return next(c for c in SUMS if c.name == name)


@lru_cache(maxsize=None)
def sum_operands(name):
    """(operand tensors, handles, coefficients, site ids): the seeded inputs of the case (treat as read-only)"""
    c = sum_case(name)
    base, _, _, _, capped = _SHAPES[c.bonds]
    rng = np.random.default_rng(c.seed)
    handles = tuple(range(c.nterms)) if c.handles is None else c.handles
    datas = [random_mpo_data(term_bonds(base, j, capped), rng, c.dtypes[j % 2]) for j in range(max(handles) + 1)]
    if c.coeffs == "real":
        coeffs = rng.standard_normal(c.nterms)
    elif c.coeffs == "complex":
        coeffs = rng.standard_normal(c.nterms) + 1j * rng.standard_normal(c.nterms)
    else:
        coeffs = np.asarray(c.coeffs)
    return datas, handles, coeffs, list(range(3, 3 + len(base) + 1))


@lru_cache(maxsize=None)
def sum_reference(name):
    """the model's direct sum of the case, computed once"""
    datas, handles, coeffs, _ = sum_operands(name)
    return tuple(direct_sum([datas[h] for h in handles], coeffs))


def check_sum_sites(name, got, got_bonds):
    """Site by site against the model: shapes, dtype and bonds (= the sums); interior and last tensors EQUAL with +0.0 off the
    blocks; the first tensor within 1e-14 of its largest entry."""
    datas, handles, _, _ = sum_operands(name)
    ref = sum_reference(name)
    n = len(ref)
    want_bonds = [sum(datas[h][i].shape[3] for h in handles) for i in range(n - 1)]
    assert list(got_bonds) == want_bonds, (name, got_bonds, want_bonds)
    assert len(got) == n
    for i in range(n):
        g = np.asarray(got[i])
        assert g.shape == ref[i].shape and g.dtype == ref[i].dtype, (name, i, g.shape, g.dtype)
        if i == 0:
            err = np.abs(g - ref[i]).max() / scale_of(ref[i])
            assert err <= 1e-14, (name, i, err)
        else:
            assert np.array_equal(g, ref[i]), (name, i)
            zero = ref[i] == 0
            assert not np.any(np.signbit(g.real[zero])), (name, i)
            if np.iscomplexobj(g):
                assert not np.any(np.signbit(g.imag[zero])), (name, i)


def check_sum_dense(name, got):
    """dense(out) within 1e-12 of scale of sum_j c_j dense(term_j) (at most 10 tensors)"""
    datas, handles, coeffs, _ = sum_operands(name)
    assert len(got) <= 10
    parts = [c * dense_mpo(datas[h]) for c, h in zip(coeffs, handles)]
    want = sum(parts)
    top = max(scale_of(want), max(scale_of(p) for p in parts))
    err = np.abs(dense_mpo([np.asarray(t) for t in got]) - want).max() / top
    assert err <= 1e-12, (name, err)
    return err


# ================================================================ overlaps
InnerCase = namedtuple("InnerCase", "name paired bonds_v bonds_w dtypes seed")


def _inner_cases():
    cases, seed = [], 400
    ragged1, ragged2 = [3, 9, 17, 6, 4], [2, 5, 13, 7, 3]                 # the operands of tests/mpo_cases.py
    for paired in (False, True):
        for d0, d1 in DTYPES:
            seed += 1
            cases.append(InnerCase(f"ragged-{'paired' if paired else 'single'}-{np.dtype(d0).kind}{np.dtype(d1).kind}", paired,
                                   ragged1, ragged2, (d0, d1), seed))
    cases.append(InnerCase("n1", False, [], [], (F, Z), 420))
    cases.append(InnerCase("bond1", True, [1] * 5, [1] * 5, (Z, F), 421))
    # the auto crossover (12), the states' crossover (16) and the chain cap (64), each from both sides, on four tensors
    for b, dts in ((12, (Z, F)), (13, (F, F)), (16, (F, F)), (17, (Z, Z)), (64, (Z, F)), (65, (F, Z))):
        cases.append(InnerCase(f"bond{b}", False, [b] * 3, [b] * 3, dts, 430 + b))
    return cases


INNERS = _inner_cases()
ROUTES = ("auto", "chain", "gemm")


def inner_case(name):
    return next(c for c in INNERS if c.name == name)


@lru_cache(maxsize=None)
def inner_operands(name):
    c = inner_case(name)
    rng = np.random.default_rng(c.seed)
    return random_mpo_data(c.bonds_v, rng, c.dtypes[0]), random_mpo_data(c.bonds_w, rng, c.dtypes[1])


@lru_cache(maxsize=None)
def inner_reference(name):
    """(np.vdot of the dense operators, |V|_F |W|_F): at most 10 tensors"""
    v, w = inner_operands(name)
    assert len(v) <= 10
    dv, dw = dense_mpo(v), dense_mpo(w)
    return complex(np.vdot(dv, dw)), float(np.linalg.norm(dv) * np.linalg.norm(dw))


def check_inner(name, got):
    """near(got, vdot(dense V, dense W), |V|_F |W|_F, 1e-12).  Returns the error in units of the scale."""
    want, scale = inner_reference(name)
    assert near(got, want, scale, 1e-12), (name, got, want, abs(got - want) / scale)
    return abs(got - want) / scale


def check_inner_agree(name, a, b):
    """two routes, or <V, W> against conj <W, V>: within 1e-13 of |V|_F |W|_F"""
    _, scale = inner_reference(name)
    assert abs(a - b) <= 1e-13 * scale, (name, a, b, abs(a - b) / scale)


# ================================================================ shifts with dyadic weights: exact integers
SHIFT_TAPS = {0: 0.5, 1: 0.25, 3: -0.125}
SHIFT_TAPS_NORM2_PER_SAMPLE = 0.25 + 0.0625 + 0.015625      # |sum_k h_k S^k|_F^2 / 2^n: distinct shifts are orthogonal
