"""The numpy reference, the bond profiles and the spec tables of the operator read-outs, shared by
tests/test_mpo_slice_cases_model.py (CPU: the reference pinned against helpers.dense_mpo) and tests/test_gpu_mpo_slice.py (GPU:
qil_mpo_entry_batch / qil_mpo_slice against it).  No fixtures, no GPU, no library import.

The reference works on the dense 2n-leg tensor T[in_1, out_1, in_2, out_2, ...] of a host MPO chain in longdouble / clongdouble
(`dense_legs`): `reference_slice` indexes fixed legs, sums summed legs, takes the generalised diagonal of a tied site and sums it
(4) or keeps it (5); kept legs stay in chain order, the first one the most significant bit, as mps_to_vector reads a state."""
from functools import lru_cache

import numpy as np

from helpers import random_mpo_data, saturated_profile

FIX0, FIX1, SUM, FREE, TIE, DIAG = 0, 1, 2, 3, 4, 5

# every form of a site that keeps no leg: fix/fix, fix/sum, sum/fix, sum/sum, traced
REMOVED_FORMS = [(0, 0), (1, 0), (0, 1), (1, 1), (0, SUM), (1, SUM), (SUM, 0), (SUM, 1), (SUM, SUM), (TIE, TIE)]
# every form of a site that keeps one leg: in kept with out 0 / 1 / summed, out kept with in 0 / 1 / summed, the diagonal
KEPT_FORMS = [(FREE, 0), (FREE, 1), (FREE, SUM), (0, FREE), (1, FREE), (SUM, FREE), (DIAG, DIAG)]

# internal bonds; every chain length is even, so every profile runs plain and paired
PROFILES = {
    "bond1": [1] * 5,
    "odd": [2, 3, 5, 7, 5, 3, 2],
    "sat48": saturated_profile(8, 48, base=4),
    "sat64": saturated_profile(8, 64, base=4),        # the c64 LDS limit of the runs
    "sat96": saturated_profile(8, 96, base=4),        # the f64 limit; the GEMM route for c64
    "straddle": [4, 16, 128, 128, 128, 16, 4],        # both sides of both limits: one call mixes the routes
}
ENTRY_ONLY_PROFILES = {"above_cap": [4, 16, 64, 1025, 64, 16, 4]}      # one bond above the chain cap of the entries
ENTRY_PROFILES = {**PROFILES, **ENTRY_ONLY_PROFILES}
SMALLEST = ("bond1", "odd")


# ================================================================ the reference
def dense_legs(data):
    """T[in_1, out_1, ..., in_n, out_n] of a chain of W_i[a, s_in, s_out, b], in longdouble / clongdouble."""
    wide = np.clongdouble if any(np.iscomplexobj(w) for w in data) else np.longdouble
    T = data[0][0].astype(wide)
    for w in data[1:]:
        T = np.tensordot(T, w.astype(wide), axes=([-1], [0]))
    return T[..., 0]


def reference_slice(data, spec, dense=None):
    """The slice of the operator that `spec` (n x 2: in, out per tensor) names, as a flat vector over the kept legs (a 0-d array
    where none is kept).  dense: dense_legs(data), where the caller has it already."""
    T = dense_legs(data) if dense is None else dense
    spec = np.asarray(spec)
    assert spec.shape == (T.ndim // 2, 2)
    for i in range(len(spec) - 1, -1, -1):                    # from the last site: the axes in front keep their numbers
        a, b = int(spec[i, 0]), int(spec[i, 1])
        if a >= TIE or b >= TIE:
            assert a == b and a <= DIAG
            T = np.diagonal(T, axis1=2 * i, axis2=2 * i + 1)  # the diagonal becomes the last axis
            T = T.sum(axis=-1) if a == TIE else np.moveaxis(T, -1, 2 * i)
            continue
        for axis, v in ((2 * i + 1, b), (2 * i, a)):          # out first: in keeps its number
            if v == SUM:
                T = T.sum(axis=axis)
            elif v != FREE:
                T = np.take(T, v, axis=axis)
    return T.reshape(-1) if T.ndim else T


@lru_cache(maxsize=None)
def case_data(case, complex_):
    """(host chain, its dense 2n-leg tensor) of a profile: made once, shared by every test, never modified."""
    rng = np.random.default_rng(2700 + sorted(ENTRY_PROFILES).index(case) * 2 + int(complex_))
    data = random_mpo_data(ENTRY_PROFILES[case], rng, np.complex128 if complex_ else np.float64)
    for w in data:
        w.setflags(write=False)
    dense = dense_legs(data)
    dense.setflags(write=False)
    return data, dense


# ================================================================ the spec tables
def kept_positions(spec):
    spec = np.asarray(spec)
    return [i for i in range(len(spec)) if spec[i, 0] == DIAG or (spec[i, 0] == FREE) != (spec[i, 1] == FREE)]


def whole_pairs(spec):
    kept = kept_positions(spec)
    return len(kept) % 2 == 0 and all(kept[j] % 2 == 0 and kept[j + 1] == kept[j] + 1 for j in range(0, len(kept), 2))


def slice_specs(n, rng):
    """name -> (n x 2) spec for a chain of n >= 6 tensors.  Kept and removed sites cycle through every form, from a random start."""
    k0, r0 = int(rng.integers(0, len(KEPT_FORMS))), int(rng.integers(0, len(REMOVED_FORMS)))
    count = [0]

    def keep_all():
        return np.array([KEPT_FORMS[(k0 + i) % len(KEPT_FORMS)] for i in range(n)], dtype=np.uint8)

    def remove(s, sites):
        for i in sites:
            s[i] = REMOVED_FORMS[(r0 + count[0]) % len(REMOVED_FORMS)]
            count[0] += 1
        return s

    out = {}
    out["leading"] = remove(keep_all(), range(3))
    out["trailing"] = remove(keep_all(), range(n - 3, n))
    out["both"] = remove(keep_all(), [0, 1, n - 2, n - 1])
    out["run1"] = remove(keep_all(), [3])
    out["run2"] = remove(keep_all(), [3, 4])
    out["run5"] = remove(keep_all(), range(1, 6))                          # trailing when n = 6
    out["several"] = remove(keep_all(), [1, 3, 4] + ([6, 7] if n >= 8 else []))
    out["odd_removed"] = remove(keep_all(), range(1, n, 2))
    out["even_removed"] = remove(keep_all(), range(0, n, 2))
    for name, k in (("only_first", 0), ("only_middle", n // 2), ("only_last", n - 1)):
        out[name] = remove(keep_all(), [i for i in range(n) if i != k])
    forms = REMOVED_FORMS + KEPT_FORMS
    s = np.array([forms[int(v)] for v in rng.integers(0, len(forms), n)], dtype=np.uint8)
    s[int(rng.integers(0, n))] = KEPT_FORMS[int(rng.integers(0, len(KEPT_FORMS)))]
    out["random"] = s
    # the named read-outs: a column, a row, the diagonal, W on the all-ones signal
    bits = rng.integers(0, 2, n)
    out["column"] = np.stack([bits, np.full(n, FREE)], axis=1).astype(np.uint8)
    out["row"] = np.stack([np.full(n, FREE), bits], axis=1).astype(np.uint8)
    out["diagonal"] = np.full((n, 2), DIAG, dtype=np.uint8)
    out["column_sums"] = np.stack([np.full(n, SUM), np.full(n, FREE)], axis=1).astype(np.uint8)
    return out


ENTRY, SUMS, TRACES = 0, 1, 2      # the kind of a row: pure entry, with summed legs, with traced sites


def entry_rows(n, rng, per_kind=100):
    """(spec (nb, n, 2), kind (nb,)): per_kind rows of each kind, the all-fixed, all-(2,2) and all-(4,4) rows among them."""
    rows, kinds = [], []
    for _ in range(per_kind):
        rows.append(rng.integers(0, 2, (n, 2)))
        kinds.append(ENTRY)
    for j in range(per_kind):
        s = rng.integers(0, 3, (n, 2))
        if j == 0:
            s[:] = SUM
        s[int(rng.integers(0, n)), int(rng.integers(0, 2))] = SUM
        rows.append(s)
        kinds.append(SUMS)
    for j in range(per_kind):
        s = rng.integers(0, 3, (n, 2))
        tied = rng.integers(0, 2, n).astype(bool)
        tied[int(rng.integers(0, n))] = True
        if j == 0:
            tied[:] = True
        s[tied] = TIE
        rows.append(s)
        kinds.append(TRACES)
    return np.array(rows, dtype=np.uint8), np.array(kinds)


def reference_entries(data, dense, specs):
    wide = dense.dtype
    return np.array([reference_slice(data, s, dense) for s in specs], dtype=wide)
