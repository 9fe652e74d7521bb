"""The case table of the read-out suite: operands, bit patterns, longdouble references and the per-coefficient rounding bound.

tests/test_readout_cases_oracle.py (CPU) asserts that every case reaches the route written beside it and that a plain float64
numpy evaluation passes every bound; tests/test_gpu_readout.py RUNS the same table on the device.  Nothing here needs a GPU or the
library.

Operand families (seeded by the case's name):
  random   helpers.random_mps_data / random_mpo_data: Gaussian entries, the sums cancel;
  cone     no cancellation: moduli uniform in [0.5, 1.5] / (2 chi_l), each physical slice of a site scaled by its own
           10^(-2 U[0, 1]), complex phases uniform in [0, pi / (8 n_tensors)] (lazy cases: half of that for W and for psi).  Every
           partial sum stays inside a cone of half-angle pi / 8, so |value| >= cos(pi / 8) * sum of moduli and the bound below is a
           small multiple of each coefficient's OWN modulus although the coefficients of one batch span many decades.

References are evaluated in np.longdouble / np.clongdouble (64-bit mantissa).  Each comes with its magnitude: the same
contraction on |re| + |im| of the operands (the model of tests/test_gpu_gemm.py), which bounds every partial sum of the value.

Bound of one coefficient:   |amplitude| * mag_q * (prod_i (1 + gamma(q_i)) * (1 + 2u) - 1),   gamma(q) = q u / (1 - q u), u = 2^-53
where q_i counts the roundings one entry of step i can collect: a dot product of length k in any order with FMAs is k, the GEMM
suite allows 8 on top (tile-edge additions, the complex product), the marginal's slice addition is 1, and a split-K product adds
its slices once more -- at most k of them (split counts are a tuning matter; k is what they cannot exceed):
    q(k) = k + 8 + 1 + k.
  chain / GEMM forms  k = chi_l of the site;
  lazy                two stages per site, k = D_l and k = 2 chi_l;
  dense block         k = max(chi_l, chi_r) per site (sites behind the last free one are folded from the right, contracting
                      chi_r), and the closing product with the boundary vector, k = the widest bond;
  sweep               the product chain is read: k = chi_l D_l, plus 2 for the two-term sum that forms each product entry;
  laplace_values      3 more for the factor dt sqrt(N) and its product with the sum.
The last factor (1 + 2u) is the multiplication by the amplitude (and the conversion of the result)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from helpers import random_mps_data, random_mpo_data

U = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble
F64, C64 = np.float64, np.complex128
DTYPES = {"f64": F64, "c64": C64}
FAMILIES = ("random", "cone")
AMPLITUDE = 1.7
CONE_RATIO = 2e-13                      # cone cases: bound_q <= CONE_RATIO * |ref_q| (a condition on the inputs)

Case = namedtuple("Case", "name kind verb route dtype family p")


def dims_of(bonds):
    return [1] + list(bonds) + [1]


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


# ---------------------------------------------------------------- operands
def cone_tensors(dims, rng, dtype, phys, phase):
    out = []
    for i in range(len(dims) - 1):
        shp = (dims[i],) + (2,) * phys + (dims[i + 1],)
        t = rng.uniform(0.5, 1.5, shp) / (2.0 * dims[i])
        t = t * 10.0 ** (-2.0 * rng.uniform(size=(1,) + (2,) * phys + (1,)))
        if np.dtype(dtype) == C64:
            t = t * np.exp(1j * rng.uniform(0.0, phase, shp))
        out.append(t.astype(dtype))
    return out


@functools.lru_cache(maxsize=None)
def mps_data(family, dtype, bonds, key, share=1):
    """Site tensors (chi_l, 2, chi_r) of a chain with the internal `bonds` (a tuple); share = 2 in lazy cases."""
    dims, rng = dims_of(bonds), _rng("mps", family, dtype, bonds, key)
    if family == "cone":
        return cone_tensors(dims, rng, DTYPES[dtype], 1, np.pi / (8 * share * (len(dims) - 1)))
    return random_mps_data(list(bonds), rng, DTYPES[dtype], normalize=False)


@functools.lru_cache(maxsize=None)
def mpo_data(family, dtype, bonds, key):
    """Site tensors (D_l, in, out, D_r)."""
    dims, rng = dims_of(bonds), _rng("mpo", family, dtype, bonds, key)
    if family == "cone":
        return cone_tensors(dims, rng, DTYPES[dtype], 2, np.pi / (16 * (len(dims) - 1)))
    return random_mpo_data(list(bonds), rng, DTYPES[dtype])


def basis_mps_data(config, bonds, dtype=F64):
    """|config>, its bonds padded with zero rows: only entry [0, config_i, 0] of site i is set."""
    dims = dims_of(bonds)
    data = [np.zeros((dims[i], 2, dims[i + 1]), dtype=dtype) for i in range(len(config))]
    for t, b in zip(data, config):
        t[0, b, 0] = 1.0
    return data


def flip_mpo_data(flips, bonds, dtype=F64):
    """The operator that flips bit i where flips[i] is set, bonds padded with zero rows."""
    dims = dims_of(bonds)
    data = [np.zeros((dims[i], 2, 2, dims[i + 1]), dtype=dtype) for i in range(len(flips))]
    for t, f in zip(data, flips):
        for s in (0, 1):
            t[0, s, s ^ int(f), 0] = 1.0
    return data


# ---------------------------------------------------------------- bit patterns
def wide_sites(dims):
    top = max(dims)
    return [i for i in range(len(dims) - 1) if max(dims[i], dims[i + 1]) == top]


def make_bits(pattern, nb, dims, key):
    """(nb, n) uint8.  Plain patterns hold 0 / 1, the m_* patterns also 2 (the site is summed)."""
    n, rng = len(dims) - 1, _rng("bits", pattern, nb, tuple(dims), key)
    name, _, arg = pattern.partition(":")
    r, i = np.arange(nb)[:, None], np.arange(n)[None, :]
    if name in ("random", "m_none"):
        b = rng.integers(0, 2, size=(nb, n))
    elif name == "zeros":
        b = np.zeros((nb, n))
    elif name == "ones":
        b = np.ones((nb, n))
    elif name == "split":                                  # the first k queries all 0, the others all 1: halves of k / nb - k rows
        b = (r >= int(arg)) + 0 * i
    elif name == "alt":                                    # ... and the two halves swap at every site
        b = (i + (r >= int(arg))) % 2
    elif name == "equal":
        b = np.repeat(rng.integers(0, 2, size=(1, n)), nb, axis=0)
    elif name == "m_all":
        b = np.full((nb, n), 2)
    elif name == "m_random":
        b = rng.integers(0, 3, size=(nb, n))
    elif name in ("m_first", "m_last"):
        b = rng.integers(0, 2, size=(nb, n))
        b[:, 0 if name == "m_first" else n - 1] = 2
    elif name == "m_wide":                                 # 2 at the wide sites; every third row without any 2; row 1 all 2
        b = rng.integers(0, 2, size=(nb, n))
        b[:, wide_sites(dims)] = 2
        b[0::3] = rng.integers(0, 2, size=b[0::3].shape)
        b[1] = 2
    else:
        raise KeyError(pattern)
    return np.ascontiguousarray(b, dtype=np.uint8)


# ---------------------------------------------------------------- working precisions
def exact(t):
    """The operand in longdouble."""
    return np.asarray(t).astype(CLD if np.iscomplexobj(t) else LD)


def modulus(t):
    """|re| + |im| of the operand, in longdouble: the operand of the magnitude."""
    t = np.asarray(t)
    return (np.abs(t.real) + np.abs(t.imag)).astype(LD)


def plain(t):
    """The operand as it is: float64 / complex128 numpy arithmetic, the oracle that stands in for the device."""
    return np.asarray(t)


def _unique_rows(bits):
    u, inv = np.unique(np.asarray(bits), axis=0, return_inverse=True)
    return u, np.asarray(inv).reshape(-1)


# ---------------------------------------------------------------- the contractions (amplitude NOT applied)
def chain_values(data, bits, work):
    """prod_i A_i[:, bit_i, :] per row of bits, a bit of 2 taking the sum of the two slices."""
    ub, inv = _unique_rows(bits)
    sites = [work(t) for t in data]
    v = np.ones((len(ub), 1), dtype=np.result_type(*[s.dtype for s in sites]))
    for i, A in enumerate(sites):
        nv = np.empty((len(ub), A.shape[2]), dtype=v.dtype)
        for b in (0, 1, 2):
            sel = ub[:, i] == b
            if sel.any():
                nv[sel] = v[sel] @ (A[:, b, :] if b < 2 else A[:, 0, :] + A[:, 1, :])
        v = nv
    return v[:, 0][inv]


def lazy_values(wdata, adata, bits, work):
    """<bits| W psi>: M'[b, beta] = sum_{s'} sum_{a, alpha} W[a, s', bit, b] M[a, alpha] A[alpha, s', beta], W first."""
    ub, inv = _unique_rows(bits)
    Ws, As = [work(t) for t in wdata], [work(t) for t in adata]
    dt = np.result_type(Ws[0].dtype, As[0].dtype)
    M = np.ones((len(ub), 1, 1), dtype=dt)                                     # [q, a, alpha]
    for i, (W, A) in enumerate(zip(Ws, As)):
        (Dl, _, _, Dr), (cl, _, cr) = W.shape, A.shape
        nM = np.empty((len(ub), Dr, cr), dtype=dt)
        A2 = np.ascontiguousarray(A.transpose(1, 0, 2)).reshape(2 * cl, cr).astype(dt)   # [(s', alpha), beta]
        for b in (0, 1):
            sel = ub[:, i] == b
            ns = int(sel.sum())
            if ns == 0:
                continue
            Wb = np.ascontiguousarray(W[:, :, b, :].reshape(Dl, 2 * Dr).T).astype(dt)    # [(s', b), a]
            X = np.matmul(Wb[None], M[sel])                                     # [q, (s', b), alpha]
            X = np.ascontiguousarray(X.reshape(ns, 2, Dr, cl).transpose(0, 2, 1, 3)).reshape(ns, Dr, 2 * cl)
            nM[sel] = np.matmul(X, A2[None])
        M = nM
    return M[:, 0, 0][inv]


def dense_tensor(data, work):
    """T[s_1, ..., s_n]."""
    T = work(data[0])[0]
    for A in data[1:]:
        T = np.tensordot(T, work(A), axes=([-1], [0]))
    return T[..., 0]


def dense_apply(wdata, T, work):
    """(W psi)[out bits] from the dense psi[in bits]: one site of W at a time (the bond of W travels in front)."""
    n = len(wdata)
    R = T[None]                                                                 # [a, s_1 .. s_n]
    for i, W in enumerate(wdata):
        # R[a, o_1 .. o_{i-1}, s_i .. s_n]: contract (a, s_i) with W[a, s_i, o_i, b] -> [o_1 .. o_{i-1}, s_{i+1} .., o_i, b]
        R = np.tensordot(R, work(W), axes=([0, i + 1], [0, 1]))
        R = np.moveaxis(R, [-1, -2], [0, i + 1])
    assert R.shape == (1,) + (2,) * n
    return R[0]


def block_of(T, spec, reverse):
    """mps_block read off the dense tensor: fixed sites indexed, summed sites summed, the free ones kept in chain order with the
    first one as the most significant bit (reverse: the least)."""
    T = T[tuple(slice(None) if s >= 2 else int(s) for s in spec)]
    kept = [s for s in spec if s >= 2]
    summed = tuple(j for j, s in enumerate(kept) if s == 2)
    if summed:
        T = T.sum(axis=summed)
    T = np.asarray(T)
    if reverse:
        T = T.transpose(tuple(range(T.ndim - 1, -1, -1)))
    return np.ascontiguousarray(T).reshape(-1)


def grid_of(T, ks, ls):
    """chi[k, l] = T[interleave(lsb(k), lsb(l))] of a paired chain's dense tensor."""
    n = T.ndim // 2
    out = np.empty((len(ks), len(ls)), dtype=T.dtype)
    for x, k in enumerate(ks):
        for y, l in enumerate(ls):
            idx = []
            for i in range(n):
                idx += [(int(k) >> i) & 1, (int(l) >> i) & 1]
            out[x, y] = T[tuple(idx)]
    return out


def laplace_of(T, ks, dt):
    """dt sqrt(N) sum_j T[interleave(lsb(k), j)]."""
    n = T.ndim // 2
    S = T.sum(axis=tuple(range(1, 2 * n, 2)))                                   # main bits, chain order
    vals = np.array([S[tuple((int(k) >> i) & 1 for i in range(n))] for k in ks], dtype=T.dtype)
    if T.dtype in (np.dtype(LD), np.dtype(CLD)):
        return LD(dt) * np.sqrt(LD(2) ** n) * vals
    return dt * np.sqrt(2.0 ** n) * vals


# ---------------------------------------------------------------- the rounding bound
def gamma(q):
    return LD(q * U) / (1 - LD(q * U))


def q_of(k):
    return k + 8 + 1 + k


def growth(qs):
    g = LD(1)
    for q in qs:
        g = g * (1 + gamma(q))
    return g * (1 + 2 * LD(U)) - 1


def chain_qs(dims):
    return [q_of(dims[i]) for i in range(len(dims) - 1)]


def lazy_qs(adims, wdims):
    return [q for i in range(len(adims) - 1) for q in (q_of(wdims[i]), q_of(2 * adims[i]))]


def block_qs(dims):
    return [q_of(max(dims[i], dims[i + 1])) for i in range(len(dims) - 1)] + [q_of(max(dims))]


def sweep_qs(adims, wdims):
    return [q_of(adims[i] * wdims[i]) + 2 for i in range(len(adims) - 1)]


def bound(mag, qs, amplitude=AMPLITUDE):
    return abs(amplitude) * np.asarray(mag, dtype=LD) * growth(qs)


Ref = namedtuple("Ref", "value bound")


def check(got, ref, what=""):
    """Every entry of `got` within its own bound of the reference; returns the worst err / bound."""
    got, value = np.asarray(got), np.asarray(ref.value)
    assert got.shape == value.shape, (what, got.shape, value.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(CLD) - value.astype(CLD)).astype(LD)
    bad = np.flatnonzero((err > ref.bound).reshape(-1))
    assert bad.size == 0, (what, f"{bad.size} of {err.size} outside their bound; first at {bad[0]}: got {got.reshape(-1)[bad[0]]!r}, "
                                 f"reference {value.reshape(-1)[bad[0]]!r}, bound {float(np.asarray(ref.bound).reshape(-1)[bad[0]]):.3e}")
    ok = np.asarray(ref.bound) > 0
    return float((err[ok] / np.asarray(ref.bound)[ok]).max()) if ok.any() else 0.0


def rel(a, b):
    """The project's batch-relative error (tests/test_gpu_parity.py)."""
    return float(np.abs(np.asarray(a) - np.asarray(b).astype(C64)).max() / max(1e-300, np.abs(np.asarray(b).astype(C64)).max()))


def worst_relative(got, ref):
    """max_q |got_q - ref_q| / |ref_q|: meaningful on cone data, where no coefficient is a cancelled sum."""
    v = np.asarray(ref.value).astype(CLD).reshape(-1)
    err = np.abs(np.asarray(got).astype(CLD).reshape(-1) - v).astype(LD)
    return float((err / np.abs(v).astype(LD)).max())


# ---------------------------------------------------------------- the table
CHAIN15 = (2, 3, 5, 9, 17, 33, 65, 127, 64, 31, 16, 7, 3, 1, 2)   # every lane-group width 1 .. 64, chi_l > 64, odd chi_r, a bond of 1
SORT_A = (2, 4, 8, 130, 128, 8, 4, 2)
SORT_B = (2, 4, 16, 33, 127, 16, 4, 2)
LAZY_PSI, LAZY_W = (2, 3, 7, 16, 5, 1, 2), (4, 9, 1, 12, 6, 3, 2)
RAGGED_PSI, RAGGED_W = (2, 4, 8, 16, 33, 64, 37, 4, 2), (4, 16, 40, 40, 29, 40, 16, 4, 2)
BLOCK_BONDS = (2, 4, 8, 40, 130, 33, 8, 4, 2)
GRID_BONDS = (2, 4, 8, 16, 32, 16, 8, 4, 2)                         # a paired chain of n = 5: ten tensors
GRID_N = 5
SWEEP_PSI = (2, 4, 8, 8, 8, 4, 2)
SWEEP_OPS = {"narrow_c": ("c64", (4, 8, 8, 8, 8, 8, 4)), "narrow_r": ("f64", (4, 8, 8, 8, 8, 8, 4)),      # product bond 64
             "wide_c": ("c64", (4, 16, 16, 16, 16, 16, 4)), "wide_r": ("f64", (4, 16, 16, 16, 16, 16, 4))}  # product bond 128
SWEEP_NB = 64
MULTIPASS_NB = 32768 + 37
LAPLACE_DT = 0.3


def _threshold_bonds(top):
    return (2, 4, 8, top, 8, 4, 2)


def _chain_cases():
    rows = []                                              # (name, verb, route, bonds, nb, pattern)
    for nb in (1, 3, 300):
        rows.append((f"chain15_nb{nb}", "plain", "CHAIN", CHAIN15, nb, "random"))
    for pat in ("m_all", "m_none", "m_first", "m_last", "m_random"):
        rows.append((f"chain15_{pat}", "marginal", "CHAIN", CHAIN15, 300, pat))
    for label, bonds in (("one_site", ()), ("two_sites", (3,))):
        rows.append((f"{label}_plain", "plain", "CHAIN", bonds, 3, "random"))
        rows.append((f"{label}_marginal", "marginal", "CHAIN", bonds, 3, "m_random"))
    # the thresholds, both sides, through both verbs
    for nb, top, gemm in ((3, 128, False), (4, 128, True), (4, 127, False), (1023, 16, False), (1024, 16, True), (1024, 15, False)):
        rows.append((f"threshold_nb{nb}_bond{top}_plain", "plain", "GEMM_SORTED" if gemm else "CHAIN", _threshold_bonds(top), nb,
                     "random"))
        rows.append((f"threshold_nb{nb}_bond{top}_marginal", "marginal", "GEMM_SELECT" if gemm else "CHAIN", _threshold_bonds(top),
                     nb, "m_random"))
    # the sorted form: every split of the queries the plan can produce
    for label, bonds, nb, pats in (("sortA", SORT_A, 4, ("random", "equal")),
                                   ("sortA", SORT_A, 49, ("random", "split:1", "alt:1")),
                                   ("sortA", SORT_A, 97, ("random", "zeros", "ones", "split:48", "alt:48", "alt:97", "equal")),
                                   ("sortB", SORT_B, 1024, ("random", "zeros", "ones", "split:48", "alt:49", "alt:1024", "equal")),
                                   ("sortB", SORT_B, 1500, ("random", "split:1", "alt:750"))):
        for pat in pats:
            rows.append((f"{label}_nb{nb}_{pat.replace(':', '')}", "plain", "GEMM_SORTED", bonds, nb, pat))
    # the selecting form: marginals with the wide sites summed
    for label, bonds, nb in (("selectA", SORT_A, 4), ("selectA", SORT_A, 97), ("selectB", SORT_B, 1024)):
        rows.append((f"{label}_nb{nb}_m_wide", "marginal", "GEMM_SELECT", bonds, nb, "m_wide"))
    rows.append(("selectA_nb97_m_none", "marginal", "GEMM_SELECT", SORT_A, 97, "m_none"))
    return [Case(f"{name}-{dt}-{fam}", "chain", verb, route, dt, fam, dict(bonds=bonds, nb=nb, pattern=pat))
            for name, verb, route, bonds, nb, pat in rows for dt in DTYPES for fam in FAMILIES]


PAIRS = (("f64", "f64"), ("c64", "f64"), ("f64", "c64"), ("c64", "c64"))     # (W, psi)
SAME = (("f64", "f64"), ("c64", "c64"))


def _lazy_cases():
    rows = []                                              # (name, route, psi bonds, W bonds, nb, pairs, families)
    for nb in (1, 15, 200):
        rows.append((f"lazy_small_nb{nb}", "LAZY_CHAIN", LAZY_PSI, LAZY_W, nb, PAIRS, FAMILIES))
    rows.append(("lazy_ragged_nb15", "LAZY_CHAIN", RAGGED_PSI, RAGGED_W, 15, SAME, FAMILIES))          # wide and few
    rows.append(("lazy_31x33_nb200", "LAZY_CHAIN", (31, 31), (33, 33), 200, SAME, FAMILIES))           # chi D = 1023
    rows.append(("lazy_32x32_nb15", "LAZY_CHAIN", (32, 32), (32, 32), 15, SAME, FAMILIES))
    rows.append(("lazy_32x32_nb16", "LAZY_GEMM", (32, 32), (32, 32), 16, PAIRS, FAMILIES))
    rows.append(("lazy_ragged_nb200", "LAZY_GEMM", RAGGED_PSI, RAGGED_W, 200, SAME, FAMILIES))
    rows.append((f"lazy_multipass_nb{MULTIPASS_NB}", "LAZY_GEMM", (32, 32), (32, 32), MULTIPASS_NB, (("c64", "f64"),), ("cone",)))
    return [Case(f"{name}-W{wd}-psi{ad}-{fam}", "lazy", "lazy", route, "c64" if "c64" in (wd, ad) else "f64", fam,
                 dict(bonds=ab, wbonds=wb, nb=nb, wdtype=wd, adtype=ad))
            for name, route, ab, wb, nb, pairs, fams in rows for wd, ad in pairs for fam in fams]


def block_specs():
    """(label, spec) for the ten-tensor chain of BLOCK_BONDS: 0 / 1 fixed, 2 summed, 3 free."""
    n, rng = len(BLOCK_BONDS) + 1, _rng("block specs")
    other = lambda size: rng.integers(0, 3, size=size)
    specs = [("all_free", np.full(n, 3)), ("none_free", other(n))]
    s = other(n)
    s[:4] = 3
    specs.append(("free_prefix", s))
    s = other(n)
    s[-4:] = 3
    specs.append(("free_suffix", s))
    s = other(n)
    s[0::2] = 3
    specs.append(("alternating", s))
    for i in range(n):
        s = other(n)
        s[i] = 3
        specs.append((f"one_free_at_{i}", s))
    for j in range(12):
        specs.append((f"random_{j}", rng.integers(0, 4, size=n)))
    # the wide sites 3 - 5 fixed, summed and in the right fold, whatever the draws above gave
    specs.append(("wide_fixed", np.array([3, 3, 2, 1, 0, 1, 3, 2, 3, 0])))
    specs.append(("wide_summed", np.array([3, 0, 3, 2, 2, 2, 1, 3, 3, 2])))
    specs.append(("wide_in_right_fold", np.array([3, 2, 3, 0, 2, 1, 2, 0, 1, 2])))
    specs.append(("wide_in_right_fold_swapped", np.array([2, 3, 1, 2, 1, 2, 0, 2, 1, 0])))
    return [(label, np.ascontiguousarray(s, dtype=np.uint8)) for label, s in specs]


def grid_axes():
    """(label, ks, ls) of coefficient_grid on the n = 5 paired chain: every block 2^a x 2^b with start bits 0 / 1 that fits
    the register (the dense fast path), and permuted index sets (the per-query path)."""
    out, rng = [], _rng("grid axes")
    for a in range(GRID_N + 1):
        for b in range(GRID_N + 1):
            for sk in (0, 1):
                for sl in (0, 1):
                    if sk + a <= GRID_N and sl + b <= GRID_N and not (a == 0 and sk) and not (b == 0 and sl):
                        out.append((f"a{a}b{b}sk{sk}sl{sl}", np.arange(2 ** a) << sk, np.arange(2 ** b) << sl))
    for a, b in ((1, 1), (2, 5), (5, 3), (5, 5), (3, 0)):
        ks, ls = rng.permutation(2 ** a), rng.permutation(2 ** b)
        if b == 0:
            ls = np.array([3, 3])                          # a repeated point instead of a one-point block
        out.append((f"permuted_a{a}b{b}", ks, ls))
    out.append(("gapped", np.array([0, 5, 6, 31, 17]), np.array([30, 1, 1, 8])))
    return out


def laplace_axes():
    """(label, ks): the full low ranges take the dense block read-out, the others one marginal chain per value."""
    out = [(f"low_a{a}", np.arange(2 ** a)) for a in range(GRID_N + 1)]
    out.append(("reversed", np.arange(32)[::-1].copy()))
    out.append(("gapped", np.array([0, 7, 8, 31, 2, 2])))
    return out


def _front_end_cases():
    cases = []
    for dt in DTYPES:
        for fam in FAMILIES:
            for paired in (False, True):
                cases.append(Case(f"block_{'paired' if paired else 'plain'}-{dt}-{fam}", "block", "block", None, dt, fam,
                                  dict(bonds=BLOCK_BONDS, paired=paired)))
            cases.append(Case(f"grid-{dt}-{fam}", "grid", "grid", None, dt, fam, dict(bonds=GRID_BONDS)))
            cases.append(Case(f"laplace-{dt}-{fam}", "laplace", "laplace", None, dt, fam, dict(bonds=GRID_BONDS)))
    return cases


SWEEP_LISTS = {                                            # name: operators of SWEEP_OPS, in call order
    "nw1": ("wide_c",),
    "nw3": ("narrow_c", "wide_r", "narrow_r"),             # under nw = 4: one operator after the other
    "nw4": ("narrow_r", "wide_c", "narrow_c", "wide_r"),   # from nw = 4: concurrent, each operator in a slot of its own
    "nw9": ("narrow_c", "wide_c", "narrow_r", "wide_r", "wide_c#2", "narrow_c#2", "wide_r#2", "narrow_r#2", "narrow_c#3"),
    "repeated": ("narrow_c", "wide_r", "narrow_c", "wide_c", "wide_r"),     # one handle twice: not distinct, no slots
}


def _sweep_cases():
    return [Case(f"sweep_{name}-psi{dt}-{fam}", "sweep", "sweep", None, dt, fam, dict(bonds=SWEEP_PSI, ops=ops, nb=SWEEP_NB))
            for name, ops in SWEEP_LISTS.items() for dt in DTYPES for fam in FAMILIES]


CHAIN_CASES, LAZY_CASES, FRONT_END_CASES, SWEEP_CASES = _chain_cases(), _lazy_cases(), _front_end_cases(), _sweep_cases()
CASES = CHAIN_CASES + LAZY_CASES + FRONT_END_CASES + SWEEP_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------- operands and references of a case
def operands(c):
    """chain: (psi data, bits); lazy: (W data, psi data, bits); block / grid / laplace: psi data; sweep: (psi data, {op: W data},
    bits)."""
    p = c.p
    if c.kind == "chain":
        return mps_data(c.family, c.dtype, p["bonds"], "chain"), make_bits(p["pattern"], p["nb"], dims_of(p["bonds"]), c.name)
    if c.kind == "lazy":
        n = len(p["bonds"]) + 1
        if p["nb"] == MULTIPASS_NB:                        # eight configurations, each many times
            bits = np.ascontiguousarray(_rng("multipass").integers(0, 2, size=(p["nb"], n)), dtype=np.uint8)
        else:
            bits = make_bits("random", p["nb"], dims_of(p["bonds"]), c.name)
        return mpo_data(c.family, p["wdtype"], p["wbonds"], "lazy"), mps_data(c.family, p["adtype"], p["bonds"], "lazy", 2), bits
    if c.kind == "sweep":
        ops = {}
        for name in p["ops"]:
            dt, wb = SWEEP_OPS[name.split("#")[0]]
            ops[name] = mpo_data(c.family, dt, wb, name)
        return mps_data(c.family, c.dtype, p["bonds"], "sweep", 2), ops, make_bits("random", p["nb"], dims_of(p["bonds"]), "sweep")
    return mps_data(c.family, c.dtype, p["bonds"], c.kind)


def sweep_dtype(c, op):
    return "c64" if "c64" in (c.dtype, SWEEP_OPS[op.split("#")[0]][0]) else "f64"


@functools.lru_cache(maxsize=None)
def _dense(family, dtype, bonds, key, share, which):
    return dense_tensor(mps_data(family, dtype, bonds, key, share), exact if which == "value" else modulus)


def _ref(value, mag, qs):
    return Ref(AMPLITUDE * value, bound(mag, qs))


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = BY_NAME[name]
    p = c.p
    if c.kind == "chain":
        data, bits = operands(c)
        return _ref(chain_values(data, bits, exact), chain_values(data, bits, modulus), chain_qs(dims_of(p["bonds"])))
    if c.kind == "lazy":
        w, a, bits = operands(c)
        return _ref(lazy_values(w, a, bits, exact), lazy_values(w, a, bits, modulus), lazy_qs(dims_of(p["bonds"]), dims_of(p["wbonds"])))
    dense = lambda which: _dense(c.family, c.dtype, p["bonds"], c.kind, 2 if c.kind == "sweep" else 1, which)
    if c.kind == "block":
        qs = block_qs(dims_of(p["bonds"]))
        return {(label, rev): _ref(block_of(dense("value"), s, rev), block_of(dense("mag"), s, rev), qs)
                for label, s in block_specs() for rev in (False, True)}
    if c.kind == "grid":
        qs = block_qs(dims_of(p["bonds"]))
        return {label: _ref(grid_of(dense("value"), ks, ls), grid_of(dense("mag"), ks, ls), qs) for label, ks, ls in grid_axes()}
    if c.kind == "laplace":
        qs = block_qs(dims_of(p["bonds"])) + [3]
        return {label: _ref(laplace_of(dense("value"), ks, LAPLACE_DT), laplace_of(dense("mag"), ks, LAPLACE_DT), qs)
                for label, ks in laplace_axes()}
    if c.kind == "sweep":
        _, ops, bits = operands(c)
        idx = tuple(bits.T.astype(np.intp))
        out = {}
        for op, w in ops.items():
            qs = sweep_qs(dims_of(p["bonds"]), dims_of(SWEEP_OPS[op.split("#")[0]][1]))
            out[op] = _ref(dense_apply(w, dense("value"), exact)[idx], dense_apply(w, dense("mag"), modulus)[idx], qs)
        return out
    raise KeyError(c.kind)


def reference(c):
    """chain / lazy: a Ref over the queries; block: {(spec label, reverse): Ref}; grid / laplace: {axes label: Ref}; sweep:
    {operator: Ref}.  Computed once per case and shared; do not modify."""
    return _reference(c.name)


def all_two_row_reference(c):
    """An all-2 row of a marginal batch is the sum of the dense tensor: (value, magnitude) with the amplitude applied."""
    data, _ = operands(c)
    return AMPLITUDE * dense_tensor(data, exact).sum(), AMPLITUDE * dense_tensor(data, modulus).sum()


# ---------------------------------------------------------------- the float64 oracle that stands in for the device
def oracle_result(c):
    """What a correct float64 implementation returns for the case, in the layout of reference(c)."""
    p = c.p
    if c.kind == "chain":
        data, bits = operands(c)
        return AMPLITUDE * chain_values(data, bits, plain)
    if c.kind == "lazy":
        w, a, bits = operands(c)
        return AMPLITUDE * lazy_values(w, a, bits, plain)
    if c.kind == "sweep":
        a, ops, bits = operands(c)
        T, idx = dense_tensor(a, plain), tuple(bits.T.astype(np.intp))
        return {op: AMPLITUDE * dense_apply(w, T, plain)[idx] for op, w in ops.items()}
    T = dense_tensor(operands(c), plain)
    if c.kind == "block":
        return {(label, rev): AMPLITUDE * block_of(T, s, rev) for label, s in block_specs() for rev in (False, True)}
    if c.kind == "grid":
        return {label: AMPLITUDE * grid_of(T, ks, ls) for label, ks, ls in grid_axes()}
    return {label: AMPLITUDE * laplace_of(T, ks, LAPLACE_DT) for label, ks in laplace_axes()}
