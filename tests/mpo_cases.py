"""The table of MPO x MPO composition cases and MPO compression cases shared by tests/test_mpo_cases_oracle.py (CPU: the oracle in
the device's place -- do the inputs keep the reference itself inside every bound?) and tests/test_gpu_mpo_ops.py (GPU: the same
assertions on qil_apply_mpo_mpo / qil_mpo_compress).  No fixtures, no GPU, no library import.

Every chain has at most 10 tensors, so helpers.dense_mpo is at most 1024 x 1024.  The references of a case (dense operator, its
singular values across every cut, the oracle's own compression) are computed once per process and shared.

The checks take the RESULT of a backend, not the backend: a composition result is `Product(data, dtype, paired, site_ids,
bond_dims)`, a compression result is the list of site tensors."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle as O
from oracle.builders import _compress
from helpers import random_mpo_data, dense_mpo

EPS = np.finfo(np.float64).eps
F, Z = np.float64, np.complex128

# ================================================================ composition
# an operand: internal bonds, element type, site labels.  A paired operand lists the labels of all its 2n tensors.
Operand = namedtuple("Operand", "bonds dtype sites")
Compose = namedtuple("Compose", "name paired first second seed")
Product = namedtuple("Product", "data dtype paired site_ids bond_dims")


def _ids(n, start=1):
    return list(range(start, start + n))


def _compose_cases():
    cases = []
    seed = 100
    ragged1, ragged2 = [3, 9, 17, 6, 4], [2, 5, 13, 7, 3]
    for paired in (False, True):
        for d1, d2 in ((F, F), (F, Z), (Z, F), (Z, Z)):
            seed += 1
            cases.append(Compose(f"ragged-{'paired' if paired else 'single'}-{np.dtype(d1).kind}{np.dtype(d2).kind}", paired,
                                 Operand(ragged1, d1, _ids(6)), Operand(ragged2, d2, _ids(6)), seed))
    cases.append(Compose("bond1-single", False, Operand([1, 1, 1], F, _ids(4)), Operand([1, 1, 1], Z, _ids(4)), 120))
    cases.append(Compose("bond1-paired", True, Operand([1, 1, 1], Z, _ids(4)), Operand([1, 1, 1], F, _ids(4)), 121))
    cases.append(Compose("one-site-both", False, Operand([], F, [5]), Operand([], Z, [5]), 122))
    cases.append(Compose("one-site-in-base", False, Operand([], Z, [3]), Operand([2, 5, 4, 3], F, _ids(5)), 123))
    # a 2-site operand at the start, middle and end of a 5-site base, in both orders, either one real: the sites outside the window are
    # copied (same type) or widened (real base, complex short operand)
    seed = 130
    for where, start in (("start", 1), ("middle", 3), ("end", 4)):
        for short_first in (True, False):
            for base_dt, short_dt in ((F, Z), (Z, F)):
                seed += 1
                short, base = Operand([3], short_dt, _ids(2, start)), Operand([2, 5, 4, 3], base_dt, _ids(5))
                first, second = (short, base) if short_first else (base, short)
                cases.append(Compose(f"embed-{where}-{'short' if short_first else 'base'}-first-base-{np.dtype(base_dt).kind}", False,
                                     first, second, seed))
    cases.append(Compose("embed-paired-middle", True, Operand([3], Z, _ids(2, 3)), Operand([2, 5, 4, 3, 2], F, _ids(6)), 150))
    cases.append(Compose("embed-paired-end-base-first", True, Operand([4, 5, 4, 3, 2], Z, _ids(6)), Operand([3], F, _ids(2, 5)), 151))
    # the middle site has 24^4 * 4 = 1 327 104 fused elements, more than the 4096 x 256 threads of the capped grid
    cases.append(Compose("grid-stride-D24", False, Operand([24, 24], F, _ids(3)), Operand([24, 24], Z, _ids(3)), 160))
    return cases


COMPOSE = _compose_cases()
# (W1 W2) psi against W2 (W1 psi): one single-register and one paired case
COMPOSE_ON_STATE = ("ragged-single-fc", "ragged-paired-cf")


@lru_cache(maxsize=None)
def compose_operands(name):
    """(w1, w2): the seeded site tensors of the two operands of the case"""
    c = next(c for c in COMPOSE if c.name == name)
    rng = np.random.default_rng(c.seed)
    return (random_mpo_data(c.first.bonds, rng, c.first.dtype), random_mpo_data(c.second.bonds, rng, c.second.dtype))


def _window(c):
    """(base operand, other operand, base_is_first, offset of the window in the base)"""
    n1, n2 = len(c.first.sites), len(c.second.sites)
    base, other = (c.first, c.second) if n1 >= n2 else (c.second, c.first)
    return base, other, n1 >= n2, base.sites.index(other.sites[0])


def compose_site_reference(t1, t2):
    """out[(a1,a2), i, o, (b1,b2)] = sum_m W1[a1,i,m,b1] W2[a2,m,o,b2], W1's bond fastest -- in longdouble, with the magnitude
    sum |W1| o |W2| the rounding bound is relative to"""
    ld = np.clongdouble if (np.iscomplexobj(t1) or np.iscomplexobj(t2)) else np.longdouble
    D1l, _, _, D1r = t1.shape
    D2l, _, _, D2r = t2.shape
    ref = np.einsum("aimb,cmod->caiodb", t1.astype(ld), t2.astype(ld)).reshape(D2l * D1l, 2, 2, D2r * D1r)
    mag = np.einsum("aimb,cmod->caiodb", np.abs(t1), np.abs(t2)).reshape(D2l * D1l, 2, 2, D2r * D1r)
    return ref, mag


def check_product_sites(name, got):
    """Site by site against longdouble.  Each element is a two-term dot product, so the bound is componentwise:
    |got - ref| <= 8 eps (|W1| o |W2|) -- gamma_2 = 2u/(1-2u) with u = eps/2 for real operands, times the 2 sqrt(2) of a complex
    product evaluated in real arithmetic, rounded up.  Outside the window the result is the base, bit for bit (widened when
    the result is complex).  Returns the largest error in units of the bound."""
    c = next(c for c in COMPOSE if c.name == name)
    w1, w2 = compose_operands(name)
    base, other, base_first, off = _window(c)
    wb = w1 if base_first else w2
    odt = np.result_type(c.first.dtype, c.second.dtype)
    assert got.dtype == odt, (got.dtype, odt)
    assert got.paired == c.paired
    assert list(got.site_ids) == list(base.sites)
    nb, no = len(base.sites), len(other.sites)
    dims = [1] + list(base.bonds) + [1]
    odims = [1] + list(other.bonds) + [1]
    for k in range(no + 1):
        dims[off + k] *= odims[k]
    assert list(got.bond_dims) == dims[1:-1], (got.bond_dims, dims[1:-1])
    assert len(got.data) == nb
    worst = 0.0
    for i in range(nb):
        g = np.asarray(got.data[i])
        assert g.shape == (dims[i], 2, 2, dims[i + 1]), (i, g.shape)
        k = i - off
        if 0 <= k < no:
            t1, t2 = (w1[i], w2[k]) if base_first else (w1[k], w2[i])
            ref, mag = compose_site_reference(t1, t2)
            err = np.abs(g.astype(ref.dtype) - ref).astype(np.float64)
            bound = 8 * EPS * mag
            assert np.all(err <= bound), (name, i, float((err - bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        else:
            assert np.array_equal(g, wb[i].astype(odt)), (name, i)
    return worst


def embed_dense(c, which):
    """the dense operator of operand `which` (0 / 1) on the base's sites: identities on the sites it does not touch"""
    base, other, base_first, off = _window(c)
    w = compose_operands(c.name)[which]
    op = (c.first, c.second)[which]
    if len(op.sites) == len(base.sites):
        return dense_mpo(w)
    eye = np.eye(2).reshape(1, 2, 2, 1)
    nb = len(base.sites)
    full = [eye] * off + list(w) + [eye] * (nb - off - len(w))
    return dense_mpo(full)


def check_product_dense(name, got):
    """dense(W1 * W2) == dense(W1) @ dense(W2) (helpers.dense_mpo is M[in, out] and W1 acts first) to 1e-13 of the product of
    norms, the project's figure for exact contractions.  Returns the error in that unit."""
    c = next(c for c in COMPOSE if c.name == name)
    m1, m2 = embed_dense(c, 0), embed_dense(c, 1)
    err = np.linalg.norm(dense_mpo(got.data) - m1 @ m2) / (np.linalg.norm(m1) * np.linalg.norm(m2))
    assert err <= 1e-13, (name, err)
    return err


def compose_state(name):
    """a seeded random state (site tensors) on the sites of the case"""
    from helpers import random_mps_data
    c = next(c for c in COMPOSE if c.name == name)
    rng = np.random.default_rng(c.seed + 1000)
    return random_mps_data([2, 4, 7, 4, 2], rng, Z)


def check_product_on_state(name, v12, v21):
    """(W1 W2) psi against W2 (W1 psi), both as dense vectors: 1e-13 of |W1| |W2| |psi|"""
    c = next(c for c in COMPOSE if c.name == name)
    w1, w2 = compose_operands(name)
    from helpers import dense_mps
    scale = np.linalg.norm(dense_mpo(w1)) * np.linalg.norm(dense_mpo(w2)) * np.linalg.norm(dense_mps(compose_state(name)))
    ref = dense_mpo(w2).T @ (dense_mpo(w1).T @ dense_mps(compose_state(name)).reshape(-1))
    for v in (v12, v21):
        assert np.linalg.norm(np.asarray(v).reshape(-1) - ref) <= 1e-13 * scale, name
    assert np.linalg.norm(np.asarray(v12).reshape(-1) - np.asarray(v21).reshape(-1)) <= 1e-13 * scale, name


# ================================================================ compression
# kind "random": seeded random sites with the given bonds; "product": the MPO x MPO product of two random operators with bonds
# `bonds` and `bonds2` (fused bonds beyond what the site count allows: rank-deficient).  Every bond index j of a random operator is
# scaled by 10^(-decay j / (D - 1)), so the spectra across the cuts decay and a cutoff of 1e-8 (on the squared weights) removes something.
# A saturated chain compounds the decay of its bonds across the middle cut, so its `decay` is gentler: the smallest singular value there has
# to stay clear of the rounding level for the lossless bond dimensions to mean something (has_gap).
Compress = namedtuple("Compress", "name kind paired dtype bonds bonds2 maxdim seed decay", defaults=(None, None, 0, 6.0))
REGIMES = [4, 16, 64, 130, 130, 130, 64, 16, 4]          # within the rank caps; (4 * 130) x 130 sites cross the SVD and QR regimes

# At cutoff 0 the oracle's two-site SVD keeps every value that is not exactly zero, so it GROWS a bond that is narrower than both of
# its neighbours' 4 D (the extra values are rounding noise); the device's one-site SVD cannot.  Bond dimensions are therefore
# comparable only for profiles that are saturated (D_k = min(4^k, 4^(N-k))) or inflated beyond that -- see has_gap -- and the table
# keeps the others (the 130-wide N = 10 profiles, one product) to a quarter of the lossless cases.
COMPRESS = [
    Compress("n2-real-single", "random", False, F, [4], maxdim=2, seed=201),
    Compress("n2-complex-paired", "random", True, Z, [4], maxdim=2, seed=202),
    Compress("n3-complex-single", "random", False, Z, [4, 4], maxdim=2, seed=203),
    Compress("n3-real-single", "random", False, F, [4, 4], maxdim=3, seed=204),
    Compress("n6-real-paired", "random", True, F, [4, 16, 64, 16, 4], maxdim=9, seed=205, decay=1.0),
    Compress("n6-complex-single", "random", False, Z, [4, 16, 64, 16, 4], maxdim=7, seed=206, decay=1.0),
    Compress("n10-complex-single-regimes", "random", False, Z, REGIMES, maxdim=24, seed=207),
    Compress("n10-real-paired-regimes", "random", True, F, REGIMES, maxdim=33, seed=208),
    # inflated past the caps 4^k: the first site is 4 x 40 ("down") and the last 40 x 4 ("up"), wider than tall
    Compress("n7-real-single-inflated", "random", False, F, [40, 40, 70, 70, 40, 40], maxdim=10, seed=209),
    Compress("n6-complex-paired-inflated", "random", True, Z, [40, 40, 70, 40, 40], maxdim=10, seed=210),
    # fused bonds 9, 30, 30, 30, 9 (the middle one below its cap of 64) and 9, 30, 64, 30, 9
    Compress("n6-complex-single-product", "product", False, Z, [3, 5, 5, 5, 3], [3, 6, 6, 6, 3], maxdim=8, seed=211),
    Compress("n6-real-paired-product", "product", True, F, [3, 5, 8, 5, 3], [3, 6, 8, 6, 3], maxdim=8, seed=212, decay=1.5),
]
DIRECTIONS = ("down", "up")
CUTOFF = 1e-8
# (mode name, cutoff, use the case's maxdim)
MODES = (("lossless", 0.0, False), ("cutoff", CUTOFF, False), ("maxdim", 0.0, True))


def compress_case(name):
    return next(c for c in COMPRESS if c.name == name)


def _decaying(bonds, rng, dtype, decay):
    data = random_mpo_data(bonds, rng, dtype)
    for k, D in enumerate(bonds):
        f = 10.0 ** (-decay * np.arange(D) / max(D - 1, 1))
        data[k] = data[k] * f[None, None, None, :]
    return data


@lru_cache(maxsize=None)
def compress_input(name):
    """the seeded site tensors of the case (treat as read-only)"""
    c = compress_case(name)
    rng = np.random.default_rng(c.seed)
    if c.kind == "random":
        data = _decaying(c.bonds, rng, c.dtype, c.decay)
    else:
        a, b = _decaying(c.bonds, rng, c.dtype, c.decay), _decaying(c.bonds2, rng, c.dtype, c.decay)
        data = O.apply_mpo_mpo(O.SingleSiteMPO(a), O.SingleSiteMPO(b)).data
    data = [np.ascontiguousarray(t) for t in data]
    for t in data:
        t.setflags(write=False)
    return tuple(data)


def caps(n):
    """the largest rank an n-tensor operator can have across each cut"""
    return [min(4 ** (k + 1), 4 ** (n - 1 - k)) for k in range(n - 1)]


@lru_cache(maxsize=None)
def dense_input(name):
    m = dense_mpo(compress_input(name))
    m.setflags(write=False)
    return m


def unfold(m, n, k):
    """dense_mpo's M[in (site 1 = MSB), out (site 1 = MSB)] as the matrix across the cut after tensor k (1-based count):
    rows (in_1, out_1, ..., in_k, out_k), columns the rest"""
    t = m.reshape((2,) * (2 * n))
    perm = [ax for j in range(n) for ax in (j, n + j)]
    return t.transpose(perm).reshape(4 ** k, 4 ** (n - k))


@lru_cache(maxsize=None)
def cut_spectra(name):
    """the exact dense operator's singular values across every cut (numpy.linalg.svd), descending"""
    m, n = dense_input(name), len(compress_input(name))
    return tuple(np.linalg.svd(unfold(m, n, k), compute_uv=False) for k in range(1, n))


@lru_cache(maxsize=None)
def oracle_compress(name, direction, mode):
    """oracle.builders._compress of the case in the given mode: the site tensors"""
    c = compress_case(name)
    _, cutoff, capped = next(m for m in MODES if m[0] == mode)
    return tuple(_compress([np.array(t) for t in compress_input(name)], direction, cutoff, c.maxdim if capped else None))


def bonds_of(data):
    return [t.shape[3] for t in data[:-1]]


def lossless_error(name, data):
    m = dense_input(name)
    return float(np.linalg.norm(dense_mpo(list(data)) - m) / np.linalg.norm(m))


@lru_cache(maxsize=None)
def oracle_lossless_error(name, direction):
    return lossless_error(name, oracle_compress(name, direction, "lossless"))


def lossless_floor(name, direction):
    """relative error a lossless compression may leave: 8 x what the oracle reaches on the same input, never below N eps"""
    return max(8 * oracle_lossless_error(name, direction), len(compress_input(name)) * EPS)


def has_gap(name, direction):
    """Can the bond dimensions of a cutoff-0 compression be compared with the oracle's?  With cutoff 0 the oracle keeps every
    singular value that is not exactly zero, so the one decision that depends on rounding is whether values at the noise level are
    kept: the oracle's two-site SVD keeps them where both neighbours are wider than the bond's true rank, the device's one-site
    SVD cannot.  The comparison is made where the smallest singular value the oracle keeps at every bond stands a factor 1e3
    clear of that level, (d eps)^2 of the squared weights for a cut of dimension d; the oracle drops nothing at cutoff 0."""
    kept = bonds_of(oracle_compress(name, direction, "lossless"))
    for s, r in zip(cut_spectra(name), kept):
        p = s * s
        if r > len(p) or p[r - 1] < 1e3 * (len(p) * EPS) ** 2 * p.sum():
            return False
    return True


def check_lossless(name, direction, data):
    """operator kept to 8 x the oracle's own error (floor N eps); bond dimensions the oracle's where the gap condition holds,
    otherwise within the rank caps and the oracle's.  Returns the relative error."""
    n = len(compress_input(name))
    got, want = bonds_of(data), bonds_of(oracle_compress(name, direction, "lossless"))
    if has_gap(name, direction):
        assert got == want, (name, direction, got, want)
    else:
        assert all(g <= min(c, w) for g, c, w in zip(got, caps(n), want)), (name, direction, got, want)
    err = lossless_error(name, data)
    assert err <= lossless_floor(name, direction), (name, direction, err, lossless_floor(name, direction))
    return err


def check_truncated(name, direction, mode, data):
    """The TT-SVD bound with nothing measured in it: |dense(got) - dense(in)|_F^2 <= (1 + 1e-8) sum_k tail_k^2 + floor^2, tail_k^2
    the weight of the exact operator's singular values beyond got's bond k.  Bonds: <= maxdim, or <= the oracle's for a cutoff."""
    c = compress_case(name)
    m = dense_input(name)
    got = bonds_of(data)
    if mode == "maxdim":
        assert all(g <= c.maxdim for g in got), (name, direction, got)
    else:
        want = bonds_of(oracle_compress(name, direction, mode))
        assert all(g <= w for g, w in zip(got, want)), (name, direction, got, want)
    tails = sum(float((s[r:] ** 2).sum()) for s, r in zip(cut_spectra(name), got))
    floor = lossless_floor(name, direction) * np.linalg.norm(m)
    err2 = float(np.linalg.norm(dense_mpo(list(data)) - m) ** 2)
    assert err2 <= (1 + 1e-8) * tails + floor ** 2, (name, direction, mode, err2, tails, floor ** 2)
    return err2, tails


def check_interrupted(name, direction, data, retried=False):
    """A compression that failed part of the way has truncated some bonds and not others: the TT-SVD bound holds for it with the
    bonds it has (a bond not yet truncated has no tail), so the operand still stands for the input.  `retried`: the same call then
    ran to its end on that operand -- a second sweep, whose projections are not orthogonal to the first's, so its errors add up
    by the triangle inequality, each still at most its tail: |dense(got) - dense(in)|_F <= sum_k tail_k + floor."""
    m = dense_input(name)
    tails = [float(np.sqrt((s[r:] ** 2).sum())) for s, r in zip(cut_spectra(name), bonds_of(data))]
    floor = lossless_floor(name, direction) * np.linalg.norm(m)
    err = float(np.linalg.norm(dense_mpo(list(data)) - m))
    bound = sum(tails) + floor if retried else np.sqrt((1 + 1e-8) * sum(t * t for t in tails) + floor ** 2)
    assert err <= bound, (name, direction, retried, err, bound)
    return err, bound


def truncation_removes_something(name, direction, mode):
    return bonds_of(oracle_compress(name, direction, mode)) != bonds_of(oracle_compress(name, direction, "lossless"))


def check_against_oracle_on_state(name, mode, data):
    """after "down": the truncated operator applied to a random state agrees with the oracle-compressed one to 1e-9 (largest
    entry, as a fraction of the largest entry of the reference)"""
    n = len(compress_input(name))
    rng = np.random.default_rng(compress_case(name).seed + 7)
    x = rng.standard_normal(2 ** n) + 1j * rng.standard_normal(2 ** n)
    ref = dense_mpo(list(oracle_compress(name, "down", mode))).T @ x
    got = dense_mpo(list(data)).T @ x
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    assert err < 1e-9, (name, mode, err)
    return err


def check_gauge(name, direction, data):
    """after "down" every site but the first is a right isometry (M M^H = I for M = (cl | 4 cr)), after "up" every site but the
    last a left isometry; 1e-10 on the largest entry"""
    worst = 0.0
    sites = list(data)[1:] if direction == "down" else list(data)[:-1]
    for t in sites:
        t = np.asarray(t)
        if direction == "down":
            mat = t.reshape(t.shape[0], -1)
            g = mat @ mat.conj().T
        else:
            mat = t.reshape(-1, t.shape[3])
            g = mat.conj().T @ mat
        worst = max(worst, float(np.abs(g - np.eye(g.shape[0])).max()))
    assert worst < 1e-10, (name, direction, worst)
    return worst
