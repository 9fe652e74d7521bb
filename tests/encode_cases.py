"""The table behind tests/test_gpu_encode.py: signals with planted tensor-train ranks, a reference encoder that reports its
truncation decisions, the route every RSVD node must take, and the cases.  No GPU import: tests/test_encode_cases_oracle.py
checks everything here on the CPU.

Signal makers (every signal is contracted densely in longdouble; site 1 is the most significant bit of the sample index):

  planted_sites      random left / right isometries around a diagonal centre.  The Schmidt values at the centre bond are the
                     prescribed ones exactly; the values claimed for the other bonds come from moving the centre bond by bond
                     (small SVDs of the centre matrix), never from the dense vector.  A site tensor with prescribed spectra on
                     BOTH of its bonds does not exist for arbitrary pairs of spectra, so this maker controls one bond.
  branch_sum         sum_j w_j (x)_i v_i[bit_i(code_j)] with a random orthonormal pair v_i[0], v_i[1] per site and
                     code_j = j | bitreverse_n(j).  Prefixes of length b of the codes agree exactly when j agrees mod 2^b, and
                     all suffixes that are long enough to hold j differ, so the Schmidt values at EVERY bond are known in closed
                     form: sqrt(sum of w_j^2 over each residue class), mirrored on the right half.  This is the maker for
                     geometric spectra, flat spectra with a cliff and clusters of equal values at the cut.
  damped_exponentials  sum of r damped complex exponentials (conjugate pairs for a real signal): TT-rank exactly r wherever the
                     cut can carry it.

reference_encode restates oracle.encode on numpy.linalg.svd with the truncation rule of oracle.linalg.svd_trunc and returns
what the oracle does not: per bond the kept rank, the spectrum, the discarded relative weight and the decision margin.
"""
from __future__ import annotations

import functools
import re
import zlib
from dataclasses import dataclass, field

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
MARGIN = 4.0          # every cutoff decision of the table is at least this factor away from flipping (same rule as gauge_cases)
RANK_TOL = 1e-9       # numerical rank of a planted operand: planted values are >= 1e-6 sigma_1, rounding noise is ~1e-16


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ld(dtype):
    return CLD if dtype == "c64" else LD


# ---------------------------------------------------------------- the length rule
def length_rule(length):
    """n of a signal of `length` samples, or None where the encoders refuse it.  n = round(log2 length), zero-fill below 2^n,
    error above (SignalConverters.jl:18-30).  length = 1 is the library's own choice: n = max(1, .), two samples, the second
    one zero (csrc/qil_truncate.hip, signal_mps_impl: `const int64_t n = std::max<int64_t>(1, llround(log2(len)))`); the
    reference has no single-site chain to offer there."""
    n = max(1, int(round(np.log2(length))))
    return n if length <= 2 ** n else None


# ---------------------------------------------------------------- makers
def _polish(Q):
    """One Newton-Schulz step in longdouble: a float64 isometry (defect 1e-16) becomes one to longdouble rounding."""
    Q = Q.astype(CLD if np.iscomplexobj(Q) else LD)
    G = Q.conj().T @ Q
    return Q @ (3 * np.eye(G.shape[0], dtype=Q.dtype) - G) / 2


def _isometry(rows, cols, dtype, rng):
    g = rng.standard_normal((rows, cols))
    if dtype == "c64":
        g = g + 1j * rng.standard_normal((rows, cols))
    return _polish(np.linalg.qr(g)[0])


def profile(n, chi):
    """Bond dimensions 1 .. n-1 of a chain of n sites capped at chi."""
    return [min(2 ** b, 2 ** (n - b), chi) for b in range(1, n)]


def planted_sites(n, chi, spectrum, centre, dtype, seed):
    """Sites (longdouble) of a chain with bond profile `profile(n, chi)`: left isometries up to bond `centre` (1-based),
    right isometries after it, diag(spectrum) on the centre bond (absorbed into site `centre`)."""
    rng = _rng("planted", n, chi, centre, dtype, seed)
    d = [1] + profile(n, chi) + [1]
    lam = np.asarray(spectrum, dtype=LD)
    assert len(lam) == d[centre], (len(lam), d[centre])
    lam = lam / np.sqrt((lam * lam).sum())
    sites = []
    for i in range(1, n + 1):
        l, r = d[i - 1], d[i]
        if i <= centre:
            A = _isometry(2 * l, r, dtype, rng).reshape(l, 2, r)
            if i == centre:
                A = A * lam[None, None, :]
        else:
            A = _isometry(2 * r, l, dtype, rng).T.reshape(l, 2, r)       # rows orthonormal: a right isometry
        sites.append(A)
    return sites


def dense(sites):
    """The vector of a chain, contracted in the precision of its sites (site 1 = most significant bit)."""
    T = sites[0].reshape(2, -1)
    for A in sites[1:]:
        T = (T @ A.reshape(A.shape[0], -1)).reshape(-1, A.shape[2])
    return T.reshape(-1)


def moved_spectra(sites, centre):
    """Schmidt values at every bond of a chain in mixed canonical form around bond `centre`, by moving the centre bond by
    bond: each step is one small SVD of the centre matrix.  Returns {bond: values}, bond = 1 .. n-1."""
    n = len(sites)
    assert 1 <= centre <= n - 1
    dt = np.complex128 if np.iscomplexobj(sites[0]) else np.float64
    sites = [A.astype(dt) for A in sites]
    out = {}
    # the centre bond itself: site `centre` holds the centre matrix on its right bond, everything left of it is an isometry
    l, _, r = sites[centre - 1].shape
    _, S, Vh = np.linalg.svd(sites[centre - 1].reshape(2 * l, r), full_matrices=False)
    out[centre] = S
    # leftward pass: the tensor W on site b carries the centre; splitting off its left bond gives bond b - 1
    W = sites[centre - 1]
    for b in range(centre, 1, -1):
        l, _, r = W.shape
        U, Sl, _ = np.linalg.svd(W.reshape(l, 2 * r), full_matrices=False)
        out[b - 1] = Sl
        W = np.einsum("asb,bc->asc", sites[b - 2], U * Sl[None, :])
    # rightward pass: the centre matrix M on bond b - 1 moves through the right isometry on site b and gives bond b
    M = S[:, None] * Vh
    for b in range(centre + 1, n):
        W = np.einsum("ab,bsc->asc", M, sites[b - 1])
        _, Sr, Vhr = np.linalg.svd(W.reshape(2 * W.shape[0], W.shape[2]), full_matrices=False)
        out[b] = Sr
        M = Sr[:, None] * Vhr
    return out


def _bitrev(j, n):
    return int(format(j, f"0{n}b")[::-1], 2)


def _local_pairs(n, dtype, rng):
    """Per site an orthonormal pair (v[0], v[1]) in longdouble: columns of [[c, -s conj(ph)], [s ph, c]]."""
    out = []
    for _ in range(n):
        th = LD(rng.uniform(0.2, np.pi / 2 - 0.2))
        ph = np.exp(CLD(1j) * LD(rng.uniform(0, 2 * np.pi))) if dtype == "c64" else LD(rng.choice([-1.0, 1.0]))
        c, s = np.cos(th), np.sin(th)
        out.append((np.array([c, s * ph], dtype=_ld(dtype)), np.array([-s * np.conj(ph), c], dtype=_ld(dtype))))
    return out


def branch_sum(n, weights, dtype, seed):
    """The signal sum_j w_j (x)_i v_i[bit_i(j | bitreverse_n(j))] (module docstring), unnormalised, in longdouble."""
    r = len(weights)
    assert r == 1 or 2 * int(np.ceil(np.log2(r))) <= n, (r, n)
    pairs = _local_pairs(n, dtype, _rng("branch", n, dtype, seed))
    x = np.zeros(2 ** n, dtype=_ld(dtype))
    for j, w in enumerate(weights):
        code = j | _bitrev(j, n)
        t = np.ones(1, dtype=_ld(dtype))
        for i in range(n):
            t = np.kron(t, pairs[i][(code >> (n - 1 - i)) & 1])
        x = x + LD(w) * t
    return x


def branch_spectra(n, weights):
    """Closed-form Schmidt values of branch_sum at bond b = 1 .. n-1 (normalised, descending)."""
    w2 = np.asarray(weights, dtype=LD) ** 2
    r = len(w2)
    bits = 0 if r == 1 else int(np.ceil(np.log2(r)))
    out = {}
    for b in range(1, n):
        keep = min(b, n - b)                      # the left (b < n/2) or right part sees j mod 2^keep, or all of j
        groups = {}
        for j in range(r):
            key = j if keep >= bits else j % (2 ** keep)
            groups[key] = groups.get(key, LD(0)) + w2[j]
        v = np.sqrt(np.array(sorted(groups.values(), reverse=True), dtype=LD) / w2.sum())
        out[b] = v.astype(np.float64)
    return out


def damped_exponentials(n, r, dtype, seed, scale=1.0):
    """sum_j a_j z_j^t, t = 0 .. 2^n - 1, |z_j| < 1: TT-rank exactly r.  A real signal takes r / 2 conjugate pairs."""
    rng = _rng("damped", n, r, dtype, seed)
    t = np.arange(2 ** n, dtype=LD)
    x = np.zeros(2 ** n, dtype=CLD)
    if dtype == "f64":
        assert r % 2 == 0
    for j in range(r if dtype == "c64" else r // 2):
        damp = LD(rng.uniform(0.5, 6.0)) / LD(2 ** n)
        freq = LD(rng.uniform(0.05, 0.45)) * 2 * LD(np.pi) * LD(2.0) ** (-int(rng.integers(0, max(1, n // 2))))
        a = CLD(rng.uniform(0.5, 1.5)) * np.exp(CLD(1j) * LD(rng.uniform(0, 2 * np.pi)))
        x = x + a * np.exp((-damp + CLD(1j) * freq) * t)
    x = x * LD(scale)
    return x if dtype == "c64" else (2 * x.real).astype(LD)


# ---------------------------------------------------------------- the reference encoder
def decide(S, cutoff, maxdim, mindim=1):
    """The truncation rule of oracle.linalg.svd_trunc on the spectrum S (descending), with what the oracle does not report:
    (kept rank, discarded relative weight, decision margin, cluster).  The margin is the factor by which `cutoff` would have to
    move to change the kept rank by one (inf where no cutoff could: nothing left to drop, or the tail is exactly zero).
    cluster: `maxdim` cuts between two values less than a factor MARGIN apart in weight -- the kept subspace is then a choice."""
    P = np.asarray(S, dtype=np.float64) ** 2
    n = len(P)
    if n <= 1 or P[0] <= 0.0:
        return 1, 0.0, np.inf, False
    scale = P.sum()
    cap = n if maxdim is None else min(n, int(maxdim))
    mindim = max(int(mindim), 1)
    cluster = cap < n and P[cap - 1] < MARGIN * P[cap] and P[cap] > 1e-24 * scale      # (values at rounding level are no cluster)
    r, err = cap, P[cap:].sum()
    while r > mindim and err + P[r - 1] <= cutoff * scale:
        err += P[r - 1]
        r -= 1
    r = max(r, 1)
    thr = cutoff * scale
    up = thr / P[r:].sum() if r < cap and P[r:].sum() > 0 else np.inf              # cutoff / this: the last dropped value stays
    down = P[r - 1:].sum() / thr if r > mindim and thr > 0 else np.inf             # cutoff * this: one more value goes
    return r, float(P[r:].sum() / scale), float(min(up, down)), bool(cluster)


@dataclass
class Bond:
    rank: int
    spectrum: np.ndarray
    discarded: float
    margin: float
    cluster: bool


@dataclass
class Node:
    m: int
    n: int
    l0: int
    branch: str                 # "exact" | "sketch"
    l: int | None = None        # deflated sketch width the node must report (planted-rank signals), None for exact
    rank: int | None = None     # numerical rank of the node's operand
    covered: bool = True        # exact, or the sketch is wider than the operand's rank

    @property
    def key(self):
        return (self.m, self.n, self.l0, self.branch, self.l)


@dataclass
class Ref:
    n: int
    amplitude: np.longdouble
    xhat: np.ndarray                      # normalised, zero-filled, longdouble
    sites: list
    bonds: list                           # Bond per bond 1 .. n-1
    nodes: list = field(default_factory=list)
    left_leaves: list = field(default_factory=list)    # sites (0-based) that are the left child of their parent node

    @property
    def bond_dims(self):
        return [b.rank for b in self.bonds]

    @property
    def covered(self):
        return all(nd.covered for nd in self.nodes)

    @property
    def discarded(self):
        return float(sum(b.discarded for b in self.bonds))


def prepare(x):
    """(x_hat in longdouble, amplitude in longdouble, n): the length rule, the zero-fill and the norm."""
    x = np.asarray(x)
    n = length_rule(len(x))
    if n is None:
        raise ValueError("_array_to_tensor: length of signal vector must be a power of 2")
    xl = np.zeros(2 ** n, dtype=CLD if np.iscomplexobj(x) else LD)
    xl[:len(x)] = x
    big = np.abs(xl).max()
    if not (big > 0 and np.isfinite(big)):
        raise ValueError("signal has zero or non-finite norm")
    amp = big * np.sqrt(((np.abs(xl) / big) ** 2).sum())
    return xl / amp, amp, n


def predict_rsvd_route(m, n, k, p):
    """("exact" | "sketch", l0) for an m x n operand (rsvd_rowmajor: l0 = min(k + p, m, n); exact when the sketch is as wide
    as the short side)."""
    l0 = min(k + p, m, n)
    return ("exact" if l0 == min(m, n) else "sketch"), l0


def deflated_width(l0, rank, mindim=1):
    """The width a sketch node reports: rank(M Omega) = min(rank M, l0) with probability one, refilled to mindim; nodes with
    l0 < 8 or l0 > 1024 do not deflate."""
    if not 8 <= l0 <= 1024:
        return l0
    return max(min(rank, l0), min(max(int(mindim), 1), l0), 1)


def mid_of(first, last):
    return (first + last + 1) // 2 - 1           # compress_tt (0-based); 1-based (first + last - 1) div 2, SignalConverters.jl:161


def bisection_nodes(n, k, p, bonds):
    """Every (m, n, l0, branch) node of the bisection of n sites in the order of the sequential recursion, from shapes alone:
    `bonds[b - 1]` is the dimension of bond b."""
    d = [1] + list(bonds) + [1]
    out = []

    def walk(first, last):
        if first == last:
            return
        mid = mid_of(first, last)
        m, nn = d[first] << (mid - first + 1), d[last + 1] << (last - mid)
        branch, l0 = predict_rsvd_route(m, nn, k, p)
        out.append(Node(m, nn, l0, branch))
        walk(first, mid)
        walk(mid + 1, last)

    walk(0, n - 1)
    return out


def _svd(M):
    return np.linalg.svd(M, full_matrices=False)


def reference_encode(x, method="svd", cutoff=1e-15, maxdim=None, k=20, p=10, mindim=1):
    """oracle.encode.signal_mps restated on numpy.linalg.svd, reporting every decision.  method="rsvd" walks the bisection with
    the SVD an ideal sketch gives: the leading min(l, .) values of the node's operand, l the (deflated) sketch width -- the
    bonds of the device when the sketch covers the rank at every node (Ref.covered), and the node list in every case."""
    xh, amp, n = prepare(x)
    v = xh.astype(np.complex128 if np.iscomplexobj(xh) else np.float64)
    ref = Ref(n, amp, xh, [None] * n, [None] * (n - 1))
    if n == 1:
        ref.sites[0] = v.reshape(1, 2, 1)
        return ref
    if method == "svd":
        cur = v.reshape(1, -1)
        for i in range(n - 1):
            r = cur.shape[0]
            U, S, Vh = _svd(cur.reshape(2 * r, -1))
            kk, disc, margin, cluster = decide(S, cutoff, maxdim)
            ref.bonds[i] = Bond(kk, S, disc, margin, cluster)
            ref.sites[i] = U[:, :kk].reshape(r, 2, kk)
            cur = S[:kk, None] * Vh[:kk]
        ref.sites[n - 1] = cur.reshape(cur.shape[0], 2, 1)
        return ref
    assert method == "rsvd"

    def walk(T, first, last, is_left):
        if first == last:
            ref.sites[first] = T.reshape(T.shape[0], 2, T.shape[2])
            if is_left:
                ref.left_leaves.append(first)
            return
        mid = mid_of(first, last)
        lb, rb = T.shape[0], T.shape[2]
        M = T.reshape(lb << (mid - first + 1), -1)
        branch, l0 = predict_rsvd_route(M.shape[0], M.shape[1], k, p)
        U, S, Vh = _svd(M)
        rank = int((S > RANK_TOL * S[0]).sum())
        if branch == "exact":
            node, width = Node(M.shape[0], M.shape[1], l0, branch, None, rank, True), len(S)
        else:
            width = deflated_width(l0, rank, mindim)
            node = Node(M.shape[0], M.shape[1], l0, branch, width, rank, rank < l0)
        ref.nodes.append(node)
        kk, disc, margin, cluster = decide(S[:width], cutoff, maxdim, mindim)
        ref.bonds[mid] = Bond(kk, S, disc + float((S[width:] ** 2).sum() / (S ** 2).sum()), margin, cluster)
        walk(U[:, :kk].reshape(lb, -1, kk), first, mid, True)
        walk((S[:kk, None] * Vh[:kk]).reshape(kk, -1, rb), mid + 1, last, False)

    walk(v.reshape(1, -1, 1), 0, n - 1, False)
    return ref


def reference_paired(ref, cutoff, maxdim=None):
    """oracle.encode.signal_ztmps on the sites of `ref`: (2n tensors, Bond per copy bond)."""
    data, bonds = [], []
    for A in ref.sites:
        cl, _, cr = A.shape
        T = np.zeros((cl, 2, 2, cr), dtype=A.dtype)
        T[:, 0, 0, :] = A[:, 0, :]
        T[:, 1, 1, :] = A[:, 1, :]
        U, S, Vh = _svd(T.reshape(2 * cl, 2 * cr))
        c, disc, margin, cluster = decide(S, cutoff, maxdim)
        bonds.append(Bond(c, S, disc, margin, cluster))
        data.append(U[:, :c].reshape(cl, 2, c))
        data.append((S[:c, None] * Vh[:c]).reshape(c, 2, cr))
    return data, bonds


def unfolding_spectra(v, n):
    """Singular values of every unfolding of the vector v (bond 1 .. n-1), normalised to unit weight."""
    v = np.asarray(v)
    v = v.astype(np.complex128 if np.iscomplexobj(v) else np.float64)
    out = []
    for b in range(1, n):
        S = np.linalg.svd(v.reshape(2 ** b, -1), compute_uv=False)
        out.append(S / np.sqrt((S * S).sum()))
    return out


# ---------------------------------------------------------------- the debug lines of QIL_RSVD_DEBUG
_ROUTE = re.compile(r"^\[rsvd\] route m=(\d+) n=(\d+) l0=(\d+) (exact|sketch l=(\d+))$")


def parse_routes(text):
    """The route lines of a stderr capture, in order: [(m, n, l0, branch, l or None)].  Other [rsvd] lines (the timing laps of
    large operands) are skipped; a line that starts like a route line and does not parse is an error."""
    out = []
    for line in text.splitlines():
        if not line.startswith("[rsvd] route"):
            continue
        mt = _ROUTE.match(line.strip())
        if not mt:
            raise ValueError(f"malformed route line: {line!r}")
        out.append((int(mt[1]), int(mt[2]), int(mt[3]), "exact" if mt[4] == "exact" else "sketch",
                    None if mt[4] == "exact" else int(mt[5])))
    return out


# ---------------------------------------------------------------- the cases
def geometric(r, g):
    return [g ** j for j in range(r)]


def cutoff_between(weights, keep):
    """The cutoff that keeps `keep` of the (squared, relative) weights with the same factor to spare on both sides."""
    P = np.sort(np.asarray(weights, dtype=np.float64) ** 2)[::-1]
    P = P / P.sum()
    return float(np.sqrt(P[keep:].sum() * P[keep - 1:].sum()))


@dataclass(frozen=True)
class Case:
    name: str
    group: str
    hits: str                       # what the case is there to reach
    maker: tuple                    # ("branch", n, weights, seed) | ("planted", n, chi, spectrum, centre, seed) | ("damped", n, r, seed)
    dtype: str = "f64"
    method: str = "svd"
    cutoff: float = 1e-15
    maxdim: int | None = None
    k: int = 20
    p: int = 10
    q: int = 0
    mindim: int = 1
    exact: bool = True              # nothing above rounding is discarded
    cluster: bool = False           # maxdim cuts inside a cluster: only subspace-independent quantities are compared
    route: bool = False             # check the node list in a child process
    refill: bool = False            # mindim keeps directions of rounding noise: only the root's bond and route are determined
    par_depths: tuple = ("0",)

    @property
    def kwargs(self):
        kw = dict(method=self.method, cutoff=self.cutoff, maxdim=self.maxdim)
        if self.method == "rsvd":
            kw.update(k=self.k, p=self.p, q=self.q, mindim=self.mindim)
        return kw

    @property
    def ref_kwargs(self):
        kw = dict(method=self.method, cutoff=self.cutoff, maxdim=self.maxdim)
        if self.method == "rsvd":
            kw.update(k=self.k, p=self.p, mindim=self.mindim)
        return kw


@functools.lru_cache(maxsize=None)
def _signal(maker, dtype):
    kind = maker[0]
    if kind == "branch":
        _, n, weights, seed = maker
        return branch_sum(n, weights, dtype, seed) * LD(1.7)
    if kind == "planted":
        _, n, chi, spectrum, centre, seed = maker
        return dense(planted_sites(n, chi, spectrum, centre, dtype, seed)) * LD(0.6)
    if kind == "damped":
        _, n, r, seed = maker
        return damped_exponentials(n, r, dtype, seed)
    raise KeyError(kind)


def signal(c):
    """The case's samples in longdouble (read-only: shared between tests)."""
    x = _signal(c.maker, c.dtype)
    x.setflags(write=False)
    return x


def samples(c):
    """What is handed to the encoders: the longdouble signal rounded to float64 / complex128."""
    x = signal(c)
    return x.astype(np.complex128 if c.dtype == "c64" else np.float64)


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = BY_NAME[name]
    return reference_encode(samples(c), **c.ref_kwargs)


def reference(c):
    return _reference(c.name)


def claimed_spectra(c):
    """{bond: Schmidt values the maker claims}, or {bond: rank} for damped exponentials."""
    kind = c.maker[0]
    if kind == "branch":
        return branch_spectra(c.maker[1], c.maker[2])
    if kind == "planted":
        _, n, chi, spectrum, centre, seed = c.maker
        return moved_spectra(planted_sites(n, chi, spectrum, centre, c.dtype, seed), centre)
    _, n, r, _ = c.maker
    return {b: min(2 ** b, 2 ** (n - b), r) for b in range(1, n)}


def _t(w):
    return tuple(float(v) for v in w)


def _build():
    cases = []

    def add(name, group, hits, maker, **kw):
        for dt in kw.pop("dtypes", ("f64", "c64")):
            cases.append(Case(f"{name}-{dt}", group, hits, maker, dtype=dt, **kw))

    G6 = _t(geometric(6, 0.2))
    # -- SVD sweep
    for n in (2, 3):
        add(f"svd-full-n{n}", "svd", "site_from_vh with r = 1, 2 and the last site; nothing truncated",
            ("planted", n, 2, (1.0, 0.4), 1, n))
    add("svd-rank1-n7", "svd", "bond 1 everywhere: rank-one signal", ("branch", 7, (1.0,), 1))
    for n in (7, 10):
        add(f"svd-cutoff-n{n}", "svd", "cutoff binds at every bond that can carry 4: keeps 4 of a geometric 6",
            ("branch", n, G6, n), cutoff=cutoff_between(G6, 4), exact=False)
        add(f"svd-exact-n{n}", "svd", "planted profile, rounding-level cutoff: every bond keeps its planted rank",
            ("planted", n, 6, G6, n // 2, n))
    cliff = _t([1.0] * 5 + [1e-4] * 3)
    add("svd-cliff-n7", "svd", "flat spectrum with a cliff: the cutoff falls into the cliff", ("branch", 7, cliff, 3),
        cutoff=1e-6, exact=False)
    for md, tag in ((4, "below"), (6, "equal"), (9, "above")):
        add(f"svd-maxdim-{tag}-n10", "svd", f"maxdim = {md} against planted rank 6", ("branch", 10, G6, 5), maxdim=md,
            exact=md >= 6)
    add("svd-geo-n8", "svd", "geometric 6 at every bond, rounding-level cutoff", ("branch", 8, G6, 8))
    clustered = _t([1.0, 0.5, 0.2, 0.2, 0.2, 0.2, 0.01])
    add("svd-cluster-n7", "svd", "four equal values straddle maxdim = 4", ("branch", 7, clustered, 9), maxdim=4, exact=False,
        cluster=True)
    add("svd-damped-n10", "svd", "sum of 4 damped exponentials: TT-rank 4, natural spectra", ("damped", 10, 4, 1), cutoff=1e-20)
    # -- RSVD, exact branch at every node
    add("rsvd-exact-n4", "rsvd-exact", "k + p = 4 = 2^ceil(n/2): every node exact", ("planted", 4, 4, (1.0, 0.5, 0.2, 0.1), 2, 1),
        method="rsvd", k=3, p=1, route=True)
    add("rsvd-exact-n9", "rsvd-exact", "k + p = 32 = 2^ceil(n/2): every node exact, site_from_chunk with lb, rb > 1",
        ("planted", 9, 6, G6, 4, 2), method="rsvd", k=22, p=10, route=True)
    # -- RSVD sketch without deflation
    for q in (0, 1, 2):
        add(f"rsvd-narrow-q{q}-n8", "rsvd-sketch", f"l0 = 5 < 8: no deflation, rank 3 covered, q = {q}",
            ("branch", 8, _t(geometric(3, 0.3)), 11), method="rsvd", k=3, p=2, q=q, route=True)
        add(f"rsvd-uncovered-q{q}-n8", "rsvd-sketch", f"rank 8 >= l0 = 5: the sketch truncates, q = {q}",
            ("branch", 8, _t(geometric(8, 0.3)), 12), method="rsvd", k=3, p=2, q=q, route=True, exact=False)
    # -- RSVD sketch, deflated
    for r, g in ((3, 0.1), (7, 0.1), (12, 0.5)):
        add(f"rsvd-deflated-r{r}-n12", "rsvd-deflated", f"planted rank {r} under k + p = 30: the root deflates to {r}",
            ("branch", 12, _t(geometric(r, g)), r), method="rsvd", k=20, p=10, q=1 if r == 7 else 0, route=True)
    add("rsvd-refill-n12", "rsvd-deflated", "mindim = 5 over a rank-2 signal: the deflation refills to 5 columns",
        ("branch", 12, (1.0, 0.5), 4), method="rsvd", k=20, p=10, mindim=5, route=True, refill=True)
    # -- RSVD, concurrent sub-trees
    add("rsvd-concurrent-n16", "rsvd-concurrent", "first size of compress_tt_root's level passes, planted rank 6",
        ("branch", 16, G6, 16), method="rsvd", k=20, p=10, q=1, route=True, par_depths=("0", None))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
SVD_CASES = [c for c in CASES if c.method == "svd"]
RSVD_CASES = [c for c in CASES if c.method == "rsvd"]
# the paired encoders: (case, cutoff, maxdim).  cutoff = 1e-10 discards nothing above rounding on these signals (checked on the
# CPU); maxdim = 3 binds on the main and on the copy bonds
PAIRED = tuple((name, 1e-10, md) for name, mds in (
    ("svd-full-n2-f64", (None,)), ("svd-full-n2-c64", (None,)), ("svd-geo-n8-f64", (None, 3)), ("svd-geo-n8-c64", (None, 3)),
    ("svd-exact-n7-c64", (None,)), ("rsvd-exact-n4-f64", (None,)), ("rsvd-narrow-q1-n8-f64", (None,)),
    ("rsvd-narrow-q1-n8-c64", (None,)), ("rsvd-deflated-r3-n12-f64", (None,))) for md in mds)

# the length rule: length -> n, None = error (each against round(log2 length), see length_rule)
LENGTHS = {1: 1, 2: 1, 3: 2, 4: 2, 5: None, 6: 3, 11: None, 12: 4, 1448: None, 1449: 11, 1024: 10}
# the norm: (name, n, dtype, scale).  N * ncomp = 2^18 fills sumsq_partial's grid exactly once; n = 18 complex takes two strides
NORMS = (("len2", 1, "f64", 1.0), ("len2", 1, "c64", 1.0), ("one-stride", 18, "f64", 1.0), ("one-stride", 17, "c64", 1.0),
         ("two-strides", 18, "c64", 1.0), ("tiny", 10, "f64", 1e-150), ("tiny", 10, "c64", 1e-150),
         ("huge", 10, "f64", 1e150), ("huge", 10, "c64", 1e150),
         # ... and where x^2 does leave the range of a double (samples of order 1): the norm's rescue passes
         ("underflow", 10, "f64", 1e-170), ("underflow", 10, "c64", 1e-170), ("overflow", 10, "f64", 1e155),
         ("overflow", 10, "c64", 1e155))


def length_signal(length, dtype):
    rng = _rng("length", length, dtype)
    x = rng.standard_normal(length) + (1j * rng.standard_normal(length) if dtype == "c64" else 0)
    x = x + 0.25             # no sample is zero: the zero tail is the library's
    # max |x| <= 1 (a hair below, so that the rounding of a complex division cannot lift it above): a bound stated
    # absolutely -- the zero tail's 1e-14 -- is then no looser than the relative one
    return x / (np.abs(x).max() * (1 + 2.0 ** -50))


def norm_signal(n, dtype, scale):
    """4 (f64) or 3 (c64) damped exponentials times `scale`, in longdouble; n = 1: two plain samples."""
    if n == 1:
        return (np.array([0.75, -1.25], dtype=LD) * LD(scale)) if dtype == "f64" else \
            (np.array([0.75 - 0.5j, -1.25 + 2j], dtype=CLD) * LD(scale))
    return damped_exponentials(n, 4 if dtype == "f64" else 3, dtype, 7, scale)


def sumsq_bound(count):
    """Relative error bound of the amplitude for `count` doubles (N * ncomp), from sumsq_partial and signal_mps_impl:
    each x^2 is rounded once; a thread adds ceil(count / 262144) terms in sequence (1024 blocks x 256 threads, grid stride);
    6 shuffle steps add pairs across the wave; 3 adds combine the 4 waves; the host adds 1024 partials in sequence.  All terms
    are non-negative, so the relative error of the sum is at most (number of roundings on the longest path) * u, u = 2^-53;
    the square root halves it and adds its own rounding."""
    terms = -(-count // 262144)
    u = 2.0 ** -53
    return 0.5 * (1 + terms + 6 + 3 + 1024) * u * (1 + 1e-10) + u


def oracle_rsvd_error(c, seeds=range(8)):
    """max over oracle seeds of |x - mps_to_vector(oracle.signal_mps(x, :rsvd))|_max / |x|_max at the case's (k, p, q)."""
    import oracle as O
    x = samples(c)
    worst = 0.0
    for s in seeds:
        psi = O.signal_mps(x, method="rsvd", cutoff=c.cutoff, maxdim=c.maxdim, k=c.k, p=c.p, q=c.q, mindim=c.mindim,
                           random_seed=1000 + s)
        worst = max(worst, float(np.abs(O.mps_to_vector(psi) - x).max() / np.abs(x).max()))
    return worst


# measured on the oracle (oracle_rsvd_error, 8 seeds; tests/test_encode_cases_oracle.py recomputes them): MEASUREMENTS.md
UNCOVERED_MARGIN, UNCOVERED_FLOOR = 10.0, 1e-12
