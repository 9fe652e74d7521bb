"""The case table of the gauge-sweep suite: chains that put ONE chosen operand in front of the one-factor SVD of canonicalize!
(svd_trunc_dev with absorb = 1 / 2 and no singular values asked for: csrc/qil_truncate.hip), the LAPACK reference, a numpy
restatement of the route rules, and the parser of the QIL_SVD_DEBUG lines.

tests/test_gauge_cases_oracle.py (CPU) checks the table itself -- the construction, that every rank decision is unambiguous,
that the reference is stable, that the oracle's canonicalize! passes every assertion the device is held to, and that every
case lies a factor MARGIN away from every threshold its route depends on; tests/test_gpu_gauge.py RUNS the same table on the
device.  Nothing here needs a GPU or the library.

The chain (right sweep; m = 2^(i+1) rows, k columns, N = i + 3 sites):
  head     sites 0 .. i-1 are the exact identity isometries eye(2^(j+1)).reshape(2^j, 2, 2^(j+1)): all their singular values
           are 1, nothing is cut at any cutoff, and they reach site i as a unitary on its left bond only -- the operand there
           is (1 (x) G) M, with the Gram matrix, triangular factor, column norms, singular values and right singular vectors
           of M, so every data-dependent route decision is that of M;
  operand  site i = M in the library's site layout: row index (alpha, s), alpha fastest;
  tail     site i+1 = T (k x 2 x d, d = ceil(k / 2)) with orthonormal rows, the last site (d x 2 x 1) of norm 1.  T is a
           co-isometry, so the singular values of site i+1 after the sweep (r x 2d) ARE the kept singular values of M;
  sweep    canonicalize(psi, "right", center = i + 2) sweeps sites 0 .. i and stops.
The mirror chain (sites reversed, bond axes swapped, center = N - i - 1) shows the same operand to a left sweep (absorb = 1,
the transposed problem).

Operand kinds, M = U0 diag(sigma) V0^H with Haar-random U0, V0 (k = the short side; cutoff 1e-12 unless said otherwise):
  flat             sigma = linspace(1, 0.5, k): nothing cut; the certificate accepts ("QR gauge")
  cap              flat for the first r, the rest the same x 1e-3; maxdim = r: the cap binds at a gap, the certificate is off
                   (r lies between the widest head bond m / 2 and k, so the head is never capped)
  graded           sigma = logspace(0, -5, k), cutoff 1e-30: nothing cut; the triangular factor is graded ("second QR")
  graded_shuffled  graded, columns scaled over 4 decades in a random order ("columns sorted by norm")
  cut              3k/4 values on linspace(1, 0.5), k/4 at 1e-8: the tail must be cut, the certificate must decline
  keep             the same with the tail at 1e-3: the tail must be kept
  deficient        `rank` values (default k / 3) on linspace(1, 0.5), the rest exactly 0: deflated routes, low-rank sketch
A case with cert = False runs under QIL_SVD_CERT=0 (the certificate's off switch): the same operand reaches the sweeps."""
import functools
import re
import zlib
from collections import namedtuple

import numpy as np

F64, C64 = np.float64, np.complex128
DTYPES = {"f64": F64, "c64": C64}
DIRECTIONS = ("right", "left")
AMPLITUDE = 1.7
MARGIN = 4.0              # every threshold a route decision depends on is at least this factor away (test_gauge_cases_oracle.py)

# route labels, in the order events are reported
LABELS = ("general", "sorted", "rotate-R", "second-QR", "deflated", "deflated-wide", "cert-mid", "cert-640", "cert-declined",
          "lowrank", "block-jacobi")

Case = namedtuple("Case", "name kind m k dtype route cutoff maxdim cert rank paired")


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(x) for x in key).encode()))


def pow2_at_least(k):
    return 1 << max(int(k) - 1, 0).bit_length()


# ---------------------------------------------------------------- the table
def shape_class(m, k, dtype):
    """Which of the three families of csrc/qil_linalg.hip a (m x k) operand of this dtype belongs to, by shape alone:
    'general' (svd_left_mid hands it back), 'mid' (the one-factor SVD), 'big' (>= 640 columns)."""
    kk, rows, e = min(m, k), max(m, k), 16 if dtype == "c64" else 8
    if kk < 17:                                                        # svd_left_mid, `k < 17`, qil_linalg.hip:3441
        return "general"
    if kk >= 640:                                                      # svd_left_mid `k >= 640` :3441, bj_min :3887, svd_trunc_dev in qil_truncate.hip
        return "big"
    if kk < 49:                                                        # fused_below, qil_linalg.hip:3442-3449
        if ((rows | 1) * kk + (kk | 1) * kk) * e <= 150 * 1024 and rows * kk <= 1 << 19:
            return "general"
    if dtype == "c64" and 16 * ((kk + 63) // 64) * 64 * e + 128 > 150 * 1024:    # `!gbb && ...`, qil_linalg.hip:3470 (f64: Gram rounds)
        return "general"
    return "mid"


def _route(kind, m, k, dtype, cert, rank):
    """The label a case is aimed at, from its kind and shape class."""
    cls, kk = shape_class(m, k, dtype), min(m, k)
    if kind == "deficient" and kk >= 384 and rank <= 128:
        return "lowrank"                                               # svd_trunc_lowrank in qil_truncate.hip
    if cls == "general":
        return "general"
    if cls == "big":
        if kind == "cap" or not cert:
            return "block-jacobi"
        return "cert-640" if kind in ("flat", "graded") else "cert-declined"
    if kind == "deficient" and kk >= 64:
        return "deflated" if m >= k else "deflated-wide"
    if kind == "flat":
        return "cert-mid" if cert else "rotate-R"
    if kind == "cut":
        return "cert-declined"
    if kind == "graded_shuffled" and m >= k:
        return "sorted"
    return "second-QR" if m >= k else "rotate-R"


def _case(kind, k, dtype, m=None, cert=True, rank=None, paired=False):
    m = pow2_at_least(k) if m is None else m
    kk = min(m, k)
    cutoff = 1e-30 if kind.startswith("graded") else 1e-12
    maxdim = (m // 2 + kk) // 2 if kind == "cap" else None
    if kind == "deficient" and rank is None:
        rank = kk // 3
    name = f"{kind}-{m}x{k}-{dtype}" + ("" if rank is None or rank == kk // 3 else f"-rank{rank}") + \
        ("" if cert else "-nocert") + ("-zt" if paired else "")
    return Case(name, kind, m, k, dtype, _route(kind, m, k, dtype, cert, rank), cutoff, maxdim, cert, rank, paired)


# boundary pairs of the decision tree: each side carries at least `flat` and `cut`
BOUNDARIES = ((16, 17), (48, 49), (63, 64), (96, 97), (383, 384), (576, 577), (639, 640))
TALL_WIDTHS = (16, 17, 33, 48, 49, 63, 64, 65, 96, 97, 129, 300, 383, 384, 511, 512, 576, 577, 639, 640, 641, 1024)
REST_WIDTHS = (64, 97, 300, 384, 512, 640, 1024)          # where the remaining kinds go


def _build():
    c = []
    for k in TALL_WIDTHS:                                 # flat and cut at every width, both dtypes
        c += [_case(kind, k, d) for kind in ("flat", "cut") for d in DTYPES]
    c.append(_case("cut", 448, "c64"))                    # complex vector rounds with 7 rows per lane
    c += [_case("cap", k, d) for k, d in ((64, "f64"), (97, "c64"), (300, "f64"), (512, "c64"), (1024, "f64"))]
    c += [_case("graded", k, d) for k, d in ((64, "c64"), (300, "f64"), (384, "c64"), (640, "f64"))]
    c += [_case("graded", k, d, cert=False) for k, d in ((300, "c64"), (512, "f64"))]
    c += [_case("graded_shuffled", k, d) for k, d in ((97, "f64"), (300, "c64"), (300, "f64"), (383, "f64"))]
    c += [_case("graded_shuffled", 300, d, cert=False) for d in ("f64", "c64")]
    c += [_case("keep", k, d) for k, d in ((64, "f64"), (97, "c64"), (300, "c64"))]
    c += [_case("keep", k, d, cert=False) for k, d in ((300, "f64"), (512, "c64"), (512, "f64"), (640, "f64"))]
    # a kept cluster of equal singular values in front of the general SVD: the fused single-workgroup kernel (48 columns, the
    # certificate does not exist there) and the in-LDS block rounds that complex operands of 577 .. 639 columns fall back to
    c += [_case("keep", 48, "f64"), _case("keep", 48, "c64"), _case("keep", 577, "c64")]
    c += [_case("deficient", k, d) for k, d in ((64, "c64"), (97, "f64"), (300, "f64"), (300, "c64"), (384, "f64"), (384, "c64"),
                                                (512, "c64"), (640, "f64"))]
    c += [_case("deficient", k, d, rank=100) for k, d in ((512, "f64"), (512, "c64"), (1024, "f64"))]
    c += [_case("flat", k, d, cert=False) for k, d in ((97, "f64"), (300, "c64"), (512, "f64"), (640, "c64"))]
    # tall and thin: too long for the fused kernel of the general path, so 40 columns take the one-factor SVD
    c += [_case("flat", 40, "c64", m=4096), _case("cut", 40, "c64", m=4096)]
    # wide operands (m < k): the short side k' = m is a power of two, k ~ 1.1 k'
    wide = {32: (("flat", "f64"), ("cut", "c64")),
            64: (("flat", "c64"), ("cut", "f64"), ("deficient", "f64")),
            128: (("flat", "f64"), ("deficient", "c64"), ("cut", "c64")),
            256: (("cut", "c64"), ("deficient", "f64"), ("cap", "f64")),
            512: (("flat", "c64"), ("deficient", "f64"), ("cut", "f64")),
            1024: (("flat", "c64"), ("cut", "f64"))}
    for kp, kinds in wide.items():
        c += [_case(kind, kp + kp // 10, d, m=kp) for kind, d in kinds]
    c += [_case("flat", 300, "f64", m=256, cert=False), _case("flat", 140, "c64", m=128, cert=False)]
    # one paired chain (ZTMPS): `center` counts the 2n-site chain
    c.append(_case("cut", 49, "f64", paired=True))
    names = [x.name for x in c]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return tuple(c)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- operands
def _haar(n, cols, dtype, rng):
    z = rng.standard_normal((n, cols))
    if dtype == "c64":
        z = z + 1j * rng.standard_normal((n, cols))
    q, r = np.linalg.qr(z)
    d = np.diagonal(r)
    return (q * (d / np.abs(d))).astype(DTYPES[dtype])


def spectrum(c):
    """The singular values the operand is built from (graded_shuffled scales columns afterwards: not its spectrum)."""
    kk = min(c.m, c.k)
    if c.kind == "flat":
        return np.linspace(1.0, 0.5, kk)
    if c.kind == "cap":
        s = np.linspace(1.0, 0.5, kk)
        s[c.maxdim:] *= 1e-3
        return s
    if c.kind.startswith("graded"):
        return np.logspace(0.0, -5.0, kk)
    if c.kind in ("cut", "keep"):
        nt = kk // 4
        return np.concatenate([np.linspace(1.0, 0.5, kk - nt), np.full(nt, 1e-8 if c.kind == "cut" else 1e-3)])
    if c.kind == "deficient":
        return np.concatenate([np.linspace(1.0, 0.5, c.rank), np.zeros(kk - c.rank)])
    raise ValueError(c.kind)


@functools.lru_cache(maxsize=4)
def operand(name):
    """M (m x k) of the case, in the case's dtype."""
    c = BY_NAME[name]
    rng = _rng("operand", c.kind, c.m, c.k, c.dtype, c.rank)
    kk = min(c.m, c.k)
    s = spectrum(c)
    nz = int(np.count_nonzero(s))                                    # exact zeros: the factors' columns are simply absent
    M = (_haar(c.m, kk, c.dtype, rng)[:, :nz] * s[:nz]) @ _haar(c.k, kk, c.dtype, rng)[:, :nz].conj().T
    if c.kind == "graded_shuffled":
        M = M * 10.0 ** (-4.0 * rng.permutation(c.k) / (c.k - 1.0))
    M.setflags(write=False)
    return M


def site_of(M, m, k):
    """M (rows alpha + cl s, cols beta) as the site tensor A[alpha, s, beta]."""
    return np.ascontiguousarray(M.reshape(2, m // 2, k).transpose(1, 0, 2))


def matrix_of(A):
    """The inverse of site_of."""
    cl, _, k = A.shape
    return A.transpose(1, 0, 2).reshape(2 * cl, k)


def site_index(c):
    """i: the operand's site in the right chain (m = 2^(i+1))."""
    return c.m.bit_length() - 2


def head_and_tail(c):
    """(head sites 0 .. i-1, [T, last]) of the right chain."""
    i, dt = site_index(c), DTYPES[c.dtype]
    rng = _rng("tail", c.m, c.k, c.dtype)
    head = [np.eye(2 ** (j + 1), dtype=dt).reshape(2 ** j, 2, 2 ** (j + 1)) for j in range(i)]
    d = (c.k + 1) // 2
    T = _haar(2 * d, c.k, c.dtype, rng).conj().T.reshape(c.k, 2, d)          # orthonormal rows
    last = rng.standard_normal((d, 2, 1)) + (1j * rng.standard_normal((d, 2, 1)) if c.dtype == "c64" else 0.0)
    last = (last / np.linalg.norm(last)).astype(dt)
    return head, [np.ascontiguousarray(T), last]


def mirror(sites):
    """The chain read from the other end: site order reversed, the bond axes of every tensor swapped."""
    return [np.ascontiguousarray(t.transpose(2, 1, 0)) for t in reversed(sites)]


def chain_with(c, M, direction):
    head, tail = head_and_tail(c)
    sites = head + [site_of(np.asarray(M, dtype=DTYPES[c.dtype]), c.m, c.k)] + tail
    return sites if direction == "right" else mirror(sites)


def chain(c, direction):
    """The site tensors uploaded for the case."""
    return chain_with(c, operand(c.name), direction)


def center(c, direction):
    i = site_index(c)
    return i + 2 if direction == "right" else (i + 3) - i - 1


def operand_position(c, direction):
    """(index of the operand's site, index of the neighbour that absorbs the other factor) in the chain of `direction`."""
    i = site_index(c)
    return (i, i + 1) if direction == "right" else (2, 1)


def swept(c, direction):
    i = site_index(c)
    return list(range(i + 1)) if direction == "right" else list(range(2, i + 3))


def dense(sites):
    """The state vector of a chain (site 1 = most significant bit), without the amplitude."""
    T = sites[0][0]
    for A in sites[1:]:
        T = np.tensordot(T, A, axes=([-1], [0]))
    return np.ascontiguousarray(T[..., 0]).reshape(-1)


# ---------------------------------------------------------------- reference
def truncation_rank(s, cutoff, maxdim):
    import oracle as O
    return O.truncation_rank(s, cutoff, maxdim)


Reference = namedtuple("Reference", "sigma r fro v")


def _svd(M, driver):
    if driver == "gesdd":
        return np.linalg.svd(M, full_matrices=False)
    import scipy.linalg
    if M.shape[0] > M.shape[1]:                   # tall: the driver works on the triangular factor (what it costs goes with k^3)
        Q, R = np.linalg.qr(M)
        U, S, Vh = scipy.linalg.svd(R, full_matrices=False, lapack_driver=driver)
        return Q @ U, S, Vh
    return scipy.linalg.svd(M, full_matrices=False, lapack_driver=driver)


def truncated(c, driver="gesdd"):
    """(sigma, r, M_r): LAPACK's singular values of M, the kept rank and the rank-r truncation of M."""
    M = operand(c.name)
    U, S, Vh = _svd(M, driver)
    r = truncation_rank(S, c.cutoff, c.maxdim)
    return S, r, (U[:, :r] * S[:r]) @ Vh[:r]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Reference(sigma, r, |M|_F, {direction: dense state of the chain with M replaced by its rank-r truncation})."""
    c = BY_NAME[name]
    S, r, Mr = truncated(c)
    v = {d: dense(chain_with(c, Mr, d)) for d in DIRECTIONS}
    return Reference(S, r, float(np.linalg.norm(operand(name))), v)


def state_tolerance(c):
    """Assertion 4: 1e-12, plus the amplitude of the weight that the header of qil_compress allows the deflation to drop --
    sqrt(min(1e-6 cutoff, 1e-18)) -- on the kinds that have something to deflate."""
    return 1e-12 + (np.sqrt(min(1e-6 * c.cutoff, 1e-18)) if c.kind in ("cut", "deficient") else 0.0)


def check_result(c, direction, sites, uploaded, amplitude):
    """Assertions 1 to 5 on the chain a sweep left behind (`sites`: every tensor, downloaded).  Returns the measured
    (isometry defect, singular-value deviation / sigma_1, state deviation / |M|_F)."""
    ref = reference(c.name)
    pos, nb = operand_position(c, direction)
    r = sites[pos].shape[2] if direction == "right" else sites[pos].shape[0]
    assert r == ref.r, (c.name, direction, r, ref.r)                                             # 1
    iso = 0.0
    sw = swept(c, direction)
    for j in sw:                                                                                 # 2
        t = sites[j]
        q = t.reshape(-1, t.shape[2]) if direction == "right" else t.reshape(t.shape[0], -1).conj().T
        iso = max(iso, float(np.abs(q.conj().T @ q - np.eye(q.shape[1])).max()))
    assert iso < 1e-11, (c.name, direction, iso)
    for j in range(len(sites)):
        if j not in sw and j != nb:
            assert sites[j].dtype == uploaded[j].dtype and np.array_equal(sites[j], uploaded[j]), (c.name, direction, j)
    t = sites[nb]
    s = np.linalg.svd(t.reshape(r, -1) if direction == "right" else t.reshape(-1, r), compute_uv=False)
    dsig = float(np.abs(s - ref.sigma[:r]).max() / ref.sigma[0])                                 # 3
    assert dsig < 1e-12, (c.name, direction, dsig)
    dv = float(np.linalg.norm(dense(sites) - ref.v[direction]) / ref.fro)                        # 4
    assert dv <= state_tolerance(c), (c.name, direction, dv, state_tolerance(c))
    assert amplitude == AMPLITUDE                                                                # 5
    return iso, dsig, dv


# ---------------------------------------------------------------- the route rules, restated
def _triangular(M):
    """R of the thin QR with a positive diagonal (what CholeskyQR2 converges to: the factor is unique for full column rank)."""
    R = np.linalg.qr(M, mode="r")
    d = np.diagonal(R)
    return R * np.where(d == 0, 1.0, np.conj(d) / np.where(d == 0, 1.0, np.abs(d)))[:, None]


def _ratio(a, b):
    """How far a lies from the threshold b, as a factor >= 1 either way."""
    a, b = max(float(a), 1e-300), max(float(b), 1e-300)
    return max(a / b, b / a)


def _certificate(R, k, cutoff, margins, tag):
    """certify_no_truncation (qil_linalg.hip:2554-2598) on the triangular factor R."""
    fro2 = float(np.sum(np.abs(R) ** 2))
    dmin = float(np.min(np.abs(np.diagonal(R)) ** 2))
    margins[tag + ": min |r_ii|^2 against 16 cutoff |R|_F^2 k"] = _ratio(dmin, 16.0 * cutoff * fro2 * k)      # :2580
    if not dmin > 16.0 * cutoff * fro2 * k:
        return False
    inv2 = float(np.sum(np.abs(np.linalg.inv(R)) ** 2))
    margins[tag + ": 4 cutoff |R|_F^2 |R^-1|_F^2 against 1"] = _ratio(4.0 * cutoff * fro2 * inv2, 1.0)        # :2594
    return 4.0 * cutoff * fro2 * inv2 < 1.0


def _deflatable(R, k, deflate, margins, tag):
    """svd_left_deflated / _wide (qil_linalg.hip:3289-3311, :3373-3392): rows of R are dropped while their weight stays below
    deflate |R|_F^2 (smallest first); the route is taken if at most 97 % of the rows stay."""
    acc = np.cumsum(np.sort(np.sum(np.abs(R) ** 2, axis=1)))

    def taken(thr):
        r = k - int(np.searchsorted(acc, thr, side="right"))
        return 1 <= r <= 0.97 * k

    # the count of dropped rows decides, not any single row: the decision must be the same with the threshold MARGIN times
    # higher and lower
    same = taken(deflate * acc[-1] * MARGIN) == taken(deflate * acc[-1] / MARGIN) == taken(deflate * acc[-1])
    margins[tag + ": same decision with deflate MARGIN times higher and lower"] = MARGIN if same else 1.0
    return taken(deflate * acc[-1])


@functools.lru_cache(maxsize=None)
def predicted(name):
    """(events, rounds, margins): the labels the code's rules imply for the case's operand, in the order of LABELS; which
    Jacobi rounds a one-factor sweep takes ('gram', 'vector' or None); and, for every data-dependent threshold on the way,
    the factor by which the operand misses it."""
    c = BY_NAME[name]
    M = operand(name)
    m, k, kk = c.m, c.k, min(c.m, c.k)
    margins, ev = {}, set()
    tall = m >= k
    Mt = M if tall else M.conj().T                                                # the tall orientation
    cert_cutoff = c.cutoff if (c.cutoff > 0 and (c.maxdim is None or kk <= c.maxdim)) else 0.0     # cert_cutoff of svd_trunc_dev
    deflate = min(1e-6 * c.cutoff, 1e-18)                                         # deflate of svd_trunc_dev
    cls = shape_class(m, k, c.dtype)

    def done(rounds=None):
        return tuple(x for x in LABELS if x in ev), rounds, margins

    if cert_cutoff > 0 and kk >= 640:                                             # svd_trunc_dev, the certificate
        if c.cert and _certificate(_triangular(Mt), kk, cert_cutoff, margins, "certificate (>= 640)"):
            ev.add("cert-640")
            return done()
        ev.add("cert-declined")
    if kk >= 384:                                                                 # svd_trunc_lowrank
        w = reference(name).sigma ** 2
        for ks in (128, 256):
            if ks * 3 > kk:
                break
            rho = float(w[ks:].sum() / w.sum())                                   # what a sketch of ks columns must leave
            margins[f"sketch of {ks}: residual against 1e-8 cutoff"] = _ratio(max(rho, 1e-30), 1e-8 * c.cutoff)
            if rho <= 1e-8 * c.cutoff:
                ev.add("lowrank")
                return done()
            margins[f"sketch of {ks}: residual against 1e-4"] = _ratio(rho, 1e-4)
            if rho > 1e-4:
                break
    if cls != "mid":
        ev.add("block-jacobi" if cls == "big" else "general")                     # svd_impl: bj_min, qil_linalg.hip:3887-3891
        return done()
    rounds = "gram" if c.dtype == "f64" else "vector"                             # qil_linalg.hip:3465-3471
    qr2 = False
    if tall:
        if k >= 17:                                                               # columns sorted by norm, :3520-3573
            cn = np.linalg.norm(M, axis=0)
            perm = np.argsort(-cn, kind="stable")
            spread = cn[perm[0]] / max(cn[perm[-1]], 1e-300)
            disorder = float(np.abs(perm - np.arange(k)).sum() / max(1.0, k * k / 3.0))
            margins["column norms: spread against sort_grade 1e3"] = _ratio(spread, 1e3)              # sort_grade, :3537
            if spread > 1e3:
                margins["column norms: disorder against sort_disorder 0.2"] = _ratio(disorder, 0.2)   # sort_disorder, :3546
                if disorder >= 0.2:
                    ev.add("sorted")
                    M = M[:, perm]
        R = _triangular(M)
        fro2 = float(np.sum(np.abs(R) ** 2))
        grade = fro2 / (kk * max(float(np.min(np.abs(np.diagonal(R)) ** 2)), 1e-300))
        margins["grade of R's diagonal against 1e3"] = _ratio(grade, 1e3)                             # grade, :3603
        margins["grade of R's diagonal against grade_max 1e24"] = _ratio(grade, 1e24)                 # grade_max, :3620
        qr2 = 1e3 < grade < 1e24                                                                      # qr2, :3621
        if grade >= 1e24 and deflate > 0 and kk >= 64:                                                # deficient, :3630-3631
            if _deflatable(R, kk, deflate, margins, "deflation"):
                ev.add("deflated")
                return done()
    else:
        R = _triangular(Mt)
        if deflate > 0 and kk >= 64 and _deflatable(R, kk, deflate, margins, "deflation (wide)"):     # svd_left_deflated_wide, :3669
            ev.add("deflated-wide")
            return done()
    if qr2:
        ev.add("second-QR")
    if cert_cutoff > 0:                                                                               # certify_no_truncation, :3682-3704
        if c.cert and _certificate(R, kk, cert_cutoff, margins, "certificate"):
            ev.add("cert-mid")
            return done()
        ev.add("cert-declined")
    if not qr2:
        ev.add("rotate-R")
    return done(rounds)


# ---------------------------------------------------------------- QIL_SVD_DEBUG lines
_LEFT = re.compile(r"^\[svd-left\] (\d+) x (\d+): (.*)$")
_CERT = re.compile(r"^\[svd-cert\] (\d+) x (\d+) \(lda \d+\), absorb \d: (QR gauge|declined)$")
_LOWRANK = re.compile(r"^\[svd-lowrank\] (\d+) x (\d+), k = \d+: sketch accepted$")
_GENERAL = re.compile(r"^\[svd\] (\d+) x (\d+): (orientation \+ QR|block sweeps) ")
_SWEEP = re.compile(r"^\[svd-left\] (gram )?sweep \d+ \((\d+) cols")


def parse_debug(text, m, k):
    """(events, rounds) of the SVD of the (m x k) operand, from the QIL_SVD_DEBUG lines of one sweep.  The lines of the head
    sites (square, at most m / 2 wide) and of nested calls (the deflated block, the sketch's factor) carry other dimensions."""
    dims, ev = {m, k}, set()
    is_op = lambda g: {int(g[0]), int(g[1])} == dims and (m != k or g[0] == g[1])
    general = swept_ = False
    rounds = None
    for line in text.splitlines():
        line = line.strip()
        g = _LEFT.match(line)
        if g and is_op(g.groups()):
            msg = g.group(3)
            if msg.startswith("columns sorted by norm"):
                ev.add("sorted")
            elif msg.startswith("mean / min") and msg.endswith("-> second QR"):
                ev.add("second-QR")
            elif msg.startswith("deflated route (wide)"):
                ev.add("deflated-wide")
            elif msg.startswith("deflated route"):
                ev.add("deflated")
            elif msg.startswith("certificate: QR gauge"):
                ev.add("cert-mid")
            elif msg.startswith("certificate: declined"):
                ev.add("cert-declined")
            elif msg.startswith("sweeps "):
                swept_ = True
            continue
        g = _CERT.match(line)
        if g and is_op(g.groups()):
            ev.add("cert-640" if g.group(3) == "QR gauge" else "cert-declined")
            continue
        g = _LOWRANK.match(line)
        if g and is_op(g.groups()):
            ev.add("lowrank")
            continue
        g = _GENERAL.match(line)
        if g and is_op(g.groups()):
            if g.group(3) == "block sweeps":
                ev.add("block-jacobi")
            general = True
            continue
        g = _SWEEP.match(line)
        if g and int(g.group(2)) == min(m, k):
            rounds = "gram" if g.group(1) else "vector"
    if general and "block-jacobi" not in ev:
        ev.add("general")
    if swept_ and "second-QR" not in ev:
        ev.add("rotate-R")
    if not swept_:
        rounds = None
    return tuple(x for x in LABELS if x in ev), rounds


# ---------------------------------------------------------------- canonicalize! itself
def planted_chain(bonds, dtype, seed, plant=()):
    """A random chain with the internal `bonds`; plant = ((site, ntail, level), ...) scales ntail right-bond directions of a
    site by `level` (a gap in the Schmidt spectrum of that bond)."""
    from helpers import random_mps_data
    rng = _rng("planted", tuple(bonds), dtype, seed)
    a = random_mps_data(list(bonds), rng, dtype=DTYPES[dtype])
    for i, ntail, level in plant:
        cr = a[i].shape[2]
        Q = _haar(cr, cr, dtype, rng)
        s = np.ones(cr)
        s[-ntail:] = level
        a[i] = np.einsum("asb,bc->asc", a[i], (Q * s) @ Q.conj().T).astype(DTYPES[dtype])
    return a
