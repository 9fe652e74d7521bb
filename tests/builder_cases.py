"""Cases and yardsticks for the tests of the operator builders (host only: numpy and the oracle; no GPU, no library).

The device builders (csrc/qil_build_persist.hip, qil_build_chain.hip, qil_build.hip, qil_build_zt.hip) run the algorithm of two
independent host restatements: `oracle.build_*` and `qilaplace_jl_amd.builders.*_tensors`.  A comparison with a closed form sees
the truncation error of the algorithm (about 1e-7 at cutoff 1e-14); a comparison of two runs of the SAME algorithm sees rounding
only, provided both make the same truncation decisions.  This file supplies what such a comparison needs:

  diff_norm(A, B)        |A - B|_F / |B|_F of two operators given as site tensors, without dense matrices;
  decision_margin(build) how far the closest truncation decision of a host build lies from its threshold;
  CASES                  the table: builder, n, damping values, cutoff, maxdim, the route the device takes, and why it is there.
Every case is required (tests/test_builder_cases_oracle.py) to have a decision margin of MARGIN_FLOOR at least, so that the
device and the oracle keep the same columns and their bond dimensions can be compared for equality."""
from dataclasses import dataclass

import numpy as np

import oracle as O

MARGIN_FLOOR = 1e-3      # a tail at 1e-14 of the weight sits at 1e-7 sigma_max; L^2 roundings of 2^-53 move it by <~ 1e-6 relative
FACTOR = 32.0            # Jacobi against LAPACK, another summation order: the allowance over the host-against-host yardstick
EPS = 2.0 ** -53


# ---------------------------------------------------------------- the norm of a difference
def _sweep_norm(chain):
    """Frobenius norm of the operator of a chain of site tensors: QR sweep left to right, |R| of the last site."""
    R = np.ones((1, 1))
    for t in chain[:-1]:
        t = np.tensordot(R, t, axes=([1], [0]))
        R = np.linalg.qr(t.reshape(t.shape[0] * 4, t.shape[3]), mode="r")
    return float(np.linalg.norm(np.tensordot(R, chain[-1], axes=([1], [0]))))


def difference_chain(A, B):
    """Site tensors of A - B as the direct sum of the two chains: the first site joined along the right bond, the last as
    [a; -b] along the left bond, block-diagonal in between."""
    if len(A) != len(B):
        raise ValueError("difference_chain: chains of different length")
    L = len(A)
    dt = np.result_type(*[t.dtype for t in A], *[t.dtype for t in B])
    if L == 1:
        return [np.asarray(A[0], dtype=dt) - np.asarray(B[0], dtype=dt)]
    out = []
    for i, (a, b) in enumerate(zip(A, B)):
        if i == 0:
            out.append(np.concatenate([a.astype(dt), b.astype(dt)], axis=3))
        elif i == L - 1:
            out.append(np.concatenate([a.astype(dt), -b.astype(dt)], axis=0))
        else:
            t = np.zeros((a.shape[0] + b.shape[0], 2, 2, a.shape[3] + b.shape[3]), dtype=dt)
            t[:a.shape[0], :, :, :a.shape[3]] = a
            t[a.shape[0]:, :, :, a.shape[3]:] = b
            out.append(t)
    return out


def diff_norm(A, B):
    """|A - B|_F / |B|_F for two site-tensor lists W[a, s_in, s_out, b] whose bond dimensions may differ.  Gauge-invariant and
    blind to zero padding.  (The three inner products <A|A> + <B|B> - 2 <A|B> bottom out at 6e-10 even in longdouble; the
    orthogonal sweep of the direct sum resolves 1e-15.)"""
    return _sweep_norm(difference_chain(A, B)) / _sweep_norm(list(B))


def frob_norm(A):
    return _sweep_norm(list(A))


def bonds_of(W):
    return [int(t.shape[3]) for t in W[:-1]]


# ---------------------------------------------------------------- truncation decisions
def decision_margin(build):
    """Run `build()` (a host builder of qilaplace_jl_amd.builders) with the truncation rule `builders._keep` wrapped; return
    (result, margin, truncations): margin is the tightest relative distance of any decision from its threshold thr = cutoff *
    total -- (thr - d_r) / thr where the rule dropped a column (d_r the discarded weight) and (d_{r-1} - thr) / thr where it
    kept one (d_{r-1} the weight it would have discarded with the next column).  Tails below 1e-3 thr are the exact zeros of
    rank-deficient bonds and decide nothing; a cap `maxdim` that binds is no decision of the cutoff."""
    import qilaplace_jl_amd.builders as Bd
    keep = Bd._keep
    box = {"margin": np.inf, "calls": 0}

    def wrapped(S, cutoff, maxdim):
        r = keep(S, cutoff, maxdim)
        box["calls"] += 1
        P = np.asarray(S, dtype=np.float64) ** 2
        if cutoff is None or len(P) <= 1 or P[0] <= 0:
            return r
        thr = cutoff * (P.sum() or 1.0)
        if thr <= 0:
            return r
        d_r = float(P[r:].sum())
        if d_r >= 1e-3 * thr and (maxdim is None or r < min(len(P), maxdim)):
            box["margin"] = min(box["margin"], (thr - d_r) / thr)        # dropped by the cutoff: d_r <= thr
        if r > 1:
            box["margin"] = min(box["margin"], (d_r + float(P[r - 1]) - thr) / thr)
        return r

    Bd._keep = wrapped
    try:
        res = build()
    finally:
        Bd._keep = keep
    return res, float(box["margin"]), box["calls"]


# ---------------------------------------------------------------- the table
@dataclass(frozen=True)
class Case:
    name: str
    builder: str             # "dt" | "qft" | "ztq" (the paired QFT chain of build_zt_mpo) | "zt"
    n: int
    wrs: tuple = ()          # damping values (one build each on the host; one batch on the device)
    cutoff: float = 1e-14
    maxdim: int = 1000
    route: str = "persistent"   # dt: persistent | launches | dcap8 | overflow;  qft, ztq: persistent | generic;  zt: verb | parts | host
    host_cutoff: float = None   # the cutoff of the host builds where it differs (cutoff 0 on the device: 1e-30 on the host)
    why: str = ""

    @property
    def sites(self):
        return self.n if self.builder == "qft" else 2 * self.n


def _dt(name, n, wrs, why, **kw):
    return Case(name, "dt", n, tuple(float(w) for w in np.atleast_1d(wrs)), why=why, **kw)


MIXED70 = tuple(float(w) for w in np.random.default_rng(70).permutation(
    np.concatenate([np.linspace(0.03, 0.5, 35), np.linspace(0.6, 12.0, 30), [0.0, 0.1707, 0.2292, 0.4648, 400.0]])))

DT_CASES = [
    # ---- persistent route, bonds at the edge of the in-LDS capacity (26)
    _dt("dt-n8-bond25", 8, 0.1707, "smallest chain with bond 25: the wide Jacobi variants (cores of more than 80 rows)"),
    _dt("dt-n8-bond26", 8, 0.2292, "bond 26 = the capacity itself"),
    _dt("dt-n8-bond17", 8, 0.0369, "small damping, bond 17: just above the 16-column variants"),
    _dt("dt-n8-bond23", 8, 0.4648, "bond 23"),
    _dt("dt-n12-bond26", 12, 0.2311, "bond 26 at n = 12"),
    _dt("dt-n12-bond27", 12, 0.155, "bond 27 that stays in the persistent kernel: its plan refuses a zipped bond above 52 "
        "(pb_zip: nb > dcap), which a truncated bond of 27 need not reach"),
    _dt("dt-n24-bond25", 24, 0.2758, "the longest chain of the workload at bond 25"),
    _dt("dt-n24-bond20", 24, 1.0, "n = 24 at an ordinary damping"),
    # ---- natural overflow: a zipped bond above 52 sends the batch to the launch-per-step builder
    _dt("dt-n12-bond30-overflow", 12, 0.0409, "bond 30 exceeds the capacity: natural fallback", route="overflow"),
    _dt("dt-n24-bond30-overflow", 24, 0.0495, "natural fallback at n = 24", route="overflow"),
    _dt("dt-n12-mixed-overflow", 12, (0.2292, 0.0409), "one value over capacity takes the whole batch to the fallback",
        route="overflow"),
    # ---- the launch-per-step builder asked for, and forced through a tiny capacity
    _dt("dt-n8-bond25-launches", 8, 0.1707, "launch-per-step route on the bond-25 chain", route="launches"),
    _dt("dt-n12-bond26-launches", 12, 0.2311, "launch-per-step route at n = 12", route="launches"),
    _dt("dt-n8-padded-launches", 8, (0.0, 0.1707, 400.0), "a batch padded to a common bond profile: bonds 1, 25 and deficient",
        route="launches"),
    _dt("dt-n8-bond26-dcap8", 8, 0.2292, "forced overflow: capacity 4, every truncated bond above it", route="dcap8"),
    _dt("dt-n5-dcap8", 5, (0.75, 2.0), "forced overflow on a short chain, two values", route="dcap8"),
    # ---- edges
    _dt("dt-n1", 1, (0.0, 1.0, 6.283185307179586), "one pair of sites: no zip, no SVD"),
    _dt("dt-n2", 2, (0.5, 6.283185307179586), "the shortest chain with both parts"),
    _dt("dt-n8-wr0", 8, 0.0, "no damping: every bond is 1, every product bond rank-deficient"),
    _dt("dt-n8-wr400", 8, 400.0, "gate factors underflow to 0: rank-deficient bonds"),
    _dt("dt-n12-wr400", 12, 400.0, "the same at n = 12"),
    _dt("dt-n3-negative", 3, -0.5, "negative damping (growing gates), short chain"),
    _dt("dt-n5-negative", 5, -0.5, "negative damping at the largest n asked for"),
    _dt("dt-n8-cutoff1e-10", 8, 0.1707, "a looser cutoff", cutoff=1e-10),
    _dt("dt-n12-cutoff1e-10", 12, 0.0409, "a looser cutoff keeps the n = 12 chain inside the capacity", cutoff=1e-10),
    _dt("dt-n8-maxdim12-small", 8, 0.05, "binding maxdim = 12, small damping", maxdim=12),
    _dt("dt-n8-maxdim12", 8, 1.0, "binding maxdim = 12", maxdim=12),
    _dt("dt-n12-maxdim12-small", 12, 0.05, "binding maxdim = 12 at n = 12, small damping", maxdim=12),
    _dt("dt-n12-maxdim12", 12, 1.0, "binding maxdim = 12 at n = 12", maxdim=12),
    _dt("dt-n8-maxdim12-launches", 8, 1.0, "binding maxdim = 12 on the launch-per-step route", maxdim=12, route="launches"),
    _dt("dt-n2-cutoff0", 2, (0.5, 2.0), "cutoff 0: the device rule stops at 1e-28", cutoff=0.0, host_cutoff=1e-30),
    _dt("dt-n3-cutoff0", 3, (0.5, 2.0), "cutoff 0 at n = 3", cutoff=0.0, host_cutoff=1e-30),
    _dt("dt-n3-cutoff0-launches", 3, (0.5, 2.0), "cutoff 0 on the launch-per-step route", cutoff=0.0, host_cutoff=1e-30,
        route="launches"),
]

# batches on the persistent route: every value is its own workgroup and workspace slice, so a batch equals the single builds
# bit for bit
BATCH_N = 8
BATCH_SIZES = (1, 2, 5, 70)


def _chain_cases(builder, ns_generic):
    out = []
    for n in (1, 2, 6, 8, 12, 24):
        for route in ("persistent", "generic"):
            if route == "generic" and n > ns_generic:
                continue
            out.append(Case(f"{builder}-n{n}-{route}", builder, n, route=route, why="every chain length, both routes"))
    for n in (8, 12):
        for route in ("persistent", "generic"):
            out.append(Case(f"{builder}-n{n}-cutoff1e-15-{route}", builder, n, cutoff=1e-15, maxdim=None, route=route,
                            why="the benchmark's cutoff, no cap"))
            out.append(Case(f"{builder}-n{n}-maxdim5-{route}", builder, n, maxdim=5, route=route, why="binding maxdim = 5"))
    return out


QFT_CASES = _chain_cases("qft", 12)
ZTQ_CASES = _chain_cases("ztq", 12)

ZT_CASES = [Case(f"zt-n{n}-{route}", "zt", n, (w,), route=route,
                 why=f"the fused product and its compression at bond {chi}")
            for n, w, chi in ((4, 0.4, 50), (6, 6.283185307179586, 74), (8, 0.7, 108)) for route in ("verb", "parts", "host")]
ZT_CASES += [
    Case("zt-n4-batch2-verb", "zt", 4, (0.5, 6.283185307179586), route="verb", why="a batch of 2: chain-at-a-time compression"),
    Case("zt-n4-batch6-verb", "zt", 4, (0.25, 0.5, 1.0, 2.0, 4.0, 6.283185307179586), route="verb",
         why="a batch of 6: lock-step table launches (from 5 values on)"),
    Case("zt-n4-batch6-parts", "zt", 4, (0.25, 0.5, 1.0, 2.0, 4.0, 6.283185307179586), route="parts",
         why="the same batch from the separate entries"),
    Case("zt-n6-batch2-parts", "zt", 6, (0.5, 6.283185307179586), route="parts", why="a batch of 2 at n = 6, bonds 100 and 74"),
]

CASES = DT_CASES + QFT_CASES + ZTQ_CASES + ZT_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------- the two host implementations of a case
def _host_cutoff(c):
    return c.cutoff if c.host_cutoff is None else c.host_cutoff


def host_builds(c):
    """[site tensors] per damping value from qilaplace_jl_amd.builders (the library's own host restatement)."""
    import qilaplace_jl_amd.builders as Bd
    cut = _host_cutoff(c)
    if c.builder == "dt":
        return [Bd.dt_mpo_tensors(c.n, w, cut, c.maxdim) for w in c.wrs]
    if c.builder == "zt":
        return [Bd.zt_mpo_tensors(c.n, w, cut, c.maxdim) for w in c.wrs]
    if c.builder == "qft":
        return [Bd.qft_mpo_tensors(c.n, cut, c.maxdim)]
    Q = Bd._zt_block(1)
    for k in range(2, c.n + 1):
        Q = Bd._compress_lr(Bd._zip_lr(Bd._pad_pair(Q, np.complex128), Bd._zt_block(k)), cut, c.maxdim)
    return [Q]


def oracle_paired_qft_chain(n, cutoff, maxdim):
    """The paired-register QFT chain of the oracle's build_zt_mpo (oracle/builders.py, zt_transformer.jl:78-99)."""
    from oracle.builders import _extend_identity, _combine_down, _compress
    Q = list(O.control_Hphase_ztmps_mpo(1).data)
    for k in range(2, n + 1):
        Q = _extend_identity(Q, np.complex128)
        Q = _compress(_combine_down(Q, O.control_Hphase_ztmps_mpo(k).data), "down", cutoff, maxdim)
    return Q


def oracle_builds(c):
    """[site tensors] per damping value from the oracle."""
    cut = _host_cutoff(c)
    if c.builder == "dt":
        return [list(O.build_dt_mpo(c.n, w, cutoff=cut, maxdim=c.maxdim).data) for w in c.wrs]
    if c.builder == "zt":
        return [list(O.build_zt_mpo(c.n, w, cutoff=cut, maxdim=c.maxdim).data) for w in c.wrs]
    if c.builder == "qft":
        return [list(O.build_qft_mpo(c.n, cutoff=cut, maxdim=c.maxdim).data)]
    return [oracle_paired_qft_chain(c.n, cut, c.maxdim)]


def truncations(c):
    """T: the number of truncating SVDs of one build (each drops at most `cutoff` of the weight in front of it)."""
    n = c.n
    dt = sum(2 * k - 1 for k in range(2, n + 1)) + (n - 1) * (2 * n - 1)
    ztq = sum(2 * k - 1 for k in range(2, n + 1))
    return {"dt": dt, "qft": n * (n - 1) // 2, "ztq": ztq, "zt": dt + ztq + (2 * n - 1 if n > 1 else 0)}[c.builder]


@dataclass(frozen=True)
class Reference:
    oracle: list             # per damping value: the oracle's site tensors
    host: list               # ... and those of qilaplace_jl_amd.builders
    y: list                  # the yardstick diff_norm(host, oracle) per value
    margin: float            # decision_margin of the host builds
    calls: int               # truncation decisions seen in them


_REF = {}


def reference(c):
    """The two host implementations of a case, computed once and shared (cases that differ in the route only share one
    entry).  Callers do not modify the arrays."""
    key = (c.builder, c.n, c.wrs, _host_cutoff(c), c.maxdim)
    if key not in _REF:
        host, margin, calls = decision_margin(lambda: host_builds(c))
        ora = oracle_builds(c)
        _REF[key] = Reference(ora, host, [diff_norm(h, o) for h, o in zip(host, ora)], margin, calls)
    return _REF[key]


def bound(c, y):
    """What the device operator may differ from the oracle's by: FACTOR x the larger of the host-against-host yardstick and
    one rounding per site and layer."""
    return FACTOR * max(y, c.sites ** 2 * EPS)
