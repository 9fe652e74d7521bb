"""The builder case table (tests/builder_cases.py) without a GPU: the references of tests/test_gpu_builders.py are validated
here before the device sees them.

  * diff_norm is the dense |A - B|_F / |B|_F (helpers.dense_mpo, n <= 4), for pairs of unequal and zero-padded bonds, in another
    gauge, and it recovers a perturbation of 1e-13 planted in one site to two digits;
  * every case of the table has a decision margin of MARGIN_FLOOR at least (see builder_cases.decision_margin), and as many
    truncations as builder_cases.truncations says;
  * in every case the library's host restatement and the oracle give equal bond dimensions; their distance, the yardstick
    y(case), is printed and lies at rounding level (< 1e-11: the bound FACTOR y asked of the device stays far below 1e-9);
  * the oracle itself meets the closed forms at n = 8, 12 and 24 in sampled entries, computed in longdouble from its site
    tensors, within sqrt(T cutoff) |W|_F (T truncations, each dropping at most `cutoff` of the weight):
        DT   entry(in = |j, j>, out = interleave(bits_lsb(k), bits(j'))) = delta_{j j'} exp(-wr k j / N) / sqrt(N)
        QFT  entry(in = k, out = j) = Q_n[j, k]                                   (oracle.qn_matrix: the bit-reversed DFT)
        paired QFT chain  entry(in = |m, j>, out = |m', o>) = delta_{m m'} Q_n[o, j]
Needs the oracle and numpy, neither the library's shared object nor a GPU."""
import numpy as np
import pytest

import oracle as O
import builder_cases as B
from helpers import dense_mpo, random_mpo_data, interleave
from oracle.analytic import int_to_bits, bitrev

IDS = [c.name for c in B.CASES]
LD = np.longdouble


# ---------------------------------------------------------------- diff_norm
def _dense_ratio(A, B_):
    a, b = dense_mpo(A), dense_mpo(B_)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _regauge(W, rng):
    """The same operator in another gauge, with every inner bond zero-padded by 2."""
    out = [t.copy() for t in W]
    for i in range(len(out) - 1):
        d = out[i].shape[3]
        G = rng.standard_normal((d, d)) + 2 * np.eye(d)
        out[i] = np.tensordot(out[i], G, axes=([3], [0]))
        out[i + 1] = np.tensordot(np.linalg.inv(G), out[i + 1], axes=([1], [0]))
        out[i] = np.concatenate([out[i], np.zeros(out[i].shape[:3] + (2,), out[i].dtype)], axis=3)
        out[i + 1] = np.concatenate([out[i + 1], np.zeros((2,) + out[i + 1].shape[1:], out[i + 1].dtype)], axis=0)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
@pytest.mark.parametrize("L,ba,bb", [(1, [], []), (2, [3], [5]), (3, [2, 4], [4, 1]), (4, [4, 7, 3], [2, 5, 4]),
                                     (4, [1, 1, 1], [4, 16, 4])])
def test_diff_norm_is_the_dense_ratio(L, ba, bb, dtype):
    rng = np.random.default_rng(100 * L + len(ba) + sum(bb))
    A, Bm = random_mpo_data(ba, rng, dtype), random_mpo_data(bb, rng, dtype)
    want = _dense_ratio(A, Bm)
    assert abs(B.diff_norm(A, Bm) - want) < 1e-13 * want
    assert abs(B.frob_norm(Bm) - np.linalg.norm(dense_mpo(Bm))) < 1e-14 * B.frob_norm(Bm)
    if L > 1:
        assert abs(B.diff_norm(_regauge(A, rng), Bm) - want) < 1e-12 * want          # gauge-invariant, blind to zero padding
        assert B.diff_norm(_regauge(Bm, rng), Bm) < 1e-13                             # the same operator: rounding only


@pytest.mark.parametrize("name", ["dt-n2", "dt-n3-negative", "qft-n2-persistent", "zt-n4-verb"])
def test_diff_norm_recovers_a_planted_perturbation(name):
    """A perturbation of 1e-13 of one site of a real operator of the table, against the dense norm of the planted term alone
    (no cancellation there: the term is a chain of its own)."""
    c = B.BY_NAME[name]
    W = [t.copy() for t in B.reference(c).oracle[0]]
    P = [t.copy() for t in W]
    site = len(W) // 2
    R = np.random.default_rng(len(W)).standard_normal(W[site].shape)
    P[site] = W[site] + 1e-13 * np.linalg.norm(W[site]) / np.linalg.norm(R) * R
    bump = [t.copy() for t in W]
    bump[site] = P[site] - W[site]                                           # what was planted, after its rounding
    want = np.linalg.norm(dense_mpo(bump)) / np.linalg.norm(dense_mpo(W))
    assert 1e-14 < want < 1e-12
    got = B.diff_norm(P, W)
    assert abs(got - want) < 1e-2 * want, (got, want)
    assert B.diff_norm(W, W) == 0.0 or B.diff_norm(W, W) < 1e-15


# ---------------------------------------------------------------- the table
def test_table_covers_what_it_says():
    names = set(B.BY_NAME)
    routes = {(c.builder, c.route) for c in B.CASES}
    assert {("dt", r) for r in ("persistent", "launches", "dcap8", "overflow")} <= routes
    assert {(b, r) for b in ("qft", "ztq") for r in ("persistent", "generic")} <= routes
    assert {("zt", r) for r in ("verb", "parts", "host")} <= routes
    for b in ("qft", "ztq"):
        assert {c.n for c in B.CASES if c.builder == b and c.route == "persistent"} == {1, 2, 6, 8, 12, 24}
        assert max(c.n for c in B.CASES if c.builder == b and c.route == "generic") == 12
    assert {c.n for c in B.ZT_CASES} == {4, 6, 8} and {len(c.wrs) for c in B.ZT_CASES} >= {1, 2, 6}
    assert {"dt-n1", "dt-n2", "dt-n8-wr0", "dt-n8-wr400", "dt-n5-negative", "dt-n12-mixed-overflow"} <= names
    assert len(B.MIXED70) == 70 == len(set(B.MIXED70)) and max(B.BATCH_SIZES) == 70
    assert all(c.why for c in B.CASES)


@pytest.mark.parametrize("c", B.CASES, ids=IDS)
def test_case_is_decided_and_the_host_builders_agree(c):
    ref = B.reference(c)
    assert ref.margin >= B.MARGIN_FLOOR, ref.margin
    assert ref.calls == B.truncations(c) * max(len(c.wrs), 1)
    for h, o in zip(ref.host, ref.oracle):
        assert B.bonds_of(h) == B.bonds_of(o)
    y = max(ref.y)
    print(f"{c.name}: margin {ref.margin:.3g}, max bond {[max(B.bonds_of(o), default=1) for o in ref.oracle]}, "
          f"y {y:.2e}, bound {B.bound(c, y):.2e}")
    assert y < 1e-11


@pytest.mark.parametrize("name,maxbond", [
    ("dt-n8-bond25", 25), ("dt-n8-bond26", 26), ("dt-n8-bond17", 17), ("dt-n8-bond23", 23), ("dt-n12-bond30-overflow", 30),
    ("dt-n12-bond27", 27), ("dt-n12-bond26", 26), ("dt-n24-bond25", 25), ("dt-n24-bond30-overflow", 30),
    ("dt-n24-bond20", 20), ("dt-n8-wr0", 1), ("dt-n8-maxdim12", 12), ("dt-n12-maxdim12-small", 12),
    ("qft-n12-maxdim5-persistent", 5), ("ztq-n8-maxdim5-generic", 5), ("zt-n4-verb", 50), ("zt-n6-verb", 74), ("zt-n8-verb", 108)])
def test_cases_reach_the_bonds_they_are_named_for(name, maxbond):
    """The persistent DT kernel holds truncated bonds up to 26: the table sits on both sides of that."""
    assert max(B.bonds_of(B.reference(B.BY_NAME[name]).oracle[0])) == maxbond


# ---------------------------------------------------------------- the oracle against the closed forms
def _entry(W, bits_in, bits_out):
    """One entry of the operator in longdouble, from the site tensors."""
    ct = np.clongdouble if np.iscomplexobj(W[0]) else LD
    v = np.ones((1,), dtype=ct)
    for t, i, o in zip(W, bits_in, bits_out):
        v = v @ t[:, i, o, :].astype(ct)
    return v[0]


def _samples(n, rng, count):
    N = 2 ** n
    pick = lambda: int(rng.integers(0, N))                                          # noqa: E731
    edge = [(0, 0), (N - 1, N - 1), (1, N - 1), (N - 1, 1), (N // 2, N // 2)]
    return edge + [(pick(), pick()) for _ in range(count)]


@pytest.mark.parametrize("name", ["dt-n8-bond25", "dt-n8-bond26", "dt-n8-wr400", "dt-n12-bond26", "dt-n12-bond30-overflow",
                                  "dt-n24-bond25", "dt-n24-bond30-overflow", "dt-n24-bond20"])
def test_oracle_dt_meets_the_closed_form(name):
    c = B.BY_NAME[name]
    n, N = c.n, 2 ** c.n
    W, wr = B.reference(c).oracle[0], c.wrs[0]
    tol = np.sqrt(B.truncations(c) * c.cutoff) * B.frob_norm(W)
    rng = np.random.default_rng(n)
    worst = 0.0
    for j, k in _samples(n, rng, 40):
        jb = int_to_bits(j, n)
        for jp in (j, j ^ 1, j ^ (N >> 1), int(rng.integers(0, N))):                # j' = j and three j' != j (mostly)
            got = _entry(W, interleave(jb, jb), interleave(int_to_bits(k, n, "lsb"), int_to_bits(jp, n)))
            want = np.exp(-LD(wr) * LD(k) * LD(j) / LD(N)) / np.sqrt(LD(N)) if jp == j else LD(0)
            worst = max(worst, float(abs(got - want)))
    print(f"{name}: worst entry error {worst:.2e}, bound {tol:.2e}")
    assert worst <= tol


@pytest.mark.parametrize("name", ["qft-n8-persistent", "qft-n12-persistent", "qft-n24-persistent",
                                  "ztq-n8-persistent", "ztq-n12-persistent", "ztq-n24-persistent"])
def test_oracle_qft_chains_meet_qn_matrix(name):
    """Entries of Q_n[j, k] = exp(-2 pi i bitrev(j) k / N) / sqrt(N) (oracle.qn_matrix, checked against it below where the
    matrix fits), phase reduced mod N in integers."""
    c = B.BY_NAME[name]
    n, N = c.n, 2 ** c.n
    W = B.reference(c).oracle[0]
    tol = np.sqrt(B.truncations(c) * c.cutoff) * B.frob_norm(W)
    rng = np.random.default_rng(n)

    def q(j, k):
        ph = LD((bitrev(j, n) * k) % N) / LD(N)
        return (np.cos(2 * np.pi * ph.astype(LD)) - 1j * np.sin(2 * np.pi * ph.astype(LD))) / np.sqrt(LD(N))

    if n <= 12:
        Q = O.qn_matrix(n)
        assert all(abs(complex(q(j, k)) - Q[j, k]) < 1e-12 for j, k in _samples(n, rng, 20))
    worst = 0.0
    for j, k in _samples(n, rng, 60):
        if c.builder == "qft":
            got, want = _entry(W, int_to_bits(k, n), int_to_bits(j, n)), q(j, k)
        else:
            m = int(rng.integers(0, N))
            mp = m if (j + k) % 3 else m ^ 1                                        # a third of the samples off the diagonal
            got = _entry(W, interleave(int_to_bits(m, n), int_to_bits(k, n)), interleave(int_to_bits(mp, n), int_to_bits(j, n)))
            want = q(j, k) if mp == m else 0.0
        worst = max(worst, float(abs(got - want)))
    print(f"{name}: worst entry error {worst:.2e}, bound {tol:.2e}")
    assert worst <= tol
