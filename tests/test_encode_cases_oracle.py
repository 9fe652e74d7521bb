"""CPU checks of tests/encode_cases.py, the table behind tests/test_gpu_encode.py: the planted signals have the spectra they
claim, no case hinges on rounding, the reference encoder agrees with the oracle, and the predicted RSVD routes are the shapes
the oracle's own recursion visits."""
import warnings

import numpy as np
import pytest

import oracle as O
import oracle.encode as OE
import encode_cases as E

IDS = [c.name for c in E.CASES]


@pytest.mark.parametrize("c", E.CASES, ids=IDS)
def test_planted_signals_have_the_spectra_they_claim(c):
    """Longdouble contraction against numpy.linalg.svd of each unfolding, 1e-12 (of the largest value, which is <= 1)."""
    n = c.maker[1]
    got = E.unfolding_spectra(E.signal(c), n)
    claim = E.claimed_spectra(c)
    assert sorted(claim) == list(range(1, n))
    for b in range(1, n):
        S = got[b - 1]
        if isinstance(claim[b], int):
            r = claim[b]
            assert (S[r:] < 1e-12).all() and S[r - 1] > E.RANK_TOL * S[0], (b, r, S[:r + 2])
        else:
            want = np.asarray(claim[b], dtype=np.float64)
            want = want / np.sqrt((want * want).sum())
            assert len(want) <= len(S), b
            assert np.abs(S[:len(want)] - want).max() < 1e-12 and (S[len(want):] < 1e-12).all(), (b, S[:len(want)], want)


def _paired_refs():
    for name, cutoff, maxdim in E.PAIRED:
        c = E.BY_NAME[name]
        kw = dict(c.ref_kwargs, cutoff=cutoff, maxdim=maxdim)
        ref = E.reference_encode(E.samples(c), **kw)
        yield c, cutoff, maxdim, ref, E.reference_paired(ref, cutoff, maxdim)


def test_no_decision_hinges_on_rounding():
    """Every cutoff decision of the table has a margin of at least 4, and `decide` is oracle.linalg.truncation_rank."""
    for c in E.CASES:
        ref = E.reference(c)
        for b, bond in enumerate(ref.bonds):
            assert bond.margin >= E.MARGIN, (c.name, b + 1, bond.margin)
            if c.method == "svd":
                assert bond.rank == O.truncation_rank(bond.spectrum, c.cutoff, c.maxdim), (c.name, b + 1)
    for c, cutoff, maxdim, ref, (_, copy_bonds) in _paired_refs():
        for b, bond in enumerate(ref.bonds + copy_bonds):
            # (a binding maxdim on a copy bond always cuts close values -- the fused site of an isometry has a flat spectrum --
            # and the split of one site touches no other: its discarded weight does not depend on the subspace kept)
            assert bond.margin >= E.MARGIN and not (bond.cluster and b < len(ref.bonds)), (c.name, maxdim, b, bond.margin)
            if c.method == "svd" or b >= len(ref.bonds):
                assert bond.rank == O.truncation_rank(bond.spectrum, cutoff, maxdim), (c.name, b)
        if maxdim is None:                       # the cutoff setting discards nothing above rounding
            assert ref.discarded + sum(b.discarded for b in copy_bonds) < 1e-20, c.name


def test_cluster_cuts_are_marked():
    """maxdim cuts inside a cluster only in cases marked `cluster` (the GPU test then compares subspace-independent
    quantities only); `exact` cases discard nothing above rounding."""
    for c in E.CASES:
        ref = E.reference(c)
        assert any(b.cluster for b in ref.bonds) == c.cluster, c.name
        if c.method == "svd" or ref.covered:
            assert (ref.discarded < 1e-20) == c.exact, (c.name, ref.discarded)
        else:
            assert not c.exact, c.name
    assert any(c.cluster for c in E.CASES)


@pytest.mark.parametrize("c", E.SVD_CASES, ids=[c.name for c in E.SVD_CASES])
def test_reference_encode_is_the_oracle_on_svd_cases(c):
    x = E.samples(c)
    ref = E.reference(c)
    psi = O.signal_mps(x, method="svd", cutoff=c.cutoff, maxdim=c.maxdim)
    if not c.cluster:                             # (inside a cluster the kept subspace, and with it later ranks, is a choice)
        assert ref.bond_dims == [t.shape[2] for t in psi.data[:-1]]
    assert abs(float(ref.amplitude) - psi.amplitude) <= 4e-16 * psi.amplitude
    # the tensor-train bound: |x_hat - rec|^2 <= sum over bonds of the discarded weight (+ the rounding of n float64 SVDs)
    rec = E.dense(ref.sites)
    err2 = float((np.abs(ref.xhat.astype(rec.dtype) - rec) ** 2).sum())
    assert err2 <= ref.discarded * (1 + 1e-9) + (50 * ref.n * np.finfo(float).eps) ** 2, (err2, ref.discarded)
    if not c.exact:
        assert err2 > 1e-20                       # ... and the case does truncate


def test_paired_references_are_the_oracles():
    for c, cutoff, maxdim, ref, (data, copy_bonds) in _paired_refs():
        if c.method != "svd":
            continue
        zt = O.signal_ztmps(E.samples(c), cutoff=cutoff, maxdim=maxdim)
        assert [t.shape[2] for t in data[:-1]] == [t.shape[2] for t in zt.data[:-1]], (c.name, maxdim)


@pytest.mark.parametrize("c", E.RSVD_CASES, ids=[c.name for c in E.RSVD_CASES])
def test_predicted_routes_are_the_shapes_the_oracle_visits(c, monkeypatch):
    """oracle.linalg.rsvd through oracle.encode's own recursion: the (m, n, l) it is called with are bisection_nodes' for the
    bonds it produced, and -- where the sketch covers the rank -- the reference's node list with the reference's bonds."""
    seen = []
    inner = OE.rsvd

    def recorder(A, **kw):
        seen.append((A.shape[0], A.shape[1], min(kw["k"] + kw["p"], *A.shape)))
        return inner(A, **kw)

    monkeypatch.setattr(OE, "rsvd", recorder)
    psi = O.signal_mps(E.samples(c), method="rsvd", cutoff=c.cutoff, maxdim=c.maxdim, k=c.k, p=c.p, q=c.q, mindim=c.mindim)
    bonds = [t.shape[2] for t in psi.data[:-1]]
    n = c.maker[1]
    nodes = E.bisection_nodes(n, c.k, c.p, bonds)
    assert seen == [(nd.m, nd.n, nd.l0) for nd in nodes]
    for nd in nodes:
        assert (nd.branch, nd.l0) == E.predict_rsvd_route(nd.m, nd.n, c.k, c.p)
    ref = E.reference(c)
    assert [nd.key[:4] for nd in ref.nodes] == [nd.key[:4] for nd in nodes]            # (uncovered cases: the ranks saturate)
    if ref.covered:
        assert ref.bond_dims == bonds
    for nd in ref.nodes:
        assert (nd.l is None) == (nd.branch == "exact")
        if nd.branch == "sketch":
            assert nd.l == (nd.l0 if nd.l0 < 8 else max(min(nd.rank, nd.l0), min(c.mindim, nd.l0)))
    assert ref.covered == ("uncovered" not in c.name)


def test_every_group_of_the_table_is_there():
    groups = {c.group for c in E.CASES}
    assert groups == {"svd", "rsvd-exact", "rsvd-sketch", "rsvd-deflated", "rsvd-concurrent"}
    sketch = [nd for c in E.RSVD_CASES for nd in E.reference(c).nodes if nd.branch == "sketch"]
    assert any(nd.l0 < 8 for nd in sketch) and any(nd.l is not None and nd.l < nd.l0 for nd in sketch)
    assert {c.q for c in E.RSVD_CASES if c.group == "rsvd-sketch"} == {0, 1, 2}
    refill = E.reference(E.BY_NAME["rsvd-refill-n12-f64"]).nodes[0]
    assert (refill.rank, refill.l) == (2, 5)
    assert all(nd.branch == "exact" for c in E.RSVD_CASES if c.group == "rsvd-exact" for nd in E.reference(c).nodes)
    for dt in ("f64", "c64"):
        assert {c.maker[1] for c in E.SVD_CASES if c.dtype == dt} >= {2, 3, 7, 10}
    assert {E.BY_NAME[name].maker[1] for name, _, _ in E.PAIRED} >= {2, 8}


def test_length_rule_is_the_oracles():
    for length, n in E.LENGTHS.items():
        assert E.length_rule(length) == n
        x = E.length_signal(length, "f64")
        if length == 1:
            # the library's own choice, n = max(1, round(log2 1)) = 1 (signal_mps_impl in csrc/qil_truncate.hip: `const int64_t n
            # = std::max<int64_t>(1, ...llround(log2(len)))`): the oracle's n = 0 has no site to put the sample on
            assert n == 1
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if n is None:
                with pytest.raises(ValueError):
                    O.array_to_tensor(x)
            else:
                xh, amp, got = O.array_to_tensor(x)
                assert got == n and len(xh) == 2 ** n and not xh[length:].any()
                mine, amp_ld, _ = E.prepare(x)
                assert abs(float(amp_ld) - amp) <= 4e-16 * amp and np.abs(mine.astype(np.float64) - xh).max() < 1e-15


def test_route_lines_parse():
    text = ("[rsvd] route m=64 n=64 l0=30 sketch l=7\n[rsvd] 4096 x 4096, l = 30: omega 0.10 ms\n"
            "[rsvd] route m=8 n=56 l0=8 exact\nsomething else\n")
    assert E.parse_routes(text) == [(64, 64, 30, "sketch", 7), (8, 56, 8, "exact", None)]
    with pytest.raises(ValueError):
        E.parse_routes("[rsvd] route m=8 n=56 l0=8 sketch\n")
    assert E.parse_routes("") == []


def test_uncovered_bounds_come_from_the_oracle():
    """The figures of MEASUREMENTS.md: the oracle's own error where the sketch does not cover the rank (8 seeds)."""
    for c in E.RSVD_CASES:
        if "uncovered" in c.name:
            worst = E.oracle_rsvd_error(c)
            print(f"{c.name}: oracle error {worst:.3e}, bound {max(E.UNCOVERED_MARGIN * worst, E.UNCOVERED_FLOOR):.3e}")
            assert 1e-6 < worst < 1e-1, (c.name, worst)


def test_amplitude_bound():
    assert E.sumsq_bound(2) == E.sumsq_bound(2 ** 18) < E.sumsq_bound(2 ** 19) < 6e-14
