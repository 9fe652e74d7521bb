"""GPU tests of the one-factor SVD of the gauge sweeps (svd_trunc_dev with absorb = 1 / 2 and no singular values asked for:
svd_left_mid, svd_left_deflated, svd_left_deflated_wide and certify_no_truncation of csrc/qil_linalg.hip, svd_trunc_lowrank and
the >= 640-column certificate of csrc/qil_truncate.hip), one operand at a time, through canonicalize!.

tests/gauge_cases.py builds, for every case of its table, a chain whose sweep puts one chosen matrix M in front of that SVD
(see there), in both sweep directions; tests/test_gauge_cases_oracle.py checks the table on the CPU.  Every case runs twice:
once with QIL_SVD_DEBUG set -- the route the library prints must be the one the code's rules imply for M
(gauge_cases.predicted), which contains the label the case is aimed at -- and once without it, for the numbers.  Debug mode
synchronises after every phase, so the two runs must also agree in every bond dimension.

Assertions on the plain run (gauge_cases.check_result; the reference is LAPACK's SVD of M on the host, r its kept rank):
  1. the new bond has dimension exactly r;
  2. every swept site is an isometry, max |Q^H Q - 1| < 1e-11 (the figure test_compress_rank_deficient_bonds_take_the_deflated_svd
     asks of these routes); the site behind the neighbour is bit-identical to what was uploaded;
  3. the singular values of the neighbouring site are LAPACK's: max |delta| < 1e-12 sigma_1 (the contract of test_svd_*);
  4. the state: |v - v_ref|_2 <= tol |M|_F with tol = 1e-12, plus sqrt(min(1e-6 cutoff, 1e-18)) on `cut` and `deficient` --
     the amplitude of the weight that the header of qil_compress allows the deflation to drop, and nothing more;
  5. the amplitude is unchanged.
The largest measured values per route are printed by the last test of the table and recorded in MEASUREMENTS.md."""
import gc
import importlib

import numpy as np
import pytest

import oracle as O
import gauge_cases as G
from helpers import saturated_profile

pytestmark = pytest.mark.gpu

IDS = [c.name for c in G.CASES]
SEEN = {}                # (direction, case name) -> (events, rounds, bond dimensions) of the debug run
MEASURED = {}            # (direction, case name) -> (isometry defect, singular-value deviation, state deviation)


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    gc.collect()
    assert qil.default_context().unowned_bytes() == 0


def _sweep(qil, c, direction, up):
    psi = (qil.ZTMPS if c.paired else qil.SignalMPS)(up, amplitude=G.AMPLITUDE)
    qil.canonicalize(psi, direction, center=G.center(c, direction), cutoff=c.cutoff, maxdim=c.maxdim)
    return psi


def _debug_run(qil, c, direction, up, monkeypatch, capfd):
    """The sweep with QIL_SVD_DEBUG set: (events, rounds, bond dimensions)."""
    monkeypatch.setenv("QIL_SVD_CERT", "1" if c.cert else "0")
    monkeypatch.setenv("QIL_SVD_DEBUG", "1")
    capfd.readouterr()
    try:
        bonds = _sweep(qil, c, direction, up).bond_dims
        qil.default_context().synchronize()
    finally:
        monkeypatch.delenv("QIL_SVD_DEBUG")
    text = capfd.readouterr().err
    SEEN[(direction, c.name)] = G.parse_debug(text, c.m, c.k) + (bonds,)
    return SEEN[(direction, c.name)] + (text,)


@pytest.mark.parametrize("direction", G.DIRECTIONS)
@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_one_operand(qil, c, direction, monkeypatch, capfd):
    up = G.chain(c, direction)
    events, rounds, bonds, text = _debug_run(qil, c, direction, up, monkeypatch, capfd)
    psi = _sweep(qil, c, direction, up)                                  # QIL_SVD_CERT stays as the case sets it
    assert psi.bond_dims == bonds, (psi.bond_dims, bonds)
    sites = psi.to_host()
    amplitude = psi.amplitude
    del psi
    MEASURED[(direction, c.name)] = iso, dsig, dv = G.check_result(c, direction, sites, up, amplitude)
    print(f"{c.name} {direction}: {'+'.join(events)} {rounds or '-'}  isometry {iso:.2e}  sigma {dsig:.2e}  state {dv:.2e} "
          f"(tol {G.state_tolerance(c):.1e})")
    want_events, want_rounds, _ = G.predicted(c.name)
    assert c.route in events and events == want_events, (c.route, events, want_events, text[-3000:])
    assert rounds == want_rounds, (rounds, want_rounds)


def test_every_route_was_reached_in_both_directions_for_each_dtype(qil, monkeypatch, capfd):
    """Each label of gauge_cases.LABELS is seen on the device for f64 and for c64 in a right and in a left sweep (run alone,
    this test makes the debug runs itself)."""
    for direction in G.DIRECTIONS:
        for c in G.CASES:
            if (direction, c.name) not in SEEN:
                _debug_run(qil, c, direction, G.chain(c, direction), monkeypatch, capfd)
    missing = [(label, dt, direction) for label in G.LABELS for dt in G.DTYPES for direction in G.DIRECTIONS
               if not any(label in SEEN[(direction, c.name)][0] for c in G.CASES if c.dtype == dt)]
    assert not missing, missing
    # f64 sweeps take the Gram rounds, complex ones the vector rounds with 1 .. 9 rows per lane
    for direction in G.DIRECTIONS:
        assert {SEEN[(direction, c.name)][1] for c in G.CASES if c.dtype == "f64"} == {None, "gram"}
        assert {SEEN[(direction, c.name)][1] for c in G.CASES if c.dtype == "c64"} == {None, "vector"}
        kms = {(min(c.m, c.k) + 63) // 64 for c in G.CASES if SEEN[(direction, c.name)][1] == "vector"}
        assert kms == set(range(1, 10)), kms
    # what the table measured, per route (the primary label a case is aimed at) and dtype
    print("route           dtype cases  isometry  sigma     state")
    for label in G.LABELS:
        for dt in G.DTYPES:
            rows = [MEASURED[(d, c.name)] for d in G.DIRECTIONS for c in G.CASES
                    if c.route == label and c.dtype == dt and (d, c.name) in MEASURED]
            if rows:
                print(f"{label:15s} {dt}   {len(rows):4d}   " + "  ".join(f"{max(r[j] for r in rows):.2e}" for j in range(3)))


# ---------------------------------------------------------------- canonicalize! itself
def _chain_cls(qil, paired):
    return (qil.ZTMPS, O.ZTMPS) if paired else (qil.SignalMPS, O.SignalMPS)


def _left_isometry(t):
    q = t.reshape(-1, t.shape[2])
    return float(np.abs(q.conj().T @ q - np.eye(q.shape[1])).max())


def _right_isometry(t):
    q = t.reshape(t.shape[0], -1)
    return float(np.abs(q @ q.conj().T - np.eye(q.shape[0])).max())


@pytest.mark.parametrize("paired", [False, True], ids=["mps", "ztmps"])
@pytest.mark.parametrize("dtype", ["f64", "c64"])
def test_canonicalize_to_every_kind_of_center(qil, dtype, paired):
    """right to c, then left to c: mixed canonical form around site c (1-based; for a ZTMPS c counts the 2n-tensor chain), the
    state preserved to 1e-12, the bonds the oracle's."""
    N = 10
    a = G.planted_chain(saturated_profile(N, 40), dtype, "center")
    v = G.dense(a)
    dev, ora = _chain_cls(qil, paired)
    for c in (1, 2, 5, 6, N - 1, N):
        psi, ref = dev([t.copy() for t in a], amplitude=G.AMPLITUDE), ora([t.copy() for t in a], amplitude=G.AMPLITUDE)
        for direction in G.DIRECTIONS:
            qil.canonicalize(psi, direction, center=c)
            O.canonicalize(ref, direction, center=c)
        assert psi.bond_dims == [t.shape[2] for t in ref.data[:-1]], c
        s = psi.to_host()
        assert max([_left_isometry(t) for t in s[:c - 1]] + [0.0]) < 1e-11, c
        assert max([_right_isometry(t) for t in s[c:]] + [0.0]) < 1e-11, c
        # the centre carries the norm: it is no isometry unless the chain is a single site wide there
        assert abs(np.linalg.norm(s[c - 1]) - np.linalg.norm(v)) < 1e-12 * np.linalg.norm(v), c
        assert np.linalg.norm(G.dense(s) - v) <= 1e-12 * np.linalg.norm(v), c
        assert psi.amplitude == G.AMPLITUDE


@pytest.mark.parametrize("paired", [False, True], ids=["mps", "ztmps"])
def test_sweeps_that_end_where_they_begin_change_nothing(qil, paired):
    a = G.planted_chain(saturated_profile(10, 40), "c64", "noop")
    L = importlib.import_module("qilaplace_jl_amd._lib")
    psi = _chain_cls(qil, paired)[0]([t.copy() for t in a], amplitude=G.AMPLITUDE)
    qil.canonicalize(psi, "right", center=1)
    qil.canonicalize(psi, "left", center=10)
    s = psi.to_host()
    assert len(s) == len(a) and all(np.array_equal(x, y) for x, y in zip(s, a))
    for direction in G.DIRECTIONS:
        for center in (-1, 11):
            with pytest.raises(L.QilDomainError, match="Center out of range"):
                qil.canonicalize(psi, direction, center=center)
    assert all(np.array_equal(x, y) for x, y in zip(psi.to_host(), a))


@pytest.mark.parametrize("direction", G.DIRECTIONS)
@pytest.mark.parametrize("dtype", ["f64", "c64"])
def test_binding_maxdim_gives_the_oracles_bonds_and_state(qil, dtype, direction):
    """A cap that binds: three bonds of 32 carry 12 directions of amplitude 1 and 20 of amplitude 1e-3 (weight 1e-6), maxdim = 12 cuts at the gap."""
    bonds = saturated_profile(12, 32)
    a = G.planted_chain(bonds, dtype, "cap", plant=((4, 20, 1e-3), (5, 20, 1e-3), (6, 20, 1e-3)))
    if direction == "left":
        a = G.mirror(a)
    psi, ref = qil.SignalMPS([t.copy() for t in a]), O.SignalMPS([t.copy() for t in a])
    qil.canonicalize(psi, direction, maxdim=12)
    O.canonicalize(ref, direction, maxdim=12)
    got = psi.bond_dims
    assert got == ref.bond_dims and max(got) == 12 and got != bonds
    v, want = G.dense(psi.to_host()), G.dense(ref.data)
    assert np.linalg.norm(v - want) <= 1e-9 * np.linalg.norm(want)            # the project's figure for truncated states
    assert 1e-5 * np.linalg.norm(want) < np.linalg.norm(want - G.dense(a))    # ... and the cap did cut something


def test_allocation_failures_leave_the_state_of_a_sorted_operand(qil, monkeypatch):
    """canonicalize! of the graded_shuffled case of 300 columns -- the route that sorts the columns of its operand in place --
    with the j-th allocation failing, j = 0, 1, ... until the call succeeds: every failing call raises MemoryError, strands no
    temporary and leaves a chain with the SAME dense state to 1e-12 |v| (the case is lossless: the finished gauge steps
    change nothing and the interrupted one must not have touched the chain)."""
    c = G.BY_NAME["graded_shuffled-512x300-f64"]
    assert "sorted" in G.predicted(c.name)[0]
    ctx = qil.default_context()
    up = G.chain(c, "right")
    v = G.dense(up)
    failures, done = 0, False
    for j in range(2000):
        psi = qil.SignalMPS(up, amplitude=G.AMPLITUDE)
        ctx.fail_alloc_after(j)
        try:
            qil.canonicalize(psi, "right", center=G.center(c, "right"), cutoff=c.cutoff)
            done = True
        except MemoryError:
            failures += 1
        finally:
            ctx.fail_alloc_after(None)
        if done:
            break
        assert ctx.unowned_bytes() == 0, j
        dv = np.linalg.norm(G.dense(psi.to_host()) - v)
        assert dv <= 1e-12 * np.linalg.norm(v), (j, dv)
        del psi
    assert done and failures >= 20, (done, failures)          # (the sweep of 10 sites allocates far more often than that)
    G.check_result(c, "right", psi.to_host(), up, psi.amplitude)
    again = _sweep(qil, c, "right", up)                       # and the call works afterwards
    G.check_result(c, "right", again.to_host(), up, again.amplitude)
