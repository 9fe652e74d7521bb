"""The thin QR on its own: every run case of tests/qr_cases.py (tests/test_qr_plan.py pins which kernels each one reaches) goes
through qil_qr_host with reorth = 0 -- qil_dev_qr_positive WITHOUT the measure-and-repair pass that qil_qr_positive always adds,
the way the RSVD power iterations call it -- and is compared with a reference that does not use the code under test: LAPACK's
Householder QR (numpy.linalg.qr) with the signs fixed to a non-negative diagonal.  The errors of both are evaluated in
numpy.longdouble (64-bit mantissa).

Per case (test_factorisation):
  plan          the report's plan equals qil_qr_plan's and the table's label; `cholesky` is the outcome the table names
  orthogonality max |Q^H Q - P|, P = diag(1 kept, 0 dropped); dropped columns of Q are exactly zero; the number kept is the planted
                rank for `deficient` operands and n otherwise
  residual      per column, |A_j - (Q R)_j|_2 / |A_j|_2 (a zero column must be reproduced exactly)
  form of R     strictly lower part exactly 0; diagonal real, exactly 0 for dropped columns (and their whole row), > 0 otherwise;
                `well` operands: |R - R_ref| against the perturbation bound of the QR factorisation (below)
  footprint     both parent buffers are uploaded whole, filled with NaNs of distinct payloads outside the operand's and the
                factor's windows; everything outside the windows comes back bit-identical (compared as uint64).  With R absent,
                Q is bit-identical to the Q of the same operand with R present.
No silent repair (test_no_silent_repair): `well`, `colscaled` and the first-order pairs again with reorth = 1: no re-factorisation
ran, and where Q^H Q was measured its worst off-diagonal lies within the bound; after a first-order CholeskyQR2 the check was
skipped (skipped_check) -- and test_factorisation has held that Q to the bound in longdouble: the "Q2^H Q2 = I + O(|E|^2) by
construction" claim, tested.
Repair contract (test_repair_contract): `deficient`, hard-graded and refused-by-Cholesky operands with reorth = 1 meet the documented contract of
test_qr_rank_deficient_inputs (kept columns unit to 1e-12, off-diagonal below 1e-10, A = Q R) with at most two repairs.

Bounds (derived, not measured).  Orthogonality and residual of the device are held to FACTOR = 8 times max(the reference's same
quantity on the same operand, u sqrt(m)), u = 2^-53: two passes (CGS2, CholeskyQR2, the tree's two levels, panel + projections),
each as good as one Householder factorisation (2), the MFMA summation orders and the three-multiplication complex form (2), headroom
(2).  |R - R_ref|: both factorisations are exact for A + dA with |dA_j| <= B |A_j| per column from the residual plus n B / 2 from
the distance of Q to an orthonormal basis (B = the bound above), and R moves by sqrt(2) kappa(A) |dA|_F / |A|_F |R|_F to first order
(Stewart 1977; kappa from the reference's singular values), so max |R - R_ref| <= sqrt(2) kappa 2 B (1 + n / 2) |R|_F.
The blocked driver on hard-graded operands (kappa(A) >= 1e10; `f64_512x128_graded_d10` measured 9.3 on 32-column Householder
panels) is the one route that needs more, and gets a term of its own.  The driver projects a panel twice against the previous
columns and only then factors it (project, project, QR -- not project, QR, project, QR).  The projected panel P~ keeps an overlap
|Q_prev^H p~_j| ~ u sqrt(m) |p~_j| per column, and the panel kernel returns Q_new = P~ R_jj^-1, so Q_prev^H Q_new = (Q_prev^H P~ D^-1)
(D R_jj^-1) with D = diag |p~_j|: the overlap is amplified by the condition number of the column-equilibrated panel.  On a spectrum
graded over 10 decades and mixed by a Haar V that number is ~1e3 for 32 columns and ~1e2 for 16 (kappa(A) itself never enters:
well inside a panel's own span Householder is exact to u).  The bound for these cases is FACTOR max(reference, u sqrt(m)) +
u sqrt(m) max_panels kappa_2(R_jj D^-1), the second term computed from the reference's R.  Single-kernel routes keep FACTOR alone at
any kappa (`c64_300x16_graded_d14`, kappa 1e14: 0.17).
Tall cases whose longdouble Gram would cost more than qr_cases.LONGDOUBLE_CAP multiply-adds -- tree panels only, asserted --
are evaluated in float64 over 4096-row chunks added pairwise, and that evaluation's own u (sqrt(4096) + n + log2(chunks)) is added
to the bound.  The worst device / reference ratios per route, dtype and kind are in MEASUREMENTS.md (every test prints its own)."""
import functools

import numpy as np
import pytest

import qr_cases as Q

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
FACTOR = 8.0
CHUNK = 4096


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: no temporary outlives a call, whether it succeeded or failed."""
    yield
    assert qil.default_context().unowned_bytes() == 0


# ---------------------------------------------------------------- evaluation
def _parts(M):
    return (M.real.astype(LD), M.imag.astype(LD)) if np.iscomplexobj(M) else (M.astype(LD), None)


def _gram(Qm):
    """Q^H Q in longdouble as (real, imaginary) parts."""
    r, i = _parts(Qm)
    if i is None:
        return r.T @ r, None
    ri = r.T @ i
    return r.T @ r + i.T @ i, ri - ri.T


def _product(Qm, Rm):
    qr, qi = _parts(Qm)
    rr, ri = _parts(Rm)
    if qi is None:
        return qr @ rr, None
    return qr @ rr - qi @ ri, qr @ ri + qi @ rr


def _abs(re, im):
    return np.abs(re) if im is None else np.hypot(re, im)


def _pairwise(blocks):
    while len(blocks) > 1:
        blocks = [blocks[i] + blocks[i + 1] if i + 1 < len(blocks) else blocks[i] for i in range(0, len(blocks), 2)]
    return blocks[0]


def _measure(c, A, Qm, Rm):
    """(max |Q^H Q - P|, per-column relative residuals, kept mask, what the evaluation itself adds to a bound)."""
    m, n = A.shape
    if Q.gram_cost(c) <= Q.LONGDOUBLE_CAP:
        gr, gi = _gram(Qm)
        pr, pi = _product(Qm, Rm)
        ar, ai = _parts(A)
        d2 = (ar - pr) ** 2 + (0 if ai is None else (ai - pi) ** 2)
        a2 = ar ** 2 + (0 if ai is None else ai ** 2)
        res2, nrm2, extra = d2.sum(axis=0), a2.sum(axis=0), 0.0
    else:
        rows = [slice(r0, min(r0 + CHUNK, m)) for r0 in range(0, m, CHUNK)]
        G = _pairwise([Qm[s].conj().T @ Qm[s] for s in rows])
        gr, gi = _parts(G)
        res2 = _pairwise([(np.abs(A[s] - Qm[s] @ Rm) ** 2).sum(axis=0) for s in rows]).astype(LD)
        nrm2 = _pairwise([(np.abs(A[s]) ** 2).sum(axis=0) for s in rows]).astype(LD)
        extra = U * (np.sqrt(CHUNK) + n + np.log2(len(rows)))
    d = np.diagonal(gr).copy()
    kept = d != 0
    gr = gr - np.diag(kept.astype(LD))
    orth = float(_abs(gr, gi).max())
    zero = nrm2 == 0
    assert (res2[zero] == 0).all(), "a zero column is not reproduced exactly"
    res = np.sqrt(res2 / np.where(zero, 1, nrm2))
    return orth, res.astype(np.float64), kept, extra


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Operand, LAPACK factors with a non-negative diagonal, the reference's own errors and kappa(A): computed once per case."""
    c = Q.BY_NAME[name]
    A = Q.operand(c)
    Qr, Rr = np.linalg.qr(A)
    d = np.diagonal(Rr)
    ph = np.where(d == 0, 1, d / np.where(d == 0, 1, np.abs(d)))
    Qr, Rr = Qr * ph, Rr * ph.conj()[:, None]
    orth, res, _, extra = _measure(c, A, Qr, Rr)
    s = np.linalg.svd(Rr, compute_uv=False)
    for x in (A, Rr):
        x.setflags(write=False)
    return dict(A=A, R=Rr, orth=orth, res=float(res.max()), extra=extra, kappa=float(s[0] / s[-1]) if s[-1] > 0 else np.inf)


def _bound(c, ref):
    floor = U * np.sqrt(c.m)
    return FACTOR * max(ref["orth"], floor) + ref["extra"], FACTOR * max(ref["res"], floor) + ref["extra"]


# ---------------------------------------------------------------- running a case
def _sentinels(elems, dt, salt):
    """NaNs with distinct payloads (both parts of a complex element)."""
    buf = np.empty(elems, dtype=dt)
    raw = buf.view(np.uint64)
    raw[:] = np.uint64(0x7FF8000000000000) | (np.arange(raw.size, dtype=np.uint64) + np.uint64(1 + salt))
    return buf


def _bits(X):
    return np.ascontiguousarray(X).view(np.uint64)


def _view(buf, off, ld, rows, cols):
    """The rows x cols window at `off` with leading dimension ld, as a view into the parent buffer."""
    return buf[off:off + ld * cols].reshape(cols, ld)[:, :rows].T


def _run(qil, c, A, reorth=False, with_R=None):
    """-> Q (m x n), R (n x n, or None), the report; asserts the footprint."""
    with_R = c.with_R if with_R is None else with_R
    L, dt = Q.layout(c), Q.np_dtype(c)
    Ab = _sentinels(L.a_elems, dt, 0)
    _view(Ab, L.a_off, L.lda, c.m, c.n)[...] = A
    Rb = _sentinels(L.r_elems, dt, 1 << 40) if with_R else None
    before = [(Ab, Ab.copy(), (L.a_off, L.lda, c.m, c.n))] + ([(Rb, Rb.copy(), (L.r_off, L.ldr, c.n, c.n))] if with_R else [])
    rep = qil.qr_host(Ab, c.m, c.n, a=(L.a_off, L.lda), R=Rb, r=(L.r_off, L.ldr), reorth=reorth, cholesky_skip=c.skip)
    for after, old, win in before:
        chk = after.copy()
        _view(chk, *win)[...] = _view(old, *win)               # the window aside, every bit must be the one that went in
        assert np.array_equal(chk.view(np.uint64), old.view(np.uint64)), "an element outside the window changed"
    return (np.asfortranarray(_view(Ab, L.a_off, L.lda, c.m, c.n)),
            np.asfortranarray(_view(Rb, L.r_off, L.ldr, c.n, c.n)) if with_R else None, rep)


def _route(c, plan):
    if c.chol in (1, 2):
        return f"cholesky-{'first-order' if c.chol == 1 else 'full'}"
    if plan["route"] == "BLOCKED":
        return f"blocked{plan['panel_width']}:{plan['panel_kind']}/{plan['last_panel_kind']}".lower()
    return {"SINGLE_CGS2": "cgs2-glob" if plan["has_cgs2_global"] else "cgs2-lds", "SINGLE_HH": "hh",
            "SINGLE_TREE": "tree" + ("" if plan["tree_in_lds"] else "-chunks-glob") + ("" if plan["tree_top_in_lds"] else "-top-glob")}[plan["route"]]


def _hard(c):
    return c.kind == "graded" and c.d > 8            # kappa(A) of 1e10 and more


def _panel_amplification(plan, Rref):
    """The largest 2-norm condition number among the column-equilibrated diagonal blocks of R_ref, one block per panel of the blocked
    driver: the conditioning of each panel as the panel kernel receives it, after the projections."""
    pw, n = plan["panel_width"], Rref.shape[0]
    blocks = (Rref[j:j + pw, j:j + pw] for j in range(0, n, pw))
    return max(float(np.linalg.cond(B / np.linalg.norm(B, axis=0))) for B in blocks)


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("c", Q.RUN, ids=[c.name for c in Q.RUN])
def test_factorisation(qil, c):
    assert np.finfo(LD).nmant >= 63, "numpy longdouble has no 64-bit mantissa here: no evaluation more precise than the kernel"
    ref = _reference(c.name)
    A = ref["A"]
    Qm, Rm, rep = _run(qil, c, A)
    # plan and outcome
    plan = qil.qr_plan(Q.np_dtype(c), c.m, c.n)
    assert rep["plan"] == plan and Q.label(plan) == c.plan
    assert rep["cholesky"] == c.chol
    assert (rep["repairs"], rep["passes"], rep["skipped_check"]) == (0, 0, 0)          # reorth = 0: nothing measured, nothing repaired
    assert np.isfinite(Qm).all()
    if Rm is None:                                                     # R absent: the same Q, bit for bit, as with R present
        Q2, Rm, _ = _run(qil, c, A, with_R=True)
        assert np.array_equal(_bits(Qm), _bits(Q2)), "Q depends on whether R is asked for"
    assert np.isfinite(Rm).all()
    # form of R
    assert np.abs(np.tril(Rm, -1)).max(initial=0.0) == 0, "R is not upper triangular"
    diag = np.diagonal(Rm)
    assert np.abs(diag.imag).max() == 0 and (diag.real >= 0).all(), "diag(R) is not real and non-negative"
    orth, res, kept, _ = _measure(c, A, Qm, Rm)
    dead = ~kept
    assert not Qm[:, dead].any(), "a dropped column of Q is not exactly zero"
    assert (diag.real[kept] > 0).all() and not Rm[dead, :].any(), "dropped columns keep a row of R, or kept ones have none"
    rank = c.rank if c.kind == "deficient" else c.n
    b_orth, b_res = _bound(c, ref)
    floor = U * np.sqrt(c.m)
    print(f"QR-RATIO {_route(c, plan)} {c.dtype} {c.kind} {c.name} orth {orth / max(ref['orth'], floor):.2f} "
          f"res {res.max() / max(ref['res'], floor):.2f} (device {orth:.2e} {res.max():.2e}, reference {ref['orth']:.2e} {ref['res']:.2e}, "
          f"kept {int(kept.sum())}/{c.n})")
    assert res.max() <= b_res, f"residual {res.max():.3e} of column {int(res.argmax())}, bound {b_res:.3e}"
    if _hard(c) and plan["route"] == "BLOCKED":
        # The one route that needs more than FACTOR (docstring, "The blocked driver on hard-graded operands"): the overlap
        # u sqrt(m) |p~_j| the projections leave is divided by the panel's triangular factor.
        amp = _panel_amplification(plan, ref["R"])
        b_orth += floor * amp
        print(f"{c.name}: panel amplification {amp:.3g}, orthogonality bound {b_orth:.3e}")
    assert int(kept.sum()) == rank, (int(kept.sum()), rank)
    assert orth <= b_orth, f"max |Q^H Q - P| = {orth:.3e}, bound {b_orth:.3e} (reference {ref['orth']:.3e})"
    if c.kind == "well":
        B = max(b_orth, b_res)
        tol = np.sqrt(2) * ref["kappa"] * 2 * B * (1 + c.n / 2) * np.linalg.norm(ref["R"])
        err = np.abs(Rm - ref["R"]).max()
        assert err <= tol, f"max |R - R_ref| = {err:.3e}, bound {tol:.3e}"


CLEAN = [c for c in Q.RUN if c.kind in ("well", "colscaled") or c.name in sum(Q.FIRST_ORDER_PAIRS, ())]


@pytest.mark.parametrize("c", CLEAN, ids=[c.name for c in CLEAN])
def test_no_silent_repair(qil, c):
    ref = _reference(c.name)
    Qm, Rm, rep = _run(qil, c, ref["A"], reorth=True)
    assert rep["cholesky"] == c.chol and rep["repairs"] == 0, rep
    if c.chol == 1:
        assert rep["skipped_check"] == 1 and rep["passes"] == 0        # (test_factorisation holds this Q to the bound in longdouble)
    elif c.n >= 2:
        # what the device measured itself: the same quantity through an f64 GEMM; u sqrt(m) for that evaluation, as for the
        # float64 evaluation of the tall cases
        assert rep["skipped_check"] == 0 and rep["passes"] == 1
        assert rep["worst"][0] <= _bound(c, ref)[0] + U * np.sqrt(c.m), rep
    else:
        assert rep["passes"] == 0                                      # one column: nothing to measure
    if Q.gram_cost(c) <= Q.LONGDOUBLE_CAP:                             # no repair ran: the factorisation of test_factorisation, bit for bit
        Q0, R0, _ = _run(qil, c, ref["A"])
        assert np.array_equal(_bits(Qm), _bits(Q0))


REPAIRED = [c for c in Q.RUN if c.kind == "deficient" or _hard(c) or c.chol == 3]


@pytest.mark.parametrize("c", REPAIRED, ids=[c.name for c in REPAIRED])
def test_repair_contract(qil, c):
    """The documented contract of the measured-and-repaired QR (the assertions of test_qr_rank_deficient_inputs and
    test_qr_blocked_panels_with_dependent_columns), with at most two re-factorisations."""
    A = _reference(c.name)["A"]
    Qm, Rm, rep = _run(qil, c, A, reorth=True, with_R=True)
    assert rep["cholesky"] == c.chol and rep["repairs"] <= 2 and 1 <= rep["passes"] <= 3, rep
    G = Qm.conj().T @ Qm
    d = np.real(np.diag(G))
    assert np.all((np.abs(d - 1) < 1e-12) | (d == 0)), d
    assert np.abs(G - np.diag(d)).max() < 1e-10
    assert np.abs(Qm @ Rm - A).max() < 1e-11 * np.abs(A).max()
    assert np.all(np.real(np.diag(Rm)) >= 0) and np.abs(np.imag(np.diag(Rm))).max() == 0
    if c.kind == "deficient":
        assert int(round(d.sum())) == c.rank, (int(round(d.sum())), c.rank)
    print(f"{c.name}: repairs {rep['repairs']}, worst {rep['worst'][:rep['passes']]}")


def test_only_tall_tree_cases_are_evaluated_in_float64(qil):
    for c in Q.RUN:
        if Q.gram_cost(c) > Q.LONGDOUBLE_CAP:
            assert qil.qr_plan(Q.np_dtype(c), c.m, c.n)["route"] == "SINGLE_TREE" and c.n <= 16, c.name


@pytest.mark.parametrize("kw, msg", [
    (dict(a=(0, 69)), "lda 69 is smaller than the 70 rows of A"),
    (dict(a=(1, None)), "A reaches beyond its buffer"),
    (dict(r=(0, 29)), "ldr 29 is smaller than the 30 rows of R"),
    (dict(r=(1, None)), "R reaches beyond its buffer"),
    (dict(m=20), "needs m >= n >= 1"),
    (dict(cholesky_skip=-1), "negative cholesky_skip"),
])
def test_hook_rejects_bad_arguments(qil, kw, msg):
    kw = dict(kw)
    m = kw.pop("m", 70)
    A, R = np.ones(70 * 30), np.ones(30 * 30)
    with pytest.raises(ValueError, match=msg):
        qil.qr_host(A, m, 30, R=R, **kw)
    assert np.array_equal(A, np.ones(70 * 30)) and np.array_equal(R, np.ones(30 * 30))
