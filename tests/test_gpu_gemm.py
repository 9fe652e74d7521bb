"""The MFMA GEMM family on its own: every case of tests/gemm_cases.py (tests/test_gemm_plan.py pins which kernel each one
reaches) is RUN through qil_gemm_batched_host and compared with a reference computed without the code under test.

  * exact: operands are integers with |x| <= 8 (imaginary parts too), so every partial sum in any order -- and the
    (ar + ai)(br + bi) of the three-multiplication complex form -- is an integer far below 2^53: the result must be
    np.array_equal to the numpy product.  Entries are drawn per element of the whole parent buffer (no symmetry, no repeats),
    and the padding of A and B is NaN: a load from outside an operand's window shows.
  * footprint: C is uploaded whole, pre-filled with distinct finite values and NaNs with distinct payloads; every element
    outside the m x n windows of the `count` outputs must come back bit-identical (compared as uint64).
  * rounding model: random and graded (each part of each entry scaled by 10**U(-8, 8)) operands against a numpy longdouble
    reference (64-bit mantissa), componentwise:  |C - ref|_ij <= gamma (|A||B|)_ij, complex gamma ((|Ar|+|Ai|)(|Br|+|Bi|))_ij,
    gamma = q u / (1 - q u), u = 2^-53, q = k + 8 + splits (a dot product of length k in any order with FMAs, the additions of
    the Gauss form, the slice reduction); with subtract, u |C_old| more.  Derived, not measured: float64 numpy products sit at
    <= 0.22 of it.  Cases whose longdouble reference would exceed gemm_cases.ROUNDING_CAP multiply-adds run the exact check only.
"""
import numpy as np
import pytest

import gemm_cases as G

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


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


def _np_dtype(c):
    return np.complex128 if c.dtype == "c64" else np.float64


def _op(M, o):
    return {"N": lambda X: X, "T": lambda X: X.T, "H": lambda X: X.conj().T, "C": lambda X: X.conj()}[o](M)


def _idx(off, ld, rows, cols):
    """element indices of a rows x cols window at `off` with leading dimension ld"""
    return off + np.arange(rows, dtype=np.int64)[:, None] + ld * np.arange(cols, dtype=np.int64)[None, :]


def _fill(rng, shape, dt, kind):
    def part():
        if kind == "int":
            return rng.integers(-8, 9, size=shape).astype(np.float64)
        x = rng.standard_normal(shape)
        return x * 10.0 ** rng.uniform(-8, 8, size=shape) if kind == "graded" else x
    return part() + 1j * part() if dt == np.complex128 else part()


def _windows(c, L):
    """per batch: index windows of A, B and of the output (a list of column-block windows when cmap scatters it)"""
    wins = []
    for b in range(c.batch.count):
        ia = _idx(L.a_off + b * L.a_bs, L.lda, L.a_rows, L.a_cols)
        sel = L.b_sel[b * L.b_sel_step] * L.b_sel_stride if L.b_sel else 0
        ib = _idx(L.b_off + b * L.b_bs + sel, L.ldb, L.b_rows, L.b_cols)
        if L.cmap:
            nb = c.n // G.CMAP_BLK
            cols = np.concatenate([L.cmap[b * nb + g] * G.CMAP_BLK + np.arange(G.CMAP_BLK) for g in range(nb)])
            ic = L.c_off + np.arange(c.m, dtype=np.int64)[:, None] + L.ldc * cols[None, :]
        else:
            ic = _idx(L.c_off + b * L.c_bs, L.ldc, c.m, c.n)
        wins.append((ia, ib, ic))
    return wins


def _setup(c, kind, seed):
    """Parent buffers of case c: A and B are NaN outside the operands' windows; C holds C_old inside the output windows (integers
    / random, what `subtract` needs) and, outside them, distinct finite sentinels and NaNs with distinct payloads."""
    L = G.layout(c)
    dt = _np_dtype(c)
    rng = np.random.default_rng(seed)
    wins = _windows(c, L)
    bufs = []
    for which, elems in ((0, L.a_elems), (1, L.b_elems)):
        buf = np.full(elems, np.nan, dtype=dt)
        seen = {}
        for w in wins:
            ix = w[which]
            key = int(ix[0, 0])
            if key not in seen:           # a shared operand (batch stride 0, or a slice several batches select) is drawn once
                seen[key] = True
                buf[ix] = _fill(rng, ix.shape, dt, kind)
        bufs.append(buf)
    Cb = np.empty(L.c_elems, dtype=dt)
    raw = Cb.view(np.uint64)
    t = np.arange(raw.size, dtype=np.uint64)
    finite = (1.0e6 + 0.5 * t.astype(np.float64)).view(np.uint64)
    nan = np.uint64(0x7FF8000000000000) | (t + np.uint64(1))
    raw[:] = np.where(t % np.uint64(3) == 0, nan, finite)
    inside = np.zeros(L.c_elems, dtype=bool)
    for _, _, ic in wins:
        assert not inside[ic].any(), "overlapping outputs"
        inside[ic] = True
        if c.subtract:
            Cb[ic] = _fill(rng, ic.shape, dt, kind)
    return L, wins, bufs[0], bufs[1], Cb, inside


def _run(qil, c, L, A, B, Cb):
    return qil.gemm_batched(A, B, Cb, c.m, c.n, c.k, c.ops[0], c.ops[1], a=(L.a_off, L.lda, L.a_bs), b=(L.b_off, L.ldb, L.b_bs),
                            c=(L.c_off, L.ldc, L.c_bs), count=c.batch.count, subtract=c.subtract, skinny_m=c.skinny,
                            b_sel=L.b_sel, b_sel_step=L.b_sel_step, b_sel_stride=L.b_sel_stride, cmap=L.cmap, cmap_blk=G.CMAP_BLK)


def _footprint_ok(before, after, inside):
    keep = ~np.repeat(inside, before.itemsize // 8)
    return np.array_equal(before.view(np.uint64)[keep], after.view(np.uint64)[keep])


def _first_bad(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} wrong entries, first (row, col) {bad[:5].tolist()}: got {got[tuple(bad[0])]}, reference {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_exact_and_footprint(qil, c):
    L, wins, A, B, Cb, inside = _setup(c, "int", 1234)
    before = Cb.copy()
    _run(qil, c, L, A, B, Cb)
    for b, (ia, ib, ic) in enumerate(wins):
        ref = _op(A[ia], c.ops[0]) @ _op(B[ib], c.ops[1])
        if c.subtract:
            ref = before[ic] - ref
        got = Cb[ic]
        assert np.array_equal(got, ref), f"batch {b}: " + _first_bad(got, ref)
    assert inside.sum() == c.m * c.n * c.batch.count
    assert _footprint_ok(before, Cb, inside), "an element outside the outputs changed"


def _parts(M):
    return (M.real.astype(LD), M.imag.astype(LD)) if np.iscomplexobj(M) else (M.astype(LD), None)


ROUNDING = [c for c in G.CASES if c.rounding]


@pytest.mark.parametrize("kind", ["random", "graded"])
@pytest.mark.parametrize("c", ROUNDING, ids=[c.name for c in ROUNDING])
def test_rounding_model(qil, c, kind):
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy longdouble has no 64-bit mantissa on this platform: no reference more precise than the kernel")
    L, wins, A, B, Cb, inside = _setup(c, kind, 4321)
    before = Cb.copy()
    _run(qil, c, L, A, B, Cb)
    q = c.k + 8 + c.plan.splits
    gamma = LD(q * U) / (1 - LD(q * U))
    worst = 0.0
    for b, (ia, ib, ic) in enumerate(wins):
        Ao, Bo = _op(A[ia], c.ops[0]), _op(B[ib], c.ops[1])
        (ar, ai), (br, bi) = _parts(Ao), _parts(Bo)
        got = Cb[ic]
        if ai is None:
            ref = ar @ br
            bound = gamma * (np.abs(ar) @ np.abs(br))
            old = np.abs(before[ic]).astype(LD)
            if c.subtract:
                ref = before[ic].astype(LD) - ref
            err = np.abs(got.astype(LD) - ref)
        else:
            rr, ri = ar @ br - ai @ bi, ar @ bi + ai @ br
            bound = gamma * ((np.abs(ar) + np.abs(ai)) @ (np.abs(br) + np.abs(bi)))
            old = np.abs(before[ic]).astype(LD)
            if c.subtract:
                rr, ri = before[ic].real.astype(LD) - rr, before[ic].imag.astype(LD) - ri
            err = np.hypot(got.real.astype(LD) - rr, got.imag.astype(LD) - ri)
        if c.subtract:
            bound = bound + LD(U) * old
        assert np.isfinite(got).all()
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        assert (err <= bound).all(), f"batch {b}: error / bound = {ratio:.3g} at {np.unravel_index(np.argmax(err / bound), err.shape)}"
    print(f"{c.name} {kind}: worst error / bound {worst:.3f}")
    assert _footprint_ok(before, Cb, inside)


@pytest.mark.parametrize("name", ["c64_HN_130x129x1025_rule1", "c64_HN_64x64x257_rule2_rounding_drops_a_slice",
                                  "c64_NH_768x768x4096_rule3", "f64_NN_700x700x1025_rule1", "f64_NN_200x30x4097_ksweep",
                                  "f64_NN_1100x900x4097_rule3", "c64_HN_64x64x513_packed_split_rule1"])
def test_split_k_is_deterministic(qil, name):
    """The slices are reduced in a fixed order: the same call twice gives the same bits (one case of each rule and dtype)."""
    c = G.BY_NAME[name]
    assert c.plan.splits > 1
    L, wins, A, B, Cb, inside = _setup(c, "random", 99)
    C2 = Cb.copy()
    _run(qil, c, L, A, B, Cb)
    _run(qil, c, L, A, B, C2)
    assert np.array_equal(Cb.view(np.uint64), C2.view(np.uint64))


SPECIAL = ["f64_NN_70x45x37_ksweep", "c64_NN_70x45x37_ksweep", "c64_NN_5x3x200_ksweep", "f64_NN_200x30x200_ksweep",
           "c64_NN_17x200x37_ksweep", "f64_NN_40x128x200_ksweep", "f64_TN_1400x133x129_staging", "c64_HH_520x520x37_staging"]


@pytest.mark.parametrize("name", SPECIAL)
def test_inf_and_nan_stay_in_their_rows(qil, name):
    """One inf and one nan in op(A): exactly those two rows of C are non-finite, the rest equals the reference.  The nan sits in the
    FIRST element of A, which is what a lane beyond the K edge loads before the tail is zeroed; the inf in the LAST row, which is
    what the clamped lanes beyond the M edge load."""
    c = G.BY_NAME[name]
    L, wins, A, B, Cb, inside = _setup(c, "int", 7)
    ia = wins[0][0]
    Ao_idx = ia if c.ops[0] in "NC" else ia.T            # op(A)[r, kk] lives at Ao_idx[r, kk]
    B[wins[0][1]] = np.where(B[wins[0][1]] == 0, 3, B[wins[0][1]])      # inf * 0 would be a nan: still non-finite, but keep it an inf
    A[Ao_idx[0, 0]] = np.nan
    A[Ao_idx[c.m - 1, c.k - 1]] = np.inf
    before = Cb.copy()
    _run(qil, c, L, A, B, Cb)
    got = Cb[wins[0][2]]
    bad_rows = sorted({0, c.m - 1})
    good = np.setdiff1d(np.arange(c.m), bad_rows)
    assert not np.isfinite(got[bad_rows]).any()
    Az = A.copy()
    Az[Ao_idx[0, 0]] = Az[Ao_idx[c.m - 1, c.k - 1]] = 0
    ref = _op(Az[ia], c.ops[0]) @ _op(B[wins[0][1]], c.ops[1])
    assert np.array_equal(got[good], ref[good]), _first_bad(got[good], ref[good])
    assert _footprint_ok(before, Cb, inside)


@pytest.mark.parametrize("name", SPECIAL)
def test_zero_operand_with_negative_zeros(qil, name):
    c = G.BY_NAME[name]
    L, wins, A, B, Cb, inside = _setup(c, "random", 8)
    ia = wins[0][0]
    z = np.where((ia // 3) % 2 == 0, 0.0, -0.0)
    A[ia] = z - 1j * z if np.iscomplexobj(A) else z
    _run(qil, c, L, A, B, Cb)
    got = Cb[wins[0][2]]
    assert np.isfinite(got).all() and np.array_equal(got, np.zeros_like(got))


# ---------------------------------------------------------------- errors
def _flat(n, dt=np.float64):
    return np.ones(n, dtype=dt)


@pytest.mark.parametrize("kw, msg", [
    (dict(a=(0, 69, 0)), "lda 69 is smaller than the 70 stored rows of A"),
    (dict(b=(0, 36, 0)), "ldb 36 is smaller than the 37 stored rows of B"),
    (dict(c=(0, 69, 0)), "ldc 69 is smaller than the 70 rows of C"),
    (dict(opA="T", a=(0, 36, 0)), "lda 36 is smaller than the 37 stored rows of A"),
    (dict(opB="T", b=(0, 44, 0)), "ldb 44 is smaller than the 45 stored rows of B"),
    (dict(k=0), "empty operand"),
    (dict(count=65536), "batch count 65536 exceeds the grid limit"),
    (dict(a=(1, None, 0)), "A reaches beyond its buffer"),
    (dict(b=(0, None, 1), count=2), "B reaches beyond its buffer"),
    (dict(c=(0, 71, 0)), "C reaches beyond its buffer"),
])
def test_batched_hook_rejects_bad_arguments(qil, kw, msg):
    kw = dict(kw)
    k = kw.pop("k", 37)
    A, B, Cb = _flat(70 * 37), _flat(37 * 45), _flat(70 * 45)
    before = Cb.copy()
    with pytest.raises(ValueError, match=msg):
        qil.gemm_batched(A, B, Cb, 70, 45, k, **kw)
    assert np.array_equal(Cb, before)
    assert qil.default_context().unowned_bytes() == 0


def test_gemm_rejects_bad_arguments(qil):
    """qil_gemm itself: leading dimensions, op codes, empty operands."""
    import ctypes
    from qilaplace_jl_amd import _lib as Lb
    ctx = qil.default_context()
    A, B, Cb = _flat(70 * 37), _flat(45 * 37), _flat(70 * 45)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)

    def call(opA, opB, m, n, k, lda, ldb, ldc):
        Lb.check(Lb.lib.qil_gemm(ctx.handle, Lb.QIL_F64, opA, opB, m, n, k, p(A), lda, p(B), ldb, p(Cb), ldc))

    for args, msg in (((0, 0, 70, 45, 37, 69, 37, 70), "lda 69 is smaller than the 70 stored rows of A"),
                      ((1, 0, 70, 45, 37, 36, 37, 70), "lda 36 is smaller than the 37 stored rows of A"),
                      ((0, 0, 70, 45, 37, 70, 36, 70), "ldb 36 is smaller than the 37 stored rows of B"),
                      ((0, 2, 70, 45, 37, 70, 44, 70), "ldb 44 is smaller than the 45 stored rows of B"),
                      ((0, 0, 70, 45, 37, 70, 37, 69), "ldc 69 is smaller than the 70 rows of C"),
                      ((4, 0, 70, 45, 37, 70, 37, 70), "bad op code"), ((0, -1, 70, 45, 37, 70, 37, 70), "bad op code"),
                      ((0, 0, 70, 45, 0, 70, 37, 70), "empty operand")):
        with pytest.raises(ValueError, match=msg):
            call(*args)
        assert ctx.unowned_bytes() == 0
    call(0, 0, 70, 45, 37, 70, 37, 70)
    assert np.array_equal(Cb, np.full(70 * 45, 37.0))


def test_failed_allocation_leaves_nothing_behind(qil):
    """Every allocation of the hook in turn fails (operands, selector, split-K workspace): MemoryError, no pool memory stranded, the
    host C untouched; the first call that gets through is right."""
    ctx = qil.default_context()
    c = G.BY_NAME["c64_HN_64x64x513_packed_split_rule1"]
    assert c.plan.splits > 1
    c = c._replace(batch=c.batch._replace(b_sel=True))
    L, wins, A, B, Cb, inside = _setup(c, "int", 5)
    before = Cb.copy()
    failures = 0
    for j in range(0, 32):
        ctx.fail_alloc_after(j)
        try:
            _run(qil, c, L, A, B, Cb)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, j
        if not failed:
            break
        failures += 1
        assert np.array_equal(Cb.view(np.uint64), before.view(np.uint64)), j
    assert failures >= 5, failures
    for ia, ib, ic in wins:
        assert np.array_equal(Cb[ic], _op(A[ia], c.ops[0]) @ _op(B[ib], c.ops[1]))
    assert _footprint_ok(before, Cb, inside)
