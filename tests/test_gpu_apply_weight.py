"""GPU tests of the lazy Born weights of W psi (qil.apply_weight_batch and its front-ends apply_weight, apply_bit_probabilities,
apply_range_weight, apply_weight_quantiles, apply_zt_row_weights, apply_zt_column_weights), none of which forms W psi.

The reference is numpy on `abs(helpers.apply_dense(W, A))**2` reshaped to (2,)*n, times amplitude^2: the fixed axes indexed, the
traced ones summed.  Tolerance: 1e-12 of the TOTAL weight, the project's read-out tolerance (a weight is a sum of non-negative
terms, so the total is its scale); a numpy restatement of exactly this contraction (lead vector, density walk, right environments)
on these shape families deviated at most 1.2e-15 of the total, so the margin belongs to the device arithmetic.  1e-10 relative at
mid size, as the full-size weight tests.

Shapes (chi bonds of psi / D bonds of W): bond 1, odd bonds that are no multiple of a tile, a small saturated pair, a wide
operator on a thin state and a wide state under a thin operator.  All have an even number of tensors, so each also runs paired.
Rows are processed in chunks of max(1, min(nb, 32768, 64 MiB / ((2 maxMid + 2 maxM + maxX) e))) rows (`_chunk`, restated from
the header)."""
import ctypes as C
import functools
import importlib
import importlib.util
import os

import numpy as np
import pytest

from helpers import random_mps_data, random_mpo_data, saturated_profile, apply_dense

pytestmark = pytest.mark.gpu

FIX0, FIX1, TRACE = 0, 1, 2
BUDGET = 64 << 20
RENV = "QIL_APPLY_WEIGHT_RENV_BYTES"
F, Z = np.float64, np.complex128
DT_PAIRS = [(F, F), (F, Z), (Z, F), (Z, Z)]                                  # (psi, W)
DT_IDS = ["f64-f64", "f64-c64", "c64-f64", "c64-c64"]
PROFILES = {
    "bond1": ([1] * 7, [1] * 7),
    "odd": ([2, 3, 5, 7, 5, 3, 2], [3, 5, 2, 7, 3, 2, 5]),
    "sat": (saturated_profile(10, 8), saturated_profile(10, 6, 4)),
    "wideD": (saturated_profile(10, 4), saturated_profile(10, 16, 4)),
    "widechi": (saturated_profile(10, 24), saturated_profile(10, 4, 4)),
}
CASES = list(PROFILES)


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    assert qil.default_context().unowned_bytes() == 0


def _amp(dt):
    return -1.3 if dt == Z else 1.7                                           # a parent amplitude != 1


def _specs(n, rng):
    """name -> spec row for an n-tensor chain (n >= 8): the rows of the weight tests"""
    def bits(m):
        return rng.integers(0, 2, m).astype(np.uint8)
    out = {}
    out["all_fixed"] = bits(n)
    out["all_traced"] = np.full(n, TRACE, dtype=np.uint8)
    s = np.full(n, TRACE, dtype=np.uint8); s[:n // 2] = bits(n // 2); out["fixed_then_traced"] = s
    s = bits(n); s[:n // 2] = TRACE; out["traced_then_fixed"] = s
    s = bits(n); s[0::2] = TRACE; out["alternating_t"] = s
    s = bits(n); s[1::2] = TRACE; out["alternating_f"] = s
    for name, k in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        s = bits(n); s[k] = TRACE; out["one_traced_" + name] = s
        s = np.full(n, TRACE, dtype=np.uint8); s[k] = rng.integers(0, 2); out["one_fixed_" + name] = s
    for j in range(16):
        out[f"random{j}"] = rng.integers(0, 3, n).astype(np.uint8)
    return out


def _dense_weight(P, spec):
    T = P
    for i in range(len(spec) - 1, -1, -1):
        T = T.sum(axis=i) if spec[i] == TRACE else np.take(T, int(spec[i]), axis=i)
    return float(T)


@functools.lru_cache(maxsize=None)
def _case(case, dta, dtw):
    """host tensors, the spec rows and their dense reference: computed once, shared by the tests, left unchanged"""
    rng = np.random.default_rng(9000 + 4 * CASES.index(case) + 2 * (dta == Z) + (dtw == Z))
    chi, D = PROFILES[case]
    a = random_mps_data(chi, rng, dta)
    w = random_mpo_data(D, rng, dtw)
    n = len(a)
    P = np.abs(apply_dense(w, a)).reshape((2,) * n) ** 2
    specs = _specs(n, rng)
    names = sorted(specs)
    rows = np.array([specs[k] for k in names], dtype=np.uint8)
    amp = _amp(dta)
    ref = amp * amp * np.array([_dense_weight(P, r) for r in rows])
    for x in (P, rows, ref):
        x.setflags(write=False)
    return a, w, P, names, rows, ref, amp * amp * float(P.sum())


def _operands(qil, a, w, paired, amp):
    if paired:
        return qil.PairedSiteMPO(w), qil.ZTMPS(a, amplitude=amp)
    return qil.SingleSiteMPO(w), qil.SignalMPS(a, amplitude=amp)


def _chunk(chi, D, nb, itemsize):
    """the documented chunk size, restated"""
    c, d = [1] + list(chi) + [1], [1] + list(D) + [1]
    mid = m = x = 1
    for i in range(len(c) - 1):
        cl, cr, dl, dr = c[i], c[i + 1], d[i], d[i + 1]
        mid = max(mid, cl * cl * dl * dl, 2 * cl * dl * dl * cr, 2 * cl * dl * dr * cr, 2 * cl * dr * dr * cr, cr * cr * dr * dr)
        m = max(m, cl * dl, cr * dr)
        x = max(x, 2 * cl * dr)
    return max(1, min(nb, 32768, BUDGET // ((2 * mid + 2 * m + x) * itemsize)))


# ---------------------------------------------------------------- 1. dense parity
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
@pytest.mark.parametrize("case", CASES)
def test_lazy_weights_match_the_dense_sum(qil, case, paired, dts):
    a, w, P, names, rows, ref, total = _case(case, *dts)
    W, psi = _operands(qil, a, w, paired, _amp(dts[0]))
    got = qil.apply_weight_batch(W, psi, rows)
    assert got.dtype == np.float64 and got.shape == ref.shape
    err = np.abs(got - ref) / total
    print(f"apply_weight_batch {case} paired={paired} {DT_IDS[DT_PAIRS.index(dts)]}: worst deviation {err.max():.2e} of the total")
    assert np.all(err <= 1e-12), (case, names[int(err.argmax())], err.max())
    k = int(np.argmax(ref))
    one = qil.apply_weight(W, psi, rows[k])
    assert isinstance(one, float) and abs(one - ref[k]) <= 1e-12 * total


# ---------------------------------------------------------------- 2. against the existing verbs
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES)
def test_lazy_weights_agree_with_the_product_the_coefficients_and_the_norm(qil, case, dts):
    a, w, P, names, rows, ref, total = _case(case, *dts)
    amp = _amp(dts[0])
    W, psi = _operands(qil, a, w, False, amp)
    got = qil.apply_weight_batch(W, psi, rows)
    prod = qil.apply(W, psi)
    formed = qil.weight_batch(prod, rows)
    del prod
    assert np.all(np.abs(got - formed) <= 1e-12 * total), np.abs(got - formed).max() / total
    fixed = [r for r in range(len(rows)) if TRACE not in rows[r]]
    assert names.index("all_fixed") in fixed
    coeff = np.abs(qil.apply_coefficient_batch(W, psi, rows[fixed])) ** 2
    assert np.all(np.abs(got[fixed] - coeff) <= 1e-12 * total)
    assert abs(got[names.index("all_traced")] - (amp * qil.apply_norm(W, psi)) ** 2) <= 1e-12 * total


# ---------------------------------------------------------------- 3. additivity
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES)
def test_a_traced_site_is_the_sum_of_its_two_fixings(qil, case, dts):
    a, w, P, names, rows, ref, total = _case(case, *dts)
    W, psi = _operands(qil, a, w, True, _amp(dts[0]))
    rng = np.random.default_rng(31)
    traced = [r for r in range(len(rows)) if TRACE in rows[r]]
    split = []
    for r in traced:
        k = int(rng.choice(np.flatnonzero(rows[r] == TRACE)))
        for b in (0, 1):
            s = rows[r].copy(); s[k] = b; split.append(s)
    whole = qil.apply_weight_batch(W, psi, rows[traced])
    halves = qil.apply_weight_batch(W, psi, np.array(split)).reshape(-1, 2)
    assert np.all(np.abs(halves[:, 0] + halves[:, 1] - whole) <= 1e-12 * total)


# ---------------------------------------------------------------- 4. the right-environment budget
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES)
def test_no_kept_right_environment_gives_the_same_weights(qil, case, dts, monkeypatch):
    a, w, P, names, rows, ref, total = _case(case, *dts)
    W, psi = _operands(qil, a, w, False, _amp(dts[0]))
    default = qil.apply_weight_batch(W, psi, rows)
    monkeypatch.setenv(RENV, "0")                                             # read on each call: every tail is walked as middle
    walked = qil.apply_weight_batch(W, psi, rows)
    monkeypatch.delenv(RENV)
    assert np.all(np.abs(walked - ref) <= 1e-12 * total), np.abs(walked - ref).max() / total
    assert np.all(np.abs(walked - default) <= 1e-12 * total)


# ---------------------------------------------------------------- 5. chunking
@pytest.mark.parametrize("dts", DT_PAIRS, ids=DT_IDS)
def test_rows_across_chunk_boundaries(qil, dts):
    a, w, P, names, rows, ref, total = _case("wideD", *dts)
    itemsize = 16 if Z in dts else 8
    chunk = _chunk(*PROFILES["wideD"], 1 << 30, itemsize)
    nb = 2 * chunk + 5
    assert 1 <= chunk < 4096 and _chunk(*PROFILES["wideD"], nb, itemsize) == chunk
    W, psi = _operands(qil, a, w, False, _amp(dts[0]))
    pick = np.random.default_rng(43).integers(0, len(rows), size=nb)
    got = qil.apply_weight_batch(W, psi, rows[pick])
    err = np.abs(got - ref[pick]) / total
    print(f"{nb} rows in chunks of {chunk}, {DT_IDS[DT_PAIRS.index(dts)]}: worst deviation {err.max():.2e} of the total weight")
    assert np.all(err <= 1e-12), err.max()


def test_strided_batches_past_the_grid_limit(qil):
    """20000 rows that are all in the middle at once: f64, psi bonds (1, 2, 4, 4, 4, 2, 1) under W bonds (1, 2, 2, 2, 2, 2, 1), the
    first site traced, the last fixed, the rest drawn from {0, 1, 2}.  Per-row temporaries are 2304 B, so one chunk holds every
    row, and at the interior sites T2 is a strided batch of 20000 * 4 = 80000 products and T3 one of 20000 * 2 * 4 = 160000: both
    go out in pieces of 65535, the grid's y limit.  Against weight_batch of the formed product, on the same rows."""
    chi, D, nb = [2, 4, 4, 4, 2], [2, 2, 2, 2, 2], 20000
    rng = np.random.default_rng(1717)
    a, w = random_mps_data(chi, rng, F), random_mpo_data(D, rng, F)
    rows = rng.integers(0, 3, size=(nb, len(a))).astype(np.uint8)
    rows[:, 0] = TRACE
    rows[:, -1] = rng.integers(0, 2, size=nb)
    assert _chunk(chi, D, nb, 8) == nb and BUDGET // nb >= 2304 and nb * 4 > 65535
    amp = _amp(F)
    total = amp * amp * float((np.abs(apply_dense(w, a)) ** 2).sum())
    W, psi = _operands(qil, a, w, False, amp)
    got = qil.apply_weight_batch(W, psi, rows)
    formed = qil.weight_batch(qil.apply(W, psi), rows)
    err = np.abs(got - formed) / total
    print(f"{nb} rows, batches of {nb * 4} and {nb * 8}: worst deviation {err.max():.2e} of the total weight")
    assert got.shape == (nb,) and np.all(err <= 1e-12), (int(err.argmax()), err.max())


# ---------------------------------------------------------------- 6. run to run
@pytest.mark.parametrize("case", ["odd", "sat"])
def test_two_runs_are_bit_equal(qil, case):
    a, w, P, names, rows, ref, total = _case(case, Z, Z)
    W, psi = _operands(qil, a, w, False, _amp(Z))
    big = np.random.default_rng(41).integers(0, 3, size=(300, rows.shape[1])).astype(np.uint8)
    big[:len(rows)] = rows
    first = qil.apply_weight_batch(W, psi, big)
    assert np.array_equal(first, qil.apply_weight_batch(W, psi, big))
    assert np.all(np.isfinite(first)) and first.min() >= -1e-12 * total


# ---------------------------------------------------------------- 7. errors and edge cases
def test_errors_and_edge_cases(qil):
    L = importlib.import_module("qilaplace_jl_amd._lib")
    rng = np.random.default_rng(71)
    a8, a7 = random_mps_data([2] * 7, rng), random_mps_data([2] * 6, rng)
    w8 = random_mpo_data([2] * 7, rng)
    W, psi = qil.SingleSiteMPO(w8), qil.SignalMPS(a8)
    with pytest.raises(ValueError, match="same number of sites"):
        qil.apply_weight_batch(W, qil.SignalMPS(a7), [[2] * 7])
    with pytest.raises(ValueError, match="same site indices"):
        qil.apply_weight_batch(qil.SingleSiteMPO(w8, sites=list(range(11, 19))), psi, [[2] * 8])
    with pytest.raises(ValueError, match=r"outside \[0,2\]"):
        qil.apply_weight_batch(W, psi, [[2, 3, 2, 2, 2, 2, 2, 2]])
    # the library's own checks, behind the front-end's
    out = (C.c_double * 2)(-7.0, -7.0)
    sp = (C.c_uint8 * 16)(0, 1, 2, 0, 2, 2, 2, 2, 2, 3, 2, 2, 0, 0, 0, 0)
    assert L.lib.qil_apply_weight_batch(W.handle, psi.handle, 2, sp, out) == L.QIL_EINVAL_CONFIG
    assert "spec value 3 outside [0,2]" in L.last_error() and list(out) == [-7.0, -7.0]
    assert L.lib.qil_apply_weight_batch(W.handle, psi.handle, -1, sp, out) == L.QIL_EINVAL_ARG
    assert L.lib.qil_apply_weight_batch(W.handle, psi.handle, 0, sp, out) == L.QIL_OK and list(out) == [-7.0, -7.0]
    assert L.lib.qil_apply_weight_batch(W.handle, psi.handle, 0, None, None) == L.QIL_OK
    assert qil.apply_weight_batch(W, psi, np.zeros((0, 8))).shape == (0,)
    for dt in (F, Z):
        zero = qil.SignalMPS([np.zeros(t.shape, dtype=dt) for t in a8], amplitude=3.0)
        rows = rng.integers(0, 3, size=(9, 8)).astype(np.uint8)
        assert np.array_equal(qil.apply_weight_batch(W, zero, rows), np.zeros(9))


def test_single_site_chain(qil):
    A = np.array([0.25, -1.5]).reshape(1, 2, 1)
    M = np.array([[0.5, -2.0], [1.0, 0.25]])                                  # M[s_in, s_out]
    W, psi = qil.SingleSiteMPO([M.reshape(1, 2, 2, 1)]), qil.SignalMPS([A], amplitude=3.0)
    y = np.array([0.25 * 0.5 - 1.5 * 1.0, 0.25 * -2.0 - 1.5 * 0.25])          # (W psi)[s_out] by hand
    got = qil.apply_weight_batch(W, psi, [[0], [1], [2]])
    assert np.allclose(got, 9.0 * np.array([y[0] ** 2, y[1] ** 2, y[0] ** 2 + y[1] ** 2]), rtol=1e-15, atol=0)


# ---------------------------------------------------------------- 8. allocation failure
def test_allocation_failure_leaves_nothing_behind(qil):
    """Fault injection (a host-side refusal by the pool) at every allocation of a call: the call raises the allocation error,
    nothing is stranded, and the first call that succeeds matches the reference with the operands unchanged."""
    a, w, P, names, rows, ref, total = _case("odd", F, Z)
    ctx = qil.default_context()
    W, psi = _operands(qil, a, w, False, _amp(F))
    failures, got = 0, None
    for j in range(400):
        ctx.fail_alloc_after(j)
        try:
            got = qil.apply_weight_batch(W, psi, rows)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, j
        if not failed:
            break
        failures += 1
    # the spec copy, the result, five site operands and five row buffers at the least
    assert got is not None and failures >= 12, failures
    assert np.all(np.abs(got - ref) <= 1e-12 * total)
    assert all(np.array_equal(psi.site(i), a[i]) for i in range(len(a)))
    assert all(np.array_equal(W.site(i), w[i]) for i in range(len(w)))


# ---------------------------------------------------------------- 9. front-ends
@pytest.mark.parametrize("dts", [(F, F), (Z, Z)], ids=["f64-f64", "c64-c64"])
def test_range_weight_bit_probabilities_and_quantiles(qil, dts):
    a, w, P, names, rows, ref, total = _case("sat", *dts)
    amp = _amp(dts[0])
    n = len(a)
    N = 2 ** n
    W, psi = _operands(qil, a, w, False, amp)
    dense = amp * amp * P.reshape(-1)                     # x big-endian: the first tensor is the most significant bit
    rng = np.random.default_rng(51)
    ranges = [(5, 5), (0, N), (77, 78), (1, N - 1), (N // 2 - 37, N // 2 + 300)]
    ranges += [tuple(sorted(int(v) for v in rng.integers(0, N + 1, size=2))) for _ in range(8)]
    for lo, hi in ranges:
        got = qil.apply_range_weight(W, psi, lo, hi)
        nblocks = max(len(qil.ops._dyadic_blocks(lo, hi, n)), 1)
        assert isinstance(got, float) and abs(got - dense[lo:hi].sum()) <= nblocks * 1e-12 * total, (lo, hi)
    marg = np.array([np.take(P, 1, axis=i).sum() for i in range(n)]) / P.sum()
    got = qil.apply_bit_probabilities(W, psi)
    assert got.shape == (n,) and np.all(np.abs(got - marg) <= 2e-12)
    cum = np.cumsum(dense)
    qs = []
    while len(qs) < 8:
        q = float(rng.uniform(0.0, 1.0))
        if np.abs(cum - q * cum[-1]).min() >= 1e-9 * cum[-1]:
            qs.append(q)
    want = np.searchsorted(cum, np.array(qs) * cum[-1], side="left")
    assert np.array_equal(qil.apply_weight_quantiles(W, psi, qs), want)
    assert qil.apply_weight_quantiles(W, psi, []).shape == (0,)
    rev = amp * amp * P.transpose(list(range(n - 1, -1, -1))).reshape(-1)
    for lo, hi in ranges[3:7]:
        nblocks = len(qil.ops._dyadic_blocks(lo, hi, n))
        assert abs(qil.apply_range_weight(W, psi, lo, hi, reverse=True) - rev[lo:hi].sum()) <= nblocks * 1e-12 * total, (lo, hi)
    cum = np.cumsum(rev)
    qs = []
    while len(qs) < 4:
        q = float(rng.uniform(0.0, 1.0))
        if np.abs(cum - q * cum[-1]).min() >= 1e-9 * cum[-1]:
            qs.append(q)
    assert np.array_equal(qil.apply_weight_quantiles(W, psi, qs, reverse=True),
                          np.searchsorted(cum, np.array(qs) * cum[-1], side="left"))


@pytest.mark.parametrize("dts", [(F, F), (Z, Z)], ids=["f64-f64", "c64-c64"])
def test_zt_row_and_column_weights_against_the_dense_grid(qil, dts):
    """A 2 x 5-tensor ZTMPS under a PairedSiteMPO: tensor 2 i is bit i (lsb first) of k, tensor 2 i + 1 bit i of l."""
    n = 5
    rng = np.random.default_rng(61 + (dts[0] == Z))
    a = random_mps_data([2, 4, 6, 8, 9, 8, 4, 3, 2], rng, dts[0])
    w = random_mpo_data([3, 4, 5, 6, 7, 5, 4, 3, 2], rng, dts[1])
    amp = _amp(dts[0])
    W, psi = qil.PairedSiteMPO(w), qil.ZTMPS(a, amplitude=amp)
    P = np.abs(apply_dense(w, a)).reshape((2,) * (2 * n)) ** 2
    order = [2 * i for i in range(n - 1, -1, -1)] + [2 * i + 1 for i in range(n - 1, -1, -1)]
    grid = amp * amp * P.transpose(order).reshape(2 ** n, 2 ** n)             # grid[k, l] = |Z(k, l)|^2
    total = grid.sum()
    idx = np.arange(2 ** n)
    assert np.all(np.abs(qil.apply_zt_row_weights(W, psi, idx) - grid.sum(axis=0)) <= 1e-12 * total)
    assert np.all(np.abs(qil.apply_zt_column_weights(W, psi, idx) - grid.sum(axis=1)) <= 1e-12 * total)
    sel = [7, 0, 31, 7]
    assert np.all(np.abs(qil.apply_zt_row_weights(W, psi, sel) - grid.sum(axis=0)[sel]) <= 1e-12 * total)
    assert abs(qil.apply_zt_column_weights(W, psi, 9)[0] - grid[9].sum()) <= 1e-12 * total


# ---------------------------------------------------------------- 10. mid size
def test_mid_size_row_weights_against_the_formed_product(qil):
    """24 paired tensors, chi <= 16, D <= 32 (a product bond of 512): 8 row energies against zt_row_weights of W psi."""
    n = 12
    psi = qil.ZTMPS.alloc(saturated_profile(2 * n, 16), dtype=F, amplitude=2.5).fill_random(20241018)
    W = qil.PairedSiteMPO.alloc(saturated_profile(2 * n, 32, 4), dtype=Z).fill_random(20241019)
    ls = [int(v) for v in np.random.default_rng(81).integers(0, 2 ** n, size=8)]
    got = qil.apply_zt_row_weights(W, psi, ls)
    prod = qil.apply(W, psi)
    ref = qil.zt_row_weights(prod, ls)
    del prod
    rel = np.abs(got - ref) / ref
    print(f"mid-size apply_zt_row_weights: worst relative deviation {rel.max():.2e}")
    assert np.all(ref > 0) and np.all(rel <= 1e-10), rel.max()


# ---------------------------------------------------------------- 11. the example
def test_lazy_band_power_example_checks_itself(qil, capsys):
    """examples/lazy_band_power.py asserts every figure it prints against weight_batch(apply(W, psi)); run in this process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lazy_band_power", os.path.join(root, "examples", "lazy_band_power.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bands, rows = mod.main()
    assert 0 <= bands["median"] <= bands["edge95"] < 2 ** 12 and len(rows) == 16
    assert "median frequency" in capsys.readouterr().out
