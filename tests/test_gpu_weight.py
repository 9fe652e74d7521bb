"""GPU tests of the Born weights (qil.weight_batch and its front-ends weight, bit_probabilities, range_weight, weight_quantiles,
zt_row_weights, zt_column_weights).

The reference is numpy on `helpers.dense_mps(data)`: `abs(T)**2`, the fixed axes indexed, the traced ones summed, times
amplitude^2 (`_dense_weight`).  Tolerance: 1e-12 of the TOTAL weight (the project's read-out tolerance; a weight is a sum of
non-negative terms, so the total is its scale), 1e-10 relative at full size (as the top-k and restrict tests).  The bond profiles,
restated here: bond 1, bonds that are no multiple of 4 or 16, a small saturated chain, a chain saturated at the LDS limit of the
walk kernel (80 for f64, 48 for c64), one just above it (the GEMM route) and one that is wide in the middle only (128, the GEMM
route too).  The GEMM route works in chunks of rows under 64 MiB of temporaries, four chi^2 buffers per row."""
import ctypes as C
import functools
import importlib
import importlib.util

import numpy as np
import pytest

from helpers import random_mps_data, saturated_profile, dense_mps

pytestmark = pytest.mark.gpu

FIX0, FIX1, TRACE, KEEP = 0, 1, 2, 3
LDS_LIMIT = {np.float64: 80, np.complex128: 48}
GEMM_BUDGET = 64 << 20
DTYPES = [np.float64, np.complex128]
DT_IDS = ["f64", "c64"]


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    assert q.device_count() >= 1
    assert (q.ops.FIX0, q.ops.FIX1, q.ops.TRACE) == (FIX0, FIX1, TRACE)
    return q


@pytest.fixture(autouse=True)
def _no_stranded_temporaries(qil):
    """After every test: all pool memory in use belongs to some MPS/MPO handle (no temporary outlives a call)."""
    yield
    assert qil.default_context().unowned_bytes() == 0


def _profile(case, dt):
    lim = LDS_LIMIT[dt]
    return {
        "bond1": [1] * 7,
        "odd": [2, 3, 5, 7, 5, 3, 2],
        "sat8": saturated_profile(12, 8),
        "limit": saturated_profile(14 if lim > 64 else 12, lim),
        "above": saturated_profile(14 if lim > 64 else 12, lim + 1),
        "wide": saturated_profile(16, 128),
    }[case]


CASES = ["bond1", "odd", "sat8", "limit", "above", "wide"]
LDS_CASES = ["bond1", "odd", "sat8", "limit"]


def _amp(dt):
    return -1.3 if dt == np.complex128 else 1.7                       # a parent amplitude != 1


def _specs(n, rng):
    """name -> spec row for an n-tensor chain (n >= 8)"""
    def bits(m):
        return rng.integers(0, 2, m).astype(np.uint8)
    out = {}
    out["all_fixed"] = bits(n)
    out["all_traced"] = np.full(n, TRACE, dtype=np.uint8)
    s = np.full(n, TRACE, dtype=np.uint8); s[:n // 2] = bits(n // 2); out["fixed_then_traced"] = s      # the dyadic shape
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
    """numpy restatement on P = abs(T)**2: fixed axes indexed, traced axes summed"""
    T = P
    for i in range(len(spec) - 1, -1, -1):
        T = T.sum(axis=i) if spec[i] == TRACE else np.take(T, int(spec[i]), axis=i)
    return float(T)


@functools.lru_cache(maxsize=None)
def _case(case, dt):
    """host tensors, the spec rows and their dense reference: computed once, shared by the tests, left unchanged"""
    rng = np.random.default_rng(7000 + CASES.index(case) * 2 + (dt == np.complex128))
    data = random_mps_data(_profile(case, dt), rng, dt)
    P = np.abs(dense_mps(data)) ** 2
    specs = _specs(len(data), rng)
    names = sorted(specs)
    rows = np.array([specs[k] for k in names], dtype=np.uint8)
    amp = _amp(dt)
    ref = amp * amp * np.array([_dense_weight(P, r) for r in rows])
    for a in (P, rows, ref):
        a.setflags(write=False)
    return data, P, names, rows, ref, amp * amp * float(P.sum())


def _mps(qil, data, paired, amp=1.0):
    return (qil.ZTMPS if paired else qil.SignalMPS)(data, amplitude=amp)


# ---------------------------------------------------------------- 1. dense parity
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
@pytest.mark.parametrize("case", CASES)
def test_weights_match_the_dense_sum(qil, case, paired, dt):
    data, P, names, rows, ref, total = _case(case, dt)
    psi = _mps(qil, data, paired, _amp(dt))
    got = qil.weight_batch(psi, rows)
    assert got.dtype == np.float64 and got.shape == ref.shape
    err = np.abs(got - ref) / total
    print(f"weight_batch {case} paired={paired} {np.dtype(dt).name}: worst deviation {err.max():.2e} of the total weight")
    assert np.all(err <= 1e-12), (case, names[int(err.argmax())], err.max())
    k = int(np.argmax(ref))
    assert qil.weight(psi, rows[k]) == pytest.approx(ref[k], abs=1e-12 * total) and isinstance(qil.weight(psi, rows[k]), float)


# ---------------------------------------------------------------- 2. against the existing verbs
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES)
def test_weights_agree_with_coefficient_norm_and_restrict(qil, case, dt):
    data, P, names, rows, ref, total = _case(case, dt)
    amp = _amp(dt)
    psi = _mps(qil, data, False, amp)
    got = qil.weight_batch(psi, rows)
    fixed = [r for r in range(len(rows)) if TRACE not in rows[r]]
    assert names.index("all_fixed") in fixed
    coeff = np.abs(qil.coefficient_batch(psi, rows[fixed])) ** 2
    assert np.all(np.abs(got[fixed] - coeff) <= 1e-12 * total)
    assert abs(got[names.index("all_traced")] - (amp * qil.norm(psi)) ** 2) <= 1e-12 * total
    worst = 0.0
    for r in range(len(rows)):
        if r in fixed:                                   # restrict rejects a spec that keeps no site: covered above
            continue
        part = qil.restrict(psi, np.where(rows[r] == TRACE, KEEP, rows[r]).astype(np.uint8))
        dev = abs(got[r] - (part.amplitude * qil.norm(part)) ** 2) / total
        worst = max(worst, dev)
        assert dev <= 1e-12, (case, names[r], dev)
    print(f"weight_batch vs restrict + norm, {case} {np.dtype(dt).name}: worst deviation {worst:.2e} of the total weight")


# ---------------------------------------------------------------- 3. additivity
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES)
def test_a_traced_site_is_the_sum_of_its_two_fixings(qil, case, dt):
    data, P, names, rows, ref, total = _case(case, dt)
    psi = _mps(qil, data, True, _amp(dt))
    rng = np.random.default_rng(31)
    traced = [r for r in range(len(rows)) if TRACE in rows[r]]
    split = []
    for r in traced:
        k = int(rng.choice(np.flatnonzero(rows[r] == TRACE)))
        for b in (0, 1):
            s = rows[r].copy(); s[k] = b; split.append(s)
    whole = qil.weight_batch(psi, rows[traced])
    halves = qil.weight_batch(psi, np.array(split)).reshape(-1, 2)
    assert np.all(np.abs(halves[:, 0] + halves[:, 1] - whole) <= 1e-12 * total)


# ---------------------------------------------------------------- 4. row independence
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", LDS_CASES)
def test_lds_rows_are_bit_identical_alone_in_a_batch_and_again(qil, case, dt):
    """3000 rows (more rows than CUs) in seeded order: bit-equal to the same rows one by one (32 of them) and to a second run."""
    data, P, names, rows, ref, total = _case(case, dt)
    psi = _mps(qil, data, False, _amp(dt))
    rng = np.random.default_rng(41)
    n = rows.shape[1]
    big = rng.integers(0, 3, size=(3000, n)).astype(np.uint8)
    big[:len(rows)] = rows
    big = big[rng.permutation(3000)]
    first = qil.weight_batch(psi, big)
    assert np.array_equal(first, qil.weight_batch(psi, big))
    for r in rng.choice(3000, size=32, replace=False):
        assert qil.weight_batch(psi, big[r:r + 1])[0] == first[r], r
    assert np.all(np.isfinite(first)) and first.min() >= -1e-12 * total


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_gemm_route_rows_across_chunk_boundaries(qil, dt):
    """Just above the LDS limit: a row count that crosses two chunk boundaries of the 64 MiB budget, against the dense sum."""
    data, P, names, rows, ref, total = _case("above", dt)
    chi = max(_profile("above", dt))
    chunk = GEMM_BUDGET // (4 * chi * chi * np.dtype(dt).itemsize)
    nb = 2 * chunk + 5
    assert nb > 2 * chunk and chunk >= 1
    psi = _mps(qil, data, False, _amp(dt))
    pick = np.random.default_rng(43).integers(0, len(rows), size=nb)
    got = qil.weight_batch(psi, rows[pick])
    err = np.abs(got - ref[pick]) / total
    print(f"GEMM route, {nb} rows in chunks of {chunk}, {np.dtype(dt).name}: worst deviation {err.max():.2e} of the total weight")
    assert np.all(err <= 1e-12), err.max()


# ---------------------------------------------------------------- 5. front-ends
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_range_weight_bit_probabilities_and_quantiles(qil, dt):
    data, P, names, rows, ref, total = _case("sat8", dt)
    amp = _amp(dt)
    n = len(data)
    N = 2 ** n
    psi = _mps(qil, data, False, amp)
    w = amp * amp * P.reshape(-1)                         # x big-endian: the first tensor is the most significant bit
    rng = np.random.default_rng(51)
    ranges = [(5, 5), (0, N), (77, 78), (1, N - 1), (N // 2 - 37, N // 2 + 300)]
    ranges += [tuple(sorted(int(v) for v in rng.integers(0, N + 1, size=2))) for _ in range(8)]
    for lo, hi in ranges:
        got = qil.range_weight(psi, lo, hi)
        # every dyadic block is one row, good to 1e-12 of the total; their sum to that times the number of blocks
        nblocks = max(len(qil.ops._dyadic_blocks(lo, hi, n)), 1)
        assert isinstance(got, float) and abs(got - w[lo:hi].sum()) <= nblocks * 1e-12 * total, (lo, hi)
    # P(bit i = 1): a ratio of two weights, each good to 1e-12 of the total, the ratio at most 1 -> 2e-12
    marg = np.array([np.take(P, 1, axis=i).sum() for i in range(n)]) / P.sum()
    got = qil.bit_probabilities(psi)
    assert got.shape == (n,) and np.all(np.abs(got - marg) <= 2e-12)
    # quantiles: targets at least 1e-9 of the total away from every cumulative value, so that rounding cannot move the answer
    cum = np.cumsum(w)
    qs = []
    while len(qs) < 8:
        q = float(rng.uniform(0.0, 1.0))
        if np.abs(cum - q * cum[-1]).min() >= 1e-9 * cum[-1]:
            qs.append(q)
    want = np.searchsorted(cum, np.array(qs) * cum[-1], side="left")
    got = qil.weight_quantiles(psi, qs)
    assert np.array_equal(got, want), (qs, got, want)
    assert qil.weight_quantiles(psi, []).shape == (0,)
    # reverse=True: the first tensor is the least significant bit (the order of a QFT output)
    wr = amp * amp * P.transpose(list(range(n - 1, -1, -1))).reshape(-1)
    for lo, hi in ranges[3:7]:
        nblocks = len(qil.ops._dyadic_blocks(lo, hi, n))
        assert abs(qil.range_weight(psi, lo, hi, reverse=True) - wr[lo:hi].sum()) <= nblocks * 1e-12 * total, (lo, hi)
    cum = np.cumsum(wr)
    qs = []
    while len(qs) < 4:
        q = float(rng.uniform(0.0, 1.0))
        if np.abs(cum - q * cum[-1]).min() >= 1e-9 * cum[-1]:
            qs.append(q)
    assert np.array_equal(qil.weight_quantiles(psi, qs, reverse=True), np.searchsorted(cum, np.array(qs) * cum[-1], side="left"))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_zt_row_and_column_weights_against_the_dense_grid(qil, dt):
    """A 2 x 5-tensor ZTMPS: tensor 2 i is bit i (lsb first) of k, tensor 2 i + 1 bit i of l."""
    n = 5
    rng = np.random.default_rng(61 + (dt == np.complex128))
    data = random_mps_data([2, 4, 6, 8, 9, 8, 4, 3, 2], rng, dt)
    amp = _amp(dt)
    psi = qil.ZTMPS(data, amplitude=amp)
    P = np.abs(dense_mps(data)) ** 2
    order = [2 * i for i in range(n - 1, -1, -1)] + [2 * i + 1 for i in range(n - 1, -1, -1)]
    grid = amp * amp * P.transpose(order).reshape(2 ** n, 2 ** n)     # grid[k, l] = |Z(k, l)|^2
    total = grid.sum()
    idx = np.arange(2 ** n)
    assert np.all(np.abs(qil.zt_row_weights(psi, idx) - grid.sum(axis=0)) <= 1e-12 * total)
    assert np.all(np.abs(qil.zt_column_weights(psi, idx) - grid.sum(axis=1)) <= 1e-12 * total)
    sel = [7, 0, 31, 7]
    assert np.all(np.abs(qil.zt_row_weights(psi, sel) - grid.sum(axis=0)[sel]) <= 1e-12 * total)
    assert abs(qil.zt_column_weights(psi, 9)[0] - grid[9].sum()) <= 1e-12 * total


# ---------------------------------------------------------------- 6. errors and edge cases
def test_errors_and_edge_cases(qil):
    L = importlib.import_module("qilaplace_jl_amd._lib")
    rng = np.random.default_rng(71)
    psi = qil.SignalMPS(random_mps_data([2, 4, 2], rng))
    with pytest.raises(ValueError, match=r"outside \[0,2\]"):
        qil.weight_batch(psi, [[2, 3, 2, 2]])
    # the library's own checks, behind the front-end's
    out = (C.c_double * 2)(-7.0, -7.0)
    sp = (C.c_uint8 * 8)(0, 1, 2, 0, 2, 3, 2, 2)
    assert L.lib.qil_weight_batch(psi.handle, 2, sp, out) == L.QIL_EINVAL_CONFIG
    assert "spec value 3 outside [0,2]" in L.last_error() and list(out) == [-7.0, -7.0]
    assert L.lib.qil_weight_batch(psi.handle, -1, sp, out) == L.QIL_EINVAL_ARG
    assert L.lib.qil_weight_batch(psi.handle, 0, sp, out) == L.QIL_OK and list(out) == [-7.0, -7.0]     # nb = 0: a no-op
    assert L.lib.qil_weight_batch(psi.handle, 0, None, None) == L.QIL_OK
    assert qil.weight_batch(psi, np.zeros((0, 4))).shape == (0,)
    for dt in DTYPES:
        zero = qil.SignalMPS([np.zeros(t.shape, dtype=dt) for t in random_mps_data([2, 3, 5, 7, 5, 3, 2], rng)], amplitude=3.0)
        rows = rng.integers(0, 3, size=(9, 8)).astype(np.uint8)
        assert np.array_equal(qil.weight_batch(zero, rows), np.zeros(9))


def test_single_site_chain(qil):
    A = np.array([0.25, -1.5]).reshape(1, 2, 1)
    psi = qil.SignalMPS([A], amplitude=3.0)
    got = qil.weight_batch(psi, [[0], [1], [2]])
    assert np.allclose(got, 9.0 * np.array([0.0625, 2.25, 2.3125]), rtol=1e-15, atol=0)


def test_allocation_failure_leaves_nothing_behind(qil):
    """Fault injection (a host-side refusal by the pool) at every allocation of a call on the GEMM route, where temporaries exist:
    the call raises the allocation error, nothing is stranded, `out` is the caller's to ignore, and the call then succeeds."""
    data, P, names, rows, ref, total = _case("above", np.float64)
    ctx = qil.default_context()
    psi = _mps(qil, data, False, _amp(np.float64))
    failures, got = 0, None
    for j in range(60):
        ctx.fail_alloc_after(j)
        try:
            got = qil.weight_batch(psi, rows)
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        assert ctx.unowned_bytes() == 0, j
        if not failed:
            break
        failures += 1
    assert got is not None and failures >= 6, failures      # the spec copy, the result and the four chi^2 buffers
    assert np.all(np.abs(got - ref) <= 1e-12 * total)
    assert all(np.array_equal(psi.site(i), data[i]) for i in range(len(data)))


# ---------------------------------------------------------------- 7. full size
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_full_size_row_weights_against_restrict_and_norm(qil, dt):
    """n = 24 paired, bonds 64: 8 rows of the zt_row_weights shape against restrict + norm, 1e-10 relative.  c64 is the case the
    z-plane work runs (64 > 48: the GEMM route); f64 at the same bonds walks in LDS."""
    n = 24
    psi = qil.ZTMPS.alloc(saturated_profile(2 * n, 64), dtype=dt, amplitude=2.5).fill_random(20241018)
    rng = np.random.default_rng(81)
    ls = [int(v) for v in rng.integers(0, 2 ** n, size=8)]
    got = qil.zt_row_weights(psi, ls)
    ref = np.array([(2.5 * qil.norm(qil.zt_row(psi, l))) ** 2 for l in ls])
    rel = np.abs(got - ref) / ref
    print(f"full-size zt_row_weights {np.dtype(dt).name}: worst relative deviation {rel.max():.2e}")
    assert np.all(ref > 0) and np.all(rel <= 1e-10), rel.max()


# ---------------------------------------------------------------- 8. the example
def test_band_power_example_checks_itself(qil, capsys):
    """examples/band_power.py asserts every figure it prints against the dense vector; run in this process."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("band_power", os.path.join(root, "examples", "band_power.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bands, (rows, cols) = mod.main()
    assert 0 <= bands["median"] <= bands["edge95"] < 2 ** 14 and rows.shape == cols.shape == (256,)
    assert "median frequency" in capsys.readouterr().out
