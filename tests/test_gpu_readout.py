"""The read-out on the device against longdouble references, case by case (tests/readout_cases.py): coefficient_batch,
marginal_batch, apply_coefficient_batch, apply_coefficient_sweep, mps_block / mps_to_vector, coefficient_grid, laplace_values.

Which route a case reaches -- per-query chain, selecting GEMM, sorted GEMM, lazy chain, lazy GEMM -- is asserted without a GPU in
tests/test_readout_cases_oracle.py; here the table is RUN:
  * every query within its OWN rounding bound of the reference (readout_cases: bound_q = |amplitude| mag_q (prod (1 + gamma) - 1)); on
    cone data that is <= 2e-13 of the coefficient's own modulus although a batch spans up to nine decades, so a query that is 1e-9
    of the peak is checked to 13 digits as well;
  * random data: also the project's batch-relative `rel < 1e-12`;
  * a repeated call returns the same bits; equal queries return equal bits; a real chain returns a zero imaginary part;
  * reads only what it selects: with NaN in the physical slice (lazy: the output bit of W) that no query selects, every route
    returns the bits of the clean run;
  * a basis state gives exactly `amplitude` at its configuration and exactly 0.0 elsewhere, on every route;
  * an allocation failure anywhere inside a call leaves no device memory behind and the operands usable;
  * what the verbs refuse.
Each test prints its figures (pytest -s): worst err / bound, worst per-coefficient relative error, device time."""
import ctypes as C
import gc
import importlib
import time

import numpy as np
import pytest

import readout_cases as R

pytestmark = pytest.mark.gpu


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


def _raw(qil, entry, handles, bits):
    """The verb through the C ABI with the output prefilled with NaN: every complex value as the library wrote it."""
    L = importlib.import_module("qilaplace_jl_amd._lib")
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    out = np.full(len(b), np.nan + 1j * np.nan, dtype=np.complex128)
    L.check(getattr(L.lib, entry)(*handles, len(b), b.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _psi(qil, data, paired=False):
    return (qil.ZTMPS if paired else qil.SignalMPS)(data, amplitude=R.AMPLITUDE)


def _sweep_handles(qil, c, ops):
    """One handle per operator NAME: a name that repeats in the list is the same handle twice."""
    return {op: qil.SingleSiteMPO(w) for op, w in ops.items()}


def device_result(qil, c):
    """The device's answer in the layout of readout_cases.reference(c)."""
    p = c.p
    if c.kind == "chain":
        data, bits = R.operands(c)
        psi = _psi(qil, data)
        got = (qil.coefficient_batch if c.verb == "plain" else qil.marginal_batch)(psi, bits)
        raw = _raw(qil, "qil_coefficient_batch" if c.verb == "plain" else "qil_coefficient_marginal_batch", [psi.handle], bits)
        return got, raw
    if c.kind == "lazy":
        w, a, bits = R.operands(c)
        W, psi = qil.SingleSiteMPO(w), _psi(qil, a)
        return qil.apply_coefficient_batch(W, psi, bits), _raw(qil, "qil_apply_coefficient_batch", [W.handle, psi.handle], bits)
    if c.kind == "sweep":
        a, ops, bits = R.operands(c)
        psi, Ws = _psi(qil, a), _sweep_handles(qil, c, ops)
        before = {op: (W * psi).to_host() for op, W in Ws.items()}
        out = qil.apply_coefficient_sweep([Ws[op] for op in p["ops"]], psi, bits)
        assert out.shape == (len(p["ops"]), len(bits)) and out.dtype == np.complex128
        got = {}
        for row, op in zip(out, p["ops"]):
            if op in got:                                  # the same handle twice: the same values twice
                assert np.array_equal(row, got[op]), op
            got[op] = row
        for op, W in Ws.items():                           # every operator is back in its home context (apply insists), unchanged
            after = (W * psi).to_host()
            assert all(np.array_equal(x, y) for x, y in zip(before[op], after)), op
        return got, None
    psi = _psi(qil, R.operands(c), paired=c.kind != "block" or p["paired"])
    if c.kind == "block":
        got = {(label, rev): qil.mps_block(psi, s, reverse=rev) for label, s in R.block_specs() for rev in (False, True)}
        for rev in (False, True):                          # mps_to_vector is the all-free block
            assert np.array_equal(qil.mps_to_vector(psi, reverse=rev), got[("all_free", rev)])
        return got, None
    if c.kind == "grid":
        return {label: qil.coefficient_grid(psi, ks, ls) for label, ks, ls in R.grid_axes()}, None
    return {label: qil.laplace_values(psi, ks, R.LAPLACE_DT) for label, ks in R.laplace_axes()}, None


def _same_bits(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same_bits(a[k], b[k]) for k in a)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_device_within_bound(qil, c):
    ref = R.reference(c)
    t0 = time.perf_counter()
    got, raw = device_result(qil, c)
    ms = 1e3 * (time.perf_counter() - t0)
    again, _ = device_result(qil, c)
    assert _same_bits(got, again), "a repeated call returned other bits"
    real = c.dtype == "f64"
    if raw is not None:
        assert np.isfinite(raw.view(np.float64)).all()
        assert np.array_equal(raw.real if real else raw, got)
        if real:
            assert not raw.imag.any(), "a real chain returned an imaginary part"
    pairs = [(k, got[k], ref[k]) for k in ref] if isinstance(ref, dict) else [("", got, ref)]
    ratio = relerr = batch_rel = 0.0
    for key, g, r in pairs:
        if c.kind == "sweep":
            if R.sweep_dtype(c, key) == "f64":
                assert not g.imag.any(), (key, "a real product returned an imaginary part")
                g = g.real
        elif c.kind == "grid":                            # always complex128, as the reference's scan
            assert g.dtype == np.complex128
            if real:
                assert not g.imag.any()
                g = g.real
        else:
            assert g.dtype == (np.float64 if real else np.complex128), key
        ratio = max(ratio, R.check(g, r, (c.name, key)))
        if c.family == "random":
            batch_rel = max(batch_rel, R.rel(g, r.value))
        else:
            relerr = max(relerr, R.worst_relative(g, r))
    print(f"\nREADOUT {c.name} kind={c.kind} route={c.route} family={c.family} err/bound={ratio:.3e} cone_rel={relerr:.3e} "
          f"batch_rel={batch_rel:.3e} first_call_ms={ms:.1f}")
    if c.family == "random":
        assert batch_rel < 1e-12
    if c.kind == "chain" and c.p["pattern"] == "equal":
        assert len(set(got.tolist())) == 1, "equal queries returned different values"
    if c.kind == "chain" and c.p["pattern"] == "m_wide":   # the all-2 row against the sum of the dense tensor
        value, mag = R.all_two_row_reference(c)
        assert abs(np.clongdouble(got[1]) - value) <= R.bound(mag / R.AMPLITUDE, R.chain_qs(R.dims_of(c.p["bonds"])))


# ---------------------------------------------------------------- reads only what it selects
def _poisoned(data, site, index):
    out = [t.copy() for t in data]
    out[site][index] = np.nan
    return out


NAN_CASES = [("CHAIN", "chain15_nb300", 7), ("GEMM_SORTED", "sortA_nb97_random", 4), ("GEMM_SELECT", "selectA_nb97_m_none", 4),
             ("LAZY_CHAIN", "lazy_small_nb200", 3), ("LAZY_GEMM", "lazy_32x32_nb16", 1)]


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("route,name,site", NAN_CASES, ids=[r for r, _, _ in NAN_CASES])
def test_reads_only_the_selected_slice(qil, route, name, site, dt):
    """The slice of one wide site that no query of the batch selects holds NaN (a copy of the state, uploaded with NaNs): the
    results are finite and the bits of the clean run.  Lazy routes: the entries of W for the output bit no query asks for."""
    lazy = route.startswith("LAZY")
    c = R.BY_NAME[f"{name}-W{dt}-psi{dt}-cone" if lazy else f"{name}-{dt}-cone"]
    assert c.route == route
    for keep in (0, 1):
        if lazy:
            w, a, bits = R.operands(c)
            bits = bits.copy()
            bits[:, site] = keep
            psi = _psi(qil, a)
            run = lambda wd: qil.apply_coefficient_batch(qil.SingleSiteMPO(wd), psi, bits)
            clean, dirty = run(w), run(_poisoned(w, site, (slice(None), slice(None), 1 - keep)))
        else:
            data, bits = R.operands(c)
            bits = bits.copy()
            bits[:, site] = keep
            fn = qil.coefficient_batch if c.verb == "plain" else qil.marginal_batch
            clean, dirty = (fn(_psi(qil, d), bits) for d in (data, _poisoned(data, site, (slice(None), 1 - keep))))
        assert np.isfinite(dirty).all() and _same_bits(clean, dirty), (route, keep)


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_block_reads_only_the_fixed_slice(qil, dt):
    data = R.mps_data("cone", dt, R.BLOCK_BONDS, "block")
    for spec in ([3, 3, 2, 1, 0, 1, 3, 2, 3, 0], [3, 2, 3, 0, 1, 1, 2, 0, 1, 2]):      # site 4 fixed: left of / behind the last free site
        spec = np.array(spec, dtype=np.uint8)
        for keep in (0, 1):
            spec[4] = keep
            clean = qil.mps_block(_psi(qil, data), spec)
            dirty = qil.mps_block(_psi(qil, _poisoned(data, 4, (slice(None), 1 - keep))), spec)
            assert np.isfinite(dirty).all() and _same_bits(clean, dirty), (spec, keep)


# ---------------------------------------------------------------- exact values
def _basis_bits(config, nb, rng, summed=0):
    bits = rng.integers(0, 2, size=(nb, len(config)), dtype=np.uint8)
    bits[::5] = config                                     # every fifth query IS the configuration
    if summed:
        bits[rng.random(bits.shape) < 0.3] = 2
    hit = ((bits == config) | (bits == 2)).all(axis=1)
    return bits, hit


@pytest.mark.parametrize("verb,route,bonds,nb", [("plain", "CHAIN", R.CHAIN15, 300), ("marginal", "CHAIN", R.CHAIN15, 300),
                                                 ("plain", "GEMM_SORTED", R.SORT_A, 97), ("marginal", "GEMM_SELECT", R.SORT_A, 97),
                                                 ("plain", "GEMM_SORTED", R.SORT_B, 1024), ("marginal", "GEMM_SELECT", R.SORT_B, 1024)])
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_basis_state_is_exact(qil, verb, route, bonds, nb, dt):
    """A basis state whose bonds are padded with zero rows: exactly `amplitude` at its configuration (a summed site adds 1 + 0),
    exactly 0.0 elsewhere."""
    assert qil.readout_route(verb, nb, R.dims_of(bonds))[0] == route
    rng = np.random.default_rng(len(bonds) * nb)
    config = rng.integers(0, 2, size=len(bonds) + 1)
    bits, hit = _basis_bits(config, nb, rng, summed=verb == "marginal")
    assert hit.any() and not hit.all()
    psi = _psi(qil, R.basis_mps_data(config, bonds, R.DTYPES[dt]))
    got = (qil.coefficient_batch if verb == "plain" else qil.marginal_batch)(psi, bits)
    assert np.array_equal(got, np.where(hit, R.AMPLITUDE, 0.0).astype(got.dtype))


@pytest.mark.parametrize("route,bonds,nb", [("LAZY_CHAIN", R.LAZY_PSI, 200), ("LAZY_GEMM", (32, 32), 16), ("LAZY_GEMM", R.RAGGED_PSI, 200)])
@pytest.mark.parametrize("wdt,adt", R.PAIRS)
def test_flipped_basis_state_is_exact(qil, route, bonds, nb, wdt, adt):
    """<bits| X^f |config> through the lazy verb, W the bit-flip operator with zero-padded bonds: amplitude at config ^ f, else 0.0."""
    wbonds = {R.LAZY_PSI: R.LAZY_W, R.RAGGED_PSI: R.RAGGED_W}.get(bonds, (32, 32))
    assert qil.readout_route("lazy", nb, R.dims_of(bonds), R.dims_of(wbonds))[0] == route
    rng = np.random.default_rng(len(bonds) + nb)
    config, flips = rng.integers(0, 2, size=(2, len(bonds) + 1))
    bits, hit = _basis_bits(config ^ flips, nb, rng)
    W = qil.SingleSiteMPO(R.flip_mpo_data(flips, wbonds, R.DTYPES[wdt]))
    got = qil.apply_coefficient_batch(W, _psi(qil, R.basis_mps_data(config, bonds, R.DTYPES[adt])), bits)
    assert hit.any() and np.array_equal(got, np.where(hit, R.AMPLITUDE, 0.0).astype(got.dtype))


def test_basis_state_through_the_dense_front_ends(qil):
    config = np.array([1, 0, 0, 1, 1, 0, 1, 0, 1, 1])
    psi = _psi(qil, R.basis_mps_data(config, R.BLOCK_BONDS), paired=True)
    j = int("".join(map(str, config)), 2)
    want = np.zeros(1024)
    want[j] = R.AMPLITUDE
    assert np.array_equal(qil.mps_to_vector(psi), want)
    k, l = (sum(int(b) << i for i, b in enumerate(config[o::2])) for o in (0, 1))
    grid = np.zeros((32, 32), dtype=np.complex128)
    grid[k, l] = R.AMPLITUDE
    assert np.array_equal(qil.coefficient_grid(psi, np.arange(32), np.arange(32)), grid)
    perm = np.random.default_rng(3).permutation(32)
    assert np.array_equal(qil.coefficient_grid(psi, perm, perm), grid[np.ix_(perm, perm)])


# ---------------------------------------------------------------- allocation failures
def _failing_then_working(qil, call, operands_ok):
    """Whichever allocation inside `call` fails: MemoryError, nothing left behind, operands usable; then the call succeeds."""
    ctx = qil.default_context()
    assert ctx.unowned_bytes() == 0
    want = call()
    failures = 0
    for k in list(range(0, 12)) + [20, 40, 80, 160, 320, 640]:
        ctx.fail_alloc_after(k)
        try:
            out = call()
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        if not failed:
            assert _same_bits(out, want)
            break                                          # the call needs fewer than k allocations
        failures += 1
        assert ctx.unowned_bytes() == 0, k                 # every temporary is back in the pool
        operands_ok()
    assert failures >= 1
    assert _same_bits(call(), want)
    assert ctx.unowned_bytes() == 0


def test_failed_readouts_leave_no_device_memory_behind(qil):
    c = R.BY_NAME["selectA_nb97_m_wide-c64-cone"]
    data, bits = R.operands(c)
    psi = _psi(qil, data)
    norm = qil.norm(psi)
    ok = lambda: np.testing.assert_equal(qil.norm(psi), norm)
    _failing_then_working(qil, lambda: qil.marginal_batch(psi, bits), ok)
    spec = dict(R.block_specs())["wide_in_right_fold"]
    blk = _psi(qil, R.mps_data("cone", "c64", R.BLOCK_BONDS, "block"))
    _failing_then_working(qil, lambda: qil.mps_block(blk, spec), lambda: np.isfinite(qil.norm(blk)))
    c = R.BY_NAME["lazy_32x32_nb16-Wc64-psif64-cone"]
    w, a, bits = R.operands(c)
    W, phi = qil.SingleSiteMPO(w), _psi(qil, a)
    before = (W * phi).to_host()
    same = lambda: all(np.array_equal(x, y) for x, y in zip((W * phi).to_host(), before))
    _failing_then_working(qil, lambda: qil.apply_coefficient_batch(W, phi, bits), lambda: same() or pytest.fail("operands changed"))
    # the smallest c64 case of each route whose temporaries belong to the read-out's own scratch: the per-query chain, the sorted
    # GEMM form (which builds a plan) and the lazy chain
    for name, route in (("one_site_plain-c64-cone", "CHAIN"), ("threshold_nb4_bond128_plain-c64-cone", "GEMM_SORTED")):
        c = R.BY_NAME[name]
        assert c.route == route
        data, cbits = R.operands(c)
        chi = _psi(qil, data)
        cnorm = qil.norm(chi)
        _failing_then_working(qil, lambda: qil.coefficient_batch(chi, cbits), lambda: np.testing.assert_equal(qil.norm(chi), cnorm))
    c = R.BY_NAME["lazy_small_nb1-Wc64-psic64-cone"]
    assert c.route == "LAZY_CHAIN"
    w, a, bits = R.operands(c)
    W, phi = qil.SingleSiteMPO(w), _psi(qil, a)
    before = (W * phi).to_host()
    _failing_then_working(qil, lambda: qil.apply_coefficient_batch(W, phi, bits), lambda: same() or pytest.fail("operands changed"))


def test_failed_sweep_returns_its_operators_home(qil):
    c = R.BY_NAME["sweep_nw9-psic64-cone"]
    a, ops, bits = R.operands(c)
    psi, Ws = _psi(qil, a), _sweep_handles(qil, c, ops)
    before = {op: (W * psi).to_host() for op, W in Ws.items()}

    def operators_ok():
        for op, W in Ws.items():                           # usable, in their home context, unchanged
            assert all(np.array_equal(x, y) for x, y in zip((W * psi).to_host(), before[op])), op

    _failing_then_working(qil, lambda: qil.apply_coefficient_sweep([Ws[op] for op in c.p["ops"]], psi, bits), operators_ok)


# ---------------------------------------------------------------- what the verbs refuse
def test_errors_and_empty_batches(qil):
    L = importlib.import_module("qilaplace_jl_amd._lib")
    a = R.mps_data("random", "f64", R.SWEEP_PSI, "sweep", 2)
    w = R.mpo_data("random", "c64", R.SWEEP_OPS["narrow_c"][1], "narrow_c")
    psi, W = _psi(qil, a), qil.SingleSiteMPO(w)
    n = len(a)
    for bad, entry, handles in ((3, "qil_coefficient_marginal_batch", [psi.handle]), (2, "qil_coefficient_batch", [psi.handle]),
                                (2, "qil_apply_coefficient_batch", [W.handle, psi.handle])):
        with pytest.raises(ValueError, match=f"bit value {bad} outside"):           # the library's own check ...
            _raw(qil, entry, handles, np.full((2, n), bad))
    with pytest.raises(ValueError, match="bit value 2 outside"):
        hs = (C.c_void_p * 1)(W.handle)
        out = np.zeros(2, dtype=np.complex128)
        b = np.full((2, n), 2, dtype=np.uint8)
        L.check(L.lib.qil_apply_coefficient_sweep(hs, 1, psi.handle, 2, b.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  out.ctypes.data_as(C.POINTER(C.c_double))))
    for call in (lambda: qil.marginal_batch(psi, np.full((1, n), 3)), lambda: qil.coefficient_batch(psi, np.full((1, n), 2)),
                 lambda: qil.apply_coefficient_batch(W, psi, np.full((1, n), 2)),
                 lambda: qil.apply_coefficient_sweep([W], psi, np.full((1, n), 2))):
        with pytest.raises(ValueError, match="outside"):                            # ... and the front-end's
            call()
    bits = np.zeros((4, n), dtype=np.uint8)
    short = qil.SingleSiteMPO(w[:-2] + [w[-2][..., :1]])
    other = qil.SingleSiteMPO(w, sites=list(range(11, 11 + n)))
    for call in (lambda: qil.apply_coefficient_batch(short, psi, bits), lambda: qil.apply_coefficient_sweep([W, short], psi, bits)):
        with pytest.raises(ValueError, match="same number of sites"):
            call()
    for call in (lambda: qil.apply_coefficient_batch(other, psi, bits), lambda: qil.apply_coefficient_sweep([W, other], psi, bits)):
        with pytest.raises(ValueError, match="same site indices"):
            call()
    none = np.zeros((0, n), dtype=np.uint8)
    assert qil.coefficient_batch(psi, none).shape == (0,) and qil.marginal_batch(psi, none).shape == (0,)
    assert qil.apply_coefficient_batch(W, psi, none).shape == (0,)
    assert qil.apply_coefficient_sweep([W], psi, none).shape == (1, 0)
    assert qil.apply_coefficient_sweep([], psi, bits).shape == (0, 4)
    assert np.array_equal(qil.apply_coefficient_sweep([W], psi, bits)[0], qil.coefficient_batch(W * psi, bits))
