"""GPU tests of the operator-valued verbs: W1 * W2 (qil_apply_mpo_mpo) and mpo_compress (qil_mpo_compress, qil_mpo_compress_batch),
on the table of tests/mpo_cases.py -- the same assertions tests/test_mpo_cases_oracle.py makes of the oracle on the CPU.

Composition: every site against a longdouble einsum with the componentwise bound 8 eps (|W1| o |W2|), sites outside the window bit
for bit, then as dense operators and on a state (1e-13 of the product of norms).  Compression: lossless within 8 x the oracle's own
error on the same input (floor N eps) with the oracle's bond dimensions where they are comparable; truncated within the TT-SVD
bound sum_k tail_k^2 of the exact operator's singular values; the gauge the call promises to 1e-10.  Then edges, errors, failed
allocations and the batch verb."""
import gc

import numpy as np
import pytest

from helpers import random_mpo_data, dense_mpo, dense_mps
import mpo_cases as MC

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
    assert qil.default_context().unowned_bytes() == 0


def _mpo(qil, data, paired, sites=None, ctx=None):
    return (qil.PairedSiteMPO if paired else qil.SingleSiteMPO)([np.array(t) for t in data], sites=sites, ctx=ctx)


def _operands(qil, name):
    c = next(c for c in MC.COMPOSE if c.name == name)
    w1, w2 = MC.compose_operands(name)
    return _mpo(qil, w1, c.paired, c.first.sites), _mpo(qil, w2, c.paired, c.second.sites)


def _product(W):
    return MC.Product(W.to_host(), W.dtype, W.paired, W.site_ids, W.bond_dims)


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- composition
@pytest.mark.parametrize("name", [c.name for c in MC.COMPOSE])
def test_product_sites_against_longdouble(qil, name):
    c = next(c for c in MC.COMPOSE if c.name == name)
    W1, W2 = _operands(qil, name)
    W12 = W1 * W2
    assert type(W12) is (qil.PairedSiteMPO if c.paired else qil.SingleSiteMPO)
    got = _product(W12)
    worst = MC.check_product_sites(name, got)
    print(f"product {name}: worst site error {worst:.3f} of the bound")
    if len(got.data) <= 6:
        MC.check_product_dense(name, got)
    w1, w2 = MC.compose_operands(name)                                  # the operands are read-only
    assert _same(W1.to_host(), [np.asarray(t) for t in w1]) and _same(W2.to_host(), [np.asarray(t) for t in w2])


@pytest.mark.parametrize("name", MC.COMPOSE_ON_STATE)
def test_product_on_a_state_w1_acts_first(qil, name):
    c = next(c for c in MC.COMPOSE if c.name == name)
    W1, W2 = _operands(qil, name)
    a = MC.compose_state(name)
    psi = (qil.ZTMPS if c.paired else qil.SignalMPS)(a, sites=c.first.sites)
    v12 = dense_mps(((W1 * W2) * psi).to_host())
    v21 = dense_mps((W2 * (W1 * psi)).to_host())
    MC.check_product_on_state(name, v12, v21)


# ---------------------------------------------------------------- compression
def _compress(qil, name, direction, mode):
    c = MC.compress_case(name)
    _, cutoff, capped = next(m for m in MC.MODES if m[0] == mode)
    W = _mpo(qil, MC.compress_input(name), c.paired)
    assert qil.mpo_compress(W, direction, cutoff=cutoff, maxdim=c.maxdim if capped else None) is W
    data = W.to_host()
    assert W.bond_dims == MC.bonds_of(data) and W.dtype == c.dtype and W.paired == c.paired
    return data


@pytest.mark.parametrize("direction", MC.DIRECTIONS)
@pytest.mark.parametrize("name", [c.name for c in MC.COMPRESS])
def test_compress_lossless(qil, name, direction):
    data = _compress(qil, name, direction, "lossless")
    gauge = MC.check_gauge(name, direction, data)
    err = MC.lossless_error(name, data)
    print(f"lossless {name} {direction}: device {err:.2e}, oracle {MC.oracle_lossless_error(name, direction):.2e}, bonds {MC.bonds_of(data)}, "
          f"oracle {MC.bonds_of(MC.oracle_compress(name, direction, 'lossless'))}, gap {MC.has_gap(name, direction)}, gauge {gauge:.1e}")
    MC.check_lossless(name, direction, data)
    # the device's one-site SVD never grows a bond (the oracle's two-site SVD does: where has_gap declines, this is the bond check)
    assert all(g <= b for g, b in zip(MC.bonds_of(data), MC.bonds_of(MC.compress_input(name)))), (name, direction)


@pytest.mark.parametrize("mode", ["cutoff", "maxdim"])
@pytest.mark.parametrize("direction", MC.DIRECTIONS)
@pytest.mark.parametrize("name", [c.name for c in MC.COMPRESS])
def test_compress_truncated(qil, name, direction, mode):
    """TT-SVD bound, bond limits, gauge, and after "down" the agreement with the oracle's truncation on a state (1e-9).  The last one
    is what caps the weight the deflated one-factor SVD may drop (svd_trunc_dev): uncapped, n7-real-single-inflated measured 1.19e-9."""
    data = _compress(qil, name, direction, mode)
    MC.check_gauge(name, direction, data)
    print(f"truncated {name} {direction} {mode}: bonds {MC.bonds_of(data)}, oracle {MC.bonds_of(MC.oracle_compress(name, direction, mode))}")
    err2, tails = MC.check_truncated(name, direction, mode, data)
    print(f"    error^2 {err2:.3e}, tails {tails:.3e}")
    if direction == "down":
        print(f"    against the oracle on a state {MC.check_against_oracle_on_state(name, mode, data):.2e}")


# ---------------------------------------------------------------- edges and errors
def test_edges_and_errors(qil):
    rng = np.random.default_rng(31)
    for dt in (np.float64, np.complex128):                                # (a paired operator has at least two tensors)
        one = random_mpo_data([], rng, dt)
        W = _mpo(qil, one, False)
        for direction in MC.DIRECTIONS:                                   # N = 1: nothing to do, nothing touched
            qil.mpo_compress(W, direction, cutoff=1e-3, maxdim=1)
            assert _same(W.to_host(), one)
    w = MC.compress_input("n6-complex-single")
    none, zero = _mpo(qil, w, False), _mpo(qil, w, False)
    qil.mpo_compress(none, "down", cutoff=0.0, maxdim=None)
    qil.mpo_compress(zero, "down", cutoff=0.0, maxdim=0)                  # 0 means "no cap" too
    assert none.bond_dims == zero.bond_dims == MC.bonds_of(w) and _same(none.to_host(), zero.to_host())
    W = _mpo(qil, w, False)
    for bad in (lambda: qil.mpo_compress(W, "down", cutoff=-1e-9), lambda: qil.mpo_compress(W, "sideways"),
                lambda: qil.mpo_compress_batch([W], "sideways"), lambda: qil.mpo_compress_batch([W], "up", cutoff=-1.0)):
        with pytest.raises(ValueError):
            bad()
        assert _same(W.to_host(), w)                                      # a refused call leaves the operand alone
    P = _mpo(qil, w, True)
    with pytest.raises(TypeError):
        W * P
    with pytest.raises(TypeError):
        P * W
    other = qil.Context(0)
    alien = _mpo(qil, w, False, ctx=other)
    with pytest.raises(ValueError, match="different contexts"):
        W * alien
    with pytest.raises(ValueError, match="another context"):
        qil.mpo_compress_batch([W, alien], "down")
    short = random_mpo_data([3, 3], rng)
    for sa, sb in (([1, 2, 3], [2, 3, 4]), ([5, 6, 7], [1, 2, 3, 4, 5, 6])):
        A = _mpo(qil, short, False, sa)
        B = _mpo(qil, short if len(sb) == 3 else w, False, sb)
        with pytest.raises(ValueError, match="partially"):
            A * B
        assert qil.default_context().unowned_bytes() == 0
    del alien
    gc.collect()
    assert other.unowned_bytes() == 0


# ---------------------------------------------------------------- failed allocations
@pytest.mark.parametrize("call", ["product", "compress-down", "compress-up"])
def test_failed_allocations_leave_operands_whole(qil, call):
    """Whichever allocation inside W1 * W2 or mpo_compress fails: no device memory is stranded, the read-only operands are untouched
    bit for bit, the in-place operand is a chain that still stands for the input operator (to the TT-SVD bound of the bonds the call
    had truncated by then; to the lossless floor if it had truncated none), and the same call then succeeds on it with a right result.
    The compression runs at cutoff 0 with a cap, so the retry truncates no bond a second time."""
    ctx = qil.default_context()
    c = next(c for c in MC.COMPOSE if c.name == "embed-middle-base-first-base-f")       # window kernels and widening copies
    w1, w2 = MC.compose_operands(c.name)
    name = "n7-real-single-inflated"                                                    # QR, wide-site SVD and truncating SVD steps
    wc, cap = MC.compress_input(name), MC.compress_case(name).maxdim
    W1, W2 = _mpo(qil, w1, False, c.first.sites), _mpo(qil, w2, False, c.second.sites)
    direction = call.split("-")[-1]
    failures, interrupted = 0, 0
    for k in list(range(0, 12)) + [20, 40, 80, 160]:
        V = _mpo(qil, wc, False)                                         # a fresh operand: one interrupted call, one retry

        def run():
            return W1 * W2 if call == "product" else qil.mpo_compress(V, direction, cutoff=0.0, maxdim=cap)

        ctx.fail_alloc_after(k)
        try:
            out = run()
            failed = False
        except MemoryError:
            failed = True
        finally:
            ctx.fail_alloc_after(None)
        if not failed:
            break                                                        # the call needs no more than k allocations
        failures += 1
        assert ctx.unowned_bytes() == 0, (call, k)
        assert _same(W1.to_host(), [np.asarray(t) for t in w1]) and _same(W2.to_host(), [np.asarray(t) for t in w2]), (call, k)
        host = V.to_host()
        dims = [1] + V.bond_dims + [1]
        assert [t.shape for t in host] == [(dims[i], 2, 2, dims[i + 1]) for i in range(len(host))], (call, k)
        if call == "product":
            assert _same(host, wc)
            MC.check_product_sites(c.name, _product(run()))              # the same call succeeds afterwards
        else:
            err, bound = MC.check_interrupted(name, direction, host)
            interrupted += MC.bonds_of(host) != MC.bonds_of(wc)
            assert run() is V
            data = V.to_host()
            assert all(b <= cap for b in MC.bonds_of(data)), (call, k, MC.bonds_of(data))
            MC.check_gauge(name, direction, data)
            err2, bound2 = MC.check_interrupted(name, direction, data, retried=True)
            print(f"{call} k={k}: interrupted at bonds {MC.bonds_of(host)} error {err:.2e} (bound {bound:.2e}), retried {err2:.2e} ({bound2:.2e})")
        assert ctx.unowned_bytes() == 0, (call, k)
    assert failures >= 1, call
    assert call == "product" or interrupted >= 1                         # some failure fell inside the sweeps, not before them
    if call != "product":                                                # uninterrupted, for comparison: the plain bound
        V = _mpo(qil, wc, False)
        qil.mpo_compress(V, direction, cutoff=0.0, maxdim=cap)
        MC.check_truncated(name, direction, "maxdim", V.to_host())


# ---------------------------------------------------------------- batch
@pytest.mark.parametrize("direction", MC.DIRECTIONS)
def test_batch_over_a_ragged_list_equals_one_at_a_time(qil, direction):
    """mpo_compress_batch over operators of different lengths, element types and profiles (from five items on the chains advance in
    lock step): bit-identical to mpo_compress one at a time."""
    names = ["n2-real-single", "n6-complex-single", "n7-real-single-inflated", "n3-complex-single", "n10-complex-single-regimes",
             "n6-complex-single-product", "n3-real-single"]
    paired_names = ["n2-complex-paired", "n6-real-paired", "n6-complex-paired-inflated", "n10-real-paired-regimes",
                    "n6-real-paired-product"]
    for group in (names, paired_names, names[:3]):
        for cutoff, maxdim in ((MC.CUTOFF, None), (0.0, 6)):
            ref = [qil.mpo_compress(_mpo(qil, MC.compress_input(n), MC.compress_case(n).paired), direction, cutoff=cutoff, maxdim=maxdim)
                   for n in group]
            items = [_mpo(qil, MC.compress_input(n), MC.compress_case(n).paired) for n in group]
            got = qil.mpo_compress_batch(items, direction, cutoff=cutoff, maxdim=maxdim)
            assert all(g is it for g, it in zip(got, items))
            for n, r, b in zip(group, ref, items):
                assert b.bond_dims == r.bond_dims, (n, cutoff, maxdim)
                assert _same(r.to_host(), b.to_host()), (n, cutoff, maxdim)
    assert qil.mpo_compress_batch([], direction) == []
