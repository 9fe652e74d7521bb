"""The read-out case table (tests/readout_cases.py) without a GPU: which route every case reaches, and whether the inputs keep a
correct float64 evaluation inside every bound that tests/test_gpu_readout.py then asks of the device.

  * every case reaches the route written beside it (qil.readout_route: the one host function the read-out verbs switch on), so a
    re-tuned crossover that silently moves a case to another kernel fails here and the table is re-aimed;
  * the table reaches all five routes for each dtype and both sides of every threshold;
  * the numpy oracle, in the device's place, passes every assertion of the GPU file: per-query bound, `rel < 1e-12` on random data,
    equal queries give equal values;
  * on cone data the bound of every query is at most CONE_RATIO of the query's own modulus -- a condition on the inputs: it is what
    makes the check per-coefficient.
Needs the library (for the route), not a GPU.  No case is skipped or sampled."""
import numpy as np
import pytest

import oracle as O
import readout_cases as R

IDS = [c.name for c in R.CASES]


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    return q


def test_longdouble_is_wider_than_the_kernels():
    """The references need a format more precise than float64: numpy's longdouble with its 64-bit mantissa."""
    assert np.finfo(np.longdouble).nmant >= 63


def _pairs(c, got):
    ref = R.reference(c)
    if isinstance(ref, dict):
        assert set(got) == set(ref)
        return [(k, got[k], ref[k]) for k in ref]
    return [("", got, ref)]


def routes_of(qil, c):
    """Every route the device call(s) of the case take, with the queries per pass."""
    p = c.p
    dims = R.dims_of(p["bonds"])
    if c.kind == "chain":
        return [qil.readout_route(c.verb, p["nb"], dims, dtype=R.DTYPES[c.dtype])]
    if c.kind == "lazy":
        return [qil.readout_route("lazy", p["nb"], dims, R.dims_of(p["wbonds"]), dtype=R.DTYPES[c.dtype])]
    if c.kind == "sweep":
        return [qil.readout_route("sweep", p["nb"], dims, R.dims_of(R.SWEEP_OPS[op.split("#")[0]][1]), dtype=R.DTYPES[R.sweep_dtype(c, op)])
                for op in p["ops"]]
    return []


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_case_reaches_its_route(qil, c):
    got = routes_of(qil, c)
    if c.kind in ("chain", "lazy"):
        assert got[0][0] == c.route
        if c.route != "LAZY_GEMM":
            assert got[0][1] == c.p["nb"]
    elif c.kind == "sweep":
        want = ["GEMM_SORTED" if op.startswith("wide") else "CHAIN" for op in c.p["ops"]]        # product bond 128 / 64, 64 queries
        assert [r for r, _ in got] == want
        # the sweep's route is the plain route of the product chain
        for op, (r, _) in zip(c.p["ops"], got):
            prod = [a * w for a, w in zip(R.dims_of(c.p["bonds"]), R.dims_of(R.SWEEP_OPS[op.split("#")[0]][1]))]
            assert qil.readout_route("plain", c.p["nb"], prod)[0] == r == qil.readout_route("sweep", c.p["nb"], prod)[0]
    else:
        assert c.route is None and not got


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_oracle_passes_every_bound(c):
    got = R.oracle_result(c)
    for key, g, ref in _pairs(c, got):
        R.check(g, ref, (c.name, key))
        if c.family == "random":
            assert R.rel(g, ref.value) < 1e-12, (c.name, key)
        else:
            assert (ref.bound <= R.CONE_RATIO * np.abs(ref.value)).all(), (c.name, key, float((ref.bound / np.abs(ref.value)).max()))
        if not np.iscomplexobj(ref.value):
            assert not np.iscomplexobj(g)
    if c.kind == "chain" and c.p["pattern"] == "equal":
        assert len(set(np.asarray(got).tolist())) == 1


def test_bound_catches_what_the_batch_relative_error_misses():
    """The gap this table closes: the smallest coefficient of a 300-query cone batch is 2e-9 (f64) / 6e-7 (c64) of the largest.
    With a relative error a tenth of what `rel < 1e-12` lets through there -- wrong from its fifth (seventh) digit on -- it passes
    `rel` and fails its own bound by eight (six) decades."""
    for dt in R.DTYPES:
        c = R.BY_NAME[f"chain15_nb300-{dt}-cone"]
        ref, good = R.reference(c), R.oracle_result(c)
        q = int(np.argmin(np.abs(ref.value)))
        eps = 0.1 * 1e-12 * float(np.abs(ref.value).max() / abs(ref.value[q]))
        assert eps > 1e-7 and eps > 1e5 * R.CONE_RATIO
        wrong = good.copy()
        wrong[q] *= 1 + eps
        assert R.rel(wrong, ref.value) < 1e-12
        with pytest.raises(AssertionError, match="outside their bound"):
            R.check(wrong, ref, c.name)


def test_project_oracle_agrees(qil):
    """The oracle package's own coefficient_batch / lazy_coefficient_batch (other contraction orders) pass the same bounds."""
    seen = 0
    for c in R.CASES:
        if c.kind == "chain" and c.verb == "plain" and c.p["nb"] <= 300:
            data, bits = R.operands(c)
            R.check(O.coefficient_batch(O.SignalMPS(data, amplitude=R.AMPLITUDE), bits), R.reference(c), c.name)
            seen += 1
        if c.kind == "lazy" and c.p["nb"] <= 200:
            w, a, bits = R.operands(c)
            R.check(O.lazy_coefficient_batch(O.SingleSiteMPO(w), O.SignalMPS(a, amplitude=R.AMPLITUDE), bits), R.reference(c), c.name)
            seen += 1
    assert seen >= 60


def test_table_reaches_every_route(qil):
    reached = {(dt, r) for c in R.CASES for dt in [c.dtype] for r, _ in routes_of(qil, c)}
    for dt in R.DTYPES:
        for r in ("CHAIN", "GEMM_SELECT", "GEMM_SORTED", "LAZY_CHAIN", "LAZY_GEMM"):
            assert (dt, r) in reached, (dt, r)
    # the front-ends' per-query paths: coefficient_grid's largest permuted grid takes the sorted form, the small ones the chain
    dims = R.dims_of(R.GRID_BONDS)
    sizes = {len(ks) * len(ls) for _, ks, ls in R.grid_axes() if not _fast_grid(qil, ks, ls)}
    assert {qil.readout_route("plain", s, dims)[0] for s in sizes} == {"CHAIN", "GEMM_SORTED"}
    assert {qil.readout_route("marginal", len(ks), dims)[0] for _, ks in R.laplace_axes()} == {"CHAIN"}


def test_both_sides_of_every_threshold(qil):
    """The neighbours of each crossover land on different routes, through both verbs, in the table and in the hook."""
    route = lambda name: R.BY_NAME[f"{name}-f64-cone"].route
    for verb, gemm in (("plain", "GEMM_SORTED"), ("marginal", "GEMM_SELECT")):
        assert route(f"threshold_nb3_bond128_{verb}") == "CHAIN" and route(f"threshold_nb4_bond128_{verb}") == gemm
        assert route(f"threshold_nb4_bond127_{verb}") == "CHAIN"
        assert route(f"threshold_nb1023_bond16_{verb}") == "CHAIN" and route(f"threshold_nb1024_bond16_{verb}") == gemm
        assert route(f"threshold_nb1024_bond15_{verb}") == "CHAIN"
    lazy = lambda name: R.BY_NAME[f"{name}-Wf64-psif64-cone"].route
    assert lazy("lazy_32x32_nb15") == "LAZY_CHAIN" and lazy("lazy_32x32_nb16") == "LAZY_GEMM"
    assert lazy("lazy_31x33_nb200") == "LAZY_CHAIN" and lazy("lazy_ragged_nb15") == "LAZY_CHAIN" and lazy("lazy_ragged_nb200") == "LAZY_GEMM"
    # the widest bond decides, wherever it sits, and the edge bonds of 1 never do
    for dims in ([1, 128, 2, 1], [1, 2, 128, 1], [1, 2, 4, 128, 4, 2, 1]):
        assert qil.readout_route("plain", 4, dims)[0] == "GEMM_SORTED" and qil.readout_route("plain", 3, dims)[0] == "CHAIN"
    # the lazy product threshold reads chi_l D_r as well as chi_r D_r
    assert qil.readout_route("lazy", 16, [1, 32, 1], [1, 4, 32])[0] == "LAZY_GEMM"
    assert qil.readout_route("lazy", 16, [1, 32, 1], [1, 4, 31])[0] == "LAZY_CHAIN"
    # sweep lists on both sides of nw = 4, one with a repeated handle
    sizes = {name: len(ops) for name, ops in R.SWEEP_LISTS.items()}
    assert sizes == {"nw1": 1, "nw3": 3, "nw4": 4, "nw9": 9, "repeated": 5}
    assert len(set(R.SWEEP_LISTS["repeated"])) < 5 and all(len(set(R.SWEEP_LISTS[k])) == sizes[k] for k in ("nw3", "nw4", "nw9"))
    for ops in R.SWEEP_LISTS.values():
        if len(ops) > 1:
            assert {R.SWEEP_OPS[o.split("#")[0]][0] for o in ops} == {"f64", "c64"}            # real and complex in one list


def test_lazy_gemm_passes(qil):
    """The queries per pass the hook reports: the multi-pass case takes two passes over eight distinct configurations, and for an
    n = 30, chi 128, D 128 shape a pass stays within the 8 GiB scratch budget."""
    c = next(c for c in R.LAZY_CASES if c.p["nb"] == R.MULTIPASS_NB)
    (route, per_pass), = routes_of(qil, c)
    assert route == "LAZY_GEMM" and per_pass == 32768 < c.p["nb"] <= 2 * per_pass
    _, _, bits = R.operands(c)
    assert len(np.unique(bits, axis=0)) == 8
    per_query = lambda chi, D, e: (2 * chi * D + 2 * chi * D) * e        # M twice and X = chi_l 2 D_r, bytes per query
    assert per_pass * per_query(32, 32, 16) == 2 << 30                   # the case's pool: 2 GiB
    dims = [1] + [128] * 29 + [1]
    for dt, e in ((np.float64, 8), (np.complex128, 16)):
        route, per_pass = qil.readout_route("lazy", 1 << 20, dims, dims, dtype=dt)
        assert route == "LAZY_GEMM" and 1 <= per_pass <= 32768
        assert per_pass * per_query(128, 128, e) <= 8 << 30 < (per_pass + 1) * per_query(128, 128, e) or per_pass == 32768
    assert qil.readout_route("lazy", 1 << 20, dims, dims, dtype=np.complex128)[1] == 8192


def _fast_grid(qil, ks, ls):
    import importlib
    ops = importlib.import_module("qilaplace_jl_amd.ops")
    return ops._bit_block_range(ks) is not None and ops._bit_block_range(ls) is not None


def test_front_end_tables_cover_their_paths(qil):
    import importlib
    ops = importlib.import_module("qilaplace_jl_amd.ops")
    specs = R.block_specs()
    labels = [l for l, _ in specs]
    assert len(set(labels)) == len(labels) and sum(l.startswith("random_") for l in labels) == 12
    assert sum(l.startswith("one_free_at_") for l in labels) == len(R.BLOCK_BONDS) + 1
    for site in (3, 4, 5):                                 # the wide sites: fixed, summed, free, and behind the last free site
        states = {("fold" if site > max(np.flatnonzero(s == 3), default=-1) else "left", int(s[site])) for _, s in specs}
        assert {st for side, st in states if side == "left"} == {0, 1, 2, 3}, site
        assert {st for side, st in states if side == "fold"} >= {2} and {st for side, st in states if side == "fold"} & {0, 1}, site
    axes = R.grid_axes()
    fast = [(l, ks, ls) for l, ks, ls in axes if _fast_grid(qil, ks, ls)]
    assert {(len(ks), len(ls)) for _, ks, ls in fast} == {(2 ** a, 2 ** b) for a in range(6) for b in range(6)}
    assert len(fast) == sum(1 for l, _, _ in axes if l.startswith("a")) and len(axes) - len(fast) >= 5
    lap = R.laplace_axes()
    assert [ops._full_low_range(ks) for _, ks in lap] == [0, 1, 2, 3, 4, 5, None, None]


def test_all_two_row_is_the_dense_sum():
    """GEMM_SELECT cases: row 1 of the m_wide pattern sums every site; the recurrence's reference is the sum of the dense tensor."""
    seen = 0
    for c in R.CHAIN_CASES:
        if c.p["pattern"] == "m_wide":
            _, bits = R.operands(c)
            assert (bits[1] == 2).all() and (bits[0] < 2).all() and (bits[2] == 2).any() and (bits[2] < 2).any()
            ref = R.reference(c)
            value, mag = R.all_two_row_reference(c)
            assert abs(ref.value[1] - value) <= ref.bound[1] * 1e-3
            assert abs(ref.bound[1] - R.bound(mag / R.AMPLITUDE, R.chain_qs(R.dims_of(c.p["bonds"])))) <= 1e-3 * ref.bound[1]
            seen += 1
    assert seen == 12


def test_route_rejects_bad_arguments(qil):
    for args, msg in ((("lazy", 4, [1, 2, 1]), "the lazy verb needs the operator"),
                      (("plain", 4, [1, 2, 1], [1, 2, 1]), "only the sweep and the lazy verb take an operator"),
                      (("plain", -1, [1, 2, 1]), "nb >= 0"),
                      (("plain", 4, [1, 0, 1]), "bond dimension 1 is not positive")):
        with pytest.raises(ValueError, match=msg):
            qil.readout_route(*args)
    with pytest.raises(ValueError, match="n \\+ 1 entries"):
        qil.readout_route("lazy", 4, [1, 2, 1], [1, 2, 2, 1])
