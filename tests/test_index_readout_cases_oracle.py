"""The case table of the read-out by index (tests/index_readout_cases.py) against itself, without a GPU: a plain float64 numpy
evaluation passes every per-coefficient bound, the cone cases keep their bound a small multiple of each coefficient's own
modulus, every case names the route the library's decision gives it, and the table holds the cases it promises."""
import numpy as np
import pytest

import index_readout_cases as X

IDS = [c.name for c in X.CASES]


@pytest.mark.parametrize("c", X.CASES, ids=IDS)
def test_float64_numpy_passes_every_bound(c):
    ref = X.reference(c)
    worst = X.check(X.oracle_result(c), ref, c.name)
    print(f"{c.name}: {int(X.valid(c).sum())} of {len(c.p['idx'])} rows, route {c.route}, worst err / bound {worst:.3g}")
    assert worst <= 1.0
    if c.family == "cone":
        assert (np.asarray(ref.bound) <= X.CONE_RATIO * np.abs(np.asarray(ref.value))).all()


@pytest.mark.parametrize("c", X.CASES, ids=IDS)
def test_every_case_names_its_route(c):
    import qilaplace_jl_amd as qil
    dims = X.dims_of(c.p["bonds"])
    assert c.route in ("wave", "bits")
    assert qil.coefficient_at_route(dims) == c.route == X.route_of(dims)
    for forced in ("wave", "bits"):
        assert qil.coefficient_at_route(dims, forced) == X.route_of(dims, forced)
    assert X.route_of(dims, "bits") == "bits"


def test_the_cap_is_the_headers_and_both_sides_of_it_are_cases():
    import importlib
    L = importlib.import_module("qilaplace_jl_amd._lib")
    assert X.CAP == L.QIL_COEFFICIENT_AT_WAVE_MAX_BOND and X.CAP < X.WAVE_FIT
    tops = {max(c.p["bonds"]): c.route for c in X.CASES if c.name.startswith("threshold")}
    assert tops == {X.CAP: "wave", X.CAP + 1: "bits"}


def test_the_table_holds_what_it_promises():
    by = {c.name.rsplit("-", 2)[0]: c for c in X.CASES if c.dtype == "f64" and c.family == "random"}
    assert len(X.CASES) == 4 * len(by)
    n = len(X.CHAIN15) + 1
    assert n == 16 and max(X.CHAIN15) > 64 and 1 in X.CHAIN15
    for count in (1, 3, 300):
        assert len(by[f"chain15_count{count}"].p["idx"]) == count
    idx = by["chain15_count300"].p["idx"]
    assert idx[0] == 0 and idx[1] == 2 ** n - 1 and idx[2] == idx[-1]
    assert list(by["one_site"].p["idx"]) == [0, 1] and list(by["two_sites"].p["idx"]) == [0, 1, 2, 3]
    long = by["long62"]
    assert X.ntensors(long) == 62 and len(long.p["idx"]) == 45
    assert list(long.p["idx"][:5]) == [0, 2 ** 61, 2 ** 62 - 1, 2 ** 32 - 1, 2 ** 32] and long.p["idx"].max() >= 2 ** 32
    assert [by[f"threshold_bond{t}_count{k}"] for t in (X.CAP, X.CAP + 1) for k in (5, 300)]
    bad = by["out_of_range"]
    assert len(bad.p["idx"]) == 50 and int((~X.valid(bad)).sum()) == 3
    assert {int(v) for v in bad.p["idx"][~X.valid(bad)]} == {-1, 2 ** n, X.INT64_MIN}
    assert all(X.valid(c).all() for c in X.CASES if not c.name.startswith("out_of_range"))


def test_bits_are_taken_most_significant_first_in_64_bits():
    b = X.bits_of(np.array([2 ** 61, 2 ** 32, 1], dtype=np.int64), 62)
    assert b[0].tolist() == [1] + [0] * 61 and b[1, 61 - 32] == 1 and b[1].sum() == 1 and b[2].tolist() == [0] * 61 + [1]


@pytest.mark.parametrize("dt", sorted(X.DTYPES))
@pytest.mark.parametrize("fam", X.FAMILIES)
def test_paired_indices_follow_the_grid_interleaving(dt, fam):
    """The chain reference at the case's indices IS coefficient_grid's (k, l) table read off the dense tensor."""
    c = X.BY_NAME[f"paired_grid-{dt}-{fam}"]
    ref, grid = X.reference(c), X.grid_reference(c)
    assert np.asarray(grid.value).shape == (7, 6)
    err = np.abs(np.asarray(ref.value) - np.asarray(grid.value).reshape(-1))
    assert (err <= np.asarray(ref.bound) + np.asarray(grid.bound).reshape(-1)).all()
