"""CPU: every assertion tests/test_gpu_mpo_ops.py makes of qil_apply_mpo_mpo and qil_mpo_compress, made of oracle.apply_mpo_mpo and
oracle.builders._compress on the same table (tests/mpo_cases.py).  It shows that the inputs keep the reference itself inside every
bound, that the truncating cases truncate, and that at most one lossless case in four falls back to the weaker bond check.  The
oracle's margins on these inputs are the "oracle" column of the MPO table in MEASUREMENTS.md."""
import numpy as np
import pytest

import oracle as O
from oracle.builders import _compress
from helpers import dense_mps
import mpo_cases as MC


def oracle_product(name):
    c = next(c for c in MC.COMPOSE if c.name == name)
    w1, w2 = MC.compose_operands(name)

    def mk(w, op):
        return O.PairedSiteMPO(w, op.sites[0::2], op.sites[1::2]) if c.paired else O.SingleSiteMPO(w, op.sites)

    A, B = mk(w1, c.first), mk(w2, c.second)
    r = O.apply_mpo_mpo(A, B)
    return (MC.Product(r.data, np.result_type(*[t.dtype for t in r.data]), isinstance(r, O.PairedSiteMPO), r.sites, r.bond_dims),
            A, B, r)


# ---------------------------------------------------------------- the table itself
def test_table_covers_what_it_is_for():
    names = [c.name for c in MC.COMPOSE]
    assert len(set(names)) == len(names)
    for paired in (False, True):
        pairs = {(c.first.dtype, c.second.dtype) for c in MC.COMPOSE if c.paired == paired and c.name.startswith("ragged")}
        assert len(pairs) == 4
    big = next(c for c in MC.COMPOSE if c.name == "grid-stride-D24")
    assert (big.first.bonds[0] * big.second.bonds[0]) ** 2 * 4 > 4096 * 256
    # a real base with a shorter complex operand (the widening copy), at the start, middle and end, in both orders
    widened = [c for c in MC.COMPOSE if c.name.startswith("embed") and not c.paired and c.name.endswith("base-f")]
    assert len(widened) == 6
    assert all(len(c.first.sites) <= 10 and len(c.second.sites) <= 10 for c in MC.COMPOSE)
    cn = [c.name for c in MC.COMPRESS]
    assert len(set(cn)) == len(cn)
    assert {len(c.bonds) + 1 for c in MC.COMPRESS} >= {2, 3, 6, 10} and max(len(c.bonds) + 1 for c in MC.COMPRESS) <= 10
    assert {(c.paired, c.dtype) for c in MC.COMPRESS} == {(p, d) for p in (False, True) for d in (MC.F, MC.Z)}
    for c in MC.COMPRESS:
        if "inflated" in c.name:                  # wider than tall at the end the gauge sweep starts from, both directions
            assert 4 * 1 < c.bonds[0] and 4 * 1 < c.bonds[-1]
            assert any(b > cap for b, cap in zip(c.bonds, MC.caps(len(c.bonds) + 1)))
        if c.kind == "product":
            fused = MC.bonds_of(MC.compress_input(c.name))
            assert any(b > cap for b, cap in zip(fused, MC.caps(len(fused) + 1)))
        assert c.maxdim < max(MC.bonds_of(MC.oracle_compress(c.name, "down", "lossless")))


def test_at_most_one_lossless_case_in_four_takes_the_weaker_bond_check():
    cases = [(c.name, d) for c in MC.COMPRESS for d in MC.DIRECTIONS]
    weak = [k for k in cases if not MC.has_gap(*k)]
    assert 4 * len(weak) <= len(cases), weak


# ---------------------------------------------------------------- composition
@pytest.mark.parametrize("name", [c.name for c in MC.COMPOSE])
def test_oracle_product_sites(name):
    got, _, _, _ = oracle_product(name)
    MC.check_product_sites(name, got)
    if len(got.data) <= 6:
        MC.check_product_dense(name, got)


@pytest.mark.parametrize("name", MC.COMPOSE_ON_STATE)
def test_oracle_product_on_a_state(name):
    _, A, B, AB = oracle_product(name)
    a = MC.compose_state(name)
    psi = O.ZTMPS(a, AB.sites_main, AB.sites_copy) if isinstance(AB, O.PairedSiteMPO) else O.SignalMPS(a, AB.sites)
    MC.check_product_on_state(name, dense_mps(O.apply(AB, psi).data), dense_mps(O.apply(B, O.apply(A, psi)).data))


# ---------------------------------------------------------------- compression
@pytest.mark.parametrize("direction", MC.DIRECTIONS)
@pytest.mark.parametrize("name", [c.name for c in MC.COMPRESS])
def test_oracle_compress(name, direction):
    for mode, _, _ in MC.MODES:
        data = MC.oracle_compress(name, direction, mode)
        MC.check_gauge(name, direction, data)
        if mode == "lossless":
            err = MC.check_lossless(name, direction, data)
            print(f"lossless {name} {direction}: oracle {err:.2e} (gap {MC.has_gap(name, direction)})")
        else:
            assert MC.truncation_removes_something(name, direction, mode), (name, direction, mode)
            MC.check_truncated(name, direction, mode, data)
            if direction == "down":
                MC.check_against_oracle_on_state(name, mode, data)


def test_oracle_edges():
    rng = np.random.default_rng(5)
    from helpers import random_mpo_data
    one = random_mpo_data([], rng)
    for direction in MC.DIRECTIONS:
        out = _compress(list(one), direction, 0.0, None)
        assert len(out) == 1 and np.array_equal(out[0], one[0])
    with pytest.raises(ValueError):
        _compress(random_mpo_data([2], rng), "sideways", 0.0, None)
    with pytest.raises(TypeError):
        O.apply_mpo_mpo(O.SingleSiteMPO(random_mpo_data([2], rng)), O.PairedSiteMPO(random_mpo_data([2], rng)))
