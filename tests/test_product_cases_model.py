"""The case table of tests/product_cases.py, checked without a GPU: a plain float64 numpy evaluation passes every per-value
bound, every case reaches the route written beside it (the marginal read-out's decision, from qil_readout_route, and the LDS
cap), and the cone cases are conditioned as the table claims."""
import os
import re

import numpy as np
import pytest

import product_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in P.CASES]


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_float64_numpy_passes_every_bound(c):
    ref = P.reference(c)
    got = P.oracle_result(c)
    assert got.shape == (c.nb,)
    worst = P.check(got, ref, c.name)
    print(f"{c.name}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


def test_the_table_holds_the_shapes_it_promises():
    by_shape = {c.name.split("-")[0]: c for c in P.CASES}
    assert P.dims(by_shape["one_tensor"]) == [1, 1] and by_shape["one_tensor"].nb == 1
    assert P.dims(by_shape["two_tensors"]) == [1, 2, 1] and by_shape["two_tensors"].nb == 3
    assert P.dims(by_shape["odd_small"]) == [1, 3, 5, 3, 1] and by_shape["odd_small"].nb == 7
    assert P.dims(by_shape["wide_left"]) == [1, 33, 65, 2, 1] and by_shape["wide_left"].nb == 5
    assert by_shape["paired6"].paired and len(P.dims(by_shape["paired6"])) == 7
    assert P.dims(by_shape["gemm_wide"]) == [1, 130, 7, 1] and by_shape["gemm_wide"].nb == 5
    assert P.dims(by_shape["gemm_many"]) == [1, 17, 17, 17, 17, 1] and by_shape["gemm_many"].nb == 1027
    assert P.dims(by_shape["gemm_many48"]) == [1, 48, 48, 48, 48, 1] and by_shape["gemm_many48"].nb == 1027
    assert P.dims(by_shape["gemm_skinny"]) == [1, 2, 128, 2, 1] and by_shape["gemm_skinny"].nb == 4
    assert P.dims(by_shape["above_cap"]) == [1, P.CHAIN_CAP + 1, 1] and by_shape["above_cap"].nb == 4
    # every shape in f64 and c64, with real and complex weights, in both families
    assert len(P.CASES) == len(P.SHAPES) * 2 * 2 * 2
    for c in P.CASES:
        data, w = P.operands(c)
        assert data[0].dtype == P.DTYPES[c.dtype] and np.iscomplexobj(w) == (c.wkind == "complex")
        assert w.shape == (c.nb, len(data), 2)


def test_the_cap_of_the_table_is_the_library_s():
    import qilaplace_jl_amd.ops as ops
    header = open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()
    m = re.search(r"#define QIL_PRODUCT_CHAIN_MAX_BOND (\d+)", header)
    assert m and int(m.group(1)) == P.CHAIN_CAP == ops.PRODUCT_CHAIN_MAX_BOND
    src = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_product.hip")).read()
    assert "kChainMaxBond = QIL_PRODUCT_CHAIN_MAX_BOND" in src and "wb <= kChainMaxBond" in src
    # ... and the verb's own many-rows constant
    m = re.search(r"constexpr long long kManyRowsChainWork = 1LL << (\d+);", src)
    assert m and 1 << int(m.group(1)) == P.MANY_ROWS_CHAIN_WORK == ops.PRODUCT_MANY_ROWS_CHAIN_WORK
    assert "route == QIL_ROUTE_CHAIN || (wb < 128 && nb * wb * wb < kManyRowsChainWork)" in src
    # the carry of the widest allowed bond fits what a kernel may ask for without an attribute call
    assert 2 * P.CHAIN_CAP * 16 <= 64 * 1024


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_every_case_reaches_its_route(c):
    import qilaplace_jl_amd as qil
    marginal, _ = qil.readout_route("marginal", c.nb, P.dims(c), dtype=P.DTYPES[c.dtype])
    assert marginal in ("CHAIN", "GEMM_SELECT")
    if c.name.startswith("gemm_many"):                     # the marginal's many-rows arm: both sides of this verb's constant
        assert marginal == "GEMM_SELECT" and c.route == ("chain" if c.nb * max(P.dims(c)) ** 2 < P.MANY_ROWS_CHAIN_WORK else "gemm")
    assert P.route_of(c, marginal) == c.route
    # forced the other way: the chain cases run as GEMMs, the GEMM cases as chains where the cap allows
    other = "gemm" if c.route == "chain" else "chain"
    fits = max(P.dims(c)) <= P.CHAIN_CAP
    assert P.route_of(c, marginal, forced=other) == (other if other == "gemm" or fits else "gemm")
    assert fits == (not c.name.startswith("above_cap"))


@pytest.mark.parametrize("c", [c for c in P.CASES if c.family == "cone"], ids=[n for n in IDS if n.endswith("cone")])
def test_cone_cases_are_conditioned_as_claimed(c):
    assert sum(P.product_qs(P.dims(c))) <= P.CONE_Q_SUM
    ref = P.reference(c)
    ratio = float((ref.bound / np.abs(ref.value).astype(P.LD)).max())
    print(f"{c.name}: bound / |value| <= {ratio:.3e}")
    assert ratio <= P.CONE_RATIO


def test_special_weights_reduce_to_the_other_read_outs():
    """e_bit is a coefficient, (1, 1) a summed site: the model agrees with readout_cases' chain on the same tensors."""
    import readout_cases as R
    c = P.BY_NAME["odd_small-c64-complex-random"]
    data, _ = P.operands(c)
    bits = R.make_bits("m_random", 11, P.dims(c), "product special")
    w = np.zeros((11, len(data), 2))
    for s in (0, 1):
        w[:, :, s] = (bits == s) | (bits == 2)
    a, b = P.product_values(data, w, P.exact), R.chain_values(data, bits, R.exact)
    assert np.abs(a - b).max() <= 1e-17 * np.abs(b).max()
