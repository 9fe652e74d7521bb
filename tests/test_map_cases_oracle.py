"""The case table of the element-wise maps (tests/map_cases.py) against the numpy model of the cross interpolation
(tests/cross_model.py), without a GPU: on g = op(dense operands), from the seeds map_states starts from, the model converges
within max_sweeps = 8 and stays within a ninth of n tol max|g| -- the yardstick of tests/test_gpu_map.py meets its own bound with
room, as in tests/test_cross_model.py.  A case for which the model alone does not is the wrong case."""
import numpy as np
import pytest

import cross_model as M
import map_cases as P


@pytest.mark.parametrize("tol", P.TOLS)
@pytest.mark.parametrize("c", P.CASES, ids=[c.name for c in P.CASES])
def test_model_meets_the_bound_with_room(c, tol):
    n = P.N_SITES
    xs = P.dense_operands(c)
    g = P.evaluate(c, *xs)
    assert np.iscomplexobj(g) == c.result_complex and np.isfinite(g).all()
    R = M.cross(lambda idx: g[idx], n, tol, P.MAXDIM, P.seeds(*xs), max_sweeps=P.MAX_SWEEPS)
    err, bound = np.abs(M.dense(R["sites"]) - g).max(), n * tol * np.abs(g).max()
    L = P.lipschitz(c, *xs)
    print(f"{c.name} tol {tol:g}: L_f {'Hoelder ' + str(c.param) if L is None else format(L, '.3g')}, max bond {max(R['ranks'])}, "
          f"sweeps {R['sweeps']}, nevals {R['nevals']}, est {R['est']:.2e}, err / bound {err / bound:.3g}")
    assert R["converged"] == 1 and R["est"] <= tol and R["sweeps"] <= P.MAX_SWEEPS
    assert err <= bound / P.ROOM, (err, bound)


def test_the_table_holds_the_issue_s_cases():
    assert [(c.op, c.operands) for c in P.CASES] == [("abs", ("chirp",)), ("power", ("gauss",)), ("log", ("gauss",)),
                                                     ("divide", ("three_modes", "b")), ("divide", ("chirp", "b")),
                                                     ("shrink", ("gauss",)), ("shrink", ("chirp",))]
    by = P.BY_NAME
    assert by["power_gauss"].param == 0.5 and by["log_gauss"].param == 1e-12
    assert by["divide_three_modes_b"].param == 0.0 and by["divide_chirp_b_reg"].param == 0.1
    for name in ("gauss", "chirp"):
        assert by[f"shrink_{name}"].param == 0.3 * np.abs(P.signal(name)).max()
    b = P.signal("b")
    assert 1.0 <= b.min() and b.max() <= 3.0
    assert P.N_SITES == 12 and P.MAXDIM == 64 and P.TOLS == (1e-9, 1e-6)


def test_lipschitz_constants_hold_on_the_operands():
    """Sampled finite differences never exceed L_f (or the Hoelder bound for power)."""
    rng = np.random.default_rng(5)
    for c in P.CASES:
        xs = P.dense_operands(c)
        for delta in (1e-3, 1e-8):
            moved = [x + delta * np.exp(2j * np.pi * rng.uniform(size=x.shape)) * (1 if np.iscomplexobj(x) else 0)
                     + (0 if np.iscomplexobj(x) else delta * rng.choice([-1.0, 1.0], size=x.shape)) for x in xs]
            diff = np.abs(P.evaluate(c, *moved) - P.evaluate(c, *xs)).max()
            room = P.perturbation(c, delta, *xs) * len(xs) * (1 + 1e-6) + 64 * 2.0 ** -53 * np.abs(P.evaluate(c, *xs)).max()
            assert diff <= room, (c.name, delta, diff, room)


def test_seeds_are_the_defaults_and_the_operands_peaks():
    x = P.signal("gauss")
    s = P.seeds(x)
    assert len(s) == 64 + P.SEED_PEAKS and np.array_equal(s[:64], M.default_seeds(P.N_SITES))
    assert set(s[64:]) == set(np.argsort(-np.abs(x))[:P.SEED_PEAKS])
