"""The numpy model of the cross-interpolation encoder (tests/cross_model.py) against dense signals: the yardstick of the GPU
tests must itself meet the bound they use.

Bound: max |model - x| <= n tol max|x|.  It is a condition, not a measurement: each of the n - 1 bonds is allowed tol fmax by the
stop rule.  The inputs are chosen so that the model keeps at least 9 x room; an input that does not is the wrong input."""
import numpy as np
import pytest

import cross_model as M

N_SITES = 12
ROOM = 9.0


@pytest.mark.parametrize("tol", [1e-9, 1e-6])
@pytest.mark.parametrize("name", sorted(M.SIGNALS))
def test_model_meets_the_bound_with_room(name, tol):
    n = N_SITES
    sig = M.SIGNALS[name]
    x = sig(np.arange(2 ** n, dtype=np.float64), float(2 ** n))
    R = M.cross(M.sampler(sig, n), n, tol, 64, M.default_seeds(n))
    err = np.abs(M.dense(R["sites"]) - x).max()
    bound = n * tol * np.abs(x).max()
    print(f"{name} tol {tol:g}: max bond {max(R['ranks'])}, sweeps {R['sweeps']}, nevals {R['nevals']}, est {R['est']:.2e}, "
          f"err / bound {err / bound:.3g}")
    assert R["converged"] == 1 and R["est"] <= tol
    assert R["nevals"] < 8 * 2 ** n
    assert err <= bound / ROOM, (err, bound)


def test_model_is_exact_on_a_full_rank_signal():
    """Every bond saturates, no block is cut: the interpolation is the signal."""
    n = 10
    rng = np.random.default_rng(3)
    x = rng.standard_normal(2 ** n) + 1j * rng.standard_normal(2 ** n)
    R = M.cross(lambda idx: x[idx], n, 1e-9, 32, M.default_seeds(n))
    assert R["ranks"] == [min(2 ** l, 2 ** (n - l), 32) for l in range(1, n)]
    assert R["converged"] == 1 and R["est"] == 0.0
    assert np.abs(M.dense(R["sites"]) - x).max() <= 64 * 2.0 ** -52 * 2 ** (n / 2) * np.abs(x).max()


def test_model_rank_cap_reports_what_is_left():
    n = N_SITES
    x = M.chirp(np.arange(2 ** n, dtype=np.float64), float(2 ** n))
    R = M.cross(M.sampler(M.chirp, n), n, 1e-9, 8, M.default_seeds(n))
    err = np.abs(M.dense(R["sites"]) - x).max()
    assert max(R["ranks"]) == 8 and R["converged"] == 0 and R["sweeps"] == 8 and R["est"] > 1e-9
    assert 0.25 * R["est"] <= err <= 4 * R["est"]          # the estimate is of the size of the error (the issue: 1.06)


def test_model_pins_the_blind_spot():
    """x = delta(k - 1234) + 1e-3 cos(0.01 k): exact with the spike among the seeds, missed without -- and converged."""
    n = N_SITES
    x = M.spike(np.arange(2 ** n, dtype=np.float64), float(2 ** n))
    seeded = M.cross(M.sampler(M.spike, n), n, 1e-9, 64, [0, 1234])
    assert np.abs(M.dense(seeded["sites"]) - x).max() <= n * 1e-9 * np.abs(x).max()
    blind = M.cross(M.sampler(M.spike, n), n, 1e-9, 64, [0])
    y = M.dense(blind["sites"])
    assert blind["converged"] == 1 and abs(y[1234] - x[1234]) > 0.5
    assert np.abs(np.delete(y - x, 1234)).max() <= n * 1e-9


@pytest.mark.parametrize("n", [1, 2, 3])
def test_model_short_chains_are_exact(n):
    x = np.array([0.3, -1.5, 2.0, 0.25, 1.0, -0.75, 0.5, 4.0])[:2 ** n]
    R = M.cross(lambda idx: x[idx], n, 1e-12, 4, [0])
    assert np.abs(M.dense(R["sites"]) - x).max() <= 1e-14


def test_pivot_ties_go_to_the_lowest_column_major_position():
    P = np.array([[1.0, 2.0, -2.0], [2.0, 1.0, 0.5]])
    _, rows, cols, r, _ = M.lu_full(P, 0.0, 1)
    assert r == 1 and rows[0] == 1 and cols[0] == 0        # |2| at (1, 0) precedes (0, 1) and (0, 2) column by column
    # an all-zero block keeps one pivot, so that the chain stays connected
    _, rows, cols, r, err = M.lu_full(np.zeros((4, 2)), 0.0, 8)
    assert r == 1 and err == 0.0 and rows[0] == 0 and cols[0] == 0
