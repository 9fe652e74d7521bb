"""The route decisions of the three two-site verbs against recorded answers (needs no GPU): qil_mps_solve_local_fits,
qil_mps_eigs_local_fits and qil_mps_evolve_local_fits share one rule, one operand count and one byte formula (qil_twosite.h), and
each adds its own vectors and blocks.  tests/golden/twosite_fits.json holds what the library answered BEFORE they were merged
(tools/_record_twosite_fits.py), on the grids the three ABI tests build, for f64 and c64, one and two sites, and the route
variable unset, `local` and `gemm`; every answer must still be the same, point for point -- a term dropped from a byte formula
moves a point near the 160 KiB budget."""
import ctypes
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "twosite_fits.json")
GRID = (1, 2, 5, 16, 17, 40)
ROUTES = ("unset", "local", "gemm")
ENV = {"solve": "QIL_SOLVE_ROUTE", "eigs": "QIL_EIGS_ROUTE", "evolve": "QIL_EVOLVE_ROUTE"}


def grids():
    """verb -> the points of its ABI test (the same seeded draws and straddle lines)."""
    rng = np.random.default_rng(5)
    solve = [tuple(int(v) for v in rng.choice(GRID, size=8)) for _ in range(300)]
    solve += [(16, 16, d, d, d, 16, 16, 16) for d in range(1, 10)] + [(x, x, 2, 2, 2, x, x, x) for x in range(1, 40, 3)]
    rng = np.random.default_rng(5)
    eigs = [tuple(int(v) for v in rng.choice(GRID, size=5)) + (int(rng.integers(2, 17)), int(rng.integers(0, 9))) for _ in range(300)]
    eigs += [(16, 16, d, d, d, 8, 0) for d in range(1, 10)] + [(x, x, 2, 2, 2, 8, 2) for x in range(1, 40, 3)]
    eigs += [(12, 12, 3, 3, 3, k, o) for k in (2, 8, 16) for o in (0, 4, 8)]
    rng = np.random.default_rng(5)
    evolve = [tuple(int(v) for v in rng.choice(GRID, size=5)) + (int(rng.integers(2, 17)),) for _ in range(300)]
    evolve += [(16, 16, d, d, d, 8) for d in range(1, 10)] + [(x, x, 2, 2, 2, 8) for x in range(1, 48, 3)]
    evolve += [(12, 12, 3, 3, 3, k) for k in (2, 8, 16)] + [(x, x, 5, 5, 5, 8) for x in range(8, 40, 2)]
    return {"solve": solve, "eigs": eigs, "evolve": evolve}


def cases():
    """(key, verb, complex, sites, route) of every recorded grid; sites is None where the verb has no such argument."""
    for verb in ("solve", "eigs", "evolve"):
        for cx in (0, 1):
            for sites in ((1, 2) if verb == "evolve" else (None,)):
                for route in ROUTES:
                    key = f"{verb}/{'c64' if cx else 'f64'}" + (f"/sites{sites}" if sites else "") + f"/{route}"
                    yield key, verb, cx, sites, route


def answers(lib, verb, cx, sites, route, points):
    """The library's answers on `points` as one string of 0 / 1, with the verb's route variable set as `route` says."""
    old = os.environ.get(ENV[verb])
    if route == "unset":
        os.environ.pop(ENV[verb], None)
    else:
        os.environ[ENV[verb]] = route
    try:
        out, f = [], ctypes.c_int(-1)
        for p in points:
            if verb == "solve":
                s = lib.qil_mps_solve_local_fits(cx, *p, ctypes.byref(f))
            elif verb == "eigs":
                s = lib.qil_mps_eigs_local_fits(cx, *p, ctypes.byref(f))
            else:
                s = lib.qil_mps_evolve_local_fits(cx, sites, *p, ctypes.byref(f))
            assert s == 0 and f.value in (0, 1), (verb, p, s, f.value)
            out.append(str(f.value))
        return "".join(out)
    finally:
        if old is None:
            os.environ.pop(ENV[verb], None)
        else:
            os.environ[ENV[verb]] = old


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(FIXTURE))


def test_the_fixture_holds_every_grid_and_both_answers_of_every_function(recorded):
    pts = grids()
    keys = [c[0] for c in cases()]
    assert sorted(recorded["answers"]) == sorted(keys) and len(keys) == 24
    assert recorded["points"] == {v: len(p) for v, p in pts.items()}
    for key, verb, cx, sites, route in cases():
        got = recorded["answers"][key]
        assert len(got) == len(pts[verb]) and set(got) <= {"0", "1"}, key
        if route == "gemm":
            assert set(got) == {"0"}, key
    for verb in ("solve", "eigs", "evolve"):
        for route in ("unset", "local"):
            seen = set("".join(v for k, v in recorded["answers"].items() if k.startswith(verb + "/") and k.endswith("/" + route)))
            assert seen == {"0", "1"}, (verb, route)


@pytest.mark.parametrize("verb", ("solve", "eigs", "evolve"))
def test_every_decision_is_the_recorded_one(recorded, verb):
    import importlib
    lib = importlib.import_module("qilaplace_jl_amd._lib").lib
    pts = grids()[verb]
    for key, v, cx, sites, route in cases():
        if v != verb:
            continue
        got, want = answers(lib, verb, cx, sites, route, pts), recorded["answers"][key]
        diff = [(p, w, g) for p, w, g in zip(pts, want, got) if w != g]
        assert not diff, (key, len(diff), diff[:5])
