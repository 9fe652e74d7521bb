"""Which kernels does a thin QR reach?  CPU test of the decision (qil_qr_plan: the one host function qr_impl switches on), over
the case table of tests/qr_cases.py that tests/test_gpu_qr.py then RUNS.  Needs the library, not a GPU.

Asserted: every case reaches the plan written beside it; the plan agrees, field by field, with the plain restatement of the rules
in qr_cases.py (Householder fit, LDS budgets, KM variants, chunking) on a grid around every threshold; the table as a whole reaches
every member of the family (test_table_covers_the_family); CholeskyQR2's eligibility flips exactly at the stated edges; and the first-order pairs
lie a factor MARGIN from the kernel's threshold in a numpy model of the first pass.

What no argument reaches (read off the rules and asserted in test_unreachable_members, so that a re-tune which opens one fails
here too):
  * f64 never takes the one-launch CGS2 kernel out of LDS on the operand itself: 16 columns of f64 leave LDS at 1198 rows, where
    the tree starts.  (f64 does run gs_fused_k<double, false>: on the tree's stacked triangles from 37889 rows on, "top-glob".)
  * the one-launch CGS2 with more than 16 columns never meets the tree; CGS2 panels of the blocked driver never have m <= 256 (a
    Householder panel always fits there), so the 16-lane row form runs only in the single launch and inside the tree;
  * the one-launch CGS2 out of LDS has at most 16 columns, so its 16-accumulator sweep never runs a FULL chunk followed by a
    partial one: the last (only) chunk is always partial, with 15 previous columns at most (n = 16) -- the table runs n = 15 too;
  * 32-column panels are never tree or out-of-LDS CGS2 panels;
  * KM = 19 never runs on c64, and the m = 1216 / 1217 edge of the Householder panel is behind the tree (f64) or the fit limit
    (c64: 13 rows per lane at most, and those with 8 waves);
  * a refusal in CholeskyQR2's second pass (outcome 4): see qr_cases.py."""
import itertools

import numpy as np
import pytest

import qr_cases as Q

KM_EDGES = (128, 256, 384, 512, 576, 832)


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    return q


@pytest.mark.parametrize("c", Q.CASES, ids=[c.name for c in Q.CASES])
def test_case_reaches_its_plan(qil, c):
    p = qil.qr_plan(Q.np_dtype(c), c.m, c.n)
    assert Q.label(p) == c.plan
    assert p == Q.restate(c.dtype, c.m, c.n)
    # what the plan says about itself
    if p["has_tree"]:
        assert (p["tree_chunks"] - 1) * p["tree_chunk"] < c.m <= p["tree_chunks"] * p["tree_chunk"]
        assert p["tree_last_rows"] == c.m - (p["tree_chunks"] - 1) * p["tree_chunk"] and 1 <= p["tree_last_rows"] <= p["tree_chunk"]
    else:
        assert not any(p[k] for k in ("tree_chunk", "tree_chunks", "tree_last_rows", "tree_in_lds", "tree_top_in_lds"))
    assert (p["hh_km"] in Q.KM_VARIANTS and p["hh_waves"] in (8, 16)) if p["has_hh"] else (p["hh_km"] == p["hh_waves"] == 0)
    if p["route"] == "BLOCKED":
        assert p["panel_width"] in (16, 32) and c.n > p["panel_width"] and 1 <= p["last_panel_width"] <= p["panel_width"]
        assert (c.n - p["last_panel_width"]) % p["panel_width"] == 0
    else:
        assert p["panel_width"] == p["last_panel_width"] == c.n and p["panel_kind"] == p["last_panel_kind"]
    assert bool(c.chol) == bool(p["cholesky_eligible"]) and (not c.skip or c.chol == 5)


def test_plan_matches_the_restated_rules_around_every_threshold(qil):
    """Every m from n to 2100 (all thresholds of both dtypes lie below), a set of widths on both sides of every width rule, and
    the tall sizes at which the tree's levels leave LDS."""
    for dt, n in itertools.product(Q.DTYPES, (1, 2, 3, 15, 16, 17, 20, 31, 32, 33, 40, 48, 63, 64, 65, 130, 256, 257)):
        for m in range(n, 2101):
            assert qil.qr_plan(Q.DTYPES[dt], m, n) == Q.restate(dt, m, n), (dt, m, n)
    for dt, n in itertools.product(Q.DTYPES, (1, 16, 48)):
        for m0 in (Q.TOP_GLOBAL_M[dt], Q.CHUNKS_GLOBAL_M[dt], 1 << 16, 1 << 20):
            for m in range(m0 - 2, m0 + 3):
                assert qil.qr_plan(Q.DTYPES[dt], m, n) == Q.restate(dt, m, n), (dt, m, n)


def test_plan_rejects_bad_arguments(qil):
    for m, n in ((3, 4), (4, 0), (0, 0)):
        with pytest.raises(ValueError, match="needs m >= n >= 1"):
            qil.qr_plan(np.float64, m, n)


def _plans():
    return [(c, Q.restate(c.dtype, c.m, c.n)) for c in Q.RUN]


def test_table_covers_the_family():
    rows = _plans()
    missing = []
    need = lambda what, wanted, got: missing.extend((what, x) for x in wanted if x not in got)
    panel = lambda c, p: not c.chol or c.chol in (3, 5)                  # the panel routes ran (no CholeskyQR2, refused or skipped)
    for dt in Q.DTYPES:
        mine = [(c, p) for c, p in rows if c.dtype == dt and panel(c, p)]
        of = lambda route, f: {f(c, p) for c, p in mine if p["route"] == route}
        # --- single CGS2 in LDS: the shapes, the m <= 256 switch, the window beyond 16 columns
        lds = [(c, p) for c, p in mine if p["route"] == "SINGLE_CGS2" and p["fused_in_lds"]]
        need((dt, "cgs2-lds shape"), [(1, 1), (7, 1)], {(c.m, c.n) for c, _ in lds})
        need((dt, "cgs2-lds n"), [2, 15, 16], {c.n for c, _ in lds})
        need((dt, "cgs2-lds square"), [True], {c.m == c.n for c, _ in lds})
        need((dt, "cgs2-lds m"), [256, 257], {c.m for c, p in lds if c.n == 16})
        need((dt, "cgs2-lds short"), [(256, 1), (257, 0)], {(c.m, p["fused_short_rows"]) for c, p in lds})
        need((dt, "cgs2-lds beyond 16 columns"), [True], {c.n == 20 and not Q.hh_panel_fits(dt, c.m, c.n) for c, _ in lds})
        # --- single Householder panel
        need((dt, "hh n"), [17, 32], of("SINGLE_HH", lambda c, p: c.n))
        need((dt, "hh square"), [17, 32], of("SINGLE_HH", lambda c, p: c.n if c.m == c.n else None))
        fit = max(m for m in range(17, 1300) if Q.restate(dt, m, 17)["route"] == "SINGLE_HH")
        sides = [m for e in KM_EDGES for m in (e, e + 1) if m <= fit]
        need((dt, "hh KM edge"), sides + [fit], of("SINGLE_HH", lambda c, p: c.m))
        need((dt, "hh KM"), {Q.hh_km(m) for m in sides}, of("SINGLE_HH", lambda c, p: p["hh_km"]))
        # --- single tree panel
        need((dt, "tree m"), [2048, 2049, 2063, 640 if dt == "c64" else 1198, Q.TOP_GLOBAL_M[dt], Q.CHUNKS_GLOBAL_M[dt]],
             of("SINGLE_TREE", lambda c, p: c.m))
        need((dt, "tree n"), [1, 3, 16], of("SINGLE_TREE", lambda c, p: c.n))
        need((dt, "tree last chunk"), ["one row", "shorter than n", "full"],
             of("SINGLE_TREE", lambda c, p: "one row" if p["tree_last_rows"] == 1 and c.n > 1 else "shorter than n"
                if p["tree_last_rows"] < c.n else "full" if p["tree_last_rows"] == p["tree_chunk"] else None))
        need((dt, "tree levels in LDS (chunks, top)"), [(1, 1), (1, 0), (0, 0)],
             of("SINGLE_TREE", lambda c, p: (p["tree_in_lds"], p["tree_top_in_lds"])))
        # --- blocked
        blocked = of("BLOCKED", lambda c, p: (p["panel_width"], p["panel_kind"], p["last_panel_kind"]))
        want = [(32, "HH", "HH"), (32, "CGS2_LDS", "HH"), (32, "CGS2_LDS", "CGS2_LDS"), (16, "HH", "HH"), (16, "CGS2_LDS", "CGS2_LDS"),
                (16, "CGS2_LDS", "HH"), (16, "TREE", "TREE")]
        if dt == "c64":
            want += [(16, "CGS2_GLOBAL", "CGS2_GLOBAL"), (16, "CGS2_GLOBAL", "HH"), (16, "CGS2_GLOBAL", "CGS2_LDS")]
        need((dt, "blocked panels"), want, blocked)
        assert not blocked - set(want), blocked - set(want)
        for pw in (16, 32):
            need((dt, f"blocked{pw} last width"), [1, 15 if pw == 16 else 31, pw],
                 of("BLOCKED", lambda c, p: p["last_panel_width"] if p["panel_width"] == pw else None))
        need((dt, "blocked n, no Cholesky"), [33, 40, 48, 63], of("BLOCKED", lambda c, p: c.n if not c.chol else None))
        need((dt, "blocked n, Cholesky skipped"), [64, 65, 130], of("BLOCKED", lambda c, p: c.n if c.chol == 5 else None))
        need((dt, "blocked square"), [True], of("BLOCKED", lambda c, p: c.m == c.n))
        # --- CholeskyQR2
        chol = [(c, p) for c, p in rows if c.dtype == dt and c.chol]
        need((dt, "cholesky outcome"), [1, 2, 3, 5], {c.chol for c, _ in chol})
        done = [(c, p) for c, p in chol if c.chol in (1, 2)]
        need((dt, "cholesky n"), [64, 65, 127, 128, 129, 320], {c.n for c, _ in done})
        need((dt, "cholesky shape"), ["square", "tall"], {"square" if c.m == c.n else "tall" if c.m >= 2 * c.n else None for c, _ in done})
        # --- layout and operand kinds on every route
        route = lambda c, p: "cholesky" if c.chol in (1, 2) else "cgs2-glob" if p["route"] == "SINGLE_CGS2" and p["has_cgs2_global"] \
            else p["route"]
        routes = ["SINGLE_CGS2", "SINGLE_HH", "SINGLE_TREE", "BLOCKED", "cholesky"] + (["cgs2-glob"] if dt == "c64" else [])
        mine = [(c, p) for c, p in rows if c.dtype == dt]
        need((dt, "padded"), routes, {route(c, p) for c, p in mine if (c.lda_pad, c.off, c.ldr_pad) == Q.PAD and c.with_R})
        need((dt, "R absent"), routes, {route(c, p) for c, p in mine if not c.with_R})
        kinds = {(route(c, p), c.kind) for c, p in mine}
        need((dt, "kind"), [(r, k) for r in routes for k in ("well", "colscaled", "graded", "deficient")
                            if (r, k) != ("cholesky", "deficient")], kinds)
    # the one-launch CGS2 out of LDS: complex only, both ends of its window, a partial last accumulator chunk
    glob = [(c, p) for c, p in rows if p["route"] == "SINGLE_CGS2" and p["has_cgs2_global"]]
    need("cgs2-glob (m, n)", [(600, 16), (639, 16)], {(c.m, c.n) for c, _ in glob})
    need("cgs2-glob n", [15, 16], {c.n for c, _ in glob})            # 14 and 15 previous columns at most (docstring)
    assert not missing, missing
    assert all(c.reorth == 0 for c in Q.CASES)                     # the GPU test adds the reorth = 1 runs itself


def test_unreachable_members():
    widths = (1, 2, 15, 16, 17, 20, 32, 33, 40, 48, 63, 64, 65, 130, 320)
    for dt, n in itertools.product(Q.DTYPES, widths):
        for m in itertools.chain(range(n, 2101), (4096, 37888, 37889, 1 << 17, 524800)):
            p = Q.restate(dt, m, n)
            if dt == "f64":
                assert not p["has_cgs2_global"], (m, n)
            if p["route"] == "SINGLE_CGS2":
                assert not p["has_tree"] and (n <= 16 or (m < 2048 and Q.cgs2_lds_bytes(dt, m, 16) <= Q.LDS_BUDGET))
            if p["route"] == "BLOCKED":
                assert not p["fused_short_rows"]
                if p["panel_width"] == 32:
                    assert not p["has_tree"] and not p["has_cgs2_global"]
            if p["has_hh"]:
                assert m <= 1197 and (dt == "f64" or (p["hh_km"] <= 13 and (p["hh_km"] < 13 or p["hh_waves"] == 8)))
            if p["has_tree"]:
                assert p["route"] in ("SINGLE_TREE", "BLOCKED") and not (p["has_hh"] or p["has_cgs2_lds"] or p["has_cgs2_global"])


def test_tall_sizes_are_the_first_to_leave_lds():
    for dt in Q.DTYPES:
        m = Q.TOP_GLOBAL_M[dt]
        assert Q.restate(dt, m, 16)["tree_top_in_lds"] == 0 and Q.restate(dt, m - 1, 16)["tree_top_in_lds"] == 1
        m = Q.CHUNKS_GLOBAL_M[dt]
        assert Q.restate(dt, m, 16)["tree_in_lds"] == 0
        assert all(Q.restate(dt, k, 16)["tree_in_lds"] == 1 for k in range(2048, m, 509)) and Q.restate(dt, m - 1, 16)["tree_in_lds"] == 1
        assert m * 16 * Q.esize(dt) < 70e6                          # the one deliberately large operand: about 67 MB


def test_eligibility_flips_at_the_stated_edges(qil):
    """n = 63 | 64 and 1024 | 1025; m n at 2^22 for n > 256 (n = 1024 exactly, n = 257 at the last multiple below) and at 2^24 for
    n <= 256."""
    flips = set()
    for a, b in Q.ELIGIBILITY_EDGES:
        ea, eb = (qil.qr_plan(Q.np_dtype(c), c.m, c.n)["cholesky_eligible"] for c in (a, b))
        assert ea != eb, (a.name, b.name)
        if a.m == b.m:
            assert abs(a.n - b.n) == 1
            flips.add(("n", min(a.n, b.n)))
        else:
            assert a.n == b.n and abs(a.m - b.m) == 1
            e = a if ea else b
            assert e.m == min(a.m, b.m)
            flips.add(("m n", e.n, e.m * e.n))
    assert flips == {("n", 63), ("n", 1024), ("m n", 1024, 1 << 22), ("m n", 257, (1 << 22) // 257 * 257), ("m n", 256, 1 << 24)}


def test_first_order_pairs_keep_their_margin():
    """The numpy model of the first pass puts n max|E| a factor MARGIN below the kernel's threshold for the first-order case and
    above it for its partner, in both dtypes."""
    for lo, hi in Q.FIRST_ORDER_PAIRS:
        a, b = Q.BY_NAME[lo], Q.BY_NAME[hi]
        assert (a.m, a.n, a.chol, b.m, b.n, b.chol) == (512, 128, 1, 512, 128, 2)
        ea, eb = Q.first_pass_model(Q.operand(a)), Q.first_pass_model(Q.operand(b))
        print(f"{lo}: n max|E| = {ea:.3e}; {hi}: {eb:.3e}; threshold {Q.FIRST_ORDER_THRESHOLD:.1e}")
        assert ea * Q.MARGIN <= Q.FIRST_ORDER_THRESHOLD <= eb / Q.MARGIN


def test_operands_are_what_the_table_says():
    """Planted ranks, conditioning and reproducibility of the generators (small cases)."""
    for c in Q.RUN:
        if c.m * c.n > 1 << 17:
            continue
        A = Q.operand(c)
        assert A.shape == (c.m, c.n) and A.dtype == Q.np_dtype(c) and A.flags.f_contiguous
        assert np.array_equal(A, Q.operand(c))
        s = np.linalg.svd(A, compute_uv=False)
        if c.kind == "deficient":
            assert int((s > 1e-10 * s[0]).sum()) == c.rank and c.rank < c.n
        elif c.kind == "well":
            assert s[0] / s[-1] < 60
        elif c.kind == "graded":
            assert abs(np.log10(s[0] / s[-1]) - c.d) < 0.01
    assert all(Q.gram_cost(c) <= Q.LONGDOUBLE_CAP or Q.restate(c.dtype, c.m, c.n)["route"] == "SINGLE_TREE" for c in Q.RUN)
