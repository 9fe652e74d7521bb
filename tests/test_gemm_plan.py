"""Which GEMM kernel does a call reach?  CPU test of the dispatch decision (qil_gemm_plan: the one host function
gemm_dispatch / gemm_launch switch on), over the case table of tests/gemm_cases.py that tests/test_gpu_gemm.py then RUNS.

Two things are asserted: every case reaches the plan written beside it (so a re-tuned heuristic that silently moves a case to
another kernel fails here, and the table is re-aimed), and the table as a whole reaches every member of the family -- tile shape x
staging pattern, split and unsplit, each split-K rule, slice rounding, short last slices, the XCD permutation and the tile order
both ways, the K-tile counts of the two-tiles-in-flight pipeline.  Needs the library, not a GPU.

What no argument reaches (read off the rules, asserted below so that a re-tune which opens one of these fails here too):
  * 128 x 128 never splits K: it is chosen from 512 tiles on, and no rule splits above 384 tiles;
  * 128 x 64 only splits by rule 3 (it starts at 128 tiles), 64 x 144 never by rule 2 (m >= 256 and more than 64 tiles of 64 x 64
    mean at least 22 row panels, rule 2 stops at four tiles);
  * 64 x 144 has one tile column, so its tile order is always "along a tile row first"."""
import itertools

import pytest

import gemm_cases as G

RULES_OF = {"128x128": (0,), "128x64": (0, 3), "64x144": (0, 1, 3)}      # every other shape: (0, 1, 2, 3)


@pytest.fixture(scope="module")
def qil():
    import qilaplace_jl_amd as q
    return q


def _plan(qil, c):
    p = qil.gemm_plan(**G.plan_args(c))
    tile = [t for t, v in G.TILES.items() if v == (p["bm"], p["bn"], p["gkt"], p["deep"])]
    assert len(tile) == 1, p
    return G.Plan(tile[0], p["arc"], p["bkc"], p["splits"], p["kchunk"], p["split_rule"], p["col_fastest"], p["xcd"]), p


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_case_reaches_its_plan(qil, c):
    got, raw = _plan(qil, c)
    assert got == c.plan
    assert c.plan.tile in G.TILES_OF[c.dtype]
    # what the plan says about itself
    bm, bn, gkt, _ = G.TILES[got.tile]
    assert raw["tiles_m"] == -(-c.m // bm) and raw["tiles_n"] == -(-c.n // bn)
    assert (got.rule == 0) == (got.splits == 1)
    if got.splits > 1:
        assert raw["can_split"] and got.kchunk % gkt == 0 and (got.splits - 1) * got.kchunk < c.k <= got.splits * got.kchunk
    else:
        assert got.kchunk == c.k


def test_non_packed_batches_do_not_split(qil):
    """Split-K of a batch reduces the workspace as one m x (n * count) matrix: only packed outputs may take it."""
    seen = 0
    for c in G.CASES:
        L = G.layout(c)
        packed = L.ldc == c.m and L.c_bs == c.m * c.n and not c.batch.cmap
        if c.batch.count > 1 and not packed:
            assert c.plan.splits == 1 and not _plan(qil, c)[1]["can_split"], c.name
            seen += c.k >= 512       # ... although K alone would have split it
    assert seen >= 4


def _tiles(c):
    bm, bn, _, _ = G.TILES[c.plan.tile]
    return -(-c.m // bm) * -(-c.n // bn)


def test_table_covers_the_family():
    by = lambda f: {f(c) for c in G.CASES}
    missing = []
    # every tile shape that exists for a dtype, with all four staging patterns
    have = by(lambda c: (c.dtype, c.plan.tile, c.plan.arc, c.plan.bkc))
    for dt, tiles in G.TILES_OF.items():
        missing += [x for x in itertools.product([dt], tiles, (0, 1), (0, 1)) if x not in have]
    # split and unsplit on every shape that can split
    have = by(lambda c: (c.dtype, c.plan.tile, c.plan.splits > 1))
    for dt, tiles in G.TILES_OF.items():
        missing += [x for x in itertools.product([dt], tiles, (False, True)) if x not in have and x[1:] != ("128x128", True)]
    # each split-K rule as the one that decided, on every shape it can reach -- and on no other
    have = by(lambda c: (c.plan.tile, c.plan.rule))
    for t in G.TILES:
        rules = RULES_OF.get(t, (0, 1, 2, 3))
        missing += [(t, "rule", r) for r in rules if (t, r) not in have]
        assert not [r for r in (0, 1, 2, 3) if r not in rules and (t, r) in have], t
    # the XCD permutation on, and off although there are 64 tiles or more, for every shape; off under 64 tiles
    have = by(lambda c: (c.plan.tile, c.plan.xcd, _tiles(c) >= 64))
    for t in G.TILES:
        missing += [(t, "xcd", x) for x in (0, 1) if (t, x, True) not in have]
        assert (t, 1, False) not in have
        if (t, 0, False) not in have:
            missing.append((t, "under 64 tiles"))
    # the tile order both ways
    have = by(lambda c: (c.plan.tile, c.plan.col_fastest))
    missing += [(t, "col_fastest", v) for t in G.TILES for v in (0, 1) if (t, v) not in have and (t, v) != ("64x144", 0)]
    assert ("64x144", 0) not in have
    # two K tiles in flight: 1, 2, 3, 4 K tiles per slice and a large odd count
    for dt in G.TILES_OF:
        for t in ("32x64D", "48x64D"):
            counts = {-(-min(c.k, c.plan.kchunk) // 16) for c in G.CASES if (c.dtype, c.plan.tile) == (dt, t)}
            missing += [(dt, t, "K tiles", x) for x in (1, 2, 3, 4) if x not in counts]
            if not any(x % 2 and x > 50 for x in counts):
                missing.append((dt, t, "large odd K-tile count"))
    assert not missing, missing


def test_table_covers_short_last_slices():
    """Split cases whose last slice is shorter than kchunk and not a multiple of the K step: the zeroed K tail inside a slice."""
    ragged = set()
    for c in G.CASES:
        gkt = G.TILES[c.plan.tile][2]
        last = c.k - (c.plan.splits - 1) * c.plan.kchunk
        if c.plan.splits > 1 and last < c.plan.kchunk and last % gkt:
            ragged.add((c.plan.tile, c.plan.rule))
    assert {t for t, _ in ragged} == set(G.TILES) - {"128x128"} and {r for _, r in ragged} == {1, 2, 3}, ragged


def test_rounding_drops_a_slice_as_named():
    """64 x 64 x 257 on the 32 x 32 tile: rule 2 asks for min(257 / 64, 32) = 4 slices of ceil(257 / 4) = 65, the 32-deep K step
    rounds the slice to 96, and 257 / 96 leaves 3 slices, the last one 65 long."""
    for name in ("f64_NN_64x64x257_rule2_rounding_drops_a_slice", "c64_HN_64x64x257_rule2_rounding_drops_a_slice"):
        c = G.BY_NAME[name]
        assert (c.plan.tile, c.plan.rule, c.plan.splits, c.plan.kchunk) == ("32x32", 2, 3, 96)
        assert min(c.k // 64, 32) == 4 and c.k - 2 * 96 == 65


def test_boundaries_of_the_shape_rules():
    """The neighbours of each threshold land on different kernels."""
    t = lambda name: G.BY_NAME[name].plan.tile
    assert t("f64_NN_1400x144x129_shape") == "64x144" and t("f64_NN_1400x145x129_shape") != "64x144"
    assert t("f64_NN_1400x96x129_shape") != "64x144" and t("f64_NN_255x133x129_shape") != "64x144"
    for dt in ("f64", "c64"):
        assert t(f"{dt}_NN_32x200x100_skinny") == "32x64D" and t(f"{dt}_NN_33x200x100_skinny") == "48x64D"
        assert t(f"{dt}_NN_48x200x100_skinny") == "48x64D"
        assert t(f"{dt}_NN_49x200x100_hint_not_honoured") not in ("32x64D", "48x64D")
        assert t(f"{dt}_NN_32x127x100_hint_not_honoured") not in ("32x64D", "48x64D")
        assert t(f"{dt}_NN_32x200x100_no_hint") not in ("32x64D", "48x64D")


def test_plan_rejects_bad_arguments(qil):
    for kw, msg in ((dict(lda=69), "lda 69 is smaller than the 70 stored rows of A"),
                    (dict(ldb=36), "ldb 36 is smaller than the 37 stored rows of B"),
                    (dict(ldc=69), "ldc 69 is smaller than the 70 rows of C"),
                    (dict(opA="T", lda=36), "lda 36 is smaller than the 37 stored rows of A"),
                    (dict(opB="H", ldb=44), "ldb 44 is smaller than the 45 stored rows of B"),
                    (dict(count=65536), "batch count 65536 exceeds the grid limit")):
        with pytest.raises(ValueError, match=msg):
            qil.gemm_plan("float64", 70, 45, 37, **kw)
    with pytest.raises(ValueError, match="empty operand"):
        qil.gemm_plan("float64", 70, 45, 0)
