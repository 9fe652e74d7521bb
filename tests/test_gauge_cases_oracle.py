"""The gauge-sweep case table (tests/gauge_cases.py) without a GPU: conditions on the INPUTS of tests/test_gpu_gauge.py.

  * the construction holds: head sites are exact isometries, T has orthonormal rows, the mirror chain is the right chain read
    from the other end, and the chain's dense state is Head M (T last);
  * the kept rank is unambiguous: the truncation rule gives the same rank at 100 x and 1 / 100 of the cutoff;
  * the reference is stable: LAPACK's gesdd and gesvd give the truncated state within 1e-13 |M|_F of each other, 10 x inside
    what is asked of the device;
  * the reference passes its own test: the oracle's canonicalize! in the device's place passes assertions 1 to 5 of the GPU file
    (gauge_cases.check_result: the same function);
  * every case lies where its label assumes: the label is among the events that the code's rules -- restated in
    gauge_cases.predicted with file and line beside each -- imply for its operand, and every data-dependent threshold on the
    way is missed by a factor MARGIN at least;
  * the table reaches every label for each dtype, and both sides of every boundary width carry `flat` and `cut`;
  * the parser of the QIL_SVD_DEBUG lines reads the lines the library prints.
Needs the oracle, neither the library nor a GPU.  No case is skipped or sampled."""
import numpy as np
import pytest

import oracle as O
import gauge_cases as G

IDS = [c.name for c in G.CASES]


# ---------------------------------------------------------------- construction
@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_construction(c):
    head, (T, last) = G.head_and_tail(c)
    i = G.site_index(c)
    assert c.m == 2 ** (i + 1) and len(head) == i
    for j, h in enumerate(head):
        q = h.reshape(2 ** (j + 1), 2 ** (j + 1))
        assert np.array_equal(q.conj().T @ q, np.eye(2 ** (j + 1)))                  # exact
    t = T.reshape(c.k, -1)
    assert np.abs(t @ t.conj().T - np.eye(c.k)).max() < 1e-14
    assert abs(np.linalg.norm(last) - 1.0) < 1e-15
    M = G.operand(c.name)
    assert M.shape == (c.m, c.k) and M.dtype == G.DTYPES[c.dtype]
    assert np.array_equal(G.matrix_of(G.site_of(M, c.m, c.k)), M)
    right, left = G.chain(c, "right"), G.chain(c, "left")
    N = i + 3
    assert len(right) == len(left) == N and (not c.paired or N % 2 == 0)
    assert all(np.array_equal(a.transpose(2, 1, 0), b) for a, b in zip(right, reversed(left)))
    assert G.operand_position(c, "right")[0] == i and np.array_equal(G.matrix_of(right[i]), M)
    p, nb = G.operand_position(c, "left")
    assert p == N - 1 - i and nb == p - 1 and G.center(c, "left") == N - i - 1 and G.center(c, "right") == i + 2
    assert left[p].shape == (c.k, 2, c.m // 2)
    # the sweeps stop behind the operand: right sweeps sites 0 .. center - 2, left sweeps sites center .. N - 1 (0-based)
    assert G.swept(c, "right") == list(range(G.center(c, "right") - 1))
    assert G.swept(c, "left") == list(range(G.center(c, "left"), N))
    # the state: the head is a permutation of the basis, so |v| = |M w| with w = T last, and the mirror reverses the bits
    v = G.dense(right)
    w = np.tensordot(T, last, axes=([2], [0])).reshape(c.k, 4)
    assert abs(np.linalg.norm(v) - np.linalg.norm(M @ w)) <= 1e-14 * np.linalg.norm(M)
    vl = G.dense(left).reshape((2,) * N).transpose(tuple(range(N - 1, -1, -1))).reshape(-1)
    assert np.abs(vl - v).max() <= 1e-14 * np.abs(v).max()


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_rank_is_unambiguous_and_reference_is_stable(c):
    ref = G.reference(c.name)
    assert ref.r == O.truncation_rank(ref.sigma, c.cutoff * 100.0, c.maxdim) == O.truncation_rank(ref.sigma, c.cutoff / 100.0, c.maxdim)
    want = {"flat": min(c.m, c.k), "graded": min(c.m, c.k), "graded_shuffled": min(c.m, c.k), "keep": min(c.m, c.k),
            "cap": c.maxdim, "cut": min(c.m, c.k) - min(c.m, c.k) // 4, "deficient": c.rank}[c.kind]
    assert ref.r == want
    S2, r2, M2 = G.truncated(c, "gesvd")
    assert r2 == ref.r
    v2 = G.dense(G.chain_with(c, M2, "right"))
    dev = np.linalg.norm(v2 - ref.v["right"]) / ref.fro
    assert dev <= 1e-13, dev


@pytest.mark.parametrize("direction", G.DIRECTIONS)
@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_oracle_passes_the_device_assertions(c, direction):
    up = G.chain(c, direction)
    data = [t.copy() for t in up]
    psi = O.ZTMPS(data, amplitude=G.AMPLITUDE) if c.paired else O.SignalMPS(data, amplitude=G.AMPLITUDE)
    O.canonicalize(psi, direction, center=G.center(c, direction), cutoff=c.cutoff, maxdim=c.maxdim)
    G.check_result(c, direction, [np.asarray(t) for t in psi.data], up, psi.amplitude)


# ---------------------------------------------------------------- routes
@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_case_lies_where_its_label_assumes(c):
    events, rounds, margins = G.predicted(c.name)
    assert c.route in G.LABELS and c.route in events, (c.route, events)
    for what, factor in margins.items():
        assert factor >= G.MARGIN, (what, factor)
    cls, kk, tall = G.shape_class(c.m, c.k, c.dtype), min(c.m, c.k), c.m >= c.k
    if cls != "general" and c.cert and c.kind == "flat":
        assert ("cert-mid" if cls == "mid" else "cert-640") in events              # flat passes the certificate's bound ...
    if cls != "general" and c.kind == "cut":
        assert "cert-declined" in events                                            # ... and cut fails it
    if cls == "mid" and tall:
        assert ("sorted" in events) == (c.kind == "graded_shuffled")               # spread > 1e3 and disorder >= 0.2
        if c.kind == "graded":
            assert "second-QR" in events                                            # grade of R's diagonal in (1e3, 1e24)
        if c.kind == "deficient" and kk >= 64 and "lowrank" not in events:
            assert events == ("deflated",)                                          # grade >= 1e24
    if c.kind == "cap":
        assert not {"cert-mid", "cert-640", "cert-declined"} & set(events)          # r0 > maxdim: no certificate
    if rounds:
        assert rounds == ("gram" if c.dtype == "f64" else "vector")


def test_every_label_for_each_dtype_and_both_sides_of_every_boundary():
    for label in G.LABELS:
        for dt in G.DTYPES:
            assert any(c.route == label and c.dtype == dt for c in G.CASES), (label, dt)
    # the vector rounds of complex operands: every row count per lane the kernels are instantiated for (km = 1 .. 9)
    kms = {(min(c.m, c.k) + 63) // 64 for c in G.CASES if c.dtype == "c64" and G.predicted(c.name)[1] == "vector"}
    assert kms == set(range(1, 10)), kms
    # every tall width of the list carries flat and cut in both dtypes (so does each side of every boundary pair)
    assert {k for pair in G.BOUNDARIES for k in pair} <= set(G.TALL_WIDTHS)
    for k in G.TALL_WIDTHS:
        for kind in ("flat", "cut"):
            dts = {c.dtype for c in G.CASES if c.kind == kind and c.k == k and c.m == G.pow2_at_least(k) and c.cert}
            assert dts == {"f64", "c64"}, (k, kind, dts)
    # the boundaries are boundaries: the two sides differ in the shape class or in a rule that reads the width
    assert G.shape_class(32, 16, "f64") == "general" and G.shape_class(64, 48, "c64") == "general"
    assert G.shape_class(64, 49, "f64") == G.shape_class(4096, 40, "c64") == "mid"
    assert G.shape_class(1024, 576, "c64") == "mid" and G.shape_class(1024, 577, "c64") == "general"
    assert G.shape_class(1024, 577, "f64") == G.shape_class(1024, 639, "f64") == "mid" and G.shape_class(1024, 640, "f64") == "big"
    for kind in sorted({c.kind for c in G.CASES} - {"flat", "cut"}):
        assert {c.k for c in G.CASES if c.kind == kind and c.m >= c.k} <= set(G.REST_WIDTHS) | {383, 48, 577}, kind
    assert sum(c.paired for c in G.CASES) == 1 and 80 <= len(G.CASES) <= 160


# ---------------------------------------------------------------- the parser
DEBUG_TEXT = """\
[svd] 16 x 16: orientation + QR 0.1 ms
[svd] 16 x 16: scalar sweeps 0.1 ms
[svd-left] 256 x 256: column norms 1 ... 1, disorder 0.000 (left as they are)
[svd-left] 256 x 256: mean / min |r_ii|^2 = 1 -> rotate R
[svd-cert] k = 256: cutoff |R|_F^2 |R^-1|_F^2 = 6.554e-08 -> nothing can be truncated: QR gauge
[svd-left] 256 x 256: certificate: QR gauge 0.21 ms
[svd-left] 512 x 300: column norms 3.1 ... 0.0004, disorder 0.331
[svd-left] 512 x 300: columns sorted by norm (3.1 ... 0.0004)
[svd-left] 512 x 300: mean / min |r_ii|^2 = 4.1e+12 -> second QR
[svd-left] 512 x 300: QR 0.80 ms
[svd-cert] k = 300: cutoff |R|_F^2 |R^-1|_F^2 = 3.1e+02 -> SVD
[svd-left] 512 x 300: certificate: declined 0.30 ms
[svd-left] gram sweep 0 (300 cols, blocks of 16): rotated=1 above-quadratic=1
[svd-left] gram sweep 1 (300 cols, blocks of 16): rotated=1 above-quadratic=0
[svd-left] 512 x 300: sweeps 2.00 ms
[svd-left] 512 x 300: factors out 0.20 ms
"""


def test_parser_reads_the_librarys_lines():
    assert G.parse_debug(DEBUG_TEXT, 512, 300) == (("sorted", "second-QR", "cert-declined"), "gram")
    assert G.parse_debug(DEBUG_TEXT, 256, 256) == (("cert-mid",), None)
    assert G.parse_debug(DEBUG_TEXT, 16, 16) == (("general",), None)
    assert G.parse_debug(DEBUG_TEXT, 300, 512) == (("sorted", "second-QR", "cert-declined"), "gram")
    big = ("[svd-cert] 700 x 1024 (lda 700), absorb 1: declined\n"
           "[svd-lowrank] 700 x 1024, k = 128: residual^2 / total = 1.000e-31 (cutoff 1.0e-12)\n"
           "[svd-lowrank] 700 x 1024, k = 128: sketch accepted\n"
           "[svd-left] 1024 x 128: column norms 1 ... 1, disorder 0.300 (left as they are)\n"
           "[svd-left] 1024 x 128: sweeps 1.00 ms\n")
    assert G.parse_debug(big, 1024, 700) == (("cert-declined", "lowrank"), None)
    bj = ("[svd-cert] 1024 x 640 (lda 1024), absorb 2: QR gauge\n", "[svd] 1024 x 640: orientation + QR 1.0 ms\n"
          "[svd] block sweep 0 (cols 640): above tol=1, worst relative off-diagonal 0.1\n[svd] 1024 x 640: block sweeps 9.0 ms\n")
    assert G.parse_debug(bj[0], 1024, 640) == (("cert-640",), None)
    assert G.parse_debug(bj[1], 1024, 640) == (("block-jacobi",), None)
    wide = ("[svd-left] deflation (wide): 42 of 128 rows of R carry all but 1.0e-30 of the weight\n"
            "[svd-left] 128 x 42: mean / min |r_ii|^2 = 1.2 -> rotate R\n[svd-left] 128 x 42: sweeps 0.30 ms\n"
            "[svd-left] 128 x 140: deflated route (wide) 1.00 ms\n")
    assert G.parse_debug(wide, 128, 140) == (("deflated-wide",), None)
    vec = "[svd-left] 128 x 140: QR 0.1 ms\n[svd-left] sweep 0 (128 cols, blocks of 8): rotated=1 above-quadratic=0\n[svd-left] 128 x 140: sweeps 0.30 ms\n"
    assert G.parse_debug(vec, 128, 140) == (("rotate-R",), "vector")
