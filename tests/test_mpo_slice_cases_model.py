"""CPU: the numpy reference of the operator read-outs (tests/mpo_slice_cases.reference_slice) pinned against helpers.dense_mpo,
the dense M[in, out] every other operator test uses -- and the device front-ends' spec builders against the same matrix, so
that what the GPU tests compare with is the convention the project already has.  No GPU, no native call."""
import numpy as np
import pytest

from helpers import dense_mpo, random_mpo_data
import mpo_slice_cases as MC
from mpo_slice_cases import FREE, SUM, TIE, DIAG, reference_slice


def _bits(j, n):
    return [(j >> (n - 1 - i)) & 1 for i in range(n)]


@pytest.fixture(scope="module", params=[np.float64, np.complex128], ids=["f64", "c64"])
def chain(request):
    rng = np.random.default_rng(2711 + (request.param == np.complex128))
    data = random_mpo_data([2, 3, 4, 3], rng, request.param)
    return data, dense_mpo(data), MC.dense_legs(data)


def _near(got, ref):
    ref = np.asarray(ref)
    assert np.shape(got) == ref.shape
    assert np.abs(np.asarray(got, dtype=np.clongdouble) - ref).max() <= 1e-14 * max(np.abs(ref).max(), 1e-300)


def test_an_all_fixed_spec_is_the_entry(chain):
    data, M, dense = chain
    n = len(data)
    rng = np.random.default_rng(1)
    for i, o in rng.integers(0, 2 ** n, (40, 2)):
        spec = np.stack([_bits(int(i), n), _bits(int(o), n)], axis=1)
        _near(reference_slice(data, spec, dense), M[i, o])


def test_ties_and_sums_are_the_trace_and_the_total(chain):
    data, M, dense = chain
    n = len(data)
    _near(reference_slice(data, np.full((n, 2), TIE), dense), np.trace(M))
    _near(reference_slice(data, np.full((n, 2), SUM), dense), M.sum())
    _near(reference_slice(data, np.full((n, 2), DIAG), dense), np.diag(M))


def test_the_column_and_row_specs_are_rows_and_columns_of_the_dense_matrix(chain):
    """'column' is the project's word for W applied to a basis state: with out[o] = sum_in M[in, o] psi[in] it is M[j, :]."""
    data, M, dense = chain
    n = len(data)
    for j in (0, 5, 2 ** n - 1):
        col = np.stack([_bits(j, n), [FREE] * n], axis=1)
        _near(reference_slice(data, col, dense), M[j, :])
        row = np.stack([[FREE] * n, _bits(j, n)], axis=1)
        _near(reference_slice(data, row, dense), M[:, j])
    _near(reference_slice(data, np.stack([[SUM] * n, [FREE] * n], axis=1), dense), M.sum(axis=0))
    _near(reference_slice(data, np.stack([[FREE] * n, [SUM] * n], axis=1), dense), M.sum(axis=1))


def test_mixed_specs_against_the_dense_matrix(chain):
    """one of each: site 0 traced, site 1 in kept / out summed, site 2 diagonal, site 3 fixed (1, 0), site 4 out kept / in 1"""
    data, M, dense = chain
    n = len(data)
    T = M.reshape([2] * (2 * n))                                 # in_1 .. in_n, out_1 .. out_n
    want = np.zeros((2, 2, 2), dtype=M.dtype)
    for s1 in range(2):
        for s2 in range(2):
            for s4 in range(2):
                want[s1, s2, s4] = sum(T[a, s1, s2, 1, 1, a, o1, s2, 0, s4] for a in range(2) for o1 in range(2))
    spec = np.array([(TIE, TIE), (FREE, SUM), (DIAG, DIAG), (1, 0), (1, FREE)])
    _near(reference_slice(data, spec, dense), want.reshape(-1))
    assert MC.kept_positions(spec) == [1, 2, 4] and not MC.whole_pairs(spec)


def test_the_tables_cover_every_form():
    rng = np.random.default_rng(3)
    for n in (6, 8):
        specs = MC.slice_specs(n, rng)
        seen = {tuple(int(v) for v in row) for s in specs.values() for row in s}
        assert set(MC.REMOVED_FORMS) <= seen and set(MC.KEPT_FORMS) <= seen
        assert all(s.shape == (n, 2) and MC.kept_positions(s) for s in specs.values())
        rows, kinds = MC.entry_rows(n, rng)
        assert rows.shape == (300, n, 2) and rows.max() == TIE and not np.any(rows == FREE)
        assert np.all(rows[kinds == MC.ENTRY] <= 1) and np.all(rows[kinds == MC.SUMS] <= SUM)
        assert np.all(rows[100] == SUM) and np.all(rows[200] == TIE)
        assert all(np.any(r == SUM) for r in rows[kinds == MC.SUMS]) and all(np.any(r == TIE) for r in rows[kinds == MC.TRACES])
        assert np.all((rows[..., 0] == TIE) == (rows[..., 1] == TIE))
    assert all(len(b) % 2 == 1 for b in MC.ENTRY_PROFILES.values())       # even chain lengths: every profile runs paired too
    assert max(MC.ENTRY_ONLY_PROFILES["above_cap"]) == 1025


class _Seen(Exception):
    pass


def test_front_end_specs_follow_the_same_convention(monkeypatch, chain):
    """mpo_entries, mpo_column, mpo_row, the sums and the diagonal build their specs so that the reference gives the dense
    matrix's entries, rows and columns: the native entries are replaced by the reference here."""
    import importlib
    import qilaplace_jl_amd as qil
    L = importlib.import_module("qilaplace_jl_amd._lib")
    data, M, dense = chain
    n = len(data)
    W = object.__new__(qil.SingleSiteMPO)
    W.handle, W.ctx = None, None
    monkeypatch.setattr(type(W), "dtype", property(lambda self: data[0].dtype.type))
    seen = {}

    def nsites(handle, ref):
        ref._obj.value = n
        return 0

    def entry_batch(handle, nb, sp, out):
        specs = np.ctypeslib.as_array(sp, shape=(nb, n, 2))
        vals = np.array([complex(reference_slice(data, s, dense)) for s in specs])
        np.ctypeslib.as_array(out, shape=(2 * nb,))[:] = vals.view(np.float64)
        return 0

    def slice_(handle, sp, out):
        seen["spec"] = np.ctypeslib.as_array(sp, shape=(n, 2)).copy()
        raise _Seen                                               # the spec is what this test is after

    monkeypatch.setattr(L.lib, "qil_mpo_nsites", nsites)
    monkeypatch.setattr(L.lib, "qil_mpo_entry_batch", entry_batch)
    monkeypatch.setattr(L.lib, "qil_mpo_slice", slice_)
    got = qil.mpo_to_matrix(W)
    assert got.dtype == M.dtype
    _near(got, M)
    _near(qil.mpo_entries(W, [3, "10110", _bits(9, n)], np.array([0, 7])), M[[3, 22, 9]][:, [0, 7]])
    _near(qil.mpo_entry(W, 5, "00011"), M[5, 3])
    for fn, want in ((lambda: qil.mpo_column(W, 6), M[6, :]), (lambda: qil.mpo_row(W, 6), M[:, 6]),
                     (lambda: qil.mpo_diagonal_state(W), np.diag(M)), (lambda: qil.mpo_column_sums(W), M.sum(axis=0)),
                     (lambda: qil.mpo_row_sums(W), M.sum(axis=1))):
        with pytest.raises(_Seen):
            fn()
        _near(reference_slice(data, seen["spec"], dense), want)
