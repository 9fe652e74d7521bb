"""Host-side operator API mirroring the reference's method names (drop-in boundary):

  apply / `*`        src/linalg/apply.jl:75-122, 124-199, 201-230, 233-236
  coefficient        src/mps.jl:669-693 (parsers :616-645)
  mps_to_vector      src/mps.jl:716-743
  norm               src/mps.jl:754-771
  inner              ITensors' inner(phi, psi) / inner(phi, W, psi) on device chains (no reference counterpart)
  sample             ITensors' sample(::MPS) on device chains (no reference counterpart)
  top_k              the k largest |psi_x| by a certified beam search (no reference counterpart: replaces argmax over grid scans)
  product_batch      the contraction of coefficient with a weighted sum of the two physical slices per site: sum_j x_j w^j at any
                     complex w (laplace_sum, dft_eval, dt_eval, zt_eval, refine_frequencies; no reference counterpart)
  hadamard, adjoint  element-wise products of states and W^dagger; convolve / correlate / power_spectrum on top of them (no
                     reference counterpart)
  mpo_linear_combination, mpo_inner   sums and Frobenius overlaps of operators, with mpo_norm / mpo_distance / mpo_trace and
                     `+`, `-`, `c *` on the MPO classes on top of them (no reference counterpart)
  mpo_entry_batch, mpo_slice   numbers and state-valued slices of an operator on its own bonds, with mpo_entries / mpo_to_matrix /
                     mpo_column / mpo_row / mpo_diagonal_state / mpo_column_sums / mpo_row_sums on top of them (no reference
                     counterpart)
  environment, esprit   the partial contraction <phi|...|psi> / <phi|W|...|psi> with open bond legs, and on top of it shift_pencil /
                     esprit_from_pencil / esprit: the poles of a sum of exponentials from the bond basis, no scan (no reference
                     counterpart)
  solve              (A + shift I) x = c by the alternating two-site solver with a CG local solve, and least_squares / smooth /
                     solve_residual on top of it (no reference counterpart)
  eigs               the smallest / largest eigenpairs of a Hermitian operator by two-site DMRG with a Lanczos local solve, and
                     eig_residual / operator_norm / condition_number on top of it (no reference counterpart)
  canonicalize       src/mps.jl:787-847, 866-901   (Julia: canonicalize!)
  compress           src/mps.jl:913-999            (Julia: compress!)
  signal_mps         src/signals/SignalConverters.jl:228-233
  signal_ztmps       src/signals/SignalConverters.jl:247-283
  rsvd               src/linalg/rsvd.jl:38-121

All arithmetic happens in libqilhip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import re
import warnings

import numpy as np

from . import _lib as L
from .containers import (SignalMPS, ZTMPS, SingleSiteMPO, PairedSiteMPO, default_context, _np_dtype)


def _wrap_like(psi, handle):
    return type(psi)(ctx=psi.ctx, _handle=handle)


# ---------------------------------------------------------------- apply
def apply(W, psi, out=None, **kwargs):
    """apply(W, psi; kwargs...) -> psi_out.  ``cutoff``/``maxdim`` kwargs are accepted and
    ignored, exactly like the reference (apply.jl:75): apply never truncates."""
    if isinstance(W, SingleSiteMPO) and isinstance(psi, SingleSiteMPO):
        if W.paired != psi.paired:
            raise TypeError("apply: cannot mix SingleSiteMPO and PairedSiteMPO")
        h = C.c_void_p()
        L.check(L.lib.qil_apply_mpo_mpo(W.handle, psi.handle, C.byref(h)))
        return type(W)(ctx=W.ctx, _handle=h)
    if not (isinstance(W, SingleSiteMPO) and isinstance(psi, SignalMPS)):
        raise TypeError("apply: unsupported operand types")
    if W.paired != psi.paired:
        raise TypeError("apply: PairedSiteMPO acts on ZTMPS, SingleSiteMPO on SignalMPS")
    if out is not None:
        L.check(L.lib.qil_apply_into(W.handle, psi.handle, out.handle))
        return out
    h = C.c_void_p()
    L.check(L.lib.qil_apply(W.handle, psi.handle, C.byref(h)))
    return _wrap_like(psi, h)


def _mul(self, other):
    return apply(self, other)


SingleSiteMPO.__mul__ = _mul          # W * psi, W1 * W2  (apply.jl:233-236)


# ---------------------------------------------------------------- coefficient
def _parse_config(spec, n):
    """Front-ends of `coefficient` (src/mps.jl:616-645, 680-693)."""
    if isinstance(spec, str):
        s = spec.strip().strip("[](){}").strip()
        if not s:
            raise ValueError("coefficient: configuration string is empty")
        if re.search(r"[,\s]", s):
            toks = [t for t in re.split(r"[,\s]+", s) if t]
            if not toks:
                raise ValueError("coefficient: configuration string did not contain any entries")
            return [int(t) for t in toks]
        if any(c not in "01" for c in s):
            raise ValueError("coefficient: bit strings may contain only '0' or '1'")
        return [1 if c == "1" else 0 for c in s]
    if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
        v = int(spec)
        if v < 0:
            raise ValueError("coefficient: integer configuration must be non-negative")
        if v >> n:
            raise ValueError(f"coefficient: integer {v} requires more than {n} bits")
        return [(v >> (n - 1 - i)) & 1 for i in range(n)]
    return [int(b) for b in spec]


def _ntensors(psi):
    return psi.ntensors if isinstance(psi, (ZTMPS, PairedSiteMPO)) else len(psi)


def _bits_array(psi, bits, max_bit=1):
    n = _ntensors(psi)
    b = np.asarray(bits)
    if b.ndim != 2 or b.shape[1] != n:
        got = b.shape[1] if b.ndim == 2 else b.shape
        raise ValueError(f"coefficient: expected {n} entries, got {got}")
    if b.size and (b.min() < 0 or b.max() > max_bit):
        bad = int(b[(b < 0) | (b > max_bit)][0])
        raise ValueError(f"coefficient: bit value {bad} outside [0,{max_bit}]")
    return np.ascontiguousarray(b, dtype=np.uint8)


def coefficient_batch(psi, bits):
    """Vectorised `coefficient`: bits is (nb, n_tensors) of {0,1}; returns (nb,) values
    (complex for complex MPS, real otherwise), each amplitude * prod_i A_i[:, bit_i, :]."""
    b = _bits_array(psi, bits)
    nb = b.shape[0]
    out = np.zeros(nb, dtype=np.complex128)
    L.check(L.lib.qil_coefficient_batch(psi.handle, nb, b.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        out.ctypes.data_as(C.POINTER(C.c_double))))
    return out if psi.dtype == np.complex128 else out.real.copy()


def marginal_batch(psi, bits):
    """Like coefficient_batch, but a bit value of 2 SUMS that site's physical index (marginal).  One
    chain then replaces 2^m coefficient calls when m sites are summed."""
    b = _bits_array(psi, bits, max_bit=2)
    nb = b.shape[0]
    out = np.zeros(nb, dtype=np.complex128)
    L.check(L.lib.qil_coefficient_marginal_batch(psi.handle, nb, b.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 out.ctypes.data_as(C.POINTER(C.c_double))))
    return out if psi.dtype == np.complex128 else out.real.copy()


def _lsb_bits(vals, n):
    v = np.asarray(vals, dtype=np.int64)
    return ((v[:, None] >> np.arange(n)[None, :]) & 1).astype(np.uint8)


def _msb_bits(vals, n):
    v = np.asarray(vals, dtype=np.int64)
    return ((v[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)


def coefficient_grid(psi, ks, ls, chunk=1 << 16):
    """chi[k, l] = coefficient(psi, interleave(lsb(k), lsb(l))) for a transformed ZTMPS (the (k, l) scans
    of docs/src/tutorials/zt.jl:152-157, 283-309) -- all pairs in batched launches."""
    n = len(psi)
    ks, ls = np.asarray(ks, dtype=np.int64), np.asarray(ls, dtype=np.int64)
    rk, rl = _bit_block_range(ks), _bit_block_range(ls)
    if rk is not None and rl is not None and rk[0] + rk[1] <= n and rl[0] + rl[1] <= n and rk[1] + rl[1] <= 30:
        # a 2^a x 2^b grid of aligned power-of-two strides (the tutorials' full and coarse scans) = every
        # configuration of a bit block of each register with the other bits fixed at 0: one dense block read-out
        # instead of 2^(a+b) chains
        (sk, a), (sl, b) = rk, rl
        spec = np.zeros(2 * n, dtype=np.uint8)
        spec[2 * sk:2 * (sk + a):2] = FREE
        spec[2 * sl + 1:2 * (sl + b) + 1:2] = FREE
        t = np.asarray(mps_block(psi, spec, reverse=True)).reshape([2] * (a + b))   # axis 0 = LAST free site
        free_sites = sorted([2 * (sk + i) for i in range(a)] + [2 * (sl + i) + 1 for i in range(b)])
        axis_of = {site: (a + b - 1 - pos) for pos, site in enumerate(free_sites)}
        order = ([axis_of[2 * (sk + i)] for i in range(a - 1, -1, -1)] +
                 [axis_of[2 * (sl + i) + 1] for i in range(b - 1, -1, -1)])
        return np.ascontiguousarray(t.transpose(order)).reshape(2 ** a, 2 ** b).astype(np.complex128)
    kb, lb = _lsb_bits(ks, n), _lsb_bits(ls, n)
    out = np.empty((len(ks), len(ls)), dtype=np.complex128)
    rows = max(1, chunk // max(len(ls), 1))
    for r0 in range(0, len(ks), rows):
        kk = kb[r0:r0 + rows]
        bits = np.empty((len(kk), len(ls), 2 * n), dtype=np.uint8)
        bits[:, :, 0::2] = kk[:, None, :]
        bits[:, :, 1::2] = lb[None, :, :]
        out[r0:r0 + rows] = np.asarray(coefficient_batch(psi, bits.reshape(-1, 2 * n))).reshape(len(kk), len(ls))
    return out


def laplace_values(psi_out, ks, dt):
    """L(s_k) = dt sqrt(N) sum_j coefficient(psi_out, interleave(lsb(k), msb(j))) for a damping-transformed
    ZTMPS (docs/src/tutorials/dt.jl:172-197).  The sum over the copy register is a marginal: one chain per
    k instead of N coefficient calls."""
    n = len(psi_out)
    a = _full_low_range(ks)
    if a is not None and a <= min(n, 30):
        # all of k = 0 .. 2^a - 1: main bits free (lsb first), copy register summed -- one dense contraction
        spec = np.full(2 * n, SUM, dtype=np.uint8)
        spec[0::2] = FIX0
        spec[0:2 * a:2] = FREE
        return dt * np.sqrt(2.0 ** n) * mps_block(psi_out, spec, reverse=True)
    kb = _lsb_bits(ks, n)
    bits = np.full((len(kb), 2 * n), 2, dtype=np.uint8)
    bits[:, 0::2] = kb
    return dt * np.sqrt(2.0 ** n) * marginal_batch(psi_out, bits)


def coefficient(psi, config):
    """coefficient(psi, config): config is a list/tuple of bits, a bit string ("101" or
    "[1,0,1]") or a non-negative integer read as an n-bit big-endian pattern."""
    n = _ntensors(psi)
    bits = _parse_config(config, n)
    if len(bits) != n:
        raise ValueError(f"coefficient: expected {n} entries, got {len(bits)}")
    return coefficient_batch(psi, [bits])[0]


def apply_coefficient_batch(W, psi, bits):
    """<bits| W psi> without materialising W*psi (lazy path; same numbers as
    coefficient_batch(apply(W, psi), bits))."""
    b = _bits_array(psi, bits)
    nb = b.shape[0]
    out = np.zeros(nb, dtype=np.complex128)
    L.check(L.lib.qil_apply_coefficient_batch(W.handle, psi.handle, nb,
                                              b.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              out.ctypes.data_as(C.POINTER(C.c_double))))
    if psi.dtype == np.complex128 or W.dtype == np.complex128:
        return out
    return out.real.copy()


def apply_coefficient_sweep(Ws, psi, bits, comm=None, n_items=None):
    """For every operator of `Ws` (e.g. the DT MPOs of a damping sweep): materialise W * psi with the apply kernel
    and read it out at the same configurations -- the loop `out = W * psi; coefficient(out, bits)` of the
    reference's sweeps (docs/src/tutorials/dt.jl:150-197) with one upload, one download and one synchronisation
    for the whole batch.  Returns a (len(Ws), nb) complex array.

    With `comm` (a `sweep.Comm`) the call is COLLECTIVE: `Ws` is this rank's round-robin share of `n_items` operators, the
    samples stay in HBM, one all-gather exchanges them (qil_apply_coefficient_sweep_gather) and every rank gets the
    (n_items, nb) table in item order."""
    Ws = list(Ws)
    b = _bits_array(psi, bits)
    nb = b.shape[0]
    if comm is not None:
        if n_items is None:
            raise ValueError("apply_coefficient_sweep: n_items is required with a communicator")
        out = np.zeros((int(n_items), nb), dtype=np.complex128)
        hs = (C.c_void_p * max(len(Ws), 1))(*[W.handle for W in Ws])
        L.check(L.lib.qil_apply_coefficient_sweep_gather(comm.handle, hs, len(Ws), psi.handle, nb, b.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                         int(n_items), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out
    out = np.zeros((len(Ws), nb), dtype=np.complex128)
    if not Ws or nb == 0:
        return out
    hs = (C.c_void_p * len(Ws))(*[W.handle for W in Ws])
    L.check(L.lib.qil_apply_coefficient_sweep(hs, len(Ws), psi.handle, nb, b.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


# ---------------------------------------------------------------- dense read-out, norm
def mps_to_vector(psi, reverse=False):
    n = _ntensors(psi)
    out = np.empty(2 ** n, dtype=psi.dtype)
    L.check(L.lib.qil_mps_to_vector(psi.handle, 1 if reverse else 0, out.ctypes.data_as(C.c_void_p)))
    return out


FIX0, FIX1, SUM, FREE = 0, 1, 2, 3


def mps_block(psi, spec, reverse=False):
    """All 2^F coefficients of the configurations that agree with `spec` on its fixed sites, as one dense
    contraction: spec[i] = 0 / 1 fixes site i's bit, 2 (SUM) sums the site, 3 (FREE) leaves it free.  The result is
    indexed by the free sites in chain order, the first one the most significant bit (reverse=False, like
    mps_to_vector) or the least (reverse=True)."""
    n = _ntensors(psi)
    sp = np.ascontiguousarray(np.asarray(spec), dtype=np.uint8)
    if sp.shape != (n,):
        raise ValueError(f"coefficient: expected {n} entries, got {sp.shape}")
    if sp.size and sp.max() > 3:
        raise ValueError(f"coefficient: spec value {int(sp.max())} outside [0,3]")
    out = np.empty(2 ** int((sp == FREE).sum()), dtype=psi.dtype)
    L.check(L.lib.qil_mps_block(psi.handle, sp.ctypes.data_as(C.POINTER(C.c_uint8)), 1 if reverse else 0,
                                out.ctypes.data_as(C.c_void_p)))
    return out


def restrict(psi, spec):
    """The part of `psi` that agrees with `spec`, as a state of its own (qil_mps_restrict): spec[i] = FIX0 / FIX1 fixes tensor
    i's bit, SUM sums the site, FREE keeps it -- the vocabulary of `mps_block`, but the kept sites stay site tensors, so the
    result works at any size with every verb that takes a state (`norm`, `top_k`, `sample`, `inner`, `hadamard`, ...).

    The result has psi's dtype and amplitude (`norm(out) * out.amplitude` is the 2-norm of the slice), the kept sites' ids and
    no bond larger than the parent's.  It is a ZTMPS when psi is one and whole (main_i, copy_i) pairs are kept, a SignalMPS
    otherwise.  A spec that keeps no site is a number: `coefficient` / `marginal_batch` return it."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("restrict: unsupported operand types")
    n = _ntensors(psi)
    sp = np.ascontiguousarray(np.asarray(spec), dtype=np.uint8)
    if sp.shape != (n,):
        raise ValueError(f"coefficient: expected {n} entries, got {sp.shape}")
    if sp.size and sp.max() > 3:
        raise ValueError(f"coefficient: spec value {int(sp.max())} outside [0,3]")
    h = C.c_void_p()
    L.check(L.lib.qil_mps_restrict(psi.handle, sp.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(h)))
    paired = C.c_int()
    L.lib.qil_mps_is_paired(h, C.byref(paired))
    return (ZTMPS if paired.value else SignalMPS)(ctx=psi.ctx, _handle=h)


def _register_spec(psi, what, fixed_offset, value, summed=False):
    """spec of a ZTMPS with one register (0 = main, 1 = copy) set to the lsb-first bits of `value` (or to SUM) and the other
    register kept"""
    if not isinstance(psi, ZTMPS):
        raise TypeError(f"{what}: needs a ZTMPS")
    n = len(psi)
    spec = np.full(2 * n, FREE, dtype=np.uint8)
    if summed:
        spec[fixed_offset::2] = SUM
        return spec
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{what}: the index must be an integer")
    if not 0 <= int(value) < 2 ** n:
        raise ValueError(f"{what}: index {int(value)} outside [0, 2^{n})")
    spec[fixed_offset::2] = [(int(value) >> i) & 1 for i in range(n)]
    return spec


def zt_row(psi, l):
    """Row l of a transformed ZTMPS's (k, l) grid as an n-site SignalMPS over k: the copy sites fixed to the bits of l, so that
    coefficient_batch(zt_row(psi, l), _lsb_bits([k], n)) == coefficient_grid(psi, [k], [l]) for every k."""
    return restrict(psi, _register_spec(psi, "zt_row", 1, l))


def zt_column(psi, k):
    """Column k of a transformed ZTMPS's (k, l) grid as an n-site SignalMPS over l: the main sites fixed to the bits of k, so
    that coefficient_batch(zt_column(psi, k), _lsb_bits([l], n)) == coefficient_grid(psi, [k], [l]) for every l."""
    return restrict(psi, _register_spec(psi, "zt_column", 0, k))


def copy_marginal(psi):
    """The copy register of a damping-transformed ZTMPS summed out; the coefficients of the n-site result are the Laplace
    values: laplace_values(psi, ks, dt) == dt * sqrt(2**n) * coefficient_batch(copy_marginal(psi), _lsb_bits(ks, n))."""
    return restrict(psi, _register_spec(psi, "copy_marginal", 1, None, summed=True))


# ---------------------------------------------------------------- Born weights
TRACE = 2


def _weight_specs(psi, specs):
    if not isinstance(psi, SignalMPS):
        raise TypeError("weight: unsupported operand types")
    n = _ntensors(psi)
    sp = np.asarray(specs)
    if sp.ndim != 2 or sp.shape[1] != n:
        got = sp.shape[1] if sp.ndim == 2 else sp.shape
        raise ValueError(f"coefficient: expected {n} entries, got {got}")
    if sp.size and (sp.min() < 0 or sp.max() > TRACE):
        bad = int(sp[(sp < 0) | (sp > TRACE)][0])
        raise ValueError(f"coefficient: spec value {bad} outside [0,2]")
    return np.ascontiguousarray(sp, dtype=np.uint8)


def weight_batch(psi, specs):
    """Born weights (qil_weight_batch): specs is (nb, n_tensors) of FIX0 / FIX1 / TRACE; returns the (nb,) float64 array
    amplitude^2 * sum |psi_x|^2 over the configurations x that agree with each row on its fixed tensors -- TRACE sums a site in
    |psi|^2, where `marginal_batch`'s 2 sums amplitudes.  A row without TRACE is abs(coefficient)^2, a row of all TRACE is
    (amplitude * norm)^2."""
    return _weigh(psi, specs, _native_weights)


def _native_weights(psi, sp):
    """the weigher of a state held on the device: qil_weight_batch on checked specs"""
    out = np.zeros(sp.shape[0], dtype=np.float64)
    if sp.shape[0]:
        L.check(L.lib.qil_weight_batch(psi.handle, sp.shape[0], sp.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _lazy_weights(W):
    """the weigher of W psi, never formed: qil_apply_weight_batch on checked specs"""
    def weigher(psi, sp):
        out = np.zeros(sp.shape[0], dtype=np.float64)
        if sp.shape[0]:
            L.check(L.lib.qil_apply_weight_batch(W.handle, psi.handle, sp.shape[0], sp.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 out.ctypes.data_as(C.POINTER(C.c_double))))
        return out
    return weigher


def _weigh(psi, specs, weigher):
    """Every front-end below ends here: the spec checks of `weight_batch`, then the weigher -- `_native_weights` for the state
    itself, `_lazy_weights(W)` for W psi."""
    return weigher(psi, _weight_specs(psi, specs))


def weight(psi, spec):
    """`weight_batch` of one spec, as a float."""
    return _weight(psi, spec, _native_weights)


def _weight(psi, spec, weigher):
    return float(_weigh(psi, np.asarray(spec)[None], weigher)[0])


def bit_probabilities(psi):
    """P(bit i = 1) under |psi|^2 for every tensor i, from one call: n rows all traced but one FIX1, and the all-traced row
    as the divisor."""
    return _bit_probabilities(psi, _native_weights)


def _bit_probabilities(psi, weigher):
    if not isinstance(psi, SignalMPS):
        raise TypeError("weight: unsupported operand types")
    n = _ntensors(psi)
    sp = np.full((n + 1, n), TRACE, dtype=np.uint8)
    sp[np.arange(n), np.arange(n)] = FIX1
    w = _weigh(psi, sp, weigher)
    return w[:n] / w[n]


def _dyadic_blocks(lo, hi, n):
    """[lo, hi) as at most 2n aligned blocks (start, log2 size), in ascending order"""
    blocks = []
    while lo < hi:
        k = min((lo & -lo).bit_length() - 1 if lo else n, (hi - lo).bit_length() - 1)
        blocks.append((lo, k))
        lo += 1 << k
    return blocks


def range_weight(psi, lo, hi, reverse=False):
    """sum of |psi_x|^2 (times amplitude^2) over lo <= x < hi, x the big-endian integer of `coefficient(psi, int)` and `sample`:
    the power in a band of a spectrum.  [lo, hi) splits into at most 2n dyadic blocks -- a fixed prefix, the rest traced --
    whose weights come from one call.  At any n: nothing dense is formed.  reverse=True reads x with the first tensor as the
    LEAST significant bit, the order in which a QFT output holds its bin index (as `mps_to_vector(..., reverse=True)`)."""
    return _range_weight(psi, lo, hi, reverse, _native_weights)


def _range_weight(psi, lo, hi, reverse, weigher):
    if not isinstance(psi, SignalMPS):
        raise TypeError("weight: unsupported operand types")
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("range_weight: the bounds must be integers")
    n = _ntensors(psi)
    lo, hi = int(lo), int(hi)
    if not 0 <= lo <= hi <= 2 ** n:
        raise ValueError(f"range_weight: need 0 <= lo <= hi <= 2^{n}, got [{lo}, {hi})")
    if lo == hi:
        return 0.0
    blocks = _dyadic_blocks(lo, hi, n)
    sp = np.full((len(blocks), n), TRACE, dtype=np.uint8)
    for r, (start, k) in enumerate(blocks):
        sp[r, :n - k] = [(start >> (n - 1 - i)) & 1 for i in range(n - k)]
    return float(np.sum(_weigh(psi, sp[:, ::-1] if reverse else sp, weigher)))


def weight_quantiles(psi, qs, reverse=False):
    """For every q of `qs` (each in [0, 1]) the smallest x, in the big-endian integer convention of `range_weight`, with
    sum_{y <= x} |psi_y|^2 >= q * total: q = 0.5 is the median frequency of a spectrum, 0.95 its 95 % edge.  The bits of all
    quantiles are found together from the top, one `weight_batch` call of len(qs) rows per tensor after one for the total.
    reverse=True as in `range_weight`: the first tensor is the least significant bit."""
    return _weight_quantiles(psi, qs, reverse, _native_weights)


def _weight_quantiles(psi, qs, reverse, weigher):
    if not isinstance(psi, SignalMPS):
        raise TypeError("weight: unsupported operand types")
    q = np.atleast_1d(np.asarray(qs, dtype=np.float64))
    if q.ndim != 1 or (q.size and not (np.all(q >= 0.0) and np.all(q <= 1.0))):
        raise ValueError("weight_quantiles: every q must lie in [0, 1]")
    n = _ntensors(psi)
    if not q.size:
        return np.zeros(0, dtype=np.int64 if n <= 62 else object)
    target = q * _weight(psi, np.full(n, TRACE, dtype=np.uint8), weigher)
    below = np.zeros(len(q))                           # the weight of everything under the prefix found so far
    sp = np.full((len(q), n), TRACE, dtype=np.uint8)
    for i in (range(n - 1, -1, -1) if reverse else range(n)):
        sp[:, i] = FIX0
        w0 = _weigh(psi, sp, weigher)
        up = below + w0 < target                       # the low half does not reach the target: the bit is 1
        sp[up, i] = FIX1
        below[up] += w0[up]
    xs = [int("".join(map(str, row[::-1] if reverse else row)), 2) for row in sp]
    return np.array(xs, dtype=np.int64 if n <= 62 else object)


def _register_weights(psi, what, fixed_offset, values, weigher=_native_weights):
    if not isinstance(psi, ZTMPS):
        raise TypeError(f"{what}: needs a ZTMPS")
    vals = list(np.atleast_1d(np.asarray(values, dtype=object)))
    sp = np.array([_register_spec(psi, what, fixed_offset, v) for v in vals], dtype=np.uint8).reshape(len(vals), 2 * len(psi))
    sp[sp == FREE] = TRACE
    return _weigh(psi, sp, weigher)


def zt_row_weights(psi, ls):
    """sum_k |Z(k, l)|^2 for every l of `ls`: the energy of damping rows of a transformed ZTMPS's (k, l) grid, in one call (the
    copy register fixed to the lsb-first bits of l as in `zt_row`, the main register traced)."""
    return _register_weights(psi, "zt_row_weights", 1, ls)


def zt_column_weights(psi, ks):
    """sum_l |Z(k, l)|^2 for every k of `ks`: the energy of frequency columns, the main register fixed as in `zt_column`."""
    return _register_weights(psi, "zt_column_weights", 0, ks)


# ---- the same read-outs of W psi, which is never formed (qil_apply_weight_batch): the bodies above with the lazy weigher
def apply_weight_batch(W, psi, specs):
    """`weight_batch(apply(W, psi), specs)` without the product: amplitude^2 * sum |(W psi)_x|^2 over the configurations that
    agree with each row, for operands whose product does not fit (the product's bond is chi * D).  A leading run of fixed
    tensors costs a lazy coefficient step per tensor, a trailing run of traced ones one quadratic form with a right environment
    shared by all rows, everything between the four products of `apply_norm` per tensor and row.  The rounding may depend on
    the other rows of the call (they decide the chunking); two identical calls give identical bits.
    Which to call (one MI355X, MEASUREMENTS section 16): where the product fits and the rows trace from the first tensor on, the
    lazy form is SLOWER -- 64 row energies of a natural zT operand at n = 20 (chi <= 8, D <= 80) take 119 ms here against 81 ms
    for `weight_batch(apply(W, psi))`.  It is faster for prefix-fixed rows (a 45-block band of the same operand: 9.9 against
    58 ms) and for wide bonds (chi 32, D 64: 48 against 319 ms for 8 rows), and it is the only exact way when the product does
    not fit."""
    _require_operator(W, psi)
    return _weigh(psi, specs, _lazy_weights(W))


def apply_weight(W, psi, spec):
    """`apply_weight_batch` of one spec, as a float."""
    _require_operator(W, psi)
    return _weight(psi, spec, _lazy_weights(W))


def apply_bit_probabilities(W, psi):
    """`bit_probabilities(apply(W, psi))` without the product."""
    _require_operator(W, psi)
    return _bit_probabilities(psi, _lazy_weights(W))


def apply_range_weight(W, psi, lo, hi, reverse=False):
    """`range_weight(apply(W, psi), lo, hi, reverse)` without the product: the power of a transformed signal in a band."""
    _require_operator(W, psi)
    return _range_weight(psi, lo, hi, reverse, _lazy_weights(W))


def apply_weight_quantiles(W, psi, qs, reverse=False):
    """`weight_quantiles(apply(W, psi), qs, reverse)` without the product."""
    _require_operator(W, psi)
    return _weight_quantiles(psi, qs, reverse, _lazy_weights(W))


def apply_zt_row_weights(W, psi, ls):
    """`zt_row_weights(apply(W, psi), ls)` without the product: psi a ZTMPS, W a PairedSiteMPO."""
    _require_operator(W, psi)
    return _register_weights(psi, "zt_row_weights", 1, ls, _lazy_weights(W))


def apply_zt_column_weights(W, psi, ks):
    """`zt_column_weights(apply(W, psi), ks)` without the product."""
    _require_operator(W, psi)
    return _register_weights(psi, "zt_column_weights", 0, ks, _lazy_weights(W))


def _bit_block_range(v):
    """(s, a) if v == arange(2^a) << s -- every pattern of bits s .. s+a-1, all other bits zero -- else None."""
    v = np.asarray(v, dtype=np.int64)
    a = int(round(np.log2(len(v)))) if len(v) else -1
    if a < 0 or len(v) != 2 ** a:
        return None
    if a == 0:
        return (0, 0) if v[0] == 0 else None
    step = int(v[1] - v[0])
    if step <= 0 or step & (step - 1) or not np.array_equal(v, step * np.arange(2 ** a, dtype=np.int64)):
        return None
    return step.bit_length() - 1, a


def _full_low_range(v):
    """log2(len) if v == arange(2^a), else None."""
    r = _bit_block_range(v)
    return r[1] if r is not None and (r[0] == 0 or r[1] == 0) else None


def norm(psi) -> float:
    v = C.c_double()
    L.check(L.lib.qil_norm(psi.handle, C.byref(v)))
    return v.value


# ---------------------------------------------------------------- overlaps
def _require_mps(x, what):
    if not isinstance(x, SignalMPS):
        raise TypeError(f"{what}: unsupported operand types")


def _require_operator(W, psi):
    """The operand checks of `apply`, made before any native call (the register kind is the container class's)."""
    if not (isinstance(W, SingleSiteMPO) and isinstance(psi, SignalMPS)):
        raise TypeError("apply: unsupported operand types")
    if W._paired() != psi._paired():
        raise TypeError("apply: PairedSiteMPO acts on ZTMPS, SingleSiteMPO on SignalMPS")


def _scalar(v, *operands):
    """float when every operand is real, complex otherwise (the rule of coefficient_batch)."""
    z = complex(v[0], v[1])
    return z if any(x.dtype == np.complex128 for x in operands) else z.real


def inner(phi, *args):
    """inner(phi, psi) = <phi|psi> and inner(phi, W, psi) = <phi|W psi>, amplitudes included: the same numbers as
    np.vdot(mps_to_vector(phi), mps_to_vector(psi)) and inner(phi, W * psi), without a dense vector or the product.
    float when every operand is real, complex otherwise."""
    v = (C.c_double * 2)()
    if len(args) == 1:
        (psi,) = args
        _require_mps(phi, "inner")
        _require_mps(psi, "inner")
        L.check(L.lib.qil_inner(phi.handle, psi.handle, v))
        return _scalar(v, phi, psi)
    if len(args) == 2:
        W, psi = args
        _require_mps(phi, "inner")
        _require_operator(W, psi)
        L.check(L.lib.qil_apply_inner(phi.handle, W.handle, psi.handle, v))
        return _scalar(v, phi, W, psi)
    raise TypeError(f"inner: expected inner(phi, psi) or inner(phi, W, psi), got {1 + len(args)} arguments")


def apply_norm(W, psi) -> float:
    """norm(W * psi) without the product (without amplitude, as `norm`)."""
    _require_operator(W, psi)
    v = C.c_double()
    L.check(L.lib.qil_apply_norm(W.handle, psi.handle, C.byref(v)))
    return v.value


def _distance(nphi2, npsi2, overlap):
    return float(np.sqrt(max(0.0, nphi2 + npsi2 - 2.0 * np.real(overlap))))


def distance(phi, psi) -> float:
    """||vec(phi) - vec(psi)||, amplitudes included, as sqrt(max(0, |phi|^2 + |psi|^2 - 2 Re<phi|psi>)).

    The expansion has a floor: the squared distance carries an absolute error of a few eps * (|phi|^2 + |psi|^2), so
    relative distances below about 1e-7 are not resolved (they come out as that floor or as 0)."""
    _require_mps(phi, "inner")
    _require_mps(psi, "inner")
    npsi = psi.amplitude * norm(psi)
    nphi = phi.amplitude * norm(phi)
    return _distance(nphi * nphi, npsi * npsi, inner(phi, psi))


def apply_distance(phi, W, psi) -> float:
    """||vec(phi) - vec(W psi)||, amplitudes included, without the product: sqrt(max(0, |phi|^2 + |W psi|^2 -
    2 Re<phi|W psi>)) from `norm`, `apply_norm` and `inner(phi, W, psi)`.

    The same floor as `distance`: the squared distance carries an absolute error of a few eps * (|phi|^2 + |W psi|^2),
    so relative distances below about 1e-7 are not resolved."""
    _require_mps(phi, "inner")
    _require_operator(W, psi)
    nphi = phi.amplitude * norm(phi)
    nwpsi = psi.amplitude * apply_norm(W, psi)
    return _distance(nphi * nphi, nwpsi * nwpsi, inner(phi, W, psi))


# ---------------------------------------------------------------- environments
ENV_SIDES = {"left": 0, "right": 1}              # QIL_ENV_LEFT / QIL_ENV_RIGHT (include/qilaplace_hip.h)
ENV_CHAIN_MAX_OP_BOND = 8                        # QIL_ENV_CHAIN_MAX_OP_BOND


def environment(phi, psi, W=None, side="right", count=None):
    """The partial contraction the overlap verbs carry and never return (qil_environment): `count` tensors of <phi|psi>, or of
    <phi|W|psi> with an operator, with the bond legs left open.  side="left" walks tensors 1 .. count and leaves the bonds to
    their right open, side="right" walks the last `count` tensors and leaves the bonds to their left open; count=None walks the
    whole chain.  For a ZTMPS `count` counts tensors of the interleaved 2n chain.

    Returns a complex128 array E[p, s] (p: the bond of phi, s: of psi), or E[p, a, s] with an operator (a: its bond).  The bra is
    conj(phi) and contracts the operator's output leg, as in inner(phi, W, psi).  The amplitudes are NOT applied (as in `norm`):
    count = all tensors gives inner(...) / (phi.amplitude * psi.amplitude), count = 0 gives [[1]]."""
    _require_mps(phi, "environment")
    _require_mps(psi, "environment")
    if W is not None:
        _require_operator(W, psi)
    if side not in ENV_SIDES:
        raise ValueError(f"environment: side must be 'left' or 'right', got {side!r}")
    n = _ntensors(psi)
    if count is None:
        count = n
    if isinstance(count, (bool, np.bool_)) or not isinstance(count, (int, np.integer)):
        raise TypeError(f"environment: count must be an integer, got {type(count).__name__}")
    if not 0 <= count <= n:
        raise ValueError(f"environment: count {int(count)} outside [0, {n}]")
    dims = (C.c_int64 * 3)()
    wh = None if W is None else W.handle
    L.check(L.lib.qil_environment(phi.handle, wh, psi.handle, ENV_SIDES[side], int(count), None, dims))
    out = np.zeros(tuple(dims), dtype=np.complex128, order="F")
    L.check(L.lib.qil_environment(phi.handle, wh, psi.handle, ENV_SIDES[side], int(count), out.ctypes.data_as(L._pdbl), dims))
    return out if W is not None else out[:, 0, :]


def environment_route(side, count, phi_dims, psi_dims, op_dims=None):
    """Which route an `environment` call takes (needs no GPU): qil_environment_route, the host function
    qil_environment switches on.  *_dims: the n + 1 bond dimensions, edges included.  Returns "CHAIN" or "GEMM"."""
    pd, sd = np.ascontiguousarray(phi_dims, dtype=np.int64), np.ascontiguousarray(psi_dims, dtype=np.int64)
    od = None if op_dims is None else np.ascontiguousarray(op_dims, dtype=np.int64)
    if pd.ndim != 1 or pd.size < 1 or sd.shape != pd.shape or (od is not None and od.shape != pd.shape):
        raise ValueError("environment_route: bond dimensions are n + 1 entries per chain")
    if side not in ENV_SIDES:
        raise ValueError(f"environment: side must be 'left' or 'right', got {side!r}")
    route = C.c_int()
    p64 = C.POINTER(C.c_int64)
    L.check(L.lib.qil_environment_route(ENV_SIDES[side], int(count), pd.size - 1, pd.ctypes.data_as(p64), sd.ctypes.data_as(p64),
                                        od.ctypes.data_as(p64) if od is not None else None, C.byref(route)))
    return "CHAIN" if route.value == 0 else "GEMM"


# ---------------------------------------------------------------- linear solver
def _solve_info(v):
    return {"sweeps": int(v[0]), "converged": bool(v[1]), "residual": float(v[2]), "matvecs": int(v[3]), "max_bond": int(v[4]),
            "local_solves": int(v[5]), "gemm_solves": int(v[6])}


def solve(A, c, x0=None, shift=0.0, maxdim=64, cutoff=1e-20, tol=1e-10, max_sweeps=6, cg_iters=100, return_info=False):
    """x with (A + shift I) x = c for a Hermitian positive definite A + shift I, as a new state of c's class, without a dense
    vector: the alternating two-site solver with a conjugate-gradient local solve (include/qilaplace_hip.h, qil_mps_solve).
    Hermiticity is the caller's promise and is not checked.  `x0` is the initial guess (default: c, compressed to `maxdim`);
    `cutoff` and `maxdim` truncate every two-site split by the project's rule; `tol` is both CG's relative residual and the
    stopping test of the sweeps (the largest local residual met before a local solve); `cg_iters` caps CG per bond.
    mps_to_vector(solve(A, c)) is the solution, amplitudes included.

    return_info=True also returns a dict: sweeps, converged, residual, matvecs, max_bond, local_solves, gemm_solves (how many
    local solves took the one-launch route and the GEMM route).  converged=False after max_sweeps is not an error: a truncation
    coarser than `tol` keeps the local residual above it.

    The verb is for solutions that compress.  With `maxdim` below the solution's rank and a right-hand side that does not
    compress (random), truncation by SVD does not converge to the best approximation at that rank: errors of 0.1 to 0.5 were
    seen in a numpy restatement."""
    _require_operator(A, c)
    if x0 is not None:
        _require_mps(x0, "solve")
    if isinstance(maxdim, (bool, np.bool_)) or (maxdim is not None and not isinstance(maxdim, (int, np.integer))):
        raise TypeError(f"solve: maxdim must be an integer, got {type(maxdim).__name__}")
    h = C.c_void_p()
    info = (C.c_double * 8)()
    L.check(L.lib.qil_mps_solve(A.handle, float(shift), c.handle, None if x0 is None else x0.handle, _maxdim(maxdim), float(cutoff),
                                float(tol), int(max_sweeps), int(cg_iters), C.byref(h), info))
    x = _wrap_like(c, h)
    return (x, _solve_info(info)) if return_info else x


def solve_local_fits(xl, xr, dl, dm, dr, cl, cm, cr, dtype=np.float64):
    """Whether the local solve of a bond takes the one-launch route (needs no GPU): qil_mps_solve_local_fits, the host function
    qil_mps_solve switches on.  xl, xr: the outer bonds of x at the two tensors; dl, dm, dr: the operator's bonds there;
    cl, cm, cr: the right-hand side's.  True where the kernel's operands fit 160 KiB of LDS and one matvec is at most 200 000
    multiply-adds (beyond that the GEMM route was measured faster; MEASUREMENTS.md section 30).  QIL_SOLVE_ROUTE=gemm makes it
    False, QIL_SOLVE_ROUTE=local drops the size rule and keeps the LDS one."""
    fits = C.c_int()
    L.check(L.lib.qil_mps_solve_local_fits(1 if np.dtype(dtype) == np.complex128 else 0, int(xl), int(xr), int(dl), int(dm), int(dr),
                                           int(cl), int(cm), int(cr), C.byref(fits)))
    return bool(fits.value)


def solve_residual(A, x, c, shift=0.0) -> float:
    """||(A + shift I) x - c|| / ||c||, amplitudes included, without the product: the expansion of the squared norm from
    `apply_norm`, `inner` and `norm`.

    The floor of `apply_distance`: the squared residual carries an absolute error of a few eps times the squared norms of its
    terms, so relative residuals below about 1e-7 are not resolved (they come out as that floor or as 0)."""
    _require_operator(A, x)
    _require_mps(c, "solve_residual")
    s = float(shift)
    nax = x.amplitude * apply_norm(A, x)
    nx = x.amplitude * norm(x)
    nc = c.amplitude * norm(c)
    r2 = nax * nax + nc * nc - 2.0 * np.real(inner(c, A, x))
    if s != 0.0:
        r2 += s * s * nx * nx + 2.0 * s * np.real(inner(x, A, x)) - 2.0 * s * np.real(inner(c, x))
    return float(np.sqrt(max(0.0, r2)) / nc)


def least_squares(W, b, reg=0.0, **solve_kwargs):
    """argmin_x ||W x - b||^2 + reg ||x||^2 by the normal equations (W^dagger W + reg I) x = W^dagger b, solved with `solve`: the
    operator is mpo_compress(apply(W, adjoint(W))) ("W first, then W^dagger"), the right-hand side apply(adjoint(W), b), the
    shift `reg`.  W need not be Hermitian or symmetric.  THE CONDITION NUMBER IS SQUARED: kappa(W^dagger W) = kappa(W)^2, so the
    attainable accuracy and CG's iteration count are those of the squared problem; `reg` > 0 bounds it by
    (|W|^2 + reg) / reg.  Keyword arguments go to `solve`."""
    _require_operator(W, b)
    A, Wd = _normal_operator(W)
    return solve(A, apply(Wd, b), shift=float(reg), **solve_kwargs)


def _normal_operator(W):
    """(W^dagger W, W^dagger) as least_squares and operator_norm form them: mpo_compress(apply(W, adjoint(W))), "W first, then
    W^dagger"; a single tensor has no bond to compress."""
    Wd = adjoint(W)
    A = apply(W, Wd)
    if _ntensors(W) > 1:
        A = mpo_compress(A)
    return A, Wd


def smooth(y, alpha, order=1, mask=None, **solve_kwargs):
    """The Whittaker smoother and gap filler: argmin_x ||M (x - y)||^2 + alpha ||Delta^order x||^2 with the periodic second
    difference L = Delta^T Delta = 2 I - S - S^dagger (build_laplacian_mpo), i.e. (M + alpha L^order) x = M y.  `mask` is a state
    of 0 / 1 weights (M = diagonal_mpo(mask), c = hadamard(mask, y)): samples with weight 0 are filled in from their neighbours.
    Without a mask M = I enters as shift = 1 and c = y.  Keyword arguments go to `solve`; with a mask the operator is only
    positive definite where the mask leaves no run of hidden samples that the null space of L^order (the constants) fits, which
    any mask with one visible sample satisfies."""
    from .builders import build_laplacian_mpo
    _require_mps(y, "smooth")
    if y._paired():
        raise TypeError("smooth: unsupported operand types (a SignalMPS is needed)")
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or order < 1:
        raise ValueError(f"smooth: order must be a positive integer, got {order!r}")
    if not float(alpha) >= 0.0:
        raise ValueError(f"smooth: alpha must be >= 0, got {alpha!r}")
    lap = build_laplacian_mpo(y)
    P = lap
    for _ in range(int(order) - 1):
        P = mpo_compress(apply(P, lap))
    if mask is None:
        return solve(mpo_scale(P, float(alpha)), y, shift=1.0, **solve_kwargs)
    _require_mps(mask, "smooth")
    A = mpo_linear_combination([diagonal_mpo(mask), P], [1.0, float(alpha)])
    return solve(A, hadamard(mask, y), **solve_kwargs)


# ---------------------------------------------------------------- extremal eigenpairs
EIGS_WHICH = {"smallest": 0, "largest": 1}
EIGS_MAX_ORTHO = 8


def _eigs_info(v):
    return {"sweeps": int(v[0]), "converged": bool(v[1]), "residual": float(v[2]), "matvecs": int(v[3]), "max_bond": int(v[4]),
            "local_solves": int(v[5]), "gemm_solves": int(v[6]), "scale": float(v[7])}


def _random_start(A, rng):
    """A random bond-2 state on A's sites, of A's kind (ZTMPS for a PairedSiteMPO), complex when A is."""
    n = _ntensors(A)
    cx = np.dtype(A.dtype) == np.complex128
    dims = [1] + [2] * (n - 1) + [1]
    data = []
    for i in range(n):
        shp = (dims[i], 2, dims[i + 1])
        t = rng.standard_normal(shp)
        if cx:
            t = t + 1j * rng.standard_normal(shp)
        data.append(t / np.sqrt(2.0 * dims[i]))
    return (ZTMPS if A.paired else SignalMPS)(data, sites=A.site_ids, ctx=A.ctx)


def eigs(A, k=1, which="smallest", x0=None, seed=0, ortho=(), weight=None, maxdim=64, cutoff=1e-20, tol=1e-10, max_sweeps=10,
         krylov=8, restarts=4, return_info=False):
    """The k smallest or largest (algebraic) eigenpairs of a Hermitian operator A as (values, states), without a dense object:
    two-site DMRG with a restarted Lanczos local solve (include/qilaplace_hip.h, qil_mps_eigs).  `values` is a float array, `states`
    a list of unit-norm states of amplitude 1 (their phase is not fixed).  It makes k calls, each deflated against `ortho` (unit
    states) plus the states found so far by a penalty `weight` that pushes them away from the wanted end; at most 8 deflation
    states in all.  `weight=None` uses 2 * scale of the first call, scale being the lower bound of |A|_2 that call returns (with a
    non-empty `ortho` the first call is deflated too, so scale then comes from one undeflated probe sweep before it): A
    GUESS THE CALLER MAY OVERRIDE -- it must exceed the distance from the wanted end to the k-th eigenvalue.  With deflation
    states a returned value is the Rayleigh quotient of the PENALISED operator, <x|A|x> + s * weight * sum_i |<phi_i|x>|^2: the
    last term is rounding-level for converged, well separated pairs; inner(x, A, x) is the plain quotient.  `x0` starts the first
    call; x0=None, and every later call, draws a random bond-2 state from np.random.default_rng(seed) (complex when A is), a fresh
    draw per call.  `cutoff` and `maxdim` truncate every two-site split; `tol` is the relative residual |A x - theta x| / scale of
    the local solves and of the stopping test of the sweeps; `krylov` (2 .. 16) and `restarts` bound the local Lanczos.

    return_info=True also returns a list of dicts, one per call: sweeps, converged, residual, matvecs, max_bond, local_solves,
    gemm_solves, scale.  converged=False after max_sweeps is not an error.

    THREE LIMITS.  Hermiticity is the caller's promise and is not checked.  The sweep converges to an eigenvector, not provably
    the extremal one: an eigenvector of small bond is a fixed point, and for circulant operators (shift, FIR, the periodic
    Laplacian) every Fourier mode is one -- a numpy restatement started from a random bond-2 state on I + 4 L at n = 8 stopped 9 %
    of |A| from lambda_min with a residual of 1e-13; for those operators the spectrum is top_k of the transfer function's
    magnitude.  Clustered ends converge slowly: the small end of a random Gram operator (relative gaps of 1e-8) did not converge
    in 10 sweeps in the restatement.  Check a result with eig_residual."""
    if not isinstance(A, SingleSiteMPO):
        raise TypeError("eigs: unsupported operand types (an operator is needed)")
    if which not in EIGS_WHICH:
        raise ValueError(f"eigs: which must be 'smallest' or 'largest', got {which!r}")
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"eigs: k must be a positive integer, got {k!r}")
    if isinstance(maxdim, (bool, np.bool_)) or (maxdim is not None and not isinstance(maxdim, (int, np.integer))):
        raise TypeError(f"eigs: maxdim must be an integer, got {type(maxdim).__name__}")
    found = list(ortho)
    for phi in found:
        _require_mps(phi, "eigs")
    if len(found) + int(k) - 1 > EIGS_MAX_ORTHO:
        raise ValueError(f"eigs: at most {EIGS_MAX_ORTHO} deflation states (got {len(found)} in ortho and k = {int(k)})")
    if x0 is not None:
        _require_operator(A, x0)
    rng = np.random.default_rng(seed)
    values, states, infos = [], [], []
    w = None if weight is None else float(weight)

    def call(start, deflate, penalty, sweeps, n_restarts):
        handles = (C.c_void_p * max(len(deflate), 1))(*[phi.handle for phi in deflate])
        h, theta, info = C.c_void_p(), C.c_double(), (C.c_double * 8)()
        L.check(L.lib.qil_mps_eigs(A.handle, EIGS_WHICH[which], start.handle, handles if deflate else None, len(deflate), penalty,
                                   _maxdim(maxdim), float(cutoff), float(tol), sweeps, int(krylov), n_restarts, C.byref(h),
                                   C.byref(theta), info))
        return _wrap_like(start, h), theta.value, info

    for j in range(int(k)):
        start = x0 if (j == 0 and x0 is not None) else _random_start(A, rng)
        if w is None and found:
            # deflation states and no weight yet: `scale` from ONE undeflated sweep of one restart per bond (its state is dropped)
            w = 2.0 * float(call(start, [], 0.0, 1, 1)[2][7])
        x, theta, info = call(start, found, 0.0 if w is None else w, int(max_sweeps), int(restarts))
        if w is None:
            w = 2.0 * float(info[7])
        values.append(theta)
        states.append(x)
        infos.append(_eigs_info(info))
        found.append(x)
    values = np.array(values, dtype=np.float64)
    return (values, states, infos) if return_info else (values, states)


def eigs_local_fits(xl, xr, dl, dm, dr, krylov=8, n_ortho=0, dtype=np.float64):
    """Whether the local eigen-solve of a bond takes the one-launch route (needs no GPU): qil_mps_eigs_local_fits, the host
    function qil_mps_eigs switches on.  xl, xr: the outer bonds of x at the two tensors; dl, dm, dr: the operator's bonds there;
    krylov, n_ortho: as in the call.  True where the kernel's operands fit 160 KiB of LDS and one matvec is at most 200 000
    multiply-adds (MEASUREMENTS.md).  QIL_EIGS_ROUTE=gemm makes it False, QIL_EIGS_ROUTE=local drops the size rule and keeps the
    LDS one."""
    fits = C.c_int()
    L.check(L.lib.qil_mps_eigs_local_fits(1 if np.dtype(dtype) == np.complex128 else 0, int(xl), int(xr), int(dl), int(dm), int(dr),
                                          int(krylov), int(n_ortho), C.byref(fits)))
    return bool(fits.value)


def eig_residual(A, x, theta) -> float:
    """||A x - theta x|| / ||x||, without the product: the expansion of the squared norm from `apply_norm`, `inner` and `norm`.

    The floor of `apply_distance`: the squared residual carries an absolute error of a few eps times the squared norms of its
    terms, so residuals below about 1e-7 * |theta| are not resolved (they come out as that floor or as 0)."""
    _require_operator(A, x)
    t = float(theta)
    nax = x.amplitude * apply_norm(A, x)
    nx = x.amplitude * norm(x)
    r2 = nax * nax - 2.0 * t * np.real(inner(x, A, x)) + t * t * nx * nx
    return float(np.sqrt(max(0.0, r2)) / nx)


def operator_norm(W, **eigs_kwargs):
    """The spectral norm |W|_2: the square root of the largest eigenvalue of W^dagger W, which is formed exactly as
    `least_squares` forms it and handed to `eigs` (keyword arguments go there).  W need not be Hermitian.  The value is a
    Rayleigh quotient, so it never exceeds |W|_2; the limits of `eigs` apply."""
    if not isinstance(W, SingleSiteMPO):
        raise TypeError("operator_norm: unsupported operand types (an operator is needed)")
    A, _ = _normal_operator(W)
    values, _ = eigs(A, 1, "largest", **eigs_kwargs)
    return float(np.sqrt(max(0.0, values[0])))


def condition_number(A, **eigs_kwargs):
    """theta_max / theta_min of a Hermitian positive definite A from two `eigs` calls (keyword arguments go there).  The value is
    always a LOWER bound of kappa: both Rayleigh quotients lie inside the spectrum.  The small end is the slow one: its relative
    gaps are the small ones, so look at return_info of eigs(A, which="smallest") before trusting it."""
    hi, _ = eigs(A, 1, "largest", **eigs_kwargs)
    lo, _ = eigs(A, 1, "smallest", **eigs_kwargs)
    return float(hi[0] / lo[0])


# ---------------------------------------------------------------- time evolution
DIFFUSE_MAX_STEPS = 4096


def _evolve_info(v):
    return {"steps": int(v[0]), "converged": bool(v[1]), "estimate": float(v[2]), "matvecs": int(v[3]), "max_bond": int(v[4]),
            "local_exps": int(v[5]), "gemm_exps": int(v[6]), "substeps": int(v[7]), "backward_growth": float(v[8]),
            "log_norm": float(v[9])}


def _positive_int(what, name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{what}: {name} must be a positive integer, got {v!r}")
    return int(v)


def evolve(A, x, t, steps=1, maxdim=64, cutoff=1e-20, tol=1e-10, krylov=8, substeps=4, return_info=False):
    """exp(t A) x for a Hermitian operator A as a new state of x's class, without a dense object: two-site TDVP, the
    projector-splitting integrator, with a Lanczos exponential as the local step (include/qilaplace_hip.h, qil_mps_evolve).
    `t` is the total, real or complex, taken in `steps` steps of tau = t / steps; the result is complex when A, x or t is.
    Hermiticity is the caller's promise and is not checked.  `cutoff` and `maxdim` truncate every two-site split; `tol` is the
    error estimate every local exponential must meet; `krylov` (2 .. 16) bounds its basis and `substeps` the passes it may take.
    mps_to_vector(evolve(A, x, t)) is the result, amplitudes included.

    return_info=True also returns a dict: steps, converged, estimate, matvecs, max_bond, local_exps, gemm_exps (how many local
    exponentials took the one-launch route and the GEMM route), substeps, backward_growth, log_norm.  converged=False is not an
    error.

    What the error is: with every bond of x at its full value the step is exact to tol per local exponential; an eigenvector of
    small bond and any state under a sum of one-site terms are evolved exactly.  A start narrower than the bonds it grows to costs
    first order in tau once.  The error with a binding maxdim is the projection error and does not fall with the step.

    THE STIFF LIMIT: the backward one-site step exp(-tau/2 H1) amplifies rounding by exp(|Re tau| / 2 * spread(A)) for
    Re tau < 0 (`backward_growth` reports the exponent met).  On the Laplacian (spread 4) tau = -2.5 is right to 6e-12 and
    tau = -20 in one step returns garbage.  Use evolve for |Re tau| * spread(A) of order one per step and for any imaginary tau;
    strong smoothing stays with `smooth` (implicit), and circulant operators have the Fourier route (`hadamard` with a transfer
    function)."""
    if not (isinstance(A, SingleSiteMPO) and isinstance(x, SignalMPS)):
        raise TypeError("evolve: unsupported operand types (an operator and a state are needed)")
    if A._paired() != x._paired():
        raise TypeError("evolve: PairedSiteMPO acts on ZTMPS, SingleSiteMPO on SignalMPS")
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, complex, np.number)):
        raise TypeError(f"evolve: t must be a real or complex number, got {type(t).__name__}")
    n_steps = _positive_int("evolve", "steps", steps)
    _positive_int("evolve", "krylov", krylov)
    _positive_int("evolve", "substeps", substeps)
    if isinstance(maxdim, (bool, np.bool_)) or (maxdim is not None and not isinstance(maxdim, (int, np.integer))):
        raise TypeError(f"evolve: maxdim must be an integer, got {type(maxdim).__name__}")
    tau = complex(t) / n_steps
    if not np.isfinite(tau) or tau == 0:
        raise ValueError(f"evolve: t must be finite and not zero, got {t!r}")
    h = C.c_void_p()
    info = (C.c_double * 10)()
    L.check(L.lib.qil_mps_evolve(A.handle, x.handle, tau.real, tau.imag, n_steps, _maxdim(maxdim), float(cutoff), float(tol),
                                 int(krylov), int(substeps), C.byref(h), info))
    y = _wrap_like(x, h)
    return (y, _evolve_info(info)) if return_info else y


def propagate(H, x, t, **evolve_kwargs):
    """exp(-i t H) x, the unitary propagation under a Hermitian H for a real time t: evolve(H, x, -1j * t).  Keyword arguments go
    to `evolve`; the norm is kept to the local tolerance and to what a binding maxdim projects away."""
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)):
        raise TypeError(f"evolve: propagate needs a real time t, got {type(t).__name__}")
    return evolve(H, x, -1j * float(t), **evolve_kwargs)


def diffuse(y, t, order=1, steps=None, **evolve_kwargs):
    """exp(-t L^order) y with the periodic second difference L = 2 I - S - S^dagger (build_laplacian_mpo): explicit diffusion for a
    time t >= 0.  The spectrum of L^order spans 4^order, so the default steps = ceil(t * 4^order / 8) keeps the backward growth
    exponent of THE STIFF LIMIT (see `evolve`) at or below 4 per step.  More than 4096 steps raise ValueError: that is strong
    smoothing, which is `smooth` (implicit) or the Fourier route.  Keyword arguments go to `evolve`."""
    from .builders import build_laplacian_mpo
    if not isinstance(y, SignalMPS) or y._paired():
        raise TypeError("evolve: diffuse: unsupported operand types (a SignalMPS is needed)")
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or order < 1:
        raise ValueError(f"evolve: diffuse: order must be a positive integer, got {order!r}")
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)) or not (0.0 < float(t) < np.inf):
        raise ValueError(f"evolve: diffuse: t must be a positive real number, got {t!r}")
    if steps is None:
        steps = max(1, int(np.ceil(float(t) * 4.0 ** int(order) / 8.0)))
        if steps > DIFFUSE_MAX_STEPS:
            raise ValueError(f"evolve: diffuse: t = {t!r} at order {int(order)} needs {steps} explicit steps (more than "
                             f"{DIFFUSE_MAX_STEPS}); this is strong smoothing: call smooth (implicit) or use the Fourier route")
    lap = build_laplacian_mpo(y)
    P = lap
    for _ in range(int(order) - 1):
        P = mpo_compress(apply(P, lap))
    return evolve(P, y, -float(t), steps=steps, **evolve_kwargs)


def evolve_local_fits(xl, xr, dl, dm, dr, sites=2, krylov=8, dtype=np.float64):
    """Whether a local exponential of `evolve` takes the one-launch route (needs no GPU): qil_mps_evolve_local_fits, the host
    function qil_mps_evolve switches on.  sites=2: xl, xr the outer bonds of x at the two tensors, dl, dm, dr the operator's bonds
    there; sites=1: the bonds at the one tensor, dm is ignored.  True where the kernel's operands fit 160 KiB of LDS and one matvec
    is at most 200 000 multiply-adds (MEASUREMENTS.md).  QIL_EVOLVE_ROUTE=gemm makes it False, QIL_EVOLVE_ROUTE=local drops the
    size rule and keeps the LDS one."""
    fits = C.c_int()
    L.check(L.lib.qil_mps_evolve_local_fits(1 if np.dtype(dtype) == np.complex128 else 0, int(sites), int(xl), int(xr), int(dl),
                                            int(dm), int(dr), int(krylov), C.byref(fits)))
    return bool(fits.value)


# ---------------------------------------------------------------- Schmidt spectra
def _spectra(entry, x, return_norm):
    dims = x.bond_dims
    out = np.zeros(max(1, sum(dims)), dtype=np.float64)
    nrm = C.c_double()
    L.check(entry(x.handle, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nrm)))
    spectra, at = [], 0
    for d in dims:
        spectra.append(out[at:at + d].copy())
        at += d
    return (spectra, nrm.value) if return_norm else spectra


def bond_spectra(psi, return_norm=False):
    """The Schmidt values of the normalised state at every bond: a list of N - 1 float64 arrays (tensor order, 2n - 1 for a
    ZTMPS), array k of length bond_dims[k], descending, squares summing to 1, exact zeros beyond what the cut can carry.
    Absolute accuracy, a modest multiple of N chi eps; tiny values carry no relative accuracy.  psi is not modified.
    return_norm=True adds ||psi|| without the amplitude, the number `norm` returns."""
    _require_mps(psi, "bond_spectra")
    return _spectra(L.lib.qil_bond_spectra, psi, return_norm)


def mpo_bond_spectra(W, return_norm=False):
    """The operator-Schmidt values of W / ||W||_F at every bond, as `bond_spectra`; return_norm=True adds ||W||_F."""
    if not isinstance(W, SingleSiteMPO):
        raise TypeError("mpo_bond_spectra: unsupported operand types")
    return _spectra(L.lib.qil_mpo_bond_spectra, W, return_norm)


def _as_spectra(x, what):
    """A handle's spectra, or a list of spectra as it is (the helpers below are pure numpy on top)."""
    if isinstance(x, SignalMPS):
        return bond_spectra(x)
    if isinstance(x, SingleSiteMPO):
        return mpo_bond_spectra(x)
    if isinstance(x, (list, tuple)):
        return [np.asarray(s, dtype=np.float64).reshape(-1) for s in x]
    raise TypeError(f"{what}: expected an MPS, an MPO or a list of spectra")


def entanglement_entropy(x, alpha=1.0, base=2.0):
    """One entropy per bond of the probabilities p = s^2 / sum(s^2): von Neumann -sum p log p at alpha = 1, Renyi
    log(sum p^alpha) / (1 - alpha) otherwise, in units of log(base).  Zero values contribute nothing."""
    alpha, base = float(alpha), float(base)
    if not (alpha > 0.0 and base > 0.0 and base != 1.0):
        raise ValueError("entanglement_entropy: needs alpha > 0 and a base > 0 other than 1")
    out = []
    for s in _as_spectra(x, "entanglement_entropy"):
        p = s * s
        tot = p.sum()
        p = p[p > 0.0] / tot if tot > 0.0 else p[:0]
        if p.size == 0:
            out.append(0.0)
        elif alpha == 1.0:
            out.append(float(-(p * np.log(p)).sum() / np.log(base)) + 0.0)
        else:
            out.append(float(np.log((p ** alpha).sum()) / (1.0 - alpha) / np.log(base)) + 0.0)
    return np.array(out, dtype=np.float64)


def _tail_weights(spectra, maxdim):
    """t_k = the squares beyond the first `maxdim` values of bond k, relative to the bond's total."""
    t = []
    for s in spectra:
        p = np.sort(s * s)[::-1]
        tot = p.sum()
        t.append(float(p[maxdim:].sum() / tot) if tot > 0.0 else 0.0)
    return np.array(t, dtype=np.float64)


def truncation_error_bounds(x, maxdim):
    """(lower, upper) for the distance of the state from its best bond-`maxdim` approximations, relative to ||psi||, with
    t_k the sum of squares beyond the first `maxdim` values of bond k: lower = sqrt(max_k t_k), the Eckart-Young bound at the
    worst cut, which no state of that bond dimension beats; upper = sqrt(sum_k t_k), what one truncating sweep stays below."""
    maxdim = int(maxdim)
    if maxdim < 1:
        raise ValueError("truncation_error_bounds: maxdim must be at least 1")
    t = _tail_weights(_as_spectra(x, "truncation_error_bounds"), maxdim)
    if t.size == 0:
        return 0.0, 0.0
    return float(np.sqrt(t.max())), float(np.sqrt(t.sum()))


def required_maxdim(x, tol):
    """The smallest maxdim whose `truncation_error_bounds` upper bound is <= tol."""
    spectra = _as_spectra(x, "required_maxdim")
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError("required_maxdim: tol must be non-negative")
    lo, hi = 1, max([1] + [len(s) for s in spectra])
    while lo < hi:                      # the upper bound does not increase with maxdim
        mid = (lo + hi) // 2
        if np.sqrt(_tail_weights(spectra, mid).sum()) <= tol:
            hi = mid
        else:
            lo = mid + 1
    return lo


# ---------------------------------------------------------------- sampling
def sample(psi, nsamples, seed=1234, uniforms=None, bits=False):
    """Perfect sampling: `nsamples` configurations x drawn with probability |psi_x|^2 / |psi|^2 (ITensors' sample), with
    those probabilities.  The amplitude does not enter.

    Sample r depends only on (psi, seed, r): with uniforms=None the draw at site i uses u = (splitmix64(seed ^
    splitmix64(r * n + i)) >> 11) * 2^-53 (n = number of site tensors); `uniforms` ((nsamples, n) in [0, 1)) replaces them.

    Returns (samples, probs).  SignalMPS: big-endian indices (site 1 = MSB), the integers `coefficient(psi, int)` reads.
    ZTMPS: a pair (k, l) decoded as `coefficient_grid` encodes it (lsb(k) on the main sites, lsb(l) on the copy sites).
    bits=True: the raw (nsamples, n) uint8 rows, the layout of `coefficient_batch` (required when n > 62)."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("sample: unsupported operand types")
    return _sample(L.lib.qil_sample, (psi,), nsamples, seed, uniforms, bits, check_uniforms=False)


def apply_sample(W, psi, nsamples, seed=1234, uniforms=None, bits=False):
    """Perfect sampling of W psi without the product (qil_apply_sample): `nsamples` configurations x drawn with probability
    |(W psi)_x|^2 / |W psi|^2, with those probabilities -- in exact arithmetic `sample(apply(W, psi), ...)`.  The amplitude does
    not enter.  `seed`, `uniforms` ((nsamples, n) in [0, 1), checked here before any native call) and the returned
    configurations are `sample`'s: big-endian indices for a SignalMPS, (k, l) for a ZTMPS, the raw (nsamples, n) uint8 rows with
    bits=True -- the rows `apply_coefficient_batch(W, psi, rows)` reads.

    The call keeps the right environments of |W psi|^2, 8 or 16 bytes times the sum of (chi_k D_k)^2 over the inner bonds,
    instead of the product; above 16 GiB it raises MemoryError with the bytes needed (QIL_APPLY_SAMPLE_RENV_BYTES raises the
    cap).  Where the product fits and the bonds are small, `sample(apply(W, psi), ...)` is faster (4x at the natural zT bonds of
    n = 20, MEASUREMENTS section 18); this call is for the operands whose product does not fit and breaks even near chi D = 2048."""
    _require_operator(W, psi)
    return _sample(L.lib.qil_apply_sample, (W, psi), nsamples, seed, uniforms, bits, check_uniforms=True)


def _sample(entry, operands, nsamples, seed, uniforms, bits, check_uniforms):
    """The argument checks, the native call and the decoding of `sample` and `apply_sample`; operands = (psi,) or (W, psi).  Only
    `apply_sample` checks the uniforms' range here; `sample` leaves that to the library, whose message names the offender."""
    psi = operands[-1]
    nb = int(nsamples)
    if nb < 0:
        raise ValueError("sample: nsamples must be non-negative")
    n = _ntensors(psi)
    paired = isinstance(psi, ZTMPS)
    if not bits and (n if not paired else n // 2) > 62:
        raise ValueError(f"sample: {n} sites do not fit an integer index; use bits=True")
    u_ptr = None
    if uniforms is not None:
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        if u.shape != (nb, n):
            raise ValueError(f"sample: uniforms must have shape ({nb}, {n}), got {u.shape}")
        if check_uniforms and u.size and not bool(np.all((u >= 0.0) & (u < 1.0))):
            raise ValueError("sample: uniform outside [0, 1)")
        u_ptr = u.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros((nb, n), dtype=np.uint8)
    probs = np.zeros(nb, dtype=np.float64)
    L.check(entry(*(x.handle for x in operands), nb, int(seed) & 0xFFFFFFFFFFFFFFFF, u_ptr, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                  probs.ctypes.data_as(C.POINTER(C.c_double))))
    return _decode_rows(out, paired, bits), probs


def _decode_rows(out, paired, bits):
    """(nb, n) bit rows -> the configurations `sample` and `top_k` return: the rows themselves (bits=True), (k, l) pairs for a
    ZTMPS (lsb(k) on the main sites, lsb(l) on the copy sites), big-endian indices (site 1 = MSB) otherwise."""
    if bits:
        return out
    n = out.shape[1]
    if paired:
        w = np.int64(1) << np.arange(n // 2, dtype=np.int64)
        return out[:, 0::2].astype(np.int64) @ w, out[:, 1::2].astype(np.int64) @ w
    w = np.int64(1) << np.arange(n - 1, -1, -1, dtype=np.int64)
    return out.astype(np.int64) @ w


# ---------------------------------------------------------------- top-k search
TOP_K_SLACK = 1e-10


def top_k(psi, k=1, beam=4096, bits=False):
    """The k configurations x with the largest |psi_x| (amplitude included), by a beam search over prefixes ranked by their
    marginal weight on the device (include/qilaplace_hip.h, qil_top_k).

    Returns (configs, values, bound, certified).  configs are decoded as `sample` decodes them (big-endian indices for a
    SignalMPS, (k, l) pairs for a ZTMPS, the raw (k, n) uint8 rows with bits=True).  values: descending |value|, the numbers
    `coefficient_batch` gives on those rows (float for a real state, complex otherwise).  bound: the square root of the largest
    prefix weight the search dropped, on the scale of the values; 0 when nothing was dropped.  certified: bound <
    |values[-1]| (1 - 1e-10), in which case the result is the exact top-k.  beam = 2**n_tensors (when it fits the cap
    documented in the header) never drops anything."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("top_k: unsupported operand types")
    return _top_k("top_k", L.lib.qil_top_k, (psi,), k, beam, bits)


def apply_top_k(W, psi, k=1, beam=4096, bits=False):
    """The k configurations x with the largest |(W psi)_x| (psi's amplitude included) without the product (qil_apply_top_k): in
    exact arithmetic `top_k(apply(W, psi), k, beam, bits)`, and the same return, (configs, values, bound, certified).  values are
    the numbers `apply_coefficient_batch(W, psi, rows)` gives on the rows found (float when both operands are real).

    The call keeps the right environments of |W psi|^2 that `apply_sample` keeps, under the same cap (16 GiB,
    QIL_APPLY_SAMPLE_RENV_BYTES), instead of the product; the beam is capped by the operands' bonds (the header has the
    formula).  Where the product fits and the bonds are a few hundred at most, `top_k(apply(W, psi))` is faster (3x to 5x at the
    natural zT bonds of n = 20); at chi D = 2048 this call is about 2x faster than forming the product and searching it
    (MEASUREMENTS section 19)."""
    _require_operator(W, psi)
    return _top_k("apply_top_k", L.lib.qil_apply_top_k, (W, psi), k, beam, bits)


def _top_k(what, entry, operands, k, beam, bits):
    """The argument checks, the native call and the decoding of `top_k` and `apply_top_k`; operands = (psi,) or (W, psi)."""
    psi = operands[-1]
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or isinstance(beam, bool) or not isinstance(beam, (int, np.integer)):
        raise TypeError(f"{what}: k and beam must be integers")
    k, beam = int(k), int(beam)
    if k < 0:
        raise ValueError(f"{what}: k must be non-negative")
    if beam < k:
        raise ValueError(f"{what}: beam ({beam}) must be at least k ({k})")
    n = _ntensors(psi)
    paired = isinstance(psi, ZTMPS)
    if n <= 62 and k > (1 << n):
        raise ValueError(f"{what}: k ({k}) exceeds the 2^{n} configurations")
    if not bits and (n if not paired else n // 2) > 62:
        raise ValueError(f"{what}: {n} sites do not fit an integer index; use bits=True")
    out = np.zeros((k, n), dtype=np.uint8)
    vals = np.zeros(k, dtype=np.complex128)
    bound = C.c_double(0.0)
    L.check(entry(*(x.handle for x in operands), k, beam, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                  vals.ctypes.data_as(C.POINTER(C.c_double)), C.byref(bound)))
    bound = float(bound.value)
    certified = k == 0 or bound < abs(vals[-1]) * (1.0 - TOP_K_SLACK)
    values = vals if any(x.dtype == np.complex128 for x in operands) else vals.real.copy()
    return _decode_rows(out, paired, bits), values, bound, bool(certified)


# ---------------------------------------------------------------- truncation
def _maxdim(m):
    return L.QIL_MAXDIM_NONE if m is None else int(m)


def canonicalize(psi, direction, center=None, cutoff=1e-12, maxdim=None):
    """canonicalize!(psi, direction; center, cutoff, maxdim) -- in place, returns psi."""
    if direction not in ("right", "left"):
        raise ValueError("Direction must be :right or :left")
    L.check(L.lib.qil_canonicalize(psi.handle, L.QIL_DIR_RIGHT if direction == "right" else L.QIL_DIR_LEFT,
                                   0 if center is None else int(center), float(cutoff), _maxdim(maxdim)))
    return psi


def compress(psi, maxdim=None, tol=1e-12, sweeps=1):
    """compress!(psi; maxdim, tol, sweeps) -- in place, returns psi."""
    L.check(L.lib.qil_compress(psi.handle, _maxdim(maxdim), float(tol), int(sweeps)))
    return psi


def mpo_compress(W, direction="down", cutoff=1e-14, maxdim=None):
    """zip_to_compress_mpo(W, direction; cutoff, maxdim) over the whole MPO (dt_transformer.jl:167-288) -- in
    place, returns W.  "down": exact gauge sweep left -> right, truncating sweep right -> left; "up": mirror."""
    if direction not in ("down", "up"):
        raise ValueError(f"zip_to_compress_mpo: unknown direction '{direction}'")
    L.check(L.lib.qil_mpo_compress(W.handle, 0 if direction == "down" else 1, float(cutoff), _maxdim(maxdim)))
    return W


def apply_compress_batch(Ws, psis, maxdim=None, tol=1e-12, sweeps=1, zip_maxdim=None):
    """apply_compress(W, psi) for every (W, psi) pair -- the (signal, damping value) items of a sweep -- concurrently on the
    context's streams.  `Ws` / `psis` may each be a single operand (used for every item) or a sequence; returns the list
    of results."""
    if hasattr(Ws, "handle"):
        Ws = [Ws] * (len(psis) if not hasattr(psis, "handle") else 1)
    if hasattr(psis, "handle"):
        psis = [psis] * len(Ws)
    Ws, psis = list(Ws), list(psis)
    if len(Ws) != len(psis):
        raise ValueError(f"apply_compress_batch: {len(Ws)} operators for {len(psis)} states")
    for W, psi in zip(Ws, psis):
        if W.paired != psi.paired:
            raise TypeError("apply: PairedSiteMPO acts on ZTMPS, SingleSiteMPO on SignalMPS")
    nb = len(Ws)
    _, wa = _handle_array(Ws)
    _, pa = _handle_array(psis)
    outs = (C.c_void_p * max(nb, 1))()
    L.check(L.lib.qil_apply_compress_batch(wa, pa, nb, _maxdim(maxdim), float(tol), int(sweeps),
                                           0 if zip_maxdim is None else int(zip_maxdim), outs))
    return [_wrap_like(psi, C.c_void_p(h)) for psi, h in zip(psis, outs[:nb])]


def _handle_array(items):
    items = list(items)
    arr = (C.c_void_p * max(len(items), 1))(*[it.handle.value if isinstance(it.handle, C.c_void_p) else it.handle
                                              for it in items])
    return items, arr


def compress_batch(psis, maxdim=None, tol=1e-12, sweeps=1):
    """compress!(psi; maxdim, tol, sweeps) for every MPS of `psis` (independent chains of one context, e.g. the signals
    of a sweep) -- in place, concurrently on the context's worker streams; returns the list."""
    items, arr = _handle_array(psis)
    L.check(L.lib.qil_compress_batch(arr, len(items), _maxdim(maxdim), float(tol), int(sweeps)))
    return items


def mpo_compress_batch(Ws, direction="down", cutoff=1e-14, maxdim=None):
    """zip_to_compress_mpo(W, direction; cutoff, maxdim) for every MPO of `Ws` (one per damping value of a sweep) -- in
    place, concurrently on the context's worker streams; returns the list."""
    if direction not in ("down", "up"):
        raise ValueError(f"zip_to_compress_mpo: unknown direction '{direction}'")
    items, arr = _handle_array(Ws)
    L.check(L.lib.qil_mpo_compress_batch(arr, len(items), 0 if direction == "down" else 1, float(cutoff), _maxdim(maxdim)))
    return items


def apply_compress(W, psi, maxdim=None, tol=1e-12, sweeps=1, zip_maxdim=None):
    """compress(apply(W, psi), maxdim, tol, sweeps) fused: a zip-up sweep that never writes the (D chi)^2
    product tensors, then the exact-gauge compress.  (The reference's `apply` ignores cutoff/maxdim, and so
    does `apply` here; this is the explicit truncating variant.)  As for every zip-up, the intermediate
    truncations are near-optimal for decaying spectra and can lose more than `compress(apply(W, psi))` -- the
    exact route -- on flat-spectrum (random) operands; `zip_maxdim` buys head-room."""
    if W.paired != psi.paired:
        raise TypeError("apply: PairedSiteMPO acts on ZTMPS, SingleSiteMPO on SignalMPS")
    h = C.c_void_p()
    L.check(L.lib.qil_apply_compress(W.handle, psi.handle, _maxdim(maxdim), float(tol), int(sweeps),
                                     0 if zip_maxdim is None else int(zip_maxdim), C.byref(h)))
    return _wrap_like(psi, h)


# ---------------------------------------------------------------- element-wise products, adjoints
def _require_pair(phi, psi, what):
    """Two states, checked before any native call (register kind, length and sites are checked natively, as for `inner`)."""
    if not (isinstance(phi, SignalMPS) and isinstance(psi, SignalMPS)):
        raise TypeError(f"{what}: unsupported operand types")


def hadamard(phi, psi, conj=False):
    """The element-wise product out_x = phi_x * psi_x (conj=True: conj(phi_x) * psi_x) as a new state of psi's class: bonds
    chi_phi * chi_psi, amplitude amp_phi * amp_psi, nothing truncated.  The same tensors as apply(diagonal_mpo(phi), psi),
    from a kernel of its own (include/qilaplace_hip.h, qil_hadamard)."""
    _require_pair(phi, psi, "hadamard")
    h = C.c_void_p()
    L.check(L.lib.qil_hadamard(phi.handle, 1 if conj else 0, psi.handle, C.byref(h)))
    return _wrap_like(psi, h)


def hadamard_compress(phi, psi, conj=False, maxdim=None, tol=1e-12, sweeps=1, zip_maxdim=None):
    """compress(hadamard(phi, psi, conj), maxdim, tol, sweeps) without the (chi_phi chi_psi)^2 product tensors: bit-identical
    to apply_compress(diagonal_mpo(phi, conj), psi, ...), the diagonal operator being a temporary of the call."""
    _require_pair(phi, psi, "hadamard")
    h = C.c_void_p()
    L.check(L.lib.qil_hadamard_compress(phi.handle, 1 if conj else 0, psi.handle, _maxdim(maxdim), float(tol), int(sweeps),
                                        0 if zip_maxdim is None else int(zip_maxdim), C.byref(h)))
    return _wrap_like(psi, h)


def diagonal_mpo(phi, conj=False):
    """diag(phi) (conj=True: diag(conj(phi))) as an operator on phi's sites -- a PairedSiteMPO for a ZTMPS -- with the
    amplitude folded into the first tensor.  Every verb that takes an operator then reads phi (.) psi without forming it:
    apply_coefficient_batch, inner(chi, W, psi), apply_norm, apply_compress."""
    if not isinstance(phi, SignalMPS):
        raise TypeError("diagonal_mpo: unsupported operand types")
    h = C.c_void_p()
    L.check(L.lib.qil_mpo_diagonal(phi.handle, 1 if conj else 0, C.byref(h)))
    return (PairedSiteMPO if phi._paired() else SingleSiteMPO)(ctx=phi.ctx, _handle=h)


def adjoint(W):
    """W^dagger, in the container class of W; exact (moves and sign flips).  adjoint(build_qft_mpo(n)) is the inverse QFT."""
    if not isinstance(W, SingleSiteMPO):
        raise TypeError("adjoint: unsupported operand types")
    h = C.c_void_p()
    L.check(L.lib.qil_mpo_adjoint(W.handle, C.byref(h)))
    return type(W)(ctx=W.ctx, _handle=h)


def _spectral_operands(x, h, F, what):
    """The operand checks of the spectral verbs and the transform they use: `F`, or build_qft_mpo(x)."""
    if not (isinstance(x, SignalMPS) and isinstance(h, SignalMPS)) or x._paired() or h._paired():
        raise TypeError(f"{what}: unsupported operand types")
    if F is not None and not (isinstance(F, SingleSiteMPO) and not F._paired()):
        raise TypeError(f"{what}: unsupported operand types")
    if len(x) != len(h):
        raise ValueError(f"{what}: signals must have the same number of sites. Found {len(x)} and {len(h)}")
    if F is None:
        from .builders import build_qft_mpo
        F = build_qft_mpo(x)
    return F


def _spectral_product(x, h, F, maxdim, tol, conj, what):
    F = _spectral_operands(x, h, F, what)
    X = apply_compress(F, x, maxdim=maxdim, tol=tol)
    H = apply_compress(F, h, maxdim=maxdim, tol=tol)
    P = hadamard_compress(X, H, conj=conj, maxdim=maxdim, tol=tol)
    y = apply_compress(adjoint(F), P, maxdim=maxdim, tol=tol)
    y.amplitude = y.amplitude * float(np.sqrt(2.0) ** len(x))
    return y


def convolve(x, h, F=None, maxdim=None, tol=1e-12):
    """Circular convolution y[m] = sum_j x[j] h[(m - j) mod N] of two SignalMPS of n sites (N = 2^n samples), in MPS form on
    the device by the convolution theorem: y = sqrt(N) F^dagger((F x) (.) (F h)).  `F` defaults to build_qft_mpo(x); its
    bit reversal cancels between F and F^dagger.  The four stages (F x, F h, the product, F^dagger) each go through
    apply_compress / hadamard_compress with `maxdim` and `tol`; the sqrt(N) goes into the amplitude.

    The QFT MPO at its default cutoff 1e-14 is unitary only to 3e-9 (n = 6) ... 3e-7 (n = 10) -- the cutoff acts on squared
    singular values -- so the result matches np.fft.ifft(fft(x) * fft(h)) to about 1e-7 of max|y|, whatever `tol` is.  Pass
    F = build_qft_mpo(x, cutoff=...) with a tighter cutoff for a tighter result."""
    return _spectral_product(x, h, F, maxdim, tol, False, "convolve")


def correlate(x, h, F=None, maxdim=None, tol=1e-12):
    """Circular cross-correlation y[m] = sum_j conj(x[j]) h[(j + m) mod N] = sqrt(N) F^dagger(conj(F x) (.) (F h)): the route,
    the stages and the 1e-7-grade accuracy of `convolve` (see there for the unitarity of the default QFT MPO)."""
    return _spectral_product(x, h, F, maxdim, tol, True, "correlate")


def power_spectrum(psi, maxdim=None, tol=1e-12, sweeps=1, zip_maxdim=None):
    """|psi_x|^2 as a state: hadamard_compress(psi, psi, conj=True, ...).  Band energies are its partial sums:
    marginal_batch with bit value 2 on the summed sites."""
    return hadamard_compress(psi, psi, conj=True, maxdim=maxdim, tol=tol, sweeps=sweeps, zip_maxdim=zip_maxdim)


# ---------------------------------------------------------------- linear combinations
def _require_terms(terms, coeffs, what="linear_combination", cls=SignalMPS, names=("SignalMPS", "ZTMPS")):
    """A non-empty sequence of states (or, with cls = SingleSiteMPO, operators) of one register kind and their coefficients as
    nb x (re, im) doubles (None: all ones), checked before any native call (context, length and sites are checked natively, as
    for `hadamard`)."""
    single, paired = names
    if isinstance(terms, cls) or not isinstance(terms, (list, tuple)):
        raise TypeError(f"{what}: unsupported operand types (expected a list of {single} / {paired})")
    terms = list(terms)
    if not terms or not all(isinstance(t, cls) for t in terms):
        raise TypeError(f"{what}: unsupported operand types (expected a non-empty list of {single} / {paired})")
    if any(t._paired() != terms[0]._paired() for t in terms):
        raise TypeError(f"{what}: unsupported operand types ({paired} combines only with {paired})")
    if coeffs is None:
        return terms, None
    try:
        c = np.asarray(coeffs, dtype=np.complex128).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: unsupported operand types (coefficients must be numbers)") from None
    if c.size != len(terms):
        raise ValueError(f"{what}: {c.size} coefficients for {len(terms)} terms")
    return terms, np.ascontiguousarray(c).view(np.float64)


def linear_combination(terms, coeffs=None):
    """sum_j coeffs[j] * terms[j] as a new state of terms[0]'s class, materialised as the direct sum of the chains: every bond
    is the sum of the terms' bonds, nothing is truncated, the amplitude is 1 (weights and amplitudes sit in the first tensor).
    `coeffs` may be complex (the result is then complex); None means all ones.  Terms may repeat.  One grouped launch
    (include/qilaplace_hip.h, qil_mps_sum)."""
    terms, c = _require_terms(terms, coeffs)
    _, arr = _handle_array(terms)
    h = C.c_void_p()
    L.check(L.lib.qil_mps_sum(arr, len(terms), None if c is None else c.ctypes.data_as(L._pdbl), C.byref(h)))
    return _wrap_like(terms[0], h)


def linear_combination_compress(terms, coeffs=None, maxdim=None, tol=1e-12, sweeps=1, zip_maxdim=None):
    """compress(linear_combination(terms, coeffs), maxdim, tol, sweeps) without the direct-sum tensors of size (sum chi)^2: the
    terms are gauged, a zip-up sweep and one variational sweep build the sum at bond <= zip_maxdim (default maxdim + 16), then
    the exact-gauge compress runs (include/qilaplace_hip.h, qil_mps_sum_compress).  Same bonds as the exact route and at most
    twice its truncation error on random operands.  What it saves is the (sum chi)^2 tensors and SVDs of that size, so it pays
    when sum(chi) is well above `maxdim`; without `maxdim` (or with sum(chi) <= maxdim + 16) it is the exact route in stacked
    form and costs what linear_combination + compress costs.  MEASUREMENTS.md section 10 has the timings that exist."""
    terms, c = _require_terms(terms, coeffs)
    _, arr = _handle_array(terms)
    h = C.c_void_p()
    L.check(L.lib.qil_mps_sum_compress(arr, len(terms), None if c is None else c.ctypes.data_as(L._pdbl), _maxdim(maxdim),
                                       float(tol), int(sweeps), 0 if zip_maxdim is None else int(zip_maxdim), C.byref(h)))
    return _wrap_like(terms[0], h)


def add(phi, psi):
    """phi + psi (linear_combination of the two with unit coefficients)."""
    return linear_combination([phi, psi], [1.0, 1.0])


def sub(phi, psi):
    """phi - psi."""
    return linear_combination([phi, psi], [1.0, -1.0])


def scale(psi, c):
    """c * psi as a new state: a real `c` gives a copy with its amplitude scaled, a complex one the one-term sum."""
    _require_terms([psi], None)
    if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, float, complex, np.number)):
        raise TypeError("linear_combination: unsupported operand types (the factor must be a number)")
    if np.imag(c) == 0:
        out = psi.copy()
        out.amplitude = psi.amplitude * float(np.real(c))
        return out
    return linear_combination([psi], [c])


# ---------------------------------------------------------------- operator algebra
def _require_mpo(W, what):
    if not isinstance(W, SingleSiteMPO):
        raise TypeError(f"{what}: unsupported operand types")


def _require_mpo_terms(terms, coeffs):
    """`_require_terms` for operators."""
    return _require_terms(terms, coeffs, "mpo_linear_combination", SingleSiteMPO, ("SingleSiteMPO", "PairedSiteMPO"))


def _is_number(c):
    return not isinstance(c, (bool, np.bool_)) and isinstance(c, (int, float, complex, np.number))


def mpo_linear_combination(terms, coeffs=None):
    """sum_j coeffs[j] * terms[j] as a new operator of terms[0]'s class, materialised as the direct sum of the chains: every
    bond is the sum of the terms' bonds, nothing is truncated, the weights sit in the first tensor (MPOs carry no amplitude).
    `coeffs` may be complex (the result is then complex); None means all ones.  Terms may repeat.  One grouped launch of the
    kernel of `linear_combination` (include/qilaplace_hip.h, qil_mpo_sum)."""
    terms, c = _require_mpo_terms(terms, coeffs)
    _, arr = _handle_array(terms)
    h = C.c_void_p()
    L.check(L.lib.qil_mpo_sum(arr, len(terms), None if c is None else c.ctypes.data_as(L._pdbl), C.byref(h)))
    return type(terms[0])(ctx=terms[0].ctx, _handle=h)


def mpo_linear_combination_compress(terms, coeffs=None, direction="down", cutoff=1e-14, maxdim=None):
    """mpo_compress(mpo_linear_combination(terms, coeffs), direction, cutoff, maxdim).  A plain composition of the two: the
    direct-sum tensors are formed, then compressed (there is no fused route for operators)."""
    return mpo_compress(mpo_linear_combination(terms, coeffs), direction=direction, cutoff=cutoff, maxdim=maxdim)


def mpo_add(V, W):
    """V + W (mpo_linear_combination of the two with unit coefficients)."""
    return mpo_linear_combination([V, W], [1.0, 1.0])


def mpo_sub(V, W):
    """V - W."""
    return mpo_linear_combination([V, W], [1.0, -1.0])


def mpo_scale(W, c):
    """c * W as a new operator: the one-term sum (MPOs have no amplitude to scale and no clone entry)."""
    _require_mpo_terms([W], None)
    if not _is_number(c):
        raise TypeError("mpo_linear_combination: unsupported operand types (the factor must be a number)")
    return mpo_linear_combination([W], [c])


def _mpo_add(self, other):
    if not isinstance(other, SingleSiteMPO) or self._paired() != other._paired():
        return NotImplemented
    return mpo_add(self, other)


def _mpo_sub(self, other):
    if not isinstance(other, SingleSiteMPO) or self._paired() != other._paired():
        return NotImplemented
    return mpo_sub(self, other)


def _mpo_neg(self):
    return mpo_scale(self, -1.0)


def _mpo_rmul(self, c):
    return mpo_scale(self, c) if _is_number(c) else NotImplemented


# V + W, V - W, -W, c * W (numbers only, from the left); W * x stays the application (W * psi, W1 * W2)
SingleSiteMPO.__add__ = _mpo_add
SingleSiteMPO.__sub__ = _mpo_sub
SingleSiteMPO.__neg__ = _mpo_neg
SingleSiteMPO.__rmul__ = _mpo_rmul


def _require_mpo_pair(V, W):
    """Two operators, checked before any native call (register kind, context, length and sites are checked natively, as for
    `inner`)."""
    _require_mpo(V, "mpo_inner")
    _require_mpo(W, "mpo_inner")


def mpo_inner(V, W):
    """The Frobenius overlap <V, W>_F = tr(V^dagger W) = sum_{x,y} conj(V[x,y]) W[x,y] of two operators of one class, without
    a dense operator (include/qilaplace_hip.h, qil_mpo_inner).  float when both operands are real, complex otherwise."""
    _require_mpo_pair(V, W)
    v = (C.c_double * 2)()
    L.check(L.lib.qil_mpo_inner(V.handle, W.handle, v))
    return _scalar(v, V, W)


def mpo_norm(W) -> float:
    """The Frobenius norm ||W||_F = sqrt(Re <W, W>_F)."""
    return float(np.sqrt(max(0.0, np.real(mpo_inner(W, W)))))


def mpo_distance(V, W) -> float:
    """||V - W||_F as sqrt(max(0, ||V||^2 + ||W||^2 - 2 Re<V, W>)), without the difference.

    The same floor as `distance`: the squared distance carries an absolute error of a few eps * (||V||^2 + ||W||^2), so
    relative distances below about 1e-7 are not resolved (they come out as that floor or as 0)."""
    _require_mpo_pair(V, W)
    return _distance(float(np.real(mpo_inner(V, V))), float(np.real(mpo_inner(W, W))), mpo_inner(V, W))


def mpo_trace(W):
    """tr W = <I, W>_F, with the identity of W's class on W's sites and context."""
    _require_mpo(W, "mpo_trace")
    eye = type(W).identity(len(W), sites=W.site_ids, ctx=W.ctx)
    return mpo_inner(eye, W)


# ---------------------------------------------------------------- operator read-outs
TIE, DIAG = 4, 5          # both legs of a site tied: traced (mpo_entry_batch, mpo_slice) / its diagonal kept (mpo_slice)


def _mpo_spec(W, spec, what, ndim):
    """A spec of `W` as contiguous uint8 ([nb,] n_tensors, 2), checked for shape, range 0 .. 5 and whole ties."""
    _require_mpo(W, what)
    n = _ntensors(W)
    sp = np.asarray(spec)
    if sp.ndim != ndim or sp.shape[-2:] != (n, 2):
        raise ValueError(f"{what}: expected {n} x 2 entries, got {sp.shape}")
    if sp.dtype.kind not in "iub":
        raise TypeError(f"{what}: the spec must hold integers")
    if sp.size and (sp.min() < 0 or sp.max() > DIAG):
        bad = int(sp[(sp < 0) | (sp > DIAG)][0])
        raise ValueError(f"{what}: spec value {bad} outside [0,5]")
    tied = sp >= TIE
    if np.any(tied[..., 0] != tied[..., 1]) or np.any((sp[..., 0] != sp[..., 1]) & tied[..., 0]):
        raise ValueError(f"{what}: 4 (TIE) and 5 (DIAG) must stand in both bytes of a site")
    return np.ascontiguousarray(sp, dtype=np.uint8)


def mpo_entry_batch(W, spec):
    """One number per row of `spec` (nb, n_tensors, 2), read on the operator's own bonds (qil_mpo_entry_batch): per tensor the
    pair (in, out) for the legs of W_i[a, s_in, s_out, b], FIX0 / FIX1 fixes the leg's bit, SUM sums it, (TIE, TIE) traces the
    site.  All-fixed rows are the entries W[in, out]; SUM gives row sums, column sums and the sum of all entries; TIE partial
    traces and the trace.  float for a real operator, complex otherwise."""
    sp = _mpo_spec(W, spec, "mpo_entry_batch", 3)
    if sp.size and np.any((sp == FREE) | (sp == DIAG)):
        raise ValueError("mpo_entry_batch: a kept leg (3) or a kept diagonal (5) makes no number; mpo_slice returns that state")
    nb = sp.shape[0]
    out = np.zeros(nb, dtype=np.complex128)
    L.check(L.lib.qil_mpo_entry_batch(W.handle, nb, sp.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(L._pdbl)))
    return out if W.dtype == np.complex128 else out.real.copy()


def mpo_slice(W, spec):
    """The part of `W` that agrees with `spec` (n_tensors, 2), as a state (qil_mpo_slice): per tensor (in, out); a site keeps
    exactly one leg (FREE in one byte, or (DIAG, DIAG) for its diagonal) or none (FIX0 / FIX1 / SUM per leg, (TIE, TIE) traced);
    removed sites are absorbed into their kept neighbours as in `restrict`.  The result has W's dtype, amplitude 1, the kept
    sites' ids and no bond larger than the parent's; a ZTMPS when W is paired and whole (main_i, copy_i) pairs are kept, a
    SignalMPS otherwise.  A spec that keeps no site is a number: `mpo_entry_batch` returns it."""
    sp = _mpo_spec(W, spec, "mpo_slice", 2)
    if np.any((sp[:, 0] == FREE) & (sp[:, 1] == FREE)):
        raise ValueError("mpo_slice: a site (3, 3) keeps both legs: sub-operators are not built")
    if not np.any((sp == FREE) | (sp == DIAG)):
        raise ValueError("mpo_slice: the spec keeps no site; that number is what mpo_entry_batch returns")
    h = C.c_void_p()
    L.check(L.lib.qil_mpo_slice(W.handle, sp.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(h)))
    paired = C.c_int()
    status = L.lib.qil_mps_is_paired(h, C.byref(paired))
    if status != L.QIL_OK:                                # no container owns the handle yet
        L.lib.qil_mps_destroy(h)
        L.check(status)
    return (ZTMPS if paired.value else SignalMPS)(ctx=W.ctx, _handle=h)


def _mpo_config(W, cfg, what):
    """One configuration of W's n_tensors legs as bits, in any form `_parse_config` takes."""
    n = _ntensors(W)
    bits = _parse_config(cfg, n)
    if len(bits) != n:
        raise ValueError(f"{what}: expected {n} entries, got {len(bits)}")
    if any(b not in (0, 1) for b in bits):
        raise ValueError(f"{what}: bit value outside [0,1]")
    return np.asarray(bits, dtype=np.uint8)


def _mpo_configs(W, cfgs, what):
    """Configurations as an (m, n_tensors) bit array: an integer array (site 1 the most significant bit, as a single integer
    configuration) or a sequence of configurations."""
    n = _ntensors(W)
    if isinstance(cfgs, (str, int, np.integer)):
        cfgs = [cfgs]
    a = cfgs if isinstance(cfgs, np.ndarray) else None
    if a is not None and a.dtype.kind in "iu" and a.ndim == 1 and n <= 62:
        if a.size and (a.min() < 0 or int(a.max()) >> n):
            raise ValueError(f"{what}: index outside [0, 2^{n})")
        return _msb_bits(a, n)
    if a is not None and a.dtype.kind in "iu" and a.ndim == 2:
        if a.shape[1] != n:
            raise ValueError(f"{what}: expected {n} entries, got {a.shape[1]}")
        if a.size and (a.min() < 0 or a.max() > 1):
            raise ValueError(f"{what}: bit value outside [0,1]")
        return a.astype(np.uint8)
    return np.array([_mpo_config(W, c, what) for c in cfgs], dtype=np.uint8).reshape(-1, n)


def mpo_entries(W, ins, outs):
    """M[in, out] for every (in, out) of `ins` x `outs`, as a (len(ins), len(outs)) array in the convention of the dense
    operator (out[o] = sum_in M[in, o] psi[in], site 1 the most significant bit): one `mpo_entry_batch` call.  Configurations
    come in any form `coefficient` takes, or as integer arrays."""
    _require_mpo(W, "mpo_entries")
    bi, bo = _mpo_configs(W, ins, "mpo_entries"), _mpo_configs(W, outs, "mpo_entries")
    n = _ntensors(W)
    spec = np.empty((len(bi), len(bo), n, 2), dtype=np.uint8)
    spec[..., 0] = bi[:, None, :]
    spec[..., 1] = bo[None, :, :]
    return mpo_entry_batch(W, spec.reshape(-1, n, 2)).reshape(len(bi), len(bo))


def mpo_entry(W, i, o):
    """The entry M[i, o] of the operator: (W psi)[o] = sum_i M[i, o] psi[i]."""
    _require_mpo(W, "mpo_entry")
    n = _ntensors(W)
    spec = np.stack([_mpo_config(W, i, "mpo_entry"), _mpo_config(W, o, "mpo_entry")], axis=-1)
    return mpo_entry_batch(W, spec.reshape(1, n, 2))[0]


def mpo_to_matrix(W):
    """The dense 2^n x 2^n matrix M[in, out] of an operator of at most 12 tensors: all 4^n entries through mpo_entry_batch."""
    _require_mpo(W, "mpo_to_matrix")
    n = _ntensors(W)
    if n > 12:
        raise ValueError(f"mpo_to_matrix: {n} tensors make 4^{n} entries; the dense form stops at 12 tensors")
    idx = np.arange(2 ** n)
    return mpo_entries(W, idx, idx)


def _leg_spec(W, what, fixed_leg, value):
    """(n_tensors, 2) spec with leg `fixed_leg` (0 = in, 1 = out) set to the bits of configuration `value` (or to SUM where
    value is None) and the other leg kept"""
    _require_mpo(W, what)
    n = _ntensors(W)
    spec = np.full((n, 2), FREE, dtype=np.uint8)
    spec[:, fixed_leg] = SUM if value is None else _mpo_config(W, value, what)
    return spec


def mpo_column(W, cfg):
    """W applied to the basis state `cfg`, as a state: the input legs fixed, the output legs kept.  In exact arithmetic
    apply(W, basis state), at the operator's own bonds."""
    return mpo_slice(W, _leg_spec(W, "mpo_column", 0, cfg))


def mpo_row(W, cfg):
    """The state r with r_j = M[j, cfg], so that (W psi)_cfg = sum_j r_j psi_j: the output legs fixed, the input legs kept.  The
    functional that produces one transform value, usable as a matched filter against any number of signals."""
    return mpo_slice(W, _leg_spec(W, "mpo_row", 1, cfg))


def mpo_diagonal_state(W):
    """The diagonal M[j, j] as a state (every site (DIAG, DIAG)): the inverse of `diagonal_mpo`."""
    _require_mpo(W, "mpo_diagonal_state")
    return mpo_slice(W, np.full((_ntensors(W), 2), DIAG, dtype=np.uint8))


def mpo_column_sums(W):
    """W applied to the all-ones signal, as a state: s_o = sum_j M[j, o]."""
    return mpo_slice(W, _leg_spec(W, "mpo_column_sums", 0, None))


def mpo_row_sums(W):
    """The state s with s_j = sum_o M[j, o]: the sum of all output values as a functional of the input."""
    return mpo_slice(W, _leg_spec(W, "mpo_row_sums", 1, None))


def _dyadic_powers(z, n):
    """z^(2^k), k = 0 .. n-1, each correctly rounded to double: repeated squaring in 256-bit fixed point with a running binary
    exponent (squaring in double loses a bit per step: 2^39 eps = 6e-5 at n = 40).  Overflow gives inf, underflow 0."""
    import math
    z = complex(z)
    if not (math.isfinite(z.real) and math.isfinite(z.imag)):
        raise ValueError("exponential_mps: z must be finite")
    (mr, er), (mi, ei) = math.frexp(z.real), math.frexp(z.imag)
    ex = min(er, ei) - 53
    re, im = int(math.ldexp(mr, 53)) << (er - 53 - ex), int(math.ldexp(mi, 53)) << (ei - 53 - ex)
    out = []

    def to_float(v, e2):
        try:
            return math.ldexp(float(v), e2)
        except OverflowError:
            return math.copysign(math.inf, v)

    for _ in range(n):
        out.append(complex(to_float(re, ex), to_float(im, ex)))
        re, im, ex = re * re - im * im, 2 * re * im, 2 * ex
        sh = max(re.bit_length(), im.bit_length()) - 256
        if sh > 0:
            re, im, ex = re >> sh, im >> sh, ex + sh
        ex = max(min(ex, 1 << 40), -(1 << 40))               # far outside double's range either way: keep the integers small
    return out


def exponential_tensors(z, n):
    """(Public because it is the part of `exponential_mps` that needs no device: callers that only want the tensors -- to save
    them, or to check them on a machine without a GPU -- get them here.)  Host tensors of the bond-1 state x_j = z^j, j < 2^n (site 1 = most significant bit): site i holds [1, z^(2^(n-i))].
    complex128 unless z is real."""
    n = int(n)
    if n < 1:
        raise ValueError("exponential_mps: n must be >= 1")
    pw = _dyadic_powers(z, n)
    real = np.imag(z) == 0
    data = []
    for i in range(1, n + 1):
        A = np.ones((1, 2, 1), dtype=np.float64 if real else np.complex128)
        A[0, 1, 0] = pw[n - i].real if real else pw[n - i]
        data.append(A)
    return data


def exponential_mps(z, n, amplitude=1.0, ctx=None):
    """The complex exponential x_j = amplitude * z^j, j < 2^n, as an exact SignalMPS of bond 1, built on the host from n numbers
    (no dense vector).  complex128 unless z is real."""
    return SignalMPS(exponential_tensors(z, n), amplitude=float(amplitude), ctx=ctx)


def exponential_sum(amps, zs, n, maxdim=None, tol=1e-12):
    """x_j = sum_k amps[k] * zs[k]^j, j < 2^n, as a SignalMPS of bond <= K without touching 2^n numbers: the K bond-1 states of
    `exponential_mps` summed by linear_combination_compress(maxdim, tol) -- or by linear_combination, untruncated at bond K,
    when both `maxdim` and `tol` are None.

    A mode with |z| > 1 overflows for large n (z^(2^(n-1)) leaves double's range near |z|^(2^n) > 1e308), one with |z| < 1
    underflows to zero in its upper sites, which is then the value of those samples.  A real damped sinusoid
    A exp(-g j) cos(w j + p) is TWO conjugate modes: z = exp(-g +- i w) with amps (A / 2) exp(+- i p); the result is complex
    with an imaginary part at rounding level.

    The truncating route is `compress`: its gauge pass drops whatever carries less than 1e-12 of the squared norm, so a mode
    that decays within a few samples of a long record (weight ~ 2^-n of the rest) is truncated away; keep such modes with
    maxdim=None, tol=None."""
    zs = list(np.atleast_1d(zs))
    amps = list(np.atleast_1d(amps))
    if len(zs) != len(amps) or not zs:
        raise ValueError(f"exponential_sum: {len(amps)} amplitudes for {len(zs)} modes")
    terms = [exponential_mps(z, n) for z in zs]
    if maxdim is None and tol is None:
        return linear_combination(terms, amps)
    return linear_combination_compress(terms, amps, maxdim=maxdim, tol=1e-12 if tol is None else tol)


# ---------------------------------------------------------------- product-vector read-outs: off-grid transform values
PRODUCT_CHAIN_MAX_BOND = 1024           # QIL_PRODUCT_CHAIN_MAX_BOND (include/qilaplace_hip.h): the chain route's LDS carry
PRODUCT_MANY_ROWS_CHAIN_WORK = 1 << 21  # kManyRowsChainWork (csrc/qil_product.hip): bonds < 128 stay on the chain below this rows * bond^2


def _product_weights(psi, v, what):
    """The checks of `product_batch`, before any native call: (nb, n_tensors, 2) numbers."""
    if not isinstance(psi, SignalMPS):
        raise TypeError(f"{what}: unsupported operand types")
    w = np.asarray(v)
    if w.dtype.kind not in "iufc":
        raise TypeError(f"{what}: the weights must be real or complex numbers, got dtype {w.dtype}")
    n = _ntensors(psi)
    if w.ndim != 3 or w.shape[1:] != (n, 2):
        raise ValueError(f"{what}: expected weights of shape (nb, {n}, 2), got {w.shape}")
    return w


def product_batch(psi, v, conj=False):
    """out[r] = amplitude * prod_i (v[r,i,0] A_i[:,0,:] + v[r,i,1] A_i[:,1,:])  (qil_product_batch): the overlap of psi with nb
    product vectors given as numbers, v of shape (nb, n_tensors, 2), real or complex.  conj=True conjugates the weights:
    <v|psi>.  v = e_bit is `coefficient_batch`, v = (1, 1) on a tensor sums it as `marginal_batch`'s 2 does.  Returns complex
    values, or real ones when the state and the weights are both real."""
    w = _product_weights(psi, v, "product_batch")
    real = not np.iscomplexobj(w) and psi.dtype != np.complex128
    w = np.ascontiguousarray(w.conj() if conj else w, dtype=np.complex128)
    nb = w.shape[0]
    out = np.zeros(nb, dtype=np.complex128)
    if nb:
        L.check(L.lib.qil_product_batch(psi.handle, nb, w.ctypes.data_as(L._pdbl), out.ctypes.data_as(L._pdbl)))
    return out.real.copy() if real else out


def laplace_weights(sigma, cycles, n):
    """(Public for the reason `exponential_tensors` is: it needs no device.)  The (nb, n, 2) weights [1, w^(2^(n-i))] of
    w = exp(-(sigma + 2 pi i c)), tensor i = 1 .. n with tensor 1 the most significant bit, for `product_batch` on an n-site
    SignalMPS; sigma and cycles (c, in cycles per sample) are broadcast against each other.

    w^(2^m) = exp(-sigma 2^m) exp(-2 pi i frac(c 2^m)): the scaling by 2^m and the reduction mod 1 are exact in double, so
    every weight is one exp, one cos and one sin away from its argument -- never a square of a rounded w, which loses a bit per
    level (2^39 u at n = 40).  sigma < 0 may overflow at a high bit: ValueError naming the bit.  Underflow to 0 is the value."""
    n = int(n)
    if n < 1:
        raise ValueError("laplace_weights: n must be >= 1")
    s, c = np.broadcast_arrays(np.asarray(sigma, dtype=np.float64), np.asarray(cycles, dtype=np.float64))
    s, c = s.reshape(-1), c.reshape(-1)
    if not (np.isfinite(s).all() and np.isfinite(c).all()):
        raise ValueError("laplace_weights: sigma and cycles must be finite")
    scale = np.ldexp(1.0, n - 1 - np.arange(n))[None, :]          # tensor i (0-based) carries bit m = n - 1 - i
    ld = np.longdouble                                            # wider than double where the platform has it: one rounding at the end
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        # a grid of points repeats its sigmas and its cycles: one exp per distinct sigma, one cos / sin per distinct c
        (us, js), (uc, jc) = np.unique(s, return_inverse=True), np.unique(c, return_inverse=True)
        t = uc[:, None] * scale                                   # exact: a scaling by a power of two
        frac = t - np.rint(t)                                     # exact: t mod 1, in [-1/2, 1/2]
        mod = np.exp(-(us[:, None] * scale).astype(ld))[js.reshape(-1)]
        ang = (-8 * np.arctan(ld(1))) * frac.astype(ld)
        t, re, im = t[jc.reshape(-1)], np.cos(ang)[jc.reshape(-1)], np.sin(ang)[jc.reshape(-1)]
        hi = (mod * re).astype(np.float64) + 1j * (mod * im).astype(np.float64)
    bad = ~(np.isfinite(hi) & np.isfinite(t))
    if bad.any():
        r, i = np.argwhere(bad)[0]
        raise ValueError(f"laplace_weights: exp(-sigma 2^m) overflows at bit m = {n - 1 - int(i)} (sigma = {float(s[r])!r})")
    out = np.ones((s.size, n, 2), dtype=np.complex128)
    out[:, :, 1] = hi
    return out


def _signal_weights(psi, hi, what):
    """(nb, n) upper weights, bit of tensor i of the signal register -> the (nb, n_tensors, 2) weights of psi: a ZTMPS of a signal
    carries main and copy tensors interleaved with the copy register delta-fused, so its copy tensors get (1, 1)."""
    if not isinstance(psi, SignalMPS):
        raise TypeError(f"{what}: unsupported operand types")
    nb, n = hi.shape
    if isinstance(psi, ZTMPS):
        w = np.ones((nb, 2 * n, 2), dtype=hi.dtype)
        w[:, 0::2, 1] = hi
    else:
        w = np.ones((nb, n, 2), dtype=hi.dtype)
        w[:, :, 1] = hi
    return w


def laplace_sum(psi, sigma, cycles):
    """sum_j x_j exp(-(sigma + 2 pi i c) j) of the signal psi encodes (a SignalMPS, or the ZTMPS of a signal), amplitude
    included, at any real sigma and c (cycles per sample; broadcast against each other; the result has the broadcast shape).
    One `product_batch` call: O(n chi^2) per point, no operator, no grid."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("laplace_sum: unsupported operand types")
    shape = np.broadcast(np.asarray(sigma), np.asarray(cycles)).shape
    w = laplace_weights(sigma, cycles, len(psi))
    out = product_batch(psi, _signal_weights(psi, w[:, :, 1], "laplace_sum"))
    return np.asarray(out, dtype=np.complex128).reshape(shape)


def power_sum(psi, w):
    """sum_j x_j w^j for callers who hold w itself (any complex numbers, any shape): the dyadic powers w^(2^m) come correctly
    rounded from `_dyadic_powers`.  A power that overflows raises ValueError."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("power_sum: unsupported operand types")
    ws = np.asarray(w, dtype=np.complex128)
    n = len(psi)
    hi = np.empty((ws.size, n), dtype=np.complex128)
    for r, z in enumerate(ws.reshape(-1)):
        hi[r] = _dyadic_powers(z, n)[::-1]
    if not np.isfinite(hi).all():
        r, i = np.argwhere(~np.isfinite(hi))[0]
        raise ValueError(f"power_sum: w^(2^{n - 1 - int(i)}) overflows for w = {ws.reshape(-1)[r]!r}")
    if not np.iscomplexobj(np.asarray(w)):
        hi = hi.real.copy()
    out = product_batch(psi, _signal_weights(psi, hi, "power_sum"))
    return np.asarray(out).reshape(ws.shape)


def dft_eval(psi, f):
    """The unitary DFT of the encoded signal at ANY real frequency f (in bins): (1 / sqrt N) sum_j x_j exp(-2 pi i f j / N)."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("dft_eval: unsupported operand types")
    N = 2.0 ** len(psi)
    return laplace_sum(psi, 0.0, np.asarray(f, dtype=np.float64) / N) / np.sqrt(N)


def dt_eval(psi, wr, k):
    """The damping transform at any real k: (1 / sqrt N) sum_j x_j exp(-wr k j / N)."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("dt_eval: unsupported operand types")
    N = 2.0 ** len(psi)
    return laplace_sum(psi, float(wr) * np.asarray(k, dtype=np.float64) / N, 0.0) / np.sqrt(N)


def zt_eval(psi, wr, k, l):
    """The z-transform at any real (k, l), broadcast against each other: (1 / N) sum_j x_j exp(-((wr k + 2 pi i l) / N) j)
    (the reference's grid values with wi = 2 pi, dt = 1)."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("zt_eval: unsupported operand types")
    N = 2.0 ** len(psi)
    return laplace_sum(psi, float(wr) * np.asarray(k, dtype=np.float64) / N, np.asarray(l, dtype=np.float64) / N) / N


_GOLDEN = (np.sqrt(5.0) - 1.0) / 2.0


def _golden_maximise(evaluate, lo, hi, tol):
    """Golden-section search for the maximiser of evaluate(x) (vectorised: one call evaluates every interval's two probes)
    inside each [lo, hi]; stops when every interval is shorter than tol.  Returns the midpoints."""
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    a, b = hi - _GOLDEN * (hi - lo), lo + _GOLDEN * (hi - lo)
    fa, fb = np.split(np.asarray(evaluate(np.concatenate([a, b]))), 2)
    while (hi - lo).max(initial=0.0) > tol:
        left = fa >= fb                                   # the maximum lies in [lo, b], else in [a, hi]
        hi, lo = np.where(left, b, hi), np.where(left, lo, a)
        na, nb_ = hi - _GOLDEN * (hi - lo), lo + _GOLDEN * (hi - lo)
        probe = np.asarray(evaluate(np.where(left, na, nb_)))     # one new point per interval, all in one call
        a, b, fa, fb = (np.where(left, na, b), np.where(left, a, nb_), np.where(left, probe, fb), np.where(left, fa, probe))
    return 0.5 * (lo + hi)


def refine_frequencies(psi, f0, half_width=0.5, sigma=0.0, tol=1e-6):
    """Sub-bin refinement of the bins `top_k` finds: for each starting bin f0 the maximiser of |laplace_sum(psi, sigma, f / N)|
    along the circle of fixed sigma within f0 +- half_width, by a golden-section search down to `tol` bins; every iteration
    evaluates all candidates' points in one `product_batch` call.  Returns (f, value at f).

    One-dimensional on purpose: the transform of a finite record is a polynomial in w, and the modulus of a polynomial has no
    interior maximum (maximum modulus principle) -- a search over (sigma, f) would run to the boundary of any window."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("refine_frequencies: unsupported operand types")
    f0 = np.atleast_1d(np.asarray(f0, dtype=np.float64))
    N = 2.0 ** len(psi)
    f = _golden_maximise(lambda x: np.abs(laplace_sum(psi, float(sigma), x / N)), f0 - half_width, f0 + half_width, float(tol))
    return f, laplace_sum(psi, float(sigma), f / N)


# ---------------------------------------------------------------- ESPRIT on the bond basis: poles without a scan
def _require_signal(psi, what):
    if not isinstance(psi, SignalMPS):
        raise TypeError(f"{what}: unsupported operand types")
    if isinstance(psi, ZTMPS):
        raise TypeError(f"{what}: unsupported operand types (a ZTMPS has no single sample register to shift; pass the SignalMPS)")


def _low_register(psi, count, what):
    """`count` as an int, after the range check: the low register has 1 .. n - 1 tensors (a cut inside the chain)."""
    n = len(psi)
    if isinstance(count, (bool, np.bool_)) or not isinstance(count, (int, np.integer)):
        raise TypeError(f"{what}: count must be an integer, got {type(count).__name__}")
    if not 1 <= count <= n - 1:
        raise ValueError(f"{what}: count {int(count)} outside [1, {n - 1}] (the low register is cut off inside the chain)")
    return int(count)


def shift_pencil(psi, count):
    """The shift pencil of the low register: with R (chi x 2^count) the matrix of the last `count` tensors of the SignalMPS psi
    (R[:, l]: the bond vector of the low bits l, site 1 being the most significant bit), returns (G, P, r_last) with
    G = R R^H, P = R[:, 1:] R[:, :-1]^H and r_last = R[:, -1] -- three right `environment`s over those tensors, O(count chi^3),
    never 2^count columns: psi with itself; psi with the one-sample shift `build_shift_mpo(psi, 1)`, of which the carry-out-0
    component is the shifted Gram matrix; the all-ones basis state against psi.  Amplitudes are not applied."""
    _require_signal(psi, "shift_pencil")
    count = _low_register(psi, count, "shift_pencil")
    from .builders import build_shift_mpo
    n = len(psi)
    one = np.zeros((1, 2, 1))
    one[0, 1, 0] = 1.0
    ones = SignalMPS([one] * n, sites=psi.site_ids, ctx=psi.ctx)
    G = environment(psi, psi, side="right", count=count).conj()                 # E[p, s] = sum_l conj(R[p, l]) R[s, l]
    P = environment(psi, psi, W=build_shift_mpo(psi, 1), side="right", count=count)[:, 0, :].conj()   # conj(R[p, l + 1]) R[s, l]
    r_last = environment(ones, psi, side="right", count=count)[0, :].copy()
    return G, P, r_last


def esprit_from_pencil(G, P, r_last, rcond=1e-12):
    """The poles from a shift pencil (host only; public so that it can be checked without a device): for R[:, l] = T diag(c) z^l
    the columns satisfy R[:, 1:] = Phi R[:, :-1] with Phi = T diag(z) T^-1, and the least-squares Phi is
    P pinv(G - r_last r_last^H): its eigenvalues are the poles.  The pencil is first scaled to a unit diagonal of G (a
    similarity of Phi); pinv drops directions below rcond of the largest.  Returns chi complex numbers: a bond that carries
    less than chi modes returns spurious ones among them (`esprit` gives those negligible amplitudes)."""
    G, P = np.asarray(G, dtype=np.complex128), np.asarray(P, dtype=np.complex128)
    r = np.asarray(r_last, dtype=np.complex128).reshape(-1)
    chi = r.size
    if G.shape != (chi, chi) or P.shape != (chi, chi):
        raise ValueError(f"esprit_from_pencil: expected G and P of shape ({chi}, {chi}), got {G.shape} and {P.shape}")
    if not (np.isfinite(G).all() and np.isfinite(P).all() and np.isfinite(r).all()):
        raise ValueError("esprit_from_pencil: the pencil is not finite")
    d = np.sqrt(np.abs(np.real(np.diag(G))))
    d = 1.0 / np.where(d > 0, d, 1.0)
    H = (G - np.outer(r, r.conj())) * np.outer(d, d)
    H = 0.5 * (H + H.conj().T)
    Phi = (P * np.outer(d, d)) @ np.linalg.pinv(H, rcond=float(rcond), hermitian=True)
    return np.linalg.eigvals(Phi)


def _esprit_amplitudes(psi, poles):
    """The least-squares amplitudes of x_j ~ sum_k a_k z_k^j over all 2^n samples, from the normal equations: the right-hand
    side <z_k^j | x> is one `product_batch`, the Gram entries sum_j q^j = prod_b (1 + q^(2^b)), q = conj(z_k) z_k', from the
    correctly rounded dyadic powers of the poles (stable at q ~ 1, where (1 - q^N) / (1 - q) is not)."""
    n, K = len(psi), len(poles)
    pw = np.array([_dyadic_powers(z, n) for z in poles], dtype=np.complex128).reshape(K, n)      # pw[k, b] = z_k^(2^b)
    if not np.isfinite(pw).all():
        k, b = np.argwhere(~np.isfinite(pw))[0]
        raise ValueError(f"esprit: z^(2^{int(b)}) overflows for the pole z = {complex(poles[k])!r} (|z| > 1: the limits of exponential_mps)")
    w = np.ones((K, n, 2), dtype=np.complex128)
    w[:, :, 1] = pw[:, ::-1]                                                   # tensor i carries bit n - 1 - i
    h = np.asarray(product_batch(psi, w, conj=True), dtype=np.complex128)
    with np.errstate(over="ignore", invalid="ignore"):
        M = np.prod(1.0 + pw.conj()[:, None, :] * pw[None, :, :], axis=2)
    if not np.isfinite(M).all():
        raise ValueError("esprit: the Gram matrix of the modes overflows (|z| > 1: the limits of exponential_mps)")
    return np.linalg.lstsq(M, h, rcond=None)[0]


def esprit(psi, maxdim=None, tol=None, count=None, return_model=False):
    """Poles and amplitudes of x_j = sum_k a_k z_k^j from the SignalMPS of x, without a scan and without a window: the bond basis of
    the state already holds the signal subspace, and `shift_pencil` + `esprit_from_pencil` read the poles off the last `count`
    tensors (ESPRIT with the Hankel SVD replaced by the truncation the encoder has done).  O(count chi^3).

    maxdim / tol: `compress` a copy first (either one given; tol defaults to 1e-12) -- the rank selection is the truncation's: one
    pole per unit of bond dimension at the cut.  count: the tensors of the low register; default: everything right of the
    leftmost bond that attains the state's largest bond dimension, the longest register that still carries the full rank
    (a long baseline is what buys accuracy).  ValueError when 2^count - 1 columns cannot determine a bond of that size.
    Returns (poles, amplitudes) sorted by |amplitude| descending; the amplitudes are the least-squares fit over all 2^n
    samples of psi (amplitude included).  A bond inflated by rounding-level junk returns spurious poles with negligible amplitudes.
    Modes with |z| > 1 inherit the overflow limits of `exponential_mps` (ValueError when a dyadic power overflows).
    return_model=True adds exponential_sum(amplitudes, poles, n) untruncated and its relative distance to psi (through the exact
    gauge of the difference: no 1e-7 floor)."""
    _require_signal(psi, "esprit")
    n = len(psi)
    if n < 2:
        raise ValueError("esprit: needs at least 2 sites")
    if count is not None:
        count = _low_register(psi, count, "esprit")
    work = psi
    if maxdim is not None or tol is not None:
        work = compress(psi.copy(), maxdim=maxdim, tol=1e-12 if tol is None else tol)
    bonds = work.bond_dims
    if count is None:
        count = n - 1 - bonds.index(max(bonds))
    chi = bonds[n - 1 - count]
    if (1 << count) - 1 < chi:
        raise ValueError(f"esprit: a register of {count} tensors has {(1 << count) - 1} shifted columns, fewer than the bond {chi} at its cut")
    poles = esprit_from_pencil(*shift_pencil(work, count))
    amps = _esprit_amplitudes(psi, poles)
    order = np.argsort(-np.abs(amps), kind="stable")
    poles, amps = poles[order], amps[order]
    if not return_model:
        return poles, amps
    model = exponential_sum(amps, poles, n, maxdim=None, tol=None)
    diff = sub(model, psi)
    try:
        _, nd = bond_spectra(diff, return_norm=True)
    except L.QilDomainError:                                                   # the difference is exactly zero
        nd = 0.0
    return poles, amps, model, abs(diff.amplitude) * nd / (abs(psi.amplitude) * norm(psi))


# ---------------------------------------------------------------- encode
def _signal_operand(x, what):
    """What an encoder hands to the library for the signal x: (the object that keeps the samples alive, pointer, length, dtype
    code, n = round(log2 length)); warns when the length is not 2^n (the library zero-fills)."""
    cai = getattr(x, "__cuda_array_interface__", None)
    if cai is not None:
        # samples already in HBM (a torch / cupy-style device array): hand the device pointer over, no PCIe
        # trip.  Must be 1-D, contiguous, float64 or complex128; the producer's stream is drained first.
        if len(cai["shape"]) != 1 or cai.get("strides") not in (None, (np.dtype(cai["typestr"]).itemsize,)):
            raise ValueError(f"{what}: device signal must be a contiguous 1-D array")
        dt = np.dtype(cai["typestr"])
        if dt not in (np.dtype(np.float64), np.dtype(np.complex128)):
            raise ValueError(f"{what}: device signal must be float64 or complex128, got {dt}")
        code = L.QIL_C64 if dt == np.dtype(np.complex128) else L.QIL_F64
        N = int(cai["shape"][0])
        ptr = C.c_void_p(int(cai["data"][0]))
        sync = getattr(x, "device", None)
        if sync is not None and "torch" in type(x).__module__:
            import torch
            torch.cuda.current_stream(x.device).synchronize()
        keep = x
    else:
        x = np.asarray(x)
        code = L.QIL_C64 if np.iscomplexobj(x) else L.QIL_F64
        keep = np.ascontiguousarray(x, dtype=_np_dtype(code))
        N = len(keep)
        ptr = keep.ctypes.data_as(C.c_void_p)
    n = max(1, int(round(np.log2(max(N, 1)))))
    if N < 2 ** n:
        warnings.warn(f"_array_to_tensor: input length {N} is not a power of 2; zero-filling to {2**n}")
    return keep, ptr, N, code, n


def _encode(fn, cls, x, method, cutoff, maxdim, k, p, q, random_seed, mindim, ctx):
    if method not in ("svd", "rsvd"):
        raise ValueError(f"tensor_to_mps: unknown method {method}. Use :svd or :rsvd.")
    ctx = ctx or default_context()
    keep, ptr, N, code, _ = _signal_operand(x, "signal_mps")
    h = C.c_void_p()
    L.check(fn(ctx.handle, ptr, N, code,
               L.QIL_METHOD_SVD if method == "svd" else L.QIL_METHOD_RSVD, float(cutoff), _maxdim(maxdim),
               int(k), int(p), int(q), C.c_uint64(random_seed), int(mindim), C.byref(h)))
    return cls(ctx=ctx, _handle=h)


def _encode_batch(fn, cls, xs, method, cutoff, maxdim, k, p, q, random_seed, mindim, ctx):
    if method not in ("svd", "rsvd"):
        raise ValueError(f"tensor_to_mps: unknown method {method}. Use :svd or :rsvd.")
    ctx = ctx or default_context()
    xs = [np.asarray(x) for x in xs]
    if not xs:
        return []
    code = L.QIL_C64 if any(np.iscomplexobj(x) for x in xs) else L.QIL_F64
    keep = [np.ascontiguousarray(x, dtype=_np_dtype(code)) for x in xs]
    N = len(keep[0])
    if any(x.ndim != 1 or len(x) != N for x in keep):
        raise ValueError("signal batch: all signals must be 1-D and of one length")
    n = max(1, int(round(np.log2(max(N, 1)))))
    if N < 2 ** n:
        warnings.warn(f"_array_to_tensor: input length {N} is not a power of 2; zero-filling to {2**n}")
    ptrs = (C.c_void_p * len(keep))(*[x.ctypes.data for x in keep])
    outs = (C.c_void_p * len(keep))()
    L.check(fn(ctx.handle, ptrs, len(keep), N, code,
               L.QIL_METHOD_SVD if method == "svd" else L.QIL_METHOD_RSVD, float(cutoff), _maxdim(maxdim),
               int(k), int(p), int(q), C.c_uint64(random_seed), int(mindim), outs))
    return [cls(ctx=ctx, _handle=C.c_void_p(h)) for h in outs]


def signal_mps_batch(xs, method="svd", cutoff=1e-15, maxdim=None, k=20, p=10, q=0, random_seed=1234, mindim=1, ctx=None):
    """signal_mps for several signals of one length (the signal kinds of a benchmark sweep), encoded concurrently on the
    context's streams; item j is exactly signal_mps(xs[j]; ...)."""
    return _encode_batch(L.lib.qil_signal_mps_batch, SignalMPS, xs, method, cutoff, maxdim, k, p, q, random_seed, mindim, ctx)


def signal_ztmps_batch(xs, cutoff=1e-10, maxdim=None, method="svd", k=20, p=10, q=0, random_seed=1234, mindim=1, ctx=None):
    """signal_ztmps for several signals of one length, encoded concurrently; item j is exactly signal_ztmps(xs[j]; ...)."""
    return _encode_batch(L.lib.qil_signal_ztmps_batch, ZTMPS, xs, method, cutoff, maxdim, k, p, q, random_seed, mindim, ctx)


def signal_mps(x, method="svd", cutoff=1e-15, maxdim=None, k=20, p=10, q=0, random_seed=1234, mindim=1,
               ctx=None):
    """signal_mps(x; method=:svd, cutoff, maxdim, k, p, q, random_seed, mindim)."""
    return _encode(L.lib.qil_signal_mps, SignalMPS, x, method, cutoff, maxdim, k, p, q, random_seed, mindim, ctx)


def signal_ztmps(x, cutoff=1e-10, maxdim=None, method="svd", k=20, p=10, q=0, random_seed=1234, mindim=1,
                 ctx=None):
    """signal_ztmps(x; cutoff=1e-10, maxdim, kwargs...)."""
    return _encode(L.lib.qil_signal_ztmps, ZTMPS, x, method, cutoff, maxdim, k, p, q, random_seed, mindim, ctx)


def _cross_seeds(n, seeds, random_seed):
    if seeds is None:
        drawn = np.random.default_rng(random_seed).integers(0, 2 ** n, size=62, dtype=np.int64)
        seeds = np.concatenate([np.array([0, 2 ** n - 1], dtype=np.int64), drawn])
    seeds = np.ascontiguousarray(np.asarray(seeds).reshape(-1), dtype=np.int64)
    return seeds, seeds.ctypes.data_as(C.POINTER(C.c_int64))


def _cross_info(est, nevals, sweeps, converged):
    return {"est": est.value, "nevals": nevals.value, "sweeps": sweeps.value, "converged": converged.value}


def _cross_from_callable(f, n, maxdim, tol, max_sweeps, seeds, random_seed, ctx):
    import torch
    if n is None:
        raise ValueError("signal_mps_cross: a callable needs n, the number of sites")
    n = int(n)
    if not 1 <= n <= 62:
        raise ValueError(f"signal_mps_cross: n = {n} outside 1 .. 62")
    dev = torch.device("cuda", ctx.device)

    def evaluate(idx, code=None):
        v = f(idx)
        if not isinstance(v, torch.Tensor) or v.device != idx.device or v.shape != idx.shape:
            raise ValueError("signal_mps_cross: the callable must return a device tensor of its argument's length")
        if v.dtype not in (torch.float64, torch.complex128):
            raise ValueError(f"signal_mps_cross: the callable must return float64 or complex128, got {v.dtype}")
        got = L.QIL_C64 if v.dtype == torch.complex128 else L.QIL_F64
        if code is not None and got != code:
            if code == L.QIL_F64:
                raise ValueError("signal_mps_cross: the callable returned complex values after real ones")
            v = v.to(torch.complex128)
            got = code
        return v.contiguous(), got

    seeds_np, seeds_p = _cross_seeds(n, seeds, random_seed)
    if len(seeds_np) < 1 or seeds_np.min() < 0 or seeds_np.max() >= 2 ** n:
        raise ValueError(f"signal_mps_cross: seeds must be indices in [0, 2^{n})")
    # the dtype comes from the first evaluation
    _, code = evaluate(torch.from_numpy(seeds_np).to(dev))
    s = C.c_void_p()
    L.check(L.lib.qil_cross_begin(ctx.handle, n, code, int(maxdim), float(tol), int(max_sweeps), seeds_p, len(seeds_np),
                                  C.byref(s)))
    try:
        count = C.c_int64()
        while True:
            L.check(L.lib.qil_cross_pending(s, C.byref(count)))
            if count.value == 0:
                break
            idx = torch.empty(count.value, dtype=torch.int64, device=dev)
            L.check(L.lib.qil_cross_indices(s, C.c_void_p(idx.data_ptr())))
            vals, _ = evaluate(idx, code)
            torch.cuda.current_stream(dev).synchronize()
            L.check(L.lib.qil_cross_supply(s, C.c_void_p(vals.data_ptr())))
        h = C.c_void_p()
        est, nevals, sweeps, converged = C.c_double(), C.c_int64(), C.c_int(), C.c_int()
        L.check(L.lib.qil_cross_finish(s, C.byref(h), C.byref(est), C.byref(nevals), C.byref(sweeps), C.byref(converged)))
    finally:
        L.lib.qil_cross_destroy(s)
    return SignalMPS(ctx=ctx, _handle=h), _cross_info(est, nevals, sweeps, converged)


def signal_mps_cross(x_or_f, n=None, maxdim=64, tol=1e-10, max_sweeps=8, seeds=None, random_seed=1234, return_info=False,
                     ctx=None):
    """The SignalMPS of a signal by tensor cross interpolation: O(n maxdim^2) samples, chosen adaptively by full-pivot LU
    factorisations of two-site blocks, instead of all 2^n of them.

    x_or_f: an array or a `__cuda_array_interface__` object, as signal_mps accepts (n = round(log2 len); a length that is not a
    power of two reads as zero-filled, with a warning), or a callable f(idx): a 1-D int64 torch tensor on the device ->
    float64 or complex128 values of the same length (requires n, up to 62; the dtype comes from the first evaluation).
    maxdim: the rank cap, 1 .. 256.  tol: pivots stop when the largest remaining |entry| of a block is <= tol times the largest
    |x| sampled; the encode has converged when that holds at every bond over a whole back-and-forth sweep.  seeds: the sample
    indices whose suffixes the first sweep starts from; by default 0, 2^n - 1 and 62 indices drawn from random_seed.
    return_info adds a dict: est (the largest remaining |entry| of the last sweep, relative to the largest |x| sampled),
    nevals (samples read), sweeps, converged.

    Known blind spot of cross interpolation: a feature that no pivot's row or column touches is invisible, and the estimate
    does not see it either -- an isolated spike is the standard case (converged, est small, spike missing).  The remedy is
    to pass its index in `seeds`."""
    ctx = ctx or default_context()
    if not isinstance(maxdim, (int, np.integer)) or isinstance(maxdim, bool):
        raise ValueError("signal_mps_cross: maxdim must be an integer, 1 .. 256")
    if callable(x_or_f):
        psi, info = _cross_from_callable(x_or_f, n, maxdim, tol, max_sweeps, seeds, random_seed, ctx)
        return (psi, info) if return_info else psi
    keep, ptr, N, code, nn = _signal_operand(x_or_f, "signal_mps_cross")
    if n is not None and int(n) != nn:
        raise ValueError(f"signal_mps_cross: n = {n} does not match a signal of {N} samples")
    seeds_np, seeds_p = _cross_seeds(min(nn, 62), seeds, random_seed)
    h = C.c_void_p()
    est, nevals, sweeps, converged = C.c_double(), C.c_int64(), C.c_int(), C.c_int()
    L.check(L.lib.qil_signal_mps_cross(ctx.handle, ptr, N, code, int(maxdim), float(tol), int(max_sweeps), seeds_p, len(seeds_np),
                                       C.byref(h), C.byref(est), C.byref(nevals), C.byref(sweeps), C.byref(converged)))
    del keep
    psi = SignalMPS(ctx=ctx, _handle=h)
    return (psi, _cross_info(est, nevals, sweeps, converged)) if return_info else psi


def ztmps_from_mps(psi, cutoff=1e-10, maxdim=None):
    """The ZTMPS of a SignalMPS that exists already: the per-site delta-fuse and split of signal_ztmps, so that
    ztmps_from_mps(signal_mps(x, cutoff=c), cutoff=c) is signal_ztmps(x, cutoff=c).  The way of a cross-encoded state
    (signal_mps_cross) into the z-transform pipeline.  psi is left intact; a paired psi raises ValueError."""
    if not isinstance(psi, SignalMPS):
        raise TypeError(f"ztmps_from_mps: unsupported operand types ({type(psi).__name__})")
    if isinstance(psi, ZTMPS) or psi.paired:
        raise ValueError("ztmps_from_mps: the operand is a paired state already")
    h = C.c_void_p()
    L.check(L.lib.qil_ztmps_from_mps(psi.handle, float(cutoff), _maxdim(maxdim), C.byref(h)))
    return ZTMPS(ctx=psi.ctx, _handle=h)


# ---------------------------------------------------------------- read-out by index on the device, element-wise functions
def coefficient_at_route(dims, forced=None):
    """The route qil_coefficient_at takes for a chain with the bond dimensions `dims` (the decision of csrc/qil_index.hip,
    mirrored): "wave" while every bond is <= QIL_COEFFICIENT_AT_WAVE_MAX_BOND, "bits" above.  forced: the value of
    QIL_COEFFICIENT_AT_ROUTE; "wave" holds while the carry fits the LDS (bonds <= 1024), "bits" always."""
    top = max([1] + [int(d) for d in dims])
    if forced == "bits":
        return "bits"
    if forced == "wave":
        return "wave" if top <= 1024 else "bits"
    return "wave" if top <= L.QIL_COEFFICIENT_AT_WAVE_MAX_BOND else "bits"


def coefficient_at(psi, idx):
    """psi at the indices idx, device to device (include/qilaplace_hip.h, qil_coefficient_at): idx is a 1-D int64 torch tensor
    on the context's device or any `__cuda_array_interface__` object; the result is a torch tensor on that device, float64 for
    a real state and complex128 otherwise, amplitude included.  Site 1 is the most significant bit of an index (for a ZTMPS:
    of the 2n interleaved tensors main_1, copy_1, ..).  An index outside [0, 2^n) gives NaN.  Host configurations go through
    coefficient_batch."""
    if not isinstance(psi, SignalMPS):
        raise TypeError("coefficient_at: unsupported operand types")
    import torch
    if isinstance(idx, torch.Tensor):
        if idx.device.type != "cuda":
            raise TypeError("coefficient_at: idx must live on the device; for host configurations use coefficient_batch")
        t = idx
    elif hasattr(idx, "__cuda_array_interface__"):
        t = torch.as_tensor(idx, device=torch.device("cuda", psi.ctx.device))
    else:
        raise TypeError("coefficient_at: idx must be a device tensor or a __cuda_array_interface__ object; for host "
                        "configurations use coefficient_batch")
    dev = torch.device("cuda", psi.ctx.device)
    if t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError(f"coefficient_at: idx must be a 1-D int64 tensor, got {t.dtype} with {t.dim()} dimensions")
    if t.device != dev:
        raise ValueError(f"coefficient_at: idx lives on {t.device}, the state on {dev}")
    t = t.contiguous()
    out = torch.empty(t.numel(), dtype=torch.complex128 if psi.dtype == np.complex128 else torch.float64, device=dev)
    if t.numel():
        torch.cuda.current_stream(dev).synchronize()
        L.check(L.lib.qil_coefficient_at(psi.handle, t.numel(), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())))
    return out


_MAP_OPS = {"abs": (L.QIL_MAP_ABS, 1, 0), "power": (L.QIL_MAP_POWER, 1, 1), "log": (L.QIL_MAP_LOG, 1, 1),
            "divide": (L.QIL_MAP_DIVIDE, 2, 1), "shrink": (L.QIL_MAP_SHRINK, 1, 1)}      # name: (code, states, parameters)


def _map_operands(what, states, count=None):
    """Unpaired SignalMPS of one length, checked before any native verb; returns the number of sites."""
    if not states or not all(isinstance(s, SignalMPS) for s in states) or (count is not None and len(states) != count):
        raise TypeError(f"{what}: unsupported operand types")
    if any(s._paired() for s in states):
        raise ValueError("map: paired states are not supported; map the SignalMPS and call ztmps_from_mps")
    n = len(states[0])
    for s in states[1:]:
        if len(s) != n:
            raise ValueError(f"{what}: states must have the same number of sites. Found {n} and {len(s)}")
    return n


def _map_seeds(states, n, seeds, seed_peaks, random_seed):
    """Explicit seeds as given; otherwise _cross_seeds' defaults and, per operand, the indices of its seed_peaks largest entries."""
    if seeds is not None or n > 62:
        return _cross_seeds(min(n, 62), seeds, random_seed)
    parts = [_cross_seeds(n, None, random_seed)[0]]
    if seed_peaks:
        for s in states:
            parts.append(np.asarray(top_k(s, k=min(int(seed_peaks), 2 ** n))[0], dtype=np.int64))
    return _cross_seeds(n, np.concatenate(parts), random_seed)


def map_states(op, *states, params=(), maxdim=64, tol=1e-10, max_sweeps=8, seeds=None, seed_peaks=8, random_seed=1234,
               return_info=False):
    """An element-wise function of states as a new SignalMPS, by cross interpolation with the samples read from the operands on
    the device (include/qilaplace_hip.h, qil_mps_map).  op: "abs" |a|, "power" |a|^p (params = (p,), p > 0), "log"
    log(|a|^2 + eps) (eps > 0), "divide" a conj(b) / (|b|^2 + lambda) of two states (lambda >= 0; 0 is a / b), "shrink"
    a max(0, 1 - tau / |a|) (tau >= 0).  Amplitudes are included.  abs, power and log give a real state, divide a complex one
    when either operand is, shrink its operand's dtype.

    maxdim, tol, max_sweeps, seeds, random_seed, return_info: as in signal_mps_cross.  By default the seeds are
    signal_mps_cross' and the indices of the seed_peaks largest entries of every operand (top_k): the features of f(psi)
    usually sit where psi's do.  seed_peaks=0 turns that off; explicit seeds are used as given.

    The blind spot of cross interpolation is inherited: a feature of the result that no pivot's row or column touches is
    invisible, and the estimate does not see it either; the remedy is to pass its index in `seeds`."""
    if op not in _MAP_OPS:
        raise ValueError(f"map_states: unknown op {op!r}; one of {sorted(_MAP_OPS)}")
    code, count, nparams = _MAP_OPS[op]
    n = _map_operands("map_states", states, count)
    if not isinstance(maxdim, (int, np.integer)) or isinstance(maxdim, bool):
        raise ValueError("map_states: maxdim must be an integer, 1 .. 256")
    par = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)).reshape(-1))
    if len(par) != nparams:
        raise ValueError(f"map_states: {op} takes {nparams} parameter(s), got {len(par)}")
    seeds_np, seeds_p = _map_seeds(states, n, seeds, seed_peaks, random_seed)
    handles = (C.c_void_p * len(states))(*[s.handle for s in states])
    h = C.c_void_p()
    est, nevals, sweeps, converged = C.c_double(), C.c_int64(), C.c_int(), C.c_int()
    L.check(L.lib.qil_mps_map(handles, len(states), code, par.ctypes.data_as(L._pdbl) if nparams else None, int(maxdim),
                              float(tol), int(max_sweeps), seeds_p, len(seeds_np), C.byref(h), C.byref(est), C.byref(nevals),
                              C.byref(sweeps), C.byref(converged)))
    out = SignalMPS(ctx=states[0].ctx, _handle=h)
    return (out, _cross_info(est, nevals, sweeps, converged)) if return_info else out


def cross_map(f, *states, n=None, maxdim=64, tol=1e-10, max_sweeps=8, seeds=None, seed_peaks=8, random_seed=1234,
              return_info=False):
    """The SignalMPS of f(psi_1[x], psi_2[x], ..) for an arbitrary torch function f of device value tensors (float64 for a real
    state, complex128 otherwise; f returns float64 or complex128 of the same length): the pull session of signal_mps_cross
    with every request answered by coefficient_at on the operands.  The arguments and the blind spot are map_states'.  The
    five built-in functions are faster through map_states, which never leaves the library, while the operands' bonds are small
    (1.6x at bond 8); at bond 32 and above this route is the faster one for them too, because coefficient_at then reads
    through MFMA GEMMs and map_states' sampler does not (MEASUREMENTS section 29)."""
    if not callable(f):
        raise TypeError("cross_map: f must be callable")
    nn = _map_operands("cross_map", states)
    if n is not None and int(n) != nn:
        raise ValueError(f"cross_map: n = {n} does not match states of {nn} sites")
    if not isinstance(maxdim, (int, np.integer)) or isinstance(maxdim, bool):
        raise ValueError("cross_map: maxdim must be an integer, 1 .. 256")
    seeds_np, _ = _map_seeds(states, nn, seeds, seed_peaks, random_seed)
    psi, info = _cross_from_callable(lambda idx: f(*[coefficient_at(s, idx) for s in states]), nn, maxdim, tol, max_sweeps,
                                     seeds_np, random_seed, states[0].ctx)
    return (psi, info) if return_info else psi


def magnitude(psi, **kwargs):
    """|psi_x| as a real state: map_states("abs", psi, ...)."""
    return map_states("abs", psi, **kwargs)


def log_power(psi, eps, **kwargs):
    """log(|psi_x|^2 + eps) as a real state (a spectrum in dB is 10 / ln 10 times it): map_states("log", psi, params=(eps,), ...)."""
    return map_states("log", psi, params=(eps,), **kwargs)


def shrink(psi, tau, **kwargs):
    """Soft thresholding psi_x max(0, 1 - tau / |psi_x|): map_states("shrink", psi, params=(tau,), ...)."""
    return map_states("shrink", psi, params=(tau,), **kwargs)


def divide(a, b, reg=0.0, **kwargs):
    """a_x conj(b_x) / (|b_x|^2 + reg); reg = 0 is the plain quotient a_x / b_x, which raises QilDomainError where a sampled
    b_x vanishes: map_states("divide", a, b, params=(reg,), ...)."""
    return map_states("divide", a, b, params=(reg,), **kwargs)


def deconvolve(y, h, reg=0.0, F=None, maxdim=None, tol=1e-12, map_tol=1e-10, map_maxdim=64):
    """The inverse of `convolve` in MPS form: x = (1 / sqrt(N)) F^dagger((F y) conj(F h) / (|F h|^2 + reg)), the x with
    convolve(x, h) = y when reg = 0 and F h vanishes nowhere.  The stages and the `F` handling are convolve's (F y, F h and
    F^dagger through apply_compress with `maxdim` and `tol`; F's bit reversal cancels between F and F^dagger); the quotient is
    divide(F y, F h, reg, tol=map_tol, maxdim=map_maxdim), a cross interpolation.

    As for convolve, the QFT MPO at its default cutoff 1e-14 is unitary only to 3e-9 (n = 6) ... 3e-7 (n = 10), and here that
    error is divided by min |F h|: the result matches the dense deconvolution to about 1e-7 max|F y| / min|F h| relative to
    the spectrum, whatever `tol` is.  Pass F = build_qft_mpo(y, cutoff=...) with a tighter cutoff for a tighter result, and
    reg > 0 where F h comes close to zero."""
    F = _spectral_operands(y, h, F, "deconvolve")
    Y = apply_compress(F, y, maxdim=maxdim, tol=tol)
    H = apply_compress(F, h, maxdim=maxdim, tol=tol)
    Q = divide(Y, H, reg, tol=map_tol, maxdim=map_maxdim)
    x = apply_compress(adjoint(F), Q, maxdim=maxdim, tol=tol)
    x.amplitude = x.amplitude / float(np.sqrt(2.0) ** len(y))
    return x


def _factor_out(m, n, r0, code):
    dt = _np_dtype(code)
    return (np.empty((m, r0), dtype=dt, order="F"), np.empty(r0, dtype=np.float64),
            np.empty(r0 * n, dtype=dt))


def rsvd(A, k=20, p=10, q=0, random_seed=1234, cutoff=1e-15, maxdim=None, mindim=1, ctx=None):
    """rsvd(A, Linds...; k, p, q, random_seed, cutoff, maxdim=k, mindim) on the matricised
    operand A (m x n).  Returns (U, S, Vh) with A ~= U diag(S) Vh."""
    ctx = ctx or default_context()
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] == 0 or A.shape[1] == 0:
        raise ValueError("In `rsvd`, left or right index set is empty.")
    code = L.QIL_C64 if np.iscomplexobj(A) else L.QIL_F64
    Af = np.asfortranarray(A, dtype=_np_dtype(code))
    m, n = Af.shape
    r0 = min(k + p, m, n)
    U, S, Vh = _factor_out(m, n, r0, code)
    r = C.c_int64()
    L.check(L.lib.qil_rsvd(ctx.handle, Af.ctypes.data_as(C.c_void_p), m, n, code, int(k), int(p), int(q),
                           C.c_uint64(random_seed), float(cutoff), int(k if maxdim is None else maxdim),
                           int(mindim), C.byref(r), U.ctypes.data_as(C.c_void_p),
                           S.ctypes.data_as(C.POINTER(C.c_double)), Vh.ctypes.data_as(C.c_void_p)))
    r = r.value
    return U[:, :r].copy(), S[:r].copy(), Vh[: r * n].reshape((r, n), order="F").copy()


def svd_trunc(A, cutoff=None, maxdim=None, mindim=1, ctx=None):
    """Truncated svd with the ITensors rule (keep largest; drop tail while the discarded squared
    weight <= cutoff * total; cap maxdim; floor mindim)."""
    ctx = ctx or default_context()
    A = np.asarray(A)
    code = L.QIL_C64 if np.iscomplexobj(A) else L.QIL_F64
    Af = np.asfortranarray(A, dtype=_np_dtype(code))
    m, n = Af.shape
    r0 = min(m, n)
    U, S, Vh = _factor_out(m, n, r0, code)
    r = C.c_int64()
    L.check(L.lib.qil_svd_trunc(ctx.handle, Af.ctypes.data_as(C.c_void_p), m, n, code,
                                -1.0 if cutoff is None else float(cutoff), _maxdim(maxdim), int(mindim),
                                C.byref(r), U.ctypes.data_as(C.c_void_p),
                                S.ctypes.data_as(C.POINTER(C.c_double)), Vh.ctypes.data_as(C.c_void_p)))
    r = r.value
    return U[:, :r].copy(), S[:r].copy(), Vh[: r * n].reshape((r, n), order="F").copy()


_OPS = {"N": 0, "T": 1, "H": 2, "C": 3}


def gemm(A, B, opA="N", opB="N", ctx=None):
    """op(A) @ op(B) on the GPU's f64 matrix cores (utility / test hook); op in N, T, H, C(onj)."""
    ctx = ctx or default_context()
    A, B = np.asarray(A), np.asarray(B)
    code = L.QIL_C64 if (np.iscomplexobj(A) or np.iscomplexobj(B)) else L.QIL_F64
    dt = _np_dtype(code)
    Af, Bf = np.asfortranarray(A, dtype=dt), np.asfortranarray(B, dtype=dt)
    m, k = (Af.shape if opA in "NC" else Af.shape[::-1])
    k2, n = (Bf.shape if opB in "NC" else Bf.shape[::-1])
    if k != k2:
        raise ValueError(f"gemm: inner dimensions disagree ({k} vs {k2})")
    Cm = np.empty((m, n), dtype=dt, order="F")
    L.check(L.lib.qil_gemm(ctx.handle, code, _OPS[opA], _OPS[opB], m, n, k, Af.ctypes.data_as(C.c_void_p),
                           Af.shape[0], Bf.ctypes.data_as(C.c_void_p), Bf.shape[0],
                           Cm.ctypes.data_as(C.c_void_p), m))
    return Cm


def gemm_plan(dtype, m, n, k, opA="N", opB="N", lda=None, ldb=None, ldc=None, count=1, c_bs=0, has_cmap=False,
              skinny_m=False):
    """What the MFMA GEMM's dispatch decides for this product (testing hook; needs no GPU): a dict of the fields of
    qil_gemm_plan_info.  Leading dimensions default to tight ones."""
    code = L.QIL_C64 if np.dtype(dtype) == np.complex128 else L.QIL_F64
    lda = (m if opA in "NC" else k) if lda is None else lda
    ldb = (k if opB in "NC" else n) if ldb is None else ldb
    ldc = m if ldc is None else ldc
    info = L.GemmPlanInfo()
    L.check(L.lib.qil_gemm_plan(code, _OPS[opA], _OPS[opB], int(m), int(n), int(k), int(lda), int(ldb), int(ldc),
                                int(count), int(c_bs), int(bool(has_cmap)), int(bool(skinny_m)), C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in info._fields_}


READOUT_VERBS = {"plain": 0, "marginal": 1, "sweep": 2, "lazy": 3}
READOUT_ROUTES = ("CHAIN", "GEMM_SELECT", "GEMM_SORTED", "LAZY_CHAIN", "LAZY_GEMM")


def readout_route(verb, nb, chain_dims, op_dims=None, dtype=np.float64):
    """Which code path a read-out call takes (testing hook; needs no GPU): qil_readout_route, the one host function
    coefficient_batch ("plain"), marginal_batch ("marginal"), apply_coefficient_sweep ("sweep") and apply_coefficient_batch
    ("lazy") switch on.  chain_dims: the n + 1 bond dimensions, edges included, of the chain that is read -- psi; for the sweep the
    product W psi, or psi together with op_dims; op_dims: the operator's (lazy: required).  dtype: complex128 when W or psi is
    complex.  Returns (route name, queries per pass): the second is smaller than nb only on LAZY_GEMM."""
    code = L.QIL_C64 if np.dtype(dtype) == np.complex128 else L.QIL_F64
    cd = np.ascontiguousarray(chain_dims, dtype=np.int64)
    od = None if op_dims is None else np.ascontiguousarray(op_dims, dtype=np.int64)
    if cd.ndim != 1 or cd.size < 2 or (od is not None and od.shape != cd.shape):
        raise ValueError("readout_route: bond dimensions are n + 1 entries per chain")
    route, per_pass = C.c_int(), C.c_int64()
    L.check(L.lib.qil_readout_route(READOUT_VERBS[verb], code, int(nb), cd.size - 1, cd.ctypes.data_as(C.POINTER(C.c_int64)),
                                    od.ctypes.data_as(C.POINTER(C.c_int64)) if od is not None else None,
                                    C.byref(route), C.byref(per_pass)))
    return READOUT_ROUTES[route.value], per_pass.value


def gemm_batched(A, B, Cbuf, m, n, k, opA="N", opB="N", a=(0, None, 0), b=(0, None, 0), c=(0, None, 0), count=1,
                 subtract=False, skinny_m=False, b_sel=None, b_sel_step=0, b_sel_stride=0, cmap=None, cmap_blk=1, ctx=None):
    """The batched / epilogue forms of the MFMA GEMM on host buffers (testing hook).  A, B, Cbuf are flat parent buffers of one
    dtype; a, b, c = (element offset, leading dimension, batch stride) of each operand inside its buffer.  Cbuf is uploaded whole,
    the product of batch i is written (or, with subtract, subtracted) at c_off + i * c_bs, and the whole buffer comes back in
    place; it is also returned."""
    ctx = ctx or default_context()
    code = L.QIL_C64 if Cbuf.dtype == np.complex128 else L.QIL_F64
    dt = _np_dtype(code)
    bufs = []
    for x in (A, B, Cbuf):
        if not (isinstance(x, np.ndarray) and x.ndim == 1 and x.dtype == dt and x.flags.c_contiguous):
            raise ValueError("gemm_batched: operands are flat contiguous arrays of the output's dtype")
        bufs.append(x)
    tight = ((m if opA in "NC" else k), (k if opB in "NC" else n), m)
    ops_ = []
    for x, (off, ld, bs), t in zip(bufs, (a, b, c), tight):
        ops_.append(L.GemmHostOperand(x.ctypes.data, x.size, int(off), int(t if ld is None else ld), int(bs)))
    sel = mp = None
    if b_sel is not None:
        sel = np.ascontiguousarray(b_sel, dtype=np.uint8)
        if sel.size < (count - 1) * b_sel_step + 1:
            raise ValueError("gemm_batched: b_sel is shorter than (count - 1) * b_sel_step + 1")
    if cmap is not None:
        mp = np.ascontiguousarray(cmap, dtype=np.int32)
        if cmap_blk < 1 or mp.size < count * (n // cmap_blk):
            raise ValueError("gemm_batched: cmap is shorter than count * n / cmap_blk")
    L.check(L.lib.qil_gemm_batched_host(
        ctx.handle, code, _OPS[opA], _OPS[opB], int(m), int(n), int(k), C.byref(ops_[0]), C.byref(ops_[1]), C.byref(ops_[2]),
        int(count), int(bool(subtract)), int(bool(skinny_m)),
        sel.ctypes.data_as(C.POINTER(C.c_uint8)) if sel is not None else None, int(b_sel_step), int(b_sel_stride),
        mp.ctypes.data_as(C.POINTER(C.c_int32)) if mp is not None else None, int(cmap_blk)))
    return Cbuf


QR_ROUTES = ("SINGLE_CGS2", "SINGLE_HH", "SINGLE_TREE", "BLOCKED")
QR_PANELS = ("NONE", "HH", "TREE", "CGS2_LDS", "CGS2_GLOBAL")


def _qr_plan_dict(info):
    d = {name: int(getattr(info, name)) for name, _ in info._fields_}
    d["route"] = QR_ROUTES[d["route"]]
    d["panel_kind"], d["last_panel_kind"] = QR_PANELS[d["panel_kind"]], QR_PANELS[d["last_panel_kind"]]
    return d


def qr_plan(dtype, m, n):
    """What the thin QR decides for an m x n operand (testing hook; needs no GPU): a dict of the fields of qil_qr_plan_info, the
    route and the panel kinds by name (QR_ROUTES, QR_PANELS)."""
    code = L.QIL_C64 if np.dtype(dtype) == np.complex128 else L.QIL_F64
    info = L.QrPlanInfo()
    L.check(L.lib.qil_qr_plan(code, int(m), int(n), C.byref(info)))
    return _qr_plan_dict(info)


def qr_host(A, m, n, a=(0, None), R=None, r=(0, None), reorth=False, cholesky_skip=0, ctx=None):
    """The thin QR with non-negative diagonal on host buffers (testing hook).  A (and R, optional) are flat parent buffers of one
    dtype; a, r = (element offset, leading dimension) of the m x n operand and of the n x n factor inside them.  Both buffers are
    uploaded whole and come back in place, Q where the operand was.  reorth: measure Q^H Q and factor again while it is off;
    cholesky_skip: CholeskyQR2 attempts to skip.  Returns the fields of qil_qr_report as a dict ("plan": as qr_plan returns it)."""
    ctx = ctx or default_context()
    code = L.QIL_C64 if A.dtype == np.complex128 else L.QIL_F64
    for x in (A,) if R is None else (A, R):
        if not (isinstance(x, np.ndarray) and x.ndim == 1 and x.dtype == _np_dtype(code) and x.flags.c_contiguous):
            raise ValueError("qr_host: operands are flat contiguous arrays of one dtype (float64 or complex128)")
    rep = L.QrReport()
    L.check(L.lib.qil_qr_host(ctx.handle, code, int(m), int(n), A.ctypes.data, A.size, int(a[0]), int(m if a[1] is None else a[1]),
                              None if R is None else R.ctypes.data, 0 if R is None else R.size, int(r[0]),
                              int(n if r[1] is None else r[1]), int(bool(reorth)), int(cholesky_skip), C.byref(rep)))
    return {"plan": _qr_plan_dict(rep.plan), "cholesky": rep.cholesky, "repairs": rep.repairs, "passes": rep.passes,
            "skipped_check": rep.skipped_check, "worst": [float(w) for w in rep.worst]}


def gemm_device_time(m, n, k, dtype=np.float64, opA="N", opB="N", reps=10, ctx=None):
    """ms per call of the device-resident MFMA GEMM (diagnostic)."""
    ctx = ctx or default_context()
    code = L.QIL_C64 if np.dtype(dtype) == np.complex128 else L.QIL_F64
    ms = C.c_double()
    L.check(L.lib.qil_gemm_device_time(ctx.handle, code, _OPS[opA], _OPS[opB], int(m), int(n), int(k),
                                       int(reps), C.byref(ms)))
    return ms.value


def qr_positive(A, ctx=None):
    """Thin QR with non-negative diagonal of R (the device Gram-Schmidt QR; utility / test hook)."""
    ctx = ctx or default_context()
    A = np.asarray(A)
    code = L.QIL_C64 if np.iscomplexobj(A) else L.QIL_F64
    Af = np.asfortranarray(A, dtype=_np_dtype(code))
    m, n = Af.shape
    Q = np.empty((m, n), dtype=Af.dtype, order="F")
    R = np.empty((n, n), dtype=Af.dtype, order="F")
    L.check(L.lib.qil_qr_positive(ctx.handle, code, m, n, Af.ctypes.data_as(C.c_void_p),
                                  Q.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p)))
    return Q, R
