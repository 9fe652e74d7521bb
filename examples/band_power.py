#!/usr/bin/env python3
"""Where is the energy?  Band powers, the median frequency and the row energies of a z-plane, read from the MPS as numbers --
`range_weight`, `weight_quantiles` and `zt_row_weights` on top of `weight_batch` (Born weights: sums of |psi_x|^2, where
every other read-out returns amplitudes).

    python examples/band_power.py

A sum of three damped complex exponentials is built directly as an MPS (`exponential_sum`: no dense vector) and transformed by
the QFT MPO.  The power in a band around each mode is one `range_weight` call: the band splits into at most 2n dyadic blocks
(high bits of the bin index fixed, low bits traced), one row of `weight_batch` each.  The QFT output holds the bin index with
the first tensor as its least significant bit, hence reverse=True.  `weight_quantiles` descends the bits for the median
frequency and the 95 % edge.  The last part transforms a short two-pole signal to its z-plane and prints the energy of every
damping row l, sum_k |Z(k, l)|^2, from ONE call.  Everything here is small enough (n <= 16 tensors) for the dense vector, and
every printed figure is checked against it in the script; the calls themselves do not change at n = 40."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

TOL = 1e-10                                            # of the total weight, against the dense vector


def spectrum_part():
    n = 14
    N = 2 ** n
    modes = [(1000.3, 2e-5, 1.0), (5000.7, 1e-4, 0.8), (12000.5, 5e-5, 0.5)]          # (bin, damping per sample, amplitude)
    zs = [np.exp(-g + 2j * np.pi * f / N) for f, g, _ in modes]
    psi = qil.exponential_sum([a for _, _, a in modes], zs, n)
    out = qil.build_qft_mpo(psi) * psi
    dense = np.abs(qil.mps_to_vector(out, reverse=True)) ** 2                          # bin order; checks only
    total = qil.weight(out, np.full(n, qil.ops.TRACE))
    assert abs(total - dense.sum()) <= TOL * dense.sum()
    print(f"three damped modes, N = 2^{n}; QFT output bonds up to {max(out.bond_dims)}, total energy {total:.6e}")
    results = {}
    for f, _, _ in modes:
        lo, hi = int(f) - 40, int(f) + 41
        p = qil.range_weight(out, lo, hi, reverse=True)
        assert abs(p - dense[lo:hi].sum()) <= TOL * total, (lo, hi)
        print(f"   band [{lo:5d}, {hi:5d}) around bin {f:8.1f}: power {p:.6e}  = {100 * p / total:6.2f} % of the total")
        results[f] = p
    qs = [0.5, 0.95]
    med, edge = (int(v) for v in qil.weight_quantiles(out, qs, reverse=True))
    want = np.searchsorted(np.cumsum(dense), np.array(qs) * dense.sum(), side="left")
    assert [med, edge] == [int(v) for v in want], ([med, edge], want)
    print(f"   median frequency: bin {med};  95 % of the energy lies at or below bin {edge}")
    probs = qil.bit_probabilities(out)
    top = np.array([dense[(np.arange(N) >> i) & 1 == 1].sum() for i in range(n)]) / dense.sum()
    assert np.abs(probs - top).max() <= TOL
    print(f"   P(most significant bin bit = 1) = {probs[n - 1]:.4f}: the share of the energy in the upper half of the spectrum")
    results["median"], results["edge95"] = med, edge
    return results


def zplane_part():
    n = 8
    N = 2 ** n
    j = np.arange(N)
    x = 0.98 ** j * np.cos(0.4 * j) + 0.5 * 0.995 ** j * np.cos(1.3 * j)
    psi = qil.signal_ztmps(x)
    phi = qil.build_zt_mpo(psi, 0.5) * psi
    idx = np.arange(N)
    rows = qil.zt_row_weights(phi, idx)                                                # sum_k |Z(k, l)|^2 for every l: one call
    cols = qil.zt_column_weights(phi, idx)
    grid = np.abs(qil.coefficient_grid(phi, idx, idx)) ** 2                            # checks only
    total = grid.sum()
    assert np.abs(rows - grid.sum(axis=0)).max() <= TOL * total
    assert np.abs(cols - grid.sum(axis=1)).max() <= TOL * total
    best = np.argsort(rows)[::-1][:4]
    print(f"two-pole signal, N = 2^{n}: z-plane of {N} x {N} points, total energy {total:.6e}")
    print("   strongest rows l: " + ", ".join(f"{int(l)} ({100 * rows[l] / total:.2f} %)" for l in best))
    print(f"   strongest column k: {int(np.argmax(cols))} ({100 * cols.max() / total:.2f} %)")
    return rows, cols


def main():
    return spectrum_part(), zplane_part()


if __name__ == "__main__":
    main()
