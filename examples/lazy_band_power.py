#!/usr/bin/env python3
"""Where is the energy of W psi -- without forming W psi?  Band powers, the median frequency and the row energies of a z-plane,
read from the operator and the state as they are: `apply_range_weight`, `apply_weight_quantiles` and `apply_zt_row_weights` on
top of `apply_weight_batch`, the lazy form of the Born weights of `examples/band_power.py`.

    python examples/lazy_band_power.py

The product W psi has the bond chi * D; when that does not fit, `weight_batch(apply(W, psi))` is not available and these calls
are.  A sum of three damped complex exponentials is built directly as an MPS and NOT transformed: the QFT MPO goes into every
call next to it.  A band splits into at most 2n dyadic blocks -- a fixed prefix, the rest traced -- and each block costs a lazy
coefficient step per fixed tensor plus one quadratic form with a right environment that all blocks share.  The QFT output holds
the bin index with the first tensor as its least significant bit, hence reverse=True, which turns the blocks into traced-then-
fixed rows: those walk the density through the chain.  The last part reads the energy of damping rows of a z-plane from the
signal's ZTMPS and the zT operator.  Everything here is small (n <= 12 tensors per register), and every printed figure is
checked in the script against `weight_batch(apply(W, psi))`, the materialised way to the same number."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

TOL = 1e-10                                            # of the total weight, against the materialised product


def spectrum_part():
    n = 12
    N = 2 ** n
    modes = [(250.3, 8e-5, 1.0), (1250.7, 4e-4, 0.8), (3000.5, 2e-4, 0.5)]             # (bin, damping per sample, amplitude)
    zs = [np.exp(-g + 2j * np.pi * f / N) for f, g, _ in modes]
    psi = qil.exponential_sum([a for _, _, a in modes], zs, n)
    W = qil.build_qft_mpo(psi)
    out = W * psi                                                                      # checks only
    trace = np.full(n, qil.ops.TRACE)
    total = qil.apply_weight(W, psi, trace)
    assert abs(total - qil.weight(out, trace)) <= TOL * total
    print(f"three damped modes, N = 2^{n}; state bonds up to {max(psi.bond_dims)}, operator bonds up to {max(W.bond_dims)}, "
          f"total energy of W psi {total:.6e}")
    results = {}
    for f, _, _ in modes:
        lo, hi = int(f) - 40, int(f) + 41
        p = qil.apply_range_weight(W, psi, lo, hi, reverse=True)
        assert abs(p - qil.range_weight(out, lo, hi, reverse=True)) <= TOL * total, (lo, hi)
        print(f"   band [{lo:5d}, {hi:5d}) around bin {f:8.1f}: power {p:.6e}  = {100 * p / total:6.2f} % of the total")
        results[f] = p
    qs = [0.5, 0.95]
    med, edge = (int(v) for v in qil.apply_weight_quantiles(W, psi, qs, reverse=True))
    assert [med, edge] == [int(v) for v in qil.weight_quantiles(out, qs, reverse=True)]
    print(f"   median frequency: bin {med};  95 % of the energy lies at or below bin {edge}")
    probs = qil.apply_bit_probabilities(W, psi)
    assert np.abs(probs - qil.bit_probabilities(out)).max() <= TOL
    print(f"   P(most significant bin bit = 1) = {probs[n - 1]:.4f}: the share of the energy in the upper half of the spectrum")
    results["median"], results["edge95"] = med, edge
    return results


def zplane_part():
    n = 8
    N = 2 ** n
    j = np.arange(N)
    x = 0.98 ** j * np.cos(0.4 * j) + 0.5 * 0.995 ** j * np.cos(1.3 * j)
    psi = qil.signal_ztmps(x)
    W = qil.build_zt_mpo(psi, 0.5)
    ls = np.arange(0, N, N // 16)
    rows = qil.apply_zt_row_weights(W, psi, ls)                                        # sum_k |Z(k, l)|^2: one call, no product
    phi = W * psi                                                                      # checks only
    ref = qil.zt_row_weights(phi, ls)
    total = qil.weight(phi, np.full(2 * n, qil.ops.TRACE))
    assert np.abs(rows - ref).max() <= TOL * total
    best = np.argsort(rows)[::-1][:4]
    print(f"two-pole signal, N = 2^{n}: {len(ls)} damping rows of the z-plane, total energy {total:.6e}")
    print("   strongest of them: " + ", ".join(f"l = {int(ls[i])} ({100 * rows[i] / total:.2f} %)" for i in best))
    return rows


def main():
    return spectrum_part(), zplane_part()


if __name__ == "__main__":
    main()
