#!/usr/bin/env python3
"""Which tones dominate QFT psi -- without forming QFT psi, and without drawing samples?  `apply_top_k` runs the beam search of
`top_k` on the operator and the state as they are: it returns the k configurations with the largest |(W psi)_x|, their exact
values, and a bound on anything the search may have dropped.  When the bound lies below the k-th value the answer is certified
to be the exact top-k.

    python examples/lazy_top_k.py

Three damped modes, built directly as an MPS (`exponential_sum`) and NOT transformed; the QFT MPO goes into the call next to it.
The three largest bins are the three tones.  The call keeps the right environments of |W psi|^2 (the sum of (chi D)^2 over the
bonds) instead of the product.  Everything here is small, and every printed figure is checked in the script against
`top_k(apply(W, psi))` on the materialised product."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402


def main():
    n = 12
    N = 2 ** n
    modes = [(250.0, 8e-5, 1.0), (1250.0, 4e-4, 0.8), (3000.0, 2e-4, 0.5)]                 # (bin, damping per sample, amplitude)
    psi = qil.exponential_sum([a for _, _, a in modes], [np.exp(-g + 2j * np.pi * f / N) for f, g, _ in modes], n)
    W = qil.build_qft_mpo(psi)
    k, beam = 3, 64
    rows, values, bound, certified = qil.apply_top_k(W, psi, k, beam=beam, bits=True)
    bins = rows.astype(np.int64) @ (1 << np.arange(n))                                 # the QFT output holds the bin lsb first
    print(f"three damped modes, N = 2^{n}: the {k} largest |X| of QFT psi, beam {beam}, product never formed")
    for b, v in zip(bins, values):
        print(f"   bin {int(b):5d}: |X| = {abs(v):.6e}")
    print(f"   dropped prefixes hold at most {bound:.3e}: the result is {'certified exact' if certified else 'not certified'}")
    # checks only: the same search on the materialised product, and the lazy coefficient read-out on the rows found
    frows, fvalues, fbound, fcertified = qil.top_k(W * psi, k, beam=beam, bits=True)
    assert np.array_equal(rows, frows) and certified == fcertified
    assert np.abs(values - fvalues).max() <= 1e-10 * np.abs(fvalues).max()
    assert abs(bound - fbound) <= 1e-9 * max(fbound, np.abs(fvalues).min())
    coeff = qil.apply_coefficient_batch(W, psi, rows)
    assert np.abs(values - coeff).max() <= 1e-10 * np.abs(coeff).max()
    return sorted(int(b) for b in bins), certified


if __name__ == "__main__":
    main()
