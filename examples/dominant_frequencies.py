#!/usr/bin/env python3
"""The dominant bins of a QFT spectrum, found without reading the spectrum: top_k on the transformed MPS.

    python examples/dominant_frequencies.py

A signal of four complex tones on N = 2^20 samples is encoded into an MPS and the QFT MPO is applied.  `top_k` then searches
the 2^20 bins for the largest |coefficients| by a beam search over prefix weights on the device, and reports whether its bound
certifies that nothing larger was missed.  The QFT output holds bin k with its bits in reverse order (lsb first), so the index
that top_k returns is k bit-reversed."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402


def main():
    n = 20
    N = 2 ** n
    t = np.arange(N)
    tones = [(5, 1.0), (4321, 0.7), (99999, 0.45), (700000, 0.2)]
    x = sum(a * np.exp(2j * np.pi * k * t / N) for k, a in tones)
    psi = qil.signal_mps(x, cutoff=1e-15)
    out = qil.build_qft_mpo(psi) * psi
    print(f"signal of {len(tones)} tones, N = 2^{n}; QFT output bonds up to {max(out.bond_dims)}")
    rev = lambda j: int(format(int(j), f"0{n}b")[::-1], 2)
    for k, beam in ((4, 64), (6, 64)):
        t0 = time.perf_counter()
        idx, vals, bound, cert = qil.top_k(out, k, beam=beam)
        dt = time.perf_counter() - t0
        print(f"top_k(k={k}, beam={beam}): bound {bound:.3e}, certified {cert}  ({dt * 1e3:.1f} ms)")
        for j, v in zip(idx, vals):
            print(f"   bin {rev(j):7d}   |X| / sqrt(N) = {abs(v) / np.sqrt(N):.6f}")
    return idx, vals, bound, cert


if __name__ == "__main__":
    main()
