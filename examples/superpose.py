#!/usr/bin/env python3
"""A three-mode damped signal on 2^30 samples built without a dense vector, and one mode subtracted from it.

    python examples/superpose.py

A sum of K complex exponentials a_k z_k^j is an exact MPS of bond <= K (`exponential_sum`: K bond-1 states added on the
device).  At n = 16, where the dense vector still fits, the same signal is also sampled and encoded with `signal_mps`, and the
`distance` of the two states is printed.  At n = 30 the QFT of the signal is searched with `top_k` before and after one mode
is subtracted (`-`): the dominant bins move from the strongest mode to the next one."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402


def modes(n):
    """three damped modes with frequencies on the FFT grid; the damping is a few e-folds over the record"""
    N = 2 ** n
    freqs, damps, amps = (5, 17, 40), (1.0, 3.0, 0.5), (1.0, 0.6, 0.3)
    zs = [complex(np.exp(-g / N + 2j * np.pi * f / N)) for f, g in zip(freqs, damps)]
    return zs, list(amps), freqs


def main():
    # (a) where both fit: the sum of exponentials against the sampled, encoded signal
    n = 16
    zs, amps, _ = modes(n)
    j = np.arange(2 ** n)
    x = sum(a * z ** j for a, z in zip(amps, zs))
    built, encoded = qil.exponential_sum(amps, zs, n), qil.signal_mps(x)
    rel = qil.distance(built, encoded) / (encoded.amplitude * qil.norm(encoded))
    print(f"n = {n}: exponential_sum bonds {max(built.bond_dims)}, signal_mps bonds {max(encoded.bond_dims)}, "
          f"relative distance {rel:.2e}")
    # (b) n = 30: no dense vector anywhere
    n = 30
    zs, amps, freqs = modes(n)
    x = qil.exponential_sum(amps, zs, n)
    F = qil.build_qft_mpo(n)
    rows, vals, _, certified = qil.top_k(qil.apply_compress(F, x, tol=1e-10), k=3, bits=True)
    print(f"n = {n}: bonds {max(x.bond_dims)}; top-3 |QFT| {np.abs(vals).round(1)} (certified: {certified})")
    strongest = qil.scale(qil.exponential_mps(zs[0], n), amps[0])
    y = qil.compress(x - strongest, tol=1e-12)
    rows2, vals2, _, certified2 = qil.top_k(qil.apply_compress(F, y, tol=1e-10), k=3, bits=True)
    print(f"after subtracting the mode at bin {freqs[0]}: bonds {max(y.bond_dims)}; top-3 |QFT| {np.abs(vals2).round(1)} "
          f"(certified: {certified2})")
    return rel, np.abs(vals), np.abs(vals2)


if __name__ == "__main__":
    main()
