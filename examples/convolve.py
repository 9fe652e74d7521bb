#!/usr/bin/env python3
"""Smoothing a signal by circular convolution, entirely in MPS form: transform, multiply, transform back.

    python examples/convolve.py

A noisy-looking signal on N = 2^20 samples (two tones under a slow envelope) and a decaying-exponential kernel are encoded
into MPS.  `convolve` takes both through the QFT MPO, multiplies the spectra element-wise (`hadamard_compress`), applies the
adjoint of the QFT MPO -- the inverse transform -- and returns y = x (*) h as an MPS.  The result is compared with numpy's FFT
convolution on sampled points.  The QFT MPO at its default cutoff is unitary to a few 1e-7, and that is the accuracy of the
round trip; build it with a tighter `cutoff` for more."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402


def main():
    n = 20
    N = 2 ** n
    t = np.arange(N) / N
    x = np.cos(2 * np.pi * 5 * t) * np.exp(-3 * t) + 0.3 * np.sin(2 * np.pi * 1700 * t)
    h = np.exp(-400 * t)
    h /= h.sum()                                               # a one-sided exponential smoother, tau = N / 400 samples
    px, ph = qil.signal_mps(x), qil.signal_mps(h)
    F = qil.build_qft_mpo(px)
    t0 = time.perf_counter()
    y = qil.convolve(px, ph, F=F, tol=1e-10)
    dt = time.perf_counter() - t0
    print(f"N = 2^{n}: bonds x {max(px.bond_dims)}, h {max(ph.bond_dims)}, QFT {max(F.bond_dims)} -> y {max(y.bond_dims)}"
          f"  ({dt * 1e3:.1f} ms)")
    ref = np.fft.ifft(np.fft.fft(x) * np.fft.fft(h)).real
    idx = np.random.default_rng(0).integers(0, N, size=4096)
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    got = qil.coefficient_batch(y, bits)
    dev = np.abs(got - ref[idx]).max() / np.abs(ref).max()
    print(f"against np.fft on {len(idx)} sampled points: max deviation {dev:.2e} of max|y|")
    fast = 0.3 * np.abs(np.fft.fft(ref)[1700]) / np.abs(np.fft.fft(x)[1700])
    print(f"the fast tone (bin 1700) is damped to {fast / 0.3:.3f} of its amplitude; the slow one passes")
    return dev


if __name__ == "__main__":
    main()
