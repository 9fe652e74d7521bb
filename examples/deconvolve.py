#!/usr/bin/env python3
"""Undoing a blur, entirely in MPS form: transform, divide, transform back.

    python examples/deconvolve.py

A three-mode signal on N = 2^12 samples is blurred by a short FIR kernel (h = delta_0 + 0.5 delta_1 + 0.25 delta_2, circular
convolution through `convolve`).  `deconvolve` takes the blurred signal and the kernel through the QFT MPO, divides the spectra
element-wise -- a cross interpolation of (F y) / (F h) whose samples are read from the two states on the device (`divide`) --
and applies the adjoint of the QFT MPO.  The error against the input and the bonds of every stage are printed.  The QFT MPO at
its default cutoff is unitary to a few 1e-7, and here that defect is divided by min |F h|; a tighter `cutoff` of build_qft_mpo
buys a tighter round trip."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402


def main():
    n = 12
    N = 2 ** n
    k = np.arange(N, dtype=np.float64)
    modes = [(1.0, np.exp(-2e-4 + 0.31j)), (0.5 - 0.2j, np.exp(-1e-3 - 1.1j)), (0.25j, np.exp(-5e-4 + 2.3j))]
    x = sum(a * z ** k for a, z in modes)
    h = np.zeros(N)
    h[:3] = [1.0, 0.5, 0.25]
    px, ph = qil.signal_mps(x), qil.signal_mps(h)
    F = qil.build_qft_mpo(px, cutoff=1e-20)
    py = qil.convolve(px, ph, F=F)
    t0 = time.perf_counter()
    back = qil.deconvolve(py, ph, F=F, map_tol=1e-10)
    dt = time.perf_counter() - t0
    print(f"N = 2^{n}: bonds x {max(px.bond_dims)}, h {max(ph.bond_dims)}, y {max(py.bond_dims)}, QFT {max(F.bond_dims)}"
          f" -> deconvolved {max(back.bond_dims)}  ({dt * 1e3:.1f} ms)")
    got = qil.mps_to_vector(back)
    err = np.abs(got - x).max() / np.abs(x).max()
    blur = np.abs(qil.mps_to_vector(py) - x).max() / np.abs(x).max()
    print(f"blurred signal against the input: max deviation {blur:.2e} of max|x|")
    print(f"deconvolved signal against the input: max deviation {err:.2e} of max|x|")
    return err


if __name__ == "__main__":
    main()
