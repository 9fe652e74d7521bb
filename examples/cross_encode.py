#!/usr/bin/env python3
"""Encode a signal of 2^40 samples that never exists as a vector: `signal_mps_cross` on a callable, then `ztmps_from_mps` and a
read-out.

    python examples/cross_encode.py

The signal is a chirp under a Gaussian envelope, x(t) = exp(-((t - 0.4) / 0.08)^2 / 2) cos(2 pi (5 t + 20 t^2)), t = k / 2^40.
`signal_mps_cross` asks the callable for the samples it wants -- some ten thousand of the 1.1e12 -- and builds the MPS by pivoted
LU factorisations of small two-site blocks.  The callable works in t = k / N: multiplying a phase by a raw index of this size
costs seven digits, and the lost digits come back as rank.  The result enters the z-transform pipeline through `ztmps_from_mps`
(the paired chain `signal_ztmps` would build), and `coefficient_batch` reads both chains at random positions.

The known blind spot of cross interpolation: a feature that no pivot's row or column touches -- an isolated spike -- is invisible,
and the error estimate does not see it either.  Pass the index of such a feature in `seeds`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

N_SITES = 40
TOL = 1e-9


def signal(t):
    """x(t) for numpy arrays and torch tensors alike."""
    lib = torch if isinstance(t, torch.Tensor) else np
    return lib.exp(-0.5 * ((t - 0.4) / 0.08) ** 2) * lib.cos(2 * np.pi * (5 * t + 20 * t * t))


def main():
    n = N_SITES
    scale = 1.0 / float(2 ** n)
    psi, info = qil.signal_mps_cross(lambda idx: signal(idx.to(torch.float64) * scale), n=n, maxdim=64, tol=TOL, return_info=True)
    print(f"2^{n} = {2 ** n:.3e} samples, samples read: {info['nevals']} ({info['sweeps']} sweep(s), converged: {bool(info['converged'])})")
    print(f"   bonds {psi.bond_dims}")
    print(f"   estimate {info['est']:.2e} of max|x|, amplitude (= |x|_2) {psi.amplitude:.6e}")

    # the signal at random positions, from the chain
    idx = np.random.default_rng(3).integers(0, 2 ** n, size=1000, dtype=np.int64)
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    want = signal(idx.astype(np.float64) * scale)
    err = np.abs(qil.coefficient_batch(psi, bits) - want).max()
    print(f"   max error at 1000 random samples: {err:.2e} (bound n tol = {n * TOL:.1e})")
    assert info["converged"] and err <= n * TOL

    # ... into the z-transform pipeline: the paired chain (main_i, copy_i), which holds x on its diagonal k = l
    # (the cut-off acts on the unit-norm chain and the amplitude is |x|_2 ~ 3e5 here: 1e-30 keeps the split exact to 1e-9)
    zt = qil.ztmps_from_mps(psi, cutoff=1e-30)
    paired = np.repeat(bits, 2, axis=1)                    # main_i = copy_i = bit i
    zerr = np.abs(qil.coefficient_batch(zt, paired) - want).max()
    off = paired.copy()
    off[:, 1] ^= 1                                         # k and l differ in their first bit: off the diagonal
    print(f"ZTMPS of {zt.ntensors} tensors, bonds up to {max(zt.bond_dims)}: diagonal error {zerr:.2e}, "
          f"largest off-diagonal entry {np.abs(qil.coefficient_batch(zt, off)).max():.1e}")
    assert zerr <= n * TOL + 1e-8


if __name__ == "__main__":
    main()
