#!/usr/bin/env python3
"""Unitary propagation on 2^40 samples: exp(-i t H) x with H = L + diag(V) by two-site TDVP, without a dense object.

    python examples/propagate.py

x is a Gaussian pulse on a carrier (the envelope encoded by `signal_mps_cross`, the carrier an exact bond-1 `exponential_mps`,
multiplied by `hadamard`), L the periodic second difference (`build_laplacian_mpo`), V(s) = 0.5 cos(2 pi s) a slow potential
(`exponential_sum`, turned into an operator by `diagonal_mpo`).  `propagate` keeps the norm and the energy <x|H|x>: both are
printed before and after, through `norm` and `inner`.  For the free case H = L a Fourier mode is an eigenvector, so its evolved
read-out has a closed form, exp(-i t lambda) x_j with lambda = 2 - 2 cos(2 pi f / N).

`evolve` is for |Re tau| * spread(A) of order one per step and for any imaginary tau (THE STIFF LIMIT, README); strong smoothing
stays with `smooth`, and circulant operators also have the Fourier route."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

N_SITES, T, STEPS = 40, 3.0, 3
MODE = int(round(0.3 * 2 ** N_SITES))


def operands(n=N_SITES):
    scale = 1.0 / float(2 ** n)
    envelope = qil.signal_mps_cross(lambda idx: torch.exp(-0.5 * ((idx.to(torch.float64) * scale - 0.4) / 0.08) ** 2), n=n,
                                    maxdim=32, tol=1e-10)
    carrier = qil.exponential_mps(np.exp(2j * np.pi * (MODE / 2.0 ** n)), n)
    x = qil.hadamard(envelope, carrier)
    x.amplitude = 1.0 / qil.norm(x)
    z = np.exp(2j * np.pi * scale)
    V = qil.exponential_sum([0.25, 0.25], [z, np.conj(z)], n, maxdim=None, tol=None)
    lap = qil.build_laplacian_mpo(x)
    H = qil.mpo_linear_combination([lap, qil.diagonal_mpo(V)], [1.0, 1.0])
    return x, lap, H


def energy(H, x):
    return float(np.real(qil.inner(x, H, x))) / (x.amplitude * qil.norm(x)) ** 2


def main(n=N_SITES):
    x, lap, H = operands(n)
    print(f"2^{n} samples, pulse bonds up to {max(x.bond_dims)}, H = L + diag(V) of bond {max(H.bond_dims)}")
    print(f"   before: norm {x.amplitude * qil.norm(x):.12f}  <x|H|x> {energy(H, x):.12f}")
    t0 = time.perf_counter()
    y, info = qil.propagate(H, x, T, steps=STEPS, maxdim=32, cutoff=1e-20, tol=1e-10, return_info=True)
    dt = time.perf_counter() - t0
    print(f"   after t = {T:g} in {STEPS} steps ({dt * 1e3:.0f} ms, {info['matvecs']} matvecs, bonds up to {info['max_bond']}, "
          f"local / gemm exponentials {info['local_exps']} / {info['gemm_exps']}, converged {info['converged']}):")
    print(f"           norm {y.amplitude * qil.norm(y):.12f}  <x|H|x> {energy(H, y):.12f}")

    # the free case on one mode: the closed form
    mode = qil.exponential_mps(np.exp(2j * np.pi * (MODE / 2.0 ** n)), n)
    lam = 2.0 - 2.0 * np.cos(2.0 * np.pi * (MODE / 2.0 ** n))
    free = qil.propagate(lap, mode, T, steps=STEPS)
    idx = np.random.default_rng(3).integers(0, 2 ** n, size=6, dtype=np.int64)
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    got, want = qil.coefficient_batch(free, bits), np.exp(-1j * T * lam) * qil.coefficient_batch(mode, bits)
    for j, g, w in zip(idx, got, want):
        print(f"   free mode, x[{int(j)}] = {g:+.12f}   closed form {w:+.12f}")
    err = float(np.abs(got - want).max())
    print(f"   worst distance from the closed form: {err:.2e}")
    return {"info": info, "free_error": err, "norm": y.amplitude * qil.norm(y), "energy": (energy(H, x), energy(H, y))}


if __name__ == "__main__":
    main()
