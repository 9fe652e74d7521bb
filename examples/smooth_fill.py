#!/usr/bin/env python3
"""Smoothing and gap filling on 2^40 samples: the Whittaker smoother as a linear solve in MPS form.

    python examples/smooth_fill.py

A real signal of two slow tones (four complex modes, `exponential_sum`) plus a rough low-bond disturbance, in a record of 2^40
samples; a mask hides two of every eight samples.  `smooth(y, alpha, mask=mask)` minimises |M (x - y)|^2 + alpha |Delta x|^2, i.e.
solves (M + alpha L) x = M y with L = 2 I - S - S^dagger (`build_laplacian_mpo`) by `solve`, without ever touching 2^40 numbers.
The result is read at a few indices, hidden ones among them, next to the clean signal."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

N40, ALPHA, NOISE = 40, 4.0, 0.05
FREQS, AMPS = (1.0 / 4096, 1.0 / 55000.7), (1.0, 0.6)
HIDDEN = (5, 6)                                     # x mod 8 in HIDDEN is not observed


def clean_modes():
    zs = [complex(np.cos(2 * np.pi * s * f), np.sin(2 * np.pi * s * f)) for f in FREQS for s in (1, -1)]
    return zs, [a / 2 for a in AMPS for _ in (1, -1)]


def clean_value(j):
    return sum(a * np.cos(2 * np.pi * ((f * j) % 1.0)) for f, a in zip(FREQS, AMPS))


def mask_tensors(n):
    """1 where x mod 8 is observed: ones on the upper n - 3 tensors, the 8 values on the last three"""
    v = np.ones(8)
    v[list(HIDDEN)] = 0.0
    U, S, Vh = np.linalg.svd(v.reshape(2, 4), full_matrices=False)
    r = int(np.sum(S > 1e-14))
    a = (U[:, :r] * S[:r]).reshape(1, 2, r)
    U2, S2, Vh2 = np.linalg.svd(Vh[:r].reshape(r * 2, 2), full_matrices=False)
    r2 = int(np.sum(S2 > 1e-14))
    return [np.ones((1, 2, 1))] * (n - 3) + [a, (U2[:, :r2] * S2[:r2]).reshape(r, 2, r2), Vh2[:r2].reshape(r2, 2, 1)]


def operands(n=N40, seed=11):
    zs, amps = clean_modes()
    clean = qil.exponential_sum(amps, zs, n, maxdim=None, tol=None)
    rough = qil.SignalMPS.alloc([min(4, 2 ** min(i + 1, n - 1 - i)) for i in range(n - 1)], dtype=np.float64).fill_random(seed)
    rough.amplitude = NOISE * 2.0 ** (n / 2) / qil.norm(rough)            # NOISE per sample, root mean square
    y = qil.linear_combination_compress([clean, rough], [1.0, 1.0], maxdim=None, tol=1e-13)
    return y, qil.SignalMPS(mask_tensors(n)), clean


def run(y, mask, **kw):
    return qil.smooth(y, ALPHA, mask=mask, maxdim=32, cutoff=1e-18, tol=1e-8, return_info=True, **kw)


def bits_of(idx, n):
    return np.array([[(int(j) >> (n - 1 - i)) & 1 for i in range(n)] for j in idx], dtype=np.uint8)


def main(n=N40):
    y, mask, clean = operands(n)
    t0 = time.perf_counter()
    x, info = run(y, mask)
    dt = time.perf_counter() - t0
    print(f"smooth with a mask, n = {n}, alpha = {ALPHA:g}: {dt * 1e3:.1f} ms, {info['sweeps']} sweeps, {info['matvecs']} matvecs, "
          f"bonds y {max(y.bond_dims)} -> x {max(x.bond_dims)}, local / gemm solves {info['local_solves']} / {info['gemm_solves']}")
    print(f"   residual |(M + alpha L) x - M y| / |M y| = {info['residual']:.2e} (largest local, before its solve)")
    rng = np.random.default_rng(3)
    idx = [int(v) for v in rng.integers(0, 2 ** n, size=6)]
    idx = [8 * (j // 8) + h for j, h in zip(idx, (0, 5, 6, 3, 5, 6))]
    b = bits_of(idx, n)
    xs, ys = np.real(qil.coefficient_batch(x, b)), np.real(qil.coefficient_batch(y, b))
    out = []
    for j, xv, yv in zip(idx, xs, ys):
        hidden = j % 8 in HIDDEN
        print(f"   x[{j}] = {xv:+.6f}   clean {clean_value(j):+.6f}   observed {'(hidden)' if hidden else format(yv, '+.6f')}")
        out.append(abs(xv - clean_value(j)))
    print(f"   worst distance from the clean signal at these indices: {max(out):.3e} (disturbance {NOISE:g} rms)")
    return {"errors": out, "info": info}


if __name__ == "__main__":
    main()
