#!/usr/bin/env python3
"""FIR filters as operators on 2^30 samples, and two operators compared without a dense matrix.

    python examples/fir_filter.py

A filter sum_k h_k S^k (S = the cyclic shift by one sample, an exact MPO of bond 2) is a linear combination of operators
followed by `mpo_compress` (`fir_mpo`): a short smoothing filter and the 3-point second difference are built that way and
applied to a three-mode `exponential_sum` signal of n = 30 sites (the exact bond-3 sum: tol=None).  A handful of output samples
is checked against the closed form: away from the wrap-around, a filter multiplies the mode z^j by its transfer function
sum_k h_k z^(-k); the powers are taken by squaring in long double, which keeps z^(2^30) to about 1e-10.  Then the verbs on
operators alone: `mpo_distance` between the QFT built at two cutoffs, and <F, F>_F / 2^n - 1, which is 0 for a unitary F."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

N_BITS = 30
SMOOTH = {0: 0.25, 1: 0.5, 2: 0.25}                   # binomial smoothing, delayed by one sample
SECOND_DIFFERENCE = {-1: 1.0, 0: -2.0, 1: 1.0}


def modes(n):
    """three damped modes at 1.3 %, 11 % and 27 % of the sampling rate: the second difference sees all of them"""
    N = 2 ** n
    rates, damps, amps = (0.013, 0.11, 0.27), (1.0, 3.0, 0.5), (1.0, 0.6, 0.3)
    return [complex(np.exp(-g / N + 2j * np.pi * r)) for r, g in zip(rates, damps)], list(amps)


def power(z, j):
    """z^j for an integer j of either sign by squaring in long double"""
    z = np.clongdouble(z)
    if j < 0:
        z, j = 1 / z, -j
    out = np.clongdouble(1)
    while j:
        if j & 1:
            out = out * z
        z, j = z * z, j >> 1
    return out


def closed_form(taps, zs, amps, idx):
    """y_x = sum_k a_k z_k^x H(z_k), H(z) = sum_t h_t z^(-t), for samples x that no tap wraps around"""
    return np.array([complex(sum(a * power(z, int(x)) * sum(h * power(z, -t) for t, h in taps.items()) for a, z in zip(amps, zs)))
                     for x in idx])


def main():
    n = N_BITS
    zs, amps = modes(n)
    x = qil.exponential_sum(amps, zs, n, tol=None)
    idx = np.array([5, 1000, 2 ** 20 + 1, 2 ** 29 + 12345, 2 ** 30 - 7])
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    worst = {}
    for name, taps in (("smoothing", SMOOTH), ("second difference", SECOND_DIFFERENCE)):
        W = qil.fir_mpo(taps, x)
        y = qil.apply(W, x)
        got, want = qil.coefficient_batch(y, bits), closed_form(taps, zs, amps, idx)
        scale = max(abs(h) for h in taps.values()) * sum(abs(a) for a in amps)
        worst[name] = float(np.abs(got - want).max() / scale)
        assert worst[name] < 1e-9, (name, worst[name])
        print(f"{name}: operator bonds {max(W.bond_dims)}, |W|_F / 2^(n/2) = {qil.mpo_norm(W) / 2 ** (n / 2):.6f}, "
              f"output bonds {max(y.bond_dims)}, worst sample error {worst[name]:.2e} of scale")
    F14, F10 = qil.build_qft_mpo(n, cutoff=1e-14), qil.build_qft_mpo(n, cutoff=1e-10)
    rel = qil.mpo_distance(F14, F10) / qil.mpo_norm(F14)
    unit = float(np.real(qil.mpo_inner(F14, F14))) / 2.0 ** n - 1.0
    print(f"QFT n = {n}: bonds {max(F14.bond_dims)} (cutoff 1e-14) / {max(F10.bond_dims)} (1e-10), relative distance {rel:.2e}, "
          f"<F, F>/2^n - 1 = {unit:.2e}")
    return worst, rel, unit


if __name__ == "__main__":
    main()
