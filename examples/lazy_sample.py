#!/usr/bin/env python3
"""Where are the peaks of W psi -- without forming W psi, and without a scan window?  `apply_sample` draws configurations x with
probability |(W psi)_x|^2 / |W psi|^2 from the operator and the state as they are; the rows it returns go straight into
`apply_coefficient_batch`, which reads the exact values there.

    python examples/lazy_sample.py

Part one: three damped modes, built directly as an MPS and NOT transformed; the QFT MPO goes into the call next to it.  A few
thousand samples land on the bins around the three tones, the most frequent ones are the peaks, and the lazy coefficient read-out
gives their exact amplitudes.  Part two: the z-plane of a two-pole signal, from its ZTMPS and the zT operator: the samples are
(k, l) cells, the most frequent cells are where |Z(k, l)| is largest.  No dense grid, no product, no hand-placed window; the call
keeps the right environments of |W psi|^2 (the sum of (chi D)^2 over the bonds) instead of the product.  Everything here is small,
and every printed figure is checked in the script against the materialised product."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

NS = 4096


def _most_frequent(rows, probs, top):
    """the distinct sampled rows, most frequent first: (row, count, returned probability)"""
    uniq, first, counts = np.unique(rows, axis=0, return_index=True, return_counts=True)
    order = np.argsort(-counts, kind="stable")[:top]
    return uniq[order], counts[order], probs[first[order]]


def spectrum_part():
    n = 12
    N = 2 ** n
    modes = [(250.0, 8e-5, 1.0), (1250.0, 4e-4, 0.8), (3000.0, 2e-4, 0.5)]                 # (bin, damping per sample, amplitude)
    psi = qil.exponential_sum([a for _, _, a in modes], [np.exp(-g + 2j * np.pi * f / N) for f, g, _ in modes], n)
    W = qil.build_qft_mpo(psi)
    rows, probs = qil.apply_sample(W, psi, NS, seed=7, bits=True)
    peaks, counts, pk = _most_frequent(rows, probs, 3)
    values = qil.apply_coefficient_batch(W, psi, peaks)                                # exact, and still no product
    norm2 = (psi.amplitude * qil.apply_norm(W, psi)) ** 2
    bins = peaks.astype(np.int64) @ (1 << np.arange(n))                                # the QFT output holds the bin lsb first
    print(f"three damped modes, N = 2^{n}: {NS} samples of W psi, {len(np.unique(rows, axis=0))} distinct bins hit")
    for b, c, p, v in zip(bins, counts, pk, values):
        assert abs(abs(v) ** 2 / norm2 - p) <= 1e-10 * p                               # the returned probability is the Born weight
        print(f"   bin {int(b):5d}: {int(c):5d} samples, probability {p:.4f}, |X| = {abs(v):.6e}")
    out = W * psi                                                                      # checks only
    dense = np.abs(qil.mps_to_vector(out)) ** 2
    want = np.sort(np.argsort(dense)[-3:])
    got = np.sort(peaks.astype(np.int64) @ (1 << np.arange(n - 1, -1, -1)))
    assert np.array_equal(got, want), (got, want)
    assert sorted(int(b) for b in bins) == [250, 1250, 3000]
    return sorted(int(b) for b in bins)


def zplane_part():
    n = 8
    N = 2 ** n
    j = np.arange(N)
    x = 0.98 ** j * np.cos(0.4 * j) + 0.5 * 0.995 ** j * np.cos(1.3 * j)
    psi = qil.signal_ztmps(x)
    W = qil.build_zt_mpo(psi, 0.5)
    rows, probs = qil.apply_sample(W, psi, NS, seed=7, bits=True)
    cells, counts, pk = _most_frequent(rows, probs, 4)
    values = qil.apply_coefficient_batch(W, psi, cells)
    w = 1 << np.arange(n)
    ks, ls = cells[:, 0::2].astype(np.int64) @ w, cells[:, 1::2].astype(np.int64) @ w
    norm2 = (psi.amplitude * qil.apply_norm(W, psi)) ** 2
    print(f"two-pole signal, N = 2^{n}: {NS} samples of the z-plane, {len(np.unique(rows, axis=0))} distinct cells hit")
    for k, l, c, p, v in zip(ks, ls, counts, pk, values):
        assert abs(abs(v) ** 2 / norm2 - p) <= 1e-10 * p
        print(f"   cell (k, l) = ({int(k):3d}, {int(l):3d}): {int(c):4d} samples, probability {p:.4f}, |Z| = {abs(v):.6e}")
    phi = W * psi                                                                      # checks only
    ref = qil.coefficient_batch(phi, cells)
    assert np.abs(values - ref).max() <= 1e-10 * np.abs(ref).max()
    return list(zip(ks.tolist(), ls.tolist()))


def main():
    return spectrum_part(), zplane_part()


if __name__ == "__main__":
    main()
