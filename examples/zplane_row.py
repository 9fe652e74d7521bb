#!/usr/bin/env python3
"""One row of a 2^40-point z-plane as a state of its own -- `restrict` / `zt_row` on the tutorial state of
examples/zt_pole_scan.py (the large example of the reference's zT tutorial, docs/src/tutorials/zt.md:318-560).

    python examples/zplane_row.py

The n = 20 two-pole signal is encoded and z-transformed at wr = 0.5 exactly as in the pole scan.  The transformed state has
2^20 x 2^20 coefficients chi(k, l), k the damping index on the main register, l the angle index on the copy register; no dense
block of it fits anywhere.  `top_k` finds the strongest point of the whole plane; `zt_row` fixes the copy register to that
point's l and returns the row through it as a 20-site SignalMPS over k, bonds no larger than the parent's.  Every verb then
works on the row alone: `norm` is its energy, `top_k` a certified peak search inside it.  The same is done for the rows of the
two peaks the tutorial publishes (fine scan: 0, 1047889; superfine scan: 320, 1047872), and the indices found are printed next
to the published ones.  The signal grows, so every row is strongest at k = 0 (r = 1); the superfine peak is a local one, and a
second restriction finds it: the high bits of k fixed as well (a zoom window, k = 256 .. 383), the 7-site slice searched."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

PUBLISHED = {"fine": (0, 1047889), "superfine": (320, 1047872)}     # docs/src/tutorials/zt.md:521, 562


def row_peaks(phi, l, k=4, beam=4096):
    """the k strongest damping indices of row l, their values, and whether the search certifies them"""
    t0 = time.perf_counter()
    row = qil.zt_row(phi, l)
    t_row = time.perf_counter() - t0
    idx, vals, bound, certified = qil.top_k(row, k, beam=beam)
    return row, [int(i) for i in _lsb_index(row, idx)], np.abs(vals), certified, t_row


def window_peak(phi, l, k_hi, low_bits):
    """the strongest k of row l inside the aligned window k >> low_bits == k_hi: copy register and the high main bits fixed"""
    n = len(phi)
    spec = np.full(2 * n, qil.ops.FREE, dtype=np.uint8)
    spec[1::2] = [(l >> i) & 1 for i in range(n)]
    spec[2 * low_bits::2] = [(k_hi >> i) & 1 for i in range(n - low_bits)]
    window = qil.restrict(phi, spec)
    idx, vals, bound, certified = qil.top_k(window, 1, beam=2 ** low_bits)
    return (k_hi << low_bits) + _lsb_index(window, idx)[0], abs(vals[0]), certified, window


def _lsb_index(row, idx):
    """top_k decodes a SignalMPS big-endian (site 1 = MSB); the row's sites carry k lsb first"""
    n = len(row)
    idx = np.asarray(idx, dtype=np.int64)
    return [sum(((int(v) >> (n - 1 - i)) & 1) << i for i in range(n)) for v in idx]


def main():
    n = 20
    N = 2 ** n
    a, w0 = 1.00015 * np.exp(0.002j), 0.0061
    j = np.arange(N)
    x = a ** j * np.cos(w0 * j)
    psi = qil.signal_ztmps(x, method="rsvd", k=50, p=5, q=2, cutoff=1e-12, maxdim=128)
    phi = qil.build_zt_mpo(psi, 0.5, cutoff=1e-12, maxdim=128) * psi
    print(f"transformed state: {phi.ntensors} tensors, largest bond {max(phi.bond_dims)}")
    (ks, ls), vals, bound, certified = qil.top_k(phi, 1, beam=4096)
    k0, l0 = int(ks[0]), int(ls[0])
    print(f" Strongest point of the plane: {k0}, {l0}  |chi| = {abs(vals[0]):.4e}  (certified: {certified})")
    out = {}
    for name, l in (("strongest", l0), ("fine", PUBLISHED["fine"][1]), ("superfine", PUBLISHED["superfine"][1])):
        row, peaks, mags, cert, t_row = row_peaks(phi, l)
        energy = qil.norm(row) * abs(row.amplitude)
        print(f" Row l = {l}: {len(row)} sites, largest bond {max(row.bond_dims)}, 2-norm {energy:.4e}, zt_row {1e3 * t_row:.2f} ms")
        print(f"   strongest damping indices k: {peaks}  |chi| = {mags[0]:.4e}  (certified: {cert})")
        if name in PUBLISHED:
            kp, lp = PUBLISHED[name]
            at = abs(qil.coefficient_grid(phi, [kp], [lp])[0, 0])
            print(f"   published {name} scan peak:   {kp}, {lp}  |chi| there = {at:.4e}")
        else:
            print(f"   the plane's strongest point:  {k0}, {l0}")
        out[name] = (peaks, l)
    kp, lp = PUBLISHED["superfine"]
    kw, mag, cert, window = window_peak(phi, lp, kp >> 7, 7)
    print(f" Window k = {(kp >> 7) << 7} .. {((kp >> 7) << 7) + 127} of row l = {lp}: {len(window)} sites, strongest k: {kw}"
          f"  |chi| = {mag:.4e}  (certified: {cert})")
    print(f"   published superfine scan peak:   {kp}, {lp}")
    out["window"] = (kw, lp)
    return out


if __name__ == "__main__":
    main()
