#!/usr/bin/env python3
"""Zooming into the z-plane without a second operator -- the fine and superfine scans of the reference's zT tutorial
(docs/src/tutorials/zt.md:485-564 of QILaplace.jl) by product-vector read-outs of the encoded signal.

    python examples/zoom_scan.py

The tutorial's signal x_j = a^j cos(w0 j), a = 1.00015 e^{0.002 i}, w0 = 0.0061, N = 2^20, is encoded ONCE as a SignalMPS.
chi(z) = (1 / N) sum_j x_j z^j is then read at any z = exp(-(wr k + 2 pi i l) / N) with real (k, l) by `zt_eval`: the same
128 x 128 fine window and 49 x 49 superfine window as the tutorial, then a window ten times finer than the grid of the
wr = 0.5 operator can give.  |chi| is the modulus of a polynomial in z, so inside a window it peaks on the window's edge; the
pole shows as the point of that edge nearest to it, and the printed error is the distance of the peak to the analytic pole, next
to the tutorial's published 1.5e-4 (fine) and 1.2e-4 (superfine)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

N_BITS = 20
A, W0 = 1.00015 * np.exp(0.002j), 0.0061
WR, WI = 0.5, 2 * np.pi
POLES = (np.exp(1j * W0) / A, np.exp(-1j * W0) / A)


def tutorial_signal(n=N_BITS):
    j = np.arange(2 ** n)
    return A ** j * np.cos(W0 * j)


def z_of(k, l, n=N_BITS, wr=WR, wi=WI):
    """The tutorial's z_from_kl, for real (k, l)."""
    r, th = np.exp(-wr * k / 2 ** n), wi * l / 2 ** n
    return r * np.cos(th) - 1j * r * np.sin(th)


def fine_window(n=N_BITS, wr=WR, wi=WI, points=128):
    """(k, l) of the tutorial's fine window, r in [1 - 1.6e-4, 1], theta in [-5e-3, 9e-3] -- not rounded to the grid."""
    N = 2 ** n
    k = (-N / wr) * np.log(np.linspace(1 - 1.6e-4, 1.0, points))
    l = (N / wi) * np.linspace(-5e-3, 9e-3, points)
    return k, l


def superfine_window(n=N_BITS, wr=WR, wi=WI, half=24.0, points=49):
    """A (2 half + 1)-bin square of (k, l) around the analytic positive pole: the tutorial's at half = 24, points = 49."""
    N = 2 ** n
    kc, lc = (-N / wr) * np.log(abs(POLES[0])), (N / wi) * (-np.angle(POLES[0]))
    return np.linspace(kc - half, kc + half, points), np.linspace(lc - half, lc + half, points)


def scan(psi, k, l, n=N_BITS, wr=WR):
    """|chi| on the window, its peak and the peak's distance to the nearest analytic pole."""
    chi = qil.zt_eval(psi, wr, k[:, None], l[None, :])
    i, j = np.unravel_index(np.argmax(np.abs(chi)), chi.shape)
    z = z_of(k[i], l[j], n, wr)
    return chi, (k[i], l[j]), z, min(abs(z - p) for p in POLES)


def main():
    x = tutorial_signal()
    t0 = time.perf_counter()
    psi = qil.signal_mps(x, method="rsvd", k=50, p=5, q=2, cutoff=1e-12, maxdim=128)
    print(f"signal_mps: bonds {psi.bond_dims}  ({time.perf_counter() - t0:.3f} s)")
    out = {}
    for name, (k, l), published in (("fine", fine_window(), 1.509e-4), ("superfine", superfine_window(), 1.185e-4),
                                    ("10x finer", superfine_window(half=2.4), None)):
        t0 = time.perf_counter()
        chi, (kp, lp), z, err = scan(psi, k, l)
        dt = time.perf_counter() - t0
        print(f" {name} window: {chi.size} points in {dt:.3f} s, step {k[1] - k[0]:.3f} x {l[1] - l[0]:.3f} bins")
        print(f"   peak at (k, l) = ({kp:.3f}, {lp:.3f}), z = {z.real:.6f} + {z.imag:.6f}i")
        print(f"   error from nearest analytic pole: {err:.3e}" + (f"   (tutorial, on the operator's grid: {published:.3e})" if published else
                                                                     "   (no grid of the wr = 0.5 operator holds these points)"))
        out[name] = (kp, lp, err)
    return out


if __name__ == "__main__":
    main()
