#!/usr/bin/env python3
"""Poles without a scan: ESPRIT on the bond basis of a SignalMPS.

    python examples/esprit_poles.py

1. Two tones 3e-10 of the sample rate apart in a record of 2^40 samples (a real signal: four complex modes), built by
   `exponential_sum` without touching 2^40 numbers.  `esprit` reads the poles off three right environments of the last 39
   tensors, O(n chi^3); with only the last 4 tensors (`count=4`, a 16-sample baseline) the two tones merge.
2. The signal of the reference's zT tutorial (x_j = a^j cos(w0 j), N = 2^20), encoded by `signal_mps`: its two poles, next to
   the error the tutorial's three z-plane scans publish (1.5e-4) and to a placed 128 x 128 `zt_eval` window."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402
import zoom_scan as Z  # noqa: E402

F, DF, N40 = 0.1734, 3e-10, 40


def two_tones():
    zs = [complex(np.cos(2 * np.pi * s * f), np.sin(2 * np.pi * s * f)) for f in (F, F + DF) for s in (1, -1)]
    return zs, [0.5, 0.5, 0.4, 0.4]


def main():
    zs, amps = two_tones()
    psi = qil.exponential_sum(amps, zs, N40, maxdim=None, tol=None)
    sep = abs(zs[0] - zs[2])
    t0 = time.perf_counter()
    poles, found = qil.esprit(psi)
    dt = time.perf_counter() - t0
    print(f"two tones {DF:g} of the sample rate apart, n = {N40} (separation {sep:.3e} in z), bonds {max(psi.bond_dims)}: {dt * 1e3:.1f} ms")
    out = {"two_tones": []}
    for z in zs[0::2]:
        j = int(np.argmin(np.abs(poles - z)))
        f = np.angle(poles[j]) / (2 * np.pi)
        print(f"   tone at f = {f:.13f} cycles / sample, |z| = {abs(poles[j]):.15f}, error {abs(poles[j] - z):.2e}, amplitude {abs(found[j]):.6f}")
        out["two_tones"].append(abs(poles[j] - z))
    short, _ = qil.esprit(psi, count=4)
    worst = max(float(np.min(np.abs(short - z))) for z in zs)
    print(f"   with the last 4 tensors only: error {worst:.2e} -- {'merged' if worst > 0.1 * sep else 'resolved'}")
    out["two_tones_count4"] = worst

    x = Z.tutorial_signal()
    psi = qil.signal_mps(x, method="rsvd", k=50, p=5, q=2, cutoff=1e-12, maxdim=128)
    t0 = time.perf_counter()
    poles, found = qil.esprit(psi, maxdim=2)
    dt = time.perf_counter() - t0
    # the tutorial's z-plane is that of chi(z) = sum x_j z^j: its poles are the reciprocals of the signal's
    err = max(float(np.min(np.abs(1.0 / poles - p))) for p in Z.POLES)
    print(f"zT tutorial signal, n = {Z.N_BITS}, bonds <= {max(psi.bond_dims)}: esprit(maxdim=2) in {dt * 1e3:.1f} ms")
    for z, a in zip(poles, found):
        print(f"   pole of chi at z = {(1 / z).real:.9f} {(1 / z).imag:+.9f}i, amplitude {abs(a):.6f}")
    print(f"   error from the analytic poles: {err:.3e}   (tutorial, three scans of the 2^40-point plane: 1.509e-04)")
    k, l = Z.fine_window()
    t0 = time.perf_counter()
    werr = Z.scan(psi, k, l)[3]
    print(f"   a placed 128 x 128 zt_eval window: {werr:.3e} in {(time.perf_counter() - t0) * 1e3:.1f} ms")
    out["tutorial"] = err
    return out


if __name__ == "__main__":
    main()
