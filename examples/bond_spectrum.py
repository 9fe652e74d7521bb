#!/usr/bin/env python3
"""How entangled is the state, and which bond dimension keeps it?  The Schmidt spectrum of every bond, read from the device --
`bond_spectra`, with `entanglement_entropy`, `truncation_error_bounds` and `required_maxdim` on top of it.

    python examples/bond_spectrum.py

The quick-start signal (two damped sines) is encoded as an MPS and transformed by the QFT MPO.  For both states the script prints
the bond dimensions, the entanglement entropy of every cut and the leading Schmidt values of the widest bond: the numbers that
`maxdim` and `tol` of `compress` cut into.  `required_maxdim` then answers "which bond dimension keeps this state to tol" from
the spectra alone, and one answer is checked the expensive way, by `compress` and `distance`."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402


def sin_decay(n, freq, decay_rate):
    """generate_signal(n; kind=:sin_decay, freq, decay_rate) of the reference (closed form)."""
    freq, decay_rate = np.atleast_1d(freq).astype(float), np.atleast_1d(decay_rate).astype(float)
    N = 2 ** n
    dt = 1.0 / (np.max(np.abs(freq)) * N)
    j = np.arange(N)
    return sum(np.sin(w * dt * j) * np.exp(-l * dt * j) for w, l in zip(freq, decay_rate))


def report(title, psi):
    spectra = qil.bond_spectra(psi)
    entropy = qil.entanglement_entropy(spectra)
    widest = int(np.argmax([len(s) for s in spectra]))
    print(f"{title}: bonds {psi.bond_dims}")
    print("   entropy per bond (bits): " + " ".join(f"{e:.3f}" for e in entropy))
    print(f"   Schmidt values of bond {widest + 1}: " + " ".join(f"{v:.2e}" for v in spectra[widest][:8]))
    for s in spectra:
        assert abs(np.sum(s * s) - 1.0) <= 1e-12 and np.all(np.diff(s) <= 0.0)
    return spectra


def main():
    n = 10
    rng = np.random.default_rng(3)
    signal = sin_decay(n, [1.0, 2.5], [0.08, 0.03]) + 1e-3 * rng.standard_normal(2 ** n)     # a noise floor worth truncating
    psi = qil.signal_mps(signal, cutoff=1e-15)
    report("signal", psi)
    out = qil.build_qft_mpo(psi, cutoff=1e-14) * psi
    spectra = report("QFT of the signal", out)

    print("   bond dimension that keeps the transformed state to tol (one truncating sweep):")
    needs = {}
    for tol in (1e-1, 1e-2, 1e-3, 1e-4):
        needs[tol] = qil.required_maxdim(spectra, tol)
        lower, upper = qil.truncation_error_bounds(spectra, needs[tol])
        print(f"      tol {tol:.0e}: maxdim {needs[tol]:3d}   (error between {lower:.2e} and {upper:.2e} of |psi|)")
    assert all(a <= b for a, b in zip(list(needs.values()), list(needs.values())[1:]))

    # ... and one of them the expensive way
    tol = 1e-3
    maxdim = needs[tol]
    lower, upper = qil.truncation_error_bounds(spectra, maxdim)
    trunc = out.copy()
    qil.compress(trunc, maxdim=maxdim, tol=0.0)
    d = qil.distance(out, trunc) / (out.amplitude * qil.norm(out))
    slack = 2.0 * np.sqrt((n - 1) * 1e-12)                 # compress's own gauge passes cut at 1e-12 per bond
    print(f"   compress(maxdim={maxdim}) is {d:.2e} of |psi| away: inside [{lower:.2e}, {upper:.2e}] and below tol {tol:.0e}")
    assert lower - slack <= d <= upper + slack and d <= tol + slack
    return {"needs": needs, "distance": d}


if __name__ == "__main__":
    main()
