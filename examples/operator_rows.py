#!/usr/bin/env python3
"""Columns and rows of operators, read on the operator's own bonds: no basis state, no `apply`, no dense matrix.

    python examples/operator_rows.py

1. A FIR filter on 2^40 samples (`fir_mpo`, a sum of cyclic shifts) applied to the unit impulse is its impulse response: the
   column `mpo_column(F, 0)` IS that state, and `top_k` finds its non-zero samples -- the taps, at their offsets (negative
   offsets wrap to the top of the register).
2. One value of a z-transform is a linear functional of the signal: `mpo_row(W, cfg)` is that functional as a state r with
   (W psi)_cfg = sum_j r_j psi_j.  Built once, it is a matched filter: for a real signal the value is `inner(psi, r)`, for any
   number of signals, without applying W to any of them.  Two signals are checked against the lazy read-out of W psi."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qilaplace_jl_amd as qil  # noqa: E402

N_FIR = 40
TAPS = {-2: 0.0625, 0: 0.5, 1: -0.25, 3: 0.125, 7: 0.03125}
N_ZT = 10


def fir_taps():
    n = N_FIR
    F = qil.fir_mpo(TAPS, n)
    response = qil.mpo_column(F, 0)                       # F applied to the impulse at sample 0
    where, values, bound, certified = qil.top_k(response, k=len(TAPS))
    found = {int(x): float(v) for x, v in zip(where, values)}
    want = {k % 2 ** n: h for k, h in TAPS.items()}
    assert certified and set(found) == set(want), (found, bound)
    worst = max(abs(found[x] - want[x]) for x in want)
    assert worst <= 1e-12, worst
    print(f"FIR on 2^{n} samples: operator bonds {max(F.bond_dims)}, impulse response bonds {max(response.bond_dims)}, "
          f"{len(found)} taps recovered, worst error {worst:.1e}")
    # ... and the sum of the taps is the response to the all-ones signal, at any sample
    dc = qil.coefficient(qil.mpo_column_sums(F), 12345)
    assert abs(dc - sum(TAPS.values())) <= 1e-12
    return found


def matched_filter():
    n = N_ZT
    N = 2 ** n
    t = np.arange(N)
    signals = [np.exp(-0.004 * t) * np.cos(0.21 * t), np.exp(-0.009 * t) * np.sin(0.05 * t) + 0.1 * np.cos(0.21 * t)]
    states = [qil.signal_ztmps(x) for x in signals]
    assert all(s.dtype == np.float64 for s in states)     # real signals: sum_j r_j psi_j = <psi|r>
    W = qil.build_zt_mpo(states[0], 0.7)
    rng = np.random.default_rng(4)
    cfg = rng.integers(0, 2, 2 * n).astype(np.uint8)      # one (k, l) point of the z-plane, as the bits of the 2n tensors
    row = qil.mpo_row(W, cfg)
    out = []
    for psi in states:
        got = qil.inner(psi, row)
        want = qil.apply_coefficient_batch(W, psi, cfg[None, :])[0]
        assert abs(got - want) <= 1e-10 * psi.amplitude * qil.norm(row), (got, want)
        out.append(got)
    print(f"zT row on {N} samples: operator bonds {max(W.bond_dims)}, row bonds {max(row.bond_dims)}, "
          f"values {out[0]:.6g} and {out[1]:.6g} match the lazy read-out of W psi")
    return out


def main():
    return fir_taps(), matched_filter()


if __name__ == "__main__":
    main()
