#!/usr/bin/env python3
"""Spectral norms and condition numbers of operators in MPS form, without a dense object.

    python examples/operator_norm.py

Two numbers no other verb returns.  |W|_2 of a built damping-transform operator (`build_dt_mpo`): the factor by which W can
amplify noise, and the bound |W psi' - W psi| <= |W|_2 |psi' - psi| after a truncation of psi.  And a lower bound of the
condition number kappa of the masked smoother M + alpha L of examples/smooth_fill.py, the number `solve`'s accuracy bound
kappa * tol + ... is stated in.  Both come from `eigs` (two-site DMRG with a Lanczos local solve); first on 10 tensors, where
numpy's dense values are printed next to them, then on 40 tensors, where no dense object exists.

The limits of `eigs` apply and show here.  Every value is a Rayleigh quotient, so |W|_2 is approached from below and the
condition number is a LOWER bound; the small end of the smoother is a cluster of smooth modes (gaps of order alpha (2 pi / N)^2), the
slow case, so `converged` is printed with it: check a result with `eig_residual`.  On one MI355X the 10-tensor smoother also
showed the other limit: the sweep for the large end settled, with a residual of zero, on theta = 16.7702 where numpy's largest
eigenvalue is 16.7979 -- an eigenvector, not the extremal one -- so the printed kappa was 24.165 against 24.380."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qilaplace_jl_amd as qil  # noqa: E402
import smooth_fill as SF  # noqa: E402

WR = 0.999                                          # the damping of the DT operator
KW = dict(maxdim=32, cutoff=1e-18, tol=1e-8)


def smoother(n):
    """M + alpha L with the mask of examples/smooth_fill.py"""
    mask = qil.SignalMPS(SF.mask_tensors(n))
    return qil.mpo_linear_combination([qil.diagonal_mpo(mask), qil.build_laplacian_mpo(mask)], [1.0, SF.ALPHA])


def report(registers, n, dense):
    W = qil.build_dt_mpo(registers, WR)
    t0 = time.perf_counter()
    nrm = qil.operator_norm(W, **KW)
    dt = time.perf_counter() - t0
    line = f"DT operator, {registers} register pairs ({2 * registers} tensors), wr = {WR}: |W|_2 = {nrm:.12g}  (|W|_F = {qil.mpo_norm(W):.6g}, {dt * 1e3:.0f} ms)"
    if dense:
        line += f"   numpy: {np.linalg.norm(qil.mpo_to_matrix(W), 2):.12g}"
    print(line)
    A = smoother(n)
    t0 = time.perf_counter()
    hi, (xh,), (ih,) = qil.eigs(A, 1, "largest", return_info=True, **KW)
    lo, (xl,), (il,) = qil.eigs(A, 1, "smallest", return_info=True, **KW)
    dt = time.perf_counter() - t0
    line = (f"masked smoother M + {SF.ALPHA:g} L, {n} tensors: theta_max = {hi[0]:.10g}, theta_min = {lo[0]:.10g}, "
            f"kappa >= {hi[0] / lo[0]:.8g}  ({dt * 1e3:.0f} ms; converged {ih['converged']} / {il['converged']}, "
            f"sweeps {ih['sweeps']} / {il['sweeps']}, residuals {qil.eig_residual(A, xh, hi[0]):.1e} / {qil.eig_residual(A, xl, lo[0]):.1e})")
    if dense:
        ev = np.linalg.eigvalsh(qil.mpo_to_matrix(A))
        line += f"   numpy: {ev[-1]:.10g}, {ev[0]:.10g}, kappa = {ev[-1] / ev[0]:.8g}"
    print(line)


def main():
    report(5, 10, dense=True)
    report(20, 40, dense=False)


if __name__ == "__main__":
    main()
