"""Times of the top-k coefficient search (qil.top_k) on one GPU (HIP events around calls, median of --reps after warm-up): an
n = 24 paired chain (48 tensors), chi = 64, c64, k = 16 at beam = 2^12, 2^14, 2^16, 2^18, next to `sample` of 2 beam rows of
the same state (the cost reference: the same environments and GEMM shapes per site, without the select step).  With
--pole-scan: the pole-scan operator of examples/zt_pole_scan.py (n = 20, wr = 0.5, a 2^40-point grid), top-1 against the
fine scan's argmax, and the beam at which the bound certifies, if one does.  --trace B: only beam B, three calls (the
target of a `rocprofv3 --kernel-trace --stats` run).  One JSON line per measurement on stdout (and in --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qilaplace_jl_amd as qil  # noqa: E402
from helpers import saturated_profile  # noqa: E402


def timed(ctx, fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return float(np.median(ts)), float(min(ts))


def pole_scan(emit):
    """the operator of examples/zt_pole_scan.py at its fine scan (wr = 0.5)"""
    n = 20
    N = 2 ** n
    a, w0 = 1.00015 * np.exp(0.002j), 0.0061
    j = np.arange(N)
    x = a ** j * np.cos(w0 * j)
    psi = qil.signal_ztmps(x, method="rsvd", k=50, p=5, q=2, cutoff=1e-12, maxdim=128)
    wr, wi = 0.5, 2 * np.pi
    phi = qil.build_zt_mpo(psi, wr, cutoff=1e-12, maxdim=128) * psi
    r_t = np.linspace(1 - 1.6e-4, 1.0, 128)
    ks = np.clip(np.rint((-N / wr) * np.log(r_t)).astype(np.int64), 0, N - 1)
    th = np.mod(np.linspace(-5e-3, 9e-3, 128), 2 * np.pi)
    ls = np.mod(np.rint((N / wi) * th).astype(np.int64), N)
    chi = qil.coefficient_grid(phi, ks, ls)
    i, jj = np.unravel_index(np.argmax(np.abs(chi)), chi.shape)
    fine = (int(ks[i]), int(ls[jj]), float(np.abs(chi[i, jj])))
    emit(what="pole_scan_fine_argmax", k=fine[0], l=fine[1], abs_value=fine[2], max_bond=int(max(phi.bond_dims)))
    ctx = qil.default_context()
    for lg in range(4, 19, 2):
        beam = 2 ** lg
        ctx.timer_start()
        try:
            (kk, ll), vals, bound, cert = qil.top_k(phi, 1, beam=beam)
        except ValueError as e:            # above the cap for this state
            emit(what="pole_scan_top1", beam=beam, error=str(e))
            break
        ms = ctx.timer_stop()
        emit(what="pole_scan_top1", beam=beam, k=int(kk[0]), l=int(ll[0]), abs_value=float(abs(vals[0])), bound=bound,
             certified=cert, ratio_to_fine_max=float(abs(vals[0])) / fine[2], ms=ms)
        if cert:
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pole-scan", action="store_true")
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    ctx = qil.default_context()
    lines = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    L = 48
    psi = qil.ZTMPS.alloc(saturated_profile(L, 64), dtype=np.complex128).fill_random(20241016)
    if args.trace:
        for _ in range(3):
            qil.top_k(psi, 16, beam=args.trace, bits=True)
        emit(what="top_k_trace_target", beam=args.trace, calls=3)
    elif args.pole_scan:
        pole_scan(emit)
    else:
        for lg in (12, 14, 16, 18):
            beam = 2 ** lg
            med, mn = timed(ctx, lambda: qil.top_k(psi, 16, beam=beam, bits=True), args.reps)
            _, vals, bound, cert = qil.top_k(psi, 16, beam=beam, bits=True)
            smed, smn = timed(ctx, lambda: qil.sample(psi, 2 * beam, seed=1, bits=True), args.reps)
            emit(what="top_k_n24p_chi64", dtype="complex128", k=16, beam=beam, ms_median=med, ms_min=mn,
                 sample_2beam_ms_median=smed, sample_2beam_ms_min=smn, top_k_over_sample=med / smed,
                 abs_value_1=float(abs(vals[0])), abs_value_k=float(abs(vals[-1])), bound=bound, certified=cert)
    if args.out:
        with open(args.out, "w") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
