"""Times of qil.evolve on one GPU: call time by HIP events around the whole call (the working copy, the gauge, the environments,
the local exponentials, the splits and the host work between them), ten repetitions after two warm-up rounds, median and range.
The routes of every comparison alternate inside one process.

  routes    ONE full step over 40 tensors (`--lengths` for others; 4 n - 6 = 154 local exponentials, 2 n - 2 two-site and
            2 n - 4 one-site) forced onto each route (QIL_EVOLVE_ROUTE, read per call) on the same operands: x0 random at bond chi
            in {4, 8, 16} with maxdim = chi and cutoff 0 (the bond stays), the Hermitian operators of tools/_solve_time.py of bond
            D in {2, 3, 5}, f64 and c64, tau = -0.01, krylov = 8, substeps = 4.  `local_exps` / `gemm_exps` say what a forced
            local really took, `matvecs` the Lanczos work of the step, `macs2` / `macs1` the multiply-adds of one two-site and one
            one-site matvec at the middle, `us_per_exp` the call time over the exponentials (both kinds together: the call is
            timed, not its parts).
  mode40    the n = 40 Fourier-mode and field cases of the tests, end to end, on each route
  diffuse24 exp(-t L) y at n = 24 for a t where three verbs apply: `diffuse` (explicit, this verb), `smooth` with alpha = t
            (implicit, one backward-Euler step: a different filter of the same strength) and the Fourier route (`convolve` with
            the heat kernel exp(-t lambda_k) brought back to samples)

One JSON line per measurement on stdout (and appended to --out)."""
import argparse
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import qilaplace_jl_amd as qil  # noqa: E402
from _product_time import gpu_name, timed_pair  # noqa: E402
from _solve_time import operator  # noqa: E402


def forced(route, fn):
    def run():
        if route is None:
            os.environ.pop("QIL_EVOLVE_ROUTE", None)
        else:
            os.environ["QIL_EVOLVE_ROUTE"] = route
        try:
            return fn()
        finally:
            os.environ.pop("QIL_EVOLVE_ROUTE", None)
    return run


def macs2(xl, xr, dl, dm, dr):
    return 4 * xl * xl * xr * dl + 8 * xl * xr * dm * (dl + dr) + 4 * xl * xr * xr * dr


def macs1(xl, xr, dl, dr):
    return 2 * xl * xl * xr * dl + 4 * xl * xr * dl * dr + 2 * xl * xr * xr * dr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="routes,mode40,diffuse24")
    ap.add_argument("--bonds", default="4,8,16")
    ap.add_argument("--op-bonds", default="2,3,5")
    ap.add_argument("--lengths", default="40")
    args = ap.parse_args()
    ctx = qil.default_context()
    box = {"gpu": gpu_name(), "host": socket.gethostname()}

    def emit(rec):
        rec = dict(rec, lib=args.tag, reps=args.reps, **box)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def stats(ts):
        return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts))}

    def compare(case, run, extra=None, routes=("local", "gemm", None)):
        """run() -> the info dict of one evolve call"""
        infos = {name: forced(name, run)() for name in routes}
        ts = timed_pair(ctx, {name: forced(name, run) for name in routes}, args.reps)
        for name, t in ts.items():
            i = infos[name]
            n_exp = i["local_exps"] + i["gemm_exps"]
            emit(dict(case=case, route=name or "auto", steps=i["steps"], matvecs=i["matvecs"], max_bond=i["max_bond"],
                      local_exps=i["local_exps"], gemm_exps=i["gemm_exps"], substeps=i["substeps"], estimate=i["estimate"],
                      converged=i["converged"], us_per_exp=1e3 * float(np.median(t)) / n_exp, **(extra or {}), **stats(t)))

    rng = np.random.default_rng(2026)
    if "routes" in args.only:
        for n in (int(v) for v in args.lengths.split(",")):
            for dt in (np.float64, np.complex128):
                for chi in (int(v) for v in args.bonds.split(",")):
                    xb = [min(chi, 2 ** min(i + 1, n - 1 - i)) for i in range(n - 1)]
                    x0 = qil.SignalMPS.alloc(xb, dtype=dt).fill_random(9)
                    for D in (int(v) for v in args.op_bonds.split(",")):
                        A, _ = operator(D, n, dt, rng)
                        mid = n // 2 - 1
                        ab, xx = [1] + list(A.bond_dims) + [1], [1] + xb + [1]
                        d2 = (xx[mid], xx[mid + 2], ab[mid], ab[mid + 1], ab[mid + 2])
                        d1 = (xx[mid], xx[mid + 1], ab[mid], ab[mid + 1])
                        run = lambda: qil.evolve(A, x0, -0.01, steps=1, maxdim=chi, cutoff=0.0, tol=1e-10, krylov=8, substeps=4,
                                                 return_info=True)[1]
                        compare(f"step_n{n}_chi{chi}_D{D}_{np.dtype(dt).name}", run, dict(macs2=macs2(*d2), macs1=macs1(*d1)))
    if "mode40" in args.only:
        import evolve_model as EV
        for name in EV.MODE40_CASES + EV.FIELD40_CASES:
            d = EV.case(name)
            A, x0 = qil.SingleSiteMPO(d["A"]), qil.SignalMPS(d["x0"])
            compare(name, lambda: qil.evolve(A, x0, d["t"], return_info=True, **d["kwargs"])[1])
    if "diffuse24" in args.only:
        import smooth_fill
        n, t = 24, 8.0
        y, _, _ = smooth_fill.operands(n)
        N = 2 ** n
        lam = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(N) / N)
        kernel = qil.signal_mps(np.real(np.fft.ifft(np.exp(-t * lam))), cutoff=1e-20)
        F = qil.build_qft_mpo(y)
        kw = dict(maxdim=32, cutoff=1e-18, tol=1e-8)
        fns = {"diffuse": lambda: qil.diffuse(y, t, **kw), "smooth": lambda: qil.smooth(y, t, **kw),
               "fourier": lambda: qil.convolve(y, kernel, F=F, maxdim=32, tol=1e-9)}
        outs = {k: f() for k, f in fns.items()}
        ts = timed_pair(ctx, fns, args.reps)
        _, info = qil.diffuse(y, t, return_info=True, **kw)
        ref = outs["diffuse"]
        for k, tt in ts.items():
            emit(dict(case=f"diffuse24_t{t:g}", verb=k, max_bond=max(outs[k].bond_dims), y_bond=max(y.bond_dims),
                      kernel_bond=max(kernel.bond_dims), distance_to_diffuse=float(qil.distance(outs[k], ref) / (ref.amplitude * qil.norm(ref))),
                      diffuse_steps=info["steps"], diffuse_matvecs=info["matvecs"], **stats(tt)))


if __name__ == "__main__":
    main()
