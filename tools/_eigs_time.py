"""Times of qil.eigs on one GPU: call time by HIP events around the whole call (the working copy, the gauge, the environments,
the local eigen-solves, the splits and the host work between them), ten repetitions after two warm-up rounds, median and range.
The two routes of every comparison alternate inside one process.

  routes    ONE full sweep (max_sweeps = 1) forced onto each route of the local solve (QIL_EIGS_ROUTE, read per call) on the
            same operands: x0 random at bond chi in {4, 8, 16} with maxdim = chi and cutoff 0 (the bond stays), the Hermitian
            operators of tools/_solve_time.py of bond D in {2, 3, 5, 8}, f64 and c64, 40 tensors (`--lengths` for others), the
            smallest eigenvalue, krylov = 8, restarts = 4.  `local_solves` / `gemm_solves` say what a forced local really took (it
            falls back where the bond does not fit), `matvecs` the Lanczos work of the sweep, `macs` the multiply-adds of one
            matvec at the middle bond.
  field40   the n = 40 field operator of the tests, both ends, end to end, on each route
  dt24      operator_norm of the n = 24 damping-transform operator (48 tensors), end to end, on each route

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
import qilaplace_jl_amd as qil  # noqa: E402
from _product_time import gpu_name, timed_pair  # noqa: E402
from _solve_time import operator  # noqa: E402


def forced(route, fn):
    def run():
        if route is None:
            os.environ.pop("QIL_EIGS_ROUTE", None)
        else:
            os.environ["QIL_EIGS_ROUTE"] = route
        try:
            return fn()
        finally:
            os.environ.pop("QIL_EIGS_ROUTE", None)
    return run


def matvec_macs(xl, xr, dl, dm, dr):
    return 4 * xl * xl * xr * dl + 8 * xl * xr * dm * (dl + dr) + 4 * xl * xr * xr * dr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="routes,field40,dt24")
    ap.add_argument("--bonds", default="4,8,16")
    ap.add_argument("--op-bonds", default="2,3,5,8")
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

    def compare(case, run, extra=None):
        """run() -> a list of info dicts (one per eigs call inside)"""
        infos = {name: forced(name, run)() for name in ("local", "gemm")}
        ts = timed_pair(ctx, {name: forced(name, run) for name in ("local", "gemm")}, args.reps)
        for name, t in ts.items():
            i = infos[name]
            emit(dict(case=case, route=name, sweeps=sum(v["sweeps"] for v in i), matvecs=sum(v["matvecs"] for v in i),
                      max_bond=max(v["max_bond"] for v in i), local_solves=sum(v["local_solves"] for v in i),
                      gemm_solves=sum(v["gemm_solves"] for v in i), residual=max(v["residual"] for v in i),
                      converged=all(v["converged"] for v in i), **(extra or {}), **stats(t)))

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
                        dims = (xx[mid], xx[mid + 2], ab[mid], ab[mid + 1], ab[mid + 2])
                        os.environ["QIL_EIGS_ROUTE"] = "local"
                        fits = qil.eigs_local_fits(*dims, dtype=dt)
                        os.environ.pop("QIL_EIGS_ROUTE")
                        run = lambda: qil.eigs(A, 1, "smallest", x0=x0, maxdim=chi, cutoff=0.0, tol=1e-8, max_sweeps=1, krylov=8,
                                               restarts=4, return_info=True)[2]
                        compare(f"sweep_n{n}_chi{chi}_D{D}_{np.dtype(dt).name}", run,
                                dict(mid_bond_fits_lds=bool(fits), macs=matvec_macs(*dims)))
    if "field40" in args.only:
        import eigs_model as EM
        A = qil.SingleSiteMPO(EM.field_tensors(40))
        for which in ("smallest", "largest"):
            compare(f"field40_{which}", lambda: qil.eigs(A, 1, which, seed=7, return_info=True, **EM.EIGS_DEFAULTS)[2])
    if "dt24" in args.only:
        W = qil.build_dt_mpo(24, 0.999)
        N, _ = qil.ops._normal_operator(W)
        out = {}

        def run():
            values, _, infos = qil.eigs(N, 1, "largest", maxdim=32, cutoff=1e-18, tol=1e-8, return_info=True)
            out["norm"] = float(np.sqrt(max(values[0], 0.0)))
            return infos
        compare("operator_norm_dt24", run, dict(op_bond=max(N.bond_dims)))
        emit(dict(case="operator_norm_dt24_value", value=out["norm"], frobenius=qil.mpo_norm(W)))


if __name__ == "__main__":
    main()
