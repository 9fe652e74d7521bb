"""Times of qil.solve on one GPU: call time by HIP events around the whole call (the working copy, the gauge, the environments,
the local solves, the splits and the host work between them), ten repetitions after two warm-up rounds, median and range.
The two routes of every comparison alternate inside one process.

  routes    ONE full sweep (max_sweeps = 1) forced onto each route of the local solve (QIL_SOLVE_ROUTE, read per call) on the
            same operands: x0 random at bond chi in {4, 8, 16} with maxdim = chi and cutoff 0 (the bond stays), a random right-hand
            side of bond 4, Hermitian positive definite operators of bond D in {2, 3, 5, 8}, f64 and c64, 12 and 40 tensors.
            D = 2: 3 I + sum_i w_i X_i;  D = 3: 3 I + the transverse Ising chain sum J X_i X_{i+1} + h Z_i (|H| <= 2);
            D = 5: I + 100 L (build_laplacian_mpo);  D = 8: the direct sum of the last two.  `local_solves` / `gemm_solves` say
            what a forced local really took (it falls back where the bond does not fit), `matvecs` the CG work of the sweep.
  exp40     the n = 40 exponential right-hand side of the tests, end to end, on each route
  example   the solve of examples/smooth_fill.py end to end (n = 40, mask, bond-7 operator), on each route

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
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import qilaplace_jl_amd as qil  # noqa: E402
from _product_time import gpu_name, timed_pair  # noqa: E402

X = np.array([[0.0, 1.0], [1.0, 0.0]])
Z = np.array([[1.0, 0.0], [0.0, -1.0]])
I2 = np.eye(2)


def field_tensors(n, rng):
    """sum_i w_i X_i, sum |w_i| = 1: bond 2"""
    w = rng.uniform(0.5, 1.0, n)
    w /= w.sum()
    out = []
    for i in range(n):
        W = np.zeros((2, 2, 2, 2))
        W[0, :, :, 0], W[1, :, :, 1], W[0, :, :, 1] = I2, I2, w[i] * X
        out.append(W[:1] if i == 0 else W)
    out[-1] = out[-1][:, :, :, 1:]
    return out


def ising_tensors(n):
    """sum_i J X_i X_{i+1} + h Z_i with J = h = 1 / n (norm <= 2): bond 3"""
    J = h = 1.0 / n
    out = []
    for i in range(n):
        W = np.zeros((3, 2, 2, 3))
        W[0, :, :, 0], W[2, :, :, 2] = I2, I2
        W[0, :, :, 1], W[1, :, :, 2], W[0, :, :, 2] = J * X, X, h * Z
        out.append(W[:1] if i == 0 else W)
    out[-1] = out[-1][:, :, :, 2:]
    return out


def operator(D, n, dt, rng):
    """(A, shift) Hermitian positive definite of bond D"""
    cast = (lambda ts: [t.astype(np.complex128) for t in ts]) if dt == np.complex128 else (lambda ts: ts)
    if D == 2:
        return qil.SingleSiteMPO(cast(field_tensors(n, rng))), 3.0
    if D == 3:
        return qil.SingleSiteMPO(cast(ising_tensors(n))), 3.0
    lap = qil.SingleSiteMPO(cast(qil.laplacian_mpo_tensors(n)))
    if D == 5:
        return qil.mpo_scale(lap, 100.0), 1.0
    if D == 8:
        return qil.mpo_linear_combination([lap, qil.SingleSiteMPO(cast(ising_tensors(n)))], [100.0, 1.0]), 3.0
    raise ValueError(f"no operator of bond {D}")


def forced(route, fn):
    def run():
        if route is None:
            os.environ.pop("QIL_SOLVE_ROUTE", None)
        else:
            os.environ["QIL_SOLVE_ROUTE"] = route
        try:
            return fn()
        finally:
            os.environ.pop("QIL_SOLVE_ROUTE", None)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="routes,exp40,example")
    ap.add_argument("--bonds", default="4,8,16")
    ap.add_argument("--op-bonds", default="2,3,5,8")
    ap.add_argument("--lengths", default="12,40")
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
        infos = {name: forced(name, run)()[1] for name in ("local", "gemm")}
        ts = timed_pair(ctx, {name: forced(name, run) for name in ("local", "gemm")}, args.reps)
        for name, t in ts.items():
            i = infos[name]
            emit(dict(case=case, route=name, sweeps=i["sweeps"], matvecs=i["matvecs"], max_bond=i["max_bond"],
                      local_solves=i["local_solves"], gemm_solves=i["gemm_solves"], residual=i["residual"], **(extra or {}), **stats(t)))

    rng = np.random.default_rng(2026)
    if "routes" in args.only:
        for n in (int(v) for v in args.lengths.split(",")):
            for dt in (np.float64, np.complex128):
                cb = [min(4, 2 ** min(i + 1, n - 1 - i)) for i in range(n - 1)]
                c = qil.SignalMPS.alloc(cb, dtype=dt).fill_random(5)
                for chi in (int(v) for v in args.bonds.split(",")):
                    xb = [min(chi, 2 ** min(i + 1, n - 1 - i)) for i in range(n - 1)]
                    x0 = qil.SignalMPS.alloc(xb, dtype=dt).fill_random(9)
                    for D in (int(v) for v in args.op_bonds.split(",")):
                        A, shift = operator(D, n, dt, rng)
                        mid = n // 2 - 1
                        ab = [1] + list(A.bond_dims) + [1]
                        fits = qil.solve_local_fits(([1] + xb + [1])[mid], ([1] + xb + [1])[mid + 2], ab[mid], ab[mid + 1], ab[mid + 2],
                                                    ([1] + cb + [1])[mid], ([1] + cb + [1])[mid + 1], ([1] + cb + [1])[mid + 2], dtype=dt)
                        run = lambda: qil.solve(A, c, x0=x0, shift=shift, maxdim=chi, cutoff=0.0, tol=1e-8, max_sweeps=1, cg_iters=30,
                                                return_info=True)
                        compare(f"sweep_n{n}_chi{chi}_D{D}_{np.dtype(dt).name}", run, dict(mid_bond_fits=bool(fits)))
    if "exp40" in args.only:
        import solve_model as SM
        d = SM.case("exp40")
        A, c = qil.SingleSiteMPO(d["A"]), qil.SignalMPS(d["c"])
        compare("exp40", lambda: qil.solve(A, c, return_info=True, **d["kwargs"]))
    if "example" in args.only:
        import smooth_fill as SF
        y, mask, _ = SF.operands()
        compare("example_smooth_fill_n40", lambda: SF.run(y, mask))


if __name__ == "__main__":
    main()
