"""Times and figures of the operator algebra (qil.mpo_inner, qil.mpo_linear_combination) on one GPU.  Call times by HIP events
around the whole call, ten repetitions after two warm-up calls, median and range; the two sides of a comparison alternate inside
one process.

  routes     mpo_inner forced onto each route (QIL_MPO_INNER_ROUTE, read per call) at n = 24 tensors, f64 and c64, saturated
             bonds capped at 8, 12, 16, 20, 24, 32 and 64: the crossover of the auto rule is the largest cap at which the chain
             route is not slower than the GEMM route in both dtypes.
  store      mpo_linear_combination of 8 terms of bond 64 on 24 tensors, c64 and f64: bytes written / kernel time (the kernel
             profile of the context), next to qil_hbm_store_peak in the same process and to linear_combination of 8 states of
             bond 64 (the same kernel on MPS-shaped sites).
  figures    what the verbs are for: <F, F>/2^n - 1 of build_qft_mpo at n = 10 and 24 and |F^dagger F - I|_F through the product,
             mpo_distance between QFT builds at cutoff 1e-14 and 1e-10, and mpo_distance between the persistent and the launch-per-step DT builder routes
             (QIL_DT_BUILDER=launches) at cutoff 0 for one damping value at n = 24.

One JSON line per measurement on stdout (and appended to --out)."""
import argparse
import json
import os
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qilaplace_jl_amd as qil  # noqa: E402
from helpers import saturated_profile  # noqa: E402


def timed_pair(ctx, fns, reps):
    """{name: times}, the functions alternating repetition by repetition after two warm-up rounds."""
    for _ in range(2):
        for fn in fns.values():
            fn()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ctx.timer_start()
            fn()
            ts[name].append(ctx.timer_stop())
    return ts


def gpu_name():
    try:
        out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
        names = [l.split(":", 1)[1].strip() for l in out.splitlines() if "Marketing Name" in l]
        names = [v for v in names if v]
        return next((v for v in names if "Instinct" in v or "MI3" in v), names[-1] if names else "unknown")
    except (OSError, subprocess.SubprocessError):
        return "unknown"


def with_env(name, value, fn):
    def run():
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        try:
            return fn()
        finally:
            os.environ.pop(name, None)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="routes,store,figures")
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

    n = 24

    def operator(bond, dt, seed):
        return qil.SingleSiteMPO.alloc(saturated_profile(n, bond, base=4), dtype=dt).fill_random(seed)

    if "routes" in args.only:
        for bond in (8, 12, 16, 20, 24, 32, 64):
            for dt in (np.float64, np.complex128):
                V, W = operator(bond, dt, 7), operator(bond, dt, 8)
                run = lambda: qil.mpo_inner(V, W)
                chain, gemm = with_env("QIL_MPO_INNER_ROUTE", "chain", run), with_env("QIL_MPO_INNER_ROUTE", "gemm", run)
                a, b = chain(), gemm()
                scale = qil.mpo_norm(V) * qil.mpo_norm(W)
                ts = timed_pair(ctx, {"chain": chain, "gemm": gemm}, args.reps)
                for name, t in ts.items():
                    emit(dict(case=f"routes_n24_bond{bond}_{np.dtype(dt).name}", route=name,
                              chain_vs_gemm_of_scale=float(abs(a - b) / scale), **stats(t)))
    if "store" in args.only:
        peak, writer = ctx.hbm_store_peak(nbytes=2 << 30, reps=5)
        emit(dict(case="hbm_store_peak", gbps=peak, writer=writer))
        for dt in (np.complex128, np.float64):
            es = np.dtype(dt).itemsize
            ops = [operator(64, dt, 20 + j) for j in range(8)]
            sts = [qil.SignalMPS.alloc(saturated_profile(n, 64), dtype=dt).fill_random(40 + j) for j in range(8)]
            c = list(np.linspace(0.5, 1.5, 8))
            for verb, fn, terms, phys in (("mpo_sum", qil.mpo_linear_combination, ops, 4), ("mps_sum", qil.linear_combination, sts, 2)):
                dims = [1] + [8 * b for b in terms[0].bond_dims] + [1]
                nbytes = sum(dims[i] * phys * dims[i + 1] for i in range(n)) * es
                for _ in range(2):
                    fn(terms, c)
                ctx.synchronize()
                ms = []
                for _ in range(args.reps):
                    ctx.profile_enable(True)
                    out = fn(terms, c)
                    ctx.synchronize()
                    launches, t = ctx.profile_read(reset=True)
                    ctx.profile_enable(False)
                    assert launches == 1, launches
                    ms.append(t)
                    del out
                med = float(np.median(ms))
                emit(dict(case=f"store_8x_bond64_n24_{np.dtype(dt).name}", verb=verb, bytes_written=int(nbytes), kernel_ms_median=med,
                          kernel_ms_min=float(min(ms)), kernel_ms_max=float(max(ms)), gbps=nbytes / med / 1e6,
                          of_store_peak=nbytes / med / 1e6 / peak))
            del ops, sts
    if "figures" in args.only:
        for nq in (10, 24):
            Fa, Fb = qil.build_qft_mpo(nq, cutoff=1e-14), qil.build_qft_mpo(nq, cutoff=1e-10)
            ff = qil.mpo_inner(Fa, Fa)
            emit(dict(case=f"qft_n{nq}", unitarity_FF_over_2n_minus_1=float(np.real(ff) / 2.0 ** nq - 1.0), imag=float(np.imag(ff)),
                      bonds_1e14=max(Fa.bond_dims), bonds_1e10=max(Fb.bond_dims),
                      distance_1e14_vs_1e10=qil.mpo_distance(Fa, Fb), norm=qil.mpo_norm(Fa),
                      distance_floor=float(np.sqrt(64 * np.finfo(np.float64).eps * 2 * 2.0 ** nq))))
            # <F, F> is the norm alone; the unitarity proper is |F^dagger F - I|_F, through the product and the distance
            G = qil.apply(qil.adjoint(Fa), Fa)
            emit(dict(case=f"qft_n{nq}_unitarity", bonds_product=max(G.bond_dims),
                      distance_FdF_to_identity=qil.mpo_distance(G, qil.SingleSiteMPO.identity(nq)),
                      distance_floor=float(np.sqrt(64 * np.finfo(np.float64).eps * 2 * 2.0 ** nq))))
        wr = 0.5
        Wp = qil.build_dt_mpo(n, wr, cutoff=0.0)
        Wl = with_env("QIL_DT_BUILDER", "launches", lambda: qil.build_dt_mpo(n, wr, cutoff=0.0))()
        nrm = qil.mpo_norm(Wp)
        emit(dict(case="dt_builder_routes_n24_cutoff0", wr=wr, bonds_persistent=max(Wp.bond_dims), bonds_launches=max(Wl.bond_dims),
                  distance=qil.mpo_distance(Wp, Wl), norm_persistent=nrm, norm_launches=qil.mpo_norm(Wl),
                  overlap=complex(qil.mpo_inner(Wp, Wl)).real,
                  distance_floor=float(np.sqrt(64 * np.finfo(np.float64).eps * 2) * nrm)))


if __name__ == "__main__":
    main()
