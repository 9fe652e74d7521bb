"""Times of perfect sampling (qil.sample) on one GPU (HIP events around calls, median of --reps after warm-up): an n = 24
paired chain (48 tensors), chi = 64, c64 at nb = 2^12, 2^16, 2^20 on both routes; the environment build on its own (a call
with nb = 1); the route crossover at nb = 2^16 over chi; one GEMM-route point on a materialised product.

Model per site: flops 8 nb chi_l 2 chi_r (T = V A) + 8 nb 2 chi_r^2 (the quadratic forms) for c64, a quarter of
that for f64; bytes V read + V' written + A_i + R_i.  A call's time includes the environments and the download of the bit
rows and probabilities; `sweep_ms` subtracts the nb = 1 call.  One JSON line per measurement on stdout (and in --out)."""
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

PEAK_TFLOPS = 78.6   # f64 MFMA peak of one MI355X


def timed(ctx, fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return float(np.median(ts)), float(min(ts))


def sweep_model(bonds, nb, cx):
    """(flops, fused bytes) of the sampling sweep"""
    d = [1] + list(bonds) + [1]
    e = 16 if cx else 8
    fl = sum(8 * nb * d[i] * 2 * d[i + 1] + 8 * nb * 2 * d[i + 1] ** 2 for i in range(len(d) - 1))
    by = sum(nb * (d[i] + d[i + 1]) * e + 2 * d[i] * d[i + 1] * e + d[i + 1] ** 2 * e for i in range(len(d) - 1))
    return (fl if cx else fl / 4), by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = qil.default_context()
    lines = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    def route_time(psi, nb, route, reps):
        os.environ["QIL_SAMPLE_ROUTE"] = route
        try:
            return timed(ctx, lambda: qil.sample(psi, nb, seed=1, bits=True), reps)
        finally:
            os.environ.pop("QIL_SAMPLE_ROUTE", None)

    # n = 24 paired, chi = 64, c64
    L = 48
    b = saturated_profile(L, 64)
    psi = qil.ZTMPS.alloc(b, dtype=np.complex128).fill_random(20241016)
    env_ms, env_min = route_time(psi, 1, "fused", args.reps)
    emit(what="sample_env_n24p_chi64", dtype="complex128", ms_median=env_ms, ms_min=env_min)
    res = {}
    for lg in (12, 16, 20):
        nb = 2 ** lg
        fl, by = sweep_model(b, nb, True)
        for route in ("fused", "gemm"):
            med, mn = route_time(psi, nb, route, args.reps)
            sw = med - env_ms
            res[(lg, route)] = med
            emit(what="sample_n24p_chi64", dtype="complex128", nb=nb, route=route, ms_median=med, ms_min=mn, sweep_ms=sw,
                 samples_per_s=nb / med * 1e3, sweep_gflop=fl / 1e9, sweep_tflops=fl / sw / 1e9,
                 frac_of_peak=fl / sw / 1e9 / PEAK_TFLOPS, fused_model_gb=by / 1e9, fused_model_tbps=by / sw / 1e9)
        emit(what="sample_n24p_chi64_speedup", nb=nb, gemm_over_fused=res[(lg, "gemm")] / res[(lg, "fused")])

    # crossover: nb = 2^16, n = 24 paired, saturated profiles
    for dt in (np.float64, np.complex128):
        for chi in (4, 16, 32, 64, 128):
            bb = saturated_profile(L, chi)
            x = qil.ZTMPS.alloc(bb, dtype=dt).fill_random(chi)
            tf, _ = route_time(x, 2 ** 16, "fused", args.reps)
            tg, _ = route_time(x, 2 ** 16, "gemm", args.reps)
            emit(what="sample_crossover", dtype=np.dtype(dt).name, nb=2 ** 16, chi=chi, fused_ms=tf, gemm_ms=tg,
                 faster="fused" if tf < tg else "gemm")

    # GEMM route on a materialised product: n = 24 paired, chi_s = 32 times D = 32 (bonds up to 1024), nb = 2^12
    cb, db = saturated_profile(L, 32), saturated_profile(L, 32, base=4)
    s = qil.ZTMPS.alloc(cb, dtype=np.float64).fill_random(5)
    W = qil.PairedSiteMPO.alloc(db, dtype=np.complex128).fill_random(6)
    prod = W * s
    pb = prod.bond_dims
    nb = 2 ** 12
    fl, _ = sweep_model(pb, nb, True)
    e1, _ = timed(ctx, lambda: qil.sample(prod, 1, seed=1, bits=True), 3)
    med, mn = timed(ctx, lambda: qil.sample(prod, nb, seed=1, bits=True), 3)
    emit(what="sample_product_gemm", max_bond=int(max(pb)), nb=nb, ms_median=med, ms_min=mn, env_ms=e1, sweep_ms=med - e1,
         sweep_gflop=fl / 1e9, sweep_tflops=fl / (med - e1) / 1e9, frac_of_peak=fl / (med - e1) / 1e9 / PEAK_TFLOPS)
    del prod
    if args.out:
        with open(args.out, "w") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
