"""Times of the overlap entries on one GPU (HIP events around calls that end in their one read-back, after warm-up):
inner on both routes for an n = 30 chi = 64 pair, the route crossover scan, <phi|W psi> and norm(W psi) at cfg3 shapes next
to the materialised route.  Flops are counted from the shapes (8 per complex MAC, 2 per real MAC; the conventional count
of DESIGN 3.4).  One JSON line per measurement on stdout (and in --out)."""
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


def inner_flops(pb, sb, cx):
    d = [1] + list(pb) + [1]
    e = [1] + list(sb) + [1]
    macs = sum(d[i] * e[i] * 2 * e[i + 1] + d[i + 1] * 2 * d[i] * e[i + 1] for i in range(len(d) - 1))
    return macs * (8 if cx else 2)


def apply_inner_flops(pb, wb, sb):
    p, w, s = [1] + list(pb) + [1], [1] + list(wb) + [1], [1] + list(sb) + [1]
    macs = 0
    for i in range(len(p) - 1):
        macs += p[i] * w[i] * s[i] * 2 * s[i + 1]               # E A_psi
        macs += s[i + 1] * p[i] * 2 * w[i] * 2 * w[i + 1]       # T1_beta W
        macs += p[i + 1] * w[i + 1] * s[i + 1] * 2 * p[i]       # A_phi^H T2
    return 8 * macs


def apply_norm_flops(wb, sb):
    w, s = [1] + list(wb) + [1], [1] + list(sb) + [1]
    macs = 0
    for i in range(len(w) - 1):
        sl, sr, Dl, Dr = s[i], s[i + 1], w[i], w[i + 1]
        macs += sl * Dl * Dl * sl * 2 * sr + sr * sl * Dl * 2 * Dl * 2 * Dr + Dr * sr * sl * 2 * Dl * 2 * Dr + sr * 2 * sl * Dr * Dr * sr
    return 8 * macs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cfg3", action="store_true")
    args = ap.parse_args()
    ctx = qil.default_context()
    lines = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    def route_time(phi, psi, route, reps):
        os.environ["QIL_INNER_ROUTE"] = route
        try:
            return timed(ctx, lambda: qil.inner(phi, psi), reps)
        finally:
            os.environ.pop("QIL_INNER_ROUTE", None)

    # inner of an n = 30, chi = 64 pair (the shapes of encoded signals), both routes
    n = 30
    for dt in (np.float64, np.complex128):
        b = saturated_profile(n, 64)
        phi = qil.SignalMPS.alloc(b, dtype=dt).fill_random(1)
        psi = qil.SignalMPS.alloc(b, dtype=dt).fill_random(2)
        fl = inner_flops(b, b, dt == np.complex128)
        res = {}
        for route in ("chain", "gemm"):
            med, mn = route_time(phi, psi, route, args.reps)
            res[route] = med
            emit(what="inner_n30_chi64", dtype=np.dtype(dt).name, route=route, ms_median=med, ms_min=mn, gflop=fl / 1e9,
                 tflops=fl / med / 1e9)
        emit(what="inner_n30_chi64_speedup", dtype=np.dtype(dt).name, gemm_over_chain=res["gemm"] / res["chain"])

    # crossover scan: n = 30 saturated profiles, both routes
    for dt in (np.float64, np.complex128):
        for chi in (2, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64):
            b = saturated_profile(n, chi)
            phi = qil.SignalMPS.alloc(b, dtype=dt).fill_random(3)
            psi = qil.SignalMPS.alloc(b, dtype=dt).fill_random(4)
            tc, _ = route_time(phi, psi, "chain", args.reps)
            tg, _ = route_time(phi, psi, "gemm", args.reps)
            emit(what="inner_crossover", dtype=np.dtype(dt).name, n=n, chi=chi, chain_ms=tc, gemm_ms=tg, faster="chain" if tc < tg else "gemm")

    if args.skip_cfg3:
        return
    # cfg3 shapes: n = 24 paired (48 tensors), chi_s = 64, D = 128; phi on the saturated chi = 64 profile
    L = 48
    cb, db = saturated_profile(L, 64), saturated_profile(L, 128, base=4)
    psi = qil.ZTMPS.alloc(cb, dtype=np.float64, amplitude=1.0).fill_random(20240064)
    W = qil.PairedSiteMPO.alloc(db, dtype=np.complex128).fill_random(777)
    phi = qil.ZTMPS.alloc(cb, dtype=np.complex128, amplitude=1.0).fill_random(99)
    fl = apply_inner_flops(cb, db, cb)
    med, mn = timed(ctx, lambda: qil.inner(phi, W, psi), args.reps)
    emit(what="apply_inner_cfg3", ms_median=med, ms_min=mn, gflop=fl / 1e9, tflops=fl / med / 1e9,
         frac_of_peak=fl / med / 1e9 / PEAK_TFLOPS)
    lazy_ms = med

    def materialised():
        prod = W * psi
        v = qil.inner(phi, prod)
        del prod
        return v

    med_m, mn_m = timed(ctx, materialised, max(2, args.reps // 3))
    pb = [c * d for c, d in zip(cb, db)]
    emit(what="apply_then_inner_cfg3", ms_median=med_m, ms_min=mn_m, inner_gflop=inner_flops(cb, pb, True) / 1e9,
         lazy_speedup=med_m / lazy_ms)
    ctx.trim()
    fl = apply_norm_flops(db, cb)
    med, mn = timed(ctx, lambda: qil.apply_norm(W, psi), 3)
    emit(what="apply_norm_cfg3", ms_median=med, ms_min=mn, tflop=fl / 1e12, tflops=fl / med / 1e9,
         frac_of_peak=fl / med / 1e9 / PEAK_TFLOPS)
    if args.out:
        with open(args.out, "w") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
