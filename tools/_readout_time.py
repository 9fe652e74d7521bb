"""Times of the read-out verbs on one GPU, one line per route at the shapes the route comments of readout_route quote: call time
by HIP events around the whole call (bit upload, the launches, the download and the host work between them), ten repetitions
after two warm-up calls, median and range.

  few_queries   coefficient_batch (CHAIN below bond 128, GEMM_SORTED from there) and marginal_batch (GEMM_SELECT) of 16 queries on
                40 complex sites, bonds 64, 128 and 512
  grid65536     coefficient_batch of 65,536 queries on 16 complex sites, bond 23 (the many-rows arm of GEMM_SORTED)
  lazy          apply_coefficient_batch of 64 queries on 12 complex sites: chi D = 32 x 16 = 512 (LAZY_CHAIN), 32 x 32 = 1024 (LAZY_GEMM)
  to_vector     mps_to_vector at n = 20, bond 64, complex (the dense block)
  sweep64       apply_coefficient_sweep of the 64 damping operators of the n = 24 sweep workload at 1024 samples (lock-step batch)

Public API only, so it runs unchanged against another build of the library through QILHIP_LIB; --tag names the library in the lines.
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
import qilaplace_jl_amd as qil  # noqa: E402
from helpers import saturated_profile  # noqa: E402

Z = np.complex128


def timed(ctx, fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = qil.default_context()
    box = {"host": socket.gethostname()}

    def emit(case, verb, route, fn, **more):
        ts = timed(ctx, fn, args.reps)
        rec = dict(case=case, verb=verb, route=route, ms_median=float(np.median(ts)), ms_min=float(min(ts)), ms_max=float(max(ts)),
                   lib=args.tag, reps=args.reps, **more, **box)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    rng = np.random.default_rng(2025)
    n = 40
    for bond in (64, 128, 512):
        prof = saturated_profile(n, bond)
        psi = qil.SignalMPS.alloc(prof, dtype=Z, amplitude=1.5).fill_random(3)
        bits = rng.integers(0, 2, size=(16, n)).astype(np.uint8)
        summed = bits.copy()
        summed[:, ::3] = 2
        dims = [1] + list(prof) + [1]
        emit(f"few_queries_n40_bond{bond}_nb16", "coefficient_batch", qil.readout_route("plain", 16, dims)[0],
             lambda: qil.coefficient_batch(psi, bits))
        emit(f"few_queries_n40_bond{bond}_nb16", "marginal_batch", qil.readout_route("marginal", 16, dims)[0],
             lambda: qil.marginal_batch(psi, summed))
        del psi
    n = 16
    prof = saturated_profile(n, 23)
    psi = qil.SignalMPS.alloc(prof, dtype=Z, amplitude=1.5).fill_random(4)
    bits = rng.integers(0, 2, size=(65536, n)).astype(np.uint8)
    emit("grid65536_n16_bond23", "coefficient_batch", qil.readout_route("plain", 65536, [1] + list(prof) + [1])[0],
         lambda: qil.coefficient_batch(psi, bits))
    n = 12
    pprof = saturated_profile(n, 32)
    psi = qil.SignalMPS.alloc(pprof, dtype=Z, amplitude=1.5).fill_random(5)
    bits = rng.integers(0, 2, size=(64, n)).astype(np.uint8)
    for D in (16, 32):
        wprof = saturated_profile(n, D, base=4)
        W = qil.SingleSiteMPO.alloc(wprof, dtype=Z).fill_random(6)
        route = qil.readout_route("lazy", 64, [1] + list(pprof) + [1], [1] + list(wprof) + [1], dtype=Z)[0]
        emit(f"lazy_n12_chi32_D{D}_nb64", "apply_coefficient_batch", route, lambda: qil.apply_coefficient_batch(W, psi, bits))
    n = 20
    psi = qil.SignalMPS.alloc(saturated_profile(n, 64), dtype=Z, amplitude=1.5).fill_random(7)
    emit("to_vector_n20_bond64", "mps_to_vector", "block", lambda: qil.mps_to_vector(psi))
    import bench
    n = 24
    psi = qil.signal_ztmps(bench.truncate_signal(n), method="rsvd", k=15, p=5, q=2, cutoff=1e-12)
    Ws = qil.build_dt_mpo_batch(psi, np.linspace(0.25, 16.0, 64))
    bits = rng.integers(0, 2, size=(1024, 2 * n)).astype(np.uint8)
    emit("sweep64_n24_nb1024", "apply_coefficient_sweep", "sweep", lambda: qil.apply_coefficient_sweep(Ws, psi, bits))


if __name__ == "__main__":
    main()
