"""Times of the MPS-valued restriction (qil.restrict) on one GPU: call time by HIP events around one call (descriptor upload +
the grouped launches), ten repetitions after two warm-up calls, median and range, on the n = 24 paired (48 tensors), chi = 64,
c64 `fill_random` state:

  zt_row, copy_marginal   24 kept sites, 24 runs of length 1 read in place: ONE launch.  Next to the time, the bytes the call
                          must move (every parent tensor read once, every kept tensor written once) and the fraction of the
                          8 TB/s HBM spec they make.
  zoom, decimate          the first / the last 12 sites fixed: one leading / trailing run of 12 factors through the run kernel
                          (or, with a library built with -DQIL_RESTRICT_LDS_MAX_F64=0 -DQIL_RESTRICT_LDS_MAX_C64=0 and named
                          by QILHIP_LIB, through the GEMM route), then the grouped launch.

One JSON line per measurement on stdout (and appended to --out); --tag names the library in the lines."""
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

HBM_SPEC = 8.0e12
FREE, SUM = qil.ops.FREE, qil.ops.SUM


def timed(ctx, fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return ts


def chain_bytes(bonds, itemsize, sites=None):
    d = [1] + list(bonds) + [1]
    return sum(d[i] * 2 * d[i + 1] for i in (range(len(d) - 1) if sites is None else sites)) * itemsize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = qil.default_context()
    n = 24
    psi = qil.ZTMPS.alloc(saturated_profile(2 * n, 64), dtype=np.complex128).fill_random(5)
    pb = psi.bond_dims
    zoom = np.full(2 * n, FREE, dtype=np.uint8)
    zoom[:12] = [0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1]
    decimate = np.full(2 * n, FREE, dtype=np.uint8)
    decimate[-12:] = [1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0]
    cases = {
        "zt_row": lambda: qil.zt_row(psi, 0x5A5A5A),
        "copy_marginal": lambda: qil.copy_marginal(psi),
        "zoom": lambda: qil.restrict(psi, zoom),
        "decimate": lambda: qil.restrict(psi, decimate),
    }

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for name, call in cases.items():
        ts = timed(ctx, call, args.reps)
        out = call()
        rec = {"case": name, "lib": args.tag, "ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts),
               "reps": args.reps, "kept": out.ntensors if isinstance(out, qil.ZTMPS) else len(out)}
        if name in ("zt_row", "copy_marginal"):
            moved = chain_bytes(pb, 16) + chain_bytes(out.bond_dims, 16)
            rec["bytes_moved"] = moved
            rec["fraction_of_hbm_spec"] = moved / (np.median(ts) * 1e-3) / HBM_SPEC
        emit(rec)


if __name__ == "__main__":
    main()
