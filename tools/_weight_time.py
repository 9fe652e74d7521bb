"""Times of the Born weights (qil.weight_batch) on one GPU: call time by HIP events around the whole call (spec upload, the
launches, the read-back and the host work between them), ten repetitions after two warm-up calls, median and range.

  rows64      64 rows of the zt_row_weights shape (copy register fixed, main register traced) in ONE call on an n = 24 paired
              (48 tensors) `fill_random` state, next to the same 64 numbers by `zt_row` + `norm` one at a time -- the route that
              existed before.  Three states: bonds 64 c64 (above the LDS limit of 48: the GEMM route either way), bonds 64 f64
              and bonds 48 c64 (both walk in LDS).
  band40      `range_weight` of one arbitrary band on an n = 40, bonds 32, c64 SignalMPS (45 dyadic blocks, one call).

With QIL_WEIGHT_NO_LDS=1 in the environment the library sends every state through the GEMM route: run the script once with and
once without it, alternately, for the A/B of the walk kernel.  One JSON line per measurement on stdout (and appended to --out);
--tag names the route in the lines."""
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


def timed(ctx, fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return ts


def gpu_name():
    try:
        out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
        names = [l.split(":", 1)[1].strip() for l in out.splitlines() if "Marketing Name" in l]
        names = [v for v in names if v]
        return next((v for v in names if "Instinct" in v or "MI3" in v), names[-1] if names else "unknown")
    except (OSError, subprocess.SubprocessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = qil.default_context()
    box = {"gpu": gpu_name(), "host": socket.gethostname(), "no_lds_env": os.environ.get("QIL_WEIGHT_NO_LDS", "")}

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
    rng = np.random.default_rng(2024)
    ls = [int(v) for v in rng.integers(0, 2 ** n, size=64)]
    for bond, dt in ((64, np.complex128), (64, np.float64), (48, np.complex128)):
        psi = qil.ZTMPS.alloc(saturated_profile(2 * n, bond), dtype=dt, amplitude=2.5).fill_random(5)
        one_call = lambda: qil.zt_row_weights(psi, ls)
        one_by_one = lambda: np.array([(psi.amplitude * qil.norm(qil.zt_row(psi, l))) ** 2 for l in ls])
        got, ref = one_call(), one_by_one()
        rel = float(np.max(np.abs(got - ref) / ref))
        name = f"rows64_n24_paired_bond{bond}_{np.dtype(dt).name}"
        emit(dict(case=name, route="weight_batch", rel_dev_vs_restrict_norm=rel, **stats(timed(ctx, one_call, args.reps))))
        emit(dict(case=name, route="restrict+norm x 64", **stats(timed(ctx, one_by_one, args.reps))))
    n = 40
    psi = qil.SignalMPS.alloc(saturated_profile(n, 32), dtype=np.complex128, amplitude=1.5).fill_random(7)
    lo, hi = 0x1234567891, 0xC0FFEE1235
    blocks = len(qil.ops._dyadic_blocks(lo, hi, n))
    band = lambda: qil.range_weight(psi, lo, hi)
    total = qil.weight(psi, np.full(n, qil.ops.TRACE))
    emit(dict(case="band40_n40_bond32_complex128", route="range_weight", blocks=blocks, share_of_total=band() / total,
              **stats(timed(ctx, band, args.reps))))


if __name__ == "__main__":
    main()
