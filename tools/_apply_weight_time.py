"""Times of the lazy Born weights (qil.apply_weight_batch) on one GPU against the ways to the same numbers that existed before,
`weight_batch(apply(W, psi))` and `weight_batch(apply_compress(W, psi))`: call time by HIP events around the whole call (uploads,
launches, the read-back and the host work between them), --reps repetitions after two warm-up calls (3 where one call takes more
than 0.3 s), median and range.

  (a) natural   a damped two-tone signal of 2^20 samples as a ZTMPS (bonds <= 4) under build_zt_mpo(psi, 2 pi) (40 tensors):
                64 row energies (`apply_zt_row_weights`: the copy register fixed, the main one traced -- every tensor a density
                step) and one band of the 40-tensor index (`apply_range_weight`: prefix-fixed rows -- a vector phase and one
                quadratic form each).
  (b) synthetic 20 tensors, `fill_random`, chi 32 (f64) under D 64 (c64), paired: 1 and 8 row energies.  The product has bond
                2048; apply_compress is not timed here (it truncates a random state).
  (c) budget    the band of (a) with QIL_APPLY_WEIGHT_RENV_BYTES=0 (no right environment kept: every tail walked) against the
                default.

One JSON line per measurement on stdout (and appended to --out)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qilaplace_jl_amd as qil  # noqa: E402
from helpers import saturated_profile  # noqa: E402

RENV = "QIL_APPLY_WEIGHT_RENV_BYTES"


def timed(ctx, fn, reps):
    fn()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    if time.perf_counter() - t0 > 0.3:
        reps = min(reps, 3)
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-synthetic", action="store_true")
    args = ap.parse_args()
    ctx = qil.default_context()
    box = {"gpu": gpu_name(), "host": socket.gethostname()}

    def emit(rec):
        rec = dict(rec, **box)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def stats(ts):
        return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "reps": len(ts)}

    def compare(case, lazy, formed, compressed=None):
        got, ref = np.atleast_1d(lazy()), np.atleast_1d(formed())
        rel = float(np.max(np.abs(got - ref) / np.abs(ref).max()))
        emit(dict(case=case, route="lazy", dev_vs_formed=rel, **stats(timed(ctx, lazy, args.reps))))
        emit(dict(case=case, route="apply + weight_batch", **stats(timed(ctx, formed, args.reps))))
        if compressed is not None:
            dev = float(np.max(np.abs(np.atleast_1d(compressed()) - ref) / np.abs(ref).max()))
            emit(dict(case=case, route="apply_compress + weight_batch", dev_vs_formed=dev, **stats(timed(ctx, compressed, args.reps))))

    # ---- (a) the natural zT operand
    n = 20
    N = 2 ** n
    j = np.arange(N, dtype=np.float64)
    x = np.sin(2 * np.pi * 5.0 * j / N) * np.exp(-3.0 * j / N) + 0.5 * np.cos(2 * np.pi * 11.0 * j / N)
    psi = qil.signal_ztmps(x, cutoff=1e-12)
    W = qil.build_zt_mpo(psi, 2 * np.pi)
    rng = np.random.default_rng(2024)
    ls = [int(v) for v in rng.integers(0, N, size=64)]
    shape = dict(n=n, chi=max(psi.bond_dims), D=max(W.bond_dims))
    compare(dict(name="a_rows64", **shape), lambda: qil.apply_zt_row_weights(W, psi, ls),
            lambda: qil.zt_row_weights(qil.apply(W, psi), ls), lambda: qil.zt_row_weights(qil.apply_compress(W, psi), ls))
    lo, hi = 0x1234567891, 0xC0FFEE1235
    blocks = len(qil.ops._dyadic_blocks(lo, hi, 2 * n))
    band = lambda: qil.apply_range_weight(W, psi, lo, hi)
    compare(dict(name="a_band", blocks=blocks, **shape), band, lambda: qil.range_weight(qil.apply(W, psi), lo, hi),
            lambda: qil.range_weight(qil.apply_compress(W, psi), lo, hi))
    # ---- (c) the same band without kept right environments
    kept = band()
    os.environ[RENV] = "0"
    try:
        walked = band()
        emit(dict(case=dict(name="c_band_budget0", blocks=blocks, **shape), route="lazy, no R_k kept",
                  dev_vs_default=abs(walked - kept) / abs(kept), **stats(timed(ctx, band, args.reps))))
    finally:
        del os.environ[RENV]
    emit(dict(case=dict(name="c_band_default", blocks=blocks, **shape), route="lazy", **stats(timed(ctx, band, args.reps))))
    if args.skip_synthetic:
        return
    # ---- (b) synthetic, wide
    m = 10
    psi = qil.ZTMPS.alloc(saturated_profile(2 * m, 32), dtype=np.float64, amplitude=2.5).fill_random(5)
    W = qil.PairedSiteMPO.alloc(saturated_profile(2 * m, 64, 4), dtype=np.complex128).fill_random(6)
    shape = dict(n=2 * m, chi=max(psi.bond_dims), D=max(W.bond_dims))
    ls = [int(v) for v in rng.integers(0, 2 ** m, size=8)]
    for rows in (1, 8):
        sel = ls[:rows]
        compare(dict(name=f"b_rows{rows}", **shape), lambda: qil.apply_zt_row_weights(W, psi, sel),
                lambda: qil.zt_row_weights(qil.apply(W, psi), sel))


if __name__ == "__main__":
    main()
