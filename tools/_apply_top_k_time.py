"""Times of the lazy top-k search (qil.apply_top_k) on one GPU, on both of its scoring routes (QIL_APPLY_SAMPLE_ROUTE=fused /
gemm), against the way to the same answer that existed before, `top_k(apply(W, psi))` with the product's time included: call time
by HIP events around the whole call (uploads, launches, the read-back and the host work between them), --reps repetitions after
two warm-up calls (3 where one call takes more than 0.3 s), median and range.  k = 16 at beam 2^12 and 2^14 (the operands' beam
cap where that is smaller: 10904 at chi D = 2048, c64), the same beam on the materialised route; each record also
carries whether the rows are the materialised route's, the largest relative difference of the values, both bounds and whether
either result is certified.

  (a) natural zT  a damped two-tone signal of 2^20 samples as a ZTMPS under build_zt_mpo(psi, 2 pi): 40 tensors at their natural
                  bonds (the operands of tools/_apply_sample_time.py (a))
  (b) natural QFT three damped modes of 2^24 samples (exponential_sum) under build_qft_mpo: 24 tensors at their natural bonds
  (c) synthetic   24 tensors, fill_random, chi 32 under D 64, paired, c64: the product's sites are 2048 x 2 x 2048

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

ROUTE = "QIL_APPLY_SAMPLE_ROUTE"
RENV = "QIL_APPLY_SAMPLE_RENV_BYTES"
K = 16
BEAMS = (2 ** 12, 2 ** 14)


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
    ap.add_argument("--cases", default="a,b,c")
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

    def compare(name, W, psi):
        chi, D = [1] + psi.bond_dims + [1], [1] + W.bond_dims + [1]
        e = 16 if np.complex128 in (psi.dtype, W.dtype) else 8
        env = e * sum((c * d) ** 2 for c, d in zip(chi[1:-1], D[1:-1]))
        case = dict(name=name, tensors=len(chi) - 1, chi=max(chi), D=max(D), P=max(c * d for c, d in zip(chi, D)), k=K,
                    env_bytes=env, product_bytes=2 * e * sum(chi[i] * D[i] * chi[i + 1] * D[i + 1] for i in range(len(chi) - 1)))
        if env > 16 << 30:
            os.environ[RENV] = str(env)
        try:
            cap = min(2 ** 29, 2 ** 30 // (3 * case["P"] * e + 4 * case["tensors"] + 64))      # the header's beam cap, restated
            for beam in sorted({min(b, cap) for b in BEAMS}):
                formed = lambda: qil.top_k(qil.apply(W, psi), K, beam=beam, bits=True)
                fr, fv, fb, fc = formed()
                emit(dict(case=case, beam=beam, route="apply + top_k", bound=fb, certified=fc, **stats(timed(ctx, formed, args.reps))))
                for route in ("gemm", "fused", None):
                    if route is None:
                        os.environ.pop(ROUTE, None)
                    else:
                        os.environ[ROUTE] = route
                    lazy = lambda: qil.apply_top_k(W, psi, K, beam=beam, bits=True)
                    r, v, b, c = lazy()
                    same = bool(np.array_equal(r, fr))
                    rel = float(np.max(np.abs(v - fv) / np.abs(fv))) if same else None
                    emit(dict(case=case, beam=beam, route="lazy " + (route or "default"), rows_same=same, value_rel_dev=rel, bound=b,
                              certified=c, **stats(timed(ctx, lazy, args.reps))))
        finally:
            os.environ.pop(ROUTE, None)
            os.environ.pop(RENV, None)

    wanted = args.cases.split(",")
    if "a" in wanted:
        n = 20
        N = 2 ** n
        j = np.arange(N, dtype=np.float64)
        x = np.sin(2 * np.pi * 5.0 * j / N) * np.exp(-3.0 * j / N) + 0.5 * np.cos(2 * np.pi * 11.0 * j / N)
        psi = qil.signal_ztmps(x, cutoff=1e-12)
        compare("a_zt_n20", qil.build_zt_mpo(psi, 2 * np.pi), psi)
    if "b" in wanted:
        n = 24
        N = 2 ** n
        modes = [(250.3, 8e-9, 1.0), (1250.7, 4e-8, 0.8), (3000.5, 2e-8, 0.5)]             # (bin, damping per sample, amplitude)
        psi = qil.exponential_sum([a for _, _, a in modes], [np.exp(-g + 2j * np.pi * f / N) for f, g, _ in modes], n)
        compare("b_qft_n24", qil.build_qft_mpo(psi), psi)
    if "c" in wanted:
        psi = qil.ZTMPS.alloc(saturated_profile(24, 32), dtype=np.complex128, amplitude=2.5).fill_random(5)
        W = qil.PairedSiteMPO.alloc(saturated_profile(24, 64, 4), dtype=np.complex128).fill_random(6)
        compare("c_chi32_D64", W, psi)


if __name__ == "__main__":
    main()
