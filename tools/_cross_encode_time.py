"""Times of the cross-interpolation encoder (qil.signal_mps_cross) against signal_mps(:svd) and signal_mps(:rsvd) on the same
device-resident structured signal, on one GPU: call time by HIP events around the whole call, --reps repetitions after two
warm-up calls, median and range.

  (a) encoders   x(t) = exp(-((t - 0.4) / 0.08)^2 / 2) cos(2 pi (5 t + 20 t^2)), t = k / N, float64 in HBM, at every n of --sizes
                 (default 24, 30): cross (maxdim 64, tol 1e-9; with the samples read, the sweeps and the time per half-sweep =
                 time / (2 sweeps + 1)), then :svd and :rsvd at cutoff 1e-15 / maxdim 64, and the max-norm distance of the cross
                 result from the signal at 4096 random samples
  (b) routes     QIL_CROSS_ROUTE=lds against =global on full-rank random signals of 2^16 samples whose blocks are 2 maxdim wide:
                 maxdim 16, 32, 64, 128 -> blocks of 32 .. 256 (f64; a 256 x 256 block is 512 KiB and takes the global route under
                 either switch, which the record says)

One JSON line per measurement on stdout (and appended to --out)."""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qilaplace_jl_amd as qil  # noqa: E402

ROUTE = "QIL_CROSS_ROUTE"


def structured_signal(n):
    """The signal of (a) as a float64 device tensor, filled in pieces so that the temporaries stay small."""
    N = 2 ** n
    x = torch.empty(N, dtype=torch.float64, device="cuda")
    piece = min(N, 1 << 24)
    for lo in range(0, N, piece):
        t = (torch.arange(lo, lo + piece, dtype=torch.float64, device="cuda")) / float(N)
        x[lo:lo + piece] = torch.exp(-0.5 * ((t - 0.4) / 0.08) ** 2) * torch.cos(2 * np.pi * (5 * t + 20 * t * t))
    torch.cuda.synchronize()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--sizes", default="24,30")
    args = ap.parse_args()
    ctx = qil.default_context()
    box = {"gpu": torch.cuda.get_device_name(0), "host": socket.gethostname()}

    def emit(rec):
        rec = dict(rec, **box)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def timed(fn, reps):
        for _ in range(2):
            out = fn()
        ts = []
        for _ in range(reps):
            ctx.timer_start()
            out = fn()
            ts.append(ctx.timer_stop())
        return out, dict(ms_median=float(np.median(ts)), ms_min=float(min(ts)), ms_max=float(max(ts)), reps=len(ts))

    wanted = args.cases.split(",")
    if "a" in wanted:
        for n in [int(s) for s in args.sizes.split(",")]:
            x = structured_signal(n)
            (psi, info), t = timed(lambda: qil.signal_mps_cross(x, maxdim=64, tol=1e-9, return_info=True), args.reps)
            idx = np.random.default_rng(9).integers(0, 2 ** n, size=4096, dtype=np.int64)
            bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
            want = x[torch.from_numpy(idx).cuda()].cpu().numpy()
            err = float(np.abs(qil.coefficient_batch(psi, bits) - want).max())
            emit(dict(case="a_encoders", encoder="cross", n=n, bonds_max=max(psi.bond_dims), max_err_4096=err,
                      ms_per_half_sweep=t["ms_median"] / (2 * info["sweeps"] + 1), **info, **t))
            del psi
            for method in ("svd", "rsvd"):
                ref, t = timed(lambda: qil.signal_mps(x, method=method, cutoff=1e-15, maxdim=64), args.reps)
                err = float(np.abs(qil.coefficient_batch(ref, bits) - want).max())
                emit(dict(case="a_encoders", encoder=method, n=n, bonds_max=max(ref.bond_dims), max_err_4096=err, **t))
                del ref
            del x
            ctx.trim()
            torch.cuda.empty_cache()
    if "b" in wanted:
        n = 16
        rng = np.random.default_rng(4)
        x = torch.from_numpy(rng.standard_normal(2 ** n)).cuda()
        try:
            for maxdim in (16, 32, 64, 128):
                for route in ("lds", "global"):
                    os.environ[ROUTE] = route
                    (psi, info), t = timed(lambda: qil.signal_mps_cross(x, maxdim=maxdim, tol=1e-9, max_sweeps=2, return_info=True),
                                           args.reps)
                    fits = (2 * maxdim) ** 2 * 8 <= 144 * 1024
                    emit(dict(case="b_routes", route=route, route_taken_by_the_largest_block=route if fits else "global", n=n,
                              maxdim=maxdim, block=2 * maxdim, ms_per_half_sweep=t["ms_median"] / (2 * info["sweeps"] + 1), **info, **t))
        finally:
            os.environ.pop(ROUTE, None)


if __name__ == "__main__":
    main()
