"""Times of qil.environment and qil.esprit on one GPU: call time by HIP events around the whole call (the size query, the site
table, the launches, the download and the host work between them), ten repetitions after two warm-up rounds, median and range.
The two sides of every comparison alternate inside one process.

  routes    environment forced onto each route (QIL_ENV_ROUTE, read per call) on a right walk: state bonds chi in {4, 8, 16}
            (phi = psi), without an operator and with one of bond 2, count in {12, 38} tensors of a 40-tensor chain, f64 and c64;
            `default` names what the unforced call takes, chain_vs_gemm_rel the deviation between the routes
  esprit    esprit(maxdim=2) end to end on the n = 20 signal of examples/zoom_scan.py, next to a 128 x 128 zt_eval window on the
            same state (the tutorial's fine window), both with the pole error they reach; the encode is outside both timings

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
from helpers import random_mpo_data  # noqa: E402
from _product_time import gpu_name, timed_pair  # noqa: E402


def forced(route, fn):
    def run():
        if route is None:
            os.environ.pop("QIL_ENV_ROUTE", None)
        else:
            os.environ["QIL_ENV_ROUTE"] = route
        try:
            return fn()
        finally:
            os.environ.pop("QIL_ENV_ROUTE", None)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="routes,esprit")
    ap.add_argument("--bonds", default="4,8,16")
    ap.add_argument("--counts", default="12,38")
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

    n = 40
    rng = np.random.default_rng(2025)
    if "routes" in args.only:
        for chi in (int(v) for v in args.bonds.split(",")):
            for dt in (np.float64, np.complex128):
                bonds = [min(chi, 2 ** min(i + 1, n - 1 - i)) for i in range(n - 1)]
                psi = qil.SignalMPS.alloc(bonds, dtype=dt).fill_random(7)
                for D in (None, 2):
                    W = None if D is None else qil.SingleSiteMPO(random_mpo_data([D] * (n - 1), rng, dtype=dt), sites=psi.site_ids)
                    dims = [1] + bonds + [1]
                    for count in (int(v) for v in args.counts.split(",")):
                        run = lambda: qil.environment(psi, psi, W=W, side="right", count=count)
                        default = qil.ops.environment_route("right", count, dims, dims, None if D is None else [1] + [D] * (n - 1) + [1])
                        a, b = forced("chain", run)(), forced("gemm", run)()
                        dev = float(np.abs(a - b).max() / np.abs(b).max())
                        ts = timed_pair(ctx, {"chain": forced("chain", run), "gemm": forced("gemm", run)}, args.reps)
                        for name, t in ts.items():
                            emit(dict(case=f"routes_n40_chi{chi}_D{D or 0}_count{count}_{np.dtype(dt).name}", route=name,
                                      default=default.lower(), chain_vs_gemm_rel=dev, **stats(t)))
    if "esprit" in args.only:
        import zoom_scan as Z
        psi = qil.signal_mps(Z.tutorial_signal(), method="rsvd", k=50, p=5, q=2, cutoff=1e-12, maxdim=128)
        k, l = Z.fine_window()
        found = {}

        def by_esprit():
            poles, _ = qil.esprit(psi, maxdim=2)
            found["esprit"] = max(float(np.min(np.abs(1.0 / poles - p))) for p in Z.POLES)

        def by_window():
            found["zt_eval"] = Z.scan(psi, k, l)[3]

        ts = timed_pair(ctx, {"esprit": by_esprit, "zt_eval": by_window}, args.reps)
        for name, t in ts.items():
            emit(dict(case="poles_n20_tutorial_signal", route=name, pole_error=float(found[name]), bonds=max(psi.bond_dims), **stats(t)))


if __name__ == "__main__":
    main()
