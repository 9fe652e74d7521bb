"""Times of the product-vector read-out (qil.product_batch) on one GPU: call time by HIP events around the whole call (weight
scan and upload, the launches, the read-back and the host work between them), ten repetitions after two warm-up calls, median and
range.  The two sides of every comparison alternate inside one process.

  marginal    product_batch next to marginal_batch (the read-out whose route decision it borrows; its code is the parent
              commit's, untouched) on the same state and row count: n = 24 tensors saturated at bond 64, c64 and f64, 64 and 4096
              rows.  The marginal's bits are uniform in {0, 1, 2}, the weights complex Gaussian.
  routes      product_batch forced onto each route (QIL_PRODUCT_ROUTE, read per call) at (rows 64, bond 64), (64, 128),
              (1024, 16 and 32), (4096, 16 / 24 / 32 / 48 / 64), c64 and f64, n = 24 tensors; `default` names what the unforced call takes.
  zoom        a 128 x 128 zt_eval window on the n = 20 signal of examples/zoom_scan.py (the tutorial's fine window), next to what
              the tutorial does for it: build_zt_mpo(wr = 0.5) + apply + coefficient_grid on the same window rounded to the grid;
              both with the pole error they reach.  The encodes (signal_mps / signal_ztmps) are outside both timings.

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
sys.path.insert(0, os.path.join(ROOT, "examples"))
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
        # a GPU agent without a marketing name still has its target as Name; never fall back to the CPU agent's name
        targets = [l.split(":", 1)[1].strip() for l in out.splitlines() if l.strip().startswith("Name:") and "gfx" in l]
        return next((v for v in names if "Instinct" in v or "MI3" in v), targets[0] if targets else "unknown")
    except (OSError, subprocess.SubprocessError):
        return "unknown"


def forced(route, fn):
    def run():
        if route is None:
            os.environ.pop("QIL_PRODUCT_ROUTE", None)
        else:
            os.environ["QIL_PRODUCT_ROUTE"] = route
        try:
            return fn()
        finally:
            os.environ.pop("QIL_PRODUCT_ROUTE", None)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="marginal,routes,zoom")
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

    rng = np.random.default_rng(2024)
    n = 24

    def state(bond, dt):
        return qil.SignalMPS.alloc(saturated_profile(n, bond), dtype=dt, amplitude=1.5).fill_random(5)

    def weights(nb):
        return rng.standard_normal((nb, n, 2)) + 1j * rng.standard_normal((nb, n, 2))

    if "marginal" in args.only:
        for dt in (np.complex128, np.float64):
            psi = state(64, dt)
            for nb in (64, 4096):
                w, bits = weights(nb), rng.integers(0, 3, size=(nb, n)).astype(np.uint8)
                route, _ = qil.readout_route("marginal", nb, [1] + psi.bond_dims + [1], dtype=dt)
                ts = timed_pair(ctx, {"product_batch": lambda: qil.product_batch(psi, w),
                                      "marginal_batch": lambda: qil.marginal_batch(psi, bits)}, args.reps)
                ratio = float(np.median(ts["product_batch"]) / np.median(ts["marginal_batch"]))
                for name, t in ts.items():
                    emit(dict(case=f"marginal_n24_bond64_{np.dtype(dt).name}_nb{nb}", verb=name, marginal_route=route,
                              product_over_marginal=ratio, **stats(t)))
    if "routes" in args.only:
        for nb, bond in ((64, 64), (64, 128), (1024, 16), (1024, 32), (4096, 16), (4096, 24), (4096, 32), (4096, 48), (4096, 64)):
            for dt in (np.complex128, np.float64):
                psi, w = state(bond, dt), weights(nb)
                route, _ = qil.readout_route("marginal", nb, [1] + psi.bond_dims + [1], dtype=dt)
                if max(psi.bond_dims) < 128 and nb * max(psi.bond_dims) ** 2 < qil.ops.PRODUCT_MANY_ROWS_CHAIN_WORK:
                    route = "CHAIN"                           # the verb's own constant (qil_product.hip)
                run = lambda: qil.product_batch(psi, w)
                a, b = forced("chain", run)(), forced("gemm", run)()
                dev = float(np.abs(a - b).max() / np.abs(b).max())
                ts = timed_pair(ctx, {"chain": forced("chain", run), "gemm": forced("gemm", run)}, args.reps)
                for name, t in ts.items():
                    emit(dict(case=f"routes_n24_bond{bond}_{np.dtype(dt).name}_nb{nb}", route=name,
                              default="chain" if route == "CHAIN" else "gemm", chain_vs_gemm_rel=dev, **stats(t)))
    if "zoom" in args.only:
        import zoom_scan as Z
        x = Z.tutorial_signal()
        kw = dict(method="rsvd", k=50, p=5, q=2, cutoff=1e-12, maxdim=128)
        psi, psi_z = qil.signal_mps(x, **kw), qil.signal_ztmps(x, **kw)
        k, l = Z.fine_window()
        N = 2 ** Z.N_BITS
        ks, ls = np.clip(np.rint(k).astype(np.int64), 0, N - 1), np.mod(np.rint(l).astype(np.int64), N)
        found = {}

        def by_product():
            found["zt_eval"] = Z.scan(psi, k, l)[3]

        def by_operator():
            phi = qil.build_zt_mpo(psi_z, Z.WR, cutoff=1e-12, maxdim=128) * psi_z
            chi = qil.coefficient_grid(phi, ks, ls)
            i, j = np.unravel_index(np.argmax(np.abs(chi)), chi.shape)
            found["operator"] = float(min(abs(Z.z_of(float(ks[i]), float(ls[j])) - p) for p in Z.POLES))

        ts = timed_pair(ctx, {"zt_eval": by_product, "operator": by_operator}, args.reps)
        for name, t in ts.items():
            emit(dict(case="zoom_128x128_n20_fine_window", route=name, pole_error=float(found[name]), **stats(t)))
        for label, (kk, ll) in (("superfine", Z.superfine_window()), ("10x_finer", Z.superfine_window(half=2.4))):
            emit(dict(case=f"zoom_49x49_n20_{label}", route="zt_eval", pole_error=float(Z.scan(psi, kk, ll)[3])))


if __name__ == "__main__":
    main()
