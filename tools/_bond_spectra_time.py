"""Times of the Schmidt spectra (qil.bond_spectra) on one GPU at the default route (every bond up to the LDS cap in ONE launch of
bond_svals_batched) and at QIL_SPECTRA_ROUTE=svd (the same two sweeps, every bond through the one-matrix SVD): call time by HIP
events around the whole call (the clone, both gauge sweeps, the launches, the read-back and the host work between them), --reps
repetitions per block after two warm-up calls, the two routes in alternating blocks (default, svd, default, svd) so that a
drift of the box shows in both; median and range over a route's blocks.  Each record also carries the largest absolute
difference between the two routes' values.

  (a) zT product  a damped two-tone signal of 2^24 samples as a ZTMPS, transformed by build_zt_mpo(psi, 2 pi) and truncated by
                  apply_compress(maxdim = 64): 48 tensors, 47 bonds, chi <= 64
  (b) chi 64      24 tensors, bonds min(2^i, 2^(24 - i), 64), fill_random, f64 and c64
  (c) chi 256     24 tensors, bonds min(2^i, 2^(24 - i), 256), fill_random, f64: the large bonds are above the cap, where both
                  routes take the same SVD
  (d) chi 138     24 tensors, bonds min(2^i, 2^(24 - i), 138), fill_random, f64: the f64 cap, 138 x 138 carries of 153 456 B of LDS
                  on the wave-per-pair sweep

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
import qilaplace_jl_amd as qil  # noqa: E402
from helpers import saturated_profile  # noqa: E402

ROUTE = "QIL_SPECTRA_ROUTE"


def gpu_name():
    """The marketing name (else the agent name) of the first GPU agent rocminfo lists."""
    try:
        out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        return "unknown"
    name = marketing = ""
    for line in out.splitlines():
        key, _, val = line.partition(":")
        key, val = key.strip(), val.strip()
        if key == "Name":
            name, marketing = val, ""
        elif key == "Marketing Name":
            marketing = val
        elif key == "Device Type" and val == "GPU":
            return marketing or name or "unknown"
    return "unknown"


def set_route(route):
    if route is None:
        os.environ.pop(ROUTE, None)
    else:
        os.environ[ROUTE] = route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="a,b,c,d")
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

    def block(psi):
        ts = []
        for _ in range(args.reps):
            ctx.timer_start()
            qil.bond_spectra(psi)
            ts.append(ctx.timer_stop())
        return ts

    def compare(name, psi):
        bonds = psi.bond_dims
        case = dict(name=name, tensors=len(bonds) + 1, bonds=len(bonds), chi=max(bonds), dtype=np.dtype(psi.dtype).name)
        times = {"default": [], "svd": []}
        values = {}
        try:
            for route in (None, "svd"):
                set_route(route)
                for _ in range(2):
                    values[route or "default"] = qil.bond_spectra(psi)
            for _ in range(2):
                for route in (None, "svd"):
                    set_route(route)
                    times[route or "default"] += block(psi)
        finally:
            set_route(None)
        dev = max(float(np.abs(a - b).max()) for a, b in zip(values["default"], values["svd"]))
        for route, ts in times.items():
            emit(dict(case=case, route=route, ms_median=float(np.median(ts)), ms_min=float(min(ts)), ms_max=float(max(ts)),
                      reps=len(ts), routes_max_abs_dev=dev))

    wanted = args.cases.split(",")
    if "a" in wanted:
        n = 24
        N = 2 ** n
        j = np.arange(N, dtype=np.float64)
        x = np.sin(2 * np.pi * 5.0 * j / N) * np.exp(-3.0 * j / N) + 0.5 * np.cos(2 * np.pi * 11.0 * j / N)
        psi = qil.signal_ztmps(x, cutoff=1e-12)
        del x, j
        out = qil.apply_compress(qil.build_zt_mpo(psi, 2 * np.pi), psi, maxdim=64, tol=1e-8)
        compare("a_zt_product_n24", out)
    if "b" in wanted:
        for dtype, seed in ((np.float64, 5), (np.complex128, 6)):
            compare("b_chi64", qil.SignalMPS.alloc(saturated_profile(24, 64), dtype=dtype).fill_random(seed))
    if "c" in wanted:
        compare("c_chi256", qil.SignalMPS.alloc(saturated_profile(24, 256), dtype=np.float64).fill_random(7))
    if "d" in wanted:
        compare("d_chi138", qil.SignalMPS.alloc(saturated_profile(24, 138), dtype=np.float64).fill_random(8))


if __name__ == "__main__":
    main()
