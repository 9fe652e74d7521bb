"""Times of the element-wise product (qil.hadamard) on one GPU: call time by HIP events (one grouped kernel launch behind a
descriptor upload), five repetitions after two warm-up calls, with the bytes stored and the fraction of the 8 TB/s HBM spec they
make, on an n = 24 paired chain (48 tensors), chi_phi x chi_psi = 64 x 64 and 64 x 128, c64 and f64 -- next to
apply(diagonal_mpo(phi), psi) (site_apply_grouped on the same shapes) in the same run.

--baseline: the route the kernel replaces, apply(PairedSiteMPO(host-built diagonal tensors), psi), and nothing newer than
`apply` -- so that this file also runs from a checkout of the commit before qil_hadamard existed.
--convolve: end-to-end qil.convolve at n = 20 and n = 24 with maxdim = 64 (encode excluded, the QFT MPO built once), next to
np.fft.ifft(fft(x) fft(h)) on the host, for information.
One JSON line per measurement on stdout (and appended to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qilaplace_jl_amd as qil  # noqa: E402
from helpers import saturated_profile  # noqa: E402

HBM_SPEC = 8.0e12
SHAPES = [(64, 64), (64, 128)]


def timed(ctx, fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return ts


def stored_bytes(pb, ab, itemsize):
    d = [1] + [p * a for p, a in zip(pb, ab)] + [1]
    return sum(d[i] * 2 * d[i + 1] for i in range(len(d) - 1)) * itemsize


def host_diagonal(phi):
    out = []
    for i, A in enumerate(phi.to_host()):
        W = np.zeros((A.shape[0], 2, 2, A.shape[2]), dtype=A.dtype)
        W[:, 0, 0, :], W[:, 1, 1, :] = A[:, 0, :], A[:, 1, :]
        out.append(W * phi.amplitude if i == 0 else W)
    return qil.PairedSiteMPO(out)


def products(emit, reps, baseline):
    ctx = qil.default_context()
    for dt in (np.complex128, np.float64):
        for cp, ca in SHAPES:
            pb, ab = saturated_profile(48, cp), saturated_profile(48, ca)
            phi = qil.ZTMPS.alloc(pb, dtype=dt).fill_random(11)
            psi = qil.ZTMPS.alloc(ab, dtype=dt).fill_random(12)
            nbytes = stored_bytes(pb, ab, np.dtype(dt).itemsize)
            routes = {}
            if baseline:
                D = host_diagonal(phi)
                routes["apply_host_diagonal"] = lambda: qil.apply(D, psi)
            else:
                D = qil.diagonal_mpo(phi)
                routes["hadamard"] = lambda: qil.hadamard(phi, psi)
                routes["apply_diagonal_mpo"] = lambda: qil.apply(D, psi)
            for name, fn in routes.items():
                ts = timed(ctx, fn, reps)
                med = float(np.median(ts))
                emit(what=name, n_tensors=48, chi_phi=cp, chi_psi=ca, dtype=np.dtype(dt).name, bytes_stored=nbytes,
                     ms=[round(t, 4) for t in ts], ms_median=med, ms_min=min(ts), ms_max=max(ts),
                     tb_per_s=nbytes / (med * 1e-3) / 1e12, fraction_of_8tbs=nbytes / (med * 1e-3) / HBM_SPEC)
            del D, phi, psi, routes
            ctx.trim()


def convolutions(emit, reps):
    ctx = qil.default_context()
    for n in (20, 24):
        N = 2 ** n
        t = np.arange(N) / N
        x = np.cos(2 * np.pi * 5 * t) * np.exp(-3 * t) + 0.3 * np.sin(2 * np.pi * 17 * t)
        h = np.exp(-40 * t) + 0.5 * np.exp(-8 * t) * np.cos(2 * np.pi * 3 * t)
        px, ph = qil.signal_mps(x), qil.signal_mps(h)
        F = qil.build_qft_mpo(px)
        ts = timed(ctx, lambda: qil.convolve(px, ph, F=F, maxdim=64), reps)
        y = qil.convolve(px, ph, F=F, maxdim=64)
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ref = np.fft.ifft(np.fft.fft(x) * np.fft.fft(h))
            host.append((time.perf_counter() - t0) * 1e3)
        idx = np.random.default_rng(n).integers(0, N, size=4096)
        bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
        dev = float(np.abs(qil.coefficient_batch(y, bits) - ref[idx]).max() / np.abs(ref).max())
        emit(what="convolve_maxdim64", n=n, ms_median=float(np.median(ts)), ms_min=min(ts), ms_max=max(ts),
             numpy_fft_host_ms_median=float(np.median(host)), max_bond=int(max(y.bond_dims)), deviation_of_max_on_4096=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--convolve", action="store_true")
    args = ap.parse_args()
    assert qil.device_count() >= 1, "needs a GPU"

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    if args.convolve:
        convolutions(emit, args.reps)
    else:
        products(emit, args.reps, args.baseline)


if __name__ == "__main__":
    main()
