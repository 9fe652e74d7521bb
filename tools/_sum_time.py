#!/usr/bin/env python3
"""Timings of the linear combinations for MEASUREMENTS section 10, one JSON line per figure on stdout.

    python tools/_sum_time.py store      store rate of linear_combination against hbm_store_peak and hadamard (>= 8 GB outputs)
    python tools/_sum_time.py fused8     8 x chi 128: fused route, host direct sum + upload + compress, device exact route
    python tools/_sum_time.py fused64    64 x chi 64: fused route
    python tools/_sum_time.py bond2      64 x chi 2: fused route (the grouped small-GEMM regime; run it under a kernel trace,
                                         with and without QIL_SUM_NO_GROUPED=1, for the launch counts)

The host route of `fused8` (download, numpy direct sum, upload, compress) needs nothing of this feature: it is what a caller
could do before it, and the script times it wherever `linear_combination` is missing, too."""
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

ctx = qil.default_context()


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps=3):
    """best of `reps` calls by HIP events, the result released between calls (the pool then serves the next one)"""
    best = None
    for _ in range(reps):
        ctx.synchronize()
        ctx.timer_start()
        r = fn()
        ms = ctx.timer_stop()
        best = ms if best is None else min(best, ms)
        del r
    return best


def nbytes(psi):
    d = [1] + psi.bond_dims + [1]
    return sum(d[i] * 2 * d[i + 1] for i in range(len(d) - 1)) * (16 if psi.dtype == np.complex128 else 8)


def store_rates():
    peak, writer = ctx.hbm_store_peak()
    emit(kind="store_peak", gbs=peak, writer=writer)
    for dt, n in ((np.complex128, 26), (np.float64, 27)):
        terms = [qil.SignalMPS.alloc(saturated_profile(n, 512), dtype=dt).fill_random(j) for j in range(8)]
        r = qil.linear_combination(terms)
        gb = nbytes(r) / 1e9
        del r
        ms = timed(lambda: qil.linear_combination(terms))
        emit(kind="sum", dtype=str(np.dtype(dt)), n=n, gb=gb, ms=ms, gbs=gb / ms * 1e3, frac_peak=gb / ms * 1e3 / peak)
        del terms
        a = qil.SignalMPS.alloc(saturated_profile(n, 64), dtype=dt).fill_random(1)
        b = qil.SignalMPS.alloc(saturated_profile(n, 64), dtype=dt).fill_random(2)
        r = qil.hadamard(a, b)
        gb = nbytes(r) / 1e9
        del r
        ms = timed(lambda: qil.hadamard(a, b))
        emit(kind="hadamard", dtype=str(np.dtype(dt)), n=n, gb=gb, ms=ms, gbs=gb / ms * 1e3, frac_peak=gb / ms * 1e3 / peak)
        del a, b
        ctx.trim()


def host_direct_sum(terms, c):
    hosts = [t.to_host() for t in terms]
    n = len(hosts[0])
    data = [np.concatenate([cj * t.amplitude * h[0] for cj, t, h in zip(c, terms, hosts)], axis=2)]
    for i in range(1, n - 1):
        A = np.zeros((sum(h[i].shape[0] for h in hosts), 2, sum(h[i].shape[2] for h in hosts)), np.complex128)
        lo = ro = 0
        for h in hosts:
            A[lo:lo + h[i].shape[0], :, ro:ro + h[i].shape[2]] = h[i]
            lo, ro = lo + h[i].shape[0], ro + h[i].shape[2]
        data.append(A)
    data.append(np.concatenate([h[n - 1] for h in hosts], axis=0))
    return data


def fused(nb, chi, n, host_route):
    terms = [qil.SignalMPS.alloc(saturated_profile(n, chi), dtype=np.complex128).fill_random(100 + j) for j in range(nb)]
    c = np.random.default_rng(1).standard_normal(nb) + 0j
    if hasattr(qil, "linear_combination_compress"):
        t0 = time.perf_counter()
        r = qil.linear_combination_compress(terms, c, maxdim=64, tol=1e-8)
        ctx.synchronize()
        t1 = time.perf_counter()
        del r
        r = qil.linear_combination_compress(terms, c, maxdim=64, tol=1e-8)
        ctx.synchronize()
        t2 = time.perf_counter()
        emit(kind="fused", nb=nb, chi=chi, n=n, first_s=t1 - t0, second_s=t2 - t1, bonds=max(r.bond_dims))
        del r
    if not host_route:
        return
    t0 = time.perf_counter()
    data = host_direct_sum(terms, c)
    t1 = time.perf_counter()
    s = qil.SignalMPS(data)
    ctx.synchronize()
    t2 = time.perf_counter()
    qil.compress(s, maxdim=64, tol=1e-8)
    ctx.synchronize()
    t3 = time.perf_counter()
    emit(kind="host_route", nb=nb, chi=chi, n=n, build_s=t1 - t0, upload_s=t2 - t1, compress_s=t3 - t2, total_s=t3 - t0,
         bonds=max(s.bond_dims))
    if hasattr(qil, "linear_combination"):
        t0 = time.perf_counter()
        s2 = qil.compress(qil.linear_combination(terms, c), maxdim=64, tol=1e-8)
        ctx.synchronize()
        emit(kind="device_exact_route", nb=nb, chi=chi, n=n, total_s=time.perf_counter() - t0, bonds=max(s2.bond_dims))


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "store":
        store_rates()
    elif what == "fused8":
        fused(8, 128, 24, True)
    elif what == "fused64":
        fused(64, 64, 24, False)
    elif what == "bond2":
        fused(64, 2, 24, False)
    else:
        raise SystemExit(__doc__)
