"""Times of qil.coefficient_at, of the element-wise maps and of qil.deconvolve on one GPU (MEASUREMENTS section 29): wall time
around the whole call with both streams synchronised, the median of up to ten repetitions after a warm-up call (fewer where one
call takes more than a tenth of the part's budget; the loop part times one call after one warm-up call).

  routes    coefficient_at forced onto each route (QIL_COEFFICIENT_AT_ROUTE, read per call): counts 64, 4096, 262144, bonds 4,
            16, 64, 128, 256 on 24 and 40 tensors, f64 and c64
  routes2   the same around the crossover: bonds 8, 16, 32, counts 64, 512, 4096, 32768, 262144
  loop      |psi| of a K-mode sum of exponentials (source bond K = 8, 32) at n = 24 and 40, maxdim 32 and 64, tol 1e-8,
            max_sweeps 3, the same seeds: cross_map on coefficient_at, the same callable on coefficient_batch with host copies,
            and map_states; total time and time per block (request)
  deconv    deconvolve of a blurred three-mode signal against torch.fft on the dense vector (n = 20, 24; the FFT alone on a
            random vector at n = 28, 30), and the MPS form at n = 40

    python tools/_index_time.py <part> [out-file]

One line per measurement on stdout (and in the out-file)."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import qilaplace_jl_amd as qil  # noqa: E402

part = sys.argv[1]
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


def sync():
    torch.cuda.synchronize(); qil.default_context().synchronize()

def timed(fn, budget=1.0):
    fn(); sync()
    t0 = time.perf_counter(); fn(); sync(); first = time.perf_counter() - t0
    reps = int(max(1, min(10, budget / max(first, 1e-6))))
    ts = [first]
    for _ in range(reps - 1):
        t0 = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3

def random_state(n, chi, dt, seed=1):
    rng = np.random.default_rng(seed)
    dims = [1] + [min(chi, 2 ** min(i, n - i)) for i in range(1, n)] + [1]
    data = []
    for i in range(n):
        shp = (dims[i], 2, dims[i + 1])
        t = rng.standard_normal(shp) / np.sqrt(2.0 * dims[i])
        if dt == np.complex128:
            t = t + 1j * rng.standard_normal(shp) / np.sqrt(2.0 * dims[i])
        data.append(np.asfortranarray(t.astype(dt)))
    return qil.SignalMPS(data)

if part == "routes":
    say("dtype n bond count wave_ms bits_ms")
    for dt, dn in ((np.float64, "f64"), (np.complex128, "c64")):
        for n in (24, 40):
            for chi in (4, 16, 64, 128, 256):
                psi = random_state(n, chi, dt)
                for count in (64, 4096, 262144):
                    idx = torch.from_numpy(np.random.default_rng(3).integers(0, 2 ** n, size=count, dtype=np.int64)).cuda()
                    res = {}
                    for route in ("wave", "bits"):
                        os.environ["QIL_COEFFICIENT_AT_ROUTE"] = route
                        res[route] = timed(lambda: qil.coefficient_at(psi, idx), budget=0.5)
                    say(dn, n, chi, count, f"{res['wave']:.3f}", f"{res['bits']:.3f}")
                del psi
    os.environ.pop("QIL_COEFFICIENT_AT_ROUTE", None)

if part == "routes2":
    say("dtype n bond count wave_ms bits_ms")
    for dt, dn in ((np.float64, "f64"), (np.complex128, "c64")):
        for n in (24, 40):
            for chi in (8, 16, 32):
                psi = random_state(n, chi, dt)
                for count in (64, 512, 4096, 32768, 262144):
                    idx = torch.from_numpy(np.random.default_rng(3).integers(0, 2 ** n, size=count, dtype=np.int64)).cuda()
                    res = {}
                    for route in ("wave", "bits"):
                        os.environ["QIL_COEFFICIENT_AT_ROUTE"] = route
                        res[route] = timed(lambda: qil.coefficient_at(psi, idx), budget=0.5)
                    say(dn, n, chi, count, f"{res['wave']:.3f}", f"{res['bits']:.3f}")
                del psi
    os.environ.pop("QIL_COEFFICIENT_AT_ROUTE", None)

if part == "loop":
    say("n srcbond maxdim variant total_ms blocks ms_per_block maxbond converged")
    for n in (24, 40):
        for K in (8, 32):
            rng = np.random.default_rng(K)
            zs = np.exp(1j * rng.uniform(0, 2 * np.pi, K) - rng.uniform(0, 2.0, K) / 2 ** n)
            amps = rng.standard_normal(K) + 1j * rng.standard_normal(K)
            psi = qil.exponential_sum(amps, zs, n, maxdim=None, tol=None)
            for maxdim in (32, 64):
                blocks = {"n": 0}
                def dev(a):
                    blocks["n"] += 1
                    return torch.abs(a)
                def host_f(idx):
                    blocks["n"] += 1
                    j = idx.cpu().numpy()
                    bits = ((j[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
                    v = qil.coefficient_batch(psi, bits)
                    return torch.from_numpy(np.abs(v)).cuda()
                seeds = importlib.import_module("qilaplace_jl_amd.ops")._map_seeds((psi,), n, None, 8, 1234)[0]
                kw = dict(maxdim=maxdim, tol=1e-8, max_sweeps=3)
                variants = {
                    "cross_map+coefficient_at": lambda: qil.cross_map(dev, psi, seeds=seeds, return_info=True, **kw),
                    "callable+coefficient_batch(host)": lambda: qil.signal_mps_cross(host_f, n=n, seeds=seeds, return_info=True, **kw),
                    "map_states": lambda: qil.map_states("abs", psi, seeds=seeds, return_info=True, **kw),
                }
                nblocks = None
                for name, fn in variants.items():
                    fn(); sync()
                    blocks["n"] = 0
                    t0 = time.perf_counter(); res, info = fn(); sync(); ms = (time.perf_counter() - t0) * 1e3
                    if name != "map_states":
                        nblocks = blocks["n"] - 1          # the dtype probe of the seeds is one extra evaluation
                    say(n, K, maxdim, name, f"{ms:.1f}", nblocks, f"{ms / nblocks:.3f}", max(res.bond_dims), info["converged"])

if part == "deconv":
    say("n variant ms err_rel bonds")
    def fir_state(n):
        terms = []
        for k in (0, 1, 2):
            data = [np.zeros((1, 2, 1)) for _ in range(n)]
            for i in range(n):
                data[i][0, (k >> (n - 1 - i)) & 1, 0] = 1.0
            terms.append(qil.SignalMPS(data))
        return qil.linear_combination_compress(terms, [1.0, 0.5, 0.25])
    modes = [(1.0, 0.31), (0.5 - 0.2j, -1.1), (0.25j, 2.3)]
    for n in (20, 24, 40):
        zs = [np.exp(1j * w - 0.3 / 2 ** n) for _, w in modes]
        px = qil.exponential_sum([a for a, _ in modes], zs, n)
        ph = fir_state(n)
        F = qil.build_qft_mpo(px)
        py = qil.convolve(px, ph, F=F)
        f = lambda: qil.deconvolve(py, ph, F=F, map_tol=1e-10)
        ms = timed(f, budget=2.0)
        back = f()
        idx = np.random.default_rng(5).integers(0, 2 ** n, size=2000, dtype=np.int64)
        bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
        got, want = qil.coefficient_batch(back, bits), qil.coefficient_batch(px, bits)
        say(n, "deconvolve(MPS)", f"{ms:.2f}", f"{np.abs(got - want).max() / np.abs(want).max():.2e}",
            f"y {max(py.bond_dims)} F {max(F.bond_dims)} out {max(back.bond_dims)}")
        if n <= 24:
            yd = torch.from_numpy(qil.mps_to_vector(py)).cuda()
            hd = torch.from_numpy(qil.mps_to_vector(ph).astype(np.complex128)).cuda()
            g = lambda: torch.fft.ifft(torch.fft.fft(yd) / torch.fft.fft(hd))
            ms = timed(g, budget=2.0)
            xd = g().cpu().numpy()
            xw = qil.mps_to_vector(px)
            say(n, "torch.fft(dense)", f"{ms:.3f}", f"{np.abs(xd - xw).max() / np.abs(xw).max():.2e}", "-")
            del yd, hd
    for n in (28, 30):
        yd = torch.randn(2 ** n, dtype=torch.complex128, device="cuda")
        hd = torch.zeros(2 ** n, dtype=torch.complex128, device="cuda"); hd[:3] = torch.tensor([1.0, 0.5, 0.25])
        g = lambda: torch.fft.ifft(torch.fft.fft(yd) / torch.fft.fft(hd))
        say(n, "torch.fft(dense, random y)", f"{timed(g, budget=2.0):.2f}", "-", "-")
        del yd, hd
        torch.cuda.empty_cache()
say("done")
