"""Bit-for-bit record of the overlap, read-out, weight, sampling, top-k, restriction and sum verbs on a fixed, seeded list of small cases,
for comparing two builds of libqilhip.so (a refactor against its parent).  Public Python API only, so it runs unchanged against
either library through QILHIP_LIB:

    QILHIP_LIB=/path/to/parent/libqilhip.so python tools/_verb_bits.py --out parent.npz
    python tools/_verb_bits.py --out new.npz
    python tools/_verb_bits.py --compare parent.npz new.npz         # numpy.array_equal on every entry; exit status 1 on a difference

Cases: chains of 6 to 8 tensors, bonds at most 8, MPO bonds at most 4, in f64, c64 and each mixed pairing: inner on both routes
(QIL_INNER_ROUTE), norm, inner(phi, W, psi), apply_norm, apply_coefficient_batch, weight_batch on both routes (QIL_WEIGHT_NO_LDS,
read once per process: that stage is a child process of its own), apply_weight_batch with QIL_APPLY_WEIGHT_RENV_BYTES unset and 0
(rows with no traced site, only traced sites, a fixed last site, and tails of different lengths, which leave the slot list from
the inside), sample on both routes (QIL_SAMPLE_ROUTE), restrict with a summed and a fixed site, linear_combination_compress with
three terms (the grouped small GEMM); top_k with k = 5 at a beam that drops prefixes (6) and at the full beam 2^n; apply_sample (70
rows, seeded and with given uniforms) and apply_top_k (the same two beams) on both QIL_APPLY_SAMPLE_ROUTE settings, each a child
process of its own.  The top-k verbs record (rows, values, bound, certified).  Beyond those: top_k and apply_top_k of 12 tensors at
beam 1500, a frontier of 3000 candidates (more than one selection tile of 1024), for the lazy verb at chi D = 1024 in c64, where
the row step's chunk (1020 rows) is below the frontier; 20000 rows of apply_weight_batch whose strided batches exceed 65535 entries
(the piece boundary inside qil_dev_gemm_batched), and apply_coefficient_batch at chi D = 1024 (its GEMM form).  The read-out verbs on
every route of theirs: readout_cases below.

The process that is started never opens the GPU: every stage is a fresh child."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, Z = np.float64, np.complex128
DT_PAIRS = [(F, F), (F, Z), (Z, F), (Z, Z)]
DT_IDS = ["f64-f64", "f64-c64", "c64-f64", "c64-c64"]
CHI = [[2, 3, 5, 7, 5, 3, 2], [2, 4, 8, 8, 8, 4, 2]]            # interior bonds of psi (cut to n - 1): odd, saturated
PHI = [2, 4, 6, 8, 6, 4, 2]
DW = [3, 4, 2, 4, 3, 4, 2]
STAGES = {"default": {}, "weight_gemm": {"QIL_WEIGHT_NO_LDS": "1"}, "apply_fused": {"QIL_APPLY_SAMPLE_ROUTE": "fused"},
          "apply_gemm": {"QIL_APPLY_SAMPLE_ROUTE": "gemm"}}
WIDE_N, WIDE_BEAM = 12, 1500                                       # frontiers 1, 2, .., 1024, 1500, 1500: 3000 candidates at the cuts


def _mps(bonds, rng, dt):
    d = [1] + list(bonds) + [1]
    out = []
    for i in range(len(d) - 1):
        shp = (d[i], 2, d[i + 1])
        a = rng.standard_normal(shp) + (1j * rng.standard_normal(shp) if dt == Z else 0.0)
        out.append((a / np.sqrt(2.0 * d[i])).astype(dt))
    return out


def _mpo(bonds, rng, dt):
    d = [1] + list(bonds) + [1]
    out = []
    for i in range(len(d) - 1):
        shp = (d[i], 2, 2, d[i + 1])
        w = rng.standard_normal(shp) + (1j * rng.standard_normal(shp) if dt == Z else 0.0)
        out.append((w / np.sqrt(2.0 * d[i])).astype(dt))
    return out


def _weight_rows(n, rng):
    rows = [rng.integers(0, 2, n), np.full(n, 2)]                                   # no traced site; only traced sites
    r = np.full(n, 2); r[-1] = 1; rows.append(r)                                    # a fixed last site
    for tail in range(1, n):                                                        # tails of every length: the rows finish at
        r = rng.integers(0, 3, n); r[0] = 2; r[n - tail - 1] = 0; r[n - tail:] = 2  # different bonds, leaving from the inside
        rows.append(r)
    for lead in range(1, n):                                                        # leads of every length
        r = rng.integers(0, 3, n); r[:lead] = rng.integers(0, 2, lead); r[lead] = 2
        rows.append(r)
    rows += [rng.integers(0, 3, n) for _ in range(12)]
    return np.array(rows, dtype=np.uint8)


def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def boundary_case(qil):
    """f64, 6 tensors, psi bonds (1, 2, 4, 4, 4, 2, 1), W bonds (1, 2, 2, 2, 2, 2, 1), 20000 rows: first site traced, last fixed, the
    rest from {0, 1, 2}.  All rows are in the middle at once (2304 B of temporaries per row: one chunk), so the interior sites run
    strided batches of 80000 and 160000 entries."""
    rng = np.random.default_rng(1717)
    a, w = _mps([2, 4, 4, 4, 2], rng, F), _mpo([2, 2, 2, 2, 2], rng, F)
    rows = rng.integers(0, 3, size=(20000, 6)).astype(np.uint8)
    rows[:, 0] = 2
    rows[:, -1] = rng.integers(0, 2, size=20000)
    return qil.SingleSiteMPO(w), qil.SignalMPS(a, amplitude=1.7), rows


def wide_lazy_case(qil):
    """c64, 12 tensors, chi D = 1024 in the middle: (2 maxM + maxX) e + 16 ceil(maxM / 64) = 65792 B per row, 1020 rows per chunk"""
    rng = np.random.default_rng(2323)
    a = _mps([2, 4, 8, 16, 32, 32, 32, 16, 8, 4, 2], rng, Z)
    w = _mpo([4, 16, 32, 32, 32, 32, 32, 32, 32, 16, 4], rng, Z)
    return qil.SingleSiteMPO(w), qil.SignalMPS(a, amplitude=1.7)


def readout_cases(qil, put):
    """Every route of the read-out verbs (the route names are asserted through qil.readout_route, which needs no device):
    coefficient_batch / marginal_batch on CHAIN (bonds <= 8), GEMM_SELECT and GEMM_SORTED (1 x 128 x 1 interior profile of four tensors,
    12 queries of which the first site's are all 0: a slice of no rows, and slices of <= 48 rows: the skinny GEMM; 200 queries: the
    wide GEMM), the many-rows arm (1024 queries at bond 16); apply_coefficient_sweep of 3 operators (one after the other) and of 5
    distinct ones (the lock-step batch), with product bonds 8 (CHAIN) and 128 (one sorted plan for all); a two-pass
    apply_coefficient_batch (32808 queries at chi D = 1024 in f64: 32768 per pass, 1 GiB of temporaries); mps_block with fixed,
    summed and free sites, the last free site last and not last, both bit orders; mps_to_vector; coefficient_grid through the dense
    block and through batches."""
    for k, dt in enumerate((F, Z)):
        tag = DT_IDS[3 * k]
        rng = np.random.default_rng(2500 + k)
        for name, bonds, nb, routes in (("chain", [2, 4, 8, 8, 4, 2], 40, ("CHAIN", "CHAIN")),
                                        ("wide", [2, 128, 2], 12, ("GEMM_SORTED", "GEMM_SELECT")),
                                        ("wide", [2, 128, 2], 200, ("GEMM_SORTED", "GEMM_SELECT")),
                                        ("many_rows", [2, 4, 16, 16, 4, 2], 1024, ("GEMM_SORTED", "GEMM_SELECT"))):
            n = len(bonds) + 1
            dims = [1] + bonds + [1]
            psi = qil.SignalMPS(_mps(bonds, rng, dt), amplitude=1.7)
            bits = rng.integers(0, 2, size=(nb, n)).astype(np.uint8)
            if name == "wide":
                bits[:, 0] = 0                                                      # no query takes slice 1 of the first site
            assert (qil.readout_route("plain", nb, dims)[0], qil.readout_route("marginal", nb, dims)[0]) == routes, (name, nb)
            put(f"coefficient_batch[{name}, nb={nb}]/{tag}", qil.coefficient_batch(psi, bits))
            summed = bits.copy()
            summed[rng.random(bits.shape) < 0.3] = 2
            put(f"marginal_batch[{name}, nb={nb}]/{tag}", qil.marginal_batch(psi, summed))
        for name, pb, wb in (("chain", [2, 4, 4, 4, 2], [2, 2, 2, 2, 2]), ("sorted", [2, 16, 16, 16, 2], [4, 8, 8, 8, 4])):
            n = len(pb) + 1
            psi = qil.SignalMPS(_mps(pb, rng, dt), amplitude=1.7)
            ops = [qil.SingleSiteMPO(_mpo(wb, rng, (F, Z)[(j + k) % 2])) for j in range(5)]
            bits = rng.integers(0, 2, size=(24, n)).astype(np.uint8)
            want = "CHAIN" if name == "chain" else "GEMM_SORTED"
            assert qil.readout_route("sweep", 24, [1] + pb + [1], [1] + wb + [1])[0] == want
            for nw in (3, 5):
                put(f"apply_coefficient_sweep[{name}, nw={nw}]/{tag}", qil.apply_coefficient_sweep(ops[:nw], psi, bits))
        n = 9
        data = _mps(CHI[1] + [2], rng, dt)
        psi = qil.SignalMPS(data, amplitude=1.7)
        for label, spec in (("free_last", [3, 0, 2, 3, 3, 1, 2, 3, 3]), ("right_fold", [1, 3, 2, 3, 0, 3, 3, 2, 1]),
                            ("none_free", [0, 1, 2, 2, 1, 0, 2, 1, 0])):
            for rev in (False, True):
                put(f"mps_block[{label}, reverse={rev}]/{tag}", qil.mps_block(psi, np.array(spec, dtype=np.uint8), reverse=rev))
        for rev in (False, True):
            put(f"mps_to_vector[reverse={rev}]/{tag}", qil.mps_to_vector(psi, reverse=rev))
        zt = qil.ZTMPS(_mps(CHI[1][:7], rng, dt), amplitude=1.7)                      # 8 tensors: 4 bits per register
        put(f"coefficient_grid[block]/{tag}", qil.coefficient_grid(zt, np.arange(8), np.arange(16)))
        perm = rng.permutation(16)
        put(f"coefficient_grid[batches]/{tag}", qil.coefficient_grid(zt, perm[:11], perm))
    rng = np.random.default_rng(2600)
    nb, dims = 32768 + 40, [1, 32, 32, 1]
    assert qil.readout_route("lazy", nb, dims, dims) == ("LAZY_GEMM", 32768)
    psi, W = qil.SignalMPS(_mps([32, 32], rng, F), amplitude=1.7), qil.SingleSiteMPO(_mpo([32, 32], rng, F))
    bits = rng.integers(0, 2, size=(nb, 3)).astype(np.uint8)
    put("apply_coefficient_batch[gemm form, two passes]/f64-f64", qil.apply_coefficient_batch(W, psi, bits))


def run_stage(stage):
    sys.path.insert(0, ROOT)
    import qilaplace_jl_amd as qil
    res = {}

    def put(key, v):
        assert key not in res, key
        res[key] = np.ascontiguousarray(v)

    def put_top_k(key, found):
        for name, v in zip(("rows", "values", "bound", "certified"), found):
            put(f"{key}/{name}", v)

    if stage.startswith("apply_"):
        for k, (dta, dtw) in enumerate(DT_PAIRS):
            n = 6 + k % 3
            rng = np.random.default_rng(500 + k)
            tag = DT_IDS[k]
            psi = qil.SignalMPS(_mps(CHI[k % 2][:n - 1], rng, dta), amplitude=1.7)
            W = qil.SingleSiteMPO(_mpo(DW[:n - 1], rng, dtw))
            for name, kw in (("seed", dict(seed=99 + k)), ("uniforms", dict(uniforms=rng.random((70, n))))):
                bits, probs = qil.apply_sample(W, psi, 70, bits=True, **kw)
                put(f"apply_sample[{stage}, {name}]/bits/{tag}", bits)
                put(f"apply_sample[{stage}, {name}]/probs/{tag}", probs)
            for beam in (6, 2 ** n):
                put_top_k(f"apply_top_k[{stage}, beam={beam}]/{tag}", qil.apply_top_k(W, psi, 5, beam=beam, bits=True))
        put_top_k(f"apply_top_k[{stage}, wide]", qil.apply_top_k(*wide_lazy_case(qil), 5, beam=WIDE_BEAM, bits=True))
        return res

    def put_sites(key, mps):
        put(key + "/bonds", np.array(mps.bond_dims, dtype=np.int64))
        for i, s in enumerate(mps.to_host()):
            put(f"{key}/site{i}", s)

    for k, (dta, dtw) in enumerate(DT_PAIRS):
        n = 6 + k % 3
        rng = np.random.default_rng(500 + k)
        tag = DT_IDS[k]
        a, b, w = _mps(CHI[k % 2][:n - 1], rng, dta), _mps(PHI[:n - 1], rng, dtw), _mpo(DW[:n - 1], rng, dtw)
        psi, phi, W = qil.SignalMPS(a, amplitude=1.7), qil.SignalMPS(b, amplitude=-0.6), qil.SingleSiteMPO(w)
        rows = _weight_rows(n, rng)
        put(f"weight_batch[{stage}]/{tag}", qil.weight_batch(psi, rows))
        put(f"weight_batch[{stage}]/phi/{tag}", qil.weight_batch(phi, rows))
        if stage != "default":
            continue
        for route in ("chain", "gemm"):
            _env("QIL_INNER_ROUTE", route)
            put(f"inner[{route}]/{tag}", qil.inner(phi, psi))
        _env("QIL_INNER_ROUTE", None)
        put(f"inner[auto]/{tag}", qil.inner(phi, psi))
        put(f"norm/{tag}", [qil.norm(psi), qil.norm(phi)])
        put(f"apply_inner/{tag}", qil.inner(phi, W, psi))
        put(f"apply_norm/{tag}", qil.apply_norm(W, psi))
        put(f"apply_coefficient_batch/{tag}", qil.apply_coefficient_batch(W, psi, rng.integers(0, 2, size=(32, n)).astype(np.uint8)))
        for budget in (None, "0"):
            _env("QIL_APPLY_WEIGHT_RENV_BYTES", budget)
            put(f"apply_weight_batch[renv={budget}]/{tag}", qil.apply_weight_batch(W, psi, rows))
        _env("QIL_APPLY_WEIGHT_RENV_BYTES", None)
        for route in ("fused", "gemm"):
            _env("QIL_SAMPLE_ROUTE", route)
            bits, probs = qil.sample(psi, 70, seed=99 + k, bits=True)
            put(f"sample[{route}]/bits/{tag}", bits)
            put(f"sample[{route}]/probs/{tag}", probs)
        _env("QIL_SAMPLE_ROUTE", None)
        for beam in (6, 2 ** n):
            put_top_k(f"top_k[beam={beam}]/{tag}", qil.top_k(psi, 5, beam=beam, bits=True))
            put_top_k(f"top_k[beam={beam}]/phi/{tag}", qil.top_k(phi, 5, beam=beam, bits=True))
        spec = np.full(n, 3, dtype=np.uint8)
        spec[1], spec[n - 2] = 2, 1                                                   # a summed and a fixed site
        put_sites(f"restrict/{tag}", qil.restrict(psi, spec))
        terms = [psi, qil.SignalMPS(_mps(PHI[:n - 1], rng, dta), amplitude=0.8), qil.SignalMPS(_mps(CHI[1][:n - 1], rng, dta))]
        put_sites(f"linear_combination_compress/{tag}", qil.linear_combination_compress(terms, [1.0, -0.5, 0.25], maxdim=6, tol=1e-10))
    if stage == "default":
        for k, dt in enumerate((F, Z)):                                               # more than one selection tile
            rng = np.random.default_rng(2300 + k)
            psi = qil.SignalMPS(_mps([2, 4, 8, 8, 8, 8, 8, 8, 8, 4, 2], rng, dt), amplitude=1.7)
            put_top_k(f"top_k[wide]/{DT_IDS[3 * k]}", qil.top_k(psi, 5, beam=WIDE_BEAM, bits=True))
        W, psi, rows = boundary_case(qil)
        put("apply_weight_batch/piece_boundary", qil.apply_weight_batch(W, psi, rows))
        for k, (dta, dtw) in enumerate(DT_PAIRS):                                     # chi D = 1024: the GEMM form of the lazy read-out
            rng = np.random.default_rng(900 + k)
            psi = qil.SignalMPS(_mps([2, 32, 32, 32, 2], rng, dta), amplitude=1.7)
            W = qil.SingleSiteMPO(_mpo([4, 32, 32, 32, 4], rng, dtw))
            put(f"apply_coefficient_batch[gemm form]/{DT_IDS[k]}", qil.apply_coefficient_batch(W, psi, rng.integers(0, 2, size=(40, 6)).astype(np.uint8)))
        readout_cases(qil, put)
    return res


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    if sorted(a.files) != sorted(b.files):
        print("the dumps hold different entries:", sorted(set(a.files) ^ set(b.files)))
        return 1
    for key in sorted(a.files):
        x, y = a[key], b[key]
        if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x, y):
            worst = float(np.abs(x - y).max()) if x.shape == y.shape else float("nan")
            print(f"first difference: {key} (dtype {x.dtype} / {y.dtype}, shape {x.shape} / {y.shape}, max |a - b| = {worst:.3e})")
            return 1
    print(f"{len(a.files)} entries, all bit-equal")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--stage", choices=sorted(STAGES), help="(internal) run one stage in this process")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not args.out:
        ap.error("--out or --compare")
    if args.stage:
        np.savez(args.out, **run_stage(args.stage))
        return 0
    merged = {}
    with tempfile.TemporaryDirectory() as tmp:
        for stage, env in STAGES.items():
            part = os.path.join(tmp, stage + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", stage, "--out", part], check=True,
                           env=dict(os.environ, **env), timeout=600)
            with np.load(part) as z:
                merged.update({k: z[k] for k in z.files})
    np.savez(args.out, **merged)
    print(f"{len(merged)} entries -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
