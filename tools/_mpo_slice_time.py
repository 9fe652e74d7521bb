"""Times of the operator read-outs (qil.mpo_entry_batch, mpo_column, mpo_row) on one GPU, each against what the library offered
for the same answer before them.  Call times by HIP events around the whole call (every call ends in a stream synchronisation),
ten repetitions after two warm-up rounds, median and range; the two sides of a comparison alternate inside one process, and
their results are compared at the sizes that are timed.

  entries    64 (8 x 8) and 4096 (64 x 64) entries M[in, out] of the n = 24 zT (48 tensors) and QFT operators: one
             mpo_entry_batch call against one apply_coefficient_batch per distinct input on a basis state.
  column     mpo_column(W, j) against apply(W, basis state j), same operators.
  row        mpo_row(W, k) against apply(adjoint(W), basis state k) with the adjoint built beforehand (its own time is a record).
  routes     mpo_entry_batch forced onto each route (QIL_MPO_ENTRY_ROUTE, read per call) at n = 24 tensors, f64 and c64, saturated
             bonds capped at 16, 64, 128 and 512, nb = 64 and 4096 rows of fixed bits (--bonds / --rows take other grids: the
             auto rule's crossover was placed with 32, 64, 96 x 64, 256, 1024, 4096 as well).  The auto route is timed next to them.

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
    """Marketing name of the first GPU agent rocminfo lists ("unknown" where there is none: the CPU agents have names too)."""
    try:
        out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        return "unknown"
    for agent in out.split("Agent ")[1:]:
        kind = [l.split(":", 1)[1].strip() for l in agent.splitlines() if l.strip().startswith("Device Type")]
        name = [l.split(":", 1)[1].strip() for l in agent.splitlines() if "Marketing Name" in l]
        if kind and kind[0] == "GPU" and name and name[0]:
            return name[0]
    return "unknown"


def with_env(name, value, fn):
    def run():
        os.environ[name] = value
        try:
            return fn()
        finally:
            os.environ.pop(name, None)
    return run


def basis(bits, like_paired, sites):
    data = []
    for b in bits:
        A = np.zeros((1, 2, 1))
        A[0, int(b), 0] = 1.0
        data.append(A)
    return (qil.ZTMPS if like_paired else qil.SignalMPS)(data, sites=sites)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="entries,column,row,routes")
    ap.add_argument("--bonds", default="16,64,128,512", help="bond caps of the route comparison")
    ap.add_argument("--rows", default="64,4096", help="row counts of the route comparison")
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

    n = 24
    rng = np.random.default_rng(27)
    if any(k in args.only for k in ("entries", "column", "row")):
        operators = {"zt": qil.build_zt_mpo(n, 0.5), "qft": qil.build_qft_mpo(n)}
    else:
        operators = {}
    for name, W in operators.items():
        paired = isinstance(W, qil.PairedSiteMPO)
        nt = 2 * n if paired else n
        ids = W.site_ids
        info = dict(operator=name, tensors=nt, max_bond=max(W.bond_dims), dtype=np.dtype(W.dtype).name)
        if "entries" in args.only:
            for side in (8, 64):
                ins, outs = rng.integers(0, 2, (side, nt)).astype(np.uint8), rng.integers(0, 2, (side, nt)).astype(np.uint8)
                states = [basis(b, paired, ids) for b in ins]
                new = lambda: qil.mpo_entries(W, ins, outs)
                old = lambda: np.stack([qil.apply_coefficient_batch(W, s, outs) for s in states])
                a, b = new(), old()
                ts = timed_pair(ctx, {"mpo_entries": new, "apply_coefficient_batch_per_input": old}, args.reps)
                for verb, t in ts.items():
                    emit(dict(case=f"entries_{name}_n24_{side}x{side}", verb=verb, entries=side * side, distinct_inputs=side,
                              new_vs_old_of_scale=float(np.abs(a - b).max() / np.abs(b).max()), **info, **stats(t)))
        bits = rng.integers(0, 2, nt).astype(np.uint8)
        state = basis(bits, paired, ids)
        probe = rng.integers(0, 2, (256, nt)).astype(np.uint8)
        if "column" in args.only:
            new, old = (lambda: qil.mpo_column(W, bits)), (lambda: qil.apply(W, state))
            a, b = qil.coefficient_batch(new(), probe), qil.coefficient_batch(old(), probe)
            ts = timed_pair(ctx, {"mpo_column": new, "apply_on_basis_state": old}, args.reps)
            for verb, t in ts.items():
                emit(dict(case=f"column_{name}_n24", verb=verb, new_vs_old_of_scale=float(np.abs(a - b).max() / np.abs(b).max()),
                          **info, **stats(t)))
        if "row" in args.only:
            ctx.timer_start()
            Wd = qil.adjoint(W)
            emit(dict(case=f"adjoint_{name}_n24", verb="adjoint", ms_once=ctx.timer_stop(), **info))
            new, old = (lambda: qil.mpo_row(W, bits)), (lambda: qil.apply(Wd, state))
            # (W^dagger e_k)_j = conj(M[j, k]): the parent's route ends with a conjugation by hand
            a, b = qil.coefficient_batch(new(), probe), np.conj(qil.coefficient_batch(old(), probe))
            ts = timed_pair(ctx, {"mpo_row": new, "apply_adjoint_on_basis_state": old}, args.reps)
            for verb, t in ts.items():
                emit(dict(case=f"row_{name}_n24", verb=verb, new_vs_old_of_scale=float(np.abs(a - b).max() / np.abs(b).max()),
                          **info, **stats(t)))
            del Wd
    operators.clear()
    if "routes" in args.only:
        for bond in [int(v) for v in args.bonds.split(",")]:
            for dt in (np.float64, np.complex128):
                W = qil.SingleSiteMPO.alloc(saturated_profile(n, bond, base=4), dtype=dt).fill_random(7)
                for nb in [int(v) for v in args.rows.split(",")]:
                    spec = rng.integers(0, 2, (nb, n, 2)).astype(np.uint8)
                    run = lambda: qil.mpo_entry_batch(W, spec)
                    chain, gemm = with_env("QIL_MPO_ENTRY_ROUTE", "chain", run), with_env("QIL_MPO_ENTRY_ROUTE", "gemm", run)
                    a, b = chain(), gemm()
                    ts = timed_pair(ctx, {"chain": chain, "gemm": gemm, "auto": run}, args.reps)
                    for route, t in ts.items():
                        emit(dict(case=f"routes_n24_bond{bond}_{np.dtype(dt).name}_nb{nb}", route=route, bond=bond, nb=nb,
                                  dtype=np.dtype(dt).name, chain_vs_gemm_of_scale=float(np.abs(a - b).max() / np.abs(b).max()),
                                  **stats(t)))
                del W


if __name__ == "__main__":
    main()
