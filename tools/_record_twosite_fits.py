"""Records tests/golden/twosite_fits.json: the answers of qil_mps_solve_local_fits, qil_mps_eigs_local_fits and
qil_mps_evolve_local_fits on the grids of tests/test_twosite_fits_golden.py (f64 / c64, one and two sites, the route variable
unset / local / gemm), one string of 0 / 1 per grid.  Needs no GPU.  Run it against the library whose decisions are the reference --
the commit BEFORE a change to the route rule or to a byte formula (QILHIP_LIB=/path/to/that/libqilhip.so) -- and commit the file.

    QILHIP_LIB=<reference library> python tools/_record_twosite_fits.py
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    T = importlib.import_module("test_twosite_fits_golden")
    L = importlib.import_module("qilaplace_jl_amd._lib")
    pts = T.grids()
    rec = {"library": L.lib.qil_version().decode(), "points": {v: len(p) for v, p in pts.items()}, "answers": {}}
    for key, verb, cx, sites, route in T.cases():
        rec["answers"][key] = T.answers(L.lib, verb, cx, sites, route, pts[verb])
        print(f"{key:28s} fits {rec['answers'][key].count('1'):4d} of {len(pts[verb])}")
    with open(T.FIXTURE, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(T.FIXTURE, ROOT), "from", L.LIB_PATH)


if __name__ == "__main__":
    main()
