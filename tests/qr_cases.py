"""The table of thin-QR cases shared by tests/test_qr_plan.py (CPU: which kernels does each case reach?) and tests/test_gpu_qr.py
(GPU: is what they compute right?).  It plays the role gemm_cases.py and gauge_cases.py play: one Case per row, the plan it is
aimed at written beside it as a label (`label` below turns a qil_qr_plan_info into the same words), so a re-tuned threshold that
silently moves a case to another kernel fails in test_qr_plan.py and the table is re-aimed.  Nothing here needs a GPU or the library.

Labels.  "chol+" in front: CholeskyQR2 is tried first; the rest is the route taken when it is not tried, is skipped or refuses.
  cgs2:lds[-short]   one launch of the CGS2 kernel, operand in LDS (-short: m <= 256, a 16-lane row per previous column)
  cgs2:glob          ... operand in global memory (16 register accumulators per sweep over the rows)
  hh:hh<KM>w<W>      one Householder panel, rows-per-lane variant KM, W waves
  tree:<c>x<r>+<l>   the row-chunk tree: c chunks of r rows, the last one l rows long; ":chunks-glob" when a chunk x n slice of the
                     first level does not fit LDS, ":top-glob" when the stacked triangles of the second level do not
  blocked<P>:<full>/<last><w>   the blocked driver with P-column panels: the kernel of the full panels, that of the last one and its
                     width (kernels: hh<KM>w<W>, lds, glob, tree -- then the tree's chunks follow as above)

Operand kinds, generated from a seed per case (`operand`):
  well       Gaussian (m >= 2 n), else U diag(logspace(0, -1)) V^H with Haar U, V: kappa about 10
  colscaled  `well` with every column scaled by 10^U(-6, 6)
  graded     U diag(logspace(0, -d)) V^H, d per case
  deficient  rank r < n: every column a combination of r generators, the first r columns independent (as in
             test_qr_blocked_panels_with_dependent_columns), column r + 1 an exact duplicate of column 0, column r + 2 a scaled
             duplicate (-2.5 x) of column 1 -- inside one panel or across panels, depending on r and the panel width -- and the
             last column exactly zero

CholeskyQR2 outcomes (Case.chol, the `cholesky` field of qil_qr_report): 0 not eligible, 1 first-order second pass, 2 full second
factorisation, 3 refused in the first pass, 5 skipped.  Outcome 4 (refused in the SECOND pass) has no case: the first pass accepts
only pivots above 1e-11 of their diagonal entry, so kappa(A)^2 < ~1e11 and Q1^H Q1 = I + E with |E| ~ kappa^2 u < ~1e-5 -- a matrix
that close to the identity has no pivot below 1e-11, and no operand was found that passes the first test and fails the second.

The first-order pairs (n = 128, m = 512, both dtypes): `first_pass_model` is a plain numpy float64 model of the first pass, and d is
chosen so that n max|E| lies a factor MARGIN (that of gauge_cases) below the kernel's 3e-8 for the `fo` case and above it for its
partner `full` (test_qr_plan.py asserts both)."""
import zlib
from collections import namedtuple

import numpy as np

from gauge_cases import MARGIN

F64, C64 = np.float64, np.complex128
DTYPES = {"f64": F64, "c64": C64}
FIRST_ORDER_THRESHOLD = 3e-8                 # n max|e_ik| of the second pass of cholqr2
LONGDOUBLE_CAP = 2.5e8                       # real longdouble multiply-adds of one evaluation (in the manner of gemm_cases.ROUNDING_CAP)

Case = namedtuple("Case", "name dtype m n kind lda_pad off ldr_pad with_R reorth skip plan chol d rank run")


# ---------------------------------------------------------------- a plain restatement of the rules of qr_plan (qil_linalg.hip)
LDS_BUDGET = 150 * 1024
KM_VARIANTS = (2, 4, 6, 8, 9, 13, 19)


def esize(dtype):
    return 16 if dtype == "c64" else 8


def cgs2_lds_bytes(dtype, rows, n):
    return (2 * (n + (n & 1)) + (rows | 1) * n) * esize(dtype)


def hh_panel_fits(dtype, m, b):
    return b <= 32 and m <= 64 * 19 and ((m + 1) | 1) * b * esize(dtype) + 2048 <= LDS_BUDGET


def hh_km(m):
    km = (m + 63) // 64
    return next(v for v in KM_VARIANTS if km <= v)


def hh_waves(dtype, km):
    return 8 if km * (esize(dtype) // 8) > 18 else 16


def tree_chunk(m):
    return max(512, (m // 512 + 255) // 256 * 256)


def cholesky_eligible(m, n):
    return 64 <= n <= 1024 and m >= n and (m * n <= 1 << 22 or (n <= 256 and m * n <= 1 << 24))


def restate(dtype, m, n):
    """The plan of an m x n operand as a dict with the keys of ops.qr_plan, from the rules written out again."""
    fits = lambda rows, b: cgs2_lds_bytes(dtype, rows, b) <= LDS_BUDGET
    tree = m >= 2048 or (not fits(m, 16) and m >= 640)
    hh_ok = not tree and n > 16 and hh_panel_fits(dtype, m, min(n, 32))
    p = dict.fromkeys(("has_hh", "has_tree", "has_cgs2_lds", "has_cgs2_global", "fused_in_lds", "fused_short_rows", "hh_km",
                       "hh_waves", "tree_chunk", "tree_chunks", "tree_last_rows", "tree_in_lds", "tree_top_in_lds"), 0)
    p["cholesky_eligible"] = int(cholesky_eligible(m, n))
    if hh_ok and n <= 32:
        p["route"] = "SINGLE_HH"
    elif n <= 16 or (fits(m, n) and not hh_ok):
        p["route"] = "SINGLE_TREE" if tree and n <= 16 else "SINGLE_CGS2"
    else:
        p["route"] = "BLOCKED"

    def panel(b):
        if tree and b <= 16:
            p["has_tree"] = 1
            return "TREE"
        if p["route"] != "SINGLE_CGS2" and hh_panel_fits(dtype, m, b):
            p["has_hh"] = 1
            return "HH"
        kind = "CGS2_LDS" if fits(m, b) else "CGS2_GLOBAL"
        p["has_cgs2_lds" if kind == "CGS2_LDS" else "has_cgs2_global"] = 1
        return kind

    if p["route"] != "BLOCKED":
        p["panel_width"] = p["last_panel_width"] = n
        p["panel_kind"] = p["last_panel_kind"] = panel(n)
    else:
        p["panel_width"] = 32 if not tree and fits(m, 32) else 16
        p["last_panel_width"] = n - (n - 1) // p["panel_width"] * p["panel_width"]
        p["panel_kind"], p["last_panel_kind"] = panel(p["panel_width"]), panel(p["last_panel_width"])
    p["fused_in_lds"] = int(p["has_cgs2_lds"] and not p["has_cgs2_global"])
    p["fused_short_rows"] = int(p["has_cgs2_lds"] and m <= 256)
    if p["has_hh"]:
        p["hh_km"] = hh_km(m)
        p["hh_waves"] = hh_waves(dtype, p["hh_km"])
    if p["has_tree"]:
        ch = tree_chunk(m)
        nch = -(-m // ch)
        b = min(n, 16)
        p.update(tree_chunk=ch, tree_chunks=nch, tree_last_rows=m - (nch - 1) * ch, tree_in_lds=int(fits(min(ch, m), b)),
                 tree_top_in_lds=int(fits(nch * b, b)))
    return p


def label(p):
    """A qil_qr_plan_info (the dict of ops.qr_plan or of `restate`) in the words of the table."""
    def kern(kind):
        return {"HH": f"hh{p['hh_km']}w{p['hh_waves']}", "TREE": "tree", "CGS2_LDS": "lds", "CGS2_GLOBAL": "glob"}[kind]
    tree = ""
    if p["has_tree"]:
        tree = f"{p['tree_chunks']}x{p['tree_chunk']}+{p['tree_last_rows']}" + ("" if p["tree_in_lds"] else ":chunks-glob") + \
            ("" if p["tree_top_in_lds"] else ":top-glob")
    if p["route"] == "SINGLE_CGS2":
        s = "cgs2:" + kern(p["panel_kind"]) + ("-short" if p["fused_short_rows"] else "")
    elif p["route"] == "SINGLE_HH":
        s = "hh:" + kern("HH")
    elif p["route"] == "SINGLE_TREE":
        s = "tree:" + tree
    else:
        s = f"blocked{p['panel_width']}:{kern(p['panel_kind'])}/{kern(p['last_panel_kind'])}{p['last_panel_width']}" + \
            (":" + tree if tree else "")
    return ("chol+" if p["cholesky_eligible"] else "") + s


# ---------------------------------------------------------------- the table
def _c(dtype, m, n, plan, kind="well", pad=(0, 0, 0), with_R=True, skip=0, chol=None, d=None, rank=None, run=True, tag=""):
    if chol is None:
        chol = 0 if not plan.startswith("chol+") else 5 if skip else 1
    if kind == "deficient" and rank is None:
        rank = max(1, n // 3)
    name = f"{dtype}_{m}x{n}_{kind}" + (f"_d{d:g}" if d is not None else "") + (f"_rank{rank}" if rank is not None else "") + \
        ("_padded" if any(pad) else "") + ("" if with_R else "_noR") + ("_skip" if skip else "") + ("" if run else "_planonly") + tag
    return Case(name, dtype, m, n, kind, pad[0], pad[1], pad[2], with_R, 0, skip, plan, chol, d, rank, run)


PAD = (3, 5, 2)          # lda = m + 3, off = 5 (A and R), ldr = n + 2

# the first tall sizes at which the tree's second level, then its first level, leave LDS (16 columns; test_qr_plan.py checks that
# these ARE the first: the plan one row shorter still has them in LDS)
TOP_GLOBAL_M = {"f64": 37889, "c64": 18945}
CHUNKS_GLOBAL_M = {"f64": 524800, "c64": 262656}

_ROWS = [
    # ---- single CGS2 launch, operand in LDS
    _c("f64", 1, 1, "cgs2:lds-short"), _c("c64", 1, 1, "cgs2:lds-short"),
    _c("f64", 7, 1, "cgs2:lds-short", pad=PAD), _c("c64", 7, 1, "cgs2:lds-short", kind="colscaled"),
    _c("f64", 9, 2, "cgs2:lds-short", kind="colscaled"), _c("c64", 9, 2, "cgs2:lds-short", with_R=False),
    _c("f64", 40, 15, "cgs2:lds-short", kind="deficient"), _c("c64", 40, 15, "cgs2:lds-short", kind="deficient"),
    _c("f64", 16, 16, "cgs2:lds-short"), _c("c64", 16, 16, "cgs2:lds-short"),
    _c("f64", 256, 16, "cgs2:lds-short", kind="colscaled"), _c("c64", 256, 16, "cgs2:lds-short"),
    _c("f64", 257, 16, "cgs2:lds"), _c("c64", 257, 16, "cgs2:lds", kind="colscaled"),
    _c("f64", 256, 3, "cgs2:lds-short", kind="graded", d=4), _c("c64", 257, 3, "cgs2:lds", kind="graded", d=4),
    _c("f64", 300, 16, "cgs2:lds", pad=PAD), _c("c64", 300, 16, "cgs2:lds", pad=PAD),
    _c("f64", 300, 16, "cgs2:lds", with_R=False), _c("c64", 300, 16, "cgs2:lds", with_R=False),
    _c("f64", 300, 16, "cgs2:lds", kind="deficient", rank=5), _c("c64", 300, 16, "cgs2:lds", kind="graded", d=14),
    _c("f64", 1197, 16, "cgs2:lds"), _c("c64", 597, 16, "cgs2:lds"),
    # (more than 16 columns where the Householder panel no longer fits but the operand still does)
    _c("f64", 950, 20, "cgs2:lds"), _c("c64", 475, 20, "cgs2:lds"),
    _c("f64", 957, 20, "cgs2:lds", kind="colscaled"), _c("c64", 477, 20, "cgs2:lds", kind="deficient"),
    _c("f64", 1120, 17, "cgs2:lds", kind="deficient"), _c("f64", 594, 32, "cgs2:lds"), _c("c64", 296, 32, "cgs2:lds"),
    # ---- single CGS2 launch out of LDS (complex only: see test_qr_plan.py)
    _c("c64", 600, 16, "cgs2:glob"), _c("c64", 639, 16, "cgs2:glob", kind="colscaled"),
    _c("c64", 600, 16, "cgs2:glob", pad=PAD), _c("c64", 600, 16, "cgs2:glob", with_R=False),
    _c("c64", 638, 15, "cgs2:glob"), _c("c64", 639, 15, "cgs2:glob", kind="deficient"),
    _c("c64", 620, 16, "cgs2:glob", kind="graded", d=4), _c("c64", 620, 16, "cgs2:glob", kind="deficient", rank=9),
    # ---- single Householder panel: squares, and one m on each side of every KM edge
    _c("f64", 17, 17, "hh:hh2w16"), _c("c64", 17, 17, "hh:hh2w16"), _c("f64", 32, 32, "hh:hh2w16"), _c("c64", 32, 32, "hh:hh2w16"),
    _c("f64", 128, 17, "hh:hh2w16"), _c("f64", 129, 17, "hh:hh4w16"), _c("f64", 256, 17, "hh:hh4w16", kind="colscaled"),
    _c("f64", 257, 17, "hh:hh6w16"), _c("f64", 384, 17, "hh:hh6w16"), _c("f64", 385, 17, "hh:hh8w16", kind="deficient"),
    _c("f64", 512, 17, "hh:hh8w16"), _c("f64", 513, 17, "hh:hh9w16"), _c("f64", 576, 17, "hh:hh9w16", kind="colscaled"),
    _c("f64", 577, 17, "hh:hh13w16"), _c("f64", 832, 17, "hh:hh13w16"), _c("f64", 833, 17, "hh:hh19w8"),
    _c("f64", 1112, 17, "hh:hh19w8", kind="graded", d=4), _c("f64", 1112, 17, "hh:hh19w8", kind="deficient"),
    _c("f64", 129, 32, "hh:hh4w16", pad=PAD), _c("f64", 129, 32, "hh:hh4w16", with_R=False), _c("f64", 129, 32, "hh:hh4w16"),
    _c("f64", 590, 32, "hh:hh13w16"), _c("f64", 300, 32, "hh:hh6w16", kind="deficient", rank=12),
    _c("c64", 128, 17, "hh:hh2w16"), _c("c64", 129, 17, "hh:hh4w16", kind="colscaled"), _c("c64", 256, 17, "hh:hh4w16"),
    _c("c64", 257, 17, "hh:hh6w16"), _c("c64", 384, 17, "hh:hh6w16", kind="deficient"), _c("c64", 385, 17, "hh:hh8w16"),
    _c("c64", 512, 17, "hh:hh8w16"), _c("c64", 513, 17, "hh:hh9w16"), _c("c64", 556, 17, "hh:hh9w16", kind="graded", d=4),
    _c("c64", 257, 32, "hh:hh6w16", pad=PAD), _c("c64", 257, 32, "hh:hh6w16", with_R=False), _c("c64", 257, 32, "hh:hh6w16"),
    _c("c64", 294, 32, "hh:hh6w16", kind="colscaled"), _c("c64", 200, 32, "hh:hh4w16", kind="deficient", rank=12),
    # ---- single tree panel
    _c("f64", 2048, 16, "tree:4x512+512"), _c("c64", 2048, 16, "tree:4x512+512"),
    _c("f64", 2049, 16, "tree:5x512+1"), _c("c64", 2049, 16, "tree:5x512+1"),
    _c("f64", 2063, 16, "tree:5x512+15", kind="colscaled"), _c("c64", 2063, 16, "tree:5x512+15", kind="colscaled"),
    _c("f64", 2049, 3, "tree:5x512+1", kind="colscaled"), _c("c64", 2049, 3, "tree:5x512+1"),
    _c("f64", 2048, 1, "tree:4x512+512"), _c("c64", 2049, 1, "tree:5x512+1"),
    _c("f64", 1198, 16, "tree:3x512+174"), _c("c64", 640, 16, "tree:2x512+128"),
    _c("f64", 1198, 1, "tree:3x512+174", kind="colscaled"), _c("c64", 640, 3, "tree:2x512+128", kind="graded", d=4),
    _c("f64", 2063, 16, "tree:5x512+15", kind="deficient", rank=7), _c("c64", 2049, 16, "tree:5x512+1", kind="deficient", rank=7),
    _c("f64", 2100, 16, "tree:5x512+52", pad=PAD), _c("c64", 2100, 16, "tree:5x512+52", pad=PAD),
    _c("f64", 2100, 16, "tree:5x512+52", with_R=False), _c("c64", 2100, 16, "tree:5x512+52", with_R=False),
    _c("f64", 2100, 16, "tree:5x512+52", kind="graded", d=4),
    _c("f64", TOP_GLOBAL_M["f64"], 16, "tree:75x512+1:top-glob"), _c("c64", TOP_GLOBAL_M["c64"], 16, "tree:38x512+1:top-glob"),
    _c("f64", CHUNKS_GLOBAL_M["f64"], 16, "tree:410x1280+1280:chunks-glob:top-glob"),
    _c("c64", CHUNKS_GLOBAL_M["c64"], 16, "tree:342x768+768:chunks-glob:top-glob"),
    # ---- blocked, 32 columns per panel, Householder panels: last panels of 1, 8, 16, 31 columns; squares
    _c("f64", 100, 33, "blocked32:hh2w16/hh2w161"), _c("c64", 100, 33, "blocked32:hh2w16/hh2w161"),
    _c("f64", 40, 40, "blocked32:hh2w16/hh2w168"), _c("c64", 40, 40, "blocked32:hh2w16/hh2w168"),
    _c("f64", 200, 40, "blocked32:hh4w16/hh4w168", kind="colscaled"), _c("c64", 200, 40, "blocked32:hh4w16/hh4w168", kind="deficient"),
    _c("f64", 300, 48, "blocked32:hh6w16/hh6w1616", pad=PAD), _c("c64", 200, 48, "blocked32:hh4w16/hh4w1616", pad=PAD),
    _c("f64", 300, 48, "blocked32:hh6w16/hh6w1616", with_R=False), _c("c64", 200, 48, "blocked32:hh4w16/hh4w1616", with_R=False),
    _c("f64", 300, 48, "blocked32:hh6w16/hh6w1616", kind="deficient", rank=20), _c("c64", 200, 48, "blocked32:hh4w16/hh4w1616", kind="graded", d=4),
    _c("f64", 400, 63, "blocked32:hh8w16/hh8w1631"), _c("c64", 200, 63, "blocked32:hh4w16/hh4w1631", kind="colscaled"),
    _c("f64", 200, 64, "chol+blocked32:hh4w16/hh4w1632", skip=1), _c("c64", 200, 64, "chol+blocked32:hh4w16/hh4w1632", skip=1),
    _c("f64", 300, 65, "chol+blocked32:hh6w16/hh6w161", skip=1), _c("c64", 250, 65, "chol+blocked32:hh4w16/hh4w161", skip=1, kind="colscaled"),
    _c("f64", 400, 130, "chol+blocked32:hh8w16/hh8w162", skip=1), _c("c64", 280, 130, "chol+blocked32:hh6w16/hh6w162", skip=1),
    # ---- blocked, 32 columns per panel, CGS2 first panels and a Householder (or CGS2) last panel
    _c("f64", 594, 40, "blocked32:lds/hh13w168"), _c("c64", 296, 40, "blocked32:lds/hh6w168"),
    _c("f64", 594, 33, "blocked32:lds/hh13w161", kind="colscaled"), _c("c64", 296, 63, "blocked32:lds/hh6w1631", kind="deficient"),
    _c("f64", 594, 64, "chol+blocked32:lds/lds32", skip=1), _c("c64", 296, 64, "chol+blocked32:lds/lds32", skip=1),
    _c("f64", 594, 130, "chol+blocked32:lds/hh13w162", skip=1, kind="graded", d=4),
    # ---- blocked, 16 columns per panel, Householder panels
    _c("f64", 700, 48, "blocked16:hh13w16/hh13w1616"), _c("c64", 400, 48, "blocked16:hh8w16/hh8w1616"),
    _c("f64", 900, 63, "blocked16:hh19w8/hh19w815", kind="colscaled"), _c("c64", 520, 63, "blocked16:hh9w16/hh9w1615"),
    _c("f64", 700, 33, "blocked16:hh13w16/hh13w161", kind="deficient"), _c("c64", 580, 33, "blocked16:hh13w8/hh13w81"),
    _c("f64", 1000, 65, "chol+blocked16:hh19w8/hh19w81", skip=1), _c("c64", 580, 130, "chol+blocked16:hh13w8/hh13w82", skip=1),
    _c("f64", 700, 48, "blocked16:hh13w16/hh13w1616", pad=PAD), _c("c64", 400, 48, "blocked16:hh8w16/hh8w1616", with_R=False),
    # ---- blocked, 16 columns per panel, CGS2 panels in LDS
    _c("f64", 1190, 48, "blocked16:lds/lds16"), _c("c64", 594, 48, "blocked16:lds/lds16"),
    _c("f64", 1190, 33, "blocked16:lds/hh19w81", kind="colscaled"), _c("c64", 594, 33, "blocked16:lds/hh13w81"),
    _c("f64", 1190, 63, "blocked16:lds/hh19w815", kind="deficient"), _c("c64", 594, 63, "blocked16:lds/hh13w815", kind="colscaled"),
    _c("f64", 1190, 64, "chol+blocked16:lds/lds16", skip=1), _c("c64", 594, 65, "chol+blocked16:lds/hh13w81", skip=1),
    _c("f64", 1190, 48, "blocked16:lds/lds16", pad=PAD), _c("c64", 594, 48, "blocked16:lds/lds16", with_R=False),
    # ---- blocked, 16 columns per panel, CGS2 panels out of LDS, and the complex mix of both modes
    _c("c64", 620, 48, "blocked16:glob/glob16"), _c("c64", 620, 33, "blocked16:glob/hh13w81", kind="colscaled"),
    _c("c64", 620, 63, "blocked16:glob/hh13w815", kind="deficient"), _c("c64", 634, 63, "blocked16:glob/lds15"),
    _c("c64", 639, 63, "blocked16:glob/glob15"), _c("c64", 620, 130, "chol+blocked16:glob/hh13w82", skip=1),
    _c("c64", 620, 48, "blocked16:glob/glob16", pad=PAD), _c("c64", 620, 48, "blocked16:glob/glob16", with_R=False),
    _c("c64", 634, 63, "blocked16:glob/lds15", kind="graded", d=4),
    # ---- blocked, 16 columns per panel, tree panels
    _c("f64", 1198, 33, "blocked16:tree/tree1:3x512+174"), _c("c64", 640, 40, "blocked16:tree/tree8:2x512+128"),
    _c("f64", 2049, 48, "blocked16:tree/tree16:5x512+1", kind="colscaled"), _c("c64", 700, 63, "blocked16:tree/tree15:2x512+188"),
    _c("f64", 1300, 63, "blocked16:tree/tree15:3x512+276", kind="deficient"), _c("c64", 2049, 33, "blocked16:tree/tree1:5x512+1", kind="deficient"),
    _c("f64", 1300, 65, "chol+blocked16:tree/tree1:3x512+276", skip=1), _c("c64", 700, 130, "chol+blocked16:tree/tree2:2x512+188", skip=1),
    _c("f64", 1300, 48, "blocked16:tree/tree16:3x512+276", pad=PAD), _c("c64", 700, 48, "blocked16:tree/tree16:2x512+188", with_R=False),
    # ---- CholeskyQR2: chol_inv's 64-blocks with a remainder of 0, 1 and 63, two trtri_merge levels; m = n and m a few times n
    _c("f64", 64, 64, "chol+blocked32:hh2w16/hh2w1632"), _c("c64", 64, 64, "chol+blocked32:hh2w16/hh2w1632"),
    _c("f64", 200, 64, "chol+blocked32:hh4w16/hh4w1632", pad=PAD), _c("c64", 200, 64, "chol+blocked32:hh4w16/hh4w1632", with_R=False),
    _c("f64", 65, 65, "chol+blocked32:hh2w16/hh2w161"), _c("c64", 260, 65, "chol+blocked32:hh6w16/hh6w161", kind="colscaled"),
    _c("f64", 400, 127, "chol+blocked32:hh8w16/hh8w1631", kind="colscaled"), _c("c64", 127, 127, "chol+blocked32:hh2w16/hh2w1631"),
    _c("f64", 128, 128, "chol+blocked32:hh2w16/hh2w1632"), _c("c64", 400, 128, "chol+blocked16:hh8w16/hh8w1616", pad=PAD),
    _c("f64", 129, 129, "chol+blocked32:hh4w16/hh4w161"), _c("c64", 390, 129, "chol+blocked16:hh8w16/hh8w161"),
    _c("f64", 400, 128, "chol+blocked32:hh8w16/hh8w1632", with_R=False),
    _c("f64", 320, 320, "chol+blocked32:hh6w16/hh6w1632"), _c("c64", 320, 320, "chol+blocked16:hh6w16/hh6w1616"),
    _c("f64", 1000, 320, "chol+blocked16:hh19w8/hh19w816"),
    # the first-order claim: n max|E| a factor MARGIN below 3e-8 (outcome 1) and above it (outcome 2)
    _c("f64", 512, 128, "chol+blocked32:hh8w16/hh8w1632", kind="graded", d=3, chol=1, tag="_fo"),
    _c("f64", 512, 128, "chol+blocked32:hh8w16/hh8w1632", kind="graded", d=4.5, chol=2, tag="_full"),
    _c("c64", 512, 128, "chol+blocked16:hh8w16/hh8w1616", kind="graded", d=3, chol=1, tag="_fo"),
    _c("c64", 512, 128, "chol+blocked16:hh8w16/hh8w1616", kind="graded", d=4.5, chol=2, tag="_full"),
    # (kappa^2 u far above the first-order threshold, the smallest pivot ~3e-8 of its diagonal entry: still far from the refusal)
    _c("f64", 512, 128, "chol+blocked32:hh8w16/hh8w1632", kind="graded", d=5.5, chol=2),
    _c("c64", 512, 128, "chol+blocked16:hh8w16/hh8w1616", kind="graded", d=5.5, chol=2),
    # refusals in the first pass: the panel routes take over inside the same call.  (d = 7, where the parity suite expects the
    # refusal, sits within a factor of about 3 of the 1e-11 pivot test and is accepted on the device: d = 10 is far beyond)
    _c("f64", 512, 128, "chol+blocked32:hh8w16/hh8w1632", kind="graded", d=10, chol=3),
    _c("c64", 512, 128, "chol+blocked16:hh8w16/hh8w1616", kind="graded", d=10, chol=3),
    _c("f64", 400, 96, "chol+blocked32:hh8w16/hh8w1632", kind="deficient", rank=40, chol=3),
    _c("c64", 700, 130, "chol+blocked16:tree/tree2:2x512+188", kind="deficient", rank=100, chol=3),
    # ---- plan-only rows: the eligibility edges of CholeskyQR2 (checked on the CPU, not run)
    _c("f64", 512, 63, "blocked32:hh8w16/hh8w1631", run=False), _c("f64", 512, 64, "chol+blocked32:hh8w16/hh8w1632", run=False),
    _c("c64", 2048, 1024, "chol+blocked16:tree/tree16:4x512+512", run=False), _c("c64", 2048, 1025, "blocked16:tree/tree1:4x512+512", run=False),
    _c("f64", 4096, 1024, "chol+blocked16:tree/tree16:8x512+512", run=False), _c("f64", 4097, 1024, "blocked16:tree/tree16:9x512+1", run=False),
    _c("f64", 16320, 257, "chol+blocked16:tree/tree1:32x512+448", run=False), _c("f64", 16321, 257, "blocked16:tree/tree1:32x512+449", run=False),
    _c("c64", 65536, 256, "chol+blocked16:tree/tree16:128x512+512:top-glob", run=False), _c("c64", 65537, 256, "blocked16:tree/tree16:129x512+1:top-glob", run=False),
]


CASES = _ROWS
assert len({c.name for c in CASES}) == len(CASES), "duplicate case names"
BY_NAME = {c.name: c for c in CASES}
RUN = [c for c in CASES if c.run]
PLAN_ONLY = [c for c in CASES if not c.run]
ELIGIBILITY_EDGES = list(zip(PLAN_ONLY[0::2], PLAN_ONLY[1::2]))   # neighbours in n or in m, one eligible and one not
FIRST_ORDER_PAIRS = [(f"{d}_512x128_graded_d3_fo", f"{d}_512x128_graded_d4.5_full") for d in DTYPES]


def np_dtype(c):
    return DTYPES[c.dtype]


def gram_cost(c):
    """Real multiply-adds of evaluating case c in longdouble: the Gram product Q^H Q and the product Q R (complex: 3 + 4 real ones)."""
    return c.m * c.n * c.n * (7 if c.dtype == "c64" else 2)


# ---------------------------------------------------------------- operands
def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(x) for x in key).encode()))


def _gauss(rng, dt, *shape):
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if dt == C64 else x


def _haar(rng, dt, m, n):
    q, r = np.linalg.qr(_gauss(rng, dt, m, n))
    d = np.diagonal(r)
    return q * (d / np.abs(d))


def _spectrum(rng, dt, m, n, sigma):
    return (_haar(rng, dt, m, n) * sigma) @ _haar(rng, dt, n, n).conj().T


def operand(c):
    """The m x n operand of case c (Fortran order), from a seed that is a function of the case's name."""
    rng, dt = _rng("qr", c.name), np_dtype(c)
    m, n = c.m, c.n
    if c.kind in ("well", "colscaled"):
        A = _gauss(rng, dt, m, n) if m >= 2 * n else _spectrum(rng, dt, m, n, np.logspace(0, -1, n))
        if c.kind == "colscaled":
            A = A * 10.0 ** rng.uniform(-6, 6, size=n)
    elif c.kind == "graded":
        A = _spectrum(rng, dt, m, n, np.logspace(0, -c.d, n))
    elif c.kind == "deficient":
        r = c.rank
        assert 1 <= r < n
        C = _gauss(rng, dt, r, n)
        C[:, :r] += 3 * np.eye(r)                                  # the first r columns independent
        A = _gauss(rng, dt, m, r) @ C
        if n > r + 2:
            A[:, r + 1] = A[:, 0]                                  # an exact duplicate, a scaled duplicate
            A[:, r + 2] = -2.5 * A[:, 1]
        if n > r + 3:
            A[:, n - 1] = 0                                        # a zero column
    else:
        raise ValueError(c.kind)
    return np.asfortranarray(A, dtype=dt)


def first_pass_model(A):
    """n max|E| of the first pass of CholeskyQR2 in plain float64 numpy: G = A^H A, R1 = chol(G), Q1 = A R1^-1, E = Q1^H Q1 - I."""
    n = A.shape[1]
    R1 = np.linalg.cholesky(A.conj().T @ A).conj().T
    Q1 = np.linalg.solve(R1.conj().T, A.conj().T).conj().T
    return n * float(np.abs(Q1.conj().T @ Q1 - np.eye(n)).max())


# ---------------------------------------------------------------- layout
Layout = namedtuple("Layout", "a_elems a_off lda r_elems r_off ldr")


def layout(c):
    """Parent buffers: the window at `off`, whole columns of the padded leading dimension, a tail behind the last one."""
    lda, ldr = c.m + c.lda_pad, c.n + c.ldr_pad
    tail = 7 if c.off else 0
    return Layout(c.off + lda * c.n + tail, c.off, lda, c.off + ldr * c.n + tail, c.off, ldr)
