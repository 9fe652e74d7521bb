"""The table of GEMM cases shared by tests/test_gemm_plan.py (CPU: which kernel does each case reach?) and
tests/test_gpu_gemm.py (GPU: is what that kernel computes right?).  No fixtures, no GPU, no library import.

A case is one call of the MFMA GEMM family: element type, op codes, m x n x k, how the three operands sit in their parent buffers
(leading-dimension padding, element offsets, batch layout), the epilogue, and the PLAN the dispatch is meant to reach for it --
(tile, arc, bkc, splits, kchunk, split rule, col_fastest, xcd).  The plan column is what the case is FOR: test_gemm_plan.py asserts
it against qil_gemm_plan, so a re-tuned heuristic that moves a case to another kernel fails there and the table is re-aimed, and
asserts that the table as a whole still reaches every kernel of the family (see its coverage test).

`layout(case)` turns the description into concrete offsets, leading dimensions, strides and buffer sizes; both test files use it, so
the plan that is asserted is the plan of the very call the GPU test makes."""
from collections import namedtuple

# tile names -> (bm, bn, gkt, deep); the last three exist for f64 only
TILES = {"32x64D": (32, 64, 16, 1), "48x64D": (48, 64, 16, 1), "32x32": (32, 32, 32, 0), "64x64": (64, 64, 16, 0),
         "64x144": (64, 144, 16, 0), "128x128": (128, 128, 16, 0), "128x64": (128, 64, 16, 0)}
TILES_OF = {"f64": tuple(TILES), "c64": ("32x64D", "48x64D", "32x32", "64x64")}

Plan = namedtuple("Plan", "tile arc bkc splits kchunk rule col_fastest xcd")
# batch: count products; a_shared / b_shared: batch stride 0 (one operand for all); c_gap: elements between consecutive outputs beyond
# ldc * n (0 with no ldc padding = packed); b_sel: per-batch slice selection of B as the lazy coefficient chain uses it; cmap: the
# outputs are column blocks of 32 scattered over one wide C by a permutation, as the block Jacobi uses it
Batch = namedtuple("Batch", "count a_shared b_shared c_gap b_sel cmap", defaults=(1, False, False, 0, False, False))
Case = namedtuple("Case", "name dtype ops m n k plan pad off batch skinny subtract rounding")

# the longdouble reference of the rounding model costs m n k multiply-adds (four times that for complex): cases above this are
# left to the exact check
ROUNDING_CAP = 3e8
CMAP_BLK = 32


def C(name, dtype, ops, m, n, k, plan, pad=(0, 0, 0), off=(0, 0, 0), batch=Batch(), skinny=False, subtract=False):
    cost = m * n * k * batch.count * (4 if dtype == "c64" else 1)
    return Case(name, dtype, ops, m, n, k, Plan(*plan), pad, off, batch, skinny, subtract, cost <= ROUNDING_CAP)


Layout = namedtuple("Layout", "a_rows a_cols b_rows b_cols lda ldb ldc a_off b_off c_off a_bs b_bs c_bs a_elems b_elems c_elems "
                              "c_cols b_sel b_sel_step b_sel_stride cmap")

SEL_SLICES = 3          # slices of B a b_sel case chooses from
SEL_STEP = 2            # the selector of batch i is b_sel[i * SEL_STEP] (the chain reads one bit of a row of bits)


def layout(c):
    """Concrete placement of the operands of case c in their parent buffers (all in elements)."""
    a_rows, a_cols = (c.m, c.k) if c.ops[0] in "NC" else (c.k, c.m)
    b_rows, b_cols = (c.k, c.n) if c.ops[1] in "NC" else (c.n, c.k)
    lda, ldb, ldc = a_rows + c.pad[0], b_rows + c.pad[1], c.m + c.pad[2]
    bt = c.batch
    a_bs = 0 if (bt.a_shared or bt.count == 1) else lda * a_cols + 3
    b_bs = 0 if (bt.b_shared or bt.b_sel or bt.count == 1) else ldb * b_cols + 5
    b_sel = cmap = None
    b_sel_stride = 0
    b_span = ldb * b_cols
    if bt.b_sel:
        b_sel_stride = ldb * b_cols + 1
        b_sel = [(7 * i + i // 3 + j) % SEL_SLICES for i in range(bt.count) for j in range(SEL_STEP)]
        b_span = (SEL_SLICES - 1) * b_sel_stride + ldb * b_cols
    if bt.cmap:
        assert c.n % CMAP_BLK == 0 and bt.c_gap == 0
        nblk = bt.count * (c.n // CMAP_BLK)
        step = next(s for s in (7, 5, 3, 1) if nblk % s)      # a permutation of the column blocks that is not the identity
        cmap = [(step * g + 2) % nblk for g in range(nblk)]
        c_bs, c_cols = 0, bt.count * c.n
        c_span = ldc * c_cols
    else:
        c_bs = 0 if bt.count == 1 else ldc * c.n + bt.c_gap
        c_cols = c.n
        c_span = (bt.count - 1) * c_bs + ldc * c.n
    a_elems = c.off[0] + (bt.count - 1) * a_bs + lda * a_cols + 5
    b_elems = c.off[1] + (bt.count - 1) * b_bs + b_span + 3
    c_elems = c.off[2] + c_span + 7
    return Layout(a_rows, a_cols, b_rows, b_cols, lda, ldb, ldc, c.off[0], c.off[1], c.off[2], a_bs, b_bs, c_bs, a_elems, b_elems,
                  c_elems, c_cols, b_sel, SEL_STEP if bt.b_sel else 0, b_sel_stride, cmap)


def plan_args(c):
    """The arguments of qil_gemm_plan / ops.gemm_plan for case c."""
    L = layout(c)
    return dict(dtype="complex128" if c.dtype == "c64" else "float64", m=c.m, n=c.n, k=c.k, opA=c.ops[0], opB=c.ops[1], lda=L.lda,
                ldb=L.ldb, ldc=L.ldc, count=c.batch.count, c_bs=L.c_bs, has_cmap=c.batch.cmap, skinny_m=c.skinny)


CASES = [
    # K sweeps: every K edge on one small shape per kernel family (tight operands)
    C("f64_NN_70x45x1_ksweep", "f64", "NN", 70, 45, 1, ('32x32', 1, 1, 1, 1, 0, 1, 0)),
    C("f64_NN_70x45x3_ksweep", "f64", "NN", 70, 45, 3, ('32x32', 1, 1, 1, 3, 0, 1, 0)),
    C("f64_NN_70x45x15_ksweep", "f64", "NN", 70, 45, 15, ('32x32', 1, 1, 1, 15, 0, 1, 0)),
    C("f64_NN_70x45x16_ksweep", "f64", "NN", 70, 45, 16, ('32x32', 1, 1, 1, 16, 0, 1, 0)),
    C("f64_NN_70x45x17_ksweep", "f64", "NN", 70, 45, 17, ('32x32', 1, 1, 1, 17, 0, 1, 0)),
    C("f64_NN_70x45x31_ksweep", "f64", "NN", 70, 45, 31, ('32x32', 1, 1, 1, 31, 0, 1, 0)),
    C("f64_NN_70x45x32_ksweep", "f64", "NN", 70, 45, 32, ('32x32', 1, 1, 1, 32, 0, 1, 0)),
    C("f64_NN_70x45x33_ksweep", "f64", "NN", 70, 45, 33, ('32x32', 1, 1, 1, 33, 0, 1, 0)),
    C("f64_NN_70x45x37_ksweep", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0)),
    C("f64_NN_70x45x127_ksweep", "f64", "NN", 70, 45, 127, ('32x32', 1, 1, 1, 127, 0, 1, 0)),
    C("f64_NN_70x45x128_ksweep", "f64", "NN", 70, 45, 128, ('32x32', 1, 1, 1, 128, 0, 1, 0)),
    C("f64_NN_70x45x129_ksweep", "f64", "NN", 70, 45, 129, ('32x32', 1, 1, 1, 129, 0, 1, 0)),
    C("f64_NN_70x45x200_ksweep", "f64", "NN", 70, 45, 200, ('32x32', 1, 1, 1, 200, 0, 1, 0)),
    C("f64_NN_70x45x511_ksweep", "f64", "NN", 70, 45, 511, ('32x32', 1, 1, 1, 511, 0, 1, 0)),
    C("f64_NN_70x45x512_ksweep", "f64", "NN", 70, 45, 512, ('32x32', 1, 1, 2, 256, 1, 1, 0)),
    C("f64_NN_70x45x513_ksweep", "f64", "NN", 70, 45, 513, ('32x32', 1, 1, 2, 288, 1, 1, 0)),
    C("f64_NN_70x45x1023_ksweep", "f64", "NN", 70, 45, 1023, ('32x32', 1, 1, 3, 352, 1, 1, 0)),
    C("f64_NN_70x45x1024_ksweep", "f64", "NN", 70, 45, 1024, ('32x32', 1, 1, 4, 256, 1, 1, 0)),
    C("f64_NN_70x45x1025_ksweep", "f64", "NN", 70, 45, 1025, ('32x32', 1, 1, 4, 288, 1, 1, 0)),
    C("f64_NN_70x45x4095_ksweep", "f64", "NN", 70, 45, 4095, ('32x32', 1, 1, 15, 288, 1, 1, 0)),
    C("f64_NN_70x45x4097_ksweep", "f64", "NN", 70, 45, 4097, ('32x32', 1, 1, 15, 288, 1, 1, 0)),
    C("c64_NN_70x45x1_ksweep", "c64", "NN", 70, 45, 1, ('32x32', 1, 1, 1, 1, 0, 1, 0)),
    C("c64_NN_70x45x3_ksweep", "c64", "NN", 70, 45, 3, ('32x32', 1, 1, 1, 3, 0, 1, 0)),
    C("c64_NN_70x45x15_ksweep", "c64", "NN", 70, 45, 15, ('32x32', 1, 1, 1, 15, 0, 1, 0)),
    C("c64_NN_70x45x16_ksweep", "c64", "NN", 70, 45, 16, ('32x32', 1, 1, 1, 16, 0, 1, 0)),
    C("c64_NN_70x45x17_ksweep", "c64", "NN", 70, 45, 17, ('32x32', 1, 1, 1, 17, 0, 1, 0)),
    C("c64_NN_70x45x31_ksweep", "c64", "NN", 70, 45, 31, ('32x32', 1, 1, 1, 31, 0, 1, 0)),
    C("c64_NN_70x45x32_ksweep", "c64", "NN", 70, 45, 32, ('32x32', 1, 1, 1, 32, 0, 1, 0)),
    C("c64_NN_70x45x33_ksweep", "c64", "NN", 70, 45, 33, ('32x32', 1, 1, 1, 33, 0, 1, 0)),
    C("c64_NN_70x45x37_ksweep", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0)),
    C("c64_NN_70x45x127_ksweep", "c64", "NN", 70, 45, 127, ('32x32', 1, 1, 1, 127, 0, 1, 0)),
    C("c64_NN_70x45x128_ksweep", "c64", "NN", 70, 45, 128, ('32x32', 1, 1, 1, 128, 0, 1, 0)),
    C("c64_NN_70x45x129_ksweep", "c64", "NN", 70, 45, 129, ('32x32', 1, 1, 1, 129, 0, 1, 0)),
    C("c64_NN_70x45x200_ksweep", "c64", "NN", 70, 45, 200, ('32x32', 1, 1, 1, 200, 0, 1, 0)),
    C("c64_NN_70x45x511_ksweep", "c64", "NN", 70, 45, 511, ('32x32', 1, 1, 1, 511, 0, 1, 0)),
    C("c64_NN_70x45x512_ksweep", "c64", "NN", 70, 45, 512, ('32x32', 1, 1, 2, 256, 1, 1, 0)),
    C("c64_NN_70x45x513_ksweep", "c64", "NN", 70, 45, 513, ('32x32', 1, 1, 2, 288, 1, 1, 0)),
    C("c64_NN_70x45x1023_ksweep", "c64", "NN", 70, 45, 1023, ('32x32', 1, 1, 3, 352, 1, 1, 0)),
    C("c64_NN_70x45x1024_ksweep", "c64", "NN", 70, 45, 1024, ('32x32', 1, 1, 4, 256, 1, 1, 0)),
    C("c64_NN_70x45x1025_ksweep", "c64", "NN", 70, 45, 1025, ('32x32', 1, 1, 4, 288, 1, 1, 0)),
    C("c64_NN_70x45x4095_ksweep", "c64", "NN", 70, 45, 4095, ('32x32', 1, 1, 15, 288, 1, 1, 0)),
    C("c64_NN_70x45x4097_ksweep", "c64", "NN", 70, 45, 4097, ('32x32', 1, 1, 15, 288, 1, 1, 0)),
    C("c64_NN_5x3x1_ksweep", "c64", "NN", 5, 3, 1, ('64x64', 1, 1, 1, 1, 0, 1, 0)),
    C("c64_NN_5x3x3_ksweep", "c64", "NN", 5, 3, 3, ('64x64', 1, 1, 1, 3, 0, 1, 0)),
    C("c64_NN_5x3x15_ksweep", "c64", "NN", 5, 3, 15, ('64x64', 1, 1, 1, 15, 0, 1, 0)),
    C("c64_NN_5x3x16_ksweep", "c64", "NN", 5, 3, 16, ('64x64', 1, 1, 1, 16, 0, 1, 0)),
    C("c64_NN_5x3x17_ksweep", "c64", "NN", 5, 3, 17, ('64x64', 1, 1, 1, 17, 0, 1, 0)),
    C("c64_NN_5x3x31_ksweep", "c64", "NN", 5, 3, 31, ('64x64', 1, 1, 1, 31, 0, 1, 0)),
    C("c64_NN_5x3x32_ksweep", "c64", "NN", 5, 3, 32, ('64x64', 1, 1, 1, 32, 0, 1, 0)),
    C("c64_NN_5x3x33_ksweep", "c64", "NN", 5, 3, 33, ('64x64', 1, 1, 1, 33, 0, 1, 0)),
    C("c64_NN_5x3x37_ksweep", "c64", "NN", 5, 3, 37, ('64x64', 1, 1, 1, 37, 0, 1, 0)),
    C("c64_NN_5x3x127_ksweep", "c64", "NN", 5, 3, 127, ('64x64', 1, 1, 1, 127, 0, 1, 0)),
    C("c64_NN_5x3x128_ksweep", "c64", "NN", 5, 3, 128, ('64x64', 1, 1, 2, 64, 2, 1, 0)),
    C("c64_NN_5x3x129_ksweep", "c64", "NN", 5, 3, 129, ('64x64', 1, 1, 2, 80, 2, 1, 0)),
    C("c64_NN_5x3x200_ksweep", "c64", "NN", 5, 3, 200, ('64x64', 1, 1, 3, 80, 2, 1, 0)),
    C("c64_NN_5x3x511_ksweep", "c64", "NN", 5, 3, 511, ('64x64', 1, 1, 7, 80, 2, 1, 0)),
    C("c64_NN_5x3x512_ksweep", "c64", "NN", 5, 3, 512, ('64x64', 1, 1, 8, 64, 2, 1, 0)),
    C("c64_NN_5x3x513_ksweep", "c64", "NN", 5, 3, 513, ('64x64', 1, 1, 7, 80, 2, 1, 0)),
    C("c64_NN_5x3x1023_ksweep", "c64", "NN", 5, 3, 1023, ('64x64', 1, 1, 13, 80, 2, 1, 0)),
    C("c64_NN_5x3x1024_ksweep", "c64", "NN", 5, 3, 1024, ('64x64', 1, 1, 16, 64, 2, 1, 0)),
    C("c64_NN_5x3x1025_ksweep", "c64", "NN", 5, 3, 1025, ('64x64', 1, 1, 13, 80, 2, 1, 0)),
    C("c64_NN_5x3x4095_ksweep", "c64", "NN", 5, 3, 4095, ('64x64', 1, 1, 32, 128, 2, 1, 0)),
    C("c64_NN_5x3x4097_ksweep", "c64", "NN", 5, 3, 4097, ('64x64', 1, 1, 29, 144, 2, 1, 0)),
    C("f64_NN_200x30x1_ksweep", "f64", "NN", 200, 30, 1, ('64x64', 1, 1, 1, 1, 0, 1, 0)),
    C("f64_NN_200x30x3_ksweep", "f64", "NN", 200, 30, 3, ('64x64', 1, 1, 1, 3, 0, 1, 0)),
    C("f64_NN_200x30x15_ksweep", "f64", "NN", 200, 30, 15, ('64x64', 1, 1, 1, 15, 0, 1, 0)),
    C("f64_NN_200x30x16_ksweep", "f64", "NN", 200, 30, 16, ('64x64', 1, 1, 1, 16, 0, 1, 0)),
    C("f64_NN_200x30x17_ksweep", "f64", "NN", 200, 30, 17, ('64x64', 1, 1, 1, 17, 0, 1, 0)),
    C("f64_NN_200x30x31_ksweep", "f64", "NN", 200, 30, 31, ('64x64', 1, 1, 1, 31, 0, 1, 0)),
    C("f64_NN_200x30x32_ksweep", "f64", "NN", 200, 30, 32, ('64x64', 1, 1, 1, 32, 0, 1, 0)),
    C("f64_NN_200x30x33_ksweep", "f64", "NN", 200, 30, 33, ('64x64', 1, 1, 1, 33, 0, 1, 0)),
    C("f64_NN_200x30x37_ksweep", "f64", "NN", 200, 30, 37, ('64x64', 1, 1, 1, 37, 0, 1, 0)),
    C("f64_NN_200x30x127_ksweep", "f64", "NN", 200, 30, 127, ('64x64', 1, 1, 1, 127, 0, 1, 0)),
    C("f64_NN_200x30x128_ksweep", "f64", "NN", 200, 30, 128, ('64x64', 1, 1, 2, 64, 2, 1, 0)),
    C("f64_NN_200x30x129_ksweep", "f64", "NN", 200, 30, 129, ('64x64', 1, 1, 2, 80, 2, 1, 0)),
    C("f64_NN_200x30x200_ksweep", "f64", "NN", 200, 30, 200, ('64x64', 1, 1, 3, 80, 2, 1, 0)),
    C("f64_NN_200x30x511_ksweep", "f64", "NN", 200, 30, 511, ('64x64', 1, 1, 7, 80, 2, 1, 0)),
    C("f64_NN_200x30x512_ksweep", "f64", "NN", 200, 30, 512, ('64x64', 1, 1, 8, 64, 2, 1, 0)),
    C("f64_NN_200x30x513_ksweep", "f64", "NN", 200, 30, 513, ('64x64', 1, 1, 7, 80, 2, 1, 0)),
    C("f64_NN_200x30x1023_ksweep", "f64", "NN", 200, 30, 1023, ('64x64', 1, 1, 13, 80, 2, 1, 0)),
    C("f64_NN_200x30x1024_ksweep", "f64", "NN", 200, 30, 1024, ('64x64', 1, 1, 16, 64, 2, 1, 0)),
    C("f64_NN_200x30x1025_ksweep", "f64", "NN", 200, 30, 1025, ('64x64', 1, 1, 13, 80, 2, 1, 0)),
    C("f64_NN_200x30x4095_ksweep", "f64", "NN", 200, 30, 4095, ('64x64', 1, 1, 32, 128, 2, 1, 0)),
    C("f64_NN_200x30x4097_ksweep", "f64", "NN", 200, 30, 4097, ('64x64', 1, 1, 29, 144, 2, 1, 0)),
    C("c64_NN_17x200x1_ksweep", "c64", "NN", 17, 200, 1, ('32x64D', 1, 1, 1, 1, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x3_ksweep", "c64", "NN", 17, 200, 3, ('32x64D', 1, 1, 1, 3, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x15_ksweep", "c64", "NN", 17, 200, 15, ('32x64D', 1, 1, 1, 15, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x16_ksweep", "c64", "NN", 17, 200, 16, ('32x64D', 1, 1, 1, 16, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x17_ksweep", "c64", "NN", 17, 200, 17, ('32x64D', 1, 1, 1, 17, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x31_ksweep", "c64", "NN", 17, 200, 31, ('32x64D', 1, 1, 1, 31, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x32_ksweep", "c64", "NN", 17, 200, 32, ('32x64D', 1, 1, 1, 32, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x33_ksweep", "c64", "NN", 17, 200, 33, ('32x64D', 1, 1, 1, 33, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x37_ksweep", "c64", "NN", 17, 200, 37, ('32x64D', 1, 1, 1, 37, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x127_ksweep", "c64", "NN", 17, 200, 127, ('32x64D', 1, 1, 1, 127, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x128_ksweep", "c64", "NN", 17, 200, 128, ('32x64D', 1, 1, 2, 64, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x129_ksweep", "c64", "NN", 17, 200, 129, ('32x64D', 1, 1, 2, 80, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x200_ksweep", "c64", "NN", 17, 200, 200, ('32x64D', 1, 1, 3, 80, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x511_ksweep", "c64", "NN", 17, 200, 511, ('32x64D', 1, 1, 7, 80, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x512_ksweep", "c64", "NN", 17, 200, 512, ('32x64D', 1, 1, 8, 64, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x513_ksweep", "c64", "NN", 17, 200, 513, ('32x64D', 1, 1, 7, 80, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x1023_ksweep", "c64", "NN", 17, 200, 1023, ('32x64D', 1, 1, 13, 80, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x1024_ksweep", "c64", "NN", 17, 200, 1024, ('32x64D', 1, 1, 16, 64, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x1025_ksweep", "c64", "NN", 17, 200, 1025, ('32x64D', 1, 1, 13, 80, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x4095_ksweep", "c64", "NN", 17, 200, 4095, ('32x64D', 1, 1, 32, 128, 2, 1, 0), skinny=True),
    C("c64_NN_17x200x4097_ksweep", "c64", "NN", 17, 200, 4097, ('32x64D', 1, 1, 29, 144, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x1_ksweep", "f64", "NN", 40, 128, 1, ('48x64D', 1, 1, 1, 1, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x3_ksweep", "f64", "NN", 40, 128, 3, ('48x64D', 1, 1, 1, 3, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x15_ksweep", "f64", "NN", 40, 128, 15, ('48x64D', 1, 1, 1, 15, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x16_ksweep", "f64", "NN", 40, 128, 16, ('48x64D', 1, 1, 1, 16, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x17_ksweep", "f64", "NN", 40, 128, 17, ('48x64D', 1, 1, 1, 17, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x31_ksweep", "f64", "NN", 40, 128, 31, ('48x64D', 1, 1, 1, 31, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x32_ksweep", "f64", "NN", 40, 128, 32, ('48x64D', 1, 1, 1, 32, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x33_ksweep", "f64", "NN", 40, 128, 33, ('48x64D', 1, 1, 1, 33, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x37_ksweep", "f64", "NN", 40, 128, 37, ('48x64D', 1, 1, 1, 37, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x127_ksweep", "f64", "NN", 40, 128, 127, ('48x64D', 1, 1, 1, 127, 0, 1, 0), skinny=True),
    C("f64_NN_40x128x128_ksweep", "f64", "NN", 40, 128, 128, ('48x64D', 1, 1, 2, 64, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x129_ksweep", "f64", "NN", 40, 128, 129, ('48x64D', 1, 1, 2, 80, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x200_ksweep", "f64", "NN", 40, 128, 200, ('48x64D', 1, 1, 3, 80, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x511_ksweep", "f64", "NN", 40, 128, 511, ('48x64D', 1, 1, 7, 80, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x512_ksweep", "f64", "NN", 40, 128, 512, ('48x64D', 1, 1, 8, 64, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x513_ksweep", "f64", "NN", 40, 128, 513, ('48x64D', 1, 1, 7, 80, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x1023_ksweep", "f64", "NN", 40, 128, 1023, ('48x64D', 1, 1, 13, 80, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x1024_ksweep", "f64", "NN", 40, 128, 1024, ('48x64D', 1, 1, 16, 64, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x1025_ksweep", "f64", "NN", 40, 128, 1025, ('48x64D', 1, 1, 13, 80, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x4095_ksweep", "f64", "NN", 40, 128, 4095, ('48x64D', 1, 1, 32, 128, 2, 1, 0), skinny=True),
    C("f64_NN_40x128x4097_ksweep", "f64", "NN", 40, 128, 4097, ('48x64D', 1, 1, 29, 144, 2, 1, 0), skinny=True),
    # staging patterns: every tile shape x (ARC, BKC), padded leading dimensions and odd element offsets
    C("f64_NN_130x129x67_staging", "f64", "NN", 130, 129, 67, ('32x32', 1, 1, 1, 67, 0, 1, 0), pad=(0, 0, 0), off=(1, 3, 5)),
    C("f64_NT_130x129x67_staging", "f64", "NT", 130, 129, 67, ('32x32', 1, 0, 1, 67, 0, 1, 0), pad=(3, 5, 1), off=(3, 1, 7)),
    C("f64_TN_130x129x67_staging", "f64", "TN", 130, 129, 67, ('32x32', 0, 1, 1, 67, 0, 1, 0), pad=(1, 7, 7), off=(5, 5, 1)),
    C("f64_TT_130x129x67_staging", "f64", "TT", 130, 129, 67, ('32x32', 0, 0, 1, 67, 0, 1, 0), pad=(7, 1, 0), off=(7, 9, 3)),
    C("f64_NN_200x30x37_staging", "f64", "NN", 200, 30, 37, ('64x64', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 0), off=(1, 3, 5)),
    C("f64_NT_200x30x37_staging", "f64", "NT", 200, 30, 37, ('64x64', 1, 0, 1, 37, 0, 1, 0), pad=(3, 5, 1), off=(3, 1, 7)),
    C("f64_TN_200x30x37_staging", "f64", "TN", 200, 30, 37, ('64x64', 0, 1, 1, 37, 0, 1, 0), pad=(1, 7, 7), off=(5, 5, 1)),
    C("f64_TT_200x30x37_staging", "f64", "TT", 200, 30, 37, ('64x64', 0, 0, 1, 37, 0, 1, 0), pad=(7, 1, 0), off=(7, 9, 3)),
    C("f64_NN_700x700x33_staging", "f64", "NN", 700, 700, 33, ('64x64', 1, 1, 1, 33, 0, 0, 0), pad=(0, 0, 0), off=(1, 3, 5)),
    C("f64_NT_700x700x33_staging", "f64", "NT", 700, 700, 33, ('64x64', 1, 0, 1, 33, 0, 0, 0), pad=(3, 5, 1), off=(3, 1, 7)),
    C("f64_TN_700x700x33_staging", "f64", "TN", 700, 700, 33, ('64x64', 0, 1, 1, 33, 0, 0, 0), pad=(1, 7, 7), off=(5, 5, 1)),
    C("f64_TT_700x700x33_staging", "f64", "TT", 700, 700, 33, ('64x64', 0, 0, 1, 33, 0, 0, 0), pad=(7, 1, 0), off=(7, 9, 3)),
    C("f64_NN_1400x133x129_staging", "f64", "NN", 1400, 133, 129, ('64x144', 1, 1, 1, 129, 0, 1, 0), pad=(0, 0, 0), off=(1, 3, 5)),
    C("f64_NT_1400x133x129_staging", "f64", "NT", 1400, 133, 129, ('64x144', 1, 0, 1, 129, 0, 1, 0), pad=(3, 5, 1), off=(3, 1, 7)),
    C("f64_TN_1400x133x129_staging", "f64", "TN", 1400, 133, 129, ('64x144', 0, 1, 1, 129, 0, 1, 0), pad=(1, 7, 7), off=(5, 5, 1)),
    C("f64_TT_1400x133x129_staging", "f64", "TT", 1400, 133, 129, ('64x144', 0, 0, 1, 129, 0, 1, 0), pad=(7, 1, 0), off=(7, 9, 3)),
    C("f64_NN_1100x900x37_staging", "f64", "NN", 1100, 900, 37, ('128x64', 1, 1, 1, 37, 0, 0, 0), pad=(0, 0, 0), off=(1, 3, 5)),
    C("f64_NT_1100x900x37_staging", "f64", "NT", 1100, 900, 37, ('128x64', 1, 0, 1, 37, 0, 0, 0), pad=(3, 5, 1), off=(3, 1, 7)),
    C("f64_TN_1100x900x37_staging", "f64", "TN", 1100, 900, 37, ('128x64', 0, 1, 1, 37, 0, 0, 0), pad=(1, 7, 7), off=(5, 5, 1)),
    C("f64_TT_1100x900x37_staging", "f64", "TT", 1100, 900, 37, ('128x64', 0, 0, 1, 37, 0, 0, 0), pad=(7, 1, 0), off=(7, 9, 3)),
    C("f64_NN_2817x2900x17_staging", "f64", "NN", 2817, 2900, 17, ('128x128', 1, 1, 1, 17, 0, 0, 0), pad=(0, 0, 0), off=(1, 3, 5)),
    C("f64_NT_2817x2900x17_staging", "f64", "NT", 2817, 2900, 17, ('128x128', 1, 0, 1, 17, 0, 0, 0), pad=(3, 5, 1), off=(3, 1, 7)),
    C("f64_TN_2817x2900x17_staging", "f64", "TN", 2817, 2900, 17, ('128x128', 0, 1, 1, 17, 0, 0, 0), pad=(1, 7, 7), off=(5, 5, 1)),
    C("f64_TT_2817x2900x17_staging", "f64", "TT", 2817, 2900, 17, ('128x128', 0, 0, 1, 17, 0, 0, 0), pad=(7, 1, 0), off=(7, 9, 3)),
    C("f64_NN_17x200x100_staging", "f64", "NN", 17, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), pad=(0, 0, 0), off=(1, 3, 5), skinny=True),
    C("f64_NT_17x200x100_staging", "f64", "NT", 17, 200, 100, ('32x64D', 1, 0, 1, 100, 0, 1, 0), pad=(3, 5, 1), off=(3, 1, 7), skinny=True),
    C("f64_TN_17x200x100_staging", "f64", "TN", 17, 200, 100, ('32x64D', 0, 1, 1, 100, 0, 1, 0), pad=(1, 7, 7), off=(5, 5, 1), skinny=True),
    C("f64_TT_17x200x100_staging", "f64", "TT", 17, 200, 100, ('32x64D', 0, 0, 1, 100, 0, 1, 0), pad=(7, 1, 0), off=(7, 9, 3), skinny=True),
    C("f64_NN_40x200x100_staging", "f64", "NN", 40, 200, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), pad=(0, 0, 0), off=(1, 3, 5), skinny=True),
    C("f64_NT_40x200x100_staging", "f64", "NT", 40, 200, 100, ('48x64D', 1, 0, 1, 100, 0, 1, 0), pad=(3, 5, 1), off=(3, 1, 7), skinny=True),
    C("f64_TN_40x200x100_staging", "f64", "TN", 40, 200, 100, ('48x64D', 0, 1, 1, 100, 0, 1, 0), pad=(1, 7, 7), off=(5, 5, 1), skinny=True),
    C("f64_TT_40x200x100_staging", "f64", "TT", 40, 200, 100, ('48x64D', 0, 0, 1, 100, 0, 1, 0), pad=(7, 1, 0), off=(7, 9, 3), skinny=True),
    C("c64_NN_130x129x67_staging", "c64", "NN", 130, 129, 67, ('32x32', 1, 1, 1, 67, 0, 1, 0), pad=(0, 0, 0), off=(1, 3, 5)),
    C("c64_NH_130x129x67_staging", "c64", "NH", 130, 129, 67, ('32x32', 1, 0, 1, 67, 0, 1, 0), pad=(3, 5, 1), off=(3, 1, 7)),
    C("c64_HN_130x129x67_staging", "c64", "HN", 130, 129, 67, ('32x32', 0, 1, 1, 67, 0, 1, 0), pad=(1, 7, 7), off=(5, 5, 1)),
    C("c64_HH_130x129x67_staging", "c64", "HH", 130, 129, 67, ('32x32', 0, 0, 1, 67, 0, 1, 0), pad=(7, 1, 0), off=(7, 9, 3)),
    C("c64_NN_520x520x37_staging", "c64", "NN", 520, 520, 37, ('64x64', 1, 1, 1, 37, 0, 0, 0), pad=(0, 0, 0), off=(1, 3, 5)),
    C("c64_NH_520x520x37_staging", "c64", "NH", 520, 520, 37, ('64x64', 1, 0, 1, 37, 0, 0, 0), pad=(3, 5, 1), off=(3, 1, 7)),
    C("c64_HN_520x520x37_staging", "c64", "HN", 520, 520, 37, ('64x64', 0, 1, 1, 37, 0, 0, 0), pad=(1, 7, 7), off=(5, 5, 1)),
    C("c64_HH_520x520x37_staging", "c64", "HH", 520, 520, 37, ('64x64', 0, 0, 1, 37, 0, 0, 0), pad=(7, 1, 0), off=(7, 9, 3)),
    C("c64_NN_32x200x100_staging", "c64", "NN", 32, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), pad=(0, 0, 0), off=(1, 3, 5), skinny=True),
    C("c64_NH_32x200x100_staging", "c64", "NH", 32, 200, 100, ('32x64D', 1, 0, 1, 100, 0, 1, 0), pad=(3, 5, 1), off=(3, 1, 7), skinny=True),
    C("c64_HN_32x200x100_staging", "c64", "HN", 32, 200, 100, ('32x64D', 0, 1, 1, 100, 0, 1, 0), pad=(1, 7, 7), off=(5, 5, 1), skinny=True),
    C("c64_HH_32x200x100_staging", "c64", "HH", 32, 200, 100, ('32x64D', 0, 0, 1, 100, 0, 1, 0), pad=(7, 1, 0), off=(7, 9, 3), skinny=True),
    C("c64_NN_33x130x100_staging", "c64", "NN", 33, 130, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), pad=(0, 0, 0), off=(1, 3, 5), skinny=True),
    C("c64_NH_33x130x100_staging", "c64", "NH", 33, 130, 100, ('48x64D', 1, 0, 1, 100, 0, 1, 0), pad=(3, 5, 1), off=(3, 1, 7), skinny=True),
    C("c64_HN_33x130x100_staging", "c64", "HN", 33, 130, 100, ('48x64D', 0, 1, 1, 100, 0, 1, 0), pad=(1, 7, 7), off=(5, 5, 1), skinny=True),
    C("c64_HH_33x130x100_staging", "c64", "HH", 33, 130, 100, ('48x64D', 0, 0, 1, 100, 0, 1, 0), pad=(7, 1, 0), off=(7, 9, 3), skinny=True),
    C("c64_CN_70x45x37_conj", "c64", "CN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    C("c64_NC_70x45x37_conj", "c64", "NC", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    C("c64_TC_70x45x37_conj", "c64", "TC", 70, 45, 37, ('32x32', 0, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    C("c64_CT_70x45x37_conj", "c64", "CT", 70, 45, 37, ('32x32', 1, 0, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    C("c64_HT_70x45x37_conj", "c64", "HT", 70, 45, 37, ('32x32', 0, 0, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    C("c64_TH_70x45x37_conj", "c64", "TH", 70, 45, 37, ('32x32', 0, 0, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    C("c64_CC_70x45x37_conj", "c64", "CC", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    C("f64_HN_70x45x37_realops", "f64", "HN", 70, 45, 37, ('32x32', 0, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    C("f64_CH_70x45x37_realops", "f64", "CH", 70, 45, 37, ('32x32', 1, 0, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 1, 1)),
    # the shapes the dispatch rules were read off
    C("c64_NN_520x520x129_shape", "c64", "NN", 520, 520, 129, ('64x64', 1, 1, 1, 129, 0, 0, 0)),
    C("c64_NN_576x512x129_shape", "c64", "NN", 576, 512, 129, ('64x64', 1, 1, 1, 129, 0, 1, 1)),
    C("f64_NN_700x700x129_shape", "f64", "NN", 700, 700, 129, ('64x64', 1, 1, 1, 129, 0, 0, 0)),
    C("f64_NN_704x512x129_shape", "f64", "NN", 704, 512, 129, ('64x64', 1, 1, 1, 129, 0, 1, 1)),
    C("f64_NN_1400x133x129_shape", "f64", "NN", 1400, 133, 129, ('64x144', 1, 1, 1, 129, 0, 1, 0)),
    C("f64_NN_2100x97x129_shape", "f64", "NN", 2100, 97, 129, ('64x144', 1, 1, 1, 129, 0, 1, 0)),
    C("f64_NN_1400x144x129_shape", "f64", "NN", 1400, 144, 129, ('64x144', 1, 1, 1, 129, 0, 1, 0)),
    C("f64_NN_1400x145x129_shape", "f64", "NN", 1400, 145, 129, ('64x64', 1, 1, 1, 129, 0, 1, 0)),
    C("f64_NN_1400x96x129_shape", "f64", "NN", 1400, 96, 129, ('32x32', 1, 1, 1, 129, 0, 1, 0)),
    C("f64_NN_255x133x129_shape", "f64", "NN", 255, 133, 129, ('32x32', 1, 1, 1, 129, 0, 1, 0)),
    C("f64_NN_1100x900x129_shape", "f64", "NN", 1100, 900, 129, ('128x64', 1, 1, 1, 129, 0, 0, 0)),
    C("f64_NN_1024x1024x129_shape", "f64", "NN", 1024, 1024, 129, ('128x64', 1, 1, 1, 129, 0, 0, 1)),
    C("f64_NN_4096x133x129_shape", "f64", "NN", 4096, 133, 129, ('64x144', 1, 1, 1, 129, 0, 1, 1)),
    C("f64_NN_4160x133x129_shape", "f64", "NN", 4160, 133, 129, ('64x144', 1, 1, 1, 129, 0, 1, 0)),
    C("f64_NN_2880x2880x33_shape", "f64", "NN", 2880, 2880, 33, ('128x128', 1, 1, 1, 33, 0, 0, 0)),
    C("f64_NN_2944x3072x33_shape", "f64", "NN", 2944, 3072, 33, ('128x128', 1, 1, 1, 33, 0, 0, 1)),
    C("f64_NN_256x256x37_shape", "f64", "NN", 256, 256, 37, ('32x32', 1, 1, 1, 37, 0, 1, 1)),
    C("f64_NN_288x288x37_shape", "f64", "NN", 288, 288, 37, ('32x32', 1, 1, 1, 37, 0, 0, 0)),
    C("f64_NN_1x128x100_skinny", "f64", "NN", 1, 128, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_1x200x100_skinny", "f64", "NN", 1, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_1x8192x129_skinny", "f64", "NN", 1, 8192, 129, ('32x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("f64_NN_17x128x100_skinny", "f64", "NN", 17, 128, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_17x200x100_skinny", "f64", "NN", 17, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_17x8192x129_skinny", "f64", "NN", 17, 8192, 129, ('32x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("f64_NN_32x128x100_skinny", "f64", "NN", 32, 128, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_32x200x100_skinny", "f64", "NN", 32, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_32x8192x129_skinny", "f64", "NN", 32, 8192, 129, ('32x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("f64_NN_33x128x100_skinny", "f64", "NN", 33, 128, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_33x200x100_skinny", "f64", "NN", 33, 200, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_33x8192x129_skinny", "f64", "NN", 33, 8192, 129, ('48x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("f64_NN_40x128x100_skinny", "f64", "NN", 40, 128, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_40x200x100_skinny", "f64", "NN", 40, 200, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_40x8192x129_skinny", "f64", "NN", 40, 8192, 129, ('48x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("f64_NN_48x128x100_skinny", "f64", "NN", 48, 128, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_48x200x100_skinny", "f64", "NN", 48, 200, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_48x8192x129_skinny", "f64", "NN", 48, 8192, 129, ('48x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("f64_NN_32x4160x100_skinny_off", "f64", "NN", 32, 4160, 100, ('32x64D', 1, 1, 1, 100, 0, 0, 0), skinny=True),
    C("f64_NN_49x200x100_hint_not_honoured", "f64", "NN", 49, 200, 100, ('32x32', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_32x127x100_hint_not_honoured", "f64", "NN", 32, 127, 100, ('32x32', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("f64_NN_32x200x100_no_hint", "f64", "NN", 32, 200, 100, ('32x32', 1, 1, 1, 100, 0, 1, 0)),
    C("c64_NN_256x256x37_shape", "c64", "NN", 256, 256, 37, ('32x32', 1, 1, 1, 37, 0, 1, 1)),
    C("c64_NN_288x288x37_shape", "c64", "NN", 288, 288, 37, ('32x32', 1, 1, 1, 37, 0, 0, 0)),
    C("c64_NN_1x128x100_skinny", "c64", "NN", 1, 128, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_1x200x100_skinny", "c64", "NN", 1, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_1x8192x129_skinny", "c64", "NN", 1, 8192, 129, ('32x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("c64_NN_17x128x100_skinny", "c64", "NN", 17, 128, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x100_skinny", "c64", "NN", 17, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_17x8192x129_skinny", "c64", "NN", 17, 8192, 129, ('32x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("c64_NN_32x128x100_skinny", "c64", "NN", 32, 128, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_32x200x100_skinny", "c64", "NN", 32, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_32x8192x129_skinny", "c64", "NN", 32, 8192, 129, ('32x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("c64_NN_33x128x100_skinny", "c64", "NN", 33, 128, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_33x200x100_skinny", "c64", "NN", 33, 200, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_33x8192x129_skinny", "c64", "NN", 33, 8192, 129, ('48x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("c64_NN_40x128x100_skinny", "c64", "NN", 40, 128, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_40x200x100_skinny", "c64", "NN", 40, 200, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_40x8192x129_skinny", "c64", "NN", 40, 8192, 129, ('48x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("c64_NN_48x128x100_skinny", "c64", "NN", 48, 128, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_48x200x100_skinny", "c64", "NN", 48, 200, 100, ('48x64D', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_48x8192x129_skinny", "c64", "NN", 48, 8192, 129, ('48x64D', 1, 1, 1, 129, 0, 0, 1), skinny=True),
    C("c64_NN_32x4160x100_skinny_off", "c64", "NN", 32, 4160, 100, ('32x64D', 1, 1, 1, 100, 0, 0, 0), skinny=True),
    C("c64_NN_49x200x100_hint_not_honoured", "c64", "NN", 49, 200, 100, ('32x32', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_32x127x100_hint_not_honoured", "c64", "NN", 32, 127, 100, ('32x32', 1, 1, 1, 100, 0, 1, 0), skinny=True),
    C("c64_NN_32x200x100_no_hint", "c64", "NN", 32, 200, 100, ('32x32', 1, 1, 1, 100, 0, 1, 0)),
    # split-K: each rule on each shape it can reach, slice rounding, short last slices
    C("f64_NN_64x64x257_rule2_rounding_drops_a_slice", "f64", "NN", 64, 64, 257, ('32x32', 1, 1, 3, 96, 2, 1, 0)),
    C("c64_HN_64x64x257_rule2_rounding_drops_a_slice", "c64", "HN", 64, 64, 257, ('32x32', 0, 1, 3, 96, 2, 1, 0), pad=(3, 3, 0), off=(1, 1, 1)),
    C("f64_TN_130x129x1025_rule1", "f64", "TN", 130, 129, 1025, ('32x32', 0, 1, 4, 288, 1, 1, 0), pad=(1, 1, 0)),
    C("c64_HN_130x129x1025_rule1", "c64", "HN", 130, 129, 1025, ('32x32', 0, 1, 4, 288, 1, 1, 0)),
    C("c64_HN_64x128x513_rule1_k512_8tiles", "c64", "HN", 64, 128, 513, ('32x32', 0, 1, 2, 288, 1, 1, 0)),
    C("f64_NN_512x512x4097_rule3", "f64", "NN", 512, 512, 4097, ('32x32', 1, 1, 2, 2080, 3, 0, 1)),
    C("c64_NN_520x520x1024_rule1", "c64", "NN", 520, 520, 1024, ('64x64', 1, 1, 4, 256, 1, 0, 0)),
    C("c64_NH_768x768x4096_rule3", "c64", "NH", 768, 768, 4096, ('64x64', 1, 0, 4, 1024, 3, 0, 1)),
    C("f64_NN_700x700x1025_rule1", "f64", "NN", 700, 700, 1025, ('64x64', 1, 1, 4, 272, 1, 0, 0)),
    C("f64_TN_320x1900x4097_rule3", "f64", "TN", 320, 1900, 4097, ('64x64', 0, 1, 4, 1040, 3, 0, 0)),
    C("f64_TN_1400x133x1025_rule1", "f64", "TN", 1400, 133, 1025, ('64x144', 0, 1, 4, 272, 1, 1, 0)),
    C("f64_TN_8192x133x4096_rule3", "f64", "TN", 8192, 133, 4096, ('64x144', 0, 1, 4, 1024, 3, 1, 1)),
    C("f64_NN_1100x900x4097_rule3", "f64", "NN", 1100, 900, 4097, ('128x64', 1, 1, 4, 1040, 3, 0, 0)),
    C("f64_NN_32x4160x1025_rule1", "f64", "NN", 32, 4160, 1025, ('32x64D', 1, 1, 4, 272, 1, 0, 0), skinny=True),
    C("f64_NN_48x4160x1025_rule1", "f64", "NN", 48, 4160, 1025, ('48x64D', 1, 1, 4, 272, 1, 0, 0), skinny=True),
    C("f64_NN_33x200x1023_rule2", "f64", "NN", 33, 200, 1023, ('48x64D', 1, 1, 13, 80, 2, 1, 0), skinny=True),
    C("c64_NN_32x4160x1025_rule1", "c64", "NN", 32, 4160, 1025, ('32x64D', 1, 1, 4, 272, 1, 0, 0), skinny=True),
    C("c64_NN_48x4160x1025_rule1", "c64", "NN", 48, 4160, 1025, ('48x64D', 1, 1, 4, 272, 1, 0, 0), skinny=True),
    C("c64_NN_33x200x1023_rule2", "c64", "NN", 33, 200, 1023, ('48x64D', 1, 1, 13, 80, 2, 1, 0), skinny=True),
    C("f64_NN_32x8192x4097_rule3", "f64", "NN", 32, 8192, 4097, ('32x64D', 1, 1, 4, 1040, 3, 0, 1), skinny=True),
    C("f64_NN_48x8192x4097_rule3", "f64", "NN", 48, 8192, 4097, ('48x64D', 1, 1, 4, 1040, 3, 0, 1), skinny=True),
    # two K tiles in flight: K-tile counts 1 to 4 and a large odd one
    C("f64_NN_17x200x16_deep_ktiles", "f64", "NN", 17, 200, 16, ('32x64D', 1, 1, 1, 16, 0, 1, 0), skinny=True),
    C("f64_NN_17x200x32_deep_ktiles", "f64", "NN", 17, 200, 32, ('32x64D', 1, 1, 1, 32, 0, 1, 0), skinny=True),
    C("f64_NN_17x200x48_deep_ktiles", "f64", "NN", 17, 200, 48, ('32x64D', 1, 1, 1, 48, 0, 1, 0), skinny=True),
    C("f64_NN_17x200x64_deep_ktiles", "f64", "NN", 17, 200, 64, ('32x64D', 1, 1, 1, 64, 0, 1, 0), skinny=True),
    C("f64_NN_17x4160x1000_deep_ktiles_odd", "f64", "NN", 17, 4160, 1000, ('32x64D', 1, 1, 1, 1000, 0, 0, 0), skinny=True),
    C("f64_NN_17x200x4097_deep_ktiles_odd_batch", "f64", "NN", 17, 200, 4097, ('32x64D', 1, 1, 1, 4097, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=2), skinny=True),
    C("f64_NN_40x200x16_deep_ktiles", "f64", "NN", 40, 200, 16, ('48x64D', 1, 1, 1, 16, 0, 1, 0), skinny=True),
    C("f64_NN_40x200x32_deep_ktiles", "f64", "NN", 40, 200, 32, ('48x64D', 1, 1, 1, 32, 0, 1, 0), skinny=True),
    C("f64_NN_40x200x48_deep_ktiles", "f64", "NN", 40, 200, 48, ('48x64D', 1, 1, 1, 48, 0, 1, 0), skinny=True),
    C("f64_NN_40x200x64_deep_ktiles", "f64", "NN", 40, 200, 64, ('48x64D', 1, 1, 1, 64, 0, 1, 0), skinny=True),
    C("f64_NN_40x4160x1000_deep_ktiles_odd", "f64", "NN", 40, 4160, 1000, ('48x64D', 1, 1, 1, 1000, 0, 0, 0), skinny=True),
    C("f64_NN_40x200x4097_deep_ktiles_odd_batch", "f64", "NN", 40, 200, 4097, ('48x64D', 1, 1, 1, 4097, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=2), skinny=True),
    C("c64_NN_17x200x16_deep_ktiles", "c64", "NN", 17, 200, 16, ('32x64D', 1, 1, 1, 16, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x32_deep_ktiles", "c64", "NN", 17, 200, 32, ('32x64D', 1, 1, 1, 32, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x48_deep_ktiles", "c64", "NN", 17, 200, 48, ('32x64D', 1, 1, 1, 48, 0, 1, 0), skinny=True),
    C("c64_NN_17x200x64_deep_ktiles", "c64", "NN", 17, 200, 64, ('32x64D', 1, 1, 1, 64, 0, 1, 0), skinny=True),
    C("c64_NN_17x4160x1000_deep_ktiles_odd", "c64", "NN", 17, 4160, 1000, ('32x64D', 1, 1, 1, 1000, 0, 0, 0), skinny=True),
    C("c64_NN_17x200x4097_deep_ktiles_odd_batch", "c64", "NN", 17, 200, 4097, ('32x64D', 1, 1, 1, 4097, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=2), skinny=True),
    C("c64_NN_40x200x16_deep_ktiles", "c64", "NN", 40, 200, 16, ('48x64D', 1, 1, 1, 16, 0, 1, 0), skinny=True),
    C("c64_NN_40x200x32_deep_ktiles", "c64", "NN", 40, 200, 32, ('48x64D', 1, 1, 1, 32, 0, 1, 0), skinny=True),
    C("c64_NN_40x200x48_deep_ktiles", "c64", "NN", 40, 200, 48, ('48x64D', 1, 1, 1, 48, 0, 1, 0), skinny=True),
    C("c64_NN_40x200x64_deep_ktiles", "c64", "NN", 40, 200, 64, ('48x64D', 1, 1, 1, 64, 0, 1, 0), skinny=True),
    C("c64_NN_40x4160x1000_deep_ktiles_odd", "c64", "NN", 40, 4160, 1000, ('48x64D', 1, 1, 1, 1000, 0, 0, 0), skinny=True),
    C("c64_NN_40x200x4097_deep_ktiles_odd_batch", "c64", "NN", 40, 200, 4097, ('48x64D', 1, 1, 1, 4097, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=2), skinny=True),
    # batch forms, epilogue and footprint
    C("f64_NN_70x45x37_ldc_plus_0", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 0), off=(0, 0, 3)),
    C("f64_NN_70x45x37_ldc_plus_1", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 1), off=(0, 0, 3)),
    C("f64_NN_70x45x37_ldc_plus_7", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 7), off=(0, 0, 3)),
    C("f64_NN_70x45x37_strided_2", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 3, 5), batch=Batch(count=2, c_gap=11)),
    C("f64_NN_70x45x37_strided_7", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 3, 5), batch=Batch(count=7, c_gap=11)),
    C("f64_NN_70x45x37_strided_130", "f64", "NN", 70, 45, 37, ('64x64', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 3, 5), batch=Batch(count=130, c_gap=11)),
    C("f64_NT_512x512x17_strided_32_big_tiles", "f64", "NT", 512, 512, 17, ('128x128', 1, 0, 1, 17, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=32, c_gap=3)),
    C("f64_TN_256x256x17_strided_32_tall_tiles", "f64", "TN", 256, 256, 17, ('128x64', 0, 1, 1, 17, 0, 1, 0), pad=(1, 0, 0), batch=Batch(count=32, c_gap=1)),
    C("f64_NN_2048x512x33_tall_8_tile_columns", "f64", "NN", 2048, 512, 33, ('128x64', 1, 1, 1, 33, 0, 1, 1), pad=(1, 1, 1)),
    C("f64_NN_70x45x37_strided_packed", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), batch=Batch(count=7)),
    C("f64_NN_70x45x37_a_shared", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=7, a_shared=True)),
    C("f64_TN_70x45x37_b_shared", "f64", "TN", 70, 45, 37, ('32x32', 0, 1, 1, 37, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=7, b_shared=True)),
    C("f64_TN_64x64x513_packed_split_rule1", "f64", "TN", 64, 64, 513, ('32x32', 0, 1, 2, 288, 1, 1, 0), batch=Batch(count=2)),
    C("f64_TN_32x64x129_packed_split_rule2", "f64", "TN", 32, 64, 129, ('32x32', 0, 1, 2, 96, 2, 1, 0), off=(1, 1, 1), batch=Batch(count=2)),
    C("f64_TN_64x64x513_not_packed_no_split_ldc", "f64", "TN", 64, 64, 513, ('32x32', 0, 1, 1, 513, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=2)),
    C("f64_TN_64x64x513_not_packed_no_split_gap", "f64", "TN", 64, 64, 513, ('32x32', 0, 1, 1, 513, 0, 1, 0), batch=Batch(count=2, c_gap=1)),
    C("f64_NN_24x40x16_b_sel_7", "f64", "NN", 24, 40, 16, ('64x64', 1, 1, 1, 16, 0, 1, 0), off=(1, 1, 1), batch=Batch(count=7, b_sel=True)),
    C("f64_NN_64x128x32_b_sel_130", "f64", "NN", 64, 128, 32, ('64x64', 1, 1, 1, 32, 0, 1, 0), batch=Batch(count=130, b_sel=True)),
    C("f64_NN_300x64x64_cmap_3", "f64", "NN", 300, 64, 64, ('32x32', 1, 1, 1, 64, 0, 1, 0), pad=(2, 0, 2), batch=Batch(count=3, cmap=True)),
    C("f64_NN_70x64x64_cmap_8", "f64", "NN", 70, 64, 64, ('32x32', 1, 1, 1, 64, 0, 1, 0), off=(0, 0, 1), batch=Batch(count=8, cmap=True)),
    C("f64_NN_300x32x64_subtract", "f64", "NN", 300, 32, 64, ('32x32', 1, 1, 1, 64, 0, 1, 0), pad=(2, 0, 2), off=(1, 1, 1), subtract=True),
    C("f64_NN_300x32x1025_subtract_split", "f64", "NN", 300, 32, 1025, ('32x32', 1, 1, 4, 288, 1, 1, 0), pad=(2, 0, 2), off=(1, 1, 1), subtract=True),
    C("f64_NN_70x45x37_subtract_batch", "f64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=7, c_gap=3), subtract=True),
    C("f64_NN_32x64x129_subtract_packed_split", "f64", "NN", 32, 64, 129, ('32x32', 1, 1, 2, 96, 2, 1, 0), batch=Batch(count=2), subtract=True),
    C("f64_NN_17x200x100_skinny_batch", "f64", "NN", 17, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=3, c_gap=5), skinny=True),
    C("c64_NN_70x45x37_ldc_plus_0", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 0), off=(0, 0, 3)),
    C("c64_NN_70x45x37_ldc_plus_1", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 1), off=(0, 0, 3)),
    C("c64_NN_70x45x37_ldc_plus_7", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 7), off=(0, 0, 3)),
    C("c64_NN_70x45x37_strided_2", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 3, 5), batch=Batch(count=2, c_gap=11)),
    C("c64_NN_70x45x37_strided_7", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 3, 5), batch=Batch(count=7, c_gap=11)),
    C("c64_NN_70x45x37_strided_130", "c64", "NN", 70, 45, 37, ('64x64', 1, 1, 1, 37, 0, 1, 0), pad=(1, 1, 1), off=(1, 3, 5), batch=Batch(count=130, c_gap=11)),
    C("c64_NN_70x45x37_strided_packed", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), batch=Batch(count=7)),
    C("c64_NN_70x45x37_a_shared", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=7, a_shared=True)),
    C("c64_TN_70x45x37_b_shared", "c64", "TN", 70, 45, 37, ('32x32', 0, 1, 1, 37, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=7, b_shared=True)),
    C("c64_HN_64x64x513_packed_split_rule1", "c64", "HN", 64, 64, 513, ('32x32', 0, 1, 2, 288, 1, 1, 0), batch=Batch(count=2)),
    C("c64_HN_32x64x129_packed_split_rule2", "c64", "HN", 32, 64, 129, ('32x32', 0, 1, 2, 96, 2, 1, 0), off=(1, 1, 1), batch=Batch(count=2)),
    C("c64_HN_64x64x513_not_packed_no_split_ldc", "c64", "HN", 64, 64, 513, ('32x32', 0, 1, 1, 513, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=2)),
    C("c64_HN_64x64x513_not_packed_no_split_gap", "c64", "HN", 64, 64, 513, ('32x32', 0, 1, 1, 513, 0, 1, 0), batch=Batch(count=2, c_gap=1)),
    C("c64_NN_24x40x16_b_sel_7", "c64", "NN", 24, 40, 16, ('64x64', 1, 1, 1, 16, 0, 1, 0), off=(1, 1, 1), batch=Batch(count=7, b_sel=True)),
    C("c64_NN_64x128x32_b_sel_130", "c64", "NN", 64, 128, 32, ('64x64', 1, 1, 1, 32, 0, 1, 0), batch=Batch(count=130, b_sel=True)),
    C("c64_NN_300x64x64_cmap_3", "c64", "NN", 300, 64, 64, ('32x32', 1, 1, 1, 64, 0, 1, 0), pad=(2, 0, 2), batch=Batch(count=3, cmap=True)),
    C("c64_NN_70x64x64_cmap_8", "c64", "NN", 70, 64, 64, ('32x32', 1, 1, 1, 64, 0, 1, 0), off=(0, 0, 1), batch=Batch(count=8, cmap=True)),
    C("c64_NN_300x32x64_subtract", "c64", "NN", 300, 32, 64, ('32x32', 1, 1, 1, 64, 0, 1, 0), pad=(2, 0, 2), off=(1, 1, 1), subtract=True),
    C("c64_NN_300x32x1025_subtract_split", "c64", "NN", 300, 32, 1025, ('32x32', 1, 1, 4, 288, 1, 1, 0), pad=(2, 0, 2), off=(1, 1, 1), subtract=True),
    C("c64_NN_70x45x37_subtract_batch", "c64", "NN", 70, 45, 37, ('32x32', 1, 1, 1, 37, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=7, c_gap=3), subtract=True),
    C("c64_NN_32x64x129_subtract_packed_split", "c64", "NN", 32, 64, 129, ('32x32', 1, 1, 2, 96, 2, 1, 0), batch=Batch(count=2), subtract=True),
    C("c64_NN_17x200x100_skinny_batch", "c64", "NN", 17, 200, 100, ('32x64D', 1, 1, 1, 100, 0, 1, 0), pad=(0, 0, 1), batch=Batch(count=3, c_gap=5), skinny=True),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
