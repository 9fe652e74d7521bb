/*
 * qilaplace_hip_testing.h -- test, fault-injection and measurement hooks of libqilhip.so.
 *
 * NOT part of the drop-in boundary: nothing here replaces a method of the reference.  The parity suite
 * (tests/), bench.py and tools/ use these entries; a Julia / C client of the boundary never needs them.  They are exported
 * by the same library so that the shipped binary is the one that is tested and measured.
 */
#ifndef QILAPLACE_HIP_TESTING_H
#define QILAPLACE_HIP_TESTING_H

#include "qilaplace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Testing aid: the n-th pool allocation from now (0 = the next one) fails with QIL_ENOMEM; n < 0 switches the
 * injection off.  Used to check that a failing call leaves no device memory behind and its operands intact. */
QIL_API int qil_context_fail_alloc_after(qil_context* ctx, int64_t n);
/* Testing aid: pool bytes in use that no MPS/MPO handle owns.  Zero between calls -- every temporary is back in
 * the pool whether the last call succeeded or failed.                                                        */
QIL_API int qil_context_unowned_bytes(qil_context* ctx, int64_t* out);

/* HIP-event timing on the context's stream (hipEventRecord / hipEventElapsedTime). */
QIL_API int qil_timer_start(qil_context* ctx);
QIL_API int qil_timer_stop(qil_context* ctx, double* elapsed_ms);   /* synchronises the stop event */
/* Per-kernel profile: when enabled every launch of the site-contraction kernel is
 * bracketed by its own event pair; read returns launches and summed device ms since
 * the last reset (synchronises).                                                   */
QIL_API int qil_profile_enable(qil_context* ctx, int on);
QIL_API int qil_profile_read(qil_context* ctx, int64_t* n_launches, double* total_ms, int reset);

/* Diagnostic: the store-only HBM ceiling of THIS GPU -- `bytes` (>= 64 MiB) written `reps` times by each of four writers
 * (hipMemsetAsync, 256 KiB span per workgroup with plain / non-temporal stores, grid-stride fill), HIP events; the best rate
 * in GB/s and which writer reached it (0..3).  bench.py prints it beside the apply's roofline fraction so that lines measured
 * on different boxes of a pool can be compared.                                                                         */
QIL_API int qil_hbm_store_peak(qil_context* ctx, int64_t bytes, int reps, double* best_gbs, int* best_kind);

/* Diagnostic: device-resident time of the same GEMM (operands generated in HBM, HIP events). */
QIL_API int qil_gemm_device_time(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                         int reps, double* ms_per_call);

/* Everything the MFMA GEMM decides on the host before it launches: THE decision, not a copy of it -- the launch code
 * switches on this struct.  (bm, bn, gkt, deep) name the kernel's output tile, K step and whether two K tiles are in
 * flight; arc / bkc: op(A)'s row index / op(B)'s k index is the contiguous one; splits K slices of kchunk each, decided
 * by split_rule (0 = none, 1 = few tiles and a long K, 2 = at most four tiles from K = 128, 3 = one wave of tiles and
 * K >= 4096); col_fastest: tiles are walked along a tile row first; xcd: the XCD-aware tile permutation is applied. */
typedef struct qil_gemm_plan_info {
    int bm, bn, wm, wn, gkt, deep;
    int arc, bkc;
    int splits, split_rule;
    int64_t kchunk;
    int col_fastest, xcd;
    int64_t tiles_m, tiles_n;
    int can_split;                      /* a batch may only split K when its outputs are packed */
} qil_gemm_plan_info;
/* The plan of C (m x n) = op(A) op(B) for a batch of `count` products whose outputs lie c_bs elements apart (has_cmap: scattered
 * column blocks; skinny_m: the caller's skinny hint).  Host only: no context, no GPU.  QIL_EINVAL_ARG for bad op codes, empty
 * operands or leading dimensions smaller than the stored rows. */
QIL_API int qil_gemm_plan(int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc,
                          int64_t count, int64_t c_bs, int has_cmap, int skinny_m, qil_gemm_plan_info* plan);

/* Which code path a read-out call takes: THE decision, not a copy of it -- qil_coefficient_batch, qil_coefficient_marginal_batch,
 * qil_apply_coefficient_sweep and qil_apply_coefficient_batch switch on the value this function returns.  Host only: no context,
 * no GPU.  verb: which entry is asked; dtype: of the chain that is contracted (QIL_C64 when W or psi is complex); nb queries;
 * chain_dims: the n + 1 bond dimensions of the chain that is read out -- psi for the plain, marginal and lazy verbs; for the sweep
 * the product W psi, or psi together with op_dims; op_dims: the operator's n + 1 bond dimensions (required for QIL_READOUT_LAZY,
 * optional for QIL_READOUT_SWEEP, null otherwise).  *pass_queries (may be null): queries per pass on QIL_ROUTE_LAZY_GEMM -- its
 * scratch is bounded by 8 GiB and its batch by the grid limit -- and nb on every other route. */
enum { QIL_READOUT_PLAIN = 0, QIL_READOUT_MARGINAL = 1, QIL_READOUT_SWEEP = 2, QIL_READOUT_LAZY = 3 };
enum {
    QIL_ROUTE_CHAIN = 0,        /* one workgroup per query walks the chain (coefficient_chain) */
    QIL_ROUTE_GEMM_SELECT = 1,  /* all queries together: one GEMM with the whole site, each query keeps its slice (or their sum) */
    QIL_ROUTE_GEMM_SORTED = 2,  /* all queries together, sorted by their bit at every site: one GEMM per slice, rows gathered */
    QIL_ROUTE_LAZY_CHAIN = 3,   /* <bits|W psi>, one workgroup per query (lazy_coefficient_chain) */
    QIL_ROUTE_LAZY_GEMM = 4     /* <bits|W psi>, two strided-batch GEMMs per site, pass_queries queries at a time */
};
QIL_API int qil_readout_route(int verb, int dtype, int64_t nb, int64_t n, const int64_t* chain_dims, const int64_t* op_dims,
                              int* route, int64_t* pass_queries);

/* One operand of qil_gemm_batched_host: a whole host buffer of `elems` elements; the product uses base + off with leading dimension
 * ld, batch b a further b * bs elements on. */
typedef struct qil_gemm_host_operand {
    void* base;
    int64_t elems, off, ld, bs;
} qil_gemm_host_operand;
/* The batched and epilogue forms of the GEMM on host operands: uploads the three parent buffers whole (C included), runs the
 * dispatch on base + off -- so the device addresses carry the offsets the internal callers produce -- and downloads the whole of
 * C.  subtract: C <- C - op(A) op(B); skinny_m: the skinny hint; b_sel (count entries b_sel_step apart, or null): batch b reads
 * B a further b_sel[b * b_sel_step] * b_sel_stride elements on; cmap (count * n / cmap_blk entries, or null): output column block
 * g of batch b goes to column block cmap[b * n / cmap_blk + g] of C.  Every element the product would touch must lie inside
 * its buffer (QIL_EINVAL_ARG otherwise). */
QIL_API int qil_gemm_batched_host(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                                  const qil_gemm_host_operand* A, const qil_gemm_host_operand* B, const qil_gemm_host_operand* C,
                                  int64_t count, int subtract, int skinny_m, const uint8_t* b_sel, int64_t b_sel_step,
                                  int64_t b_sel_stride, const int32_t* cmap, int64_t cmap_blk);

/* Everything the thin QR (qr_impl: under every gauge sweep, zip-up, the RSVD encoder and the Schmidt spectra) decides on the host before
 * it launches: THE decision, not a copy of it -- qr_impl switches on this struct, and the launchers of the panel kernels take
 * their LDS size, KM variant and chunk length from the same helpers that fill it.
 *   cholesky_eligible: CholeskyQR2 is tried first (unless a refusal earlier in the same call makes qr_impl skip it); the other
 *     fields describe the route taken when it is not tried, is skipped or refuses.
 *   route: one launch of the CGS2 kernel, one Householder panel, one row-chunk tree, or the blocked driver.
 *   panel_width: columns per panel (blocked: 16 or 32; single routes: n); last_panel_width: of the last panel.
 *   panel_kind / last_panel_kind: the kernel of the full-width panels / of the last panel (equal when there is one panel or n is a
 *     multiple of panel_width); has_hh, has_tree, has_cgs2_lds, has_cgs2_global: the table of panels contains that kind.
 *   fused_in_lds: a CGS2 kernel runs on the operand's rows and every such launch keeps its panel in LDS; fused_short_rows: ... and
 *     m <= 256, where a 16-lane row, not a wave, takes each previous column.
 *   hh_km, hh_waves: the rows-per-lane variant (2, 4, 6, 8, 9, 13, 19) and waves of the Householder panel kernel; 0 without one.
 *   tree_chunk rows per chunk, tree_chunks of them, the last one tree_last_rows long; tree_in_lds: a chunk x 16 (single tree
 *     panel: x n) slice of the first level stays in LDS; tree_top_in_lds: so do the stacked triangles of the second level.  All 0
 *     without a tree panel. */
enum { QIL_QR_SINGLE_CGS2 = 0, QIL_QR_SINGLE_HH = 1, QIL_QR_SINGLE_TREE = 2, QIL_QR_BLOCKED = 3 };
enum { QIL_QR_PANEL_NONE = 0, QIL_QR_PANEL_HH = 1, QIL_QR_PANEL_TREE = 2, QIL_QR_PANEL_CGS2_LDS = 3, QIL_QR_PANEL_CGS2_GLOBAL = 4 };
typedef struct qil_qr_plan_info {
    int cholesky_eligible;
    int route;
    int panel_width, last_panel_width;
    int panel_kind, last_panel_kind;
    int has_hh, has_tree, has_cgs2_lds, has_cgs2_global;
    int fused_in_lds, fused_short_rows;
    int hh_km, hh_waves;
    int64_t tree_chunk, tree_chunks, tree_last_rows;
    int tree_in_lds, tree_top_in_lds;
} qil_qr_plan_info;
/* The plan of the thin QR of an m x n operand (m >= n >= 1).  Host only: no context, no GPU. */
QIL_API int qil_qr_plan(int dtype, int64_t m, int64_t n, qil_qr_plan_info* plan);

/* What one qil_qr_host call did.  plan: as qr_impl filled it for the outer factorisation.  cholesky: 0 not eligible; 1 done, first-
 * order second pass; 2 done, full second factorisation; 3 refused in the first pass; 4 refused in the second; 5 skipped after an
 * earlier refusal.  repairs: re-factorisations qr_reorthogonalise ran (0..2); passes: how often it measured Q^H Q, worst[i] the
 * off-diagonal maximum of pass i; skipped_check: it returned early because Q was known orthonormal (outcome 1). */
typedef struct qil_qr_report {
    qil_qr_plan_info plan;
    int cholesky, repairs, passes, skipped_check;
    double worst[3];
} qil_qr_report;
/* The thin QR with non-negative diagonal on host operands: uploads the parent buffer of A whole (a_elems elements; the operand is
 * m x n at a_base + a_off with leading dimension lda >= m) and, unless r_base is null, that of R (n x n at r_off, ldr >= n), runs
 * qil_dev_qr_positive on the offset device addresses and downloads both parents whole: Q in place of A.  reorth: the `orthonormal`
 * flag (measure Q^H Q, factor again while it is off).  cholesky_skip: CholeskyQR2 attempts to skip, as after a refusal earlier in
 * the same call.  Every element of both windows must lie inside its buffer (QIL_EINVAL_ARG otherwise). */
QIL_API int qil_qr_host(qil_context* ctx, int dtype, int64_t m, int64_t n, void* a_base, int64_t a_elems, int64_t a_off, int64_t lda,
                        void* r_base, int64_t r_elems, int64_t r_off, int64_t ldr, int reorth, int cholesky_skip,
                        qil_qr_report* report);

#ifdef __cplusplus
}
#endif
#endif /* QILAPLACE_HIP_TESTING_H */
