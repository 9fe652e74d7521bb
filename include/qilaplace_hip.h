/*
 * qilaplace_hip.h -- C ABI of libqilhip.so, the MI355X (gfx950) implementation of
 * QILaplace.jl's MPO x MPS apply / coefficient / compress / encode hot path.
 *
 * The reference (SUTD-MDQS/QILaplace.jl v0.1.1) has NO FFI layer: its boundary is
 * Julia multiple dispatch on ITensors-backed containers.  Each entry point below
 * names the reference method it stands in for (file:line relative to the
 * reference tree); INTEGRATION.md shows the `ccall` methods a maintainer adds so
 * `apply`, `*`, `coefficient`, `compress!`, `signal_mps` ... dispatch here.
 *
 * Data layout at the boundary (fixed, canonical; all COLUMN-MAJOR, first index
 * fastest, complex = interleaved (re, im) doubles):
 *     MPS site   A[alpha, s, beta]          dims (chi_l, 2, chi_r)
 *     MPO site   W[a, s_in, s_out, b]       dims (D_l, 2, 2, D_r)
 *         s_in  = the reference's primed leg  s'  (contracted with the MPS)
 *         s_out = the reference's unprimed leg s  (survives)    src/linalg/apply.jl:98-101
 * Edge tensors carry explicit dimension-1 bonds.  Paired-register objects
 * (ZTMPS / PairedSiteMPO) are passed as their interleaved 2n-tensor chain
 * main_1, copy_1, main_2, ... (src/mps.jl:421-444, src/linalg/apply.jl:16-32)
 * with `paired = 1`.
 *
 * Ownership: handles returned through `out` parameters belong to the caller and
 * must be released with the matching *_destroy.  The library never keeps a host
 * pointer after a call returns.  Device buffers belong to the handle.
 *
 * Errors: every function returns a qil_status; qil_last_error() gives the
 * thread-local message.  The host shims re-raise QIL_EINVAL_* as ArgumentError
 * and QIL_EDOMAIN as DomainError (Julia) / ValueError and ArithmeticError (Python).
 *
 * Threading: one HIP stream per qil_context; calls on one context are serialised
 * by the caller, calls on different contexts are independent.  There is no global
 * RNG (the reference's rsvd reseeds Julia's global RNG, src/linalg/rsvd.jl:74):
 * seeds are explicit parameters.
 */
#ifndef QILAPLACE_HIP_H
#define QILAPLACE_HIP_H

#include <stdint.h>

/* The library is built with -fvisibility=hidden: the entries declared QIL_API (here and in qilaplace_hip_testing.h) are
 * its whole dynamic symbol table -- no C++ internals, no template instantiations (tests/test_cabi_symbols.py). */
#ifndef QIL_API
#define QIL_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qil_context qil_context;
typedef struct qil_mps qil_mps;   /* SignalMPS (src/mps.jl:70-79) or ZTMPS chain (:98-117) */
typedef struct qil_mpo qil_mpo;   /* SingleSiteMPO / PairedSiteMPO (src/mpo.jl:26-74)       */

typedef enum { QIL_F64 = 0, QIL_C64 = 1 } qil_dtype;

typedef enum {
    QIL_OK = 0,
    QIL_EINVAL_LENGTH = 1, /* ArgumentError: site-count mismatch (apply.jl:76-80, 202-203; mps.jl:671-672) */
    QIL_EINVAL_SITES = 2,  /* ArgumentError: site-identity mismatch (apply.jl:81-85, 130)                 */
    QIL_EINVAL_CONFIG = 3, /* ArgumentError: bad bit configuration (mps.jl:612, 619-628, 634-643)         */
    QIL_EDOMAIN = 4,       /* DomainError: N < 2 in compress! (mps.jl:918), bad center (:800, :820)       */
    QIL_ENOMEM = 5,
    QIL_EHIP = 6,          /* a HIP runtime call failed; message carries hipGetErrorString                */
    QIL_EINVAL_ARG = 7,    /* null handle, bad dtype / method / direction (SignalConverters.jl:200-201)   */
    QIL_EEMPTY = 8         /* rsvd: left or right index set empty (rsvd.jl:56-60)                         */
} qil_status;

typedef enum { QIL_METHOD_SVD = 0, QIL_METHOD_RSVD = 1 } qil_method;     /* method=:svd / :rsvd   */
typedef enum { QIL_DIR_RIGHT = 0, QIL_DIR_LEFT = 1 } qil_direction;      /* :right / :left        */

/* "no cap": the reference's typemax(Int) defaults for maxdim */
#define QIL_MAXDIM_NONE INT64_MAX

/* ------------------------------------------------------------------ library / context */
QIL_API const char* qil_last_error(void);
QIL_API const char* qil_version(void);
/* number of visible HIP devices (does not initialise a context) */
QIL_API int qil_device_count(int* out);

/* One context = one device + one HIP stream + a caching device-memory pool.
 * `stream` may be NULL (the context creates its own non-blocking stream) or an
 * existing hipStream_t to enqueue on (e.g. torch's current stream).            */
QIL_API int qil_context_create(int device, void* stream, qil_context** out);
QIL_API int qil_context_destroy(qil_context* ctx);
QIL_API int qil_context_synchronize(qil_context* ctx);
/* release cached (free) device blocks back to the driver */
QIL_API int qil_context_trim(qil_context* ctx);
QIL_API int qil_context_mem_info(qil_context* ctx, int64_t* pool_bytes_in_use, int64_t* pool_bytes_cached,
                         int64_t* device_free, int64_t* device_total);
/* Host CPUs the batch runners of this process may keep busy: min(cgroup CPU quota, affinity mask) / LOCAL_WORLD_SIZE
 * (the ranks torch.distributed.run / bench.py place on this node), overridden by QIL_CPU_BUDGET.  The lock-step batch
 * entry points (qil_*_batch) never run more polling launcher threads than this minus one.  No reference counterpart
 * (the reference is single-threaded Julia + BLAS threads, benchmarking.md:12).                                      */
QIL_API int qil_host_cpu_budget(int* out);

/* (fault injection, pool accounting, HIP-event timers and the apply-kernel profile are not part of the boundary:
 * include/qilaplace_hip_testing.h) */

/* ------------------------------------------------------------------ containers (T1-T3) */
/* Construct from HOST tensors.  bond_dims: the n-1 internal bonds.  site_ids: n
 * labels playing the role of the reference's Index identities (may be NULL =>
 * 1..n).  site_ptrs[i]: host tensor i in the canonical layout above.
 * Replaces SignalMPS(data, sites, bonds; amplitude) src/mps.jl:121-146 and
 * ZTMPS(...) :148-184 (paired = 1, n even).                                       */
QIL_API int qil_mps_create(qil_context* ctx, int64_t n, int dtype, int paired, const int64_t* bond_dims,
                   const int64_t* site_ids, const void* const* site_ptrs, double amplitude,
                   qil_mps** out);
/* Same, but tensors left uninitialised on the device (fill through qil_mps_site_device_ptr). */
QIL_API int qil_mps_alloc(qil_context* ctx, int64_t n, int dtype, int paired, const int64_t* bond_dims,
                  const int64_t* site_ids, double amplitude, qil_mps** out);
QIL_API int qil_mps_destroy(qil_mps* psi);
QIL_API int qil_mps_clone(const qil_mps* psi, qil_mps** out);
QIL_API int qil_mps_nsites(const qil_mps* psi, int64_t* n);
QIL_API int qil_mps_dtype(const qil_mps* psi, int* dtype);
QIL_API int qil_mps_is_paired(const qil_mps* psi, int* paired);
QIL_API int qil_mps_bond_dims(const qil_mps* psi, int64_t* bond_dims /* n-1 */);
QIL_API int qil_mps_site_ids(const qil_mps* psi, int64_t* site_ids /* n */);
QIL_API int qil_mps_amplitude(const qil_mps* psi, double* amplitude);
QIL_API int qil_mps_set_amplitude(qil_mps* psi, double amplitude);
QIL_API int qil_mps_site_nbytes(const qil_mps* psi, int64_t i, int64_t* nbytes);
QIL_API int qil_mps_download_site(const qil_mps* psi, int64_t i, void* host_dst);
QIL_API int qil_mps_upload_site(qil_mps* psi, int64_t i, const void* host_src);
QIL_API int qil_mps_site_device_ptr(const qil_mps* psi, int64_t i, void** dev_ptr);
/* seeded device-side fill with i.i.d. N(0,1)/sqrt(2 chi_l) entries (synthetic workloads) */
QIL_API int qil_mps_fill_random(qil_mps* psi, uint64_t seed);

/* SingleSiteMPO(data, sites, bonds) src/mpo.jl:30-43 / PairedSiteMPO :62-73 (paired = 1) */
QIL_API int qil_mpo_create(qil_context* ctx, int64_t n, int dtype, int paired, const int64_t* bond_dims,
                   const int64_t* site_ids, const void* const* site_ptrs, qil_mpo** out);
QIL_API int qil_mpo_alloc(qil_context* ctx, int64_t n, int dtype, int paired, const int64_t* bond_dims,
                  const int64_t* site_ids, qil_mpo** out);
QIL_API int qil_mpo_destroy(qil_mpo* W);
QIL_API int qil_mpo_nsites(const qil_mpo* W, int64_t* n);
QIL_API int qil_mpo_dtype(const qil_mpo* W, int* dtype);
QIL_API int qil_mpo_is_paired(const qil_mpo* W, int* paired);
QIL_API int qil_mpo_bond_dims(const qil_mpo* W, int64_t* bond_dims /* n-1 */);
QIL_API int qil_mpo_site_ids(const qil_mpo* W, int64_t* site_ids /* n */);
QIL_API int qil_mpo_site_nbytes(const qil_mpo* W, int64_t i, int64_t* nbytes);
QIL_API int qil_mpo_download_site(const qil_mpo* W, int64_t i, void* host_dst);
QIL_API int qil_mpo_site_device_ptr(const qil_mpo* W, int64_t i, void** dev_ptr);
QIL_API int qil_mpo_fill_random(qil_mpo* W, uint64_t seed);

/* ------------------------------------------------------------------ apply (A1-A3) */
/* apply(W::SingleSiteMPO, psi::SignalMPS) src/linalg/apply.jl:75-122 and
 * apply(W::PairedSiteMPO, psi::ZTMPS) :201-218 (and `*`, :233-236).
 *   B_i[(a,alpha), s, (b,beta)] = sum_{s'} W_i[a, s', s, b] * A_i[alpha, s', beta]
 * written once, directly in the fused layout row = alpha + chi_l*a, col = beta + chi_r*b.
 * No truncation (the reference ignores cutoff/maxdim kwargs, apply.jl:75).  Output
 * shares psi's site ids and amplitude (apply.jl:121, :216); dtype = promote(W, psi).
 * Errors: QIL_EINVAL_LENGTH (apply.jl:76-80, 202-203), QIL_EINVAL_SITES (:81-85).  */
QIL_API int qil_apply(const qil_mpo* W, const qil_mps* psi, qil_mps** out);
/* Same, into an existing handle of identical shape/dtype (no allocation). */
QIL_API int qil_apply_into(const qil_mpo* W, const qil_mps* psi, qil_mps* out);
/* apply(W1, W2) MPO x MPO, "W1 first, then W2", window semantics of apply.jl:124-199
 * (paired: :220-230).  QIL_EINVAL_SITES when the supports are disjoint (:130).     */
QIL_API int qil_apply_mpo_mpo(const qil_mpo* W1, const qil_mpo* W2, qil_mpo** out);

/* ------------------------------------------------------------------ read-out (C1, C2, K3) */
/* coefficient(psi, cfg) src/mps.jl:669-693 for nb configurations at once.
 * bits: host, nb x n bytes, query-major, bits[q*n + i] in {0,1} for site i+1 (site 1
 * first = MSB of a signal index; paired: interleaved main_1, copy_1, ...).
 * out: host, nb complex doubles (re, im) = amplitude * prod_i A_i[:, bit_i, :].
 * Errors: QIL_EINVAL_CONFIG for a bit outside [0,1] (mps.jl:612).                  */
QIL_API int qil_coefficient_batch(const qil_mps* psi, int64_t nb, const uint8_t* bits, double* out);
/* Same with bit value 2 allowed = "sum over this site's physical index" (marginal / partial trace with
 * the all-ones vector).  Serves the coefficient-grid and Laplace-value scans of the tutorials
 * (docs/src/tutorials/dt.jl:187-197 sums N coefficient calls per value; zt.jl:283-309 scans 256 x 256
 * grids) with one chain per value instead of N. */
QIL_API int qil_coefficient_marginal_batch(const qil_mps* psi, int64_t nb, const uint8_t* bits, double* out);
/* Product-vector read-out, the contraction of coefficient (src/mps.jl:669-678) with a weighted sum of the two physical
 * slices in place of one of them:
 *   out[r] = amplitude * prod_i ( v[r,i,0] A_i[:,0,:] + v[r,i,1] A_i[:,1,:] ),  r < nb, i < n tensors (2n for a paired state).
 * v: host, nb * n * 2 complex values (re, im interleaved; row-major in r, i, s).  out: host, nb complex values.
 * With v = e_bit it is qil_coefficient_batch; with v = (1, 1) on a site, that site's marginal.  With v[r,i,:] = (1, w^(2^(n-i)))
 * it is sum_j x_j w^j of the encoded signal, at any complex w: O(n chi^2) per row, no operator and no grid.
 * The carry is complex for either site dtype; real weights on a real state give an imaginary part of exactly zero.
 * Errors, before the context is activated: QIL_EINVAL_ARG for a null psi, nb < 0, a null v or out with nb > 0, or a weight that
 * is not finite (the message names the row and the tensor).  nb = 0 is a no-op.
 * Route: the marginal read-out's decision for (nb, bonds), except that bonds below 128 stay on the first route while
 * nb * bond^2 < 2^21.  One workgroup per row with the carry in LDS (bonds up to QIL_PRODUCT_CHAIN_MAX_BOND), or one f64-MFMA GEMM
 * per tensor for all rows and a kernel that combines each row's two slices; QIL_PRODUCT_ROUTE=chain / gemm (read per call)
 * forces one where it fits. */
#define QIL_PRODUCT_CHAIN_MAX_BOND 1024
#define QIL_MPO_ENTRY_CHAIN_MAX_BOND 1024   /* qil_mpo_entry_batch's one-launch route, below */
QIL_API int qil_product_batch(const qil_mps* psi, int64_t nb, const double* v, double* out);
/* Read-out by index, device to device:
 *   out_dev[j] = amplitude * prod_i A_i[:, bit_i(idx_dev[j]), :],  j < count,
 * tensor 1 the most significant bit of the index, as in qil_signal_mps; for a paired state the bits are the 2n interleaved
 * tensors main_1, copy_1, ...  idx_dev: count int64 indices in HBM.  out_dev: count values of psi's dtype in HBM -- a real
 * state gives doubles, not (re, im) pairs: the layout qil_cross_supply takes.
 * Errors, before the context is activated: QIL_EINVAL_ARG for a null psi, count < 0, a null idx_dev or out_dev with count > 0,
 * and for a chain of more than 62 tensors.  count = 0 is a no-op.  An index outside [0, 2^n) is NOT an error (finding it would
 * need a read-back): out_dev holds NaN at that position, in both parts for a complex state.
 * Stream rule, that of qil_cross_indices / qil_cross_supply: the caller orders the producer of idx_dev before the call; the
 * verb runs on the context's stream and synchronises it before returning.  No index or value is copied to or from the host;
 * every temporary is a pool block that returns before the call does.
 * Route: bonds up to QIL_COEFFICIENT_AT_WAVE_MAX_BOND: one launch, one wave per index with the carry vector in LDS private to
 * the wave; wider chains: the indices are expanded to device bits and take the marginal read-out's routes (one workgroup per
 * index, or one f64-MFMA GEMM per tensor for all of them).  QIL_COEFFICIENT_AT_ROUTE=wave / bits (read per call) forces one;
 * wave only while the carry fits the LDS (bonds up to 1024).  The cap is measured (MEASUREMENTS section 29): up to bond 8 the
 * wave route never loses (equal at 64 indices, 2.9x faster at 262144); at bond 16 it wins near 4096 indices only, from bond
 * 32 on it loses at all counts but a tie near 4096 (4x to 5x at 262144 indices, 9x to 11x at bond 64). */
#define QIL_COEFFICIENT_AT_WAVE_MAX_BOND 8
QIL_API int qil_coefficient_at(const qil_mps* psi, int64_t count, const int64_t* idx_dev, void* out_dev);
/* <bits| W psi> without materialising W*psi (same numbers as
 * qil_coefficient_batch(qil_apply(W, psi))).                                      */
QIL_API int qil_apply_coefficient_batch(const qil_mpo* W, const qil_mps* psi, int64_t nb,
                                const uint8_t* bits, double* out);
/* The body of a damping sweep: for each of the nw operators (the reference's loop `W = build_dt_mpo(psi, wr);
 * out = W * psi; coefficient(out, ...)`, docs/src/tutorials/dt.jl:150-197, zt.jl:300-348) the product W_j psi is
 * materialised by the apply kernel (apply.jl:75-122) and read out at the same nb configurations (mps.jl:669-693).
 * out: host, nw x nb complex doubles, operator-major.  One upload, one download, one synchronisation for the batch.  */
QIL_API int qil_apply_coefficient_sweep(const qil_mpo* const* Ws, int64_t nw, const qil_mps* psi, int64_t nb,
                                const uint8_t* bits, double* out);
/* mps_to_vector(psi; reverse) src/mps.jl:716-743: 2^n values of psi's dtype, times amplitude. */
QIL_API int qil_mps_to_vector(const qil_mps* psi, int reverse, void* host_out);
/* Dense read-out of a sub-lattice of configurations: spec[i] = 0 / 1 fixes site i's bit, 2 sums the site
 * (marginal), 3 leaves it free; host_out receives the 2^(#free) coefficients (psi's dtype, times amplitude),
 * free sites in chain order, the first one the most significant bit (reverse = 0) or the least (reverse = 1).
 * All free = mps_to_vector (mps.jl:716-743), none free = coefficient (mps.jl:669-678); in between it is the
 * (k, l) grid scan of docs/src/tutorials/zt.jl:283-309 or the N-term Laplace sums of dt.jl:187-197 as one
 * contraction.  QIL_EINVAL_CONFIG for spec values > 3, QIL_EINVAL_LENGTH for more than 34 free sites.      */
QIL_API int qil_mps_block(const qil_mps* psi, const uint8_t* spec, int reverse, void* host_out);
/* norm(psi) src/mps.jl:754-771 (without amplitude). */
QIL_API int qil_norm(const qil_mps* psi, double* out);
/* Perfect sampling (ITensors' sample(::MPS)): nb configurations x drawn with probability |psi_x|^2 / |psi|^2.
 * For the chain's n site tensors A_i[alpha, s, beta] (paired: the 2n interleaved tensors):
 *   Right environments: R_n = [1], R_{i-1} = sum_s A_i[:, s, :] R_i A_i[:, s, :]^H (Hermitian PSD, chi_{i-1} x chi_{i-1}),
 *   each normalised on the device by its trace (only ratios matter).
 *   Sample r carries a row vector v (v = [1] at the start).  At site i: w_s = v A_i[:, s, :], q_s = Re(w_s R_i w_s^H);
 *   s = 0 iff u_{r,i} (q_0 + q_1) < q_0, else s = 1; then v <- w_s / sqrt(q_s) and the sample's probability is
 *   multiplied by q_s / (q_0 + q_1).
 *   Uniforms: the caller's (host, nb x n, sample-major, each in [0, 1)), or when uniforms is null
 *   u_{r,i} = (splitmix64(seed ^ splitmix64(r n + i)) >> 11) 2^-53.  Sample r depends only on (psi, seed, r): not on nb,
 *   on the internal chunking of rows or on the route, up to rounding at a threshold.
 *   The amplitude does not enter; prob_out (nullable, host, nb doubles) receives |psi_x|^2 / |psi|^2.
 *   If q_0 + q_1 <= 0 on a reached prefix (rounding only), the larger q is taken, s = 0 when both are 0, and the
 *   probability factor is 0.
 * bits_out: host, nb x n bytes, the layout of qil_coefficient_batch's bits (the rows go straight back into it).
 * Errors, before the context is activated: QIL_EINVAL_ARG for a null psi or bits_out or nb < 0, QIL_EINVAL_CONFIG
 * for a uniform outside [0, 1).  QIL_EDOMAIN for a state of norm 0.  nb = 0 is a no-op.
 * Bonds <= 64 (f64) / 32 (c64) take one fused f64-MFMA kernel per site, larger ones GEMMs and a reduce-and-choose kernel. */
QIL_API int qil_sample(const qil_mps* psi, int64_t nb, uint64_t seed, const double* uniforms, uint8_t* bits_out,
                       double* prob_out);
/* Top-k coefficient search: the k configurations x with the largest |psi_x|, and a bound on what the search may have missed.
 * A beam search over prefixes x_1..x_i ranked by their marginal weight w(prefix) = sum over completions of |psi_x|^2, which
 * bounds every completion: |psi_x|^2 <= w(prefix).
 *   Right environments as in qil_sample, with their normalisation kept as a cumulative log-scale (log |psi|^2).
 *   The frontier starts as one empty prefix, v = [1].  At site i every prefix yields two children, T_s = v A_i[:, s, :] with
 *   weight Re(T_s R_i T_s^H); the at most `beam` children of largest weight are kept (ties: the lower parent row, then bit 0),
 *   rescaled with a per-row log-scale; the largest weight dropped is recorded.  After the last site the frontier holds
 *   complete configurations with their exact values.
 * bits_out: host, k x n_tensors bytes, the layout of qil_coefficient_batch's bits.  val_out: host, k complex (re, im), the
 * numbers qil_coefficient_batch gives on those rows (amplitude included), in descending |value| (equal magnitudes: the order
 * of the candidates).  bound_out: sqrt(largest weight dropped before the last site), on the scale of the values (amplitude
 * included), 0 if nothing was dropped.  The result is certified to be the exact top-k when bound < |value_k| (1 - 1e-10):
 * the slack covers the rounding of the weights (relative ~1e-15 per site).
 * Bit-identical from run to run; nothing is chunked.  Limits: beam <= min(2^29, 2^30 / (3 chi s + 4 n + 64)), chi = the largest
 * bond, s = 8 (f64) / 16 (c64), n = n_tensors: the frontier, both children and the per-row bookkeeping fit in 1 GiB (T_s R
 * adds 2 chi s bytes per row).  At n = 24 paired, chi = 64, c64 the cap is 322638.
 * Errors, before the context is activated: QIL_EINVAL_ARG for a null psi, k < 0, beam < k, beam above the cap,
 * k > 2^n_tensors (n_tensors <= 62) or, when k > 0, a null output.  QIL_EDOMAIN for a state of norm 0.  k = 0 is a no-op.
 * Route: qil_dev_gemm for T = V A and T_s R at any bond size, a scoring kernel for both children, a radix select and a
 * prefix-scan compaction on the device. */
QIL_API int qil_top_k(const qil_mps* psi, int64_t k, int64_t beam, uint8_t* bits_out, double* val_out, double* bound_out);

/* ------------------------------------------------------------------ overlaps (ITensors' inner on device chains) */
/* <phi|psi> = amp_phi * amp_psi * sum_x conj(phi_x) psi_x
 *           = vdot(mps_to_vector(phi), mps_to_vector(psi)).  out: host, one complex double (re, im).
 * phi and psi: same context, same paired flag (QIL_EINVAL_ARG), same number of sites (QIL_EINVAL_LENGTH), same
 * site ids (QIL_EINVAL_SITES); bonds and dtypes (f64 / c64) are free.  Chains whose bonds are all <= 16 take
 * one launch (the whole walk in one workgroup), the others two f64-MFMA GEMMs per site.                     */
QIL_API int qil_inner(const qil_mps* phi, const qil_mps* psi, double* out);
/* <phi|W psi> without materialising W psi: the same number as qil_inner(phi, qil_apply(W, psi)).
 * (W, psi) pass the checks of qil_apply; phi is checked against psi as in qil_inner.                       */
QIL_API int qil_apply_inner(const qil_mps* phi, const qil_mpo* W, const qil_mps* psi, double* out);
/* norm(W psi) without materialising W psi: the same number as qil_norm(qil_apply(W, psi))
 * (without amplitude, as qil_norm / mps.jl:754-771).  (W, psi) pass the checks of qil_apply.              */
QIL_API int qil_apply_norm(const qil_mpo* W, const qil_mps* psi, double* out);
/* ------------------------------------------------------------------ environments (no reference counterpart) */
/* The partial contraction the overlap verbs carry and never return: E[p, a, s], the contraction of `count` tensors of
 * <phi|psi> (W null: a has extent 1) or <phi|W|psi> with the bond legs left open -- p the bond of phi, a of W, s of psi.  The
 * conventions are qil_apply_inner's: the bra is conj(phi) and contracts the operator's s_out, the ket psi contracts s_in.
 * QIL_ENV_LEFT walks tensors 1 .. count, the open legs are the bonds to the right of tensor `count`; QIL_ENV_RIGHT walks tensors
 * n - count + 1 .. n, the open legs are the bonds to their left.  The amplitudes are NOT applied, as in qil_norm: count = n
 * gives <phi|psi> or <phi|W psi> divided by amp_phi amp_psi, count = 0 gives [1].
 * dims (three values) always receives (p, a, s).  out null: the size query, nothing else happens.  Otherwise out (host) receives p a s
 * interleaved complex doubles, column-major [p, a, s], whatever the operand dtypes (all f64 / c64 mixes, contracted in c64 when
 * any operand is complex).  The operands pass the checks of qil_inner (W null) or qil_apply_inner; for paired (ZTMPS) chains
 * `count` counts tensors of the 2n chain, and n above is that chain's length.
 * Routes: "chain", possible while both state bonds over the walked tensors are <= 16 and the operator's are
 * <= QIL_ENV_CHAIN_MAX_OP_BOND: one launch, one workgroup, the environment in LDS for the whole walk in either direction;
 * "gemm": the per-site f64-MFMA products of qil_inner / qil_apply_inner, on mirrored site copies for QIL_ENV_RIGHT, any bonds.
 * The chain route is taken where it fits; QIL_ENV_ROUTE=chain / gemm forces one (read per call; the chain only where it fits).
 * Errors, before the context is activated: QIL_EINVAL_ARG ("environment: null argument") for a null phi, psi or dims,
 * QIL_EINVAL_ARG for a side that is neither 0 nor 1 and for a count outside [0, n]; then the operand errors of qil_inner /
 * qil_apply_inner.  Every temporary belongs to the call; a failed call leaves nothing behind.                              */
#define QIL_ENV_LEFT  0
#define QIL_ENV_RIGHT 1
#define QIL_ENV_CHAIN_MAX_OP_BOND 8   /* two ping-pong blocks of 2 * 16 * 8 * 16 c64 and one site's operands: 148 of 160 KiB of LDS */
QIL_API int qil_environment(const qil_mps* phi, const qil_mpo* W, const qil_mps* psi, int side, int64_t count, double* out,
                            int64_t* dims);
/* Which route a qil_environment call takes: THE decision, not a copy of it -- qil_environment switches on the value this function
 * returns.  Host only: no context, no GPU.  side, count: as in the call; phi_dims, psi_dims: the n + 1 bond dimensions of the two
 * states, edges included; op_dims: the operator's, or null without one.  *route: 0 = the one-workgroup chain, 1 = the per-site
 * GEMMs.  Only the bonds of the walked tensors count; QIL_ENV_ROUTE is honoured.  QIL_EINVAL_ARG for a null pointer, a side that
 * is neither 0 nor 1 or a count outside [0, n].  (Declared here, beside the verb: the symbol set of qilaplace_hip_testing.h is
 * pinned by tests/test_cabi_symbols.py.) */
QIL_API int qil_environment_route(int side, int64_t count, int64_t n, const int64_t* phi_dims, const int64_t* psi_dims,
                                  const int64_t* op_dims, int* route);
/* ------------------------------------------------------------------ linear solver (no reference counterpart) */
/* Solves (A + shift I) x = c for A + shift I Hermitian positive definite, by the alternating two-site solver (ALS / DMRG for
 * linear systems) with a conjugate-gradient local solve.  HERMITICITY IS THE CALLER'S PROMISE: it cannot be checked cheaply and
 * is not; a non-Hermitian operator gives a wrong answer, not an error.  (A, c) pass the checks of qil_apply; x0, the initial
 * guess, may be null (a clone of c, compressed to maxdim where it is wider) and otherwise passes the checks of qil_inner against
 * c.  Single-register and paired chains (their 2n tensors) both work; every f64 / c64 mix is accepted, and the contraction and
 * the result are c64 when any operand is complex.  The solve runs on the tensors; *out carries c's amplitude (the solver factors
 * no scalar out of the tensors: the weight sits in the first tensor), so that qil_mps_to_vector(*out) is the solution.
 * Per bond k and half-sweep (a full sweep goes left to right, then right to left): the local right-hand side
 * g = Lc c_k c_{k+1} Rc and the local operator H v = L_A A_k A_{k+1} R_A v + shift v are formed from environments that are
 * updated one tensor at a time; CG runs from the current two-site tensor until |r| <= tol |g| or cg_iters iterations; the
 * result is split by the SVD under the project's truncation rule (drop the tail while the dropped weight <= cutoff * total,
 * at most maxdim, at least 1).  Each local step records |g - H y| / |g| before its CG; the verb stops after the first full
 * sweep whose largest such value is <= tol, or after max_sweeps (converged = 0; not an error: a truncation coarser than tol
 * keeps the value above tol).  With maxdim below the solution's rank and a right-hand side that does not compress, truncation
 * by SVD does not converge to the best approximation: the verb is for solutions that compress.
 * info (8 doubles, may be null): full sweeps done; converged (0 / 1); the largest pre-solve local residual of the last sweep;
 * matvecs in total; the largest bond of *out; local solves by the one-launch route; by the GEMM route; 0.
 * Routes of the local solve, per bond: "local", one launch of one workgroup with the whole CG in it, where
 * qil_mps_solve_local_fits says so (it fits the LDS and is small enough to win); "gemm", four f64-MFMA products per matvec and CG's scalars in device memory, any bonds.
 * QIL_SOLVE_ROUTE=local / gemm forces one (read per call; local only where the bond fits, else gemm, and info shows it).
 * Errors, before the context is activated: QIL_EINVAL_ARG for a null A, c or out, for maxdim, max_sweeps or cg_iters < 1, for
 * a shift, cutoff or tol that is not finite, for cutoff < 0 or tol <= 0; the operand errors of qil_apply and qil_inner;
 * QIL_EINVAL_LENGTH for a chain of one tensor (the two-site step needs a bond).  During the solve: QIL_EDOMAIN, "solve: operator
 * not positive definite on the local space (bond k)".  Every temporary belongs to the call; a failed call leaves nothing behind
 * and *out untouched. */
QIL_API int qil_mps_solve(const qil_mpo* A, double shift, const qil_mps* c, const qil_mps* x0 /* may be null */,
                          int64_t maxdim, double cutoff, double tol, int max_sweeps, int cg_iters,
                          qil_mps** out, double* info /* 8 doubles, may be null */);
/* Whether the local solve of a bond takes the one-launch route: THE decision, not a copy of it -- qil_mps_solve switches on this
 * value for every bond.  Host only: no context, no GPU.  complex_: the contraction type is c64; xl, xr: the outer bonds of x at
 * the two tensors; dl, dm, dr: the operator's three bonds there; cl, cm, cr: those of c.  *fits = 1 when the LDS the kernel needs,
 *     128 + e * (xl^2 dl + xr^2 dr + 4 dl dm + 4 dm dr + 12 xl xr + 2 blk) bytes,   e = 8 (f64) / 16 (c64),
 *     blk = max(4 xl xr max(dl, dm, dr), 2 xl cm, 4 xl cr)
 * (both environments, both operator tensors, y, r, p and two ping-pong blocks), is within 160 KiB, QIL_SOLVE_ROUTE is not
 * gemm, and -- unless QIL_SOLVE_ROUTE is local -- one matvec is at most 200000 multiply-adds,
 *     4 xl^2 xr dl + 8 xl xr dm (dl + dr) + 4 xl xr^2 dr,
 * the size up to which the one workgroup was measured to beat the GEMMs (MEASUREMENTS.md).  Growing a dimension never turns 0
 * into 1.  QIL_EINVAL_ARG for a null fits or a dimension < 1. */
QIL_API int qil_mps_solve_local_fits(int complex_, int64_t xl, int64_t xr, int64_t dl, int64_t dm, int64_t dr,
                                     int64_t cl, int64_t cm, int64_t cr, int* fits);
/* ------------------------------------------------------------------ extremal eigenpairs (no reference counterpart) */
/* The smallest (which = 0) or largest (which = 1, both algebraic) eigenpair of a Hermitian operator A in MPS form, by the
 * alternating two-site sweep of qil_mps_solve with the local linear solve replaced by a local eigenvalue solve (two-site DMRG).
 * Sweep structure, gauge handling and operand rules are those of qil_mps_solve: (A, x0) pass the checks of qil_apply, every
 * ortho[i] those of qil_inner against x0; single-register and paired chains (their 2n tensors) both work; every f64 / c64 mix is
 * accepted and the contraction and the result are c64 when any operand is complex.  x0, the start, is mandatory (this layer
 * invents no start vector): it is copied, widened, truncated to maxdim where it is wider and normalised; its amplitude is ignored.
 * A full sweep goes left to right, then right to left.
 * The local problem at bond k: H v = L_A A_k A_{k+1} R_A v + s weight sum_i g_i (g_i^H v), g_i = Lphi_i phi_i,k phi_i,k+1 Rphi_i
 * the projection of the deflation state ortho[i] onto the local space, s = +1 for which = 0 and -1 for which = 1: the penalty
 * pushes states found already away from the wanted end, so that a second call with the first result in `ortho` returns the next
 * eigenpair (ortho states should have norm 1 with their amplitude 1: the tensors alone enter; n_ortho <= 8).
 * The local solver is restarted Lanczos with full reorthogonalisation from the current two-site tensor y (unit norm): at most
 * `krylov` vectors (2 .. 16), each new one orthogonalised twice against all earlier ones, the tridiagonal projected matrix
 * diagonalised, the Ritz pair at the wanted end the next start, at most `restarts` times.  A restart begins with
 * theta = <y|H y> and r = H y - theta y and the iteration stops when |r| <= tol * scale or on a breakdown
 * (beta <= 1e-14 * scale: an invariant subspace, e.g. A = I).  scale is the largest |Ritz value| any local solve of this call
 * has seen, a lower bound of |A|_2 that Lanczos delivers for free (with deflation states only Ritz values at the wanted end count,
 * since the penalty moves the other end by up to `weight`); it keeps the test meaningful where theta ~ 0.  After the local solve
 * y is split by the SVD under the project's truncation rule (cutoff, maxdim), the kept singular values are rescaled to norm 1
 * and the sweep moves on.  The call ends after the first full sweep whose largest pre-solve |r| / scale is <= tol, otherwise after
 * max_sweeps with converged = 0, which is not an error.
 * *out has amplitude 1 and norm 1 (the weight sits in tensor 0); its phase is not fixed.  *theta is the Rayleigh quotient of the
 * last local solve, of the PENALISED local operator: with deflation states it is <x|A|x> + s weight sum_i |<ortho_i|x>|^2, and the
 * last term is the square of how far *out is from orthogonal to them (rounding level for converged, well separated pairs).  info (8 doubles, may be null): full sweeps done; converged (0 / 1); the largest pre-solve |r| / scale of the
 * last sweep; matvecs; the largest bond of *out; local solves by the one-launch route; by the GEMM route; scale.
 * Routes of the local solve, per bond: "local", one launch of one 256-thread workgroup with the whole restarted iteration in LDS,
 * where qil_mps_eigs_local_fits says so; "gemm", four f64-MFMA products per matvec, the basis in device memory, the vector steps
 * and the projected problem as small kernels, one read-back of the flags per restart, any bonds.  QIL_EIGS_ROUTE=local / gemm
 * forces one (read per call; local only where the bond fits, else gemm, and info shows it).
 * THREE LIMITS.  (1) HERMITICITY IS THE CALLER'S PROMISE: it cannot be checked cheaply and is not; a non-Hermitian operator
 * gives a wrong answer, not an error.  (2) The sweep converges to an eigenvector, NOT PROVABLY THE EXTREMAL ONE: an eigenvector
 * of small bond is a fixed point.  For circulant operators (shift, FIR, the periodic Laplacian) every Fourier mode is one: a numpy
 * restatement started from a random bond-2 state on I + 4 L at n = 8 stopped 9 % of |A| from lambda_min with a residual of 1e-13.
 * For those operators the spectrum is top_k of the transfer function's magnitude.  (3) CLUSTERED ENDS CONVERGE SLOWLY: the small
 * end of a random Gram operator, with relative gaps of 1e-8, did not converge in 10 sweeps in the restatement.
 * Errors, before the context is activated: QIL_EINVAL_ARG for a null A, x0, out or theta, a `which` that is not 0 / 1, n_ortho
 * outside 0 .. 8, a null ortho or entry with n_ortho > 0, krylov outside 2 .. 16, restarts < 1, maxdim or max_sweeps < 1, a
 * weight, cutoff or tol that is not finite, weight < 0, cutoff < 0 or tol <= 0; the operand errors of qil_apply for (A, x0) and
 * of qil_inner for (ortho[i], x0); QIL_EINVAL_LENGTH for a chain of one tensor.  During the call: QIL_EDOMAIN for a zero or
 * non-finite x0 and for a Ritz value that is not finite (the message names the bond).  Every temporary belongs to the call; a
 * failed call leaves nothing behind and *out and *theta untouched. */
QIL_API int qil_mps_eigs(const qil_mpo* A, int which /* 0 smallest, 1 largest (algebraic) */,
                         const qil_mps* x0, const qil_mps* const* ortho /* may be null */, int n_ortho, double weight,
                         int64_t maxdim, double cutoff, double tol, int max_sweeps, int krylov, int restarts,
                         qil_mps** out, double* theta, double* info /* 8 doubles, may be null */);
/* Whether the local eigen-solve of a bond takes the one-launch route: THE decision, not a copy of it -- qil_mps_eigs switches on
 * this value for every bond.  Host only: no context, no GPU.  complex_: the contraction type is c64; xl, xr: the outer bonds of
 * x at the two tensors; dl, dm, dr: the operator's three bonds there; krylov, n_ortho: as in the call.  *fits = 1 when the LDS the
 * kernel needs,
 *     128 + 4608 + e * (xl^2 dl + xr^2 dr + 4 dl dm + 4 dm dr + (krylov + 1 + n_ortho) * 4 xl xr + 2 * 4 xl xr max(dl, dm, dr))
 * bytes, e = 8 (f64) / 16 (c64) (the reduction scratch, the projected problem, both environments, both operator tensors, the
 * Krylov basis, the work vector, the projected deflation states and two ping-pong blocks), is within 160 KiB, krylov <= 16,
 * n_ortho <= 8, QIL_EIGS_ROUTE is not gemm, and -- unless QIL_EIGS_ROUTE is local -- one matvec is at most 200000 multiply-adds,
 *     4 xl^2 xr dl + 8 xl xr dm (dl + dr) + 4 xl xr^2 dr
 * (MEASUREMENTS.md).  Growing any argument never turns 0 into 1.  QIL_EINVAL_ARG for a null fits, a dimension < 1, krylov < 1
 * or n_ortho < 0. */
QIL_API int qil_mps_eigs_local_fits(int complex_, int64_t xl, int64_t xr, int64_t dl, int64_t dm, int64_t dr,
                                    int krylov, int n_ortho, int* fits);
/* ------------------------------------------------------------------ time evolution (no reference counterpart) */
/* *out ~ exp(steps * tau * A) x0, tau = tau_re + i tau_im, for a Hermitian operator A in MPS form (the caller's promise, not
 * checked, as in qil_mps_eigs) by two-site TDVP, the projector-splitting integrator, on the sweep of qil_mps_solve and
 * qil_mps_eigs.  Operand rules are those of qil_apply; single-register and paired chains both work.  The contraction type is c64
 * when A or x0 is c64 or tau_im != 0, else f64; *out has that type, x0's kind and x0's site ids.
 * One step is a sweep left to right, then right to left.  At bond k the two-site tensor goes through exp(+tau/2 H2),
 * H2 = L_A A_k A_{k+1} R_A, and is split by the SVD under the project's truncation rule (maxdim, cutoff).  Unless the bond is the
 * last of its half sweep, the centre tensor that moves on then goes through exp(-tau/2 H1), H1 = L_A A_j R_A at the tensor the
 * centre now sits on: that tensor was advanced as part of bond k and will be advanced again as part of the next bond, so it is
 * taken back once.  The start: x0 is copied, widened, cut to maxdim where it is wider, with the centre at tensor 0.
 * Norm: every local exponential starts from v / |v| and reports |v| g, g the growth of the unit vector; the host sums the
 * logarithms.  The tensors of *out have norm 1 to rounding, out->amplitude = x0->amplitude * exp(sum log); what a truncation
 * drops enters the sum at its split.
 * The local exponential is a Lanczos exponential: a basis with full reorthogonalisation (each vector orthogonalised twice against
 * all earlier ones) from the unit start, at most `krylov` vectors (2 .. 16); after every vector from the second on the tridiagonal
 * T_m is diagonalised, c = exp(delta T_m) e_1 with delta the remaining local time, est = beta_m |c_m| / |c|.  A pass ends when
 * est <= tol, when beta_m <= 1e-14 scale (the space is invariant and the result exact; also at m = 1; scale = the largest
 * |alpha|, beta of this exponential) or at m = krylov.  There, with est > tol and passes left (at most `substeps` passes), delta is
 * halved, at most 30 times, until est <= tol (the small exponential alone, no matvec), the vector advances by that part and the
 * next pass takes the rest.  The last permitted pass takes all that remains and the call reports converged = 0, which is not an
 * error.
 * Routes, per local exponential: "local", one launch of one 256-thread workgroup with every pass in LDS, where
 * qil_mps_evolve_local_fits says so; "gemm", four (two-site) or three (one-site) f64-MFMA products per matvec, the basis in device
 * memory, the vector steps as small kernels, every launch of a pass issued and a no-op behind the stop, one read-back per pass.
 * QIL_EVOLVE_ROUTE=local / gemm forces one (read per call; local only where the tensor fits).
 * WHAT THE ERROR IS.  With every bond of x0 at its full value the step is exact to N_loc * tol, N_loc = steps (4 n - 6); an
 * eigenvector of small bond and any state under a sum of one-site terms are evolved exactly.  A start narrower than the bonds it
 * grows to costs first order in tau once (from the first sweep alone).  The error with a binding maxdim is the projection error
 * and does not fall with the step.
 * THE STIFF LIMIT.  The backward one-site step is exp(-tau/2 H1): for Re tau < 0 it amplifies rounding by
 * exp(|Re tau| / 2 * spread(A)).  On the periodic Laplacian (spread 4) a numpy restatement reached 4e-13 at tau = -1.25, 6e-12
 * at -2.5, 4e-10 at -5 and returned garbage (error 1e12) at tau = -20 in one step.  The verb is for |Re tau| * spread(A) of order
 * one per step and for any imaginary tau; strong smoothing stays with qil_mps_solve (implicit) and the Fourier route.  info[8]
 * reports the exponent met.
 * info (10 doubles, may be null): steps done; converged (1 when every local exponential met tol); the worst accepted estimate;
 * matvecs; the largest bond of *out; exponentials by the one-launch route; by the GEMM route; passes beyond the first; the
 * largest |Re tau| / 2 * (theta_max - theta_min) over the Ritz values of the one-site steps; the sum of the logarithms.
 * Errors, before the context is activated, in this order: QIL_EINVAL_ARG for a null A, x0 or out; steps, maxdim or substeps < 1;
 * krylov outside 2 .. 16; a tau, cutoff or tol that is not finite; cutoff < 0 or tol <= 0; tau = 0; the operand errors of
 * qil_apply; QIL_EINVAL_LENGTH for a chain of one tensor.  During the call: QIL_EDOMAIN for a zero or non-finite start and for a
 * Lanczos coefficient that is not finite (the message names the bond).  Every temporary belongs to the call; a failed call leaves
 * nothing behind and *out untouched. */
QIL_API int qil_mps_evolve(const qil_mpo* A, const qil_mps* x0, double tau_re, double tau_im, int steps,
                           int64_t maxdim, double cutoff, double tol, int krylov, int substeps,
                           qil_mps** out, double* info /* 10 doubles, may be null */);
/* Whether a local exponential takes the one-launch route: THE decision, not a copy of it -- qil_mps_evolve switches on this value
 * for every two-site and one-site step.  Host only: no context, no GPU.  sites = 2: xl, xr the outer bonds of x at the two
 * tensors, dl, dm, dr the operator's three bonds there.  sites = 1: xl, xr, dl, dr the bonds at the one tensor, dm is ignored.
 * *fits = 1 when the LDS the kernel needs,
 *     sites = 2:  128 + 4736 + e * (xl^2 dl + xr^2 dr + 4 dl dm + 4 dm dr + (krylov + 1) * 4 xl xr + 2 * 4 xl xr max(dl, dm, dr))
 *     sites = 1:  128 + 4736 + e * (xl^2 dl + xr^2 dr + 4 dl dr + (krylov + 1) * 2 xl xr + 2 * 2 xl xr max(dl, dr))
 * bytes, e = 8 (f64) / 16 (c64) (the reduction scratch, the small area, both environments, the operator tensor or tensors, the
 * Krylov basis, the work vector and two ping-pong blocks), is within 160 KiB, krylov <= 16, QIL_EVOLVE_ROUTE is not gemm, and --
 * unless QIL_EVOLVE_ROUTE is local -- one matvec is at most 200000 multiply-adds,
 *     sites = 2:  4 xl^2 xr dl + 8 xl xr dm (dl + dr) + 4 xl xr^2 dr
 *     sites = 1:  2 xl^2 xr dl + 4 xl xr dl dr + 2 xl xr^2 dr
 * (the solver's rule; the one-launch route measured 2.1 to 1.08 times faster than the GEMM route wherever it fits, x bond 4 to
 * 16, operator bond 2 to 5, so no shape class is excluded: MEASUREMENTS.md section 32).  Growing any argument never turns 0
 * into 1, and for dm >= min(dl, dr) sites = 1 fits wherever sites = 2 does
 * (every term of both formulas is then no larger).  QIL_EINVAL_ARG for a null fits, sites not 1 or 2, a dimension < 1 or
 * krylov < 1. */
QIL_API int qil_mps_evolve_local_fits(int complex_, int sites /* 1 or 2 */, int64_t xl, int64_t xr,
                                      int64_t dl, int64_t dm /* ignored for sites == 1 */, int64_t dr,
                                      int krylov, int* fits);
/* Schmidt spectra of every bond (ITensors' svd(...).spec at every cut; no entry of the reference returns them).  S_out: host,
 * sum_k bond_k doubles; bond k (k = 1 .. N - 1 in tensor order, interleaved for paired chains) owns the bond_k slots that start
 * at the sum of the earlier bond dimensions, as qil_mps_bond_dims reports them at the time of the call.  Each block holds the
 * Schmidt values of the NORMALISED state at that cut in descending order (their squares sum to 1); slots beyond what the cut
 * can carry (non-minimal or rank-deficient bonds) are exact zeros.  The accuracy is absolute, a modest multiple of
 * N chi eps on the unit scale; relative accuracy of tiny values is not promised (the QR sweeps do not preserve it).
 * norm_out (nullable): |psi| without the amplitude, the number qil_norm returns, from the logarithms of what the sweep divides
 * out -- finite also where |psi|^2 is outside the double range.  psi is not modified: the work happens on a clone in pool
 * memory.  N = 1: no bonds, S_out is not written (may be NULL), norm_out is.
 *   route     exact right-orthonormal gauge of the clone, then a left-to-right sweep of thin QRs that keeps the triangular carry
 *             of every bond; the singular values of all carries in ONE launch (one workgroup per bond, values-only one-sided
 *             Jacobi in LDS) while the bond is <= 138 (f64) / 97 (c64); larger bonds, and any whose iteration reaches its
 *             sweep cap, through the one-matrix SVD.  QIL_SPECTRA_ROUTE=svd (read on each call) sends every bond there.
 *   syncs     the packed values, the logarithms and the per-bond flags come back in one read-back at the end; before it the call
 *             reads one flag back (a zero or non-finite site, ahead of the gauge sweep), and every QR step of the two sweeps
 *             reads its orthonormality measure.
 * Errors: QIL_EINVAL_ARG "bond_spectra: null argument" (psi, or S_out with N > 1); QIL_EDOMAIN "bond_spectra: zero or
 * non-finite state" for a site or a carry that is exactly zero or holds a non-finite entry -- a state that vanishes only by
 * cancellation between non-zero sites is reported so when its carry comes out exactly zero; otherwise the call returns the
 * spectrum of the rounding residue with a norm_out at rounding level of the sites' scale.  QIL_ENOMEM leaves nothing allocated. */
QIL_API int qil_bond_spectra(const qil_mps* psi, double* S_out, double* norm_out);
/* The same for an operator: the operator-Schmidt values of W / |W|_F at every bond (physical block 4 wide), layout by
 * qil_mpo_bond_dims; norm_out (nullable) receives |W|_F.                                                              */
QIL_API int qil_mpo_bond_spectra(const qil_mpo* W, double* S_out, double* norm_out);

/* ------------------------------------------------------------------ element-wise products, adjoints (no reference counterpart) */
/* The element-wise (Hadamard) product out_x = (conj?)(phi_x) psi_x, materialised: amplitude amp_phi * amp_psi, dtype
 * promote(phi, psi), psi's site ids and paired flag, bonds chi_phi * chi_psi.  Site tensors in the fused layout of qil_apply
 * with phi in the operator's place,
 *   C_i[(a, alpha), s, (b, beta)] = phi_i[a, s, b] psi_i[alpha, s, beta],   row = alpha + chi_l a,  col = beta + chi_r b,
 * element for element what qil_apply(qil_mpo_diagonal(phi), psi) writes (for amp_phi = 1, which the diagonal operator folds
 * into its first tensor).  conj_phi != 0 conjugates phi.  One grouped launch for all sites, HBM-store bound.
 * phi and psi: same context, same paired flag (QIL_EINVAL_ARG), same number of sites (QIL_EINVAL_LENGTH), same site ids
 * (QIL_EINVAL_SITES), all checked before the context is activated; bonds and dtypes (f64 / c64) are free.            */
QIL_API int qil_hadamard(const qil_mps* phi, int conj_phi, const qil_mps* psi, qil_mps** out);
/* diag(phi) as an MPO with phi's bonds, site ids, paired flag and dtype: W_i[a, s', s, b] = delta_{s s'} (conj?)(phi_i[a, s, b]),
 * the amplitude multiplied into the first tensor (MPOs carry none).  The door from states to every verb that takes an
 * operator: qil_apply_compress(diag(phi), psi) is the truncated product that never forms the (chi_phi chi_psi)^2 tensors;
 * qil_apply_coefficient_batch, qil_apply_inner and qil_apply_norm read phi (.) psi without forming it.  One launch.   */
QIL_API int qil_mpo_diagonal(const qil_mps* phi, int conj_phi, qil_mpo** out);
/* W^dagger: out_i[a, s', s, b] = conj(W_i[a, s, s', b]); same bonds, site ids, paired flag and dtype.  Only moves and sign
 * flips, so the result is exact and the adjoint of the adjoint is W bit for bit.  The adjoint of the QFT MPO is the inverse
 * transform (to the unitarity its build cutoff leaves: 3e-9 ... 3e-7 at cutoff = 1e-14, n = 6 ... 10).  One launch.    */
QIL_API int qil_mpo_adjoint(const qil_mpo* W, qil_mpo** out);
/* compress!(phi (.) psi; maxdim, tol, sweeps) without the product tensors: bit-identical to
 * qil_apply_compress(qil_mpo_diagonal(phi, conj_phi), psi, maxdim, tol, sweeps, zip_maxdim), with the diagonal operator a
 * temporary of the call (nothing but the result outlives it, also when an allocation fails midway).  Operand checks as
 * qil_hadamard, then the error codes of qil_apply_compress.                                                            */
QIL_API int qil_hadamard_compress(const qil_mps* phi, int conj_phi, const qil_mps* psi, int64_t maxdim, double tol, int sweeps,
                          int64_t zip_maxdim, qil_mps** out);

/* ------------------------------------------------------------------ linear combinations (no reference counterpart) */
/* out = sum_j c_j terms[j], materialised as the direct sum of the chains; nothing is truncated.
 *   coeffs    host memory, nb complex values as interleaved (re, im) doubles; null = all ones.
 *   terms     entries may repeat (psi + psi); repeated and zero-weight terms keep their block, so the structure of the result
 *             depends on the operands' shapes only.
 *   dtype     promote(terms); c64 as well when any coefficient has a non-zero imaginary part.
 *   metadata  site ids and paired flag of terms[0]; amplitude 1.0: the weights w_j = c_j * amplitude_j are multiplied into the
 *             first tensor's blocks (the way qil_mpo_diagonal folds its amplitude).
 *   bonds     every internal bond is sum_j chi_j.
 *   layout    term j occupies rows [off_l(j), off_l(j) + chi_l(j)) and columns [off_r(j), off_r(j) + chi_r(j)), offsets in
 *             term order: the first tensor is the row [w_1 A^1 | w_2 A^2 | ...] (1 x 2 x sum chi), the last tensor the column
 *             stack (sum chi x 2 x 1); for n = 1 the single tensor is sum_j w_j A^j.
 *   exactness interior and last tensors are copies: block entries equal the operand's bit for bit (a real operand of a c64
 *             result is widened with imaginary part +0.0), every off-block entry is exactly +0.0; only the first tensor
 *             carries one rounding, from the multiply by w_j.
 * One grouped launch writes all sites, every output element exactly once, zeros included: HBM-store bound like qil_hadamard.
 * Errors, all returned before the context is activated: QIL_EINVAL_ARG for a null terms / out / entry ("mps_sum: null
 * argument"), nb < 1, a non-finite coefficient, terms of different contexts or mixed paired flags; QIL_EINVAL_LENGTH for
 * different numbers of sites; QIL_EINVAL_SITES for different site ids (each term against terms[0], in that order).       */
QIL_API int qil_mps_sum(const qil_mps* const* terms, int64_t nb, const double* coeffs, qil_mps** out);
/* compress!(sum_j c_j terms[j]; maxdim, tol, sweeps); with a cap (maxdim) below sum chi, without the direct-sum tensors of
 * size (sum chi)^2: the terms are copied
 * and brought to right-canonical gauge by exact QRs, a zip-up sweep carries one environment per term (stored concatenated) and
 * builds a basis per bond with intermediate cap zip_maxdim (<= 0: the default of qil_apply_compress, max(maxdim + 16, maxdim +
 * ceil(maxdim / 8)); sketched on capped bonds), ONE variational sweep replaces every site by the best tensor given the others
 * (re-gauged at canonicalize!'s cutoff 1e-12: it stands in for the gauge pass compress! opens with), then the exact-gauge
 * compress! runs.  Where a concatenated bond fits under zip_maxdim the sweep takes the exact route's gauge step literally (the SVD
 * of the stacked operand at cutoff 1e-12); when every bond does -- small sums, calls without a cap -- the operands are read as
 * they are, no copy, no zip-up, and the bonds are those of qil_mps_sum + qil_compress.  Such a call saves the (sum chi)^2 site
 * tensors but not the work: its stacked operands are sum chi x 2 r' with r' up to sum chi, so an uncapped sum costs what
 * qil_mps_sum + qil_compress costs.  Two departures from a plain zip-up + QR-gauged sweep, both so that the bonds are those of
 * the exact route on decaying spectra too: this literal step, and the 1e-12 cutoff of the sweep.  The result has the post-conditions of compress!: bonds by the ITensors rule with cutoff
 * = tol^2 / ((N - 1) sweeps), unit-norm tensors, the norm in `amplitude`.  The per-term products of a step run in one grouped
 * f64-MFMA launch while every term's bond is <= 64 and the carried bond of the step <= 128, through the GEMM per term above that.  Nothing but the result outlives
 * the call, also when an allocation fails midway.  Operand checks as qil_mps_sum under the name "mps_sum_compress", then the
 * error codes of qil_apply_compress (QIL_EDOMAIN for n < 2, sweeps >= 1).  Accuracy against qil_mps_sum + qil_compress (the
 * exact route): identical bonds and a state error <= 2x the truncation's own on random operands (tests/test_gpu_sum.py).   */
QIL_API int qil_mps_sum_compress(const qil_mps* const* terms, int64_t nb, const double* coeffs, int64_t maxdim, double tol,
                                 int sweeps, int64_t zip_maxdim, qil_mps** out);

/* ------------------------------------------------------------------ operator algebra (no reference counterpart) */
/* out = sum_j c_j terms[j] for operators, materialised as the direct sum of the chains: the operator twin of qil_mps_sum, with
 * its promises.  coeffs, repeated and zero-weight terms, dtype (promote(terms), c64 when a coefficient has a non-zero imaginary
 * part), site ids and paired flag (of terms[0]) and bonds (sum_j D_j) as there; MPOs carry no amplitude, so w_j = c_j.
 *   layout    an MPO site [Dl, 2, 2, Dr] (column-major) is the MPS-shaped site [Dl, 2, 2 Dr] with column s_out + 2 b: term j
 *             occupies rows [off_l(j), off_l(j) + Dl(j)) and bond columns [off_r(j), off_r(j) + Dr(j)) -- columns
 *             [2 off_r(j), 2 off_r(j) + 2 Dr(j)) of the MPS-shaped site.  First tensor: the row of weighted blocks; interior:
 *             block-diagonal; last: the column stack; n = 1: the single tensor is sum_j c_j W^j.
 *   exactness as qil_mps_sum: interior and last tensors are copies bit for bit (+0.0 imaginary part for a widened real operand),
 *             every off-block entry is exactly +0.0, the first tensor carries the one rounding of the multiply.
 * The kernel is qil_mps_sum's (its site table with doubled column counts; four physical slices on the last and the only site):
 * one grouped launch, every output element stored exactly once, zeros included, no memset.
 * Errors, all returned before the context is activated, in qil_mps_sum's order under the name "mpo_sum": QIL_EINVAL_ARG for a
 * null terms / out / entry, nb < 1, a non-finite coefficient, different contexts or paired flags; QIL_EINVAL_LENGTH;
 * QIL_EINVAL_SITES (each term against terms[0]).                                                                        */
QIL_API int qil_mpo_sum(const qil_mpo* const* terms, int64_t nb, const double* coeffs, qil_mpo** out);
/* The Frobenius overlap <V, W>_F = tr(V^dagger W) = sum_{x,y} conj(V[x,y]) W[x,y].  out: host, one complex double (re, im).
 * <W, W>_F = |W|_F^2 (qil_mpo_bond_spectra's norm_out squared); <I, W>_F = tr W; <F, F>_F / 2^n = 1 for a unitary F.
 * V and W: same context, same paired flag (QIL_EINVAL_ARG), same number of sites (QIL_EINVAL_LENGTH), same site ids
 * (QIL_EINVAL_SITES), after the null check ("mpo_inner: null argument") and before the context is activated; bonds and dtypes
 * are free, mixed dtypes contract in c64.  V and W are not modified; every temporary is returned to the pool.
 * Routes, as qil_inner with four physical slices per site: two f64-MFMA GEMMs per site at any bonds (T = E W_i, pl x 4 sr;
 * E' = V_i^H T, V_i as (4 pl) x pr), or the whole walk in one launch of one workgroup (E and one slice of T in LDS, bonds of
 * both chains <= 64).  Auto: the one launch while both chains' bonds are <= 12, the measured crossover at n = 24 (past it the
 * one workgroup loses to the GEMMs in f64, past 20 in c64 too: at D = 64 it is 40x slower; MEASUREMENTS.md section 26).
 * QIL_MPO_INNER_ROUTE=chain|gemm, read per call, forces a route; chain only where the bonds fit.  Integer-valued operands whose partial sums stay below 2^53 give the exact integer on both routes. */
QIL_API int qil_mpo_inner(const qil_mpo* V, const qil_mpo* W, double* out);

/* ------------------------------------------------------------------ restriction (no reference counterpart) */
/* The MPS-valued counterpart of qil_mps_block: spec (host, n_tensors bytes, the vocabulary and layout of qil_mps_block's spec)
 * fixes a site's bit (0 / 1), sums the site (2) or keeps it (3); out is the chain of the KEPT tensors, in order -- one damping
 * row or frequency column of a z-plane, a zoom window (high bits fixed), a decimated signal (low bits fixed), the copy-register
 * marginal -- ready for every verb that takes a state, at sizes where no dense block fits.
 *   removed   a fixed site contributes S_i = A_i[:, b, :], a summed site S_i = A_i[:, 0, :] + A_i[:, 1, :] (slice 0 + slice 1);
 *             a maximal run p..q of removed sites contributes M = S_p ... S_q (chi_{p-1} x chi_q).
 *   absorbed  into the kept tensor on the run's right, A'_k = M A_k with A_k viewed as chi_l x 2 chi_r.  A leading run is a row
 *             vector.  A trailing run (no kept tensor on its right) is a column vector c and goes into the last kept tensor
 *             from the right, A'_k[:, s] = A_k[:, s, :] c.
 *   order     (it fixes the rounding) M = ((S_p S_p+1) S_p+2) ..., left to right, leading runs included; c = S_p (S_p+1 (... S_q)),
 *             right to left; a last kept tensor that takes both is M (A_k c).  A run of length 1 is not formed: its slice is
 *             read in place from the removed site's tensor, the sum of a summed site made in the operand load.
 *   result    psi's dtype and amplitude (tensors are not renormalised: qil_norm(out) * amplitude is the 2-norm of the slice), the
 *             kept sites' ids; internal bonds = the parent's right bonds of the kept sites but the last.  paired = 1 iff psi is
 *             paired and the kept tensors are whole (main_i, copy_i) pairs, otherwise a plain chain.
 *   exactness a kept tensor that absorbs nothing is a bit-for-bit copy (spec all 3: a bit-identical clone); results are
 *             bit-identical from run to run.
 * One grouped f64-MFMA launch writes all kept sites, copies included, every output element once.  Runs of length >= 2 and
 * trailing runs are multiplied in one further launch, one workgroup per run with the running product in LDS, while every bond
 * the run touches is <= 96 (f64) / 64 (c64): two buffers of chi^2 elements within the 160 KiB of a CU; wider runs go through the
 * GEMM with summed sites materialised, as in qil_mps_block.  One call may mix the routes; their roundings differ.
 * Nothing but the result outlives the call, also when an allocation fails midway.
 * Errors: QIL_EINVAL_ARG ("mps_restrict: null argument") for a null psi, spec or out, before the context is activated; then
 * QIL_EINVAL_CONFIG for a spec value above 3 and for a spec that keeps no site (that number is what qil_coefficient_batch /
 * qil_coefficient_marginal_batch return).
 * Deliberately not here: the lazy form (a slice of W psi without forming it), a batch of specs in one call, Born marginals
 * (tracing a site in |psi|^2).                                                                                            */
QIL_API int qil_mps_restrict(const qil_mps* psi, const uint8_t* spec, qil_mps** out);

/* ------------------------------------------------------------------ operator read-outs (no reference counterpart) */
/* Rows, columns, diagonals and entries of an operator on its own bonds, O(n D^2) per number: no basis state, no qil_apply and
 * no product of bond chi D is formed.  A spec gives two bytes per tensor, (in_i, out_i), for the legs of W_i[a, s_in, s_out, b]:
 *   0 / 1     fixes the leg's bit;  2 sums the leg;  3 keeps it (qil_mpo_slice only);
 *   (4, 4)    traces the site, sum_s W_i[:, s, s, :];  (5, 5) keeps its diagonal, A[:, s, :] = W_i[:, s, s, :] (qil_mpo_slice
 *             only).  4 and 5 tie the legs and must stand in both bytes of a site.
 * Slice (s_in, s_out) of a site is the D_l x D_r matrix at offset D_l (s_in + 2 s_out) with leading dimension 4 D_l.
 *   removed   a site that keeps no leg is the D_l x D_r factor S_i, the sum of 1, 2 or 4 slices added in ascending
 *             s_in + 2 s_out, left-associated, in the operand load; no S_i goes to HBM on the LDS routes.
 *   kept      a site that keeps exactly one leg (3 in exactly one byte, or (5, 5)) is the MPS-shaped tensor whose slice s is one
 *             slice of W_i, or the sum of two where the other leg is summed.
 *
 * qil_mpo_entry_batch: out[r] = prod_i S_i(r) for nb rows; spec: host, nb x n_tensors x 2 bytes, row-major; out: host, nb complex
 * values (re, im) for either dtype -- a real operator is contracted in real arithmetic and gives an imaginary part of exactly
 * zero.  Allowed are 0, 1, 2 and (4, 4): all-fixed rows are the entries W[in, out], 2 gives row sums, column sums and the sum
 * of all entries, (4, 4) partial traces and the trace.  In exact arithmetic row r depends on (W, row r) only; its rounding
 * depends on the route, and the route auto takes depends on nb (below).
 * Routes: "chain", possible while every bond is <= QIL_MPO_ENTRY_CHAIN_MAX_BOND: one launch, one workgroup per row, the carry a
 * row vector in LDS (two buffers), v <- v S_i left to right.  "gemm", at any bonds: per tensor one f64-MFMA GEMM of the
 * nb x D_l carry with the site as the plain D_l x 4 D_r matrix it is in memory, and a kernel that adds each row's slices of the
 * product (qil_product_batch's second route with four slices), rows in chunks under 64 MiB of temporaries.  That route adds
 * the slices AFTER the product, so its rounding differs from the chain's.
 * Bits: on the chain route, forced or chosen, a row's result is bit-identical alone, in any batch, and from run to run.  On
 * the gemm route it is bit-identical from run to run for the same batch.  Under auto the same row may take the chain in a small
 * batch and the GEMMs in a large one; force a route where bits must not depend on nb.
 * Auto: the chain while every bond is <= 64 and nb * bond^2 < 2^21 (bond: the widest), the GEMMs otherwise -- the measured
 * crossover at 24 tensors, chain / gemm in ms (f64): 64 rows, bond 16: 0.09 / 0.21, bond 64: 0.25 / 0.22, bond 96: 0.47 / 0.23,
 * bond 512: 5.0 / 0.39; 1024 rows, bond 32: 0.17 / 0.25, bond 64: 0.34 / 0.27; 4096 rows, bond 16: 0.31 / 0.40, bond 32:
 * 0.44 / 0.52, bond 64: 1.02 / 0.62, bond 512: 12.3 / 3.8 (c64 alike, MEASUREMENTS.md section 27).  Every workgroup of the
 * chain streams the whole operator, so the rule keeps it to the calls it wins or loses by less than a quarter.
 * QIL_MPO_ENTRY_ROUTE=chain|gemm, read per call, forces a route; chain only where the bonds fit.  Integer-valued operands
 * whose partial sums stay below 2^53 give the exact integer on both routes.
 * Errors, all before the context is activated: QIL_EINVAL_ARG ("mpo_entry_batch: null argument") for a null W or, when nb > 0,
 * a null spec or out; QIL_EINVAL_ARG for nb < 0; QIL_EINVAL_CONFIG for a value 3, 5 or above 5 and for a 4 that is not in both
 * bytes of its site (the message names the row and the tensor).  nb = 0 is a no-op.  Nothing but `out` outlives the call, also
 * when an allocation fails midway.                                                                                          */
QIL_API int qil_mpo_entry_batch(const qil_mpo* W, int64_t nb, const uint8_t* spec, double* out);
/* qil_mpo_slice: the chain of the KEPT tensors of spec (host, n_tensors x 2 bytes), a state: a column of W (in fixed, out kept:
 * W applied to a basis state), a row (out fixed, in kept: the functional that produces one transform value), the diagonal (all
 * (5, 5): the inverse of qil_mpo_diagonal), W applied to the all-ones signal (in summed, out kept), and every mixture.  Runs of
 * removed sites are absorbed exactly as in qil_mps_restrict: an interior or leading run p..q goes into the kept tensor on its
 * right as M = ((S_p S_p+1) ...); a trailing run goes from the right into the last kept tensor as c = S_p (... S_q),
 * A'_k[:, s] = A_k[:, s, :] c; a last kept tensor that takes both is M (A_k c); runs of length 1 are read in place.
 *   result    W's dtype, amplitude 1.0, the kept sites' ids, bonds = the parent's right bonds of the kept sites but the last;
 *             paired = 1 iff W is paired and whole (main_i, copy_i) pairs are kept.
 *   exactness a kept tensor that absorbs nothing is the gather of W's slices bit for bit, where a leg is summed the one IEEE
 *             addition; results are bit-identical from run to run.
 * One grouped launch writes all kept tensors, every element exactly once; a kept tensor that absorbs a run is 16 x 16 f64-MFMA
 * tiles.  Runs of length >= 2 and trailing runs go in one further launch, one workgroup per run with the running product in
 * LDS, while every bond the run touches is <= 96 (f64) / 64 (c64): two buffers within the 160 KiB of a CU, the limits of
 * qil_mps_restrict; wider runs go through the GEMM with multi-term factors materialised.  One call may mix the routes; their
 * roundings differ.  Nothing but the result outlives the call, also when an allocation fails midway.
 * Errors, all before the context is activated: QIL_EINVAL_ARG ("mpo_slice: null argument") first; QIL_EINVAL_CONFIG for a value
 * above 5, for 4 / 5 in one byte of a site only, for a site (3, 3) ("keeps both legs: sub-operators are not built") and for a
 * spec that keeps no site ("that number is what mpo_entry_batch returns").
 * Deliberately not here: sub-operators (sites that keep both legs), the lazy form (a slice of a product of operators without
 * forming it), a device-resident out for the entries.                                                                     */
QIL_API int qil_mpo_slice(const qil_mpo* W, const uint8_t* spec, qil_mps** out);

/* ------------------------------------------------------------------ Born weights (no reference counterpart) */
/* Energy read-out: out[r] = amplitude^2 * sum over the configurations x that match row r of |psi_x|^2 -- the power in a
 * frequency band, the energy of one damping row of a z-plane, the probability that a bit is set.  spec (host, nb x n_tensors
 * bytes, row-major, the layout of qil_coefficient_marginal_batch's bits): 0 / 1 fixes the tensor's bit, 2 TRACES the site in
 * |psi|^2 (qil_coefficient_marginal_batch's 2 sums amplitudes; this sums their squares).  out: host, nb doubles.
 *   chain     rho_0 = [1]; a fixed site with bit b gives rho_i = A_b^H rho_{i-1} A_b with A_b = A_i[:, b, :]; a traced site
 *             rho_i = A_0^H rho_{i-1} A_0 + A_1^H rho_{i-1} A_1, the slice-0 term first; the result is amplitude^2 * Re rho_n.
 *   order     (it fixes the rounding) each term is A_s^H (rho A_s).  A leading run of fixed sites keeps rho at rank one: the row
 *             vector v <- v A_b is carried through it, as the coefficient chain does, and rho = v^H v is formed at the first
 *             traced site.  A row with no traced site gives |coefficient|^2, a row of all 2 gives (amplitude * norm)^2.  Nothing
 *             is rescaled along the way and the result is not clamped at 0.
 *   rows      row r depends on (psi, row r) only, not on nb or on the other rows.
 * Two routes, chosen from the state's bonds alone (never from the spec), so a given state always takes one route.  While every
 * bond is <= 80 (f64) / 48 (c64) one launch serves the batch, one workgroup per row, with rho, rho A_s and the next rho in LDS
 * and both products per slice on the f64 MFMA: three buffers of ld^2 elements and two vectors within the 160 KiB of a CU, ld =
 * 80 (f64: 154 880 B; = 16 mod 32 against bank conflicts of the 8-byte operand reads) or 48 (c64: 112 128 B; = 0 mod 16 for the
 * 16-byte reads); the next admissible ld, 112 / 64, does not fit.  On this route a row's result is bit-identical whether it is
 * computed alone or in any batch, and from run to run.  Wider states go through strided-batch GEMMs with rho per row in pool
 * memory, in chunks of rows under 64 MiB of temporaries; that route starts from rho_0 = [1] without the vector phase (the same
 * number in exact arithmetic) and its rounding may depend on the chunk.
 * Nothing but `out` outlives the call, also when an allocation fails midway.
 * Errors, all before the context is activated: QIL_EINVAL_ARG ("weight_batch: null argument") for a null psi or, when nb > 0, a
 * null spec or out; QIL_EINVAL_ARG for nb < 0; QIL_EINVAL_CONFIG for a spec value above 2 (a kept site makes no number).
 * nb = 0 is a no-op (out is not touched); a state of norm 0 gives zeros.
 * Left out: weights of operators, a device-resident out.  The lazy form on W psi is qil_apply_weight_batch, below.        */
QIL_API int qil_weight_batch(const qil_mps* psi, int64_t nb, const uint8_t* spec, double* out);
/* The same read-out on a transformed state, without forming it: out[r] = amplitude^2 * sum over the configurations x that
 * match row r of |(W psi)_x|^2, in exact arithmetic qil_weight_batch(qil_apply(W, psi), nb, spec, out).  spec and its values
 * 0 / 1 / 2 are qil_weight_batch's; amplitude is psi's.  The operand checks are qil_apply's; the contraction runs in c64 if
 * either operand is c64, a real operand being widened per site.  Every row has three parts, and its route through them
 * depends on the row's spec and the operands' shapes only:
 *   lead      the leading run of fixed sites carries the lazy row vector of qil_apply_coefficient_batch,
 *             M'[beta, b] = sum W[a, s', bit, b] M[alpha, a] A[alpha, s', beta], two strided-batch products per site.
 *   middle    at the row's first traced site E[alpha', a', a, alpha] = conj(M[alpha', a']) M[alpha, a]; every further site up
 *             to the tail runs the four products of qil_apply_norm (T1 = E A, T2 = T1 W, T3 = T2 conj(W), E' = A^H T3) for
 *             all rows of a chunk at once, with the s_out != bit half of T2 zeroed where the row fixes the site (ket and bra
 *             share the output leg, so one side carries the projector).
 *   tail      R_k[alpha', a', a, alpha], the right environment of |W psi|^2 with the sites k+1 .. n all traced (R_n = [1]),
 *             does not depend on the row: one right-to-left pass per call, the four products mirrored.  Kept are the R_k at
 *             which some row's trailing run of traced sites starts, from the right, while their total stays within 256 MiB
 *             (QIL_APPLY_WEIGHT_RENV_BYTES overrides the figure, read on each call; 0 keeps none); the pass itself holds two
 *             more buffers of the size of its largest intermediate.  A row stops at the first kept R_k of its trailing run and
 *             gives amplitude^2 Re sum E o R_k -- Re(m R_k m^H), m = vec(M), when it has no middle, so a prefix-fixed row (the
 *             blocks of a range, the steps of a quantile search) is a vector phase and one quadratic form.  A row with no kept
 *             R_k walks to the end as middle and gives Re E[0]; a row with no traced site gives |M|^2.  Each result is a
 *             fixed-order sum of one workgroup, without atomics.
 * Rows are processed in chunks under 64 MiB of per-row temporaries:
 *   chunk = max(1, min(nb, 32768, 64 MiB / ((2 maxMid + 2 maxM + maxX) e))),  e = 8 (f64) or 16 (c64) bytes, and over the sites
 *   (chi_l, chi_r the bonds of psi, D_l, D_r those of W)
 *   maxMid = max(chi_l^2 D_l^2, 2 chi_l D_l^2 chi_r, 2 chi_l D_l D_r chi_r, 2 chi_l D_r^2 chi_r, chi_r^2 D_r^2),
 *   maxM = max(chi_l D_l, chi_r D_r),  maxX = 2 chi_l D_r.
 * A result is bit-identical from run to run.  Its rounding may differ between chunkings (hence with nb and the other rows)
 * and between kept and not-kept R_k.  Nothing but `out` outlives the call, also when an allocation fails midway.
 * Errors, all before the context is activated: QIL_EINVAL_ARG ("apply_weight_batch: null argument") for a null W or psi or,
 * when nb > 0, a null spec or out; QIL_EINVAL_ARG for nb < 0; the operand errors of qil_apply; QIL_EINVAL_CONFIG for a spec
 * value above 2.  nb = 0 is a no-op (out is not touched).
 * Left out: weights of operators, a device-resident out.                                                                   */
QIL_API int qil_apply_weight_batch(const qil_mpo* W, const qil_mps* psi, int64_t nb, const uint8_t* spec, double* out);
/* Perfect sampling of a transformed state, without forming it: nb configurations x drawn with probability
 * |(W psi)_x|^2 / |W psi|^2, in exact arithmetic qil_sample(qil_apply(W, psi), nb, seed, uniforms, bits_out, prob_out).  bits_out
 * (host, nb x n_tensors bytes, the layout of qil_coefficient_batch: the rows go straight into qil_apply_coefficient_batch),
 * prob_out (nullable, host, nb doubles: |(W psi)_x|^2 / |W psi|^2), seed and uniforms are qil_sample's; the amplitude does not
 * enter.  The operand checks are qil_apply's; the contraction runs in c64 if either operand is c64, a real operand being
 * widened per site as in qil_apply_weight_batch.  W psi is never formed:
 *   environments  R_n = [1];  R_k[alpha', a', a, alpha], the right environment of |W psi|^2 with the tensors k+1 .. n traced, by
 *                 ONE right-to-left pass of the mirrored four-product step of qil_apply_norm (the pass of
 *                 qil_apply_weight_batch's tail).  Each R_k is scaled on the device by 1 / t_k, t_k = Re sum_{alpha, a}
 *                 R_k[alpha, a, a, alpha], and the pass goes on from the scaled R_k: only ratios matter afterwards, and a chain
 *                 of 48 tensors neither overflows nor underflows.  All R_k, k = 1 .. n - 1, are kept for the call:
 *                 e sum_k (chi_k D_k)^2 bytes, e = 8 (f64) or 16 (c64).  Above 16 GiB the call returns QIL_ENOMEM before it
 *                 allocates anything, the message naming the bytes needed; QIL_APPLY_SAMPLE_RENV_BYTES overrides the figure
 *                 (read on each call).  16 GiB is a stated condition, not a measurement: the natural zT operands at n = 24 need
 *                 about 0.4 GiB, the padded headline shapes (chi 64, D 128) 48 GiB, which the caller has to ask for.
 *   sweep         row r carries the lazy row vector M[alpha, a] of qil_apply_coefficient_batch, [1] at the start.  At tensor i
 *                 both children M_s (s = 0, 1) are that read-out's step with the output bit s,
 *                 M_s[beta, b] = sum W[a, s', s, b] M[alpha, a] A[alpha, s', beta], and q_s = Re(m_s R_{i+1} m_s^H) with
 *                 m_s = vec(M_s) in the index pairing of qil_apply_weight_batch's prefix-fixed rows (at the last tensor
 *                 q_s = |M_s|^2).  Then qil_sample's rule verbatim: s = 0 iff u_{r,i} (q_0 + q_1) < q_0, else s = 1;
 *                 M <- M_s / sqrt(q_s); the probability is multiplied by q_s / (q_0 + q_1).  If q_0 + q_1 <= 0 on a reached
 *                 prefix (rounding only), the larger q is taken, s = 0 when both are 0, and the probability factor is 0.
 *   uniforms      the caller's (host, nb x n_tensors, sample-major, each in [0, 1)), or when uniforms is null
 *                 u_{r,i} = (splitmix64(seed ^ splitmix64(r n + i)) >> 11) 2^-53, n = n_tensors.  Sample r depends only on
 *                 (W, psi, seed, r): not on nb, on the chunking of the rows or on the route, up to rounding at a threshold.
 * Rows are processed in chunks under 64 MiB of per-row temporaries (M, the next M, both children, their products with R_{i+1},
 * the step's X, the partial sums):
 *   chunk = max(1, min(nb, 32768, 64 MiB / ((5 maxM + maxX) e + 16 ceil(maxM / 64)))),  and over the tensors (chi_l, chi_r the
 *   bonds of psi, D_l, D_r those of W)  maxM = max(chi_l D_l, chi_r D_r),  maxX = 2 chi_l D_r.
 * Two routes form the q_s, each a fixed-order sum without atomics (QIL_APPLY_SAMPLE_ROUTE=fused / gemm forces one; unforced, the
 * operands' bonds alone decide, so a given (W, psi) always takes one route): gemm, R^H [M_0 M_1] as one product and a reduce
 * kernel; fused, an f64-MFMA kernel that keeps the products in registers and reads each tile of R once for both children.  The
 * gemm route measured faster or equal at every bond tried (chi D = 24, 504, 2048), so it is the unforced route at every bond.
 * A result is bit-identical from run to run.  Nothing but the outputs outlives the call, also when an allocation fails midway.
 * Errors, all before the context is activated: QIL_EINVAL_ARG ("apply_sample: null argument") for a null W or psi or, when
 * nb > 0, a null bits_out; QIL_EINVAL_ARG for nb < 0; the operand errors of qil_apply; QIL_EINVAL_CONFIG for a uniform outside
 * [0, 1); QIL_ENOMEM for the environment cap.  After it: QIL_EDOMAIN ("apply_sample: the transformed state has zero norm") when
 * a trace t_k is <= 0 or not finite.  nb = 0 is a no-op.
 * The environment pass, its budget (QIL_APPLY_SAMPLE_RENV_BYTES) and the scoring routes (QIL_APPLY_SAMPLE_ROUTE) are shared with
 * qil_apply_top_k below, the beam search on the same scoring step.
 * Left out: a device-resident output.                                                                                        */
QIL_API int qil_apply_sample(const qil_mpo* W, const qil_mps* psi, int64_t nb, uint64_t seed, const double* uniforms,
                             uint8_t* bits_out, double* prob_out);
/* Top-k coefficient search of a transformed state, without forming it: the k configurations x with the largest |(W psi)_x|,
 * their values and a bound on what the search may have dropped; in exact arithmetic
 * qil_top_k(qil_apply(W, psi), k, beam, bits_out, val_out, bound_out).  bits_out: host, k x n_tensors bytes, the layout of
 * qil_coefficient_batch (the rows go straight into qil_apply_coefficient_batch).  val_out: host, k complex (re, im), the numbers
 * qil_apply_coefficient_batch gives on those rows (psi's amplitude included), in descending |value| (equal magnitudes: the order
 * of the candidates).  bound_out: sqrt(largest key dropped before the last tensor) |W psi| |amp|, on the scale of the values;
 * 0 if nothing was dropped.  The result is certified to be the exact top-k when bound < |value_k| (1 - 1e-10), qil_top_k's slack.
 * The operand checks are qil_apply's; the contraction runs in c64 if either operand is c64.  W psi is never formed:
 *   environments  qil_apply_sample's: R_n = [1], R_k[alpha', a', a, alpha] by the mirrored four-product step, each scaled on the
 *                 device by 1 / t_k, t_k = Re sum R_k[alpha, a, a, alpha].  log |W psi|^2 = sum_{k=0}^{n-1} log t_k (t_0 = the trace
 *                 of the last step's one number) is kept on the device, added up in the order k = n - 1 .. 0 by one workgroup,
 *                 and read back with the outputs: a chain of 48 tensors with amplitude e^157 neither overflows nor underflows.
 *                 The budget is qil_apply_sample's: e sum_k (chi_k D_k)^2 bytes against 16 GiB or QIL_APPLY_SAMPLE_RENV_BYTES
 *                 (the same variable: the environments are the shared step), QIL_ENOMEM before anything is allocated.
 *   search        the frontier starts as one row, M = [1], g = 0, p = 1 (row r carries the lazy row vector M[alpha, a] of
 *                 qil_apply_coefficient_batch up to e^g, and p = its key).  At tensor i the children of every row are that
 *                 read-out's step with the output bit s, M_s[beta, b] = sum W[a, s', s, b] M[alpha, a] A[alpha, s', beta], and
 *                 q_s = Re(m_s R_{i+1} m_s^H), m_s = vec(M_s), in the index pairing of qil_apply_sample (at the last tensor
 *                 R = [1]: q_s = |M_s|^2); a q_s that rounding made negative, or a NaN, counts as 0.  Candidate 2 r + s has
 *                 key = p (q_s / (q_0 + q_1)), 0 when q_0 + q_1 <= 0.  The at most `beam` largest keys are kept (k at the last
 *                 tensor), ties at the cut going to the lower candidate 2 r + s; the next frontier is in candidate order;
 *                 the largest key dropped before the last tensor is recorded.  A kept row becomes M_s / sqrt(q_s) with
 *                 g' = g + log(q_s) / 2 and p' = key.  At the last tensor value = amp M_s e^g.
 * Memory.  Held for the whole frontier (at most min(2^(n-1), beam) rows): the rows, maxM e bytes each, both children, 2 maxM e,
 * and the per-row bookkeeping (keys, q_s, g, p, the selection, 4 bytes per tensor for the back-walk); over the tensors
 * maxM = max(chi_l D_l, chi_r D_r) and maxX = 2 chi_l D_r (chi the bonds of psi, D those of W), e = 8 (f64) or 16 (c64).  Hence
 *   beam <= min(2^29, 2^30 / (3 maxM e + 4 n + 64)),  n = n_tensors: a function of the operands' shapes alone, checked before
 *   the context is activated (1 GiB for the frontier; candidate indices stay below 2^30).
 * The children's steps (strided batches of at most 32768 rows), their product with R_{i+1} and the step's X run over chunks of
 * frontier rows under qil_apply_sample's 64 MiB of per-chunk temporaries:
 *   chunk = max(1, min(largest frontier, 32768, 64 MiB / ((2 maxM + maxX) e + 16 ceil(maxM / 64)))).
 * The keys of all 2 f candidates stay resident and the selection is over the whole candidate set.  Frontier sizes are
 * min(2^i, beam), known on the host: no count is read back, and the result is bit-identical from run to run.
 * Routes: the q_s through qil_apply_sample's two, chosen the same way (gemm unforced at every bond, QIL_APPLY_SAMPLE_ROUTE=fused /
 * gemm forces one), each the other's check; the selection is qil_top_k's radix select and compaction.
 * Nothing but the outputs outlives the call, also when an allocation fails midway.
 * Errors, all before the context is activated, in this order: QIL_EINVAL_ARG ("apply_top_k: null argument") for a null W or
 * psi; QIL_EINVAL_ARG for k < 0; for beam < k; the operand errors of qil_apply; QIL_EINVAL_ARG for beam above the cap; for
 * k > 2^n_tensors (n_tensors <= 62); k = 0 is a no-op (the outputs are not touched); QIL_EINVAL_ARG ("apply_top_k: null
 * argument") for a null output; QIL_ENOMEM for the environment budget.  After it: QIL_EDOMAIN ("apply_top_k: the transformed
 * state has zero norm") when a trace t_k is <= 0 or not finite.
 * Left out: a device-resident output, both children of the row step in one strided batch, a batch of (W, psi) pairs.         */
QIL_API int qil_apply_top_k(const qil_mpo* W, const qil_mps* psi, int64_t k, int64_t beam, uint8_t* bits_out, double* val_out,
                            double* bound_out);

/* ------------------------------------------------------------------ truncation (K1, K2) */
/* canonicalize!(psi, direction; center, cutoff=1e-12, maxdim) src/mps.jl:787-847.
 * center = 0 selects the default (N for :right, 1 for :left); 1-based otherwise.    */
QIL_API int qil_canonicalize(qil_mps* psi, int direction, int64_t center, double cutoff, int64_t maxdim);
/* compress!(psi; maxdim, tol=1e-12, sweeps=1) src/mps.jl:913-999.  In place.
 * Accuracy contract: same bond dimensions and amplitude as the reference's rule (cutoff = tol^2 / ((N-1) sweeps),
 * mps.jl:920; gauge passes at canonicalize!'s cutoff 1e-12), truncated state within 1e-9 of the CPU restatement's on
 * sampled coefficients (tests: test_compress_*, test_bench_truncate_operands_against_oracle).  One deliberate
 * deviation from "full SVD of every site": when a site's triangular factor is numerically rank-deficient (every
 * product bond before its truncation) the one-factor SVD first DROPS the rows of that factor whose summed squared
 * weight stays below 1e-6 of the caller's cutoff x |A|_F^2 and factors only the rest (svd_left_deflated).  A dropped
 * weight w costs sqrt(w) in amplitude, i.e. at most 1e-3 of what the cutoff itself is allowed to discard per site:
 * measured on the bond-1008 zT product (maxdim 64, tol 1e-8) the truncated state differs from the CPU restatement's
 * by 4e-10 of the scale with the rule and 1e-11 without it, against 1.8e-5 of truncation error of the algorithm
 * itself.                                                                                                            */
QIL_API int qil_compress(qil_mps* psi, int64_t maxdim, double tol, int sweeps);

/* zip_to_compress_mpo over a whole MPO, in place (src/transforms/dt_transformer.jl:167-288; the step the
 * reference runs on the MPO x MPO product in zt_transformer.jl:103-104).  direction 0 = "down" (exact gauge
 * sweep left -> right, truncating SVD sweep right -> left), 1 = "up" (mirror).  cutoff / maxdim follow the
 * ITensors truncation rule (maxdim <= 0: no cap).  QIL_EINVAL_ARG for any other direction (the reference's
 * `error("unknown direction")`).                                                                         */
QIL_API int qil_mpo_compress(qil_mpo* W, int direction, double cutoff, int64_t maxdim);

/* Batches of independent chains (the serial loops over signals / damping values of
 * scripts/benchmark/zt_full_runtime.jl:151-221 and docs/src/tutorials/zt.jl:300-348 call compress! /
 * zip_to_compress_mpo once per item).  Item j receives exactly qil_compress(items[j], ...) resp.
 * qil_mpo_compress(items[j], ...), in place; the nb chains run concurrently (each is a latency chain of small
 * factorisations that fills a few percent of the chip): up to 4 on streams of their own, larger batches as four lock-step
 * groups whose chains share ONE table launch per step; bit-identical to the item-by-item calls; the call
 * returns when all are done.  All items must live in one context and be distinct handles (QIL_EINVAL_ARG);
 * the first failing item's status is returned, the other items are still processed.                        */
QIL_API int qil_compress_batch(qil_mps* const* items, int64_t nb, int64_t maxdim, double tol, int sweeps);
QIL_API int qil_mpo_compress_batch(qil_mpo* const* items, int64_t nb, int direction, double cutoff, int64_t maxdim);

/* Fused apply-and-truncate: compress!(apply(W, psi); maxdim, tol, sweeps) (apply.jl:75-122 followed by
 * mps.jl:913-973) without materialising the (D chi)^2 product: psi is brought to right-canonical gauge by exact QRs, a zip-up
 * sweep with intermediate bond cap zip_maxdim (<= 0: max(1.5 maxdim, maxdim + 16)) builds a basis per bond (sketched on capped
 * bonds), ONE variational sweep replaces every site by the best tensor given the others, then the exact-gauge compress!
 * runs.  Same error codes as qil_apply / qil_compress.  Not a reference entry point (the reference's apply ignores its
 * cutoff / maxdim kwargs); qil_apply keeps that behaviour.  Accuracy against qil_apply + qil_compress (the exact route):
 * identical bond dimensions and a state error <= 2x the truncation's own on random flat-spectrum products; on transform
 * pipelines identical bonds at tol >= 1e-4 and, below that, bonds that are never larger with a SMALLER error than the exact
 * route, whose gauge passes carry canonicalize!'s fixed cutoff 1e-12 (tests/test_gpu_parity.py,
 * test_apply_compress_*_against_oracle).                                                                          */
QIL_API int qil_apply_compress(const qil_mpo* W, const qil_mps* psi, int64_t maxdim, double tol, int sweeps,
                       int64_t zip_maxdim, qil_mps** out);
/* The same for nb independent (operator, state) pairs of one context -- the (signal, damping value) items of a sweep;
 * Ws / psis entries may repeat (one operator on many signals, many operators on one signal).  outs[j] receives
 * exactly qil_apply_compress(Ws[j], psis[j], ...); the chains run concurrently on the context's streams (see
 * qil_compress_batch).  On failure the first failing item's status is returned and NO handle is handed out.      */
QIL_API int qil_apply_compress_batch(const qil_mpo* const* Ws, const qil_mps* const* psis, int64_t nb, int64_t maxdim,
                             double tol, int sweeps, int64_t zip_maxdim, qil_mps** outs);

/* ------------------------------------------------------------------ encode (E1-E4) */
/* signal_mps(x; method, cutoff, maxdim, k, p, q, random_seed, mindim)
 * src/signals/SignalConverters.jl:228-233.  x: len values of `dtype`, in host memory OR already in HBM (a device
 * pointer is recognised through unified addressing; the caller orders its producer before the call).       */
QIL_API int qil_signal_mps(qil_context* ctx, const void* x, int64_t len, int dtype, int method,
                   double cutoff, int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed,
                   int64_t mindim, qil_mps** out);
/* signal_ztmps(x; cutoff=1e-10, maxdim, kwargs...) SignalConverters.jl:247-283. */
QIL_API int qil_signal_ztmps(qil_context* ctx, const void* x, int64_t len, int dtype, int method,
                     double cutoff, int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed,
                     int64_t mindim, qil_mps** out);
/* nb signals of one length and dtype encoded concurrently on the context's streams -- the serial loop over signal kinds
 * of scripts/benchmark/zt_full_runtime.jl:151-221.  outs[j] receives exactly qil_signal_mps / qil_signal_ztmps(xs[j], ...).
 * On failure the first failing signal's status is returned and NO handle is handed out.                            */
QIL_API int qil_signal_mps_batch(qil_context* ctx, const void* const* xs, int64_t nb, int64_t len, int dtype, int method,
                         double cutoff, int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed, int64_t mindim,
                         qil_mps** outs);
QIL_API int qil_signal_ztmps_batch(qil_context* ctx, const void* const* xs, int64_t nb, int64_t len, int dtype, int method,
                           double cutoff, int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed, int64_t mindim,
                           qil_mps** outs);
/* Cross-interpolation encoder: the MPS of a signal of 2^n samples from O(n maxdim^2) of them, chosen adaptively by
 * full-pivot LU factorisations of two-site blocks (two-site sweeps l = 1 .. n-1 and back; a final forward sweep writes the
 * sites).  Sample j has the bits b_1 .. b_n, site 1 the most significant, as in qil_signal_mps.  The result obeys the
 * invariants of qil_signal_mps: a unit-norm chain whose amplitude is the norm of the represented signal.
 *   n 1 .. 62; maxdim finite, 1 .. 256 (QIL_MAXDIM_NONE is an error); tol >= 0, relative to the largest |x| sampled;
 *   max_sweeps >= 1; seeds: 1 .. 1024 host indices in [0, 2^n), the suffixes the first sweep starts from.
 *   *est: the largest remaining |entry| over the last back-and-forth sweep, relative to the largest |x| sampled;
 *   *nevals: samples asked for (the seeds not counted); *converged: every bond's estimate of that sweep was <= tol.
 * A feature that no pivot's row or column touches is invisible to the interpolation AND to its estimate (an isolated
 * spike is the standard case): pass its index among the seeds.  QIL_EDOMAIN when every sampled value is 0.
 *
 * The evaluator of a session is the caller (pull style, no callbacks): while qil_cross_pending reports count > 0, fetch the
 * count int64 sample indices into a device buffer (qil_cross_indices), evaluate them, and hand count values of `dtype`
 * back in a device buffer (qil_cross_supply: factors the block and advances; the buffer may be reused on return).  When
 * count is 0, qil_cross_finish delivers the chain once.  qil_cross_destroy frees the session at any point; destroy it
 * before its context.  qil_cross_indices / _supply with nothing pending and qil_cross_finish with samples pending are
 * QIL_EINVAL_ARG.  The first request is the seeds themselves.                                                        */
typedef struct qil_cross qil_cross;
QIL_API int qil_cross_begin(qil_context* ctx, int64_t n, int dtype, int64_t maxdim, double tol, int max_sweeps,
                    const int64_t* seeds, int64_t nseeds, qil_cross** out);
QIL_API int qil_cross_pending(qil_cross* s, int64_t* count);
QIL_API int qil_cross_indices(qil_cross* s, int64_t* idx_dev);
QIL_API int qil_cross_supply(qil_cross* s, const void* values_dev);
QIL_API int qil_cross_finish(qil_cross* s, qil_mps** out, double* est, int64_t* nevals, int* sweeps, int* converged);
QIL_API int qil_cross_destroy(qil_cross* s);
/* The same session driven by a gather from a dense signal: x is len values of `dtype` in host memory or in HBM, as in
 * qil_signal_mps; n = round(log2 len), a shorter signal reads as zero-filled, len > 2^n is QIL_EINVAL_LENGTH.       */
QIL_API int qil_signal_mps_cross(qil_context* ctx, const void* x, int64_t len, int dtype, int64_t maxdim, double tol,
                         int max_sweeps, const int64_t* seeds, int64_t nseeds, qil_mps** out, double* est,
                         int64_t* nevals, int* sweeps, int* converged);
/* The paired chain of a SignalMPS: the per-site delta-fuse and split of qil_signal_ztmps (SignalConverters.jl:261-276) on
 * a state that exists already, so that qil_ztmps_from_mps(qil_signal_mps(x, cutoff), cutoff) is qil_signal_ztmps(x, cutoff).
 * psi is left intact; a paired psi is QIL_EINVAL_ARG.  maxdim <= 0: no cap.                                          */
QIL_API int qil_ztmps_from_mps(const qil_mps* psi, double cutoff, int64_t maxdim, qil_mps** out);
/* An element-wise function of up to four states as a new state: out_x = f(states[0]_x, states[1]_x, ..), by the cross
 * interpolation of qil_signal_mps_cross with the samples read from the operands on the device (one launch per block reads
 * every operand at the block's indices and applies f; nothing of a block crosses the host).  Each value includes its state's
 * amplitude.  The result carries the site ids of states[0] and obeys the encoder's invariants: a unit-norm chain whose
 * amplitude is the norm.
 *   op               states  params[0]    value                                    result dtype
 *   QIL_MAP_ABS      1       --           |a|                                      f64
 *   QIL_MAP_POWER    1       p > 0        |a|^p                                    f64
 *   QIL_MAP_LOG      1       eps > 0      log(|a|^2 + eps)                         f64
 *   QIL_MAP_DIVIDE   2       lambda >= 0  a conj(b) / (|b|^2 + lambda)  (0: a / b) c64 when a or b is, else f64
 *   QIL_MAP_SHRINK   1       tau >= 0     a max(0, 1 - tau / |a|), 0 at a = 0      dtype of a
 * maxdim, tol, max_sweeps, seeds, nseeds and the outputs est, nevals, sweeps, converged: as in qil_signal_mps_cross.
 * Errors, before the context is activated and before a state is read: QIL_EINVAL_ARG for a null argument (states, a state,
 * out, params of an op that takes one), an unknown op, nstates not matching the op, a parameter outside its range or not
 * finite, and maxdim, tol, max_sweeps or seeds outside the ranges of qil_cross_begin.  Then: QIL_EINVAL_ARG for states of
 * different contexts, for a paired state ("map: paired states are not supported; map the SignalMPS and call ztmps_from_mps"),
 * for a chain of more than 62 tensors, for a seed >= 2^n and for a bond above 1024 (the carry of the sampler lives in LDS);
 * QIL_EINVAL_LENGTH for states of different lengths; QIL_EINVAL_SITES for site ids that differ from states[0]'s.
 * QIL_EDOMAIN when a sampled value is not finite (QIL_MAP_DIVIDE with lambda = 0 where b vanishes: every non-finite quotient
 * is sampled as +inf) and when every sampled value is 0, both through the session's own checks.  A failed call leaves the
 * pool as it was.
 * The blind spot of cross interpolation is inherited: a feature of f(psi) that no pivot's row or column touches is invisible
 * to the interpolation and to its estimate; pass its index among the seeds (the features of f(psi) usually sit where psi's do). */
enum { QIL_MAP_ABS = 0, QIL_MAP_POWER = 1, QIL_MAP_LOG = 2, QIL_MAP_DIVIDE = 3, QIL_MAP_SHRINK = 4 };
QIL_API int qil_mps_map(const qil_mps* const* states, int64_t nstates, int op, const double* params,
                int64_t maxdim, double tol, int max_sweeps, const int64_t* seeds, int64_t nseeds,
                qil_mps** out, double* est, int64_t* nevals, int* sweeps, int* converged);
/* rsvd(A, Linds...; k, p, q, random_seed, cutoff, maxdim, mindim) src/linalg/rsvd.jl:38-121
 * on the matricised operand A (m x n, host, column-major).  Outputs (host, caller
 * allocated for rank min(k+p, m, n)): U m x r, S r, Vh r x n; *rank = r kept.        */
QIL_API int qil_rsvd(qil_context* ctx, const void* A, int64_t m, int64_t n, int dtype, int64_t k,
             int64_t p, int q, uint64_t seed, double cutoff, int64_t maxdim, int64_t mindim,
             int64_t* rank, void* U, double* S, void* Vh);
/* truncated svd(A; cutoff, maxdim, mindim) with the ITensors truncation rule (the
 * call sites mps.jl:929,946; SignalConverters.jl:84,266).  Same output contract.   */
QIL_API int qil_svd_trunc(qil_context* ctx, const void* A, int64_t m, int64_t n, int dtype, double cutoff,
                  int64_t maxdim, int64_t mindim, int64_t* rank, void* U, double* S, void* Vh);

/* ------------------------------------------------------------------ transform producers (P2) */
/* build_dt_mpo(n, wr; cutoff=1e-14, maxdim=1000) src/transforms/dt_transformer.jl:312-407 for a BATCH of
 * damping values wr[0..nb): ONE kernel launch, one workgroup per damping value runs that value's whole chain of
 * zip_to_combine / zip_to_compress steps (:20-288) with the tensors being factorised resident in LDS.
 * out[nb] receives PairedSiteMPO handles (f64, 2n tensors), each with its own bond dimensions -- those of a
 * single build_dt_mpo call.  site_ids: the 2n labels of the operand the MPOs will act on (build_dt_mpo(psi::ZTMPS,
 * ...) builds on psi's own sites, dt_transformer.jl:409-412); NULL => 1..2n.  maxdim <= 0: no cap.
 * Bonds beyond the in-LDS capacity (truncated bond > 26; never at the reference's cutoffs) take a launch-per-step
 * route that pads every MPO of the batch to a common bond profile with zero components (same operators).
 * The persistent builders (this one, qil_build_qft_mpo, qil_build_zt_qft_chain, qil_build_zt_mpo_batch) run their truncation rule
 * at max(cutoff, 1e-28): directions below 1e-28 of a bond's weight are rounding residue of exactly rank-deficient product bonds
 * (the reference's LAPACK SVD would keep them at cutoff = 0 as noise-level singular values; the operator is the same to rounding).
 * QIL_EINVAL_ARG, naming the index, for a damping value that is NaN or infinite or whose largest gate entry exp(-w 2^(n-2))
 * (exp(-w) for n <= 2) overflows -- a negative w at large n; checked on the host before anything is allocated or launched. */
QIL_API int qil_build_dt_mpo_batch(qil_context* ctx, int64_t n, int64_t nb, const double* wrs, double cutoff,
                           int64_t maxdim, const int64_t* site_ids, qil_mpo** out);

/* build_qft_mpo(n, sites; cutoff=1e-14, maxdim=1000) src/transforms/qft_transformer.jl:121-165 ENTIRELY on the device: one
 * launch of one workgroup runs the whole chain of zip-ups (:13-66) and truncating zip-downs (:69-101) with the tensors in
 * LDS (bonds <= 8, <= 16 before a truncation); only the 2 x 2 gate blocks of control_Hphase_mpo (qft_gates.jl:43-97)
 * come from the host.  Result: a SingleSiteMPO handle (complex) with the reference's bond dimensions and, to rounding,
 * its dense operator (gauges differ).  *fallback = 1 (and no handle) when a bond exceeded the in-LDS capacity: the
 * caller takes the generic route (qil_apply_mpo_mpo + qil_mpo_compress per layer).                                    */
QIL_API int qil_build_qft_mpo(qil_context* ctx, int64_t n, double cutoff, int64_t maxdim, const int64_t* site_ids,
                      qil_mpo** out, int* fallback);
/* The paired-register QFT half of build_zt_mpo (src/transforms/zt_transformer.jl:78-99: identity extension, zip_to_combine
 * "down", zip_to_compress "down" per block control_Hphase_ztmps_mpo, zt_gates.jl:12-114), same persistent kernel; a
 * PairedSiteMPO handle over 2 n tensors main_1, copy_1, ...                                                          */
QIL_API int qil_build_zt_qft_chain(qil_context* ctx, int64_t n, double cutoff, int64_t maxdim, const int64_t* site_ids,
                           qil_mpo** out, int* fallback);

/* build_zt_mpo(n, wr, sites_main, sites_copy; cutoff=1e-14, maxdim=1000) src/transforms/zt_transformer.jl:41-112 for a BATCH
 * of damping values wr[0..nb), every step on the device: the DT halves (:74, one launch, one workgroup per value) and the
 * paired-register QFT chain (:78-99, one launch of one workgroup, built once for the whole batch) run CONCURRENTLY on two
 * streams of the context, then per value the MPO x MPO product apply(W_dt, mpo_qft) (:103) and zip_to_compress_mpo "down"
 * (:104; the nb compressions run as one batch).  out[nb] receives PairedSiteMPO handles (complex, 2n tensors) with the bond
 * dimensions of a single build_zt_mpo call each.  site_ids: the 2n labels main_1, copy_1, ... of the operand (build_zt_mpo(
 * psi::ZTMPS, wr), :107-111); NULL => 1..2n.  maxdim <= 0: no cap.  n == 1 returns the bare product (:66-70).
 * QIL_EINVAL_ARG for n < 1 (the reference's ArgumentError, :49) and for the damping values qil_build_dt_mpo_batch refuses.  */
QIL_API int qil_build_zt_mpo_batch(qil_context* ctx, int64_t n, int64_t nb, const double* wrs, double cutoff,
                           int64_t maxdim, const int64_t* site_ids, qil_mpo** out);

/* C (m x n) = opA(A) * opB(B) on host operands, column-major; op: 0 = N, 1 = T, 2 = H, 3 = conj.
 * The f64-MFMA GEMM every contraction of the truncation/encode path goes through (the `*` of
 * mps.jl:930,947; rsvd.jl:79,89,93,98,114); exported as a utility and test hook.                */
QIL_API int qil_gemm(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
             const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc);

/* Thin QR with non-negative real diagonal (qr(...; positive=true), rsvd.jl:83,90,94) of a host operand
 * A (m x n, m >= n, column-major): Q (m x n), R (n x n).  Utility / test hook.                       */
QIL_API int qil_qr_positive(qil_context* ctx, int dtype, int64_t m, int64_t n, const void* A, void* Q, void* R);
/* ------------------------------------------------------------------ multi-GPU: the batched gather */
/* Independent (signal, damping value) items are dealt round-robin to one process per GPU (item i belongs to rank
 * i mod world); nothing is exchanged until the end, when every rank needs all coefficient batches: ONE RCCL all-gather
 * over xGMI.  The reference's callers loop serially over the damping values (docs/src/tutorials/zt.jl:300-348,
 * scripts/benchmark/zt_full_runtime.jl:151-221); this is the verb a Julia host uses in place of torch.distributed.
 * RCCL is loaded at run time by qil_comm_unique_id / qil_comm_create (QIL_RCCL_LIB, else the librccl.so next to the
 * process's libamdhip64, else the loader path): libqilhip.so itself links the HIP runtime only.
 *
 * Rendezvous: rank 0 calls qil_comm_unique_id and ships the QIL_COMM_ID_BYTES bytes to the other ranks over any host
 * channel (a file, Distributed.jl, MPI); then EVERY rank calls qil_comm_create (collective: returns when all have).   */
#define QIL_COMM_ID_BYTES 128
typedef struct qil_comm qil_comm;
QIL_API int qil_comm_unique_id(void* id_out);
QIL_API int qil_comm_create(qil_context* ctx, int rank, int world, const void* id, qil_comm** out);
/* In any order with qil_context_destroy: a context that goes first tears its communicators down and leaves their handles
 * valid and empty (a GC'd host -- Julia finalizers, Python at shutdown -- cannot promise an order).                 */
QIL_API int qil_comm_destroy(qil_comm* comm);
QIL_API int qil_comm_info(const qil_comm* comm, int* rank, int* world);
/* local: this rank's items in its own order (item rank, rank + world, ...), each `width` complex values (interleaved
 * doubles), host memory.  out: n_items x width complex values in ITEM order, host memory, on every rank.  Collective. */
QIL_API int qil_gather_coefficients(qil_comm* comm, int64_t n_items, int64_t width, const double* local, double* out);
/* The same gather for samples that are already in HBM (a sweep's read-outs start there): local_dev = this rank's
 * ceil-share x width complex values in slot order, out_dev = n_items x width in item order, both DEVICE memory of the
 * communicator's context; stream-ordered on that context's stream, no host synchronisation, no PCIe trip.  Every rank must
 * pass the same n_items and width (they size the collective).  A rank that fails before the collective aborts the
 * communicator (ncclCommAbort) so that its peers fail instead of waiting for ever.                                        */
QIL_API int qil_gather_coefficients_device(qil_comm* comm, int64_t n_items, int64_t width, const void* local_dev, void* out_dev);
/* The body of a damping sweep across the ranks of a communicator (docs/src/tutorials/dt.jl:150-197, zt.jl:300-348): Ws[0..nw)
 * = THIS rank's round-robin share of n_items operators (slot k = item rank + k world; nw must equal that share, else
 * QIL_EINVAL_LENGTH); every W psi is read out at the nb configurations (as qil_apply_coefficient_sweep), the samples stay in HBM,
 * ONE all-gather exchanges them, and out[n_items x nb] (item order, complex, host) is filled on every rank.  Collective.       */
QIL_API int qil_apply_coefficient_sweep_gather(qil_comm* comm, const qil_mpo* const* Ws, int64_t nw, const qil_mps* psi, int64_t nb,
                                       const uint8_t* bits, int64_t n_items, double* out);
/* The layout rule of that gather as a host function (no GPU, no RCCL): `gathered` = world blocks of
 * ceil(n_items / world) x width complex values in rank order -> `out` in item order.                                 */
QIL_API int qil_sweep_unshuffle(int world, int64_t n_items, int64_t width, const double* gathered, double* out);
/* ... and as the kernel the device gather uses (device buffers of `ctx`, stream-ordered): same rule, tested against the host one. */
QIL_API int qil_sweep_unshuffle_device(qil_context* ctx, int world, int64_t n_items, int64_t width, const void* gathered_dev, void* out_dev);

#ifdef __cplusplus
}
#endif
#endif /* QILAPLACE_HIP_H */
