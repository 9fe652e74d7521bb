// Truncation and encoding on the device: canonicalize! (K2), compress! (K1), truncated SVD,
// rsvd (E3), signal_mps (E1/E2), signal_ztmps (E4).
//
//   canonicalize!   src/mps.jl:787-847 (ZTMPS :866-901)
//   compress!       src/mps.jl:913-973 (ZTMPS :975-999)
//   rsvd            src/linalg/rsvd.jl:38-121
//   signal_mps      src/signals/SignalConverters.jl:16-46, 49-104 (:svd), 107-196 (:rsvd), 228-233
//   signal_ztmps    src/signals/SignalConverters.jl:247-283
//
// Matricisations are chosen so that every reshape is free in the canonical column-major layouts
// and the one-sided Jacobi SVD always rotates the SHORT side (see the notes at each call site).
#include <algorithm>
#include <chrono>
#include <cmath>

#include "qil_internal.h"
#include "qil_launch.h"
#include "qil_device_utils.h"

namespace {

using namespace qil_dev;

constexpr int64_t kNoCap = INT64_MAX;

// dst (rows x cols, ldd) <- src (rows x cols, lds): strided device copy
int copy_2d(qil_context* ctx, int dtype, int64_t rows, int64_t cols, const void* src, int64_t lds_, void* dst,
            int64_t ldd) {
    if (rows == 0 || cols == 0) return QIL_OK;
    const size_t e = qil_elem_size(dtype);
    QIL_TRY(qil_dev_copy2d(ctx, dst, (size_t)ldd * e, src, (size_t)lds_ * e, (size_t)rows * e, (size_t)cols));
    return QIL_OK;
}

// out[2 * block] += |A - D|_F^2 over this block's elements, out[2 * block + 1] += |A|_F^2   (A: lda, D: ldd; doubles viewed
// as reals: nre = 1 real / 2 complex values per element)
__device__ __forceinline__ void residual_sumsq_body(const uint3 blockIdx, const uint3 gridDim, const double* __restrict__ A, long long lda, const double* __restrict__ D,
                                                       long long ldd, long long m, long long n, int nre,
                                                       double* __restrict__ out) {
    __shared__ double red[8];
    double r2 = 0, a2 = 0;
    const long long rows = m * nre;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < rows * n; t += (long long)gridDim.x * 256) {
        const long long i = t % rows, j = t / rows;
        const double a = A[i + lda * nre * j], d = D[i + ldd * nre * j];
        r2 = fma(a - d, a - d, r2);
        a2 = fma(a, a, a2);
    }
    for (int o = 32; o > 0; o >>= 1) {
        r2 += __shfl_xor(r2, o);
        a2 += __shfl_xor(a2, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave] = r2;
        red[4 + wave] = a2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        out[2 * blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}
struct residual_sumsq_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        residual_sumsq_body(b, g, a...);
    }
};

int svd_trunc_dev(qil_context* ctx, int dtype, int64_t m, int64_t n, void* A, int64_t lda, double cutoff,
                  bool use_cutoff, int64_t maxdim, int64_t mindim, int absorb, int64_t* rank, void** U_out,
                  void** Vh_out, std::vector<double>* S_out);

// Low-rank fast path of a TRUNCATING SVD of a large operand (every product bond before its truncation is heavily
// rank-deficient: bond 1008 of the zT product carries ~60 singular values above 1e-6 of the largest).  Range finder
// with one power iteration, Q = orth(A (A^H (A Omega))) (k = 128 columns, then 256), B = Q^H A, and the residual
// |A - Q B|_F^2 is MEASURED: the path is taken only if it is below 1e-8 of the weight the caller's cutoff allows to be
// discarded -- then the truncation rule sees the same decision as on A itself -- and the truncated SVD of the k x n
// matrix B gives the factors (U = Q U_B).  Otherwise *done = 0 and A is intact.
static int svd_trunc_lowrank(qil_context* ctx, int dtype, int64_t m, int64_t n, void* A, int64_t lda, double cutoff,
                             int64_t maxdim, int64_t mindim, int absorb, int64_t* rank, void** U_out, void** Vh_out,
                             std::vector<double>* S_out, int* done) {
    *done = 0;
    const int64_t r0 = std::min(m, n);
    if (r0 < 384 || !(cutoff > 0)) return QIL_OK;
    const bool dbg = getenv("QIL_SVD_DEBUG") != nullptr;
    const size_t e = qil_elem_size(dtype);
    const int cj = dtype == QIL_C64 ? 2 : 1;
    const int nre = dtype == QIL_C64 ? 2 : 1;
    for (int64_t k : {(int64_t)128, (int64_t)256}) {
        if (k * 3 > r0) break;
        void *Om = nullptr, *Y = nullptr, *Z = nullptr, *B = nullptr, *D = nullptr, *part = nullptr;
        qil_scratch scratch(ctx);                        // this attempt's blocks: freed when it ends, whichever way
        QIL_TRY(scratch.alloc((size_t)(n * k) * e, &Om));
        QIL_TRY(qil_dev_fill_normal(ctx, dtype, Om, n * k, 0x10a4c0deull + (uint64_t)k, 1.0));
        QIL_TRY(scratch.alloc((size_t)(m * k) * e, &Y));
        QIL_TRY(scratch.alloc((size_t)(n * k) * e, &Z));
        QIL_TRY(qil_dev_gemm(ctx, dtype, 0, 0, m, k, n, A, lda, Om, n, Y, m));                       // Y = A Omega
        QIL_TRY(qil_dev_qr_positive(ctx, dtype, m, k, Y, m, nullptr, 0, false));
        QIL_TRY(qil_dev_gemm(ctx, dtype, cj, 0, n, k, m, A, lda, Y, m, Z, n));                       // Z = A^H Y
        QIL_TRY(qil_dev_qr_positive(ctx, dtype, n, k, Z, n, nullptr, 0, false));
        QIL_TRY(qil_dev_gemm(ctx, dtype, 0, 0, m, k, n, A, lda, Z, n, Y, m));                        // Y = A Z
        QIL_TRY(qil_dev_qr_positive(ctx, dtype, m, k, Y, m, nullptr, 0, true));                      // Q (orthonormal)
        QIL_TRY(scratch.alloc((size_t)(k * n) * e, &B));
        QIL_TRY(qil_dev_gemm(ctx, dtype, cj, 0, k, n, m, Y, m, A, lda, B, k));                       // B = Q^H A
        QIL_TRY(scratch.alloc((size_t)(m * n) * e, &D));
        QIL_TRY(qil_dev_gemm(ctx, dtype, 0, 0, m, n, k, Y, m, B, k, D, m));                          // D = Q B
        const unsigned nblk_ = (unsigned)std::min<long long>((m * n * nre + 255) / 256, 1024);
        QIL_TRY(scratch.alloc((size_t)nblk_ * 2 * sizeof(double), &part));
        QIL_TRY((qil_klaunch<residual_sumsq_k>(ctx, dim3(nblk_), dim3(256), 0, (const double*)A, (long long)lda, (const double*)D, (long long)m, (long long)m, (long long)n, nre, (double*)part)));
        std::vector<double> hp((size_t)nblk_ * 2);
        QIL_TRY(qil_read_back(ctx, hp.data(), part, hp.size() * sizeof(double)));
        double rho = 0, tot = 0;
        for (unsigned b = 0; b < nblk_; ++b) {
            rho += hp[2 * b];
            tot += hp[2 * b + 1];
        }
        if (dbg) fprintf(stderr, "[svd-lowrank] %lld x %lld, k = %lld: residual^2 / total = %.3e (cutoff %.1e)\n",
                                             (long long)m, (long long)n, (long long)k, tot > 0 ? rho / tot : 0.0, cutoff);
        if (!(rho <= 1e-8 * cutoff * tot)) {
            // a sketch twice as wide cannot help an operand that is nowhere near low rank (flat spectra leave > 50 % of
            // the weight outside 128 columns): only residuals that are already small earn the second attempt
            if (rho > 1e-4 * tot) break;
            continue;
        }
        if (dbg) fprintf(stderr, "[svd-lowrank] %lld x %lld, k = %lld: sketch accepted\n", (long long)m, (long long)n, (long long)k);
        int64_t r = 0;
        void *Ub = nullptr, *Vh = nullptr;
        std::vector<double> S;
        QIL_TRY(svd_trunc_dev(ctx, dtype, k, n, B, k, cutoff, true, maxdim, mindim, absorb, &r, &Ub, &Vh, &S));
        scratch.own(Ub);
        scratch.own(Vh);
        void* U = nullptr;
        QIL_TRY(scratch.alloc((size_t)(m * std::min(m, n)) * e, &U));          // callers index U with ld m only
        QIL_TRY(qil_dev_gemm(ctx, dtype, 0, 0, m, r, k, Y, m, Ub, k, U, m));                         // U = Q U_B
        scratch.free(Ub);
        *rank = r;
        *U_out = scratch.give(U);
        *Vh_out = scratch.give(Vh);
        if (S_out) *S_out = std::move(S);
        *done = 1;
        return QIL_OK;
    }
    return QIL_OK;
}

// Truncated SVD of the device matrix A (m x n, lda; destroyed).  Outputs are fresh pool blocks:
//   U  (m x r, ld m)   -- optionally scaled by S (absorb = 1)
//   Vh (r x n, ld r)   -- optionally scaled by S (absorb = 2)
// They are the caller's from the return on (qil_scratch::own); a failed call leaves nothing behind.
int svd_trunc_dev(qil_context* ctx, int dtype, int64_t m, int64_t n, void* A, int64_t lda, double cutoff,
                  bool use_cutoff, int64_t maxdim, int64_t mindim, int absorb, int64_t* rank, void** U_out,
                  void** Vh_out, std::vector<double>* S_out) {
    const int64_t r0 = std::min(m, n);
    const size_t e = qil_elem_size(dtype);
    qil_scratch tmp(ctx);
    // Gauge sweeps that truncate by cutoff only and do not read the singular values (canonicalize!(cutoff), the first pass of
    // compress!): where the site's triangular factor certifies that nothing can be dropped, the thin QR is the gauge step
    // (qil_linalg.hip, "nothing can be truncated" certificate).  97..639 columns: inside the one-factor SVD, which has the QR
    // at hand; from 640 columns on: here, before the GEMM-shaped block Jacobi.
    const double cert_cutoff = (!S_out && use_cutoff && cutoff > 0.0 && r0 <= maxdim && (absorb == 1 || absorb == 2)) ? cutoff : 0.0;
    if (cert_cutoff > 0.0 && r0 >= 640) {
        const int64_t rows = std::max(m, n);
        void *Qb = nullptr, *Rb = nullptr;
        QIL_TRY(tmp.alloc((size_t)(rows * r0) * e, &Qb));
        QIL_TRY(tmp.alloc((size_t)(r0 * r0) * e, &Rb));
        bool certified = false;
        QIL_TRY(qil_dev_qr_certified(ctx, dtype, m, n, A, lda, cert_cutoff, Qb, Rb, &certified));
        if (getenv("QIL_SVD_DEBUG"))
            fprintf(stderr, "[svd-cert] %lld x %lld (lda %lld), absorb %d: %s\n", (long long)m, (long long)n, (long long)lda, absorb,
                    certified ? "QR gauge" : "declined");
        if (certified) {
            void *U = nullptr, *Vh = nullptr;
            QIL_TRY(tmp.alloc((size_t)(m * r0) * e, &U));
            QIL_TRY(tmp.alloc((size_t)(r0 * n) * e, &Vh));
            if (absorb == 2) {                       // U isometric, the rest absorbed
                if (m >= n) {                        // A = Q R
                    QIL_TRY(copy_2d(ctx, dtype, m, r0, Qb, rows, U, m));
                    QIL_TRY(copy_2d(ctx, dtype, r0, n, Rb, r0, Vh, r0));
                } else {                             // every row direction is kept: U = I, the rest = A
                    QIL_TRY(qil_dev_zero(ctx, U, (size_t)(m * r0) * e));
                    QIL_TRY(qil_dev_set_identity(ctx, dtype, U, m, r0));
                    QIL_TRY(copy_2d(ctx, dtype, m, n, A, lda, Vh, r0));
                }
            } else {                                 // Vh isometric, U S absorbed
                if (m < n) {                         // A^H = Q R  =>  A = R^H Q^H   (m == n: the factor is of A itself)
                    QIL_TRY(qil_dev_transpose(ctx, dtype, 1, rows, r0, Qb, rows, Vh, r0));
                    QIL_TRY(qil_dev_transpose(ctx, dtype, 1, r0, r0, Rb, r0, U, m));
                } else {                             // every column direction is kept: Vh = I, U S = A
                    QIL_TRY(qil_dev_zero(ctx, Vh, (size_t)(r0 * n) * e));
                    QIL_TRY(qil_dev_set_identity(ctx, dtype, Vh, r0, r0));
                    QIL_TRY(copy_2d(ctx, dtype, m, n, A, lda, U, m));
                }
            }
            tmp.free(Qb);
            tmp.free(Rb);
            *rank = r0;
            *U_out = tmp.give(U);
            *Vh_out = tmp.give(Vh);
            return QIL_OK;
        }
        tmp.free(Qb);
        tmp.free(Rb);
    }
    if (use_cutoff) {
        int done = 0;
        QIL_TRY(svd_trunc_lowrank(ctx, dtype, m, n, A, lda, cutoff, maxdim, mindim, absorb, rank, U_out, Vh_out, S_out, &done));
        if (done) return QIL_OK;
    }
    void *U = nullptr, *Vh = nullptr;
    QIL_TRY(tmp.alloc((size_t)(m * r0) * e, &U));
    QIL_TRY(tmp.alloc((size_t)(r0 * n) * e, &Vh));
    std::vector<double> S((size_t)r0);
    // with a truncating cutoff, columns 100x below it (and never above 1e-30 |A|_F^2) are not worth rotating
    const double negl_rel = use_cutoff && cutoff > 0 ? std::min(1e-30, 1e-2 * cutoff) : 0.0;
    // Gauge sweeps keep ONE factor as the site (isometric) and multiply the other into the neighbour: the mid-size path
    // that accumulates no rotation matrix (qil_dev_svd_left) serves them; everything else takes the general SVD.
    int handled = 0;
    // the one-factor SVD may drop 1e-6 of what the cutoff allows with the negligible rows of its triangular factor
    // (the weight w the one-factor SVD may drop costs sqrt(w) in amplitude.  Measured on the exact compress! of the bond-1008 zT
    // product, w = 1e-3 / 1e-5 / 1e-6 / 1e-8 of the cutoff: 253-260 / 282 / 266-273 / 270 ms (295 without), state against the
    // CPU oracle's compress! 1.2e-7 / 1.6e-9 / 4e-10 / 3e-10 (1e-11 without; the algorithm's own error there is 1.8e-5))
    // ... and never more than 1e-18 of the total, sqrt(w) = 1e-9 in amplitude, the figure device and oracle truncations are held to:
    // at cutoff 1e-8 the plain 1e-6 left the compressed 7-site MPO of tests/mpo_cases.py (bond 70 of rank 64) 1.2e-9 from the oracle's.
    // Cutoffs up to 1e-12 (every compress! tolerance, the builders' 1e-14) are below the cap and unchanged.
    const double deflate = (use_cutoff && cutoff > 0.0) ? std::min(1e-6 * cutoff, 1e-18) : 0.0;
    if (absorb == 2) {            // U isometric, S Vh absorbed
        QIL_TRY(qil_dev_svd_left(ctx, dtype, m, n, A, lda, U, m, S.data(), Vh, r0, negl_rel, &handled, cert_cutoff, deflate));
    } else if (absorb == 1) {     // Vh isometric, U S absorbed: the same problem on A^H
        void *At = nullptr, *Vi = nullptr, *SU = nullptr;
        QIL_TRY(tmp.alloc((size_t)(m * n) * e, &At));
        QIL_TRY(qil_dev_transpose(ctx, dtype, 1, m, n, A, lda, At, n));                         // A^H (n x m)
        QIL_TRY(tmp.alloc((size_t)(n * r0) * e, &Vi));
        QIL_TRY(tmp.alloc((size_t)(r0 * m) * e, &SU));
        QIL_TRY(qil_dev_svd_left(ctx, dtype, n, m, At, n, Vi, n, S.data(), SU, r0, negl_rel, &handled, cert_cutoff, deflate));
        if (handled) {
            QIL_TRY(qil_dev_transpose(ctx, dtype, 1, n, r0, Vi, n, Vh, r0));                    // Vh = V^H   (r0 x n)
            QIL_TRY(qil_dev_transpose(ctx, dtype, 1, r0, m, SU, r0, U, m));                     // U S = (S U^H)^H
        }
        tmp.free(At);
        tmp.free(Vi);
        tmp.free(SU);
    }
    if (!handled) QIL_TRY(qil_dev_svd(ctx, dtype, m, n, A, lda, U, m, S.data(), Vh, r0, negl_rel));
    // handled == 2: certified that nothing can be truncated (S was not computed)
    const int64_t r = handled == 2 ? r0 : qil_truncation_rank(S.data(), r0, cutoff, use_cutoff, maxdim, mindim);
    if (!handled && absorb == 1) QIL_TRY(qil_dev_scale(ctx, dtype, 1, m, r, U, m, S.data()));
    if (!handled && absorb == 2) QIL_TRY(qil_dev_scale(ctx, dtype, 0, r, n, Vh, r0, S.data()));
    if (r < r0) {  // compact Vh rows to leading dimension r
        void* Vc = nullptr;
        QIL_TRY(tmp.alloc((size_t)(r * n) * e, &Vc));
        QIL_TRY(copy_2d(ctx, dtype, r, n, Vh, r0, Vc, r));
        tmp.free(Vh);
        Vh = Vc;
    }
    S.resize((size_t)r);
    *rank = r;
    *U_out = tmp.give(U);  // first r columns are the kept ones (contiguous)
    *Vh_out = tmp.give(Vh);
    if (S_out) *S_out = std::move(S);
    return QIL_OK;
}

// ---------------------------------------------------------------- canonicalize!
// Works on any chain: the physical block is 2 (MPS site A[a,s,b]) or 4 (MPO site W[a,s',s,b]) wide and sits
// between the two bonds in memory, so "rows (a, phys) | cols b" and "rows a | cols (phys, b)" are the site
// buffer as it lies in both cases.
// Exact gauge sweep by thin QR (no truncation): the first pass of zip_to_compress_mpo (dt_transformer.jl:190, :237
// use `qr`, only the return pass uses `svd`).  Same site layouts as canonicalize_impl below; a site whose matrix is
// wider than tall has no thin QR that shrinks nothing, so it takes the SVD route with cutoff 0.
// Every gauge step here and below factors a COPY of site i and replaces the two sites only when nothing can fail any more: a
// call that runs out of memory half way leaves the chain, and the operator or state it stands for, as the last finished step left it.
// The blocks of a step are its scratch's until the chain takes them.
static int site_copy(qil_scratch& tmp, qil_chain* psi, int64_t i, void** out) {
    QIL_TRY(tmp.alloc(psi->site_bytes(i), out));
    return qil_dev_copy(psi->ctx, *out, psi->site[(size_t)i], psi->site_bytes(i));
}

static int gauge_qr_site_right(qil_chain* psi, int64_t i, int64_t pd) {
    qil_context* ctx = psi->ctx;
    const int dt = psi->dtype;
    const size_t e = qil_elem_size(dt);
    const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1], cr2 = psi->dims[(size_t)i + 2];
    qil_scratch tmp(ctx);
    void *Q = nullptr, *Rf = nullptr, *next = nullptr;
    QIL_TRY(site_copy(tmp, psi, i, &Q));
    QIL_TRY(tmp.alloc((size_t)(cr * cr) * e, &Rf));
    QIL_TRY(qil_dev_qr_positive(ctx, dt, pd * cl, cr, Q, pd * cl, Rf, cr, true));   // Q in place of the copy
    QIL_TRY(tmp.alloc((size_t)(cr * pd * cr2) * e, &next));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, cr, pd * cr2, cr, Rf, cr, psi->site[(size_t)i + 1], cr, next, cr));
    tmp.free(Rf);
    QIL_TRY(qil_chain_set_site(psi, i, tmp.give(Q), cl, cr));
    QIL_TRY(qil_chain_set_site(psi, i + 1, tmp.give(next), cr, cr2));
    return QIL_OK;
}

static int gauge_qr_site_left(qil_chain* psi, int64_t i, int64_t pd) {
    qil_context* ctx = psi->ctx;
    const int dt = psi->dtype;
    const size_t e = qil_elem_size(dt);
    const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1], cl0 = psi->dims[(size_t)i - 1];
    // A (cl x pd cr) = L Q with orthonormal rows of Q:  A^H = Qt Rt  =>  Q = Qt^H, L = Rt^H
    qil_scratch tmp(ctx);
    void *Ah = nullptr, *Rt = nullptr, *prev = nullptr, *Q = nullptr;
    QIL_TRY(tmp.alloc((size_t)(pd * cr * cl) * e, &Ah));
    QIL_TRY(qil_dev_transpose(ctx, dt, 1, cl, pd * cr, psi->site[(size_t)i], cl, Ah, pd * cr));
    QIL_TRY(tmp.alloc((size_t)(cl * cl) * e, &Rt));
    QIL_TRY(qil_dev_qr_positive(ctx, dt, pd * cr, cl, Ah, pd * cr, Rt, cl, true));
    QIL_TRY(tmp.alloc(psi->site_bytes(i), &Q));
    QIL_TRY(qil_dev_transpose(ctx, dt, 1, pd * cr, cl, Ah, pd * cr, Q, cl));
    tmp.free(Ah);
    QIL_TRY(tmp.alloc((size_t)(cl0 * pd * cl) * e, &prev));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 2, pd * cl0, cl, cl, psi->site[(size_t)i - 1], pd * cl0, Rt, cl, prev, pd * cl0));
    tmp.free(Rt);
    QIL_TRY(qil_chain_set_site(psi, i, tmp.give(Q), cl, cr));
    QIL_TRY(qil_chain_set_site(psi, i - 1, tmp.give(prev), cl0, cl));
    return QIL_OK;
}

// One step of the left-to-right gauge sweep (mps.jl:802-817): site i becomes a left isometry (rows (alpha, phys) | cols
// beta), its right factor is multiplied into site i+1.  gauge_qr: exact thin QR where the site is tall enough,
// truncated SVD otherwise (and always when gauge_qr is off).
static int gauge_site_right(qil_chain* psi, int64_t i, double cutoff, int64_t maxdim, bool gauge_qr) {
    const int64_t pd = psi->phys_rank == 1 ? 2 : 4;
    qil_context* ctx = psi->ctx;
    const int dt = psi->dtype;
    const size_t e = qil_elem_size(dt);
    const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
    const int64_t cr2 = psi->dims[(size_t)i + 2];
    if (gauge_qr && pd * cl >= cr) return gauge_qr_site_right(psi, i, pd);
    int64_t r = 0;
    qil_scratch tmp(ctx);
    void *A = nullptr, *U = nullptr, *SV = nullptr;
    // rows (alpha, s) | cols beta : the site buffer as it lies
    QIL_TRY(site_copy(tmp, psi, i, &A));
    QIL_TRY(svd_trunc_dev(ctx, dt, pd * cl, cr, A, pd * cl, cutoff, true, maxdim, 1, 2, &r, &U, &SV, nullptr));
    tmp.own(U);
    tmp.own(SV);
    tmp.free(A);
    void* next = nullptr;
    QIL_TRY(tmp.alloc((size_t)(r * pd * cr2) * e, &next));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, r, pd * cr2, cr, SV, r, psi->site[(size_t)i + 1], cr, next, r));
    tmp.free(SV);
    QIL_TRY(qil_chain_set_site(psi, i, tmp.give(U), cl, r));
    QIL_TRY(qil_chain_set_site(psi, i + 1, tmp.give(next), r, cr2));
    return QIL_OK;
}

// The mirror step of the right-to-left sweep (mps.jl:822-837): site i becomes a right isometry (rows alpha | cols
// (phys, beta)), its left factor is multiplied into site i-1.
static int gauge_site_left(qil_chain* psi, int64_t i, double cutoff, int64_t maxdim, bool gauge_qr) {
    const int64_t pd = psi->phys_rank == 1 ? 2 : 4;
    qil_context* ctx = psi->ctx;
    const int dt = psi->dtype;
    const size_t e = qil_elem_size(dt);
    const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
    const int64_t cl0 = psi->dims[(size_t)i - 1];
    if (gauge_qr && pd * cr >= cl) return gauge_qr_site_left(psi, i, pd);
    int64_t r = 0;
    qil_scratch tmp(ctx);
    void *A = nullptr, *US = nullptr, *Vh = nullptr;
    // rows alpha | cols (s, beta)
    QIL_TRY(site_copy(tmp, psi, i, &A));
    QIL_TRY(svd_trunc_dev(ctx, dt, cl, pd * cr, A, cl, cutoff, true, maxdim, 1, 1, &r, &US, &Vh, nullptr));
    tmp.own(US);
    tmp.own(Vh);
    tmp.free(A);
    void* prev = nullptr;
    QIL_TRY(tmp.alloc((size_t)(cl0 * pd * r) * e, &prev));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, pd * cl0, r, cl, psi->site[(size_t)i - 1], pd * cl0, US, cl, prev, pd * cl0));
    tmp.free(US);
    QIL_TRY(qil_chain_set_site(psi, i, tmp.give(Vh), r, cr));
    QIL_TRY(qil_chain_set_site(psi, i - 1, tmp.give(prev), cl0, r));
    return QIL_OK;
}

int canonicalize_impl(qil_chain* psi, int direction, int64_t center, double cutoff, int64_t maxdim,
                      bool gauge_qr = false) {
    qil_context* ctx = psi->ctx;
    const int64_t N = psi->n();
    if (direction == QIL_DIR_RIGHT) {
        const int64_t c = center == 0 ? N : center;
        QIL_REQUIRE(c >= 1 && c <= N, QIL_EDOMAIN, "Center out of range [1,%lld]", (long long)N);
        for (int64_t i = 0; i + 1 < c; ++i) {  // mps.jl:802-817
            qil_progress_step(ctx, i == 0, i);                                  // lock-step batches: where this chain is
            QIL_TRY(gauge_site_right(psi, i, cutoff, maxdim, gauge_qr));
        }
    } else if (direction == QIL_DIR_LEFT) {
        const int64_t c = center == 0 ? 1 : center;
        QIL_REQUIRE(c >= 1 && c <= N, QIL_EDOMAIN, "Center out of range [1,%lld]", (long long)N);
        for (int64_t i = N - 1; i >= c; --i) {                                                             // mps.jl:822-837
            qil_progress_step(ctx, i == N - 1, N - 1 - i);
            QIL_TRY(gauge_site_left(psi, i, cutoff, maxdim, gauge_qr));
        }
    } else {
        return qil_fail(QIL_EINVAL_ARG, "Direction must be :right or :left");
    }
    return QIL_OK;
}

// ---------------------------------------------------------------- helper kernels (layout permutations)
// site A[alpha + cl*(s + 2*k)] = Vyh[k + ldv*(s + 2*alpha)]      (signal_mps :svd, see below)
template <class T>
__device__ __forceinline__ void site_from_vh_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ Vyh, long long ldv, int cl, int k, T* __restrict__ A) {
    const long long total = 2LL * cl * k;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int alpha = (int)(t % cl);
        const long long u = t / cl;
        const int s = (int)(u & 1);
        const int kk = (int)(u >> 1);
        A[t] = Vyh[kk + ldv * (s + 2LL * alpha)];
    }
}
template <class T>
struct site_from_vh_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        site_from_vh_body<T>(b, g, a...);
    }
};

// canonical site A[lb + cl*(s + 2*rb)] from the chunk layout X[rb + cr*(s + 2*lb)]
template <class T>
__device__ __forceinline__ void site_from_chunk_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ X, int cl, int cr, T* __restrict__ A) {
    const long long total = 2LL * cl * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int lb = (int)(t % cl);
        const long long u = t / cl;
        const int s = (int)(u & 1);
        const int rb = (int)(u >> 1);
        A[t] = X[rb + (long long)cr * (s + 2LL * lb)];
    }
}
template <class T>
struct site_from_chunk_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        site_from_chunk_body<T>(b, g, a...);
    }
};

// T[(alpha, m), (c, beta)] = A[alpha, m, beta] * delta(m, c)   (signal_ztmps, SignalConverters.jl:263)
template <class T>
__device__ __forceinline__ void fuse_delta_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ A, int cl, int cr, T* __restrict__ Tm) {
    const long long total = 4LL * cl * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long row = t % (2LL * cl), col = t / (2LL * cl);
        const int alpha = (int)(row % cl), m = (int)(row / cl);
        const int c = (int)(col & 1);
        const long long beta = col >> 1;
        Tm[t] = (m == c) ? A[alpha + (long long)cl * (m + 2 * beta)] : T{};
    }
}
template <class T>
struct fuse_delta_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        fuse_delta_body<T>(b, g, a...);
    }
};

inline unsigned nblk(long long total) { return (unsigned)std::min<long long>((total + 255) / 256, 65536); }

// per-workgroup partial sums of squares (fixed grid => the host-side final sum has a fixed order)
__device__ __forceinline__ void sumsq_partial_body(const uint3 blockIdx, const uint3 gridDim, const double* __restrict__ x, long long n,
                                                     double* __restrict__ part) {
    __shared__ double red[4];
    double v = 0;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < n; t += (long long)gridDim.x * 256) v += x[t] * x[t];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
struct sumsq_partial_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        sumsq_partial_body(b, g, a...);
    }
};
// The rescue pass of the norm (signal_mps_impl): per-workgroup partial sums of (s x)^2 with s a power of two, so that s x is
// exact, or -- sq == 0 -- per-workgroup partial maxima of |x|.  Same grid and reduction tree as sumsq_partial.
__device__ __forceinline__ void sumsq_rescue_body(const uint3 blockIdx, const uint3 gridDim, const double* __restrict__ x, long long n,
                                                    double s, int sq, double* __restrict__ part) {
    __shared__ double red[4];
    double v = 0;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const double a = x[t] * s;
        v = sq ? v + a * a : fmax(v, fabs(a));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(v, m, 64);
        v = sq ? v + o : fmax(v, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = sq ? (red[0] + red[1]) + (red[2] + red[3]) : fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
struct sumsq_rescue_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        sumsq_rescue_body(b, g, a...);
    }
};
__device__ __forceinline__ void scale_inplace_body(const uint3 blockIdx, const uint3 gridDim, double* __restrict__ x, long long n, double s) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n;
         t += (long long)gridDim.x * blockDim.x)
        x[t] *= s;
}
struct scale_inplace_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        scale_inplace_body(b, g, a...);
    }
};
// y = s x (out of place: the caller's device-resident samples are read once for the norm and once here)
__device__ __forceinline__ void scale_copy_body(const uint3 blockIdx, const uint3 gridDim, const double* __restrict__ x, double* __restrict__ y, long long n, double s) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n;
         t += (long long)gridDim.x * blockDim.x)
        y[t] = x[t] * s;
}
struct scale_copy_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        scale_copy_body(b, g, a...);
    }
};

// ---------------------------------------------------------------- rsvd on a device operand
// `Z` holds M^T (plain transpose) column-major: Z is (n x m) for the m x n operand M ("M stored
// row-major").  Produces, with k = kept rank,
//   left  = U_M^T        (k x m, ld k)      -- U_M = Q * Uhat
//   right = (S V_M^h)^T  (n x k, ld n)
// Steps follow src/linalg/rsvd.jl:72-114; the small SVD is taken of B^T = Z conj(Q) (n x l), whose
// short side is l, so the Jacobi rotations act on l columns and (S V^h)^T falls out of the rotated
// work matrix directly.
//
// The route line of QIL_RSVD_DEBUG: one per call of rsvd_rowmajor, whatever the size, and no stream synchronisation (nothing
// it prints comes from the device).  `l` is the sketch width after the deflation, negative for the exact branch:
//   [rsvd] route m=<m> n=<n> l0=<l0> exact
//   [rsvd] route m=<m> n=<n> l0=<l0> sketch l=<l>
// One write per line, so the lines of concurrent sub-trees do not interleave (tests/encode_cases.py parses them).
static void rsvd_route_line(int64_t m, int64_t n, int64_t l0, int64_t l) {
    char line[160];
    if (l < 0)
        snprintf(line, sizeof line, "[rsvd] route m=%lld n=%lld l0=%lld exact\n", (long long)m, (long long)n, (long long)l0);
    else
        snprintf(line, sizeof line, "[rsvd] route m=%lld n=%lld l0=%lld sketch l=%lld\n", (long long)m, (long long)n, (long long)l0,
                 (long long)l);
    fputs(line, stderr);
}

int rsvd_rowmajor(qil_context* ctx, int dt, int64_t m, int64_t n, const void* Z, int64_t k, int64_t p, int q,
                  uint64_t seed, double cutoff, int64_t maxdim, int64_t mindim, int64_t* rank, void** left,
                  void** right, std::vector<double>* S_out) {
    QIL_REQUIRE(m >= 1 && n >= 1, QIL_EEMPTY, "In `rsvd`, left or right index set is empty.");
    const size_t e = qil_elem_size(dt);
    const int64_t l0 = std::min(std::min(k + p, m), n);  // rsvd.jl:72
    const bool route = getenv("QIL_RSVD_DEBUG") != nullptr;
    qil_scratch tmp(ctx);
    if (l0 == std::min(m, n)) {
        if (route) rsvd_route_line(m, n, l0, -1);
        // The sketch is as wide as the short side: Q spans the whole range of M and the procedure returns the exact
        // truncated SVD (up to rounding) after 2 + 2q products and 1 + 2q QRs of matrices no larger than M itself.
        // Take the SVD directly: Z = M^T = Uz Sz Vz^h  =>  U_M^T = Vz^h,  (S V_M^h)^T = Uz Sz.  Every deep split of
        // the bisection encoder ends up here (SignalConverters.jl:161: m or n <= k + p).
        void* Zc = nullptr;
        QIL_TRY(tmp.alloc((size_t)(m * n) * e, &Zc));
        QIL_TRY(qil_dev_copy(ctx, Zc, Z, (size_t)(m * n) * e));
        int64_t r = 0;
        void *UzS = nullptr, *Vzh = nullptr;
        QIL_TRY(svd_trunc_dev(ctx, dt, n, m, Zc, n, cutoff, true, maxdim, mindim, 1, &r, &UzS, &Vzh, S_out));   // the caller's from here
        *rank = r;
        *left = Vzh;    // r x m, ld r
        *right = UzS;   // n x (>= r) columns, ld n
        return QIL_OK;
    }
    void *Om = nullptr, *Y = nullptr, *Zq = nullptr, *Bt = nullptr;
    const bool dbg = route && m * n >= ((1LL << 24));                              // the timing laps synchronise: large operands only
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        (void)qil_stream_sync(ctx);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[rsvd] %lld x %lld, l = %lld: %s %.2f ms\n", (long long)m, (long long)n, (long long)l0, what,
                std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    };
    QIL_TRY(tmp.alloc((size_t)(n * l0) * e, &Om));
    QIL_TRY(tmp.alloc((size_t)(m * l0) * e, &Y));
    QIL_TRY(qil_dev_fill_normal(ctx, dt, Om, n * l0, seed, 1.0));                        // rsvd.jl:74-76
    lap("omega");
    QIL_TRY(qil_dev_gemm(ctx, dt, 1, 0, m, l0, n, Z, n, Om, n, Y, m));                   // Y = M Omega (:79)
    lap("Y = M Omega");
    // the basis that B = Q^H M and U = Q Uhat are built from (the last QR) must be orthonormal even when the sketch is
    // wider than the rank of M; the power iteration's intermediate bases only stabilise it
    // Deflation of a sketch wider than the operand's numerical rank (r05).  The signals this library is for compress to bonds of
    // 4 ... 20 while the sketch has k + p = 25 ... 133 columns: Y = M Omega then has numerical rank r << l, the columns of Q
    // beyond a basis of range(Y) are orthonormalised rounding noise -- orthogonal to range(M), so their rows of B = Q^H M
    // vanish to rounding and no cutoff >= 1e-24 keeps them -- and every later product and QR carried them at full price (n = 30,
    // rank-4 signal: 6 products of 32768 x 32768 x 133 where 32768 x 32768 x 8 do).  Columns j with |r_jj| <= 1e-13 max |r_ii|
    // leave the basis (R's diagonal is read back: one small transfer); the kept ones are a basis of range(Y) because QR without
    // pivoting gives r_jj = 0 exactly for a column that lies in the span of its predecessors.
    int64_t l = l0;
    {
        void* Rq = nullptr;
        QIL_TRY(tmp.alloc((size_t)(l0 * l0) * e, &Rq));
        QIL_TRY(qil_dev_qr_positive(ctx, dt, m, l0, Y, m, Rq, l0, q == 0));             // Q (:83)
        lap("qr(Y)");
        if (l0 <= 1024 && l0 >= 8) {
            std::vector<double> d2((size_t)l0);
            QIL_TRY(qil_dev_diag_abs2(ctx, dt, Rq, l0, l0, d2.data()));
            double dmax = 0;
            for (double v : d2) dmax = std::max(dmax, v);
            std::vector<int64_t> keep;
            for (int64_t j = 0; j < l0; ++j)
                if (d2[(size_t)j] > 1e-26 * dmax && d2[(size_t)j] > 0.0) keep.push_back(j);
            if (keep.empty()) keep.push_back(0);
            // never fewer columns than the caller's mindim keeps (the reference's svd(B; mindim) returns mindim
            // columns whatever the spectrum, rsvd.jl:103-111): dropped columns come back in index order (they are orthonormal
            // columns of Q like the others)
            if ((int64_t)keep.size() < std::min<int64_t>(mindim, l0)) {
                std::vector<char> in((size_t)l0, 0);
                for (int64_t j : keep) in[(size_t)j] = 1;
                for (int64_t j = 0; j < l0 && (int64_t)keep.size() < std::min<int64_t>(mindim, l0); ++j)
                    if (!in[(size_t)j]) keep.push_back(j);
                std::sort(keep.begin(), keep.end());
            }
            if ((int64_t)keep.size() < l0) {
                for (size_t t = 0; t < keep.size(); ++t)                                 // compact the kept columns to the front (usually a prefix already)
                    if (keep[t] != (int64_t)t)
                        QIL_TRY(qil_dev_copy(ctx, static_cast<char*>(Y) + (size_t)t * (size_t)m * e,
                                             static_cast<const char*>(Y) + (size_t)keep[t] * (size_t)m * e, (size_t)m * e));
                l = (int64_t)keep.size();
                if (dbg) fprintf(stderr, "[rsvd] %lld x %lld: sketch of %lld columns has numerical rank %lld: deflated\n", (long long)m, (long long)n, (long long)l0, (long long)l);
            }
        }
        tmp.free(Rq);
    }
    if (route) rsvd_route_line(m, n, l0, l);
    if (q > 0) QIL_TRY(tmp.alloc((size_t)(n * l) * e, &Zq));
    for (int it = 0; it < q; ++it) {                                                    // :86-95
        QIL_TRY(qil_dev_gemm(ctx, dt, 3, 0, n, l, m, Z, n, Y, m, Zq, n));               // M^H Q = conj(Z) Q
        QIL_TRY(qil_dev_qr_positive(ctx, dt, n, l, Zq, n, nullptr, 0));
        QIL_TRY(qil_dev_gemm(ctx, dt, 1, 0, m, l, n, Z, n, Zq, n, Y, m));               // M Qz
        QIL_TRY(qil_dev_qr_positive(ctx, dt, m, l, Y, m, nullptr, 0, it + 1 == q));
        lap("power iteration (2 products + 2 QRs)");
    }
    tmp.free(Om);
    tmp.free(Zq);                                                                       // (none without a power iteration)
    QIL_TRY(tmp.alloc((size_t)(n * l) * e, &Bt));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 3, n, l, m, Z, n, Y, m, Bt, n));                   // B^T = Z conj(Q) (:98)
    lap("B^T = Z conj(Q)");
    // B^T = Ub Sb Vbh  =>  Uhat = Vbh^T,  (S V^h)^T = Ub Sb
    int64_t r = 0;
    void *UbS = nullptr, *Vbh = nullptr;
    QIL_TRY(svd_trunc_dev(ctx, dt, n, l, Bt, n, cutoff, true, maxdim, mindim, 1, &r, &UbS, &Vbh, S_out));  // :103
    tmp.own(UbS);
    tmp.own(Vbh);
    tmp.free(Bt);
    void* L = nullptr;
    QIL_TRY(tmp.alloc((size_t)(r * m) * e, &L));
    lap("svd(B^T)");
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 1, r, m, l, Vbh, r, Y, m, L, r));                  // U_M^T = Vbh Q^T (:114)
    lap("U^T = Vbh Q^T");
    tmp.free(Vbh);
    tmp.free(Y);
    *rank = r;
    *left = tmp.give(L);
    *right = tmp.give(UbS);  // first r columns, ld n
    return QIL_OK;
}

struct EncodeParams {
    int method;
    double cutoff;
    int64_t maxdim, k, p;
    int q;
    uint64_t seed;
    int64_t mindim;
};

// _tensor_to_mps_rsvd recursion (SignalConverters.jl:145-184).  Chunk layout (fastest -> slowest):
// (rb, s_last, ..., s_first, lb) == M^T column-major for the split (lb, left sites | right sites, rb),
// with M's row index ordered (s_mid fastest, ..., s_first, lb) and its column index (rb fastest,
// s_last, ..., s_mid+1).  Both children come out in the same chunk layout with no transposition:
// left = U_M^T (k x rows), right = (S V^h)^T (cols x k).
// Sub-trees of the bisection are independent: with `defer`, the children of the nodes at depth `defer_depth - 1` are not
// descended into but recorded, and the caller runs them concurrently (qil_run_batch_on) -- below the first splits every
// node is a short chain of small factorisations.
// The call consumes X.  What it leaves behind -- the finished sites and the operands of the deferred sub-trees -- belongs to
// `keep`, a scratch of the same context, so a failure anywhere in the tree strands nothing.
struct TtTask {
    void* X;
    int64_t lb, rb, first, last;
};
int compress_tt(qil_context* ctx, int dt, qil_scratch& keep, void* X, int64_t lb, int64_t rb, int64_t first, int64_t last,
                const EncodeParams& P, std::vector<void*>& sites, std::vector<int64_t>& dims, int depth = 0,
                std::vector<TtTask>* defer = nullptr, int defer_depth = 0) {
    qil_scratch tmp(ctx);
    tmp.own(X);
    const size_t e = qil_elem_size(dt);
    if (first == last) {
        void* A = nullptr;
        QIL_TRY(keep.alloc((size_t)(lb * 2 * rb) * e, &A));
        if (dt == QIL_C64)
            QIL_TRY((qil_klaunch<site_from_chunk_k<c64>>(ctx, dim3(nblk(2 * lb * rb)), dim3(256), 0, (const c64*)X, (int)lb, (int)rb, (c64*)A)));
        else
            QIL_TRY((qil_klaunch<site_from_chunk_k<double>>(ctx, dim3(nblk(2 * lb * rb)), dim3(256), 0, (const double*)X, (int)lb, (int)rb, (double*)A)));
        QIL_HIP(hipGetLastError());
        sites[(size_t)first] = A;
        dims[(size_t)first] = lb;
        dims[(size_t)first + 1] = rb;
        return QIL_OK;
    }
    const int64_t mid = (first + last + 1) / 2 - 1;  // 1-based (first+last-1) div 2, SignalConverters.jl:161
    const int64_t m = lb << (mid - first + 1), n = rb << (last - mid);
    int64_t r = 0;
    void *L = nullptr, *R = nullptr;
    // explicit cutoff/maxdim override the rsvd defaults (SignalConverters.jl:133)
    QIL_TRY(rsvd_rowmajor(ctx, dt, m, n, X, P.k, P.p, P.q, P.seed, P.cutoff, P.maxdim, P.mindim, &r, &L, &R,
                          nullptr));
    tmp.own(L);
    tmp.own(R);
    tmp.free(X);
    if (defer && depth + 1 == defer_depth) {
        defer->push_back(TtTask{keep.own(tmp.give(L)), lb, r, first, mid});
        defer->push_back(TtTask{keep.own(tmp.give(R)), r, rb, mid + 1, last});
        return QIL_OK;
    }
    QIL_TRY(compress_tt(ctx, dt, keep, tmp.give(L), lb, r, first, mid, P, sites, dims, depth + 1, defer, defer_depth));
    QIL_TRY(compress_tt(ctx, dt, keep, tmp.give(R), r, rb, mid + 1, last, P, sites, dims, depth + 1, defer, defer_depth));
    return QIL_OK;
}

// The whole bisection.  The nodes of one level are independent, and so are the sub-trees below any level: the first
// `par_depth` levels run level by level, the nodes of a level concurrently on the context's streams (qil_run_batch_on), and
// the 2^par_depth sub-trees below them concurrently, each as a sequential recursion.  Same kernels on the same operands in
// every order, so the MPS is bit-identical to the sequential recursion (QIL_ENCODE_PAR_DEPTH=0).
// Who owns what: `keep` is the caller's scratch on the home context; X, every task that has not started and everything a level
// has brought home are listed there.  A task that starts belongs to its node, whose scratch on the working context holds what
// the node produces until the node has succeeded.  A block is in no scratch while qil_ctx_transfer moves it.
static int compress_tt_root(qil_context* ctx, int dt, qil_scratch& keep, void* X, int64_t n, const EncodeParams& P,
                            std::vector<void*>& sites, std::vector<int64_t>& dims) {
    const int par_depth = getenv("QIL_ENCODE_PAR_DEPTH") ? atoi(getenv("QIL_ENCODE_PAR_DEPTH")) : 3;   // tuning aid (read per call); 0 = off
    // (a context that is already one slot of a batch -- qil_signal_mps_batch -- encodes sequentially)
    if (par_depth <= 0 || n < 16 || ctx->parent || ctx->lending)
        return compress_tt(ctx, dt, keep, keep.give(X), 1, 1, 0, n - 1, P, sites, dims);
    std::vector<TtTask> frontier{TtTask{X, 1, 1, 0, n - 1}};
    int s = QIL_OK;
    for (int level = 0; level <= par_depth && !frontier.empty() && s == QIL_OK; ++level) {
        const bool whole = level == par_depth;               // last pass: every task is a whole sub-tree
        const int64_t nt = (int64_t)frontier.size();
        std::vector<qil_context*> where((size_t)nt, ctx);
        std::vector<std::vector<int64_t>> tdims((size_t)nt, std::vector<int64_t>(dims.size(), 1));
        std::vector<std::vector<TtTask>> kids((size_t)nt);
        std::vector<char> started((size_t)nt, 0);            // (the batch skips the tasks of a slot it could not set up)
        auto node = [&](int64_t j, qil_context* work) {
            const TtTask& t = frontier[(size_t)j];
            started[(size_t)j] = 1;
            qil_scratch made(work);
            const int st = compress_tt(work, dt, made, t.X, t.lb, t.rb, t.first, t.last, P, sites, tdims[(size_t)j], 0,
                                       whole ? nullptr : &kids[(size_t)j], 1);
            if (st == QIL_OK) {                                  // the level's collection takes over what the node made
                for (int64_t i = t.first; i <= t.last; ++i) made.give(sites[(size_t)i]);
                for (const TtTask& c : kids[(size_t)j]) made.give(c.X);
            } else {                                             // `made` frees it
                std::fill(sites.begin() + t.first, sites.begin() + t.last + 1, nullptr);
                kids[(size_t)j].clear();
            }
            return st;
        };
        for (const TtTask& t : frontier) keep.give(t.X);
        if (nt == 1)
            s = node(0, ctx);
        else
            s = qil_run_batch_on(
                ctx, nt,
                [&](int64_t j, qil_context* slot) {
                    qil_ctx_transfer(ctx, slot, frontier[(size_t)j].X);
                    where[(size_t)j] = slot;
                },
                node);
        // everything the level produced comes home: finished sites, and the operands of the next level
        std::vector<TtTask> next;
        for (int64_t j = 0; j < nt; ++j) {
            const TtTask& t = frontier[(size_t)j];
            if (!started[(size_t)j]) {
                qil_ctx_transfer(where[(size_t)j], ctx, t.X);
                keep.own(t.X);
            }
            for (int64_t i = t.first; i <= t.last; ++i)
                if (sites[(size_t)i] && (whole || t.first == t.last)) {
                    qil_ctx_transfer(where[(size_t)j], ctx, sites[(size_t)i]);
                    keep.own(sites[(size_t)i]);
                    dims[(size_t)i] = tdims[(size_t)j][(size_t)i];
                    dims[(size_t)i + 1] = tdims[(size_t)j][(size_t)i + 1];
                }
            for (const TtTask& c : kids[(size_t)j]) {
                qil_ctx_transfer(where[(size_t)j], ctx, c.X);
                keep.own(c.X);
                next.push_back(c);
            }
        }
        frontier.swap(next);
    }
    return s;
}

// _tensor_to_mps_svd (SignalConverters.jl:77-98).  The carried tensor X[(s_n..s_i), alpha] is viewed
// for free as Y[low, (s_i, alpha)] = M^T (L x 2r): the Jacobi SVD rotates its 2r columns, the site
// tensor is V_y^h permuted, and the carry S V^h is U_y S -- already in the layout of the next step.
// The sweep consumes X; the finished sites belong to `keep` (as in compress_tt).
int svd_sweep(qil_context* ctx, int dt, qil_scratch& keep, void* X, int64_t n, const EncodeParams& P, std::vector<void*>& sites,
              std::vector<int64_t>& dims) {
    qil_scratch tmp(ctx);
    tmp.own(X);
    const size_t e = qil_elem_size(dt);
    int64_t r = 1;
    dims[0] = 1;
    for (int64_t i = 0; i + 1 < n; ++i) {
        const int64_t L = 1LL << (n - 1 - i);
        int64_t k = 0;
        void *UyS = nullptr, *Vyh = nullptr;
        QIL_TRY(svd_trunc_dev(ctx, dt, L, 2 * r, X, L, P.cutoff, true, P.maxdim, 1, 1, &k, &UyS, &Vyh, nullptr));
        tmp.own(UyS);
        tmp.own(Vyh);
        tmp.free(X);
        void* A = nullptr;
        QIL_TRY(keep.alloc((size_t)(r * 2 * k) * e, &A));
        if (dt == QIL_C64)
            QIL_TRY((qil_klaunch<site_from_vh_k<c64>>(ctx, dim3(nblk(2 * r * k)), dim3(256), 0, (const c64*)Vyh, (long long)k, (int)r, (int)k, (c64*)A)));
        else
            QIL_TRY((qil_klaunch<site_from_vh_k<double>>(ctx, dim3(nblk(2 * r * k)), dim3(256), 0, (const double*)Vyh, (long long)k, (int)r, (int)k, (double*)A)));
        QIL_HIP(hipGetLastError());
        tmp.free(Vyh);
        sites[(size_t)i] = A;
        dims[(size_t)i + 1] = k;
        X = UyS;  // (L x k): X'[(s_n..s_{i+1}), alpha']
        r = k;
    }
    // last site: X[(s_n), alpha] -> A[alpha, s_n, 1]  == chunk layout with rb = 1
    void* A = nullptr;
    QIL_TRY(keep.alloc((size_t)(r * 2) * e, &A));
    if (dt == QIL_C64)
        QIL_TRY((qil_klaunch<site_from_chunk_k<c64>>(ctx, dim3(1), dim3(256), 0, (const c64*)X, (int)r, 1, (c64*)A)));
    else
        QIL_TRY((qil_klaunch<site_from_chunk_k<double>>(ctx, dim3(1), dim3(256), 0, (const double*)X, (int)r, 1, (double*)A)));
    QIL_HIP(hipGetLastError());
    sites[(size_t)n - 1] = A;
    dims[(size_t)n] = 1;
    return QIL_OK;
}

int signal_mps_impl(qil_context* ctx, const void* x, int64_t len, int dtype, const EncodeParams& P,
                    qil_mps** out) {
    QIL_REQUIRE(ctx && x && out, QIL_EINVAL_ARG, "signal_mps: null argument");
    QIL_REQUIRE(dtype == QIL_F64 || dtype == QIL_C64, QIL_EINVAL_ARG, "signal_mps: unknown dtype %d", dtype);
    QIL_REQUIRE(P.method == QIL_METHOD_SVD || P.method == QIL_METHOD_RSVD, QIL_EINVAL_ARG,
                "tensor_to_mps: unknown method %d. Use :svd or :rsvd.", P.method);
    QIL_REQUIRE(len >= 1, QIL_EINVAL_LENGTH, "signal_mps: empty signal");
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    // _array_to_tensor (SignalConverters.jl:16-46): n = round(log2 N), zero-fill, normalise
    const int64_t n = std::max<int64_t>(1, (int64_t)std::llround(std::log2((double)len)));
    const int64_t N = 1LL << n;
    QIL_REQUIRE(len <= N, QIL_EINVAL_LENGTH,
                "_array_to_tensor: Length of signal vector must be a power of 2 (got %lld)", (long long)len);
    // upload the raw samples, zero-fill the tail, then norm + scale ON THE DEVICE (the host never makes
    // a pass over the 2^n samples)
    const int ncomp = dtype == QIL_C64 ? 2 : 1;
    const size_t e = qil_elem_size(dtype);
    void* X = nullptr;
    QIL_TRY(tmp.alloc((size_t)N * e, &X));
    // `x` may live on the host or already in HBM (unified addressing resolves the direction).  Samples that are ALREADY on this
    // device and fill the register (an n = 30 signal: 8.6 GB) are not copied first: the norm reads them in place and the scaled
    // copy is written in one pass (r05: copy + norm + scale in place moved 43 GB through HBM, 9 ms; now 26 GB)
    bool in_place = false;
    if (len == N) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, x) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == ctx->device) in_place = true;
        else (void)hipGetLastError();
    }
    if (!in_place) {
        QIL_HIP(hipMemcpyAsync(X, x, (size_t)len * e, hipMemcpyDefault, qil_stream(ctx)));
        if (len < N)
            QIL_TRY(qil_dev_zero(ctx, static_cast<char*>(X) + (size_t)len * e, (size_t)(N - len) * e));
    }
    const void* src = in_place ? x : X;
    void* part = nullptr;
    constexpr int kPartBlocks = 1024;
    QIL_TRY(tmp.alloc(kPartBlocks * sizeof(double), &part));
    QIL_TRY((qil_klaunch<sumsq_partial_k>(ctx, dim3(kPartBlocks), dim3(256), 0, (const double*)src, (long long)(N * ncomp), (double*)part)));
    std::vector<double> ph(kPartBlocks);
    QIL_TRY(qil_read_back(ctx, ph.data(), part, kPartBlocks * sizeof(double)));   // also completes the upload of caller memory `x`
    double ss = 0;
    for (double v : ph) ss += v;                  // fixed order: deterministic
    double amp = std::sqrt(ss);
    if (ss == 0.0 || std::isinf(ss)) {
        // every x^2 underflowed to zero (samples below about 1e-162) or the sum overflowed (samples from about 1e+154), or the
        // signal is zero or holds an Inf: the reference's norm(x) (SignalConverters.jl:36) scales, so finite samples must
        // encode.  Two more passes, on this path only: max |x|, then the same sum over s x with s the power of two that brings
        // the maximum into [1/2, 1) (s x is exact).  A NaN makes ss NaN and never comes here; every other signal takes the
        // plain sum above, bit for bit as before -- also samples of 1e-155 ... 1e-162, whose squares are subnormal: their sum is
        // non-zero with few bits, so the amplitude is coarse and the state not normalised, while amplitude * state stays right.
        QIL_TRY((qil_klaunch<sumsq_rescue_k>(ctx, dim3(kPartBlocks), dim3(256), 0, (const double*)src, (long long)(N * ncomp), 1.0, 0, (double*)part)));
        QIL_TRY(qil_read_back(ctx, ph.data(), part, kPartBlocks * sizeof(double)));
        double mx = 0;
        for (double v : ph) mx = std::max(mx, v);
        if (mx > 0 && std::isfinite(mx)) {
            int ex = 0;
            (void)std::frexp(mx, &ex);
            const int sh = std::min(-ex, 1023);
            QIL_TRY((qil_klaunch<sumsq_rescue_k>(ctx, dim3(kPartBlocks), dim3(256), 0, (const double*)src, (long long)(N * ncomp), std::ldexp(1.0, sh), 1, (double*)part)));
            QIL_TRY(qil_read_back(ctx, ph.data(), part, kPartBlocks * sizeof(double)));
            ss = 0;
            for (double v : ph) ss += v;
            amp = std::ldexp(std::sqrt(ss), -sh);
        }
    }
    tmp.free(part);
    QIL_REQUIRE(amp > 0 && std::isfinite(amp) && std::isfinite(1.0 / amp), QIL_EINVAL_ARG,
                "signal_mps: signal has zero or non-finite norm");
    if (in_place) {
        QIL_TRY((qil_klaunch<scale_copy_k>(ctx, dim3(nblk(N * ncomp)), dim3(256), 0, (const double*)x, (double*)X, (long long)(N * ncomp), 1.0 / amp)));
        QIL_HIP(qil_stream_sync(ctx));             // `x` is caller memory: read completely before anything else can return
    } else
        QIL_TRY((qil_klaunch<scale_inplace_k>(ctx, dim3(nblk(N * ncomp)), dim3(256), 0, (double*)X, (long long)(N * ncomp), 1.0 / amp)));
    QIL_HIP(hipGetLastError());
    std::vector<void*> sites((size_t)n, nullptr);
    std::vector<int64_t> dims((size_t)n + 1, 1);
    // the encoders consume X; the sites they finish are in tmp, on this context, until the handle adopts them
    if (n == 1)
        sites[0] = X;                                      // single site: A[1, s, 1] = x_hat[s]
    else if (P.method == QIL_METHOD_SVD)
        QIL_TRY(svd_sweep(ctx, dtype, tmp, tmp.give(X), n, P, sites, dims));
    else
        QIL_TRY(compress_tt_root(ctx, dtype, tmp, X, n, P, sites, dims));
    for (void* p : sites) QIL_REQUIRE(p && tmp.give(p), QIL_EHIP, "signal_mps: internal error, a finished site is not in the call's scratch");
    qil_mps* psi = qil_mps_empty(ctx, n, dtype, 0, nullptr, amp);
    psi->dims = dims;
    for (size_t i = 0; i < sites.size(); ++i) qil_chain_adopt(psi, (int64_t)i, sites[i]);
    *out = psi;
    return QIL_OK;
}


// ---------------------------------------------------------------- fused apply-and-truncate (zip-up) kernels
__device__ __forceinline__ c64 zmul(c64 a, c64 b) { return c64{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ c64 zmul(c64 a, double b) { return c64{a.re * b, a.im * b}; }
__device__ __forceinline__ double zmul(double a, double b) { return a * b; }
__device__ __forceinline__ c64 zadd(c64 a, c64 b) { return c64{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ double zadd(double a, double b) { return a + b; }

// X[r, a, s', beta] = sum_alpha Rm[r, alpha, a] * A[alpha, s', beta]      (Rm index: r + R*(alpha + cl*a))
template <class TO, class TA>
__device__ __forceinline__ void zip_stage1_body(const uint3 blockIdx, const uint3 gridDim, const TO* __restrict__ Rm, const TA* __restrict__ A, TO* __restrict__ X, int R, int Dl,
                           int cl, int cr) {
    const long long total = (long long)R * Dl * 2 * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        long long u = t;
        const int r = (int)(u % R);
        u /= R;
        const int a = (int)(u % Dl);
        u /= Dl;
        const int sp = (int)(u & 1);
        const int beta = (int)(u >> 1);
        const TO* rp = Rm + r + (long long)R * cl * a;
        const TA* ap = A + (long long)cl * (sp + 2LL * beta);
        TO acc{};
        for (int al = 0; al < cl; ++al) acc = zadd(acc, zmul(rp[(long long)R * al], ap[al]));
        X[t] = acc;
    }
}
template <class TO, class TA>
struct zip_stage1_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        zip_stage1_body<TO, TA>(b, g, a...);
    }
};

// theta[(r, s), (beta, b)] = sum_{a, s'} X[r, a, s', beta] * W[a, s', s, b]
template <class TO, class TW>
__device__ __forceinline__ void zip_stage2_body(const uint3 blockIdx, const uint3 gridDim, const TO* __restrict__ X, const TW* __restrict__ W, TO* __restrict__ theta, int R, int Dl,
                           int Dr, int cr) {
    const long long total = (long long)R * 2 * cr * Dr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        long long u = t;
        const int r = (int)(u % R);
        u /= R;
        const int s_ = (int)(u & 1);
        u >>= 1;
        const int beta = (int)(u % cr);
        const int b = (int)(u / cr);
        TO acc{};
        for (int sp = 0; sp < 2; ++sp) {
            const TO* xp = X + r + (long long)R * Dl * (sp + 2LL * beta);            // + R * a
            const TW* wp = W + (long long)Dl * (sp + 2 * (s_ + 2LL * b));            // + a
            for (int a = 0; a < Dl; ++a) acc = zadd(acc, zmul(xp[(long long)R * a], wp[a]));
        }
        theta[t] = acc;
    }
}
template <class TO, class TW>
struct zip_stage2_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        zip_stage2_body<TO, TW>(b, g, a...);
    }
};

template <class TO, class TW, class TA>
int zip_theta(qil_context* ctx, const void* Rm, const void* W, const void* A, int R, int Dl, int Dr, int cl, int cr,
              void** theta_out) {
    qil_scratch tmp(ctx);
    void *X = nullptr, *th = nullptr;
    QIL_TRY(tmp.alloc((size_t)R * Dl * 2 * cr * sizeof(TO), &X));
    QIL_TRY(tmp.alloc((size_t)R * 2 * cr * Dr * sizeof(TO), &th));
    QIL_TRY((qil_klaunch<zip_stage1_k<TO, TA>>(ctx, dim3(nblk((long long)R * Dl * 2 * cr)), dim3(256), 0, (const TO*)Rm, (const TA*)A, (TO*)X, R, Dl, cl, cr)));
    QIL_TRY((qil_klaunch<zip_stage2_k<TO, TW>>(ctx, dim3(nblk((long long)R * 2 * cr * Dr)), dim3(256), 0, (const TO*)X, (const TW*)W, (TO*)th, R, Dl, Dr, cr)));
    QIL_HIP(hipGetLastError());
    *theta_out = tmp.give(th);                          // (X goes back with tmp)
    return QIL_OK;
}

// Z[(alpha, a), (s, r')] = sum_{s', b} Y[alpha, s', b, r'] W[a, s', s, b]     (right environment of the fit sweep)
//   Y index (alpha + cl s') + 2 cl (b + Dr r'),  W index a + Dl (s' + 2 (s + 2 b)),  Z index (alpha + cl a) + cl Dl (s + 2 r')
template <class T>
__device__ __forceinline__ void fit_env_stage_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ Y, const T* __restrict__ W, T* __restrict__ Z, int cl, int Dl,
                              int Dr, int rp) {
    const long long total = (long long)cl * Dl * 2 * rp;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        long long u = t;
        const int alpha = (int)(u % cl);
        u /= cl;
        const int a = (int)(u % Dl);
        u /= Dl;
        const int s_ = (int)(u & 1);
        const int r = (int)(u >> 1);
        T acc{};
        for (int sp = 0; sp < 2; ++sp) {
            const T* yp = Y + (alpha + (long long)cl * sp) + 2LL * cl * Dr * r;        // + 2 cl b
            const T* wp = W + a + (long long)Dl * (sp + 2 * s_);                       // + 4 Dl b
            for (int b = 0; b < Dr; ++b) acc = zadd(acc, zmul(yp[2LL * cl * b], wp[4LL * Dl * b]));
        }
        Z[t] = acc;
    }
}
template <class T>
struct fit_env_stage_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        fit_env_stage_body<T>(b, g, a...);
    }
};

__device__ __forceinline__ void widen_f64_body(const uint3 blockIdx, const uint3 gridDim, const double* __restrict__ in, c64* __restrict__ out, long long n) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x)
        out[t] = c64{in[t], 0.0};
}
struct widen_f64_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        widen_f64_body(b, g, a...);
    }
};

}  // namespace

// the exact QR gauge sweep for the other translation units (qil_spectra.hip): canonicalize_impl(c, direction, center, 0, none,
// gauge_qr = true).  Context active, call scope open.
int qil_gauge_exact(qil_chain* c, int direction, int64_t center) {
    return canonicalize_impl(c, direction, center, 0.0, kNoCap, true);
}

// ---------------------------------------------------------------- exported
extern "C" int qil_canonicalize(qil_mps* psi, int direction, int64_t center, double cutoff, int64_t maxdim) {
    QIL_REQUIRE(psi, QIL_EINVAL_ARG, "canonicalize!: null handle");
    QIL_REQUIRE(direction == QIL_DIR_RIGHT || direction == QIL_DIR_LEFT, QIL_EINVAL_ARG,
                "Direction must be :right or :left");
    QIL_TRY(qil_ctx_activate(psi->ctx));
    qil_call_scope call_scope(psi->ctx);
    // the ZTMPS method forwards `center` unchanged to the 2n-site chain (mps.jl:880-881)
    return canonicalize_impl(psi, direction, center, cutoff, maxdim);
}

// right_canonical: the caller guarantees every site but the first is a right isometry (the fused apply-and-truncate
// after its variational sweep).  canonicalize!(:left) of such a state can neither truncate nor change anything but the
// gauge (all its singular values are 1), so it is not run.
static int compress_impl(qil_mps* psi, int64_t maxdim, double tol, int sweeps, bool right_canonical) {
    QIL_REQUIRE(psi, QIL_EINVAL_ARG, "compress!: null handle");
    const int64_t N = psi->n();
    QIL_REQUIRE(N >= 2, QIL_EDOMAIN, "SignalMPS must have at least 2 sites.");   // mps.jl:918
    QIL_REQUIRE(sweeps >= 1, QIL_EINVAL_ARG, "compress!: sweeps must be >= 1");
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int dt = psi->dtype;
    const double cutoff = tol * tol / ((double)(N - 1) * sweeps);               // mps.jl:920
    if (!right_canonical) QIL_TRY(canonicalize_impl(psi, QIL_DIR_LEFT, 0, 1e-12, kNoCap));            // mps.jl:923
    // The reference truncates the two-site tensor psi[j] psi[j+1] (mps.jl:929, :946).  In canonical gauge --
    // which every step of the sweep maintains -- that tensor has the same singular values and the same kept
    // subspace as the single site next to the orthogonality centre (its neighbour is an isometry), so each
    // sweep is run as a truncating gauge sweep on one-site matrices: (2 chi_l x chi) instead of
    // (2 chi_l x 2 chi_r), no theta product, and the Jacobi SVD rotates half as many columns.
    for (int sw = 0; sw < sweeps; ++sw) {
        QIL_TRY(canonicalize_impl(psi, QIL_DIR_RIGHT, 0, cutoff, maxdim));      // L -> R: U | S V   (mps.jl:927-942)
        QIL_TRY(canonicalize_impl(psi, QIL_DIR_LEFT, 0, cutoff, maxdim));       // R -> L: U S | V   (mps.jl:944-959)
    }
    // mps.jl:963 re-gauges once more (canonicalize!(:left), cutoff 1e-12).  The sweep that just ended left every site
    // but the first an isometry (all its singular values are 1), so that pass can neither truncate nor change anything
    // but the gauge -- it is not run.
    double nrm = 0;
    QIL_TRY(qil_norm(psi, &nrm));                                               // mps.jl:967-971
    if (nrm != 0) {
        psi->amplitude *= nrm;
        const double inv = 1.0 / nrm;
        std::vector<double> s((size_t)psi->dims[1], inv);
        QIL_TRY(qil_dev_scale(ctx, dt, 1, 2 * psi->dims[0], psi->dims[1], psi->site[0], 2 * psi->dims[0], s.data()));
    }
    return QIL_OK;
}

extern "C" int qil_compress(qil_mps* psi, int64_t maxdim, double tol, int sweeps) {
    return compress_impl(psi, maxdim, tol, sweeps, false);
}

// ---------------------------------------------------------------- steps the fused routes share
// Default intermediate bond cap of the zip-up and the variational sweep: maxdim + 16.  With the variational sweep behind it the zip-up
// only has to deliver a basis that contains the kept space: an oversampling of 16 columns gives the same verdicts as 2 maxdim
// (r01), max(1.5 maxdim, maxdim + 16) (r02/r03) -- 200 random flat-spectrum products with maxdim 8 ... 128 each, 0 bad
// (tools/_fuzz_product_compress.py, QIL_FUZZ_ZIP=plus16) -- and the oracle tests, while an oversampling of 4 (1.5 maxdim at
// maxdim = 8) fails 2 of 200.  Bench product, maxdim 64: cap 96 117 ms, cap 80 108.6 ms (MEASUREMENTS R04.7).
// The evidence covers maxdim <= 128 with flat spectra only: beyond that a relative floor of 1.125 maxdim
// keeps the oversampling proportional (maxdim 256: 288, 512: 576) until a slowly-decaying case at that size is fuzzed.
static int64_t zip_default_cap(int64_t maxdim) {
    const int64_t zip_over = 16;
    return maxdim > kNoCap / 2 ? kNoCap : std::max(maxdim + zip_over, maxdim + (maxdim + 7) / 8);
}

// Sketch matrix for capped bonds (om_ld x zip_maxdim; one for the whole call: any sub-block of a Gaussian matrix is Gaussian);
// *Om stays null when no bond of the call (the widest is om_ld) exceeds the cap.
static int zip_sketch(qil_scratch& scratch, int dt, int64_t om_ld, int64_t zip_maxdim, void** Om) {
    *Om = nullptr;
    if (zip_maxdim >= om_ld) return QIL_OK;
    QIL_TRY(scratch.alloc((size_t)(om_ld * zip_maxdim) * qil_elem_size(dt), Om));
    return qil_dev_fill_normal(scratch.ctx, dt, *Om, om_ld * zip_maxdim, 0x51b0e7c5ull, 1.0);
}

// One zip-up step: theta (rows x Pc, left intact) -> the provisional site U (rows x r, orthonormal columns) and the next
// environment SV = U^H theta (r x Pc), both fresh pool blocks the caller owns.
// Capped bond: an orthonormal basis of theta Omega (Omega: Pc x zip_maxdim, seeded Gaussian) instead of theta's truncated
// SVD -- the variational sweep re-optimises every site anyway, and with it the sketched zip-up reproduces the oracle's
// compress!(apply) on all 24 random products exactly as the SVD one does (numpy prototype, then tests); one GEMM + one thin QR +
// one GEMM instead of a 2r x D chi SVD.  Otherwise: the truncated SVD at zip_cutoff.
static int zip_step(qil_context* ctx, int dt, int64_t rows, int64_t Pc, void* theta, int64_t zip_maxdim, double zip_cutoff,
                    const void* Om, int64_t om_ld, int64_t* r, void** U, void** SV) {
    if (zip_maxdim >= std::min(rows, Pc))
        return svd_trunc_dev(ctx, dt, rows, Pc, theta, rows, zip_cutoff, true, zip_maxdim, 1, 2, r, U, SV, nullptr);
    const size_t e = qil_elem_size(dt);
    const int64_t k = zip_maxdim;
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(rows * k) * e, U));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, rows, k, Pc, theta, rows, Om, om_ld, *U, rows));
    QIL_TRY(qil_dev_qr_positive(ctx, dt, rows, k, *U, rows, nullptr, 0, true));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)(k * Pc) * e, SV));
    QIL_TRY(qil_dev_gemm(ctx, dt, dt == QIL_C64 ? 2 : 1, 0, k, Pc, rows, *U, rows, theta, rows, *SV, k));
    *r = k;
    return QIL_OK;
}

// *out = a fresh block with the ne real numbers at src as c64 (a real operand of a complex result is widened once: KB..MB)
static int widen_site(qil_context* ctx, const void* src, long long ne, void** out) {
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)ne * sizeof(c64), out));
    return qil_klaunch<widen_f64_k>(ctx, dim3(nblk(ne)), dim3(256), 0, (const double*)src, (c64*)*out, ne);
}

// a few doubles to a fresh block owned by `scratch`, complete on return (the source may die with the caller's frame)
static int upload_small(qil_scratch& scratch, const double* host, size_t n, void** p) {
    QIL_TRY(scratch.alloc(n * sizeof(double), p));
    QIL_HIP(hipMemcpyAsync(*p, host, n * sizeof(double), hipMemcpyHostToDevice, qil_stream(scratch.ctx)));
    QIL_HIP(qil_stream_sync(scratch.ctx));
    return QIL_OK;
}

// Fused apply-and-truncate: compress!(apply(W, psi); maxdim, tol, sweeps) WITHOUT ever writing the
// (D chi)^2 product tensors.
//   1. zip-up: psi is brought to right-canonical gauge (a copy); one left-to-right sweep carries the left
//      environment L[r, alpha, a] = <phi_{<i} | W psi_{<i}> and per site forms only
//          theta[(r, s), (beta, b)] = sum L[r, alpha, a] W[a, s', s, b] A[alpha, s', beta]      (2 r x D chi)
//      whose truncated SVD (cap zip_maxdim = 2 maxdim, 100x tighter cutoff) gives the site phi_i (U) and the next
//      environment (S V^h).  Its truncations see only psi's gauge, not the operator's right part: on flat-spectrum
//      operands they discard weight the exact route keeps (1e-2 in 5 of 24 random products).
//   2. one variational sweep right to left repairs that: with the left environments of step 1 and right environments
//      R[(beta, b), r'] = <phi_{>i} | W psi_{>i}> built on the way, every site is replaced by the best tensor given the
//      others,  phi_i = L_i A_i W_i R_i  (two small contraction kernels + one GEMM), and re-gauged by a thin QR.  No SVD,
//      nothing of size (D chi)^2.  After it the state agrees with compress!(apply(W, psi)) of the CPU oracle to rounding on
//      22 of the 24 random products and within the truncation's own error on the other two (numpy prototype and
//      tests/test_gpu_parity.py::test_apply_compress_random_products_against_oracle).
//   3. the exact-gauge compress! (src/mps.jl:913-973) fixes the reference's post-conditions (bonds <= maxdim by the
//      ITensors rule, unit norm in the tensors, norm moved into `amplitude`).
// Cost O(n r D chi (D + chi + r)) instead of O(n (D chi)^3).
// `ctx` = working context (stream + pool) of the call: psi's own, or a worker of it (qil_apply_compress_batch); the
// operands are only read
static int apply_compress_on(qil_context* ctx, const qil_mpo* W, const qil_mps* psi, int64_t maxdim, double tol, int sweeps,
                             int64_t zip_maxdim, qil_mps** out) {
    QIL_REQUIRE(W && psi && out, QIL_EINVAL_ARG, "apply_compress: null argument");
    QIL_REQUIRE(W->ctx == psi->ctx, QIL_EINVAL_ARG, "apply: MPO and MPS belong to different contexts");
    QIL_REQUIRE(W->paired == psi->paired, QIL_EINVAL_ARG, "apply: cannot mix paired and single-register operands");
    QIL_REQUIRE(W->n() == psi->n(), QIL_EINVAL_LENGTH,
                "apply: MPO and MPS must have the same number of sites. Found length(W)=%lld, length(psi)=%lld",
                (long long)W->n(), (long long)psi->n());
    QIL_REQUIRE(W->site_ids == psi->site_ids, QIL_EINVAL_SITES, "apply: MPO and MPS must have the same site indices.");
    const int64_t N = psi->n();
    QIL_REQUIRE(N >= 2, QIL_EDOMAIN, "SignalMPS must have at least 2 sites.");
    QIL_REQUIRE(sweeps >= 1, QIL_EINVAL_ARG, "compress!: sweeps must be >= 1");
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    if (maxdim <= 0) maxdim = kNoCap;
    if (zip_maxdim <= 0) zip_maxdim = zip_default_cap(maxdim);
    const double cutoff = tol * tol / ((double)(N - 1) * sweeps);
    const double zip_cutoff = cutoff * 1e-2;
    const bool wc = W->dtype == QIL_C64, ac = psi->dtype == QIL_C64;
    const int odt = (wc || ac) ? QIL_C64 : QIL_F64;
    const size_t e = qil_elem_size(odt);
    const bool fdbg = getenv("QIL_FUSED_DEBUG") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!fdbg) return;
        (void)qil_stream_sync(ctx);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[apply_compress] %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    };
    qil_result_guard<qil_mps> res_own(qil_mps_empty(ctx, N, odt, psi->paired, psi->site_ids.data(), psi->amplitude));
    qil_mps* const res = res_own.p;
    {   // steps 1 and 2; the gauged copy and every temporary are gone before step 3
        // right-canonical copy of psi: the zip's truncations then see (nearly) orthonormal environments
        qil_result_guard<qil_mps> phi_own(nullptr);
        QIL_TRY(qil_mps_clone_to(ctx, psi, &phi_own.p));
        qil_mps* const phi = phi_own.p;
        qil_scratch scratch(ctx);                            // every pool block this call owns outside a handle
        QIL_TRY(canonicalize_impl(phi, QIL_DIR_LEFT, 0, 0.0, kNoCap, true));      // exact thin-QR gauge: psi loses nothing
        // operands in the output dtype
        std::vector<void*> Asite(phi->site), Wsite(W->site), Lenv((size_t)N, nullptr);
        std::vector<int> Rdim((size_t)N + 1, 1);
        for (int64_t i = 0; i < N; ++i) {
            if (odt == QIL_C64 && !ac) {
                QIL_TRY(widen_site(ctx, phi->site[(size_t)i], phi->site_elems(i), &Asite[(size_t)i]));
                scratch.own(Asite[(size_t)i]);
            }
            if (odt == QIL_C64 && !wc) {
                QIL_TRY(widen_site(ctx, W->site[(size_t)i], W->site_elems(i), &Wsite[(size_t)i]));
                scratch.own(Wsite[(size_t)i]);
            }
        }
        auto theta_of = [&](int64_t i, void** theta) -> int {
            const int Dl = (int)W->dims[(size_t)i], Dr = (int)W->dims[(size_t)i + 1];
            const int cl = (int)phi->dims[(size_t)i], cr = (int)phi->dims[(size_t)i + 1];
            if (odt == QIL_F64)
                QIL_TRY((zip_theta<double, double, double>(ctx, Lenv[(size_t)i], Wsite[(size_t)i], Asite[(size_t)i], Rdim[(size_t)i],
                                                           Dl, Dr, cl, cr, theta)));
            else
                QIL_TRY((zip_theta<c64, c64, c64>(ctx, Lenv[(size_t)i], Wsite[(size_t)i], Asite[(size_t)i], Rdim[(size_t)i], Dl, Dr,
                                                  cl, cr, theta)));
            scratch.own(*theta);
            return QIL_OK;
        };
        void* Om = nullptr;
        int64_t om_ld = 1;
        for (int64_t i = 0; i + 1 < N; ++i) om_ld = std::max<int64_t>(om_ld, phi->dims[(size_t)i + 1] * W->dims[(size_t)i + 1]);
        QIL_TRY(zip_sketch(scratch, odt, om_ld, zip_maxdim, &Om));
        const double one[2] = {1.0, 0.0};                // the 1 x 1 environments at both ends
        // ---- 1. zip-up, keeping the left environments
        QIL_TRY(upload_small(scratch, one, e / sizeof(double), &Lenv[0]));
        for (int64_t i = 0; i < N; ++i) {
            const int Dr = (int)W->dims[(size_t)i + 1], cr = (int)phi->dims[(size_t)i + 1];
            const int R = Rdim[(size_t)i];
            void* theta = nullptr;
            QIL_TRY(theta_of(i, &theta));
            if (i + 1 == N) {                       // last site: theta is (R, 2, 1)
                qil_chain_adopt(res, i, scratch.give(theta));
                res->dims[(size_t)i] = R;
                break;
            }
            int64_t r = 0;
            void *U = nullptr, *SV = nullptr;
            QIL_TRY(zip_step(ctx, odt, 2LL * R, (int64_t)cr * Dr, theta, zip_maxdim, zip_cutoff, Om, om_ld, &r, &U, &SV));
            scratch.free(theta);
            qil_chain_adopt(res, i, U);             // [R, s, r]
            res->dims[(size_t)i] = R;
            res->dims[(size_t)i + 1] = r;
            Lenv[(size_t)i + 1] = scratch.own(SV);      // [r, (beta, b)] == L[r, alpha, a] of the next site
            Rdim[(size_t)i + 1] = (int)r;
        }
        lap("gauge + zip-up");
        // ---- 2. variational sweep right to left
        void* Renv = nullptr;                       // [(beta, b), r']
        int rp = 1;
        QIL_TRY(upload_small(scratch, one, e / sizeof(double), &Renv));
        for (int64_t i = N - 1; i >= 0; --i) {
            const int Dl = (int)W->dims[(size_t)i], Dr = (int)W->dims[(size_t)i + 1];
            const int cl = (int)phi->dims[(size_t)i], cr = (int)phi->dims[(size_t)i + 1];
            const int R = Rdim[(size_t)i];
            void *theta = nullptr, *T = nullptr;
            QIL_TRY(theta_of(i, &theta));
            QIL_TRY(scratch.alloc((size_t)2 * R * rp * e, &T));
            QIL_TRY(qil_dev_gemm(ctx, odt, 0, 0, 2LL * R, rp, (int64_t)cr * Dr, theta, 2LL * R, Renv, (int64_t)cr * Dr, T, 2LL * R));
            scratch.free(theta);
            QIL_TRY(qil_chain_set_site(res, i, scratch.give(T), R, rp));
            if (i == 0) break;
            QIL_TRY(gauge_site_left(res, i, 0.0, kNoCap, true));
            const int K = (int)res->dims[(size_t)i];
            void *Y = nullptr, *Z = nullptr, *Rn = nullptr;
            QIL_TRY(scratch.alloc((size_t)2 * cl * Dr * rp * e, &Y));
            QIL_TRY(qil_dev_gemm(ctx, odt, 0, 0, 2LL * cl, (int64_t)Dr * rp, cr, Asite[(size_t)i], 2LL * cl, Renv, cr, Y, 2LL * cl));
            QIL_TRY(scratch.alloc((size_t)cl * Dl * 2 * rp * e, &Z));
            if (odt == QIL_F64)
                QIL_TRY((qil_klaunch<fit_env_stage_k<double>>(ctx, dim3(nblk((long long)cl * Dl * 2 * rp)), dim3(256), 0, (const double*)Y, (const double*)Wsite[(size_t)i], (double*)Z, cl, Dl, Dr, rp)));
            else
                QIL_TRY((qil_klaunch<fit_env_stage_k<c64>>(ctx, dim3(nblk((long long)cl * Dl * 2 * rp)), dim3(256), 0, (const c64*)Y, (const c64*)Wsite[(size_t)i], (c64*)Z, cl, Dl, Dr, rp)));
            QIL_TRY(scratch.alloc((size_t)cl * Dl * K * e, &Rn));
            // R_{i-1}[(alpha, a), k] = sum_{s, r'} Z[(alpha, a), (s, r')] conj(phi_i[k, (s, r')])
            QIL_TRY(qil_dev_gemm(ctx, odt, 0, 2, (int64_t)cl * Dl, K, 2LL * rp, Z, (int64_t)cl * Dl, res->site[(size_t)i], K, Rn,
                                 (int64_t)cl * Dl));
            scratch.free(Y);
            scratch.free(Z);
            scratch.free(Renv);
            Renv = Rn;
            rp = K;
        }
        lap("variational sweep");
    }
    // ---- 3. exact-gauge truncation
    const int st = compress_impl(res, maxdim, tol, sweeps, true);    // the variational sweep left res right-canonical
    lap("compress!");
    QIL_TRY(st);
    *out = res_own.release();
    return QIL_OK;
}

extern "C" int qil_apply_compress(const qil_mpo* W, const qil_mps* psi, int64_t maxdim, double tol, int sweeps,
                                  int64_t zip_maxdim, qil_mps** out) {
    QIL_REQUIRE(W && psi && out, QIL_EINVAL_ARG, "apply_compress: null argument");
    return apply_compress_on(psi->ctx, W, psi, maxdim, tol, sweeps, zip_maxdim, out);
}

extern "C" int qil_apply_compress_batch(const qil_mpo* const* Ws, const qil_mps* const* psis, int64_t nb, int64_t maxdim,
                                        double tol, int sweeps, int64_t zip_maxdim, qil_mps** outs) {
    QIL_REQUIRE(nb >= 0 && ((Ws && psis && outs) || nb == 0), QIL_EINVAL_ARG, "apply_compress_batch: null argument");
    if (nb == 0) return QIL_OK;
    for (int64_t j = 0; j < nb; ++j) {
        outs[j] = nullptr;
        QIL_REQUIRE(Ws[j] && psis[j], QIL_EINVAL_ARG, "apply_compress_batch: item %lld is null", (long long)j);
        QIL_REQUIRE(Ws[j]->ctx && Ws[j]->ctx == psis[0]->ctx && psis[j]->ctx == psis[0]->ctx, QIL_EINVAL_ARG,
                    "apply_compress_batch: item %lld lives in another context", (long long)j);
    }
    const int st = qil_run_batch_on(psis[0]->ctx, nb, nullptr, [&](int64_t j, qil_context* work) {
        return apply_compress_on(work, Ws[j], psis[j], maxdim, tol, sweeps, zip_maxdim, &outs[j]);
    });
    if (st != QIL_OK)                                   // all or nothing: a failed batch hands out no handles
        for (int64_t j = 0; j < nb; ++j) {
            if (outs[j]) qil_mps_destroy(outs[j]);
            outs[j] = nullptr;
        }
    return st;
}

// Fused sum-and-truncate: compress!(sum_j w_j psi_j; maxdim, tol, sweeps) WITHOUT the direct-sum tensors of size (sum chi)^2.
// The structure of apply_compress_on with the terms in the operator's place, on the same steps (zip_default_cap, zip_sketch, zip_step):
//   1. every (distinct) term is copied and brought to right-canonical gauge by exact thin QRs; the weights are the 1 x 1
//      environments the zip-up starts from, so no term tensor is touched for them;
//   2. zip-up left to right: term j carries C_j (r x chi_j), all of them stored concatenated as ONE r x sum(chi) array; per site
//          theta = [C_1 A^1 | C_2 A^2 | ...]     (2r x sum(chi_right), each product into its own column slice)
//      zip_step gives the provisional site U and the next concatenated environment C' = U^H theta;
//   3. one variational sweep right to left with the kept C's and right environments R_j (chi_j x r', stacked by rows):
//          site_i = [C_1 ... C_nb] * rowstack(A^j R_j)        ONE GEMM over the concatenated inner dimension
//      re-gauged by an SVD at canonicalize!'s cutoff 1e-12 (this sweep stands in for the gauge pass compress! opens with), then
//      R_j <- (A^j R_j) conj(site), again one GEMM on the stacked operand;
//   4. compress_impl on the right-canonical result.
// The per-term products C_j A^j (r x chi x 2 chi) and A^j R_j (chi x chi x r') go through the grouped small GEMM (one launch per
// step for ALL terms) while every term's bond is <= kSumGroupedMaxBond and the carried side r resp. r' of the step is
// <= kSumGroupedMaxSide: a product of at most 128 x 128 x 64.  The kernel is one 16 x 16 tile per wave without LDS reuse, made
// for steps whose cost is the dispatch; larger products go to qil_dev_gemm's tiling, one call per term.  Both bounds were
// chosen by that argument, not by a sweep (MEASUREMENTS section 10 records the launch counts and what was not measured).
constexpr int64_t kSumGroupedMaxBond = 64;
constexpr int64_t kSumGroupedMaxSide = 128;

int qil_sum_compress_impl(qil_context* ctx, const qil_mps* const* terms, int64_t nb, const double* w, int odt, int64_t maxdim,
                          double tol, int sweeps, int64_t zip_maxdim, qil_mps** out) {
    const int64_t N = terms[0]->n();
    if (maxdim <= 0) maxdim = kNoCap;
    if (zip_maxdim <= 0) zip_maxdim = zip_default_cap(maxdim);
    const double cutoff = tol * tol / ((double)(N - 1) * sweeps);
    const double zip_cutoff = cutoff * 1e-2;
    const size_t e = qil_elem_size(odt);
    const int nre = odt == QIL_C64 ? 2 : 1;          // doubles per element
    // the weights carry the amplitudes
    qil_result_guard<qil_mps> res_own(qil_mps_empty(ctx, N, odt, terms[0]->paired, terms[0]->site_ids.data(), 1.0));
    qil_mps* const res = res_own.p;
    {   // steps 1 to 3; the gauged copies and every temporary are gone before step 4
        std::vector<qil_result_guard<qil_mps>> own;      // the distinct right-canonical copies
        std::vector<const qil_mps*> seen;
        std::vector<const qil_mps*> phi((size_t)nb, nullptr);
        qil_scratch scratch(ctx);                            // every pool block this call owns outside a handle
        // `literal`: every concatenated bond of the operands fits under the cap.  Then the sweep of step 3 takes the exact route's
        // gauge step at every site (see there), which needs neither the zip-up nor gauged terms: the operands are read as they are,
        // and the decisions are those of compress! on the direct sum, bond for bond.
        bool literal = true;
        for (int64_t i = 1; i < N && literal; ++i) {
            int64_t sc = 0;
            for (int64_t j = 0; j < nb; ++j) sc += terms[j]->dims[(size_t)i];
            literal = sc <= zip_maxdim;
        }
        // ---- 1. gauge (a repeated handle is copied once)
        for (int64_t j = 0; j < nb; ++j) {
            if (literal && (odt == QIL_F64 || terms[j]->dtype == QIL_C64)) {
                phi[(size_t)j] = terms[j];
                continue;
            }
            for (size_t t = 0; t < seen.size(); ++t)
                if (seen[t] == terms[j]) phi[(size_t)j] = own[t].p;
            if (phi[(size_t)j]) continue;
            own.emplace_back(nullptr);
            QIL_TRY(qil_mps_clone_to(ctx, terms[j], &own.back().p));
            qil_mps* const c = own.back().p;
            seen.push_back(terms[j]);
            phi[(size_t)j] = c;
            if (!literal) QIL_TRY(canonicalize_impl(c, QIL_DIR_LEFT, 0, 0.0, kNoCap, true));
            if (odt == QIL_C64 && c->dtype == QIL_F64) {
                for (int64_t i = 0; i < N; ++i) {
                    void* p = nullptr;
                    QIL_TRY(widen_site(ctx, c->site[(size_t)i], c->site_elems(i), &p));
                    QIL_TRY(qil_chain_set_site(c, i, p, c->dims[(size_t)i], c->dims[(size_t)i + 1]));
                }
                c->dtype = QIL_C64;
            }
        }
        // offsets of the terms inside every concatenated bond (the edge bonds included: nb entries of 1)
        std::vector<std::vector<int64_t>> off((size_t)N + 1, std::vector<int64_t>((size_t)nb + 1, 0));
        int64_t maxbond = 1, om_ld = 1;
        for (int64_t i = 0; i <= N; ++i) {
            for (int64_t j = 0; j < nb; ++j) {
                off[(size_t)i][(size_t)j + 1] = off[(size_t)i][(size_t)j] + phi[(size_t)j]->dims[(size_t)i];
                maxbond = std::max(maxbond, phi[(size_t)j]->dims[(size_t)i]);
            }
            if (i >= 1 && i < N) om_ld = std::max(om_ld, off[(size_t)i][(size_t)nb]);
        }
        auto sig = [&](int64_t i) { return off[(size_t)i][(size_t)nb]; };
        // QIL_SUM_NO_GROUPED: the per-term GEMMs everywhere (A/B of the grouped kernel, tools/_sum_time.py)
        const bool grouped = maxbond <= kSumGroupedMaxBond && qil_dev_gemm_grouped_fits((size_t)(2 * nb)) && !getenv("QIL_SUM_NO_GROUPED");
        auto at = [&](const void* base, int64_t elems) { return (void*)((char*)base + (size_t)elems * e); };
        std::vector<qil_gemm_problem> probs;
        auto run_products = [&](int64_t side) -> int {   // one launch for all terms, or one GEMM per term
            if (grouped && side <= kSumGroupedMaxSide) return qil_dev_gemm_grouped(ctx, odt, probs);
            for (const qil_gemm_problem& p : probs)
                QIL_TRY(qil_dev_gemm(ctx, odt, 0, 0, p.m, p.n, p.k, p.A, p.lda, p.B, p.ldb, p.C, p.ldc));
            return QIL_OK;
        };
        void* Om = nullptr;
        QIL_TRY(zip_sketch(scratch, odt, om_ld, zip_maxdim, &Om));
        // ---- 2. zip-up, keeping the concatenated environments C_i (Rdim[i] x sig(i)); C_0 = the row of weights
        std::vector<void*> Ckeep((size_t)N, nullptr);
        std::vector<int64_t> Rdim((size_t)N + 1, 1);
        {
            std::vector<double> h((size_t)(nb * nre));
            for (int64_t j = 0; j < nb; ++j)
                for (int c = 0; c < nre; ++c) h[(size_t)(nre * j + c)] = w[2 * j + c];
            QIL_TRY(upload_small(scratch, h.data(), h.size(), &Ckeep[0]));
        }
        for (int64_t i = 0; i + 1 < N && !literal; ++i) {   // the last site is formed by the variational sweep
            const int64_t R = Rdim[(size_t)i], rows = 2 * R, Pc = sig(i + 1);
            void* theta = nullptr;
            QIL_TRY(scratch.alloc((size_t)(rows * Pc) * e, &theta));
            probs.clear();
            for (int64_t j = 0; j < nb; ++j) {           // theta[:, slice j] = C_j (R x chi_l) A^j (chi_l x 2 chi_r), layout [r, s, beta]
                const qil_mps* t = phi[(size_t)j];
                const int64_t cl = t->dims[(size_t)i], cr = t->dims[(size_t)i + 1];
                probs.push_back(qil_gemm_problem{at(Ckeep[(size_t)i], R * off[(size_t)i][(size_t)j]), t->site[(size_t)i],
                                                 at(theta, rows * off[(size_t)i + 1][(size_t)j]), (int)R, (int)(2 * cr), (int)cl,
                                                 (int)R, (int)cl, (int)R, 0, 0});
            }
            QIL_TRY(run_products(R));
            int64_t r = 0;
            void *U = nullptr, *SV = nullptr;
            QIL_TRY(zip_step(ctx, odt, rows, Pc, theta, zip_maxdim, zip_cutoff, Om, om_ld, &r, &U, &SV));
            scratch.free(theta);
            qil_chain_adopt(res, i, U);                  // [R, s, r]
            res->dims[(size_t)i] = R;
            res->dims[(size_t)i + 1] = r;
            Ckeep[(size_t)i + 1] = scratch.own(SV);          // [r, sig(i + 1)]: the C_j of the next site, concatenated
            Rdim[(size_t)i + 1] = r;
        }
        // ---- 3. variational sweep right to left; Rcat = row stack of the R_j (sig(i + 1) x rp)
        void* Rcat = nullptr;
        int64_t rp = 1;
        {
            std::vector<double> h((size_t)(nb * nre), 0.0);
            for (int64_t j = 0; j < nb; ++j) h[(size_t)(nre * j)] = 1.0;
            QIL_TRY(upload_small(scratch, h.data(), h.size(), &Rcat));
        }
        for (int64_t i = N - 1; i >= 0; --i) {
            const int64_t R = Rdim[(size_t)i], Sl = sig(i), Sr = sig(i + 1);
            void *AR = nullptr, *T = nullptr;
            QIL_TRY(scratch.alloc((size_t)(Sl * 2 * rp) * e, &AR));
            probs.clear();
            for (int64_t j = 0; j < nb; ++j) {           // AR[rows of j, (s, r')] = A^j[:, s, :] (chi_l x chi_r) R_j (chi_r x rp)
                const qil_mps* t = phi[(size_t)j];
                const int64_t cl = t->dims[(size_t)i], cr = t->dims[(size_t)i + 1];
                for (int s = 0; s < 2; ++s)
                    probs.push_back(qil_gemm_problem{at(t->site[(size_t)i], cl * s), at(Rcat, off[(size_t)i + 1][(size_t)j]),
                                                     at(AR, off[(size_t)i][(size_t)j] + Sl * s), (int)cl, (int)rp, (int)cr,
                                                     (int)(2 * cl), (int)Sr, (int)(2 * Sl), 0, 0});
            }
            QIL_TRY(run_products(rp));
            void* Rn = nullptr;                          // the stack of the new R_j
            int64_t K = 0;
            if (i > 0 && Sl <= zip_maxdim) {
                // The stacked operand is no larger than a capped site: take the gauge step of the exact route literally.  AR IS the
                // matrix canonicalize!(:left) factors at this bond of the direct sum (rows: the concatenated left bond, columns: an
                // orthonormal basis of everything to the right), so its SVD at that pass's cutoff 1e-12 makes the same decision:
                // site_i = V^H, and U S is the stack of the new R_j.  Uncapped calls and small sums run entirely through here.
                void* Vh = nullptr;
                QIL_TRY(svd_trunc_dev(ctx, odt, Sl, 2 * rp, AR, Sl, 1e-12, true, kNoCap, 1, 1, &K, &Rn, &Vh, nullptr));
                scratch.own(Rn);
                QIL_TRY(qil_chain_set_site(res, i, Vh, K, rp));
            } else {
                QIL_TRY(scratch.alloc((size_t)(2 * R * rp) * e, &T));
                QIL_TRY(qil_dev_gemm(ctx, odt, 0, 0, R, 2 * rp, Sl, Ckeep[(size_t)i], R, AR, Sl, T, R));
                QIL_TRY(qil_chain_set_site(res, i, scratch.give(T), R, rp));
                if (i == 0) break;
                // This sweep is the right-to-left gauge pass compress! opens with (mps.jl:923, canonicalize!(:left) at its fixed
                // cutoff 1e-12), so it carries that cutoff: site i is the orthogonality centre here, its singular values are the
                // bond's Schmidt values, and what the exact route's gauge pass drops from the direct sum is dropped here too.
                // compress_impl below is then told the state is right-canonical and skips the pass.
                QIL_TRY(gauge_site_left(res, i, 1e-12, kNoCap, false));
                K = res->dims[(size_t)i];
                QIL_TRY(scratch.alloc((size_t)(Sl * K) * e, &Rn));
                // R_j'[alpha, k] = sum_{s, r'} AR[alpha, (s, r')] conj(site_i[k, (s, r')]) for all terms at once
                QIL_TRY(qil_dev_gemm(ctx, odt, 0, 2, Sl, K, 2 * rp, AR, Sl, res->site[(size_t)i], K, Rn, Sl));
            }
            scratch.free(AR);
            scratch.free(Rcat);
            scratch.free(Ckeep[(size_t)i]);                  // (none on the literal route past site 0)
            Ckeep[(size_t)i] = nullptr;
            Rcat = Rn;
            rp = K;
        }
    }
    // ---- 4. exact-gauge truncation
    QIL_TRY(compress_impl(res, maxdim, tol, sweeps, true));    // the variational sweep left res right-canonical
    *out = res_own.release();
    return QIL_OK;
}

// zip_to_compress_mpo over a whole MPO (dt_transformer.jl:167-288; called on the MPO x MPO product in
// zt_transformer.jl:103-104): an exact gauge sweep towards one end, then a truncating sweep back.  In the gauged
// chain the reference's two-site core has the singular values of the single site next to the centre, so the
// truncating sweep is the same one-site sweep compress! uses.  direction 0 = "down" (gauge left -> right, truncate
// right -> left), 1 = "up" (mirror image).  The gauge sweep runs with cutoff 0: only exactly-zero singular
// values (rank-deficient bonds of a product) are dropped.
extern "C" int qil_mpo_compress(qil_mpo* W, int direction, double cutoff, int64_t maxdim) {
    QIL_REQUIRE(W, QIL_EINVAL_ARG, "mpo_compress: null argument");
    QIL_REQUIRE(direction == 0 || direction == 1, QIL_EINVAL_ARG,
                "zip_to_compress_mpo: unknown direction %d (0 = down, 1 = up)", direction);
    QIL_REQUIRE(cutoff >= 0, QIL_EINVAL_ARG, "mpo_compress: cutoff must be >= 0");
    if (W->n() < 2) return QIL_OK;
    QIL_TRY(qil_ctx_activate(W->ctx));
    qil_call_scope call_scope(W->ctx);
    if (maxdim <= 0) maxdim = kNoCap;
    const int gauge = direction == 0 ? QIL_DIR_RIGHT : QIL_DIR_LEFT;
    const int trunc = direction == 0 ? QIL_DIR_LEFT : QIL_DIR_RIGHT;
    // exact gauge pass by thin QRs, like the reference's (an SVD here would drop exactly-zero singular values and change
    // the bond dimensions the truncating pass starts from)
    QIL_TRY(canonicalize_impl(W, gauge, 0, 0.0, kNoCap, true));
    QIL_TRY(canonicalize_impl(W, trunc, 0, cutoff, maxdim));
    return QIL_OK;
}

extern "C" int qil_compress_batch(qil_mps* const* items, int64_t nb, int64_t maxdim, double tol, int sweeps) {
    QIL_REQUIRE(nb >= 0 && (items || nb == 0), QIL_EINVAL_ARG, "compress_batch: null item array");
    std::vector<qil_chain*> chains(items, items + nb);
    return qil_run_batch(chains.data(), nb, [&](qil_chain* c) {
        return compress_impl(static_cast<qil_mps*>(c), maxdim, tol, sweeps, false);
    });
}

extern "C" int qil_mpo_compress_batch(qil_mpo* const* items, int64_t nb, int direction, double cutoff, int64_t maxdim) {
    QIL_REQUIRE(nb >= 0 && (items || nb == 0), QIL_EINVAL_ARG, "mpo_compress_batch: null item array");
    std::vector<qil_chain*> chains(items, items + nb);
    return qil_run_batch(chains.data(), nb, [&](qil_chain* c) {
        return qil_mpo_compress(static_cast<qil_mpo*>(c), direction, cutoff, maxdim);
    });
}

extern "C" int qil_svd_trunc(qil_context* ctx, const void* A, int64_t m, int64_t n, int dtype, double cutoff,
                             int64_t maxdim, int64_t mindim, int64_t* rank, void* U, double* S, void* Vh) {
    QIL_REQUIRE(ctx && A && rank && U && S && Vh, QIL_EINVAL_ARG, "svd: null argument");
    QIL_REQUIRE(m >= 1 && n >= 1, QIL_EEMPTY, "svd: empty matrix");
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    const size_t e = qil_elem_size(dtype);
    void* dA = nullptr;
    QIL_TRY(tmp.alloc((size_t)(m * n) * e, &dA));
    QIL_HIP(hipMemcpyAsync(dA, A, (size_t)(m * n) * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));
    int64_t r = 0;
    void *dU = nullptr, *dVh = nullptr;
    std::vector<double> Sv;
    QIL_TRY(svd_trunc_dev(ctx, dtype, m, n, dA, m, cutoff, cutoff >= 0, maxdim, mindim, 0, &r, &dU, &dVh, &Sv));
    tmp.own(dU);
    tmp.own(dVh);
    QIL_HIP(hipMemcpyAsync(U, dU, (size_t)(m * r) * e, hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_TRY(qil_read_back(ctx, Vh, dVh, (size_t)(r * n) * e));
    for (int64_t i = 0; i < r; ++i) S[i] = Sv[(size_t)i];
    *rank = r;
    return QIL_OK;
}

// rsvd(A, Linds...; kwargs) on a host operand A (m x n, column-major): src/linalg/rsvd.jl:38-121.
extern "C" int qil_rsvd(qil_context* ctx, const void* A, int64_t m, int64_t n, int dtype, int64_t k, int64_t p,
                        int q, uint64_t seed, double cutoff, int64_t maxdim, int64_t mindim, int64_t* rank,
                        void* U, double* S, void* Vh) {
    QIL_REQUIRE(ctx && rank && U && S && Vh, QIL_EINVAL_ARG, "rsvd: null argument");
    QIL_REQUIRE(m >= 1 && n >= 1 && A, QIL_EEMPTY,
                "In `rsvd`, left or right index set is empty.");               // rsvd.jl:56-60
    QIL_REQUIRE(k >= 1 && p >= 0 && q >= 0, QIL_EINVAL_ARG, "rsvd: need k >= 1, p >= 0, q >= 0");
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    const size_t e = qil_elem_size(dtype);
    void *dA = nullptr, *Z = nullptr;
    QIL_TRY(tmp.alloc((size_t)(m * n) * e, &dA));
    QIL_TRY(tmp.alloc((size_t)(m * n) * e, &Z));
    QIL_HIP(hipMemcpyAsync(dA, A, (size_t)(m * n) * e, hipMemcpyHostToDevice, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));
    QIL_TRY(qil_dev_transpose(ctx, dtype, 0, m, n, dA, m, Z, n));               // Z = A^T ("A row-major")
    tmp.free(dA);
    if (maxdim <= 0) maxdim = k;                                                // maxdim = k default (rsvd.jl:47)
    int64_t r = 0;
    void *L = nullptr, *R = nullptr;
    std::vector<double> Sv;
    QIL_TRY(rsvd_rowmajor(ctx, dtype, m, n, Z, k, p, q, seed, cutoff, maxdim, mindim < 1 ? 1 : mindim, &r, &L, &R,
                          &Sv));
    tmp.own(L);
    tmp.own(R);
    tmp.free(Z);
    // L = U^T (r x m); R = (S V^h)^T (n x r).  Return U (m x r) and V^h (r x n) = (R diag(1/S))^T.
    std::vector<double> inv((size_t)r);
    for (int64_t i = 0; i < r; ++i) inv[(size_t)i] = Sv[(size_t)i] > 0 ? 1.0 / Sv[(size_t)i] : 0.0;
    QIL_TRY(qil_dev_scale(ctx, dtype, 1, n, r, R, n, inv.data()));
    void *dU = nullptr, *dVh = nullptr;
    QIL_TRY(tmp.alloc((size_t)(m * r) * e, &dU));
    QIL_TRY(tmp.alloc((size_t)(r * n) * e, &dVh));
    QIL_TRY(qil_dev_transpose(ctx, dtype, 0, r, m, L, r, dU, m));
    QIL_TRY(qil_dev_transpose(ctx, dtype, 0, n, r, R, n, dVh, r));
    QIL_HIP(hipMemcpyAsync(U, dU, (size_t)(m * r) * e, hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_TRY(qil_read_back(ctx, Vh, dVh, (size_t)(r * n) * e));
    for (int64_t i = 0; i < r; ++i) S[i] = Sv[(size_t)i];
    *rank = r;
    return QIL_OK;
}

extern "C" int qil_signal_mps(qil_context* ctx, const void* x, int64_t len, int dtype, int method, double cutoff,
                              int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed, int64_t mindim,
                              qil_mps** out) {
    EncodeParams P{method, cutoff, maxdim <= 0 ? kNoCap : maxdim, k, p, q, seed, mindim < 1 ? 1 : mindim};
    return signal_mps_impl(ctx, x, len, dtype, P, out);
}

static int ztmps_from_sites(qil_context* ctx, const qil_mps* sig, double cutoff, int64_t maxdim, qil_mps** out);

extern "C" int qil_signal_ztmps(qil_context* ctx, const void* x, int64_t len, int dtype, int method,
                                double cutoff, int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed,
                                int64_t mindim, qil_mps** out) {
    QIL_REQUIRE(ctx && out, QIL_EINVAL_ARG, "signal_ztmps: null argument");
    qil_call_scope call_scope(ctx);
    EncodeParams P{method, cutoff, maxdim <= 0 ? kNoCap : maxdim, k, p, q, seed, mindim < 1 ? 1 : mindim};
    qil_result_guard<qil_mps> sig_own(nullptr);       // gone on every return: only zt leaves the call
    QIL_TRY(signal_mps_impl(ctx, x, len, dtype, P, &sig_own.p));                  // SignalConverters.jl:251
    return ztmps_from_sites(ctx, sig_own.p, P.cutoff, P.maxdim, out);
}

extern "C" int qil_ztmps_from_mps(const qil_mps* psi, double cutoff, int64_t maxdim, qil_mps** out) {
    QIL_REQUIRE(psi && out, QIL_EINVAL_ARG, "ztmps_from_mps: null argument");
    QIL_REQUIRE(!psi->paired && psi->phys_rank == 1, QIL_EINVAL_ARG, "ztmps_from_mps: the operand is a paired state already");
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    return ztmps_from_sites(ctx, psi, cutoff, maxdim <= 0 ? kNoCap : maxdim, out);
}

// The per-site delta-fuse and split of SignalConverters.jl:261-276: site i of sig becomes core_main [b_{i-1}, s_main, c] and
// core_copy [c, s_copy, b_i] of a paired chain with sig's amplitude.  Context active, call scope open; sig is left intact.
static int ztmps_from_sites(qil_context* ctx, const qil_mps* sig, double cutoff, int64_t maxdim, qil_mps** out) {
    const int dtype = sig->dtype;
    const int64_t n = sig->n();
    const size_t e = qil_elem_size(dtype);
    qil_result_guard<qil_mps> zt_own(qil_mps_empty(ctx, 2 * n, dtype, 1, nullptr, sig->amplitude));
    qil_mps* const zt = zt_own.p;
    qil_scratch tmp(ctx);
    for (int64_t i = 0; i < n; ++i) {                                             // :261-276
        const int64_t cl = sig->dims[(size_t)i], cr = sig->dims[(size_t)i + 1];
        void* T = nullptr;
        QIL_TRY(tmp.alloc((size_t)(4 * cl * cr) * e, &T));
        if (dtype == QIL_C64)
            QIL_TRY((qil_klaunch<fuse_delta_k<c64>>(ctx, dim3(nblk(4 * cl * cr)), dim3(256), 0, (const c64*)sig->site[(size_t)i], (int)cl, (int)cr, (c64*)T)));
        else
            QIL_TRY((qil_klaunch<fuse_delta_k<double>>(ctx, dim3(nblk(4 * cl * cr)), dim3(256), 0, (const double*)sig->site[(size_t)i], (int)cl, (int)cr, (double*)T)));
        int64_t r = 0;
        void *U = nullptr, *SV = nullptr;
        QIL_TRY(svd_trunc_dev(ctx, dtype, 2 * cl, 2 * cr, T, 2 * cl, cutoff, true, maxdim, 1, 2, &r, &U, &SV, nullptr));
        tmp.free(T);
        qil_chain_adopt(zt, 2 * i, U);        // core_main [b_{i-1}, s_main, c]
        qil_chain_adopt(zt, 2 * i + 1, SV);   // core_copy [c, s_copy, b_i]
        zt->dims[(size_t)(2 * i)] = cl;
        zt->dims[(size_t)(2 * i + 1)] = r;
        zt->dims[(size_t)(2 * i + 2)] = cr;
    }
    *out = zt_own.release();
    return QIL_OK;
}

// nb signals of one length encoded concurrently (the serial loop over signal kinds of
// scripts/benchmark/zt_full_runtime.jl:151-221): outs[j] = signal_mps / signal_ztmps(xs[j]; ...), each encoder on one slot
// of the context's streams.  All or nothing on failure.
static int signal_batch(qil_context* ctx, const void* const* xs, int64_t nb, int64_t len, int dtype, int method, double cutoff,
                        int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed, int64_t mindim, int paired,
                        qil_mps** outs) {
    QIL_REQUIRE(ctx && nb >= 0 && ((xs && outs) || nb == 0), QIL_EINVAL_ARG, "signal batch: null argument");
    for (int64_t j = 0; j < nb; ++j) {
        outs[j] = nullptr;
        QIL_REQUIRE(xs[j], QIL_EINVAL_ARG, "signal batch: signal %lld is null", (long long)j);
    }
    const int st = qil_run_batch_on(ctx, nb, nullptr, [&](int64_t j, qil_context* work) {
        return paired ? qil_signal_ztmps(work, xs[j], len, dtype, method, cutoff, maxdim, k, p, q, seed, mindim, &outs[j])
                      : qil_signal_mps(work, xs[j], len, dtype, method, cutoff, maxdim, k, p, q, seed, mindim, &outs[j]);
    });
    if (st != QIL_OK)
        for (int64_t j = 0; j < nb; ++j) {
            if (outs[j]) qil_mps_destroy(outs[j]);
            outs[j] = nullptr;
        }
    return st;
}

extern "C" int qil_signal_mps_batch(qil_context* ctx, const void* const* xs, int64_t nb, int64_t len, int dtype, int method,
                                    double cutoff, int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed, int64_t mindim,
                                    qil_mps** outs) {
    return signal_batch(ctx, xs, nb, len, dtype, method, cutoff, maxdim, k, p, q, seed, mindim, 0, outs);
}

extern "C" int qil_signal_ztmps_batch(qil_context* ctx, const void* const* xs, int64_t nb, int64_t len, int dtype, int method,
                                      double cutoff, int64_t maxdim, int64_t k, int64_t p, int q, uint64_t seed,
                                      int64_t mindim, qil_mps** outs) {
    return signal_batch(ctx, xs, nb, len, dtype, method, cutoff, maxdim, k, p, q, seed, mindim, 1, outs);
}
