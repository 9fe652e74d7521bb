// Linear combinations of MPS for gfx950: qil_mps_sum (the direct sum of the chains), qil_mps_sum_compress (the fused
// sum-and-truncate, driver in qil_truncate.hip) and the grouped small GEMM the fused route runs its per-term products through;
// and qil_mpo_sum, the direct sum of operator chains through the same kernel (launch_sum: an MPO site is an MPS-shaped site).
//
// out = sum_j c_j terms[j] has the block tensors
//     first     [ w_1 A^1 | w_2 A^2 | ... ]              1 x 2 x sum(chi)         w_j = c_j amplitude_j
//     interior  diag(A^1, A^2, ...)                      sum(chi_l) x 2 x sum(chi_r)
//     last      column stack of the A^j                  sum(chi) x 2 x 1
// Copies and zeros, one multiply on the first tensor: HBM-STORE bound like the apply and the element-wise product, so
// site_sum_grouped is organised around the store stream exactly as site_hadamard_grouped is -- one lane per output ROW (two for
// real results, packed into one 16-B store), so every wave-level store is 1 KiB contiguous; a workgroup owns a row tile and a
// range of columns; ALL sites in ONE grouped launch; every output element is stored exactly once, the zeros included (no
// memset + block copies, which would store the tensor twice).  For each column the workgroup finds the term whose column range
// contains it (the <= kNC terms its columns can touch are staged in LDS, the walk over them is wave-uniform); a lane stores the
// operand's entry when its row lies in that term's row range and +0.0 otherwise.  The operand is read once, coalesced along
// rows; the zeros cost no loads.
#include <algorithm>
#include <cmath>
#include <vector>

#include "qil_internal.h"
#include "qil_device_utils.h"

namespace {

using namespace qil_dev;

struct SumTerm {
    const void* A;         // operand site [rows, 2, cols]
    int row_off, rows;     // its row range in the result
    int col_off, cols;     // its column range in the result
    double wre, wim;       // weight (read on the first site only)
    int cplx;              // operand dtype is c64 (read by the mixed-dtype instantiation only)
    int pad;
};

enum { kByColumn = 0, kByRow = 1, kAccumulate = 2 };

struct SumSite {
    void* C;               // result [R, 2, ncols]
    long long R;           // rows
    int ncols;             // right bond of the result
    int nterms;
    long long term_begin;  // first entry of this site in the term table
    int row_tiles;         // ceil(R / tile rows)
    int kind;              // kByColumn: first and interior sites; kByRow: the last site; kAccumulate: the only site of n = 1
    int scale;             // multiply by the weight (first site)
    int nphys;             // physical slices of a kByRow / kAccumulate site: 2 (MPS), 4 (MPO); kByColumn sites are MPS-shaped
    long long block_begin; // first workgroup of this site in the grouped grid
};

constexpr int kRows = 256;  // lanes per workgroup
constexpr int kNC = 16;     // result columns (of the right bond) per workgroup = terms staged in LDS

// one rounding per component: the imaginary part of a widened real operand is +0.0, and fma(-wim, +0.0, x) == x
__device__ __forceinline__ double wmul(double v, double wre, double) { return wre * v; }
__device__ __forceinline__ c64 wmul(c64 v, double wre, double wim) {
    return c64{fma(-wim, v.im, wre * v.re), fma(wim, v.re, wre * v.im)};
}

// MIXED: the terms' dtypes differ; T.cplx is the same for every lane of the workgroup (the term is chosen per column)
template <class TA, class TO, bool MIXED>
__device__ __forceinline__ TO load_term(const SumTerm& T, long long idx) {
    if constexpr (MIXED) {
        if (T.cplx) return static_cast<const c64*>(T.A)[idx];
        return c64{static_cast<const double*>(T.A)[idx], 0.0};
    } else {
        return cast_elem<TO>(static_cast<const TA*>(T.A)[idx]);
    }
}

template <class TA, class TO, bool MIXED>
__global__ __launch_bounds__(kRows) void site_sum_grouped(const SumSite* __restrict__ sites, const SumTerm* __restrict__ terms,
                                                          int nsites) {
    constexpr int RPL = rows_per_lane<TO>::value;
    constexpr int kTileRows = kRows * RPL;
    __shared__ SumTerm st[kNC];
    const long long blk = blockIdx.x;
    const SumSite S = sites[last_entry_le<&SumSite::block_begin>(sites, nsites, blk)];   // block -> site
    const SumTerm* __restrict__ T = terms + S.term_begin;
    TO* __restrict__ C = static_cast<TO*>(S.C);
    const long long R = S.R;
    if (S.kind == kAccumulate) {                       // n = 1: the nphys numbers sum_j w_j A^j[s]
        if ((int)threadIdx.x < S.nphys) {
            TO acc{};
            for (int j = 0; j < S.nterms; ++j)
                acc = add_t(acc, wmul(load_term<TA, TO, MIXED>(T[j], threadIdx.x), T[j].wre, T[j].wim));
            store_out<false>(C + threadIdx.x, acc);
        }
        return;
    }
    // row tile fastest: concurrently resident workgroups cover whole output columns
    const long long local = blk - S.block_begin;
    const int row_tile = (int)(local % S.row_tiles);
    const int chunk = (int)(local / S.row_tiles);
    const long long t_lo = (long long)row_tile * kTileRows;
    const long long r_first = t_lo + (long long)threadIdx.x * RPL;
    if (S.kind == kByRow) {                            // last site: every term covers the one column, the rows are split
        const long long t_hi = min(t_lo + kTileRows, R);
        int a = 0, b = S.nterms - 1;
        while (a < b) {
            int mid = (a + b + 1) >> 1;
            if (T[mid].row_off <= t_lo) a = mid; else b = mid - 1;
        }
        for (int j = a; j < S.nterms && T[j].row_off < t_hi; ++j) {      // wave-uniform walk over the tile's terms
            const SumTerm Tj = T[j];
#pragma unroll
            for (int k = 0; k < RPL; ++k) {
                const long long r = r_first + k;
                if (r < R && r >= Tj.row_off && r < (long long)Tj.row_off + Tj.rows) {
                    const long long off = r - Tj.row_off;
                    for (int s = 0; s < S.nphys; ++s)
                        store_out<true>(C + r + R * s, load_term<TA, TO, MIXED>(Tj, off + (long long)Tj.rows * s));
                }
            }
        }
        return;
    }
    // ---- first and interior sites: the term is a function of the column
    const int c0 = chunk * kNC, c1 = min(c0 + kNC, S.ncols);
    int j0 = 0, j1 = S.nterms - 1;
    while (j0 < j1) {
        int mid = (j0 + j1 + 1) >> 1;
        if (T[mid].col_off <= c0) j0 = mid; else j1 = mid - 1;
    }
    // every term has at least one column: columns c0 .. c1-1 touch at most kNC terms, j0 .. j0 + kNC - 1
    if ((int)threadIdx.x < kNC && j0 + (int)threadIdx.x < S.nterms) st[threadIdx.x] = T[j0 + threadIdx.x];
    __syncthreads();
    if (r_first >= R) return;
    const bool second = RPL == 2 && r_first + 1 < R;              // this lane's second row exists
    const bool packed = RPL == 2 && second && (R & 1) == 0;       // 16-B aligned pair for every column
    int jl = 0;
    for (int c = c0; c < c1; ++c) {
        if (c >= st[jl].col_off + st[jl].cols) ++jl;               // wave-uniform: the next column is in this term or the next
        const SumTerm& Tj = st[jl];
        const long long rel = r_first - Tj.row_off;
        bool in[RPL];
#pragma unroll
        for (int k = 0; k < RPL; ++k) in[k] = rel + k >= 0 && rel + k < Tj.rows && r_first + k < R;
        const long long abase = rel + (long long)Tj.rows * (2LL * (c - Tj.col_off));
        TO* cp = C + r_first + R * (2LL * c);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            TO v[RPL];
#pragma unroll
            for (int k = 0; k < RPL; ++k) {
                v[k] = TO{};
                if (in[k]) {
                    v[k] = load_term<TA, TO, MIXED>(Tj, abase + k + (long long)Tj.rows * s);
                    if (S.scale) v[k] = wmul(v[k], Tj.wre, Tj.wim);
                }
            }
            if constexpr (RPL == 2) {
                if (packed) {
                    store_pair(cp + R * s, v[0], v[1]);
                } else {
                    store_out<true>(cp + R * s, v[0]);
                    if (second) store_out<true>(cp + R * s + 1, v[1]);
                }
            } else {
                store_out<true>(cp + R * s, v[0]);
            }
        }
    }
}

// ---- grouped small GEMM: a table of independent products, one 16 x 16 output tile per wave, one launch
// the tile step and its lane layout: mfma_step (qil_device_utils.h)
template <class T>
__global__ __launch_bounds__(64) void gemm_grouped_small(const qil_gemm_problem* __restrict__ probs, int count) {
    const int blk = (int)blockIdx.x;
    const qil_gemm_problem P = probs[last_entry_le<&qil_gemm_problem::tile_begin>(probs, count, blk)];   // tile -> problem
    const int t = blk - P.tile_begin, tm = (P.m + 15) >> 4;
    const int ti = t % tm, tj = t / tm;
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const int row = 16 * ti + li, col = 16 * tj + li;
    const T* __restrict__ A = static_cast<const T*>(P.A);
    const T* __restrict__ B = static_cast<const T*>(P.B);
    d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0};
    for (int k0 = 0; k0 < P.k; k0 += 4) {
        const int k = k0 + lk;
        T a{}, b{};
        if (row < P.m && k < P.k) a = A[row + (long long)P.lda * k];
        if (col < P.n && k < P.k) b = B[k + (long long)P.ldb * col];
        mfma_step(a, b, rr, ii);
    }
    T* __restrict__ Cm = static_cast<T*>(P.C);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int orow = 16 * ti + lk + 4 * r;
        if (orow < P.m && col < P.n) Cm[orow + (long long)P.ldc * col] = make_elem(rr[r], ii[r], (T*)nullptr);
    }
}

// the operand checks of every entry, all of them before the context is activated: arguments, coefficients, then every term
// against terms[0] in the order of check_pair (context, paired, length, sites).  H = qil_mps or qil_mpo.
template <class H>
int check_terms(const char* verb, const H* const* terms, int64_t nb, const double* coeffs, H* const* out) {
    QIL_REQUIRE(terms && out, QIL_EINVAL_ARG, "%s: null argument", verb);
    QIL_REQUIRE(nb >= 1, QIL_EINVAL_ARG, "%s: needs at least one term, got nb = %lld", verb, (long long)nb);
    for (int64_t j = 0; j < nb; ++j) QIL_REQUIRE(terms[j], QIL_EINVAL_ARG, "%s: null argument", verb);
    if (coeffs)
        for (int64_t j = 0; j < 2 * nb; ++j)
            QIL_REQUIRE(std::isfinite(coeffs[j]), QIL_EINVAL_ARG, "%s: coefficient %lld is not finite", verb, (long long)(j / 2));
    for (int64_t j = 1; j < nb; ++j) QIL_TRY(qil_check_pair(verb, terms[0], terms[j]));
    return QIL_OK;
}

// w_j = c_j amplitude_j as (re, im) pairs, and the result dtype: promote(terms), c64 when a coefficient has an imaginary part
// (MPOs carry no amplitude: w_j = c_j)
inline double amplitude_of(const qil_mps* t) { return t->amplitude; }
inline double amplitude_of(const qil_mpo*) { return 1.0; }
template <class H>
int weights_of(const H* const* terms, int64_t nb, const double* coeffs, std::vector<double>& w) {
    int odt = QIL_F64;
    w.resize((size_t)(2 * nb));
    for (int64_t j = 0; j < nb; ++j) {
        const double cre = coeffs ? coeffs[2 * j] : 1.0, cim = coeffs ? coeffs[2 * j + 1] : 0.0;
        w[(size_t)(2 * j)] = cre * amplitude_of(terms[j]);
        w[(size_t)(2 * j + 1)] = cim * amplitude_of(terms[j]);
        if (terms[j]->dtype == QIL_C64 || cim != 0.0) odt = QIL_C64;
    }
    return odt;
}

// H = qil_mps or qil_mpo.  An MPO site [Dl, 2, 2, Dr] is the MPS-shaped site [Dl, 2, 2 Dr] with column s_out + 2 b, so the first
// and interior sites of an operator sum are kByColumn sites with the column counts and offsets doubled; the last site and the only
// site of n = 1 have four physical slices instead of two.
template <class H>
int launch_sum(const char* verb, const H* const* terms, int64_t nb, const std::vector<double>& w, H* out) {
    qil_context* ctx = out->ctx;
    const int64_t n = out->n();
    const int cmul = out->phys_rank == 2 ? 2 : 1;
    const int tile_rows = out->dtype == QIL_F64 ? 2 * kRows : kRows;
    std::vector<SumSite> stab((size_t)n);
    std::vector<SumTerm> ttab((size_t)(n * nb));
    long long blocks = 0;
    for (int64_t i = 0; i < n; ++i) {
        SumSite& s = stab[(size_t)i];
        s.C = out->site[(size_t)i];
        s.R = out->dims[(size_t)i];
        s.ncols = cmul * (int)out->dims[(size_t)i + 1];
        s.nterms = (int)nb;
        s.term_begin = i * nb;
        s.kind = n == 1 ? kAccumulate : i + 1 == n ? kByRow : kByColumn;
        s.scale = i == 0;
        s.nphys = 2 * cmul;
        s.row_tiles = (int)((s.R + tile_rows - 1) / tile_rows);
        s.block_begin = blocks;
        blocks += s.kind == kAccumulate ? 1 : s.kind == kByRow ? s.row_tiles : (long long)s.row_tiles * ((s.ncols + kNC - 1) / kNC);
        int64_t ro = 0, co = 0;
        for (int64_t j = 0; j < nb; ++j) {
            SumTerm& t = ttab[(size_t)(i * nb + j)];
            t.A = terms[j]->site[(size_t)i];
            t.rows = (int)terms[j]->dims[(size_t)i];
            t.cols = cmul * (int)terms[j]->dims[(size_t)i + 1];
            t.row_off = i == 0 ? 0 : (int)ro;                 // the edge bonds are shared: every term starts at 0 there
            t.col_off = i + 1 == n ? 0 : (int)co;
            t.wre = w[(size_t)(2 * j)];
            t.wim = w[(size_t)(2 * j + 1)];
            t.cplx = terms[j]->dtype == QIL_C64;
            t.pad = 0;
            ro += t.rows;
            co += t.cols;
        }
    }
    QIL_REQUIRE(blocks < (1LL << 31), QIL_EINVAL_ARG, "%s: grid too large (%lld workgroups)", verb, blocks);
    // both tables in one upload, the terms behind the sites (64 terms x 48 sites is past a descriptor slot)
    const size_t sbytes = stab.size() * sizeof(SumSite);
    qil_dev_table dev(ctx);
    QIL_TRY(dev.upload(stab.data(), sbytes, ttab.data(), ttab.size() * sizeof(SumTerm)));
    QIL_TRY(qil_ctx_prof_begin(ctx));
    const SumSite* dsites = dev.as<SumSite>();
    const SumTerm* dterms = dev.as<SumTerm>(sbytes);
    const dim3 grid((unsigned)blocks), block(kRows);
    bool any_c = false, any_r = false;
    for (int64_t j = 0; j < nb; ++j) (terms[j]->dtype == QIL_C64 ? any_c : any_r) = true;
#define QIL_SUM_LAUNCH(TA, TO, MIXED) \
    hipLaunchKernelGGL((site_sum_grouped<TA, TO, MIXED>), grid, block, 0, qil_stream(ctx), dsites, dterms, (int)n)
    if (out->dtype == QIL_F64) QIL_SUM_LAUNCH(double, double, false);
    else if (any_c && any_r) QIL_SUM_LAUNCH(double, c64, true);
    else if (any_c) QIL_SUM_LAUNCH(c64, c64, false);
    else QIL_SUM_LAUNCH(double, c64, false);
#undef QIL_SUM_LAUNCH
    QIL_HIP(hipGetLastError());
    QIL_TRY(qil_ctx_prof_end(ctx));
    return dev.release();
}

}  // namespace

int qil_dev_gemm_grouped(qil_context* ctx, int dtype, std::vector<qil_gemm_problem>& probs) {
    if (probs.empty()) return QIL_OK;
    long long tiles = 0;
    for (qil_gemm_problem& p : probs) {
        p.tile_begin = (int)tiles;
        tiles += (long long)((p.m + 15) / 16) * ((p.n + 15) / 16);
    }
    QIL_REQUIRE(tiles < (1LL << 31), QIL_EINVAL_ARG, "gemm_grouped: table too large (%zu problems)", probs.size());
    qil_dev_table dev(ctx);
    QIL_TRY(dev.upload(probs.data(), probs.size() * sizeof(qil_gemm_problem)));
    const qil_gemm_problem* dtab = dev.as<qil_gemm_problem>();
    if (dtype == QIL_C64)
        hipLaunchKernelGGL((gemm_grouped_small<c64>), dim3((unsigned)tiles), dim3(64), 0, qil_stream(ctx), dtab, (int)probs.size());
    else
        hipLaunchKernelGGL((gemm_grouped_small<double>), dim3((unsigned)tiles), dim3(64), 0, qil_stream(ctx), dtab, (int)probs.size());
    QIL_HIP(hipGetLastError());
    return dev.release();
}

bool qil_dev_gemm_grouped_fits(size_t nproblems) { return nproblems * sizeof(qil_gemm_problem) <= qil_context::kDescSlotBytes; }

extern "C" int qil_mps_sum(const qil_mps* const* terms, int64_t nb, const double* coeffs, qil_mps** out) {
    QIL_TRY(check_terms("mps_sum", terms, nb, coeffs, out));
    qil_context* ctx = terms[0]->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int64_t n = terms[0]->n();
    std::vector<double> w;
    const int odt = weights_of(terms, nb, coeffs, w);
    std::vector<int64_t> bonds((size_t)(n > 1 ? n - 1 : 0), 0);
    for (int64_t i = 0; i + 1 < n; ++i)
        for (int64_t j = 0; j < nb; ++j) bonds[(size_t)i] += terms[j]->dims[(size_t)i + 1];
    qil_mps* res = nullptr;
    QIL_TRY(qil_mps_alloc(ctx, n, odt, terms[0]->paired, bonds.data(), terms[0]->site_ids.data(), 1.0, &res));
    qil_result_guard<qil_mps> guard(res);
    QIL_TRY(launch_sum("mps_sum", terms, nb, w, res));
    *out = guard.release();
    return QIL_OK;
}

extern "C" int qil_mps_sum_compress(const qil_mps* const* terms, int64_t nb, const double* coeffs, int64_t maxdim, double tol,
                                    int sweeps, int64_t zip_maxdim, qil_mps** out) {
    QIL_TRY(check_terms("mps_sum_compress", terms, nb, coeffs, out));
    QIL_REQUIRE(terms[0]->n() >= 2, QIL_EDOMAIN, "SignalMPS must have at least 2 sites.");
    QIL_REQUIRE(sweeps >= 1, QIL_EINVAL_ARG, "compress!: sweeps must be >= 1");
    qil_context* ctx = terms[0]->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    std::vector<double> w;
    const int odt = weights_of(terms, nb, coeffs, w);
    return qil_sum_compress_impl(ctx, terms, nb, w.data(), odt, maxdim, tol, sweeps, zip_maxdim, out);
}

extern "C" int qil_mpo_sum(const qil_mpo* const* terms, int64_t nb, const double* coeffs, qil_mpo** out) {
    QIL_TRY(check_terms("mpo_sum", terms, nb, coeffs, out));
    qil_context* ctx = terms[0]->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int64_t n = terms[0]->n();
    std::vector<double> w;
    const int odt = weights_of(terms, nb, coeffs, w);
    std::vector<int64_t> bonds((size_t)(n > 1 ? n - 1 : 0), 0);
    for (int64_t i = 0; i + 1 < n; ++i)
        for (int64_t j = 0; j < nb; ++j) bonds[(size_t)i] += terms[j]->dims[(size_t)i + 1];
    qil_mpo* res = nullptr;
    QIL_TRY(qil_mpo_alloc(ctx, n, odt, terms[0]->paired, bonds.data(), terms[0]->site_ids.data(), &res));
    qil_result_guard<qil_mpo> guard(res);
    QIL_TRY(launch_sum("mpo_sum", terms, nb, w, res));
    *out = guard.release();
    return QIL_OK;
}
