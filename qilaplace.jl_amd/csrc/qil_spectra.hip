// Schmidt spectra of every bond of a chain: qil_bond_spectra (MPS) and qil_mpo_bond_spectra (operator-Schmidt values of an MPO).
//
//   1. clone the chain into pool memory and divide every site by its Frobenius norm (one launch, the logarithms kept on the
//      device): the gauge sweep below squares its entries, and a chain whose norm^2 leaves the double range would overflow there;
//   2. exact right-orthonormal gauge of the clone (qil_gauge_exact: thin QR, the SVD at cut-off 0 where a site has none);
//   3. left-to-right sweep: site i (with the carry multiplied in) = Q C_i, Q an isometry that is dropped, C_i (min(pd cl, cr) x cr)
//      kept in a per-bond buffer, divided by its Frobenius norm (logarithm kept) and multiplied into site i + 1.  Everything to the
//      right of the carry is a right isometry, so the singular values of the normalised C_i are the Schmidt values of bond i + 1;
//   4. bond_svals_batched: ONE launch, one workgroup per bond, values-only one-sided Jacobi of C_i in LDS; bonds above the LDS cap
//      (kCapF64 / kCapC64) or whose iteration hit the sweep cap go through qil_dev_svd with the factors discarded;
//   5. one read-back of the packed values, the logarithms (their sum is log |psi|) and the per-bond flags.
// A call synchronises more often than that: the zero-site flag of step 1 is read back before the gauge sweep runs on the
// clone, and every qil_dev_qr_positive(orthonormal = true) of steps 2 and 3 reads its orthonormality measure back.
//
// QIL_SPECTRA_ROUTE=svd (read on every call) sends every bond through qil_dev_svd: the yardstick and the escape hatch.
#include "qil_internal.h"
#include "qil_launch.h"
#include "qil_device_utils.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace {

using namespace qil_dev;

// The dynamic LDS the fused Jacobi kernels of qil_linalg.hip request at most (svd_impl: lds_a, lds_av <= 150 KiB).  A factor
// with sides (long, short) is staged as `short` columns of (long | 1) elements; the cap K of a dtype is the largest side for
// which the square factor fits:  (K | 1) K sizeof(T) <= 150 KiB  ->  139 * 138 * 8 = 153456 (f64), 97 * 97 * 16 = 150544 (c64).
constexpr size_t kJacobiLdsBytes = 150 * 1024;
constexpr int kCapF64 = 138, kCapC64 = 97;
constexpr bool fits_lds(int side, size_t elem) { return (size_t)(side | 1) * (size_t)side * elem <= kJacobiLdsBytes; }
static_assert(fits_lds(kCapF64, 8) && !fits_lds(kCapF64 + 1, 8), "f64 cap is the largest side that fits");
static_assert(fits_lds(kCapC64, 16) && !fits_lds(kCapC64 + 1, 16), "c64 cap is the largest side that fits");
constexpr int kMaxCols = 144;          // the column norms of one bond
static_assert(kMaxCols >= kCapF64 && kMaxCols >= kCapC64, "s_nrm holds the norms of a factor at either cap");
constexpr int kNormThreads = 256;      // workgroup of the normalisation kernels: their stride, their partials, their NT
static_assert(kNormThreads % 64 == 0, "whole waves");
constexpr int kSweepCap = 40;          // the fused Jacobi kernels' limit

// ---- Frobenius normalisation -------------------------------------------------------------------------------------------
// p[0 .. count) /= |p|_F, *log_out = log |p|_F.  The norm is max |x| * sqrt(sum |x / max|^2), so that neither a norm near the
// ends of the double range nor its square costs anything.  A norm that is 0 or not finite raises *flag and leaves p alone.
template <class T>
__device__ __forceinline__ void frob_normalise(T* __restrict__ p, long long count, double* __restrict__ log_out,
                                                 int* __restrict__ flag) {
    constexpr int NWV = kNormThreads / 64;
    __shared__ double red[NWV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mx = 0.0;
    bool bad = false;
    for (long long t = threadIdx.x; t < count; t += kNormThreads) {
        const T v = p[t];
        const double a = fmax(fabs(re_of(v)), fabs(im_of(v)));
        bad |= !(a <= 1.79769313486231570e308);          // inf or NaN
        mx = fmax(mx, a);
    }
    if (bad) mx = INFINITY;
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < NWV; ++w) mx = fmax(mx, red[w]);
    __syncthreads();
    if (!(mx > 0.0) || !(mx <= 1.79769313486231570e308)) {
        if (threadIdx.x == 0) {
            *flag = 1;
            *log_out = 0.0;
        }
        return;
    }
    double s = 0.0;
    for (long long t = threadIdx.x; t < count; t += kNormThreads) {
        const T v = p[t];
        const double xr = re_of(v) / mx, xi = im_of(v) / mx;
        s = fma(xr, xr, s);
        s = fma(xi, xi, s);
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = red[0];
    for (int w = 1; w < NWV; ++w) s += red[w];            // >= 1: the largest entry contributes 1
    const double rs = sqrt(s);
    for (long long t = threadIdx.x; t < count; t += kNormThreads) {
        const T v = p[t];
        p[t] = make_elem((re_of(v) / mx) / rs, (im_of(v) / mx) / rs, static_cast<T*>(nullptr));
    }
    if (threadIdx.x == 0) *log_out = log(mx) + 0.5 * log(s);
}

template <class T>
__device__ __forceinline__ void frob_normalise_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ p, long long count,
                                                      double* __restrict__ log_out, int* __restrict__ flag) {
    frob_normalise<T>(p, count, log_out, flag);
}
template <class T>
struct frob_normalise_k {
    static constexpr int NT = kNormThreads, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        frob_normalise_body<T>(b, g, a...);
    }
};

// the same for every site of a chain in one launch: workgroup i normalises site i, its logarithm goes to logs[i]
struct NormSite {
    void* p;
    long long count;
};
template <class T>
__device__ __forceinline__ void frob_normalise_sites_body(const uint3 blockIdx, const uint3 gridDim, const NormSite* __restrict__ tab,
                                                            double* __restrict__ logs, int* __restrict__ flag) {
    const NormSite S = tab[blockIdx.x];
    frob_normalise<T>(static_cast<T*>(S.p), S.count, logs + blockIdx.x, flag);
}
template <class T>
struct frob_normalise_sites_k {
    static constexpr int NT = kNormThreads, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        frob_normalise_sites_body<T>(b, g, a...);
    }
};

// ---- singular values of many small factors -----------------------------------------------------------------------------
struct BondFactor {
    const void* C;     // rows x cols, column-major
    int rows, cols, ld;
    int out_off;       // first slot of this bond in the packed values
    int flag;          // its slot in the flags
    int pad;
};

// One sweep loop of the values-only one-sided (Hestenes) Jacobi iteration on the n columns (length m, leading dimension la) of
// A in LDS: round-robin over the column pairs (an odd n plays against a bye), a group of G lanes per pair, the pairs of a round
// disjoint.  A pair is left alone when |g_pq| <= tol sqrt(g_pp g_qq) or when one of its columns is exactly zero, so nothing
// divides 0 by 0.  Returns (to every thread) whether the last sweep still rotated: the sweep cap was reached.
// A sibling of jacobi_sweeps / jacobi_sweeps_nov (qil_device_utils.h), which stay as they are: the same tournament, reductions
// and barriers.  Three differences: complex columns without a V (jacobi_sweeps_nov is real only), the stop on a sweep that
// rotated NOTHING instead of the quadratic-phase rule and the negligible-column threshold, and the returned flag.  A change to
// the pairing or the barriers there belongs here as well.
template <class T, int G>
__device__ __forceinline__ bool svals_sweeps(T* A, int la, int m, int n, double tol, int max_sweeps, int* s_rot) {
    constexpr int NT = 1024, NW = NT / G;
    const int tid = threadIdx.x, lane = tid & (G - 1), grp = tid / G;
    const int npad = n + (n & 1);
    int any = 0;
    for (int sweep = 0; sweep < max_sweeps && n > 1; ++sweep) {
        if (tid == 0) *s_rot = 0;
        __syncthreads();
        for (int round = 0; round < npad - 1; ++round) {
            for (int i = grp; i < npad / 2; i += NW) {
                int p, q;
                if (i == 0) {
                    p = npad - 1;
                    q = round;
                } else {
                    p = round + i;
                    q = round + npad - 1 - i;
                    if (p >= npad - 1) p -= npad - 1;
                    if (q >= npad - 1) q -= npad - 1;
                }
                if (p >= n || q >= n) continue;               // the bye of an odd column count
                T* ap = A + la * p;
                T* aq = A + la * q;
                double al = 0, be = 0, gr = 0, gi = 0;
                for (int r = lane; r < m; r += G) {
                    const T x = ap[r], y = aq[r];
                    al += abs2_t(x);
                    be += abs2_t(y);
                    dot_parts(x, y, gr, gi);
                }
                al = group_sum<G>(al);
                be = group_sum<G>(be);
                gr = group_sum<G>(gr);
                if (sizeof(T) == 16) gi = group_sum<G>(gi);
                if (al == 0.0 || be == 0.0) continue;
                double c, sn, pr, pi;
                bool big;
                if (!jacobi_rotation<sizeof(T) == 16>(al, be, gr, gi, tol, c, sn, pr, pi, big)) continue;
                if (lane == 0) atomicOr(s_rot, 1);            // LDS
                for (int r = lane; r < m; r += G) {
                    T x = ap[r], y = aq[r];
                    rotate_pair(x, y, c, sn, pr, pi);
                    ap[r] = x;
                    aq[r] = y;
                }
            }
            __threadfence_block();
            __syncthreads();
        }
        any = *s_rot;
        __syncthreads();
        if (!any) break;                                      // a whole sweep rotated nothing
    }
    return any != 0;
}

// Workgroup b: the singular values of factor b, descending, into S[out_off .. out_off + rows).  Every factor is a carry, k x c
// with k <= c (the host refuses anything else), so it is staged TRANSPOSED: its short side becomes the n = rows columns of
// length m = cols (a triangular factor's rows are also closer to orthogonal than its columns), with an odd leading dimension;
// it is rotated until a whole sweep rotates nothing, and the column norms are ranked inside the workgroup.  flags[flag] = 1 when the sweep cap was reached.  Reads the factor, writes S and flags only.
template <class T>
__device__ __forceinline__ void bond_svals_batched_body(const uint3 blockIdx, const uint3 gridDim, const BondFactor* __restrict__ tab,
                                                          double* __restrict__ S, int* __restrict__ flags, int max_sweeps) {
    extern __shared__ __attribute__((aligned(16))) char sv_smem[];
    __shared__ int s_rot;
    __shared__ double s_nrm[kMaxCols];
    const BondFactor B = tab[blockIdx.x];
    const T* __restrict__ C = static_cast<const T*>(B.C);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = B.cols, n = B.rows;
    const int la = m | 1;
    T* A = reinterpret_cast<T*>(sv_smem);
    for (int t = tid; t < B.rows * B.cols; t += 1024) {
        const int r = t % B.rows, c = t / B.rows;
        const T v = C[r + (long long)B.ld * c];
        A[c + la * r] = v;
    }
    __threadfence_block();
    __syncthreads();
    // |a_p . a_q| / (|a_p| |a_q|) <= 1e-15, but never below the rounding noise of the dot products themselves
    const double tol = fmax(1e-15, 4.0 * 1.1e-16 * sqrt((double)m));
    const bool capped = m <= 128 ? svals_sweeps<T, 16>(A, la, m, n, tol, max_sweeps, &s_rot)
                                 : svals_sweeps<T, 64>(A, la, m, n, tol, max_sweeps, &s_rot);
    for (int j = wave; j < n; j += 16) {
        const T* a = A + la * j;
        double v = 0;
        for (int r = lane; r < m; r += 64) v += abs2_t(a[r]);
        v = wave_sum(v);
        if (lane == 0) s_nrm[j] = sqrt(v);
    }
    __syncthreads();
    if (tid < n) {
        const double v = s_nrm[tid];
        int rank = 0;
        for (int k = 0; k < n; ++k) {
            const double w = s_nrm[k];
            rank += (w > v || (w == v && k < tid)) ? 1 : 0;
        }
        S[B.out_off + rank] = v;
    }
    if (tid == 0 && capped) flags[B.flag] = 1;
}
template <class T>
struct bond_svals_batched_k {
    static constexpr int NT = 1024, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        bond_svals_batched_body<T>(b, g, a...);
    }
};

// ---- host side ---------------------------------------------------------------------------------------------------------
// releases the working clone's sites on every return path (they belong to the chain, not to the call scope)
struct clone_guard {
    qil_chain* c;
    ~clone_guard() { qil_chain_release(c); }
};

static int normalise_one(qil_context* ctx, int dt, void* p, long long count, double* log_out, int* flag) {
    if (dt == QIL_C64) return qil_klaunch<frob_normalise_k<c64>>(ctx, dim3(1), dim3(kNormThreads), 0, static_cast<c64*>(p), count, log_out, flag);
    return qil_klaunch<frob_normalise_k<double>>(ctx, dim3(1), dim3(kNormThreads), 0, static_cast<double*>(p), count, log_out, flag);
}

// the existing one-matrix SVD with its factors discarded: the values of C (k x c, ld k; left intact) to host
static int svals_by_svd(qil_context* ctx, int dt, int64_t k, int64_t c, const void* C, double* S_host) {
    const size_t e = qil_elem_size(dt);
    const int64_t r0 = std::min(k, c);
    qil_scratch tmp(ctx);
    void *A = nullptr, *U = nullptr, *Vh = nullptr;
    QIL_TRY(tmp.alloc((size_t)(k * c) * e, &A));
    QIL_TRY(tmp.alloc((size_t)(k * r0) * e, &U));
    QIL_TRY(tmp.alloc((size_t)(r0 * c) * e, &Vh));
    QIL_TRY(qil_dev_copy(ctx, A, C, (size_t)(k * c) * e));
    return qil_dev_svd(ctx, dt, k, c, A, k, U, k, S_host, Vh, r0);
}

static int bond_spectra_impl(const qil_chain* src, double* S_out, double* norm_out) {
    qil_context* ctx = src->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int64_t N = src->n();
    const int dt = src->dtype;
    const size_t e = qil_elem_size(dt);
    const int64_t pd = src->phys_rank == 1 ? 2 : 4;
    const int cap = dt == QIL_C64 ? kCapC64 : kCapF64;
    const char* route = getenv("QIL_SPECTRA_ROUTE");
    const bool all_svd = route && !strcmp(route, "svd");

    // packed output: bond b (0-based) owns the src->dims[b + 1] slots from off[b]
    std::vector<int64_t> off((size_t)N, 0);
    for (int64_t b = 0; b + 1 < N; ++b) off[(size_t)b + 1] = off[(size_t)b] + src->dims[(size_t)b + 1];
    const int64_t total = off[(size_t)N - 1];
    QIL_REQUIRE(total < (1LL << 31), QIL_EINVAL_ARG, "bond_spectra: %lld values do not fit the packed index", (long long)total);

    // 1. the working clone
    qil_chain work;
    clone_guard guard{&work};
    QIL_TRY(qil_chain_alloc(ctx, &work, N, dt, src->paired, src->phys_rank, src->dims.data() + 1, src->site_ids.data()));
    for (int64_t i = 0; i < N; ++i) QIL_TRY(qil_dev_copy(ctx, work.site[(size_t)i], src->site[(size_t)i], src->site_bytes(i)));

    // one block for everything that goes back to the host: values | logarithms (N sites, N carries) | flags (state, bonds)
    qil_scratch tmp(ctx);
    const size_t val_bytes = (size_t)total * sizeof(double), log_bytes = (size_t)(2 * N) * sizeof(double);
    const size_t flag_bytes = (size_t)N * sizeof(int), out_bytes = val_bytes + log_bytes + flag_bytes;
    void* outd = nullptr;
    QIL_TRY(tmp.alloc(out_bytes, &outd));
    QIL_TRY(qil_dev_zero(ctx, outd, out_bytes));
    double* dS = static_cast<double*>(outd);
    double* dlog = dS + total;
    int* dflag = reinterpret_cast<int*>(dlog + 2 * N);

    {
        std::vector<NormSite> sites((size_t)N);
        for (int64_t i = 0; i < N; ++i) sites[(size_t)i] = NormSite{work.site[(size_t)i], (long long)work.site_elems(i)};
        qil_dev_table dtab(ctx);
        QIL_TRY(dtab.upload(sites.data(), sites.size() * sizeof(NormSite)));
        if (dt == QIL_C64)
            QIL_TRY((qil_klaunch<frob_normalise_sites_k<c64>>(ctx, dim3((unsigned)N), dim3(kNormThreads), 0, dtab.as<NormSite>(), dlog, dflag)));
        else
            QIL_TRY((qil_klaunch<frob_normalise_sites_k<double>>(ctx, dim3((unsigned)N), dim3(kNormThreads), 0, dtab.as<NormSite>(), dlog, dflag)));
        QIL_TRY(dtab.release());
        int zero_site = 0;
        QIL_TRY(qil_read_back(ctx, &zero_site, dflag, sizeof(int)));
        QIL_REQUIRE(!zero_site, QIL_EDOMAIN, "bond_spectra: zero or non-finite state");
    }

    // 2. right-orthonormal gauge (may shrink a bond that is wider than the cut can carry)
    if (N > 1) QIL_TRY(qil_gauge_exact(&work, QIL_DIR_LEFT, 1));

    // 3. left-to-right sweep of the carry
    std::vector<int64_t> ck((size_t)N, 0), cc((size_t)N, 0), coff((size_t)N, 0);     // C_b: ck x cc at element coff
    int64_t celems = 0;
    {
        int64_t k = 1;
        for (int64_t b = 0; b + 1 < N; ++b) {
            const int64_t cr = work.dims[(size_t)b + 1];
            k = std::min(pd * k, cr);
            QIL_REQUIRE(k <= src->dims[(size_t)b + 1], QIL_EHIP, "bond_spectra: bond %lld grew in the gauge sweep", (long long)(b + 1));
            ck[(size_t)b] = k, cc[(size_t)b] = cr, coff[(size_t)b] = celems;
            celems += k * cr;
        }
    }
    void* Cbuf = nullptr;
    if (N > 1) QIL_TRY(tmp.alloc((size_t)celems * e, &Cbuf));
    void* cur = work.site[0];          // site i with the carry multiplied in: (pd kprev) x cr
    int64_t kprev = 1;
    for (int64_t b = 0; b + 1 < N; ++b) {
        const int64_t rows = pd * kprev, cr = cc[(size_t)b], k = ck[(size_t)b], cr2 = work.dims[(size_t)b + 2];
        void* Cb = static_cast<char*>(Cbuf) + (size_t)coff[(size_t)b] * e;
        if (rows >= cr) QIL_TRY(qil_dev_qr_positive(ctx, dt, rows, cr, cur, rows, Cb, cr, true));
        else QIL_TRY(qil_dev_copy(ctx, Cb, cur, (size_t)(rows * cr) * e));            // Q = 1: the site is its own carry
        QIL_TRY(normalise_one(ctx, dt, Cb, k * cr, dlog + N + b, dflag));
        void* next = nullptr;
        QIL_TRY(tmp.alloc((size_t)(k * pd * cr2) * e, &next));
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, k, pd * cr2, cr, Cb, k, work.site[(size_t)b + 1], cr, next, k));
        if (b > 0) tmp.free(cur);
        cur = next;
        kprev = k;
    }
    // the last carry: a vector whose norm completes log |psi|
    QIL_TRY(normalise_one(ctx, dt, cur, pd * kprev * work.dims[(size_t)N], dlog + 2 * N - 1, dflag));

    // 4. the values: one launch for every bond that fits, the existing SVD for the rest
    std::vector<BondFactor> tab;
    std::vector<int64_t> by_svd;
    size_t lds = 0;
    for (int64_t b = 0; b + 1 < N; ++b) {
        const int64_t k = ck[(size_t)b], c = cc[(size_t)b];
        // routed by the operand's bond as the caller sees it: the factor is never larger (k <= c <= bond), so it fits
        if (all_svd || src->dims[(size_t)b + 1] > cap) {
            by_svd.push_back(b);
            continue;
        }
        tab.push_back(BondFactor{static_cast<const char*>(Cbuf) + (size_t)coff[(size_t)b] * e, (int)k, (int)c, (int)k,
                                 (int)off[(size_t)b], (int)(1 + b), 0});
        QIL_REQUIRE(k <= c, QIL_EHIP, "bond_spectra: carry %lld is %lld x %lld", (long long)(b + 1), (long long)k, (long long)c);
        lds = std::max(lds, (size_t)(c | 1) * (size_t)k * e);
    }
    if (!tab.empty()) {
        QIL_REQUIRE(lds <= kJacobiLdsBytes, QIL_EHIP, "bond_spectra: a factor of %zu bytes does not fit the LDS", lds);
        qil_dev_table dtab(ctx);
        QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(BondFactor)));
        if (dt == QIL_C64)
            QIL_TRY((qil_klaunch<bond_svals_batched_k<c64>>(ctx, dim3((unsigned)tab.size()), dim3(1024), lds, dtab.as<BondFactor>(), dS,
                                                            dflag, kSweepCap)));
        else
            QIL_TRY((qil_klaunch<bond_svals_batched_k<double>>(ctx, dim3((unsigned)tab.size()), dim3(1024), lds, dtab.as<BondFactor>(), dS,
                                                               dflag, kSweepCap)));
        QIL_TRY(dtab.release());
    }

    // 5. the one read-back of the results, then the bonds of the SVD route (the ones the kernel flagged included) on top of it
    std::vector<double> host((out_bytes + sizeof(double) - 1) / sizeof(double), 0.0);
    QIL_TRY(qil_read_back(ctx, host.data(), outd, out_bytes));
    const double* hlog = host.data() + total;
    const int* hflag = reinterpret_cast<const int*>(hlog + 2 * N);
    double lognorm = 0.0;
    for (int64_t i = 0; i < 2 * N; ++i) lognorm += hlog[i];
    QIL_REQUIRE(!hflag[0] && std::isfinite(lognorm), QIL_EDOMAIN, "bond_spectra: zero or non-finite state");
    for (int64_t b = 0; b + 1 < N; ++b)
        if (hflag[1 + b]) by_svd.push_back(b);
    std::vector<double> sv;
    for (int64_t b : by_svd) {
        const int64_t k = ck[(size_t)b], c = cc[(size_t)b], r0 = std::min(k, c);
        sv.assign((size_t)r0, 0.0);
        QIL_TRY(svals_by_svd(ctx, dt, k, c, static_cast<const char*>(Cbuf) + (size_t)coff[(size_t)b] * e, sv.data()));
        double* dst = host.data() + off[(size_t)b];
        std::fill(dst, dst + src->dims[(size_t)b + 1], 0.0);
        std::copy(sv.begin(), sv.end(), dst);
    }
    if (total > 0) memcpy(S_out, host.data(), val_bytes);
    if (norm_out) *norm_out = exp(lognorm);
    return QIL_OK;
}

}  // namespace

extern "C" int qil_bond_spectra(const qil_mps* psi, double* S_out, double* norm_out) {
    QIL_REQUIRE(psi && (S_out || psi->n() <= 1), QIL_EINVAL_ARG, "bond_spectra: null argument");
    return bond_spectra_impl(psi, S_out, norm_out);
}

extern "C" int qil_mpo_bond_spectra(const qil_mpo* W, double* S_out, double* norm_out) {
    QIL_REQUIRE(W && (S_out || W->n() <= 1), QIL_EINVAL_ARG, "bond_spectra: null argument");
    return bond_spectra_impl(W, S_out, norm_out);
}
