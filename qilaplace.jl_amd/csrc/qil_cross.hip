// Tensor cross interpolation of a signal of 2^n samples into an MPS: qil_cross_* (a pull-style session: the caller evaluates
// the samples the session asks for) and qil_signal_mps_cross (the same session driven by a gather from a dense signal).
//
// Sample j < 2^n has the bits b_1 .. b_n, site 1 the most significant.  For every bond l there is a list I_l of prefixes (the
// values of b_1 .. b_l) and a list J_l of suffixes (b_{l+1} .. b_n); I_0 = J_n = {empty}, J_l starts as the unique suffixes of
// the caller's seeds.  A step at bond l evaluates the two-site block P_l = x(I_{l-1} x {0,1} x {0,1} x J_{l+1})
// (2 |I_{l-1}| x 2 |J_{l+1}|, row 2 p + s, column s |J| + q) and factors it by LU with full pivoting: the pivot rows become I_l,
// the pivot columns J_l, the largest remaining |entry| is the bond's error estimate.  Pivots stop at rank maxdim, and after the
// first one when the largest remaining |entry| <= tol fmax, fmax the largest |x| sampled so far.  Sweeps run l = 1 .. n-1 and
// back; the iteration has converged when every estimate of a whole back-and-forth sweep is <= tol fmax.  A final forward
// sweep writes the sites: site l = L L11^-1 (L the unit lower factor, L11 its pivot rows), site n = the pivot rows of P_{n-1}.
//
// Kernels (one launch each per step, everything a step needs to know about the ranks stays on the device in CrossState):
//   cross_index    the 4 r r' int64 sample indices of a block
//   cross_gather   out[q] = idx[q] < len ? x[idx[q]] : 0          (the dense-signal route; zero fill as in qil_signal_mps)
//   cross_scan     max |value| of the seed samples (and the whole chain of n = 1)
//   cross_lu       one workgroup: arg-max search, swap bookkeeping (two permutations, nothing moves), rank-1 update fused with
//                  the next search, new I_l / J_l, rank, estimate; on the final sweep the triangular solve and the site.
//                  The block lives in LDS while the bound on its size fits kLdsBlockBytes, in a global work buffer otherwise:
//                  the same code on another pointer.  QIL_CROSS_ROUTE=lds|global (read per call) forces a route; a block that
//                  does not fit the LDS takes the global route whatever the switch says.
// The host knows upper bounds of the ranks only (they size the grids and choose the route); it reads CrossState back once per
// half-sweep.  A pull session additionally reads the sample count back once per block, because its caller needs it.
#include "qil_internal.h"
#include "qil_launch.h"
#include "qil_device_utils.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace {

using namespace qil_dev;

constexpr int kMaxSites = 64;              // n <= 62: bonds 0 .. n
constexpr int kMaxRank = 256;              // maxdim
constexpr int kMaxSeeds = 1024;            // seeds: the first sweep's blocks have up to 2 * kMaxSeeds columns
constexpr int kMaxRows = 2 * kMaxRank;
constexpr int kMaxCols = 2 * kMaxSeeds;
constexpr int kLuThreads = 1024;
constexpr int kLuWaves = kLuThreads / 64;
// LDS of cross_lu: the block (dynamic) + the two permutations + the reduction slots.  160 KiB per workgroup on gfx950.
constexpr size_t kLdsBlockBytes = 144 * 1024;
static_assert(kLdsBlockBytes + (kMaxRows + kMaxCols) * sizeof(int) + kLuWaves * 16 + 64 <= 160 * 1024, "cross_lu fits the LDS");

struct CrossState {
    double fmax;                  // largest |x| sampled so far
    double estmax;                // largest estimate of the running back-and-forth sweep
    unsigned long long nev;       // samples asked for (the seeds not counted)
    int cnt;                      // samples of the pending request
    int bad;                      // a block did not fit its buffers (never, unless the host's bounds are wrong)
    double est[kMaxSites];        // per bond: the largest remaining |entry| of its last factorisation
    int rI[kMaxSites];            // |I_l|
    int rJ[kMaxSites];            // |J_l|
};
static_assert(sizeof(CrossState) % 8 == 0 && sizeof(CrossState) <= 8192, "one read-back slot");

// the magnitude the pivot search orders by, and |v| from it
__device__ __forceinline__ double mag_t(double v) { return fabs(v); }
__device__ __forceinline__ double mag_t(c64 v) { return v.re * v.re + v.im * v.im; }
__device__ __forceinline__ double abs_of_mag(double m, const double*) { return m; }
__device__ __forceinline__ double abs_of_mag(double m, const c64*) { return sqrt(m); }
__device__ __forceinline__ double div_t(double a, double b) { return a / b; }
__device__ __forceinline__ c64 div_t(c64 a, c64 b) {
    const double d = b.re * b.re + b.im * b.im;
    return c64{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
__device__ __forceinline__ double mul_t(double a, double b) { return a * b; }
__device__ __forceinline__ c64 mul_t(c64 a, c64 b) { return c64{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// ---- sample indices of the block at bond l ------------------------------------------------------------------------------
__device__ __forceinline__ void cross_index_body(const uint3 blockIdx, const uint3 gridDim, const long long* __restrict__ Iprev,
                                                   const long long* __restrict__ Jnext, CrossState* __restrict__ st, int l, int n,
                                                   long long cap_elems, long long* __restrict__ idx) {
    const int kJ = st->rJ[l + 1];
    const long long m = 2LL * st->rI[l - 1], total = m * 2LL * kJ;
    if (total > cap_elems) {
        if (blockIdx.x == 0 && threadIdx.x == 0) st->bad = 1, st->cnt = 0;
        return;
    }
    for (long long q = blockIdx.x * 256LL + threadIdx.x; q < total; q += gridDim.x * 256LL) {
        const long long pr = q % m, pc = q / m;
        const long long row = (Iprev[pr >> 1] << 1) | (pr & 1);
        const long long s = pc / kJ;
        const long long col = (s << (n - l - 1)) | Jnext[pc - s * kJ];
        idx[q] = (row << (n - l)) | col;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->cnt = (int)total;
        st->nev += (unsigned long long)total;
    }
}
struct cross_index_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        cross_index_body(b, g, a...);
    }
};

// ---- the dense-signal evaluator -------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void cross_gather_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ x, long long len,
                                                    const long long* __restrict__ idx, const int* __restrict__ cnt,
                                                    T* __restrict__ out) {
    const long long total = *cnt;
    for (long long q = blockIdx.x * 256LL + threadIdx.x; q < total; q += gridDim.x * 256LL) {
        const long long j = idx[q];
        out[q] = j < len ? x[j] : T{};
    }
}
template <class T>
struct cross_gather_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        cross_gather_body<T>(b, g, a...);
    }
};

// ---- fmax of a plain list of samples: the seeds, and the two samples that are the whole chain of n = 1 ----------------------
template <class T>
__device__ __forceinline__ void cross_scan_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ vals,
                                                  CrossState* __restrict__ st, T* __restrict__ site, int add_nev) {
    __shared__ double red[4];
    const int count = st->cnt;
    double mx = 0.0;
    for (int t = threadIdx.x; t < count; t += 256) {
        const T v = vals[t];
        mx = fmax(mx, abs_of_mag(mag_t(v), static_cast<const T*>(nullptr)));
        if (site) site[t] = v;
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        st->fmax = fmax(st->fmax, fmax(fmax(red[0], red[1]), fmax(red[2], red[3])));
        if (add_nev) st->nev += (unsigned long long)count;
    }
}
template <class T>
struct cross_scan_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        cross_scan_body<T>(b, g, a...);
    }
};

// ---- LU with full pivoting of one block -------------------------------------------------------------------------------------
// The largest magnitude of the workgroup's candidates and its position (logical column * m + logical row: the lowest
// column-major position wins a tie), to every thread.  Two barriers.
__device__ __forceinline__ void lu_reduce(double& mag, unsigned& pos, double* s_mag, unsigned* s_pos) {
    for (int o = 32; o > 0; o >>= 1) {
        const double om = __shfl_xor(mag, o, 64);
        const unsigned op = (unsigned)__shfl_xor((int)pos, o, 64);
        if (om > mag || (om == mag && op < pos)) mag = om, pos = op;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_mag[wave] = mag, s_pos[wave] = pos;
    __syncthreads();
    mag = s_mag[0], pos = s_pos[0];
    for (int w = 1; w < kLuWaves; ++w) {
        const double om = s_mag[w];
        const unsigned op = s_pos[w];
        if (om > mag || (om == mag && op < pos)) mag = om, pos = op;
    }
    __syncthreads();
}

constexpr int kFlagFirst = 1;    // first block of a back-and-forth sweep: estmax starts afresh
constexpr int kFlagSite = 2;     // final sweep: write site l
constexpr int kFlagLast = 4;     // ... and site n (l = n - 1)

struct LuArgs {
    CrossState* st;
    const long long* Iprev;      // I_{l-1}
    const long long* Jnext;      // J_{l+1}
    long long* Iout;             // I_l
    long long* Jout;             // J_l
    void* site;                  // A[alpha, s, beta], alpha fastest (kFlagSite)
    void* site_last;             // (kFlagLast)
    long long cap_elems;         // elements the block may occupy
    double tol;
    int l, n, maxdim, flags;
};

// Logical entry (i, j) of the block lies at A[rowp[i] + m colp[j]]: a pivot swaps two entries of a permutation and moves nothing.
// Thread (ti, tj) = (tid % 64, tid / 64) owns the logical rows ti, ti + 64, .. of the logical columns tj, tj + 16, ..
template <class T, bool LDS>
__device__ __forceinline__ void cross_lu_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ vals, T* work,
                                                LuArgs P) {
    extern __shared__ __attribute__((aligned(16))) char cross_smem[];
    __shared__ int s_rowp[kMaxRows];
    __shared__ int s_colp[kMaxCols];
    __shared__ double s_mag[kLuWaves];
    __shared__ unsigned s_pos[kLuWaves];
    CrossState* st = P.st;
    const int tid = threadIdx.x, ti = tid & 63, tj = tid >> 6;
    const int l = P.l, n = P.n;
    const int cl = st->rI[l - 1], kJ = st->rJ[l + 1];
    const int m = 2 * cl, k = 2 * kJ;
    if (m > kMaxRows || k > kMaxCols || (long long)m * k > P.cap_elems) {
        if (tid == 0) st->bad = 1;
        return;
    }
    T* A = LDS ? reinterpret_cast<T*>(cross_smem) : work;
    for (int t = tid; t < m * k; t += kLuThreads) A[t] = vals[t];
    for (int t = tid; t < m; t += kLuThreads) s_rowp[t] = t;
    for (int t = tid; t < k; t += kLuThreads) s_colp[t] = t;
    const double fmax0 = st->fmax;
    __threadfence_block();
    __syncthreads();

    // the first search: the whole block
    double mag = -1.0;
    unsigned pos = 0xffffffffu;
    for (int j = tj; j < k; j += kLuWaves)
        for (int i = ti; i < m; i += 64) {
            const double v = mag_t(A[i + m * j]);
            if (v > mag) mag = v, pos = (unsigned)(j * m + i);
        }
    lu_reduce(mag, pos, s_mag, s_pos);

    const int full = min(m, k);
    int r = 0;
    double est = 0.0, fmx = fmax0, tol_abs = 0.0;
    while (r < full) {
        const double v = abs_of_mag(fmax(mag, 0.0), static_cast<const T*>(nullptr));
        if (r == 0) {
            fmx = fmax(fmax0, v);
            tol_abs = P.tol * fmx;
        }
        if (r >= P.maxdim || (r > 0 && (v <= tol_abs || v == 0.0))) {
            est = v;
            break;
        }
        // an all-zero block still takes one pivot (its first entry, nothing to divide): the chain stays connected
        const int pi = mag > 0.0 ? (int)(pos % (unsigned)m) : r, pj = mag > 0.0 ? (int)(pos / (unsigned)m) : r;
        if (tid == 0) {
            const int a = s_rowp[r], b = s_colp[r];
            s_rowp[r] = s_rowp[pi], s_rowp[pi] = a;
            s_colp[r] = s_colp[pj], s_colp[pj] = b;
        }
        __syncthreads();
        const int pr = s_rowp[r], pc = s_colp[r];
        if (mag > 0.0) {
            const T piv = A[pr + m * pc];
            for (int i = r + 1 + tid; i < m; i += kLuThreads) {
                const int q = s_rowp[i] + m * pc;
                A[q] = div_t(A[q], piv);
            }
        }
        __threadfence_block();
        __syncthreads();
        // rank-1 update of the trailing block and the search of the next pivot in one pass
        mag = -1.0, pos = 0xffffffffu;
        for (int j = r + 1 + tj; j < k; j += kLuWaves) {
            const int cj = s_colp[j];
            const T u = A[pr + m * cj];
            for (int i = r + 1 + ti; i < m; i += 64) {
                const int ri = s_rowp[i];
                const T a = sub_t(A[ri + m * cj], mul_t(A[ri + m * pc], u));
                A[ri + m * cj] = a;
                const double w = mag_t(a);
                if (w > mag) mag = w, pos = (unsigned)(j * m + i);
            }
        }
        __threadfence_block();
        lu_reduce(mag, pos, s_mag, s_pos);
        ++r;
    }

    // the new lists, the rank, the estimate
    for (int a = tid; a < r; a += kLuThreads) {
        const int pr = s_rowp[a], pc = s_colp[a];
        P.Iout[a] = (P.Iprev[pr >> 1] << 1) | (long long)(pr & 1);
        const int s = pc / kJ;
        P.Jout[a] = ((long long)s << (n - l - 1)) | P.Jnext[pc - s * kJ];
    }
    if (tid == 0) {
        st->fmax = fmx;
        st->est[l] = est;
        st->estmax = (P.flags & kFlagFirst) ? est : fmax(st->estmax, est);
        st->rI[l] = r;
        st->rJ[l] = r;
    }
    if (!(P.flags & kFlagSite)) return;

    // X = L L11^-1 in place: rows a >= r of the columns < r.  x L11 = l, L11 unit lower: for beta = r-1 .. 1 the final x_beta
    // leaves the columns gamma < beta.
    for (int beta = r - 1; beta >= 1; --beta) {
        const int cb = s_colp[beta], rb = s_rowp[beta];
        for (int g = tj; g < beta; g += kLuWaves) {
            const int cg = s_colp[g];
            const T lbg = A[rb + m * cg];
            for (int a = r + ti; a < m; a += 64) {
                const int ra = s_rowp[a];
                A[ra + m * cg] = sub_t(A[ra + m * cg], mul_t(A[ra + m * cb], lbg));
            }
        }
        __threadfence_block();
        __syncthreads();
    }
    // site l: physical row 2 alpha + s of the block is A[alpha, s, :]
    T* site = static_cast<T*>(P.site);
    for (int t = tid; t < m * r; t += kLuThreads) {
        const int a = t % m, beta = t / m;
        const int pr = s_rowp[a];
        const T v = a < r ? make_elem(a == beta ? 1.0 : 0.0, 0.0, static_cast<T*>(nullptr)) : A[pr + m * s_colp[beta]];
        site[(pr >> 1) + cl * ((pr & 1) + 2 * beta)] = v;
    }
    if (P.flags & kFlagLast) {                 // l = n - 1: |J_n| = 1, the block has the two columns s = 0, 1
        T* last = static_cast<T*>(P.site_last);
        for (int t = tid; t < 2 * r; t += kLuThreads) {
            const int a = t % r, s = t / r;
            last[a + r * s] = vals[s_rowp[a] + m * s];
        }
    }
}
template <class T, bool LDS>
struct cross_lu_k {
    static constexpr int NT = kLuThreads, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        cross_lu_body<T, LDS>(b, g, a...);
    }
};

}  // namespace

// ---- the session ------------------------------------------------------------------------------------------------------------
enum { kPhSeeds = 0, kPhBlock = 1, kPhSingle = 2, kPhDone = 3, kPhFinished = 4 };
enum { kDirFwd = 0, kDirBack = 1, kDirFinal = 2 };

struct qil_cross {
    qil_context* ctx = nullptr;
    int64_t n = 0, maxdim = 0, nseeds = 0, cap = 0, cap_elems = 0;
    int dtype = QIL_F64, max_sweeps = 0;
    double tol = 0;
    bool pull = true;                      // a caller evaluates: the sample count is read back for every block
    // device (pool blocks of ctx, all allocated by begin)
    CrossState* st = nullptr;
    long long *I = nullptr, *J = nullptr, *idx = nullptr;   // I_l at I + l cap, J_l at J + l cap
    void *vals = nullptr, *work = nullptr, *sites = nullptr;
    std::vector<int64_t> ubI, ubJ, soff;   // upper bounds of |I_l|, |J_l|; element offset of site i (0-based) in `sites`
    // where the iteration is
    int phase = kPhSeeds, dir = kDirFwd, sweeps_done = 0, converged = 0;
    int64_t l = 1, count = 0;
    double est_abs = 0;
    CrossState host = {};
};

namespace {

void cross_free(qil_cross* s) {
    if (!s) return;
    for (void* p : {(void*)s->st, (void*)s->I, (void*)s->J, (void*)s->idx, s->vals, s->work, s->sites})
        if (p) (void)qil_ctx_free(s->ctx, p);
    delete s;
}
struct cross_guard {
    qil_cross* s;
    ~cross_guard() { cross_free(s); }
    qil_cross* release() {
        qil_cross* t = s;
        s = nullptr;
        return t;
    }
};

int cross_read_state(qil_cross* s) {
    QIL_TRY(qil_read_back(s->ctx, &s->host, s->st, sizeof(CrossState)));
    QIL_REQUIRE(!s->host.bad, QIL_EHIP, "cross: a block outgrew its buffers");
    QIL_REQUIRE(std::isfinite(s->host.fmax), QIL_EDOMAIN, "cross: a sampled value is not finite");
    return QIL_OK;
}

// the index kernel of bond s->l; a pull session learns the count
int cross_prepare(qil_cross* s) {
    const int64_t l = s->l;
    const long long bound = 4LL * s->ubI[(size_t)l - 1] * s->ubJ[(size_t)l + 1];
    QIL_REQUIRE(bound <= s->cap_elems, QIL_EHIP, "cross: block bound %lld above the buffers", bound);
    QIL_TRY((qil_klaunch<cross_index_k>(s->ctx, dim3(qil_grid_for(bound)), dim3(256), 0, (const long long*)(s->I + (l - 1) * s->cap),
                                        (const long long*)(s->J + (l + 1) * s->cap), s->st, (int)l, (int)s->n,
                                        (long long)s->cap_elems, s->idx)));
    if (s->pull) {
        int cnt = 0;
        QIL_TRY(qil_read_back(s->ctx, &cnt, &s->st->cnt, sizeof(int)));
        QIL_REQUIRE(cnt > 0, QIL_EHIP, "cross: a block outgrew its buffers");
        s->count = cnt;
    }
    return QIL_OK;
}

template <class T>
int cross_launch_lu(qil_cross* s, const void* vals, int flags) {
    const int64_t l = s->l;
    const size_t bytes = (size_t)(4 * s->ubI[(size_t)l - 1] * s->ubJ[(size_t)l + 1]) * sizeof(T);
    const char* route = getenv("QIL_CROSS_ROUTE");
    const bool lds = bytes <= kLdsBlockBytes && !(route && !strcmp(route, "global"));
    LuArgs P;
    P.st = s->st;
    P.Iprev = s->I + (l - 1) * s->cap;
    P.Jnext = s->J + (l + 1) * s->cap;
    P.Iout = s->I + l * s->cap;
    P.Jout = s->J + l * s->cap;
    P.site = static_cast<T*>(s->sites) + s->soff[(size_t)l - 1];
    P.site_last = static_cast<T*>(s->sites) + s->soff[(size_t)s->n - 1];
    P.cap_elems = lds ? (long long)(bytes / sizeof(T)) : (long long)s->cap_elems;    // what the block may fill: the LDS asked for, or the work buffer
    P.tol = s->tol;
    P.l = (int)l, P.n = (int)s->n, P.maxdim = (int)s->maxdim, P.flags = flags;
    if (lds) return qil_klaunch<cross_lu_k<T, true>>(s->ctx, dim3(1), dim3(kLuThreads), bytes, static_cast<const T*>(vals), static_cast<T*>(s->work), P);
    return qil_klaunch<cross_lu_k<T, false>>(s->ctx, dim3(1), dim3(kLuThreads), 0, static_cast<const T*>(vals), static_cast<T*>(s->work), P);
}

template <class T>
int cross_launch_scan(qil_cross* s, const void* vals, void* site, int add_nev) {
    return qil_klaunch<cross_scan_k<T>>(s->ctx, dim3(1), dim3(256), 0, static_cast<const T*>(vals), s->st, static_cast<T*>(site), add_nev);
}

// the values of the pending request have arrived: factor, move on, ask for the next block
int cross_consume(qil_cross* s, const void* vals) {
    const bool c64v = s->dtype == QIL_C64;
    const int64_t n = s->n;
    if (s->phase == kPhSeeds) {
        QIL_TRY(c64v ? cross_launch_scan<c64>(s, vals, nullptr, 0) : cross_launch_scan<double>(s, vals, nullptr, 0));
        if (n == 1) {
            const int two = 2;                                            // the chain is the samples 0 and 1
            const long long both[2] = {0, 1};
            QIL_HIP(hipMemcpyAsync(s->idx, both, sizeof(both), hipMemcpyHostToDevice, qil_stream(s->ctx)));
            QIL_HIP(hipMemcpyAsync(&s->st->cnt, &two, sizeof(int), hipMemcpyHostToDevice, qil_stream(s->ctx)));
            QIL_HIP(qil_stream_sync(s->ctx));
            s->phase = kPhSingle, s->count = 2;
            return QIL_OK;
        }
        s->phase = kPhBlock, s->dir = kDirFwd, s->l = 1;
        return cross_prepare(s);
    }
    if (s->phase == kPhSingle) {
        QIL_TRY(c64v ? cross_launch_scan<c64>(s, vals, s->sites, 1) : cross_launch_scan<double>(s, vals, s->sites, 1));
        QIL_TRY(cross_read_state(s));
        s->phase = kPhDone, s->count = 0, s->sweeps_done = 1, s->converged = 1, s->est_abs = 0;
        return QIL_OK;
    }
    const int64_t l = s->l;
    int flags = 0;
    if (s->dir == kDirFwd && l == 1) flags |= kFlagFirst;
    if (s->dir == kDirFinal) flags |= kFlagSite | (l == n - 1 ? kFlagLast : 0);
    QIL_TRY(c64v ? cross_launch_lu<c64>(s, vals, flags) : cross_launch_lu<double>(s, vals, flags));
    s->ubI[(size_t)l] = s->ubJ[(size_t)l] = std::min({s->maxdim, 2 * s->ubI[(size_t)l - 1], 2 * s->ubJ[(size_t)l + 1]});
    // the next block, or the end of a half-sweep
    const bool half_done = s->dir == kDirBack ? l == 1 : l == n - 1;
    if (!half_done) {
        s->l += s->dir == kDirBack ? -1 : 1;
        return cross_prepare(s);
    }
    QIL_TRY(cross_read_state(s));
    QIL_REQUIRE(s->host.fmax > 0, QIL_EDOMAIN, "signal_mps_cross: every sampled value is 0");
    if (s->dir == kDirFwd) {
        s->dir = kDirBack, s->l = n - 1;
    } else if (s->dir == kDirBack) {
        ++s->sweeps_done;
        s->est_abs = s->host.estmax;
        s->converged = s->host.estmax <= s->tol * s->host.fmax ? 1 : 0;
        s->dir = s->converged || s->sweeps_done >= s->max_sweeps ? kDirFinal : kDirFwd;
        s->l = 1;
    } else {
        s->phase = kPhDone, s->count = 0;
        return QIL_OK;
    }
    return cross_prepare(s);
}

int cross_begin_impl(qil_context* ctx, int64_t n, int dtype, int64_t maxdim, double tol, int max_sweeps, const int64_t* seeds,
                     int64_t nseeds, bool pull, qil_cross** out) {
    qil_cross* s = new qil_cross();
    cross_guard guard{s};
    s->ctx = ctx, s->n = n, s->dtype = dtype, s->maxdim = maxdim, s->tol = tol, s->max_sweeps = max_sweeps, s->nseeds = nseeds;
    s->pull = pull;
    const size_t e = qil_elem_size(dtype);
    // J_l = the unique suffixes of the seeds, ascending
    std::vector<std::vector<long long>> J0((size_t)n + 1);
    for (int64_t l = 1; l < n; ++l) {
        std::vector<long long>& v = J0[(size_t)l];
        const long long mask = (1LL << (n - l)) - 1;
        for (int64_t t = 0; t < nseeds; ++t) v.push_back((long long)seeds[t] & mask);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
    }
    J0[(size_t)n] = {0};
    s->cap = maxdim;
    for (const auto& v : J0) s->cap = std::max<int64_t>(s->cap, (int64_t)v.size());
    s->ubI.assign((size_t)n + 1, 1);
    s->ubJ.assign((size_t)n + 1, 1);
    auto pow2cap = [&](int64_t bits) { return bits >= 9 ? maxdim : std::min<int64_t>(maxdim, 1LL << bits); };
    s->cap_elems = std::max<int64_t>(nseeds, 2);
    for (int64_t l = 0; l <= n; ++l) {
        s->ubI[(size_t)l] = pow2cap(l);
        s->ubJ[(size_t)l] = (int64_t)J0[(size_t)l].size();
    }
    s->ubJ[0] = 1;
    for (int64_t l = 1; l < n; ++l)
        s->cap_elems = std::max(s->cap_elems, 4 * pow2cap(l - 1) * std::max<int64_t>(s->ubJ[(size_t)l + 1], pow2cap(n - l - 1)));
    s->soff.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i)                                       // site i + 1: 2 |I_i| |I_{i+1}|, |I_l| <= 2^(n-l) as well
        s->soff[(size_t)i + 1] = s->soff[(size_t)i] + 2 * pow2cap(i) * std::min(pow2cap(i + 1), pow2cap(n - i - 1));

    void* p = nullptr;
    QIL_TRY(qil_ctx_alloc(ctx, sizeof(CrossState), &p));
    s->st = static_cast<CrossState*>(p);
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)((n + 1) * s->cap) * sizeof(long long), &p));
    s->I = static_cast<long long*>(p);
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)((n + 1) * s->cap) * sizeof(long long), &p));
    s->J = static_cast<long long*>(p);
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)s->cap_elems * sizeof(long long), &p));
    s->idx = static_cast<long long*>(p);
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)s->cap_elems * e, &s->vals));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)s->cap_elems * e, &s->work));
    QIL_TRY(qil_ctx_alloc(ctx, (size_t)s->soff[(size_t)n] * e, &s->sites));

    // the start: state, lists, and the seeds as the first request
    std::vector<long long> lists((size_t)((n + 1) * s->cap), 0);
    CrossState h = {};
    h.cnt = (int)nseeds;
    h.rI[0] = 1;
    for (int64_t l = 1; l <= n; ++l) {
        h.rJ[l] = (int)J0[(size_t)l].size();
        std::copy(J0[(size_t)l].begin(), J0[(size_t)l].end(), lists.begin() + l * s->cap);
    }
    std::vector<long long> sd(seeds, seeds + nseeds);
    const hipStream_t stream = qil_stream(ctx);
    QIL_HIP(hipMemcpyAsync(s->st, &h, sizeof(h), hipMemcpyHostToDevice, stream));
    QIL_HIP(hipMemcpyAsync(s->J, lists.data(), lists.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
    QIL_TRY(qil_dev_zero(ctx, s->I, (size_t)((n + 1) * s->cap) * sizeof(long long)));
    QIL_HIP(hipMemcpyAsync(s->idx, sd.data(), sd.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
    QIL_HIP(qil_stream_sync(ctx));
    s->phase = kPhSeeds, s->count = nseeds;
    *out = guard.release();
    return QIL_OK;
}

// the chain of a finished session in the gauge of qil_signal_mps: unit norm, amplitude = the norm of the represented signal
int cross_finish_impl(qil_cross* s, qil_mps** out, double* est, int64_t* nevals, int* sweeps, int* converged) {
    qil_context* ctx = s->ctx;
    const int64_t n = s->n;
    const size_t e = qil_elem_size(s->dtype);
    qil_result_guard<qil_mps> own(qil_mps_empty(ctx, n, s->dtype, 0, nullptr, 1.0));
    qil_mps* psi = own.p;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t cl = i == 0 ? 1 : s->host.rI[i], cr = i == n - 1 ? 1 : s->host.rI[i + 1];
        QIL_REQUIRE(cl >= 1 && cr >= 1 && 2 * cl * cr <= s->soff[(size_t)i + 1] - s->soff[(size_t)i], QIL_EHIP,
                    "cross: site %lld is %lld x 2 x %lld", (long long)(i + 1), (long long)cl, (long long)cr);
        void* p = nullptr;
        QIL_TRY(qil_ctx_alloc(ctx, (size_t)(2 * cl * cr) * e, &p));
        qil_chain_adopt(psi, i, p);
        psi->dims[(size_t)i] = cl, psi->dims[(size_t)i + 1] = cr;
        QIL_TRY(qil_dev_copy(ctx, p, static_cast<const char*>(s->sites) + (size_t)s->soff[(size_t)i] * e, (size_t)(2 * cl * cr) * e));
    }
    if (n > 1) QIL_TRY(qil_gauge_exact(psi, QIL_DIR_LEFT, 1));
    double nrm = 0;
    QIL_TRY(qil_norm(psi, &nrm));
    QIL_REQUIRE(nrm > 0 && std::isfinite(nrm), QIL_EDOMAIN, "signal_mps_cross: the interpolant has zero or non-finite norm");
    psi->amplitude = nrm;
    std::vector<double> inv((size_t)psi->dims[1], 1.0 / nrm);
    QIL_TRY(qil_dev_scale(ctx, s->dtype, 1, 2 * psi->dims[0], psi->dims[1], psi->site[0], 2 * psi->dims[0], inv.data()));
    if (est) *est = s->est_abs / s->host.fmax;
    if (nevals) *nevals = (int64_t)s->host.nev;
    if (sweeps) *sweeps = s->sweeps_done;
    if (converged) *converged = s->converged;
    s->phase = kPhFinished;
    *out = own.release();
    return QIL_OK;
}

int cross_check_args(const char* verb, qil_context* ctx, int64_t n, int dtype, int64_t maxdim, double tol, int max_sweeps,
                     const int64_t* seeds, int64_t nseeds, const void* out) {
    QIL_REQUIRE(ctx && out, QIL_EINVAL_ARG, "%s: null argument", verb);
    QIL_REQUIRE(dtype == QIL_F64 || dtype == QIL_C64, QIL_EINVAL_ARG, "%s: unknown dtype %d", verb, dtype);
    QIL_REQUIRE(n >= 1 && n <= 62, QIL_EINVAL_ARG, "%s: n = %lld outside 1 .. 62", verb, (long long)n);
    QIL_REQUIRE(maxdim >= 1 && maxdim <= kMaxRank, QIL_EINVAL_ARG, "%s: maxdim must be finite, 1 .. %d", verb, kMaxRank);
    QIL_REQUIRE(tol >= 0, QIL_EINVAL_ARG, "%s: tol must be >= 0", verb);
    QIL_REQUIRE(max_sweeps >= 1, QIL_EINVAL_ARG, "%s: max_sweeps must be >= 1", verb);
    QIL_REQUIRE(seeds && nseeds >= 1 && nseeds <= kMaxSeeds, QIL_EINVAL_ARG, "%s: between 1 and %d seeds", verb, kMaxSeeds);
    for (int64_t t = 0; t < nseeds; ++t)
        QIL_REQUIRE(seeds[t] >= 0 && seeds[t] < (1LL << n), QIL_EINVAL_ARG, "%s: seed %lld outside [0, 2^%lld)", verb,
                    (long long)seeds[t], (long long)n);
    return QIL_OK;
}

}  // namespace

int qil_cross_check_args(const char* verb, qil_context* ctx, int64_t n, int dtype, int64_t maxdim, double tol, int max_sweeps,
                         const int64_t* seeds, int64_t nseeds, const void* out) {
    return cross_check_args(verb, ctx, n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, out);
}

// The session with its evaluator inside the library (qil_signal_mps_cross: a gather from the signal; qil_mps_map: the index
// read-out of the operands): the sample count stays in CrossState::cnt, the grids are sized by the host's bounds.
int qil_cross_run(qil_context* ctx, int64_t n, int dtype, int64_t maxdim, double tol, int max_sweeps, const int64_t* seeds,
                  int64_t nseeds, const qil_cross_eval& eval, qil_mps** out, double* est, int64_t* nevals, int* sweeps,
                  int* converged) {
    qil_cross* s = nullptr;
    QIL_TRY(cross_begin_impl(ctx, n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, false, &s));
    cross_guard guard{s};
    while (s->phase < kPhDone) {
        const long long bound = s->phase == kPhBlock ? 4LL * s->ubI[(size_t)s->l - 1] * s->ubJ[(size_t)s->l + 1] : std::max<long long>(nseeds, 2);
        QIL_TRY(eval((const long long*)s->idx, (const int*)&s->st->cnt, bound, s->vals));
        QIL_TRY(cross_consume(s, s->vals));
    }
    return cross_finish_impl(s, out, est, nevals, sweeps, converged);
}

extern "C" int qil_cross_begin(qil_context* ctx, int64_t n, int dtype, int64_t maxdim, double tol, int max_sweeps,
                               const int64_t* seeds, int64_t nseeds, qil_cross** out) {
    QIL_TRY(cross_check_args("cross_begin", ctx, n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, out));
    *out = nullptr;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    return cross_begin_impl(ctx, n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, true, out);
}

extern "C" int qil_cross_pending(qil_cross* s, int64_t* count) {
    QIL_REQUIRE(s && count, QIL_EINVAL_ARG, "cross_pending: null argument");
    *count = s->phase >= kPhDone ? 0 : s->count;
    return QIL_OK;
}

extern "C" int qil_cross_indices(qil_cross* s, int64_t* idx_dev) {
    QIL_REQUIRE(s && idx_dev, QIL_EINVAL_ARG, "cross_indices: null argument");
    QIL_REQUIRE(s->phase < kPhDone, QIL_EINVAL_ARG, "cross_indices: nothing is pending");
    QIL_TRY(qil_ctx_activate(s->ctx));
    qil_call_scope call_scope(s->ctx);
    QIL_TRY(qil_dev_copy(s->ctx, idx_dev, s->idx, (size_t)s->count * sizeof(long long)));
    QIL_HIP(qil_stream_sync(s->ctx));             // the caller reads them on a stream of its own
    return QIL_OK;
}

extern "C" int qil_cross_supply(qil_cross* s, const void* values_dev) {
    QIL_REQUIRE(s && values_dev, QIL_EINVAL_ARG, "cross_supply: null argument");
    QIL_REQUIRE(s->phase < kPhDone, QIL_EINVAL_ARG, "cross_supply: nothing is pending");
    QIL_TRY(qil_ctx_activate(s->ctx));
    qil_call_scope call_scope(s->ctx);
    // the caller's buffer is read by kernels of this call only: copy first, so that it may be reused when the call returns
    QIL_TRY(qil_dev_copy(s->ctx, s->vals, values_dev, (size_t)s->count * qil_elem_size(s->dtype)));
    QIL_TRY(cross_consume(s, s->vals));
    QIL_HIP(qil_stream_sync(s->ctx));
    return QIL_OK;
}

extern "C" int qil_cross_finish(qil_cross* s, qil_mps** out, double* est, int64_t* nevals, int* sweeps, int* converged) {
    QIL_REQUIRE(s && out, QIL_EINVAL_ARG, "cross_finish: null argument");
    QIL_REQUIRE(s->phase == kPhDone, QIL_EINVAL_ARG, "cross_finish: %s",
                s->phase == kPhFinished ? "the session has delivered its result" : "samples are still pending");
    QIL_TRY(qil_ctx_activate(s->ctx));
    qil_call_scope call_scope(s->ctx);
    return cross_finish_impl(s, out, est, nevals, sweeps, converged);
}

extern "C" int qil_cross_destroy(qil_cross* s) {
    if (!s) return QIL_OK;
    cross_free(s);
    return QIL_OK;
}

extern "C" int qil_signal_mps_cross(qil_context* ctx, const void* x, int64_t len, int dtype, int64_t maxdim, double tol,
                                    int max_sweeps, const int64_t* seeds, int64_t nseeds, qil_mps** out, double* est,
                                    int64_t* nevals, int* sweeps, int* converged) {
    QIL_REQUIRE(ctx && x && out, QIL_EINVAL_ARG, "signal_mps_cross: null argument");
    QIL_REQUIRE(len >= 1, QIL_EINVAL_LENGTH, "signal_mps_cross: empty signal");
    // _array_to_tensor: n = round(log2 N), a shorter signal is zero-filled, a longer one refused
    const int64_t n = std::max<int64_t>(1, (int64_t)std::llround(std::log2((double)len)));
    QIL_REQUIRE(n <= 62 && len <= (1LL << n), QIL_EINVAL_LENGTH,
                "_array_to_tensor: Length of signal vector must be a power of 2 (got %lld)", (long long)len);
    QIL_TRY(cross_check_args("signal_mps_cross", ctx, n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, out));
    *out = nullptr;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const size_t e = qil_elem_size(dtype);
    qil_scratch tmp(ctx);
    const void* xd = x;
    hipPointerAttribute_t at;
    if (!(hipPointerGetAttributes(&at, x) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == ctx->device)) {
        (void)hipGetLastError();
        void* up = nullptr;
        QIL_TRY(qil_upload_bytes(tmp, x, (size_t)len * e, &up));
        xd = up;
    }
    const qil_cross_eval gather = [&](const long long* idx, const int* cnt, long long bound, void* vals) {
        if (dtype == QIL_C64)
            return qil_klaunch<cross_gather_k<c64>>(ctx, dim3(qil_grid_for(bound)), dim3(256), 0, static_cast<const c64*>(xd), (long long)len,
                                                    idx, cnt, static_cast<c64*>(vals));
        return qil_klaunch<cross_gather_k<double>>(ctx, dim3(qil_grid_for(bound)), dim3(256), 0, static_cast<const double*>(xd), (long long)len,
                                                   idx, cnt, static_cast<double*>(vals));
    };
    QIL_TRY(qil_cross_run(ctx, n, dtype, maxdim, tol, max_sweeps, seeds, nseeds, gather, out, est, nevals, sweeps, converged));
    QIL_HIP(qil_stream_sync(ctx));                 // `x` is caller memory: read completely before the call returns
    return QIL_OK;
}
