// The eigen-solver (qil_mps_eigs): the smallest or largest eigenpair of a Hermitian operator in MPS form by the alternating
// two-site sweep (two-site DMRG).  The sweep, the environments, the matvec, the split and the frame of both routes are shared with
// the linear solver and the time evolution (qil_twosite.h, qil_twosite.hip); the local problem at bond k is
//     H v = L_A A_k A_{k+1} R_A v + s weight sum_i g_i (g_i^H v),   g_i = Lphi_i phi_i,k phi_i,k+1 Rphi_i,   s = +1 / -1,
// the penalty pushing the deflation states phi_i away from the wanted end, and it is solved by restarted Lanczos with full
// reorthogonalisation from the current two-site tensor y: at most `krylov` vectors, each orthogonalised twice against all earlier
// ones, the tridiagonal projected matrix diagonalised by cyclic Jacobi rotations, the Ritz pair at the wanted end the next start,
// at most `restarts` times.  A restart begins with theta = <y|H y> and r = H y - theta y and the iteration stops when
// |r| <= tol scale, scale = the largest |Ritz value| the call has seen (with deflation states only Ritz values at the wanted end
// count: the penalty moves the other end by up to `weight`).
//
//   local route   ONE launch, one workgroup (eigs_local): both environments, both operator sites, the Krylov basis, the work
//                 vector, the g_i, two ping-pong blocks and the projected problem in LDS, the whole restarted iteration in it
//   gemm route    the matvec as four f64-MFMA products, the basis in device memory, the same vector steps as small one-workgroup
//                 kernels (eigs_begin, eigs_step, eigs_ritz) with alpha, beta and the flags in device memory; the host reads the
//                 flags once per restart, behind its first step (the stopping test); any bonds
//
// Both routes run the same device functions on their vectors (lanczos_step, ritz_restart), so they differ by the rounding of the
// matvec alone.  The g_i are formed in device memory for both routes (Sweep::overlap_local).  Every temporary belongs to the
// call's qil_scratch; the working copy of x is the result handle.
#include "qil_twosite.h"

namespace {

using namespace qil_twosite;

constexpr int kMaxOrtho = 8;
constexpr long long kSmallBytes = 4608;             // alpha, beta, the Ritz coefficients and two 16 x 16 matrices, behind block_sum's 128

// what a local solve reports and, on the gemm route, carries between its kernels (doubles)
enum {
    ST_STATUS = 0,   // 0 fine, 1 a Ritz value is not finite, 2 the start vector is zero or not finite
    ST_MATVECS = 1,
    ST_RES0 = 2,     // |H y - theta y| before the solve
    ST_THETA = 3,
    ST_SCALE = 4,
    ST_YNORM = 5,
    ST_DONE = 6,     // the stopping test passed
    ST_RESTARTS = 7,
    ST_READ = 8,     // what the host reads back
    ST_J = 8,        // gemm route: vectors built in this restart
    ST_HALT = 9,     // gemm route: breakdown in this restart
    ST_ALPHA = 16,
    ST_BETA = 32,
    ST_WORDS = 48
};
// the small LDS area, in doubles
enum { SM_ALPHA = 0, SM_BETA = 16, SM_COEF = 32, SM_OUT = 48, SM_T = 64, SM_Z = 64 + 256, SM_WORDS = 64 + 512 };
static_assert(SM_WORDS * 8 <= kSmallBytes, "the small area");

// LDS bytes of eigs_local:
//   128 + 4608 + e * (xl^2 dl + xr^2 dr + 4 dl dm + 4 dm dr + (krylov + 1 + n_ortho) * 4 xl xr + 2 * 4 xl xr max(dl, dm, dr)),
//   e = 8 (f64) / 16 (c64)
long long local_lds_bytes(bool cx, long long xl, long long xr, long long dl, long long dm, long long dr, long long krylov,
                          long long n_ortho) {
    const long long nv = 4 * xl * xr;
    return local_bytes(cx, kSmallBytes, frame_elems(2, xl, xr, dl, dm, dr), krylov + 1 + n_ortho, nv, nv * std::max({dl, dm, dr}));
}

struct EigArgs : FrameArgs {           // y: (xl, 2, 2, xr), the Ritz vector on return; stat: ST_WORDS doubles; shift 0
    const void* G;                     // n_ortho projected deflation states (TE), 4 xl xr each
    int krylov, restarts, n_ortho, which;
    double tol, scale;
    double sw;                         // s * weight
};

// The eigenpair of the m x m tridiagonal matrix (alpha, beta) at the wanted end, by ONE thread (tridiagonal_eig): the eigenvector
// goes to coef, out = {its value, the largest |eigenvalue|}.
__device__ inline void tridiagonal_ritz(int m, const double* alpha, const double* beta, int which, double* T, double* Z, double* coef,
                                        double* out) {
    tridiagonal_eig(m, alpha, beta, T, Z);
    int best = 0;
    double amax = 0.0;
    for (int i = 0; i < m; ++i) {
        const double v = T[i * 16 + i];
        if (which ? v > T[best * 16 + best] : v < T[best * 16 + best]) best = i;
        amax = fmax(amax, fabs(v));
        if (!isfinite(v)) amax = v - v;                                    // NaN: the caller reports it
    }
    for (int i = 0; i < m; ++i) coef[i] = Z[i * 16 + best];
    out[0] = T[best * 16 + best];
    out[1] = amax;
}

// The end of a restart: thread 0 diagonalises the projected matrix of the m vectors built (alpha, beta at sm), publishes the Ritz
// pair through sm behind a barrier, and all threads form the Ritz vector in w, normalise it and make it v_0.  Ends behind a
// barrier.  theta: the Ritz value at the wanted end, amax: the largest |Ritz value|.
template <class TE>
__device__ __forceinline__ void ritz_restart(int m, int nv, TE* V, TE* w, double* sm, int which, double* red, double& theta,
                                             double& amax) {
    if (threadIdx.x == 0) tridiagonal_ritz(m, sm + SM_ALPHA, sm + SM_BETA, which, sm + SM_T, sm + SM_Z, sm + SM_COEF, sm + SM_OUT);
    __syncthreads();
    theta = sm[SM_OUT], amax = sm[SM_OUT + 1];
    for (int t = threadIdx.x; t < nv; t += kThreads) {
        TE acc{};
        for (int i = 0; i < m; ++i) acc = add_t(acc, scale_t(V[(size_t)i * nv + t], sm[SM_COEF + i]));
        w[t] = acc;
    }
    const double nrm = wg_norm<TE>(w, nv, red);
    const double f = nrm > 0.0 ? 1.0 / nrm : 0.0;
    for (int t = threadIdx.x; t < nv; t += kThreads) V[t] = scale_t(w[t], f);
    __syncthreads();
}

// how the scale follows a restart's Ritz values: all of them without deflation states, the wanted end's alone with them
__device__ __forceinline__ double next_scale(double scale, double theta, double amax, int n_ortho) {
    return fmax(scale, n_ortho > 0 ? fabs(theta) : amax);
}

// One workgroup runs the whole restarted iteration for one bond.  Every loop around a barrier has uniform bounds: alpha, beta, the
// norms and the Ritz pair come out of block_sum or out of LDS behind a barrier, which hand every thread the same bits, so all
// threads take the same branches.  No spin, no atomics: at most krylov * restarts matvecs.
template <class TA, class TE>
__global__ __launch_bounds__(kThreads) void eigs_local(const EigArgs g) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double* red = reinterpret_cast<double*>(lds_raw);
    double* sm = reinterpret_cast<double*>(lds_raw + kRedBytes);
    const int nv = 4 * g.xl * g.xr;
    const auto [Ls, Rs, W0, W1, V] = stage_frame<TA, TE, 2>(g, lds_raw + kRedBytes + kSmallBytes);
    TE* wv = V + g.krylov * nv;
    TE* Gs = wv + nv;
    TE* X = Gs + g.n_ortho * nv;
    TE* Y = X + g.blk;
    const TE* G0 = static_cast<const TE*>(g.G);
    for (int t = threadIdx.x; t < g.n_ortho * nv; t += kThreads) Gs[t] = G0[t];
    __syncthreads();
    bool bad;
    const double ynorm = unit_start<TE>(V, V, nv, red, bad);
    double scale = g.scale, theta = 0.0, res0 = 0.0;
    int status = bad ? 2 : 0, matvecs = 0, done = 0, restarts = 0;
    for (int rs = 0; rs < g.restarts && status == 0 && !done; ++rs) {
        int m = 0;
        for (int j = 0; j < g.krylov; ++j) {
            __syncthreads();                                               // v_j is complete
            local_matvec<TE>(g, Ls, Rs, W0, W1, V + j * nv, X, Y);
            for (int t = threadIdx.x; t < nv; t += kThreads) wv[t] = Y[t];
            double alpha, beta;
            lanczos_step<TE>(j, nv, V, wv, Gs, g.n_ortho, g.sw, red, alpha, beta);
            ++matvecs;
            if (!isfinite(alpha) || !isfinite(beta)) {
                status = 1;
                break;
            }
            if (threadIdx.x == 0) sm[SM_ALPHA + j] = alpha, sm[SM_BETA + j] = beta;
            m = j + 1;
            if (j == 0) {
                theta = alpha;
                scale = fmax(scale, fabs(alpha));
                if (rs == 0) res0 = beta;
                if (beta <= g.tol * scale) {
                    done = 1;
                    break;
                }
            }
            if (beta <= kBreakdown * scale) break;
            if (j + 1 < g.krylov) next_vector<TE>(V + (j + 1) * nv, wv, nv, beta);
        }
        if (status != 0 || done) break;
        __syncthreads();                                                   // alpha, beta and the basis are complete
        double amax;
        ritz_restart<TE>(m, nv, V, wv, sm, g.which, red, theta, amax);
        ++restarts;
        if (!isfinite(theta)) status = 1;
        else scale = next_scale(scale, theta, amax, g.n_ortho);
    }
    __syncthreads();
    TE* yo = static_cast<TE*>(g.y);
    for (int t = threadIdx.x; t < nv; t += kThreads) yo[t] = V[t];
    if (threadIdx.x == 0) {
        g.stat[ST_STATUS] = status;
        g.stat[ST_MATVECS] = matvecs;
        g.stat[ST_RES0] = res0;
        g.stat[ST_THETA] = theta;
        g.stat[ST_SCALE] = scale;
        g.stat[ST_YNORM] = ynorm;
        g.stat[ST_DONE] = done;
        g.stat[ST_RESTARTS] = restarts;
    }
}

// ---- gemm route: the same steps on vectors in device memory, one workgroup each, the state in `st` (device)
// v_0 = y / |y|, the state of a fresh local solve
template <class TE>
__global__ __launch_bounds__(kThreads) void eigs_begin(const TE* __restrict__ y, TE* __restrict__ V, int nv, double scale,
                                                       double* __restrict__ st) {
    __shared__ double red[8];
    bool bad;
    const double ynorm = unit_start<TE>(y, V, nv, red, bad);
    for (int t = threadIdx.x; t < ST_WORDS; t += kThreads) st[t] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        st[ST_STATUS] = bad ? 2.0 : 0.0;
        st[ST_SCALE] = scale;
        st[ST_YNORM] = ynorm;
    }
}
// the Lanczos step of the vector this restart has reached, w = the matvec of v_j; a no-op once the solve or the restart is over
template <class TE>
__global__ __launch_bounds__(kThreads) void eigs_step(TE* __restrict__ V, TE* __restrict__ w, const TE* __restrict__ G, int nv,
                                                      int n_ortho, double sw, double tol, int krylov, double* __restrict__ st) {
    __shared__ double red[8];
    const double status = st[ST_STATUS], fin = st[ST_DONE], halt = st[ST_HALT], scale0 = st[ST_SCALE], first = st[ST_RESTARTS];
    const int j = (int)st[ST_J];
    if (status != 0.0 || fin != 0.0 || halt != 0.0 || j >= krylov) return;   // uniform: thread 0 writes st behind the barriers below
    double alpha, beta;
    lanczos_step<TE>(j, nv, V, w, G, n_ortho, sw, red, alpha, beta);
    const bool finite = isfinite(alpha) && isfinite(beta);
    double scale = scale0;
    bool done = false;
    if (finite && j == 0) {
        scale = fmax(scale, fabs(alpha));
        done = beta <= tol * scale;
    }
    const bool halted = !finite || done || beta <= kBreakdown * scale;
    if (!halted && j + 1 < krylov) next_vector<TE>(V + (size_t)(j + 1) * nv, w, nv, beta);
    if (threadIdx.x == 0) {
        st[ST_MATVECS] += 1.0;
        if (!finite) {
            st[ST_STATUS] = 1.0;
            return;
        }
        st[ST_ALPHA + j] = alpha, st[ST_BETA + j] = beta;
        st[ST_J] = j + 1;
        if (j == 0) {
            st[ST_THETA] = alpha;
            st[ST_SCALE] = scale;
            if (first == 0.0) st[ST_RES0] = beta;
            if (done) st[ST_DONE] = 1.0;
        }
        if (halted) st[ST_HALT] = 1.0;
    }
}
// the end of a restart; a no-op once the solve is over
template <class TE>
__global__ __launch_bounds__(kThreads) void eigs_ritz(TE* __restrict__ V, TE* __restrict__ w, int nv, int which, int n_ortho,
                                                      double* __restrict__ st) {
    __shared__ double red[8];
    __shared__ double sm[SM_WORDS];
    const double status = st[ST_STATUS], fin = st[ST_DONE], scale = st[ST_SCALE];
    const int m = (int)st[ST_J];
    if (status != 0.0 || fin != 0.0 || m < 1) return;
    if (threadIdx.x < m) sm[SM_ALPHA + threadIdx.x] = st[ST_ALPHA + threadIdx.x], sm[SM_BETA + threadIdx.x] = st[ST_BETA + threadIdx.x];
    __syncthreads();
    double theta, amax;
    ritz_restart<TE>(m, nv, V, w, sm, which, red, theta, amax);
    if (threadIdx.x == 0) {
        st[ST_RESTARTS] += 1.0;
        st[ST_J] = 0.0;
        st[ST_HALT] = 0.0;
        if (!isfinite(theta)) {
            st[ST_STATUS] = 1.0;
        } else {
            st[ST_THETA] = theta;
            st[ST_SCALE] = next_scale(scale, theta, amax, n_ortho);
        }
    }
}

struct EigSolver : Sweep {
    int which = 0, krylov = 8, restarts = 4;
    double weight = 0.0, tol = 0.0;
    void* stat = nullptr;
    double scale = 0.0, theta = 0.0, sweep_res = 0.0;

    EigSolver(qil_context* ctx_, qil_scratch& tmp_, const qil_mpo* A_, qil_mps* x_, int dt_) : Sweep(ctx_, tmp_, A_, x_, dt_) {}

    double sw() const { return (which == 0 ? 1.0 : -1.0) * weight; }

    int init() {
        QIL_TRY(tmp.alloc(ST_WORDS * sizeof(double), &stat));
        return init_envs();
    }

    // the g_i of bond k in one block (n_ortho x nv); null without deflation states
    int project_ortho(int64_t k, void** G) {
        *G = nullptr;
        if (phi.empty()) return QIL_OK;
        const int64_t nv = 4 * xd(k) * xd(k + 2);
        QIL_TRY(tmp.alloc(phi.size() * (size_t)nv * e, G));
        for (size_t i = 0; i < phi.size(); ++i) {
            void *T1 = nullptr, *T2 = nullptr;
            const size_t blk = (size_t)overlap_block_elems(i, k) * e;
            QIL_TRY(tmp.alloc(blk, &T1));
            QIL_TRY(tmp.alloc(blk, &T2));
            QIL_TRY(overlap_local(i, k, T1, T2, static_cast<char*>(*G) + i * (size_t)nv * e));
            tmp.free(T2);
            tmp.free(T1);
        }
        return QIL_OK;
    }

    int bond_local(int64_t k, void* y, const void* G, double* hst) {
        EigArgs g{frame(2, k, y, stat)};
        g.G = G, g.krylov = krylov, g.restarts = restarts, g.n_ortho = (int)phi.size(), g.which = which;
        g.sw = sw(), g.tol = tol, g.scale = scale;
        const bool cx = dt == QIL_C64;
        const size_t lds = (size_t)local_lds_bytes(cx, g.xl, g.xr, g.dl, g.dm, g.dr, krylov, g.n_ortho);
        QIL_REQUIRE((long long)lds <= kLdsBudget, QIL_EINVAL_ARG, "eigs: bond %lld does not fit the local route", (long long)k);
        return for_sweep_types(A->dtype == QIL_C64, cx, [&](auto a, auto t) {
            return launch_local<eigs_local<decltype(a), decltype(t)>>(g, lds, ST_READ, hst);
        });
    }

    int bond_gemm(int64_t k, void* y, const void* G, double* hst) {
        const Dims d = dims_of(2, k);
        const int64_t nv = 4 * d.xl * d.xr;
        QIL_REQUIRE(nv < (1LL << 31) / kMaxKrylov, QIL_EINVAL_ARG, "eigs: a two-site tensor of %lld elements", (long long)nv);
        Work w;
        QIL_TRY(work_alloc(2, k, nv * std::max({d.dl, d.dm, d.dr}), krylov, &w));
        const void *A0 = w.A0, *A1 = w.A1;
        void *V = w.V, *H = w.H;
        const int no = (int)phi.size();
        QIL_TRY(launch_wg([](auto t) { return &eigs_begin<decltype(t)>; }, y, V, (int)nv, scale, stat));
        auto step = [&](int j) -> int {
            QIL_TRY(gemm_matvec(k, A0, A1, static_cast<char*>(V) + (size_t)(j * nv) * e, w.T1, w.T2, H));
            return launch_wg([](auto t) { return &eigs_step<decltype(t)>; }, V, H, G, (int)nv, no, sw(), tol, krylov, stat);
        };
        // The one read-back of a restart follows its FIRST step, the stopping test: a bond that has converged (every bond of a
        // sweep's last pass) then costs one matvec and one step, not krylov of each.  What the rest of a restart leaves in the
        // flags is seen by the next restart's read, or by the last one below.
        bool over = false;
        for (int rs = 0; rs < restarts && !over; ++rs) {
            QIL_TRY(step(0));
            QIL_TRY(qil_read_back(ctx, hst, stat, ST_READ * sizeof(double)));
            over = hst[ST_STATUS] != 0.0 || hst[ST_DONE] != 0.0;
            if (over) break;
            for (int j = 1; j < krylov; ++j) QIL_TRY(step(j));
            QIL_TRY(launch_wg([](auto t) { return &eigs_ritz<decltype(t)>; }, V, H, (int)nv, which, no, stat));
        }
        if (!over) QIL_TRY(qil_read_back(ctx, hst, stat, ST_READ * sizeof(double)));
        QIL_TRY(qil_dev_copy(ctx, y, V, (size_t)nv * e));
        work_free(w);
        return QIL_OK;
    }

    // one local step at bond k
    int step(int64_t k, bool to_right) {
        void *y = nullptr, *G = nullptr;
        QIL_TRY(two_site(k, &y));
        QIL_TRY(project_ortho(k, &G));
        int fits = 0;
        QIL_TRY(qil_mps_eigs_local_fits(dt == QIL_C64, xd(k), xd(k + 2), ad(k), ad(k + 1), ad(k + 2), krylov, (int)phi.size(), &fits));
        double st[ST_READ] = {};
        if (fits) {
            QIL_TRY(bond_local(k, y, G, st));
            ++n_local;
        } else {
            QIL_TRY(bond_gemm(k, y, G, st));
            ++n_gemm;
        }
        if (G) tmp.free(G);
        matvecs += (long long)st[ST_MATVECS];
        QIL_REQUIRE(st[ST_STATUS] != 2.0, QIL_EDOMAIN, "eigs: the start vector is zero or not finite (bond %lld)", (long long)(k + 1));
        QIL_REQUIRE(st[ST_STATUS] == 0.0 && std::isfinite(st[ST_THETA]) && std::isfinite(st[ST_SCALE]) && std::isfinite(st[ST_RES0]),
                    QIL_EDOMAIN, "eigs: a Ritz value at bond %lld is not finite", (long long)(k + 1));
        scale = st[ST_SCALE], theta = st[ST_THETA];
        const double rel = scale > 0.0 ? st[ST_RES0] / scale : (st[ST_RES0] > 0.0 ? INFINITY : 0.0);
        sweep_res = std::max(sweep_res, rel);
        return split(k, to_right, y, true);
    }

    int sweep() {
        sweep_res = 0.0;
        return Sweep::sweep([&](int64_t k, bool to_right) { return step(k, to_right); });
    }
};

}  // namespace

// The decision qil_mps_eigs switches on for every bond: local_route_fits with the LDS eigs_local needs for these dimensions
// (local_lds_bytes above).
extern "C" int qil_mps_eigs_local_fits(int complex_, int64_t xl, int64_t xr, int64_t dl, int64_t dm, int64_t dr, int krylov,
                                       int n_ortho, int* fits) {
    QIL_REQUIRE(fits, QIL_EINVAL_ARG, "eigs_local_fits: null argument");
    QIL_REQUIRE(xl >= 1 && xr >= 1 && dl >= 1 && dm >= 1 && dr >= 1, QIL_EINVAL_ARG, "eigs_local_fits: dimensions must be positive");
    QIL_REQUIRE(krylov >= 1 && n_ortho >= 0, QIL_EINVAL_ARG, "eigs_local_fits: krylov must be >= 1 and n_ortho >= 0 (got %d, %d)",
                krylov, n_ortho);
    const bool over = std::max({xl, xr, dl, dm, dr}) > kKrylovDimCap || krylov > kMaxKrylov || n_ortho > kMaxOrtho;
    const long long bytes = over ? 0 : local_lds_bytes(complex_ != 0, xl, xr, dl, dm, dr, krylov, n_ortho);
    *fits = local_route_fits(getenv("QIL_EIGS_ROUTE"), over, bytes, over ? 0 : local_matvec_macs(xl, xr, dl, dm, dr));
    return QIL_OK;
}

extern "C" int qil_mps_eigs(const qil_mpo* A, int which, const qil_mps* x0, const qil_mps* const* ortho, int n_ortho, double weight,
                            int64_t maxdim, double cutoff, double tol, int max_sweeps, int krylov, int restarts, qil_mps** out,
                            double* theta, double* info) {
    QIL_REQUIRE(A && x0 && out && theta, QIL_EINVAL_ARG, "eigs: null argument");
    QIL_REQUIRE(which == 0 || which == 1, QIL_EINVAL_ARG, "eigs: which must be 0 (smallest) or 1 (largest), got %d", which);
    QIL_REQUIRE(n_ortho >= 0 && n_ortho <= kMaxOrtho, QIL_EINVAL_ARG, "eigs: n_ortho must be in 0 .. %d, got %d", kMaxOrtho, n_ortho);
    QIL_REQUIRE(n_ortho == 0 || ortho, QIL_EINVAL_ARG, "eigs: null ortho with n_ortho = %d", n_ortho);
    for (int i = 0; i < n_ortho; ++i) QIL_REQUIRE(ortho[i], QIL_EINVAL_ARG, "eigs: ortho[%d] is null", i);
    QIL_REQUIRE(krylov >= 2 && krylov <= kMaxKrylov, QIL_EINVAL_ARG, "eigs: krylov must be in 2 .. %d, got %d", kMaxKrylov, krylov);
    QIL_REQUIRE(restarts >= 1, QIL_EINVAL_ARG, "eigs: restarts must be >= 1, got %d", restarts);
    QIL_REQUIRE(maxdim >= 1 && max_sweeps >= 1, QIL_EINVAL_ARG, "eigs: maxdim and max_sweeps must be >= 1 (got %lld, %d)",
                (long long)maxdim, max_sweeps);
    QIL_REQUIRE(std::isfinite(weight) && std::isfinite(cutoff) && std::isfinite(tol), QIL_EINVAL_ARG,
                "eigs: weight, cutoff and tol must be finite");
    QIL_REQUIRE(weight >= 0.0 && cutoff >= 0.0 && tol > 0.0, QIL_EINVAL_ARG,
                "eigs: weight and cutoff must be >= 0 and tol > 0 (got %g, %g, %g)", weight, cutoff, tol);
    const int64_t n = x0->n();
    QIL_REQUIRE(n != 1, QIL_EINVAL_LENGTH, "eigs: the two-site step needs a bond, the chain has one tensor");
    QIL_TRY(qil_check_apply_operands(A, x0));
    for (int i = 0; i < n_ortho; ++i) QIL_TRY(qil_check_overlap_pair(ortho[i], x0));
    QIL_REQUIRE(n >= 2, QIL_EINVAL_LENGTH, "eigs: the two-site step needs a bond, the chain has %lld tensor(s)", (long long)n);
    qil_context* ctx = x0->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    QIL_REQUIRE(x0->amplitude != 0.0 && std::isfinite(x0->amplitude), QIL_EDOMAIN, "eigs: x0 is zero or not finite (amplitude %g)",
                x0->amplitude);
    int dt = (A->dtype == QIL_C64 || x0->dtype == QIL_C64) ? QIL_C64 : QIL_F64;
    for (int i = 0; i < n_ortho; ++i)
        if (ortho[i]->dtype == QIL_C64) dt = QIL_C64;

    qil_mps* xh = nullptr;
    QIL_TRY(start_chain(ctx, x0, dt, 1.0, &xh));
    qil_result_guard<qil_mps> x_own(xh);
    QIL_TRY(start_gauge(xh, maxdim));

    qil_scratch tmp(ctx);
    EigSolver sv(ctx, tmp, A, xh, dt);
    for (int i = 0; i < n_ortho; ++i) sv.phi.push_back(ortho[i]);
    sv.which = which, sv.krylov = krylov, sv.restarts = restarts, sv.weight = weight, sv.tol = tol;
    sv.cutoff = cutoff, sv.maxdim = maxdim;
    QIL_TRY(sv.init());
    int sweeps = 0, converged = 0;
    QIL_TRY(sweep_until([&] { return sv.sweep(); }, sv.sweep_res, tol, max_sweeps, &sweeps, &converged));
    if (info) sv.info_head(info, sweeps, converged, sv.sweep_res), info[7] = sv.scale;
    *theta = sv.theta;
    *out = x_own.release();
    return QIL_OK;
}
