// Time evolution (qil_mps_evolve): y = exp(steps tau A) x0 for a Hermitian operator in MPS form by two-site TDVP, the
// projector-splitting integrator.  The sweep, the environments, the matvecs, the split and the frame of both routes are shared with
// the linear solver and the eigen-solver (qil_twosite.h, qil_twosite.hip).
// One step is a sweep left to right and a sweep right to left; at bond k the two-site tensor goes
// through exp(+tau/2 H2), H2 = L_A A_k A_{k+1} R_A, and is split; unless the bond is the last of its half sweep the centre tensor
// that moves on goes through exp(-tau/2 H1), H1 = L_A A_j R_A at the tensor the centre now sits on: the two-site step has advanced
// that tensor in time as part of bond k, and the next bond will advance it again, so it is taken back once in between.
//
// Every local exponential is a Lanczos exponential from the unit start v / |v|: a basis with full reorthogonalisation (lanczos_step,
// no deflation states), after every vector from the second on the tridiagonal T_m diagonalised by ONE thread (tridiagonal_eig),
// c = exp(delta T_m) e_1 and est = beta_m |c_m| / |c|.  A pass ends when est <= tol, when beta_m <= 1e-14 scale (the space is
// invariant: exact) or at m = krylov; there, with est > tol and passes left, delta is halved (the small exponential alone, at most 30
// times) until est <= tol, the vector advances by that part and the next pass starts from it with the rest.  The last permitted pass
// takes all that remains.  The result is V c, normalised; |v| and the growth |V c| go to the host as logarithms.
//
//   local route   ONE launch, one workgroup (evolve_local<.., sites>): both environments, the operator tensor(s), the Krylov basis,
//                 the work vector, two ping-pong blocks and the small area in LDS, every pass in it
//   gemm route    the matvec as four (two-site) or three (one-site) f64-MFMA products, the basis in device memory, the vector steps
//                 in small one-workgroup kernels (evolve_begin, evolve_step) with the state in device memory; the launches of a
//                 pass are issued unconditionally and are no-ops behind the stop; one read-back per pass
//
// Both routes run the same device functions (lanczos_step, pass_decide, pass_finish).  Every temporary belongs to the call's
// qil_scratch; the working copy of x is the result handle.
#include "qil_twosite.h"

namespace {

using namespace qil_twosite;

constexpr int kMaxHalvings = 30;
constexpr long long kSmallBytes = 4736;             // alpha, beta, c (re, im), the decision and two 16 x 16 matrices

enum {
    ST_STATUS = 0,   // 0 fine, 1 a Lanczos coefficient or the growth is not finite, 2 the start is zero or not finite
    ST_MATVECS = 1,
    ST_LOGNORM = 2,  // log(|v| g)
    ST_EST = 3,      // the worst accepted estimate
    ST_CONV = 4,     // every accepted part met tol
    ST_PASSES = 5,
    ST_SPREAD = 6,   // the largest theta_max - theta_min of the passes
    ST_FIN = 7,      // nothing of delta remains
    ST_READ = 8,     // what the host reads back
    ST_J = 8,        // gemm route: vectors built in this pass
    ST_DRE = 9,      // gemm route: what remains of delta
    ST_DIM = 10,
    ST_SCALE = 11,
    ST_ALPHA = 16,
    ST_BETA = 32,
    ST_WORDS = 48
};
enum { SM_ALPHA = 0, SM_BETA = 16, SM_CRE = 32, SM_CIM = 48, SM_OUT = 64, SM_T = 80, SM_Z = 80 + 256, SM_WORDS = 80 + 512 };
enum { O_END = 0, O_EST, O_PRE, O_PIM, O_ALL, O_CONV, O_SPREAD, O_BAD };
static_assert(SM_WORDS * 8 <= kSmallBytes, "the small area");

// LDS bytes of evolve_local, e = 8 (f64) / 16 (c64):
//   sites = 2: 128 + 4736 + e * (xl^2 dl + xr^2 dr + 4 dl dm + 4 dm dr + (krylov + 1) * 4 xl xr + 2 * 4 xl xr max(dl, dm, dr))
//   sites = 1: 128 + 4736 + e * (xl^2 dl + xr^2 dr + 4 dl dr + (krylov + 1) * 2 xl xr + 2 * 2 xl xr max(dl, dr))
long long local_lds_bytes(bool cx, int sites, long long xl, long long xr, long long dl, long long dm, long long dr, long long krylov) {
    const long long nv = (sites == 2 ? 4 : 2) * xl * xr;
    return local_bytes(cx, kSmallBytes, frame_elems(sites, xl, xr, dl, dm, dr), krylov + 1, nv,
                       nv * (sites == 2 ? std::max({dl, dm, dr}) : std::max(dl, dr)));
}

struct EvoArgs : FrameArgs {           // y: the unit result on return; stat: ST_WORDS doubles; shift 0
    int krylov, substeps;
    double dre, dim, tol;
};

// c = exp((dre + i dim) T_m) e_1 from the eigenpairs tridiagonal_eig left (the diagonal of T, the columns of Z); returns
// est = beta_m |c_m| / |c|.  ONE thread.
__device__ inline double krylov_exp(int m, const double* T, const double* Z, double dre, double dim, double beta_m, double* cre,
                                    double* cim) {
    for (int k = 0; k < m; ++k) cre[k] = 0.0, cim[k] = 0.0;
    for (int i = 0; i < m; ++i) {
        const double th = T[i * 16 + i], mag = exp(dre * th) * Z[i];
        const double zr = mag * cos(dim * th), zi = mag * sin(dim * th);
        for (int k = 0; k < m; ++k) cre[k] = fma(Z[k * 16 + i], zr, cre[k]), cim[k] = fma(Z[k * 16 + i], zi, cim[k]);
    }
    double n2 = 0.0;
    for (int k = 0; k < m; ++k) n2 += cre[k] * cre[k] + cim[k] * cim[k];
    return beta_m * sqrt(cre[m - 1] * cre[m - 1] + cim[m - 1] * cim[m - 1]) / sqrt(n2);
}

// The stopping rule after the m-th vector of a pass, by ONE thread: alpha, beta at sm; (dre, dim) is what remains of delta.  Leaves
// at sm + SM_OUT whether the pass ends, the accepted estimate, the part of delta taken, whether that is all of it and whether it
// met tol, and with an ended pass the coefficients c at SM_CRE, SM_CIM.
__device__ inline void pass_decide(int m, int krylov, bool last_pass, double tol, double scale, double dre, double dim, double* sm) {
    double* o = sm + SM_OUT;
    const double beta = sm[SM_BETA + m - 1];
    const bool invariant = beta <= kBreakdown * scale;
    o[O_END] = 0.0, o[O_EST] = 0.0, o[O_PRE] = dre, o[O_PIM] = dim, o[O_ALL] = 1.0, o[O_CONV] = 1.0, o[O_SPREAD] = 0.0, o[O_BAD] = 0.0;
    if (m == 1 && !invariant) return;
    tridiagonal_eig(m, sm + SM_ALPHA, sm + SM_BETA, sm + SM_T, sm + SM_Z);
    double lo = sm[SM_T], hi = sm[SM_T];
    for (int i = 0; i < m; ++i) {
        const double th = sm[SM_T + i * 16 + i];
        lo = fmin(lo, th), hi = fmax(hi, th);
        if (!isfinite(th)) o[O_BAD] = 1.0;
    }
    o[O_SPREAD] = hi - lo;
    double est = krylov_exp(m, sm + SM_T, sm + SM_Z, dre, dim, beta, sm + SM_CRE, sm + SM_CIM);
    if (!isfinite(est)) o[O_BAD] = 1.0;
    if (invariant) est = 0.0;
    if (est <= tol) {
        o[O_END] = 1.0, o[O_EST] = est;
        return;
    }
    if (m < krylov) return;
    o[O_END] = 1.0;
    if (last_pass) {                                                       // takes all that remains, as it is
        o[O_EST] = est, o[O_CONV] = 0.0;
        return;
    }
    double f = 1.0;
    for (int h = 0; h < kMaxHalvings && est > tol; ++h) {
        f *= 0.5;
        est = krylov_exp(m, sm + SM_T, sm + SM_Z, dre * f, dim * f, beta, sm + SM_CRE, sm + SM_CIM);
    }
    o[O_EST] = est, o[O_PRE] = dre * f, o[O_PIM] = dim * f, o[O_ALL] = 0.0, o[O_CONV] = est <= tol ? 1.0 : 0.0;
}

// The end of a pass, all threads: w = V c, the growth g = |w|, v_0 = w / g.  Every thread works on its own elements.
template <class TE>
__device__ __forceinline__ double pass_finish(int m, int nv, TE* V, TE* w, const double* sm, double* red) {
    for (int t = threadIdx.x; t < nv; t += kThreads) {
        TE acc{};
        for (int i = 0; i < m; ++i) acc = cmul_add(acc, make_elem(sm[SM_CRE + i], sm[SM_CIM + i], (TE*)nullptr), V[(size_t)i * nv + t]);
        w[t] = acc;
    }
    const double g = wg_norm<TE>(w, nv, red);
    const double f = g > 0.0 && isfinite(g) ? 1.0 / g : 0.0;
    for (int t = threadIdx.x; t < nv; t += kThreads) V[t] = scale_t(w[t], f);
    return g;
}

// One workgroup runs every pass of one local exponential.  Every loop around a barrier has uniform bounds: alpha, beta and the
// norms come out of block_sum, the decision out of LDS behind a barrier, so all threads take the same branches.  No spin, no
// atomics: at most krylov * substeps matvecs.
template <class TA, class TE, int SITES>
__global__ __launch_bounds__(kThreads) void evolve_local(const EvoArgs g) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double* red = reinterpret_cast<double*>(lds_raw);
    double* sm = reinterpret_cast<double*>(lds_raw + kRedBytes);
    const int nv = (SITES == 2 ? 4 : 2) * g.xl * g.xr;
    const auto [Ls, Rs, W0, W1, V] = stage_frame<TA, TE, SITES>(g, lds_raw + kRedBytes + kSmallBytes);
    TE* wv = V + g.krylov * nv;
    TE* X = wv + nv;
    TE* Y = X + g.blk;
    __syncthreads();
    bool bad;
    const double ynorm = unit_start<TE>(V, V, nv, red, bad);
    double dre = g.dre, dim = g.dim, scale = 0.0, lognorm = bad ? 0.0 : log(ynorm), worst = 0.0, spread = 0.0;
    int status = bad ? 2 : 0, matvecs = 0, conv = 1, passes = 0, fin = 0;
    for (int pass = 0; pass < g.substeps && status == 0 && !fin; ++pass) {
        ++passes;
        for (int j = 0; j < g.krylov; ++j) {
            __syncthreads();                                               // v_j is complete
            const TE* hv;
            if constexpr (SITES == 2) {
                local_matvec<TE>(g, Ls, Rs, W0, W1, V + j * nv, X, Y);
                hv = Y;
            } else {
                local_matvec1<TE>(g, Ls, Rs, W0, V + j * nv, X, Y);
                hv = X;
            }
            for (int t = threadIdx.x; t < nv; t += kThreads) wv[t] = hv[t];
            double alpha, beta;
            lanczos_step<TE>(j, nv, V, wv, static_cast<const TE*>(nullptr), 0, 0.0, red, alpha, beta);
            ++matvecs;
            if (!isfinite(alpha) || !isfinite(beta)) {
                status = 1;
                break;
            }
            scale = fmax(scale, fmax(fabs(alpha), beta));
            if (threadIdx.x == 0) {
                sm[SM_ALPHA + j] = alpha, sm[SM_BETA + j] = beta;
                pass_decide(j + 1, g.krylov, pass + 1 == g.substeps, g.tol, scale, dre, dim, sm);
            }
            __syncthreads();                                               // the decision is complete
            const double* o = sm + SM_OUT;
            if (o[O_BAD] != 0.0) {
                status = 1;
                break;
            }
            if (o[O_END] != 0.0) {
                const double est = o[O_EST], pre = o[O_PRE], pim = o[O_PIM], sp = o[O_SPREAD];
                const bool all = o[O_ALL] != 0.0, cv = o[O_CONV] != 0.0;
                const double gf = pass_finish<TE>(j + 1, nv, V, wv, sm, red);
                if (!(gf > 0.0) || !isfinite(gf)) {
                    status = 1;
                    break;
                }
                lognorm += log(gf), worst = fmax(worst, est), spread = fmax(spread, sp);
                if (!cv) conv = 0;
                if (all) fin = 1;
                else dre -= pre, dim -= pim;
                break;
            }
            next_vector<TE>(V + (j + 1) * nv, wv, nv, beta);
        }
    }
    __syncthreads();
    TE* yo = static_cast<TE*>(g.y);
    for (int t = threadIdx.x; t < nv; t += kThreads) yo[t] = V[t];
    if (threadIdx.x == 0) {
        g.stat[ST_STATUS] = status;
        g.stat[ST_MATVECS] = matvecs;
        g.stat[ST_LOGNORM] = lognorm;
        g.stat[ST_EST] = worst;
        g.stat[ST_CONV] = conv;
        g.stat[ST_PASSES] = passes;
        g.stat[ST_SPREAD] = spread;
        g.stat[ST_FIN] = fin;
    }
}

// ---- gemm route: the same steps on vectors in device memory, one workgroup each, the state in `st` (device)
template <class TE>
__global__ __launch_bounds__(kThreads) void evolve_begin(const TE* __restrict__ y, TE* __restrict__ V, int nv, double dre, double dim,
                                                         double* __restrict__ st) {
    __shared__ double red[8];
    bool bad;
    const double ynorm = unit_start<TE>(y, V, nv, red, bad);
    for (int t = threadIdx.x; t < ST_WORDS; t += kThreads) st[t] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        st[ST_STATUS] = bad ? 2.0 : 0.0;
        st[ST_LOGNORM] = bad ? 0.0 : log(ynorm);
        st[ST_CONV] = 1.0;
        st[ST_DRE] = dre, st[ST_DIM] = dim;
    }
}
// the Lanczos step of the vector this pass has reached, w = the matvec of v_j, with the stopping rule and, where the pass ends, its
// end; a no-op once the exponential is over
template <class TE>
__global__ __launch_bounds__(kThreads) void evolve_step(TE* __restrict__ V, TE* __restrict__ w, int nv, double tol, int krylov,
                                                        int last_pass, double* __restrict__ st) {
    __shared__ double red[8];
    __shared__ double sm[SM_WORDS];
    const double status = st[ST_STATUS], fin = st[ST_FIN], scale0 = st[ST_SCALE], dre = st[ST_DRE], dim = st[ST_DIM];
    const int j = (int)st[ST_J];
    if (status != 0.0 || fin != 0.0 || j >= krylov) return;               // uniform: thread 0 writes st behind the barriers below
    if (threadIdx.x < j) sm[SM_ALPHA + threadIdx.x] = st[ST_ALPHA + threadIdx.x], sm[SM_BETA + threadIdx.x] = st[ST_BETA + threadIdx.x];
    double alpha, beta;
    lanczos_step<TE>(j, nv, V, w, static_cast<const TE*>(nullptr), 0, 0.0, red, alpha, beta);
    if (!isfinite(alpha) || !isfinite(beta)) {
        if (threadIdx.x == 0) st[ST_MATVECS] += 1.0, st[ST_STATUS] = 1.0;
        return;
    }
    const double scale = fmax(scale0, fmax(fabs(alpha), beta));
    if (threadIdx.x == 0) {
        sm[SM_ALPHA + j] = alpha, sm[SM_BETA + j] = beta;
        pass_decide(j + 1, krylov, last_pass != 0, tol, scale, dre, dim, sm);
    }
    __syncthreads();
    const double* o = sm + SM_OUT;
    const bool bad = o[O_BAD] != 0.0, ended = o[O_END] != 0.0, all = o[O_ALL] != 0.0;
    double gf = 1.0;
    if (!bad && ended) {
        gf = pass_finish<TE>(j + 1, nv, V, w, sm, red);
    } else if (!bad && j + 1 < krylov) {
        next_vector<TE>(V + (size_t)(j + 1) * nv, w, nv, beta);
    }
    if (threadIdx.x == 0) {
        st[ST_MATVECS] += 1.0;
        st[ST_SCALE] = scale;
        if (bad || !(gf > 0.0) || !isfinite(gf)) {
            st[ST_STATUS] = 1.0;
            return;
        }
        st[ST_ALPHA + j] = alpha, st[ST_BETA + j] = beta;
        if (j == 0) st[ST_PASSES] += 1.0;
        if (!ended) {
            st[ST_J] = j + 1;
            return;
        }
        st[ST_J] = 0.0;
        st[ST_LOGNORM] += log(gf);
        st[ST_EST] = fmax(st[ST_EST], o[O_EST]);
        st[ST_SPREAD] = fmax(st[ST_SPREAD], o[O_SPREAD]);
        if (o[O_CONV] == 0.0) st[ST_CONV] = 0.0;
        if (all) st[ST_FIN] = 1.0;
        else st[ST_DRE] = dre - o[O_PRE], st[ST_DIM] = dim - o[O_PIM];
    }
}

struct Evolver : Sweep {
    int krylov = 8, substeps = 4;
    double tol = 0.0, tau_re = 0.0, tau_im = 0.0;
    void* stat = nullptr;
    double log_sum = 0.0, worst = 0.0, growth = 0.0;
    long long extra_passes = 0;
    int converged = 1;

    Evolver(qil_context* ctx_, qil_scratch& tmp_, const qil_mpo* A_, qil_mps* x_, int dt_) : Sweep(ctx_, tmp_, A_, x_, dt_) {}

    int init() {
        QIL_TRY(tmp.alloc(ST_WORDS * sizeof(double), &stat));
        return init_envs();
    }

    template <int SITES>
    int exp_local(int64_t j, void* y, double dre, double dim, double* hst) {
        EvoArgs g{frame(SITES, j, y, stat)};
        g.krylov = krylov, g.substeps = substeps, g.dre = dre, g.dim = dim, g.tol = tol;
        const bool cx = dt == QIL_C64;
        const size_t lds = (size_t)local_lds_bytes(cx, SITES, g.xl, g.xr, g.dl, g.dm, g.dr, krylov);
        QIL_REQUIRE((long long)lds <= kLdsBudget, QIL_EINVAL_ARG, "evolve: tensor %lld does not fit the local route", (long long)j);
        return for_sweep_types(A->dtype == QIL_C64, cx, [&](auto a, auto t) {
            return launch_local<evolve_local<decltype(a), decltype(t), SITES>>(g, lds, ST_READ, hst);
        });
    }

    template <int SITES>
    int exp_gemm(int64_t j, void* y, double dre, double dim, double* hst) {
        const Dims d = dims_of(SITES, j);
        const int64_t nv = (SITES == 2 ? 4 : 2) * d.xl * d.xr;
        QIL_REQUIRE(nv < (1LL << 31) / kMaxKrylov, QIL_EINVAL_ARG, "evolve: a local tensor of %lld elements", (long long)nv);
        Work w;
        QIL_TRY(work_alloc(SITES, j, nv * std::max({d.dl, d.dm, d.dr}), krylov, &w));
        const void *A0 = w.A0, *A1 = w.A1;
        void *V = w.V, *H = w.H;
        QIL_TRY(launch_wg([](auto t) { return &evolve_begin<decltype(t)>; }, y, V, (int)nv, dre, dim, stat));
        // every launch of a pass is issued; behind the stop they return at once.  One read-back per pass.
        for (int pass = 0; pass < substeps; ++pass) {
            for (int i = 0; i < krylov; ++i) {
                const void* vi = static_cast<char*>(V) + (size_t)(i * nv) * e;
                if (SITES == 2) QIL_TRY(gemm_matvec(j, A0, A1, vi, w.T1, w.T2, H));
                else QIL_TRY(gemm_matvec1(j, A0, vi, w.T1, w.T2, H));
                QIL_TRY(launch_wg([](auto t) { return &evolve_step<decltype(t)>; }, V, H, (int)nv, tol, krylov,
                                  pass + 1 == substeps ? 1 : 0, stat));
            }
            QIL_TRY(qil_read_back(ctx, hst, stat, ST_READ * sizeof(double)));
            if (hst[ST_STATUS] != 0.0 || hst[ST_FIN] != 0.0) break;
        }
        QIL_TRY(qil_dev_copy(ctx, y, V, (size_t)nv * e));
        work_free(w);
        return QIL_OK;
    }

    // y <- the unit vector along exp((dre + i dim) H) y, H the local operator of bond j (sites 2) or of tensor j (sites 1)
    template <int SITES>
    int local_exp(int64_t j, void* y, double dre, double dim) {
        const Dims d = dims_of(SITES, j);
        int fits = 0;
        QIL_TRY(qil_mps_evolve_local_fits(dt == QIL_C64, SITES, d.xl, d.xr, d.dl, d.dm, d.dr, krylov, &fits));
        double st[ST_READ] = {};
        if (fits) {
            QIL_TRY(exp_local<SITES>(j, y, dre, dim, st));
            ++n_local;
        } else {
            QIL_TRY(exp_gemm<SITES>(j, y, dre, dim, st));
            ++n_gemm;
        }
        matvecs += (long long)st[ST_MATVECS];
        const long long bond = SITES == 2 ? j + 1 : j;
        QIL_REQUIRE(st[ST_STATUS] != 2.0, QIL_EDOMAIN, "evolve: the start is zero or not finite (bond %lld)", bond);
        QIL_REQUIRE(st[ST_STATUS] == 0.0 && std::isfinite(st[ST_LOGNORM]) && std::isfinite(st[ST_EST]), QIL_EDOMAIN,
                    "evolve: a Lanczos coefficient at bond %lld is not finite", bond);
        log_sum += st[ST_LOGNORM];
        worst = std::max(worst, st[ST_EST]);
        if (st[ST_CONV] == 0.0 || st[ST_FIN] == 0.0) converged = 0;
        extra_passes += std::max(0LL, (long long)st[ST_PASSES] - 1);
        if (SITES == 1) growth = std::max(growth, 0.5 * std::fabs(tau_re) * st[ST_SPREAD]);
        return QIL_OK;
    }

    int bond(int64_t k, bool to_right) {
        void* y = nullptr;
        QIL_TRY(two_site(k, &y));
        QIL_TRY(local_exp<2>(k, y, 0.5 * tau_re, 0.5 * tau_im));
        QIL_TRY(split(k, to_right, y, true));
        QIL_REQUIRE(kept > 0.0 && std::isfinite(kept), QIL_EDOMAIN, "evolve: the split at bond %lld kept nothing", (long long)(k + 1));
        log_sum += std::log(kept);
        return QIL_OK;
    }

    // one step: a sweep left to right, then right to left, the centre taken back by -tau/2 between bonds
    int step() {
        for (int64_t k = 0; k + 1 < n; ++k) {
            QIL_TRY(bond(k, true));
            if (k + 2 < n) {
                QIL_TRY(extend(k, false));
                QIL_TRY(local_exp<1>(k + 1, x->site[(size_t)k + 1], -0.5 * tau_re, -0.5 * tau_im));
            }
        }
        for (int64_t k = n - 2; k >= 0; --k) {
            QIL_TRY(bond(k, false));
            if (k >= 1) {
                QIL_TRY(extend(k + 1, true));
                QIL_TRY(local_exp<1>(k, x->site[(size_t)k], -0.5 * tau_re, -0.5 * tau_im));
            }
        }
        return QIL_OK;
    }
};

}  // namespace

// The decision qil_mps_evolve switches on for every local exponential: local_route_fits with the LDS evolve_local needs for these
// dimensions (local_lds_bytes above) and the multiply-adds of the two-site or the one-site matvec.
extern "C" int qil_mps_evolve_local_fits(int complex_, int sites, int64_t xl, int64_t xr, int64_t dl, int64_t dm, int64_t dr,
                                         int krylov, int* fits) {
    QIL_REQUIRE(fits, QIL_EINVAL_ARG, "evolve_local_fits: null argument");
    QIL_REQUIRE(sites == 1 || sites == 2, QIL_EINVAL_ARG, "evolve_local_fits: sites must be 1 or 2, got %d", sites);
    if (sites == 1) dm = 1;
    QIL_REQUIRE(xl >= 1 && xr >= 1 && dl >= 1 && dm >= 1 && dr >= 1, QIL_EINVAL_ARG,
                "evolve_local_fits: dimensions must be positive");
    QIL_REQUIRE(krylov >= 1, QIL_EINVAL_ARG, "evolve_local_fits: krylov must be >= 1 (got %d)", krylov);
    const bool over = std::max({xl, xr, dl, dm, dr}) > kKrylovDimCap || krylov > kMaxKrylov;
    const long long bytes = over ? 0 : local_lds_bytes(complex_ != 0, sites, xl, xr, dl, dm, dr, krylov);
    const long long macs = over ? 0 : (sites == 2 ? local_matvec_macs(xl, xr, dl, dm, dr) : local_matvec1_macs(xl, xr, dl, dr));
    *fits = local_route_fits(getenv("QIL_EVOLVE_ROUTE"), over, bytes, macs);
    return QIL_OK;
}

extern "C" int qil_mps_evolve(const qil_mpo* A, const qil_mps* x0, double tau_re, double tau_im, int steps, int64_t maxdim,
                              double cutoff, double tol, int krylov, int substeps, qil_mps** out, double* info) {
    QIL_REQUIRE(A && x0 && out, QIL_EINVAL_ARG, "evolve: null argument");
    QIL_REQUIRE(steps >= 1 && maxdim >= 1 && substeps >= 1, QIL_EINVAL_ARG, "evolve: steps, maxdim and substeps must be >= 1 (got %d, %lld, %d)",
                steps, (long long)maxdim, substeps);
    QIL_REQUIRE(krylov >= 2 && krylov <= kMaxKrylov, QIL_EINVAL_ARG, "evolve: krylov must be in 2 .. %d, got %d", kMaxKrylov, krylov);
    QIL_REQUIRE(std::isfinite(tau_re) && std::isfinite(tau_im) && std::isfinite(cutoff) && std::isfinite(tol), QIL_EINVAL_ARG,
                "evolve: tau, cutoff and tol must be finite");
    QIL_REQUIRE(cutoff >= 0.0 && tol > 0.0, QIL_EINVAL_ARG, "evolve: cutoff must be >= 0 and tol > 0 (got %g, %g)", cutoff, tol);
    QIL_REQUIRE(tau_re != 0.0 || tau_im != 0.0, QIL_EINVAL_ARG, "evolve: tau must not be zero");
    QIL_TRY(qil_check_apply_operands(A, x0));
    const int64_t n = x0->n();
    QIL_REQUIRE(n >= 2, QIL_EINVAL_LENGTH, "evolve: the two-site step needs a bond, the chain has %lld tensor(s)", (long long)n);
    qil_context* ctx = x0->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    QIL_REQUIRE(x0->amplitude != 0.0 && std::isfinite(x0->amplitude), QIL_EDOMAIN, "evolve: x0 is zero or not finite (amplitude %g)",
                x0->amplitude);
    const int dt = (A->dtype == QIL_C64 || x0->dtype == QIL_C64 || tau_im != 0.0) ? QIL_C64 : QIL_F64;

    qil_mps* xh = nullptr;
    QIL_TRY(start_chain(ctx, x0, dt, 1.0, &xh));
    qil_result_guard<qil_mps> x_own(xh);
    QIL_TRY(start_gauge(xh, maxdim));

    qil_scratch tmp(ctx);
    Evolver ev(ctx, tmp, A, xh, dt);
    ev.krylov = krylov, ev.substeps = substeps, ev.tol = tol, ev.tau_re = tau_re, ev.tau_im = tau_im;
    ev.cutoff = cutoff, ev.maxdim = maxdim;
    QIL_TRY(ev.init());
    for (int s = 0; s < steps; ++s) QIL_TRY(ev.step());
    xh->amplitude = x0->amplitude * xh->amplitude * std::exp(ev.log_sum);
    if (info) {
        ev.info_head(info, steps, ev.converged, ev.worst);
        info[7] = (double)ev.extra_passes, info[8] = ev.growth, info[9] = ev.log_sum;
    }
    *out = x_own.release();
    return QIL_OK;
}
