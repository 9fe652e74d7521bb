// The linear solver (qil_mps_solve): (A + shift I) x = c for a Hermitian positive definite A + shift I, by the alternating
// two-site solver (ALS / DMRG for linear systems).  x is kept in an orthonormal gauge around the bond k being solved; with the
// environments L_A[p, a, s], R_A[q, b, l] of <x|A|x> and Lc[p, s], Rc[q, l] of <x|c> (conventions of qil_environment: the bra is
// conj(x) and contracts the operator's s_out) the two-site tensor y[p, s1, s2, q] = x_k x_{k+1} solves the local system
//     H y = g,   H v = L_A A_k A_{k+1} R_A v + shift v,   g = Lc c_k c_{k+1} Rc
// by conjugate gradients, is split by the SVD under the project's truncation rule, and the sweep moves on by one site.
//
// The matvec is the four dependent products of qil_twosite.h (the sweep's host steps are defined in qil_twosite.hip):
//   local route   ONE launch, one workgroup (solve_local): L_A, R_A, both operator sites, y, r, p and two ping-pong blocks in LDS,
//                 g, the first residual and the whole CG in it; the iteration count is bounded inside the kernel
//   gemm route    the four products as qil_dev_gemm / qil_dev_gemm_batched, CG's scalars in device memory (cg_start, cg_step), the
//                 host reads the flags once per 8 iterations; any bonds
//
// The local problem is the same for both sweep directions (the direction only decides which SVD factor keeps the weights and
// which environment grows), so the kernel needs no re-indexing; operands are widened while they are staged.
// Every temporary belongs to the call's qil_scratch; the working copy of x is the result handle.
#include "qil_twosite.h"

namespace {

using namespace qil_twosite;

constexpr int kPoll = 8;                            // gemm route: iterations enqueued per read-back of the flags

// what a local solve reports (doubles, one read-back)
enum { ST_STATUS = 0, ST_ITERS = 1, ST_RES0 = 2, ST_RES = 3, ST_GNORM = 4, ST_RS = 5, ST_DONE = 6, ST_WORDS = 8 };

// elements of one ping-pong block: the matvec's T1, T2, T3 and g's two intermediates Lc c_k, (Lc c_k) c_{k+1}
long long local_block_elems(long long xl, long long xr, long long dl, long long dm, long long dr, long long cm, long long cr) {
    return std::max({4 * xl * xr * std::max({dl, dm, dr}), 2 * xl * cm, 4 * xl * cr});
}
// LDS bytes of solve_local:
//   128 + e * (xl^2 dl + xr^2 dr + 4 dl dm + 4 dm dr + 3 * 4 xl xr + 2 * blk),   e = 8 (f64) / 16 (c64),
//   blk = max(4 xl xr max(dl, dm, dr), 2 xl cm, 4 xl cr)
long long local_lds_bytes(bool cx, long long xl, long long xr, long long dl, long long dm, long long dr, long long cm, long long cr) {
    return local_bytes(cx, 0, frame_elems(2, xl, xr, dl, dm, dr), 3, 4 * xl * xr, local_block_elems(xl, xr, dl, dm, dr, cm, cr));
}

struct LocalArgs : FrameArgs {         // y: (xl, 2, 2, xr), the solution on return; stat: ST_WORDS doubles
    const void *Lc, *Rc, *C0, *C1;     // environments of <x|c> (TE), sites of c (TC)
    int cl, cm, cr;
    int cg_iters;
    double tol;
};

// One workgroup solves H y = g for one bond.  Every loop around a barrier has uniform bounds; alpha, beta and the stopping test
// come out of wg_sum, which hands every thread the same bits, so all threads take the same branches.  No spin, no atomics: the
// loop ends after cg_iters iterations at the latest.
template <class TA, class TC, class TE>
__global__ __launch_bounds__(kThreads) void solve_local(const LocalArgs g) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double* red = reinterpret_cast<double*>(lds_raw);
    const int xl = g.xl, xr = g.xr, nv = 4 * xl * xr;
    const int dl = g.dl, dm = g.dm, dr = g.dr;
    TE* Ls = reinterpret_cast<TE*>(lds_raw + kRedBytes);
    TE* Rs = Ls + xl * dl * xl;
    TE* W0 = Rs + xr * dr * xr;
    TE* W1 = W0 + 4 * dl * dm;
    TE* yv = W1 + 4 * dm * dr;
    TE* rv = yv + nv;
    TE* pv = rv + nv;
    TE* X = pv + nv;
    TE* Y = X + g.blk;
    {   // stage, spelled out here and not through stage_frame (the frame of qil_twosite.h, same layout): inlined into this kernel the
        // helper's address arithmetic costs two VGPRs in the variants with a complex right-hand side (MEASUREMENTS 33)
        const TE* LA = static_cast<const TE*>(g.LA);
        const TE* RA = static_cast<const TE*>(g.RA);
        const TA* A0 = static_cast<const TA*>(g.A0);
        const TA* A1 = static_cast<const TA*>(g.A1);
        const TE* y0 = static_cast<const TE*>(g.y);
        for (int t = threadIdx.x; t < xl * dl * xl; t += kThreads) Ls[t] = LA[t];
        for (int t = threadIdx.x; t < xr * dr * xr; t += kThreads) Rs[t] = RA[t];
        for (int t = threadIdx.x; t < 4 * dl * dm; t += kThreads) W0[t] = cast_elem<TE>(A0[t]);
        for (int t = threadIdx.x; t < 4 * dm * dr; t += kThreads) W1[t] = cast_elem<TE>(A1[t]);
        for (int t = threadIdx.x; t < nv; t += kThreads) yv[t] = y0[t];
    }
    {   // g = Lc c_k c_{k+1} Rc -> rv, its operands straight from global memory (read once)
        const TE* Lc = static_cast<const TE*>(g.Lc);
        const TE* Rc = static_cast<const TE*>(g.Rc);
        const TC* C0 = static_cast<const TC*>(g.C0);
        const TC* C1 = static_cast<const TC*>(g.C1);
        const int cl = g.cl, cm = g.cm, cr = g.cr;
        for (int t = threadIdx.x; t < xl * 2 * cm; t += kThreads) {        // [p, s1, m] -> X
            const int p = t % xl, u = t / xl;
            TE acc{};
            for (int k = 0; k < cl; ++k) acc = cmul_add(acc, Lc[p + xl * k], C0[k + cl * u]);
            X[t] = acc;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < 2 * xl * 2 * cr; t += kThreads) {    // [(p, s1), s2, l] -> Y
            const int ps = t % (2 * xl), u = t / (2 * xl);
            TE acc{};
            for (int m = 0; m < cm; ++m) acc = cmul_add(acc, X[ps + 2 * xl * m], C1[m + cm * u]);
            Y[t] = acc;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < nv; t += kThreads) {                 // [(p, s1, s2), q] -> rv
            const int pss = t % (4 * xl), q = t / (4 * xl);
            TE acc{};
            for (int l = 0; l < cr; ++l) acc = cmul_add(acc, Y[pss + 4 * xl * l], Rc[q + xr * l]);
            rv[t] = acc;
        }
        __syncthreads();
    }
    double part = 0.0;
    for (int t = threadIdx.x; t < nv; t += kThreads) part += abs2_t(rv[t]);
    const double gnorm = sqrt(wg_sum(part, red));
    local_matvec<TE>(g, Ls, Rs, W0, W1, yv, X, Y);
    part = 0.0;
    for (int t = threadIdx.x; t < nv; t += kThreads) {
        const TE r = sub_t(rv[t], Y[t]);
        rv[t] = r;
        pv[t] = r;
        part += abs2_t(r);
    }
    double rs = wg_sum(part, red);
    const double res0 = sqrt(rs), thr = g.tol * gnorm;
    int it = 0, status = 0;
    while (it < g.cg_iters && sqrt(rs) > thr) {
        __syncthreads();                                                   // pv is complete
        local_matvec<TE>(g, Ls, Rs, W0, W1, pv, X, Y);
        part = 0.0;
        for (int t = threadIdx.x; t < nv; t += kThreads) {
            double gr = 0.0, gi = 0.0;
            dot_parts(pv[t], Y[t], gr, gi);
            part += gr;
        }
        const double pAp = wg_sum(part, red);
        if (!(pAp > 0.0) || !isfinite(pAp)) {                              // not positive definite on this space: uniform exit
            status = 1;
            break;
        }
        const double alpha = rs / pAp;
        part = 0.0;
        for (int t = threadIdx.x; t < nv; t += kThreads) {
            const TE p = pv[t];
            yv[t] = add_t(yv[t], scale_t(p, alpha));
            const TE r = sub_t(rv[t], scale_t(Y[t], alpha));
            rv[t] = r;
            part += abs2_t(r);
        }
        const double rs_new = wg_sum(part, red);
        const double beta = rs_new / rs;
        for (int t = threadIdx.x; t < nv; t += kThreads) pv[t] = add_t(rv[t], scale_t(pv[t], beta));
        rs = rs_new;
        ++it;
    }
    __syncthreads();
    TE* yo = static_cast<TE*>(g.y);
    for (int t = threadIdx.x; t < nv; t += kThreads) yo[t] = yv[t];
    if (threadIdx.x == 0) {
        g.stat[ST_STATUS] = status;
        g.stat[ST_ITERS] = it;
        g.stat[ST_RES0] = res0;
        g.stat[ST_RES] = sqrt(rs);
        g.stat[ST_GNORM] = gnorm;
        g.stat[ST_RS] = rs;
        g.stat[ST_DONE] = 1.0;
        g.stat[7] = 0.0;
    }
}

// ---- gemm route: CG's vector steps, one workgroup each, the scalars in `st` (device)
// r holds g on entry, Hy the product without the shift: r = g - (Hy + shift y), p = r; st = the start of the iteration
template <class TE>
__global__ __launch_bounds__(kThreads) void cg_start(const TE* __restrict__ Hy, const TE* __restrict__ y, TE* __restrict__ r,
                                                     TE* __restrict__ p, int nv, double shift, double tol, double* __restrict__ st) {
    __shared__ double red[8];
    double a[2] = {0.0, 0.0};
    const TE sh = cast_elem<TE>(shift);
    for (int t = threadIdx.x; t < nv; t += kThreads) {
        const TE gv = r[t];
        const TE rr = sub_t(gv, cmul_add(Hy[t], sh, y[t]));
        r[t] = rr;
        p[t] = rr;
        a[0] += abs2_t(gv);
        a[1] += abs2_t(rr);
    }
    block_sum<2>(a, red);
    if (threadIdx.x == 0) {
        const double gnorm = sqrt(a[0]), res0 = sqrt(a[1]);
        st[ST_STATUS] = 0.0;
        st[ST_ITERS] = 0.0;
        st[ST_RES0] = res0;
        st[ST_RES] = res0;
        st[ST_GNORM] = gnorm;
        st[ST_RS] = a[1];
        st[ST_DONE] = res0 <= tol * gnorm ? 1.0 : 0.0;
        st[7] = 0.0;
    }
}
// one iteration given Hp (without the shift); a no-op once the done flag is set or cg_iters iterations have run
template <class TE>
__global__ __launch_bounds__(kThreads) void cg_step(const TE* __restrict__ Hp, TE* __restrict__ y, TE* __restrict__ r, TE* __restrict__ p,
                                                    int nv, double shift, double tol, int cg_iters, double* __restrict__ st) {
    __shared__ double red[4];
    const double done = st[ST_DONE], iters = st[ST_ITERS], rs = st[ST_RS], gnorm = st[ST_GNORM];
    if (done != 0.0 || iters >= (double)cg_iters) return;                  // uniform: thread 0 writes st behind the barriers below
    const TE sh = cast_elem<TE>(shift);
    double a[1] = {0.0};
    for (int t = threadIdx.x; t < nv; t += kThreads) {
        double gr = 0.0, gi = 0.0;
        dot_parts(p[t], cmul_add(Hp[t], sh, p[t]), gr, gi);
        a[0] += gr;
    }
    block_sum<1>(a, red);
    const double pAp = a[0];
    if (!(pAp > 0.0) || !isfinite(pAp)) {
        if (threadIdx.x == 0) st[ST_STATUS] = 1.0, st[ST_DONE] = 1.0;
        return;
    }
    const double alpha = rs / pAp;
    a[0] = 0.0;
    for (int t = threadIdx.x; t < nv; t += kThreads) {
        const TE pp = p[t];
        y[t] = add_t(y[t], scale_t(pp, alpha));
        const TE rr = sub_t(r[t], scale_t(cmul_add(Hp[t], sh, pp), alpha));
        r[t] = rr;
        a[0] += abs2_t(rr);
    }
    block_sum<1>(a, red);
    const double rs_new = a[0], beta = rs_new / rs;
    for (int t = threadIdx.x; t < nv; t += kThreads) p[t] = add_t(r[t], scale_t(p[t], beta));
    if (threadIdx.x == 0) {
        st[ST_RS] = rs_new;
        st[ST_RES] = sqrt(rs_new);
        st[ST_ITERS] = iters + 1.0;
        if (sqrt(rs_new) <= tol * gnorm) st[ST_DONE] = 1.0;
    }
}

struct Solver : Sweep {
    const qil_mps* c;
    double shift, tol;
    int cg_iters;
    void* stat = nullptr;
    double sweep_res = 0.0;

    Solver(qil_context* ctx_, qil_scratch& tmp_, const qil_mpo* A_, const qil_mps* c_, qil_mps* x_, int dt_)
        : Sweep(ctx_, tmp_, A_, x_, dt_), c(c_) {
        phi.push_back(c_);
    }

    int64_t cd(int64_t j) const { return c->dims[(size_t)j]; }

    int init() {
        QIL_TRY(tmp.alloc(ST_WORDS * sizeof(double), &stat));
        return init_envs();
    }

    int solve_bond_local(int64_t k, void* y, double* hst) {
        LocalArgs g{frame(2, k, y, stat)};
        g.Lc = Lp[0][(size_t)k], g.Rc = Rp[0][(size_t)k + 2], g.C0 = c->site[(size_t)k], g.C1 = c->site[(size_t)k + 1];
        g.cl = (int)cd(k), g.cm = (int)cd(k + 1), g.cr = (int)cd(k + 2);
        g.blk = (int)local_block_elems(g.xl, g.xr, g.dl, g.dm, g.dr, g.cm, g.cr);
        g.cg_iters = cg_iters, g.shift = shift, g.tol = tol;
        const bool cx = dt == QIL_C64;
        const size_t lds = (size_t)local_lds_bytes(cx, g.xl, g.xr, g.dl, g.dm, g.dr, g.cm, g.cr);
        QIL_REQUIRE((long long)lds <= kLdsBudget, QIL_EINVAL_ARG, "solve: bond %lld does not fit the local route", (long long)k);
        auto launch = [&](auto a, auto cc, auto t) {
            return launch_local<solve_local<decltype(a), decltype(cc), decltype(t)>>(g, lds, ST_WORDS, hst);
        };
        if (!cx) return launch(double{}, double{}, double{});          // a real sweep has real operands
        return for_elem_types(A->dtype == QIL_C64, c->dtype == QIL_C64, [&](auto a, auto cc) { return launch(a, cc, c64{}); });
    }

    int solve_bond_gemm(int64_t k, void* y, double* hst) {
        const int64_t xl = xd(k), xr = xd(k + 2), nv = 4 * xl * xr;
        QIL_REQUIRE(nv < (1LL << 31), QIL_EINVAL_ARG, "solve: a two-site tensor of %lld elements", (long long)nv);
        Work w;
        void *r = nullptr, *p = nullptr;
        QIL_TRY(work_alloc(2, k, local_block_elems(xl, xr, ad(k), ad(k + 1), ad(k + 2), cd(k + 1), cd(k + 2)), 0, &w));
        QIL_TRY(tmp.alloc((size_t)nv * e, &r));
        QIL_TRY(tmp.alloc((size_t)nv * e, &p));
        const void *A0 = w.A0, *A1 = w.A1;
        QIL_TRY(overlap_local(0, k, w.T1, w.T2, r));                       // g = Lc c_k c_{k+1} Rc -> r
        QIL_TRY(gemm_matvec(k, A0, A1, y, w.T1, w.T2, w.H));
        QIL_TRY(launch_wg([](auto t) { return &cg_start<decltype(t)>; }, w.H, y, r, p, (int)nv, shift, tol, stat));
        QIL_TRY(qil_read_back(ctx, hst, stat, ST_WORDS * sizeof(double)));
        int enq = 0;
        while (hst[ST_DONE] == 0.0 && enq < cg_iters) {
            const int batch = std::min(kPoll, cg_iters - enq);
            for (int j = 0; j < batch; ++j) {
                QIL_TRY(gemm_matvec(k, A0, A1, p, w.T1, w.T2, w.H));
                QIL_TRY(launch_wg([](auto t) { return &cg_step<decltype(t)>; }, w.H, y, r, p, (int)nv, shift, tol, cg_iters, stat));
            }
            enq += batch;
            QIL_TRY(qil_read_back(ctx, hst, stat, ST_WORDS * sizeof(double)));
        }
        tmp.free(p);
        tmp.free(r);
        work_free(w);
        return QIL_OK;
    }

    // one local step at bond k; to_right: the isometry stays at k and S V^H moves on, else U S moves to k
    int step(int64_t k, bool to_right) {
        const int64_t xl = xd(k), xr = xd(k + 2);
        void* y = nullptr;
        QIL_TRY(two_site(k, &y));
        int fits = 0;
        QIL_TRY(qil_mps_solve_local_fits(dt == QIL_C64, xl, xr, ad(k), ad(k + 1), ad(k + 2), cd(k), cd(k + 1), cd(k + 2), &fits));
        double st[ST_WORDS] = {};
        if (fits) {
            QIL_TRY(solve_bond_local(k, y, st));
            ++n_local;
        } else {
            QIL_TRY(solve_bond_gemm(k, y, st));
            ++n_gemm;
        }
        matvecs += 1 + (long long)st[ST_ITERS];
        QIL_REQUIRE(st[ST_STATUS] == 0.0, QIL_EDOMAIN, "solve: operator not positive definite on the local space (bond %lld)",
                    (long long)(k + 1));
        QIL_REQUIRE(std::isfinite(st[ST_RES]) && std::isfinite(st[ST_GNORM]), QIL_EDOMAIN,
                    "solve: the local solve at bond %lld is not finite", (long long)(k + 1));
        const double rel = st[ST_GNORM] > 0.0 ? st[ST_RES0] / st[ST_GNORM] : (st[ST_RES0] > 0.0 ? INFINITY : 0.0);
        sweep_res = std::max(sweep_res, rel);
        return split(k, to_right, y, false);
    }

    int sweep() {
        sweep_res = 0.0;
        return Sweep::sweep([&](int64_t k, bool to_right) { return step(k, to_right); });
    }
};

}  // namespace

// The decision qil_mps_solve switches on for every bond: local_route_fits with the LDS solve_local needs for these dimensions
// (local_lds_bytes above).  The multiply-adds are counted only where the bytes fit: up to kDimCap their formula could overflow.
extern "C" int qil_mps_solve_local_fits(int complex_, int64_t xl, int64_t xr, int64_t dl, int64_t dm, int64_t dr, int64_t cl, int64_t cm,
                                        int64_t cr, int* fits) {
    QIL_REQUIRE(fits, QIL_EINVAL_ARG, "solve_local_fits: null argument");
    QIL_REQUIRE(xl >= 1 && xr >= 1 && dl >= 1 && dm >= 1 && dr >= 1 && cl >= 1 && cm >= 1 && cr >= 1, QIL_EINVAL_ARG,
                "solve_local_fits: dimensions must be positive");
    const bool over = std::max({xl, xr, dl, dm, dr, cl, cm, cr}) > kDimCap;
    const long long bytes = over ? 0 : local_lds_bytes(complex_ != 0, xl, xr, dl, dm, dr, cm, cr);
    const long long macs = over || bytes > kLdsBudget ? 0 : local_matvec_macs(xl, xr, dl, dm, dr);
    *fits = local_route_fits(getenv("QIL_SOLVE_ROUTE"), over, bytes, macs);
    return QIL_OK;
}

extern "C" int qil_mps_solve(const qil_mpo* A, double shift, const qil_mps* c, const qil_mps* x0, int64_t maxdim, double cutoff,
                             double tol, int max_sweeps, int cg_iters, qil_mps** out, double* info) {
    QIL_REQUIRE(A && c && out, QIL_EINVAL_ARG, "solve: null argument");
    QIL_REQUIRE(maxdim >= 1 && max_sweeps >= 1 && cg_iters >= 1, QIL_EINVAL_ARG,
                "solve: maxdim, max_sweeps and cg_iters must be >= 1 (got %lld, %d, %d)", (long long)maxdim, max_sweeps, cg_iters);
    QIL_REQUIRE(std::isfinite(shift) && std::isfinite(cutoff) && std::isfinite(tol), QIL_EINVAL_ARG,
                "solve: shift, cutoff and tol must be finite");
    QIL_REQUIRE(cutoff >= 0.0 && tol > 0.0, QIL_EINVAL_ARG, "solve: cutoff must be >= 0 and tol > 0 (got %g, %g)", cutoff, tol);
    const int64_t n = c->n();
    QIL_REQUIRE(n != 1, QIL_EINVAL_LENGTH, "solve: the two-site step needs a bond, the chain has one tensor");
    QIL_TRY(qil_check_apply_operands(A, c));
    if (x0) QIL_TRY(qil_check_overlap_pair(x0, c));
    QIL_REQUIRE(n >= 2, QIL_EINVAL_LENGTH, "solve: the two-site step needs a bond, the chain has %lld tensor(s)", (long long)n);
    qil_context* ctx = c->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int dt = (A->dtype == QIL_C64 || c->dtype == QIL_C64 || (x0 && x0->dtype == QIL_C64)) ? QIL_C64 : QIL_F64;

    // the working copy: x0 (or c) in dt, in units of c's amplitude
    const qil_mps* src = x0 ? x0 : c;
    qil_mps* xh = nullptr;
    QIL_TRY(start_chain(ctx, src, dt, c->amplitude, &xh));
    qil_result_guard<qil_mps> x_own(xh);
    if (x0 && c->amplitude != 0.0 && x0->amplitude != c->amplitude) {
        const double f = x0->amplitude / c->amplitude;
        if (std::isfinite(f)) {
            std::vector<double> s((size_t)xh->dims[1], f);
            QIL_TRY(qil_dev_scale(ctx, dt, 1, 2 * xh->dims[0], xh->dims[1], xh->site[0], 2 * xh->dims[0], s.data()));
        }
    }
    QIL_TRY(start_gauge(xh, maxdim));

    qil_scratch tmp(ctx);
    Solver sv(ctx, tmp, A, c, xh, dt);
    sv.shift = shift, sv.cutoff = cutoff, sv.tol = tol, sv.maxdim = maxdim, sv.cg_iters = cg_iters;
    QIL_TRY(sv.init());
    int sweeps = 0, converged = 0;
    QIL_TRY(sweep_until([&] { return sv.sweep(); }, sv.sweep_res, tol, max_sweeps, &sweeps, &converged));
    if (info) sv.info_head(info, sweeps, converged, sv.sweep_res), info[7] = 0.0;
    *out = x_own.release();
    return QIL_OK;
}
