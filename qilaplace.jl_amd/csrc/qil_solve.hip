// The linear solver (qil_mps_solve): (A + shift I) x = c for a Hermitian positive definite A + shift I, by the alternating
// two-site solver (ALS / DMRG for linear systems).  x is kept in an orthonormal gauge around the bond k being solved; with the
// environments L_A[p, a, s], R_A[q, b, l] of <x|A|x> and Lc[p, s], Rc[q, l] of <x|c> (conventions of qil_environment: the bra is
// conj(x) and contracts the operator's s_out) the two-site tensor y[p, s1, s2, q] = x_k x_{k+1} solves the local system
//     H y = g,   H v = L_A A_k A_{k+1} R_A v + shift v,   g = Lc c_k c_{k+1} Rc
// by conjugate gradients, is split by the SVD under the project's truncation rule, and the sweep moves on by one site.
//
// The matvec is the four dependent products of qil_twosite.h (its host steps, shared with qil_eigs.hip, are defined below):
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
    const long long e = cx ? 16 : 8;
    return kRedBytes + e * (xl * xl * dl + xr * xr * dr + 4 * dl * dm + 4 * dm * dr + 12 * xl * xr +
                            2 * local_block_elems(xl, xr, dl, dm, dr, cm, cr));
}

// The auto rule inside the fit.  One full sweep, local vs gemm, same operands (tools/_solve_time.py, median of 10, one MI355X, ms,
// 40 tensors, f64 / c64): chi 4, D 2 .. 8: 10.9 - 13.1 vs 22.8 - 26.5 / 12.8 - 15.5 vs 28.2 - 34.7; chi 8, D 8 (98 k multiply-adds
// per matvec): 30.0 vs 39.1 / 38.4 vs 52.0; chi 16, D 3 (135 k): 47.5 vs 52.2; chi 16, D 5 (266 k, f64 only: c64 does not fit):
// 81.4 vs 71.9, and 17.1 vs 16.1 at 12 tensors -- the one workgroup loses once a matvec is a quarter of a million multiply-adds,
// whatever the element type (the products are latency-bound).  So auto takes the local route up to 200 k; QIL_SOLVE_ROUTE=local
// takes it wherever it fits.
constexpr long long kLocalMaxMacs = 200000;

struct LocalArgs {
    const void *LA, *RA, *A0, *A1;     // environments (TE), operator sites (TA)
    const void *Lc, *Rc, *C0, *C1;     // environments of <x|c> (TE), sites of c (TC)
    void* y;                           // (xl, 2, 2, xr) TE: the start on entry, the solution on return
    double* stat;                      // ST_WORDS doubles
    int xl, xr, dl, dm, dr, cl, cm, cr;
    int blk, cg_iters;
    double shift, tol;
};

// One workgroup solves H y = g for one bond.  Every loop around a barrier has uniform bounds; alpha, beta and the stopping test
// come out of wg_sum, which hands every thread the same bits, so all threads take the same branches.  No spin, no atomics: the
// loop ends after cg_iters iterations at the latest.
template <class TA, class TC, class TE>
__global__ __launch_bounds__(kThreads) void solve_local(const LocalArgs g) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double* red = reinterpret_cast<double*>(lds_raw);
    const int xl = g.xl, xr = g.xr, dl = g.dl, dm = g.dm, dr = g.dr, nv = 4 * xl * xr;
    TE* Ls = reinterpret_cast<TE*>(lds_raw + kRedBytes);
    TE* Rs = Ls + xl * dl * xl;
    TE* W0 = Rs + xr * dr * xr;
    TE* W1 = W0 + 4 * dl * dm;
    TE* yv = W1 + 4 * dm * dr;
    TE* rv = yv + nv;
    TE* pv = rv + nv;
    TE* X = pv + nv;
    TE* Y = X + g.blk;
    {   // stage: the operator sites are widened on the way
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

    template <class TA, class TC, class TE>
    int launch_local(const LocalArgs& g, size_t lds) {
        static qil_lds_grant grant;
        QIL_HIP(grant.ensure(ctx->device, reinterpret_cast<const void*>(&solve_local<TA, TC, TE>), lds));
        hipLaunchKernelGGL((solve_local<TA, TC, TE>), dim3(1), dim3(kThreads), lds, qil_stream(ctx), g);
        QIL_HIP(hipGetLastError());
        return QIL_OK;
    }

    int solve_bond_local(int64_t k, void* y, double* hst) {
        LocalArgs g{};
        g.LA = LA[(size_t)k], g.RA = RA[(size_t)k + 2], g.A0 = A->site[(size_t)k], g.A1 = A->site[(size_t)k + 1];
        g.Lc = Lp[0][(size_t)k], g.Rc = Rp[0][(size_t)k + 2], g.C0 = c->site[(size_t)k], g.C1 = c->site[(size_t)k + 1];
        g.y = y, g.stat = static_cast<double*>(stat);
        g.xl = (int)xd(k), g.xr = (int)xd(k + 2), g.dl = (int)ad(k), g.dm = (int)ad(k + 1), g.dr = (int)ad(k + 2);
        g.cl = (int)cd(k), g.cm = (int)cd(k + 1), g.cr = (int)cd(k + 2);
        g.blk = (int)local_block_elems(g.xl, g.xr, g.dl, g.dm, g.dr, g.cm, g.cr);
        g.cg_iters = cg_iters, g.shift = shift, g.tol = tol;
        const bool cx = dt == QIL_C64;
        const size_t lds = (size_t)local_lds_bytes(cx, g.xl, g.xr, g.dl, g.dm, g.dr, g.cm, g.cr);
        QIL_REQUIRE((long long)lds <= kLdsBudget, QIL_EINVAL_ARG, "solve: bond %lld does not fit the local route", (long long)k);
        if (!cx) {
            QIL_TRY((launch_local<double, double, double>(g, lds)));
        } else {
            QIL_TRY(for_elem_types(A->dtype == QIL_C64, c->dtype == QIL_C64, [&](auto a, auto cc) {
                return launch_local<decltype(a), decltype(cc), c64>(g, lds);
            }));
        }
        uint64_t ticket = 0;
        QIL_TRY(qil_read_back_post(ctx, stat, ST_WORDS * sizeof(double), &ticket));
        return qil_read_back_wait(ctx, ticket, hst, ST_WORDS * sizeof(double));
    }

    int solve_bond_gemm(int64_t k, void* y, double* hst) {
        const int64_t xl = xd(k), xr = xd(k + 2), dl = ad(k), dm = ad(k + 1), dr = ad(k + 2);
        const int64_t cm = cd(k + 1), cr = cd(k + 2), nv = 4 * xl * xr;
        QIL_REQUIRE(nv < (1LL << 31), QIL_EINVAL_ARG, "solve: a two-site tensor of %lld elements", (long long)nv);
        const long long blk = local_block_elems(xl, xr, dl, dm, dr, cm, cr);
        void *T1 = nullptr, *T2 = nullptr, *H = nullptr, *r = nullptr, *p = nullptr, *Aw0 = nullptr, *Aw1 = nullptr;
        const void *A0 = nullptr, *A1 = nullptr;
        QIL_TRY(tmp.alloc((size_t)blk * e, &T1));
        QIL_TRY(tmp.alloc((size_t)blk * e, &T2));
        QIL_TRY(tmp.alloc((size_t)nv * e, &H));
        QIL_TRY(tmp.alloc((size_t)nv * e, &r));
        QIL_TRY(tmp.alloc((size_t)nv * e, &p));
        if (A->dtype != dt) {
            QIL_TRY(tmp.alloc((size_t)(4 * dl * dm) * e, &Aw0));
            QIL_TRY(tmp.alloc((size_t)(4 * dm * dr) * e, &Aw1));
        }
        QIL_TRY(qil_site_operand(ctx, dt, A, k, Aw0, &A0));
        QIL_TRY(qil_site_operand(ctx, dt, A, k + 1, Aw1, &A1));
        QIL_TRY(overlap_local(0, k, T1, T2, r));                           // g = Lc c_k c_{k+1} Rc -> r
        QIL_TRY(gemm_matvec(k, A0, A1, y, T1, T2, H));
        double* st = static_cast<double*>(stat);
        const bool cx = dt == QIL_C64;
        for_elem_type(cx, [&](auto t) {
            using TE = decltype(t);
            hipLaunchKernelGGL((cg_start<TE>), dim3(1), dim3(kThreads), 0, qil_stream(ctx), (const TE*)H, (const TE*)y, (TE*)r, (TE*)p,
                               (int)nv, shift, tol, st);
            return 0;
        });
        QIL_HIP(hipGetLastError());
        QIL_TRY(qil_read_back(ctx, hst, stat, ST_WORDS * sizeof(double)));
        int enq = 0;
        while (hst[ST_DONE] == 0.0 && enq < cg_iters) {
            const int batch = std::min(kPoll, cg_iters - enq);
            for (int j = 0; j < batch; ++j) {
                QIL_TRY(gemm_matvec(k, A0, A1, p, T1, T2, H));
                for_elem_type(cx, [&](auto t) {
                    using TE = decltype(t);
                    hipLaunchKernelGGL((cg_step<TE>), dim3(1), dim3(kThreads), 0, qil_stream(ctx), (const TE*)H, (TE*)y, (TE*)r, (TE*)p,
                                       (int)nv, shift, tol, cg_iters, st);
                    return 0;
                });
                QIL_HIP(hipGetLastError());
            }
            enq += batch;
            QIL_TRY(qil_read_back(ctx, hst, stat, ST_WORDS * sizeof(double)));
        }
        for (void* q : {Aw1, Aw0, p, r, H, T2, T1})
            if (q) tmp.free(q);
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

// ---- the host steps of qil_twosite.h (declared there, used by this file and by qil_eigs.hip)
namespace qil_twosite {

int Sweep::init_envs() {
    LA.assign((size_t)n + 1, nullptr), RA = LA;
    Lp.assign(phi.size(), LA), Rp = Lp;
    std::vector<std::vector<void*>*> left{&LA}, right{&RA};
    for (size_t i = 0; i < phi.size(); ++i) left.push_back(&Lp[i]), right.push_back(&Rp[i]);
    for (std::vector<void*>* v : left) {
        QIL_TRY(tmp.alloc(e, &(*v)[0]));
        QIL_TRY(qil_dev_fill_ones(ctx, dt, (*v)[0], 1));
    }
    for (std::vector<void*>* v : right) {
        QIL_TRY(tmp.alloc(e, &(*v)[(size_t)n]));
        QIL_TRY(qil_dev_fill_ones(ctx, dt, (*v)[(size_t)n], 1));
    }
    for (int64_t j = n - 1; j >= 2; --j) QIL_TRY(extend(j, true));
    return QIL_OK;
}

int Sweep::extend(int64_t j, bool right) {
    int64_t xi = xd(j), xo = xd(j + 1), di = ad(j), dq = ad(j + 1);
    const long long nx = 2 * xi * xo, na = 4 * di * dq;
    void *Xw = nullptr, *Aw = nullptr, *T1 = nullptr, *T2 = nullptr, *En = nullptr;
    const void *Xs = nullptr, *As = nullptr;
    if (right) QIL_TRY(tmp.alloc((size_t)nx * e, &Xw));
    if (right || A->dtype != dt) QIL_TRY(tmp.alloc((size_t)na * e, &Aw));
    if (right) {
        std::swap(xi, xo), std::swap(di, dq);
        QIL_TRY(qil_put_mps_site(ctx, dt, x, j, QIL_SITE_REVERSED, Xw));
        QIL_TRY(qil_put_mpo_site(ctx, dt, A, j, QIL_SITE_REVERSED, Aw));
        Xs = Xw, As = Aw;
    } else {
        Xs = x->site[(size_t)j];
        QIL_TRY(qil_site_operand(ctx, dt, A, j, Aw, &As));
    }
    const long long nT = 2 * std::max(xi, xo) * std::max(di, dq) * std::max(xi, xo);
    QIL_TRY(tmp.alloc((size_t)nT * e, &T1));
    QIL_TRY(tmp.alloc((size_t)nT * e, &T2));
    QIL_TRY(tmp.alloc((size_t)(xo * dq * xo) * e, &En));
    QIL_TRY(qil_apply_overlap_env_step(ctx, dt, xi, xo, xi, xo, di, dq, Xs, Xs, As, right ? RA[(size_t)j + 1] : LA[(size_t)j], T1,
                                       T2, En));
    tmp.free(T2);
    tmp.free(T1);
    const int64_t to = right ? j : j + 1;
    replace(right ? RA : LA, to, En);
    for (size_t i = 0; i < phi.size(); ++i) {
        int64_t ci = pd(i, j), co = pd(i, j + 1);
        void *Cw = nullptr, *Ecn = nullptr;
        const void* Cs = nullptr;
        if (right || phi[i]->dtype != dt) QIL_TRY(tmp.alloc((size_t)(2 * ci * co) * e, &Cw));
        if (right) {
            std::swap(ci, co);
            QIL_TRY(qil_put_mps_site(ctx, dt, phi[i], j, QIL_SITE_REVERSED, Cw));
            Cs = Cw;
        } else {
            QIL_TRY(qil_site_operand(ctx, dt, phi[i], j, Cw, &Cs));
        }
        QIL_TRY(tmp.alloc((size_t)(xo * co) * e, &Ecn));
        QIL_TRY(tmp.alloc((size_t)(2 * xi * co) * e, &T1));
        QIL_TRY(qil_overlap_env_step(ctx, dt, 2, xi, xo, ci, co, Xs, Cs, right ? Rp[i][(size_t)j + 1] : Lp[i][(size_t)j], T1, Ecn));
        tmp.free(T1);
        if (Cw) tmp.free(Cw);
        replace(right ? Rp[i] : Lp[i], to, Ecn);
    }
    if (Aw) tmp.free(Aw);
    if (Xw) tmp.free(Xw);
    return QIL_OK;
}

int Sweep::overlap_local(size_t i, int64_t k, void* T1, void* T2, void* out) {
    const int64_t xl = xd(k), xr = xd(k + 2), cl = pd(i, k), cm = pd(i, k + 1), cr = pd(i, k + 2);
    void *Cw0 = nullptr, *Cw1 = nullptr;
    const void *C0 = nullptr, *C1 = nullptr;
    if (phi[i]->dtype != dt) {
        QIL_TRY(tmp.alloc((size_t)(2 * cl * cm) * e, &Cw0));
        QIL_TRY(tmp.alloc((size_t)(2 * cm * cr) * e, &Cw1));
    }
    QIL_TRY(qil_site_operand(ctx, dt, phi[i], k, Cw0, &C0));
    QIL_TRY(qil_site_operand(ctx, dt, phi[i], k + 1, Cw1, &C1));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, xl, 2 * cm, cl, Lp[i][(size_t)k], xl, C0, cl, T1, xl));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, 2 * xl, 2 * cr, cm, T1, 2 * xl, C1, cm, T2, 2 * xl));
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 1, 4 * xl, xr, cr, T2, 4 * xl, Rp[i][(size_t)k + 2], xr, out, 4 * xl));
    for (void* q : {Cw1, Cw0})
        if (q) tmp.free(q);
    return QIL_OK;
}

int Sweep::gemm_matvec(int64_t k, const void* A0, const void* A1, const void* v, void* T1, void* T2, void* out) {
    const int64_t xl = xd(k), xr = xd(k + 2), dl = ad(k), dm = ad(k + 1), dr = ad(k + 2);
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, xl * dl, 4 * xr, xl, LA[(size_t)k], xl * dl, v, xl, T1, xl * dl));
    qil_gemm_batch b2, b3;
    b2.count = 2 * xr, b2.a_bs = xl * 2 * dl, b2.c_bs = xl * 2 * dm;
    QIL_TRY(qil_dev_gemm_batched(ctx, dt, 0, 0, xl, 2 * dm, 2 * dl, T1, xl, A0, 2 * dl, T2, xl, &b2));
    b3.count = xr, b3.a_bs = 2 * xl * 2 * dm, b3.c_bs = 2 * xl * 2 * dr;
    QIL_TRY(qil_dev_gemm_batched(ctx, dt, 0, 0, 2 * xl, 2 * dr, 2 * dm, T2, 2 * xl, A1, 2 * dm, T1, 2 * xl, &b3));
    return qil_dev_gemm(ctx, dt, 0, 1, 4 * xl, xr, dr * xr, T1, 4 * xl, RA[(size_t)k + 2], xr, out, 4 * xl);
}

int Sweep::gemm_matvec1(int64_t j, const void* A0, const void* v, void* T1, void* T2, void* out) {
    const int64_t xl = xd(j), xr = xd(j + 1), dl = ad(j), dr = ad(j + 1);
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, xl * dl, 2 * xr, xl, LA[(size_t)j], xl * dl, v, xl, T1, xl * dl));
    qil_gemm_batch b2;
    b2.count = xr, b2.a_bs = xl * 2 * dl, b2.c_bs = xl * 2 * dr;
    QIL_TRY(qil_dev_gemm_batched(ctx, dt, 0, 0, xl, 2 * dr, 2 * dl, T1, xl, A0, 2 * dl, T2, xl, &b2));
    return qil_dev_gemm(ctx, dt, 0, 1, 2 * xl, xr, dr * xr, T2, 2 * xl, RA[(size_t)j + 1], xr, out, 2 * xl);
}

int Sweep::two_site(int64_t k, void** y) {
    const int64_t m = 2 * xd(k), nn = 2 * xd(k + 2), xm = xd(k + 1);
    QIL_TRY(tmp.alloc((size_t)(m * nn) * e, y));
    return qil_dev_gemm(ctx, dt, 0, 0, m, nn, xm, x->site[(size_t)k], m, x->site[(size_t)k + 1], xm, *y, m);
}

int Sweep::split(int64_t k, bool to_right, void* y, bool unit) {
    const int64_t xl = xd(k), xr = xd(k + 2);
    const int64_t m = 2 * xl, nn = 2 * xr, r0 = std::min(m, nn);
    void *U = nullptr, *Vh = nullptr;
    QIL_TRY(tmp.alloc((size_t)(m * r0) * e, &U));
    QIL_TRY(tmp.alloc((size_t)(r0 * nn) * e, &Vh));
    std::vector<double> S((size_t)r0, 0.0);
    QIL_TRY(qil_dev_svd(ctx, dt, m, nn, y, m, U, m, S.data(), Vh, r0));
    const int64_t r = qil_truncation_rank(S.data(), r0, cutoff, true, maxdim, 1);
    double s2 = 0.0;
    for (int64_t i = 0; i < r; ++i) s2 += S[(size_t)i] * S[(size_t)i];
    kept = std::sqrt(s2);
    if (unit) {
        const double f = s2 > 0.0 ? 1.0 / std::sqrt(s2) : 1.0;
        for (int64_t i = 0; i < r; ++i) S[(size_t)i] *= f;
    }
    void *s0 = nullptr, *s1 = nullptr;
    QIL_TRY(tmp.alloc((size_t)(m * r) * e, &s0));
    QIL_TRY(tmp.alloc((size_t)(r * nn) * e, &s1));
    QIL_TRY(qil_dev_copy(ctx, s0, U, (size_t)(m * r) * e));
    QIL_TRY(qil_dev_copy2d(ctx, s1, (size_t)r * e, Vh, (size_t)r0 * e, (size_t)r * e, (size_t)nn));
    if (to_right) QIL_TRY(qil_dev_scale(ctx, dt, 0, r, nn, s1, r, S.data()));
    else QIL_TRY(qil_dev_scale(ctx, dt, 1, m, r, s0, m, S.data()));
    QIL_TRY(qil_chain_set_site(x, k, tmp.give(s0), xl, r));
    QIL_TRY(qil_chain_set_site(x, k + 1, tmp.give(s1), r, xr));
    tmp.free(Vh);
    tmp.free(U);
    tmp.free(y);
    return QIL_OK;
}

int start_gauge(qil_mps* xh, int64_t maxdim) {
    int64_t widest = 1;
    for (int64_t d : xh->dims) widest = std::max(widest, d);
    if (widest > maxdim) {                                   // left-orthonormal, then the truncating sweep back
        QIL_TRY(qil_gauge_exact(xh, QIL_DIR_RIGHT, 0));
        return qil_canonicalize(xh, QIL_DIR_LEFT, 0, 0.0, maxdim);
    }
    return qil_gauge_exact(xh, QIL_DIR_LEFT, 0);
}

}  // namespace qil_twosite

// The decision qil_mps_solve switches on for every bond: 1 when the LDS solve_local needs for these dimensions (local_lds_bytes
// above) is within the 160 KiB budget, QIL_SOLVE_ROUTE does not say gemm and -- unless it says local -- a matvec stays within
// kLocalMaxMacs multiply-adds (where the one workgroup was measured to win).
extern "C" int qil_mps_solve_local_fits(int complex_, int64_t xl, int64_t xr, int64_t dl, int64_t dm, int64_t dr, int64_t cl, int64_t cm,
                                        int64_t cr, int* fits) {
    QIL_REQUIRE(fits, QIL_EINVAL_ARG, "solve_local_fits: null argument");
    QIL_REQUIRE(xl >= 1 && xr >= 1 && dl >= 1 && dm >= 1 && dr >= 1 && cl >= 1 && cm >= 1 && cr >= 1, QIL_EINVAL_ARG,
                "solve_local_fits: dimensions must be positive");
    *fits = 0;
    const int route = route_from(getenv("QIL_SOLVE_ROUTE"));
    if (route == ROUTE_GEMM) return QIL_OK;
    if (std::max({xl, xr, dl, dm, dr, cl, cm, cr}) > kDimCap) return QIL_OK;
    if (local_lds_bytes(complex_ != 0, xl, xr, dl, dm, dr, cm, cr) > kLdsBudget) return QIL_OK;
    *fits = route == ROUTE_LOCAL || local_matvec_macs(xl, xr, dl, dm, dr) <= kLocalMaxMacs ? 1 : 0;
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
    while (sweeps < max_sweeps) {
        QIL_TRY(sv.sweep());
        ++sweeps;
        if (sv.sweep_res <= tol) {
            converged = 1;
            break;
        }
    }
    if (info) {
        int64_t bond = 1;
        for (int64_t d : xh->dims) bond = std::max(bond, d);
        info[0] = sweeps, info[1] = converged, info[2] = sv.sweep_res, info[3] = (double)sv.matvecs, info[4] = (double)bond;
        info[5] = (double)sv.n_local, info[6] = (double)sv.n_gemm, info[7] = 0.0;
    }
    *out = x_own.release();
    return QIL_OK;
}
