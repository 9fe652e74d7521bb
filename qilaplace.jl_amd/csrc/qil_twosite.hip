// The host steps of the two-site sweeps (declared in qil_twosite.h; used by qil_solve.hip, qil_eigs.hip and qil_evolve.hip): the
// environments and how they grow, the projection of a further state onto the local space, the matvecs as GEMMs, the two-site
// tensor and its split, the argument frame of the one-workgroup kernels, the work blocks of the gemm routes, the head of the
// info vector and the gauge a sweep starts in.  Nothing here depends on the local problem.
#include "qil_twosite.h"

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

FrameArgs Sweep::frame(int sites, int64_t j, void* y, void* stat) const {
    const Dims d = dims_of(sites, j);
    FrameArgs f{};
    f.LA = LA[(size_t)j], f.RA = RA[(size_t)j + sites], f.A0 = A->site[(size_t)j], f.A1 = sites == 2 ? A->site[(size_t)j + 1] : nullptr;
    f.y = y, f.stat = static_cast<double*>(stat);
    f.xl = (int)d.xl, f.xr = (int)d.xr, f.dl = (int)d.dl, f.dm = (int)d.dm, f.dr = (int)d.dr;
    f.blk = (sites == 2 ? 4 : 2) * f.xl * f.xr * (int)std::max({d.dl, d.dm, d.dr});
    return f;
}

int Sweep::work_alloc(int sites, int64_t j, long long blk, int krylov, Work* w) {
    const Dims d = dims_of(sites, j);
    const int64_t nv = (sites == 2 ? 4 : 2) * d.xl * d.xr;
    QIL_TRY(tmp.alloc((size_t)blk * e, &w->T1));
    QIL_TRY(tmp.alloc((size_t)blk * e, &w->T2));
    QIL_TRY(tmp.alloc((size_t)nv * e, &w->H));
    if (krylov > 0) {
        QIL_TRY(tmp.alloc((size_t)(krylov * nv) * e, &w->V));
        QIL_TRY(qil_dev_zero(ctx, w->V, (size_t)(krylov * nv) * e));
    }
    if (A->dtype != dt) {
        QIL_TRY(tmp.alloc((size_t)(4 * ad(j) * ad(j + 1)) * e, &w->Aw0));
        if (sites == 2) QIL_TRY(tmp.alloc((size_t)(4 * ad(j + 1) * ad(j + 2)) * e, &w->Aw1));
    }
    QIL_TRY(qil_site_operand(ctx, dt, A, j, w->Aw0, &w->A0));
    if (sites == 2) QIL_TRY(qil_site_operand(ctx, dt, A, j + 1, w->Aw1, &w->A1));
    return QIL_OK;
}

void Sweep::work_free(const Work& w) {
    for (void* q : {w.Aw1, w.Aw0, w.V, w.H, w.T2, w.T1})
        if (q) tmp.free(q);
}

void Sweep::info_head(double* info, double count, double converged, double res) const {
    int64_t bond = 1;
    for (int64_t d : x->dims) bond = std::max(bond, d);
    info[0] = count, info[1] = converged, info[2] = res, info[3] = (double)matvecs, info[4] = (double)bond;
    info[5] = (double)n_local, info[6] = (double)n_gemm;
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
