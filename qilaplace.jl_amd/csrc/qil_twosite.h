// What the alternating two-site sweeps share (qil_solve.hip: the linear solver, qil_eigs.hip: the eigen-solver, qil_evolve.hip: time
// evolution, which adds a one-site step: local_matvec1 and Sweep::gemm_matvec1, and shares the Lanczos step and the small
// tridiagonal eigen-solver with the eigen-solver: lanczos_step, tridiagonal_eig).  x is kept in an
// orthonormal gauge around the bond k being worked on; with the environments L_A[p, a, s], R_A[q, b, l] of <x|A|x> (conventions of
// qil_environment: the bra is conj(x) and contracts the operator's s_out) the local operator on the two-site tensor
// y[p, s1, s2, q] = x_k x_{k+1} is four dependent products (the operands lie so that none needs a layout copy):
//     T1[p, a, s1, s2, l]   = sum_k      L_A[p, a, k] v[k, s1, s2, l]
//     T2[p, t1, m, s2, l]   = sum_{a,s1} T1[p, a, s1, s2, l] A_k[a, s1, t1, m]
//     T3[p, t1, t2, b, l]   = sum_{m,s2} T2[p, t1, m, s2, l] A_{k+1}[m, s2, t2, b]
//     (Hv)[p, t1, t2, q]    = sum_{b,l}  T3[p, t1, t2, b, l] R_A[q, b, l]
// All three files include this header; the host steps declared here are defined once, in qil_solve.hip.
// Here: that matvec inside one workgroup on LDS operands (local_matvec) and as four f64-MFMA GEMMs (Sweep::gemm_matvec), its
// multiply-add count, the environments of <x|A|x> and of the overlaps <x|phi_i> with further states (the right-hand side of the
// solver, the deflation states of the eigen-solver) and how they grow by one tensor (Sweep::extend), the projection of such a
// state onto the local space, g_i = Lphi phi_k phi_{k+1} Rphi, by three small GEMMs (Sweep::overlap_local), and the SVD split of
// the two-site tensor under the project's truncation rule (Sweep::split).
#pragma once

#include "qil_internal.h"
#include "qil_device_utils.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace qil_twosite {

using namespace qil_dev;

constexpr int kThreads = 256;
constexpr long long kLdsBudget = 160 * 1024;        // one workgroup may claim all of it
constexpr long long kRedBytes = 128;                // block_sum's scratch, at the base
constexpr long long kDimCap = 1 << 20;              // the solver's cap: beyond this nothing fits

// multiply-adds of one matvec (the four products): what the single workgroup of a local route runs through per iteration
inline long long local_matvec_macs(long long xl, long long xr, long long dl, long long dm, long long dr) {
    return xl * dl * 4 * xr * xl + xl * 2 * dm * 2 * xr * 2 * dl + 2 * xl * 2 * dr * xr * 2 * dm + 4 * xl * xr * dr * xr;
}

enum { ROUTE_AUTO = 0, ROUTE_LOCAL = 1, ROUTE_GEMM = 2 };
inline int route_from(const char* r) {            // the value of QIL_SOLVE_ROUTE / QIL_EIGS_ROUTE
    if (r && !strcmp(r, "local")) return ROUTE_LOCAL;
    if (r && !strcmp(r, "gemm")) return ROUTE_GEMM;
    return ROUTE_AUTO;
}

// sum over the workgroup of one double per thread, the same value in every thread (it went through LDS)
__device__ __forceinline__ double wg_sum(double v, double* red) {
    double a[1] = {v};
    block_sum<1>(a, red);
    return a[0];
}

// out (block Y) = H v + shift v, v in LDS; X, Y the ping-pong blocks; g carries xl, xr, dl, dm, dr and shift.  Ends behind a barrier.
template <class TE, class G>
__device__ __forceinline__ void local_matvec(const G& g, const TE* Ls, const TE* Rs, const TE* W0, const TE* W1, const TE* v, TE* X,
                                             TE* Y) {
    const int xl = g.xl, xr = g.xr, dl = g.dl, dm = g.dm, dr = g.dr;
    const int PA = xl * dl;
    for (int t = threadIdx.x; t < PA * 4 * xr; t += kThreads) {          // T1 -> X
        const int pa = t % PA, u = t / PA;
        const TE* vc = v + xl * u;
        TE acc{};
        for (int k = 0; k < xl; ++k) acc = cmul_add(acc, Ls[pa + PA * k], vc[k]);
        X[t] = acc;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < xl * 2 * dm * 2 * xr; t += kThreads) {   // T2 -> Y
        const int p = t % xl, u = t / xl, c = u % (2 * dm), bc = u / (2 * dm);
        const TE* t1 = X + p + xl * 2 * dl * bc;
        const TE* w = W0 + 2 * dl * c;
        TE acc{};
        for (int j = 0; j < 2 * dl; ++j) acc = cmul_add(acc, t1[xl * j], w[j]);
        Y[t] = acc;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * xl * 2 * dr * xr; t += kThreads) {   // T3 -> X
        const int pt = t % (2 * xl), u = t / (2 * xl), c = u % (2 * dr), l = u / (2 * dr);
        const TE* t2 = Y + pt + 2 * xl * 2 * dm * l;
        const TE* w = W1 + 2 * dm * c;
        TE acc{};
        for (int j = 0; j < 2 * dm; ++j) acc = cmul_add(acc, t2[2 * xl * j], w[j]);
        X[t] = acc;
    }
    __syncthreads();
    const TE sh = cast_elem<TE>(g.shift);
    for (int t = threadIdx.x; t < 4 * xl * xr; t += kThreads) {           // H v -> Y
        const int ptt = t % (4 * xl), q = t / (4 * xl);
        TE acc = cmul_add(TE{}, sh, v[t]);
        for (int j = 0; j < dr * xr; ++j) acc = cmul_add(acc, X[ptt + 4 * xl * j], Rs[q + xr * j]);
        Y[t] = acc;
    }
    __syncthreads();
}

// one-site counterpart: out (block X) = L_A A_j R_A v for the one-site tensor v[k, s, l] in LDS, three dependent products
//     T1[p, a, s, l] = sum_k L_A[p, a, k] v[k, s, l],  T2[p, t, b, l] = sum_{a,s} T1 A_j[a, s, t, b],  (Hv)[p, t, q] = sum_{b,l} T2 R_A[q, b, l]
// g carries xl, xr, dl, dr; X and Y hold 2 xl xr max(dl, dr) elements each.  Ends behind a barrier.
template <class TE, class G>
__device__ __forceinline__ void local_matvec1(const G& g, const TE* Ls, const TE* Rs, const TE* W0, const TE* v, TE* X, TE* Y) {
    const int xl = g.xl, xr = g.xr, dl = g.dl, dr = g.dr;
    const int PA = xl * dl;
    for (int t = threadIdx.x; t < PA * 2 * xr; t += kThreads) {            // T1 -> X
        const int pa = t % PA, u = t / PA;
        const TE* vc = v + xl * u;
        TE acc{};
        for (int k = 0; k < xl; ++k) acc = cmul_add(acc, Ls[pa + PA * k], vc[k]);
        X[t] = acc;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < xl * 2 * dr * xr; t += kThreads) {        // T2 -> Y
        const int p = t % xl, u = t / xl, c = u % (2 * dr), l = u / (2 * dr);
        const TE* t1 = X + p + xl * 2 * dl * l;
        const TE* w = W0 + 2 * dl * c;
        TE acc{};
        for (int j = 0; j < 2 * dl; ++j) acc = cmul_add(acc, t1[xl * j], w[j]);
        Y[t] = acc;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * xl * xr; t += kThreads) {             // H v -> X
        const int pt = t % (2 * xl), q = t / (2 * xl);
        TE acc{};
        for (int j = 0; j < dr * xr; ++j) acc = cmul_add(acc, Y[pt + 2 * xl * j], Rs[q + xr * j]);
        X[t] = acc;
    }
    __syncthreads();
}
inline long long local_matvec1_macs(long long xl, long long xr, long long dl, long long dr) {
    return xl * dl * 2 * xr * xl + xl * 2 * dr * xr * 2 * dl + 2 * xl * xr * dr * xr;
}

// ---- the Lanczos steps the eigen-solver and the exponential share, on vectors in LDS or in device memory
// <a|b> over the workgroup, the same bits in every thread
template <class TE>
__device__ __forceinline__ void wg_dot(const TE* a, const TE* b, int nv, double* red, double& re, double& im) {
    double s[2] = {0.0, 0.0};
    for (int t = threadIdx.x; t < nv; t += kThreads) dot_parts(a[t], b[t], s[0], s[1]);
    if constexpr (sizeof(TE) == 16) {
        block_sum<2>(s, red);
    } else {
        double one[1] = {s[0]};
        block_sum<1>(one, red);
        s[0] = one[0];
    }
    re = s[0], im = s[1];
}
template <class TE>
__device__ __forceinline__ double wg_norm(const TE* a, int nv, double* red) {
    double part = 0.0;
    for (int t = threadIdx.x; t < nv; t += kThreads) part += abs2_t(a[t]);
    return sqrt(wg_sum(part, red));
}
// w -= (cr + i ci) v on the thread's own elements
template <class TE>
__device__ __forceinline__ void axpy_own(TE* w, const TE* v, int nv, double cr, double ci) {
    const TE c = make_elem(-cr, -ci, (TE*)nullptr);
    for (int t = threadIdx.x; t < nv; t += kThreads) w[t] = cmul_add(w[t], c, v[t]);
}

// One Lanczos step: w holds the matvec of v_j on entry.  Adds the penalty of the n_ortho states G (none: n_ortho = 0), takes alpha_j, orthogonalises w twice against
// v_0 .. v_j (modified Gram-Schmidt; the coefficient against v_j of both passes is alpha_j) and returns beta_j = |w|.  Every thread
// works on its own elements t = threadIdx.x (mod 256) between the sums, and every sum hands all threads the same bits.
template <class TE>
__device__ __forceinline__ void lanczos_step(int j, int nv, const TE* V, TE* w, const TE* G, int n_ortho, double sw, double* red,
                                             double& alpha, double& beta) {
    const TE* vj = V + (size_t)j * nv;
    for (int i = 0; i < n_ortho; ++i) {
        const TE* gi = G + (size_t)i * nv;
        double cr, ci;
        wg_dot<TE>(gi, vj, nv, red, cr, ci);
        axpy_own<TE>(w, gi, nv, -sw * cr, -sw * ci);
    }
    alpha = 0.0;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i <= j; ++i) {
            const TE* vi = V + (size_t)i * nv;
            double cr, ci;
            wg_dot<TE>(vi, w, nv, red, cr, ci);
            axpy_own<TE>(w, vi, nv, cr, ci);
            if (i == j) alpha += cr;
        }
    beta = wg_norm<TE>(w, nv, red);
}

// Eigenpairs of the m x m tridiagonal matrix (alpha, beta) by cyclic Jacobi rotations, in plain C++ by ONE thread: T and Z are
// 16 x 16 work areas; on return the eigenvalues are the diagonal of T and the eigenvectors the columns of Z.
__device__ inline void tridiagonal_eig(int m, const double* alpha, const double* beta, double* T, double* Z) {
    for (int i = 0; i < m; ++i)
        for (int k = 0; k < m; ++k) {
            T[i * 16 + k] = i == k ? alpha[i] : ((i == k + 1) ? beta[k] : ((k == i + 1) ? beta[i] : 0.0));
            Z[i * 16 + k] = i == k ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < m; ++p) {
            diag += T[p * 16 + p] * T[p * 16 + p];
            for (int q = p + 1; q < m; ++q) off += T[p * 16 + q] * T[p * 16 + q];
        }
        if (!(off > 1e-34 * (diag + off))) break;                          // also leaves on a NaN
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = T[p * 16 + q];
                if (apq == 0.0) continue;
                const double zeta = (T[q * 16 + q] - T[p * 16 + p]) / (2.0 * apq);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < m; ++k) {                              // columns p, q
                    const double akp = T[k * 16 + p], akq = T[k * 16 + q];
                    T[k * 16 + p] = c * akp - s * akq;
                    T[k * 16 + q] = s * akp + c * akq;
                }
                for (int k = 0; k < m; ++k) {                              // rows p, q
                    const double apk = T[p * 16 + k], aqk = T[q * 16 + k];
                    T[p * 16 + k] = c * apk - s * aqk;
                    T[q * 16 + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < m; ++k) {
                    const double zkp = Z[k * 16 + p], zkq = Z[k * 16 + q];
                    Z[k * 16 + p] = c * zkp - s * zkq;
                    Z[k * 16 + q] = s * zkp + c * zkq;
                }
            }
    }
}

// The host side of a sweep: the working copy x, the environments and the steps that do not depend on the local problem.
struct Sweep {
    qil_context* ctx;
    qil_scratch& tmp;
    const qil_mpo* A;
    qil_mps* x;                        // the working copy, in dt; becomes the result
    int dt;
    size_t e;
    double cutoff = 0.0;
    int64_t maxdim = 1;
    int64_t n;
    std::vector<const qil_mps*> phi;   // the states whose overlaps with x are carried along
    std::vector<void*> LA, RA;         // [j]: LA contracts the tensors < j, RA the tensors >= j
    std::vector<std::vector<void*>> Lp, Rp;   // [i][j]: the same for <x|phi_i>
    long long matvecs = 0, n_local = 0, n_gemm = 0;
    double kept = 1.0;                 // the norm of the singular values the last split kept, before any rescaling

    Sweep(qil_context* ctx_, qil_scratch& tmp_, const qil_mpo* A_, qil_mps* x_, int dt_)
        : ctx(ctx_), tmp(tmp_), A(A_), x(x_), dt(dt_), e(qil_elem_size(dt_)), n(x_->n()) {}

    int64_t xd(int64_t j) const { return x->dims[(size_t)j]; }
    int64_t ad(int64_t j) const { return A->dims[(size_t)j]; }
    int64_t pd(size_t i, int64_t j) const { return phi[i]->dims[(size_t)j]; }

    int replace(std::vector<void*>& v, int64_t j, void* p) {
        if (v[(size_t)j]) tmp.free(v[(size_t)j]);
        v[(size_t)j] = p;
        return QIL_OK;
    }

    // the edge environments, then the right ones of a start in the left gauge (centre at tensor 0)
    int init_envs();

    // the environments grow by tensor j: LA[j + 1], Lp[i][j + 1] from the left, RA[j], Rp[i][j] from the right (the same steps on
    // REVERSED copies with the bonds exchanged, as qil_environment's GEMM route)
    int extend(int64_t j, bool right);

    // elements of the two blocks overlap_local works in
    long long overlap_block_elems(size_t i, int64_t k) const {
        return std::max(2 * xd(k) * pd(i, k + 1), 4 * xd(k) * pd(i, k + 2));
    }
    // out (4 xl xr) = Lp_i phi_k phi_{k+1} Rp_i, the projection of phi_i onto the local space of bond k; T1, T2: the call's blocks
    int overlap_local(size_t i, int64_t k, void* T1, void* T2, void* out);

    // out (nv) = L_A A_k A_{k+1} R_A v; A0, A1: the operator's tensors in dt; T1, T2: the call's blocks (4 xl xr max(dl, dm, dr))
    int gemm_matvec(int64_t k, const void* A0, const void* A1, const void* v, void* T1, void* T2, void* out);
    // the one-site counterpart at tensor j, three products: out (2 xl xr) = L_A A_j R_A v with LA[j] and RA[j + 1]; T1, T2: the
    // call's blocks (2 xl xr max(dl, dr))
    int gemm_matvec1(int64_t j, const void* A0, const void* v, void* T1, void* T2, void* out);

    // the two-site tensor of bond k (2 xl x 2 xr), a block of the call
    int two_site(int64_t k, void** y);

    // y (2 xl x 2 xr) is split by the SVD and cut by the project's rule; to_right: the isometry stays at k and S V^H moves on,
    // else U S moves to k.  unit: the kept singular values are rescaled to norm 1.  Frees y.
    int split(int64_t k, bool to_right, void* y, bool unit);

    // a full sweep: left to right, then right to left; step(k, to_right) is the local problem and its split
    template <class Step>
    int sweep(Step step) {
        for (int64_t k = 0; k + 1 < n; ++k) {
            QIL_TRY(step(k, true));
            if (k + 2 < n) QIL_TRY(extend(k, false));
        }
        for (int64_t k = n - 2; k >= 0; --k) {
            QIL_TRY(step(k, false));
            if (k >= 1) QIL_TRY(extend(k + 1, true));
        }
        return QIL_OK;
    }
};

// The start of a sweep: src copied into a fresh chain of dt (amplitude as given; start_chain), then cut to maxdim where it is
// wider and left in the gauge whose centre is tensor 0 (start_gauge).
inline int start_chain(qil_context* ctx, const qil_mps* src, int dt, double amplitude, qil_mps** out) {
    const int64_t n = src->n();
    qil_mps* xh = nullptr;
    QIL_TRY(qil_mps_alloc(ctx, n, dt, src->paired, src->dims.data() + 1, src->site_ids.data(), amplitude, &xh));
    qil_result_guard<qil_mps> own(xh);
    for (int64_t i = 0; i < n; ++i) QIL_TRY(qil_put_mps_site(ctx, dt, src, i, QIL_SITE_PLAIN, xh->site[(size_t)i]));
    *out = own.release();
    return QIL_OK;
}
int start_gauge(qil_mps* xh, int64_t maxdim);

}  // namespace qil_twosite
