// What the alternating two-site sweeps share (qil_solve.hip: the linear solver, qil_eigs.hip: the eigen-solver).  x is kept in an
// orthonormal gauge around the bond k being worked on; with the environments L_A[p, a, s], R_A[q, b, l] of <x|A|x> (conventions of
// qil_environment: the bra is conj(x) and contracts the operator's s_out) the local operator on the two-site tensor
// y[p, s1, s2, q] = x_k x_{k+1} is four dependent products (the operands lie so that none needs a layout copy):
//     T1[p, a, s1, s2, l]   = sum_k      L_A[p, a, k] v[k, s1, s2, l]
//     T2[p, t1, m, s2, l]   = sum_{a,s1} T1[p, a, s1, s2, l] A_k[a, s1, t1, m]
//     T3[p, t1, t2, b, l]   = sum_{m,s2} T2[p, t1, m, s2, l] A_{k+1}[m, s2, t2, b]
//     (Hv)[p, t1, t2, q]    = sum_{b,l}  T3[p, t1, t2, b, l] R_A[q, b, l]
// Both files include this header; the host steps declared here are defined once, in qil_solve.hip.
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
