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
// All three files include this header; the host steps declared here are defined once, in qil_twosite.hip.
// Here: that matvec inside one workgroup on LDS operands (local_matvec) and as four f64-MFMA GEMMs (Sweep::gemm_matvec), its
// multiply-add count, the environments of <x|A|x> and of the overlaps <x|phi_i> with further states (the right-hand side of the
// solver, the deflation states of the eigen-solver) and how they grow by one tensor (Sweep::extend), the projection of such a
// state onto the local space, g_i = Lphi phi_k phi_{k+1} Rphi, by three small GEMMs (Sweep::overlap_local), the SVD split of
// the two-site tensor under the project's truncation rule (Sweep::split), and the frame every verb builds its local problem in:
// the route decision (local_route_fits, frame_elems, local_bytes), the argument fields, the staging and the launch of the
// one-workgroup kernels (FrameArgs, stage_frame, Sweep::launch_local), the work blocks and the helper launches of the gemm
// routes (Sweep::Work, Sweep::launch_wg) and the verbs' tails (sweep_until, Sweep::info_head).
#pragma once

#include "qil_internal.h"
#include "qil_device_utils.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace qil_twosite {

using namespace qil_dev;

constexpr int kThreads = 256;
constexpr long long kLdsBudget = 160 * 1024;        // one workgroup may claim all of it
constexpr long long kRedBytes = 128;                // block_sum's scratch, at the base
// The solver's cap: beyond this nothing fits.  It stays wider than kKrylovDimCap: cl does not enter the solver's LDS formula, so
// the narrower cap would change its answer for cl in (2^14, 2^20].
constexpr long long kDimCap = 1 << 20;
// The cap of the eigen-solver and of the evolution: one dimension beyond this alone needs more than 160 KiB (8 * 2^14 * 4 bytes in
// every term it enters), and below it every term of the byte and multiply-add formulas stays under 2^50: no overflow for any
// arguments of the public host entries
constexpr long long kKrylovDimCap = 1 << 14;
constexpr int kMaxKrylov = 16;
constexpr double kBreakdown = 1e-14;                // beta <= kBreakdown * scale: the Krylov space is invariant

// The auto rule of every verb's fit.  One full sweep of the solver, local vs gemm, same operands (tools/_solve_time.py, median of 10,
// one MI355X, ms, 40 tensors, f64 / c64): chi 4, D 2 .. 8: 10.9 - 13.1 vs 22.8 - 26.5 / 12.8 - 15.5 vs 28.2 - 34.7; chi 8, D 8 (98 k
// multiply-adds per matvec): 30.0 vs 39.1 / 38.4 vs 52.0; chi 16, D 3 (135 k): 47.5 vs 52.2; chi 16, D 5 (266 k, f64 only: c64 does
// not fit): 81.4 vs 71.9, and 17.1 vs 16.1 at 12 tensors -- the one workgroup loses once a matvec is a quarter of a million
// multiply-adds, whatever the element type (the products are latency-bound).  So auto takes the local route up to 200 k (the
// two-site count, or the one-site count for the evolution's one-site step); QIL_*_ROUTE=local takes it wherever it fits.
constexpr long long kLocalMaxMacs = 200000;

// multiply-adds of one matvec (the four products): what the single workgroup of a local route runs through per iteration
inline long long local_matvec_macs(long long xl, long long xr, long long dl, long long dm, long long dr) {
    return xl * dl * 4 * xr * xl + xl * 2 * dm * 2 * xr * 2 * dl + 2 * xl * 2 * dr * xr * 2 * dm + 4 * xl * xr * dr * xr;
}

enum { ROUTE_AUTO = 0, ROUTE_LOCAL = 1, ROUTE_GEMM = 2 };
inline int route_from(const char* r) {            // the value of QIL_SOLVE_ROUTE / QIL_EIGS_ROUTE / QIL_EVOLVE_ROUTE
    if (r && !strcmp(r, "local")) return ROUTE_LOCAL;
    if (r && !strcmp(r, "gemm")) return ROUTE_GEMM;
    return ROUTE_AUTO;
}
// The route rule of the three *_local_fits entries: 1 when the variable does not say gemm, no argument is over the verb's cap, the
// kernel's LDS is within the budget and -- unless the variable says local -- a matvec stays within kLocalMaxMacs multiply-adds.
// Over the cap the byte and multiply-add counts are not looked at (their formulas may have overflowed).
inline int local_route_fits(const char* env, bool over_cap, long long lds_bytes, long long macs) {
    const int route = route_from(env);
    if (route == ROUTE_GEMM || over_cap || lds_bytes > kLdsBudget) return 0;
    return route == ROUTE_LOCAL || macs <= kLocalMaxMacs ? 1 : 0;
}
// elements of the operands every local kernel stages: both environments and the operator tensor(s)
inline long long frame_elems(int sites, long long xl, long long xr, long long dl, long long dm, long long dr) {
    return xl * xl * dl + xr * xr * dr + (sites == 2 ? 4 * dl * dm + 4 * dm * dr : 4 * dl * dr);
}
// LDS bytes of a local kernel: block_sum's scratch, the verb's small area, the frame, n_vec vectors of nv and two ping-pong blocks
inline long long local_bytes(bool cx, long long small, long long frame, long long n_vec, long long nv, long long blk) {
    return kRedBytes + small + (cx ? 16 : 8) * (frame + n_vec * nv + 2 * blk);
}

// sum over the workgroup of one double per thread, the same value in every thread (it went through LDS)
__device__ __forceinline__ double wg_sum(double v, double* red) {
    double a[1] = {v};
    block_sum<1>(a, red);
    return a[0];
}

// The argument fields every local kernel has; its own struct derives from this one, so local_matvec finds g.xl .. g.shift.
struct FrameArgs {
    const void *LA, *RA, *A0, *A1;     // environments (TE), operator tensor(s) (TA); A1 unused for one site
    double shift;                      // the matvec's identity term
    void* y;                           // the local tensor (TE): the start on entry, the result on return
    double* stat;                      // what the kernel reports
    int xl, xr, dl, dm, dr;
    int blk;                           // elements of one ping-pong block
};
// What stage_frame hands back: the staged operands and v, the start vector (nv elements), which is the first free element
template <class TE>
struct Frame {
    TE *Ls, *Rs, *W0, *W1, *v;
};
// Carves Ls, Rs, W0, W1 and the start vector from `lds` on and stages them: the environments, the operator tensor(s), widened on
// the way, and g.y.  No barrier.
template <class TA, class TE, int SITES>
__device__ __forceinline__ Frame<TE> stage_frame(const FrameArgs& g, unsigned char* lds) {
    const int xl = g.xl, xr = g.xr, dl = g.dl, dm = g.dm, dr = g.dr, nv = (SITES == 2 ? 4 : 2) * xl * xr;
    const int n0 = SITES == 2 ? 4 * dl * dm : 4 * dl * dr, n1 = SITES == 2 ? 4 * dm * dr : 0;
    Frame<TE> f;
    f.Ls = reinterpret_cast<TE*>(lds);
    f.Rs = f.Ls + xl * dl * xl;
    f.W0 = f.Rs + xr * dr * xr;
    f.W1 = f.W0 + n0;
    f.v = f.W1 + n1;
    const TE* LA = static_cast<const TE*>(g.LA);
    const TE* RA = static_cast<const TE*>(g.RA);
    const TA* A0 = static_cast<const TA*>(g.A0);
    const TA* A1 = static_cast<const TA*>(g.A1);
    const TE* y0 = static_cast<const TE*>(g.y);
    for (int t = threadIdx.x; t < xl * dl * xl; t += kThreads) f.Ls[t] = LA[t];
    for (int t = threadIdx.x; t < xr * dr * xr; t += kThreads) f.Rs[t] = RA[t];
    for (int t = threadIdx.x; t < n0; t += kThreads) f.W0[t] = cast_elem<TE>(A0[t]);
    for (int t = threadIdx.x; t < n1; t += kThreads) f.W1[t] = cast_elem<TE>(A1[t]);
    for (int t = threadIdx.x; t < nv; t += kThreads) f.v[t] = y0[t];
    return f;
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

// The unit start of a local problem: V = y / |y| (y may be V), returns |y|; bad: |y| is zero or not finite, and V = 0 y then.
template <class TE>
__device__ __forceinline__ double unit_start(const TE* y, TE* V, int nv, double* red, bool& bad) {
    const double ynorm = wg_norm<TE>(y, nv, red);
    bad = !(ynorm > 0.0) || !isfinite(ynorm);
    const double f = bad ? 0.0 : 1.0 / ynorm;
    for (int t = threadIdx.x; t < nv; t += kThreads) V[t] = scale_t(y[t], f);
    return ynorm;
}
// the next Lanczos vector vn = w / beta, on the thread's own elements
template <class TE>
__device__ __forceinline__ void next_vector(TE* vn, const TE* w, int nv, double beta) {
    const double f = 1.0 / beta;
    for (int t = threadIdx.x; t < nv; t += kThreads) vn[t] = scale_t(w[t], f);
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

    // the dimensions of a local problem: the two-site tensor of bond j (sites 2) or the tensor j (sites 1)
    struct Dims {
        int64_t xl, xr, dl, dm, dr;
    };
    Dims dims_of(int sites, int64_t j) const {
        if (sites == 2) return {xd(j), xd(j + 2), ad(j), ad(j + 1), ad(j + 2)};
        return {xd(j), xd(j + 1), ad(j), ad(j + 1), ad(j + 1)};
    }

    // ---- local routes
    // the shared argument fields of the local problem (sites, j): shift 0 and blk = nv max(dl, dm, dr), for the verb to overwrite
    // (dimensions and blk as int: the caller has the verb's fits decision behind it, or checks its lds against kLdsBudget before the launch)
    FrameArgs frame(int sites, int64_t j, void* y, void* stat) const;

    // One launch of the one-workgroup kernel `Kernel` with lds bytes of LDS, then its `words` doubles at g.stat read back to hst.
    // Keyed on the kernel's VALUE: all instantiations of one kernel template share a pointer type, and the grant of
    // MaxDynamicSharedMemorySize is per kernel.
    template <auto Kernel, class Args>
    int launch_local(const Args& g, size_t lds, int words, double* hst) {
        static qil_lds_grant grant;
        QIL_HIP(grant.ensure(ctx->device, reinterpret_cast<const void*>(Kernel), lds));
        hipLaunchKernelGGL(Kernel, dim3(1), dim3(kThreads), lds, qil_stream(ctx), g);
        QIL_HIP(hipGetLastError());
        uint64_t ticket = 0;
        QIL_TRY(qil_read_back_post(ctx, g.stat, (size_t)words * sizeof(double), &ticket));
        return qil_read_back_wait(ctx, ticket, hst, (size_t)words * sizeof(double));
    }

    // ---- gemm routes
    // The blocks of a gemm route for the local problem (sites, j): T1, T2 (blk elements each) and H (nv) of the matvec, the Krylov
    // basis V (krylov x nv, zeroed; none with krylov = 0) and the operator tensor(s) as operands in dt, A0 / A1 (Aw0 / Aw1: their
    // widened copies where the operator is real and dt complex).  A failed call leaves what it has to the qil_scratch.
    struct Work {
        void *T1 = nullptr, *T2 = nullptr, *H = nullptr, *V = nullptr, *Aw0 = nullptr, *Aw1 = nullptr;
        const void *A0 = nullptr, *A1 = nullptr;
    };
    int work_alloc(int sites, int64_t j, long long blk, int krylov, Work* w);
    void work_free(const Work& w);

    // One workgroup of the helper kernel kernel_of(element of dt) on the context's stream; pointer arguments are given untyped and
    // take the kernel's parameter types.
    template <class K, class... Args>
    int launch_wg(K kernel_of, Args... args) {
        for_elem_type(dt == QIL_C64, [&](auto t) {
            launch_as(kernel_of(t), args...);
            return 0;
        });
        QIL_HIP(hipGetLastError());
        return QIL_OK;
    }
    template <class... P, class... Args>
    void launch_as(void (*kernel)(P...), Args... args) {
        hipLaunchKernelGGL(kernel, dim3(1), dim3(kThreads), 0, qil_stream(ctx), wg_arg<P>(args)...);
    }
    // an untyped pointer becomes the parameter's pointer type; anything else is passed as it is, so a number in a pointer's place
    // (or the reverse, or a pointer of another type) does not compile
    template <class P, class A>
    static auto wg_arg(A a) {
        if constexpr (std::is_pointer_v<P> && std::is_pointer_v<A>) return static_cast<P>(a);
        else return a;
    }

    // info[0 .. 6] of every verb: sweeps or steps, converged, residual or worst estimate, matvecs, widest bond, local and gemm solves
    void info_head(double* info, double count, double converged, double res) const;
};

// go(operand element, work element) for the pairs a sweep has: dt is complex wherever the operand is, so a real sweep has a real
// operand and only a complex one switches on the operand's type.
template <class F>
int for_sweep_types(bool complex_op, bool complex_dt, F go) {
    if (!complex_dt) return go(double{}, double{});
    return for_elem_type(complex_op, [&](auto a) { return go(a, c64{}); });
}

// Sweeps until the worst local residual of a sweep (res, which sweep() sets) is within tol, max_sweeps times at most.
template <class F>
int sweep_until(F sweep, const double& res, double tol, int max_sweeps, int* sweeps, int* converged) {
    for (*sweeps = 0, *converged = 0; *sweeps < max_sweeps && !*converged;) {
        QIL_TRY(sweep());
        ++*sweeps;
        *converged = res <= tol;
    }
    return QIL_OK;
}

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
