// Environments: the partial contraction E[p, a, s] of `count` tensors of <phi|psi> or <phi|W|psi> with the bond legs open
// (qil_environment) -- what the overlap verbs of qil_inner.hip carry from site to site and never return.  Conventions of
// qil_apply_inner: the bra is conj(phi) and contracts the operator's s_out, the ket psi contracts s_in; amplitudes are not applied.
//
//   chain route   ONE launch, one workgroup (env_chain): the environment stays in LDS for the whole walk, in either direction by
//                 index arithmetic while a site is staged into LDS; state bonds <= 16, operator bonds <= QIL_ENV_CHAIN_MAX_OP_BOND
//   GEMM route    the per-site products of qil_inner / qil_apply_inner (qil_overlap_env_step, qil_apply_overlap_env_step of
//                 qil_contract.hip), on REVERSED site copies for the right-to-left walk; any bonds
//
// Every temporary belongs to the call's qil_scratch.
#include "qil_internal.h"
#include "qil_device_utils.h"

#include <algorithm>
#include <cstdlib>

namespace {

using namespace qil_dev;

struct EnvSite {
    const void* P;   // phi site (pl, 2, pr)
    const void* W;   // operator site (dl, 2, 2, dr), null without an operator
    const void* S;   // psi site (sl, 2, sr)
    int pl, pr, dl, dr, sl, sr;
};
constexpr int kThreads = 256;
constexpr int kStateMax = 16;                          // qil_inner's chain cap
constexpr int kOpMax = QIL_ENV_CHAIN_MAX_OP_BOND;
constexpr int kStatePer = 2 * kStateMax * kStateMax / kThreads;   // elements of a staged state site per thread (registers)
constexpr int kOpPer = 4 * kOpMax * kOpMax / kThreads;
static_assert(kStatePer * kThreads == 2 * kStateMax * kStateMax && kOpPer * kThreads == 4 * kOpMax * kOpMax, "staging registers");

// Element g of a site as it lies, (l, phys, r) with np physical values -> its place in the walk's layout (in, phys, out):
// the site itself left to right, (r, phys, l) right to left.
__device__ __forceinline__ int walk_index(int g, int L, int R, int np, int side) {
    if (side == QIL_ENV_LEFT) return g;
    const int l = g % L, u = g / L;
    return u / np + R * (u % np + np * l);
}
template <class T, class TE, int PER>
__device__ __forceinline__ void site_fetch(const T* __restrict__ g, int total, TE (&r)[PER]) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int t = threadIdx.x + j * kThreads;
        if (t < total) r[j] = cast_elem<TE>(g[t]);
    }
}
template <class TE, int PER>
__device__ __forceinline__ void site_stage(TE* lds, int total, int L, int R, int np, int side, bool conj, const TE (&r)[PER]) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int t = threadIdx.x + j * kThreads;
        if (t < total) lds[walk_index(t, L, R, np, side)] = conj ? conj_t(r[j]) : r[j];
    }
}

// One workgroup walks `count` sites, tab[0] first.  With (pi, di, si) the bonds the walk enters a site by and (po, dq, so) the ones
// it leaves by, per site and in the contraction type TE (operands are widened while they are staged):
//   T1[p, a, x, beta]  = sum_k  E[p, a, k] A_psi[k, x, beta]                          inner length si
//   T2[p, y, b, beta]  = sum_x sum_a T1[p, a, x, beta] W[a, x, y, b]                  inner length 2 di      (HASW; else T2 = T1)
//   E'[q, b, beta]     = sum_y sum_p conj(A_phi[p, y, q]) T2[p, y, b, beta]           inner length 2 pi
// X and Y are two LDS blocks in ping-pong (E in X, T1 in Y, T2 in X, E' in Y, then swapped; without an operator E' returns to
// X); As, Ps, Ws hold the site's operands in the walk's layout.  The next site's ket and operator are fetched into registers
// ahead of the third product and staged behind it, the bra ahead of the first: one global latency per site, behind arithmetic.
// Every barrier is reached by all threads: the loops around them have uniform bounds.
template <class TP, class TW, class TS, class TE, bool HASW>
__global__ __launch_bounds__(kThreads) void env_chain(const EnvSite* __restrict__ tab, int count, int side, int blk, int nstate,
                                                      c64* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    TE* X = reinterpret_cast<TE*>(lds_raw);
    TE* Y = X + blk;
    TE* As = Y + blk;
    TE* Ps = As + nstate;
    TE* Ws = Ps + nstate;
    TE rA[kStatePer], rP[kStatePer], rW[kOpPer];
    {
        const EnvSite S = tab[0];
        site_fetch(static_cast<const TS*>(S.S), 2 * S.sl * S.sr, rA);
        if constexpr (HASW) site_fetch(static_cast<const TW*>(S.W), 4 * S.dl * S.dr, rW);
        site_stage(As, 2 * S.sl * S.sr, S.sl, S.sr, 2, side, false, rA);
        if constexpr (HASW) site_stage(Ws, 4 * S.dl * S.dr, S.dl, S.dr, 4, side, false, rW);
        if (threadIdx.x == 0) X[0] = cast_elem<TE>(1.0);
    }
    __syncthreads();
    int nE = 1;
    for (int i = 0; i < count; ++i) {
        const EnvSite S = tab[i];
        const bool left = side == QIL_ENV_LEFT;
        const int pi = left ? S.pl : S.pr, po = left ? S.pr : S.pl;
        const int di = left ? S.dl : S.dr, dq = left ? S.dr : S.dl;
        const int si = left ? S.sl : S.sr, so = left ? S.sr : S.sl;
        const int PA = pi * di;
        // ---- T1 = E A_psi (X -> Y); the bra site on its way
        site_fetch(static_cast<const TP*>(S.P), 2 * S.pl * S.pr, rP);
        const int nT1 = PA * 2 * so;
        for (int t = threadIdx.x; t < nT1; t += kThreads) {
            const int pa = t % PA, u = t / PA;               // u = x + 2 beta
            const TE* a = As + si * u;
            TE v{};
            for (int k = 0; k < si; ++k) v = cmul_add(v, X[pa + PA * k], a[k]);
            Y[t] = v;
        }
        site_stage(Ps, 2 * S.pl * S.pr, S.pl, S.pr, 2, side, true, rP);
        __syncthreads();
        TE* T2 = Y;
        TE* En = X;
        if constexpr (HASW) {
            // ---- T2 = T1 W (Y -> X)
            const int nT2 = pi * 2 * dq * so;
            for (int t = threadIdx.x; t < nT2; t += kThreads) {
                const int p = t % pi, u = t / pi, y = u & 1, v2 = u >> 1, b = v2 % dq, beta = v2 / dq;
                TE v{};
                for (int x = 0; x < 2; ++x) {
                    const TE* t1 = Y + p + pi * di * (x + 2 * beta);
                    const TE* w = Ws + di * (x + 2 * (y + 2 * b));
                    for (int a = 0; a < di; ++a) v = cmul_add(v, t1[pi * a], w[a]);
                }
                X[t] = v;
            }
            __syncthreads();
            T2 = X;
            En = Y;
        }
        // ---- E' = A_phi^H T2; the next site's ket and operator on their way
        const bool more = i + 1 < count;
        EnvSite N = S;
        if (more) {
            N = tab[i + 1];
            site_fetch(static_cast<const TS*>(N.S), 2 * N.sl * N.sr, rA);
            if constexpr (HASW) site_fetch(static_cast<const TW*>(N.W), 4 * N.dl * N.dr, rW);
        }
        nE = po * dq * so;
        const int J = 2 * pi;
        for (int t = threadIdx.x; t < nE; t += kThreads) {
            const int q = t % po, u = t / po;                // u = b + dq beta
            const TE* pc = Ps + J * q;
            const TE* tc = T2 + J * u;
            TE v{};
            for (int j = 0; j < J; ++j) v = cmul_add(v, pc[j], tc[j]);
            En[t] = v;
        }
        if (more) {
            site_stage(As, 2 * N.sl * N.sr, N.sl, N.sr, 2, side, false, rA);
            if constexpr (HASW) site_stage(Ws, 4 * N.dl * N.dr, N.dl, N.dr, 4, side, false, rW);
        }
        __syncthreads();
        if constexpr (HASW) {
            TE* t = X;
            X = Y;
            Y = t;
        }
    }
    for (int t = threadIdx.x; t < nE; t += kThreads) out[t] = to_c64(X[t]);
}

// the bonds of the walked tensors: dims[lo .. hi]
static void walked_span(int side, int64_t count, int64_t n, int64_t* lo, int64_t* hi) {
    *lo = side == QIL_ENV_LEFT ? 0 : n - count;
    *hi = side == QIL_ENV_LEFT ? count : n;
}
static long long span_max(const int64_t* dims, int64_t lo, int64_t hi) {
    long long m = 1;
    for (int64_t i = lo; i <= hi; ++i) m = std::max<long long>(m, dims[i]);
    return m;
}

// Crossover between the routes: the chain wherever it fits (state bonds <= 16, qil_inner's chain cap; operator bonds
// <= QIL_ENV_CHAIN_MAX_OP_BOND, the LDS budget).  Measured on a right walk of a 40-tensor chain (tools/_environment_time.py, median
// of 10, chain vs GEMM, f64 / c64): chi 4, 38 tensors 0.09 / 0.09 ms vs 0.47 / 0.53 ms; chi 16, no operator, 38 tensors 0.20 / 0.27 vs
// 0.47 / 0.61; chi 16, operator of bond 2, 38 tensors 0.36 / 0.52 vs 0.71 / 0.88, 12 tensors 0.13 / 0.17 vs 0.25 / 0.30 -- the chain
// loses nowhere inside its caps, so the threshold inherited from qil_inner stays.
// QIL_ENV_ROUTE=chain / gemm forces one (read per call; the chain route only where its bonds fit).
static int env_route(int side, int64_t count, int64_t n, const int64_t* phi_dims, const int64_t* psi_dims, const int64_t* op_dims) {
    int64_t lo, hi;
    walked_span(side, count, n, &lo, &hi);
    const bool fits = span_max(phi_dims, lo, hi) <= kStateMax && span_max(psi_dims, lo, hi) <= kStateMax &&
                      (!op_dims || span_max(op_dims, lo, hi) <= kOpMax);
    bool chain = fits;
    const char* route = getenv("QIL_ENV_ROUTE");
    if (route && !strcmp(route, "gemm")) chain = false;
    return chain ? QIL_ROUTE_CHAIN : QIL_ROUTE_GEMM_SELECT;
}

template <class TP, class TW, class TS, class TE, bool HASW>
static int launch_env_chain(qil_context* ctx, const EnvSite* dtab, int count, int side, int blk, int nstate, int nop, c64* dout) {
    static qil_lds_grant grant;
    const size_t lds = ((size_t)2 * blk + 2 * nstate + nop) * sizeof(TE);
    QIL_HIP(grant.ensure(ctx->device, reinterpret_cast<const void*>(&env_chain<TP, TW, TS, TE, HASW>), lds));
    hipLaunchKernelGGL((env_chain<TP, TW, TS, TE, HASW>), dim3(1), dim3(kThreads), lds, qil_stream(ctx), dtab, count, side, blk, nstate,
                       dout);
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

// site index of step j of the walk
static int64_t walk_site(int side, int64_t n, int64_t j) { return side == QIL_ENV_LEFT ? j : n - 1 - j; }

static int env_chain_route(const qil_mps* phi, const qil_mpo* W, const qil_mps* psi, int side, int64_t count, int64_t nout, void* dout) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    int64_t lo, hi;
    walked_span(side, count, n, &lo, &hi);
    const long long mp = span_max(phi->dims.data(), lo, hi), ms = span_max(psi->dims.data(), lo, hi);
    const long long md = W ? span_max(W->dims.data(), lo, hi) : 1;
    QIL_REQUIRE(mp <= kStateMax && ms <= kStateMax && md <= kOpMax, QIL_EINVAL_ARG, "environment: the chain route does not hold these bonds");
    // every block of a site: E, E' <= mp md ms; T1, T2 <= 2 mp md ms
    const int blk = (int)(2 * mp * md * ms), nstate = (int)(2 * std::max(mp * mp, ms * ms)), nop = W ? (int)(4 * md * md) : 0;
    QIL_REQUIRE(nout <= blk, QIL_EINVAL_ARG, "environment: output larger than the chain's block");
    std::vector<EnvSite> tab((size_t)count);
    for (int64_t j = 0; j < count; ++j) {
        const size_t i = (size_t)walk_site(side, n, j);
        tab[(size_t)j] = EnvSite{phi->site[i], W ? W->site[i] : nullptr, psi->site[i], (int)phi->dims[i], (int)phi->dims[i + 1],
                                 W ? (int)W->dims[i] : 1, W ? (int)W->dims[i + 1] : 1, (int)psi->dims[i], (int)psi->dims[i + 1]};
    }
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(EnvSite)));
    const EnvSite* t = dtab.as<EnvSite>();
    c64* o = static_cast<c64*>(dout);
    const bool pc = phi->dtype == QIL_C64, sc = psi->dtype == QIL_C64, wc = W && W->dtype == QIL_C64;
    const int c = (int)count;
    if (!(pc || sc || wc)) {
        if (W) QIL_TRY((launch_env_chain<double, double, double, double, true>(ctx, t, c, side, blk, nstate, nop, o)));
        else QIL_TRY((launch_env_chain<double, double, double, double, false>(ctx, t, c, side, blk, nstate, nop, o)));
    } else if (!W) {
        QIL_TRY(for_elem_types(pc, sc, [&](auto p, auto s) {
            return launch_env_chain<decltype(p), double, decltype(s), c64, false>(ctx, t, c, side, blk, nstate, nop, o);
        }));
    } else {
        QIL_TRY(for_elem_types(pc, sc, [&](auto p, auto s) {
            return for_elem_type(wc, [&](auto w) {
                return launch_env_chain<decltype(p), decltype(w), decltype(s), c64, true>(ctx, t, c, side, blk, nstate, nop, o);
            });
        }));
    }
    return dtab.release();
}

// The walk of qil_inner / qil_apply_inner stopped after `count` sites; right to left it is the same step on REVERSED site copies
// with the left and right bonds exchanged.  dout receives the environment as complex doubles.
static int env_gemm_route(qil_scratch& tmp, const qil_mps* phi, const qil_mpo* W, const qil_mps* psi, int side, int64_t count, int dt,
                          int64_t nout, void* dout) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    const size_t e = qil_elem_size(dt);
    const bool right = side == QIL_ENV_RIGHT;
    long long maxE = 1, maxT = 1, maxP = 1, maxS = 1, maxW = 1;
    for (int64_t j = 0; j < count; ++j) {
        const size_t i = (size_t)walk_site(side, n, j);
        const long long pl = phi->dims[i], pr = phi->dims[i + 1], sl = psi->dims[i], sr = psi->dims[i + 1];
        const long long Dl = W ? W->dims[i] : 1, Dr = W ? W->dims[i + 1] : 1;
        maxE = std::max(maxE, std::max(pl * Dl * sl, pr * Dr * sr));
        maxT = std::max(maxT, 2 * std::max(pl, pr) * std::max(Dl, Dr) * std::max(sl, sr));
        maxP = std::max(maxP, pl * 2 * pr);
        maxS = std::max(maxS, sl * 2 * sr);
        maxW = std::max(maxW, Dl * 4 * Dr);
    }
    void *E = nullptr, *En = nullptr, *T1 = nullptr, *T2 = nullptr, *Pw = nullptr, *Sw = nullptr, *Ww = nullptr;
    QIL_TRY(tmp.alloc((size_t)maxE * e, &E));
    QIL_TRY(tmp.alloc((size_t)maxE * e, &En));
    QIL_TRY(tmp.alloc((size_t)maxT * e, &T1));
    if (W) QIL_TRY(tmp.alloc((size_t)maxT * e, &T2));
    if (right || dt != phi->dtype) QIL_TRY(tmp.alloc((size_t)maxP * e, &Pw));
    if (right || dt != psi->dtype) QIL_TRY(tmp.alloc((size_t)maxS * e, &Sw));
    if (W && (right || dt != W->dtype)) QIL_TRY(tmp.alloc((size_t)maxW * e, &Ww));
    QIL_TRY(qil_dev_fill_ones(ctx, dt, E, 1));
    for (int64_t j = 0; j < count; ++j) {
        const int64_t i = walk_site(side, n, j);
        const size_t u = (size_t)i;
        int64_t pi = phi->dims[u], po = phi->dims[u + 1], si = psi->dims[u], so = psi->dims[u + 1];
        int64_t di = W ? W->dims[u] : 1, dq = W ? W->dims[u + 1] : 1;
        const void *Ap = Pw, *As = Sw, *Wd = Ww;
        if (right) {
            std::swap(pi, po), std::swap(si, so), std::swap(di, dq);
            QIL_TRY(qil_put_mps_site(ctx, dt, phi, i, QIL_SITE_REVERSED, Pw));
            QIL_TRY(qil_put_mps_site(ctx, dt, psi, i, QIL_SITE_REVERSED, Sw));
            if (W) QIL_TRY(qil_put_mpo_site(ctx, dt, W, i, QIL_SITE_REVERSED, Ww));
        } else {
            QIL_TRY(qil_site_operand(ctx, dt, phi, i, Pw, &Ap));
            QIL_TRY(qil_site_operand(ctx, dt, psi, i, Sw, &As));
            if (W) QIL_TRY(qil_site_operand(ctx, dt, W, i, Ww, &Wd));
        }
        if (W) QIL_TRY(qil_apply_overlap_env_step(ctx, dt, pi, po, si, so, di, dq, Ap, As, Wd, E, T1, T2, En));
        else QIL_TRY(qil_overlap_env_step(ctx, dt, 2, pi, po, si, so, Ap, As, E, T1, En));
        std::swap(E, En);
    }
    return qil_dev_finish_coeff(ctx, dt, E, nout, 1.0, dout);
}

}  // namespace

extern "C" int qil_environment_route(int side, int64_t count, int64_t n, const int64_t* phi_dims, const int64_t* psi_dims,
                                     const int64_t* op_dims, int* route) {
    QIL_REQUIRE(phi_dims && psi_dims && route, QIL_EINVAL_ARG, "environment_route: null argument");
    QIL_REQUIRE(side == QIL_ENV_LEFT || side == QIL_ENV_RIGHT, QIL_EINVAL_ARG, "environment_route: side must be 0 (left) or 1 (right), got %d",
                side);
    QIL_REQUIRE(n >= 0 && count >= 0 && count <= n, QIL_EINVAL_ARG, "environment_route: count %lld outside [0, %lld]", (long long)count,
                (long long)n);
    *route = env_route(side, count, n, phi_dims, psi_dims, op_dims);
    return QIL_OK;
}

extern "C" int qil_environment(const qil_mps* phi, const qil_mpo* W, const qil_mps* psi, int side, int64_t count, double* out,
                               int64_t* dims) {
    QIL_REQUIRE(phi && psi && dims, QIL_EINVAL_ARG, "environment: null argument");
    QIL_REQUIRE(side == QIL_ENV_LEFT || side == QIL_ENV_RIGHT, QIL_EINVAL_ARG, "environment: side must be 0 (left) or 1 (right), got %d", side);
    QIL_REQUIRE(count >= 0 && count <= psi->n(), QIL_EINVAL_ARG, "environment: count %lld outside [0, %lld]", (long long)count,
                (long long)psi->n());
    if (W) QIL_TRY(qil_check_apply_operands(W, psi));
    QIL_TRY(qil_check_overlap_pair(phi, psi));
    const int64_t n = psi->n();
    const size_t open = (size_t)(side == QIL_ENV_LEFT ? count : n - count);      // the bond the walk stops at
    dims[0] = phi->dims[open];
    dims[1] = W ? W->dims[open] : 1;
    dims[2] = psi->dims[open];
    if (!out) return QIL_OK;                                                      // the size query
    const int64_t nout = dims[0] * dims[1] * dims[2];
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    if (count == 0) {                                                             // the boundary [1]
        out[0] = 1.0;
        out[1] = 0.0;
        return QIL_OK;
    }
    const int route = env_route(side, count, n, phi->dims.data(), psi->dims.data(), W ? W->dims.data() : nullptr);
    const int dt = (phi->dtype == QIL_C64 || psi->dtype == QIL_C64 || (W && W->dtype == QIL_C64)) ? QIL_C64 : QIL_F64;
    qil_scratch tmp(ctx);
    void* dout = nullptr;
    QIL_TRY(tmp.alloc((size_t)nout * 16, &dout));
    if (route == QIL_ROUTE_CHAIN) QIL_TRY(env_chain_route(phi, W, psi, side, count, nout, dout));
    else QIL_TRY(env_gemm_route(tmp, phi, W, psi, side, count, dt, nout, dout));
    return qil_download(ctx, out, dout, (size_t)nout * 16);
}
