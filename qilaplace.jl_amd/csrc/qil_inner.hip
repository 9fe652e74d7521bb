// Overlaps: <phi|psi> (qil_inner), norm(psi) (qil_norm), <phi|W psi> (qil_apply_inner) and norm(W psi) (qil_apply_norm),
// none of which forms a product or a dense vector.  Every call walks the chain left to right carrying one environment
// tensor (column-major, the boundary's convention) on the device; nothing crosses to the host between sites and the one
// value is read back at the end.
//
//   qil_inner        E[phi, psi]:            E' = A_phi^H (E A_psi)                         (GEMM route, any bonds)
//                                            the same contraction in ONE launch, E in LDS   (chain route, bonds <= 16)
//   qil_norm         E[psi, psi]:            the GEMM route of qil_inner with phi = psi
//   qil_mpo_inner    E[V, W]:                tr(V^H W): both routes of qil_inner with four physical slices per site instead of two
//   qil_apply_inner  E[phi, a, psi]:         T1 = E A_psi, T2_beta = T1_beta W, E' = A_phi^H T2
//   qil_apply_norm   E[psi', a', a, psi]:    ket A, ket W, bra conj(W), bra conj(A)
//
// Mixed dtypes contract in c64; a real operand is widened once per site into a scratch block (qil_site_operand).  The four
// products of qil_apply_norm are qil_norm_env_step (qil_contract.hip).  Every temporary belongs to the call's qil_scratch.
#include "qil_internal.h"
#include "qil_device_utils.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace {

using namespace qil_dev;

// the environment's last 1 x 1 value to the host
static int read_scalar(qil_context* ctx, int dt, const void* E, double h[2]) {
    h[0] = h[1] = 0.0;
    return qil_read_back(ctx, h, E, qil_elem_size(dt));
}

// ---- <phi|psi>: chain route -------------------------------------------------------------------------------------
struct InnerSite {
    const void* P;   // phi site  (pl, NS, pr): NS = 2 physical slices for states, 4 for operators (s_in + 2 s_out)
    const void* S;   // psi site  (sl, NS, sr)
    int pl, pr, sl, sr;
};
constexpr int kChainMax = 64;        // largest bond of either chain the one-workgroup route holds
constexpr int kChainThreads = 512;
constexpr int kChainPer = kChainMax * kChainMax / kChainThreads;   // entries of E' per thread (registers)

// One workgroup walks every site.  E (pl x sl) and one physical slice of T = E A_psi (pl x sr) live in LDS; E' (pr x sr)
// accumulates in registers over the NS slices and replaces E at the end of the site:
//   T_s[p, b]   = sum_k E[p, k] A_psi[k, s, b]
//   E'[q, b]   += sum_p conj(A_phi[p, s, q]) T_s[p, b]
template <class TP, class TS, class TE, int NS>
__global__ __launch_bounds__(kChainThreads) void inner_chain(const InnerSite* __restrict__ sites, int n, double amplitude,
                                                             c64* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    TE* E = reinterpret_cast<TE*>(lds_raw);
    TE* T = E + kChainMax * kChainMax;
    if (threadIdx.x == 0) E[0] = cast_elem<TE>(1.0);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const InnerSite S = sites[i];
        const TP* __restrict__ P = static_cast<const TP*>(S.P);
        const TS* __restrict__ A = static_cast<const TS*>(S.S);
        TE acc[kChainPer];
#pragma unroll
        for (int r = 0; r < kChainPer; ++r) acc[r] = TE{};
        const int nT = S.pl * S.sr, nE = S.pr * S.sr;
        for (int s = 0; s < NS; ++s) {
            for (int t = threadIdx.x; t < nT; t += kChainThreads) {
                const int p = t % S.pl, b = t / S.pl;
                const TS* col = A + (long long)S.sl * (s + NS * b);
                TE v{};
                for (int k = 0; k < S.sl; ++k) v = cmul_add(v, E[p + S.pl * k], col[k]);
                T[t] = v;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kChainPer; ++r) {
                const int t = threadIdx.x + r * kChainThreads;
                if (t < nE) {
                    const int q = t % S.pr, b = t / S.pr;
                    const TP* pc = P + (long long)S.pl * (s + NS * q);
                    const TE* tc = T + S.pl * b;
                    TE v = acc[r];
                    for (int p = 0; p < S.pl; ++p) v = cmul_add(v, conj_t(pc[p]), tc[p]);
                    acc[r] = v;
                }
            }
            // before the last slice: T is overwritten next; the last: every read of E (by its T products) happened before the
            // barrier above
            if (s + 1 < NS) __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < kChainPer; ++r) {
            const int t = threadIdx.x + r * kChainThreads;
            if (t < nE) E[t] = acc[r];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const c64 r = to_c64(E[0]);
        out[0] = c64{r.re * amplitude, r.im * amplitude};
    }
}

template <class TP, class TS, class TE, int NS>
static int launch_inner_chain(qil_context* ctx, const InnerSite* dtab, int n, double amp, c64* dout) {
    static qil_lds_grant grant;
    const size_t lds = 2 * (size_t)kChainMax * kChainMax * sizeof(TE);
    QIL_HIP(grant.ensure(ctx->device, reinterpret_cast<const void*>(&inner_chain<TP, TS, TE, NS>), lds));
    hipLaunchKernelGGL((inner_chain<TP, TS, TE, NS>), dim3(1), dim3(kChainThreads), lds, qil_stream(ctx), dtab, n, amp, dout);
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

// Crossover between the routes (bonds of both chains at most this: one launch).  Measured at n = 30 (f64 / c64, median of 10):
// chi 16 chain 0.15 / 0.20 ms vs GEMM 0.25 / 0.35 ms, chi 24 0.34 / 0.51 vs 0.31 / 0.46, chi 64 3.3 / 6.4 vs 0.31 / 0.40 -- past
// chi ~ 20 the one workgroup is bound by the arithmetic of ONE CU (2 chi^3 complex MACs per slice and site), not by launches.
// QIL_INNER_ROUTE=chain / gemm forces one (read per call; the chain route only where its bonds fit).
constexpr long long kChainAutoMax = 16;

// The operator overlap's crossover, measured at n = 24 tensors (f64 / c64, median of 10, tools/_mpo_algebra_time.py): D 8 chain
// 0.18 / 0.18 ms vs GEMM 0.20 / 0.29 ms, D 12 0.229 / 0.235 vs 0.230 / 0.339, D 16 0.31 / 0.32 vs 0.25 / 0.38, D 20 0.47 / 0.47 vs
// 0.30 / 0.48, D 24 0.88 / 0.89 vs 0.33 / 0.53, D 32 1.46 / 1.47 vs 0.24 / 0.31, D 64 11.2 / 12.3 vs 0.27 / 0.37.  12 is the largest
// bond at which the one workgroup is not slower in BOTH dtypes (at 16 it still wins in c64 and loses in f64): below the states'
// 16, as four slices instead of two double the one-CU arithmetic per site.  QIL_MPO_INNER_ROUTE=chain / gemm forces a route, as
// QIL_INNER_ROUTE does.
constexpr long long kMpoChainAutoMax = 12;

// phi, psi: two states (NS = 2) or two operators (NS = 4, amplitude 1)
template <int NS>
static int inner_chain_route(const qil_chain* phi, const qil_chain* psi, double h[2]) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    std::vector<InnerSite> tab((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        tab[(size_t)i] = InnerSite{phi->site[(size_t)i], psi->site[(size_t)i], (int)phi->dims[(size_t)i], (int)phi->dims[(size_t)i + 1],
                                   (int)psi->dims[(size_t)i], (int)psi->dims[(size_t)i + 1]};
    qil_scratch tmp(ctx);
    void* dout = nullptr;
    QIL_TRY(tmp.alloc(16, &dout));
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(InnerSite)));
    const double amp = phi->amplitude * psi->amplitude;
    const bool pc = phi->dtype == QIL_C64, sc = psi->dtype == QIL_C64;
    const InnerSite* t = dtab.as<InnerSite>();
    c64* o = static_cast<c64*>(dout);
    if (pc && sc) QIL_TRY((launch_inner_chain<c64, c64, c64, NS>(ctx, t, (int)n, amp, o)));
    else if (pc) QIL_TRY((launch_inner_chain<c64, double, c64, NS>(ctx, t, (int)n, amp, o)));
    else if (sc) QIL_TRY((launch_inner_chain<double, c64, c64, NS>(ctx, t, (int)n, amp, o)));
    else QIL_TRY((launch_inner_chain<double, double, double, NS>(ctx, t, (int)n, amp, o)));
    QIL_TRY(dtab.release());
    return qil_read_back(ctx, h, dout, 16);
}

// ---- <phi|psi>: GEMM route --------------------------------------------------------------------------------------
// the contraction alone: the amplitudes are not applied (qil_inner scales, qil_norm takes phi = psi); two states, or two
// operators with ph = 4 physical slices (s_in + 2 s_out, the same order in both operands) in the place of the states' 2
static int inner_gemm_raw(const qil_chain* phi, const qil_chain* psi, double h[2]) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    const int64_t ph = psi->phys_rank == 2 ? 4 : 2;
    const int dt = (phi->dtype == QIL_C64 || psi->dtype == QIL_C64) ? QIL_C64 : QIL_F64;
    const size_t e = qil_elem_size(dt);
    long long maxE = 1, maxT = 1, maxP = 1, maxS = 1;
    for (int64_t i = 0; i < n; ++i) {
        const long long pl = phi->dims[(size_t)i], pr = phi->dims[(size_t)i + 1];
        const long long sl = psi->dims[(size_t)i], sr = psi->dims[(size_t)i + 1];
        maxE = std::max(maxE, std::max(pl * sl, pr * sr));
        maxT = std::max(maxT, pl * ph * sr);
        maxP = std::max(maxP, pl * ph * pr);
        maxS = std::max(maxS, sl * ph * sr);
    }
    qil_scratch tmp(ctx);
    void *E = nullptr, *En = nullptr, *T = nullptr, *Pw = nullptr, *Sw = nullptr;
    QIL_TRY(tmp.alloc((size_t)maxE * e, &E));
    QIL_TRY(tmp.alloc((size_t)maxE * e, &En));
    QIL_TRY(tmp.alloc((size_t)maxT * e, &T));
    if (dt != phi->dtype) QIL_TRY(tmp.alloc((size_t)maxP * e, &Pw));
    if (dt != psi->dtype) QIL_TRY(tmp.alloc((size_t)maxS * e, &Sw));
    QIL_TRY(qil_dev_fill_ones(ctx, dt, E, 1));
    for (int64_t i = 0; i < n; ++i) {
        const int64_t pl = phi->dims[(size_t)i], pr = phi->dims[(size_t)i + 1];
        const int64_t sl = psi->dims[(size_t)i], sr = psi->dims[(size_t)i + 1];
        const void *Ap = nullptr, *As = nullptr;
        QIL_TRY(qil_site_operand(ctx, dt, phi, i, Pw, &Ap));
        QIL_TRY(qil_site_operand(ctx, dt, psi, i, Sw, &As));
        QIL_TRY(qil_overlap_env_step(ctx, dt, ph, pl, pr, sl, sr, Ap, As, E, T, En));
        std::swap(E, En);
    }
    return read_scalar(ctx, dt, E, h);
}

static long long max_bond(const qil_chain* c) {
    long long m = 1;
    for (int64_t d : c->dims) m = std::max<long long>(m, d);
    return m;
}

}  // namespace

// phi against psi (or against the product W psi, which has psi's chain shape): same context, register kind, length, sites
int qil_check_overlap_pair(const qil_mps* phi, const qil_mps* psi) {
    QIL_REQUIRE(phi->ctx == psi->ctx, QIL_EINVAL_ARG, "inner: MPS belong to different contexts");
    QIL_REQUIRE(phi->paired == psi->paired, QIL_EINVAL_ARG, "inner: cannot mix paired and single-register operands");
    QIL_REQUIRE(phi->n() == psi->n(), QIL_EINVAL_LENGTH,
                "inner: MPS must have the same number of sites. Found length(phi)=%lld, length(psi)=%lld",
                (long long)phi->n(), (long long)psi->n());
    QIL_REQUIRE(phi->site_ids == psi->site_ids, QIL_EINVAL_SITES, "inner: MPS must have the same site indices.");
    return QIL_OK;
}

int qil_check_pair(const char* verb, const qil_mpo* V, const qil_mpo* W) {
    QIL_REQUIRE(V->ctx == W->ctx, QIL_EINVAL_ARG, "%s: MPOs belong to different contexts", verb);
    QIL_REQUIRE(V->paired == W->paired, QIL_EINVAL_ARG, "%s: cannot mix paired and single-register operands", verb);
    QIL_REQUIRE(V->n() == W->n(), QIL_EINVAL_LENGTH,
                "%s: MPOs must have the same number of sites. Found length(V)=%lld, length(W)=%lld", verb, (long long)V->n(),
                (long long)W->n());
    QIL_REQUIRE(V->site_ids == W->site_ids, QIL_EINVAL_SITES, "%s: MPOs must have the same site indices.", verb);
    return QIL_OK;
}

extern "C" int qil_inner(const qil_mps* phi, const qil_mps* psi, double* out) {
    QIL_REQUIRE(phi && psi && out, QIL_EINVAL_ARG, "inner: null argument");
    QIL_TRY(qil_check_overlap_pair(phi, psi));
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const char* route = getenv("QIL_INNER_ROUTE");
    const long long mb = std::max(max_bond(phi), max_bond(psi));
    const bool fits = mb <= kChainMax;
    bool chain = fits && mb <= kChainAutoMax;
    if (route && !strcmp(route, "chain")) chain = fits;
    else if (route && !strcmp(route, "gemm")) chain = false;
    double h[2] = {0.0, 0.0};
    if (chain) {
        QIL_TRY(inner_chain_route<2>(phi, psi, h));   // the amplitudes are applied in the kernel
    } else {
        QIL_TRY(inner_gemm_raw(phi, psi, h));
        const double amp = phi->amplitude * psi->amplitude;
        h[0] *= amp;
        h[1] *= amp;
    }
    out[0] = h[0];
    out[1] = h[1];
    return QIL_OK;
}

// <V, W>_F = tr(V^H W): qil_inner's two routes with four physical slices per site; MPOs carry no amplitude
extern "C" int qil_mpo_inner(const qil_mpo* V, const qil_mpo* W, double* out) {
    QIL_REQUIRE(V && W && out, QIL_EINVAL_ARG, "mpo_inner: null argument");
    QIL_TRY(qil_check_pair("mpo_inner", V, W));
    qil_context* ctx = W->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const char* route = getenv("QIL_MPO_INNER_ROUTE");
    const long long mb = std::max(max_bond(V), max_bond(W));
    const bool fits = mb <= kChainMax;
    bool chain = fits && mb <= kMpoChainAutoMax;
    if (route && !strcmp(route, "chain")) chain = fits;
    else if (route && !strcmp(route, "gemm")) chain = false;
    double h[2] = {0.0, 0.0};
    if (chain) QIL_TRY(inner_chain_route<4>(V, W, h));
    else QIL_TRY(inner_gemm_raw(V, W, h));
    out[0] = h[0];
    out[1] = h[1];
    return QIL_OK;
}

// norm(psi) = sqrt(|<psi|psi>|) without the amplitude (mps.jl:754-771), on the GEMM route
extern "C" int qil_norm(const qil_mps* psi, double* out) {
    QIL_REQUIRE(psi && out, QIL_EINVAL_ARG, "norm: null argument");
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    double h[2] = {0.0, 0.0};
    QIL_TRY(inner_gemm_raw(psi, psi, h));
    *out = sqrt(sqrt(h[0] * h[0] + h[1] * h[1]));
    return QIL_OK;
}

// <phi|W psi>: E[p, a, s] (pl x Dl x sl) per site
//   T1 ((pl Dl) x 2sr)      = E ((pl Dl) x sl) * A_psi (sl x 2sr)                    T1[p, a, s_in, beta]
//   T2_beta (pl x 2Dr)      = T1_beta (pl x 2Dl) * W (2Dl x 2Dr)    (batch = beta)   T2[p, s_out, b, beta]
//   E' (pr x Dr sr)         = A_phi^H (pr x 2pl) * T2 (2pl x Dr sr)                  E'[q, b, beta]
extern "C" int qil_apply_inner(const qil_mps* phi, const qil_mpo* W, const qil_mps* psi, double* out) {
    QIL_REQUIRE(phi && W && psi && out, QIL_EINVAL_ARG, "apply_inner: null argument");
    QIL_TRY(qil_check_apply_operands(W, psi));
    QIL_TRY(qil_check_overlap_pair(phi, psi));
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int64_t n = psi->n();
    const int dt = (phi->dtype == QIL_C64 || W->dtype == QIL_C64 || psi->dtype == QIL_C64) ? QIL_C64 : QIL_F64;
    const size_t e = qil_elem_size(dt);
    long long maxE = 1, maxT1 = 1, maxT2 = 1, maxP = 1, maxS = 1, maxW = 1;
    for (int64_t i = 0; i < n; ++i) {
        const long long pl = phi->dims[(size_t)i], pr = phi->dims[(size_t)i + 1];
        const long long sl = psi->dims[(size_t)i], sr = psi->dims[(size_t)i + 1];
        const long long Dl = W->dims[(size_t)i], Dr = W->dims[(size_t)i + 1];
        maxE = std::max(maxE, std::max(pl * Dl * sl, pr * Dr * sr));
        maxT1 = std::max(maxT1, pl * Dl * 2 * sr);
        maxT2 = std::max(maxT2, pl * 2 * Dr * sr);
        maxP = std::max(maxP, pl * 2 * pr);
        maxS = std::max(maxS, sl * 2 * sr);
        maxW = std::max(maxW, Dl * 4 * Dr);
    }
    qil_scratch tmp(ctx);
    void *E = nullptr, *En = nullptr, *T1 = nullptr, *T2 = nullptr, *Pw = nullptr, *Sw = nullptr, *Ww = nullptr;
    QIL_TRY(tmp.alloc((size_t)maxE * e, &E));
    QIL_TRY(tmp.alloc((size_t)maxE * e, &En));
    QIL_TRY(tmp.alloc((size_t)maxT1 * e, &T1));
    QIL_TRY(tmp.alloc((size_t)maxT2 * e, &T2));
    if (dt != phi->dtype) QIL_TRY(tmp.alloc((size_t)maxP * e, &Pw));
    if (dt != psi->dtype) QIL_TRY(tmp.alloc((size_t)maxS * e, &Sw));
    if (dt != W->dtype) QIL_TRY(tmp.alloc((size_t)maxW * e, &Ww));
    QIL_TRY(qil_dev_fill_ones(ctx, dt, E, 1));
    for (int64_t i = 0; i < n; ++i) {
        const int64_t pl = phi->dims[(size_t)i], pr = phi->dims[(size_t)i + 1];
        const int64_t sl = psi->dims[(size_t)i], sr = psi->dims[(size_t)i + 1];
        const int64_t Dl = W->dims[(size_t)i], Dr = W->dims[(size_t)i + 1];
        const void *Ap = nullptr, *As = nullptr, *Wd = nullptr;
        QIL_TRY(qil_site_operand(ctx, dt, phi, i, Pw, &Ap));
        QIL_TRY(qil_site_operand(ctx, dt, psi, i, Sw, &As));
        QIL_TRY(qil_site_operand(ctx, dt, W, i, Ww, &Wd));
        QIL_TRY(qil_apply_overlap_env_step(ctx, dt, pl, pr, sl, sr, Dl, Dr, Ap, As, Wd, E, T1, T2, En));
        std::swap(E, En);
    }
    double h[2];
    QIL_TRY(read_scalar(ctx, dt, E, h));
    const double amp = phi->amplitude * psi->amplitude;
    out[0] = h[0] * amp;
    out[1] = h[1] * amp;
    return QIL_OK;
}

// norm(W psi): E[s', a', a, s] (sl x Dl x Dl x sl) per site, two buffers in ping-pong (X: E, T2, E'; Y: T1, T3); the four products
// are qil_norm_env_step (qil_contract.hip) on one environment:
//   T1 ((sl Dl Dl) x 2sr)   = E * A_psi                                                T1[s', a', a, s_in, beta]
//   T2_beta ((sl Dl) x 2Dr) = T1_beta ((sl Dl) x 2Dl) * W (2Dl x 2Dr)   (batch = beta) T2[s', a', s_out, b, beta]
//   T3_bb (sl x 2Dr)        = T2_bb (sl x 2Dl) * conj(Wr) (2Dl x 2Dr)   (batch = (b, beta), Wr = W with s_in <-> s_out)
//                                                                                      T3[s', s_in', b', b, beta]
//   E' (sr x Dr Dr sr)      = A_psi^H (sr x 2sl) * T3 (2sl x Dr Dr sr)                 E'[beta', b', b, beta]
extern "C" int qil_apply_norm(const qil_mpo* W, const qil_mps* psi, double* out) {
    QIL_REQUIRE(W && psi && out, QIL_EINVAL_ARG, "apply_norm: null argument");
    QIL_TRY(qil_check_apply_operands(W, psi));
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int64_t n = psi->n();
    const int dt = (W->dtype == QIL_C64 || psi->dtype == QIL_C64) ? QIL_C64 : QIL_F64;
    const size_t e = qil_elem_size(dt);
    long long maxX = 1, maxY = 1, maxS = 1, maxW = 1;
    for (int64_t i = 0; i < n; ++i) {
        const long long sl = psi->dims[(size_t)i], sr = psi->dims[(size_t)i + 1];
        const long long Dl = W->dims[(size_t)i], Dr = W->dims[(size_t)i + 1];
        maxX = std::max({maxX, sl * Dl * Dl * sl, sl * Dl * 2 * Dr * sr, sr * Dr * Dr * sr});
        maxY = std::max({maxY, sl * Dl * Dl * 2 * sr, sl * 2 * Dr * Dr * sr});
        maxS = std::max(maxS, sl * 2 * sr);
        maxW = std::max(maxW, Dl * 4 * Dr);
    }
    qil_scratch tmp(ctx);
    void *X = nullptr, *Y = nullptr, *Sw = nullptr, *Ww = nullptr, *Wr = nullptr;
    QIL_TRY(tmp.alloc((size_t)maxX * e, &X));
    QIL_TRY(tmp.alloc((size_t)maxY * e, &Y));
    QIL_TRY(tmp.alloc((size_t)maxW * e, &Wr));
    if (dt != psi->dtype) QIL_TRY(tmp.alloc((size_t)maxS * e, &Sw));
    if (dt != W->dtype) QIL_TRY(tmp.alloc((size_t)maxW * e, &Ww));
    QIL_TRY(qil_dev_fill_ones(ctx, dt, X, 1));
    for (int64_t i = 0; i < n; ++i) {
        const void *As = nullptr, *Wd = nullptr;
        QIL_TRY(qil_site_operand(ctx, dt, psi, i, Sw, &As));
        QIL_TRY(qil_site_operand(ctx, dt, W, i, Ww, &Wd));
        QIL_TRY(qil_put_mpo_site(ctx, dt, W, i, QIL_SITE_SWAPPED, Wr));
        QIL_TRY(qil_norm_env_step(ctx, dt, psi->dims[(size_t)i], psi->dims[(size_t)i + 1], W->dims[(size_t)i], W->dims[(size_t)i + 1], 1,
                                  As, Wd, Wr, X, Y, X, X));
    }
    double h[2];
    QIL_TRY(read_scalar(ctx, dt, X, h));
    *out = sqrt(sqrt(h[0] * h[0] + h[1] * h[1]));
    return QIL_OK;
}
