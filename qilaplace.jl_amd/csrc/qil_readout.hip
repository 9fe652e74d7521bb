// Read-out kernels: coefficient (C1), lazy <bits|W psi>, mps_to_vector (C2).  norm (K3) is in qil_inner.hip.
//
//   coefficient(psi, cfg)   src/mps.jl:669-678   amplitude * prod_i A_i[:, cfg_i, :]
//   mps_to_vector           src/mps.jl:716-743
//
// The reference contracts the row vector with the WHOLE site tensor and projects afterwards
// (mps.jl:675); here the physical slice is selected first (half the bytes, same arithmetic).
// Every query is a left-to-right vector-matrix chain: HBM-read bound on the selected slices.
// One workgroup owns one query and walks all sites inside ONE launch; each output entry is a
// dot product along the contiguous alpha axis, reduced with wavefront shuffles.
#include "qil_internal.h"
#include "qil_launch.h"
#include "qil_device_utils.h"
#include "qilaplace_hip_testing.h"
#include <set>

// elements per query of the lazy chain's row vector M and of each half of its X: max over the sites of D_r chi_r and D_r chi_l
static long long lazy_chain_elems(int64_t n, const int64_t* dims, const int64_t* wdims) {
    long long msz = 1;
    for (int64_t i = 0; i < n; ++i) msz = std::max<long long>({msz, wdims[i + 1] * dims[i + 1], wdims[i + 1] * dims[i]});
    return msz;
}

// The route of a read-out call: THE decision, not a copy of it -- wants_sort_plan, coefficient_enqueue, the sweep and the lazy verb
// switch on the value returned here, and qil_readout_route hands the same function to the tests.  dims: the n + 1 bond dimensions
// of the chain that is read (for QIL_READOUT_SWEEP with wdims: of psi, the product W psi having bonds dims[i] * wdims[i]);
// wdims: the operator's n + 1 bond dimensions (QIL_READOUT_LAZY, optional for the sweep).  *pass_queries: queries per pass of
// QIL_ROUTE_LAZY_GEMM (bounded scratch -- X is the big one -- and the grid's batch limit), nb on every other route.
static int readout_route(int verb, bool cx, int64_t nb, int64_t n, const int64_t* dims, const int64_t* wdims, int64_t* pass_queries) {
    if (pass_queries) *pass_queries = nb;
    if (verb == QIL_READOUT_LAZY) {
        // Many queries on a wide product bond: the per-query chains (one workgroup each, vector ALU) give way to batched MFMA
        // GEMMs.  Measured crossover of chi * D: 1.0 vs 2.0 ms at 1024, 0.85 vs 0.77 at 512.
        if (!(nb >= 16 && lazy_chain_elems(n, dims, wdims) >= 1024)) return QIL_ROUTE_LAZY_CHAIN;
        const qil_apply_bond_sizes b = qil_apply_sizes_of(n, dims, wdims);
        const long long per_query = (2 * b.maxM + b.maxX) * (cx ? 16LL : 8LL);
        if (pass_queries)
            *pass_queries = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nb, 32768), (8LL << 30) / per_query));
        return QIL_ROUTE_LAZY_GEMM;
    }
    long long maxchi = 1;
    for (int64_t i = 1; i <= n; ++i) maxchi = std::max<long long>(maxchi, dims[i] * (wdims ? wdims[i] : 1));
    // Crossover between one-workgroup-per-query chains and the all-queries-together GEMM forms.  Measured on a 256 x 256 grid
    // scan (65,536 queries): bond 504 chains 0.40 s vs GEMM 0.09 s; bond 23 chains 4.9 ms vs GEMM 3.2 ms -- many queries favour
    // the GEMM form at any bond dimension.  Few queries, 40 complex sites: bond 64 chains 0.37 ms vs GEMM 0.55 ms, bond 128 1.07
    // vs 0.81 ms, bond 512 9.2 vs 2.1 ms.
    if (!(nb >= 4 && (maxchi >= 128 || (nb >= 1024 && maxchi >= 16)))) return QIL_ROUTE_CHAIN;
    // a marginal (bit 2) needs both slices of its site: one product with the whole site, then each query keeps its own columns;
    // plain bits are sorted by site so that every query multiplies with ONE slice
    return verb == QIL_READOUT_MARGINAL ? QIL_ROUTE_GEMM_SELECT : QIL_ROUTE_GEMM_SORTED;
}

extern "C" int qil_readout_route(int verb, int dtype, int64_t nb, int64_t n, const int64_t* chain_dims, const int64_t* op_dims,
                                 int* route, int64_t* pass_queries) {
    QIL_REQUIRE(route && chain_dims, QIL_EINVAL_ARG, "readout_route: null argument");
    QIL_REQUIRE(verb >= QIL_READOUT_PLAIN && verb <= QIL_READOUT_LAZY, QIL_EINVAL_ARG, "readout_route: unknown verb %d", verb);
    QIL_REQUIRE(dtype == QIL_F64 || dtype == QIL_C64, QIL_EINVAL_ARG, "readout_route: unknown dtype %d", dtype);
    QIL_REQUIRE(nb >= 0 && n >= 1, QIL_EINVAL_ARG, "readout_route: needs nb >= 0 and at least one site");
    QIL_REQUIRE(verb != QIL_READOUT_LAZY || op_dims, QIL_EINVAL_ARG, "readout_route: the lazy verb needs the operator's bond dimensions");
    QIL_REQUIRE(!op_dims || verb >= QIL_READOUT_SWEEP, QIL_EINVAL_ARG, "readout_route: only the sweep and the lazy verb take an operator");
    for (int64_t i = 0; i <= n; ++i)
        QIL_REQUIRE(chain_dims[i] >= 1 && (!op_dims || op_dims[i] >= 1), QIL_EINVAL_ARG, "readout_route: bond dimension %lld is not positive",
                    (long long)i);
    *route = readout_route(verb, dtype == QIL_C64, nb, n, chain_dims, op_dims, pass_queries);
    return QIL_OK;
}

namespace {

using namespace qil_dev;

struct ChainSite {
    const void* A;  // MPS site
    const void* W;  // MPO site (lazy path) or null
    int cl, cr, Dl, Dr;
};
// the site table of the per-query chains; W null: the direct verbs
std::vector<ChainSite> chain_sites(const qil_mps* psi, const qil_mpo* W) {
    std::vector<ChainSite> tab((size_t)psi->n());
    for (size_t i = 0; i < tab.size(); ++i)
        tab[i] = ChainSite{psi->site[i], W ? W->site[i] : nullptr, (int)psi->dims[i], (int)psi->dims[i + 1],
                           W ? (int)W->dims[i] : 1, W ? (int)W->dims[i + 1] : 1};
    return tab;
}

constexpr int kThreads = 256;

// v_out[beta] = sum_alpha v_in[alpha] * A[alpha, bit, beta]; groups of G lanes share one beta.
template <class T>
__global__ __launch_bounds__(kThreads) void coefficient_chain(const ChainSite* __restrict__ sites, int n,
                                                              const uint8_t* __restrict__ bits,
                                                              T* __restrict__ scratch, long long maxchi,
                                                              c64* __restrict__ out, double amplitude) {
    const long long q = blockIdx.x;
    T* v_in = scratch + (2 * q) * maxchi;
    T* v_out = v_in + maxchi;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int nwaves = kThreads / 64;
    if (threadIdx.x == 0) v_in[0] = cast_elem<T>(1.0);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const ChainSite S = sites[i];
        const int bit = bits[q * n + i];
        // bit == 2: the site's physical index is summed (marginal): v' = v (A[:,0,:] + A[:,1,:])
        const bool both = bit == 2;
        const T* __restrict__ M = static_cast<const T*>(S.A) + (long long)S.cl * (both ? 0 : bit);
        int G = 64;  // lanes per dot product: smallest power of two >= cl (cap 64)
        while (G > 1 && (G >> 1) >= S.cl) G >>= 1;
        const int per_wave = 64 / G;
        const int grp = lane / G, gl = lane - grp * G;
        for (int beta = wave * per_wave + grp; beta < S.cr; beta += nwaves * per_wave) {
            const T* col = M + 2LL * S.cl * beta;
            T acc{};
            if (both)
                for (int al = gl; al < S.cl; al += G) acc = cmul_add(acc, v_in[al], add_t(col[al], col[al + S.cl]));
            else
                for (int al = gl; al < S.cl; al += G) acc = cmul_add(acc, v_in[al], col[al]);
            for (int m = G >> 1; m >= 1; m >>= 1) acc = add_t(acc, shfl_xor_t(acc, m));
            if (gl == 0) v_out[beta] = acc;
        }
        // the block's own global writes become visible to its other waves here
        __threadfence_block();
        __syncthreads();
        T* t = v_in;
        v_in = v_out;
        v_out = t;
    }
    if (threadIdx.x == 0) {
        c64 r = to_c64(v_in[0]);
        out[q] = c64{r.re * amplitude, r.im * amplitude};
    }
}

// Lazy path: carry M[a, alpha] (Dl x cl) per query.
//   M'[b, beta] = sum_{s'} sum_{a, alpha} W[a, s', bit, b] M[a, alpha] A[alpha, s', beta]
// two stages per site, both through global scratch owned by the workgroup:
//   X[s'][b, alpha] = sum_a W[a, s', bit, b] M[a, alpha]
//   M'[b, beta]     = sum_{s'} sum_alpha X[s'][b, alpha] A[alpha, s', beta]
template <class TW, class TA>
__global__ __launch_bounds__(kThreads) void lazy_coefficient_chain(const ChainSite* __restrict__ sites, int n,
                                                                   const uint8_t* __restrict__ bits,
                                                                   c64* __restrict__ scratch, long long msz,
                                                                   c64* __restrict__ out, double amplitude) {
    const long long q = blockIdx.x;
    c64* M = scratch + (4 * q) * msz;   // [alpha + cl * a]  (alpha fastest)
    c64* Mn = M + msz;
    c64* X = M + 2 * msz;               // 2 * msz: X[s'][alpha + cl * b]
    if (threadIdx.x == 0) M[0] = c64{1.0, 0.0};
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const ChainSite S = sites[i];
        const int bit = bits[q * n + i];
        const TW* __restrict__ W = static_cast<const TW*>(S.W);
        const TA* __restrict__ A = static_cast<const TA*>(S.A);
        // stage 1: X[sp][alpha + cl*b] = sum_a W[a + Dl*(sp + 2*(bit + 2*b))] * M[alpha + cl*a]
        const long long n1 = 2LL * S.cl * S.Dr;
        for (long long t = threadIdx.x; t < n1; t += kThreads) {
            const int alpha = (int)(t % S.cl);
            long long u = t / S.cl;
            const int b = (int)(u % S.Dr);
            const int sp = (int)(u / S.Dr);
            const TW* w = W + (long long)S.Dl * (sp + 2 * (bit + 2LL * b));
            c64 acc{};
            for (int a = 0; a < S.Dl; ++a) acc = cmul_add(acc, M[alpha + (long long)S.cl * a], w[a]);
            X[sp * msz + alpha + (long long)S.cl * b] = acc;
        }
        __threadfence_block();
        __syncthreads();
        // stage 2: Mn[beta + cr*b] = sum_sp sum_alpha X[sp][alpha + cl*b] * A[alpha + cl*(sp + 2*beta)]
        const long long n2 = (long long)S.cr * S.Dr;
        for (long long t = threadIdx.x; t < n2; t += kThreads) {
            const int beta = (int)(t % S.cr);
            const int b = (int)(t / S.cr);
            c64 acc{};
            for (int sp = 0; sp < 2; ++sp) {
                const c64* x = X + sp * msz + (long long)S.cl * b;
                const TA* acol = A + (long long)S.cl * (sp + 2LL * beta);
                for (int alpha = 0; alpha < S.cl; ++alpha) acc = cmul_add(acc, x[alpha], acol[alpha]);
            }
            Mn[beta + (long long)S.cr * b] = acc;
        }
        __threadfence_block();
        __syncthreads();
        c64* t = M;
        M = Mn;
        Mn = t;
    }
    if (threadIdx.x == 0) out[q] = c64{M[0].re * amplitude, M[0].im * amplitude};
}

// The bit-sorted / slice-selecting read-out steps, in the table form of qil_launch.h: in a lock-step batch (the per-operator read-outs of a damping sweep)
// the `select_slice` of up to 16 chains is ONE launch instead of one per chain and site (r04: 3 072 launches of 3.5 us per sweep
// of 64 operators, each of which also drained its chain's ring to get onto the stream).
template <class T>
__device__ __forceinline__ void select_slice_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ Tm, long long nb, int cr,
                                                  const uint8_t* __restrict__ bits, int n, int site, T* __restrict__ Vn) {
    const long long total = nb * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long q = t % nb;
        const long long beta = t / nb;
        const int bit = bits[q * n + site];
        Vn[t] = bit == 2 ? add_t(Tm[q + nb * (2 * beta)], Tm[q + nb * (1 + 2 * beta)]) : Tm[q + nb * (bit + 2 * beta)];
    }
}
template <class T>
struct select_slice_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        select_slice_body<T>(b, g, a...);
    }
};
// Bit-sorted read-out: rows of Tm are in site i's order (queries with bit 0 first), the next site wants its own order:
// Vn[r + nb * beta] = Tm[map[r] + nb * beta]
template <class T>
__device__ __forceinline__ void gather_rows_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ Tm, long long nb, int cr,
                                                 const int* __restrict__ map, T* __restrict__ Vn) {
    const long long total = nb * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long r = t % nb, beta = t / nb;
        Vn[t] = Tm[map[r] + nb * beta];
    }
}
template <class T>
struct gather_rows_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        gather_rows_body<T>(b, g, a...);
    }
};
template <class T>
__device__ __forceinline__ void finish_coeff_body(const uint3 blockIdx, const uint3 gridDim, const T* __restrict__ v, long long nb,
                                                  double amplitude, c64* __restrict__ out) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < nb; t += (long long)gridDim.x * blockDim.x) {
        const c64 r = to_c64(v[t]);
        out[t] = c64{r.re * amplitude, r.im * amplitude};
    }
}
template <class T>
struct finish_coeff_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        finish_coeff_body<T>(b, g, a...);
    }
};

// ---- dense read-out of a sub-lattice of configurations (grid scans) --------------------------------------
template <class T>
__global__ void slice_sum(const T* __restrict__ A, int cl, int cr, T* __restrict__ out) {
    // out[alpha, beta] = A[alpha, 0, beta] + A[alpha, 1, beta]
    const long long total = (long long)cl * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int al = (int)(t % cl);
        const long long be = t / cl;
        out[t] = add_t(A[al + (long long)cl * (2 * be)], A[al + (long long)cl * (2 * be + 1)]);
    }
}
template <class T>
__global__ void bit_reverse_scale(const T* __restrict__ in, T* __restrict__ out, int nbits, double scale, int rev) {
    const long long N = 1LL << nbits;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < N; t += (long long)gridDim.x * blockDim.x) {
        long long d = t;
        if (rev) d = nbits == 0 ? 0 : (long long)(__brevll((unsigned long long)t) >> (64 - nbits));
        T v = in[t];
        reinterpret_cast<double*>(&v)[0] *= scale;
        if (sizeof(T) == 16) reinterpret_cast<double*>(&v)[1] *= scale;
        out[d] = v;
    }
}

// ---- lazy read-out, GEMM form (many queries, large chi * D) ----------------------------------------------
// All queries advance together; per site two strided-batch MFMA GEMMs (batch = query):
//   X_q[alpha, (s', b)] = M_q[alpha, a] W[a, (s', b) | s = bit_q]               (chi_l x D_l) (D_l x 2 D_r)
//   M'_q[beta, b]     = sum_{(alpha, s')} A[(alpha, s'), beta] X_q[(alpha, s'), b]  (chi_r x 2 chi_l) (2 chi_l x D_r)
// The MPO site is re-laid once per site with the output bit slowest (qil_put_mpo_site, QIL_SITE_BIT_MAJOR), so each query's
// output-bit slice is one contiguous operand picked by the per-batch operand shift of the GEMM; A is used
// exactly as it lies in HBM, and X_q comes out of the first product in the layout the second one reads.
int lazy_gemm_path(qil_context* ctx, const qil_mpo* W, const qil_mps* psi, int64_t nb, int64_t chunk, const uint8_t* dbits,
                   c64* dout) {
    const int64_t n = psi->n();
    const bool wc = W->dtype == QIL_C64, ac = psi->dtype == QIL_C64;
    const int dt = (wc || ac) ? QIL_C64 : QIL_F64;
    const size_t e = qil_elem_size(dt);
    const qil_apply_bond_sizes b = qil_apply_sizes_of(W, psi);
    // chunk = queries per pass (readout_route)
    qil_scratch tmp(ctx);
    void *M0 = nullptr, *M1 = nullptr, *X = nullptr, *Wc = nullptr, *Ac = nullptr;
    QIL_TRY(tmp.alloc((size_t)(chunk * b.maxM) * e, &M0));
    QIL_TRY(tmp.alloc((size_t)(chunk * b.maxM) * e, &M1));
    QIL_TRY(tmp.alloc((size_t)(chunk * b.maxX) * e, &X));
    QIL_TRY(tmp.alloc((size_t)b.maxW * e, &Wc));
    if (dt == QIL_C64 && !ac) QIL_TRY(tmp.alloc((size_t)b.maxA * 16, &Ac));
    for (int64_t q0 = 0; q0 < nb; q0 += chunk) {
        const int64_t nq = std::min<int64_t>(chunk, nb - q0);
        QIL_TRY(qil_dev_fill_ones(ctx, dt, M0, nq));
        void *Mc = M0, *Mn = M1;
        for (int64_t i = 0; i < n; ++i) {
            QIL_TRY(qil_lazy_row_step(ctx, dt, W, psi, i, Mc, Mn, X, Wc, Ac, nq, dbits + q0 * n + i, n));
            std::swap(Mc, Mn);
        }
        QIL_TRY(qil_dev_finish_coeff(ctx, dt, Mc, nq, psi->amplitude, dout + q0));
    }
    return QIL_OK;
}

// Lazy read-out, chain form: one workgroup per query walks all sites in ONE launch
int lazy_chain_path(qil_context* ctx, qil_scratch& tmp, const qil_mpo* W, const qil_mps* psi, int64_t nb, const uint8_t* dbits,
                    c64* dout) {
    const int64_t n = psi->n();
    const long long msz = lazy_chain_elems(n, psi->dims.data(), W->dims.data());
    void* scratch = nullptr;
    QIL_TRY(tmp.alloc((size_t)(4 * nb * msz) * 16, &scratch));
    const std::vector<ChainSite> tab = chain_sites(psi, W);
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(ChainSite)));
    for_elem_types(W->dtype == QIL_C64, psi->dtype == QIL_C64, [&](auto w, auto a) {
        hipLaunchKernelGGL((lazy_coefficient_chain<decltype(w), decltype(a)>), dim3((unsigned)nb), dim3(kThreads), 0, qil_stream(ctx),
                           dtab.as<ChainSite>(), (int)n, dbits, (c64*)scratch, msz, dout, psi->amplitude);
    });
    QIL_HIP(hipGetLastError());
    return dtab.release();
}

// the caller's bits, checked, in a block of the call's scratch
int upload_bits(qil_scratch& tmp, int64_t nb, int64_t n, const uint8_t* bits, uint8_t** dbits, int max_bit = 1) {
    for (int64_t t = 0; t < nb * n; ++t)
        QIL_REQUIRE(bits[t] <= max_bit, QIL_EINVAL_CONFIG, "coefficient: bit value %d outside [0,%d]", (int)bits[t],
                    max_bit);
    return qil_upload_bytes(tmp, bits, (size_t)(nb * n), reinterpret_cast<void**>(dbits));
}

}  // namespace

// One site of the lazy row vector, shared by lazy_gemm_path above and the lead phase of qil_apply_weight_batch
// (qil_apply_weight.hip): Mn_q = the two products in front of lazy_gemm_path for the nq rows whose output bit at this site is
// sel[q * sel_step] (0 / 1).  Wc (D_l 4 D_r elements of dt) receives the re-laid MPO site, Ac (chi_l 2 chi_r c64, or null when psi
// needs no widening) the widened MPS site, X is nq * chi_l 2 D_r elements; Mc / Mn are packed per row (chi_l D_l and chi_r D_r).
int qil_lazy_row_step(qil_context* ctx, int dt, const qil_mpo* W, const qil_mps* psi, int64_t i, const void* Mc, void* Mn, void* X,
                      void* Wc, void* Ac, int64_t nq, const uint8_t* sel, int64_t sel_step) {
    const long long cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
    const long long Dl = W->dims[(size_t)i], Dr = W->dims[(size_t)i + 1];
    const void* Ap = nullptr;
    QIL_TRY(qil_put_mpo_site(ctx, dt, W, i, QIL_SITE_BIT_MAJOR, Wc));
    QIL_TRY(qil_site_operand(ctx, dt, psi, i, Ac, &Ap));
    qil_gemm_batch b1, b2;
    b1.count = nq;
    b1.a_bs = cl * Dl;
    b1.c_bs = cl * 2 * Dr;
    b1.b_sel = sel;
    b1.b_sel_step = sel_step;
    b1.b_sel_stride = Dl * 2 * Dr;
    QIL_TRY(qil_dev_gemm_batched(ctx, dt, 0, 0, cl, 2 * Dr, Dl, Mc, cl, Wc, Dl, X, cl, &b1));
    b2.count = nq;
    b2.b_bs = cl * 2 * Dr;
    b2.c_bs = cr * Dr;
    return qil_dev_gemm_batched(ctx, dt, 1, 0, cr, Dr, 2 * cl, Ap, 2 * cl, X, 2 * cl, Mn, cr, &b2);
}

// out[t] = amplitude * v[t], t < nb: the last step of the GEMM read-outs, for qil_product_batch (qil_product.hip) as well
int qil_dev_finish_coeff(qil_context* ctx, int dt, const void* v, int64_t nb, double amplitude, void* dout) {
    return for_elem_type(dt == QIL_C64, [&](auto t) {
        using T = decltype(t);
        return qil_klaunch<finish_coeff_k<T>>(ctx, dim3(qil_grid_for(nb)), dim3(256), 0, (const T*)v, (long long)nb, amplitude, (c64*)dout);
    });
}

static int coefficient_impl(const qil_mps* psi, int64_t nb, const uint8_t* bits, double* out, int max_bit);

extern "C" int qil_coefficient_batch(const qil_mps* psi, int64_t nb, const uint8_t* bits, double* out) {
    return coefficient_impl(psi, nb, bits, out, 1);
}

// Marginals: bit value 2 sums the site's physical index (a partial trace with the all-ones vector), so
// e.g. a Laplace value L(s_k) = dt sqrt(N) sum_j <k, j | psi>  (docs/src/tutorials/dt.jl:187-197: N
// coefficient calls per value) is ONE chain with every copy-site bit set to 2.
extern "C" int qil_coefficient_marginal_batch(const qil_mps* psi, int64_t nb, const uint8_t* bits, double* out) {
    return coefficient_impl(psi, nb, bits, out, 2);
}

// Plan of the bit-sorted GEMM read-out (built on the host from the caller's bits, shared by every chain read at the same
// configurations): before site i the query vectors are stored in order_i = queries with bit_i = 0 first (stable), so the site
// costs two products with ONE slice each -- n0[i] x chi_l by chi_l x chi_r and (nb - n0[i]) x chi_l by chi_l x chi_r -- instead
// of one nb x chi_l by chi_l x 2 chi_r product that computes both slices for every query and throws half away.  map[i][r] = row
// of site i's result that becomes row r of site i + 1's operand (the last map restores the caller's order).  The map is a block
// of the scratch of the call that built the plan: the plan does not own it.
struct SortPlan {
    const int* dmap = nullptr;           // [n][nb], device
    std::vector<int64_t> n0;             // per site: queries with bit 0
};
static int build_sort_plan(qil_scratch& tmp, int64_t nb, int64_t n, const uint8_t* bits, SortPlan* plan) {
    std::vector<int> map((size_t)(n * nb)), order((size_t)nb), next((size_t)nb), pos((size_t)nb);
    plan->n0.assign((size_t)n, 0);
    auto order_of = [&](int64_t site, std::vector<int>& o) -> int64_t {
        int64_t z = 0;
        if (site >= n) {
            for (int64_t q = 0; q < nb; ++q) o[(size_t)q] = (int)q;
            return nb;
        }
        for (int64_t q = 0; q < nb; ++q)
            if (bits[q * n + site] == 0) o[(size_t)z++] = (int)q;
        int64_t w = z;
        for (int64_t q = 0; q < nb; ++q)
            if (bits[q * n + site] != 0) o[(size_t)w++] = (int)q;
        return z;
    };
    plan->n0[0] = order_of(0, order);
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t r = 0; r < nb; ++r) pos[(size_t)order[(size_t)r]] = (int)r;
        const int64_t z = order_of(i + 1, next);
        if (i + 1 < n) plan->n0[(size_t)i + 1] = z;
        for (int64_t r = 0; r < nb; ++r) map[(size_t)(i * nb + r)] = pos[(size_t)next[(size_t)r]];
        order.swap(next);
    }
    void* p = nullptr;
    QIL_TRY(qil_upload_bytes(tmp, map.data(), map.size() * sizeof(int), &p));
    plan->dmap = static_cast<const int*>(p);
    return QIL_OK;
}
// the read-out of psi under `verb` takes the sorted GEMM form: it needs a plan
static bool wants_sort_plan(const qil_mps* psi, int64_t nb, int verb) {
    return readout_route(verb, psi->dtype == QIL_C64, nb, psi->n(), psi->dims.data(), nullptr, nullptr) == QIL_ROUTE_GEMM_SORTED;
}

// QIL_ROUTE_CHAIN: one workgroup per query walks all sites in ONE launch
static int readout_chain(qil_scratch& tmp, const qil_mps* psi, int64_t nb, const uint8_t* dbits, void* dout) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    const long long maxchi = *std::max_element(psi->dims.begin() + 1, psi->dims.end());
    void* scratch = nullptr;
    QIL_TRY(tmp.alloc((size_t)(2 * nb * maxchi) * qil_elem_size(psi->dtype), &scratch));
    const std::vector<ChainSite> tab = chain_sites(psi, nullptr);
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(ChainSite)));
    for_elem_type(psi->dtype == QIL_C64, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(coefficient_chain<T>, dim3((unsigned)nb), dim3(kThreads), 0, qil_stream(ctx), dtab.as<ChainSite>(), (int)n,
                           dbits, (T*)scratch, maxchi, (c64*)dout, psi->amplitude);
    });
    QIL_HIP(hipGetLastError());
    return dtab.release();
}

// The GEMM routes (large bonds): all queries advance together, V (nb x chi_l) -> Vn (nb x chi_r) through Tm per site, on f64-MFMA
// GEMMs.  What both share: the three blocks, the start V = ones, and qil_dev_finish_coeff at the end.
struct GemmRows {
    void *V = nullptr, *Vn = nullptr, *Tm = nullptr;
};
static int gemm_rows_begin(qil_scratch& tmp, const qil_mps* psi, int64_t nb, GemmRows* r) {
    const long long maxchi = *std::max_element(psi->dims.begin() + 1, psi->dims.end());
    const size_t esz = qil_elem_size(psi->dtype);
    QIL_TRY(tmp.alloc((size_t)(nb * maxchi) * esz, &r->V));
    QIL_TRY(tmp.alloc((size_t)(nb * maxchi) * esz, &r->Vn));
    QIL_TRY(tmp.alloc((size_t)(2 * nb * maxchi) * esz, &r->Tm));
    return qil_dev_fill_ones(tmp.ctx, psi->dtype, r->V, nb);
}

// QIL_ROUTE_GEMM_SELECT: the site tensor is read ONCE for the whole batch, T (nb x 2 chi_r) = V (nb x chi_l) * A_i (chi_l x 2 chi_r),
// then each query keeps the column block of its own bit (a marginal: the sum of both)
static int readout_gemm_select(qil_scratch& tmp, const qil_mps* psi, int64_t nb, const uint8_t* dbits, void* dout) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    GemmRows r;
    QIL_TRY(gemm_rows_begin(tmp, psi, nb, &r));
    for (int64_t i = 0; i < n; ++i) {
        const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        QIL_TRY(qil_dev_gemm(ctx, psi->dtype, 0, 0, nb, 2 * cr, cl, r.V, nb, psi->site[(size_t)i], cl, r.Tm, nb));
        QIL_TRY(for_elem_type(psi->dtype == QIL_C64, [&](auto t) {
            using T = decltype(t);
            return qil_klaunch<select_slice_k<T>>(ctx, dim3(qil_grid_for(nb * cr, 65536)), dim3(256), 0, (const T*)r.Tm, (long long)nb,
                                                  (int)cr, dbits, (int)n, (int)i, (T*)r.Vn);
        }));
        std::swap(r.V, r.Vn);
    }
    return qil_dev_finish_coeff(ctx, psi->dtype, r.V, nb, psi->amplitude, dout);
}

// QIL_ROUTE_GEMM_SORTED: rows [0, n0) take slice 0, rows [n0, nb) slice 1 (slice s of A[alpha, s, beta]: offset s chi_l, ld 2 chi_l),
// then the rows move into the next site's order
static int readout_gemm_sorted(qil_scratch& tmp, const qil_mps* psi, int64_t nb, const SortPlan& plan, void* dout) {
    qil_context* ctx = psi->ctx;
    const size_t esz = qil_elem_size(psi->dtype);
    GemmRows r;
    QIL_TRY(gemm_rows_begin(tmp, psi, nb, &r));
    for (int64_t i = 0; i < psi->n(); ++i) {
        const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        const int64_t z = plan.n0[(size_t)i];
        const char* site = static_cast<const char*>(psi->site[(size_t)i]);
        for (int sl = 0; sl < 2; ++sl) {
            const int64_t r0 = sl ? z : 0, rows = sl ? nb - z : z;
            if (rows == 0) continue;
            const void* Vs = static_cast<const char*>(r.V) + (size_t)r0 * esz;
            void* Ts = static_cast<char*>(r.Tm) + (size_t)r0 * esz;
            const void* As = site + (size_t)(sl * cl) * esz;
            if (rows <= 48) QIL_TRY(qil_dev_gemm_skinny(ctx, psi->dtype, 0, 0, rows, cr, cl, Vs, nb, As, 2 * cl, Ts, nb));
            else QIL_TRY(qil_dev_gemm(ctx, psi->dtype, 0, 0, rows, cr, cl, Vs, nb, As, 2 * cl, Ts, nb));
        }
        const int* map = plan.dmap + (size_t)(i * nb);
        QIL_TRY(for_elem_type(psi->dtype == QIL_C64, [&](auto t) {
            using T = decltype(t);
            return qil_klaunch<gather_rows_k<T>>(ctx, dim3(qil_grid_for(nb * cr, 65536)), dim3(256), 0, (const T*)r.Tm, (long long)nb,
                                                 (int)cr, map, (T*)r.Vn);
        }));
        std::swap(r.V, r.Vn);
    }
    return qil_dev_finish_coeff(ctx, psi->dtype, r.V, nb, psi->amplitude, dout);
}

// Enqueue the read-out of nb configurations (device bits) of psi into dout (nb complex, device); no synchronisation, every
// temporary is a block of a scratch of psi's context (in a sweep batch: the product's slot) and goes back to the pool in stream
// order.
static int coefficient_enqueue(const qil_mps* psi, int64_t nb, const uint8_t* dbits, void* dout, int verb, const SortPlan* plan) {
    qil_scratch tmp(psi->ctx);
    switch (readout_route(verb, psi->dtype == QIL_C64, nb, psi->n(), psi->dims.data(), nullptr, nullptr)) {
        case QIL_ROUTE_CHAIN: return readout_chain(tmp, psi, nb, dbits, dout);
        case QIL_ROUTE_GEMM_SELECT: return readout_gemm_select(tmp, psi, nb, dbits, dout);
        default:
            QIL_REQUIRE(plan && plan->dmap, QIL_EINVAL_ARG, "coefficient: the sorted read-out was not given its plan");
            return readout_gemm_sorted(tmp, psi, nb, *plan, dout);
    }
}

// the device-to-device form for qil_coefficient_at (qil_index.hip): the marginal verb's routes take device bits as they are
int qil_coefficient_enqueue_select(const qil_mps* psi, int64_t nb, const uint8_t* dbits, void* dout) {
    return coefficient_enqueue(psi, nb, dbits, dout, QIL_READOUT_MARGINAL, nullptr);
}

static int coefficient_impl(const qil_mps* psi, int64_t nb, const uint8_t* bits, double* out, int max_bit) {
    QIL_REQUIRE(psi && (nb == 0 || (bits && out)), QIL_EINVAL_ARG, "coefficient: null argument");
    if (nb == 0) return QIL_OK;
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    uint8_t* dbits = nullptr;
    QIL_TRY(upload_bits(tmp, nb, psi->n(), bits, &dbits, max_bit));
    const int verb = max_bit > 1 ? QIL_READOUT_MARGINAL : QIL_READOUT_PLAIN;
    SortPlan plan;
    if (wants_sort_plan(psi, nb, verb)) QIL_TRY(build_sort_plan(tmp, nb, psi->n(), bits, &plan));
    void* dout = nullptr;
    QIL_TRY(tmp.alloc((size_t)nb * 16, &dout));
    QIL_TRY(coefficient_enqueue(psi, nb, dbits, dout, verb, &plan));
    return qil_download(ctx, out, dout, (size_t)nb * 16);
}

// The body of a damping sweep (BASELINE.json configs[3]; the reference loops `W = build_dt_mpo(psi, wr); out = W * psi;
// coefficient(out, ...)` per damping value, docs/src/tutorials/dt.jl:150-197, zt.jl:300-348): for every operator of the
// batch the product W_j psi is materialised by the apply kernel and read out at the same nb configurations.  One bit
// upload, one download and ONE host synchronisation for the whole batch; each product's blocks return to the pool in
// stream order and serve the next one.
// The sweep body with its results LEFT IN HBM: dout = nw x nb complex values (operator-major) in psi's context, complete when
// the call returns (every slot's stream has been synchronised by the batch runner / the home stream holds the rest in order).
// qil_apply_coefficient_sweep copies them to the host; qil_apply_coefficient_sweep_gather (qil_comm.hip) all-gathers them first.
int qil_apply_coefficient_sweep_dev(const qil_mpo* const* Ws, int64_t nw, const qil_mps* psi, int64_t nb, const uint8_t* bits,
                                    void* dout) {
    qil_context* ctx = psi->ctx;
    qil_scratch tmp(ctx);
    uint8_t* dbits = nullptr;
    QIL_TRY(upload_bits(tmp, nb, psi->n(), bits, &dbits, 1));
    bool distinct = true;                                 // operators change context for the batch: each must be its own handle
    bool sorted = false;                                  // some product W_j psi is read out in the sorted GEMM form
    {
        std::set<const qil_mpo*> seen;
        for (int64_t j = 0; j < nw; ++j) {
            QIL_REQUIRE(Ws[j], QIL_EINVAL_ARG, "apply_coefficient_sweep: null operator %lld", (long long)j);
            QIL_REQUIRE(Ws[j]->ctx == ctx, QIL_EINVAL_ARG, "apply: MPO and MPS belong to different contexts");
            distinct = distinct && seen.insert(Ws[j]).second;
            // (an operator of another length is refused by the apply below)
            sorted = sorted || (Ws[j]->n() == psi->n() &&
                                readout_route(QIL_READOUT_SWEEP, true, nb, psi->n(), psi->dims.data(), Ws[j]->dims.data(), nullptr) ==
                                    QIL_ROUTE_GEMM_SORTED);
        }
    }
    SortPlan plan;                                        // one plan for every operator's read-out (same configurations)
    if (sorted) QIL_TRY(build_sort_plan(tmp, nb, psi->n(), bits, &plan));
    auto one = [&](const qil_mpo* W, const qil_mps* state, int64_t j) {
        qil_mps* prod = nullptr;
        QIL_TRY(qil_apply_shared_state(W, state, &prod));
        const int st = coefficient_enqueue(prod, nb, dbits, static_cast<char*>(dout) + (size_t)(j * nb) * 16, QIL_READOUT_SWEEP, &plan);
        qil_mps_destroy(prod);
        return st;
    };
    if (distinct && nw >= 4) {
        // every value's product + read-out is a chain of ~100 small launches: the values run concurrently on the context's
        // streams.  The operators move to their slot for the duration of the call (bookkeeping only); the state, the bits and the
        // results are shared device buffers (the state is read-only here and every slot's stream waits for the home stream first).
        const int st = qil_run_batch_on(
            ctx, nw, [&](int64_t j, qil_context* slot) { qil_chain_rebind(const_cast<qil_mpo*>(Ws[j]), slot); },
            [&](int64_t j, qil_context*) { return one(Ws[j], psi, j); });
        QIL_TRY(st);
    } else {
        for (int64_t j = 0; j < nw; ++j) QIL_TRY(one(Ws[j], psi, j));
    }
    return QIL_OK;
}

extern "C" int qil_apply_coefficient_sweep(const qil_mpo* const* Ws, int64_t nw, const qil_mps* psi, int64_t nb,
                                           const uint8_t* bits, double* out) {
    QIL_REQUIRE(Ws && psi && (nb == 0 || (bits && out)), QIL_EINVAL_ARG, "apply_coefficient_sweep: null argument");
    if (nw == 0 || nb == 0) return QIL_OK;
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    void* dout = nullptr;
    QIL_TRY(tmp.alloc((size_t)(nw * nb) * 16, &dout));
    QIL_TRY(qil_apply_coefficient_sweep_dev(Ws, nw, psi, nb, bits, dout));
    return qil_download(ctx, out, dout, (size_t)(nw * nb) * 16);
}

extern "C" int qil_apply_coefficient_batch(const qil_mpo* W, const qil_mps* psi, int64_t nb,
                                           const uint8_t* bits, double* out) {
    QIL_REQUIRE(W && psi && (nb == 0 || (bits && out)), QIL_EINVAL_ARG, "apply_coefficient: null argument");
    QIL_REQUIRE(W->ctx == psi->ctx, QIL_EINVAL_ARG, "apply: MPO and MPS belong to different contexts");
    QIL_REQUIRE(W->n() == psi->n(), QIL_EINVAL_LENGTH,
                "apply: MPO and MPS must have the same number of sites. Found length(W)=%lld, length(psi)=%lld",
                (long long)W->n(), (long long)psi->n());
    QIL_REQUIRE(W->site_ids == psi->site_ids, QIL_EINVAL_SITES,
                "apply: MPO and MPS must have the same site indices.");
    if (nb == 0) return QIL_OK;
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    const int64_t n = psi->n();
    uint8_t* dbits = nullptr;
    QIL_TRY(upload_bits(tmp, nb, n, bits, &dbits));
    void* dout = nullptr;
    QIL_TRY(tmp.alloc((size_t)nb * 16, &dout));
    int64_t pass = nb;
    const bool cx = W->dtype == QIL_C64 || psi->dtype == QIL_C64;
    if (readout_route(QIL_READOUT_LAZY, cx, nb, n, psi->dims.data(), W->dims.data(), &pass) == QIL_ROUTE_LAZY_GEMM)
        QIL_TRY(lazy_gemm_path(ctx, W, psi, nb, pass, dbits, (c64*)dout));
    else
        QIL_TRY(lazy_chain_path(ctx, tmp, W, psi, nb, dbits, (c64*)dout));
    return qil_download(ctx, out, dout, (size_t)nb * 16);
}

// All 2^F coefficients of the configurations that agree with `spec` on the fixed sites -- the (k, l) grid scans
// of docs/src/tutorials/zt.jl:283-309 and the Laplace-value sums of dt.jl:187-197 as ONE dense contraction
// instead of 2^F chains.  spec[i]: 0 / 1 = the site's bit is fixed, 2 = the site is summed (marginal),
// 3 = the site is free.  The running tensor T[idx, beta] (idx over the free sites so far) advances by one MFMA
// GEMM per site: a fixed site multiplies by the slice A[:, b, :], a summed site by A[:, 0, :] + A[:, 1, :], a
// free site by the whole site viewed as (chi_l x 2 chi_r) -- the product's (idx, s, beta) order IS the next
// T[(idx, s), beta], nothing is permuted.  Output index: free sites in chain order, first free site = most
// significant bit (reverse = 0, as mps_to_vector) or least significant (reverse = 1).
extern "C" int qil_mps_block(const qil_mps* psi, const uint8_t* spec, int reverse, void* host_out) {
    QIL_REQUIRE(psi && spec && host_out, QIL_EINVAL_ARG, "mps_block: null argument");
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    const int64_t n = psi->n();
    int nfree = 0;
    for (int64_t i = 0; i < n; ++i) {
        QIL_REQUIRE(spec[i] <= 3, QIL_EINVAL_CONFIG, "mps_block: spec value %d outside [0,3]", (int)spec[i]);
        nfree += spec[i] == 3;
    }
    QIL_REQUIRE(nfree <= 34, QIL_EINVAL_LENGTH, "mps_block: %d free sites is too many for a dense block", nfree);
    const int dt = psi->dtype;
    const size_t e = qil_elem_size(dt);
    long long maxel = 1, rows = 1, maxslice = 1;
    for (int64_t i = 0; i < n; ++i) {
        if (spec[i] == 3) rows *= 2;
        maxel = std::max<long long>(maxel, rows * psi->dims[(size_t)i + 1]);
        maxslice = std::max<long long>(maxslice, psi->dims[(size_t)i] * psi->dims[(size_t)i + 1]);
    }
    void *bufA = nullptr, *bufB = nullptr, *sl = nullptr;
    QIL_TRY(tmp.alloc((size_t)maxel * e, &bufA));
    QIL_TRY(tmp.alloc((size_t)maxel * e, &bufB));
    QIL_TRY(tmp.alloc((size_t)maxslice * e, &sl));
    QIL_TRY(qil_dev_fill_ones(ctx, dt, bufA, 1));
    // the fixed / summed sites BEHIND the last free one fold into a right boundary vector first (O(chi^2) each,
    // instead of dragging the 2^F rows of T through them)
    int64_t last_free = -1;
    for (int64_t i = 0; i < n; ++i)
        if (spec[i] == 3) last_free = i;
    long long maxchi = 1;
    for (int64_t i = 0; i <= n; ++i) maxchi = std::max<long long>(maxchi, psi->dims[(size_t)i]);
    void *rv = nullptr, *rv2 = nullptr;
    QIL_TRY(tmp.alloc((size_t)maxchi * e, &rv));
    QIL_TRY(tmp.alloc((size_t)maxchi * e, &rv2));
    QIL_TRY(qil_dev_fill_ones(ctx, dt, rv, 1));
    auto site_slice = [&](int64_t i, const void** B, long long* ldb) -> int {   // the (chi_l x chi_r) factor of site i
        const long long cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        const char* A = static_cast<const char*>(psi->site[(size_t)i]);
        if (spec[i] == 2) {
            for_elem_type(dt == QIL_C64, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(slice_sum<T>, dim3(qil_grid_for(cl * cr)), dim3(256), 0, qil_stream(ctx), (const T*)A, (int)cl, (int)cr,
                                   (T*)sl);
            });
            *B = sl;
            *ldb = cl;
        } else {
            *B = A + (size_t)spec[i] * (size_t)cl * e;
            *ldb = 2 * cl;
        }
        return QIL_OK;
    };
    for (int64_t i = n - 1; i > last_free; --i) {
        const long long cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        const void* B = nullptr;
        long long ldb = 0;
        QIL_TRY(site_slice(i, &B, &ldb));
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, cl, 1, cr, B, ldb, rv, cr, rv2, cl));
        std::swap(rv, rv2);
    }
    void *cur = bufA, *nxt = bufB;
    rows = 1;
    for (int64_t i = 0; i <= last_free; ++i) {
        const long long cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        if (spec[i] == 3) {
            QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, rows, 2 * cr, cl, cur, rows, psi->site[(size_t)i], cl, nxt, rows));
            rows *= 2;
        } else {
            const void* B = nullptr;
            long long ldb = 0;
            QIL_TRY(site_slice(i, &B, &ldb));
            QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, rows, cr, cl, cur, rows, B, ldb, nxt, rows));
        }
        std::swap(cur, nxt);
    }
    {   // close with the boundary vector: T (rows x chi) r (chi x 1)
        const long long cb = psi->dims[(size_t)(last_free + 1)];
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, rows, 1, cb, cur, rows, rv, cb, nxt, rows));
        std::swap(cur, nxt);
    }
    // natural order: the first free site is the LOWEST bit of idx
    for_elem_type(dt == QIL_C64, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(bit_reverse_scale<T>, dim3(qil_grid_for(rows, 65536)), dim3(256), 0, qil_stream(ctx), (const T*)cur, (T*)nxt,
                           nfree, psi->amplitude, reverse ? 0 : 1);
    });
    QIL_HIP(hipGetLastError());
    return qil_download(ctx, host_out, nxt, (size_t)rows * e);
}

extern "C" int qil_mps_to_vector(const qil_mps* psi, int reverse, void* host_out) {
    // every site free: the dense block read-out above (one MFMA GEMM per site; at n = 24 with 4096-wide bonds 0.73 s
    // of vector-ALU steps became a few tens of ms)
    QIL_REQUIRE(psi && host_out, QIL_EINVAL_ARG, "mps_to_vector: null argument");
    QIL_REQUIRE(psi->n() <= 34, QIL_EINVAL_LENGTH, "mps_to_vector: %lld sites is too many for a dense vector",
                (long long)psi->n());
    std::vector<uint8_t> spec((size_t)psi->n(), (uint8_t)3);
    return qil_mps_block(psi, spec.data(), reverse, host_out);
}
