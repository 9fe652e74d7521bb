// Product-vector read-out: out[r] = amplitude * prod_i ( v[r,i,0] A_i[:,0,:] + v[r,i,1] A_i[:,1,:] ).
//
//   coefficient(psi, cfg)   src/mps.jl:669-678   the contraction this generalises: there the row vector meets ONE physical
//                                                slice per site (v = e_bit), here a weighted sum of the two
//
// The weights are numbers, the carry is a row vector of the bond: O(n chi^2) per row, no operator, no truncation.  With
// v[r,i,:] = (1, w_r^(2^(n-i))) the value is sum_j x_j w_r^j, the transform of the encoded signal at ANY complex w_r.
// The carry is complex whatever the site is (the weights are); a real site is never widened: the chain kernel multiplies the
// complex carry with real entries, the GEMM route runs a real product on the carry's (re, im) rows.
// Two routes, chosen as the marginal read-out chooses (qil_readout_route with QIL_READOUT_MARGINAL: both slices of every site
// are needed for every row): one workgroup per row walking all tensors in one launch with the carry in LDS, or all rows
// together with one MFMA GEMM per tensor and a kernel that combines the two slices of each row.
#include "qil_internal.h"
#include "qil_launch.h"
#include "qil_device_utils.h"
#include "qilaplace_hip_testing.h"

namespace {

using namespace qil_dev;

struct ProductChainSite {
    const void* A;  // MPS site [cl, 2, cr]
    int cl, cr;
};

constexpr int kThreads = 256;
// The chain route keeps the carry ping-ponged in LDS: 2 * 16 B per bond entry.  1024 entries = 32 KiB of dynamic LDS, inside the
// 64 KiB a kernel may ask for without hipFuncSetAttribute; the launch asks for the call's own largest bond only.  Wider chains
// take the GEMM route whatever QIL_PRODUCT_ROUTE says.
constexpr long long kChainMaxBond = QIL_PRODUCT_CHAIN_MAX_BOND;
static_assert(2 * kChainMaxBond * sizeof(c64) <= 64 * 1024, "the LDS carry must fit the default dynamic LDS limit");
// In the marginal's many-rows arm (nb >= 1024, bond 16 .. 127) this verb stays on the chain while rows * bond^2 is below this:
// its carry is in LDS, and it is ahead of the GEMMs there (MEASUREMENTS 24).
constexpr long long kManyRowsChainWork = 1LL << 21;

// c0 a0 + c1 a1: the weighted sum of the two physical slices of one site entry
__device__ __forceinline__ c64 weigh(c64 c0, double a0, c64 c1, double a1) {
    return cmul_add(cmul_add(c64{0.0, 0.0}, c0, a0), c1, a1);
}
__device__ __forceinline__ c64 weigh(c64 c0, c64 a0, c64 c1, c64 a1) {
    return cmul_add(cmul_add(c64{0.0, 0.0}, c0, a0), c1, a1);
}

// v_out[beta] = sum_alpha v_in[alpha] * (c0 A[alpha, 0, beta] + c1 A[alpha, 1, beta]); groups of G lanes share one beta
// (coefficient_chain's lane grouping).  One workgroup per row, every tensor in this one launch; the carry lives in LDS
// (maxchi entries each way), so a tensor boundary is a workgroup barrier and nothing else.
template <class T>
__global__ __launch_bounds__(kThreads) void product_chain(const ProductChainSite* __restrict__ sites, int n,
                                                          const c64* __restrict__ w, int maxchi, c64* __restrict__ out,
                                                          double amplitude) {
    extern __shared__ __align__(16) unsigned char product_carry[];
    c64* v_in = reinterpret_cast<c64*>(product_carry);
    c64* v_out = v_in + maxchi;
    const long long q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int nwaves = kThreads / 64;
    if (threadIdx.x == 0) v_in[0] = c64{1.0, 0.0};
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const ProductChainSite S = sites[i];
        const c64 c0 = w[(q * n + i) * 2], c1 = w[(q * n + i) * 2 + 1];
        const T* __restrict__ A = static_cast<const T*>(S.A);
        int G = 64;  // lanes per dot product: smallest power of two >= cl (cap 64)
        while (G > 1 && (G >> 1) >= S.cl) G >>= 1;
        const int per_wave = 64 / G;
        const int grp = lane / G, gl = lane - grp * G;
        for (int beta = wave * per_wave + grp; beta < S.cr; beta += nwaves * per_wave) {
            const T* col = A + 2LL * S.cl * beta;   // both slices of the column: [0, cl) and [cl, 2 cl)
            c64 acc{0.0, 0.0};
            for (int al = gl; al < S.cl; al += G) acc = cmul_add(acc, v_in[al], weigh(c0, col[al], c1, col[al + S.cl]));
            for (int m = G >> 1; m >= 1; m >>= 1) acc = add_t(acc, shfl_xor_t(acc, m));
            if (gl == 0) v_out[beta] = acc;
        }
        __syncthreads();
        c64* t = v_in;
        v_in = v_out;
        v_out = t;
    }
    if (threadIdx.x == 0) out[q] = c64{v_in[0].re * amplitude, v_in[0].im * amplitude};
}

// The GEMM route's per-row step: Tm (nb x 2 chi_r, column s + 2 beta) holds V A_i for both slices, each row keeps its own
// combination  Vn[q + nb beta] = c0[q] Tm[q + nb 2 beta] + c1[q] Tm[q + nb (2 beta + 1)].  The weights lie tensor-major, so
// consecutive threads (consecutive q) read consecutive weights.  The carry is complex for either site type -- a real site's
// product leaves its (re, im) rows interleaved, which IS this layout -- so the kernel has no site-type parameter.
__device__ __forceinline__ void combine_slices_body(const uint3 blockIdx, const uint3 gridDim, const c64* __restrict__ Tm, long long nb,
                                                    int cr, const c64* __restrict__ c0, const c64* __restrict__ c1,
                                                    c64* __restrict__ Vn) {
    const long long total = nb * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long q = t % nb, beta = t / nb;
        Vn[t] = weigh(c0[q], Tm[q + nb * (2 * beta)], c1[q], Tm[q + nb * (2 * beta + 1)]);
    }
}
struct combine_slices_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        combine_slices_body(b, g, a...);
    }
};
// The caller's weights (row-major in r, i, s) re-laid tensor-major for combine_slices, once per call and on the device:
// wt[(2 i + s) nb + q] = w[(q n + i) 2 + s].  (On the host this transposition of nb n 2 scattered 16-byte stores was three
// quarters of a 4096-row call.)  The stores are coalesced; the strided loads are a few MB that stay in L2.
__device__ __forceinline__ void weights_tensor_major_body(const uint3 blockIdx, const uint3 gridDim, const c64* __restrict__ w, long long nb,
                                                          int n, c64* __restrict__ wt) {
    const long long total = nb * 2 * n;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long q = t % nb, is = t / nb;
        wt[t] = w[q * 2 * n + is];
    }
}
struct weights_tensor_major_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        weights_tensor_major_body(b, g, a...);
    }
};

long long widest_bond(const qil_mps* psi) {
    long long m = 1;
    for (int64_t d : psi->dims) m = std::max<long long>(m, d);
    return m;
}

// one workgroup per row; dw: the caller's weights as they came (row-major in r, i, s)
int product_chain_route(const qil_mps* psi, int64_t nb, const c64* dw, c64* dout) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    std::vector<ProductChainSite> tab((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        tab[(size_t)i] = ProductChainSite{psi->site[(size_t)i], (int)psi->dims[(size_t)i], (int)psi->dims[(size_t)i + 1]};
    const long long maxchi = widest_bond(psi);
    const size_t lds = 2 * (size_t)maxchi * sizeof(c64);
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(ProductChainSite)));
    if (psi->dtype == QIL_C64)
        hipLaunchKernelGGL(product_chain<c64>, dim3((unsigned)nb), dim3(kThreads), lds, qil_stream(ctx), dtab.as<ProductChainSite>(),
                           (int)n, dw, (int)maxchi, dout, psi->amplitude);
    else
        hipLaunchKernelGGL(product_chain<double>, dim3((unsigned)nb), dim3(kThreads), lds, qil_stream(ctx), dtab.as<ProductChainSite>(),
                           (int)n, dw, (int)maxchi, dout, psi->amplitude);
    QIL_HIP(hipGetLastError());
    return dtab.release();
}

// all rows together; w: the caller's weights as they came, re-laid here: c_s of tensor i at dw + (2 i + s) nb
int product_gemm_route(const qil_mps* psi, qil_scratch& tmp, int64_t nb, const c64* w, c64* dout) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    void* wt = nullptr;
    QIL_TRY(tmp.alloc((size_t)(nb * n) * 32, &wt));
    QIL_TRY((qil_klaunch<weights_tensor_major_k>(ctx, dim3(qil_grid_for(2 * nb * n, 65536)), dim3(256), 0, w, (long long)nb, (int)n,
                                                 (c64*)wt)));
    const c64* dw = static_cast<const c64*>(wt);
    long long maxchi = 1;
    for (int64_t i = 1; i <= n; ++i) maxchi = std::max<long long>(maxchi, psi->dims[(size_t)i]);
    void *V = nullptr, *Vn = nullptr, *Tm = nullptr;
    QIL_TRY(tmp.alloc((size_t)(nb * maxchi) * 16, &V));
    QIL_TRY(tmp.alloc((size_t)(nb * maxchi) * 16, &Vn));
    QIL_TRY(tmp.alloc((size_t)(2 * nb * maxchi) * 16, &Tm));
    QIL_TRY(qil_dev_fill_ones(ctx, QIL_C64, V, nb));
    // A real site multiplies the complex carry as a REAL product with 2 nb rows: V [q + nb alpha] complex is the real
    // (2 nb x chi_l) matrix of leading dimension 2 nb, rows (re_q, im_q) adjacent, and Tm comes out laid the same way.
    const int64_t rows = psi->dtype == QIL_C64 ? nb : 2 * nb;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        if (rows <= 48) QIL_TRY(qil_dev_gemm_skinny(ctx, psi->dtype, 0, 0, rows, 2 * cr, cl, V, rows, psi->site[(size_t)i], cl, Tm, rows));
        else QIL_TRY(qil_dev_gemm(ctx, psi->dtype, 0, 0, rows, 2 * cr, cl, V, rows, psi->site[(size_t)i], cl, Tm, rows));
        const unsigned g = (unsigned)std::min<long long>((nb * cr + 255) / 256, 65536);
        QIL_TRY((qil_klaunch<combine_slices_k>(ctx, dim3(g), dim3(256), 0, (const c64*)Tm, (long long)nb, (int)cr,
                                               dw + (size_t)(2 * i) * nb, dw + (size_t)(2 * i + 1) * nb, (c64*)Vn)));
        std::swap(V, Vn);
    }
    return qil_dev_finish_coeff(ctx, QIL_C64, V, nb, psi->amplitude, dout);
}

}  // namespace

extern "C" int qil_product_batch(const qil_mps* psi, int64_t nb, const double* v, double* out) {
    QIL_REQUIRE(psi && (nb <= 0 || (v && out)), QIL_EINVAL_ARG, "product_batch: null argument");
    QIL_REQUIRE(nb >= 0, QIL_EINVAL_ARG, "product_batch: nb must be non-negative, got %lld", (long long)nb);
    if (nb == 0) return QIL_OK;
    const int64_t n = psi->n();
    for (int64_t r = 0; r < nb; ++r)
        for (int64_t i = 0; i < n; ++i) {
            const double* x = v + (r * n + i) * 4;
            QIL_REQUIRE(std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]) && std::isfinite(x[3]), QIL_EINVAL_ARG,
                        "product_batch: the weights of row %lld, tensor %lld are not finite", (long long)r, (long long)i);
        }
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    // The marginal's decision -- the work has its shape: both slices of every site for every row -- with one constant of this
    // verb's own.  The marginal sends many rows (nb >= 1024) to the GEMMs from bond 16 on; this chain keeps its carry in LDS and
    // is still ahead at small rows * bond^2.  n = 24, chain against GEMM in ms: 1024 rows, bond 32: 0.18 / 0.26; 4096 rows, bond
    // 16: 0.25 / 0.36, bond 24: 0.38 / 0.37, bond 32: 0.45 / 0.38, bond 64: 1.25 / 0.51.
    int route = QIL_ROUTE_CHAIN;
    QIL_TRY(qil_readout_route(QIL_READOUT_MARGINAL, psi->dtype, nb, n, psi->dims.data(), nullptr, &route, nullptr));
    const long long wb = widest_bond(psi);
    bool chain = route == QIL_ROUTE_CHAIN || (wb < 128 && nb * wb * wb < kManyRowsChainWork);
    const char* forced = getenv("QIL_PRODUCT_ROUTE");
    if (forced && !strcmp(forced, "chain")) chain = true;
    else if (forced && !strcmp(forced, "gemm")) chain = false;
    chain = chain && wb <= kChainMaxBond;    // the LDS carry bounds the bond
    void *dw = nullptr, *dout = nullptr;
    QIL_TRY(tmp.alloc((size_t)nb * 16, &dout));
    QIL_TRY(qil_upload_bytes(tmp, v, (size_t)(nb * n) * 32, &dw));
    if (chain) QIL_TRY(product_chain_route(psi, nb, static_cast<const c64*>(dw), static_cast<c64*>(dout)));
    else QIL_TRY(product_gemm_route(psi, tmp, nb, static_cast<const c64*>(dw), static_cast<c64*>(dout)));
    QIL_HIP(hipMemcpyAsync(out, dout, (size_t)nb * 16, hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));
    return QIL_OK;
}
