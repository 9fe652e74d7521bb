// Born weights for gfx950: qil_weight_batch returns, per spec row, amplitude^2 times the sum of |psi_x|^2 over the configurations
// x that agree with the row -- a site is fixed (0 / 1) or traced in |psi|^2 (2).  The contraction and its order are fixed in
// include/qilaplace_hip.h: a row vector v through the leading fixed sites, rho = v^H v at the first traced site, then
// rho <- A_s^H (rho A_s) per slice, slice 0 before slice 1 on a traced site.  Two routes, chosen from the state's bonds alone:
//   weight_walk_lds     ONE launch for the whole batch, one workgroup (16 waves) per row.  The row's bits come from a device copy of the
//                       spec, the site tensors straight from HBM / L2 (all rows share them; the site table goes through
//                       qil_dev_table).  The vector phase runs in LDS; after the first traced site rho, U^T = (rho A_s)^T and
//                       rho' are three LDS buffers, and both products of a slice, U = rho A_s and rho' (+)= A_s^H U, run in
//                       16 x 16 tiles on v_mfma_f64_16x16x4_f64 (one tile per wave and step, edge tiles zero-filled in the operand
//                       loads and masked in the stores).  Both products read their LDS operand as 16 consecutive rows of 4 columns
//                       and store their result transposed, so every LDS access of a 16-lane row is contiguous.
//                       No atomics, a fixed order: a row's result is bit-identical alone, in any batch and from run to run.
//   GEMM route          any bonds: rho per row in pool memory, per site and slice two strided-batch products through
//                       qil_dev_gemm_batched (A_s shared by the batch, stride 0) and weight_combine, which keeps slice 0, slice 1
//                       or their sum by the row's spec.  It carries rho from rho_0 = [1] (no vector phase: v^H v in exact
//                       arithmetic), in chunks of rows under kGemmBudget = 64 MiB of temporaries (four chi^2 buffers per row).
// LDS limits.  Three buffers of ld x ld elements and two vectors of ld: (3 ld^2 + 2 ld) e bytes within the 160 KiB of a CU.  The
// leading dimension ld is padded so that the MFMA operand read, 16 rows of columns k and k + 1 per 32-lane half (f64, ds_read_b64,
// banks (a / 4) mod 64) has the two columns in opposite halves of the bank row: ld = 16 mod 32.  For c64 (ds_read_b128, 16-lane
// groups that take rows 0-3 and 12-15 of one column and rows 4-11 of the next) the columns must start on the same bank: ld = 0 mod
// 16.  f64: ld = 80 -> 154 880 B (ld = 112 does not fit), so every bond <= 80; c64: ld = 48 -> 112 128 B (ld = 64 -> 198 656 B does
// not fit), so every bond <= 48.  A state with a wider bond anywhere takes the GEMM route for every row.
// Left out: weights of operators, a device-resident result (the lazy form on W psi is qil_apply_weight.hip).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "qil_internal.h"
#include "qil_device_utils.h"

#ifndef QIL_WEIGHT_LDS_MAX_F64
#define QIL_WEIGHT_LDS_MAX_F64 80
#endif
#ifndef QIL_WEIGHT_LDS_MAX_C64
#define QIL_WEIGHT_LDS_MAX_C64 48
#endif

namespace {

using namespace qil_dev;

constexpr int64_t kLdsMaxBond[2] = {QIL_WEIGHT_LDS_MAX_F64, QIL_WEIGHT_LDS_MAX_C64};   // indexed by qil_dtype
constexpr size_t kLdsBytes = 160 * 1024;
constexpr int64_t kGemmBudget = 64LL << 20;       // bytes of rho / U / slice products per chunk of rows
constexpr int kThreads = 1024;                    // sixteen waves: one LDS-bound workgroup per CU, a tile of a 64 x 64 product each

static_assert((3 * kLdsMaxBond[0] * kLdsMaxBond[0] + 2 * kLdsMaxBond[0]) * 8 <= (int64_t)kLdsBytes, "f64 limit exceeds the LDS");
static_assert((3 * kLdsMaxBond[1] * kLdsMaxBond[1] + 2 * kLdsMaxBond[1]) * 16 <= (int64_t)kLdsBytes, "c64 limit exceeds the LDS");

struct WalkSite {
    const void* A;         // the site tensor [cl, 2, cr]
    int cl, cr;
};

// out[j + ld i] (+)= sum_k X[i + ld k] Y(k, j) for i < M, j < N, k < K: X in LDS, Y = slice entries A[k + 2 K j] of the site
// tensor in HBM (conjugated when CONJ), the result stored transposed.  All waves of the workgroup take tiles in turn; the caller
// puts the barriers.
template <class T, bool CONJ>
__device__ __forceinline__ void tile_product(const T* __restrict__ X, int ld, int M, int K, const T* __restrict__ A, int N,
                                             T* __restrict__ out, bool accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int tm = (M + 15) >> 4, tn = (N + 15) >> 4;
    for (int t = wave; t < tm * tn; t += kThreads / 64) {
        const int row0 = 16 * (t % tm), col = 16 * (t / tm) + li;
        const int row = row0 + li;
        d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0};
        for (int k0 = 0; k0 < K; k0 += 4) {
            const int k = k0 + lk;
            T x{}, y{};
            if (row < M && k < K) x = X[row + ld * k];
            if (col < N && k < K) y = A[k + 2LL * K * col];
            if constexpr (CONJ) y = conj_t(y);
            mfma_step(x, y, rr, ii);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int orow = row0 + lk + 4 * r;
            if (orow < M && col < N) {
                T v = make_elem(rr[r], ii[r], (T*)nullptr);
                T* dst = out + col + ld * orow;
                *dst = accumulate ? add_t(*dst, v) : v;
            }
        }
    }
}

template <class T>
__global__ __launch_bounds__(kThreads) void weight_walk_lds(const WalkSite* __restrict__ sites, int n,
                                                            const uint8_t* __restrict__ spec, int ld, double amp2,
                                                            double* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* rho = reinterpret_cast<T*>(lds_raw);
    T* ut = rho + ld * ld;
    T* nxt = ut + ld * ld;
    T* v_in = nxt + ld * ld;
    T* v_out = v_in + ld;
    const uint8_t* __restrict__ bits = spec + (long long)blockIdx.x * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int nwaves = kThreads / 64;
    if (tid == 0) v_in[0] = cast_elem<T>(1.0);
    __syncthreads();
    // the vector phase: v <- v A_b through the leading fixed sites, the dot products of coefficient_chain
    int i = 0;
    for (; i < n; ++i) {
        const int bit = bits[i];
        if (bit == 2) break;
        const WalkSite S = sites[i];
        const T* __restrict__ M = static_cast<const T*>(S.A) + (long long)S.cl * bit;
        int G = 64;                                    // lanes per dot product: smallest power of two >= cl (cap 64)
        while (G > 1 && (G >> 1) >= S.cl) G >>= 1;
        const int per_wave = 64 / G;
        const int grp = lane / G, gl = lane - grp * G;
        for (int beta0 = wave * per_wave; beta0 < S.cr; beta0 += nwaves * per_wave) {   // uniform trip count per wave
            const int beta = beta0 + grp;
            T acc{};
            if (beta < S.cr) {
                const T* col = M + 2LL * S.cl * beta;
                for (int al = gl; al < S.cl; al += G) acc = cmul_add(acc, v_in[al], col[al]);
            }
            for (int m = G >> 1; m >= 1; m >>= 1) acc = add_t(acc, shfl_xor_t(acc, m));
            if (gl == 0 && beta < S.cr) v_out[beta] = acc;
        }
        __syncthreads();
        T* t = v_in;
        v_in = v_out;
        v_out = t;
    }
    if (i == n) {                                      // no traced site: |coefficient|^2
        if (tid == 0) out[blockIdx.x] = amp2 * abs2_t(v_in[0]);
        return;
    }
    {
        const int cl = sites[i].cl;                    // rho = v^H v
        for (int idx = tid; idx < cl * cl; idx += kThreads) {
            const int a = idx % cl, b = idx / cl;
            rho[a + ld * b] = cmul_add(T{}, conj_t(v_in[a]), v_in[b]);
        }
    }
    __syncthreads();
    for (; i < n; ++i) {
        const WalkSite S = sites[i];
        const int bit = bits[i];
        const int s0 = bit == 2 ? 0 : bit, s1 = bit == 2 ? 1 : bit;
        for (int s = s0; s <= s1; ++s) {
            const T* __restrict__ As = static_cast<const T*>(S.A) + (long long)S.cl * s;
            tile_product<T, false>(rho, ld, S.cl, S.cl, As, S.cr, ut, false);           // U^T: ut[b + ld a] = (rho A_s)[a][b]
            __syncthreads();
            tile_product<T, true>(ut, ld, S.cr, S.cl, As, S.cr, nxt, s != s0);          // nxt[b' + ld b] (+)= (A_s^H U)[b'][b]
            __syncthreads();
        }
        T* t = rho;
        rho = nxt;
        nxt = t;
    }
    if (tid == 0) out[blockIdx.x] = amp2 * re_of(rho[0]);
}

// ---- the GEMM route
// rho_r <- P0_r, P1_r or P0_r + P1_r (slice 0 first) by the row's spec at this site
template <class T>
__global__ void weight_combine(const T* __restrict__ P0, const T* __restrict__ P1, T* __restrict__ rho, long long stride,
                               long long elems, long long rows, const uint8_t* __restrict__ spec, int n, int site) {
    const long long total = rows * elems;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long r = t / elems, idx = r * stride + t % elems;
        const int bit = spec[r * n + site];
        rho[idx] = bit == 0 ? P0[idx] : bit == 1 ? P1[idx] : add_t(P0[idx], P1[idx]);
    }
}
template <class T>
__global__ void weight_finish(const T* __restrict__ rho, long long stride, long long rows, double amp2, double* __restrict__ out) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x)
        out[r] = amp2 * re_of(rho[r * stride]);
}

constexpr long long kGridCap = 65536;              // workgroups of the GEMM route's element-wise kernels

template <class T>
int walk_by_gemm(qil_context* ctx, const qil_mps* psi, int64_t nb, const uint8_t* dspec, double amp2, double* dout) {
    const int64_t n = psi->n();
    const int dt = psi->dtype;
    long long stride = 1;
    for (int64_t i = 0; i <= n; ++i) stride = std::max<long long>(stride, psi->dims[(size_t)i] * psi->dims[(size_t)i]);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nb, 65535), kGemmBudget / (4 * stride * (int64_t)sizeof(T))));
    qil_scratch tmp(ctx);
    void* buf[4] = {};                                 // rho, U, P0, P1: chunk x stride elements each
    for (void*& b : buf) QIL_TRY(tmp.alloc((size_t)(chunk * stride) * sizeof(T), &b));
    T *rho = static_cast<T*>(buf[0]), *U = static_cast<T*>(buf[1]);
    T* P[2] = {static_cast<T*>(buf[2]), static_cast<T*>(buf[3])};
    for (int64_t r0 = 0; r0 < nb; r0 += chunk) {
        const int64_t rows = std::min<int64_t>(chunk, nb - r0);
        QIL_TRY(qil_dev_fill_ones(ctx, dt, rho, rows, stride));
        for (int64_t i = 0; i < n; ++i) {
            const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
            for (int s = 0; s < 2; ++s) {
                const T* As = static_cast<const T*>(psi->site[(size_t)i]) + s * cl;
                qil_gemm_batch b1, b2;
                b1.count = b2.count = rows;
                b1.a_bs = b1.c_bs = stride;            // U_r = rho_r A_s
                b2.b_bs = b2.c_bs = stride;            // P_s,r = A_s^H U_r
                QIL_TRY(qil_dev_gemm_batched(ctx, dt, 0, 0, cl, cr, cl, rho, cl, As, 2 * cl, U, cl, &b1));
                QIL_TRY(qil_dev_gemm_batched(ctx, dt, 2, 0, cr, cr, cl, As, 2 * cl, U, cl, P[s], cr, &b2));
            }
            hipLaunchKernelGGL(weight_combine<T>, dim3(qil_grid_for(rows * cr * cr, kGridCap)), dim3(256), 0, qil_stream(ctx), (const T*)P[0],
                               (const T*)P[1], rho, stride, (long long)(cr * cr), (long long)rows, dspec + r0 * n, (int)n, (int)i);
            QIL_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(weight_finish<T>, dim3(qil_grid_for(rows, kGridCap)), dim3(256), 0, qil_stream(ctx), (const T*)rho, stride,
                           (long long)rows, amp2, dout + r0);
        QIL_HIP(hipGetLastError());
    }
    return QIL_OK;
}

template <class T>
int walk_in_lds(qil_context* ctx, const qil_mps* psi, int64_t nb, const uint8_t* dspec, double amp2, double* dout) {
    const int64_t n = psi->n();
    std::vector<WalkSite> tab((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        tab[(size_t)i] = WalkSite{psi->site[(size_t)i], (int)psi->dims[(size_t)i], (int)psi->dims[(size_t)i + 1]};
    const int ld = (int)kLdsMaxBond[psi->dtype];
    const size_t lds = (3 * (size_t)ld * ld + 2 * (size_t)ld) * sizeof(T);
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(WalkSite)));
    static qil_lds_grant grant;                        // per device and instantiation (qil_internal.h)
    QIL_HIP(grant.ensure(ctx->device, reinterpret_cast<const void*>(&weight_walk_lds<T>), lds));
    for (int64_t r0 = 0; r0 < nb; r0 += 1LL << 30) {   // the grid's x limit
        const int64_t rows = std::min<int64_t>(1LL << 30, nb - r0);
        hipLaunchKernelGGL(weight_walk_lds<T>, dim3((unsigned)rows), dim3(kThreads), lds, qil_stream(ctx), dtab.as<WalkSite>(),
                           (int)n, dspec + r0 * n, ld, amp2, dout + r0);
        QIL_HIP(hipGetLastError());
    }
    return dtab.release();
}

// the route of a state: its bonds alone decide (QIL_WEIGHT_NO_LDS=1 sends every state through the GEMM route: the A/B of
// MEASUREMENTS.md)
bool fits_lds(const qil_mps* psi) {
    static const bool off = [] {
        const char* v = getenv("QIL_WEIGHT_NO_LDS");
        return v && v[0] == '1';
    }();
    if (off) return false;
    int64_t top = 1;
    for (int64_t d : psi->dims) top = std::max(top, d);
    return top <= kLdsMaxBond[psi->dtype];
}

}  // namespace

extern "C" int qil_weight_batch(const qil_mps* psi, int64_t nb, const uint8_t* spec, double* out) {
    QIL_REQUIRE(psi && (nb <= 0 || (spec && out)), QIL_EINVAL_ARG, "weight_batch: null argument");
    QIL_REQUIRE(nb >= 0, QIL_EINVAL_ARG, "weight_batch: negative row count %lld", (long long)nb);
    const int64_t n = psi->n();
    for (int64_t t = 0; t < nb * n; ++t)
        QIL_REQUIRE(spec[t] <= 2, QIL_EINVAL_CONFIG,
                    "weight_batch: spec value %d outside [0,2] (a kept site makes no number: qil_mps_restrict keeps sites)", (int)spec[t]);
    if (nb == 0) return QIL_OK;
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    void *dspec = nullptr, *dout = nullptr;
    QIL_TRY(qil_upload_bytes(tmp, spec, (size_t)(nb * n), &dspec));
    QIL_TRY(tmp.alloc((size_t)nb * sizeof(double), &dout));
    const double amp2 = psi->amplitude * psi->amplitude;
    const bool lds = fits_lds(psi), cx = psi->dtype == QIL_C64;
    if (lds && cx) QIL_TRY(walk_in_lds<c64>(ctx, psi, nb, static_cast<const uint8_t*>(dspec), amp2, static_cast<double*>(dout)));
    else if (lds) QIL_TRY(walk_in_lds<double>(ctx, psi, nb, static_cast<const uint8_t*>(dspec), amp2, static_cast<double*>(dout)));
    else if (cx) QIL_TRY(walk_by_gemm<c64>(ctx, psi, nb, static_cast<const uint8_t*>(dspec), amp2, static_cast<double*>(dout)));
    else QIL_TRY(walk_by_gemm<double>(ctx, psi, nb, static_cast<const uint8_t*>(dspec), amp2, static_cast<double*>(dout)));
    QIL_HIP(hipMemcpyAsync(out, dout, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));
    return QIL_OK;
}
