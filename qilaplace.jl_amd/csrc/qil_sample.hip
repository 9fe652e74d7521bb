// Perfect sampling (qil_sample): configurations x drawn with probability |psi_x|^2 / |psi|^2, exactly, by one right-to-left
// environment pass and one left-to-right conditional sweep per batch of samples.  Nothing crosses to the host between sites.
//
//   environments   R_n = [1],  R_{i-1} = sum_s A_i[:, s, :] R_i A_i[:, s, :]^H      (two GEMMs per site, right to left)
//                  each R_i scaled by 1 / trace on the device (only ratios matter); qil_top_k builds the same environments
//                  (qil_dev_right_envs) and also sums the log traces, the log of |psi|^2
//   sweep          per sample r: v = [1];  at site i  w_s = v A_i[:, s, :],  q_s = Re(w_s R_i w_s^H),
//                  s = 0 iff u_{r,i} (q_0 + q_1) < q_0,  v <- w_s / sqrt(q_s),  p_r *= q_s / (q_0 + q_1)
//
// Two routes for the sweep (QIL_SAMPLE_ROUTE=fused / gemm forces one):
//   fused  bonds <= 128 (chosen up to 64 for f64, 32 for c64): ONE kernel per site; a workgroup owns 32 sample rows, T = V A_i (both slices) and T_s R_i on f64 MFMA,
//          T in LDS (transposed, so the second product can take it as its row operand), neither T nor T R_i goes to HBM
//   gemm   any bonds: T = V A_i and U_s = T_s R_i through qil_dev_gemm, then a reduce-and-choose kernel
// Sample rows live column-major (row fastest, ld = rows of the chunk) on both routes.
// Shared: the uniforms and the choice (seeded_uniform, choose) and the GEMM route's row sums (children_row_sums, qil_top_k's
// too) are in qil_device_utils.h, where qil_apply_sample finds the same rule.  Every pool block of a call belongs to the
// qil_scratch of sample_impl; qil_dev_right_envs takes its caller's.
#include "qil_internal.h"
#include "qil_device_utils.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace {

using namespace qil_dev;

// ---- small kernels ---------------------------------------------------------------------------------------------
// v[r] = 1 (column 0 of the sample rows), p[r] = 1
template <class T>
__global__ void start_rows(T* __restrict__ V, double* __restrict__ prob, long long rows) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < rows; t += (long long)gridDim.x * blockDim.x) {
        V[t] = cast_elem<T>(1.0);
        prob[t] = 1.0;
    }
}
// inv[0] = 1 / Re tr(R) (R m x m), or 1 when the trace is not positive (a zero environment stays zero); logsum (nullable)
// accumulates log tr(R) over the sites, so that the unnormalised environment is R e^logsum
template <class T>
__global__ __launch_bounds__(256) void env_trace(const T* __restrict__ R, int m, double* __restrict__ inv, double* __restrict__ logsum) {
    __shared__ double lds[4];
    double v[1] = {0.0};
    for (int j = threadIdx.x; j < m; j += 256) v[0] += re_of(R[j + (long long)m * j]);
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) {
        inv[0] = v[0] > 0.0 ? 1.0 / v[0] : 1.0;
        if (logsum && v[0] > 0.0) logsum[0] += log(v[0]);
    }
}
template <class T>
__global__ void env_scale(T* __restrict__ R, long long total, const double* __restrict__ inv) {
    const double s = inv[0];
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x)
        R[t] = scale_t(R[t], s);
}
// A[alpha, s, beta] -> As[beta + cr (alpha + cl s)]: the fused kernel's column operand, beta fastest
template <class T>
__global__ void site_rows(const T* __restrict__ A, T* __restrict__ As, int cl, int cr) {
    const long long total = 2LL * cl * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int beta = (int)(t % cr);
        const long long u = t / cr;
        const int alpha = (int)(u % cl), s = (int)(u / cl);
        As[t] = A[alpha + (long long)cl * (s + 2LL * beta)];
    }
}

// ---- fused sampling step ----------------------------------------------------------------------------------------
constexpr int kRows = 32;               // sample rows per workgroup: two 16-row MFMA tiles
constexpr int kFusedThreads = 256;
constexpr int kFusedMaxBond = 128;      // chi_r held in LDS (T of 32 rows x 2 x 128 complex = 132 KiB)
constexpr int kFusedAutoMaxF64 = 64, kFusedAutoMaxC64 = 32;   // largest bond the fused route is chosen for when unforced
constexpr int kLdr = kRows + 1;         // LDS pitch of a T column: odd, so the C/D-layout stores spread over the banks

__host__ __device__ constexpr size_t fused_lds_bytes(int cp, bool cx) {
    return (size_t)(cx ? 2 : 1) * 2 * cp * kLdr * 8 + 2 * 8 * kRows * 8 + kRows * 8 + kRows * 4;
}

// One site for kRows sample rows.  v_mfma_f64_16x16x4_f64: lane l supplies A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15],
// and holds D[row = (l >> 4) + 4 reg][col = l & 15].
//   stage 1  T_s (rows x chi_r) = V (rows x chi_l) A_s         tiles (row tile, s, column tile) over the 4 waves -> LDS
//   stage 2  U_s = T_s R  (R Hermitian: R[k][c] = conj(R[c + chi_r k]), read contiguously),  q_s partials per column tile
//   stage 3  per row: q_s, the choice, the bit and the probability; then the chosen row of T, rescaled, is V'
template <class T>
__global__ __launch_bounds__(kFusedThreads) void sample_fused(const T* __restrict__ V, long long rows, int cl, int cr,
                                                              const T* __restrict__ As, const T* __restrict__ R,
                                                              const double* __restrict__ U, uint64_t seed, long long gbase, int n,
                                                              int site, uint8_t* __restrict__ bits, double* __restrict__ prob,
                                                              T* __restrict__ Vn) {
    constexpr bool CX = sizeof(T) == 16;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int CT = (cr + 15) >> 4, CP = 16 * CT;
    double* Tr = reinterpret_cast<double*>(lds_raw);             // T[s][col][row] at (s CP + col) kLdr + row
    double* Ti = Tr + 2 * CP * kLdr;                             // imaginary plane (complex only)
    double* part = Tr + (CX ? 2 : 1) * 2 * CP * kLdr;            // q partials [s][column tile][row]
    double* sscl = part + 2 * 8 * kRows;
    int* ssel = reinterpret_cast<int*>(sscl + kRows);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const long long r0 = (long long)blockIdx.x * kRows;
    const int ntile = 4 * CT;

    // ---- stage 1
    for (int t = wave; t < ntile; t += kFusedThreads / 64) {
        const int rt = t & 1, s = (t >> 1) & 1, ct = t >> 2;
        const long long row = r0 + 16 * rt + li;
        const int col = 16 * ct + li;
        const T* __restrict__ Bs = As + (long long)cr * cl * s;
        d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0};
        for (int k0 = 0; k0 < cl; k0 += 4) {
            const int k = k0 + lk;
            T a{}, b{};
            if (row < rows && k < cl) a = V[row + rows * k];
            if (col < cr && k < cl) b = Bs[col + (long long)cr * k];
            mfma_step(a, b, rr, ii);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = (s * CP + col) * kLdr + 16 * rt + lk + 4 * r;
            Tr[idx] = rr[r];
            if constexpr (CX) Ti[idx] = ii[r];
        }
    }
    __syncthreads();

    // ---- stage 2
    for (int t = wave; t < ntile; t += kFusedThreads / 64) {
        const int rt = t & 1, s = (t >> 1) & 1, ct = t >> 2;
        const int col = 16 * ct + li;
        const double* __restrict__ Tsr = Tr + s * CP * kLdr + 16 * rt;
        const double* __restrict__ Tsi = Ti + s * CP * kLdr + 16 * rt;
        d4 ur = {0, 0, 0, 0}, ui = {0, 0, 0, 0};
        for (int k0 = 0; k0 < cr; k0 += 4) {
            const int k = k0 + lk;                     // k < CP: T is zero past chi_r
            T b{};
            if (col < cr && k < cr) b = R[col + (long long)cr * k];
            const double ar = Tsr[k * kLdr + li], br = re_of(b);
            ur = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, ur, 0, 0, 0);
            if constexpr (CX) {
                const double ai = Tsi[k * kLdr + li], bi = -im_of(b);   // R[k][col] = conj(R[col][k])
                ur = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bi, ur, 0, 0, 0);
                ui = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ui, 0, 0, 0);
                ui = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ui, 0, 0, 0);
            }
        }
        // q_s[row] += sum over this tile's columns of Re(U conj(T)); a row's 16 columns are one DPP row of lanes
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lrow = lk + 4 * r;
            const int idx = col * kLdr + lrow;
            double v = ur[r] * Tsr[idx];
            if constexpr (CX) v = fma(ui[r], Tsi[idx], v);
            v = row16_sum(v);
            if (li == 0) part[(s * 8 + ct) * kRows + 16 * rt + lrow] = v;
        }
    }
    __syncthreads();

    // ---- stage 3
    if (threadIdx.x < kRows) {
        const int r = threadIdx.x;
        const long long row = r0 + r;
        int s = 0;
        double scl = 0.0;
        if (row < rows) {
            double q0 = 0.0, q1 = 0.0;
            for (int ct = 0; ct < CT; ++ct) {
                q0 += part[ct * kRows + r];
                q1 += part[(8 + ct) * kRows + r];
            }
            const double u = U ? U[row * n + site] : seeded_uniform(seed, gbase + row, n, site);
            double f;
            s = choose(q0, q1, u, f, scl);
            bits[row * n + site] = (uint8_t)s;
            prob[row] *= f;
        }
        ssel[r] = s;
        sscl[r] = scl;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kRows * cr; t += kFusedThreads) {
        const int r = t % kRows, beta = t / kRows;
        const long long row = r0 + r;
        if (row < rows) {
            const int idx = (ssel[r] * CP + beta) * kLdr + r;
            const double sc = sscl[r];
            Vn[row + rows * beta] = make_elem(Tr[idx] * sc, CX ? Ti[idx] * sc : 0.0, (T*)nullptr);
        }
    }
}

template <class T>
static int launch_fused(qil_context* ctx, const void* V, long long rows, int cl, int cr, const void* As, const void* R,
                        const double* U, uint64_t seed, long long gbase, int n, int site, uint8_t* bits, double* prob, void* Vn) {
    static qil_lds_grant grant;
    const size_t lds = fused_lds_bytes(16 * ((cr + 15) / 16), sizeof(T) == 16);
    QIL_HIP(grant.ensure(ctx->device, reinterpret_cast<const void*>(&sample_fused<T>), lds));
    hipLaunchKernelGGL(sample_fused<T>, dim3((unsigned)((rows + kRows - 1) / kRows)), dim3(kFusedThreads), lds, qil_stream(ctx),
                       (const T*)V, rows, cl, cr, (const T*)As, (const T*)R, U, seed, gbase, n, site, bits, prob, (T*)Vn);
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

// ---- GEMM route: reduce and choose -------------------------------------------------------------------------------
// T (rows x 2 chi_r) and U_s = T_s R in the layout of children_row_sums (qil_device_utils.h, qil_top_k's reduction too): a
// workgroup owns 32 rows, its 8 groups of 32 threads split the columns; then the choice, and the chosen child rescaled.
constexpr int kChooseRows = 32, kChooseGroups = 8;
template <class T>
__global__ __launch_bounds__(kChooseRows* kChooseGroups) void gemm_choose(const T* __restrict__ Tm, const T* __restrict__ Us,
                                                                          long long rows, int cr, const double* __restrict__ U,
                                                                          uint64_t seed, long long gbase, int n, int site,
                                                                          uint8_t* __restrict__ bits, double* __restrict__ prob,
                                                                          T* __restrict__ Vn) {
    __shared__ double qs[2][kChooseGroups][kChooseRows];
    __shared__ double sscl[kChooseRows];
    __shared__ int ssel[kChooseRows];
    const int r = threadIdx.x % kChooseRows, g = threadIdx.x / kChooseRows;
    const long long row = (long long)blockIdx.x * kChooseRows + r;
    double a = 0.0, b = 0.0;
    const bool mine = children_row_sums<kChooseRows, kChooseGroups>(Tm, Us, rows, cr, qs, a, b);
    if (g == 0) {
        int s = 0;
        double scl = 0.0;
        if (mine) {
            const double u = U ? U[row * n + site] : seeded_uniform(seed, gbase + row, n, site);
            double f;
            s = choose(a, b, u, f, scl);
            bits[row * n + site] = (uint8_t)s;
            prob[row] *= f;
        }
        ssel[r] = s;
        sscl[r] = scl;
    }
    __syncthreads();
    if (row < rows)
        for (int beta = g; beta < cr; beta += kChooseGroups)
            Vn[row + rows * (long long)beta] = scale_t(Tm[row + rows * (ssel[r] + 2LL * beta)], sscl[r]);
}

// ---- right environments (shared with qil_top_k) -------------------------------------------------------------------
template <class T>
static int right_envs(const qil_mps* psi, qil_scratch& tmp, const char* verb, void** Rall, std::vector<long long>& roff,
                      double* log_norm2) {
    qil_context* ctx = psi->ctx;
    const int dt = psi->dtype;
    const size_t e = sizeof(T);
    const int64_t n = psi->n();
    const std::vector<int64_t>& d = psi->dims;
    long long maxT = 1, envsum = 0;
    roff.assign((size_t)n + 1, 0);
    for (int64_t b = 0; b <= n; ++b) {
        roff[(size_t)b] = envsum;
        envsum += d[(size_t)b] * d[(size_t)b];
    }
    for (int64_t i = 0; i < n; ++i) maxT = std::max<long long>(maxT, 2 * d[(size_t)i] * d[(size_t)i + 1]);
    void *Tenv = nullptr, *inv = nullptr;
    QIL_TRY(tmp.alloc((size_t)envsum * e, Rall));
    QIL_TRY(tmp.alloc((size_t)maxT * e, &Tenv));
    QIL_TRY(tmp.alloc(log_norm2 ? 16 : 8, &inv));
    T* Rb = static_cast<T*>(*Rall);
    double* logsum = log_norm2 ? static_cast<double*>(inv) + 1 : nullptr;
    if (logsum) QIL_HIP(hipMemsetAsync(logsum, 0, 8, qil_stream(ctx)));
    QIL_TRY(qil_dev_fill_ones(ctx, dt, Rb + roff[(size_t)n], 1));
    for (int64_t i = n - 1; i >= 0; --i) {
        const int64_t cl = d[(size_t)i], cr = d[(size_t)i + 1];
        const void* A = psi->site[(size_t)i];
        // T (2 chi_l x chi_r) = A (rows alpha + chi_l s) R_{i+1};  R_i (chi_l x chi_l) = T (chi_l x 2 chi_r) A^H
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, 2 * cl, cr, cr, A, 2 * cl, Rb + roff[(size_t)i + 1], cr, Tenv, 2 * cl));
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 2, cl, cl, 2 * cr, Tenv, cl, A, cl, Rb + roff[(size_t)i], cl));
        hipLaunchKernelGGL(env_trace<T>, dim3(1), dim3(256), 0, qil_stream(ctx), (const T*)(Rb + roff[(size_t)i]), (int)cl, (double*)inv,
                           logsum);
        hipLaunchKernelGGL(env_scale<T>, dim3(qil_grid_for(cl * cl)), dim3(256), 0, qil_stream(ctx), Rb + roff[(size_t)i], (long long)(cl * cl),
                           (const double*)inv);
        QIL_HIP(hipGetLastError());
    }
    {
        double h[2] = {0.0, 0.0};
        QIL_TRY(qil_read_back(ctx, h, Rb + roff[0], e));
        QIL_REQUIRE(h[0] > 0.0, QIL_EDOMAIN, "%s: the state has zero norm", verb);
        if (logsum) QIL_TRY(qil_read_back(ctx, log_norm2, logsum, 8));
    }
    tmp.free(Tenv);                                    // the pool recycles in stream order
    tmp.free(inv);
    return QIL_OK;
}

// ---- the call -----------------------------------------------------------------------------------------------------
template <class T>
static int sample_impl(const qil_mps* psi, int64_t nb, uint64_t seed, const double* uniforms, uint8_t* bits_out, double* prob_out) {
    qil_context* ctx = psi->ctx;
    const int dt = psi->dtype;
    const size_t e = sizeof(T);
    const int64_t n = psi->n();
    const std::vector<int64_t>& d = psi->dims;
    long long maxchi = 1, sitesum = 0;
    std::vector<long long> roff, soff((size_t)n);
    for (int64_t b = 0; b <= n; ++b) maxchi = std::max<long long>(maxchi, d[(size_t)b]);
    for (int64_t i = 0; i < n; ++i) {
        soff[(size_t)i] = sitesum;
        sitesum += 2 * d[(size_t)i] * d[(size_t)i + 1];
    }
    // route: the fused kernel holds chi_r <= 128 in LDS.  Measured crossover (n = 24 paired, nb = 2^16, median of 10; MEASUREMENTS
    // section 7): f64 fused 4.9 vs GEMM 5.9 ms at chi 64, 25.1 vs 12.8 at 128; c64 3.4 vs 6.0 at chi 32, 11.0 vs 10.7 at 64 (and
    // 178 vs 155 ms at nb = 2^20) -- past that the 32-row workgroups re-read A_i and R_i from L2 more often than the GEMM tiles do.
    // QIL_SAMPLE_ROUTE=fused / gemm forces one (fused only where it fits).
    const bool fits = maxchi <= kFusedMaxBond;
    bool fused = maxchi <= (dt == QIL_C64 ? kFusedAutoMaxC64 : kFusedAutoMaxF64);
    const char* route = getenv("QIL_SAMPLE_ROUTE");
    if (route && !strcmp(route, "fused")) fused = fits;
    else if (route && !strcmp(route, "gemm")) fused = false;

    // ---- environments, right to left
    qil_scratch tmp(ctx);
    void* Rall = nullptr;
    QIL_TRY(right_envs<T>(psi, tmp, "sample", &Rall, roff, nullptr));
    T* Rb = static_cast<T*>(Rall);

    // ---- the sweep, in chunks of rows (row buffers ~1 GB)
    const long long per_row = (long long)(fused ? 2 : 6) * maxchi * (long long)e + n + 8 + (uniforms ? 8 * n : 0);
    long long chunk = std::max<long long>(kRows, ((1LL << 30) / per_row) / kRows * kRows);
    chunk = std::min<long long>(chunk, nb);
    void *V = nullptr, *Vn = nullptr, *dbits = nullptr, *dprob = nullptr, *dU = nullptr, *Tm = nullptr, *Us = nullptr, *Ast = nullptr;
    QIL_TRY(tmp.alloc((size_t)(chunk * maxchi) * e, &V));
    QIL_TRY(tmp.alloc((size_t)(chunk * maxchi) * e, &Vn));
    QIL_TRY(tmp.alloc((size_t)(chunk * n), &dbits));
    QIL_TRY(tmp.alloc((size_t)chunk * 8, &dprob));
    if (uniforms) QIL_TRY(tmp.alloc((size_t)(chunk * n) * 8, &dU));
    if (fused) {
        QIL_TRY(tmp.alloc((size_t)sitesum * e, &Ast));
        for (int64_t i = 0; i < n; ++i) {
            const int64_t cl = d[(size_t)i], cr = d[(size_t)i + 1];
            hipLaunchKernelGGL(site_rows<T>, dim3(qil_grid_for(2 * cl * cr)), dim3(256), 0, qil_stream(ctx), (const T*)psi->site[(size_t)i],
                               static_cast<T*>(Ast) + soff[(size_t)i], (int)cl, (int)cr);
        }
        QIL_HIP(hipGetLastError());
    } else {
        QIL_TRY(tmp.alloc((size_t)(chunk * 2 * maxchi) * e, &Tm));
        QIL_TRY(tmp.alloc((size_t)(chunk * 2 * maxchi) * e, &Us));
    }
    for (long long r0 = 0; r0 < nb; r0 += chunk) {
        const long long rows = std::min<long long>(chunk, nb - r0);
        if (uniforms)
            QIL_HIP(hipMemcpyAsync(dU, uniforms + r0 * n, (size_t)(rows * n) * 8, hipMemcpyHostToDevice, qil_stream(ctx)));
        hipLaunchKernelGGL(start_rows<T>, dim3(qil_grid_for(rows)), dim3(256), 0, qil_stream(ctx), static_cast<T*>(V), (double*)dprob, rows);
        QIL_HIP(hipGetLastError());
        const double* du = static_cast<const double*>(dU);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t cl = d[(size_t)i], cr = d[(size_t)i + 1];
            const T* R = Rb + roff[(size_t)i + 1];
            if (fused) {
                QIL_TRY(launch_fused<T>(ctx, V, rows, (int)cl, (int)cr, static_cast<const T*>(Ast) + soff[(size_t)i], R, du, seed, r0,
                                        (int)n, (int)i, (uint8_t*)dbits, (double*)dprob, Vn));
            } else {
                // T (rows x 2 chi_r) = V A;  U_s (rows x chi_r) = T_s R  (slice s: offset s rows, ld 2 rows)
                QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, rows, 2 * cr, cl, V, rows, psi->site[(size_t)i], cl, Tm, rows));
                for (int s = 0; s < 2; ++s)
                    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, rows, cr, cr, static_cast<const T*>(Tm) + s * rows, 2 * rows, R, cr,
                                         static_cast<T*>(Us) + s * rows * cr, rows));
                hipLaunchKernelGGL(gemm_choose<T>, dim3((unsigned)((rows + kChooseRows - 1) / kChooseRows)), dim3(kChooseRows * kChooseGroups), 0,
                                   qil_stream(ctx), (const T*)Tm, (const T*)Us, rows, (int)cr, du, seed, r0, (int)n, (int)i,
                                   (uint8_t*)dbits, (double*)dprob, (T*)Vn);
                QIL_HIP(hipGetLastError());
            }
            std::swap(V, Vn);
        }
        QIL_HIP(hipMemcpyAsync(bits_out + r0 * n, dbits, (size_t)(rows * n), hipMemcpyDeviceToHost, qil_stream(ctx)));
        if (prob_out) QIL_HIP(hipMemcpyAsync(prob_out + r0, dprob, (size_t)rows * 8, hipMemcpyDeviceToHost, qil_stream(ctx)));
        QIL_HIP(qil_stream_sync(ctx));
    }
    return QIL_OK;
}

}  // namespace

int qil_dev_right_envs(const qil_mps* psi, qil_scratch& tmp, const char* verb, void** Rall, std::vector<long long>& roff,
                       double* log_norm2) {
    if (psi->dtype == QIL_C64) return right_envs<c64>(psi, tmp, verb, Rall, roff, log_norm2);
    return right_envs<double>(psi, tmp, verb, Rall, roff, log_norm2);
}

extern "C" int qil_sample(const qil_mps* psi, int64_t nb, uint64_t seed, const double* uniforms, uint8_t* bits_out, double* prob_out) {
    QIL_REQUIRE(psi, QIL_EINVAL_ARG, "sample: null argument");
    QIL_REQUIRE(nb >= 0, QIL_EINVAL_ARG, "sample: negative number of samples %lld", (long long)nb);
    if (nb == 0) return QIL_OK;
    QIL_REQUIRE(bits_out, QIL_EINVAL_ARG, "sample: null argument");
    if (uniforms) {
        const int64_t total = nb * psi->n();
        for (int64_t t = 0; t < total; ++t)
            QIL_REQUIRE(uniforms[t] >= 0.0 && uniforms[t] < 1.0, QIL_EINVAL_CONFIG,
                        "sample: uniform %lld (%g) outside [0, 1)", (long long)t, uniforms[t]);
    }
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    if (psi->dtype == QIL_C64) return sample_impl<c64>(psi, nb, seed, uniforms, bits_out, prob_out);
    return sample_impl<double>(psi, nb, seed, uniforms, bits_out, prob_out);
}
