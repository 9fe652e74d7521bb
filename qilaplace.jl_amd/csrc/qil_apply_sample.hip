// Lazy perfect sampling for gfx950: qil_apply_sample draws configurations x with probability |(W psi)_x|^2 / |W psi|^2 without
// forming W psi.  The arithmetic is fixed in include/qilaplace_hip.h.  A call is two passes:
//   environments   R_n = [1];  R_k[alpha', a', a, alpha], the right environment of |W psi|^2 with the tensors k+1 .. n traced, by
//                  ONE right-to-left pass of the mirrored four-product step (qil_norm_env_step, qil_contract.hip: the step
//                  qil_apply_weight_batch's tail takes).  apply_sample_env_scale divides each R_k by its trace
//                  t_k = Re sum R_k[alpha, a, a, alpha] on the device (a fixed-order sum, every workgroup the same one) and raises
//                  the zero-norm flag for a trace that is <= 0 or not finite; the next step starts from the scaled R_k, so a long
//                  chain neither overflows nor underflows.  All R_k, k = 1 .. n - 1, stay for the call.
//   sweep          per row the lazy row vector M[alpha, a] of qil_apply_coefficient_batch ([1] at the start).  At tensor i both
//                  children M_s are qil_lazy_row_step (qil_readout.hip) with the output bit s for every row, packed per tensor
//                  (child s of row r at (s rows + r) P, P = chi_{i+1} D_{i+1}); q_s = Re(m_s R_{i+1} m_s^H), m_s = vec(M_s), in
//                  the index pairing of apply_weight_finish's vector kind (R[p + P q] pairs m[p] with m[q / D + chi (q % D)]);
//                  apply_sample_choose applies qil_sample's rule and writes M_s / sqrt(q_s) as the next M.
// Two routes for the quadratic forms (QIL_APPLY_SAMPLE_ROUTE=fused / gemm forces one; otherwise the operands' bonds decide, see
// fused_by_default below), each the other's check:
//   gemm    U = R^H [M_0 M_1] (P x P by P x 2 rows) through qil_dev_gemm, then apply_sample_reduce: q_s = Re sum U o conj(m_s)
//   fused   apply_sample_score on f64 MFMA: a workgroup owns 32 rows and one 64-column panel of R for BOTH children and loops K
//           over P, so each R tile it reads serves both; the accumulators are multiplied by conj(m_s) and reduced in the epilogue
//           (row16_sum + LDS), one partial per (child, panel, row): U never goes to HBM.  R is read along its contiguous index
//           (column tau(k) = k / chi + D (k % chi) of R is row k of the paired matrix), the rows' tile goes through LDS.
// No atomics anywhere: apply_sample_choose sums the partials in panel order.
// Chunks.  The rows of a call are processed in chunks of
//     chunk = max(1, min(nb, 32768, kChunkBudget / ((5 maxM + maxX) e + 16 ceil(maxM / 64))))     kChunkBudget = 64 MiB
// rows: M, the next M, both children and U (5 maxM), the lead's X and the partials; maxM = max(chi_l D_l, chi_r D_r) and
// maxX = 2 chi_l D_r over the tensors, e the element size of the contraction dtype.
// The start of a call and the scoring step are also qil_apply_top_k's (qil_apply_topk.hip): qil_apply_right_envs (the bond
// sizes of qil_apply_sizes_of, the site scratch, the selector, the environment pass and the read-back of its flag) and
// qil_apply_score_children below, declared in qil_internal.h with the budget and the route they go with.  The uniforms and
// the choice (seeded_uniform, choose) are qil_sample's, in qil_device_utils.h.
// Left out: a device-resident output.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "qil_internal.h"
#include "qil_device_utils.h"

namespace {

using namespace qil_dev;

constexpr int64_t kChunkBudget = 64LL << 20;        // bytes of per-row temporaries per chunk
constexpr int64_t kRightEnvBudget = 16LL << 30;     // bytes of right environments a call may keep (a stated condition)
constexpr int64_t kMaxChunk = 32768;                // rows per chunk: the batch limit of the lead's products
constexpr int kTileRows = 32;                       // rows per workgroup of the scoring kernel: two 16-row MFMA tiles
constexpr int kPanel = 64;                          // columns of R per workgroup: one 16-column MFMA tile per wave
constexpr int kKTile = 32;                          // K elements of the rows' tile staged in LDS per round
constexpr int kScoreThreads = 256;
constexpr int kLdA = kTileRows + 1;                 // LDS pitch of a K line: odd, so the transposing stores spread over the banks
constexpr int kChooseRows = 4;                      // rows per workgroup of the reduce and choose kernels: one wave each

// the column of R that pairs with the vector index k = alpha + chi a: a + D alpha
__device__ __forceinline__ long long paired_column(int k, int chi, int D) { return k / chi + (long long)D * (k % chi); }

// R (P x P, P = chi D) = X / t, t = Re sum_p X[p + P paired_column(p)].  Every workgroup sums the trace in the same fixed order
// and scales its own share; X and R are different buffers.  flag[0] = 1 for a trace that is <= 0 or not finite (R = X then).
// log_trace (nullable): workgroup 0 adds log t to it, so the launches of a pass add up in their stream order.
template <class T>
__global__ __launch_bounds__(256) void apply_sample_env_scale(const T* __restrict__ X, T* __restrict__ R, int chi, int D,
                                                              int* __restrict__ flag, double* __restrict__ log_trace) {
    __shared__ double lds[4];
    const long long P = (long long)chi * D, total = P * P;
    double v[1] = {0.0};
    for (long long p = threadIdx.x; p < P; p += 256) v[0] += re_of(X[p + P * paired_column((int)p, chi, D)]);
    block_sum<1>(v, lds);
    const bool good = v[0] > 0.0 && v[0] <= 1.79769313486231570815e308;
    if (!good && blockIdx.x == 0 && threadIdx.x == 0) flag[0] = 1;
    if (log_trace && good && blockIdx.x == 0 && threadIdx.x == 0) log_trace[0] += log(v[0]);
    const double s = good ? 1.0 / v[0] : 1.0;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += (long long)gridDim.x * 256) R[t] = scale_t(X[t], s);
}

// q_s partials of kTileRows rows against one kPanel-column panel of R, both children.  Mch: child s of row r at (s rows + r) P.
// v_mfma_f64_16x16x4_f64 (mfma_step): lane l supplies X[l & 15][l >> 4] and Y[l >> 4][l & 15] and holds D[(l >> 4) + 4 reg][l & 15].
//   V_s[row][c] = sum_k m_s[row][k] R[c + P paired_column(k)]         wave w owns the columns c of tile w, both row tiles, both s
//   part[(s panels + panel) rows + row] = sum over the panel's c of Re(conj(m_s[row][c]) V_s[row][c])
// Rows, columns and K past the edge are zero-filled by the predicated loads.
template <class T>
__global__ __launch_bounds__(kScoreThreads) void apply_sample_score(const T* __restrict__ Mch, long long rows, int P, int chi, int D,
                                                                    const T* __restrict__ R, double* __restrict__ part) {
    constexpr bool CX = sizeof(T) == 16;
    __shared__ double Ar[2][kKTile][kLdA];
    __shared__ double Ai[CX ? 2 : 1][CX ? kKTile : 1][kLdA];
    __shared__ double red[2][kScoreThreads / 64][kTileRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const long long r0 = (long long)blockIdx.x * kTileRows;
    const int c = (int)blockIdx.y * kPanel + 16 * wave + li;
    d4 ur[2][2], ui[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) ur[s][rt] = d4{0, 0, 0, 0}, ui[s][rt] = d4{0, 0, 0, 0};

    // A round is kKTile lines of K.  The rows' tile of the NEXT round is loaded into registers while this one is multiplied and goes
    // to LDS behind the barrier; the lane's elements of R are replaced by the next round's as soon as the step that read them is
    // issued: the loads of both operands are a whole round ahead of their use.  Lane group lk takes the line
    // 16 (lk & 1) + 8 (lk >> 1) + j at step j, so the two groups of a 32-lane half read LDS lines 16 apart, which at the odd pitch
    // are opposite halves of the bank row.
    constexpr int kSteps = kKTile / 4, kStage = 2 * kTileRows * kKTile / kScoreThreads;
    const int kline = 16 * (lk & 1) + 8 * (lk >> 1);
    const int skk = threadIdx.x % kKTile, srr = threadIdx.x / kKTile;      // the staging thread's K line and first row
    auto load_rows = [&](int k0, T(&v)[kStage]) {
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int rr = (srr + u * (kScoreThreads / kKTile)) % kTileRows, s = u * kScoreThreads / (kKTile * kTileRows);
            const long long row = r0 + rr;
            v[u] = T{};
            if (row < rows && k0 + skk < P) v[u] = Mch[((long long)s * rows + row) * P + k0 + skk];
        }
    };
    auto load_env = [&](int k) {
        T b{};
        if (c < P && k < P) b = R[c + (long long)P * paired_column(k, chi, D)];
        return b;
    };
    T stage[kStage], b[kSteps];
    load_rows(0, stage);
#pragma unroll
    for (int j = 0; j < kSteps; ++j) b[j] = load_env(kline + j);
    for (int k0 = 0; k0 < P; k0 += kKTile) {
        __syncthreads();                               // the previous round's reads
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int rr = (srr + u * (kScoreThreads / kKTile)) % kTileRows, s = u * kScoreThreads / (kKTile * kTileRows);
            Ar[s][skk][rr] = re_of(stage[u]);
            if constexpr (CX) Ai[s][skk][rr] = im_of(stage[u]);
        }
        __syncthreads();
        const bool more = k0 + kKTile < P;
        if (more) load_rows(k0 + kKTile, stage);
#pragma unroll
        for (int j = 0; j < kSteps; ++j) {
            if (k0 + j < P) {                          // else every line of the step lies past P
                const int kk = kline + j;
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) {
                        const T a = make_elem(Ar[s][kk][16 * rt + li], CX ? Ai[s][kk][16 * rt + li] : 0.0, (T*)nullptr);
                        mfma_step(a, b[j], ur[s][rt], ui[s][rt]);
                    }
            }
            if (more) b[j] = load_env(k0 + kKTile + kline + j);
        }
    }
    // a row's 16 columns of a tile are one DPP row of lanes
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lrow = 16 * rt + lk + 4 * r;
                const long long row = r0 + lrow;
                T m{};
                if (row < rows && c < P) m = Mch[((long long)s * rows + row) * P + c];
                double v = ur[s][rt][r] * re_of(m);
                if constexpr (CX) v = fma(ui[s][rt][r], im_of(m), v);
                v = row16_sum(v);
                if (li == 0) red[s][wave][lrow] = v;
            }
    __syncthreads();
    if (threadIdx.x < 2 * kTileRows) {
        const int s = threadIdx.x / kTileRows, r = threadIdx.x % kTileRows;
        if (r0 + r < rows)
            part[((long long)s * gridDim.y + blockIdx.y) * rows + r0 + r] = ((red[s][0][r] + red[s][1][r]) + red[s][2][r]) + red[s][3][r];
    }
}

// GEMM route: part[s rows + row] = Re sum_q conj(U[q]) m[q / D + chi (q % D)] for the column s rows + row of U = R^H [M_0 M_1] and
// of the children; one wave per column, a strided sum per lane and a fixed-order wave sum
template <class T>
__global__ __launch_bounds__(64 * kChooseRows) void apply_sample_reduce(const T* __restrict__ Uc, const T* __restrict__ Mch,
                                                                        long long cols, int P, int chi, int D,
                                                                        double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * kChooseRows + (threadIdx.x >> 6);
    double acc = 0.0;
    if (j < cols)
        for (int q = lane; q < P; q += 64) {
            const T u = Uc[j * P + q], m = Mch[j * P + q / D + chi * (q % D)];
            acc += re_of(u) * re_of(m) + im_of(u) * im_of(m);
        }
    acc = wave_sum(acc);
    if (j < cols && lane == 0) part[j] = acc;
}

// One wave per row, both routes: q_s = the partials summed in panel order, u given or seeded, qil_sample's choice, the bit, the
// probability factor, and the chosen child rescaled as the row's next M (P elements, packed per row)
template <class T>
__global__ __launch_bounds__(64 * kChooseRows) void apply_sample_choose(const double* __restrict__ part, int panels, long long rows,
                                                                        int P, const T* __restrict__ Mch,
                                                                        const double* __restrict__ U, uint64_t seed, long long gbase,
                                                                        int n, int site, uint8_t* __restrict__ bits,
                                                                        double* __restrict__ prob, T* __restrict__ Mn) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kChooseRows + (threadIdx.x >> 6);
    if (row >= rows) return;
    double q0 = 0.0, q1 = 0.0;
    for (int p = 0; p < panels; ++p) {
        q0 += part[(long long)p * rows + row];
        q1 += part[((long long)panels + p) * rows + row];
    }
    const double u = U ? U[row * n + site] : seeded_uniform(seed, gbase + row, n, site);
    double f, scl;
    const int s = choose(q0, q1, u, f, scl);
    if (lane == 0) {
        bits[row * n + site] = (uint8_t)s;
        prob[row] *= f;
    }
    const T* __restrict__ src = Mch + ((long long)s * rows + row) * P;
    for (int k = lane; k < P; k += 64) Mn[row * P + k] = scale_t(src[k], scl);
}

// The default route, a function of the operands' bonds alone.  Measured on one MI355X (MEASUREMENTS section 18; 4096 samples, c64,
// median of 7): fused 42.0 vs gemm 40.6 ms at the natural zT bonds of n = 20 (chi D <= 504), 179 vs 149 ms at chi D = 2048, and
// 5.62 vs 5.67 ms -- inside each other's spread -- at chi D <= 24, where the call is bound by its launches.  The fused kernel
// measured faster at no bond, so no bond selects it; QIL_APPLY_SAMPLE_ROUTE=fused does.
bool fused_by_default(long long /* largest chi D */) { return false; }

template <class T>
int sample_lazy(qil_context* ctx, const qil_mpo* W, const qil_mps* psi, int64_t nb, uint64_t seed, const double* uniforms,
                uint8_t* bits_out, double* prob_out) {
    const int64_t n = psi->n();
    const int dt = sizeof(T) == 16 ? QIL_C64 : QIL_F64;
    const int64_t e = (int64_t)sizeof(T);
    // ---- device memory: everything belongs to `tmp`.  Environments, right to left; R_0 (one number, |W psi|^2 on the scale of
    // R_1) is only checked
    qil_scratch tmp(ctx);
    qil_apply_lazy lz;
    int bad = 0;
    QIL_TRY(qil_apply_right_envs(ctx, tmp, dt, W, psi, lz, &bad, nullptr));
    QIL_REQUIRE(bad == 0, QIL_EDOMAIN, "apply_sample: the transformed state has zero norm");
    const long long maxM = lz.b.maxM, maxX = lz.b.maxX;
    const bool fused = qil_apply_score_fused(maxM);
    const long long maxPanels = qil_apply_score_panels(maxM);
    const int64_t chunk = qil_apply_chunk_rows(nb, (5 * maxM + maxX) * e + 16 * maxPanels);

    // ---- the sweep, in chunks of rows
    void *M0 = nullptr, *M1 = nullptr, *Mch = nullptr, *Xb = nullptr, *Uc = nullptr, *part = nullptr, *dbits = nullptr, *dprob = nullptr,
         *dU = nullptr;
    QIL_TRY(tmp.alloc((size_t)(chunk * maxM * e), &M0));
    QIL_TRY(tmp.alloc((size_t)(chunk * maxM * e), &M1));
    QIL_TRY(tmp.alloc((size_t)(chunk * 2 * maxM * e), &Mch));
    QIL_TRY(tmp.alloc((size_t)(chunk * maxX * e), &Xb));
    if (!fused) QIL_TRY(tmp.alloc((size_t)(chunk * 2 * maxM * e), &Uc));
    QIL_TRY(tmp.alloc((size_t)(chunk * 2 * (fused ? maxPanels : 1) * 8), &part));
    QIL_TRY(tmp.alloc((size_t)(chunk * n), &dbits));
    QIL_TRY(tmp.alloc((size_t)chunk * 8, &dprob));
    if (uniforms) QIL_TRY(tmp.alloc((size_t)(chunk * n) * 8, &dU));
    for (int64_t r0 = 0; r0 < nb; r0 += chunk) {
        const int64_t nr = std::min<int64_t>(chunk, nb - r0);
        if (uniforms) QIL_HIP(hipMemcpyAsync(dU, uniforms + r0 * n, (size_t)(nr * n) * 8, hipMemcpyHostToDevice, qil_stream(ctx)));
        T *Mc = static_cast<T*>(M0), *Mn = static_cast<T*>(M1);
        QIL_TRY(qil_dev_fill_ones(ctx, dt, Mc, nr));
        QIL_TRY(qil_dev_fill_ones(ctx, QIL_F64, dprob, nr));
        for (int64_t i = 0; i < n; ++i) {
            const int64_t cr = psi->dims[(size_t)i + 1], Dr = W->dims[(size_t)i + 1], P = cr * Dr;
            T* child = static_cast<T*>(Mch);
            for (int s = 0; s < 2; ++s)
                QIL_TRY(qil_lazy_row_step(ctx, dt, W, psi, i, Mc, child + s * nr * P, Xb, lz.Wc, lz.As, nr, lz.both + s, 0));
            int panels = 1;
            QIL_TRY(qil_apply_score_children(ctx, dt, fused, child, nr, cr, Dr, lz.Rk[(size_t)i + 1], Uc, (double*)part, &panels));
            hipLaunchKernelGGL(apply_sample_choose<T>, dim3((unsigned)((nr + kChooseRows - 1) / kChooseRows)), dim3(64 * kChooseRows), 0,
                               qil_stream(ctx), (const double*)part, panels, (long long)nr, (int)P, (const T*)child, (const double*)dU,
                               seed, (long long)r0, (int)n, (int)i, (uint8_t*)dbits, (double*)dprob, Mn);
            QIL_HIP(hipGetLastError());
            std::swap(Mc, Mn);
        }
        QIL_HIP(hipMemcpyAsync(bits_out + r0 * n, dbits, (size_t)(nr * n), hipMemcpyDeviceToHost, qil_stream(ctx)));
        if (prob_out) QIL_HIP(hipMemcpyAsync(prob_out + r0, dprob, (size_t)nr * 8, hipMemcpyDeviceToHost, qil_stream(ctx)));
        QIL_HIP(qil_stream_sync(ctx));
    }
    return QIL_OK;
}

}  // namespace

// ---- the steps shared with qil_apply_top_k (qil_internal.h) ----------------------------------------------------------------
int64_t qil_apply_env_budget() {
    int64_t budget = kRightEnvBudget;                  // QIL_APPLY_SAMPLE_RENV_BYTES: read on each call
    if (const char* v = getenv("QIL_APPLY_SAMPLE_RENV_BYTES")) {
        char* end = nullptr;
        const long long b = strtoll(v, &end, 10);
        if (end != v && b >= 0) budget = b;
    }
    return budget;
}

double qil_apply_env_bytes(const qil_mpo* W, const qil_mps* psi) {   // e sum_k (chi_k D_k)^2, k = 1 .. n - 1
    const bool cx = W->dtype == QIL_C64 || psi->dtype == QIL_C64;
    double need = 0.0;
    for (int64_t k = 1; k < psi->n(); ++k) {
        const double P = (double)psi->dims[(size_t)k] * (double)W->dims[(size_t)k];
        need += P * P * (cx ? 16.0 : 8.0);
    }
    return need;
}

qil_apply_bond_sizes qil_apply_sizes_of(const qil_mpo* W, const qil_mps* psi) {
    return qil_apply_sizes_of(psi->n(), psi->dims.data(), W->dims.data());
}
qil_apply_bond_sizes qil_apply_sizes_of(int64_t n, const int64_t* chain_dims, const int64_t* op_dims) {
    qil_apply_bond_sizes b;
    for (int64_t i = 0; i < n; ++i) {
        const long long cl = chain_dims[i], cr = chain_dims[i + 1];
        const long long Dl = op_dims[i], Dr = op_dims[i + 1];
        b.maxM = std::max({b.maxM, cl * Dl, cr * Dr});
        b.maxX = std::max(b.maxX, 2 * cl * Dr);
        b.maxW = std::max(b.maxW, 4 * Dl * Dr);
        b.maxA = std::max(b.maxA, 2 * cl * cr);
    }
    return b;
}

int64_t qil_apply_score_panels(int64_t P) { return (P + kPanel - 1) / kPanel; }

int64_t qil_apply_chunk_rows(int64_t rows, int64_t per_row_bytes) {
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(rows, kMaxChunk), kChunkBudget / per_row_bytes));
}

bool qil_apply_score_fused(long long max_bond) {
    const char* route = getenv("QIL_APPLY_SAMPLE_ROUTE");
    if (route && !strcmp(route, "fused")) return true;
    if (route && !strcmp(route, "gemm")) return false;
    return fused_by_default(max_bond);
}

template <class T>
static int right_envs(qil_context* ctx, qil_scratch& tmp, const qil_mpo* W, const qil_mps* psi, void* At, void* Wd, void* Wr,
                      std::vector<void*>& Rk, int* flag, double* log_trace) {
    const int64_t n = psi->n();
    const int dt = sizeof(T) == 16 ? QIL_C64 : QIL_F64;
    const int64_t e = (int64_t)sizeof(T);
    auto bond = [&](int64_t k) { return psi->dims[(size_t)k] * W->dims[(size_t)k]; };
    long long maxPass = 1;
    for (int64_t i = 0; i < n; ++i) {
        const long long cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        const long long Dl = W->dims[(size_t)i], Dr = W->dims[(size_t)i + 1];
        maxPass = std::max({maxPass, cr * cr * Dr * Dr, 2 * cr * Dr * Dr * cl, 2 * cr * Dr * Dl * cl, 2 * cr * Dl * Dl * cl, cl * cl * Dl * Dl});
    }
    Rk.assign((size_t)n + 1, nullptr);
    for (int64_t k = 1; k <= n; ++k) QIL_TRY(tmp.alloc((size_t)(bond(k) * bond(k) * e), &Rk[(size_t)k]));
    // right to left; R_0 (one number, |W psi|^2 on the scale of R_1) only serves the flag and the log trace
    void *X = nullptr, *Y = nullptr;
    QIL_TRY(tmp.alloc((size_t)(maxPass * e), &X));
    QIL_TRY(tmp.alloc((size_t)(maxPass * e), &Y));
    QIL_HIP(hipMemsetAsync(flag, 0, sizeof(int), qil_stream(ctx)));
    if (log_trace) QIL_HIP(hipMemsetAsync(log_trace, 0, sizeof(double), qil_stream(ctx)));
    QIL_TRY(qil_dev_fill_ones(ctx, dt, Rk[(size_t)n], 1));
    for (int64_t i = n - 1; i >= 0; --i) {
        const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1], Dl = W->dims[(size_t)i], Dr = W->dims[(size_t)i + 1];
        QIL_TRY(qil_put_mps_site(ctx, dt, psi, i, QIL_SITE_REVERSED, At));
        QIL_TRY(qil_put_mpo_site(ctx, dt, W, i, QIL_SITE_REVERSED, Wd));
        QIL_TRY(qil_put_mpo_site(ctx, dt, W, i, QIL_SITE_REV_SWAPPED, Wr));
        QIL_TRY(qil_norm_env_step(ctx, dt, cr, cl, Dr, Dl, 1, At, Wd, Wr, Rk[(size_t)i + 1], Y, X, X));
        T* dst = static_cast<T*>(i > 0 ? Rk[(size_t)i] : Y);
        hipLaunchKernelGGL(apply_sample_env_scale<T>, dim3(qil_grid_for(cl * Dl * cl * Dl)), dim3(256), 0, qil_stream(ctx),
                           (const T*)X, dst, (int)cl, (int)Dl, flag, log_trace);
        QIL_HIP(hipGetLastError());
    }
    tmp.free(X);                                       // the pool recycles in stream order
    tmp.free(Y);
    return QIL_OK;
}

int qil_apply_right_envs(qil_context* ctx, qil_scratch& tmp, int dt, const qil_mpo* W, const qil_mps* psi, qil_apply_lazy& lz,
                         int* bad, double** log_trace) {
    const size_t e = qil_elem_size(dt);
    void *dflag = nullptr, *dlog = nullptr, *dsel = nullptr;
    lz.b = qil_apply_sizes_of(W, psi);
    if (psi->dtype != dt) QIL_TRY(tmp.alloc((size_t)lz.b.maxA * e, &lz.As));
    QIL_TRY(tmp.alloc((size_t)lz.b.maxA * e, &lz.At));
    QIL_TRY(tmp.alloc((size_t)lz.b.maxW * e, &lz.Wd));
    QIL_TRY(tmp.alloc((size_t)lz.b.maxW * e, &lz.Wr));
    QIL_TRY(tmp.alloc((size_t)lz.b.maxW * e, &lz.Wc));
    QIL_TRY(tmp.alloc(sizeof(int), &dflag));
    if (log_trace) QIL_TRY(tmp.alloc(sizeof(double), &dlog));
    const uint8_t both[2] = {0, 1};                    // the output bit of every row of a child's step (selector step 0)
    QIL_TRY(qil_upload_bytes(tmp, both, 2, &dsel));
    lz.both = static_cast<const uint8_t*>(dsel);
    if (log_trace) *log_trace = static_cast<double*>(dlog);
    if (dt == QIL_C64) QIL_TRY(right_envs<c64>(ctx, tmp, W, psi, lz.At, lz.Wd, lz.Wr, lz.Rk, (int*)dflag, (double*)dlog));
    else QIL_TRY(right_envs<double>(ctx, tmp, W, psi, lz.At, lz.Wd, lz.Wr, lz.Rk, (int*)dflag, (double*)dlog));
    return qil_read_back(ctx, bad, dflag, sizeof(int));
}

template <class T>
static int score_children(qil_context* ctx, bool fused, const T* child, int64_t nr, int64_t cr, int64_t Dr, const T* R, T* Uc,
                          double* part, int* panels) {
    const int dt = sizeof(T) == 16 ? QIL_C64 : QIL_F64;
    const int64_t P = cr * Dr;
    *panels = 1;
    if (fused) {
        *panels = (int)qil_apply_score_panels(P);
        hipLaunchKernelGGL(apply_sample_score<T>, dim3((unsigned)((nr + kTileRows - 1) / kTileRows), (unsigned)*panels),
                           dim3(kScoreThreads), 0, qil_stream(ctx), child, (long long)nr, (int)P, (int)cr, (int)Dr, R, part);
    } else {
        QIL_TRY(qil_dev_gemm(ctx, dt, 2, 0, P, 2 * nr, P, R, P, child, P, Uc, P));
        hipLaunchKernelGGL(apply_sample_reduce<T>, dim3((unsigned)((2 * nr + kChooseRows - 1) / kChooseRows)),
                           dim3(64 * kChooseRows), 0, qil_stream(ctx), (const T*)Uc, child, (long long)(2 * nr), (int)P, (int)cr,
                           (int)Dr, part);
    }
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

int qil_apply_score_children(qil_context* ctx, int dt, bool fused, const void* children, int64_t rows, int64_t chi, int64_t D,
                             const void* R, void* U, double* part, int* panels) {
    if (dt == QIL_C64) return score_children<c64>(ctx, fused, (const c64*)children, rows, chi, D, (const c64*)R, (c64*)U, part, panels);
    return score_children<double>(ctx, fused, (const double*)children, rows, chi, D, (const double*)R, (double*)U, part, panels);
}

extern "C" int qil_apply_sample(const qil_mpo* W, const qil_mps* psi, int64_t nb, uint64_t seed, const double* uniforms,
                                uint8_t* bits_out, double* prob_out) {
    QIL_REQUIRE(W && psi && (nb <= 0 || bits_out), QIL_EINVAL_ARG, "apply_sample: null argument");
    QIL_REQUIRE(nb >= 0, QIL_EINVAL_ARG, "apply_sample: negative number of samples %lld", (long long)nb);
    QIL_TRY(qil_check_apply_operands(W, psi));
    const int64_t n = psi->n();
    if (uniforms)
        for (int64_t t = 0; t < nb * n; ++t)
            QIL_REQUIRE(uniforms[t] >= 0.0 && uniforms[t] < 1.0, QIL_EINVAL_CONFIG, "apply_sample: uniform %lld (%g) outside [0, 1)",
                        (long long)t, uniforms[t]);
    if (nb == 0) return QIL_OK;
    const bool cx = W->dtype == QIL_C64 || psi->dtype == QIL_C64;
    const int64_t budget = qil_apply_env_budget();
    const double need = qil_apply_env_bytes(W, psi);
    QIL_REQUIRE(need <= (double)budget, QIL_ENOMEM,
                "apply_sample: the right environments need %.0f bytes, above the %lld allowed (QIL_APPLY_SAMPLE_RENV_BYTES raises it)",
                need, (long long)budget);
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    if (cx) return sample_lazy<c64>(ctx, W, psi, nb, seed, uniforms, bits_out, prob_out);
    return sample_lazy<double>(ctx, W, psi, nb, seed, uniforms, bits_out, prob_out);
}
