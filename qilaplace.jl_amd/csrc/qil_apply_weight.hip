// Lazy Born weights for gfx950: qil_apply_weight_batch returns, per spec row, amplitude^2 times the sum of |(W psi)_x|^2 over the
// configurations x that agree with the row, without forming W psi.  The contraction and its order are fixed in
// include/qilaplace_hip.h.  Every row is three parts; the route through them depends on the row's spec and the shapes only:
//   lead     the leading run of fixed sites carries the lazy row vector M_r[alpha, a] of qil_apply_coefficient_batch: two
//            strided-batch GEMMs per site (qil_lazy_row_step, shared with qil_readout.hip).  The rows of a call are sorted by the
//            length of that run, longest first, so the rows still in the lead at a site are a prefix of their chunk.
//   middle   at the row's first traced site apply_weight_seed forms E[alpha', a', a, alpha] = conj(M[alpha', a']) M[alpha, a], the
//            layout of qil_apply_norm; every further site up to the row's tail runs its four products (T1 = E A, T2 = T1 W,
//            T3 = T2 conj(Wr), E' = A^H T3: qil_norm_env_ket / qil_norm_env_bra, qil_contract.hip) for all rows in the middle at once.  The buffers are packed per site -- row slot j's
//            block sits at j * (block size of this site) -- so the row index and the batch index of each product collapse into
//            one strided batch, and E' is ONE product.  Between T2 and T3 apply_weight_mask zeroes the s_out != bit half of T2 for
//            the rows whose site is fixed: ket and bra share the output leg, so masking one side is the projector.  Rows enter
//            at the end of the slot list (seeded in place); rows that leave are dropped from its end, and only when a row leaves
//            from the inside apply_weight_gather copies the survivors' blocks into the other buffer.
//   tail     R_k[alpha', a', a, alpha], the right environment of |W psi|^2 with the sites k+1 .. n all traced, is shared by all
//            rows: ONE right-to-left pass per call (the same step with left and right exchanged, R_n = [1]) from n down to the
//            leftmost R_k kept.
//            Kept are the R_k at which some row's trailing run of traced sites starts, from the right, while their total stays
//            within kRightEnvBudget bytes (QIL_APPLY_WEIGHT_RENV_BYTES overrides it, read on each call).  A row stops at the first
//            kept R_k inside its trailing run (t_r); with none kept it walks to the end as middle.
//   finish   apply_weight_finish, one workgroup per row, a strided sum per thread and an LDS tree, no atomics:
//            amplitude^2 Re sum E o R_t;  Re(m R_t m^H) with m = vec(M) for a row with no middle;  Re E[0] for t_r = n;
//            |M|^2 for a row with no traced site.
// Chunks.  The rows of a call are processed in chunks of
//     chunk = max(1, min(nb, 32768, kChunkBudget / ((2 maxMid + 2 maxM + maxX) e)))           kChunkBudget = 64 MiB
// rows, e the element size of the contraction dtype and, over the sites i (chi_l, chi_r the bonds of psi, D_l, D_r those of W):
//     maxMid = max(chi_l^2 D_l^2, 2 chi_l D_l^2 chi_r, 2 chi_l D_l D_r chi_r, 2 chi_l D_r^2 chi_r, chi_r^2 D_r^2)   E, T1, T2, T3, E'
//     maxM   = max(chi_l D_l, chi_r D_r),   maxX = 2 chi_l D_r                                                   the lead's M and X
// A result is bit-identical from run to run; its rounding may differ between chunkings (the batch width of a product picks its
// tiling) and between kept and not-kept R_k (another order of the same sum).
// Left out: weights of operators, a device-resident result.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "qil_internal.h"
#include "qil_device_utils.h"

namespace {

using namespace qil_dev;

constexpr int64_t kChunkBudget = 64LL << 20;        // bytes of per-row temporaries (E / T1 / T2 / T3 ping-pong, M, X) per chunk
constexpr int64_t kRightEnvBudget = 256LL << 20;    // bytes of kept right environments R_k per call
constexpr int64_t kMaxChunk = 32768;                // rows per chunk: the batch limit of the lead's products
constexpr int kFinishThreads = 256;
enum { kNoTrace = 0, kDensity = 1, kVector = 2 };   // how a row finishes

__device__ __forceinline__ double re_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double re_mul(c64 a, c64 b) { return a.re * b.re - a.im * b.im; }

// E_slot[alpha', a', a, alpha] = conj(M_j[alpha', a']) M_j[alpha, a] for the slots first .. first + count - 1, j = act[slot] the
// row's place in the chunk (its M block, P = cl Dl elements, M_j[alpha, a] at alpha + cl a)
template <class T>
__global__ void apply_weight_seed(const int* __restrict__ act, int first, long long count, const T* __restrict__ M,
                                  T* __restrict__ E, int cl, int Dl) {
    const long long P = (long long)cl * Dl, PP = P * P, total = count * PP;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long slot = first + t / PP, idx = t % PP;
        const T* __restrict__ m = M + (long long)act[slot] * P;
        const long long pb = idx % P, q = idx / P;
        const long long a = q % Dl, al = q / Dl;
        E[slot * PP + idx] = cmul_add(T{}, conj_t(m[pb]), m[al + cl * a]);
    }
}

// out block d = in block src[d], blocks of S elements: the survivors of the slot list, packed again
template <class T>
__global__ void apply_weight_gather(const int* __restrict__ src, long long count, const T* __restrict__ in, T* __restrict__ out,
                                    long long S) {
    const long long total = count * S;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long d = t / S;
        out[t] = in[(long long)src[d] * S + t % S];
    }
}

// T2_slot[x, s_out, y] (x < X = cl Dl, y < Y = Dr cr) = 0 for s_out != bit where the slot's row fixes this site; spec = the
// chunk's rows (n bytes each), act[slot] the row's place in the chunk
template <class T>
__global__ void apply_weight_mask(T* __restrict__ T2, const int* __restrict__ act, long long count, long long X, long long Y,
                                  const uint8_t* __restrict__ spec, int n, int site) {
    const long long half = X * Y, total = count * half;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long slot = t / half, rem = t % half;
        const int bit = spec[(long long)act[slot] * n + site];
        if (bit < 2) T2[slot * 2 * half + rem % X + X * ((1 - bit) + 2 * (rem / X))] = T{};
    }
}

// One workgroup per finishing row; tab holds (out index, kind, slot, -) per row.  P = cl Dl of the bond the rows finish at, R that
// bond's right environment (null at bond n: R_n = [1], P = 1).  Every thread sums its strided share in a fixed order, then an LDS
// tree: no atomics, the same bits on every run.
template <class T>
__global__ __launch_bounds__(kFinishThreads) void apply_weight_finish(const int* __restrict__ tab, const T* __restrict__ E,
                                                                      const T* __restrict__ M, const T* __restrict__ R, int cl,
                                                                      int Dl, double amp2, double* __restrict__ out) {
    __shared__ double red[kFinishThreads];
    const int* __restrict__ e = tab + 4LL * blockIdx.x;
    const int kind = e[1], tid = threadIdx.x;
    const long long slot = e[2], P = (long long)cl * Dl;
    double acc = 0.0;
    if (kind == kNoTrace) {
        if (tid == 0) acc = abs2_t(M[slot * P]);
    } else if (kind == kDensity) {
        const T* __restrict__ Er = E + slot * P * P;
        for (long long idx = tid; idx < P * P; idx += kFinishThreads) acc += R ? re_mul(Er[idx], R[idx]) : re_of(Er[idx]);
    } else {
        const T* __restrict__ m = M + slot * P;
        for (long long q = tid; q < P; q += kFinishThreads) {
            const T* __restrict__ col = R + P * q;
            T inner{};
            for (long long p = 0; p < P; ++p) inner = cmul_add(inner, conj_t(m[p]), col[p]);
            acc += re_mul(m[q / Dl + cl * (q % Dl)], inner);
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kFinishThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[e[0]] = amp2 * red[0];
}

struct RowPlan {
    int64_t f;      // the first traced site (n: none), i.e. the length of the lead
    int64_t k;      // where the trailing run of traced sites starts (n: the last site is fixed)
    int64_t t;      // the bond the row finishes at: the first kept R_k with k >= its k, else n
    int64_t row;    // its place in the caller's batch
};

// the per-site operand scratch of a call (element counts are the maxima over the sites)
template <class T>
struct SiteScratch {
    T *As = nullptr, *At = nullptr, *Wd = nullptr, *Wr = nullptr, *Wc = nullptr;
};

// the right-to-left pass: R_k for every kept k into Rk[k] (allocated by the caller), from bond n down to kmin
template <class T>
int right_environments(qil_context* ctx, int dt, const qil_mpo* W, const qil_mps* psi, const std::vector<T*>& Rk, int64_t kmin,
                       const SiteScratch<T>& sc, T* X, T* Y) {
    const int64_t n = psi->n();
    const T* cur = X;                                  // R_n = [1] (never kept: a row that reaches bond n reads Re E[0])
    QIL_TRY(qil_dev_fill_ones(ctx, dt, X, 1));
    for (int64_t i = n - 1; i >= kmin; --i) {
        QIL_TRY(qil_put_mps_site(ctx, dt, psi, i, QIL_SITE_REVERSED, sc.At));             // At[beta, sigma, s]
        QIL_TRY(qil_put_mpo_site(ctx, dt, W, i, QIL_SITE_REVERSED, sc.Wd));               // Wk[b, sigma, tau, a]
        QIL_TRY(qil_put_mpo_site(ctx, dt, W, i, QIL_SITE_REV_SWAPPED, sc.Wr));            // Wb[b', tau, sigma', a']
        // the step of the middle with left and right exchanged: R_i[s', a', a, s] from R_{i+1}[beta', b', b, beta]
        T* dst = Rk[(size_t)i] ? Rk[(size_t)i] : X;
        QIL_TRY(qil_norm_env_step(ctx, dt, psi->dims[(size_t)i + 1], psi->dims[(size_t)i], W->dims[(size_t)i + 1], W->dims[(size_t)i], 1,
                                  sc.At, sc.Wd, sc.Wr, cur, Y, X, dst));
        cur = dst;
    }
    return QIL_OK;
}

template <class T>
int weigh(qil_context* ctx, const qil_mpo* W, const qil_mps* psi, int64_t nb, const uint8_t* spec, int64_t renv_budget,
          double* out) {
    const int64_t n = psi->n();
    const int dt = sizeof(T) == 16 ? QIL_C64 : QIL_F64;
    const int64_t e = (int64_t)sizeof(T);
    // ---- the rows: lead length, tail start, sorted by lead length (longest first; stable, so the order is the spec's alone)
    std::vector<RowPlan> rows((size_t)nb);
    for (int64_t r = 0; r < nb; ++r) {
        const uint8_t* s = spec + r * n;
        int64_t f = n, k = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (s[i] == 2 && f == n) f = i;
            if (s[i] != 2) k = i + 1;
        }
        rows[(size_t)r] = RowPlan{f, k, n, r};
    }
    std::stable_sort(rows.begin(), rows.end(), [](const RowPlan& a, const RowPlan& b) { return a.f > b.f; });
    // ---- which right environments are kept: those some row's tail starts at, from the right, within the budget
    auto env_elems = [&](int64_t k) { return psi->dims[(size_t)k] * W->dims[(size_t)k] * W->dims[(size_t)k] * psi->dims[(size_t)k]; };
    std::vector<char> wanted((size_t)n + 1, 0), kept((size_t)n + 1, 0);
    for (const RowPlan& r : rows)
        if (r.f < n && r.k < n) wanted[(size_t)r.k] = 1;
    int64_t kmin = n + 1, total = 0;
    for (int64_t k = n - 1; k >= 0; --k) {
        if (!wanted[(size_t)k]) continue;
        if (total + env_elems(k) * e > renv_budget) break;
        total += env_elems(k) * e;
        kept[(size_t)k] = 1;
        kmin = k;
    }
    for (RowPlan& r : rows)
        if (r.f < n)
            for (int64_t k = r.k; k < n; ++k)
                if (kept[(size_t)k]) {
                    r.t = k;
                    break;
                }
    // ---- sizes
    long long maxMid = 1, maxM = 1, maxX = 1, maxW = 1, maxA = 1, maxPass = 1;
    for (int64_t i = 0; i < n; ++i) {
        const long long cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        const long long Dl = W->dims[(size_t)i], Dr = W->dims[(size_t)i + 1];
        maxMid = std::max({maxMid, cl * cl * Dl * Dl, 2 * cl * Dl * Dl * cr, 2 * cl * Dl * Dr * cr, 2 * cl * Dr * Dr * cr, cr * cr * Dr * Dr});
        maxM = std::max({maxM, cl * Dl, cr * Dr});
        maxX = std::max(maxX, 2 * cl * Dr);
        maxW = std::max(maxW, 4 * Dl * Dr);
        maxA = std::max(maxA, 2 * cl * cr);
        if (i >= kmin)
            maxPass = std::max({maxPass, cr * cr * Dr * Dr, 2 * cr * Dr * Dr * cl, 2 * cr * Dr * Dl * cl, 2 * cr * Dl * Dl * cl, cl * cl * Dl * Dl});
    }
    const int64_t per_row = (2 * maxMid + 2 * maxM + maxX) * e;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nb, kMaxChunk), kChunkBudget / per_row));
    // ---- device memory: everything belongs to `tmp`
    qil_scratch tmp(ctx);
    void *dspec = nullptr, *dout = nullptr;
    QIL_TRY(tmp.alloc((size_t)nb * sizeof(double), &dout));
    SiteScratch<T> sc;
    QIL_TRY(tmp.alloc((size_t)maxA * e, (void**)&sc.As));
    QIL_TRY(tmp.alloc((size_t)maxA * e, (void**)&sc.At));
    QIL_TRY(tmp.alloc((size_t)maxW * e, (void**)&sc.Wd));
    QIL_TRY(tmp.alloc((size_t)maxW * e, (void**)&sc.Wr));
    QIL_TRY(tmp.alloc((size_t)maxW * e, (void**)&sc.Wc));
    std::vector<T*> Rk((size_t)n + 1, nullptr);
    for (int64_t k = 0; k < n; ++k)
        if (kept[(size_t)k]) QIL_TRY(tmp.alloc((size_t)(env_elems(k) * e), (void**)&Rk[(size_t)k]));
    if (kmin <= n) {
        void *X = nullptr, *Y = nullptr;
        QIL_TRY(tmp.alloc((size_t)(maxPass * e), &X));
        QIL_TRY(tmp.alloc((size_t)(maxPass * e), &Y));
        QIL_TRY(right_environments<T>(ctx, dt, W, psi, Rk, kmin, sc, static_cast<T*>(X), static_cast<T*>(Y)));
        tmp.free(X);                                   // the pool recycles in stream order
        tmp.free(Y);
    }
    // the spec in sorted order (the lead's products pick the output bit of row j of a chunk at dspec[(r0 + j) n + i])
    std::vector<uint8_t> sorted((size_t)std::max<int64_t>(nb * n, 1));
    for (int64_t j = 0; j < nb; ++j) std::copy(spec + rows[(size_t)j].row * n, spec + (rows[(size_t)j].row + 1) * n, sorted.begin() + j * n);
    QIL_TRY(qil_upload_bytes(tmp, sorted.data(), (size_t)(nb * n), &dspec));
    void* buf[5] = {};                                 // P, Q (the middle's ping-pong), M0, M1, X (the lead)
    const long long bufElems[5] = {maxMid, maxMid, maxM, maxM, maxX};
    for (int b = 0; b < 5; ++b) QIL_TRY(tmp.alloc((size_t)(chunk * bufElems[b] * e), &buf[b]));
    T *P = static_cast<T*>(buf[0]), *Q = static_cast<T*>(buf[1]);
    const double amp2 = psi->amplitude * psi->amplitude;
    const uint8_t* dsp = static_cast<const uint8_t*>(dspec);
    double* dres = static_cast<double*>(dout);

    for (int64_t r0 = 0; r0 < nb; r0 += chunk) {
        const int64_t nr = std::min<int64_t>(chunk, nb - r0);
        const RowPlan* rw = rows.data() + r0;
        // ---- the chunk's plan, one table: per bond the finishing rows, the survivors' source slots, the slot list
        struct BondPlan {
            size_t fin = 0, nfin = 0, gat = 0, ngat = 0, act = 0, nact = 0, nsurv = 0;
            bool gather = false, any_fixed = false;
            int64_t nlead = 0;
        };
        std::vector<BondPlan> bp((size_t)n + 1);
        std::vector<int> tab;
        std::vector<int> active;                       // slot -> the row's place in the chunk
        for (int64_t i = 0; i <= n; ++i) {
            BondPlan& b = bp[(size_t)i];
            b.fin = tab.size();
            std::vector<int> surv_src, surv;
            for (size_t s = 0; s < active.size(); ++s) {
                const RowPlan& r = rw[active[s]];
                if (r.t == i) {
                    tab.insert(tab.end(), {(int)r.row, (int)kDensity, (int)s, 0});
                } else {
                    surv_src.push_back((int)s);
                    surv.push_back(active[s]);
                }
            }
            std::vector<int> enter;
            for (int64_t j = 0; j < nr; ++j) {
                const RowPlan& r = rw[j];
                if (r.f == n && i == n) tab.insert(tab.end(), {(int)r.row, (int)kNoTrace, (int)j, 0});
                else if (r.f == i && r.t == i) tab.insert(tab.end(), {(int)r.row, (int)kVector, (int)j, 0});
                else if (r.f == i) enter.push_back((int)j);
                if (r.f > i) b.nlead = j + 1;          // sorted by f, longest first: a prefix
            }
            b.nfin = (tab.size() - b.fin) / 4;
            if (i == n) break;
            // the rows that finish first go last, so that they leave from the end of the list
            std::stable_sort(enter.begin(), enter.end(), [&](int x, int y) { return rw[x].t > rw[y].t; });
            b.nsurv = surv.size();
            for (size_t s = 0; s < surv_src.size(); ++s) b.gather = b.gather || surv_src[s] != (int)s;
            if (b.gather) {
                b.gat = tab.size();
                b.ngat = surv_src.size();
                tab.insert(tab.end(), surv_src.begin(), surv_src.end());
            }
            active = surv;
            active.insert(active.end(), enter.begin(), enter.end());
            b.act = tab.size();
            b.nact = active.size();
            tab.insert(tab.end(), active.begin(), active.end());
            for (int j : active) b.any_fixed = b.any_fixed || spec[rw[j].row * n + i] != 2;
        }
        if (tab.empty()) tab.push_back(0);
        qil_dev_table dtab(ctx);
        QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(int)));
        const int* dt_tab = dtab.as<int>();
        // ---- the walk
        T *Mc = static_cast<T*>(buf[2]), *Mn = static_cast<T*>(buf[3]);
        T *E = P, *O = Q;                              // E holds the slots' environments, O is the other buffer
        QIL_TRY(qil_dev_fill_ones(ctx, dt, Mc, nr));
        for (int64_t i = 0; i <= n; ++i) {
            const BondPlan& b = bp[(size_t)i];
            const int64_t cl = psi->dims[(size_t)i], Dl = W->dims[(size_t)i];
            if (b.nfin) {
                hipLaunchKernelGGL(apply_weight_finish<T>, dim3((unsigned)b.nfin), dim3(kFinishThreads), 0, qil_stream(ctx),
                                   dt_tab + b.fin, (const T*)E, (const T*)Mc, (const T*)Rk[(size_t)i], (int)cl, (int)Dl, amp2, dres);
                QIL_HIP(hipGetLastError());
            }
            if (i == n) break;
            const int64_t cr = psi->dims[(size_t)i + 1], Dr = W->dims[(size_t)i + 1];
            const int64_t sE = cl * Dl * Dl * cl;
            if (b.gather) {
                hipLaunchKernelGGL(apply_weight_gather<T>, dim3(qil_grid_for((long long)b.ngat * sE)), dim3(256), 0, qil_stream(ctx),
                                   dt_tab + b.gat, (long long)b.ngat, (const T*)E, O, (long long)sE);
                QIL_HIP(hipGetLastError());
                std::swap(E, O);
            }
            if (b.nact > b.nsurv) {
                hipLaunchKernelGGL(apply_weight_seed<T>, dim3(qil_grid_for((long long)(b.nact - b.nsurv) * sE)), dim3(256), 0,
                                   qil_stream(ctx), dt_tab + b.act, (int)b.nsurv, (long long)(b.nact - b.nsurv), (const T*)Mc, E,
                                   (int)cl, (int)Dl);
                QIL_HIP(hipGetLastError());
            }
            if (b.nlead) {
                QIL_TRY(qil_lazy_row_step(ctx, dt, W, psi, i, Mc, Mn, buf[4], sc.Wc, psi->dtype != dt ? sc.As : nullptr, b.nlead,
                                          dsp + r0 * n + i, n));
                std::swap(Mc, Mn);
            }
            if (b.nact) {
                const int64_t na = (int64_t)b.nact;
                const void *As = nullptr, *Wd = nullptr;
                QIL_TRY(qil_site_operand(ctx, dt, psi, i, sc.As, &As));
                QIL_TRY(qil_site_operand(ctx, dt, W, i, sc.Wd, &Wd));
                QIL_TRY(qil_put_mpo_site(ctx, dt, W, i, QIL_SITE_SWAPPED, sc.Wr));
                QIL_TRY(qil_norm_env_ket(ctx, dt, cl, cr, Dl, Dr, na, As, Wd, E, O, E));   // T1 in O, T2 in E
                if (b.any_fixed) {
                    hipLaunchKernelGGL(apply_weight_mask<T>, dim3(qil_grid_for(na * cl * Dl * Dr * cr)), dim3(256), 0, qil_stream(ctx), E,
                                       dt_tab + b.act, (long long)na, (long long)(cl * Dl), (long long)(Dr * cr), dsp + r0 * n, (int)n,
                                       (int)i);
                    QIL_HIP(hipGetLastError());
                }
                QIL_TRY(qil_norm_env_bra(ctx, dt, cl, cr, Dl, Dr, na, As, sc.Wr, E, O, E));    // T3 in O, E' in E
            }
        }
        QIL_TRY(dtab.release());
    }
    QIL_HIP(hipMemcpyAsync(out, dout, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));
    return QIL_OK;
}

}  // namespace

extern "C" int qil_apply_weight_batch(const qil_mpo* W, const qil_mps* psi, int64_t nb, const uint8_t* spec, double* out) {
    QIL_REQUIRE(W && psi && (nb <= 0 || (spec && out)), QIL_EINVAL_ARG, "apply_weight_batch: null argument");
    QIL_REQUIRE(nb >= 0, QIL_EINVAL_ARG, "apply_weight_batch: negative row count %lld", (long long)nb);
    QIL_TRY(qil_check_apply_operands(W, psi));
    const int64_t n = psi->n();
    for (int64_t t = 0; t < nb * n; ++t)
        QIL_REQUIRE(spec[t] <= 2, QIL_EINVAL_CONFIG, "apply_weight_batch: spec value %d outside [0,2] (a kept site makes no number)",
                    (int)spec[t]);
    if (nb == 0) return QIL_OK;
    int64_t renv_budget = kRightEnvBudget;             // QIL_APPLY_WEIGHT_RENV_BYTES: read on each call (0 keeps no R_k)
    if (const char* v = getenv("QIL_APPLY_WEIGHT_RENV_BYTES")) {
        char* end = nullptr;
        const long long b = strtoll(v, &end, 10);
        if (end != v && b >= 0) renv_budget = b;
    }
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    if (W->dtype == QIL_C64 || psi->dtype == QIL_C64) return weigh<c64>(ctx, W, psi, nb, spec, renv_budget, out);
    return weigh<double>(ctx, W, psi, nb, spec, renv_budget, out);
}
