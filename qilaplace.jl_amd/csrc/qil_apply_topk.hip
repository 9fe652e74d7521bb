// Lazy top-k search for gfx950: qil_apply_top_k returns the k configurations x with the largest |(W psi)_x|, their values and a
// bound on what the search may have dropped, without forming W psi.  The arithmetic is fixed in include/qilaplace_hip.h.  It is
// qil_top_k's beam search (qil_beam_search, qil_topk.hip: bookkeeping, selection, back-walk levels, read-back, delivery, bound)
// over the lazy row vector of qil_apply_coefficient_batch in place of the prefix vector: lazy_rows below is its qil_beam_rows.
// It joins three things that exist:
//   start          qil_apply_right_envs (qil_apply_sample.hip): site scratch, selector and the trace-normalised right environments
//                  R_k of |W psi|^2, here with the log trace: log |W psi|^2 = sum_k log t_k stays on the device until the
//                  search reads it back with the outputs
//   scoring        qil_apply_score_children (qil_apply_sample.hip), either route: partial sums of q_s = Re(m_s R_{i+1} m_s^H)
//                  for both children M_s = qil_lazy_row_step (qil_readout.hip) of every frontier row
//   search         qil_beam_search (qil_topk.hip), with its radix select + compaction over all 2 f candidates
// and adds the per-tensor kernels of the lazy row layout (a row is P = chi D contiguous elements), whose per-row arithmetic
// (beam_keys, beam_child_scale, beam_gather_row, beam_finish_row; qil_device_utils.h) is the one of qil_top_k's kernels:
//   apply_top_k_keys     one wave per row: the partials of both children summed in panel order (apply_sample_choose's order),
//                        q_s and key(2 r + s) = p_r q_s / (q_0 + q_1)
//   apply_top_k_gather   the kept children, scaled by 1 / sqrt(q_s), become the next frontier; g' = g + log(q_s) / 2, p' = key
//                        and the candidate index for the back-walk
//   apply_top_k_finish   the last tensor (P = 1): value = amp M_s e^g, the bit rows by walking the candidate indices back
// Buffers.  Held for the whole frontier (fcap = the largest frontier, min(2^(n-1), beam) rows): the rows (maxM e each), both
// children (2 maxM e), the keys, q, g, p, the selection and the back-walk.  The children of row r lie chunk by chunk:
//     child s of row r at (2 r0 + s nr + (r - r0)) P,   r0 = chunk (r / chunk),  nr = min(chunk, f - r0)
// which is the packing the scoring step reads ([M_0 M_1] of nr rows).  Per chunk of
//     chunk = max(1, min(fcap, 32768, 64 MiB / ((2 maxM + maxX) e + 16 ceil(maxM / 64))))     (qil_apply_chunk_rows)
// rows: U = R^H [M_0 M_1] (2 maxM; gemm route), the row step's X and the partials.  maxM, maxX, e as in qil_apply_sample.hip.
// Frontier sizes are min(2^i, beam), known on the host: no count is read back, and with the fixed-order sums and the
// selection's integer atomics the result is bit-identical from run to run.
// Left out: a device-resident output, both children of the row step in one strided batch, a batch of (W, psi) pairs.
#include <algorithm>
#include <cmath>
#include <vector>

#include "qil_internal.h"
#include "qil_device_utils.h"

namespace {

using namespace qil_dev;

constexpr int kKeyRows = 4;                         // rows per workgroup of the keys kernel: one wave each
constexpr long long kBeamHardCap = 1LL << 29;       // candidate indices 2 r + s stay below 2^30 (int)

// where child s of frontier row `row` starts in the children buffer, in rows of P elements (the head comment's packing)
__device__ __forceinline__ long long child_row(long long row, int s, long long f, long long chunk) {
    const long long r0 = row / chunk * chunk;
    const long long nr = f - r0 < chunk ? f - r0 : chunk;
    return 2 * r0 + (s ? nr : 0) + (row - r0);
}

// a row element through one 16-byte access for c64 (rows start at multiples of 16 bytes of a pool block), 8 bytes for f64
typedef double dv2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double load_elem(const double* p) { return *p; }
__device__ __forceinline__ c64 load_elem(const c64* p) {
    const dv2 v = *reinterpret_cast<const dv2*>(p);
    return c64{v.x, v.y};
}
__device__ __forceinline__ void store_elem(double* p, double v) { *p = v; }
__device__ __forceinline__ void store_elem(c64* p, c64 v) { *reinterpret_cast<dv2*>(p) = dv2{v.re, v.im}; }

// One wave per row of a chunk: q_s = the partials summed in panel order, clamped at 0 (rounding of a PSD form; NaN counts as 0),
// key(2 row + s) = p q_s / (q_0 + q_1), 0 when the sum is not positive.  part: [(s panels + panel) rows + row]; p, keys and q
// start at the chunk's first row.  Every lane of the wave forms the same sums from the same addresses; lane 0 writes.
__global__ __launch_bounds__(64 * kKeyRows) void apply_top_k_keys(const double* __restrict__ part, int panels, long long rows,
                                                                  const double* __restrict__ p, double* __restrict__ keys,
                                                                  double* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kKeyRows + (threadIdx.x >> 6);
    if (row >= rows) return;
    double q0 = 0.0, q1 = 0.0;
    for (int t = 0; t < panels; ++t) {
        q0 += part[(long long)t * rows + row];
        q1 += part[((long long)panels + t) * rows + row];
    }
    if (lane == 0) beam_keys(q0, q1, row, p, keys, q);
}

// Next frontier row j = the kept candidate c = sel[j] (c = j when everything is kept): child c & 1 of row c >> 1, scaled by
// 1 / sqrt(q_c) (zeroed when q_c <= 0).  Consecutive threads take consecutive elements of a row, and the rows of Mn are packed:
// reads and writes are contiguous along P.  The thread of an element 0 writes the row's g', p' and back-walk index.
template <class T>
__global__ __launch_bounds__(256) void apply_top_k_gather(const T* __restrict__ Mch, long long f, long long chunk, int P,
                                                          const double* __restrict__ keys, const double* __restrict__ q,
                                                          const double* __restrict__ g, const int* __restrict__ sel, long long M,
                                                          T* __restrict__ Mn, double* __restrict__ gn, double* __restrict__ pn,
                                                          int* __restrict__ anc) {
    const long long total = M * P;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long j = t / P;
        const int k = (int)(t - j * P);
        const int c = sel ? sel[j] : (int)j;
        const long long row = c >> 1;
        const double qq = q[c];
        const T v = load_elem(Mch + child_row(row, c & 1, f, chunk) * P + k);
        store_elem(Mn + t, scale_t(v, beam_child_scale(qq)));
        if (k == 0) beam_gather_row(j, c, qq, keys, g, gn, pn, anc);
    }
}

// The last tensor: a child is one number, the complete product up to e^g.  value = sgn e^{g + lamp} M_s (lamp = log |amp|), the
// bits are the candidate indices walked back level by level (anc: level lvl at lvl * stride).
template <class T>
__global__ __launch_bounds__(256) void apply_top_k_finish(const T* __restrict__ Mch, long long f, long long chunk,
                                                          const double* __restrict__ g, const int* __restrict__ sel, long long M,
                                                          const int* __restrict__ anc, long long stride, int n, double lamp,
                                                          double sgn, double* __restrict__ val, uint8_t* __restrict__ bits) {
    for (long long j = blockIdx.x * 256LL + threadIdx.x; j < M; j += (long long)gridDim.x * 256) {
        const int c = sel ? sel[j] : (int)j;
        beam_finish_row(j, c, Mch[child_row(c >> 1, c & 1, f, chunk)], g, anc, stride, n, lamp, sgn, val, bits);
    }
}

// beam <= min(2^29, 2^30 / (3 maxM e + 4 n + 64)): the rows (maxM e per row), both children (2 maxM e) and the per-row
// bookkeeping fit in 1 GiB.  A function of the operands' shapes alone.
int64_t beam_cap(const qil_mpo* W, const qil_mps* psi) {
    const long long e = W->dtype == QIL_C64 || psi->dtype == QIL_C64 ? 16 : 8;
    const long long per_row = 3 * qil_apply_sizes_of(W, psi).maxM * e + 4 * psi->n() + 64;
    return std::min<long long>(kBeamHardCap, (1LL << 30) / per_row);
}

// the rows of qil_apply_top_k: the lazy row vectors (Mf, packed, P elements each) and their children (Mch, the head comment's
// packing), scored chunk by chunk through Xb, Uc and part
template <class T>
struct lazy_rows final : qil_beam_rows {
    static constexpr int dt = sizeof(T) == 16 ? QIL_C64 : QIL_F64;
    qil_context* ctx;
    const qil_mpo* W;
    const qil_mps* psi;
    const qil_apply_lazy& lz;
    bool fused;
    int64_t chunk;
    void *Mf = nullptr, *Mch = nullptr, *Xb = nullptr, *Uc = nullptr, *part = nullptr;
    lazy_rows(qil_context* c, const qil_mpo* w, const qil_mps* x, const qil_apply_lazy& l, bool fu, int64_t ch)
        : ctx(c), W(w), psi(x), lz(l), fused(fu), chunk(ch) {}
    int64_t bond(int64_t k) const { return psi->dims[(size_t)k] * W->dims[(size_t)k]; }

    int expand(int64_t i, long long f, const double* p, double* keys, double* q) override {
        const int64_t cr = psi->dims[(size_t)i + 1], Dr = W->dims[(size_t)i + 1], Pl = bond(i), P = cr * Dr;
        for (int64_t r0 = 0; r0 < f; r0 += chunk) {
            const int64_t nr = std::min<int64_t>(chunk, f - r0);
            T* child = static_cast<T*>(Mch) + 2 * r0 * P;
            for (int s = 0; s < 2; ++s)
                QIL_TRY(qil_lazy_row_step(ctx, dt, W, psi, i, static_cast<const T*>(Mf) + r0 * Pl, child + s * nr * P, Xb, lz.Wc, lz.As, nr,
                                          lz.both + s, 0));
            int panels = 1;
            QIL_TRY(qil_apply_score_children(ctx, dt, fused, child, nr, cr, Dr, lz.Rk[(size_t)i + 1], Uc, (double*)part, &panels));
            hipLaunchKernelGGL(apply_top_k_keys, dim3((unsigned)((nr + kKeyRows - 1) / kKeyRows)), dim3(64 * kKeyRows), 0, qil_stream(ctx),
                               (const double*)part, panels, (long long)nr, p + r0, keys + 2 * r0, q + 2 * r0);
        }
        return QIL_OK;
    }
    void gather(int64_t i, long long f, const double* keys, const double* q, const double* g, const int* sel, long long M, double* gn,
                double* pn, int* anc) override {
        const int64_t P = bond(i + 1);
        hipLaunchKernelGGL(apply_top_k_gather<T>, dim3(qil_grid_for(M * P)), dim3(256), 0, qil_stream(ctx), (const T*)Mch, f,
                           (long long)chunk, (int)P, keys, q, g, sel, M, static_cast<T*>(Mf), gn, pn, anc);
    }
    void finish(long long f, const double* g, const int* sel, long long M, const int* anc, long long stride, double lamp, double sgn,
                double* val, uint8_t* bits) override {
        hipLaunchKernelGGL(apply_top_k_finish<T>, dim3(qil_grid_for(M)), dim3(256), 0, qil_stream(ctx), (const T*)Mch, f,
                           (long long)chunk, g, sel, M, anc, stride, (int)psi->n(), lamp, sgn, val, bits);
    }
};

template <class T>
int top_k_lazy(qil_context* ctx, const qil_mpo* W, const qil_mps* psi, int64_t k, int64_t beam, uint8_t* bits_out, double* val_out,
               double* bound_out) {
    const int64_t e = (int64_t)sizeof(T);
    // ---- device memory: everything belongs to `tmp`.  Environments, right to left, with log |W psi|^2 (it stays on the device)
    qil_scratch tmp(ctx);
    qil_apply_lazy lz;
    int bad = 0;
    double* dlog = nullptr;
    QIL_TRY(qil_apply_right_envs(ctx, tmp, lazy_rows<T>::dt, W, psi, lz, &bad, &dlog));
    QIL_REQUIRE(bad == 0, QIL_EDOMAIN, "apply_top_k: the transformed state has zero norm");

    // ---- the frontier's rows and children, then the chunk's buffers
    const bool fused = qil_apply_score_fused(lz.b.maxM);
    const long long maxPanels = qil_apply_score_panels(lz.b.maxM);
    const long long fcap = qil_beam_frontier_cap(psi->n(), beam);
    const int64_t chunk = qil_apply_chunk_rows(fcap, (2 * lz.b.maxM + lz.b.maxX) * e + 16 * maxPanels);
    lazy_rows<T> rows(ctx, W, psi, lz, fused, chunk);
    QIL_TRY(tmp.alloc((size_t)(fcap * lz.b.maxM * e), &rows.Mf));
    QIL_TRY(tmp.alloc((size_t)(fcap * 2 * lz.b.maxM * e), &rows.Mch));
    QIL_TRY(tmp.alloc((size_t)(chunk * lz.b.maxX * e), &rows.Xb));
    if (!fused) QIL_TRY(tmp.alloc((size_t)(chunk * 2 * lz.b.maxM * e), &rows.Uc));
    QIL_TRY(tmp.alloc((size_t)(chunk * 2 * (fused ? maxPanels : 1) * 8), &rows.part));
    QIL_TRY(qil_dev_fill_ones(ctx, lazy_rows<T>::dt, rows.Mf, 1));
    return qil_beam_search(ctx, tmp, rows, psi->n(), k, beam, psi->amplitude, 0.0, dlog, bits_out, val_out, bound_out);
}

}  // namespace

extern "C" int qil_apply_top_k(const qil_mpo* W, const qil_mps* psi, int64_t k, int64_t beam, uint8_t* bits_out, double* val_out,
                               double* bound_out) {
    QIL_REQUIRE(W && psi, QIL_EINVAL_ARG, "apply_top_k: null argument");
    QIL_REQUIRE(k >= 0, QIL_EINVAL_ARG, "apply_top_k: negative k %lld", (long long)k);
    QIL_REQUIRE(beam >= k, QIL_EINVAL_ARG, "apply_top_k: beam %lld below k %lld", (long long)beam, (long long)k);
    QIL_TRY(qil_check_apply_operands(W, psi));
    QIL_REQUIRE(beam <= beam_cap(W, psi), QIL_EINVAL_ARG, "apply_top_k: beam %lld above the cap %lld for these operands",
                (long long)beam, (long long)beam_cap(W, psi));
    QIL_REQUIRE(psi->n() > 62 || k <= (1LL << psi->n()), QIL_EINVAL_ARG, "apply_top_k: k %lld above the 2^%lld configurations",
                (long long)k, (long long)psi->n());
    if (k == 0) return QIL_OK;
    QIL_REQUIRE(bits_out && val_out && bound_out, QIL_EINVAL_ARG, "apply_top_k: null argument");
    const int64_t budget = qil_apply_env_budget();     // qil_apply_sample's: the environments are the shared step
    const double need = qil_apply_env_bytes(W, psi);
    QIL_REQUIRE(need <= (double)budget, QIL_ENOMEM,
                "apply_top_k: the right environments need %.0f bytes, above the %lld allowed (QIL_APPLY_SAMPLE_RENV_BYTES raises it)",
                need, (long long)budget);
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    if (W->dtype == QIL_C64 || psi->dtype == QIL_C64) return top_k_lazy<c64>(ctx, W, psi, k, beam, bits_out, val_out, bound_out);
    return top_k_lazy<double>(ctx, W, psi, k, beam, bits_out, val_out, bound_out);
}
