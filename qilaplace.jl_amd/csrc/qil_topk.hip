// Top-k coefficient search (qil_top_k): the k configurations x with the largest |psi_x|, by a level-by-level beam search over
// prefixes ranked by their marginal weight, with a bound on what the search may have missed.  Nothing crosses to the host
// between sites.
//
//   environments   qil_dev_right_envs (qil_sample's): R_i trace-normalised, plus log |psi|^2 as the sum of the log traces
//   frontier       f rows (f = 1 and v = [1] at the start); row r carries v_r (ld f, row fastest), a log-scale g_r (the prefix
//                  product is v_r e^{g_r}) and p_r = w(prefix_r) / |psi|^2
//   site i         T = V A_i (f x 2 chi_r) and U_s = T_s R_i through qil_dev_gemm; score_children reduces q_s = Re(T_s R_i T_s^H)
//                  for both children and writes key(2r + s) = p_r q_s / (q_0 + q_1), the child's weight / |psi|^2
//   select         keep the M = min(2f, beam) largest keys (min(2f, k) at the last site): an MSD radix select on the keys' bit
//                  patterns (8 passes of 8 bits, order-preserving for non-negative doubles), then a prefix-scan compaction in
//                  candidate order; ties at the cut go to the lower candidate position 2r + s.  The largest key dropped before
//                  the last site is kept on the device (an atomic max on the bit pattern).
//   gather         v' = T_s / sqrt(q_s), g' = g + log(q_s) / 2, p' = key, and the candidate index for the backtrack
//   last site      value = amp T_s e^g (R_n = [1]), bits by walking the candidate indices back; the host orders the k rows
// Frontier sizes are min(2^i, beam): known on the host, so no count is read back.  All reductions have a fixed order and the
// counts are integer atomics: the output is bit-identical from run to run.
// One search for two verbs.  qil_beam_search below owns the bookkeeping (keys, q, g, p, the selection, the back-walk levels),
// the frontier sizes, the read-back, the delivery and the bound; it sees the rows through qil_beam_rows (qil_internal.h):
// expand, gather, finish.  prefix_rows is qil_top_k's (V, T, U_s and the three kernels here), lazy_rows qil_apply_top_k's
// (qil_apply_topk.hip).  The per-row arithmetic of those kernels -- beam_keys, beam_child_scale, beam_gather_row,
// beam_finish_row -- and the row sums of score_children (children_row_sums, qil_sample's too) are in qil_device_utils.h.
#include "qil_internal.h"
#include "qil_device_utils.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace {

using namespace qil_dev;

constexpr int kThreads = 256;
constexpr int kTile = 4 * kThreads;             // candidates per compaction workgroup, 4 consecutive per thread
constexpr int kScoreRows = 32, kScoreGroups = 8;
constexpr long long kBeamHardCap = 1LL << 29;    // candidate indices 2r + s stay below 2^30 (int)

__device__ __forceinline__ unsigned long long key_bits(double k) { return (unsigned long long)__double_as_longlong(k); }

// ---- frontier start ----------------------------------------------------------------------------------------------------
// g_0 = 0, p_0 = 1 and nothing dropped yet; the one row itself ([1]) is the verb's
__global__ void start_frontier(double* __restrict__ g, double* __restrict__ p, unsigned long long* __restrict__ drop) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        g[0] = 0.0;
        p[0] = 1.0;
        drop[0] = 0;
    }
}

// ---- scoring: both children's weights ------------------------------------------------------------------------------------
// T (rows x 2 chi_r) and U_s = T_s R in the layout of children_row_sums (qil_device_utils.h): a workgroup owns 32 rows, its 8
// groups of 32 threads split the columns; then the keys (beam_keys).
template <class T>
__global__ __launch_bounds__(kScoreRows* kScoreGroups) void score_children(const T* __restrict__ Tm, const T* __restrict__ Us,
                                                                           long long rows, int cr, const double* __restrict__ p,
                                                                           double* __restrict__ keys, double* __restrict__ q) {
    __shared__ double qs[2][kScoreGroups][kScoreRows];
    double a = 0.0, b = 0.0;
    if (children_row_sums<kScoreRows, kScoreGroups>(Tm, Us, rows, cr, qs, a, b))
        beam_keys(a, b, (long long)blockIdx.x * kScoreRows + threadIdx.x % kScoreRows, p, keys, q);
}

// ---- radix select -------------------------------------------------------------------------------------------------------
// After the 8 passes, prefix is the bit pattern of the M-th largest key tau, and need the number of candidates with key tau
// that are kept (the M - need others have keys > tau).
struct select_state {
    unsigned long long prefix, mask;
    long long need;
    unsigned hist[256];
    unsigned ticket;
};

__global__ void select_init(select_state* st, long long keep) {
    st->hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        st->prefix = 0;
        st->mask = 0;
        st->need = keep;
        st->ticket = 0;
    }
}

// One pass: histogram of digit (key >> shift) & 255 over the candidates that match the prefix so far; the last workgroup to
// finish picks the digit of the need-th largest, extends the prefix and clears the histogram for the next pass.
__global__ __launch_bounds__(kThreads) void select_pass(const double* __restrict__ keys, long long C, int shift, select_state* st) {
    __shared__ unsigned h[256];
    __shared__ bool last;
    const int t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const unsigned long long prefix = st->prefix, mask = st->mask;
    for (long long c = blockIdx.x * (long long)kThreads + t; c < C; c += (long long)gridDim.x * kThreads) {
        const unsigned long long u = key_bits(keys[c]);
        if ((u & mask) == prefix) atomicAdd(&h[(u >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[t]) atomicAdd(&st->hist[t], h[t]);
    __threadfence();
    __syncthreads();
    if (t == 0) last = atomicAdd(&st->ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    const unsigned mine = atomicAdd(&st->hist[t], 0u);
    h[t] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // h[d] <- sum of the counts of digits >= d
        const unsigned v = t + off < 256 ? h[t + off] : 0u;
        __syncthreads();
        h[t] += v;
        __syncthreads();
    }
    const long long need = st->need;
    const long long above = (long long)h[t] - mine;
    __syncthreads();
    if ((long long)h[t] >= need && above < need) {
        st->prefix = prefix | ((unsigned long long)t << shift);
        st->mask = mask | (255ull << shift);
        st->need = need - above;
    }
    st->hist[t] = 0;
    if (t == 0) st->ticket = 0;
}

// ---- compaction -----------------------------------------------------------------------------------------------------------
// gt: key > tau, eq: key == tau.  Candidate c is kept iff gt, or eq and fewer than need eq candidates precede it; its place in
// the next frontier is (gt before c) + min(eq before c, need).
__device__ __forceinline__ void tile_flags(const double* __restrict__ keys, long long C, unsigned long long tau, long long c0,
                                           int (&cls)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long c = c0 + j;
        cls[j] = -1;
        if (c < C) {
            const unsigned long long u = key_bits(keys[c]);
            cls[j] = u > tau ? 1 : (u == tau ? 2 : 0);
        }
    }
}

__global__ __launch_bounds__(kThreads) void compact_count(const double* __restrict__ keys, long long C, const select_state* st,
                                                          unsigned* __restrict__ blk) {
    __shared__ unsigned sg[kThreads / 64], se[kThreads / 64];
    const int t = threadIdx.x;
    int cls[4];
    tile_flags(keys, C, st->prefix, (long long)blockIdx.x * kTile + 4 * t, cls);
    unsigned gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gt += cls[j] == 1;
        eq += cls[j] == 2;
    }
    for (int off = 32; off > 0; off >>= 1) {
        gt += __shfl_down(gt, off);
        eq += __shfl_down(eq, off);
    }
    if ((t & 63) == 0) {
        sg[t >> 6] = gt;
        se[t >> 6] = eq;
    }
    __syncthreads();
    if (t == 0) {
        unsigned a = 0, b = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            a += sg[w];
            b += se[w];
        }
        blk[2 * blockIdx.x] = a;
        blk[2 * blockIdx.x + 1] = b;
    }
}

// exclusive scan of the workgroups' (gt, eq) counts, in place; one workgroup, chunks of 256 with a carry
__global__ __launch_bounds__(kThreads) void compact_scan(unsigned* __restrict__ blk, long long nblk) {
    __shared__ unsigned sg[kThreads], se[kThreads];
    __shared__ unsigned carry[2];
    const int t = threadIdx.x;
    if (t == 0) carry[0] = carry[1] = 0;
    __syncthreads();
    for (long long b0 = 0; b0 < nblk; b0 += kThreads) {
        const long long b = b0 + t;
        const unsigned g = b < nblk ? blk[2 * b] : 0u, e = b < nblk ? blk[2 * b + 1] : 0u;
        sg[t] = g;
        se[t] = e;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const unsigned vg = t >= off ? sg[t - off] : 0u, ve = t >= off ? se[t - off] : 0u;
            __syncthreads();
            sg[t] += vg;
            se[t] += ve;
            __syncthreads();
        }
        if (b < nblk) {
            blk[2 * b] = carry[0] + sg[t] - g;
            blk[2 * b + 1] = carry[1] + se[t] - e;
        }
        __syncthreads();
        if (t == kThreads - 1) {
            carry[0] += sg[t];
            carry[1] += se[t];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void compact_write(const double* __restrict__ keys, long long C, const select_state* st,
                                                          const unsigned* __restrict__ boff, int* __restrict__ sel,
                                                          unsigned long long* __restrict__ dropmax) {
    __shared__ unsigned sg[kThreads], se[kThreads];
    __shared__ unsigned long long smax;
    const int t = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * kTile + 4 * t;
    const unsigned long long tau = st->prefix;
    const long long need = st->need;
    int cls[4];
    tile_flags(keys, C, tau, c0, cls);
    unsigned gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gt += cls[j] == 1;
        eq += cls[j] == 2;
    }
    sg[t] = gt;
    se[t] = eq;
    if (t == 0) smax = 0;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const unsigned vg = t >= off ? sg[t - off] : 0u, ve = t >= off ? se[t - off] : 0u;
        __syncthreads();
        sg[t] += vg;
        se[t] += ve;
        __syncthreads();
    }
    long long gb = (long long)boff[2 * blockIdx.x] + sg[t] - gt, eb = (long long)boff[2 * blockIdx.x + 1] + se[t] - eq;
    unsigned long long dmax = 0;   // every key below tau is below tau's bit pattern: a dropped tie sets it to tau
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long c = c0 + j;
        if (cls[j] == 1) {
            sel[gb + (eb < need ? eb : need)] = (int)c;
            ++gb;
        } else if (cls[j] == 2) {
            if (eb < need) sel[gb + eb] = (int)c;
            else dmax = tau;
            ++eb;
        } else if (cls[j] == 0) {
            const unsigned long long u = key_bits(keys[c]);
            dmax = u > dmax ? u : dmax;
        }
    }
    if (dropmax) {
        if (dmax) atomicMax(&smax, dmax);
        __syncthreads();
        if (t == 0 && smax) atomicMax(dropmax, smax);
    }
}

// ---- gather the kept children into the next frontier ---------------------------------------------------------------------
template <class T>
__global__ void gather_frontier(const T* __restrict__ Tm, long long f, int cr, const double* __restrict__ keys,
                                const double* __restrict__ q, const double* __restrict__ g, const int* __restrict__ sel,
                                long long M, T* __restrict__ V, double* __restrict__ gn, double* __restrict__ pn,
                                int* __restrict__ anc) {
    const long long total = M * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long j = t % M;
        const int beta = (int)(t / M);
        const int c = sel ? sel[j] : (int)j;
        const long long row = c >> 1;
        const int s = c & 1;
        const double qq = q[c];
        V[j + M * beta] = scale_t(Tm[row + f * (s + 2LL * beta)], beam_child_scale(qq));
        if (beta == 0) beam_gather_row(j, c, qq, keys, g, gn, pn, anc);
    }
}

// ---- the last site: values and bit rows ----------------------------------------------------------------------------------
// T (f x 2, chi_r = 1) holds the complete products up to e^g: beam_finish_row on child c & 1 of row c >> 1
template <class T>
__global__ void finish_rows(const T* __restrict__ Tm, long long f, const double* __restrict__ g, const int* __restrict__ sel,
                            long long M, const int* __restrict__ anc, long long stride, int n, double lamp, double sgn,
                            double* __restrict__ val, uint8_t* __restrict__ bits) {
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < M; j += (long long)gridDim.x * blockDim.x) {
        const int c = sel ? sel[j] : (int)j;
        beam_finish_row(j, c, Tm[(c >> 1) + f * (c & 1)], g, anc, stride, n, lamp, sgn, val, bits);
    }
}

}  // namespace

// ---- the selection, for qil_top_k and qil_apply_top_k (qil_internal.h) -----------------------------------------------------
size_t qil_dev_select_state_bytes() { return sizeof(select_state); }
size_t qil_dev_select_block_bytes(long long C) { return (size_t)(2 * ((C + kTile - 1) / kTile)) * 4; }

int qil_dev_select_largest(qil_context* ctx, const double* keys, long long C, long long M, int* sel, unsigned long long* dropmax,
                           void* state, void* blk) {
    select_state* sst = static_cast<select_state*>(state);
    const long long nblk = (C + kTile - 1) / kTile;
    hipLaunchKernelGGL(select_init, dim3(1), dim3(256), 0, qil_stream(ctx), sst, M);
    // few workgroups: a pass costs ~10 us at 64 of them and ~34 us at 512 (every workgroup's fence and ticket), not bandwidth
    const unsigned pgrid = (unsigned)std::max<long long>(1, std::min<long long>((C + 2047) / 2048, 512));
    for (int shift = 56; shift >= 0; shift -= 8)
        hipLaunchKernelGGL(select_pass, dim3(pgrid), dim3(kThreads), 0, qil_stream(ctx), keys, C, shift, sst);
    hipLaunchKernelGGL(compact_count, dim3((unsigned)nblk), dim3(kThreads), 0, qil_stream(ctx), keys, C, (const select_state*)sst,
                       (unsigned*)blk);
    hipLaunchKernelGGL(compact_scan, dim3(1), dim3(kThreads), 0, qil_stream(ctx), (unsigned*)blk, nblk);
    hipLaunchKernelGGL(compact_write, dim3((unsigned)nblk), dim3(kThreads), 0, qil_stream(ctx), keys, C, (const select_state*)sst,
                       (const unsigned*)blk, sel, dropmax);
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

void qil_top_k_deliver(int64_t k, int64_t n, const double* val, const uint8_t* bits, uint8_t* bits_out, double* val_out) {
    std::vector<int64_t> ord((size_t)k);
    std::iota(ord.begin(), ord.end(), 0);
    auto mag = [&](int64_t j) { return std::hypot(val[2 * j], val[2 * j + 1]); };
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return mag(a) > mag(b); });
    for (int64_t j = 0; j < k; ++j) {
        const int64_t o = ord[(size_t)j];
        val_out[2 * j] = val[2 * o];
        val_out[2 * j + 1] = val[2 * o + 1];
        std::copy_n(bits + o * n, n, bits_out + j * n);
    }
}

// ---- the search, for qil_top_k and qil_apply_top_k (qil_internal.h) ---------------------------------------------------------
long long qil_beam_frontier_cap(int64_t n, int64_t beam) {
    long long fcap = 1;
    for (long long f = 1, i = 0; i < n; ++i, f = std::min<long long>(2 * f, beam)) fcap = std::max(fcap, f);
    return fcap;
}

int qil_beam_search(qil_context* ctx, qil_scratch& tmp, qil_beam_rows& rows, int64_t n, int64_t k, int64_t beam, double amp,
                    double log_norm2, const double* dev_log_norm2, uint8_t* bits_out, double* val_out, double* bound_out) {
    const long long fcap = qil_beam_frontier_cap(n, beam);
    // ---- the per-candidate and per-row bookkeeping, the selection's state, the back-walk, the result
    void *keys = nullptr, *q = nullptr, *g[2] = {nullptr, nullptr}, *p[2] = {nullptr, nullptr};
    void *sel = nullptr, *anc = nullptr, *blk = nullptr, *st = nullptr, *drop = nullptr, *dval = nullptr, *dbits = nullptr;
    QIL_TRY(tmp.alloc((size_t)(2 * fcap) * 8, &keys));
    QIL_TRY(tmp.alloc((size_t)(2 * fcap) * 8, &q));
    for (int b = 0; b < 2; ++b) {
        QIL_TRY(tmp.alloc((size_t)fcap * 8, &g[b]));
        QIL_TRY(tmp.alloc((size_t)fcap * 8, &p[b]));
    }
    QIL_TRY(tmp.alloc((size_t)(2 * fcap) * 4, &sel));
    QIL_TRY(tmp.alloc((size_t)(std::max<int64_t>(n - 1, 1) * fcap) * 4, &anc));
    QIL_TRY(tmp.alloc(qil_dev_select_block_bytes(2 * fcap), &blk));
    QIL_TRY(tmp.alloc(qil_dev_select_state_bytes(), &st));
    QIL_TRY(tmp.alloc(8, &drop));   // bit pattern of the largest key dropped before the last site (all levels)
    QIL_TRY(tmp.alloc((size_t)k * 16, &dval));
    QIL_TRY(tmp.alloc((size_t)(k * n), &dbits));
    hipLaunchKernelGGL(start_frontier, dim3(1), dim3(64), 0, qil_stream(ctx), (double*)g[0], (double*)p[0], (unsigned long long*)drop);
    QIL_HIP(hipGetLastError());

    // ---- site by site: frontier sizes f_0 = 1, f_{i+1} = min(2 f_i, beam)
    const double lamp = std::log(std::fabs(amp)), sgn = amp < 0.0 ? -1.0 : 1.0;
    long long f = 1;
    int cur = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool last = i == n - 1;
        QIL_TRY(rows.expand(i, f, (const double*)p[cur], (double*)keys, (double*)q));
        QIL_HIP(hipGetLastError());
        const long long C = 2 * f, M = std::min<long long>(C, last ? k : beam);
        const int* kept = nullptr;
        if (M < C) {
            QIL_TRY(qil_dev_select_largest(ctx, (const double*)keys, C, M, (int*)sel, last ? nullptr : (unsigned long long*)drop, st, blk));
            kept = static_cast<const int*>(sel);
        }
        if (last) {
            rows.finish(f, (const double*)g[cur], kept, M, (const int*)anc, fcap, lamp, sgn, (double*)dval, (uint8_t*)dbits);
        } else {
            rows.gather(i, f, (const double*)keys, (const double*)q, (const double*)g[cur], kept, M, (double*)g[1 - cur],
                        (double*)p[1 - cur], static_cast<int*>(anc) + i * fcap);
            cur = 1 - cur;
            f = M;
        }
        QIL_HIP(hipGetLastError());
    }
    std::vector<double> hval((size_t)(2 * k));
    std::vector<uint8_t> hbits((size_t)(k * n));
    unsigned long long hdrop = 0;
    QIL_HIP(hipMemcpyAsync(hval.data(), dval, (size_t)k * 16, hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_HIP(hipMemcpyAsync(hbits.data(), dbits, (size_t)(k * n), hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_HIP(hipMemcpyAsync(&hdrop, drop, 8, hipMemcpyDeviceToHost, qil_stream(ctx)));
    if (dev_log_norm2) QIL_HIP(hipMemcpyAsync(&log_norm2, dev_log_norm2, 8, hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));

    qil_top_k_deliver(k, n, hval.data(), hbits.data(), bits_out, val_out);
    double dropped = 0.0;
    std::memcpy(&dropped, &hdrop, 8);
    *bound_out = dropped > 0.0 ? std::exp(0.5 * (std::log(dropped) + log_norm2) + lamp) : 0.0;
    return QIL_OK;
}

namespace {

// ---- the call -----------------------------------------------------------------------------------------------------------
// the rows of qil_top_k: the prefix vectors v_r (f x chi, ld f, row fastest), both children T = V A_i and U_s = T_s R_{i+1}
template <class T>
struct prefix_rows final : qil_beam_rows {
    qil_context* ctx;
    const qil_mps* psi;
    const T* Rb;
    const std::vector<long long>& roff;
    void *V, *Tm, *Us;
    prefix_rows(const qil_mps* x, const void* R, const std::vector<long long>& off, void* v, void* t, void* u)
        : ctx(x->ctx), psi(x), Rb(static_cast<const T*>(R)), roff(off), V(v), Tm(t), Us(u) {}

    int expand(int64_t i, long long f, const double* p, double* keys, double* q) override {
        const int dt = psi->dtype;
        const int64_t cl = psi->dims[(size_t)i], cr = psi->dims[(size_t)i + 1];
        const T* R = Rb + roff[(size_t)i + 1];
        // T (f x 2 chi_r) = V A;  U_s (f x chi_r) = T_s R  (slice s: offset s rows, ld 2 rows)
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, f, 2 * cr, cl, V, f, psi->site[(size_t)i], cl, Tm, f));
        for (int s = 0; s < 2; ++s)
            QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, f, cr, cr, static_cast<const T*>(Tm) + s * f, 2 * f, R, cr, static_cast<T*>(Us) + s * f * cr, f));
        hipLaunchKernelGGL(score_children<T>, dim3((unsigned)((f + kScoreRows - 1) / kScoreRows)), dim3(kScoreRows * kScoreGroups), 0,
                           qil_stream(ctx), (const T*)Tm, (const T*)Us, f, (int)cr, p, keys, q);
        return QIL_OK;
    }
    void gather(int64_t i, long long f, const double* keys, const double* q, const double* g, const int* sel, long long M, double* gn,
                double* pn, int* anc) override {
        const int64_t cr = psi->dims[(size_t)i + 1];
        hipLaunchKernelGGL(gather_frontier<T>, dim3(qil_grid_for(M * cr)), dim3(256), 0, qil_stream(ctx), (const T*)Tm, f, (int)cr, keys, q,
                           g, sel, M, static_cast<T*>(V), gn, pn, anc);
    }
    void finish(long long f, const double* g, const int* sel, long long M, const int* anc, long long stride, double lamp, double sgn,
                double* val, uint8_t* bits) override {
        hipLaunchKernelGGL(finish_rows<T>, dim3(qil_grid_for(M)), dim3(256), 0, qil_stream(ctx), (const T*)Tm, f, g, sel, M, anc, stride,
                           (int)psi->n(), lamp, sgn, val, bits);
    }
};

template <class T>
static int top_k_impl(const qil_mps* psi, int64_t k, int64_t beam, uint8_t* bits_out, double* val_out, double* bound_out) {
    qil_context* ctx = psi->ctx;
    const size_t e = sizeof(T);
    long long maxchi = 1;
    for (int64_t b : psi->dims) maxchi = std::max<long long>(maxchi, b);
    const long long fcap = qil_beam_frontier_cap(psi->n(), beam);
    qil_scratch tmp(ctx);

    // ---- environments, right to left
    void* Rall = nullptr;
    std::vector<long long> roff;
    double log_norm2 = 0.0;
    QIL_TRY(qil_dev_right_envs(psi, tmp, "top_k", &Rall, roff, &log_norm2));

    // ---- the rows: frontier, both children, T_s R
    void *V = nullptr, *Tm = nullptr, *Us = nullptr;
    QIL_TRY(tmp.alloc((size_t)(fcap * maxchi) * e, &V));
    QIL_TRY(tmp.alloc((size_t)(fcap * 2 * maxchi) * e, &Tm));
    QIL_TRY(tmp.alloc((size_t)(fcap * 2 * maxchi) * e, &Us));
    QIL_TRY(qil_dev_fill_ones(ctx, psi->dtype, V, 1));
    prefix_rows<T> rows(psi, Rall, roff, V, Tm, Us);
    return qil_beam_search(ctx, tmp, rows, psi->n(), k, beam, psi->amplitude, log_norm2, nullptr, bits_out, val_out, bound_out);
}

// beam <= min(2^29, 2^30 / (3 chi s + 4 n + 64)): chi = the largest bond, s = 8 (f64) / 16 (c64), n = the number of site
// tensors.  The frontier (chi per row), both children (2 chi) and the per-row bookkeeping fit in 1 GiB; T_s R adds 2 chi s per row.
static int64_t beam_cap(const qil_mps* psi) {
    long long maxchi = 1;
    for (int64_t b : psi->dims) maxchi = std::max<long long>(maxchi, b);
    const long long per_row = 3 * maxchi * (long long)qil_elem_size(psi->dtype) + 4 * psi->n() + 64;
    return std::min<long long>(kBeamHardCap, (1LL << 30) / per_row);
}

}  // namespace

extern "C" int qil_top_k(const qil_mps* psi, int64_t k, int64_t beam, uint8_t* bits_out, double* val_out, double* bound_out) {
    QIL_REQUIRE(psi, QIL_EINVAL_ARG, "top_k: null argument");
    QIL_REQUIRE(k >= 0, QIL_EINVAL_ARG, "top_k: negative k %lld", (long long)k);
    QIL_REQUIRE(beam >= k, QIL_EINVAL_ARG, "top_k: beam %lld below k %lld", (long long)beam, (long long)k);
    QIL_REQUIRE(beam <= beam_cap(psi), QIL_EINVAL_ARG, "top_k: beam %lld above the cap %lld for this state", (long long)beam,
                (long long)beam_cap(psi));
    QIL_REQUIRE(psi->n() > 62 || k <= (1LL << psi->n()), QIL_EINVAL_ARG, "top_k: k %lld above the 2^%lld configurations", (long long)k,
                (long long)psi->n());
    if (k == 0) return QIL_OK;
    QIL_REQUIRE(bits_out && val_out && bound_out, QIL_EINVAL_ARG, "top_k: null argument");
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    if (psi->dtype == QIL_C64) return top_k_impl<c64>(psi, k, beam, bits_out, val_out, bound_out);
    return top_k_impl<double>(psi, k, beam, bits_out, val_out, bound_out);
}
