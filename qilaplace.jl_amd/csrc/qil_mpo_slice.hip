// Read-outs of operators for gfx950: numbers (qil_mpo_entry_batch, the twin of qil_coefficient_marginal_batch) and state-valued
// slices (qil_mpo_slice, the twin of qil_mps_restrict), both on the operator's own bonds: no basis state, no apply.
//
// A spec gives two bytes per tensor, (in_i, out_i), for the legs of W_i[a, s_in, s_out, b]: 0 / 1 fixes the leg's bit, 2 sums
// it, 3 keeps it; (4,4) traces the site, (5,5) keeps its diagonal.  Slice (s_in, s_out) of a site is the D_l x D_r matrix at
// offset D_l (s_in + 2 s_out) with leading dimension 4 D_l.  A removed site is the factor S_i, the sum of 1, 2 or 4 slices in
// ascending s_in + 2 s_out, left-associated, made in the operand load (load_terms); a kept site keeps exactly one leg and is
// the MPS-shaped tensor whose slice s is one slice of W_i or the sum of two.
// Kernels:
//   mpo_entry_chain       one workgroup per row of the batch, every tensor in one launch: the carry is a row vector in LDS (two
//                         buffers), v <- v S_i left to right (qil_product.hip's chain with the factor summed in the load).
//   mpo_entry_combine     the GEMM route's per-row step: (V W_i) holds all four slices for every row, each row adds its own.
//   mpo_slice_grouped     ONE launch for all kept tensors, every output element written exactly once.  A tensor that absorbs a
//                         run is M (R x D_l) . A_k (D_l x 2 D_r) in 16 x 16 f64-MFMA tiles, one per wave, A_k gathered from W_k's
//                         slices by strides; a tensor that absorbs nothing is that gather alone.  A run of length 1 is read in
//                         place from the removed site's tensor.
//   mpo_slice_runs_lds    ONE launch for all runs of length >= 2 and every trailing run, one workgroup per run, the running
//                         product in LDS (qil_restrict.hip's run kernel with multi-term factors and a strided last step).
// A run takes the LDS kernel while every bond it touches is <= 96 (f64) / 64 (c64); wider runs go through qil_dev_gemm with
// multi-term factors materialised (slice_factor).  One call may mix the routes.  Contract: include/qilaplace_hip.h.
#include <algorithm>
#include <vector>

#include "qil_internal.h"
#include "qil_device_utils.h"

#ifndef QIL_MPO_SLICE_LDS_MAX_F64
#define QIL_MPO_SLICE_LDS_MAX_F64 96
#endif
#ifndef QIL_MPO_SLICE_LDS_MAX_C64
#define QIL_MPO_SLICE_LDS_MAX_C64 64
#endif

namespace {

using namespace qil_dev;

constexpr int64_t kRunLdsMaxBond[2] = {QIL_MPO_SLICE_LDS_MAX_F64, QIL_MPO_SLICE_LDS_MAX_C64};   // indexed by qil_dtype
constexpr int kThreads = 256;                     // four waves: four output tiles of the absorb, one run, one row of the batch
constexpr int kGatherElems = kThreads * 8;        // elements a workgroup gathers
constexpr long long kChainMaxBond = QIL_MPO_ENTRY_CHAIN_MAX_BOND;
static_assert(2 * kChainMaxBond * sizeof(c64) <= 64 * 1024, "the LDS carry must fit the default dynamic LDS limit");
// Unforced, the chain serves the calls it wins or loses by less than a quarter: bonds up to 64 and rows * bond^2 below 2^21
constexpr long long kChainAutoBond = 64, kChainAutoWork = 1LL << 21;

// ---- the vocabulary
// The slices t = s_in + 2 s_out a removed site adds, ascending: nt = 1: t0; 2: t0, t1; 4: 0, 1, 2, 3.
struct SiteTerms {
    int nt, t0, t1;
};
__host__ __device__ inline SiteTerms removed_terms(int in, int out) {
    if (in == 4) return SiteTerms{2, 0, 3};
    const int ni = in < 2 ? 1 : 2, no = out < 2 ? 1 : 2;
    const int t0 = (in < 2 ? in : 0) + 2 * (out < 2 ? out : 0);
    return SiteTerms{ni * no, t0, t0 + (ni == 2 ? 1 : 2)};
}
// A kept site: slice s of the result is slice t0 + ts s of W_i, plus slice t0 + ts s + t2 where t2 != 0 (the other leg summed).
struct KeptTerms {
    int t0, ts, t2;
};
inline KeptTerms kept_terms(int in, int out) {
    if (in == 5) return KeptTerms{0, 3, 0};
    if (in == 3) return out < 2 ? KeptTerms{2 * out, 1, 0} : KeptTerms{0, 1, 2};
    return in < 2 ? KeptTerms{in, 2, 0} : KeptTerms{0, 2, 1};
}
inline bool is_kept(int in, int out) { return in == 5 || (in == 3) != (out == 3); }

// the further terms of a factor, as element distances from its first slice
struct Terms {
    long long off[3];
    int nterms, pad;
};
// the fused operand load: entry idx of a factor, its 1, 2 or 4 slices added in ascending order
template <class T>
__device__ __forceinline__ T load_terms(const T* __restrict__ p, long long idx, const Terms& t) {
    T v = p[idx];
    if (t.nterms > 1) v = add_t(v, p[idx + t.off[0]]);
    if (t.nterms > 2) {
        v = add_t(v, p[idx + t.off[1]]);
        v = add_t(v, p[idx + t.off[2]]);
    }
    return v;
}

// ---- (a) entries, chain route
struct EntrySite {
    const void* W;  // MPO site [Dl, 2, 2, Dr]
    int Dl, Dr;
};

// v_out[beta] = sum_alpha v_in[alpha] S[alpha, beta]; groups of G lanes share one beta (product_chain's lane grouping).  The
// carry has the operator's dtype: a real operator never meets a complex number, its imaginary part is the constant 0.
template <class T>
__global__ __launch_bounds__(kThreads) void mpo_entry_chain(const EntrySite* __restrict__ sites, int n,
                                                            const uint8_t* __restrict__ spec, int maxD, c64* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char entry_carry[];
    T* v_in = reinterpret_cast<T*>(entry_carry);
    T* v_out = v_in + maxD;
    const long long q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int nwaves = kThreads / 64;
    if (threadIdx.x == 0) v_in[0] = cast_elem<T>(1.0);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const EntrySite S = sites[i];
        const SiteTerms st = removed_terms(spec[(q * n + i) * 2], spec[(q * n + i) * 2 + 1]);
        const T* __restrict__ A = static_cast<const T*>(S.W);
        Terms tm;
        tm.nterms = st.nt;
        tm.off[0] = (long long)S.Dl * (st.t1 - st.t0);
        tm.off[1] = 2LL * S.Dl;
        tm.off[2] = 3LL * S.Dl;
        int G = 64;  // lanes per dot product: smallest power of two >= Dl (cap 64)
        while (G > 1 && (G >> 1) >= S.Dl) G >>= 1;
        const int per_wave = 64 / G;
        const int grp = lane / G, gl = lane - grp * G;
        for (int beta = wave * per_wave + grp; beta < S.Dr; beta += nwaves * per_wave) {
            const T* col = A + (long long)S.Dl * (st.t0 + 4LL * beta);   // the four slices of the column: Dl entries each
            T acc{};
            for (int al = gl; al < S.Dl; al += G) acc = cmul_add(acc, v_in[al], load_terms(col, al, tm));
            for (int m = G >> 1; m >= 1; m >>= 1) acc = add_t(acc, shfl_xor_t(acc, m));
            if (gl == 0) v_out[beta] = acc;
        }
        __syncthreads();
        T* t = v_in;
        v_in = v_out;
        v_out = t;
    }
    if (threadIdx.x == 0) out[q] = to_c64(v_in[0]);
}

// ---- (b) entries, GEMM route: Tm (nb x 4 Dr, column t + 4 beta) holds V W_i for all four slices; row q keeps its own sum
template <class T>
__global__ void mpo_entry_combine(const T* __restrict__ Tm, long long nb, int Dr, const uint8_t* __restrict__ spec, int n, int i,
                                  T* __restrict__ Vn) {
    const long long total = nb * Dr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long q = t % nb, beta = t / nb;
        const SiteTerms st = removed_terms(spec[(q * n + i) * 2], spec[(q * n + i) * 2 + 1]);
        const T* x = Tm + q + nb * 4 * beta;
        T v = x[nb * st.t0];
        if (st.nt > 1) v = add_t(v, x[nb * st.t1]);
        if (st.nt > 2) {
            v = add_t(v, x[nb * 2]);
            v = add_t(v, x[nb * 3]);
        }
        Vn[t] = v;
    }
}

// ---- (c) slices: the grouped launch of the kept tensors
struct SliceSite {
    void* C;               // result [R, ncols], column s + 2 beta
    const void* B;         // the kept operand [K, ncols]: entry (k, s + 2 beta) = B[k + sstride s + bstride beta] (+ B[.. + boff2])
    const void* M;         // the absorbed factor [R, K]: M[r, k] = the terms of M[r + ldm k]; null = gather (R == K)
    long long ldm;
    Terms mt;
    long long sstride, bstride, boff2;
    long long ncols;       // 2 D_r
    long long block_begin; // first workgroup of this site in the grouped grid
    int R, K;
    int tiles_m, pad;      // ceil(R / 16)
};

template <class T>
__device__ __forceinline__ T load_kept(const SliceSite& S, const T* __restrict__ B, long long k, long long col) {
    const long long idx = k + S.sstride * (col & 1) + S.bstride * (col >> 1);
    T v = B[idx];
    if (S.boff2) v = add_t(v, B[idx + S.boff2]);     // the summed leg: the one IEEE addition
    return v;
}

template <class T>
__global__ __launch_bounds__(kThreads) void mpo_slice_grouped(const SliceSite* __restrict__ sites, int nsites) {
    const long long blk = blockIdx.x;
    const SliceSite S = sites[last_entry_le<&SliceSite::block_begin>(sites, nsites, blk)];   // block -> site
    const long long local = blk - S.block_begin;
    const T* __restrict__ B = static_cast<const T*>(S.B);
    T* __restrict__ C = static_cast<T*>(S.C);
    if (!S.M) {                                        // nothing absorbed: the gather of W's slices, bit for bit
        const long long elems = (long long)S.R * S.ncols;
        const long long e1 = min(elems, (local + 1) * kGatherElems);
        for (long long u = local * kGatherElems + threadIdx.x; u < e1; u += kThreads) C[u] = load_kept(S, B, u % S.R, u / S.R);
        return;
    }
    const long long t = local * (kThreads / 64) + (threadIdx.x >> 6);
    const long long ti = t % S.tiles_m, tj = t / S.tiles_m;
    if (16 * tj >= S.ncols) return;                    // the last workgroup's spare waves (no barrier below)
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const T* __restrict__ M = static_cast<const T*>(S.M);
    const long long row = 16 * ti + li;                // this lane's row of M (operand) and of C (result)
    const long long col = 16 * tj + li;                // this lane's column of B (operand)
    d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0};
    for (int k0 = 0; k0 < S.K; k0 += 4) {
        const int k = k0 + lk;
        T a{}, b{};
        if (row < S.R && k < S.K) a = load_terms(M, row + S.ldm * k, S.mt);
        if (col < S.ncols && k < S.K) b = load_kept(S, B, k, col);
        mfma_step(b, a, rr, ii);                       // D[i][j] = C[row0 + j][col0 + i]
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long ocol = 16 * tj + lk + 4 * r;
        if (row < S.R && ocol < S.ncols) C[row + (long long)S.R * ocol] = make_elem(rr[r], ii[r], (T*)nullptr);
    }
}

// ---- (d) slices: run products in LDS
struct RunStep {
    const void* p;         // the factor [K, N]: entry (k, c) at p[k + ld c], at p[c + ld k] when trans, or -- the last kept tensor
    long long ld;          // of a trailing run, split = D_l -- at p[c % split + sstride (c / split) + ld k]; its terms added
    Terms t;
    long long sstride;
    int K, N;
    int trans, split;
};
struct Run {
    void* out;             // the product [R, N of the last step], leading dimension R
    int R;
    int step_begin, nsteps;   // step 0 loads its factor (R x N), every further step multiplies from the right
    int pad;
};

template <class T>
__device__ __forceinline__ T load_step(const RunStep& s, long long k, long long c) {
    const long long idx = s.split ? c % s.split + s.sstride * (c / s.split) + s.ld * k : s.trans ? c + s.ld * k : k + s.ld * c;
    return load_terms(static_cast<const T*>(s.p), idx, s.t);
}

template <class T>
__global__ __launch_bounds__(kThreads) void mpo_slice_runs_lds(const Run* __restrict__ runs, const RunStep* __restrict__ steps,
                                                               int half_elems) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* cur = reinterpret_cast<T*>(lds_raw);
    T* nxt = cur + half_elems;
    const Run run = runs[blockIdx.x];
    const int R = run.R, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    int N = 0;
    {
        const RunStep s = steps[run.step_begin];
        N = s.N;
        for (int idx = tid; idx < R * N; idx += kThreads) cur[idx] = load_step<T>(s, idx % R, idx / R);
    }
    __syncthreads();
    const int tm = (R + 15) >> 4;
    for (int q = 1; q < run.nsteps; ++q) {
        const RunStep s = steps[run.step_begin + q];
        const int K = s.K, tn = (s.N + 15) >> 4;
        for (int t = wave; t < tm * tn; t += kThreads / 64) {
            const int row = 16 * (t % tm) + li, col = 16 * (t / tm) + li;
            d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0};
            for (int k0 = 0; k0 < K; k0 += 4) {
                const int k = k0 + lk;
                T a{}, b{};
                if (row < R && k < K) a = cur[row + R * k];
                if (col < s.N && k < K) b = load_step<T>(s, k, col);
                mfma_step(a, b, rr, ii);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int orow = 16 * (t % tm) + lk + 4 * r;
                if (orow < R && col < s.N) nxt[orow + R * col] = make_elem(rr[r], ii[r], (T*)nullptr);
            }
        }
        __syncthreads();
        T* sw = cur;
        cur = nxt;
        nxt = sw;
        N = s.N;
    }
    T* __restrict__ out = static_cast<T*>(run.out);
    for (int idx = tid; idx < R * N; idx += kThreads) out[idx] = cur[idx];
}

// ---- the GEMM route's materialisation of a multi-term factor: out[a + rows b] = the terms of p[a + ld b]
template <class T>
__global__ void slice_factor(const T* __restrict__ p, long long ld, Terms t, long long rows, long long cols, T* __restrict__ out) {
    const long long total = rows * cols;
    for (long long u = blockIdx.x * (long long)blockDim.x + threadIdx.x; u < total; u += (long long)gridDim.x * blockDim.x)
        out[u] = load_terms(p, u % rows + ld * (u / rows), t);
}

enum { kLeading = 0, kInterior = 1, kTrailing = 2 };
struct RunPlan {
    int64_t p, q;          // removed sites p .. q
    int64_t kept;          // index (in the result) of the kept tensor that absorbs the run
    int kind;
    void* out = nullptr;   // the product, where one is formed (runs of length >= 2, trailing runs)
};

// a D_l x D_r matrix inside a site, read in place
struct Factor {
    const void* p;
    long long ld;
    Terms t;
};

struct Slicing {
    const qil_mpo* W;
    const uint8_t* spec;
    qil_context* ctx;
    int dt;
    size_t e;
    std::vector<int64_t> kept;       // parent indices of the kept tensors
    std::vector<RunPlan> runs;
    std::vector<void*> temps;        // every pool block of the call, freed at the end (stream-ordered reuse)

    int64_t cl(int64_t i) const { return W->dims[(size_t)i]; }
    int64_t cr(int64_t i) const { return W->dims[(size_t)i + 1]; }
    int alloc(size_t elems, void** out) {
        QIL_TRY(qil_ctx_alloc(ctx, std::max<size_t>(elems, 1) * e, out));
        temps.push_back(*out);
        return QIL_OK;
    }
    // removed site i's factor S_i
    Factor factor(int64_t i) const {
        const SiteTerms st = removed_terms(spec[2 * i], spec[2 * i + 1]);
        Factor f{};
        f.p = static_cast<const char*>(W->site[(size_t)i]) + (size_t)st.t0 * (size_t)cl(i) * e;
        f.ld = 4 * cl(i);
        f.t.nterms = st.nt;
        f.t.off[0] = (long long)(st.t1 - st.t0) * cl(i);
        f.t.off[1] = 2 * cl(i);
        f.t.off[2] = 3 * cl(i);
        return f;
    }
    // slice s of kept site k
    Factor kept_slice(int64_t k, int s) const {
        const KeptTerms kt = kept_terms(spec[2 * k], spec[2 * k + 1]);
        Factor f{};
        f.p = static_cast<const char*>(W->site[(size_t)k]) + (size_t)(kt.t0 + kt.ts * s) * (size_t)cl(k) * e;
        f.ld = 4 * cl(k);
        f.t.nterms = kt.t2 ? 2 : 1;
        f.t.off[0] = (long long)kt.t2 * cl(k);
        return f;
    }
    bool forms_product(const RunPlan& r) const { return r.kind == kTrailing || r.q > r.p; }
    bool fits_lds(const RunPlan& r) const {
        int64_t top = 1;
        for (int64_t i = r.p; i <= r.q; ++i) top = std::max(top, std::max(cl(i), cr(i)));
        if (r.kind == kTrailing) top = std::max(top, cl(r.p - 1));       // the last kept tensor closes the chain
        return top <= kRunLdsMaxBond[dt];
    }
    // a factor (rows x cols) of a GEMM-route step as a plain matrix: in place for one term, materialised into `sl` otherwise
    int gemm_factor(const Factor& f, int64_t rows, int64_t cols, void* sl, const void** B, long long* ldb) {
        *B = f.p;
        *ldb = f.ld;
        if (f.t.nterms == 1) return QIL_OK;
        const unsigned g = (unsigned)std::min<long long>((rows * cols + 255) / 256, 4096);
        if (dt == QIL_C64)
            hipLaunchKernelGGL(slice_factor<c64>, dim3(g), dim3(256), 0, qil_stream(ctx), (const c64*)f.p, f.ld, f.t, (long long)rows,
                               (long long)cols, (c64*)sl);
        else
            hipLaunchKernelGGL(slice_factor<double>, dim3(g), dim3(256), 0, qil_stream(ctx), (const double*)f.p, f.ld, f.t,
                               (long long)rows, (long long)cols, (double*)sl);
        QIL_HIP(hipGetLastError());
        *B = sl;
        *ldb = rows;
        return QIL_OK;
    }
    int run_by_gemm(const RunPlan& r);
    int launch_runs_lds(const std::vector<const RunPlan*>& sel);
    int launch_grouped(qil_mps* res);
};

// bonds above the LDS limit: the same association order through qil_dev_gemm
int Slicing::run_by_gemm(const RunPlan& r) {
    int64_t wide = 1, slice = 1;
    for (int64_t i = r.p; i <= r.q; ++i) {
        wide = std::max(wide, std::max(cl(i), cr(i)));
        slice = std::max(slice, cl(i) * cr(i));
    }
    if (r.kind == kTrailing) slice = std::max(slice, cl(r.p - 1) * cr(r.p - 1));
    const int64_t R = r.kind == kTrailing ? 1 : cl(r.p);
    void *ping = nullptr, *pong = nullptr, *sl = nullptr;
    QIL_TRY(alloc((size_t)(R * wide), &ping));
    QIL_TRY(alloc((size_t)(R * wide), &pong));
    QIL_TRY(alloc((size_t)slice, &sl));
    const void* cur = nullptr;
    long long ldc = 0;
    if (r.kind != kTrailing) {                                  // ((S_p S_p+1) S_p+2) ...
        QIL_TRY(gemm_factor(factor(r.p), cl(r.p), cr(r.p), ping, &cur, &ldc));   // a multi-term S_p goes straight into the first buffer
        for (int64_t i = r.p + 1; i <= r.q; ++i) {
            const void* B = nullptr;
            long long ldb = 0;
            QIL_TRY(gemm_factor(factor(i), cl(i), cr(i), sl, &B, &ldb));
            void* dest = i == r.q ? r.out : (cur == pong ? ping : pong);
            QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, R, cr(i), cl(i), cur, ldc, B, ldb, dest, R));
            cur = dest;
            ldc = R;
        }
        return QIL_OK;
    }
    QIL_TRY(gemm_factor(factor(r.q), cl(r.q), 1, ping, &cur, &ldc));   // S_q is a column: D x 1
    for (int64_t i = r.q - 1; i >= r.p; --i) {                  // S_p (S_p+1 (... S_q))
        const void* A = nullptr;
        long long lda = 0;
        QIL_TRY(gemm_factor(factor(i), cl(i), cr(i), sl, &A, &lda));
        void* dest = cur == pong ? ping : pong;
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, cl(i), 1, cr(i), A, lda, cur, cr(i), dest, cl(i)));
        cur = dest;
    }
    const int64_t k = r.p - 1;                                  // A_k[:, s, :] c, one product per kept slice: (D_l x D_r) (D_r x 1)
    for (int s = 0; s < 2; ++s) {
        const void* A = nullptr;
        long long lda = 0;
        QIL_TRY(gemm_factor(kept_slice(k, s), cl(k), cr(k), sl, &A, &lda));
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, cl(k), 1, cr(k), A, lda, cur, cr(k), static_cast<char*>(r.out) + (size_t)s * (size_t)cl(k) * e,
                             cl(k)));
    }
    return QIL_OK;
}

int Slicing::launch_runs_lds(const std::vector<const RunPlan*>& sel) {
    if (sel.empty()) return QIL_OK;
    std::vector<Run> rtab;
    std::vector<RunStep> stab;
    long long half = 1;
    for (const RunPlan* r : sel) {
        Run run{};
        run.out = r->out;
        run.R = r->kind == kInterior ? (int)cl(r->p) : 1;
        run.step_begin = (int)stab.size();
        auto push = [&](int64_t i, int K, int N, int trans) {
            const Factor f = factor(i);
            RunStep s{};
            s.p = f.p;
            s.ld = f.ld;
            s.t = f.t;
            s.K = K;
            s.N = N;
            s.trans = trans;
            stab.push_back(s);
            half = std::max(half, (long long)run.R * N);
        };
        if (r->kind != kTrailing) {
            for (int64_t i = r->p; i <= r->q; ++i) push(i, (int)cl(i), (int)cr(i), 0);
        } else {                                                // the column is carried transposed: c^T S_i^T
            for (int64_t i = r->q; i >= r->p; --i) push(i, (int)cr(i), (int)cl(i), 1);
            const int64_t k = r->p - 1;
            const Factor f0 = kept_slice(k, 0), f1 = kept_slice(k, 1);
            RunStep s{};                                         // the last kept tensor: column a + D_l s, row b
            s.p = f0.p;
            s.ld = f0.ld;
            s.t = f0.t;
            s.sstride = (long long)((static_cast<const char*>(f1.p) - static_cast<const char*>(f0.p)) / (long long)e);
            s.split = (int)cl(k);
            s.K = (int)cr(k);
            s.N = (int)(2 * cl(k));
            stab.push_back(s);
            half = std::max(half, (long long)s.N);
        }
        run.nsteps = (int)stab.size() - run.step_begin;
        rtab.push_back(run);
    }
    const size_t rbytes = rtab.size() * sizeof(Run);
    const size_t lds = 2 * (size_t)half * e;                    // <= 144 KiB by kRunLdsMaxBond
    qil_dev_table tab(ctx);
    QIL_TRY(tab.upload(rtab.data(), rbytes, stab.data(), stab.size() * sizeof(RunStep)));
    const Run* druns = tab.as<Run>();
    const RunStep* dsteps = tab.as<RunStep>(rbytes);
    const dim3 grid((unsigned)rtab.size()), block(kThreads);
    static qil_lds_grant grant_r, grant_c;                      // per device (qil_internal.h)
    if (dt == QIL_C64) {
        QIL_HIP(grant_c.ensure(ctx->device, reinterpret_cast<const void*>(&mpo_slice_runs_lds<c64>), lds));
        hipLaunchKernelGGL(mpo_slice_runs_lds<c64>, grid, block, lds, qil_stream(ctx), druns, dsteps, (int)half);
    } else {
        QIL_HIP(grant_r.ensure(ctx->device, reinterpret_cast<const void*>(&mpo_slice_runs_lds<double>), lds));
        hipLaunchKernelGGL(mpo_slice_runs_lds<double>, grid, block, lds, qil_stream(ctx), druns, dsteps, (int)half);
    }
    QIL_HIP(hipGetLastError());
    return tab.release();
}

int Slicing::launch_grouped(qil_mps* res) {
    const int64_t m = res->n();
    std::vector<SliceSite> tab((size_t)m);
    for (int64_t j = 0; j < m; ++j) {                           // every kept tensor starts as the gather of its parent's slices
        const int64_t k = kept[(size_t)j];
        const Factor f0 = kept_slice(k, 0), f1 = kept_slice(k, 1);
        SliceSite& s = tab[(size_t)j];
        s = SliceSite{};
        s.C = res->site[(size_t)j];
        s.B = f0.p;
        s.sstride = (long long)((static_cast<const char*>(f1.p) - static_cast<const char*>(f0.p)) / (long long)e);
        s.bstride = f0.ld;
        s.boff2 = f0.t.nterms == 2 ? f0.t.off[0] : 0;
        s.R = s.K = (int)cl(k);
        s.ncols = 2 * cr(k);
    }
    for (const RunPlan& r : runs) {
        SliceSite& s = tab[(size_t)r.kept];
        if (r.kind == kTrailing) {                              // A_k c comes from the run stage: D_l x 2 x 1, plain
            s.B = r.out;
            s.sstride = s.K;
            s.bstride = 2LL * s.K;
            s.boff2 = 0;
            s.ncols = 2;
            continue;
        }
        s.R = r.kind == kLeading ? 1 : (int)cl(r.p);
        if (r.out) {
            s.M = r.out;
            s.ldm = s.R;
            s.mt = Terms{};
            s.mt.nterms = 1;
        } else {
            const Factor f = factor(r.p);                        // a run of length 1, in place
            s.M = f.p;
            s.ldm = f.ld;
            s.mt = f.t;
        }
    }
    long long blocks = 0;
    for (SliceSite& s : tab) {
        s.tiles_m = (s.R + 15) / 16;
        s.block_begin = blocks;
        if (s.M) {
            const long long tiles = (long long)s.tiles_m * ((s.ncols + 15) / 16);
            blocks += (tiles + kThreads / 64 - 1) / (kThreads / 64);
        } else {
            blocks += std::max<long long>(1, ((long long)s.R * s.ncols + kGatherElems - 1) / kGatherElems);
        }
    }
    QIL_REQUIRE(blocks < (1LL << 31), QIL_EINVAL_ARG, "mpo_slice: grid too large (%lld workgroups)", blocks);
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(SliceSite)));
    const SliceSite* dsites = dtab.as<SliceSite>();
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (dt == QIL_C64) hipLaunchKernelGGL(mpo_slice_grouped<c64>, grid, block, 0, qil_stream(ctx), dsites, (int)m);
    else hipLaunchKernelGGL(mpo_slice_grouped<double>, grid, block, 0, qil_stream(ctx), dsites, (int)m);
    QIL_HIP(hipGetLastError());
    return dtab.release();
}

// ---- entries: the two routes
long long widest_bond(const qil_mpo* W) {
    long long m = 1;
    for (int64_t d : W->dims) m = std::max<long long>(m, d);
    return m;
}

int entry_chain_route(const qil_mpo* W, int64_t nb, const uint8_t* dspec, c64* dout) {
    qil_context* ctx = W->ctx;
    const int64_t n = W->n();
    std::vector<EntrySite> tab((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        tab[(size_t)i] = EntrySite{W->site[(size_t)i], (int)W->dims[(size_t)i], (int)W->dims[(size_t)i + 1]};
    const long long maxD = widest_bond(W);
    const size_t lds = 2 * (size_t)maxD * qil_elem_size(W->dtype);
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(EntrySite)));
    if (W->dtype == QIL_C64)
        hipLaunchKernelGGL(mpo_entry_chain<c64>, dim3((unsigned)nb), dim3(kThreads), lds, qil_stream(ctx), dtab.as<EntrySite>(), (int)n,
                           dspec, (int)maxD, dout);
    else
        hipLaunchKernelGGL(mpo_entry_chain<double>, dim3((unsigned)nb), dim3(kThreads), lds, qil_stream(ctx), dtab.as<EntrySite>(),
                           (int)n, dspec, (int)maxD, dout);
    QIL_HIP(hipGetLastError());
    return dtab.release();
}

// all rows of a chunk together: one product per tensor with the site as the D_l x 4 D_r matrix it is in memory
int entry_gemm_route(const qil_mpo* W, qil_scratch& tmp, int64_t nb, const uint8_t* dspec, c64* dout) {
    qil_context* ctx = W->ctx;
    const int64_t n = W->n();
    const int dt = W->dtype;
    const size_t e = qil_elem_size(dt);
    long long maxD = 1;
    for (int64_t i = 1; i <= n; ++i) maxD = std::max<long long>(maxD, W->dims[(size_t)i]);
    const int64_t chunk = qil_apply_chunk_rows(nb, (int64_t)(6 * maxD * (long long)e));   // V, Vn and the four slices of Tm
    void *V = nullptr, *Vn = nullptr, *Tm = nullptr;
    QIL_TRY(tmp.alloc((size_t)(chunk * maxD) * e, &V));
    QIL_TRY(tmp.alloc((size_t)(chunk * maxD) * e, &Vn));
    QIL_TRY(tmp.alloc((size_t)(4 * chunk * maxD) * e, &Tm));
    for (int64_t r0 = 0; r0 < nb; r0 += chunk) {
        const int64_t rows = std::min(chunk, nb - r0);
        const uint8_t* sp = dspec + (size_t)r0 * (size_t)n * 2;
        QIL_TRY(qil_dev_fill_ones(ctx, dt, V, rows));
        for (int64_t i = 0; i < n; ++i) {
            const int64_t Dl = W->dims[(size_t)i], Dr = W->dims[(size_t)i + 1];
            QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, rows, 4 * Dr, Dl, V, rows, W->site[(size_t)i], Dl, Tm, rows));
            const unsigned g = (unsigned)std::min<long long>((rows * Dr + 255) / 256, 65536);
            if (dt == QIL_C64)
                hipLaunchKernelGGL(mpo_entry_combine<c64>, dim3(g), dim3(256), 0, qil_stream(ctx), (const c64*)Tm, (long long)rows,
                                   (int)Dr, sp, (int)n, (int)i, (c64*)Vn);
            else
                hipLaunchKernelGGL(mpo_entry_combine<double>, dim3(g), dim3(256), 0, qil_stream(ctx), (const double*)Tm,
                                   (long long)rows, (int)Dr, sp, (int)n, (int)i, (double*)Vn);
            QIL_HIP(hipGetLastError());
            std::swap(V, Vn);
        }
        QIL_TRY(qil_dev_finish_coeff(ctx, dt, V, rows, 1.0, dout + r0));
    }
    return QIL_OK;
}

}  // namespace

extern "C" int qil_mpo_entry_batch(const qil_mpo* W, int64_t nb, const uint8_t* spec, double* out) {
    QIL_REQUIRE(W && (nb <= 0 || (spec && out)), QIL_EINVAL_ARG, "mpo_entry_batch: null argument");
    QIL_REQUIRE(nb >= 0, QIL_EINVAL_ARG, "mpo_entry_batch: nb must be non-negative, got %lld", (long long)nb);
    if (nb == 0) return QIL_OK;
    const int64_t n = W->n();
    for (int64_t r = 0; r < nb; ++r)
        for (int64_t i = 0; i < n; ++i) {
            const int a = spec[(r * n + i) * 2], b = spec[(r * n + i) * 2 + 1];
            QIL_REQUIRE((a <= 2 && b <= 2) || (a == 4 && b == 4), QIL_EINVAL_CONFIG,
                        "mpo_entry_batch: spec (%d, %d) of row %lld, tensor %lld: a leg is 0, 1 or 2, a traced site (4, 4); a kept "
                        "leg makes no number",
                        a, b, (long long)r, (long long)i);
        }
    QIL_REQUIRE(nb < (1LL << 31), QIL_EINVAL_ARG, "mpo_entry_batch: nb = %lld is too large for one call", (long long)nb);
    qil_context* ctx = W->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    // The auto rule, from the measured crossover (24 tensors, chain against GEMM in ms, f64 / c64): 64 rows, bond 16: 0.09 / 0.09
    // against 0.21 / 0.23, bond 64: 0.25 / 0.30 against 0.22 / 0.25, bond 96: 0.47 / 0.52 against 0.23 / 0.28; 1024 rows, bond 32:
    // 0.17 / 0.20 against 0.25 / 0.28, bond 64: 0.34 / 0.51 against 0.27 / 0.33; 4096 rows, bond 16: 0.31 / 0.32 against 0.40 /
    // 0.45, bond 512: 12.3 / 28.0 against 3.8 / 10.9.  Every workgroup of the chain streams the whole operator, so it loses
    // where the operator is large or the rows are many.
    const long long wb = widest_bond(W);
    bool chain = wb <= kChainAutoBond && nb * wb * wb < kChainAutoWork;
    const char* forced = getenv("QIL_MPO_ENTRY_ROUTE");
    if (forced && !strcmp(forced, "chain")) chain = true;
    else if (forced && !strcmp(forced, "gemm")) chain = false;
    chain = chain && wb <= kChainMaxBond;    // the LDS carry bounds the bond
    void *dspec = nullptr, *dout = nullptr;
    QIL_TRY(tmp.alloc((size_t)nb * 16, &dout));
    QIL_TRY(qil_upload_bytes(tmp, spec, (size_t)(nb * n) * 2, &dspec));
    if (chain) QIL_TRY(entry_chain_route(W, nb, static_cast<const uint8_t*>(dspec), static_cast<c64*>(dout)));
    else QIL_TRY(entry_gemm_route(W, tmp, nb, static_cast<const uint8_t*>(dspec), static_cast<c64*>(dout)));
    QIL_HIP(hipMemcpyAsync(out, dout, (size_t)nb * 16, hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));
    return QIL_OK;
}

extern "C" int qil_mpo_slice(const qil_mpo* W, const uint8_t* spec, qil_mps** out) {
    QIL_REQUIRE(W && spec && out, QIL_EINVAL_ARG, "mpo_slice: null argument");
    const int64_t n = W->n();
    Slicing sl{W, spec, W->ctx, W->dtype, qil_elem_size(W->dtype)};
    for (int64_t i = 0; i < n; ++i) {
        const int a = spec[2 * i], b = spec[2 * i + 1];
        QIL_REQUIRE(a <= 5 && b <= 5, QIL_EINVAL_CONFIG, "mpo_slice: spec value %d of tensor %lld outside [0,5]", std::max(a, b),
                    (long long)i);
        QIL_REQUIRE((a < 4 && b < 4) || a == b, QIL_EINVAL_CONFIG,
                    "mpo_slice: spec (%d, %d) of tensor %lld: 4 (trace) and 5 (diagonal) tie both legs of a site", a, b, (long long)i);
        QIL_REQUIRE(!(a == 3 && b == 3), QIL_EINVAL_CONFIG,
                    "mpo_slice: tensor %lld keeps both legs: sub-operators are not built", (long long)i);
        if (is_kept(a, b)) sl.kept.push_back(i);
    }
    QIL_REQUIRE(!sl.kept.empty(), QIL_EINVAL_CONFIG, "mpo_slice: the spec keeps no site; that number is what mpo_entry_batch returns");
    qil_context* ctx = W->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int64_t m = (int64_t)sl.kept.size();
    // the maximal runs of removed sites and the kept tensor each goes into: the one on its right, the last one for a trailing run
    for (int64_t j = 0; j <= m; ++j) {
        const int64_t p = j == 0 ? 0 : sl.kept[(size_t)j - 1] + 1, q = (j == m ? n : sl.kept[(size_t)j]) - 1;
        if (q < p) continue;
        RunPlan r{};
        r.p = p;
        r.q = q;
        r.kind = j == m ? kTrailing : j == 0 ? kLeading : kInterior;
        r.kept = j == m ? m - 1 : j;
        sl.runs.push_back(r);
    }
    // whole (main_i, copy_i) pairs kept: the result is a paired chain
    int paired = W->paired && m % 2 == 0;
    for (int64_t j = 0; paired && j < m; j += 2)
        paired = sl.kept[(size_t)j] % 2 == 0 && sl.kept[(size_t)j + 1] == sl.kept[(size_t)j] + 1;
    std::vector<int64_t> bonds, ids;
    for (int64_t j = 0; j < m; ++j) {
        if (j + 1 < m) bonds.push_back(sl.cr(sl.kept[(size_t)j]));
        ids.push_back(W->site_ids[(size_t)sl.kept[(size_t)j]]);
    }
    qil_mps* res = nullptr;
    QIL_TRY(qil_mps_alloc(ctx, m, W->dtype, paired, bonds.data(), ids.data(), 1.0, &res));
    qil_result_guard<qil_mps> guard(res);     // the call scope returns the temporaries; the result is a handle of its own
    std::vector<const RunPlan*> in_lds;
    for (RunPlan& r : sl.runs) {
        if (!sl.forms_product(r)) continue;
        const int64_t k = sl.kept[(size_t)r.kept];
        const int64_t elems = r.kind == kTrailing ? 2 * sl.cl(k) : (r.kind == kLeading ? 1 : sl.cl(r.p)) * sl.cr(r.q);
        QIL_TRY(sl.alloc((size_t)elems, &r.out));
        if (sl.fits_lds(r)) in_lds.push_back(&r);
    }
    QIL_TRY(sl.launch_runs_lds(in_lds));
    for (const RunPlan& r : sl.runs)
        if (sl.forms_product(r) && !sl.fits_lds(r)) QIL_TRY(sl.run_by_gemm(r));
    QIL_TRY(sl.launch_grouped(res));
    for (void* t : sl.temps) QIL_TRY(qil_ctx_free(ctx, t));
    *out = guard.release();
    return QIL_OK;
}
