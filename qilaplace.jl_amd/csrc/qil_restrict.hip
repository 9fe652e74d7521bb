// MPS-valued restriction for gfx950: qil_mps_restrict fixes (spec 0 / 1), sums (2) or keeps (3) every site of a chain and returns
// the chain of the kept tensors -- the counterpart of qil_mps_block whose kept sites stay site tensors.
//
// A removed site is a chi_l x chi_r factor S_i (a bit slice, or the sum of the two slices); a maximal run of removed sites is
// the product M of its factors and is absorbed into a kept neighbour (contract and association order: include/qilaplace_hip.h).
// Two kernels:
//   restrict_absorb_grouped   ONE launch for all kept sites, every output element written exactly once.  A site that absorbs
//                             a run is the product M (chi' x chi_l) . A_k (chi_l x 2 chi_r) in 16 x 16 f64-MFMA tiles, one tile
//                             per wave; a site that absorbs nothing is copied in 16-byte units by the same launch.  A run of
//                             length 1 -- every run when all copy bits of a paired chain are fixed -- is read IN PLACE from the
//                             removed site's tensor: the bit select is a stride (2 chi_l) and the two-slice sum is made in the
//                             operand load, no S_i goes to HBM.  The product is accumulated transposed (D = B^T M^T) so that a
//                             lane's 16-lane row stores 16 consecutive rows of one output column.
//   restrict_runs_lds         ONE launch for all runs of length >= 2 (and every trailing run), one workgroup per run: the
//                             running product lives in LDS (two buffers, ping-pong), the factors stream from HBM through the
//                             same fused load.  Leading runs are row-vector chains (1 x chi), trailing runs column-vector chains
//                             walked from the right (carried transposed, 1 x chi, through the last kept tensor).
// A run takes the LDS kernel while every bond it touches is <= kRunLdsMaxBond (96 for f64: 2 x 96 x 96 x 8 B = 144 KiB; 64 for
// c64: 2 x 64 x 64 x 16 B = 128 KiB; a CU has 160 KiB); above that its factors are materialised (restrict_factor) where they are
// sums and multiplied by qil_dev_gemm, as qil_mps_block does.  One call may mix both routes.
// Deliberately absent: the lazy form (a slice of W psi without forming it), a batch of specs in one call, Born marginals.
#include <algorithm>
#include <vector>

#include "qil_internal.h"
#include "qil_device_utils.h"

#ifndef QIL_RESTRICT_LDS_MAX_F64
#define QIL_RESTRICT_LDS_MAX_F64 96
#endif
#ifndef QIL_RESTRICT_LDS_MAX_C64
#define QIL_RESTRICT_LDS_MAX_C64 64
#endif

namespace {

using namespace qil_dev;

constexpr int64_t kRunLdsMaxBond[2] = {QIL_RESTRICT_LDS_MAX_F64, QIL_RESTRICT_LDS_MAX_C64};   // indexed by qil_dtype
constexpr int kThreads = 256;                     // four waves: four output tiles of the absorb, one run of the run kernel
constexpr int kCopyUnits = kThreads * 8;          // 16-byte units a workgroup copies (32 KiB)

typedef double d2 __attribute__((ext_vector_type(2)));

// the fused operand load: entry idx of a removed site's factor, slice 0 + slice 1 when the site is summed (off2 != 0)
template <class T>
__device__ __forceinline__ T load_factor(const T* __restrict__ p, long long idx, long long off2) {
    T v = p[idx];
    if (off2) v = add_t(v, p[idx + off2]);
    return v;
}

// ---- (a) grouped absorb
struct AbsorbSite {
    void* C;               // result [R, ncols]
    const void* B;         // the kept operand [K, ncols], leading dimension K
    const void* M;         // the absorbed factor [R, K]: M[r, k] = M[r + ldm k] (+ M[r + ldm k + off2]); null = copy (R == K)
    long long ldm, off2;
    long long ncols;       // 2 chi_r
    long long block_begin; // first workgroup of this site in the grouped grid
    int R, K;
    int tiles_m, pad;      // ceil(R / 16)
};

template <class T>
__global__ __launch_bounds__(kThreads) void restrict_absorb_grouped(const AbsorbSite* __restrict__ sites, int nsites) {
    const long long blk = blockIdx.x;
    const AbsorbSite S = sites[last_entry_le<&AbsorbSite::block_begin>(sites, nsites, blk)];   // block -> site
    const long long local = blk - S.block_begin;
    if (!S.M) {                                        // nothing absorbed: a bit-for-bit copy, 16 bytes per lane and step
        const long long units = (long long)S.R * S.ncols * (long long)sizeof(T) / 16;   // ncols is even
        const d2* __restrict__ src = static_cast<const d2*>(S.B);
        d2* __restrict__ dst = static_cast<d2*>(S.C);
        const long long u1 = min(units, (local + 1) * kCopyUnits);
        for (long long u = local * kCopyUnits + threadIdx.x; u < u1; u += kThreads) dst[u] = src[u];
        return;
    }
    const long long t = local * (kThreads / 64) + (threadIdx.x >> 6);
    const long long ti = t % S.tiles_m, tj = t / S.tiles_m;
    if (16 * tj >= S.ncols) return;                    // the last workgroup's spare waves (no barrier below)
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const T* __restrict__ M = static_cast<const T*>(S.M);
    const T* __restrict__ B = static_cast<const T*>(S.B);
    const long long row = 16 * ti + li;                // this lane's row of M (operand) and of C (result)
    const long long col = 16 * tj + li;                // this lane's column of B (operand)
    d4 rr = {0, 0, 0, 0}, ii = {0, 0, 0, 0};
    for (int k0 = 0; k0 < S.K; k0 += 4) {
        const int k = k0 + lk;
        T a{}, b{};
        if (row < S.R && k < S.K) a = load_factor(M, row + S.ldm * k, S.off2);
        if (col < S.ncols && k < S.K) b = B[k + (long long)S.K * col];
        mfma_step(b, a, rr, ii);                       // D[i][j] = C[row0 + j][col0 + i]
    }
    T* __restrict__ C = static_cast<T*>(S.C);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long ocol = 16 * tj + lk + 4 * r;
        if (row < S.R && ocol < S.ncols) C[row + (long long)S.R * ocol] = make_elem(rr[r], ii[r], (T*)nullptr);
    }
}

// ---- (b) run products in LDS
struct RunStep {
    const void* p;         // the factor [K, N]: entry (k, c) at p[k + ld c], or at p[c + ld k] when trans
    long long ld, off2;
    int K, N;
    int trans, pad;
};
struct Run {
    void* out;             // the product [R, N of the last step], leading dimension R
    int R;
    int step_begin, nsteps;   // step 0 loads its factor (R x N), every further step multiplies from the right
    int pad;
};

template <class T>
__device__ __forceinline__ T load_step(const RunStep& s, long long k, long long c) {
    return load_factor(static_cast<const T*>(s.p), s.trans ? c + s.ld * k : k + s.ld * c, s.off2);
}

template <class T>
__global__ __launch_bounds__(kThreads) void restrict_runs_lds(const Run* __restrict__ runs, const RunStep* __restrict__ steps,
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

// ---- the GEMM route's materialisation of a summed site: out[a, b] = A[a, 0, b] + A[a, 1, b]
template <class T>
__global__ void restrict_factor(const T* __restrict__ A, long long cl, long long cr, T* __restrict__ out) {
    const long long total = cl * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x)
        out[t] = load_factor(A, t % cl + 2 * cl * (t / cl), cl);
}

enum { kLeading = 0, kInterior = 1, kTrailing = 2 };
struct RunPlan {
    int64_t p, q;          // removed sites p .. q
    int64_t kept;          // index (in the result) of the kept tensor that absorbs the run
    int kind;
    void* out = nullptr;   // the product, where one is formed (runs of length >= 2, trailing runs)
};

struct Restriction {
    const qil_mps* psi;
    const uint8_t* spec;
    qil_context* ctx;
    int dt;
    size_t e;
    std::vector<int64_t> kept;       // parent indices of the kept tensors
    std::vector<RunPlan> runs;
    std::vector<void*> temps;        // every pool block of the call, freed at the end (stream-ordered reuse)

    int64_t cl(int64_t i) const { return psi->dims[(size_t)i]; }
    int64_t cr(int64_t i) const { return psi->dims[(size_t)i + 1]; }
    int alloc(size_t elems, void** out) {
        QIL_TRY(qil_ctx_alloc(ctx, std::max<size_t>(elems, 1) * e, out));
        temps.push_back(*out);
        return QIL_OK;
    }
    // site i's factor read in place: base pointer, leading dimension and the distance to the second slice (0: a fixed bit)
    void factor(int64_t i, const void** p, long long* ld, long long* off2) const {
        const char* A = static_cast<const char*>(psi->site[(size_t)i]);
        const bool sum = spec[i] == 2;
        *p = sum ? A : A + (size_t)spec[i] * (size_t)cl(i) * e;
        *ld = 2 * cl(i);
        *off2 = sum ? cl(i) : 0;
    }
    bool forms_product(const RunPlan& r) const { return r.kind == kTrailing || r.q > r.p; }
    bool fits_lds(const RunPlan& r) const {
        int64_t top = 1;
        for (int64_t i = r.p; i <= r.q; ++i) top = std::max(top, std::max(cl(i), cr(i)));
        if (r.kind == kTrailing) top = std::max(top, cl(r.p - 1));       // the last kept tensor closes the chain
        return top <= kRunLdsMaxBond[dt];
    }
    // the factor of a GEMM-route step as a plain matrix: in place for a fixed bit, materialised into `sl` for a summed site
    int gemm_factor(int64_t i, void* sl, const void** B, long long* ldb) {
        long long off2 = 0;
        factor(i, B, ldb, &off2);
        if (!off2) return QIL_OK;
        const unsigned g = (unsigned)std::min<long long>((cl(i) * cr(i) + 255) / 256, 4096);
        if (dt == QIL_C64)
            hipLaunchKernelGGL(restrict_factor<c64>, dim3(g), dim3(256), 0, qil_stream(ctx), (const c64*)*B, (long long)cl(i),
                               (long long)cr(i), (c64*)sl);
        else
            hipLaunchKernelGGL(restrict_factor<double>, dim3(g), dim3(256), 0, qil_stream(ctx), (const double*)*B, (long long)cl(i),
                               (long long)cr(i), (double*)sl);
        QIL_HIP(hipGetLastError());
        *B = sl;
        *ldb = cl(i);
        return QIL_OK;
    }
    int run_by_gemm(const RunPlan& r);
    int launch_runs_lds(const std::vector<const RunPlan*>& sel);
    int launch_absorb(qil_mps* res);
};

// bonds above the LDS limit: the same association order through qil_dev_gemm
int Restriction::run_by_gemm(const RunPlan& r) {
    int64_t wide = 1, slice = 1;
    for (int64_t i = r.p; i <= r.q; ++i) {
        wide = std::max(wide, std::max(cl(i), cr(i)));
        slice = std::max(slice, cl(i) * cr(i));
    }
    const int64_t R = r.kind == kTrailing ? 1 : cl(r.p);
    void *ping = nullptr, *pong = nullptr, *sl = nullptr;
    QIL_TRY(alloc((size_t)(R * wide), &ping));
    QIL_TRY(alloc((size_t)(R * wide), &pong));
    QIL_TRY(alloc((size_t)slice, &sl));
    const void* cur = nullptr;
    long long ldc = 0;
    if (r.kind != kTrailing) {                                  // ((S_p S_p+1) S_p+2) ...
        QIL_TRY(gemm_factor(r.p, ping, &cur, &ldc));            // a summed S_p is materialised straight into the first buffer
        for (int64_t i = r.p + 1; i <= r.q; ++i) {
            const void* B = nullptr;
            long long ldb = 0;
            QIL_TRY(gemm_factor(i, sl, &B, &ldb));
            void* dest = i == r.q ? r.out : (cur == pong ? ping : pong);
            QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, R, cr(i), cl(i), cur, ldc, B, ldb, dest, R));
            cur = dest;
            ldc = R;
        }
        return QIL_OK;
    }
    QIL_TRY(gemm_factor(r.q, ping, &cur, &ldc));                // S_q is a column: chi x 1
    for (int64_t i = r.q - 1; i >= r.p; --i) {                  // S_p (S_p+1 (... S_q))
        const void* A = nullptr;
        long long lda = 0;
        QIL_TRY(gemm_factor(i, sl, &A, &lda));
        void* dest = cur == pong ? ping : pong;
        QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, cl(i), 1, cr(i), A, lda, cur, cr(i), dest, cl(i)));
        cur = dest;
    }
    const int64_t k = r.p - 1;                                  // A_k[:, s, :] c for both s: (2 chi_l x chi_r) (chi_r x 1)
    return qil_dev_gemm(ctx, dt, 0, 0, 2 * cl(k), 1, cr(k), psi->site[(size_t)k], 2 * cl(k), cur, cr(k), r.out, 2 * cl(k));
}

int Restriction::launch_runs_lds(const std::vector<const RunPlan*>& sel) {
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
            RunStep s{};
            factor(i, &s.p, &s.ld, &s.off2);
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
            RunStep s{};                                         // the last kept tensor as a (2 chi_l) x chi_r matrix
            s.p = psi->site[(size_t)k];
            s.ld = 2 * cl(k);
            s.K = (int)cr(k);
            s.N = (int)(2 * cl(k));
            s.trans = 1;
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
        QIL_HIP(grant_c.ensure(ctx->device, reinterpret_cast<const void*>(&restrict_runs_lds<c64>), lds));
        hipLaunchKernelGGL(restrict_runs_lds<c64>, grid, block, lds, qil_stream(ctx), druns, dsteps, (int)half);
    } else {
        QIL_HIP(grant_r.ensure(ctx->device, reinterpret_cast<const void*>(&restrict_runs_lds<double>), lds));
        hipLaunchKernelGGL(restrict_runs_lds<double>, grid, block, lds, qil_stream(ctx), druns, dsteps, (int)half);
    }
    QIL_HIP(hipGetLastError());
    return tab.release();
}

int Restriction::launch_absorb(qil_mps* res) {
    const int64_t m = res->n();
    std::vector<AbsorbSite> tab((size_t)m);
    for (int64_t j = 0; j < m; ++j) {                           // every kept tensor starts as a copy of its parent
        const int64_t k = kept[(size_t)j];
        AbsorbSite& s = tab[(size_t)j];
        s = AbsorbSite{};
        s.C = res->site[(size_t)j];
        s.B = psi->site[(size_t)k];
        s.R = s.K = (int)cl(k);
        s.ncols = 2 * cr(k);
    }
    for (const RunPlan& r : runs) {
        AbsorbSite& s = tab[(size_t)r.kept];
        if (r.kind == kTrailing) {                              // A_k c comes from the run stage: chi_l x 2 x 1
            s.B = r.out;
            s.ncols = 2;
            continue;
        }
        s.R = r.kind == kLeading ? 1 : (int)cl(r.p);
        if (r.out) {
            s.M = r.out;
            s.ldm = s.R;
            s.off2 = 0;
        } else {
            factor(r.p, &s.M, &s.ldm, &s.off2);                 // a run of length 1, in place
        }
    }
    long long blocks = 0;
    for (AbsorbSite& s : tab) {
        s.tiles_m = (s.R + 15) / 16;
        s.block_begin = blocks;
        if (s.M) {
            const long long tiles = (long long)s.tiles_m * ((s.ncols + 15) / 16);
            blocks += (tiles + kThreads / 64 - 1) / (kThreads / 64);
        } else {
            const long long units = (long long)s.R * s.ncols * (long long)e / 16;
            blocks += std::max<long long>(1, (units + kCopyUnits - 1) / kCopyUnits);
        }
    }
    QIL_REQUIRE(blocks < (1LL << 31), QIL_EINVAL_ARG, "mps_restrict: grid too large (%lld workgroups)", blocks);
    qil_dev_table dtab(ctx);
    QIL_TRY(dtab.upload(tab.data(), tab.size() * sizeof(AbsorbSite)));
    const AbsorbSite* dsites = dtab.as<AbsorbSite>();
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (dt == QIL_C64) hipLaunchKernelGGL(restrict_absorb_grouped<c64>, grid, block, 0, qil_stream(ctx), dsites, (int)m);
    else hipLaunchKernelGGL(restrict_absorb_grouped<double>, grid, block, 0, qil_stream(ctx), dsites, (int)m);
    QIL_HIP(hipGetLastError());
    return dtab.release();
}

}  // namespace

extern "C" int qil_mps_restrict(const qil_mps* psi, const uint8_t* spec, qil_mps** out) {
    QIL_REQUIRE(psi && spec && out, QIL_EINVAL_ARG, "mps_restrict: null argument");
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int64_t n = psi->n();
    Restriction rs{psi, spec, ctx, psi->dtype, qil_elem_size(psi->dtype)};
    for (int64_t i = 0; i < n; ++i) {
        QIL_REQUIRE(spec[i] <= 3, QIL_EINVAL_CONFIG, "mps_restrict: spec value %d outside [0,3]", (int)spec[i]);
        if (spec[i] == 3) rs.kept.push_back(i);
    }
    QIL_REQUIRE(!rs.kept.empty(), QIL_EINVAL_CONFIG,
                "mps_restrict: the spec keeps no site; a number is what coefficient / marginal return");
    const int64_t m = (int64_t)rs.kept.size();
    // the maximal runs of removed sites and the kept tensor each goes into: the one on its right, the last one for a trailing run
    for (int64_t j = 0; j <= m; ++j) {
        const int64_t p = j == 0 ? 0 : rs.kept[(size_t)j - 1] + 1, q = (j == m ? n : rs.kept[(size_t)j]) - 1;
        if (q < p) continue;
        RunPlan r{};
        r.p = p;
        r.q = q;
        r.kind = j == m ? kTrailing : j == 0 ? kLeading : kInterior;
        r.kept = j == m ? m - 1 : j;
        rs.runs.push_back(r);
    }
    // whole (main_i, copy_i) pairs kept: the result is a paired chain again
    int paired = psi->paired && m % 2 == 0;
    for (int64_t j = 0; paired && j < m; j += 2)
        paired = rs.kept[(size_t)j] % 2 == 0 && rs.kept[(size_t)j + 1] == rs.kept[(size_t)j] + 1;
    std::vector<int64_t> bonds, ids;
    for (int64_t j = 0; j < m; ++j) {
        if (j + 1 < m) bonds.push_back(rs.cr(rs.kept[(size_t)j]));
        ids.push_back(psi->site_ids[(size_t)rs.kept[(size_t)j]]);
    }
    qil_mps* res = nullptr;
    QIL_TRY(qil_mps_alloc(ctx, m, psi->dtype, paired, bonds.data(), ids.data(), psi->amplitude, &res));
    qil_result_guard<qil_mps> guard(res);     // the call scope returns the temporaries; the result is a handle of its own
    std::vector<const RunPlan*> in_lds;
    for (RunPlan& r : rs.runs) {
        if (!rs.forms_product(r)) continue;
        const int64_t k = rs.kept[(size_t)r.kept];
        const int64_t elems = r.kind == kTrailing ? 2 * rs.cl(k) : (r.kind == kLeading ? 1 : rs.cl(r.p)) * rs.cr(r.q);
        QIL_TRY(rs.alloc((size_t)elems, &r.out));
        if (rs.fits_lds(r)) in_lds.push_back(&r);
    }
    QIL_TRY(rs.launch_runs_lds(in_lds));
    for (const RunPlan& r : rs.runs)
        if (rs.forms_product(r) && !rs.fits_lds(r)) QIL_TRY(rs.run_by_gemm(r));
    QIL_TRY(rs.launch_absorb(res));
    for (void* t : rs.temps) QIL_TRY(qil_ctx_free(ctx, t));
    *out = guard.release();
    return QIL_OK;
}
