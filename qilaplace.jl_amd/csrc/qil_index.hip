// Read-out by index, device to device: qil_coefficient_at, and the sampler of qil_mps_map (qil_map.hip).
//
//   out[j] = amplitude * prod_i A_i[:, bit_i(idx[j]), :],   bit_i(x) = (x >> (n - i)) & 1, tensor 1 the most significant bit
//
// The indices are int64 in HBM and the values go to HBM: nothing of a call crosses the host.  Two routes:
//   wave   index_wave: ONE WAVE owns one index and walks all sites, several waves per workgroup.  The carry vector lives in
//          LDS private to its wave, double buffered; a site is v'[beta] = sum_alpha v[alpha] A[alpha, bit, beta] with groups of
//          G lanes over alpha (A is read along its contiguous leg) and a shuffle reduction, as in coefficient_chain
//          (qil_readout.hip).  The waves of a workgroup never meet: no workgroup barrier, no global scratch.  The same kernel
//          reads up to four states at one index and applies an element-wise function to the values in its epilogue, with the
//          count on the device (the CrossState::cnt pattern of cross_gather_k): the grid is launched for an upper bound.
//   bits   chains with a bond above QIL_COEFFICIENT_AT_WAVE_MAX_BOND: the indices are expanded to the uint8 bit table of
//          the read-outs by bit (index_bits) and go through qil_coefficient_enqueue_select (CHAIN / GEMM_SELECT of
//          qil_readout.hip, both on device bits, no host plan); index_finish converts and marks the rows out of range.
// An index outside [0, 2^n) gives NaN on both routes.  QIL_COEFFICIENT_AT_ROUTE=wave|bits (read per call) forces a route;
// wave only where the carry fits the LDS (bond <= kWaveFitBond).
#include "qil_internal.h"
#include "qil_launch.h"
#include "qil_device_utils.h"

#include <cmath>
#include <cstdlib>

namespace {

using namespace qil_dev;

constexpr int kAtWaves = 4;                 // waves (= indices in flight) per workgroup
constexpr int kAtThreads = 64 * kAtWaves;
constexpr int kWaveFitBond = 1024;          // kAtWaves * 2 * 1024 * 16 B = 128 KiB of the CU's 160 KiB
static_assert(QIL_COEFFICIENT_AT_WAVE_MAX_BOND <= kWaveFitBond, "the auto route must fit the LDS");
static_assert((size_t)kAtWaves * 2 * kWaveFitBond * 16 <= 160 * 1024, "the carry vectors fit the LDS");
constexpr int64_t kBitsPass = 1 << 16;      // indices per pass of the bits route (bounds the GEMM form's rows)

struct AtSite {
    const void* A;   // [cl, 2, cr], alpha fastest
    int cl, cr;
    int cx;          // the site holds c64
    int pad;
};

struct AtArgs {
    const AtSite* sites;       // [nstates][n]
    const long long* idx;
    const int* cnt;            // device count, or null: `count`
    long long count;
    void* out;
    double amp[QIL_MAP_MAX_STATES];
    double param;
    int n, nstates, maxchi, op;   // op < 0: the value of state 0 itself
};

template <class T>
__device__ __forceinline__ T load_site(const AtSite& S, long long off);
template <>
__device__ __forceinline__ double load_site<double>(const AtSite& S, long long off) {
    return static_cast<const double*>(S.A)[off];
}
template <>
__device__ __forceinline__ c64 load_site<c64>(const AtSite& S, long long off) {
    if (S.cx) return static_cast<const c64*>(S.A)[off];
    return c64{static_cast<const double*>(S.A)[off], 0.0};
}

// what one lane wrote to the wave's LDS is read by the others: order the accesses, for the compiler and the LDS queue
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double abs_elem(double v) { return fabs(v); }
__device__ __forceinline__ double abs_elem(c64 v) { return hypot(v.re, v.im); }
__device__ __forceinline__ bool finite_elem(double v) { return isfinite(v); }
__device__ __forceinline__ bool finite_elem(c64 v) { return isfinite(v.re) && isfinite(v.im); }

// the element-wise functions of qil_mps_map; a (and b) carry their amplitudes
template <class T>
__device__ __forceinline__ double map_real(int op, double param, T a) {
    const double m = abs_elem(a);
    if (op == QIL_MAP_ABS) return m;
    if (op == QIL_MAP_POWER) return pow(m, param);
    return log(abs2_t(a) + param);                         // QIL_MAP_LOG
}
template <class T>
__device__ __forceinline__ T map_same(int op, double param, T a, T b) {
    if (op == QIL_MAP_SHRINK) {
        const double m = abs_elem(a);
        return m > 0.0 ? scale_t(a, fmax(0.0, 1.0 - param / m)) : a;
    }
    // QIL_MAP_DIVIDE: a conj(b) / (|b|^2 + lambda)
    const T num = cmul_add(T{}, a, conj_t(b));
    T v = scale_t(num, 1.0 / (abs2_t(b) + param));
    // 0 / 0 is NaN, which the session's largest-|value| search would pass over: every non-finite quotient reads as infinite
    if (!finite_elem(v)) v = make_elem(INFINITY, 0.0, static_cast<T*>(nullptr));
    return v;
}

template <class T, bool RealOut>
__device__ __forceinline__ void index_wave_body(const uint3 blockIdx, const uint3 gridDim, AtArgs P) {
    extern __shared__ __attribute__((aligned(16))) char at_smem[];
    using TO = typename std::conditional<RealOut, double, T>::type;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long total = P.cnt ? (long long)*P.cnt : P.count;
    T* buf = reinterpret_cast<T*>(at_smem) + (size_t)wave * 2 * P.maxchi;
    const int n = P.n;
    for (long long q = (long long)blockIdx.x * kAtWaves + wave; q < total; q += (long long)gridDim.x * kAtWaves) {
        const long long j = P.idx[q];
        TO* out = static_cast<TO*>(P.out);
        if (j < 0 || (j >> n) != 0) {                      // n <= 62: outside [0, 2^n)
            if (lane == 0) out[q] = make_elem(NAN, NAN, static_cast<TO*>(nullptr));
            continue;
        }
        T val[QIL_MAP_MAX_STATES];
        for (int s = 0; s < P.nstates; ++s) {
            T* v_in = buf;
            T* v_out = buf + P.maxchi;
            if (lane == 0) v_in[0] = cast_elem<T>(1.0);
            wave_lds_sync();
            for (int i = 0; i < n; ++i) {
                const AtSite S = P.sites[s * n + i];
                const int bit = (int)((j >> (n - 1 - i)) & 1);
                int G = 64;  // lanes per dot product: smallest power of two >= cl (cap 64)
                while (G > 1 && (G >> 1) >= S.cl) G >>= 1;
                const int per_wave = 64 / G;
                const int grp = lane / G, gl = lane - grp * G;
                for (int beta = grp; beta < S.cr; beta += per_wave) {
                    const long long col = (long long)S.cl * (bit + 2LL * beta);
                    T acc{};
                    for (int al = gl; al < S.cl; al += G) acc = cmul_add(acc, v_in[al], load_site<T>(S, col + al));
                    for (int m = G >> 1; m >= 1; m >>= 1) acc = add_t(acc, shfl_xor_t(acc, m));
                    if (gl == 0) v_out[beta] = acc;
                }
                wave_lds_sync();
                T* t = v_in;
                v_in = v_out;
                v_out = t;
            }
            val[s] = scale_t(v_in[0], P.amp[s]);
            wave_lds_sync();                               // every lane has read it before lane 0 starts the next state
        }
        if (lane != 0) continue;
        if (P.op < 0) {
            if constexpr (!RealOut) out[q] = val[0];
        } else if (P.op <= QIL_MAP_LOG) {
            if constexpr (RealOut || sizeof(T) == 8) static_cast<double*>(P.out)[q] = map_real(P.op, P.param, val[0]);
        } else {
            if constexpr (!RealOut) out[q] = map_same(P.op, P.param, val[0], P.nstates > 1 ? val[1] : val[0]);
        }
    }
}
template <class T, bool RealOut>
struct index_wave_k {
    static constexpr int NT = kAtThreads, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        index_wave_body<T, RealOut>(b, g, a...);
    }
};

// bits[q, i] = bit_i(idx[q]); a row out of range reads as index 0 here and is marked by index_finish
__device__ __forceinline__ void index_bits_body(const uint3 blockIdx, const uint3 gridDim, const long long* __restrict__ idx,
                                                long long count, int n, uint8_t* __restrict__ bits) {
    const long long total = count * n;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += gridDim.x * 256LL) {
        const long long q = t / n;
        const int i = (int)(t - q * n);
        long long j = idx[q];
        if (j < 0 || (j >> n) != 0) j = 0;
        bits[t] = (uint8_t)((j >> (n - 1 - i)) & 1);
    }
}
struct index_bits_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        index_bits_body(b, g, a...);
    }
};
template <class T>
__device__ __forceinline__ void index_finish_body(const uint3 blockIdx, const uint3 gridDim, const long long* __restrict__ idx,
                                                  long long count, int n, const c64* __restrict__ vals, T* __restrict__ out) {
    for (long long q = blockIdx.x * 256LL + threadIdx.x; q < count; q += gridDim.x * 256LL) {
        const long long j = idx[q];
        const c64 v = vals[q];
        out[q] = (j < 0 || (j >> n) != 0) ? make_elem(NAN, NAN, static_cast<T*>(nullptr)) : make_elem(v.re, v.im, static_cast<T*>(nullptr));
    }
}
template <class T>
struct index_finish_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        index_finish_body<T>(b, g, a...);
    }
};

// The route of a call: THE decision, which tests mirror through coefficient_at_route (ops.py)
bool at_route_wave(const qil_mps* psi) {
    const long long maxchi = *std::max_element(psi->dims.begin(), psi->dims.end());
    const char* route = getenv("QIL_COEFFICIENT_AT_ROUTE");
    if (route && !strcmp(route, "bits")) return false;
    if (route && !strcmp(route, "wave")) return maxchi <= kWaveFitBond;
    return maxchi <= QIL_COEFFICIENT_AT_WAVE_MAX_BOND;
}

int at_bits_route(qil_context* ctx, const qil_mps* psi, int64_t count, const long long* idx, void* out) {
    const int64_t n = psi->n();
    const int64_t pass = std::min<int64_t>(count, kBitsPass);
    qil_scratch tmp(ctx);
    void *bits = nullptr, *vals = nullptr;
    QIL_TRY(tmp.alloc((size_t)(pass * n), &bits));
    QIL_TRY(tmp.alloc((size_t)pass * 16, &vals));
    const size_t e = qil_elem_size(psi->dtype);
    for (int64_t q0 = 0; q0 < count; q0 += pass) {
        const int64_t nq = std::min<int64_t>(pass, count - q0);
        QIL_TRY((qil_klaunch<index_bits_k>(ctx, dim3(qil_grid_for(nq * n, 65536)), dim3(256), 0, idx + q0, (long long)nq, (int)n,
                                           static_cast<uint8_t*>(bits))));
        QIL_TRY(qil_coefficient_enqueue_select(psi, nq, static_cast<const uint8_t*>(bits), vals));
        QIL_TRY(for_elem_type(psi->dtype == QIL_C64, [&](auto t) {
            using T = decltype(t);
            return qil_klaunch<index_finish_k<T>>(ctx, dim3(qil_grid_for(nq)), dim3(256), 0, idx + q0, (long long)nq, (int)n,
                                                  static_cast<const c64*>(vals), reinterpret_cast<T*>(static_cast<char*>(out) + (size_t)q0 * e));
        }));
    }
    return QIL_OK;
}

}  // namespace

int qil_index_reader_begin(qil_scratch& tmp, const qil_mps* const* states, int nstates, qil_index_reader* r) {
    const int64_t n = states[0]->n();
    std::vector<AtSite> tab((size_t)(nstates * n));
    r->n = (int)n, r->nstates = nstates, r->maxchi = 1, r->cx = false;
    for (int s = 0; s < nstates; ++s) {
        const qil_mps* psi = states[s];
        r->cx = r->cx || psi->dtype == QIL_C64;
        r->amp[s] = psi->amplitude;
        for (int64_t i = 0; i < n; ++i) {
            tab[(size_t)(s * n + i)] = AtSite{psi->site[(size_t)i], (int)psi->dims[(size_t)i], (int)psi->dims[(size_t)i + 1],
                                              psi->dtype == QIL_C64 ? 1 : 0, 0};
            r->maxchi = std::max<int>(r->maxchi, (int)psi->dims[(size_t)i + 1]);
        }
    }
    QIL_REQUIRE(r->maxchi <= kWaveFitBond, QIL_EINVAL_ARG, "index read-out: bond %d above %d does not fit the LDS", r->maxchi, kWaveFitBond);
    void* p = nullptr;
    QIL_TRY(qil_upload_bytes(tmp, tab.data(), tab.size() * sizeof(AtSite), &p));
    r->tab = p;
    return QIL_OK;
}

int qil_index_reader_enqueue(qil_context* ctx, const qil_index_reader& r, int op, double param, const long long* idx,
                             const int* cnt_dev, int64_t bound, void* out) {
    AtArgs P;
    P.sites = static_cast<const AtSite*>(r.tab);
    P.idx = idx;
    P.cnt = cnt_dev;
    P.count = bound;
    P.out = out;
    for (int s = 0; s < QIL_MAP_MAX_STATES; ++s) P.amp[s] = s < r.nstates ? r.amp[s] : 0.0;
    P.param = param;
    P.n = r.n, P.nstates = r.nstates, P.maxchi = r.maxchi, P.op = op;
    const size_t lds = (size_t)kAtWaves * 2 * (size_t)r.maxchi * (r.cx ? 16 : 8);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((bound + kAtWaves - 1) / kAtWaves, 65536)));
    const bool real_out = op >= QIL_MAP_ABS && op <= QIL_MAP_LOG;
    if (!r.cx) return qil_klaunch<index_wave_k<double, false>>(ctx, grid, dim3(kAtThreads), lds, P);
    if (real_out) return qil_klaunch<index_wave_k<c64, true>>(ctx, grid, dim3(kAtThreads), lds, P);
    return qil_klaunch<index_wave_k<c64, false>>(ctx, grid, dim3(kAtThreads), lds, P);
}

extern "C" int qil_coefficient_at(const qil_mps* psi, int64_t count, const int64_t* idx_dev, void* out_dev) {
    QIL_REQUIRE(psi && (count <= 0 || (idx_dev && out_dev)), QIL_EINVAL_ARG, "coefficient_at: null argument");
    QIL_REQUIRE(count >= 0, QIL_EINVAL_ARG, "coefficient_at: count = %lld must be >= 0", (long long)count);
    QIL_REQUIRE(psi->n() >= 1 && psi->n() <= 62, QIL_EINVAL_ARG, "coefficient_at: %lld tensors outside 1 .. 62", (long long)psi->n());
    if (count == 0) return QIL_OK;
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    const long long* idx = reinterpret_cast<const long long*>(idx_dev);
    if (at_route_wave(psi)) {
        qil_index_reader r;
        QIL_TRY(qil_index_reader_begin(tmp, &psi, 1, &r));
        QIL_TRY(qil_index_reader_enqueue(ctx, r, -1, 0.0, idx, nullptr, count, out_dev));
    } else {
        QIL_TRY(at_bits_route(ctx, psi, count, idx, out_dev));
    }
    QIL_HIP(qil_stream_sync(ctx));
    return QIL_OK;
}
