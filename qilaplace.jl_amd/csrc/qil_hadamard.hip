// Element-wise MPS products and MPO adjoints for gfx950: qil_hadamard, qil_mpo_diagonal, qil_mpo_adjoint, qil_hadamard_compress.
//
// phi (.) psi has the site tensors of apply(diag(phi), psi) (qil_apply.hip), written once in the same fused layout
//     C[row, s, col],  row = alpha + chi_l * a,  col = beta + chi_r * b     (column-major)
//     C[row, s, col] = phi[a, s, b] * psi[alpha, s, beta].
// One multiply per stored element: HBM-STORE bound like the apply, so site_hadamard_grouped is organised around the store stream
// exactly as site_apply_grouped is -- one lane per output ROW (two for real results, packed into one 16-B store), so every
// wave-level store is 1 KiB contiguous; the lane's psi[alpha, :, beta-tile] in registers; the workgroup's slab of
// phi[a_lo..a_hi, :, b-chunk] (<= 16 KiB, conjugated on the way in) staged in LDS once; ALL sites in ONE grouped launch.
// Against the apply on diag(phi) it reads an operand half the size (no structural zeros) and issues one multiply where the
// apply issues a 2-term FMA chain; the products are rounded the same way, so the two routes agree element for element.
#include <algorithm>
#include <vector>

#include "qil_internal.h"
#include "qil_device_utils.h"

namespace {

using namespace qil_dev;

constexpr int kRows = 256;  // lanes per workgroup
constexpr int kTB = 8;      // beta values cached in registers per lane
constexpr int kNB = 16;     // phi right-bond values streamed per workgroup

// the products of site_apply_grouped's mad2 with the structural zero of diag(phi) dropped: fma(0, x, p * a) == p * a
__device__ __forceinline__ double mul1(double p, double a) { return p * a; }
__device__ __forceinline__ c64 mul1(c64 p, double a) { return c64{p.re * a, p.im * a}; }
__device__ __forceinline__ c64 mul1(double p, c64 a) { return c64{p * a.re, p * a.im}; }
__device__ __forceinline__ c64 mul1(c64 p, c64 a) {
    return c64{fma(-p.im, a.im, p.re * a.re), fma(p.im, a.re, p.re * a.im)};
}

template <class TP, class TA, bool CONJ>
__global__ __launch_bounds__(kRows) void site_hadamard_grouped(const ProductSite* __restrict__ sites, int nsites) {
    using TO = typename out_type<TP, TA>::type;
    constexpr int RPL = rows_per_lane<TO>::value;
    constexpr int kTileRows = kRows * RPL;
    const long long blk = blockIdx.x;
    const ProductSite S = sites[last_entry_le<&ProductSite::block_begin>(sites, nsites, blk)];   // block -> site
    long long local = blk - S.block_begin;
    // row tile fastest: concurrently resident workgroups cover whole output columns
    const int row_tile = (int)(local % S.row_tiles);
    local /= S.row_tiles;
    const int beta_tile = (int)(local % S.beta_tiles);
    const int b_chunk = (int)(local / S.beta_tiles);

    const long long R = S.R;
    const long long r_first = (long long)row_tile * kTileRows + (long long)threadIdx.x * RPL;
    const bool valid = r_first < R;
    long long rr[RPL];
    int a[RPL], alpha[RPL];
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
        rr[k] = min(r_first + k, R - 1);   // clamped: idle lanes and the odd last row stay on a real row
        a[k] = (int)(rr[k] / S.cl);
        alpha[k] = (int)(rr[k] - (long long)a[k] * S.cl);
    }
    const bool second = RPL == 2 && r_first + 1 < R;              // this lane's second row exists
    const bool packed = RPL == 2 && second && (R & 1) == 0;       // 16-B aligned pair for every column
    const int beta0 = beta_tile * kTB;
    const int nbeta = min(kTB, S.cr - beta0);
    const int b0 = b_chunk * kNB;
    const int b1 = min(b0 + kNB, S.Dr);

    const TA* __restrict__ A = static_cast<const TA*>(S.A);
    const TP* __restrict__ P = static_cast<const TP*>(S.L);
    TO* __restrict__ C = static_cast<TO*>(S.C);

    // ---- this lane's slice of psi's site: A[alpha, s, beta0 .. beta0+TB)
    TA A0[RPL][kTB], A1[RPL][kTB];
#pragma unroll
    for (int k = 0; k < RPL; ++k)
#pragma unroll
        for (int t = 0; t < kTB; ++t) {
            if (t < nbeta) {
                const long long off = alpha[k] + (long long)S.cl * (2LL * (beta0 + t));
                A0[k][t] = A[off];
                A1[k][t] = A[off + S.cl];
            } else {
                A0[k][t] = TA{};
                A1[k][t] = TA{};
            }
        }

    const long long pstride = (long long)S.Dl;  // phi[a, s, b]: a + Dl*(s + 2*b)
    // ---- stage this workgroup's slab of phi's site, phi[a_lo..a_hi, :, b0..b1), in LDS once
    constexpr int kPCap = 16384 / (int)sizeof(TP);
    __shared__ TP ptile[kPCap];
    const int a_lo = (int)(((long long)row_tile * kTileRows) / S.cl);
    const int a_hi = (int)(min((long long)row_tile * kTileRows + kTileRows - 1, R - 1) / S.cl);
    const int na = a_hi - a_lo + 1;
    const bool staged = na * 2 * (b1 - b0) <= kPCap;
    if (staged)
        for (int idx = threadIdx.x; idx < na * 2 * (b1 - b0); idx += kRows) {
            const int al = idx % na, q = (idx / na) & 1, bl = idx / (2 * na);
            const TP v = P[(a_lo + al) + pstride * (q + 2LL * (b0 + bl))];
            ptile[idx] = CONJ ? conj_t(v) : v;
        }
    __syncthreads();
    if (!valid) return;
    for (int b = b0; b < b1; ++b) {
        TP p0[RPL], p1[RPL];
#pragma unroll
        for (int k = 0; k < RPL; ++k) {
            if (staged) {
                const TP* pl = ptile + (a[k] - a_lo) + na * 2 * (b - b0);
                p0[k] = pl[0];
                p1[k] = pl[na];
            } else {
                const TP* pp = P + a[k] + pstride * (2LL * b);
                p0[k] = CONJ ? conj_t(pp[0]) : pp[0];
                p1[k] = CONJ ? conj_t(pp[pstride]) : pp[pstride];
            }
        }
        TO* cp = C + r_first + R * (2LL * ((long long)beta0 + (long long)S.cr * b));
#pragma unroll
        for (int t = 0; t < kTB; ++t) {
            if (nbeta == kTB || t < nbeta) {
                const TO v0 = mul1(p0[0], A0[0][t]);
                const TO v1 = mul1(p1[0], A1[0][t]);
                if constexpr (RPL == 2) {
                    const TO u0 = mul1(p0[1], A0[1][t]);
                    const TO u1 = mul1(p1[1], A1[1][t]);
                    if (packed) {
                        store_pair(cp, v0, u0);
                        store_pair(cp + R, v1, u1);
                    } else {
                        store_out<true>(cp, v0);
                        store_out<true>(cp + R, v1);
                        if (second) {
                            store_out<true>(cp + 1, u0);
                            store_out<true>(cp + R + 1, u1);
                        }
                    }
                } else {
                    store_out<true>(cp, v0);
                    store_out<true>(cp + R, v1);
                }
            }
            cp += 2 * R;
        }
    }
}

// ---- diag(phi) and W^dagger: moves and sign flips of small tensors, one launch for the chain, one thread per output element
struct MoveSite {
    const void* src;
    void* dst;
    int Dl, Dr;
    double scale;          // diag: the amplitude on the first tensor, 1 elsewhere
    long long elem_begin;  // first output element of this site in the flattened chain
};

// ADJ = false: W[a, s', s, b] = delta_{s s'} scale (conj?) phi[a, s, b];  ADJ = true: out[a, s', s, b] = conj(W[a, s, s', b])
template <class T, bool ADJ>
__global__ void chain_move_sites(const MoveSite* __restrict__ sites, int nsites, long long total, int conj) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        // element -> site, spelled out: inside this grid-stride loop qil_dev::last_entry_le is scheduled differently, and the
        // kernels of this file keep the instruction streams they were measured with
        int lo = 0, hi = nsites - 1;
        while (lo < hi) {
            int mid = (lo + hi + 1) >> 1;
            if (sites[mid].elem_begin <= idx) lo = mid; else hi = mid - 1;
        }
        const MoveSite S = sites[lo];
        long long t = idx - S.elem_begin;      // a + Dl*(si + 2*(so + 2*b))
        const int a = (int)(t % S.Dl);
        t /= S.Dl;
        const int si = (int)(t & 1), so = (int)((t >> 1) & 1);
        const long long b = t >> 2;
        const T* src = static_cast<const T*>(S.src);
        T v;
        if (ADJ) {
            v = conj_t(src[a + (long long)S.Dl * (so + 2 * (si + 2 * b))]);
        } else if (si == so) {
            v = src[a + (long long)S.Dl * (si + 2 * b)];
            if (conj) v = conj_t(v);
            v = scale_t(v, S.scale);
        } else {
            v = T{};
        }
        static_cast<T*>(S.dst)[idx - S.elem_begin] = v;
    }
}

// phi against psi: the operand checks of qil_inner under this verb's name
int check_pair(const char* verb, const qil_mps* phi, const qil_mps* psi) {
    QIL_REQUIRE(phi->ctx == psi->ctx, QIL_EINVAL_ARG, "%s: MPS belong to different contexts", verb);
    QIL_REQUIRE(phi->paired == psi->paired, QIL_EINVAL_ARG, "%s: cannot mix paired and single-register operands", verb);
    QIL_REQUIRE(phi->n() == psi->n(), QIL_EINVAL_LENGTH,
                "%s: MPS must have the same number of sites. Found length(phi)=%lld, length(psi)=%lld", verb,
                (long long)phi->n(), (long long)psi->n());
    QIL_REQUIRE(phi->site_ids == psi->site_ids, QIL_EINVAL_SITES, "%s: MPS must have the same site indices.", verb);
    return QIL_OK;
}

int launch_hadamard(const qil_mps* phi, int conj_phi, const qil_mps* psi, qil_mps* out) {
    qil_context* ctx = psi->ctx;
    const int64_t n = psi->n();
    // real x real results pack two rows per lane (16-B stores): 512-row tiles
    const int tile_rows = (phi->dtype == QIL_F64 && psi->dtype == QIL_F64) ? 2 * kRows : kRows;
    std::vector<ProductSite> tab;
    const long long blocks = qil_product_sites(phi, psi, out, tile_rows, kTB, kNB, tab);
    QIL_REQUIRE(blocks < (1LL << 31), QIL_EINVAL_ARG, "hadamard: grid too large (%lld workgroups)", blocks);
    qil_dev_table dev(ctx);
    QIL_TRY(dev.upload(tab.data(), tab.size() * sizeof(ProductSite)));
    QIL_TRY(qil_ctx_prof_begin(ctx));
    const ProductSite* dtab = dev.as<ProductSite>();
    const dim3 grid((unsigned)blocks), block(kRows);
    const bool pc = phi->dtype == QIL_C64, ac = psi->dtype == QIL_C64;
#define QIL_HADAMARD_LAUNCH(TP, TA, CJ) \
    hipLaunchKernelGGL((site_hadamard_grouped<TP, TA, CJ>), grid, block, 0, qil_stream(ctx), dtab, (int)n)
    if (pc && ac) {
        if (conj_phi) QIL_HADAMARD_LAUNCH(c64, c64, true); else QIL_HADAMARD_LAUNCH(c64, c64, false);
    } else if (pc) {
        if (conj_phi) QIL_HADAMARD_LAUNCH(c64, double, true); else QIL_HADAMARD_LAUNCH(c64, double, false);
    } else if (ac) {
        QIL_HADAMARD_LAUNCH(double, c64, false);
    } else {
        QIL_HADAMARD_LAUNCH(double, double, false);
    }
#undef QIL_HADAMARD_LAUNCH
    QIL_HIP(hipGetLastError());
    QIL_TRY(qil_ctx_prof_end(ctx));
    return dev.release();
}

// one launch of chain_move_sites over the whole chain: src (MPS for the diagonal, MPO for the adjoint) -> the MPO dst
int launch_move(const qil_chain* src, qil_mpo* dst, bool adjoint, int conj, double scale) {
    qil_context* ctx = src->ctx;
    const int64_t n = src->n();
    std::vector<MoveSite> tab((size_t)n);
    long long total = 0;
    for (int64_t i = 0; i < n; ++i) {
        MoveSite& s = tab[(size_t)i];
        s.src = src->site[(size_t)i];
        s.dst = dst->site[(size_t)i];
        s.Dl = (int)src->dims[(size_t)i];
        s.Dr = (int)src->dims[(size_t)i + 1];
        s.scale = i == 0 ? scale : 1.0;
        s.elem_begin = total;
        total += dst->site_elems(i);
    }
    qil_dev_table dev(ctx);
    QIL_TRY(dev.upload(tab.data(), tab.size() * sizeof(MoveSite)));
    const MoveSite* dtab = dev.as<MoveSite>();
    const long long want = (total + 255) / 256;
    const dim3 grid((unsigned)std::min<long long>(want, 64LL * ctx->num_cus)), block(256);
    const bool cx = src->dtype == QIL_C64;
#define QIL_MOVE_LAUNCH(T, ADJ) \
    hipLaunchKernelGGL((chain_move_sites<T, ADJ>), grid, block, 0, qil_stream(ctx), dtab, (int)n, total, conj)
    if (adjoint) {
        if (cx) QIL_MOVE_LAUNCH(c64, true); else QIL_MOVE_LAUNCH(double, true);
    } else {
        if (cx) QIL_MOVE_LAUNCH(c64, false); else QIL_MOVE_LAUNCH(double, false);
    }
#undef QIL_MOVE_LAUNCH
    QIL_HIP(hipGetLastError());
    return dev.release();
}

// diag(phi) as a new MPO handle (the caller has activated the context and opened its call scope)
int make_diagonal(const qil_mps* phi, int conj_phi, qil_mpo** out) {
    qil_mpo* D = nullptr;
    QIL_TRY(qil_mpo_alloc(phi->ctx, phi->n(), phi->dtype, phi->paired, phi->dims.data() + 1, phi->site_ids.data(), &D));
    qil_result_guard<qil_mpo> guard(D);
    QIL_TRY(launch_move(phi, D, false, conj_phi, phi->amplitude));
    *out = guard.release();
    return QIL_OK;
}

}  // namespace

int qil_check_pair(const char* verb, const qil_mps* phi, const qil_mps* psi) { return check_pair(verb, phi, psi); }

extern "C" int qil_hadamard(const qil_mps* phi, int conj_phi, const qil_mps* psi, qil_mps** out) {
    QIL_REQUIRE(phi && psi && out, QIL_EINVAL_ARG, "hadamard: null argument");
    QIL_TRY(check_pair("hadamard", phi, psi));
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    const int64_t n = psi->n();
    std::vector<int64_t> bonds((size_t)(n > 1 ? n - 1 : 0));
    for (int64_t i = 0; i + 1 < n; ++i) bonds[(size_t)i] = phi->dims[(size_t)i + 1] * psi->dims[(size_t)i + 1];
    const int odt = (phi->dtype == QIL_C64 || psi->dtype == QIL_C64) ? QIL_C64 : QIL_F64;
    qil_mps* res = nullptr;
    QIL_TRY(qil_mps_alloc(ctx, n, odt, psi->paired, bonds.data(), psi->site_ids.data(), phi->amplitude * psi->amplitude, &res));
    qil_result_guard<qil_mps> guard(res);
    QIL_TRY(launch_hadamard(phi, conj_phi, psi, res));
    *out = guard.release();
    return QIL_OK;
}

extern "C" int qil_mpo_diagonal(const qil_mps* phi, int conj_phi, qil_mpo** out) {
    QIL_REQUIRE(phi && out, QIL_EINVAL_ARG, "mpo_diagonal: null argument");
    QIL_TRY(qil_ctx_activate(phi->ctx));
    qil_call_scope call_scope(phi->ctx);
    return make_diagonal(phi, conj_phi, out);
}

extern "C" int qil_mpo_adjoint(const qil_mpo* W, qil_mpo** out) {
    QIL_REQUIRE(W && out, QIL_EINVAL_ARG, "mpo_adjoint: null argument");
    QIL_TRY(qil_ctx_activate(W->ctx));
    qil_call_scope call_scope(W->ctx);
    qil_mpo* res = nullptr;
    QIL_TRY(qil_mpo_alloc(W->ctx, W->n(), W->dtype, W->paired, W->dims.data() + 1, W->site_ids.data(), &res));
    qil_result_guard<qil_mpo> guard(res);
    QIL_TRY(launch_move(W, res, true, 1, 1.0));
    *out = guard.release();
    return QIL_OK;
}

// compress!(phi (.) psi) = qil_apply_compress on the temporary diag(phi): the zip-up and the variational sweep read the
// operator's Dl x 2 x 2 x Dr tensors, and a diagonal one is what turns them into an element-wise product
extern "C" int qil_hadamard_compress(const qil_mps* phi, int conj_phi, const qil_mps* psi, int64_t maxdim, double tol, int sweeps,
                                     int64_t zip_maxdim, qil_mps** out) {
    QIL_REQUIRE(phi && psi && out, QIL_EINVAL_ARG, "hadamard_compress: null argument");
    QIL_TRY(check_pair("hadamard_compress", phi, psi));
    qil_context* ctx = psi->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_mpo* D = nullptr;
    QIL_TRY(make_diagonal(phi, conj_phi, &D));
    const int st = qil_apply_compress(D, psi, maxdim, tol, sweeps, zip_maxdim, out);
    qil_mpo_destroy(D);
    return st;
}
