// The host-side steps the overlap and Born-weight verbs share (qil_inner, qil_readout, qil_weight, qil_apply_weight, qil_sample):
//   qil_dev_fill_ones    1 into count elements, `stride` apart: the left boundary [1] of an environment, the start of a batch of rows
//   qil_put_mps_site /   a site in the contraction dtype and in the layout a product reads (qil_site_layout); qil_site_operand
//   qil_put_mpo_site     returns the site itself where it already has that dtype
//   qil_norm_env_ket /   the four-product environment step of |W psi|^2, E' = A^H ((E A) W) conj(Wr), on nslots packed environments
//   qil_norm_env_bra
//   qil_overlap_env_step /        the environment steps of <phi|psi> and <phi|W psi> (qil_inner, qil_apply_inner, qil_environment):
//   qil_apply_overlap_env_step    two and three products per site
//   qil_upload_bytes    caller memory into a block of the call's qil_scratch
//   qil_download         device memory to the caller, complete when it returns
// Declared in qil_internal.h.  The f64 MFMA tile step and the small type helpers of the kernels are in qil_device_utils.h.
#include "qil_internal.h"
#include "qil_launch.h"
#include "qil_device_utils.h"

namespace {

using namespace qil_dev;

// in the table form of qil_launch.h: the starts of the read-outs of a lock-step batch are ONE launch
template <class T>
__device__ __forceinline__ void fill_ones_body(const uint3 blockIdx, const uint3 gridDim, T* __restrict__ p, long long count, long long stride) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < count; t += (long long)gridDim.x * blockDim.x)
        p[t * stride] = cast_elem<T>(1.0);
}
template <class T>
struct fill_ones_k {
    static constexpr int NT = 256, MINW = 1;
    template <class... QA>
    static __device__ __forceinline__ void run(const uint3 b, const uint3 g, QA... a) {
        fill_ones_body<T>(b, g, a...);
    }
};

// A[s, sigma, beta] -> Ap (cast to TD): QIL_SITE_PLAIN as it lies (a widened copy), QIL_SITE_REVERSED Ap[beta, sigma, s]
template <class TS, class TD>
__global__ void put_mps_site(const TS* __restrict__ A, TD* __restrict__ Ap, int cl, int cr, int layout) {
    const long long total = 2LL * cl * cr;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        long long src = t;
        if (layout == QIL_SITE_REVERSED) {
            const long long be = t % cr, u = t / cr;
            src = (u >> 1) + (long long)cl * ((u & 1) + 2 * be);
        }
        Ap[t] = cast_elem<TD>(A[src]);
    }
}
// W[a, s_in, s_out, b] -> Wp (cast to TD):
//   QIL_SITE_PLAIN         as it lies                       the ket operand of T2
//   QIL_SITE_SWAPPED       Wp[a, s_out, s_in, b]            the bra operand of T3: it contracts (a', s_out), which are then adjacent
//   QIL_SITE_REVERSED      Wp[b, s_in, s_out, a]            the ket operand of the mirrored pass
//   QIL_SITE_REV_SWAPPED   Wp[b, s_out, s_in, a]            the bra operand of the mirrored pass
//   QIL_SITE_BIT_MAJOR     Wp[a, s_in, b, s_out]            each output-bit slice is one contiguous (D_l x 2 D_r) operand
template <class TS, class TD>
__global__ void put_mpo_site(const TS* __restrict__ W, TD* __restrict__ Wp, int Dl, int Dr, int layout) {
    const long long total = 4LL * Dl * Dr;
    const bool mirrored = layout == QIL_SITE_REVERSED || layout == QIL_SITE_REV_SWAPPED;
    const int d0 = mirrored ? Dr : Dl;               // the fastest index of the target
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        long long src = t;
        if (layout == QIL_SITE_BIT_MAJOR) {
            const long long a = t % Dl, u = t / Dl, v = u >> 1;
            src = a + (long long)Dl * ((u & 1) + 2 * (v / Dr + 2 * (v % Dr)));
        } else if (layout != QIL_SITE_PLAIN) {
            const long long x = t % d0, u = t / d0, y = u >> 2;
            const int p = (int)(u & 1), q = (int)((u >> 1) & 1);
            const long long a = mirrored ? y : x, b = mirrored ? x : y;
            const bool swapped = layout == QIL_SITE_SWAPPED || layout == QIL_SITE_REV_SWAPPED;
            src = a + (long long)Dl * ((swapped ? q : p) + 2 * ((swapped ? p : q) + 2 * b));
        }
        Wp[t] = cast_elem<TD>(W[src]);
    }
}

// the one dtype switch of the site kernels: go(source element, target element)
template <class F>
void for_site_dtypes(int dt, int src_dt, F go) {
    if (dt == QIL_F64) go(double{}, double{});
    else if (src_dt == QIL_C64) go(c64{}, c64{});
    else go(double{}, c64{});
}

}  // namespace

int qil_dev_fill_ones(qil_context* ctx, int dt, void* p, int64_t count, int64_t stride) {
    return for_elem_type(dt == QIL_C64, [&](auto t) {
        using T = decltype(t);
        return qil_klaunch<fill_ones_k<T>>(ctx, dim3(qil_grid_for(count, 65536)), dim3(256), 0, (T*)p, (long long)count, (long long)stride);
    });
}

int qil_put_mps_site(qil_context* ctx, int dt, const qil_mps* psi, int64_t i, int layout, void* dst) {
    const int cl = (int)psi->dims[(size_t)i], cr = (int)psi->dims[(size_t)i + 1];
    for_site_dtypes(dt, psi->dtype, [&](auto s, auto d) {
        hipLaunchKernelGGL((put_mps_site<decltype(s), decltype(d)>), dim3(qil_grid_for(2LL * cl * cr)), dim3(256), 0, qil_stream(ctx),
                           (const decltype(s)*)psi->site[(size_t)i], (decltype(d)*)dst, cl, cr, layout);
    });
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

int qil_put_mpo_site(qil_context* ctx, int dt, const qil_mpo* W, int64_t i, int layout, void* dst) {
    const int Dl = (int)W->dims[(size_t)i], Dr = (int)W->dims[(size_t)i + 1];
    for_site_dtypes(dt, W->dtype, [&](auto s, auto d) {
        hipLaunchKernelGGL((put_mpo_site<decltype(s), decltype(d)>), dim3(qil_grid_for(4LL * Dl * Dr)), dim3(256), 0, qil_stream(ctx),
                           (const decltype(s)*)W->site[(size_t)i], (decltype(d)*)dst, Dl, Dr, layout);
    });
    QIL_HIP(hipGetLastError());
    return QIL_OK;
}

int qil_site_operand(qil_context* ctx, int dt, const qil_chain* c, int64_t i, void* buf, const void** use) {
    *use = c->site[(size_t)i];
    if (c->dtype == dt) return QIL_OK;
    *use = buf;
    if (c->phys_rank == 1) return qil_put_mps_site(ctx, dt, static_cast<const qil_mps*>(c), i, QIL_SITE_PLAIN, buf);
    return qil_put_mpo_site(ctx, dt, static_cast<const qil_mpo*>(c), i, QIL_SITE_PLAIN, buf);
}

// Per slot (blocks packed per site: slot j's block at j * the block size of the product's operand):
//   T1[s', a', a, s_in, beta]   = E A                        in -> s1      batch = slot
//   T2[s', a', s_out, b, beta]  = T1_beta W                  s1 -> s2      batch = (beta, slot)
int qil_norm_env_ket(qil_context* ctx, int dt, int64_t cl, int64_t cr, int64_t Dl, int64_t Dr, int64_t nslots, const void* As,
                     const void* Wd, const void* in, void* s1, void* s2) {
    const int64_t rE = cl * Dl * Dl;
    qil_gemm_batch b1, b2;
    b1.count = nslots, b1.a_bs = rE * cl, b1.c_bs = rE * 2 * cr;
    b2.count = nslots * cr, b2.a_bs = rE * 2, b2.c_bs = cl * Dl * 2 * Dr;
    QIL_TRY(qil_dev_gemm_batched(ctx, dt, 0, 0, rE, 2 * cr, cl, in, rE, As, cl, s1, rE, &b1));
    return qil_dev_gemm_batched(ctx, dt, 0, 0, cl * Dl, 2 * Dr, 2 * Dl, s1, cl * Dl, Wd, 2 * Dl, s2, cl * Dl, &b2);
}
//   T3[s', s_in', b', b, beta]  = T2_(b, beta) conj(Wr)      s2 -> s1      batch = (b, beta, slot)
//   E'[beta', b', b, beta]      = A^H T3                     s1 -> out     the slots' blocks are the columns of ONE product
int qil_norm_env_bra(qil_context* ctx, int dt, int64_t cl, int64_t cr, int64_t Dl, int64_t Dr, int64_t nslots, const void* As,
                     const void* Wr, const void* s2, void* s1, void* out) {
    qil_gemm_batch b3;
    b3.count = nslots * Dr * cr, b3.a_bs = cl * 2 * Dl, b3.c_bs = cl * 2 * Dr;
    QIL_TRY(qil_dev_gemm_batched(ctx, dt, 0, 3, cl, 2 * Dr, 2 * Dl, s2, cl, Wr, 2 * Dl, s1, cl, &b3));
    return qil_dev_gemm(ctx, dt, 2, 0, cr, nslots * Dr * Dr * cr, 2 * cl, As, 2 * cl, s1, 2 * cl, out, cr);
}

//   T[p, s, b]  = E A_psi,   E'[q, b] = A_phi^H T        (ph physical slices: 2 for states, 4 for operators)
int qil_overlap_env_step(qil_context* ctx, int dt, int64_t ph, int64_t pl, int64_t pr, int64_t sl, int64_t sr, const void* Ap,
                         const void* As, const void* E, void* T, void* En) {
    // T (pl x ph sr) = E (pl x sl) * A_psi (sl x ph sr):  T[p, s, b]
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, pl, ph * sr, sl, E, pl, As, sl, T, pl));
    // E' (pr x sr) = A_phi^H ((ph pl) x pr)^H * T ((ph pl) x sr)
    return qil_dev_gemm(ctx, dt, 2, 0, pr, sr, ph * pl, Ap, ph * pl, T, ph * pl, En, pr);
}
//   T1[p, a, s_in, beta] = E A_psi,   T2[p, s_out, b, beta] = T1_beta W (batch = beta),   E'[q, b, beta] = A_phi^H T2
int qil_apply_overlap_env_step(qil_context* ctx, int dt, int64_t pl, int64_t pr, int64_t sl, int64_t sr, int64_t Dl, int64_t Dr,
                               const void* Ap, const void* As, const void* Wd, const void* E, void* T1, void* T2, void* En) {
    QIL_TRY(qil_dev_gemm(ctx, dt, 0, 0, pl * Dl, 2 * sr, sl, E, pl * Dl, As, sl, T1, pl * Dl));
    qil_gemm_batch bt;                             // batch = beta
    bt.count = sr, bt.a_bs = pl * 2 * Dl, bt.c_bs = pl * 2 * Dr;
    QIL_TRY(qil_dev_gemm_batched(ctx, dt, 0, 0, pl, 2 * Dr, 2 * Dl, T1, pl, Wd, 2 * Dl, T2, pl, &bt));
    return qil_dev_gemm(ctx, dt, 2, 0, pr, Dr * sr, 2 * pl, Ap, 2 * pl, T2, 2 * pl, En, pr);
}

int qil_upload_bytes(qil_scratch& tmp, const void* host, size_t bytes, void** dev) {
    QIL_TRY(tmp.alloc(bytes ? bytes : 1, dev));
    if (bytes) {
        QIL_HIP(hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, qil_stream(tmp.ctx)));
        QIL_HIP(qil_stream_sync(tmp.ctx));             // `host` is the caller's memory
    }
    return QIL_OK;
}

int qil_download(qil_context* ctx, void* host_dst, const void* dev_src, size_t bytes) {
    QIL_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, qil_stream(ctx)));
    QIL_HIP(qil_stream_sync(ctx));
    return QIL_OK;
}
